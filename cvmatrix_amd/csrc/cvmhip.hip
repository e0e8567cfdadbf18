// cvmhip.hip -- MI355X (gfx950 / CDNA4) kernels + C ABI for the cvmatrix hot path.
//
// Two stages of the reference are replaced (see include/cvmhip.h for the mapping):
//   fit stage   cvmatrix/cvmatrix.py:1193-1243   G = X^T W X, H = X^T W Y, column sums
//   fold stage  cvmatrix/cvmatrix.py:589-1129    per fold: G - G_V, rank-1 centring,
//                                                outer-std scaling
// Both are the same contraction  A^T diag(w) [A | B]  reduced over ROWS, so one MFMA kernel
// (`wgram_kernel`) serves both: the fit stage runs it over all rows, the fold stage over
// the validation rows of every fold of a batch gathered by index.  Small deterministic
// finalize kernels then reduce the row-split partials in a fixed order and apply the
// reference's correction arithmetic in the reference's operation order.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// (-ffp-contract=off: the finalize arithmetic must round like NumPy's separate ufuncs,
//  and the VALU column sums must round like the MFMA's A operand (w*x rounded first).)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <queue>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/cvmhip.h"

namespace {

#include "geometry.hpp"
#include "wgram_fallback.hpp"
#include "wgram4.hpp"
#include "finalize.hpp"
#include "colstats.hpp"
#include "small_folds.hpp"
#include "resident.hpp"
#include "mid_tile.hpp"
#include "fold_plan.hpp"
#include "host.hpp"
#include "fold_unions.hpp"
#include "stream_accumulate.hpp"
#include "partition.hpp"
#include "fit_plan.hpp"
#include "pls.hpp"
#include "ridge.hpp"
#include "lda.hpp"
#include "pcr.hpp"
#include "pcr_blocked.hpp"
#include "enet.hpp"
#include "omp.hpp"
#include "pcalda.hpp"
#include "tile_product.hpp"
#include "validation_sse.hpp"
#include "predict.hpp"

}  // namespace

// ----------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------
extern "C" {

// CVM_SRC_SHA: sha256 (first 16 hex digits) over the sources the library was built from
// (cvmatrix_amd/build.py computes it; the Python loader compares it with the sources it finds
// next to the library, so a stale prebuilt .so cannot be used by accident)
#ifndef CVM_SRC_SHA
#define CVM_SRC_SHA "unknown"
#endif
const char *cvm_version(void) { return "cvmhip 0.3.0 (gfx950) src " CVM_SRC_SHA; }
const char *cvm_source_hash(void) { return CVM_SRC_SHA; }
const char *cvm_last_error(void) { return g_err; }

size_t cvm_gstats_len(int K, int M) { return 2 * (size_t)K + 2 * (size_t)M + 2; }

size_t cvm_fit_workspace_bytes(int64_t N, int K, int M, int dtype) {
  const Geom g = make_geom(K, M, esize_of(dtype), 0);
  return (size_t)plan_stride(1, N, g, esize_of(dtype)) * g.unit_bytes + QUEUE_RESERVE;
}

int cvm_gram_fit(const void *X, const void *Y, const void *w, int64_t N, int K, int M, int dtype,
                 void *G, void *H, double *gstats, int32_t *neg_flag, void *ws, size_t ws_bytes,
                 void *stream) {
  if (!X || !G || !gstats || !ws) return fail(CVM_EINVAL, "cvm_gram_fit: null pointer%s");
  if (N < 0 || K <= 0 || M < 0 || (M > 0 && (!Y || !H)) || (M == 0 && Y))
    return fail(CVM_EINVAL, "cvm_gram_fit: bad shape%s");
  return by_dtype(dtype, "cvm_gram_fit", [&](auto t) {
    return gram_fit_impl<decltype(t)>(X, Y, w, N, K, M, dtype, G, H, gstats, neg_flag, ws, ws_bytes, (hipStream_t)stream);
  });
}

size_t cvm_fold_workspace_bytes(int64_t n_folds, int64_t n_idx, int64_t max_fold_rows, int K, int M,
                                int dtype, unsigned flags) {
  (void)n_idx;
  if (max_fold_rows <= SMALL_ROWS) {   // direct path: only the per-fold statistics live in ws
    const int64_t nb = n_folds < 32768 ? (n_folds > 0 ? n_folds : 1) : 32768;
    const size_t small = (size_t)nb * small_ws_per_fold(K, M, esize_of(dtype), max_fold_rows) + 512;
    // (batches of folds of 8 rows or more may take mid_tile_kernel behind the statistics pre-pass: one
    //  statistics unit and one statistics vector per fold)
    const size_t pre = (size_t)nb * (stat_geom(K, M, esize_of(dtype)).unit_bytes + align_up(fstat_len(K, M) * 8, 256));
    return (small > pre ? small : pre) + QUEUE_RESERVE;
  }
  const Geom g = make_geom(K, M, esize_of(dtype), !(flags & CVM_RET_XTX));
  const int splits = plan_stride(n_folds, max_fold_rows, g, esize_of(dtype));
  const size_t per_fold = (size_t)splits * g.unit_bytes + align_up(fstat_len(K, M) * 8, 256);
  size_t want = per_fold * (size_t)(n_folds > 0 ? n_folds : 1);
  const size_t cap = (size_t)8 << 30;   // beyond 8 GiB walk the folds in batches
  if (want > cap) want = (cap / per_fold > 0 ? cap / per_fold : 1) * per_fold;
  return want + QUEUE_RESERVE;
}

int cvm_fold_update_ex(const void *X, const void *Y, const void *w, const int64_t *idx,
                       const int64_t *offsets, const int64_t *host_offsets, int64_t n_folds, int64_t N,
                       int K, int M, int dtype, unsigned flags, double ddof, double resolution,
                       const void *G, const void *H, const double *gstats, void *out_XTX,
                       void *out_XTY, void *out_muX, void *out_sdX, void *out_muY, void *out_sdY,
                       double *out_fold, void *ws, size_t ws_bytes, void *stream, int32_t *status) {
  if (!X || !offsets || !host_offsets || !G || !gstats || !ws)
    return fail(CVM_EINVAL, "cvm_fold_update: null pointer%s");
  if (n_folds < 0 || N < 0 || K <= 0 || M < 0 || (M > 0 && !Y))
    return fail(CVM_EINVAL, "cvm_fold_update: bad shape%s");
  if (!idx && host_offsets[n_folds] > 0) return fail(CVM_EINVAL, "cvm_fold_update: idx is null%s");
  if ((flags & CVM_RET_XTY) && (M == 0 || !H))
    return fail(CVM_EINVAL, "cvm_fold_update: CVM_RET_XTY needs Y and H%s");
  if (n_folds == 0) return CVM_OK;
  if ((flags & CVM_IDX_HOST) && (n_folds != 1 || host_offsets[1] - host_offsets[0] > SMALL_ROWS ||
                                host_offsets[1] < host_offsets[0]))
    return fail(CVM_EINVAL, "cvm_fold_update: CVM_IDX_HOST takes one fold of at most 32 rows%s");
  const FoldCall c{X, Y, w, idx, offsets, N, K, M, flags, ddof, resolution, w != nullptr, G, H, gstats, out_XTX, out_XTY,
                   out_muX, out_sdX, out_muY, out_sdY, out_fold, (flags & CVM_RET_XTY) && out_XTY, status};
  return by_dtype(dtype, "cvm_fold_update", [&](auto t) {
    return fold_update_impl<decltype(t)>(c, host_offsets, n_folds, dtype, ws, ws_bytes, (hipStream_t)stream);
  });
}

int cvm_fold_update(const void *X, const void *Y, const void *w, const int64_t *idx,
                    const int64_t *offsets, const int64_t *host_offsets, int64_t n_folds, int64_t N,
                    int K, int M, int dtype, unsigned flags, double ddof, double resolution,
                    const void *G, const void *H, const double *gstats, void *out_XTX,
                    void *out_XTY, void *out_muX, void *out_sdX, void *out_muY, void *out_sdY,
                    double *out_fold, void *ws, size_t ws_bytes, void *stream) {
  return cvm_fold_update_ex(X, Y, w, idx, offsets, host_offsets, n_folds, N, K, M, dtype, flags, ddof, resolution,
                            G, H, gstats, out_XTX, out_XTY, out_muX, out_sdX, out_muY, out_sdY, out_fold, ws,
                            ws_bytes, stream, nullptr);
}

#ifdef CVM_STAMPS
int cvm_debug_stamps(unsigned long long *host_out) {
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 1024 * 8 * 4));
  return CVM_OK;
}
int cvm_debug_pls_stamps(unsigned long long *host_out, int reset) {
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_pls_stamps), sizeof(unsigned long long) * 16));
  if (reset) {
    unsigned long long z[16] = {0};
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_pls_stamps), z, sizeof(z)));
  }
  return CVM_OK;
}
int cvm_debug_sse_stamps(unsigned long long *host_out, int reset) {
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_sse_stamps), sizeof(unsigned long long) * 8));
  if (reset) {
    unsigned long long z[8] = {0};
    HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_sse_stamps), z, sizeof(z)));
  }
  return CVM_OK;
}
int cvm_debug_stamps4(unsigned long long *host_out) {
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps4), sizeof(unsigned long long) * 1024 * 8));
  return CVM_OK;
}
int cvm_debug_stamps3(unsigned long long *host_out) {
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps3), sizeof(unsigned long long) * 1024 * 8 * 2));
  return CVM_OK;
}
int cvm_debug_stamps5(unsigned long long *host_out, int reset) {   // CVM_ITEM_STAMPS x 4 waves x 8 (wgram_fallback.hpp)
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps5), sizeof(unsigned long long) * CVM_ITEM_STAMPS * 4 * 8));
  if (reset) {
    void *p = nullptr;
    HIP_OK(hipGetSymbolAddress(&p, HIP_SYMBOL(g_stamps5)));
    HIP_OK(hipMemset(p, 0, sizeof(unsigned long long) * CVM_ITEM_STAMPS * 4 * 8));
  }
  return CVM_OK;
}
int cvm_debug_stamps2(unsigned long long *host_out) {
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps2), sizeof(unsigned long long) * 1024 * 8 * 4));
  return CVM_OK;
}
#endif

size_t cvm_sweep_workspace_bytes(int64_t n_folds, int64_t max_fold_rows, int K, int M, int dtype) {
  const Geom g = make_geom(K, M, esize_of(dtype), 0);
  const int splits = plan_stride(n_folds, max_fold_rows, g, esize_of(dtype));
  return ((size_t)splits * g.unit_bytes + align_up(fstat_len(K, M) * 8, 256)) * (size_t)(n_folds > 0 ? n_folds : 1) +
         QUEUE_RESERVE;
}

int cvm_sweep_fit(const void *X, const void *Y, const void *w, const int64_t *idx,
                  const int64_t *offsets, const int64_t *host_offsets, int64_t n_folds, int64_t N,
                  int K, int M, int dtype, void *G, void *H, double *gstats, int32_t *neg_flag,
                  void *ws, size_t ws_bytes, void *stream, int64_t *splits_out) {
  if (!X || !idx || !offsets || !host_offsets || !G || !gstats || !ws)
    return fail(CVM_EINVAL, "cvm_sweep_fit: null pointer%s");
  if (n_folds <= 0 || N <= 0 || K <= 0 || M < 0 || (M > 0 && (!Y || !H)) || (M == 0 && Y))
    return fail(CVM_EINVAL, "cvm_sweep_fit: bad shape%s");
  return by_dtype(dtype, "cvm_sweep_fit", [&](auto t) {
    return sweep_fit_impl<decltype(t)>(X, Y, w, idx, offsets, host_offsets, n_folds, N, K, M, dtype, G, H, gstats, neg_flag,
                                       ws, ws_bytes, (hipStream_t)stream, splits_out);
  });
}

int cvm_sweep_all(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                  const int64_t *host_offsets, int64_t n_folds, int64_t N, int K, int M, int dtype, unsigned flags,
                  double ddof, double resolution, void *G, void *H, double *gstats, int32_t *neg_flag,
                  void *out_XTX, void *out_XTY, void *out_muX, void *out_sdX, void *out_muY, void *out_sdY,
                  double *out_fold, void *ws, size_t ws_bytes, void *stream, int64_t *splits_out) {
  if (!X || !idx || !offsets || !host_offsets || !G || !gstats || !ws)
    return fail(CVM_EINVAL, "cvm_sweep_all: null pointer%s");
  if (n_folds <= 0 || N <= 0 || K <= 0 || M < 0 || (M > 0 && (!Y || !H)) || (M == 0 && Y))
    return fail(CVM_EINVAL, "cvm_sweep_all: bad shape%s");
  if ((flags & CVM_RET_XTY) && M == 0) return fail(CVM_EINVAL, "cvm_sweep_all: CVM_RET_XTY needs Y and H%s");
  const FoldCall c{X, Y, w, idx, offsets, N, K, M, flags, ddof, resolution, w != nullptr, G, H, gstats, out_XTX, out_XTY,
                   out_muX, out_sdX, out_muY, out_sdY, out_fold, (flags & CVM_RET_XTY) && out_XTY, nullptr};
  return by_dtype(dtype, "cvm_sweep_all", [&](auto t) {
    return sweep_all_impl<decltype(t)>(c, host_offsets, n_folds, dtype, G, H, gstats, neg_flag, ws, ws_bytes,
                                       (hipStream_t)stream, splits_out);
  });
}

int cvm_sweep_fold_range(const int64_t *offsets, int64_t n_total, int64_t fold0, int64_t n_folds, int K, int M,
                         int dtype, unsigned flags, double ddof, double resolution, int weighted, const void *G,
                         const void *H, const double *gstats, void *out_XTX, void *out_XTY, void *out_muX,
                         void *out_sdX, void *out_muY, void *out_sdY, double *out_fold, void *ws, size_t ws_bytes,
                         int64_t splits, void *stream) {
  if (!offsets || !G || !gstats || !ws) return fail(CVM_EINVAL, "cvm_sweep_folds: null pointer%s");
  if (n_total <= 0 || fold0 < 0 || n_folds <= 0 || fold0 + n_folds > n_total || K <= 0 || M < 0 || splits <= 0)
    return fail(CVM_EINVAL, "cvm_sweep_folds: bad shape%s");
  if ((flags & CVM_RET_XTY) && (M == 0 || !H))
    return fail(CVM_EINVAL, "cvm_sweep_folds: CVM_RET_XTY needs Y and H%s");
  const FoldCall c{nullptr, nullptr, nullptr, nullptr, offsets, 0, K, M, flags, ddof, resolution, weighted, G, H, gstats,
                   out_XTX, out_XTY, out_muX, out_sdX, out_muY, out_sdY, out_fold, (flags & CVM_RET_XTY) && out_XTY, nullptr};
  return by_dtype(dtype, "cvm_sweep_folds", [&](auto t) {
    return sweep_folds_impl<decltype(t)>(c, n_total, fold0, n_folds, ws, ws_bytes, splits, (hipStream_t)stream);
  });
}

int cvm_sweep_folds(const int64_t *offsets, int64_t n_folds, int K, int M, int dtype, unsigned flags,
                    double ddof, double resolution, int weighted, const void *G, const void *H,
                    const double *gstats, void *out_XTX, void *out_XTY, void *out_muX, void *out_sdX,
                    void *out_muY, void *out_sdY, double *out_fold, void *ws, size_t ws_bytes,
                    int64_t splits, void *stream) {
  return cvm_sweep_fold_range(offsets, n_folds, 0, n_folds, K, M, dtype, flags, ddof, resolution, weighted, G, H,
                              gstats, out_XTX, out_XTY, out_muX, out_sdX, out_muY, out_sdY, out_fold, ws, ws_bytes,
                              splits, stream);
}

size_t cvm_sweep_unions_workspace_bytes(int64_t n_unions, int K, int M) {
  if (n_unions < 0 || K <= 0 || M < 0) return 0;
  return union_workspace_bytes(n_unions, K, M);
}

int cvm_sweep_unions(const int64_t *fold_offsets, int64_t n_total, const int64_t *union_folds,
                     const int64_t *union_offsets, const int64_t *host_union_offsets, int64_t n_unions, int K, int M,
                     int dtype, unsigned flags, double ddof, double resolution, int weighted, const void *G, const void *H,
                     const double *gstats, void *out_XTX, void *out_XTY, void *out_muX, void *out_sdX, void *out_muY,
                     void *out_sdY, double *out_fold, const void *sweep_ws, size_t sweep_ws_bytes, int64_t splits, void *ws,
                     size_t ws_bytes, void *stream) {
  // (everything below is decided before the device is touched)
  if (n_unions < 0 || n_total <= 0 || K <= 0 || M < 0) return fail(CVM_EINVAL, "cvm_sweep_unions: bad shape%s");
  if (dtype != CVM_F64 && dtype != CVM_F32) return fail(CVM_EINVAL, "cvm_sweep_unions: dtype must be CVM_F32 or CVM_F64%s");
  if (!fold_offsets || !host_union_offsets || !G || !gstats || !sweep_ws)
    return fail(CVM_EINVAL, "cvm_sweep_unions: null pointer%s");
  if ((flags & CVM_RET_XTX) && !out_XTX) return fail(CVM_EINVAL, "cvm_sweep_unions: CVM_RET_XTX needs out_XTX%s");
  if ((flags & CVM_RET_XTY) && (M == 0 || !H || !out_XTY))
    return fail(CVM_EINVAL, "cvm_sweep_unions: CVM_RET_XTY needs Y, H and out_XTY%s");
  PlanToken token;
  if (!unpack_token(splits, token)) return fail(CVM_EINVAL, "cvm_sweep_unions: not a plan token of cvm_sweep_fit%s");
  if (host_union_offsets[0] < 0) return fail(CVM_EINVAL, "cvm_sweep_unions: negative union offset%s");
  for (int64_t u = 0; u < n_unions; ++u) {
    const int64_t n = host_union_offsets[u + 1] - host_union_offsets[u];
    if (n < 0) return fail(CVM_EINVAL, "cvm_sweep_unions: union offsets must be non-decreasing%s");
    if (n == 0) return fail(CVM_EINVAL, "cvm_sweep_unions: a union of no fold%s");
    if (n > n_total) return fail(CVM_EINVAL, "cvm_sweep_unions: a union of more folds than the sweep has%s");
  }
  if (n_unions > 0 && (!union_folds || !union_offsets || !ws)) return fail(CVM_EINVAL, "cvm_sweep_unions: null pointer%s");
  const Geom g = make_geom(K, M, esize_of(dtype), 0);
  const size_t stride = (size_t)(token.s_off > token.s_diag ? token.s_off : token.s_diag);
  if ((size_t)n_total * stride * g.unit_bytes > sweep_ws_bytes)
    return fail(CVM_EWORKSPACE, "cvm_sweep_unions: sweep workspace smaller than the one cvm_sweep_fit filled%s");
  if (union_workspace_bytes(n_unions, K, M) > ws_bytes)
    return fail(CVM_EWORKSPACE, "cvm_sweep_unions: workspace smaller than cvm_sweep_unions_workspace_bytes%s");
  if (n_unions == 0) return CVM_OK;
  const FoldCall c{nullptr, nullptr, nullptr, nullptr, fold_offsets, 0, K, M, flags, ddof, resolution, weighted, G, H, gstats,
                   out_XTX, out_XTY, out_muX, out_sdX, out_muY, out_sdY, out_fold, (flags & CVM_RET_XTY) != 0, nullptr};
  return by_dtype(dtype, "cvm_sweep_unions", [&](auto t) {
    return sweep_unions_impl<decltype(t)>(c, union_folds, union_offsets, n_unions, g, token, sweep_ws, ws, (hipStream_t)stream);
  });
}

size_t cvm_stream_workspace_bytes(int what, int64_t n_folds, int64_t max_fold_rows, int K, int M, int dtype) {
  if (n_folds <= 0 || max_fold_rows < 0 || K <= 0 || M < 0 || (dtype != CVM_F64 && dtype != CVM_F32)) return 0;
  if (what == CVM_STREAM_ACCUMULATOR) return stream_units_bytes(n_folds, K, M, 8);
  if (what == CVM_STREAM_SCRATCH) return stream_scratch_bytes(n_folds, max_fold_rows, K, M, dtype);
  if (what == CVM_STREAM_CLOSE) return dtype == CVM_F64 ? 0 : stream_units_bytes(n_folds, K, M, 4);
  return 0;
}

int cvm_stream_reset(void *acc, size_t acc_bytes, int64_t n_folds, int K, int M, int dtype, int64_t *state, void *stream) {
  // (everything below is decided before the device is touched)
  if (!acc || !state) return fail(CVM_EINVAL, "cvm_stream_reset: null pointer%s");
  if (n_folds <= 0 || n_folds > 0x7fffffff || K <= 0 || M < 0) return fail(CVM_EINVAL, "cvm_stream_reset: bad shape%s");
  if (dtype != CVM_F64 && dtype != CVM_F32) return fail(CVM_EINVAL, "cvm_stream_reset: dtype must be CVM_F32 or CVM_F64%s");
  if ((uintptr_t)acc % 16) return fail(CVM_EINVAL, "cvm_stream_reset: the accumulator must be 16-byte aligned%s");
  state[SS_MAGIC] = 0;
  if (stream_units_bytes(n_folds, K, M, 8) > acc_bytes)
    return fail(CVM_EWORKSPACE, "cvm_stream_reset: accumulator smaller than cvm_stream_workspace_bytes(CVM_STREAM_ACCUMULATOR)%s");
  HIP_OK(hipMemsetAsync(acc, 0, stream_units_bytes(n_folds, K, M, 8), (hipStream_t)stream));
  state[SS_FOLDS] = n_folds; state[SS_K] = K; state[SS_M] = M; state[SS_DTYPE] = dtype;
  state[SS_CHUNKS] = 0; state[SS_ROWS] = 0; state[SS_WEIGHTED] = -1;
  state[SS_MAGIC] = STREAM_MAGIC;
  return CVM_OK;
}

int cvm_stream_add(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                   const int64_t *host_offsets, int64_t n_folds, int64_t n_rows, int K, int M, int dtype, void *acc,
                   size_t acc_bytes, int64_t *state, void *ws, size_t ws_bytes, void *stream, int64_t *info) {
  // (everything below is decided before the device is touched)
  if (n_folds <= 0 || n_rows < 0 || K <= 0 || M < 0) return fail(CVM_EINVAL, "cvm_stream_add: bad shape%s");
  if (dtype != CVM_F64 && dtype != CVM_F32) return fail(CVM_EINVAL, "cvm_stream_add: dtype must be CVM_F32 or CVM_F64%s");
  if (const char *bad = stream_bad_state(state, n_folds, K, M, dtype)) return fail(CVM_EINVAL, bad);
  if (!acc || !host_offsets) return fail(CVM_EINVAL, "cvm_stream_add: null pointer%s");
  if (host_offsets[0] < 0) return fail(CVM_EINVAL, "cvm_stream_add: negative offset%s");
  int64_t max_rows = 0, present = 0;
  if (int bad = fold_rows(host_offsets, n_folds, "cvm_stream_add", &max_rows, &present)) return bad;
  if (!folds_cover(host_offsets, n_folds, n_rows))
    return fail(CVM_EINVAL, "cvm_stream_add: the folds must cover each of the chunk's n_rows rows exactly once%s");
  if (stream_units_bytes(n_folds, K, M, 8) > acc_bytes)
    return fail(CVM_EWORKSPACE, "cvm_stream_add: accumulator smaller than cvm_stream_workspace_bytes(CVM_STREAM_ACCUMULATOR)%s");
  if (info) { info[0] = 0; info[1] = 0; }
  if (n_rows == 0) return CVM_OK;                    // an empty chunk: nothing is launched
  if (!X || !idx || !offsets || !ws) return fail(CVM_EINVAL, "cvm_stream_add: null pointer%s");
  if ((M > 0) != (Y != nullptr)) return fail(CVM_EINVAL, "cvm_stream_add: Y goes with M > 0, and only with it%s");
  if (state[SS_WEIGHTED] >= 0 && state[SS_WEIGHTED] != (w != nullptr))
    return fail(CVM_EINVAL, "cvm_stream_add: every chunk of a stream has weights, or none has%s");
  // (a workspace too small for one slot per fold: CVM_EWORKSPACE from the plan, before the first launch)
  return by_dtype(dtype, "cvm_stream_add", [&](auto t) {
    return stream_add_impl<decltype(t)>(X, Y, w, idx, offsets, max_rows, present, n_folds, n_rows, K, M, dtype, acc, state, ws,
                                        ws_bytes, (hipStream_t)stream, info);
  });
}

int cvm_stream_close(void *acc, size_t acc_bytes, const int64_t *state, int64_t n_folds, int K, int M, int dtype, void *G,
                     void *H, double *gstats, int32_t *neg_flag, void *ws, size_t ws_bytes, void *stream, void **units_out,
                     size_t *units_bytes_out, int64_t *splits_out) {
  // (everything below is decided before the device is touched)
  if (n_folds <= 0 || K <= 0 || M < 0) return fail(CVM_EINVAL, "cvm_stream_close: bad shape%s");
  if (dtype != CVM_F64 && dtype != CVM_F32) return fail(CVM_EINVAL, "cvm_stream_close: dtype must be CVM_F32 or CVM_F64%s");
  if (const char *bad = stream_bad_state(state, n_folds, K, M, dtype)) return fail(CVM_EINVAL, bad);
  if (!acc || !G || !gstats || (M > 0 && !H) || (dtype == CVM_F32 && !ws))
    return fail(CVM_EINVAL, "cvm_stream_close: null pointer%s");
  if (stream_units_bytes(n_folds, K, M, 8) > acc_bytes)
    return fail(CVM_EWORKSPACE, "cvm_stream_close: accumulator smaller than cvm_stream_workspace_bytes(CVM_STREAM_ACCUMULATOR)%s");
  if (dtype == CVM_F32 && stream_units_bytes(n_folds, K, M, 4) > ws_bytes)
    return fail(CVM_EWORKSPACE, "cvm_stream_close: workspace smaller than cvm_stream_workspace_bytes(CVM_STREAM_CLOSE)%s");
  if (units_bytes_out) *units_bytes_out = stream_units_bytes(n_folds, K, M, esize_of(dtype));
  if (splits_out) *splits_out = pack_token(1, 1);      // one slot per fold
  return by_dtype(dtype, "cvm_stream_close", [&](auto t) {
    return stream_close_impl<decltype(t)>(acc, n_folds, K, M, G, H, gstats, neg_flag, ws, (hipStream_t)stream, units_out);
  });
}

size_t cvm_partition_workspace_bytes(int64_t N, int64_t n_labels) { return partition_workspace_bytes(N, n_labels); }

int cvm_partition_labels(const int64_t *labels, int64_t N, int64_t n_labels, int64_t *idx_out,
                         int64_t *offsets_out, int64_t *first_out, int32_t *err_flag, void *ws,
                         size_t ws_bytes, void *stream) {
  if (!labels || !idx_out || !offsets_out || !first_out || !err_flag || !ws || N < 0)
    return fail(CVM_EINVAL, "cvm_partition_labels: bad argument%s");
  return partition_impl(labels, N, n_labels, idx_out, offsets_out, first_out, err_flag, ws, ws_bytes,
                        (hipStream_t)stream);
}

int cvm_partition_periodic(const int64_t *labels, int64_t N, int64_t n_labels, const void *w, int dtype,
                           int64_t *idx_out, int64_t *offsets_out, int64_t *nz_out, int32_t *not_periodic, void *stream) {
  if (!labels || !idx_out || !offsets_out || !not_periodic || N < 1)
    return fail(CVM_EINVAL, "cvm_partition_periodic: bad argument%s");
  if (dtype != CVM_F64 && dtype != CVM_F32) return fail(CVM_EINVAL, "cvm_partition_periodic: dtype must be CVM_F32 or CVM_F64%s");
  return partition_periodic_impl(labels, N, n_labels, w, dtype, idx_out, offsets_out, nz_out, not_periodic,
                                 (hipStream_t)stream);
}

int cvm_weights_check(const void *w, int64_t N, int dtype, int64_t *out2, void *stream) {
  if (!out2 || N < 0 || (N > 0 && !w)) return fail(CVM_EINVAL, "cvm_weights_check: bad argument%s");
  if (dtype != CVM_F64 && dtype != CVM_F32) return fail(CVM_EINVAL, "cvm_weights_check: dtype must be CVM_F32 or CVM_F64%s");
  return weights_check_impl(w, N, dtype, out2, (hipStream_t)stream);
}

size_t cvm_pls_workspace_bytes(int64_t n_folds, int K, int M, int A, int dtype) {
  if (n_folds < 0 || K <= 0 || M <= 0 || M > PLS_MAXM || A <= 0 || A > PLS_MAXA) return 0;
  return pls_workspace_bytes(n_folds, K, M, A, esize_of(dtype), pls_cu_count());
}

int cvm_pls_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int dtype,
                void *B, void *W, void *P, void *Q, void *R, int32_t *n_fit, int32_t *status,
                void *ws, size_t ws_bytes, void *stream) {
  if (!XTX || !XTY || !B || !n_fit || !status || !ws) return fail(CVM_EINVAL, "cvm_pls_fit: null pointer%s");
  if (n_folds < 0 || K <= 0 || M <= 0 || A <= 0) return fail(CVM_EINVAL, "cvm_pls_fit: bad shape%s");
  if (M > PLS_MAXM) return fail(CVM_EINVAL, "cvm_pls_fit: at most 64 responses%s");
  if (A > PLS_MAXA) return fail(CVM_EINVAL, "cvm_pls_fit: at most 512 components%s");
  return by_dtype(dtype, "cvm_pls_fit", [&](auto t) {
    return pls_fit_impl<decltype(t)>(XTX, XTY, n_folds, K, M, A, B, W, P, Q, R, n_fit, status, ws, ws_bytes,
                                     (hipStream_t)stream);
  });
}

size_t cvm_pls_sse_workspace_bytes(int64_t n_folds, int64_t max_fold_rows, int M, int A) {
  if (n_folds < 0 || max_fold_rows < 0 || M <= 0 || A <= 0) return 0;
  return pls_sse_workspace_bytes(n_folds, max_fold_rows, M, A);
}

int cvm_pls_validation_sse(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                           int64_t n_folds, int64_t max_fold_rows, int K, int M, int A, int dtype, const void *muX,
                           const void *sdX, const void *muY, const void *sdY, const void *B, double *sse,
                           double *wsum, void *ws, size_t ws_bytes, void *stream) {
  if (!X || !Y || !offsets || !B || !sse || !wsum || !ws) return fail(CVM_EINVAL, "cvm_pls_validation_sse: null pointer%s");
  if (n_folds < 0 || max_fold_rows < 0 || K <= 0 || M <= 0 || A <= 0 || (!idx && max_fold_rows > 0))
    return fail(CVM_EINVAL, "cvm_pls_validation_sse: bad shape%s");
  return by_dtype(dtype, "cvm_pls_validation_sse", [&](auto t) {
    return pls_sse_impl<decltype(t)>(X, Y, w, idx, offsets, n_folds, max_fold_rows, K, M, A, muX, sdX, muY, sdY, B, sse,
                                     wsum, ws, ws_bytes, (hipStream_t)stream);
  });
}

size_t cvm_ridge_workspace_bytes(int64_t n_folds, int K, int M, int L) {
  if (n_folds < 0 || K <= 0 || K > RIDGE_MAXK || M <= 0 || M > RIDGE_MAXM || L <= 0 || L > RIDGE_MAXL) return 0;
  return ridge_workspace_bytes(n_folds, K, M, L);
}

int cvm_ridge_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, const double *lambdas, int L,
                  int dtype, void *B, int32_t *info, void *ws, size_t ws_bytes, void *stream) {
  if (!XTX || !XTY || !lambdas || !B || !info || !ws) return fail(CVM_EINVAL, "cvm_ridge_fit: null pointer%s");
  if (n_folds < 0 || K <= 0 || K > RIDGE_MAXK || M <= 0 || M > RIDGE_MAXM)
    return fail(CVM_EINVAL, "cvm_ridge_fit: bad shape (1 <= K <= 4096, 1 <= M <= 64)%s");
  if (L <= 0 || L > RIDGE_MAXL) return fail(CVM_EINVAL, "cvm_ridge_fit: 1 <= L <= 256 penalties%s");
  for (int l = 0; l < L; ++l)
    if (!(lambdas[l] >= 0.0) || lambdas[l] == HUGE_VAL)
      return fail(CVM_EINVAL, "cvm_ridge_fit: every penalty must be finite and >= 0%s");
  return by_dtype(dtype, "cvm_ridge_fit", [&](auto t) {
    return ridge_fit_impl<decltype(t)>(XTX, XTY, n_folds, K, M, lambdas, L, B, info, ws, ws_bytes, (hipStream_t)stream);
  });
}

size_t cvm_lda_workspace_bytes(int64_t n_folds, int K, int C, int L) {
  if (n_folds < 0 || K <= 0 || K > RIDGE_MAXK || C < 2 || C > LDA_MAXC || L <= 0 || L > RIDGE_MAXL) return 0;
  return lda_workspace_bytes(n_folds, K, C, L);
}

int cvm_lda_fit(const void *XTX, const void *XTY, const double *class_w, int64_t n_folds, int K, int C,
                const double *shrinkage, int L, int dtype, void *coef, void *intercept, int32_t *info, void *ws,
                size_t ws_bytes, void *stream) {
  // (everything below is decided before the device is touched)
  if (!XTX || !XTY || !class_w || !shrinkage || !coef || !intercept || !info || !ws)
    return fail(CVM_EINVAL, "cvm_lda_fit: null pointer%s");
  if (n_folds < 0 || K <= 0 || K > RIDGE_MAXK || C < 2 || C > LDA_MAXC)
    return fail(CVM_EINVAL, "cvm_lda_fit: bad shape (1 <= K <= 4096, 2 <= C <= 64)%s");
  if (L <= 0 || L > RIDGE_MAXL) return fail(CVM_EINVAL, "cvm_lda_fit: 1 <= L <= 256 shrinkage values%s");
  for (int l = 0; l < L; ++l)
    if (!(shrinkage[l] >= 0.0 && shrinkage[l] <= 1.0))
      return fail(CVM_EINVAL, "cvm_lda_fit: every shrinkage must lie in [0, 1]%s");
  return by_dtype(dtype, "cvm_lda_fit", [&](auto t) {
    return lda_fit_impl<decltype(t)>(XTX, XTY, class_w, n_folds, K, C, shrinkage, L, coef, intercept, info, ws, ws_bytes,
                                     (hipStream_t)stream);
  });
}

size_t cvm_enet_workspace_bytes(int64_t n_folds, int K, int M, int L) {
  if (n_folds < 0 || K <= 0 || K > ENET_MAXK || M <= 0 || M > ENET_MAXM || L <= 0 || L > ENET_MAXL) return 0;
  return enet_workspace_bytes(n_folds, K, M);
}

int cvm_enet_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, const double *lambdas, int L,
                 double l1_ratio, double tol, int max_sweeps, int dtype, void *B, int32_t *info, int32_t *sweeps,
                 void *ws, size_t ws_bytes, void *stream) {
  if (!XTX || !XTY || !lambdas || !B || !info || !sweeps || !ws)
    return fail(CVM_EINVAL, "cvm_enet_fit: null pointer%s");
  if (n_folds < 0 || K <= 0 || K > ENET_MAXK || M <= 0 || M > ENET_MAXM)
    return fail(CVM_EINVAL, "cvm_enet_fit: bad shape (1 <= K <= 4096, 1 <= M <= 64)%s");
  if (L <= 0 || L > ENET_MAXL) return fail(CVM_EINVAL, "cvm_enet_fit: 1 <= L <= 256 penalties%s");
  for (int l = 0; l < L; ++l)
    if (!(lambdas[l] > 0.0) || lambdas[l] == HUGE_VAL)
      return fail(CVM_EINVAL, "cvm_enet_fit: every penalty must be finite and > 0%s");
  if (!(l1_ratio > 0.0 && l1_ratio <= 1.0))
    return fail(CVM_EINVAL, "cvm_enet_fit: 0 < l1_ratio <= 1 (l1_ratio = 0 is cvm_ridge_fit)%s");
  if (!(tol >= 1e-12 && tol < 1.0)) return fail(CVM_EINVAL, "cvm_enet_fit: 1e-12 <= tol < 1%s");
  if (max_sweeps < 1) return fail(CVM_EINVAL, "cvm_enet_fit: max_sweeps >= 1%s");
  return by_dtype(dtype, "cvm_enet_fit", [&](auto t) {
    return enet_fit_impl<decltype(t)>(XTX, XTY, n_folds, K, M, lambdas, L, l1_ratio, tol, max_sweeps, B, info, sweeps, ws,
                                      ws_bytes, (hipStream_t)stream);
  });
}

size_t cvm_omp_workspace_bytes(int64_t n_folds, int K, int M, int A) {
  if (n_folds < 0 || K <= 0 || K > OMP_MAXK || M <= 0 || M > OMP_MAXM || A <= 0 || A > K || A > OMP_CAP) return 0;
  return omp_workspace_bytes(n_folds, K, M);
}

int cvm_omp_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int normalize, double rank_tol,
                int dtype, void *B, int32_t *support, int32_t *n_fit, void *ws, size_t ws_bytes, void *stream) {
  // (everything below is decided before the device is touched)
  if (!XTX || !XTY || !B || !support || !n_fit || !ws) return fail(CVM_EINVAL, "cvm_omp_fit: null pointer%s");
  if (n_folds < 0 || K <= 0 || K > OMP_MAXK || M <= 0 || M > OMP_MAXM)
    return fail(CVM_EINVAL, "cvm_omp_fit: bad shape (1 <= K <= 4096, 1 <= M <= 64)%s");
  if (A <= 0 || A > K || A > OMP_CAP) return fail(CVM_EINVAL, "cvm_omp_fit: 1 <= A <= min(K, 64) selected variables%s");
  if (normalize != 0 && normalize != 1) return fail(CVM_EINVAL, "cvm_omp_fit: normalize must be 0 or 1%s");
  if (!(rank_tol < 1.0)) return fail(CVM_EINVAL, "cvm_omp_fit: rank_tol must be below 1 (<= 0: the default)%s");
  if (rank_tol <= 0.0) rank_tol = 32.0 * A * 0x1p-52;
  return by_dtype(dtype, "cvm_omp_fit", [&](auto t) {
    return omp_fit_impl<decltype(t)>(XTX, XTY, n_folds, K, M, A, normalize, rank_tol, B, support, n_fit, ws, ws_bytes,
                                     (hipStream_t)stream);
  });
}

size_t cvm_pcalda_workspace_bytes(int64_t n_folds, int K, int C, int A) {
  if (n_folds < 0 || K <= 0 || K > PCL_MAXK || C < 2 || C > PCL_MAXC || A <= 0 || A > K || A > PCL_CAP) return 0;
  return pcalda_workspace_bytes(n_folds, K, C, A);
}

int cvm_pcalda_fit(const void *V, const double *eigenvalues, const int32_t *n_comp, const void *XTY,
                   const double *class_w, int64_t n_folds, int K, int C, int A, int dtype, double pivot_tol,
                   void *coef, void *intercept, int32_t *n_fit, int32_t *info, void *ws, size_t ws_bytes,
                   void *stream) {
  // (everything below is decided before the device is touched)
  if (n_folds < 0 || K <= 0 || K > PCL_MAXK || C < 2 || C > PCL_MAXC)
    return fail(CVM_EINVAL, "cvm_pcalda_fit: bad shape (1 <= K <= 4096, 2 <= C <= 64)%s");
  if (A <= 0 || A > K || A > PCL_CAP) return fail(CVM_EINVAL, "cvm_pcalda_fit: 1 <= A <= min(K, 64) components%s");
  if (!(pivot_tol < 1.0)) return fail(CVM_EINVAL, "cvm_pcalda_fit: pivot_tol must be below 1 (<= 0: the default)%s");
  if (dtype != CVM_F64 && dtype != CVM_F32) return fail(CVM_EINVAL, "cvm_pcalda_fit: dtype must be CVM_F32 or CVM_F64%s");
  if (n_folds == 0) return CVM_OK;
  if (!V || !eigenvalues || !n_comp || !XTY || !class_w || !coef || !intercept || !n_fit || !info || !ws)
    return fail(CVM_EINVAL, "cvm_pcalda_fit: null pointer%s");
  if (pivot_tol <= 0.0) pivot_tol = PCL_PIVOT_TOL;
  return by_dtype(dtype, "cvm_pcalda_fit", [&](auto t) {
    return pcalda_fit_impl<decltype(t)>(V, eigenvalues, n_comp, XTY, class_w, n_folds, K, C, A, pivot_tol, coef, intercept,
                                        n_fit, info, ws, ws_bytes, (hipStream_t)stream);
  });
}

size_t cvm_pcr_workspace_bytes(int64_t n_folds, int K, int M, int A) {
  if (n_folds < 0 || K <= 0 || K > PCR_MAXK || M < 0 || M > PCR_MAXM || A <= 0 || A > K) return 0;
  return pcr_workspace_bytes(n_folds, K, M);
}

int cvm_pcr_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int dtype, double rank_tol,
                void *B, double *eigenvalues, void *V, int32_t *n_fit, int32_t *sweeps, void *ws, size_t ws_bytes,
                void *stream) {
  if (!XTX || !eigenvalues || !n_fit || !sweeps || !ws) return fail(CVM_EINVAL, "cvm_pcr_fit: null pointer%s");
  if (n_folds < 0 || K <= 0 || K > PCR_MAXK || M < 0 || M > PCR_MAXM || A <= 0 || A > K)
    return fail(CVM_EINVAL, "cvm_pcr_fit: bad shape (1 <= K <= 512, 1 <= A <= K, 0 <= M <= 64)%s");
  if (M > 0 ? (!XTY || !B) : (XTY || B))
    return fail(CVM_EINVAL, "cvm_pcr_fit: XTY and B go with M > 0, neither with M == 0 (PCA only)%s");
  if (!(rank_tol < 1.0)) return fail(CVM_EINVAL, "cvm_pcr_fit: rank_tol must be below 1 (<= 0: the default)%s");
  if (rank_tol <= 0.0) rank_tol = 32.0 * K * 0x1p-52;
  return by_dtype(dtype, "cvm_pcr_fit", [&](auto t) {
    return pcr_fit_impl<decltype(t)>(XTX, XTY, n_folds, K, M, A, rank_tol, B, eigenvalues, V, n_fit, sweeps, ws, ws_bytes,
                                     (hipStream_t)stream);
  });
}

size_t cvm_pcr_blocked_workspace_bytes(int64_t n_folds, int K, int M, int A) {
  if (n_folds < 0 || K <= 0 || K > PCRB_MAXK || M < 0 || M > PCR_MAXM || A <= 0 || A > K) return 0;
  return pcr_blocked_workspace_bytes(n_folds, K, M);
}

int cvm_pcr_blocked_fit(const void *XTX, const void *XTY, int64_t n_folds, int K, int M, int A, int dtype,
                        double rank_tol, int max_sweeps, void *B, double *eigenvalues, void *V, int32_t *n_fit,
                        int32_t *sweeps, void *ws, size_t ws_bytes, void *stream) {
  if (!XTX || !eigenvalues || !n_fit || !sweeps || !ws) return fail(CVM_EINVAL, "cvm_pcr_blocked_fit: null pointer%s");
  if (n_folds < 0 || K <= 0 || K > PCRB_MAXK || M < 0 || M > PCR_MAXM || A <= 0 || A > K)
    return fail(CVM_EINVAL, "cvm_pcr_blocked_fit: bad shape (1 <= K <= 4096, 1 <= A <= K, 0 <= M <= 64)%s");
  if (M > 0 ? (!XTY || !B) : (XTY || B))
    return fail(CVM_EINVAL, "cvm_pcr_blocked_fit: XTY and B go with M > 0, neither with M == 0 (PCA only)%s");
  if (!(rank_tol < 1.0)) return fail(CVM_EINVAL, "cvm_pcr_blocked_fit: rank_tol must be below 1 (<= 0: the default)%s");
  if (max_sweeps < 1 || max_sweeps > PCR_MAXSWEEPS)
    return fail(CVM_EINVAL, "cvm_pcr_blocked_fit: max_sweeps must be 1 .. 60%s");
  if (rank_tol <= 0.0) rank_tol = 32.0 * K * 0x1p-52;
  return by_dtype(dtype, "cvm_pcr_blocked_fit", [&](auto t) {
    return pcr_blocked_fit_impl<decltype(t)>(XTX, XTY, n_folds, K, M, A, rank_tol, max_sweeps, B, eigenvalues, V, n_fit,
                                             sweeps, ws, ws_bytes, (hipStream_t)stream);
  });
}

// shapes of cvm_cv_predict / cvm_cv_predict_plan: an error message, or nullptr
static const char *predict_bad_shape(int64_t n_folds, int64_t max_fold_rows, int64_t ldX, int K, int M, int A, int dtype) {
  if (n_folds < 0 || max_fold_rows < 0 || K <= 0 || A <= 0 || ldX < K) return "cvm_cv_predict: bad shape%s";
  if (M <= 0 || M > PLS_MAXM) return "cvm_cv_predict: 1 <= M <= 64 responses%s";
  if (A > PLS_MAXA) return "cvm_cv_predict: at most 512 models per fold%s";
  if (dtype != CVM_F64 && dtype != CVM_F32) return "cvm_cv_predict: dtype must be CVM_F32 or CVM_F64%s";
  // (folds x groups x chunks is counted in 64 bits: 2^40 folds of 2^40 rows are refused here, not wrapped)
  if (n_folds > ((int64_t)1 << 40) || max_fold_rows > ((int64_t)1 << 40) ||
      (n_folds > 0 && (max_fold_rows / SSE_ROWS + 1) > (((int64_t)1 << 52) / n_folds)))
    return "cvm_cv_predict: more than 2^61 workgroups%s";
  return nullptr;
}

int cvm_cv_predict(const void *X, int64_t ldX, const int64_t *idx, const int64_t *offsets, int64_t n_folds,
                   int64_t max_fold_rows, int K, int M, int A, int dtype, const void *muX, const void *sdX,
                   const void *muY, const void *sdY, const void *B, void *out, int by_row, void *stream) {
  // (everything below is decided before the device is touched)
  if (!X || !offsets || !B || !out) return fail(CVM_EINVAL, "cvm_cv_predict: null pointer%s");
  if (by_row != 0 && by_row != 1) return fail(CVM_EINVAL, "cvm_cv_predict: by_row must be 0 or 1%s");
  if (const char *bad = predict_bad_shape(n_folds, max_fold_rows, ldX, K, M, A, dtype)) return fail(CVM_EINVAL, bad);
  return by_dtype(dtype, "cvm_cv_predict", [&](auto t) {
    return predict_impl<decltype(t)>(X, ldX, idx, offsets, n_folds, max_fold_rows, K, M, A, muX, sdX, muY, sdY, B, out,
                                     by_row, (hipStream_t)stream);
  });
}

int cvm_cv_predict_plan(int64_t n_folds, int64_t max_fold_rows, int64_t ldX, int K, int M, int A, int dtype, int aligned,
                        int64_t *info) {
  if (!info) return fail(CVM_EINVAL, "cvm_cv_predict_plan: null pointer%s");
  if (const char *bad = predict_bad_shape(n_folds, max_fold_rows, ldX, K, M, A, dtype)) return fail(CVM_EINVAL, bad);
  const int esize = esize_of(dtype);
  const void *where = aligned ? nullptr : reinterpret_cast<const void *>(8);      // (stands for every address)
  const TilePlan t = tile_plan(K, M, A, esize, tile_vec(16 / esize, where, ldX, K, M, where, where, where));
  const PredictPlan p = predict_plan(n_folds, max_fold_rows, t.groups);
  info[0] = t.nt; info[1] = t.groups; info[2] = p.chunks; info[3] = p.total; info[4] = p.launches;
  info[5] = p.total < PREDICT_MAX_WGS ? p.total : PREDICT_MAX_WGS;
  info[6] = (int64_t)t.lds; info[7] = t.st_in_lds; info[8] = t.vec;
  return CVM_OK;
}

int cvm_pls_plan(int64_t n_folds, int K, int M, int A, int dtype, int64_t *info) {
  if (!info || n_folds < 0 || K <= 0 || M <= 0 || M > PLS_MAXM || A <= 0 || A > PLS_MAXA)
    return fail(CVM_EINVAL, "cvm_pls_plan: bad argument%s");
  PlsPlan p;
  if (!make_pls_plan(n_folds, K, M, A, esize_of(dtype), pls_cu_count(), p))
    return fail(CVM_EINVAL, "cvm_pls_plan: K too large for the LDS plan%s");
  info[0] = p.S; info[1] = p.rows; info[2] = p.folds_per_launch; info[3] = p.xres; info[4] = (int64_t)p.lds;
  PlsRepPlan r;
  if (make_pls_rep_plan(n_folds, K, M, A, esize_of(dtype), pls_cu_count(), r)) {      // few folds: the one-barrier kernel
    info[0] = r.S; info[1] = r.rows; info[2] = r.folds_per_launch; info[3] = 2; info[4] = (int64_t)r.lds;
  }
  return CVM_OK;
}

int cvm_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_timing_mu);
  g_timing.store(on != 0);
  g_ntimed = 0;
  return CVM_OK;
}

static int timing_collect(double *ms, int64_t *n) {      // ms[N_KINDS], n[N_KINDS] by kind; resets the list
  std::lock_guard<std::mutex> lk(g_timing_mu);
  for (int k = 0; k < N_KINDS; ++k) { ms[k] = 0; n[k] = 0; }
  for (int i = 0; i < g_ntimed; ++i) {
    HIP_OK(hipEventSynchronize(g_timed[i].b));
    float t = 0;
    HIP_OK(hipEventElapsedTime(&t, g_timed[i].a, g_timed[i].b));
    const int k = g_timed[i].kind;
    if (k >= 0 && k < N_KINDS) { ms[k] += t; ++n[k]; }
  }
  g_ntimed = 0;
  return CVM_OK;
}

int cvm_timing_read(double *ms_fit, int64_t *n_fit, double *ms_fold, int64_t *n_fold) {
  double ms[N_KINDS];
  int64_t n[N_KINDS];
  const int rc = timing_collect(ms, n);
  if (rc != CVM_OK) return rc;
  if (ms_fit) *ms_fit = ms[0];
  if (n_fit) *n_fit = n[0];
  if (ms_fold) *ms_fold = ms[1];
  if (n_fold) *n_fold = n[1];
  return CVM_OK;
}

int cvm_timing_read_kinds(double *ms4, int64_t *n4) {
  if (!ms4 || !n4) return fail(CVM_EINVAL, "cvm_timing_read_kinds: null pointer%s");
  double ms[N_KINDS];
  int64_t n[N_KINDS];
  const int rc = timing_collect(ms, n);
  for (int k = 0; k < 4; ++k) { ms4[k] = ms[k]; n4[k] = n[k]; }
  return rc;
}

int cvm_timing_read_stream(double *ms_gram, int64_t *n_gram, double *ms_acc, int64_t *n_acc) {
  double ms[N_KINDS];
  int64_t n[N_KINDS];
  const int rc = timing_collect(ms, n);
  if (rc != CVM_OK) return rc;
  if (ms_gram) *ms_gram = ms[KIND_FOLD];
  if (n_gram) *n_gram = n[KIND_FOLD];
  if (ms_acc) *ms_acc = ms[KIND_STREAM];
  if (n_acc) *n_acc = n[KIND_STREAM];
  return CVM_OK;
}

int cvm_clock_probe(void *device_buf, size_t bytes) {
  if (device_buf && ((uintptr_t)device_buf % 8 || bytes < 32)) return fail(CVM_EINVAL, "cvm_clock_probe: an 8-byte aligned buffer of at least 32 bytes%s");
  const size_t wgs = device_buf ? bytes / 32 : 0;
  g_clock_buf.store(nullptr, std::memory_order_release);
  g_clock_wgs.store((int)(wgs > 65536 ? 65536 : wgs), std::memory_order_relaxed);
  g_clock_buf.store((unsigned long long *)device_buf, std::memory_order_release);
  return CVM_OK;
}

int cvm_fill_probe(void *buf, size_t bytes, void *stream) {
  if (!buf || bytes % 16 || (uintptr_t)buf % 16) return fail(CVM_EINVAL, "cvm_fill_probe: 16-byte pieces%s");
  const size_t pieces = bytes / 16;
  if (!pieces) return CVM_OK;
  hipLaunchKernelGGL(fill_probe_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (float *)buf, pieces);
  HIP_OK(hipGetLastError());
  return CVM_OK;
}

int cvm_debug_force_splits(int s_off, int s_diag) {
  if (s_off == 0 && s_diag == 0) { g_force_splits.store(0, std::memory_order_relaxed); return CVM_OK; }
  if (s_off < 1 || s_diag < 1 || s_off > 65535 || s_diag > 65535) return fail(CVM_EINVAL, "cvm_debug_force_splits: 1 <= splits <= 65535, or 0, 0%s");
  g_force_splits.store(((unsigned)s_off << 16) | (unsigned)s_diag, std::memory_order_relaxed);
  return CVM_OK;
}

int cvm_debug_resident(int mode) {
  if (mode < 0 || mode > 2) return fail(CVM_EINVAL, "cvm_debug_resident: 0 (never), 1 (wherever the shape allows) or 2 (the default rule)%s");
  g_resident.store(mode, std::memory_order_relaxed);
  return CVM_OK;
}

int cvm_plan_fold(int64_t n_folds, int64_t max_fold_rows, int K, int M, int dtype, unsigned flags,
                  size_t ws_bytes, int64_t *info) {
  if (!info || K <= 0 || M < 0) return fail(CVM_EINVAL, "cvm_plan_fold: bad argument%s");
  Plan p;
  const bool fold_mode = (flags & 0x80000000u) == 0;   // bit 31 set: plan the fit stage
  int rc = make_plan(n_folds, max_fold_rows, K, M, dtype, flags & 0x7fffffffu, ws_bytes, fold_mode, p);
  if (rc != CVM_OK) return fail(rc, "cvm_plan_fold: workspace too small%s");
  info[0] = p.s_off;
  {
    const int per0 = p.g.diag_only ? 0 : p.g.nTiles - p.g.P, per1 = p.g.P * p.g.Yc;
    info[1] = (int64_t)p.folds_per_batch * ((int64_t)p.s_off * per0 + (int64_t)p.s_diag * per1);
  }
  info[6] = p.s_diag;
  info[7] = p.splits;
  info[2] = p.g.P;
  info[3] = p.g.nT;
  info[4] = p.folds_per_batch;
  // MFMA instructions issued per 4 rows of one unit (executed work, incl. padding)
  int64_t per4 = 0;
  // MFMAs per k-step: an off-diagonal tile 4 waves x 16; a diagonal tile in the float64 LDS-DMA
  // kernel 36 (the upper triangle of its 8 x 8 grid) + 8 per 16 live columns of the first Y
  // chunk; in the general kernel, or when folds are finished in the epilogue, 3 blocks of 16 +
  // 16 for XTY
  const int es_ = esize_of(dtype);
  const bool tri = ((size_t)K * es_) % 16 == 0 && (es_ == 4 || M % 2 == 0) &&
                   !(es_ == 8 && fold_mode && p.splits == 1);
  if (!p.g.diag_only) per4 += (int64_t)(p.g.nTiles - p.g.P) * 64 + (int64_t)p.g.P * (tri ? 36 : 48);
  if (M > 0) {
    if (tri && !p.g.diag_only) per4 += (int64_t)p.g.P * (M > 16 ? 16 : 8) + (int64_t)p.g.P * (p.g.Yc - 1) * 16;
    else per4 += (int64_t)p.g.P * p.g.Yc * 16;
  }
  info[5] = per4;
  return CVM_OK;
}

}  // extern "C"
