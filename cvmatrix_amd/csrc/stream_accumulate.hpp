// stream_accumulate.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace).
// Streaming cross-validation (cvm_stream_*): the folds' raw updates  U_f = X_f^T W X_f | X_f^T W Y_f, their
// column sums and sw_f, nz_f are sums over ROWS, hence sums over row CHUNKS.  Every chunk runs the Gram kernel
// exactly as cvm_sweep_fit does (same plan, same launch, into a scratch workspace of the chunk's own) and
// stream_accumulate_kernel then adds every fold's chunk update to a float64 ACCUMULATOR: one unit per fold at
// slot stride 1, the unit layout of make_geom(K, M, 8, 0) -- for float64 the very layout the finalize kernels
// read with s_off = s_diag = 1.  cvm_stream_close makes the accumulated state readable by cvm_sweep_fold_range
// and cvm_sweep_unions as they are: float64 reads the accumulator in place, float32 rounds every accumulated
// element ONCE into a float32 unit workspace; G, H, gstats are the fold-ordered sum of the units
// (launch_fit_apply).  G, H, gstats are not formed per chunk.
//
// Order of every sum: a fold's row-split slots of the chunk in slot order in float64 (s_off slots for
// off-diagonal tiles, s_diag for diagonal tiles, XTY panels and statistics) -- apply_kernel's "segment sum" --
// and that sum is added to the accumulated element.  A stream of ONE chunk leaves 0 + U_f: the bits of
// cvm_sweep_fit's fold updates.  A fold without rows in the chunk is skipped: its scratch slots are never read.
// Nor are the strictly lower 16 x 16 blocks of a diagonal tile, which the Gram launch does not write (the finalize
// kernels mirror the upper ones): the scratch is whatever the allocator hands out, and what it held there -- a NaN
// of an earlier stream, say -- stays out of the accumulator, whose elements there stay zero.
// No atomics, no workgroup waits for another.
//
// Traffic per chunk: every chunk partial read once + the accumulator units of the folds present read and
// written once, in 16-byte pieces, lane l of a wave on piece l of a 1 KiB run (loads and stores coalesced);
// no LDS.  HBM-bound.
#pragma once

constexpr int STREAM_THREADS = 256;
constexpr int STREAM_UNR = 4;                                   // 16-byte accumulator pieces per thread
constexpr int STREAM_BLOCK_ELEMS = STREAM_THREADS * STREAM_UNR * 2;   // float64 elements per workgroup (2048)
static_assert((TILE * TILE) % STREAM_BLOCK_ELEMS == 0, "a workgroup of stream_accumulate_kernel stays inside one tile");
static_assert(STREAM_BLOCK_ELEMS == 16 * TILE, "a workgroup of stream_accumulate_kernel is one row of 16 x 16 blocks of a tile");

// the host header of a stream (int64[CVM_STREAM_STATE_LEN], filled by cvm_stream_reset)
constexpr int64_t STREAM_MAGIC = 0x43564d5354524d31ll;         // "CVMSTRM1"
enum { SS_MAGIC = 0, SS_FOLDS, SS_K, SS_M, SS_DTYPE, SS_CHUNKS, SS_ROWS, SS_WEIGHTED };

struct StreamArgs {
  const char *ws;        // the chunk's partials (unit = fold * splits + sp, geometry gp) | close: the accumulator
  char *acc;             // float64 units, one per fold (geometry ga)                     | close: the float32 units
  const int64_t *offs;   // device: the chunk's fold offsets (a fold without rows is skipped)
  Geom gp, ga;
  int splits, s_off, s_diag;
  int64_t fold0;         // first fold of the launch
  unsigned nb_t, nb_h, nb_s;   // workgroups per fold: tiles, XTY panels, statistics
};

__host__ __device__ __forceinline__ size_t up256(size_t v) { return (v + 255) / 256 * 256; }      // (region starts of a unit)

inline size_t stream_units_bytes(int64_t n_folds, int K, int M, int esize) {
  const Geom g = make_geom(K, M, esize, 0);
  // (the fstats region cvm_sweep_fold_range carves behind the units rides along)
  return align_up((size_t)(n_folds > 0 ? n_folds : 1) * (g.unit_bytes + fstat_len(K, M) * 8), 256);
}

inline void stream_blocks(StreamArgs &a) {
  a.nb_t = (unsigned)(a.ga.tile_elems / STREAM_BLOCK_ELEMS);
  a.nb_h = (unsigned)((a.ga.h_elems + STREAM_BLOCK_ELEMS - 1) / STREAM_BLOCK_ELEMS);
  a.nb_s = (unsigned)((a.ga.stat_len + STREAM_BLOCK_ELEMS - 1) / STREAM_BLOCK_ELEMS);
}

// One workgroup: STREAM_BLOCK_ELEMS consecutive elements of one region (tiles | XTY panels | statistics) of
// one fold's unit.  S: the element type of the region in the chunk's partials (T, or double for statistics).
// `skip_cols`: the leading columns of every 128-element row of the run that no Gram launch writes and nothing reads
// (a diagonal tile's strictly lower 16 x 16 blocks): left out, their accumulator elements stay as reset left them.
// `n_written` (odd): the run's last element, n_elems - 1, is one no Gram launch writes; it is not added either.
template <typename S>
__device__ __forceinline__ void stream_add_run(const char *src, size_t slot_bytes, int nsp, double *dst, size_t e0, size_t n_elems,
                                               int skip_cols = 0, size_t n_written = ~(size_t)0) {
  typedef S vs_t __attribute__((ext_vector_type(2)));
  typedef double vd_t __attribute__((ext_vector_type(2)));
  size_t e[STREAM_UNR];
  vd_t acc[STREAM_UNR], us[STREAM_UNR];
#pragma unroll
  for (int j = 0; j < STREAM_UNR; ++j) {
    e[j] = e0 + 2 * ((size_t)j * STREAM_THREADS + threadIdx.x);
    if ((int)(e[j] % TILE) < skip_cols) e[j] = n_elems;          // (past the end: every guard below leaves it out)
    us[j] = (vd_t){0.0, 0.0};
    if (e[j] < n_elems) acc[j] = *reinterpret_cast<const vd_t *>(dst + e[j]);
  }
  for (int sp = 0; sp < nsp; ++sp) {                 // slot order; the four pieces of a slot in flight together
    const S *p = reinterpret_cast<const S *>(src + (size_t)sp * slot_bytes);
    vs_t v[STREAM_UNR];
#pragma unroll
    for (int j = 0; j < STREAM_UNR; ++j)
      if (e[j] < n_elems) v[j] = *reinterpret_cast<const vs_t *>(p + e[j]);
#pragma unroll
    for (int j = 0; j < STREAM_UNR; ++j)
      if (e[j] < n_elems) { us[j][0] += (double)v[j][0]; if (e[j] + 1 < n_written) us[j][1] += (double)v[j][1]; }
  }
#pragma unroll
  for (int j = 0; j < STREAM_UNR; ++j)
    if (e[j] < n_elems) {
      acc[j][0] += us[j][0]; acc[j][1] += us[j][1];
      *reinterpret_cast<vd_t *>(dst + e[j]) = acc[j];
    }
}

template <typename T> __global__ __launch_bounds__(STREAM_THREADS) void stream_accumulate_kernel(const StreamArgs a) {
  const unsigned bpf = a.nb_t + a.nb_h + a.nb_s;
  const int64_t f = a.fold0 + blockIdx.x / bpf;
  unsigned b = blockIdx.x % bpf;
  if (a.offs[f + 1] == a.offs[f]) return;            // no row of the fold in this chunk
  const Geom &gp = a.gp, &ga = a.ga;
  const char *src = a.ws + (size_t)f * a.splits * gp.unit_bytes;
  char *dst = a.acc + (size_t)f * ga.unit_bytes;
  if (b < a.nb_t) {
    const size_t e0 = (size_t)b * STREAM_BLOCK_ELEMS;
    int ti, tj;
    decode_tile((int)(e0 / (TILE * TILE)), gp.P, ti, tj);
    // a workgroup = the 16 rows of one row of 16 x 16 blocks: on a diagonal tile the blocks left of the diagonal one
    // are never written by the Gram launch (wgram4_diag_body stores the upper triangle of the 8 x 8 grid; the
    // finalize kernels mirror it) -- adding them would carry whatever the scratch held into the accumulator
    const int skip = ti == tj ? (int)(e0 % (TILE * TILE) / STREAM_BLOCK_ELEMS) * 16 : 0;
    stream_add_run<T>(src, gp.unit_bytes, ti == tj ? a.s_diag : a.s_off, (double *)dst, e0, ga.tile_elems, skip);
  } else if ((b -= a.nb_t) < a.nb_h) {
    stream_add_run<T>(src + up256(gp.tile_elems * sizeof(T)), gp.unit_bytes, a.s_diag,
                      (double *)(dst + up256(ga.tile_elems * 8)), (size_t)b * STREAM_BLOCK_ELEMS, ga.h_elems);
  } else {
    b -= a.nb_h;
    // (the statistics end in sw, nz, the count of negative weights and one spare word that nothing writes)
    stream_add_run<double>(src + up256(gp.tile_elems * sizeof(T)) + up256(gp.h_elems * sizeof(T)),
                           gp.unit_bytes, a.s_diag,
                           (double *)(dst + up256(ga.tile_elems * 8) + up256(ga.h_elems * 8)),
                           (size_t)b * STREAM_BLOCK_ELEMS, ga.stat_len, 0, ga.stat_len - 1);
  }
}

// cvm_stream_close, float32: every accumulated element rounded once into a float32 unit (the statistics stay
// float64).  Thread = 4 elements: two 16-byte loads, one 16-byte store.
__global__ __launch_bounds__(STREAM_THREADS) void stream_round_kernel(const StreamArgs a) {
  typedef double vd_t __attribute__((ext_vector_type(2)));
  typedef float vf_t __attribute__((ext_vector_type(4)));
  const unsigned bpf = a.nb_t + a.nb_h + a.nb_s;
  const int64_t f = a.fold0 + blockIdx.x / bpf;
  unsigned b = blockIdx.x % bpf;
  const Geom &gs = a.ga, &gd = a.gp;                 // source: the float64 units; destination: float32 units
  const char *src = a.ws + (size_t)f * gs.unit_bytes;
  char *dst = a.acc + (size_t)f * gd.unit_bytes;
  size_t n_elems;
  bool stats = false;
  if (b < a.nb_t) {
    n_elems = gs.tile_elems;
  } else if ((b -= a.nb_t) < a.nb_h) {
    n_elems = gs.h_elems;
    src += up256(gs.tile_elems * 8); dst += up256(gd.tile_elems * 4);
  } else {
    b -= a.nb_h;
    n_elems = gs.stat_len; stats = true;
    src += up256(gs.tile_elems * 8) + up256(gs.h_elems * 8);
    dst += up256(gd.tile_elems * 4) + up256(gd.h_elems * 4);
  }
  for (int j = 0; j < STREAM_UNR / 2; ++j) {
    const size_t e = (size_t)b * STREAM_BLOCK_ELEMS + 4 * ((size_t)j * STREAM_THREADS + threadIdx.x);
    if (e >= n_elems) continue;                      // (every region is a whole number of 4-element pieces)
    const vd_t lo = *reinterpret_cast<const vd_t *>((const double *)src + e);
    const vd_t hi = *reinterpret_cast<const vd_t *>((const double *)src + e + 2);
    if (stats) {
      *reinterpret_cast<vd_t *>((double *)dst + e) = lo;
      *reinterpret_cast<vd_t *>((double *)dst + e + 2) = hi;
    } else {
      *reinterpret_cast<vf_t *>((float *)dst + e) = (vf_t){(float)lo[0], (float)lo[1], (float)hi[0], (float)hi[1]};
    }
  }
}

// a launch's global size in x stays below 2^32 (fold_unions.hpp's note): whole folds per launch
template <typename KERNEL> int stream_launch_folds(KERNEL kernel, StreamArgs a, int64_t n_folds, hipStream_t st) {
  const int64_t bpf = (int64_t)a.nb_t + a.nb_h + a.nb_s;
  const int64_t per_launch = UNION_MAX_WGS / bpf > 0 ? UNION_MAX_WGS / bpf : 1;
  for (int64_t f0 = 0; f0 < n_folds; f0 += per_launch) {
    const int64_t nb = n_folds - f0 < per_launch ? n_folds - f0 : per_launch;
    a.fold0 = f0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(nb * bpf)), dim3(STREAM_THREADS), 0, st, a);
  }
  HIP_OK(hipGetLastError());
  return CVM_OK;
}

// bytes stream_accumulate_kernel moves for one chunk (the model the measurements are held against): the
// partials of the folds present read once, their accumulator units read and written once
inline size_t stream_add_traffic(const Geom &gp, const Geom &ga, int s_off, int s_diag, int64_t folds_present, int esize) {
  // (a diagonal tile: the 36 of its 64 blocks of 16 x 16 on and above the diagonal)
  const size_t off_tiles = (size_t)(gp.nTiles - gp.P) * TILE * TILE, diag_tiles = (size_t)gp.P * 36 * 256;
  const size_t partial = (off_tiles * s_off + (diag_tiles + gp.h_elems) * s_diag) * esize + gp.stat_len * 8 * s_diag;
  const size_t unit = (off_tiles + diag_tiles + ga.h_elems + ga.stat_len) * 8;
  return (size_t)folds_present * (partial + 2 * unit);
}

// shapes of cvm_stream_add / cvm_stream_close against the stream's header: an error message, or nullptr
inline const char *stream_bad_state(const int64_t *state, int64_t n_folds, int K, int M, int dtype) {
  if (!state || state[SS_MAGIC] != STREAM_MAGIC) return "cvm_stream: not a stream header of cvm_stream_reset%s";
  if (state[SS_FOLDS] != n_folds || state[SS_K] != K || state[SS_M] != M || state[SS_DTYPE] != dtype)
    return "cvm_stream: n_folds, K, M, dtype differ from what the accumulator was reset with%s";
  return nullptr;
}

// A forced row-split plan (cvm_debug_force_splits / CVM_FORCE_SPLITS: tests) as the stream takes it: the planner
// clamps a forced plan to 64 rows per split of the longest fold -- chunks are short by nature, and the sums
// over several slots per fold could then never be exercised -- so here it is taken as given (at most 128
// splits), wherever the planner would take a forced plan at all.  Short and empty splits are nothing new to
// the Gram kernel: every ragged batch has them.
inline int stream_forced_stride(const Geom &g, int &so, int &sd) {
  const unsigned force = forced_splits();
  if (!force || g.diag_only || g.nTiles <= g.P) return 0;
  so = (int)(force >> 16); sd = (int)(force & 0xffffu);
  if (so > 128) so = 128;
  if (sd > 128) sd = 128;
  return so > sd ? so : sd;
}

// the plan of a chunk: make_plan's, as cvm_sweep_fit asks for it (all folds in one batch)
inline int stream_plan(int64_t n_folds, int64_t max_rows, int K, int M, int dtype, size_t usable, Plan &p) {
  const int rc = make_plan(n_folds, max_rows, K, M, dtype, CVM_RET_XTX | CVM_RET_XTY, usable, true, p);
  if (rc != CVM_OK || p.folds_per_batch < n_folds) return CVM_EWORKSPACE;
  int so = 0, sd = 0;
  const int stride = stream_forced_stride(p.g, so, sd);
  if (stride && ((size_t)stride * p.g.unit_bytes + p.fstat_bytes_per_fold) * (size_t)n_folds <= usable) set_plan_splits(p, so, sd);
  return CVM_OK;
}

inline size_t stream_scratch_bytes(int64_t n_folds, int64_t max_rows, int K, int M, int dtype) {
  const int esize = esize_of(dtype);
  const Geom g = make_geom(K, M, esize, 0);
  int so = 0, sd = 0, stride = plan_stride(n_folds, max_rows, g, esize);
  const int forced = stream_forced_stride(g, so, sd);
  if (forced > stride) stride = forced;
  return ((size_t)stride * g.unit_bytes + align_up(fstat_len(K, M) * 8, 256)) * (size_t)(n_folds > 0 ? n_folds : 1) + QUEUE_RESERVE;
}

template <typename T>
int stream_add_impl(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                    int64_t max_rows, int64_t present, int64_t n_folds, int64_t n_rows, int K, int M, int dtype, void *acc,
                    int64_t *state, void *ws, size_t ws_bytes, hipStream_t st, int64_t *splits_out) {
  // (max_rows, present: the longest fold of the chunk and its folds that have rows, fold_rows)
  // the chunk's Gram launch, planned and launched as cvm_sweep_fit does
  const WsCarve wq = carve_queue(ws, ws_bytes);
  Plan p;
  if (stream_plan(n_folds, max_rows, K, M, dtype, wq.usable, p) != CVM_OK)
    return fail(CVM_EWORKSPACE, "cvm_stream_add: the workspace must hold the chunk's partials of all folds%s");
  int rc = launch_wgram<T>(gram_args<T>(X, Y, w, idx, offsets, n_rows, 0, p, n_folds, ws), w != nullptr, true,
                           rows_aligned(X, K, sizeof(T)), st, KIND_FOLD, wq.queue);
  if (rc != CVM_OK) return rc;
  StreamArgs s;
  memset(&s, 0, sizeof(s));
  s.ws = (const char *)ws; s.acc = (char *)acc; s.offs = offsets;
  s.gp = p.g; s.ga = make_geom(K, M, 8, 0);
  s.splits = p.splits; s.s_off = p.s_off; s.s_diag = p.s_diag;
  stream_blocks(s);
  TimedLaunch *tl = timed_begin(KIND_STREAM, st);
  rc = stream_launch_folds(stream_accumulate_kernel<T>, s, n_folds, st);
  timed_end(tl, st);
  if (rc != CVM_OK) return rc;
  state[SS_CHUNKS] += 1; state[SS_ROWS] += n_rows; state[SS_WEIGHTED] = w != nullptr;
  if (splits_out) {
    splits_out[0] = pack_token(p.s_off, p.s_diag);
    splits_out[1] = (int64_t)stream_add_traffic(s.gp, s.ga, p.s_off, p.s_diag, present, sizeof(T));
  }
  return CVM_OK;
}

template <typename T>
int stream_close_impl(void *acc, int64_t n_folds, int K, int M, void *G, void *H, double *gstats, int32_t *neg_flag,
                      void *ws, hipStream_t st, void **units_out) {
  const Geom g = make_geom(K, M, sizeof(T), 0);
  void *units = acc;
  if (sizeof(T) == 4) {
    StreamArgs s;
    memset(&s, 0, sizeof(s));
    s.ws = (const char *)acc; s.acc = (char *)ws; s.gp = g; s.ga = make_geom(K, M, 8, 0);
    stream_blocks(s);
    const int rc = stream_launch_folds(stream_round_kernel, s, n_folds, st);
    if (rc != CVM_OK) return rc;
    units = ws;
  }
  Plan p;
  p.g = g;
  set_plan_splits(p, 1, 1);
  FinArgs f = fin_base(p, (int)n_folds, 1, 0, units);       // G = sum_f U_f in fold order
  fin_fit_side(f, nullptr, G, M > 0 ? H : nullptr, neg_flag);
  launch_fit_apply<T>(f, g, gstats, st);
  HIP_OK(hipGetLastError());
  if (units_out) *units_out = units;
  return CVM_OK;
}
