// validation_sse.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after
// tile_product.hpp).
// Validation errors of the folds' linear models (PLS, ridge and PCR coefficients alike): the last step of a
// cross-validation on the device.  For fold f, model a, response m:
//   sse[f][a][m] = sum over the fold's validation rows i of
//                  w_i ( ((x_i - muX_f) / sdX_f) . B[f][a][:, m] * sdY_f[m] + muY_f[m] - y_im )^2
//   wsum[f]      = sum w_i
// (centre / scale vectors are the fold stage's statistics outputs; a NULL one means 0 / 1).
// One workgroup = 64 validation rows x 64 NT of the A M columns (a, m); the products are the shared loop's
// (tile_product_loop.hpp; tile_product.hpp: the scheme, the variants and the choice among them), with X
// contiguous (row pitch K) and ScorerRcp.  What this file adds: the squared errors, summed over the rows in a
// fixed order (registers -> lanes -> a second small kernel over the row chunks: no float atomics).
#pragma once

struct SseArgs {
  const void *X, *Y, *w, *muX, *sdX, *muY, *sdY, *B;
  const int64_t *idx, *offs;
  int K, M, A, n_chunks;        // n_chunks: row chunks of the longest fold
  int st_in_lds;                // the fold's K means and reciprocal standard deviations fit in LDS next to the stages
  double *part;                 // [F][n_chunks][A M] partial sums, [F][n_chunks] weight sums behind them
  double *sse, *wsum;
  int64_t F;
};

template <typename T, int NT, int V>
__global__ __launch_bounds__(256) void pls_sse_kernel(const SseArgs a) {
  constexpr int W = 64 * NT;
  SSE_STAMP_START;
  const int K = a.K, M = a.M, C = a.A * M;
  const int chunk = blockIdx.x, cg = blockIdx.y, f = blockIdx.z;
  const int64_t o0 = a.offs[f];
  const int n = (int)(a.offs[f + 1] - o0);
  const int r0 = chunk * SSE_ROWS;
  double *part = a.part + ((size_t)f * a.n_chunks + chunk) * C;
  double *wpart = a.part + (size_t)a.F * a.n_chunks * C + (size_t)f * a.n_chunks + chunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lk = lane >> 4, lc = lane & 15;
  const int c0 = cg * W;
  const int Cg = C - c0 < W ? C - c0 : W;                     // columns of this group
  if (r0 >= n) {                                              // past this fold's rows: zeros
    for (int c = tid; c < Cg; c += 256) part[c0 + c] = 0.0;
    if (cg == 0 && tid == 0) *wpart = 0.0;
    return;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char sse_smem[];
  __shared__ int64_t rows[SSE_ROWS];
  __shared__ double wl[SSE_ROWS];
  const T *Y = (const T *)a.Y, *Wt = (const T *)a.w;
  const T *X = (const T *)a.X;
  const int64_t ldX = K;                                      // (X is contiguous)
  const T *muX = a.muX ? (const T *)a.muX + (size_t)f * K : nullptr;
  const T *sdX = a.sdX ? (const T *)a.sdX + (size_t)f * K : nullptr;
  const T *Bf = (const T *)a.B + (size_t)f * a.A * K * M;
  if (tid < SSE_ROWS) {
    const bool ok = r0 + tid < n;
    const int64_t r = ok ? a.idx[o0 + r0 + tid] : 0;          // (rows past the end re-read row 0)
    rows[tid] = r;
    wl[tid] = ok ? (Wt ? (double)Wt[r] : 1.0) : 0.0;
  }
  __syncthreads();
  const int nr = n - r0 < SSE_ROWS ? n - r0 : SSE_ROWS;       // rows of this chunk
  const int st_in_lds = a.st_in_lds;
  unsigned char *smem = sse_smem;
  using Rcp = ScorerRcp;
#include "tile_product_loop.hpp"
  // squared errors: register r of tile (rt, t) is (row 16 rt + drow(lane, r), column 16 (wave NT + t) + lc);
  // summed over registers, row tiles, then the four lane groups -- a fixed order
  const T *muY = a.muY ? (const T *)a.muY + (size_t)f * M : nullptr;
  const T *sdY = a.sdY ? (const T *)a.sdY + (size_t)f * M : nullptr;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int lcol = 16 * (wave * NT + t) + lc;
    const bool valid = lcol < Cg;
    const int col = c0 + lcol;
    const int m = valid ? col % M : 0;
    const double sy = sdY ? (double)sdY[m] : 1.0, my = muY ? (double)muY[m] : 0.0;
    double sacc = 0.0;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 16 * rt + MF<T>::drow(lane, r);
        if (valid && r0 + lr < n) {
          const double e = (double)acc[rt][t][r] * sy + my - (double)Y[rows[lr] * (int64_t)M + m];
          sacc += wl[lr] * (e * e);
        }
      }
    const double s1 = __shfl(sacc, lc + 16), s2 = __shfl(sacc, lc + 32), s3 = __shfl(sacc, lc + 48);
    const double sw = ((__shfl(sacc, lc) + s1) + s2) + s3;
    if (lk == 0 && valid) part[col] = sw;
  }
  if (cg == 0 && tid == 0) {
    double t = 0.0;
    for (int i = 0; i < SSE_ROWS; ++i) t += wl[i];
    *wpart = t;
  }
  SSE_STAMP(5);
}

// sums over a fold's row chunks, in chunk order
__global__ void pls_sse_reduce_kernel(const SseArgs a) {
  const int C = a.A * a.M;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < a.F * C) {
    const int64_t f = e / C;
    const int c = (int)(e - f * C);
    const int64_t n = a.offs[f + 1] - a.offs[f];
    const int used = (int)((n + SSE_ROWS - 1) / SSE_ROWS);
    double s = 0.0;
    for (int ch = 0; ch < used; ++ch) s += a.part[((size_t)f * a.n_chunks + ch) * C + c];
    a.sse[e] = s;
  }
  if (e < a.F) {
    const int64_t n = a.offs[e + 1] - a.offs[e];
    const int used = (int)((n + SSE_ROWS - 1) / SSE_ROWS);
    double s = 0.0;
    for (int ch = 0; ch < used; ++ch) s += a.part[(size_t)a.F * a.n_chunks * C + (size_t)e * a.n_chunks + ch];
    a.wsum[e] = s;
  }
}

size_t pls_sse_workspace_bytes(int64_t F, int64_t max_rows, int M, int A) {
  const int64_t chunks = (max_rows + SSE_ROWS - 1) / SSE_ROWS;
  return (size_t)F * (chunks > 0 ? chunks : 1) * ((size_t)A * M + 1) * 8 + 256;
}

template <typename T>
int pls_sse_impl(const void *X, const void *Y, const void *w, const int64_t *idx, const int64_t *offsets,
                 int64_t F, int64_t max_rows, int K, int M, int A, const void *muX, const void *sdX, const void *muY,
                 const void *sdY, const void *B, double *sse, double *wsum, void *ws, size_t ws_bytes, hipStream_t st) {
  if (ws_bytes < pls_sse_workspace_bytes(F, max_rows, M, A)) return fail(CVM_EWORKSPACE, "cvm_pls_validation_sse: workspace too small%s");
  if (F == 0) return CVM_OK;
  SseArgs a;
  memset(&a, 0, sizeof(a));
  a.X = X; a.Y = Y; a.w = w; a.muX = muX; a.sdX = sdX; a.muY = muY; a.sdY = sdY; a.B = B;
  a.idx = idx; a.offs = offsets; a.K = K; a.M = M; a.A = A; a.F = F;
  int64_t chunks = (max_rows + SSE_ROWS - 1) / SSE_ROWS;
  if (chunks < 1) chunks = 1;
  a.n_chunks = (int)chunks;
  a.part = reinterpret_cast<double *>(ws);
  a.sse = sse; a.wsum = wsum;
  const int C = A * M;
  if (F > 65535) return fail(CVM_EINVAL, "cvm_pls_validation_sse: at most 65535 folds per call%s");
  const TilePlan p = tile_plan(K, M, A, (int)sizeof(T), tile_vec(16 / (int)sizeof(T), X, K, K, M, muX, sdX, B));
  a.st_in_lds = p.st_in_lds;
  void (*kern)(const SseArgs) = nullptr;
  TILE_PICK(pls_sse_kernel, T, p, kern)
  if (!kern) return fail(CVM_EINVAL, "cvm_pls_validation_sse: no kernel for this shape%s");
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)chunks, (unsigned)p.groups, (unsigned)F), dim3(256), p.lds, st, a);
  const int64_t ne = F * C > F ? F * C : F;
  hipLaunchKernelGGL(pls_sse_reduce_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, a);
  HIP_OK(hipGetLastError());
  return CVM_OK;
}
