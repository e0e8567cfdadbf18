// predict.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after
// tile_product.hpp).
// Out-of-fold predictions of every fold's linear models, and predictions for new rows: the stage after the
// model fitters.  For fold f, row i of the fold, model a and response m
//   out[r][a][m] = ((x_i - muX[f]) / sdX[f]) . B[f][a][:, m] * sdY[f][m] + muY[f][m]
// -- the products the scorer (validation_sse.hpp) reduces to one sum per (fold, model, response), here stored
// whole.  The products are the shared loop's (tile_product_loop.hpp; tile_product.hpp: the scheme, the variants
// and the choice among them), with any row pitch and PredictRcp.  What this file adds: any number of folds of
// any length (a flat workgroup number cut into launches), rows by position or by number, and the epilogue.
//
// FIXED ORDER.  One prediction is ONE accumulator chain (tile_product.hpp), and z = (T)((x - mu) * (1 / sd))
// is formed in float64 with ONE reciprocal (predict_rcp) on every route.  So the bits of one prediction
// depend on its row of X, its fold's statistics and its column of B alone -- not on the fold's other rows,
// the row's place in the fold, the other folds, A, the other columns of B, ldX, by_row, alignment or the
// stream.
//
// EPILOGUE.  acc * sdY + muY in float64, rounded once to T.  For a fixed accumulator register the lanes
// lc = 0..15 hold 16 consecutive (a, m) columns of one output row, the four lane groups four rows: a wave
// instruction stores four whole runs of 16 elements (128 bytes in float64), and a wave's NT tiles of one
// register continue each other's run (16 NT consecutive columns of a row, stored back to back).  Columns
// past A M and rows past the fold's end are masked at the store; no workspace, no atomics.
#pragma once

struct PredictArgs {
  const void *X, *muX, *sdX, *muY, *sdY, *B;
  void *out;
  const int64_t *idx, *offs;    // idx == nullptr: the fold's rows are offs[f] .. offs[f + 1] - 1 themselves
  int64_t ldX;                  // row pitch of X in elements
  int64_t b0;                   // flat number of this launch's first workgroup
  int64_t n_chunks;             // row chunks of the longest fold
  int K, M, A;
  int groups;                   // column groups: the workgroups are folds x groups x chunks, flat, cut into launches
  int st_in_lds;                // the fold's K means and reciprocal standard deviations fit in LDS next to the stages
  int by_row;                   // output row: 0 = position in idx, 1 = the row number
};

template <typename T, int NT, int V>
__global__ __launch_bounds__(256) void predict_kernel(const PredictArgs a) {
  constexpr int W = 64 * NT;
  SSE_STAMP_START;
  const int K = a.K, M = a.M, C = a.A * M;
  // flat workgroup number (any number of folds, folds of any length): chunk fastest, then the column group,
  // then the fold
  const int64_t wg = a.b0 + blockIdx.x;
  const int64_t per_fold = a.n_chunks * a.groups;
  const int64_t f = wg / per_fold, rem = wg - f * per_fold;
  const int cg = (int)(rem / a.n_chunks);
  const int64_t r0 = (rem - cg * a.n_chunks) * SSE_ROWS;
  const int64_t o0 = a.offs[f];
  const int64_t n = a.offs[f + 1] - o0;
  if (r0 >= n) return;                                        // past this fold's rows (an empty fold: every chunk)
  const int nr = n - r0 < SSE_ROWS ? (int)(n - r0) : SSE_ROWS;  // rows of this chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lk = lane >> 4, lc = lane & 15;
  const int c0 = cg * W;
  const int Cg = C - c0 < W ? C - c0 : W;                     // columns of this group
  extern __shared__ __attribute__((aligned(16))) unsigned char predict_smem[];
  __shared__ int64_t rows[SSE_ROWS];
  const T *X = (const T *)a.X;
  const int64_t ldX = a.ldX;
  const T *muX = a.muX ? (const T *)a.muX + (size_t)f * K : nullptr;
  const T *sdX = a.sdX ? (const T *)a.sdX + (size_t)f * K : nullptr;
  const T *Bf = (const T *)a.B + (size_t)f * a.A * K * M;
  if (tid < SSE_ROWS) {
    const bool ok = tid < nr;                                 // (rows past the end re-read the chunk's first row)
    const int64_t p = o0 + r0 + (ok ? tid : 0);
    rows[tid] = a.idx ? a.idx[p] : p;
  }
  __syncthreads();
  const int st_in_lds = a.st_in_lds;
  unsigned char *smem = predict_smem;
  using Rcp = PredictRcp;
#include "tile_product_loop.hpp"
  // register r of tile (rt, t) is (row 16 rt + drow(lane, r), column 16 (wave NT + t) + lc): per register the
  // wave's NT tiles one after the other, so that consecutive store instructions continue the same four rows
  const T *muY = a.muY ? (const T *)a.muY + (size_t)f * M : nullptr;
  const T *sdY = a.sdY ? (const T *)a.sdY + (size_t)f * M : nullptr;
  T *out = (T *)a.out;
  double sy[NT], my[NT];
  bool valid[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int lcol = 16 * (wave * NT + t) + lc;
    valid[t] = lcol < Cg;
    const int m = valid[t] ? (c0 + lcol) % M : 0;
    sy[t] = sdY ? (double)sdY[m] : 1.0;
    my[t] = muY ? (double)muY[m] : 0.0;
  }
  // (the statistics are in registers HERE: left to itself the compiler sinks each load into the branch around
  //  the store that uses it, and every store then waits for all vector-memory work in flight, the stores before
  //  it included)
#pragma unroll
  for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(sy[t]), "+v"(my[t]));
  const int colw = c0 + 16 * wave * NT + lc;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 16 * rt + MF<T>::drow(lane, r);
      const bool rok = lr < nr;
      const int64_t orow = a.by_row ? rows[lr] : o0 + r0 + lr;
      T *op = out + orow * (int64_t)C + colw;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const T v = (T)((double)acc[rt][t][r] * sy[t] + my[t]);
        if (rok && valid[t]) op[16 * t] = v;
      }
    }
}

// The launch plan, host arithmetic alone (cvm_cv_predict_plan hands it out, next to tile_plan's choices: tests
// check both without a device).
// A launch's global size in x, workgroups x 256 threads, must stay below 2^32 (the HIP runtime refuses more),
// so a launch has at most 2^24 - 1 workgroups; the flat list of folds x groups x chunks workgroups is cut into
// launches of that many wherever the cut falls -- inside a fold too -- and a kernel finds its place from the
// launch's first flat number.  No limit on the number of folds or on the length of a fold follows from it.
constexpr int64_t PREDICT_MAX_WGS = ((int64_t)1 << 32) / 256 - 1;
struct PredictPlan {
  int64_t chunks, total, launches;    // row chunks of the longest fold, workgroups in all, launches
};

PredictPlan predict_plan(int64_t F, int64_t max_rows, int groups) {
  PredictPlan p;
  p.chunks = (max_rows + SSE_ROWS - 1) / SSE_ROWS;
  if (p.chunks < 1) p.chunks = 1;
  p.total = F * p.chunks * groups;
  p.launches = (p.total + PREDICT_MAX_WGS - 1) / PREDICT_MAX_WGS;
  return p;
}

template <typename T>
int predict_impl(const void *X, int64_t ldX, const int64_t *idx, const int64_t *offsets, int64_t F, int64_t max_rows,
                 int K, int M, int A, const void *muX, const void *sdX, const void *muY, const void *sdY,
                 const void *B, void *out, int by_row, hipStream_t st) {
  if (F == 0) return CVM_OK;
  PredictArgs a;
  memset(&a, 0, sizeof(a));
  a.X = X; a.muX = muX; a.sdX = sdX; a.muY = muY; a.sdY = sdY; a.B = B; a.out = out;
  a.idx = idx; a.offs = offsets; a.ldX = ldX; a.K = K; a.M = M; a.A = A; a.by_row = by_row;
  const TilePlan t = tile_plan(K, M, A, (int)sizeof(T), tile_vec(16 / (int)sizeof(T), X, ldX, K, M, muX, sdX, B));
  const PredictPlan p = predict_plan(F, max_rows, t.groups);
  a.n_chunks = p.chunks; a.groups = t.groups; a.st_in_lds = t.st_in_lds;
  void (*kern)(const PredictArgs) = nullptr;
  TILE_PICK(predict_kernel, T, t, kern)
  if (!kern) return fail(CVM_EINVAL, "cvm_cv_predict: no kernel for this shape%s");
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds));
  for (int64_t b0 = 0; b0 < p.total; b0 += PREDICT_MAX_WGS) {
    const int64_t nb = p.total - b0 < PREDICT_MAX_WGS ? p.total - b0 : PREDICT_MAX_WGS;
    a.b0 = b0;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), t.lds, st, a);
    HIP_OK(hipGetLastError());
  }
  return CVM_OK;
}
