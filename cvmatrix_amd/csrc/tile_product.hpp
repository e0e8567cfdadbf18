// tile_product.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, before its
// two users validation_sse.hpp and predict.hpp).
// The products both of them form, for one workgroup's 64 rows of one fold and W = 64 NT of the fold's A M
// coefficient columns (a, m):
//   acc[row][column] = sum over k of z[row][k] B[k][column],   z = (T)((x - muX) * (1 / sdX))
// with the rows of X gathered by number and standardised on the way to LDS.  The scorer (pls_sse_kernel)
// reduces them to one squared-error sum per column, cvm_cv_predict (predict_kernel) stores them whole; each
// kernel keeps its own grid decoding, `rows` prologue and epilogue.  Here: the constants, the two reciprocals
// and the host's choice among the variants (tile_plan, TILE_PICK); the loop itself is tile_product_loop.hpp,
// which each of the two kernels includes in its body.
//
// THE SCHEME, found out on this chip.  One workgroup per CU where the tiles are wide (the two LDS stages of B
// take most of it), one wave per SIMD; wave w owns the 16 NT columns from 16 NT w on, for all 64 rows: 4 x NT
// MFMA tiles (MF<T>, 16 x 16 x 4), 4 A and NT B fragment reads per 4 NT MFMAs.  The matrix pipe of a SIMD is
// never shared with another wave's vector arithmetic: a VALU instruction behind a stream of float64 MFMAs of
// ANOTHER wave waits hundreds of cycles (tools/dma_vs_mfma.hip -- 64 x 64 tiles at several workgroups per CU
// stood at 24 TFLOP/s).  The standardised rows and the coefficient columns go through two LDS stages 16 k at a
// time, one barrier per stage: the next stage is requested while this one is multiplied and written to the
// other buffer behind it.
// V: elements per global load -- 16 bytes' worth where K, M, the row pitch and every address allow it
// (tile_vec), else 1.  A vector-memory instruction costs the issuing wave hundreds of cycles on a busy CU
// (tools/dma_issue.hip) and these waves also feed the matrix cores: 32 eight-byte loads per thread and stage
// held the float64 kernel at 25 TFLOP/s; with 16-byte loads and the statistics in LDS a stage takes 12, and
// dealing them out between the MFMAs (below) brought 33.
// FIXED ORDER.  One product is ONE accumulator chain: k runs over stages of 16 and steps of 4 (k past K
// multiplies zeros), whatever NT, V, the number of column groups and the place of the statistics are.
#pragma once

constexpr int SSE_ROWS = 64, SSE_KS = 16, SSE_ZP = 80, SSE_MAXNT = 6;   // (Z pitch 80: conflict-free MFMA operand reads)

// The -DCVM_STAMPS build (tools/sse_stamps.py): workgroup 0 of whichever kernel runs the loop adds the cycles
// since its last stamp to counter i -- 0 prologue, 2 the stage's MFMAs with the next stage's requests and
// writes, 4 the barrier, 5 the kernel's epilogue.  The normal build holds no trace of them.
#ifdef CVM_STAMPS
__device__ unsigned long long g_sse_stamps[8];
#define SSE_STAMP_START unsigned long long sstamp_ = __builtin_readcyclecounter()
#define SSE_STAMP(i) do { if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) { const unsigned long long now_ = __builtin_readcyclecounter(); g_sse_stamps[i] += now_ - sstamp_; sstamp_ = now_; } } while (0)
#else
#define SSE_STAMP_START
#define SSE_STAMP(i)
#endif

// The reciprocal of a standard deviation.  `lds`: where the fold's K reciprocals are formed once and kept in
// LDS; `reg`: where every thread forms its own from the loaded sdX, stage by stage.  Two instances, because
// each kernel's bits are what they were before the loop was shared: the scorer divides on the first route and
// takes v_rcp_f64 with ONE Newton step on the second (within a unit of the division), so its sums may differ
// in the last places between the routes; predictions promise the same bits on every route (predict.hpp,
// FIXED ORDER) and use predict_rcp on both.  (The scorer could take predict_rcp too -- a change of its bits,
// left for a pull request of its own: DESIGN.md 4.9.)
//
// predict_rcp: v_rcp_f64 and TWO Newton steps.  The instruction's result is good to about 2^-24 relative (its
// documented accuracy is 2^29 units in the last place), one step r (2 - sd r) squares that to 2^-48 -- tens of
// units -- and the second to 2^-96; each step is two fused multiply-adds whose first forms the residual
// 1 - sd r with one rounding of a number that small, so what is left is the last step's own rounding:
// r = (1 / sd) (1 + d), |d| <= 2^-53 + 2^-94, one unit as the gate of the tests takes it.  (A zero, infinite
// or NaN sd gives NaN, never a finite number.)
__device__ __forceinline__ double predict_rcp(double sd) {
  double r = __builtin_amdgcn_rcp(sd);
  r = fma(fma(-sd, r, 1.0), r, r);
  return fma(fma(-sd, r, 1.0), r, r);
}
struct ScorerRcp {
  // (the division alone would turn an infinite sd into the reciprocal 0 and the fold's sums into finite numbers
  //  that ignore the column; NaN as on the other route and in predict_rcp.  sd - sd is +0 for a finite sd, which
  //  keeps the division's bits -- 1 / sd is never -0 -- and NaN for an infinite or NaN one; no compare, no select:
  //  a select cost pls_sse_kernel<double, 1, 2> three SGPRs, this form none in any variant.)
  static __device__ __forceinline__ double lds(double sd) { return 1.0 / sd + (sd - sd); }
  static __device__ __forceinline__ double reg(double sd) {
    const double r = __builtin_amdgcn_rcp(sd);
    return fma(fma(-sd, r, 1.0), r, r);
  }
};
struct PredictRcp {
  static __device__ __forceinline__ double lds(double sd) { return predict_rcp(sd); }
  static __device__ __forceinline__ double reg(double sd) { return predict_rcp(sd); }
};

// ----------------------------------------------------------------------------------
// The host's choice among the variants, arithmetic alone (cvm_cv_predict_plan hands it out: tests check it
// without a device).  None of the choices changes a bit of a product (FIXED ORDER).
// ----------------------------------------------------------------------------------
// `vec`: K, M, the row pitch and every address allow 16-byte loads of VW elements.
bool tile_vec(int VW, const void *X, int64_t ldX, int K, int M, const void *muX, const void *sdX, const void *B) {
  auto al16 = [](const void *q) { return !q || (uintptr_t)q % 16 == 0; };
  return K % VW == 0 && M % VW == 0 && ldX % VW == 0 && K >= 4 && al16(X) && al16(B) && al16(muX) && al16(sdX);
}

// Which (T, NT, V) exist: float64 takes five column tiles per wave at most, four without 16-byte pieces -- the
// wider variants of those combinations spill (33 / 90 registers at six tiles, 3 at five scalar ones).
constexpr int tile_max_nt(int esize, bool vec) { return esize == 8 ? (vec ? 5 : 4) : SSE_MAXNT; }

struct TilePlan {
  int nt, vec, groups, st_in_lds;
  size_t lds;
};

TilePlan tile_plan(int K, int M, int A, int esize, bool vec) {
  TilePlan p;
  p.vec = vec ? 1 : 0;
  const int C = A * M;
  // 16 NT columns per wave: as few column groups as possible (every group stages the rows again), then as
  // little padding as possible
  int best = 1 << 30;
  p.nt = 1;
  for (int c = 1; c <= tile_max_nt(esize, vec); ++c) {
    const int groups = (C + 64 * c - 1) / (64 * c);
    const int cost = groups * (4 * c + 1);
    if (cost < best) { best = cost; p.nt = c; }
  }
  p.groups = (C + 64 * p.nt - 1) / (64 * p.nt);
  p.lds = (size_t)2 * SSE_KS * (SSE_ZP + 64 * p.nt + 16) * esize;
  // (statistics in LDS only where they do not cost residency: one workgroup per CU anyway, or a short K)
  p.st_in_lds = (p.lds + (size_t)K * 16 + 2048 <= LDS_BUDGET && (p.lds > 80 * 1024 || K <= 512)) ? 1 : 0;
  if (p.st_in_lds) p.lds += (size_t)K * 16;
  return p;
}

// kern = KERNEL<T, p.nt, 16 bytes' worth or 1>, for a kernel template KERNEL<T, NT, V>; left as it is where
// the plan names a variant that does not exist
#define TILE_PICK_CASE(KERNEL, T, N, p, kern)                                                  \
  case N:                                                                                      \
    if constexpr (N <= tile_max_nt(sizeof(T), true)) { if ((p).vec) kern = KERNEL<T, N, 16 / (int)sizeof(T)>; } \
    if constexpr (N <= tile_max_nt(sizeof(T), false)) { if (!(p).vec) kern = KERNEL<T, N, 1>; } \
    break;
#define TILE_PICK(KERNEL, T, p, kern)                                                          \
  switch ((p).nt) {                                                                            \
    TILE_PICK_CASE(KERNEL, T, 1, p, kern) TILE_PICK_CASE(KERNEL, T, 2, p, kern)                \
    TILE_PICK_CASE(KERNEL, T, 3, p, kern) TILE_PICK_CASE(KERNEL, T, 4, p, kern)                \
    TILE_PICK_CASE(KERNEL, T, 5, p, kern) TILE_PICK_CASE(KERNEL, T, 6, p, kern)                \
    default: break;                                                                            \
  }
static_assert(SSE_MAXNT == 6, "TILE_PICK lists the tile counts");
