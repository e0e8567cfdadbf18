// ridge.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after pls.hpp).
// Ridge regression over a grid of penalties for every fold: for fold f and penalty l,
//   (XTX[f] + lambda_l I) B[f][l] = XTY[f]
// F x L independent SPD problems of order K with M right-hand sides, one persistent workgroup per workspace slot,
// the problems dealt to the slots by slot_first (fit_plan.hpp).
//
// Per problem (all arithmetic in float64, inputs widened on load, B rounded once on store):
//   * blocked left-looking Cholesky of the augmented K + M rows [XTX + lambda I ; XTY^T]: its last M rows
//     come out as Z^T with L Z = XTY, so the forward substitution rides along in the same passes;
//   * the factor lives in the workgroup's workspace slot COLUMN-major (W[k][r] = L[r][k], leading dimension
//     ld = K + M rounded up to 32), so both MFMA operands of a panel update are 16 consecutive rows of a column;
//   * panel j (32 columns): (A + lambda I)[r][j..] - L[r][:j] L[j..][:j]^T, the products summed from zero on
//     v_mfma_f64_16x16x4_f64 and taken from A once, lambda added as the panel is read from XTX; the 32 x 32
//     diagonal block factored by one wave in registers (lane i holds row i, fixed order); the rows below it
//     solved against it, one thread per row;
//   * back substitution L^T B = Z by blocks of 32 rows from the bottom: the update by the rows below on MFMA,
//     cut over the four waves in a fixed interleave and summed in a fixed order, then the 32 x 32 solve.
// A pivot that is not finite or not > 0 ends the problem: info = its 1-based column, B all NaN (B is written
// only by the back substitution, so it is never half-written).  No float atomics; a problem's bits depend on
// its inputs alone, not on which workgroup ran it or what else was in the batch.
#pragma once

constexpr int RIDGE_THREADS = 256;
constexpr int RIDGE_NB = 32;            // panel width
constexpr int RIDGE_MAXK = 4096;
constexpr int RIDGE_MAXM = 64;
constexpr int RIDGE_MAXL = 256;
constexpr int RIDGE_MAXWG = 512;        // workgroups (problems in flight) at most

struct RidgeArgs {
  const void *XTX, *XTY;                // [F][K][K], [F][K][M]
  void *B;                              // [F][L][K][M]
  int32_t *info;                        // [F][L]
  double *ws;                           // G slots of `per` doubles
  int64_t P;                            // problems F * L
  size_t per;
  int K, M, L, ld, G;
  double lambdas[RIDGE_MAXL];
};

__host__ __device__ inline int ridge_ld(int K, int M) { return (K + M + 31) & ~31; }
// bytes of one problem's slot: the augmented factor, K columns of ld float64 (256-byte aligned)
inline size_t ridge_problem_bytes(int K, int M) { return align_up((size_t)K * ridge_ld(K, M) * 8, 256); }

template <typename T>
__global__ __launch_bounds__(RIDGE_THREADS) void ridge_kernel(const RidgeArgs a) {
  __shared__ double dg[RIDGE_NB][RIDGE_NB + 1];               // diagonal block of L
  __shared__ double part[4][RIDGE_NB][RIDGE_MAXM + 1];        // back substitution: one partial sum per wave
  __shared__ double colb[64];
  __shared__ int fail_at;
  const int K = a.K, M = a.M, L = a.L, ld = a.ld, G = a.G;
  const int R = K + M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, sub = lane >> 4;
  const int b = blockIdx.x, t = slot_first(b, G);
  double *W = a.ws + (size_t)b * a.per;

  for (int64_t s = t; s < a.P; s += G) {
    const int64_t f = s / L;
    const double lam = a.lambdas[s - f * L];
    const T *X = (const T *)a.XTX + (size_t)f * K * K;
    const T *Y = (const T *)a.XTY + (size_t)f * K * M;
    T *Bo = (T *)a.B + (size_t)s * K * M;
    if (tid == 0) fail_at = 0;
    __syncthreads();

    for (int j0 = 0; j0 < K; j0 += RIDGE_NB) {
      const int nbp = K - j0 < RIDGE_NB ? K - j0 : RIDGE_NB;
      // 1. panel: rows [j0, R) x columns [j0, j0 + nbp); wave w takes row blocks of 32 in turn
      for (int r0 = j0 + 32 * wave; r0 < R; r0 += 128) {
        // acc = -L[r][:j0] L[j0 + c][:j0]^T, summed from zero and added to A once at the end: a sum that starts
        // from the entry of A rounds at the size of that entry at every one of its j0 steps, which on a matrix
        // with a heavy diagonal (a large lambda) costs sqrt(K) roundings where the products themselves are small.
        // Rows past R hold whatever the slot holds: they feed only output rows that are not stored (ld is a
        // multiple of 32, so the reads stay inside the column).
        // (the entries of A are loaded ahead of the loop, so their latency passes under it)
        pls_v4d acc[2][2], av[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int cj = 0; cj < 2; ++cj) {
            acc[ti][cj] = pls_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int r = r0 + 16 * ti + sub + 4 * q, c = 16 * cj + col;
              double v = 0.0;
              if (c < nbp && r < R) {
                // (XTX symmetric: row j0 + c read along r is column j0 + c)
                v = r < K ? (double)X[(size_t)(j0 + c) * K + r] : (double)Y[(size_t)(j0 + c) * M + (r - K)];
                if (r == j0 + c) v += lam;
              }
              av[ti][cj][q] = v;
            }
          }
#pragma unroll 4
        for (int k0 = 0; k0 < j0; k0 += 4) {
          const double *wk = W + (size_t)(k0 + sub) * ld;
          const double a0 = -wk[r0 + col], a1 = -wk[r0 + 16 + col];
          const double b0 = wk[j0 + col], b1 = wk[j0 + 16 + col];
          acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int cj = 0; cj < 2; ++cj)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int r = r0 + 16 * ti + sub + 4 * q, c = 16 * cj + col;
              if (c < nbp && r < R) W[(size_t)(j0 + c) * ld + r] = av[ti][cj][q] + acc[ti][cj][q];
            }
      }
      __syncthreads();
      // 2. diagonal block: one wave, lane i holds row i; right-looking, columns in order
      if (wave == 0) {
        double rw[RIDGE_NB];
#pragma unroll
        for (int c = 0; c < RIDGE_NB; ++c)
          rw[c] = (lane < nbp && c <= lane) ? W[(size_t)(j0 + c) * ld + j0 + lane] : 0.0;
        int bad = 0;
#pragma unroll
        for (int j = 0; j < RIDGE_NB; ++j) {
          if (j < nbp && !bad) {
            const double piv = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(rw[j]), j),
                                                __builtin_amdgcn_readlane(__double2loint(rw[j]), j));
            if (!(piv > 0.0) || isinf(piv)) {
              bad = j0 + j + 1;
            } else {
              const double d = sqrt(piv);
              const double lij = lane == j ? d : rw[j] / d;
              rw[j] = lane >= j ? lij : 0.0;
              colb[lane] = lij;                                // column j, read back by every lane
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
              for (int k = j + 1; k < RIDGE_NB; ++k)
                if (lane >= k) rw[k] = fma(-lij, colb[k], rw[k]);
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_wave_barrier();
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
          }
        }
        if (bad) {
          if (lane == 0) fail_at = bad;
        } else if (lane < nbp) {
#pragma unroll
          for (int c = 0; c < RIDGE_NB; ++c)
            if (c <= lane) {
              dg[lane][c] = rw[c];
              W[(size_t)(j0 + c) * ld + j0 + lane] = rw[c];
            }
        }
      }
      __syncthreads();
      if (fail_at) break;
      // 3. rows below the block: x L_jj^T = panel row, one thread per row (the barrier that ends a round
      //    also keeps the compiler from hoisting the whole block into registers across the rounds)
      for (int rb = j0 + nbp; rb < R; rb += RIDGE_THREADS) {
        const int r = rb + tid;
        if (r < R) {
          double x[RIDGE_NB];
#pragma unroll
          for (int c = 0; c < RIDGE_NB; ++c) x[c] = c < nbp ? W[(size_t)(j0 + c) * ld + r] : 0.0;
#pragma unroll
          for (int c = 0; c < RIDGE_NB; ++c) {
            if (c < nbp) {
              double v = x[c];
#pragma unroll
              for (int u = 0; u < c; ++u) v = fma(-x[u], dg[c][u], v);
              x[c] = v / dg[c][c];
            }
          }
#pragma unroll
          for (int c = 0; c < RIDGE_NB; ++c)
            if (c < nbp) W[(size_t)(j0 + c) * ld + r] = x[c];
        }
        __syncthreads();
      }
      __syncthreads();
    }

    const int bad = fail_at;
    if (bad) {
      const double nan = __builtin_nan("");
      for (size_t i = tid; i < (size_t)K * M; i += RIDGE_THREADS) Bo[i] = (T)nan;
      if (tid == 0) a.info[s] = bad;
      __syncthreads();
      continue;
    }

    // 4. back substitution L^T B = Z from the bottom block up; B (float64) replaces Z in rows K.. of the slot
    const int MT = (M + 15) >> 4;
    for (int k0 = ((K - 1) / RIDGE_NB) * RIDGE_NB; k0 >= 0; k0 -= RIDGE_NB) {
      const int nbk = K - k0 < RIDGE_NB ? K - k0 : RIDGE_NB;
      const int i0 = k0 + nbk;
      if (i0 < K) {
        // part[w][c][m] = sum over the rows i >= i0 of wave w's k-steps of L[i][k0 + c] B[i][m]
        pls_v4d acc[2][4];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) acc[ti][mt] = pls_v4d{0.0, 0.0, 0.0, 0.0};
        for (int i = i0 + 4 * wave; i < K; i += 16) {
          const int ii = i + sub;
          const bool in = ii < K;
          const double a0 = in ? W[(size_t)(k0 + col) * ld + ii] : 0.0;
          const double a1 = in ? W[(size_t)(k0 + 16 + col) * ld + ii] : 0.0;
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) {
            if (mt < MT) {
              const int m = 16 * mt + col;
              const double bv = (in && m < M) ? W[(size_t)ii * ld + K + m] : 0.0;
              acc[0][mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc[0][mt], 0, 0, 0);
              acc[1][mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc[1][mt], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int c = 16 * ti + sub + 4 * q, m = 16 * mt + col;
              if (mt < MT && m < M) part[wave][c][m] = acc[ti][mt][q];
            }
      }
      for (int e = tid; e < nbk * nbk; e += RIDGE_THREADS) {
        const int rr = e / nbk, c = e - rr * nbk;
        if (rr >= c) dg[rr][c] = W[(size_t)(k0 + c) * ld + k0 + rr];
      }
      __syncthreads();
      if (tid < M) {
        const int m = tid;
        double x[RIDGE_NB];
#pragma unroll
        for (int c = 0; c < RIDGE_NB; ++c) {
          if (c < nbk) {
            double v = W[(size_t)(k0 + c) * ld + K + m];
            if (i0 < K) v -= ((part[0][c][m] + part[1][c][m]) + part[2][c][m]) + part[3][c][m];
            x[c] = v;
          }
        }
#pragma unroll
        for (int c = RIDGE_NB - 1; c >= 0; --c) {
          if (c < nbk) {
            double v = x[c];
#pragma unroll
            for (int u = c + 1; u < RIDGE_NB; ++u)
              if (u < nbk) v = fma(-dg[u][c], x[u], v);
            x[c] = v / dg[c][c];
            W[(size_t)(k0 + c) * ld + K + m] = x[c];
            Bo[(size_t)(k0 + c) * M + m] = (T)x[c];
          }
        }
      }
      __syncthreads();
    }
    if (tid == 0) a.info[s] = 0;
  }
}

// Workspace for full concurrency: min(F L, RIDGE_MAXWG) slots.  Host arithmetic only (no device query).
size_t ridge_workspace_bytes(int64_t F, int K, int M, int L) {
  return slot_workspace_bytes(F * (int64_t)L, ridge_problem_bytes(K, M), RIDGE_MAXWG);
}

template <typename T>
int ridge_fit_impl(const void *XTX, const void *XTY, int64_t F, int K, int M, const double *lambdas, int L, void *B,
                   int32_t *info, void *ws, size_t ws_bytes, hipStream_t st) {
  const size_t per = ridge_problem_bytes(K, M);
  if (ws_bytes < per) return fail(CVM_EWORKSPACE, "cvm_ridge_fit: workspace too small for one problem%s");
  if (F == 0) return CVM_OK;
  RidgeArgs a;
  memset(&a, 0, sizeof(a));
  a.XTX = XTX; a.XTY = XTY; a.B = B; a.info = info;
  a.ws = reinterpret_cast<double *>(ws);
  a.P = F * (int64_t)L;
  a.per = per / 8;
  a.K = K; a.M = M; a.L = L; a.ld = ridge_ld(K, M);
  a.G = slot_count(a.P, per, ws_bytes, RIDGE_MAXWG);
  for (int l = 0; l < L; ++l) a.lambdas[l] = lambdas[l];
  hipLaunchKernelGGL(ridge_kernel<T>, dim3((unsigned)a.G), dim3(RIDGE_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
  return CVM_OK;
}
