// omp.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after enet.hpp, whose
// enet_lane / enet_sync / enet_finite it uses).
// Orthogonal matching pursuit (greedy forward selection) on the training matrices of every fold: for fold f and
// response m, with G = XTX[f], h = XTY[f][:, m], and S the ordered list of selected indices, step a = 0 .. A - 1
//   1. alpha = h - G[:, S] gamma           (gamma: the least-squares coefficients on S; alpha = h while S is empty)
//   2. score_k = |alpha_k|  (normalize: |alpha_k| / sqrt(G_kk), columns whose G_kk is not > 0 left out), k not in S
//   3. j = the index of the largest score, the lowest index among equal scores; a largest score that is not > 0
//      (no candidate, or nothing left to explain) ends the path
//   4. w = L^-1 G[S, j], d^2 = G_jj - w'w extend the Cholesky factor L of G_SS; d^2 <= rank_tol G_jj ends the path
//   5. L L' gamma = h_S;  B[f][a][:, m] = gamma scattered to S, exactly 0 elsewhere.
// F x M independent PATHS, one wavefront (a workgroup of 64 threads) per path, dealt to the workspace
// slots by slot_first (fit_plan.hpp).  All arithmetic in float64, inputs widened on load, B rounded once on store.
//
// Per path: lane i holds the index, gamma, z = (L^-1 h_S)_i and the diagonal L_ii of selected variable i in
// registers.  The strict lower triangle of L (64 x 64) lies in LDS with a pitch of 65 doubles: the column read of
// the forward substitution (lane i reads L[i][c]) then touches 32 distinct bank pairs per half wave, and the row
// read of the backward substitution is contiguous.  The part of that array to the right of the diagonal keeps the
// coefficients of every step (gamma of step a in column a + 1, rows 0 .. a), so B is written once, after the path's
// status is known: steps 0 .. n_fit - 1, the padding (steps >= n_fit repeat step n_fit - 1) and the all-NaN path
// of status -1 in one loop.  A K-byte slot map in LDS tells a lane whether a coordinate is selected; the path's
// workspace slot holds the score scale of every coordinate (1, or 1 / sqrt(G_kk), 0 where the column may not be
// selected), screened once so that the strided diagonal is read once.
//   * alpha and the argmax in one pass over K in pieces of 256 coordinates, four per lane: the rows of G of the
//     selected variables (G is symmetric: row idx_a is contiguous) in ascending slot order, one fma per term;
//     alpha is never stored.  Each lane keeps its best (score, index) and a not-finite flag (fmax and > both
//     drop a NaN); a butterfly over the pair with the lowest-index tie-break ends the pass.
//   * the new row: lane i gathers G[j][idx_i]; n dependent steps of a lane broadcast, a division and one LDS
//     column read; w'w and w'z by a butterfly sum (a fixed order).
//   * the coefficients: z gains one entry, then n dependent steps of the backward substitution L' gamma = z.
// No workgroup barrier, no atomics; order of every sum and comparison depends on the path's inputs alone:
// bit-reproducible, whatever the batch around the path or the workspace size.
#pragma once

constexpr int OMP_MAXK = 4096;
constexpr int OMP_MAXM = 64;
constexpr int OMP_CAP = 64;               // selected variables at most: one per lane
constexpr int OMP_PITCH = OMP_CAP + 1;    // doubles per row of L: odd, so a column read across lanes is conflict-free
constexpr int OMP_MAXWG = 1024;           // paths in flight at most

struct OmpArgs {
  const void *XTX, *XTY;                  // [F][K][K], [F][K][M]
  void *B;                                // [F][A][K][M]
  int32_t *support, *n_fit;               // [F][A][M], [F][M]
  double *ws;                             // G slots of `per` doubles: the score scale of the path's coordinates
  int64_t P;                              // paths F * M
  size_t per;
  int K, M, A, G, normalize;
  double rank_tol;
};

inline size_t omp_path_bytes(int K) { return align_up((size_t)K * 8, 256); }

__device__ inline double omp_wave_sum(double v) {              // all 64 lanes active; the same bits in every lane
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__global__ __launch_bounds__(64) void omp_kernel(const OmpArgs a) {
  __shared__ double Ls[OMP_CAP * OMP_PITCH];                   // L below the diagonal, the steps' gamma to its right
  __shared__ unsigned char slotof[OMP_MAXK];                   // K bytes: slot + 1, or 0
  const int K = a.K, M = a.M, A = a.A, G = a.G;
  const int lane = threadIdx.x;
  const bool normalize = a.normalize != 0;
  const int b = blockIdx.x, t = slot_first(b, G);
  double *scale = a.ws + (size_t)b * a.per;
  const double nan = __builtin_nan("");

  for (int64_t s = t; s < a.P; s += G) {
    const int64_t f = s / M;
    const int m = (int)(s - f * M);
    const T *Gm = (const T *)a.XTX + (size_t)f * K * K;
    const T *H = (const T *)a.XTY + (size_t)f * K * M + m;
    // the score scale into the slot, and whether the diagonal or h holds a non-finite value
    bool bad = false;
    for (int k = lane; k < K; k += 64) {
      const double d = (double)Gm[(size_t)k * K + k], h = (double)H[(size_t)k * M];
      bad |= !enet_finite(d) || !enet_finite(h);
      scale[k] = normalize ? (d > 0.0 ? 1.0 / sqrt(d) : 0.0) : 1.0;
      slotof[k] = 0;
    }
    bool dead = __any(bad);
    enet_sync();
    int n = 0, idx = 0;
    double gam = 0.0, z = 0.0, diag = 1.0;

    for (int step = 0; step < A && !dead; ++step) {
      // ---- alpha = h - G[:, S] gamma and the best candidate, in one pass
      double best = -1.0;
      int bidx = 0x7fffffff;
      for (int k0 = 0; k0 < K; k0 += 256) {
        double acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + 64 * u + lane;
          acc[u] = k < K ? (double)H[(size_t)k * M] : 0.0;
        }
        for (int j = 0; j < n; ++j) {
          const double gj = enet_lane(gam, j);
          const T *row = Gm + (size_t)__builtin_amdgcn_readlane(idx, j) * K;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u + lane;
            if (k < K) acc[u] = fma(-gj, (double)row[k], acc[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + 64 * u + lane;
          if (k < K) {
            const double sc = scale[k], sk = fabs(acc[u]) * sc;
            bad |= !enet_finite(acc[u]) || !enet_finite(sk);
            if (!slotof[k] && sc > 0.0 && sk > best) {         // (ascending k within a lane: the lowest index stays)
              best = sk;
              bidx = k;
            }
          }
        }
      }
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const double s2 = __shfl_xor(best, o);
        const int i2 = __shfl_xor(bidx, o);
        if (s2 > best || (s2 == best && i2 < bidx)) {
          best = s2;
          bidx = i2;
        }
      }
      if (__any(bad)) { dead = true; break; }
      if (!(best > 0.0)) break;                                // no candidate, or every remaining alpha is zero
      const int j = __builtin_amdgcn_readfirstlane(bidx);
      // ---- the new row of L: w = L^-1 G[S, j] by n dependent column steps
      const double Gjj = (double)Gm[(size_t)j * K + j], hj = (double)H[(size_t)j * M];
      double g = lane < n ? (double)Gm[(size_t)j * K + idx] : 0.0;
      double w = 0.0;
      for (int c = 0; c < n; ++c) {
        const double wc = enet_lane(g, c) / enet_lane(diag, c);
        if (lane == c) w = wc;
        if (lane > c && lane < n) g = fma(-Ls[lane * OMP_PITCH + c], wc, g);
      }
      const double ww = omp_wave_sum(w * w), wz = omp_wave_sum(w * z);
      const double d2 = Gjj - ww;
      if (!enet_finite(d2)) { dead = true; break; }
      if (d2 <= a.rank_tol * Gjj) break;                       // the best candidate depends on S: the path ends
      const double d = sqrt(d2);
      if (lane < n) Ls[n * OMP_PITCH + lane] = w;
      if (lane == n) {
        idx = j;
        diag = d;
        z = (hj - wz) / d;
        slotof[j] = (unsigned char)(n + 1);
      }
      ++n;
      enet_sync();
      // ---- L' gamma = z by n dependent row steps
      double zz = z;
      for (int c = n - 1; c >= 0; --c) {
        const double gc = enet_lane(zz, c) / enet_lane(diag, c);
        if (lane == c) gam = gc;
        if (lane < c) zz = fma(-Ls[c * OMP_PITCH + lane], gc, zz);
      }
      if (__any(lane < n && !enet_finite(gam))) { dead = true; break; }
      if (lane < n) Ls[lane * OMP_PITCH + n] = gam;            // step n - 1 of the path: column n, rows 0 .. n - 1
    }
    enet_sync();

    // ---- B[f][:][:, m], support and n_fit, written here and nowhere else: the steps taken, then the padding
    for (int ai = 0; ai < A; ++ai) {
      const int col = ai < n ? ai + 1 : n;                     // (n == 0: column 0, which no slot reaches: zeros)
      T *Bo = (T *)a.B + ((size_t)(f * A + ai) * K) * M + m;
      for (int k = lane; k < K; k += 64) {
        const int sl = slotof[k];
        double v = (sl && sl <= col) ? Ls[(sl - 1) * OMP_PITCH + col] : 0.0;
        if (dead) v = nan;
        Bo[(size_t)k * M] = (T)v;
      }
    }
    if (lane < A) a.support[(f * A + lane) * M + m] = (!dead && lane < n) ? idx : -1;
    if (lane == 0) a.n_fit[s] = dead ? -1 : n;
    enet_sync();
  }
}

// Workspace for full concurrency: min(F M, OMP_MAXWG) slots.  Host arithmetic only (no device query).
size_t omp_workspace_bytes(int64_t F, int K, int M) {
  return slot_workspace_bytes(F * (int64_t)M, omp_path_bytes(K), OMP_MAXWG);
}

template <typename T>
int omp_fit_impl(const void *XTX, const void *XTY, int64_t F, int K, int M, int A, int normalize, double rank_tol,
                 void *B, int32_t *support, int32_t *n_fit, void *ws, size_t ws_bytes, hipStream_t st) {
  const size_t per = omp_path_bytes(K);
  if (ws_bytes < per) return fail(CVM_EWORKSPACE, "cvm_omp_fit: workspace too small for one path%s");
  if (F == 0) return CVM_OK;
  OmpArgs a;
  memset(&a, 0, sizeof(a));
  a.XTX = XTX; a.XTY = XTY; a.B = B; a.support = support; a.n_fit = n_fit;
  a.ws = reinterpret_cast<double *>(ws);
  a.P = F * (int64_t)M;
  a.per = per / 8;
  a.K = K; a.M = M; a.A = A; a.normalize = normalize;
  a.rank_tol = rank_tol;
  a.G = slot_count(a.P, per, ws_bytes, OMP_MAXWG);
  hipLaunchKernelGGL((omp_kernel<T>), dim3((unsigned)a.G), dim3(64), 0, st, a);
  HIP_OK(hipGetLastError());
  return CVM_OK;
}
