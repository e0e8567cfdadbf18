// pcr.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after ridge.hpp).
// PCA and principal component regression for every fold: the A leading eigenpairs of XTX[f] and the
// coefficients with 1 .. A components,
//   B[f][a] = sum over j <= a of v_j (v_j^T XTY[f]) / lambda_j,
// F independent symmetric eigenproblems of order K, one persistent workgroup per fold.
//
// Per fold (all arithmetic in float64, inputs widened on load, outputs rounded once on store):
//   * cyclic two-sided Jacobi with the round-robin ordering: with m = K rounded up to even, a sweep is m - 1
//     rounds of m / 2 disjoint pairs, round r pairing (m-1, r) and ((r+i) mod (m-1), (r-i) mod (m-1)); a pair
//     with index K (odd K) sits out;
//   * S (starts as XTX[f]) and V (starts as I) live in the workgroup's workspace slot, row-major with leading
//     dimension ld; a round computes the rotation of every pair from S as the last round left it, then applies
//     S <- J^T S J by 2 x 2 blocks (rows of pair i, columns of pair j; each block owned by one thread and
//     written once) and V <- V J by row and pair.  Every entry of the block is the sum of the same four
//     products in block (i,j) and in block (j,i), grouped alike, so S stays symmetric to the bit;
//   * pair (p,q) rotates iff |S_pq| > 2^-52 ||XTX[f]||_F (absolute: a relative test never ends on a matrix
//     without full rank); a sweep without a rotation ends the iteration, 60 sweeps are the cap;
//   * eigenvalues = diag(S) ordered by a counting rank (descending, ties by index), every component's entry
//     of largest magnitude made positive, n_fit from rank_tol, then the coefficients summed in the order
//     j = 0, 1, ... with their running sum in the slot (where S was); v_j^T XTY by a compensated dot product.
// A NaN or infinity in XTX[f] or XTY[f] (or a norm that overflows): every output of the fold NaN, n_fit -1,
// sweeps 0; the cap reached: the same with sweeps -1.  No float atomics, every sum in a fixed order; a fold's
// bits depend on its own matrices alone.
#pragma once

constexpr int PCR_THREADS = 256;
constexpr int PCR_MAXK = 512;
constexpr int PCR_MAXM = 64;
constexpr int PCR_MAXWG = 512;          // workgroups (folds in flight) at most
constexpr int PCR_MAXSWEEPS = 60;
constexpr int PCR_GBATCH = 2048;        // v_j^T XTY of a batch of components: float64 entries kept in LDS
constexpr int PCR_UN = 4;               // blocks a thread loads before it stores any (loads in flight)

struct PcrArgs {
  const void *XTX, *XTY;                // [F][K][K], [F][K][M] (XTY NULL: PCA only)
  void *B, *V;                          // [F][A][K][M], [F][K][A] (each may be NULL)
  double *eig;                          // [F][A]
  int32_t *n_fit, *sweeps;              // [F]
  double *ws;                           // G slots of `per` doubles
  int64_t F;
  size_t per;
  double rank_tol;
  int K, M, A, ld, G;
};

// leading dimension of S and V: K, or M where that is larger (the running sum of the coefficients, K x M,
// takes the place of S), rounded up to 4
__host__ __device__ inline int pcr_ld(int K, int M) { return ((K > M ? K : M) + 3) & ~3; }
// bytes of one fold's slot: S and V, K rows of ld float64 each (256-byte aligned)
inline size_t pcr_slot_bytes(int K, int M) { return align_up((size_t)2 * K * pcr_ld(K, M) * 8, 256); }

// Steps 3 and 4 for one fold whose S is diagonal to the threshold, by the NT threads of its workgroup: what
// pcr_kernel and the finish of the blocked solver (pcr_blocked.hpp) both end with.  S and V have leading
// dimension ld; lam (K), sgn (A), ord (K) and gs (PCR_GBATCH) are the caller's, in LDS or in its slot; the
// running sum acc (K x M) may take the place of S.
template <typename T, int NT, typename O>
__device__ __forceinline__ void pcr_finish_fold(const double *S, const double *V, const int ld, const int K, const int M,
                                                const int A, const double rank_tol, const int sweeps_run, const T *Y,
                                                T *Bo, T *Vo, double *Eo, int32_t *n_fit_out, int32_t *sweeps_out,
                                                double *lam, double *sgn, double *gs, O *ord, int *nfit_s, double *acc,
                                                const int tid) {
  // 3. eigenvalues in descending order (counting rank, ties by index)
  for (int j = tid; j < K; j += NT) {
    lam[j] = S[(size_t)j * ld + j];
    ord[j] = (O)j;                                    // (every entry an index, whatever the comparisons below say)
  }
  __syncthreads();
  for (int j = tid; j < K; j += NT) {
    const double lj = lam[j];
    int rank = 0;
    for (int i = 0; i < K; ++i) rank += (lam[i] > lj) || (lam[i] == lj && i < j);
    ord[rank] = (O)j;
  }
  __syncthreads();
  if (tid == 0) {
    const double cut = rank_tol * lam[ord[0]];
    int n = 0;
    for (int j = 0; j < K; ++j) n += lam[j] > cut;
    *nfit_s = n < A ? n : A;
  }
  // sign: the entry of largest magnitude positive, the lowest index among equals
  for (int c = tid; c < A; c += NT) {
    const int col = ord[c];
    double best = -1.0, sg = 1.0;
    for (int k = 0; k < K; ++k) {
      const double v = V[(size_t)k * ld + col];
      if (fabs(v) > best) { best = fabs(v); sg = v < 0.0 ? -1.0 : 1.0; }
    }
    sgn[c] = sg;
  }
  __syncthreads();
  const int nfit = *nfit_s;
  for (int c = tid; c < A; c += NT) Eo[c] = lam[ord[c]];
  if (Vo)
    for (int e = tid; e < K * A; e += NT) {
      const int k = e / A, c = e - k * A;
      Vo[e] = c < nfit ? (T)(sgn[c] * V[(size_t)k * ld + ord[c]]) : (T)0.0;
    }
  if (tid == 0) {
    *n_fit_out = nfit;
    *sweeps_out = sweeps_run;
  }

  // 4. coefficients: the running sum acc[k][m], components in batches whose (v_j^T XTY) / lambda_j fit gs
  if (Bo) {
    const int KM = K * M;
    __syncthreads();                                  // (lam was read from S by other threads)
    if (nfit == 0)
      for (size_t i = tid; i < (size_t)A * KM; i += NT) Bo[i] = (T)0.0;
    const int jb = PCR_GBATCH / M;                    // components per batch (>= 32)
    for (int j0 = 0; j0 < nfit; j0 += jb) {
      const int nj = nfit - j0 < jb ? nfit - j0 : jb;
      for (int e = tid; e < nj * M; e += NT) {
        const int j = e / M, mm = e - j * M;
        const int col = ord[j0 + j];
        // v^T XTY[:, mm] cancels (a random direction against K entries): the products exactly by fma and
        // the roundings of the running sum carried along (a compensated dot product, k in order), so that
        // its error is a rounding of the result and not K roundings of the largest partial sum
        double g = 0.0, comp = 0.0;
        for (int k = 0; k < K; ++k) {
          const double x = V[(size_t)k * ld + col], y = (double)Y[(size_t)k * M + mm];
          const double pr = x * y, pe = fma(x, y, -pr);
          const double t = g + pr, z = t - g;
          comp += ((g - (t - z)) + (pr - z)) + pe;
          g = t;
        }
        gs[e] = (g + comp) / lam[col];
      }
      __syncthreads();
      for (int e = tid; e < KM; e += NT) {
        const int k = e / M, mm = e - k * M;
        double s = j0 ? acc[e] : 0.0;
        for (int j = 0; j < nj; ++j) {
          s += V[(size_t)k * ld + ord[j0 + j]] * gs[j * M + mm];
          Bo[(size_t)(j0 + j) * KM + e] = (T)s;
        }
        if (j0 + nj < nfit) {
          acc[e] = s;
        } else {
          for (int c = nfit; c < A; ++c) Bo[(size_t)c * KM + e] = (T)s;   // more components than exist
        }
      }
      __syncthreads();
    }
  }
}

template <typename T>
__global__ __launch_bounds__(PCR_THREADS) void pcr_kernel(const PcrArgs a) {
  __shared__ double red[PCR_THREADS];
  __shared__ double lam[PCR_MAXK];                    // diag(S) by index
  __shared__ double sgn[PCR_MAXK];                    // sign of component a
  __shared__ double gs[PCR_GBATCH];                   // (v_j^T XTY) / lambda_j of a batch of components
  __shared__ double rc[PCR_MAXK / 2], rs[PCR_MAXK / 2], rt[PCR_MAXK / 2], rb[PCR_MAXK / 2];
  __shared__ short rp[PCR_MAXK / 2], rq[PCR_MAXK / 2];
  __shared__ short ord[PCR_MAXK];                     // index of the a-th largest eigenvalue
  __shared__ unsigned char rf[PCR_MAXK / 2];          // pair rotates in this round
  __shared__ int flag, nfit_s;
  const int K = a.K, M = a.M, A = a.A, ld = a.ld, G = a.G;
  const int tid = threadIdx.x;
  const int m = (K + 1) & ~1, h = m >> 1;
  double *S = a.ws + (size_t)blockIdx.x * a.per;
  double *V = S + (size_t)K * ld;
  const double nan = __builtin_nan("");

  for (int64_t f = blockIdx.x; f < a.F; f += G) {
    const T *X = (const T *)a.XTX + (size_t)f * K * K;
    const T *Y = a.XTY ? (const T *)a.XTY + (size_t)f * K * M : nullptr;
    T *Bo = a.B ? (T *)a.B + (size_t)f * A * K * M : nullptr;
    T *Vo = a.V ? (T *)a.V + (size_t)f * K * A : nullptr;
    double *Eo = a.eig + (size_t)f * A;

    // 1. S = XTX[f], V = I; ||XTX[f]||_F^2 by thread in index order, then a fixed tree; anything not finite
    if (tid == 0) flag = 0;
    __syncthreads();
    double ss = 0.0;
    int bad = 0;
    for (int e = tid; e < K * K; e += PCR_THREADS) {
      const int r = e / K, c = e - r * K;
      const double v = (double)X[e];
      if (!(fabs(v) <= 1.79769313486231570815e+308)) bad = 1;
      ss += v * v;
      S[(size_t)r * ld + c] = v;
      V[(size_t)r * ld + c] = r == c ? 1.0 : 0.0;
    }
    if (Y)
      for (int e = tid; e < K * M; e += PCR_THREADS)
        if (!(fabs((double)Y[e]) <= 1.79769313486231570815e+308)) bad = 1;
    red[tid] = ss;
    if (bad) flag = 1;
    __syncthreads();
    for (int w = PCR_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) red[tid] = red[tid] + red[tid + w];
      __syncthreads();
    }
    const double fro = sqrt(red[0]);
    int status = 0;                                   // value of sweeps[f]
    if (flag || !(fro <= 1.79769313486231570815e+308)) status = -2;      // (-2: not finite, reported as 0)
    const double thr = 0x1p-52 * fro;
    __syncthreads();

    // 2. the sweeps
    for (int sweep = 1; status == 0; ++sweep) {
      if (sweep > PCR_MAXSWEEPS) { status = -1; break; }
      if (tid == 0) flag = 0;                         // a rotation in this sweep
      __syncthreads();
      for (int r = 0; r < m - 1; ++r) {
        // 2a. the pairs of round r and their rotations
        if (tid < h) {
          int u = tid == 0 ? m - 1 : (r + tid) % (m - 1);
          int v = tid == 0 ? r : (r - tid + (m - 1)) % (m - 1);
          const int p = u < v ? u : v, q = u < v ? v : u;
          double c = 1.0, s = 0.0, t = 0.0, spq = 0.0;
          int rot = 0;
          if (q < K) {
            spq = S[(size_t)p * ld + q];
            if (fabs(spq) > thr) {
              const double zeta = (S[(size_t)q * ld + q] - S[(size_t)p * ld + p]) / (2.0 * spq);
              t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
              c = 1.0 / sqrt(1.0 + t * t);
              s = c * t;
              rot = 1;
              flag = 1;
            }
          }
          rp[tid] = (short)p; rq[tid] = (short)q;     // (q == K: the bye; its row and column are not touched)
          rc[tid] = c; rs[tid] = s; rt[tid] = t; rb[tid] = spq; rf[tid] = (unsigned char)rot;
        }
        __syncthreads();
        // 2b. S <- J^T S J: block (i, j) = rows of pair i x columns of pair j, j fastest over the threads
        for (int e0 = tid; e0 < h * h; e0 += PCR_THREADS * PCR_UN) {
          double ba[PCR_UN], bb[PCR_UN], bc[PCR_UN], bd[PCR_UN];
          int act[PCR_UN];
#pragma unroll
          for (int un = 0; un < PCR_UN; ++un) {
            const int e = e0 + un * PCR_THREADS;
            act[un] = 0;
            ba[un] = bb[un] = bc[un] = bd[un] = 0.0;
            if (e < h * h) {
              const int i = e / h, j = e - i * h;
              if (rf[i] | rf[j]) {
                act[un] = 1;
                const int pi = rp[i], qi = rq[i], pj = rp[j], qj = rq[j];
                ba[un] = S[(size_t)pi * ld + pj];
                if (qj < K) bb[un] = S[(size_t)pi * ld + qj];
                if (qi < K) bc[un] = S[(size_t)qi * ld + pj];
                if (qi < K && qj < K) bd[un] = S[(size_t)qi * ld + qj];
              }
            }
          }
#pragma unroll
          for (int un = 0; un < PCR_UN; ++un) {
            if (!act[un]) continue;
            const int e = e0 + un * PCR_THREADS;
            const int i = e / h, j = e - i * h;
            const int pi = rp[i], qi = rq[i], pj = rp[j], qj = rq[j];
            double r11, r12, r21, r22;
            if (i == j) {                             // (rf[i] is set here)
              r11 = ba[un] - rt[i] * rb[i];
              r22 = bd[un] + rt[i] * rb[i];
              r12 = r21 = 0.0;
            } else {
              const double ci = rc[i], si = rs[i], cj = rc[j], sj = rs[j];
              const double cc = ci * cj, sc = si * cj, cs = ci * sj, s2 = si * sj;
              const double xa = ba[un], xb = bb[un], xc = bc[un], xd = bd[un];
              r11 = (cc * xa + s2 * xd) - (cs * xb + sc * xc);
              r12 = (cs * xa - sc * xd) + (cc * xb - s2 * xc);
              r21 = (sc * xa - cs * xd) + (cc * xc - s2 * xb);
              r22 = (s2 * xa + cc * xd) + (sc * xb + cs * xc);
            }
            S[(size_t)pi * ld + pj] = r11;
            if (qj < K) S[(size_t)pi * ld + qj] = r12;
            if (qi < K) S[(size_t)qi * ld + pj] = r21;
            if (qi < K && qj < K) S[(size_t)qi * ld + qj] = r22;
          }
        }
        // V <- V J: row k, pair j
        for (int e0 = tid; e0 < K * h; e0 += PCR_THREADS * PCR_UN) {
          double vp[PCR_UN], vq[PCR_UN];
          int act[PCR_UN];
#pragma unroll
          for (int un = 0; un < PCR_UN; ++un) {
            const int e = e0 + un * PCR_THREADS;
            act[un] = 0;
            vp[un] = vq[un] = 0.0;
            if (e < K * h) {
              const int k = e / h, j = e - k * h;
              if (rf[j]) {
                act[un] = 1;
                vp[un] = V[(size_t)k * ld + rp[j]];
                vq[un] = V[(size_t)k * ld + rq[j]];
              }
            }
          }
#pragma unroll
          for (int un = 0; un < PCR_UN; ++un) {
            if (!act[un]) continue;
            const int e = e0 + un * PCR_THREADS;
            const int k = e / h, j = e - k * h;
            const double c = rc[j], s = rs[j];
            V[(size_t)k * ld + rp[j]] = c * vp[un] - s * vq[un];
            V[(size_t)k * ld + rq[j]] = s * vp[un] + c * vq[un];
          }
        }
        __syncthreads();
      }
      const int any = flag;
      __syncthreads();
      if (!any) { status = sweep; break; }
    }

    if (status < 0) {
      // not finite, or not converged: nothing but NaN
      if (Bo)
        for (size_t i = tid; i < (size_t)A * K * M; i += PCR_THREADS) Bo[i] = (T)nan;
      if (Vo)
        for (size_t i = tid; i < (size_t)K * A; i += PCR_THREADS) Vo[i] = (T)nan;
      for (int i = tid; i < A; i += PCR_THREADS) Eo[i] = nan;
      if (tid == 0) {
        a.n_fit[f] = -1;
        a.sweeps[f] = status == -2 ? 0 : -1;
      }
      __syncthreads();
      continue;
    }

    // 3. and 4. the ordering, the signs, n_fit and the coefficients; the running sum takes the place of S
    //    (K * M <= K * ld)
    pcr_finish_fold<T, PCR_THREADS>(S, V, ld, K, M, A, a.rank_tol, status, Y, Bo, Vo, Eo, a.n_fit + f, a.sweeps + f, lam,
                                    sgn, gs, ord, &nfit_s, S, tid);
    __syncthreads();
  }
}

// Workspace for full concurrency: min(F, PCR_MAXWG) slots.  Host arithmetic only (no device query).
size_t pcr_workspace_bytes(int64_t F, int K, int M) {
  return slot_workspace_bytes(F, pcr_slot_bytes(K, M), PCR_MAXWG);
}

template <typename T>
int pcr_fit_impl(const void *XTX, const void *XTY, int64_t F, int K, int M, int A, double rank_tol, void *B,
                 double *eig, void *V, int32_t *n_fit, int32_t *sweeps, void *ws, size_t ws_bytes, hipStream_t st) {
  const size_t per = pcr_slot_bytes(K, M);
  if (ws_bytes < per) return fail(CVM_EWORKSPACE, "cvm_pcr_fit: workspace too small for one fold%s");
  if (F == 0) return CVM_OK;
  PcrArgs a;
  memset(&a, 0, sizeof(a));
  a.XTX = XTX; a.XTY = XTY; a.B = B; a.V = V; a.eig = eig; a.n_fit = n_fit; a.sweeps = sweeps;
  a.ws = reinterpret_cast<double *>(ws);
  a.F = F;
  a.per = per / 8;
  a.rank_tol = rank_tol;
  a.K = K; a.M = M; a.A = A; a.ld = pcr_ld(K, M);
  a.G = slot_count(F, per, ws_bytes, PCR_MAXWG);
  hipLaunchKernelGGL(pcr_kernel<T>, dim3((unsigned)a.G), dim3(PCR_THREADS), 0, st, a);
  HIP_OK(hipGetLastError());
  return CVM_OK;
}
