// enet.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after pcr.hpp).
// Elastic net and lasso over a grid of penalties for every fold: for fold f, response m and penalty l, with
// G = XTX[f], h = XTY[f][:, m], rho = l1_ratio,
//   minimise over beta:  1/2 beta' G beta - h' beta + lambda_l (rho |beta|_1 + 1/2 (1 - rho) |beta|_2^2)
// by cyclic coordinate descent with covariance updates (g = h - G beta kept current by the row of G of every
// coefficient that moves).  F x M independent penalty PATHS, one wavefront (a workgroup of 64 threads) per path,
// dealt to the workspace slots by slot_first (fit_plan.hpp): the path walks its penalties from the largest down,
// each warm-started from the one before.  All arithmetic in float64, inputs widened on load, B rounded once on
// store.
//
// Per path and penalty:
//   * ACTIVE mode.  Up to 64 coordinates are active; lane i holds the index, coefficient, g and diagonal of
//     active coordinate i in registers, G_AA (64 x 64) lies in LDS.  A sweep visits the active coordinates in the
//     order they were admitted: three v_readlane pairs, the update, one LDS row read.  No LDS write, no global
//     access and no barrier in that loop.
//   * CERTIFICATE pass: g is formed afresh for all K coordinates from h and the rows of G of the nonzero
//     coefficients (ascending slot order, one fma per term), the KKT violation is evaluated for every coordinate
//     and the problem is converged when its largest value is <= tol max|h|.  Nothing else counts as converged.
//     The pass also hands the fresh g back to the active lanes (the incrementally updated one drifts) and
//     admits the inactive coordinates whose violation exceeds the threshold, in ascending index order.
//   * FALLBACK mode, once more than 64 coordinates would be active, for the rest of the path: beta and g for
//     all K coordinates in LDS (over the space G_AA had), sweeps over all coordinates in natural order with the
//     rows of G read from memory (the head of row j + 1 loaded while coordinate j is worked on), the same
//     certificate pass.
// A pass over coordinates (active set or all) and a certificate pass each count as one sweep; a problem whose
// count reaches max_sweeps without a passed certificate has info 1 and its last iterate in B.
// Order of every sum and of every admission depends on the path's inputs alone: no atomics, bit-reproducible,
// whatever the batch around the path or the workspace size.
#pragma once

constexpr int ENET_MAXK = 4096;
constexpr int ENET_MAXM = 64;
constexpr int ENET_MAXL = 256;
constexpr int ENET_CAP = 64;              // active coordinates at most: one per lane
constexpr int ENET_SMALLK = 2048;         // up to here the 34.75 KiB LDS layout (four waves per CU), above it 64 KiB
constexpr int ENET_LDS_SMALL = 4096 + 64 + 32 + ENET_SMALLK / 8;   // doubles: G_AA | fresh g | new indices | slot map
constexpr int ENET_LDS_LARGE = 2 * ENET_MAXK;                      // doubles: beta | g of the fallback at K = 4096
constexpr int ENET_MAXWG = 1024;          // paths in flight at most
constexpr int ENET_PRE = 8;               // 64-entry pieces of the next row of G the fallback sweep loads ahead

struct EnetArgs {
  const void *XTX, *XTY;                  // [F][K][K], [F][K][M]
  void *B;                                // [F][L][K][M]
  int32_t *info, *sweeps;                 // [F][L][M]
  double *ws;                             // G slots of `per` doubles: the diagonal of the path's XTX
  int64_t P;                              // paths F * M
  size_t per;
  int K, M, L, G, max_sweeps;
  double rho, tol;
  double lam[ENET_MAXL];                  // descending
  int32_t order[ENET_MAXL];               // lam[i] is the caller's lambdas[order[i]]
};

inline size_t enet_path_bytes(int K) { return align_up((size_t)K * 8, 256); }

__device__ inline double enet_lane(double v, int l) {          // l wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ inline double enet_wave_max(double v) {             // all 64 lanes active
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
// a wave's own LDS / workspace writes, visible to its other lanes' reads that follow
__device__ inline void enet_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ inline bool enet_finite(double v) { return fabs(v) < __builtin_inf(); }     // false for NaN
// the coordinate update: S(z, lr) / den, zero where the denominator is not > 0
__device__ inline double enet_update(double z, double lr, double den) {
  const double sz = z > lr ? z - lr : (z < -lr ? z + lr : 0.0);
  return den > 0.0 ? sz / den : 0.0;
}
// KKT violation of one coordinate from r = g - lambda (1 - rho) beta
__device__ inline double enet_violation(double r, double b, double lr) {
  return b != 0.0 ? fabs(r - (b > 0.0 ? lr : -lr)) : fmax(0.0, fabs(r) - lr);
}

template <typename T, int LD>
__global__ __launch_bounds__(64) void enet_kernel(const EnetArgs a) {
  __shared__ double lds[LD];
  double *GAA = lds;                                           // active mode
  double *gnew = lds + ENET_CAP * ENET_CAP;
  int *inew = (int *)(gnew + ENET_CAP);
  unsigned char *slotof = (unsigned char *)(gnew + ENET_CAP + ENET_CAP / 2);   // K bytes: slot + 1, or 0
  const int K = a.K, M = a.M, L = a.L, G = a.G;
  double *bl = lds, *gl = lds + K;                             // fallback mode
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const double rho = a.rho;
  const int b = blockIdx.x, t = slot_first(b, G);
  double *dg = a.ws + (size_t)b * a.per;
  const double nan = __builtin_nan("");

  for (int64_t s = t; s < a.P; s += G) {
    const int64_t f = s / M;
    const int m = (int)(s - f * M);
    const T *Gm = (const T *)a.XTX + (size_t)f * K * K;
    const T *H = (const T *)a.XTY + (size_t)f * K * M + m;
    // the diagonal into the slot, max|h|, and whether either holds a non-finite value
    double hmax = 0.0;
    bool bad0 = false;
    for (int k = lane; k < K; k += 64) {
      const double d = (double)Gm[(size_t)k * K + k], h = (double)H[(size_t)k * M];
      dg[k] = d;
      bad0 |= !enet_finite(d) || !enet_finite(h);
      hmax = fmax(hmax, fabs(h));
      slotof[k] = 0;
    }
    hmax = enet_wave_max(hmax);
    const bool dead = __any(bad0);
    const double thr = a.tol * hmax;
    enet_sync();
    int nA = 0, mode = 0;                                      // mode 1: fallback
    int idx = 0;
    double beta = 0.0, g = 0.0, dgl = 0.0;

    for (int li = 0; li < L; ++li) {
      const double lam = a.lam[li];
      const double lr = lam * rho, l2 = lam * (1.0 - rho);
      const int64_t out = f * L + a.order[li];
      int status = dead ? 2 : -1, sw = 0;

      while (status < 0) {
        // ---- certificate pass: g afresh, the violation of every coordinate
        ++sw;
        double vmax = 0.0;
        bool bad = false;
        int nnew = 0;
        for (int k0 = 0; k0 < K; k0 += 256) {
          double acc[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u + lane;
            acc[u] = k < K ? (double)H[(size_t)k * M] : 0.0;
          }
          if (mode == 0) {
            for (int j = 0; j < nA; ++j) {
              const double bj = enet_lane(beta, j);
              if (bj != 0.0) {
                const T *row = Gm + (size_t)__builtin_amdgcn_readlane(idx, j) * K;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  const int k = k0 + 64 * u + lane;
                  if (k < K) acc[u] = fma(-bj, (double)row[k], acc[u]);
                }
              }
            }
          } else {
            for (int j = 0; j < K; ++j) {
              const double bj = bl[j];
              if (bj != 0.0) {
                const T *row = Gm + (size_t)j * K;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                  const int k = k0 + 64 * u + lane;
                  if (k < K) acc[u] = fma(-bj, (double)row[k], acc[u]);
                }
              }
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u + lane;
            const bool in = k < K;
            double bk;
            int sl = 0;
            if (mode == 0) {
              sl = in ? slotof[k] : 0;
              bk = __shfl(beta, sl ? sl - 1 : 0);
              if (!sl) bk = 0.0;
            } else {
              bk = in ? bl[k] : 0.0;
            }
            const double r = acc[u] - l2 * bk;
            const double v = enet_violation(r, bk, lr);
            if (in) {
              bad |= !enet_finite(r);
              vmax = fmax(vmax, v);
            }
            if (mode == 0) {
              if (sl) gnew[sl - 1] = acc[u];
              // admit, in ascending index order
              const bool viol = in && !sl && v > thr;
              const unsigned long long mask = __ballot(viol);
              const int pos = nA + nnew + __popcll(mask & below);
              if (viol && pos < ENET_CAP) {
                gnew[pos] = acc[u];
                inew[pos] = k;
              }
              nnew += __popcll(mask);
            } else if (in) {
              gl[k] = acc[u];
            }
          }
        }
        vmax = enet_wave_max(vmax);
        bad = __any(bad);
        enet_sync();
        if (mode == 0 && lane < nA) g = gnew[lane];
        if (bad) { status = 2; break; }
        if (vmax <= thr) { status = 0; break; }
        if (sw >= a.max_sweeps) { status = 1; break; }

        if (mode == 0 && nA + nnew > ENET_CAP) {
          // ---- more than the lanes hold: beta for all coordinates into LDS, the fallback from here on
          enet_sync();
          for (int k = lane; k < K; k += 64) bl[k] = 0.0;
          enet_sync();
          if (lane < nA) bl[idx] = beta;
          enet_sync();
          mode = 1;
          continue;                                            // (the certificate pass forms g in LDS)
        }

        if (mode == 0) {
          // ---- admit the violators, complete G_AA, sweep the active set
          if (nnew) {
            const int nOld = nA;
            nA += nnew;
            if (lane >= nOld && lane < nA) {
              idx = inew[lane];
              g = gnew[lane];
              beta = 0.0;
              dgl = dg[idx];
              slotof[idx] = (unsigned char)(lane + 1);
            }
            for (int j = 0; j < nA; ++j) {
              const int ij = __builtin_amdgcn_readlane(idx, j);
              if (lane < nA && (j >= nOld || lane >= nOld)) GAA[j * ENET_CAP + lane] = (double)Gm[(size_t)ij * K + idx];
            }
            enet_sync();
          }
          bool nf;
          double vin;
          do {
            ++sw;
            for (int j = 0; j < nA; ++j) {
              const double bj = enet_lane(beta, j), gj = enet_lane(g, j), d = enet_lane(dgl, j);
              const double bn = enet_update(fma(d, bj, gj), lr, d + l2);
              const double delta = bn - bj;
              if (delta != 0.0) {
                if (lane < nA) g = fma(-delta, GAA[j * ENET_CAP + lane], g);
                if (lane == j) beta = bn;
              }
            }
            const double r = g - l2 * beta;
            const bool on = lane < nA;
            nf = __any(on && !enet_finite(r));
            vin = enet_wave_max(on ? enet_violation(r, beta, lr) : 0.0);
          } while (!nf && vin > 0.5 * thr && sw < a.max_sweeps);
          if (nf) status = 2;
          else if (sw >= a.max_sweeps) status = 1;
        } else {
          // ---- sweeps over all coordinates, rows of G from memory
          bool nf;
          double vin;
          do {
            ++sw;
            // the first 512 entries of row j + 1 are loaded while coordinate j is worked on, whether or not
            // that coordinate will move: the row's latency is then off the chain of dependent updates
            double pre[ENET_PRE];
#pragma unroll
            for (int u = 0; u < ENET_PRE; ++u) {
              const int k = lane + 64 * u;
              pre[u] = k < K ? (double)Gm[k] : 0.0;
            }
            for (int j0 = 0; j0 < K; j0 += 64) {
              const double dch = j0 + lane < K ? dg[j0 + lane] : 0.0;
              const int nj = K - j0 < 64 ? K - j0 : 64;
              for (int jj = 0; jj < nj; ++jj) {
                const int j = j0 + jj;
                const T *row = Gm + (size_t)j * K;
                double nxt[ENET_PRE];
#pragma unroll
                for (int u = 0; u < ENET_PRE; ++u) {
                  const int k = lane + 64 * u;
                  nxt[u] = (j + 1 < K && k < K) ? (double)row[K + k] : 0.0;
                }
                const double d = enet_lane(dch, jj);
                const double bj = bl[j], gj = gl[j];
                const double bn = enet_update(fma(d, bj, gj), lr, d + l2);
                const double delta = bn - bj;
                if (delta != 0.0) {
#pragma unroll
                  for (int u = 0; u < ENET_PRE; ++u) {
                    const int k = lane + 64 * u;
                    if (k < K) gl[k] = fma(-delta, pre[u], gl[k]);
                  }
                  for (int k = lane + 64 * ENET_PRE; k < K; k += 64) gl[k] = fma(-delta, (double)row[k], gl[k]);
                  if (lane == 0) bl[j] = bn;
                  enet_sync();
                }
#pragma unroll
                for (int u = 0; u < ENET_PRE; ++u) pre[u] = nxt[u];
              }
            }
            bool nfl = false;
            double v = 0.0;
            for (int k = lane; k < K; k += 64) {
              const double bk = bl[k], r = gl[k] - l2 * bk;
              nfl |= !enet_finite(r);
              v = fmax(v, enet_violation(r, bk, lr));
            }
            nf = __any(nfl);
            vin = enet_wave_max(v);
          } while (!nf && vin > 0.5 * thr && sw < a.max_sweeps);
          if (nf) status = 2;
          else if (sw >= a.max_sweeps) status = 1;
        }
      }

      // ---- a coefficient that is not finite is status 2, whatever ended the iteration
      if (status != 2) {
        bool nfl = false;
        if (mode == 0) {
          nfl = lane < nA && !enet_finite(beta);
        } else {
          for (int k = lane; k < K; k += 64) nfl |= !enet_finite(bl[k]);
        }
        if (__any(nfl)) status = 2;
      }
      // ---- B[f][l][:, m], written here and nowhere else
      T *Bo = (T *)a.B + (size_t)out * K * M + m;
      for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < K;
        double v;
        if (mode == 0) {
          const int sl = in ? slotof[k] : 0;
          v = __shfl(beta, sl ? sl - 1 : 0);
          if (!sl) v = 0.0;
        } else {
          v = in ? bl[k] : 0.0;
        }
        if (status == 2) v = nan;
        if (in) Bo[(size_t)k * M] = (T)v;
      }
      if (lane == 0) {
        a.info[out * M + m] = status;
        a.sweeps[out * M + m] = sw;
      }
      if (status == 2) {
        // what ended non-finite seeds nothing: the next penalty starts from zero
        enet_sync();
        for (int k = lane; k < K; k += 64) slotof[k] = 0;
        enet_sync();
        nA = 0; mode = 0; idx = 0;
        beta = 0.0; g = 0.0; dgl = 0.0;
      }
    }
    enet_sync();
  }
}

// Workspace for full concurrency: min(F M, ENET_MAXWG) slots.  Host arithmetic only (no device query).
size_t enet_workspace_bytes(int64_t F, int K, int M) {
  return slot_workspace_bytes(F * (int64_t)M, enet_path_bytes(K), ENET_MAXWG);
}

template <typename T>
int enet_fit_impl(const void *XTX, const void *XTY, int64_t F, int K, int M, const double *lambdas, int L, double rho,
                  double tol, int max_sweeps, void *B, int32_t *info, int32_t *sweeps, void *ws, size_t ws_bytes,
                  hipStream_t st) {
  const size_t per = enet_path_bytes(K);
  if (ws_bytes < per) return fail(CVM_EWORKSPACE, "cvm_enet_fit: workspace too small for one path%s");
  if (F == 0) return CVM_OK;
  EnetArgs a;
  memset(&a, 0, sizeof(a));
  a.XTX = XTX; a.XTY = XTY; a.B = B; a.info = info; a.sweeps = sweeps;
  a.ws = reinterpret_cast<double *>(ws);
  a.P = F * (int64_t)M;
  a.per = per / 8;
  a.K = K; a.M = M; a.L = L; a.max_sweeps = max_sweeps;
  a.rho = rho; a.tol = tol;
  a.G = slot_count(a.P, per, ws_bytes, ENET_MAXWG);
  // largest penalty first; equal penalties in the caller's order
  for (int l = 0; l < L; ++l) a.order[l] = l;
  std::stable_sort(a.order, a.order + L, [&](int32_t x, int32_t y) { return lambdas[x] > lambdas[y]; });
  for (int l = 0; l < L; ++l) a.lam[l] = lambdas[a.order[l]];
  if (K <= ENET_SMALLK)
    hipLaunchKernelGGL((enet_kernel<T, ENET_LDS_SMALL>), dim3((unsigned)a.G), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((enet_kernel<T, ENET_LDS_LARGE>), dim3((unsigned)a.G), dim3(64), 0, st, a);
  HIP_OK(hipGetLastError());
  return CVM_OK;
}
