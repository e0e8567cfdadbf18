// pcalda.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after omp.hpp, whose
// enet_lane / enet_sync / enet_finite (enet.hpp) it uses).
// PCA-LDA for every fold: linear discriminant analysis on the scores of the first 1, 2, .., A principal
// components, from the eigenpairs (cvm_pcr_fit / cvm_pcr_blocked_fit), the class sums XTY and the class weights.
// With h_c = XTY[f][:, c], n_c = class_w[f][c], n = sum_c n_c, V (K x A) and lambda the leading eigenpairs of XTX[f]:
//   P = V' H (A x C),  m~_c = p_c / n_c  (0 for an absent class)
//   S = diag(lambda) - sum_c p_c p_c' / n_c                  within-class scatter of the scores, classes in order
//   S = L L' column by column; the path ends before component j (0-based) when j >= n_comp or the pivot
//       d_j^2 = S_jj - sum_{i<j} L_ji^2 is not > pivot_tol lambda_j                        -> n_fit = j
//   Z = L^-1 M~ (A x C),  W = V L^-T (K x A)
//   coef[a] = coef[a-1] + w_a (n z_a)',  intercept[a] = intercept[a-1] - 1/2 (n z_a) o z_a,  intercept[-1] = log(n_c / n)
// The Cholesky factor of a leading block is the leading block of the factor: one A x A factorisation gives the
// models on 1 .. A components.  A <= PCL_CAP = 64: the factor lies in LDS with one row per lane (as OMP_CAP).
//
// Per chunk of folds, three launches (all arithmetic in float64, inputs widened on load, outputs rounded once on
// store):
//   1. pcalda_project_kernel, one workgroup per (fold, slice of PCL_KSLICE = 128 rows of K): the slice's share of
//      P into the workspace, rows in ascending order with one fma per term, and the slice's flag (a value of V in a
//      column < n_comp, or of XTY, that is not finite).  No atomics: slice s writes words of its own;
//   2. pcalda_factor_kernel, one workgroup per fold: adds the slices in ascending order, forms the lower triangle
//      of S, runs the Cholesky with the pivot rule on one wavefront (lane r owns row r; pitch 65 doubles, so the
//      column read across lanes is conflict-free), then Z by forward substitution (lane c owns class c) and
//      X = L^-1 (lane c owns column c; X' is kept in the upper triangle of the array of L), writes X and n Z into
//      the fold's record, n_fit, info and EVERY intercept of the fold (padding and NaN fill included);
//   3. pcalda_expand_kernel, one workgroup per (fold, tile of R = min(32, 512 / C) rows of V): W = V X' for the
//      tile through LDS (sum over i <= j ascending), then the running sum over a with one fma per element and
//      step, stored for every a: consecutive threads on consecutive (k, c) elements of coef[f][a], so every
//      a-slice is written along rows.  Padding (a >= n_fit repeats n_fit - 1) and the NaN fill of a flagged fold
//      are the same loop.
// Every sum runs in a fixed order, nothing but integer flags written by their own workgroup is shared, no
// workgroup waits for another: a fold's bits depend on its own V, eig, n_comp, XTY, class_w, A and pivot_tol
// alone, not on the batch around it, on the workspace size or on the chunking.
#pragma once

constexpr int PCL_MAXK = 4096;
constexpr int PCL_MAXC = 64;
constexpr int PCL_CAP = 64;               // components at most: one row of the factor per lane
constexpr int PCL_PITCH = PCL_CAP + 1;    // doubles per row of L, of P' and of the V tile: odd, column reads conflict-free
constexpr int PCL_THREADS = 256;
constexpr int PCL_KSLICE = 128;           // rows of K per project workgroup
constexpr int PCL_CHUNK = 32;             // rows staged in LDS at a time by the project kernel
constexpr int PCL_ROWS = 32;              // rows of V per expand tile at most
constexpr int PCL_TILE = 512;             // (k, c) elements per expand tile at most: two per thread
constexpr double PCL_PIVOT_TOL = 0x1p-26;

inline int pcl_slices(int K) { return (K + PCL_KSLICE - 1) / PCL_KSLICE; }
inline int pcl_tile_rows(int C) { const int r = PCL_TILE / C; return r > PCL_ROWS ? PCL_ROWS : r; }   // 8 .. 32

struct PclLayout {                        // byte offsets of a chunk of nf folds in the workspace
  size_t part, sflag, X, nZ, end;
};

// regions: the slices' shares of P [nf][NS][A][C], X = L^-1 [nf][A][A], n Z [nf][A][C] (float64); slice flags [nf][NS] (int32)
inline PclLayout pcl_layout(int64_t nf, int K, int C, int A) {
  PclLayout o;
  const size_t NS = (size_t)pcl_slices(K);
  size_t p = 0;
  o.part = p;  p += align_up((size_t)nf * NS * A * C * 8, 256);
  o.sflag = p; p += align_up((size_t)nf * NS * 4, 256);
  o.X = p;     p += align_up((size_t)nf * A * A * 8, 256);
  o.nZ = p;    p += align_up((size_t)nf * A * C * 8, 256);
  o.end = p;
  return o;
}

size_t pcalda_workspace_bytes(int64_t F, int K, int C, int A) {
  if (F < 1) F = 1;
  return pcl_layout(F, K, C, A).end;
}

struct PclProjectArgs {
  const void *V, *XTY;                    // [nf][K][A], [nf][K][C]
  const int32_t *n_comp;                  // [nf]
  double *part;                           // [nf][NS][A][C]
  int32_t *sflag;                         // [nf][NS]
  int K, C, A, NS;
};

template <typename T>
__global__ __launch_bounds__(PCL_THREADS) void pcalda_project_kernel(const PclProjectArgs a) {
  __shared__ double Vt[PCL_CHUNK][PCL_CAP];
  __shared__ double Ht[PCL_CHUNK][PCL_MAXC];
  const int K = a.K, C = a.C, A = a.A, tid = threadIdx.x;
  const size_t f = blockIdx.x / (unsigned)a.NS;
  const int s = (int)(blockIdx.x - f * (unsigned)a.NS);
  const int k0 = s * PCL_KSLICE, k1 = k0 + PCL_KSLICE < K ? k0 + PCL_KSLICE : K;
  const T *V = (const T *)a.V + f * K * A;
  const T *H = (const T *)a.XTY + f * K * C;
  int nc = a.n_comp[f];
  nc = nc > A ? A : nc;                   // (negative: the factor kernel flags the fold; no column is checked here)
  const int AC = A * C, nq = (AC + PCL_THREADS - 1) / PCL_THREADS;      // outputs per thread: 1 .. 16
  double acc[16];
  int ia[16], ic[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int o = tid + q * PCL_THREADS;
    acc[q] = 0.0;
    ia[q] = o < AC ? o / C : 0;
    ic[q] = o < AC ? o - (o / C) * C : 0;
  }
  int bad = 0;
  for (int kb = k0; kb < k1; kb += PCL_CHUNK) {
    const int rows = k1 - kb < PCL_CHUNK ? k1 - kb : PCL_CHUNK;
    __syncthreads();
    for (int e = tid; e < rows * A; e += PCL_THREADS) {
      const int r = e / A, i = e - r * A;
      const double v = (double)V[(size_t)kb * A + e];
      if (i < nc && !enet_finite(v)) bad = 1;
      Vt[r][i] = v;
    }
    for (int e = tid; e < rows * C; e += PCL_THREADS) {
      const int r = e / C, c = e - r * C;
      const double h = (double)H[(size_t)kb * C + e];
      if (!enet_finite(h)) bad = 1;
      Ht[r][c] = h;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q < nq) acc[q] = fma(Vt[r][ia[q]], Ht[r][ic[q]], acc[q]);
    }
  }
  double *out = a.part + (f * a.NS + s) * (size_t)AC;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int o = tid + q * PCL_THREADS;
    if (o < AC) out[o] = acc[q];
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) a.sflag[f * a.NS + s] = bad ? 1 : 0;
}

struct PclFactorArgs {
  const double *part, *eig, *class_w;     // [nf][NS][A][C], [nf][A], [nf][C]
  const int32_t *n_comp, *sflag;
  double *X, *nZ;                         // [nf][A][A], [nf][A][C]
  void *intercept;                        // [nf][A][C]
  int32_t *n_fit, *info;                  // [nf]
  int C, A, NS;
  double pivot_tol;
};

// dynamic LDS: L (A rows of PCL_PITCH) and P' (C rows of PCL_PITCH), 66,560 bytes at A = C = 64
inline size_t pcl_factor_lds(int C, int A) { return (size_t)(A + C) * PCL_PITCH * 8; }

template <typename T>
__global__ __launch_bounds__(PCL_THREADS) void pcalda_factor_kernel(const PclFactorArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pcl_smem[];
  __shared__ double lam[PCL_CAP], ncs[PCL_MAXC], rn[PCL_MAXC], dinv[PCL_CAP];
  __shared__ double n_sh;
  __shared__ int bad_sh, nfit_sh, info_sh;
  const int C = a.C, A = a.A, NS = a.NS, tid = threadIdx.x;
  const size_t f = blockIdx.x;
  double *Ls = reinterpret_cast<double *>(pcl_smem);          // [A][PITCH]: S, then L below and X' above the diagonal
  double *Pt = Ls + (size_t)A * PCL_PITCH;                     // [C][PITCH]: P', then M~', then Z'
  const int ncomp_in = a.n_comp[f];
  const int nc = ncomp_in > A ? A : ncomp_in;
  T *icpt = (T *)a.intercept + f * (size_t)A * C;
  const double nan = __builtin_nan("");

  if (tid == 0) bad_sh = ncomp_in < 0 ? 1 : 0;
  __syncthreads();
  // the flags of the slices, the eigenvalues that exist, the class weights
  {
    int bad = 0;
    for (int s = tid; s < NS; s += PCL_THREADS) bad |= a.sflag[f * NS + s];
    if (tid < A) {
      const double l = a.eig[f * A + tid];
      if (tid < nc && !enet_finite(l)) bad = 1;
      lam[tid] = l;
    }
    if (tid < C) {
      const double w = a.class_w[f * C + tid];
      const bool ok = enet_finite(w) && w >= 0.0;
      if (!ok) bad = 1;
      ncs[tid] = ok ? w : 0.0;
      rn[tid] = ok && w > 0.0 ? 1.0 / w : 0.0;
    }
    if (bad) bad_sh = 1;                  // (every writer stores the same value)
  }
  __syncthreads();
  if (tid == 0) {
    double n = 0.0;
    for (int c = 0; c < C; ++c) n += ncs[c];
    n_sh = n;
    if (!(n > 0.0) || !enet_finite(n)) bad_sh = 1;
  }
  // P = the slices' shares added in ascending order, kept as P'[c][a]
  const double *part = a.part + f * NS * (size_t)A * C;
  for (int e = tid; e < A * C; e += PCL_THREADS) {
    const int i = e / C, c = e - i * C;
    double p = part[e];
    for (int s = 1; s < NS; ++s) p += part[(size_t)s * A * C + e];
    Pt[c * PCL_PITCH + i] = p;
  }
  __syncthreads();
  if (bad_sh) {
    // the flagged fold: every intercept NaN, the expand kernel fills coef
    for (int e = tid; e < A * C; e += PCL_THREADS) icpt[e] = (T)nan;
    if (tid == 0) { a.n_fit[f] = -1; a.info[f] = -1; }
    return;
  }
  // the lower triangle of S = diag(lambda) - sum_c (p_c[i] / n_c) p_c[j], classes in ascending order
  for (int e = tid; e < A * A; e += PCL_THREADS) {
    const int i = e / A, j = e - i * A;
    if (j > i) continue;
    double sum = i == j ? lam[i] : 0.0;
    for (int c = 0; c < C; ++c) sum = fma(-(Pt[c * PCL_PITCH + i] * rn[c]), Pt[c * PCL_PITCH + j], sum);
    Ls[i * PCL_PITCH + j] = sum;
  }
  __syncthreads();
  // M~' in place of P' (every element by the thread that reads it)
  for (int e = tid; e < A * C; e += PCL_THREADS) {
    const int c = e / A, i = e - c * A;
    Pt[c * PCL_PITCH + i] = ncs[c] > 0.0 ? Pt[c * PCL_PITCH + i] / ncs[c] : 0.0;
  }
  // the Cholesky factorisation, left-looking, on the first wavefront: lane r owns row r
  if (tid < 64) {
    const int r = tid;
    int nf = 0, info = 0;
    for (int j = 0; j < A; ++j) {
      if (j >= nc) { info = 1; break; }
      double t = 0.0;
      if (r >= j && r < A) {
        t = Ls[r * PCL_PITCH + j];
        for (int i = 0; i < j; ++i) t = fma(-Ls[r * PCL_PITCH + i], Ls[j * PCL_PITCH + i], t);
      }
      const double d2 = enet_lane(t, j);
      if (!enet_finite(d2)) { info = -1; break; }
      if (!(d2 > a.pivot_tol * lam[j]) || !(d2 > 0.0)) { info = 2; break; }
      const double d = sqrt(d2);
      if (r == j) Ls[r * PCL_PITCH + j] = d;
      if (r > j && r < A) Ls[r * PCL_PITCH + j] = t / d;
      nf = j + 1;
      enet_sync();
    }
    if (r == 0) { nfit_sh = nf; info_sh = info; }
  }
  __syncthreads();
  const int nf = nfit_sh, info = info_sh;
  if (info < 0) {                         // a pivot that is not finite (overflow): flagged like bad input
    for (int e = tid; e < A * C; e += PCL_THREADS) icpt[e] = (T)nan;
    if (tid == 0) { a.n_fit[f] = -1; a.info[f] = -1; }
    return;
  }
  // first wavefront: Z' = (L^-1 M~)' in place, lane c owns class c; second wavefront: X = L^-1, lane c owns column c,
  // X[r][c] kept at Ls[c][r] (above the diagonal), X[c][c] in dinv
  if (tid < 64) {
    const int c = tid;
    if (c < C) {
      for (int j = 0; j < nf; ++j) {
        double z = Pt[c * PCL_PITCH + j];
        for (int i = 0; i < j; ++i) z = fma(-Ls[j * PCL_PITCH + i], Pt[c * PCL_PITCH + i], z);
        Pt[c * PCL_PITCH + j] = z / Ls[j * PCL_PITCH + j];
      }
    }
  } else if (tid < 128) {
    const int c = tid - 64;
    if (c < nf) {
      const double xcc = 1.0 / Ls[c * PCL_PITCH + c];
      dinv[c] = xcc;
      for (int r = c + 1; r < nf; ++r) {
        double sum = -Ls[r * PCL_PITCH + c] * xcc;
        for (int i = c + 1; i < r; ++i) sum = fma(-Ls[r * PCL_PITCH + i], Ls[c * PCL_PITCH + i], sum);
        Ls[c * PCL_PITCH + r] = sum / Ls[r * PCL_PITCH + r];
      }
    }
  }
  __syncthreads();
  // the fold's record: X (rows j < n_fit, columns i <= j; zero elsewhere) and n Z
  const double n = n_sh;
  double *Xg = a.X + f * (size_t)A * A;
  for (int e = tid; e < A * A; e += PCL_THREADS) {
    const int j = e / A, i = e - j * A;
    Xg[e] = (j < nf && i <= j) ? (i == j ? dinv[j] : Ls[i * PCL_PITCH + j]) : 0.0;
  }
  double *nZg = a.nZ + f * (size_t)A * C;
  for (int e = tid; e < A * C; e += PCL_THREADS) {
    const int j = e / C, c = e - j * C;
    nZg[e] = j < nf ? n * Pt[c * PCL_PITCH + j] : 0.0;
  }
  // every intercept of the fold: the running sum, then the padding
  if (tid < C) {
    const int c = tid;
    const bool present = ncs[c] > 0.0;
    double v = present ? log(ncs[c] / n) : -HUGE_VAL;
    for (int j = 0; j < A; ++j) {
      if (j < nf && present) {
        const double z = Pt[c * PCL_PITCH + j];
        v = fma(-0.5 * (n * z), z, v);
      }
      icpt[j * C + c] = (T)v;
    }
  }
  if (tid == 0) { a.n_fit[f] = nf; a.info[f] = info; }
}

struct PclExpandArgs {
  const void *V;                          // [nf][K][A]
  const double *X, *nZ;                   // [nf][A][A], [nf][A][C]
  const int32_t *n_fit, *info;            // [nf]
  void *coef;                             // [nf][A][K][C]
  int K, C, A, R, ntile;                  // R rows a tile, ntile tiles a fold
};

template <typename T>
__global__ __launch_bounds__(PCL_THREADS) void pcalda_expand_kernel(const PclExpandArgs a) {
  __shared__ double Xs[PCL_CAP * PCL_PITCH];                   // X [j][PITCH]; then n Z [a][C]
  __shared__ double Vt[PCL_ROWS * PCL_PITCH];                  // the tile of V, then of W, [r][PITCH]
  const int K = a.K, C = a.C, A = a.A, tid = threadIdx.x;
  const size_t f = blockIdx.x / (unsigned)a.ntile;
  const int tile = (int)(blockIdx.x - f * (unsigned)a.ntile);
  const int k0 = tile * a.R;
  const int rows = K - k0 < a.R ? K - k0 : a.R;
  const int nel = rows * C;                                    // <= PCL_TILE
  T *coef = (T *)a.coef + f * (size_t)A * K * C + (size_t)k0 * C;
  const size_t slice = (size_t)K * C;
  const int e0 = tid, e1 = tid + PCL_THREADS;
  if (a.info[f] < 0) {
    const double nan = __builtin_nan("");
    for (int j = 0; j < A; ++j) {
      if (e0 < nel) coef[j * slice + e0] = (T)nan;
      if (e1 < nel) coef[j * slice + e1] = (T)nan;
    }
    return;
  }
  const int nf = a.n_fit[f];
  const double *Xg = a.X + f * (size_t)A * A;
  const T *V = (const T *)a.V + f * (size_t)K * A + (size_t)k0 * A;
  for (int e = tid; e < nf * A; e += PCL_THREADS) {
    const int j = e / A, i = e - j * A;
    Xs[j * PCL_PITCH + i] = Xg[e];
  }
  for (int e = tid; e < rows * A; e += PCL_THREADS) {
    const int r = e / A, i = e - r * A;
    Vt[r * PCL_PITCH + i] = (double)V[e];
  }
  __syncthreads();
  // W[r][j] = sum_{i <= j} V[r][i] X[j][i]: thread (r, g) takes j = g, g + 8, ..
  const int r = tid & (PCL_ROWS - 1), g = tid >> 5;
  double w[PCL_CAP / 8];
#pragma unroll
  for (int q = 0; q < PCL_CAP / 8; ++q) {
    const int j = g + 8 * q;
    double sum = 0.0;
    if (r < rows && j < nf)
      for (int i = 0; i <= j; ++i) sum = fma(Vt[r * PCL_PITCH + i], Xs[j * PCL_PITCH + i], sum);
    w[q] = sum;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PCL_CAP / 8; ++q) {
    const int j = g + 8 * q;
    if (r < rows && j < nf) Vt[r * PCL_PITCH + j] = w[q];
  }
  const double *nZg = a.nZ + f * (size_t)A * C;
  for (int e = tid; e < nf * C; e += PCL_THREADS) Xs[e] = nZg[e];
  __syncthreads();
  // the running sum over a, stored for every a: the models that exist, then the padding
  const int r0 = e0 < nel ? e0 / C : 0, c0 = e0 < nel ? e0 - (e0 / C) * C : 0;
  const int r1 = e1 < nel ? e1 / C : 0, c1 = e1 < nel ? e1 - (e1 / C) * C : 0;
  double acc0 = 0.0, acc1 = 0.0;
  for (int j = 0; j < A; ++j) {
    if (j < nf) {
      acc0 = fma(Vt[r0 * PCL_PITCH + j], Xs[j * C + c0], acc0);
      acc1 = fma(Vt[r1 * PCL_PITCH + j], Xs[j * C + c1], acc1);
    }
    if (e0 < nel) coef[j * slice + e0] = (T)acc0;
    if (e1 < nel) coef[j * slice + e1] = (T)acc1;
  }
}

template <typename T>
int pcalda_fit_impl(const void *V, const double *eig, const int32_t *n_comp, const void *XTY, const double *class_w,
                    int64_t F, int K, int C, int A, double pivot_tol, void *coef, void *intercept, int32_t *n_fit,
                    int32_t *info, void *ws, size_t ws_bytes, hipStream_t st) {
  if (ws_bytes < pcl_layout(1, K, C, A).end)
    return fail(CVM_EWORKSPACE, "cvm_pcalda_fit: workspace too small for one fold's record%s");
  const int NS = pcl_slices(K), R = pcl_tile_rows(C), ntile = (K + R - 1) / R;
  // folds per chunk: as many as the workspace holds, never more workgroups than a grid holds
  int64_t top = F;
  const int64_t per = NS > ntile ? NS : ntile;
  if (top > (int64_t)(0x40000000 / per)) top = 0x40000000 / per;
  const int64_t nf = folds_per_chunk(top, ws_bytes, [&](int64_t n) { return pcl_layout(n, K, C, A).end; });
  const size_t lds = pcl_factor_lds(C, A);
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(pcalda_factor_kernel<T>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const PclLayout o = pcl_layout(nf, K, C, A);
  char *w = reinterpret_cast<char *>(ws);
  const size_t esz = sizeof(T);
  for (int64_t f0 = 0; f0 < F; f0 += nf) {
    const int64_t n = F - f0 < nf ? F - f0 : nf;
    const char *cV = (const char *)V + (size_t)f0 * K * A * esz;
    PclProjectArgs pa;
    pa.V = cV; pa.XTY = (const char *)XTY + (size_t)f0 * K * C * esz; pa.n_comp = n_comp + f0;
    pa.part = (double *)(w + o.part); pa.sflag = (int32_t *)(w + o.sflag);
    pa.K = K; pa.C = C; pa.A = A; pa.NS = NS;
    hipLaunchKernelGGL(pcalda_project_kernel<T>, dim3((unsigned)(n * NS)), dim3(PCL_THREADS), 0, st, pa);
    HIP_OK(hipGetLastError());
    PclFactorArgs fa;
    fa.part = pa.part; fa.eig = eig + (size_t)f0 * A; fa.class_w = class_w + (size_t)f0 * C;
    fa.n_comp = pa.n_comp; fa.sflag = pa.sflag;
    fa.X = (double *)(w + o.X); fa.nZ = (double *)(w + o.nZ);
    fa.intercept = (char *)intercept + (size_t)f0 * A * C * esz;
    fa.n_fit = n_fit + f0; fa.info = info + f0;
    fa.C = C; fa.A = A; fa.NS = NS; fa.pivot_tol = pivot_tol;
    hipLaunchKernelGGL(pcalda_factor_kernel<T>, dim3((unsigned)n), dim3(PCL_THREADS), lds, st, fa);
    HIP_OK(hipGetLastError());
    PclExpandArgs ea;
    ea.V = cV; ea.X = fa.X; ea.nZ = fa.nZ; ea.n_fit = fa.n_fit; ea.info = fa.info;
    ea.coef = (char *)coef + (size_t)f0 * A * K * C * esz;
    ea.K = K; ea.C = C; ea.A = A; ea.R = R; ea.ntile = ntile;
    hipLaunchKernelGGL(pcalda_expand_kernel<T>, dim3((unsigned)(n * ntile)), dim3(PCL_THREADS), 0, st, ea);
    HIP_OK(hipGetLastError());
  }
  return CVM_OK;
}
