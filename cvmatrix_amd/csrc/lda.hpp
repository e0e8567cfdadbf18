// lda.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after ridge.hpp).
// Linear discriminant analysis with shrinkage for every fold, from the training matrices alone.  With
// h_c = XTY[f][:, c] (the class sums of the centred X), n_c = class_w[f][c], n = sum_c n_c, m_c = h_c / n_c:
//   S_w      = XTX[f] - sum_c h_c h_c^T / n_c                   within-class scatter
//   Sigma_g  = (1 - g) S_w / n + g (tr S_w / (n K)) I            shrunk pooled covariance
//   coef_c   = Sigma_g^-1 m_c,   intercept_c = -1/2 m_c^T coef_c + log(n_c / n)
// Scaled to trace K, S' = (K / tr S_w) S_w, the covariance is (tr S_w / (n K)) (1 - g) (S' + lambda I) with
// lambda = g / (1 - g): one penalty grid for all folds, and the solve is the ridge solve of ridge.hpp.
//
// Per chunk of folds (all arithmetic in float64, inputs widened on load, outputs rounded once on store):
//   1a. lda_moments_kernel, one workgroup per fold: n, m_c (the right-hand sides), tr S_w from its diagonal,
//       the fold's flag (a value of XTY or class_w that is not finite, a negative class_w, n or tr S_w not > 0);
//   1b. lda_scatter_kernel, one workgroup per 32 x 32 tile of the upper triangle: S' into the workspace.  The
//       trace must be known before the first scaled entry is written, hence the launch in front.  A tile off
//       the diagonal is computed once and stored twice (the mirror through LDS, so both stores run along
//       rows); a diagonal tile takes entry (i, j) from (min, max): S' is symmetric to the bit whatever XTX is.
//       Both triangles of XTX are read for the finite check (integer atomicOr into the fold's flag);
//   2.  ridge_fit_impl<double> on the workspace matrices for the penalties with g < 1;
//   3.  lda_finish_kernel, one workgroup per (fold, g): scales the solution, forms the intercepts, merges the
//       fold's flag and the factorisation's info, writes NaN where either is set.
// Every sum runs in a fixed order and nothing but the flag is shared between workgroups: a fold's bits depend
// on its own XTX, XTY, class_w and the grid alone, not on the batch around it or on the workspace size.
#pragma once

constexpr int LDA_THREADS = 256;
constexpr int LDA_TILE = 32;
constexpr int LDA_MAXC = RIDGE_MAXM;
constexpr int LDA_HEAD = 4;             // float64 per fold: K / tr S_w, n K / tr S_w, n, tr S_w

struct LdaLayout {                      // byte offsets of a chunk of nf folds in the workspace
  size_t S, Mr, X, head, flag, rinfo, ridge;
};

// regions: S' [nf][K][K], m [nf][K][C], x [nf][L][K][C], head [nf][4] (float64); flag [nf], ridge info [nf][L] (int32)
inline LdaLayout lda_layout(int64_t nf, int K, int C, int L) {
  LdaLayout o;
  size_t p = 0;
  o.S = p;     p += align_up((size_t)nf * K * K * 8, 256);
  o.Mr = p;    p += align_up((size_t)nf * K * C * 8, 256);
  o.X = p;     p += align_up((size_t)nf * L * K * C * 8, 256);
  o.head = p;  p += align_up((size_t)nf * LDA_HEAD * 8, 256);
  o.flag = p;  p += align_up((size_t)nf * 4, 256);
  o.rinfo = p; p += align_up((size_t)nf * L * 4, 256);
  o.ridge = p;
  return o;
}

// every fold and every factorisation in flight at once
size_t lda_workspace_bytes(int64_t F, int K, int C, int L) {
  if (F < 1) F = 1;
  return lda_layout(F, K, C, L).ridge + ridge_workspace_bytes(F, K, C, L);
}

struct LdaMomentsArgs {
  const void *XTX, *XTY;                // [nf][K][K], [nf][K][C]
  const double *class_w;                // [nf][C]
  double *Mr, *head;
  int32_t *flag;
  int K, C;
};

template <typename T>
__global__ __launch_bounds__(LDA_THREADS) void lda_moments_kernel(const LdaMomentsArgs a) {
  __shared__ double ncs[LDA_MAXC];      // n_c, 0 where the class is absent or its weight is no weight
  __shared__ double red[LDA_THREADS];
  __shared__ double n_sh;
  __shared__ int bad_sh;
  const int K = a.K, C = a.C, tid = threadIdx.x;
  const size_t f = blockIdx.x;
  const T *X = (const T *)a.XTX + f * K * K;
  const T *Y = (const T *)a.XTY + f * K * C;
  double *Mr = a.Mr + f * K * C;
  if (tid == 0) bad_sh = 0;
  __syncthreads();
  if (tid < C) {
    const double w = a.class_w[f * C + tid];
    const bool ok = isfinite(w) && w >= 0.0;
    if (!ok) bad_sh = 1;                // (every writer stores the same value)
    ncs[tid] = ok ? w : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double n = 0.0;
    for (int c = 0; c < C; ++c) n += ncs[c];
    n_sh = n;
  }
  // the diagonal of S_w, row k by thread k % 256, with the products the scatter kernel forms for (k, k)
  double part = 0.0;
  int bad = 0;
  for (int k = tid; k < K; k += LDA_THREADS) {
    const double xkk = (double)X[(size_t)k * K + k];
    double s = 0.0;
    for (int c = 0; c < C; ++c) {
      const double h = (double)Y[(size_t)k * C + c];
      if (!isfinite(h)) bad = 1;
      const double g = ncs[c] > 0.0 ? h / ncs[c] : 0.0;
      Mr[(size_t)k * C + c] = g;
      s = fma(g, h, s);
    }
    part += xkk - s;
  }
  red[tid] = part;
  if (bad) bad_sh = 1;
  __syncthreads();
  for (int s = LDA_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const double tr = red[0], n = n_sh;
    const bool ok = !bad_sh && tr > 0.0 && isfinite(tr) && n > 0.0 && isfinite(n);
    const double scale = ok ? (double)K / tr : 0.0;
    double *hd = a.head + f * LDA_HEAD;
    hd[0] = scale;
    hd[1] = n * scale;
    hd[2] = n;
    hd[3] = tr;
    a.flag[f] = ok ? 0 : 1;
  }
}

struct LdaScatterArgs {
  const void *XTX, *XTY;
  const double *Mr, *head;
  double *S;
  int32_t *flag;
  int K, C, T, ntile;                   // T tiles a side, ntile = T (T + 1) / 2
};

template <typename T>
__global__ __launch_bounds__(LDA_THREADS) void lda_scatter_kernel(const LdaScatterArgs a) {
  __shared__ double gi[LDA_TILE][LDA_MAXC + 1];     // m_c of the tile's rows
  __shared__ double hj[LDA_TILE][LDA_MAXC + 1];     // h_c of the tile's columns
  __shared__ double tile[LDA_TILE][LDA_TILE + 1];
  const int K = a.K, C = a.C, NT = a.T, tid = threadIdx.x;
  const size_t f = blockIdx.x / (unsigned)a.ntile;
  const int t = (int)(blockIdx.x - f * (unsigned)a.ntile);
  // tile t of the upper triangle, rows first: row bi starts at bi NT - bi (bi - 1) / 2
  int bi = (int)(((2.0 * NT + 1.0) - sqrt((2.0 * NT + 1.0) * (2.0 * NT + 1.0) - 8.0 * t)) * 0.5);
  bi = bi < 0 ? 0 : (bi > NT - 1 ? NT - 1 : bi);
  while (bi > 0 && bi * NT - bi * (bi - 1) / 2 > t) --bi;
  while (bi + 1 < NT && (bi + 1) * NT - (bi + 1) * bi / 2 <= t) ++bi;
  const int bj = bi + (t - (bi * NT - bi * (bi - 1) / 2));
  const int i0 = bi * LDA_TILE, j0 = bj * LDA_TILE;
  const bool diag = bi == bj;
  const T *X = (const T *)a.XTX + f * K * K;
  const T *Y = (const T *)a.XTY + f * K * C;
  const double *Mr = a.Mr + f * K * C;
  double *S = a.S + f * K * K;
  const double scale = a.head[f * LDA_HEAD];

  // 32 rows of m and of h are 32 C consecutive elements each
  for (int e = tid; e < LDA_TILE * C; e += LDA_THREADS) {
    const int r = e / C, c = e - r * C;
    gi[r][c] = i0 + r < K ? Mr[(size_t)i0 * C + e] : 0.0;
    hj[r][c] = j0 + r < K ? (double)Y[(size_t)j0 * C + e] : 0.0;
  }
  const int tx = tid & 31, ty = tid >> 5;
  double u[4];
  int bad = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    const bool in = i0 + r < K && j0 + tx < K;
    u[q] = in ? (double)X[(size_t)(i0 + r) * K + j0 + tx] : 0.0;
    if (!isfinite(u[q])) bad = 1;
    // the mirrored entry feeds the check only
    if (!diag && j0 + r < K && i0 + tx < K && !isfinite((double)X[(size_t)(j0 + r) * K + i0 + tx])) bad = 1;
    if (diag) tile[r][tx] = u[q];
  }
  __syncthreads();
  if (bad) atomicOr(&a.flag[f], 1);
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    // row = the smaller index: entry (i, j) and entry (j, i) of a diagonal tile are one computation
    const int lo = diag && tx < r ? tx : r, hi = diag && tx < r ? r : tx;
    const double x = diag ? tile[lo][hi] : u[q];
    double s = 0.0;
    for (int c = 0; c < C; ++c) s = fma(gi[lo][c], hj[hi][c], s);
    v[q] = scale * (x - s);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    if (i0 + r < K && j0 + tx < K) S[(size_t)(i0 + r) * K + j0 + tx] = v[q];
    if (!diag) tile[r][tx] = v[q];
  }
  if (diag) return;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    if (j0 + r < K && i0 + tx < K) S[(size_t)(j0 + r) * K + i0 + tx] = tile[tx][r];
  }
}

struct LdaFinishArgs {
  const double *Mr, *X, *head, *class_w;
  const int32_t *flag, *rinfo;
  void *coef, *intercept;               // [nf][L][K][C], [nf][L][C]
  int32_t *info;                        // [nf][L]
  int K, C, L, Lr;
  double omg[RIDGE_MAXL];               // 1 - g
  short ridx[RIDGE_MAXL];               // the penalty's place among those with g < 1, -1 for g = 1
};

template <typename T>
__global__ __launch_bounds__(LDA_THREADS) void lda_finish_kernel(const LdaFinishArgs a) {
  __shared__ double part[LDA_THREADS];
  const int K = a.K, C = a.C, L = a.L, tid = threadIdx.x;
  const size_t f = blockIdx.x / (unsigned)L;
  const int l = (int)(blockIdx.x - f * (unsigned)L);
  const int ri = a.ridx[l];
  const int info = a.flag[f] ? -1 : (ri >= 0 ? a.rinfo[f * a.Lr + ri] : 0);
  T *coef = (T *)a.coef + (f * L + l) * (size_t)K * C;
  T *icpt = (T *)a.intercept + (f * L + l) * (size_t)C;
  if (tid == 0) a.info[f * L + l] = info;
  if (info != 0) {
    const double nan = __builtin_nan("");
    for (size_t e = tid; e < (size_t)K * C; e += LDA_THREADS) coef[e] = (T)nan;
    if (tid < C) icpt[tid] = (T)nan;
    return;
  }
  const double *hd = a.head + f * LDA_HEAD;
  const double n = hd[2];
  const double mul = ri >= 0 ? hd[1] / a.omg[l] : hd[1];
  const double *m = a.Mr + f * K * C;
  const double *x = ri >= 0 ? a.X + (f * a.Lr + ri) * (size_t)K * C : m;
  // thread (rr, c) walks rows rr, rr + R, ...: consecutive threads on consecutive elements
  const int R = LDA_THREADS / C, rr = tid / C, c = tid - rr * C;
  double dot = 0.0;
  if (rr < R) {
    const double nc = a.class_w[f * C + c];
    for (int k = rr; k < K; k += R) {
      const size_t e = (size_t)k * C + c;
      const double b = nc > 0.0 ? mul * x[e] : 0.0;
      coef[e] = (T)b;
      dot = fma(m[e], b, dot);
    }
  }
  part[tid] = dot;
  __syncthreads();
  if (tid < C) {
    const double nc = a.class_w[f * C + tid];
    double s = 0.0;
    for (int q = 0; q < R; ++q) s += part[q * C + tid];
    icpt[tid] = (T)(nc > 0.0 ? -0.5 * s + log(nc / n) : -HUGE_VAL);
  }
}

template <typename T>
int lda_fit_impl(const void *XTX, const void *XTY, const double *class_w, int64_t F, int K, int C,
                 const double *shrinkage, int L, void *coef, void *intercept, int32_t *info, void *ws,
                 size_t ws_bytes, hipStream_t st) {
  const size_t slot = ridge_problem_bytes(K, C);
  if (ws_bytes < lda_layout(1, K, C, L).ridge + slot)
    return fail(CVM_EWORKSPACE, "cvm_lda_fit: workspace too small for one fold%s");
  if (F == 0) return CVM_OK;
  LdaFinishArgs fa;
  memset(&fa, 0, sizeof(fa));
  double lambdas[RIDGE_MAXL];
  int Lr = 0;
  for (int l = 0; l < L; ++l) {
    fa.omg[l] = 1.0 - shrinkage[l];
    fa.ridx[l] = -1;
    if (shrinkage[l] < 1.0) {
      fa.ridx[l] = (short)Lr;
      lambdas[Lr++] = shrinkage[l] / fa.omg[l];
    }
  }
  const int NT = (K + LDA_TILE - 1) / LDA_TILE, ntile = NT * (NT + 1) / 2;
  // folds per chunk: as many as run with every factorisation in flight, at least one; never more tiles or
  // (fold, g) pairs than a grid holds
  auto need = [&](int64_t n) { return lda_layout(n, K, C, L).ridge + ridge_workspace_bytes(n, K, C, L); };
  int64_t top = F;
  if (top > (int64_t)(0x40000000 / ntile)) top = 0x40000000 / ntile;
  if (top > (int64_t)(0x40000000 / L)) top = 0x40000000 / L;
  // (need(1) may exceed ws_bytes: one fold then runs with fewer ridge slots)
  const int64_t nf = folds_per_chunk(top, ws_bytes, need);
  const LdaLayout o = lda_layout(nf, K, C, L);
  char *w = reinterpret_cast<char *>(ws);
  const size_t esz = sizeof(T);
  for (int64_t f0 = 0; f0 < F; f0 += nf) {
    const int64_t n = F - f0 < nf ? F - f0 : nf;
    const char *cX = (const char *)XTX + (size_t)f0 * K * K * esz;
    const char *cY = (const char *)XTY + (size_t)f0 * K * C * esz;
    const double *cw = class_w + (size_t)f0 * C;
    LdaMomentsArgs ma;
    ma.XTX = cX; ma.XTY = cY; ma.class_w = cw;
    ma.Mr = (double *)(w + o.Mr); ma.head = (double *)(w + o.head); ma.flag = (int32_t *)(w + o.flag);
    ma.K = K; ma.C = C;
    hipLaunchKernelGGL(lda_moments_kernel<T>, dim3((unsigned)n), dim3(LDA_THREADS), 0, st, ma);
    HIP_OK(hipGetLastError());
    LdaScatterArgs sa;
    sa.XTX = cX; sa.XTY = cY; sa.Mr = ma.Mr; sa.head = ma.head; sa.S = (double *)(w + o.S); sa.flag = ma.flag;
    sa.K = K; sa.C = C; sa.T = NT; sa.ntile = ntile;
    hipLaunchKernelGGL(lda_scatter_kernel<T>, dim3((unsigned)(n * ntile)), dim3(LDA_THREADS), 0, st, sa);
    HIP_OK(hipGetLastError());
    if (Lr > 0) {
      const int rc = ridge_fit_impl<double>(w + o.S, w + o.Mr, n, K, C, lambdas, Lr, w + o.X, (int32_t *)(w + o.rinfo),
                                            w + o.ridge, ws_bytes - o.ridge, st);
      if (rc != CVM_OK) return rc;
    }
    fa.Mr = ma.Mr; fa.X = (const double *)(w + o.X); fa.head = ma.head; fa.class_w = cw;
    fa.flag = ma.flag; fa.rinfo = (const int32_t *)(w + o.rinfo);
    fa.coef = (char *)coef + (size_t)f0 * L * K * C * esz;
    fa.intercept = (char *)intercept + (size_t)f0 * L * C * esz;
    fa.info = info + (size_t)f0 * L;
    fa.K = K; fa.C = C; fa.L = L; fa.Lr = Lr;
    hipLaunchKernelGGL(lda_finish_kernel<T>, dim3((unsigned)(n * L)), dim3(LDA_THREADS), 0, st, fa);
    HIP_OK(hipGetLastError());
  }
  return CVM_OK;
}
