// fold_unions.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace).
// Training matrices of the complements of UNIONS of folds of a sweep (cvm_sweep_unions): nested
// cross-validation and repeated leave-several-groups-out need "all rows except folds f and g" for many
// sets of folds.  After cvm_sweep_fit the workspace holds every fold's raw validation update U_f and its
// column sums, so the matrix of the complement of a union S is  G - sum_{f in S} U_f  finished with the
// statistics of that complement (what the reference returns for the concatenated validation indices,
// cvmatrix.py:754-896) -- a few matrix reads and one matrix write per union, no row of X read again.
//
// Order of every sum: the folds of a union in ascending order, each fold's own ordered sum over its row
// splits formed first and then added to the running total -- apply_kernel's "segment sums, then their
// sum".  A compacted workspace (slot 0 = U_f, one partial per fold) and an uncompacted one therefore give
// the same bits, and a union of ONE fold gives the bits of cvm_sweep_fold_range (0 + U_f).  Everything
// behind the sums is finalize.hpp's: fold_column_finish, stage_tile_stats, finish_store_tile<T, true>.
// No atomics, no workgroup waits for another.
#pragma once

struct UnionArgs {
  FinArgs f;              // ws: the sweep's partials (fold 0 first, read only); fstats: the statistics vectors of the
                          // launch's unions (this call's scratch); seg0: first union of the launch (outputs, lists);
                          // offs: the folds' offsets; gx, gy: sub-tiles + panels, unions of the launch
  const int64_t *ufolds;  // device: the unions' fold numbers
  const int64_t *uoffs;   // device: union u owns ufolds[uoffs[u] .. uoffs[u + 1])
};

// The partial slots of a union in summing order: fold by fold (ascending), a fold's row splits in order.
struct UnionCursor {
  const int64_t *fl;
  int i, sp, nsp;
  long stride;
  __device__ __forceinline__ UnionCursor(const int64_t *fl_, int nsp_, int stride_) : fl(fl_), i(0), sp(0), nsp(nsp_), stride(stride_) {}
  __device__ __forceinline__ long next() {
    const long u = (long)fl[i] * stride + sp;
    if (++sp == nsp) { sp = 0; ++i; }
    return u;
  }
};

// Statistics of the complement of every union: one workgroup per (union, column chunk), modelled on
// fold_stats_kernel.  Writes the union's statistics vector (means, reciprocal stds, sw_train), the
// statistics outputs and out_fold.
template <typename T> __global__ __launch_bounds__(256) void union_stats_kernel(const UnionArgs ua) {
  const FinArgs &a = ua.f;
  const Geom &g = a.g;
  const int u = blockIdx.x;
  const int K = g.K, M = g.M;
  const int64_t o0 = ua.uoffs[a.seg0 + u];
  const int nf = (int)(ua.uoffs[a.seg0 + u + 1] - o0);
  const int64_t *fl = ua.ufolds + o0;
  const bool weighted = a.w != nullptr;
  // weight sum / non-zero count of the union's rows: every fold's own sum (split order), then their sum
  double swv = 0, nzv = 0;
  for (int i = 0; i < nf; ++i) {
    const long fo = (long)fl[i];
    double sf = 0, nn = 0;
    if (weighted) {
      for (int p = 0; p < a.s_diag; ++p) {
        const double *st = unit_stats<T>((char *)a.ws, g, fo * a.splits + p);
        sf += st[2 * g.Kp + 2 * g.Mp + 0]; nn += st[2 * g.Kp + 2 * g.Mp + 1];
      }
    } else {
      sf = nn = (double)(a.offs[fo + 1] - a.offs[fo]);
    }
    swv += sf; nzv += nn;
  }
  const double gsw = a.gstats[2 * K + 2 * M], gnz = a.gstats[2 * K + 2 * M + 1];
  const double swt = gsw - swv, nzt = gnz - nzv;
  const double divisor = (nzt - a.ddof) * swt / nzt;
  double *fs = a.fstats + (size_t)u * fstat_len(K, M);
  if (threadIdx.x == 0 && blockIdx.y == 0) {
    fs[2 * K + 2 * M] = swt;
    if (a.out_fold) {
      double *o = a.out_fold + 4 * (a.seg0 + u);
      o[0] = swt; o[1] = nzt; o[2] = swv; o[3] = nzv;
    }
  }
  const bool cX = a.flags & CVM_CENTER_X, cY = a.flags & CVM_CENTER_Y;
  const bool sX = a.flags & CVM_SCALE_X, sY = a.flags & CVM_SCALE_Y;
  const bool rXTY = a.flags & CVM_RET_XTY;
  const bool want_muX = cX || sX || (rXTY && cY), want_sdX = sX;
  const bool want_muY = rXTY && (cX || cY || sY), want_sdY = rXTY && sY;
  const int np = nf * a.s_diag;
  for (int c = blockIdx.y * blockDim.x + threadIdx.x; c < K + M; c += gridDim.y * blockDim.x) {
    const bool isX = c < K;
    const int cc = isX ? c : c - K;
    if (isX ? !(want_muX) : !(want_muY)) continue;
    const int s_src = isX ? cc : 2 * g.Kp + cc;
    const int q_src = isX ? g.Kp + cc : 2 * g.Kp + g.Mp + cc;
    // eight partials (16 loads) in flight; the adds stay one chain per fold, the folds' sums one chain
    double sv = 0, qv = 0, us = 0, uq = 0;
    int kk = 0, p = 0;
    UnionCursor cur(fl, a.s_diag, a.splits);
    for (; p + 8 <= np; p += 8) {
      double s8[8], q8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double *st = unit_stats<T>((char *)a.ws, g, cur.next());
        s8[j] = st[s_src]; q8[j] = st[q_src];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        us += s8[j]; uq += q8[j];
        if (++kk == a.s_diag) { sv += us; qv += uq; us = 0; uq = 0; kk = 0; }
      }
    }
    for (; p < np; ++p) {
      const double *st = unit_stats<T>((char *)a.ws, g, cur.next());
      us += st[s_src]; uq += st[q_src];
      if (++kk == a.s_diag) { sv += us; qv += uq; us = 0; uq = 0; kk = 0; }
    }
    const double gs = isX ? a.gstats[cc] : a.gstats[2 * K + cc];
    const double gq = isX ? a.gstats[K + cc] : a.gstats[2 * K + M + cc];
    fold_column_finish<T>(a, u, isX, cc, sv, qv, gs, gq, swt, divisor, isX ? want_sdX : want_sdY, fs);
  }
}

// One 64x64 sub-tile of a 128x128 upper tile (or one 128 x M panel of H) of one union, modelled on
// apply_kernel<T, true>: the folds' partials of the sub-tile summed in registers (16-byte loads, the
// pieces of UP partials -- of several folds -- requested before the first is added), staged in LDS,
// then finish_store_tile: total - update, rank-1 centring, reciprocal-std scaling, mirrored nontemporal
// store.  HBM-bound.
template <typename T> __global__ __launch_bounds__(APPLY_THREADS) void union_apply_kernel(const UnionArgs ua) {
  constexpr int NTHR = APPLY_THREADS;
  const FinArgs &a = ua.f;
  const Geom &g = a.g;
  __shared__ __attribute__((aligned(16))) double union_lds[ST * (ST + 1) + 4 * ST];
  // apply_kernel's numbering: a 1-D launch of 8 * ceil(gx * gy / 8) workgroups, every XCD a contiguous
  // range of (union, sub-tile) -- the sub-tiles of one union, which read the same folds' partials and the
  // same G tiles, meet in one L2
  const unsigned lin = blockIdx.x, tot = (unsigned)a.gx * (unsigned)a.gy;
  const unsigned per = (tot + 7) / 8;
  const unsigned item = (lin & 7) * per + (lin >> 3);
  if (item >= tot) return;
  const int x = (int)(item % (unsigned)a.gx);
  const int u = (int)(item / (unsigned)a.gx);
  const int K = g.K, M = g.M;
  const int64_t o0 = ua.uoffs[a.seg0 + u];
  const int nf = (int)(ua.uoffs[a.seg0 + u + 1] - o0);
  const int64_t *fl = ua.ufolds + o0;
  const double *fs = a.fstats + (size_t)u * fstat_len(K, M);
  const double swt = fs[2 * K + 2 * M];
  const bool cX = a.flags & CVM_CENTER_X, cY = a.flags & CVM_CENTER_Y;
  const bool sX = a.flags & CVM_SCALE_X, sY = a.flags & CVM_SCALE_Y;
  const size_t uo = (size_t)(a.seg0 + u);
  if (x < g.nTiles * APPLY_SUB) {
    if (!a.out_XTX) return;
    const int t = x / APPLY_SUB, sub = x - t * APPLY_SUB;
    int ti, tj;
    decode_tile(t, g.P, ti, tj);
    const int si = sub >> 1, sj = sub & 1;
    if (ti == tj && si > sj) return;                 // strictly lower: mirror of sub-tile (0,1)
    const int a0 = ti * TILE + si * ST, b0 = tj * TILE + sj * ST;
    if (a0 >= K || b0 >= K) return;
    double *st_lds = union_lds + ST * (ST + 1);
    double (*Ts)[ST + 1] = reinterpret_cast<double (*)[ST + 1]>(union_lds);
    constexpr int VW = 16 / sizeof(T);
    constexpr int LPR = ST / VW;
    typedef T vld_t __attribute__((ext_vector_type(VW)));
    const int tid = threadIdx.x;
    stage_tile_stats(st_lds, fs, a0, b0, K, tid);   // (visible after the barrier below)
    constexpr int NQ = ST * LPR / NTHR;
    double v[NQ][VW], uu[NQ][VW];
    const char *pp[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int q = tid + j * NTHR;
      const int lr = q / LPR, lc = (q - lr * LPR) * VW;
      const size_t off = (size_t)t * TILE * TILE + (size_t)(si * ST + lr) * TILE + sj * ST + lc;
      pp[j] = a.ws + off * sizeof(T);
#pragma unroll
      for (int e = 0; e < VW; ++e) { v[j][e] = 0; uu[j][e] = 0; }
    }
    constexpr int UP = 16 / (int)sizeof(T);          // partials requested before the first is added
    const int nsp = (ti == tj) ? a.s_diag : a.s_off;
    const int np = nf * nsp;
    UnionCursor cur(fl, nsp, a.splits);
    int kk = 0;
    auto close_fold = [&]() {                        // the fold's own sum joins the running total
#pragma unroll
      for (int j = 0; j < NQ; ++j)
#pragma unroll
        for (int e = 0; e < VW; ++e) { v[j][e] += uu[j][e]; uu[j][e] = 0; }
      kk = 0;
    };
    int p = 0;
    for (; p + UP <= np; p += UP) {
      vld_t qv[UP][NQ];
#pragma unroll
      for (int w = 0; w < UP; ++w) {
        const size_t so = (size_t)cur.next() * g.unit_bytes;
#pragma unroll
        for (int j = 0; j < NQ; ++j) qv[w][j] = *reinterpret_cast<const vld_t *>(pp[j] + so);
      }
#pragma unroll
      for (int w = 0; w < UP; ++w) {
#pragma unroll
        for (int j = 0; j < NQ; ++j)
#pragma unroll
          for (int e = 0; e < VW; ++e) uu[j][e] += (double)qv[w][j][e];
        if (++kk == nsp) close_fold();
      }
    }
    for (; p < np; ++p) {
      vld_t qv[NQ];
      const size_t so = (size_t)cur.next() * g.unit_bytes;
#pragma unroll
      for (int j = 0; j < NQ; ++j) qv[j] = *reinterpret_cast<const vld_t *>(pp[j] + so);
#pragma unroll
      for (int j = 0; j < NQ; ++j)
#pragma unroll
        for (int e = 0; e < VW; ++e) uu[j][e] += (double)qv[j][e];
      if (++kk == nsp) close_fold();
    }
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int q = tid + j * NTHR;
      const int lr = q / LPR, lc = (q - lr * LPR) * VW;
#pragma unroll
      for (int e = 0; e < VW; ++e) Ts[lr][lc + e] = v[j][e];
    }
    __syncthreads();
    T *out = (T *)a.out_XTX + uo * (size_t)K * K;
    finish_store_tile<T, true>(Ts, ti == tj && si == sj, a0, b0, K, (const T *)a.G, out, st_lds, swt, cX, sX, tid, NTHR);
  } else {
    if (!a.out_XTY || M == 0) return;
    const int ti = x - g.nTiles * APPLY_SUB;
    T *out = (T *)a.out_XTY + uo * (size_t)K * M;
    const T *Ht = (const T *)a.H;
    const size_t hoff = (g.tile_elems * sizeof(T) + 255) / 256 * 256;
    const int np = nf * a.s_diag;
    for (int e = threadIdx.x; e < TILE * M; e += NTHR) {
      const int ra = e / M, m = e - ra * M;
      const int ga = ti * TILE + ra;
      if (ga >= K) continue;
      const char *pp = a.ws + hoff + ((size_t)ga * g.Mp + m) * sizeof(T);
      UnionCursor cur(fl, a.s_diag, a.splits);
      double v = 0, us = 0;
      int kk = 0;
#pragma unroll 4
      for (int p = 0; p < np; ++p) {
        us += (double)*reinterpret_cast<const T *>(pp + (size_t)cur.next() * g.unit_bytes);
        if (++kk == a.s_diag) { v += us; us = 0; kk = 0; }     // (fold sums, then their sum)
      }
      const double mx = fs[ga], ix = fs[K + ga];
      const double my = fs[2 * K + m], iy = fs[2 * K + M + m];
      v = (double)Ht[(size_t)ga * M + m] - v;                  // apply_kernel's formula
      if (cX || cY) v -= swt * (mx * my);
      if (sX && sY) v = v * (ix * iy);
      else if (sX) v = v * ix;
      else if (sY) v = v * iy;
      out[(size_t)ga * M + m] = (T)v;
    }
  }
}

// A launch's global size in x (workgroups x 256 threads) stays below 2^32 (predict.hpp's note): a long list
// of unions is cut into launches of whole unions.
constexpr int64_t UNION_MAX_WGS = ((int64_t)1 << 32) / 256 - 1;

inline size_t union_workspace_bytes(int64_t n_unions, int K, int M) {
  return align_up((size_t)(n_unions > 0 ? n_unions : 1) * fstat_len(K, M) * 8, 256);
}

template <typename T>
int sweep_unions_impl(const FoldCall &c, const int64_t *union_folds, const int64_t *union_offsets, int64_t n_unions,
                      const Geom &g, const PlanToken &token, const void *sweep_ws, void *ws, hipStream_t st) {
  const int K = g.K, M = g.M;
  Plan p;
  p.g = g;
  set_plan_splits(p, token.s_off, token.s_diag);
  FinArgs f = fin_base(p, 1, 0, 0, sweep_ws);     // (segments: set per launch)
  if (token.compacted) f.s_off = f.s_diag = 1;    // (f.splits stays the slot stride)
  fin_fold_side(f, c);
  f.gx = g.nTiles * APPLY_SUB + g.P;
  const bool mats = f.out_XTX || f.out_XTY;
  const int64_t per_launch = (UNION_MAX_WGS - 7) / f.gx > 0 ? (UNION_MAX_WGS - 7) / f.gx : 1;
  for (int64_t u0 = 0; u0 < n_unions; u0 += per_launch) {
    const int64_t nb = n_unions - u0 < per_launch ? n_unions - u0 : per_launch;
    UnionArgs ua;
    ua.f = f;
    ua.f.seg0 = u0; ua.f.n_seg = (int)nb; ua.f.gy = (int)nb;
    ua.f.fstats = (double *)ws + (size_t)u0 * fstat_len(K, M);
    ua.ufolds = union_folds; ua.uoffs = union_offsets;
    hipLaunchKernelGGL((union_stats_kernel<T>), dim3((unsigned)nb, (unsigned)fold_stats_chunks(K, M, nb)), dim3(256), 0, st, ua);
    if (mats)
      hipLaunchKernelGGL((union_apply_kernel<T>), dim3((unsigned)(8 * (((size_t)f.gx * nb + 7) / 8))), dim3(APPLY_THREADS),
                         0, st, ua);
    HIP_OK(hipGetLastError());
  }
  return CVM_OK;
}
