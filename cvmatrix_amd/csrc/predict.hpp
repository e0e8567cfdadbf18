// predict.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after pcr.hpp).
// Out-of-fold predictions of every fold's linear models, and predictions for new rows: the stage after the
// model fitters.  For fold f, row i of the fold, model a and response m
//   out[r][a][m] = ((x_i - muX[f]) / sdX[f]) . B[f][a][:, m] * sdY[f][m] + muY[f][m]
// -- the products pls_sse_kernel (pls.hpp) forms and reduces to one sum per (fold, model, response), here
// stored whole.  The main loop is that kernel's scheme, found out on this chip and documented there: one
// workgroup = 64 rows x 64 NT of the A M columns, one wave per SIMD, wave w owns 16 NT columns for all 64
// rows; the standardised rows and the coefficient columns go through two LDS stages 16 k at a time, 16-byte
// global loads where K, M, the row pitch and the addresses allow (scalar ones otherwise), the fold's means
// and reciprocal standard deviations in LDS when they fit, the next stage's requests and LDS writes dealt
// out between the stage's groups of four MFMAs, every load branch-free and zeroed at the LDS write.
//
// FIXED ORDER.  One prediction is ONE accumulator chain: k runs over stages of 16 and steps of 4 (MF<T>,
// 16 x 16 x 4; k past K multiplies zeros), whatever NT, the vector width, the number of column groups and
// the place of the statistics are; z = (T)((x - mu) * (1 / sd)) is formed in float64 with ONE reciprocal
// (predict_rcp) on every route.  So the bits of one prediction depend on its row of X, its fold's
// statistics and its column of B alone -- not on the fold's other rows, the row's place in the fold, the
// other folds, A, the other columns of B, ldX, by_row, alignment or the stream.
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

// The reciprocal of a standard deviation, one formula on every route: v_rcp_f64 and TWO Newton steps.  The
// instruction's result is good to about 2^-24 relative (its documented accuracy is 2^29 units in the last
// place), one step r (2 - sd r) squares that to 2^-48 -- tens of units -- and the second to 2^-96; each step is
// two fused multiply-adds whose first forms the residual 1 - sd r with one rounding of a number that small, so
// what is left is the last step's own rounding: r = (1 / sd) (1 + d), |d| <= 2^-53 + 2^-94, one unit as the
// gate of the tests takes it.  (A zero, infinite or NaN sd gives NaN, never a finite number.)
__device__ __forceinline__ double predict_rcp(double sd) {
  double r = __builtin_amdgcn_rcp(sd);
  r = fma(fma(-sd, r, 1.0), r, r);
  return fma(fma(-sd, r, 1.0), r, r);
}

template <typename T, int NT, int V>
__global__ __launch_bounds__(256) void predict_kernel(const PredictArgs a) {
  constexpr int W = 64 * NT, BP = W + 16;                     // LDS pitch of B: conflict-free fragment reads
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
  T *Zs = reinterpret_cast<T *>(predict_smem);                // [2][KS][ZP], [k][row]: the A operand's lanes run over rows
  T *Bs = Zs + 2 * SSE_KS * SSE_ZP;                           // [2][KS][BP], [k][column]
  __shared__ int64_t rows[SSE_ROWS];
  const T *X = (const T *)a.X;
  const T *muX = a.muX ? (const T *)a.muX + (size_t)f * K : nullptr;
  const T *sdX = a.sdX ? (const T *)a.sdX + (size_t)f * K : nullptr;
  const T *Bf = (const T *)a.B + (size_t)f * a.A * K * M;
  if (tid < SSE_ROWS) {
    const bool ok = tid < nr;                                 // (rows past the end re-read the chunk's first row)
    const int64_t p = o0 + r0 + (ok ? tid : 0);
    rows[tid] = a.idx ? a.idx[p] : p;
  }
  __syncthreads();
  typedef typename MF<T>::acc_t acc_t;
  acc_t acc[4][NT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = (acc_t){0, 0, 0, 0};
  // staging maps, as in pls_sse_kernel.  Z: thread -> (row zr = tid / 4, k quad zq = tid % 4): four
  // consecutive k of one row, 4 / V loads.  B: piece e = tid + 256 i of the stage's 16 x (W / V) pieces of V
  // columns: k = e / (W / V), columns (e % (W / V)) V ...  All loads are branch-free -- rows past the fold's
  // end re-read a row of the fold, k past K re-reads the last piece, columns past the group's end re-read
  // column 0 -- and the values are zeroed (selected, never multiplied: a NaN stays where it belongs) at the
  // LDS write.
  typedef T vec_t __attribute__((ext_vector_type(V)));
  constexpr int ZL = 4 / V < 1 ? 1 : 4 / V;                   // Z loads per thread and stage
  constexpr int ZV = 4 / ZL;                                  // elements per Z load
  static_assert(V == 1 || V == 2 || V == 4, "V is 1 or 16 bytes' worth");
  constexpr int WP = W / V;                                   // pieces per k row
  constexpr int NB = SSE_KS * WP / 256;                       // B loads per thread and stage
  const int zr = tid >> 2, zq = tid & 3;
  const bool zok = zr < nr;
  const T *xrow = X + rows[zr] * a.ldX;
  const bool has_mu = muX != nullptr, has_sd = sdX != nullptr;
  double *stl = reinterpret_cast<double *>(Bs + 2 * SSE_KS * BP);   // (mean, 1 / sd) of all K columns
  const bool st_lds = a.st_in_lds != 0;
  if (st_lds) {
    for (int k = tid; k < K; k += 256) {
      stl[2 * k] = has_mu ? (double)muX[k] : 0.0;
      stl[2 * k + 1] = has_sd ? predict_rcp((double)sdX[k]) : 1.0;
    }
  }
  const T *mup = has_mu ? muX : xrow, *sdp = has_sd ? sdX : xrow;   // (absent statistics: a harmless second read of the row)
  size_t boff[NB];
  int blds[NB];
  bool bok[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int e = tid + 256 * i;
    const int kk = e / WP, col = (e - kk * WP) * V;
    bok[i] = c0 + col < C;                                    // (C is a multiple of V in the vector build)
    const int gcol = bok[i] ? c0 + col : 0;
    const int ba = gcol / M, bm = gcol - ba * M;
    boff[i] = ((size_t)ba * K + kk) * M + bm;
    blds[i] = kk * BP + col;
  }
  vec_t zv[ZL], zm[ZL], zs[ZL], bv[NB];
  auto loadZ = [&](int j, int k0) {
    const int k = k0 + 4 * zq + ZV * j;
    const int kc = k < K ? k : K - ZV;
    zv[j] = *reinterpret_cast<const vec_t *>(xrow + kc);
    if (!st_lds) {
      zm[j] = *reinterpret_cast<const vec_t *>(mup + kc);
      zs[j] = *reinterpret_cast<const vec_t *>(sdp + kc);
    }
  };
  auto loadB = [&](int i, int k0) {
    // (k0 + kk < K except in the last stage: there the row K - 1 is re-read and zeroed in storeB)
    const int kk = (tid + 256 * i) / WP;
    const size_t ko = (size_t)(k0 + kk < K ? k0 : K - 1 - kk) * M;
    bv[i] = *reinterpret_cast<const vec_t *>(Bf + boff[i] + ko);
  };
  auto storeZ = [&](int j, int k0, int buf) {
    T *Zb = Zs + buf * SSE_KS * SSE_ZP;
#pragma unroll
    for (int e = 0; e < ZV; ++e) {
      const int kq = 4 * zq + ZV * j + e, k = k0 + kq;
      double mu, isd;
      if (st_lds) {
        const int kc = k < K ? k : K - 1;
        mu = stl[2 * kc]; isd = stl[2 * kc + 1];
      } else {
        mu = has_mu ? (double)zm[j][e] : 0.0;
        isd = has_sd ? predict_rcp((double)zs[j][e]) : 1.0;
      }
      const T z = (T)(((double)zv[j][e] - mu) * isd);
      Zb[kq * SSE_ZP + zr] = (zok && k < K) ? z : (T)0;
    }
  };
  auto storeB = [&](int i, int k0, int buf) {
    T *Bb = Bs + buf * SSE_KS * BP;
    const int kk = (tid + 256 * i) / WP;
    const bool ok = bok[i] && k0 + kk < K;
    vec_t v = bv[i];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = ok ? v[e] : (T)0;
    *reinterpret_cast<vec_t *>(Bb + blds[i]) = v;
  };
  // the next stage's requests in the first half of the stage's 4 NT groups of four MFMAs (rows first), its
  // LDS writes in the second half (coefficients first, rows last), one or two per group and pinned there
  constexpr int STEPS = 4 * NT, NL = ZL + NB, NLS = (STEPS + 1) / 2, LPS = (NL + NLS - 1) / NLS;
  constexpr int NSS = STEPS - NLS, SPS = (NL + NSS - 1) / NSS;
  auto aux = [&](int step, int k1, int buf) {
    if (step < NLS) {
#pragma unroll
      for (int q = 0; q < LPS; ++q) {
        const int idx = step * LPS + q;
        if (idx < ZL) loadZ(idx, k1);
        else if (idx < NL) loadB(idx - ZL, k1);
      }
    } else {
#pragma unroll
      for (int q = 0; q < SPS; ++q) {
        const int idx = (step - NLS) * SPS + q;
        if (idx < NB) storeB(idx, k1, buf);
        else if (idx < NL) storeZ(idx - NB, k1, buf);
      }
    }
  };
  const int nst = (K + SSE_KS - 1) / SSE_KS;
#pragma unroll
  for (int j = 0; j < ZL; ++j) loadZ(j, 0);
#pragma unroll
  for (int i = 0; i < NB; ++i) loadB(i, 0);
  if (st_lds) __syncthreads();                                // (stl)
#pragma unroll
  for (int i = 0; i < NB; ++i) storeB(i, 0, 0);
#pragma unroll
  for (int j = 0; j < ZL; ++j) storeZ(j, 0, 0);
  __syncthreads();
  // (narrow groups, NT < 3: several workgroups share a CU and hide each other's latencies; the requests go
  //  first, the writes last, unpinned)
  constexpr bool PIN = NT >= 3;
  for (int s = 0; s < nst; ++s) {
    const bool more = s + 1 < nst;
    const int k1 = (s + 1) * SSE_KS, nbuf = (s + 1) & 1;      // (that buffer was last read before the previous barrier)
    const T *Zb = Zs + (s & 1) * SSE_KS * SSE_ZP, *Bb = Bs + (s & 1) * SSE_KS * BP;
    if (!PIN && more) {
#pragma unroll
      for (int j = 0; j < ZL; ++j) loadZ(j, k1);
#pragma unroll
      for (int i = 0; i < NB; ++i) loadB(i, k1);
    }
#pragma unroll
    for (int ks = 0; ks < SSE_KS; ks += 4) {
      T af[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) af[rt] = Zb[(ks + lk) * SSE_ZP + 16 * rt + lc];
      T bf[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) bf[t] = Bb[(ks + lk) * BP + 16 * (wave * NT + t) + lc];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt][t] = MF<T>::mfma(af[rt], bf[t], acc[rt][t]);
        if (PIN) {
          if (more) aux((ks / 4) * NT + t, k1, nbuf);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (!PIN && more) {
#pragma unroll
      for (int i = 0; i < NB; ++i) storeB(i, k1, nbuf);
#pragma unroll
      for (int j = 0; j < ZL; ++j) storeZ(j, k1, nbuf);
    }
    __syncthreads();
  }
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

// The launch plan, host arithmetic alone (cvm_cv_predict_plan hands it out: tests check it without a device).
// A launch's global size in x, workgroups x 256 threads, must stay below 2^32 (the HIP runtime refuses more),
// so a launch has at most 2^24 - 1 workgroups; the flat list of folds x groups x chunks workgroups is cut into
// launches of that many wherever the cut falls -- inside a fold too -- and a kernel finds its place from the
// launch's first flat number.  No limit on the number of folds or on the length of a fold follows from it.
constexpr int64_t PREDICT_MAX_WGS = ((int64_t)1 << 32) / 256 - 1;
struct PredictPlan {
  int nt, vec, groups, st_in_lds;
  int64_t chunks, total, launches;    // row chunks of the longest fold, workgroups in all, launches
  size_t lds;
};

// `vec`: K, M, the row pitch and every address allow 16-byte loads.  None of the choices changes a bit of the
// result (FIXED ORDER above); the variants and the choice among them are the scorer's (pls_sse_impl): as few
// column groups as possible (every group stages the rows again), then as little padding as possible.
bool predict_vec(int VW, const void *X, int64_t ldX, int K, int M, const void *muX, const void *sdX, const void *B) {
  auto al16 = [](const void *q) { return !q || (uintptr_t)q % 16 == 0; };
  return K % VW == 0 && M % VW == 0 && ldX % VW == 0 && K >= 4 && al16(X) && al16(B) && al16(muX) && al16(sdX);
}

PredictPlan predict_plan(int64_t F, int64_t max_rows, int K, int M, int A, int esize, bool vec) {
  PredictPlan p;
  p.vec = vec ? 1 : 0;
  p.chunks = (max_rows + SSE_ROWS - 1) / SSE_ROWS;
  if (p.chunks < 1) p.chunks = 1;
  const int C = A * M;
  // (float64 takes five column tiles per wave at most, four without 16-byte pieces: the wider variants of
  //  those combinations run out of registers)
  const int max_nt = esize == 8 ? (vec ? 5 : 4) : SSE_MAXNT;
  int best = 1 << 30;
  p.nt = 1;
  for (int c = 1; c <= max_nt; ++c) {
    const int groups = (C + 64 * c - 1) / (64 * c);
    const int cost = groups * (4 * c + 1);
    if (cost < best) { best = cost; p.nt = c; }
  }
  p.groups = (C + 64 * p.nt - 1) / (64 * p.nt);
  p.lds = (size_t)2 * SSE_KS * (SSE_ZP + 64 * p.nt + 16) * esize;
  // (statistics in LDS only where they do not cost residency: one workgroup per CU anyway, or a short K)
  p.st_in_lds = (p.lds + (size_t)K * 16 + 2048 <= PLS_LDS_BUDGET && (p.lds > 80 * 1024 || K <= 512)) ? 1 : 0;
  if (p.st_in_lds) p.lds += (size_t)K * 16;
  p.total = F * p.chunks * p.groups;
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
  constexpr int VW = 16 / (int)sizeof(T);
  const PredictPlan p = predict_plan(F, max_rows, K, M, A, (int)sizeof(T), predict_vec(VW, X, ldX, K, M, muX, sdX, B));
  const bool vec = p.vec != 0;
  const int nt = p.nt;
  const size_t lds = p.lds;
  a.n_chunks = p.chunks; a.groups = p.groups; a.st_in_lds = p.st_in_lds;
  void (*kern)(const PredictArgs) = nullptr;
#define CVM_PREDICT_PICK(N) kern = vec ? predict_kernel<T, N, VW> : predict_kernel<T, N, 1>
  switch (nt) {
    case 1: CVM_PREDICT_PICK(1); break;
    case 2: CVM_PREDICT_PICK(2); break;
    case 3: CVM_PREDICT_PICK(3); break;
    case 4: CVM_PREDICT_PICK(4); break;
    case 5:
      if constexpr (sizeof(T) == 8) kern = predict_kernel<T, 5, VW>;      // (vec only: see max_nt)
      else CVM_PREDICT_PICK(5);
      break;
    default:
      if constexpr (sizeof(T) == 4) CVM_PREDICT_PICK(6);
      break;
  }
#undef CVM_PREDICT_PICK
  if (!kern) return fail(CVM_EINVAL, "cvm_cv_predict: no kernel for this shape%s");
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int64_t b0 = 0; b0 < p.total; b0 += PREDICT_MAX_WGS) {
    const int64_t nb = p.total - b0 < PREDICT_MAX_WGS ? p.total - b0 : PREDICT_MAX_WGS;
    a.b0 = b0;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(256), lds, st, a);
    HIP_OK(hipGetLastError());
  }
  return CVM_OK;
}
