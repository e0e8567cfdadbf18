// tile_product_loop.hpp -- the main loop of pls_sse_kernel (validation_sse.hpp) and predict_kernel (predict.hpp):
// TEXT, included once inside each of the two kernel bodies, after the kernel's own grid decoding, early return
// and `rows` prologue and before its epilogue.  (Text and not a device function: a force-inlined function is
// optimised once on its own before it is inlined, and the register allocation and the instruction order of
// the kernels then differ from the ones that were tuned and measured -- DESIGN.md 4.9.  Included, both
// kernels compile to what they were.)  The scheme, the constants and the host's choice among the variants:
// tile_product.hpp.
//
// Forms, for the workgroup's chunk of nr rows and its group of W = 64 NT columns from c0 on,
//   acc[rt][t] (MF<T>::acc_t [4][NT], declared here) = the chunk's standardised rows x the group's columns:
//   register r of acc[rt][t] is (row 16 rt + drow(lane, r), column 16 (wave NT + t) + lane % 16) of the group.
// Reads these names of the including kernel:
//   T, NT, V        the kernel's template parameters; W = 64 NT
//   Rcp             ScorerRcp or PredictRcp (tile_product.hpp)
//   X, ldX          const T *, int64_t: rows by number, pitch ldX elements
//   muX, sdX, Bf    const T *: the fold's K means, K standard deviations (nullptr: 0 / 1), [A][K][M] coefficients
//   K, M, C, c0     int: C = A M columns in all, c0 the group's first
//   nr              int: rows of this chunk, 1 .. 64
//   st_in_lds       int: the fold's K means and reciprocal standard deviations fit in LDS next to the stages
//   rows            int64_t [64] in LDS: the chunk's row numbers, written and synchronised (past nr: any readable row)
//   smem            unsigned char *: the dynamic LDS, tile_plan's `lds` bytes
//   tid, lane, wave, lk, lc   int: threadIdx.x, tid % 64, tid / 64, lane / 16, lane % 16
// SSE_STAMP: the -DCVM_STAMPS build (tile_product.hpp); nothing in the normal one.
  constexpr int BP = W + 16;                                  // LDS pitch of B: conflict-free fragment reads
  T *Zs = reinterpret_cast<T *>(smem);                        // [2][KS][ZP], [k][row]: the A operand's lanes run over rows
  T *Bs = Zs + 2 * SSE_KS * SSE_ZP;                           // [2][KS][BP], [k][column]
  typedef typename MF<T>::acc_t acc_t;
  acc_t acc[4][NT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = (acc_t){0, 0, 0, 0};
  // staging maps.  Z: thread -> (row zr = tid / 4, k quad zq = tid % 4): four CONSECUTIVE k of one
  // row (a wave instruction touches 16 rows' lines once), 4 / V loads.  B: piece e = tid + 256 i of
  // the stage's 16 x (W / V) pieces of V columns: k = e / (W / V), columns (e % (W / V)) V ...
  // All loads are branch-free -- rows past the chunk's end re-read a row of the fold, k past K re-reads
  // the last piece, columns past the group's end re-read column 0 -- and the values are zeroed (selected,
  // never multiplied: a NaN stays where it belongs) at the LDS write: a per-thread branch around a load
  // makes the compiler wait for everything in flight.
  typedef T vec_t __attribute__((ext_vector_type(V)));
  constexpr int ZL = 4 / V < 1 ? 1 : 4 / V;                   // Z loads per thread and stage
  constexpr int ZV = 4 / ZL;                                  // elements per Z load
  static_assert(V == 1 || V == 2 || V == 4, "V is 1 or 16 bytes' worth");
  constexpr int WP = W / V;                                   // pieces per k row
  constexpr int NB = SSE_KS * WP / 256;                       // B loads per thread and stage
  const int zr = tid >> 2, zq = tid & 3;
  const bool zok = zr < nr;
  const T *xrow = X + rows[zr] * ldX;
  const bool has_mu = muX != nullptr, has_sd = sdX != nullptr;
  // statistics: (mean, 1 / sd) of all K columns in LDS when they fit, else read per stage
  double *stl = reinterpret_cast<double *>(Bs + 2 * SSE_KS * BP);
  const bool st_lds = st_in_lds != 0;
  if (st_lds) {
    for (int k = tid; k < K; k += 256) {
      stl[2 * k] = has_mu ? (double)muX[k] : 0.0;
      stl[2 * k + 1] = has_sd ? Rcp::lds((double)sdX[k]) : 1.0;
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
        isd = has_sd ? Rcp::reg((double)zs[j][e]) : 1.0;
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
  // The next stage's requests and LDS writes are dealt out over the stage's 4 NT groups of four MFMAs
  // ("steps"), one or two per step and pinned there: a vector-memory instruction takes its wave
  // 150-450 cycles to issue on a busy CU and the matrix pipe runs dry behind a clump of them
  // (tools/sse_stamps.py: 12 loads 2.0 k, arithmetic and LDS writes 1.9 k cycles per stage next to
  // 6.8 k of MFMAs, one after the other).  Requests in the first half of the steps (rows first),
  // writes in the second half (coefficients first, rows -- the longest latency -- last).
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
  SSE_STAMP(0);
  // (narrow groups, NT < 3: several workgroups share a CU and hide each other's latencies; the
  //  requests go first, the writes last, unpinned -- C = 20 at K = 4096 in float32: 0.95 ms against
  //  1.6 ms with the pinned interleave)
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
      // (tiles past the group's last column multiply zeros: the four waves run side by side on
      //  their SIMDs, skipping a tile in one of them would not shorten the stage)
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
    SSE_STAMP(2);
    __syncthreads();
    SSE_STAMP(4);
  }
