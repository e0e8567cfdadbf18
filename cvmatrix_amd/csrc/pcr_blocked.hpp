// pcr_blocked.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, after pcr.hpp).
// The second eigensolver behind the contract of pcr.hpp (cvm_pcr_blocked_fit): a cyclic two-sided BLOCK Jacobi
// method, many workgroups per fold, the heavy part 64 x 64 x 64 float64 products on v_mfma_f64_16x16x4_f64.
// 1 <= K <= 4096.
//
// Per fold, with b = PCRB_BLOCK = 32, nb = ceil(K / b) blocks, m = nb rounded up to even (at least 2), h = m / 2:
//   * S (starts as XTX[f]) and V (starts as I) live in the fold's workspace slot, Kp x Kp with Kp = m b, the
//     padding zero.  A padded index never rotates (its off-diagonal entries are exactly 0) and is left out of
//     the ordering; the padding block is paired like any other, so that the block beside it still sweeps its own
//     diagonal block in that round (with nb = 1 it is the only partner there is).
//   * a sweep is m - 1 rounds in the round-robin order of pcr_kernel applied to blocks: round r pairs blocks
//     (m-1, r) and ((r+i) mod (m-1), (r-i) mod (m-1)).  A round is two launches, ordered by the stream alone:
//       pcrb_sub_kernel  one workgroup per (fold, pair P = (I, J)): gathers [S_II S_IJ; S_JI S_JJ] (64 x 64) into
//                        LDS with Q = I beside it, runs ONE cyclic scalar Jacobi sweep on it (63 rounds of 32
//                        pairs, the rotation formulas and the rule |S_pq| > 2^-52 ||XTX[f]||_F of pcr_kernel, 2 x 2
//                        blocks owned by one thread each so that the tile stays symmetric to the bit), writes the
//                        tile and Q_P back and the word "pair P rotated in this round"; a tile with nothing above
//                        the threshold is left alone;
//       pcrb_upd_kernel  one workgroup per (fold, P < R) tile of S: Q_P^T S_PR Q_R, the mirror tile written as the
//                        transpose of the same numbers; one per (fold, 64 rows of V, P): V[:, P] <- V[:, P] Q_P.
//                        A workgroup loads its whole tile before it stores any of it; a tile neither of whose
//                        pairs rotated is not touched.  Every output element is the sum over k = 0 .. 63 in the
//                        fixed order of the MFMA chain.
//   * after a sweep pcrb_collect_kernel closes the fold's "rotated in this sweep" word; the host reads one word
//     per fold of the batch (a copy on the caller's stream and a wait for it: ONE WAIT PER SWEEP, unlike
//     cvm_pcr_fit).  A fold whose word is clear gets pcrb_finish_kernel (steps 3 and 4 of pcr_kernel: ordering,
//     signs, n_fit, compensated scores, coefficients summed in the order j = 0, 1, ...) and is done: its
//     workgroups in later launches exit on the done word.
// No workgroup ever waits for another: no grid barrier, no flag is spun on.  No float atomics; a fold's bits
// depend on its own matrices, rank_tol and max_sweeps alone.
#pragma once

constexpr int PCRB_BLOCK = 32;
constexpr int PCRB_TILE = 2 * PCRB_BLOCK;
constexpr int PCRB_LD = PCRB_TILE + 2;      // LDS row stride in float64: 132 dwords = 4 mod 64, so the 16 rows x 2 k
                                            // of an MFMA A operand (ds_read_b64, groups of 32 lanes) fall on 64 banks
constexpr int PCRB_THREADS = 256;
constexpr int PCRB_MAXK = 4096;
constexpr int PCRB_MAXSLOTS = 512;          // folds in flight at most
constexpr int PCRB_WORDS = 8;               // rotated in this sweep, done, to finish, sweeps run
constexpr size_t PCRB_SUB_LDS = (size_t)2 * PCRB_TILE * PCRB_LD * 8 + 4 * PCRB_BLOCK * 8 + (3 * PCRB_BLOCK + 2) * 4;
constexpr size_t PCRB_UPD_LDS = (size_t)2 * PCRB_TILE * PCRB_LD * 8;
static_assert(PCRB_BLOCK == 32 && PCRB_THREADS == 256, "the index arithmetic below is written for 32 and 256");

struct PcrbArgs {
  const void *XTX, *XTY;                // [F][K][K], [F][K][M] (XTY NULL: PCA only)
  void *B, *V;                          // [F][A][K][M], [F][K][A] (each may be NULL)
  double *eig;                          // [F][A]
  int32_t *n_fit, *sweeps;              // [F]
  char *ws;                             // G slots of `per` bytes
  size_t per;
  int64_t f0;                           // slot g holds fold f0 + g
  double rank_tol;
  int K, M, A, Kp, h, G;
};

__host__ __device__ inline int pcrb_m(int K) {
  const int nb = (K + PCRB_BLOCK - 1) / PCRB_BLOCK;
  return (nb + 1) & ~1;
}
// a slot: S, V (Kp x Kp), h matrices Q (64 x 64), the coefficient sum (K x M), the signs (Kp), the threshold,
// then int32: the ordering (Kp), "pair rotated in this round" (h), the fold's words, the batch's status array
// (PCRB_MAXSLOTS, used in slot 0 only).  The one statement of that layout, as byte offsets (S at 0): the slot's
// size, the kernels' pointers and the host's read of the status array all come from it.
struct PcrbLayout {
  size_t V, Q, acc, sgn, thr, ord, rot, word, status, end;
};
__host__ __device__ inline PcrbLayout pcrb_layout(int K, int M, int Kp, int h) {
  PcrbLayout o;
  o.V = (size_t)Kp * Kp * 8;
  o.Q = 2 * o.V;
  o.acc = o.Q + (size_t)h * PCRB_TILE * PCRB_TILE * 8;
  o.sgn = o.acc + (size_t)K * M * 8;
  o.thr = o.sgn + (size_t)Kp * 8;
  o.ord = o.thr + 2 * 8;
  o.rot = o.ord + (size_t)Kp * 4;
  o.word = o.rot + (size_t)h * 4;
  o.status = o.word + PCRB_WORDS * 4;
  o.end = o.status + PCRB_MAXSLOTS * 4;
  return o;
}
inline size_t pcrb_slot_bytes(int K, int M) {
  const int m = pcrb_m(K);
  return align_up(pcrb_layout(K, M, m * PCRB_BLOCK, m / 2).end, 256);
}

struct PcrbSlot {
  double *S, *V, *Q, *acc, *sgn, *thr;
  int *ord, *rot, *word, *status;
};
__device__ inline PcrbSlot pcrb_slot(const PcrbArgs &a, int g) {
  const PcrbLayout o = pcrb_layout(a.K, a.M, a.Kp, a.h);
  char *p = a.ws + (size_t)g * a.per;
  auto d = [p](size_t off) { return reinterpret_cast<double *>(p + off); };
  auto i = [p](size_t off) { return reinterpret_cast<int *>(p + off); };
  return PcrbSlot{d(0), d(o.V), d(o.Q), d(o.acc), d(o.sgn), d(o.thr), i(o.ord), i(o.rot), i(o.word), i(o.status)};
}

// pair i of round r among m players, the round-robin order of pcr_kernel: p < q
__device__ inline void pcrb_pair(int r, int i, int m, int &p, int &q) {
  const int u = i == 0 ? m - 1 : (r + i) % (m - 1);
  const int v = i == 0 ? r : (r - i + (m - 1)) % (m - 1);
  p = u < v ? u : v;
  q = u < v ? v : u;
}

template <typename T>
__device__ inline void pcrb_nan_fold(const PcrbArgs &a, int64_t f, int tid, int sweeps) {
  const double nan = __builtin_nan("");
  const int K = a.K, M = a.M, A = a.A;
  if (a.B) {
    T *Bo = (T *)a.B + (size_t)f * A * K * M;
    for (size_t i = tid; i < (size_t)A * K * M; i += PCRB_THREADS) Bo[i] = (T)nan;
  }
  if (a.V) {
    T *Vo = (T *)a.V + (size_t)f * K * A;
    for (size_t i = tid; i < (size_t)K * A; i += PCRB_THREADS) Vo[i] = (T)nan;
  }
  for (int i = tid; i < A; i += PCRB_THREADS) a.eig[(size_t)f * A + i] = nan;
  if (tid == 0) {
    a.n_fit[f] = -1;
    a.sweeps[f] = sweeps;
  }
}

// S = XTX[f] and V = I with their padding: block (g, y) fills rows 64 y .. 64 y + 63.  Block (g, 0) also
// takes ||XTX[f]||_F in the order of pcr_kernel (by thread in index order, then a fixed tree), looks for
// anything not finite and sets the fold's words.
template <typename T>
__global__ __launch_bounds__(PCRB_THREADS) void pcrb_init_kernel(const PcrbArgs a) {
  __shared__ double red[PCRB_THREADS];
  __shared__ int flag;
  const int g = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
  const int K = a.K, M = a.M, Kp = a.Kp;
  const int64_t f = a.f0 + g;
  const PcrbSlot s = pcrb_slot(a, g);
  const T *X = (const T *)a.XTX + (size_t)f * K * K;
  for (int e = tid; e < PCRB_TILE * Kp; e += PCRB_THREADS) {
    const int rl = e / Kp, c = e - rl * Kp, r = PCRB_TILE * y + rl;
    s.S[(size_t)r * Kp + c] = (r < K && c < K) ? (double)X[(size_t)r * K + c] : 0.0;
    s.V[(size_t)r * Kp + c] = r == c ? 1.0 : 0.0;
  }
  if (y) return;
  if (tid == 0) flag = 0;
  __syncthreads();
  double ss = 0.0;
  int bad = 0;
  for (int e = tid; e < K * K; e += PCRB_THREADS) {
    const double v = (double)X[e];
    if (!(fabs(v) <= 1.79769313486231570815e+308)) bad = 1;
    ss += v * v;
  }
  if (a.XTY) {
    const T *Y = (const T *)a.XTY + (size_t)f * K * M;
    for (int e = tid; e < K * M; e += PCRB_THREADS)
      if (!(fabs((double)Y[e]) <= 1.79769313486231570815e+308)) bad = 1;
  }
  red[tid] = ss;
  if (bad) flag = 1;
  __syncthreads();
  for (int w = PCRB_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] = red[tid] + red[tid + w];
    __syncthreads();
  }
  const double fro = sqrt(red[0]);
  const int notfinite = flag || !(fro <= 1.79769313486231570815e+308);
  if (tid == 0) {
    *s.thr = 0x1p-52 * fro;
    s.word[0] = 0;                      // rotated in this sweep
    s.word[1] = notfinite;              // done
    s.word[2] = 0;                      // to finish
    s.word[3] = 0;                      // sweeps run
  }
  if (notfinite) pcrb_nan_fold<T>(a, f, tid, 0);
}

// Launch 1 of a round: one cyclic scalar Jacobi sweep on the 64 x 64 diagonal tile of pair blockIdx.x.
__global__ __launch_bounds__(PCRB_THREADS) void pcrb_sub_kernel(const PcrbArgs a, const int r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pcrb_smem[];
  double *T = reinterpret_cast<double *>(pcrb_smem), *Q = T + PCRB_TILE * PCRB_LD;
  double *rc = Q + PCRB_TILE * PCRB_LD, *rs = rc + PCRB_BLOCK, *rt = rs + PCRB_BLOCK, *rb = rt + PCRB_BLOCK;
  int *rp = reinterpret_cast<int *>(rb + PCRB_BLOCK), *rq = rp + PCRB_BLOCK, *rf = rq + PCRB_BLOCK, *fl = rf + PCRB_BLOCK;
  const int i = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const PcrbSlot s = pcrb_slot(a, g);
  if (s.word[1]) return;
  const int Kp = a.Kp;
  int I, J;
  pcrb_pair(r, i, 2 * a.h, I, J);
  const double thr = *s.thr;
  int big = 0;
  for (int e = tid; e < PCRB_TILE * PCRB_TILE; e += PCRB_THREADS) {
    const int x = e >> 6, c = e & 63;
    const int gx = (x < PCRB_BLOCK ? I : J) * PCRB_BLOCK + (x & 31), gc = (c < PCRB_BLOCK ? I : J) * PCRB_BLOCK + (c & 31);
    const double v = s.S[(size_t)gx * Kp + gc];
    T[x * PCRB_LD + c] = v;
    Q[x * PCRB_LD + c] = x == c ? 1.0 : 0.0;
    if (x != c && fabs(v) > thr) big = 1;
  }
  if (tid == 0) fl[0] = 0;
  if (!__syncthreads_or(big)) {         // nothing above the threshold: no pair of this tile would rotate
    if (tid == 0) s.rot[i] = 0;
    return;
  }
  constexpr int mm = PCRB_TILE, hh = PCRB_BLOCK;
  for (int rr = 0; rr < mm - 1; ++rr) {
    if (tid < hh) {
      int p, q;
      pcrb_pair(rr, tid, mm, p, q);
      double c = 1.0, sn = 0.0, t = 0.0;
      const double spq = T[p * PCRB_LD + q];
      int rot = 0;
      if (fabs(spq) > thr) {
        const double zeta = (T[q * PCRB_LD + q] - T[p * PCRB_LD + p]) / (2.0 * spq);
        t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        c = 1.0 / sqrt(1.0 + t * t);
        sn = c * t;
        rot = 1;
        fl[0] = 1;
      }
      rp[tid] = p; rq[tid] = q;
      rc[tid] = c; rs[tid] = sn; rt[tid] = t; rb[tid] = spq; rf[tid] = rot;
    }
    __syncthreads();
    // T <- J^T T J by 2 x 2 blocks (rows of pair ii, columns of pair jj), each owned by one thread
#pragma unroll
    for (int un = 0; un < hh * hh / PCRB_THREADS; ++un) {
      const int e = tid + un * PCRB_THREADS;
      const int ii = e >> 5, jj = e & 31;
      if (!(rf[ii] | rf[jj])) continue;
      const int pi = rp[ii], qi = rq[ii], pj = rp[jj], qj = rq[jj];
      const double xa = T[pi * PCRB_LD + pj], xb = T[pi * PCRB_LD + qj], xc = T[qi * PCRB_LD + pj], xd = T[qi * PCRB_LD + qj];
      double r11, r12, r21, r22;
      if (ii == jj) {
        r11 = xa - rt[ii] * rb[ii];
        r22 = xd + rt[ii] * rb[ii];
        r12 = r21 = 0.0;
      } else {
        const double ci = rc[ii], si = rs[ii], cj = rc[jj], sj = rs[jj];
        const double cc = ci * cj, sc = si * cj, cs = ci * sj, s2 = si * sj;
        r11 = (cc * xa + s2 * xd) - (cs * xb + sc * xc);
        r12 = (cs * xa - sc * xd) + (cc * xb - s2 * xc);
        r21 = (sc * xa - cs * xd) + (cc * xc - s2 * xb);
        r22 = (s2 * xa + cc * xd) + (sc * xb + cs * xc);
      }
      T[pi * PCRB_LD + pj] = r11;
      T[pi * PCRB_LD + qj] = r12;
      T[qi * PCRB_LD + pj] = r21;
      T[qi * PCRB_LD + qj] = r22;
    }
    // Q <- Q J: row k, pair jj
#pragma unroll
    for (int un = 0; un < mm * hh / PCRB_THREADS; ++un) {
      const int e = tid + un * PCRB_THREADS;
      const int k = e >> 5, jj = e & 31;
      if (!rf[jj]) continue;
      const int pj = rp[jj], qj = rq[jj];
      const double c = rc[jj], sn = rs[jj];
      const double vp = Q[k * PCRB_LD + pj], vq = Q[k * PCRB_LD + qj];
      Q[k * PCRB_LD + pj] = c * vp - sn * vq;
      Q[k * PCRB_LD + qj] = sn * vp + c * vq;
    }
    __syncthreads();
  }
  const int any = fl[0];
  if (any) {
    for (int e = tid; e < PCRB_TILE * PCRB_TILE; e += PCRB_THREADS) {
      const int x = e >> 6, c = e & 63;
      const int gx = (x < PCRB_BLOCK ? I : J) * PCRB_BLOCK + (x & 31), gc = (c < PCRB_BLOCK ? I : J) * PCRB_BLOCK + (c & 31);
      s.S[(size_t)gx * Kp + gc] = T[x * PCRB_LD + c];
      s.Q[(size_t)i * PCRB_TILE * PCRB_TILE + e] = Q[x * PCRB_LD + c];
    }
  }
  if (tid == 0) {
    s.rot[i] = any;
    if (any) s.word[0] = 1;             // (a plain store of 1 from every workgroup that rotated)
  }
}

typedef double pcrb_v4d __attribute__((ext_vector_type(4)));

// acc[c] (C/D map: register q of lane l = element (16 w + (l >> 4) + 4 q, 16 c + (l & 15))) into the tile X
__device__ inline void pcrb_store_acc(double *X, const pcrb_v4d (&acc)[4], int w, int lr, int lk) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) X[(16 * w + lk + 4 * q) * PCRB_LD + 16 * c + lr] = acc[c][q];
}

// Launch 2 of a round: the off-diagonal tiles of S and the column tiles of V.
__global__ __launch_bounds__(PCRB_THREADS) void pcrb_upd_kernel(const PcrbArgs a, const int r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pcrb_smem[];
  double *Xa = reinterpret_cast<double *>(pcrb_smem), *Xb = Xa + PCRB_TILE * PCRB_LD;
  const int g = blockIdx.y, tid = threadIdx.x;
  const PcrbSlot s = pcrb_slot(a, g);
  if (s.word[1]) return;
  const int h = a.h, Kp = a.Kp, nS = h * (h - 1) / 2;
  int t = blockIdx.x;
  int rb0, rb1, cb0, cb1;               // first row / column of the tile's two blocks
  int pi = -1, pj, fi = 0, fj;
  double *X;
  if (t < nS) {                         // tile (pair pi, pair pj) of S, pi < pj
    pi = 0;
    while (t >= h - 1 - pi) { t -= h - 1 - pi; ++pi; }
    pj = pi + 1 + t;
    fi = s.rot[pi]; fj = s.rot[pj];
    if (!(fi | fj)) return;
    pcrb_pair(r, pi, 2 * h, rb0, rb1);
    rb0 *= PCRB_BLOCK; rb1 *= PCRB_BLOCK;
    X = s.S;
  } else {                              // 64 rows of V, the columns of pair pj
    t -= nS;
    const int rowtile = t / h;
    pj = t - rowtile * h;
    fj = s.rot[pj];
    if (!fj) return;
    rb0 = PCRB_TILE * rowtile; rb1 = rb0 + PCRB_BLOCK;
    X = s.V;
  }
  pcrb_pair(r, pj, 2 * h, cb0, cb1);
  cb0 *= PCRB_BLOCK; cb1 *= PCRB_BLOCK;
  const int lane = tid & 63, w = tid >> 6, lr = lane & 15, lk = lane >> 4;

  for (int e = tid; e < PCRB_TILE * PCRB_TILE; e += PCRB_THREADS) {
    const int x = e >> 6, c = e & 63;
    Xa[x * PCRB_LD + c] = X[(size_t)((x < PCRB_BLOCK ? rb0 : rb1) + (x & 31)) * Kp + (c < PCRB_BLOCK ? cb0 : cb1) + (c & 31)];
    if (fj) Xb[x * PCRB_LD + c] = s.Q[(size_t)pj * PCRB_TILE * PCRB_TILE + e];
  }
  __syncthreads();
  pcrb_v4d acc[4];
  if (fj) {                             // X <- X Q_pj
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = pcrb_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int k0 = 0; k0 < PCRB_TILE; k0 += 4) {
      const double av = Xa[(16 * w + lr) * PCRB_LD + k0 + lk];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Xb[(k0 + lk) * PCRB_LD + 16 * c + lr], acc[c], 0, 0, 0);
    }
    __syncthreads();
    pcrb_store_acc(Xa, acc, w, lr, lk);
  }
  if (fi) {                             // X <- Q_pi^T X
    for (int e = tid; e < PCRB_TILE * PCRB_TILE; e += PCRB_THREADS)
      Xb[(e >> 6) * PCRB_LD + (e & 63)] = s.Q[(size_t)pi * PCRB_TILE * PCRB_TILE + e];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = pcrb_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int k0 = 0; k0 < PCRB_TILE; k0 += 4) {
      const double av = Xb[(k0 + lk) * PCRB_LD + 16 * w + lr];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Xa[(k0 + lk) * PCRB_LD + 16 * c + lr], acc[c], 0, 0, 0);
    }
    __syncthreads();
    pcrb_store_acc(Xa, acc, w, lr, lk);
  }
  __syncthreads();
  for (int e = tid; e < PCRB_TILE * PCRB_TILE; e += PCRB_THREADS) {
    const int x = e >> 6, c = e & 63;
    X[(size_t)((x < PCRB_BLOCK ? rb0 : rb1) + (x & 31)) * Kp + (c < PCRB_BLOCK ? cb0 : cb1) + (c & 31)] = Xa[x * PCRB_LD + c];
  }
  if (pi >= 0)                          // the mirror tile of S: the transpose of the same numbers
    for (int e = tid; e < PCRB_TILE * PCRB_TILE; e += PCRB_THREADS) {
      const int c = e >> 6, x = e & 63;
      X[(size_t)((c < PCRB_BLOCK ? cb0 : cb1) + (c & 31)) * Kp + (x < PCRB_BLOCK ? rb0 : rb1) + (x & 31)] = Xa[x * PCRB_LD + c];
    }
}

// After a sweep: a fold that made no rotation is marked to finish and done; the status array of the batch
// (bit 0 done, bit 1 to finish) goes to slot 0 for the host's one copy.
__global__ __launch_bounds__(PCRB_MAXSLOTS) void pcrb_collect_kernel(const PcrbArgs a, const int sweep) {
  const int g = threadIdx.x;
  if (g >= a.G) return;
  const PcrbSlot s = pcrb_slot(a, g);
  if (!s.word[1]) {
    if (s.word[0] == 0) {
      s.word[1] = 1;
      s.word[2] = 1;
      s.word[3] = sweep;
    }
    s.word[0] = 0;
  }
  pcrb_slot(a, 0).status[g] = s.word[1] | (s.word[2] << 1);
}

// Steps 3 and 4 of pcr_kernel (pcr_finish_fold, pcr.hpp) for the folds marked to finish; last != 0: the folds
// that are not done are out of sweeps and become NaN with sweeps -1.
template <typename T>
__global__ __launch_bounds__(PCRB_THREADS) void pcrb_finish_kernel(const PcrbArgs a, const int last) {
  __shared__ double lam[PCRB_MAXK];                   // diag(S) by index
  __shared__ double gs[PCR_GBATCH];                   // (v_j^T XTY) / lambda_j of a batch of components
  __shared__ int nfit_s;
  const int g = blockIdx.x, tid = threadIdx.x;
  const PcrbSlot s = pcrb_slot(a, g);
  const int64_t f = a.f0 + g;
  const int fin = s.word[2], done = s.word[1];
  if (!fin) {
    if (last && !done) pcrb_nan_fold<T>(a, f, tid, -1);
    return;
  }
  const int K = a.K, M = a.M, A = a.A;
  const T *Y = a.XTY ? (const T *)a.XTY + (size_t)f * K * M : nullptr;
  T *Bo = a.B ? (T *)a.B + (size_t)f * A * K * M : nullptr;
  T *Vo = a.V ? (T *)a.V + (size_t)f * K * A : nullptr;
  // diag(S) and the scores in LDS, the ordering, the signs and the running sum of the coefficients in the slot
  pcr_finish_fold<T, PCRB_THREADS>(s.S, s.V, a.Kp, K, M, A, a.rank_tol, s.word[3], Y, Bo, Vo, a.eig + (size_t)f * A,
                                   a.n_fit + f, a.sweeps + f, lam, s.sgn, gs, s.ord, &nfit_s, s.acc, tid);
  if (tid == 0) s.word[2] = 0;                        // (every thread read it before the barriers of the finish)
}

// min(F, PCRB_MAXSLOTS) slots.  Host arithmetic only (no device query).
size_t pcr_blocked_workspace_bytes(int64_t F, int K, int M) {
  return slot_workspace_bytes(F, pcrb_slot_bytes(K, M), PCRB_MAXSLOTS);
}

template <typename T>
int pcr_blocked_fit_impl(const void *XTX, const void *XTY, int64_t F, int K, int M, int A, double rank_tol,
                         int max_sweeps, void *B, double *eig, void *V, int32_t *n_fit, int32_t *sweeps, void *ws,
                         size_t ws_bytes, hipStream_t st) {
  const size_t per = pcrb_slot_bytes(K, M);
  if (ws_bytes < per) return fail(CVM_EWORKSPACE, "cvm_pcr_blocked_fit: workspace too small for one fold%s");
  if (F == 0) return CVM_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
  if (cs != hipStreamCaptureStatusNone)
    return fail(CVM_EINVAL, "cvm_pcr_blocked_fit: the stream is being captured and this entry waits for the device "
                            "once per sweep%s");
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(pcrb_sub_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)PCRB_SUB_LDS));
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(pcrb_upd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)PCRB_UPD_LDS));
  PcrbArgs a;
  memset(&a, 0, sizeof(a));
  a.XTX = XTX; a.XTY = XTY; a.B = B; a.V = V; a.eig = eig; a.n_fit = n_fit; a.sweeps = sweeps;
  a.ws = reinterpret_cast<char *>(ws);
  a.per = per;
  a.rank_tol = rank_tol;
  const int m = pcrb_m(K), h = m / 2;
  a.K = K; a.M = M; a.A = A; a.Kp = m * PCRB_BLOCK; a.h = h;
  const int64_t cap = slot_count(F, per, ws_bytes, PCRB_MAXSLOTS);
  // where the collect kernel leaves the status array: in slot 0
  const size_t off = pcrb_layout(K, M, a.Kp, h).status;
  const unsigned tiles = (unsigned)(h * (h - 1) / 2 + h * h);
  std::vector<int> status((size_t)cap);
  for (int64_t f0 = 0; f0 < F; f0 += cap) {
    const int G = (int)(F - f0 < cap ? F - f0 : cap);
    a.f0 = f0;
    a.G = G;
    hipLaunchKernelGGL(pcrb_init_kernel<T>, dim3((unsigned)G, (unsigned)h), dim3(PCRB_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    int left = G;
    for (int sweep = 1; sweep <= max_sweeps && left > 0; ++sweep) {
      for (int r = 0; r < m - 1; ++r) {
        hipLaunchKernelGGL(pcrb_sub_kernel, dim3((unsigned)h, (unsigned)G), dim3(PCRB_THREADS), PCRB_SUB_LDS, st, a, r);
        hipLaunchKernelGGL(pcrb_upd_kernel, dim3(tiles, (unsigned)G), dim3(PCRB_THREADS), PCRB_UPD_LDS, st, a, r);
      }
      hipLaunchKernelGGL(pcrb_collect_kernel, dim3(1), dim3(PCRB_MAXSLOTS), 0, st, a, sweep);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(status.data(), a.ws + off, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      int to_finish = 0;
      left = 0;
      for (int g = 0; g < G; ++g) {
        left += !(status[g] & 1);
        to_finish += (status[g] >> 1) & 1;
      }
      if (to_finish) {
        hipLaunchKernelGGL(pcrb_finish_kernel<T>, dim3((unsigned)G), dim3(PCRB_THREADS), 0, st, a, 0);
        HIP_OK(hipGetLastError());
      }
    }
    if (left > 0) {                     // out of sweeps
      hipLaunchKernelGGL(pcrb_finish_kernel<T>, dim3((unsigned)G), dim3(PCRB_THREADS), 0, st, a, 1);
      HIP_OK(hipGetLastError());
    }
  }
  return CVM_OK;
}
