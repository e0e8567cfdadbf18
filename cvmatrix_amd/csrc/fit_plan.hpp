// fit_plan.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, before pls.hpp).
// What the fit-stage solvers share on the host side: how many workspace slots run at once, which problems a slot's
// workgroup takes, how many folds a chunked solver handles per pass, and the dispatch on the element type.
// Plain C++: a host-only program may include this file (tests/fit_plan_check.cpp does).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include "../../include/cvmhip.h"

#ifdef __HIPCC__
#define CVM_HD __host__ __device__
#else
#define CVM_HD
#endif

int fail(int code, const char *fmt, const char *detail);       // host.hpp

// ---- slot plan (ridge, enet, omp, pcr, pcr_blocked): P independent problems, `per` bytes of workspace each while
// it runs, at most `cap` in flight.  Less workspace than the full size runs fewer at once with the same bits.
inline size_t slot_workspace_bytes(int64_t P, size_t per, int cap) {
  return (size_t)(P < 1 ? 1 : P > cap ? cap : P) * per;
}
// slots that run at once: min(P, ws_bytes / per, cap), P >= 0; so 0 when not even one fits.  A solver refuses
// ws_bytes < per (CVM_EWORKSPACE) before it looks at P: an empty batch with too small a workspace is refused too.
inline int slot_count(int64_t P, size_t per, size_t ws_bytes, int cap) {
  const size_t fit = ws_bytes / per;
  const int64_t G = P < cap ? P : cap;
  return (int)((size_t)G < fit ? (size_t)G : fit);
}

// ---- slot-to-problem map (ridge, enet, omp): workgroup b of G takes problems slot_first(b, G), + G, + 2 G, ...
// Workgroups that share b % 8 take consecutive first problems (the map is a permutation of 0 .. G-1), so the
// problems of one fold, consecutive in the problem order, run on one XCD and read XTX[f] from that XCD's L2
// (speed only).
CVM_HD inline int slot_first(int b, int G) {
  int t = b >> 3;
  for (int y = 0; y < (b & 7); ++y) t += (G - y + 7) >> 3;
  return t;
}

// ---- chunk plan (lda, pcalda): the workspace holds the records of n folds at a time.  The largest n in
// [1, top] with need(n) <= ws_bytes, need non-decreasing; 1 if there is none (the caller has refused what
// cannot run one fold).
template <class Need>
inline int64_t folds_per_chunk(int64_t top, size_t ws_bytes, Need &&need) {
  if (top < 1) return 1;
  if (need(top) <= ws_bytes) return top;
  int64_t lo = 1, hi = top;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (need(mid) <= ws_bytes) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- dtype dispatch: fn(double{}) or fn(float{}), the argument list written once in a generic lambda
template <class Fn>
inline int by_dtype(int dtype, const char *who, Fn &&fn) {
  if (dtype == CVM_F64) return fn(double{});
  if (dtype == CVM_F32) return fn(float{});
  return fail(CVM_EINVAL, "%s: dtype must be CVM_F32 or CVM_F64", who);
}
