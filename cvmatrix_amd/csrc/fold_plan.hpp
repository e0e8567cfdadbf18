// fold_plan.hpp -- part of libcvmhip.so (included by cvmhip.hip inside its anonymous namespace, before host.hpp).
// What the fold-stage entries share on the host side before any launch: the plan token of the sweep, the scan of
// the folds' host offsets, the route switches of the environment, the element size of a dtype.
// Plain C++: a host-only program may include this file (tests/fold_plan_check.cpp does).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/cvmhip.h"

int fail(int code, const char *fmt, const char *detail);       // host.hpp

inline int esize_of(int dtype) { return dtype == CVM_F64 ? 8 : 4; }

// ---- plan token: what cvm_sweep_fit / cvm_sweep_all / cvm_stream_add / cvm_stream_close hand to the calls that read
// the partials they left: s_off | s_diag << 20 | compacted << 40
struct PlanToken { int s_off, s_diag; bool compacted; };
inline int64_t pack_token(int s_off, int s_diag, bool compacted = false) {
  return (int64_t)s_off | ((int64_t)s_diag << 20) | ((int64_t)(compacted ? 1 : 0) << 40);
}
// false for anything pack_token cannot have produced from splits >= 1
inline bool unpack_token(int64_t token, PlanToken &t) {
  if (token <= 0 || (token >> 41) != 0) return false;
  t.s_off = (int)(token & 0xfffff); t.s_diag = (int)((token >> 20) & 0xfffff);
  t.compacted = (token >> 40) & 1;
  return t.s_off >= 1 && t.s_diag >= 1;
}

// ---- the folds' rows from the host copy of the offsets: the longest fold and the folds that have rows (either
// may be null); CVM_EINVAL for a fold of negative length
inline int fold_rows(const int64_t *host_offsets, int64_t n_folds, const char *who, int64_t *max_rows, int64_t *present) {
  int64_t longest = 0, have = 0;
  for (int64_t f = 0; f < n_folds; ++f) {
    const int64_t n = host_offsets[f + 1] - host_offsets[f];
    if (n < 0) return fail(CVM_EINVAL, "%s: offsets must be non-decreasing", who);
    if (n > longest) longest = n;
    have += n > 0;
  }
  if (max_rows) *max_rows = longest;
  if (present) *present = have;
  return CVM_OK;
}
// do the (non-decreasing) offsets cut N rows into the folds?  Every caller has its own sentence for "no".
inline bool folds_cover(const int64_t *host_offsets, int64_t n_folds, int64_t N) {
  return host_offsets[n_folds] - host_offsets[0] == N;
}

// ---- route switches of the fold stage: read from the environment ONCE per process, at the first call of
// fold_switches() (tests, tools/route_matrix.sh and the experiment scripts set them in a child's environment; none
// is needed in production).  Not in the record: CVM_FORCE_SPLITS and CVM_RESIDENT, which have run-time setters
// (cvm_debug_force_splits, cvm_debug_resident) and so live in atomics of their own; CVM_DEBUG, which exists in the
// -DCVM_STAMPS diagnostic build only.
struct FoldSwitches {
  int mid_minn, mid_maxn;      // CVM_MID_MINN / CVM_MID_MAXN: row limits of mid_tile_kernel (0: the measured table)
  bool mid_off;                // CVM_MID_TILE=0: never mid_tile_kernel
  bool force_fallback;         // CVM_FORCE_FALLBACK=1: the general Gram kernel
  bool no_fused;               // CVM_NO_FUSED=1: partials + apply_kernel for one-unit folds too
  bool prepass;                // CVM_FUSED_PREPASS=1: statistics by colstats_kernel + fold_stats_kernel, not in the launch
  int fused_order;             // CVM_FUSED_ORDER: 2 = fold-major lists (default), 1 = every list's diagonal items first
  int fused_test;              // CVM_FUSED_TEST_TIMEOUT: WgramArgs::test_mode
  int small_maxn;              // CVM_SMALL_MAXN: row limit of the direct small-fold kernels, clamped (0: the measured table)
  bool no_direct;              // CVM_NO_DIRECT (set): never small_rows_kernel
  bool no_compact;             // CVM_NO_COMPACT (set): the sweep's fit finalize leaves the partials as they are
  bool no_inline_stats;        // CVM_NO_INLINE_STATS (set): fold_stats_kernel in front of apply_kernel, always
  bool no_sweep_merge;         // CVM_NO_SWEEP_MERGE (set): cvm_sweep_all by the kernels of its two halves
};
constexpr int SWITCH_SMALL_LO = 32, SWITCH_SMALL_HI = 128;     // SMALL_ROWS, SMALL_MAXN (host.hpp asserts it)
// the record from `get(name)` -> the variable's text or null; small_maxn clamped to [small_lo, small_hi]
template <class Get>
inline FoldSwitches parse_fold_switches(Get &&get, int small_lo, int small_hi) {
  auto num = [&](const char *name, int dflt) { const char *e = get(name); return e ? atoi(e) : dflt; };
  auto set = [&](const char *name) { return get(name) != nullptr; };
  FoldSwitches f;
  f.mid_minn = num("CVM_MID_MINN", 0); f.mid_maxn = num("CVM_MID_MAXN", 0);
  f.mid_off = num("CVM_MID_TILE", 1) == 0;
  f.force_fallback = num("CVM_FORCE_FALLBACK", 0) != 0;
  f.no_fused = num("CVM_NO_FUSED", 0) != 0;
  f.prepass = num("CVM_FUSED_PREPASS", 0) != 0;
  f.fused_order = num("CVM_FUSED_ORDER", 2) == 1 ? 1 : 2;
  f.fused_test = num("CVM_FUSED_TEST_TIMEOUT", 0);
  f.small_maxn = num("CVM_SMALL_MAXN", 0);
  if (set("CVM_SMALL_MAXN") && f.small_maxn < small_lo) f.small_maxn = small_lo;
  if (f.small_maxn > small_hi) f.small_maxn = small_hi;
  f.no_direct = set("CVM_NO_DIRECT");
  f.no_compact = set("CVM_NO_COMPACT");
  f.no_inline_stats = set("CVM_NO_INLINE_STATS");
  f.no_sweep_merge = set("CVM_NO_SWEEP_MERGE");
  return f;
}
inline const FoldSwitches &fold_switches() {
  static const FoldSwitches sw = parse_fold_switches([](const char *name) { return getenv(name); }, SWITCH_SMALL_LO, SWITCH_SMALL_HI);
  return sw;
}
