// Host-only check of cvmatrix_amd/csrc/fold_plan.hpp (built and run by tests/test_fold_plan_host.py):
// the plan token, the scan of the folds' offsets, the parser of the route switches and the element size.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../cvmatrix_amd/csrc/fold_plan.hpp"

static char g_err[128];
int fail(int code, const char *fmt, const char *detail) { snprintf(g_err, sizeof(g_err), fmt, detail); return code; }

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  // token: round trip, the layout the callers of the C ABI see, refusal of what no call hands out
  for (int so : {1, 2, 7, (1 << 20) - 1})
    for (int sd : {1, 2, 7, (1 << 20) - 1})
      for (bool compacted : {false, true}) {
        const int64_t tok = pack_token(so, sd, compacted);
        CHECK(tok == ((int64_t)so | ((int64_t)sd << 20) | ((int64_t)compacted << 40)));
        PlanToken t{0, 0, !compacted};
        CHECK(unpack_token(tok, t) && t.s_off == so && t.s_diag == sd && t.compacted == compacted);
      }
  CHECK(pack_token(1, 1) == 1048577 && pack_token(4, 7) == pack_token(4, 7, false));
  PlanToken t;
  for (int64_t bad : {(int64_t)0, (int64_t)-1, INT64_MIN, (int64_t)1 << 41, pack_token(3, 5) | ((int64_t)1 << 41),
                      pack_token(3, 5) | ((int64_t)1 << 62), pack_token(0, 5), pack_token(3, 0), pack_token(0, 0, true)})
    CHECK(!unpack_token(bad, t));

  // fold_rows / folds_cover against a plain loop
  const std::vector<std::vector<int64_t>> cases = {
      {0}, {5}, {0, 0}, {0, 9}, {3, 3, 3, 3}, {0, 1, 9, 34, 124, 274}, {7, 7, 20, 20, 21}, {0, 150, 150, 151, 3000}};
  for (const auto &offs : cases) {
    const int64_t nf = (int64_t)offs.size() - 1;
    int64_t want_max = 0, want_present = 0;
    for (int64_t f = 0; f < nf; ++f) {
      const int64_t n = offs[f + 1] - offs[f];
      if (n > want_max) want_max = n;
      if (n > 0) ++want_present;
    }
    int64_t max_rows = -1, present = -1;
    CHECK(fold_rows(offs.data(), nf, "x", &max_rows, &present) == CVM_OK && max_rows == want_max && present == want_present);
    CHECK(fold_rows(offs.data(), nf, "x", nullptr, nullptr) == CVM_OK);
    const int64_t N = offs.back() - offs.front();
    CHECK(folds_cover(offs.data(), nf, N) && !folds_cover(offs.data(), nf, N - 1) && !folds_cover(offs.data(), nf, N + 1));
  }
  {
    const int64_t down[] = {0, 4, 3, 9};
    int64_t max_rows = -1, present = -1;
    g_err[0] = 0;
    CHECK(fold_rows(down, 3, "cvm_sweep_fit", &max_rows, &present) == CVM_EINVAL);
    CHECK(!strcmp(g_err, "cvm_sweep_fit: offsets must be non-decreasing") && max_rows == -1 && present == -1);
    CHECK(fold_rows(down, 1, "x", &max_rows, nullptr) == CVM_OK && max_rows == 4);      // (the pair is not looked at)
  }

  // the switch record from a table of strings
  using Env = std::map<std::string, const char *>;
  auto parse = [](const Env &env) {
    return parse_fold_switches([&](const char *name) { auto it = env.find(name); return it == env.end() ? nullptr : it->second; },
                               32, 128);
  };
  {
    const FoldSwitches d = parse({});
    CHECK(d.mid_minn == 0 && d.mid_maxn == 0 && !d.mid_off && !d.force_fallback && !d.no_fused && !d.prepass);
    CHECK(d.fused_order == 2 && d.fused_test == 0 && d.small_maxn == 0);
    CHECK(!d.no_direct && !d.no_compact && !d.no_inline_stats && !d.no_sweep_merge);
  }
  CHECK(parse({{"CVM_SMALL_MAXN", "1"}}).small_maxn == 32 && parse({{"CVM_SMALL_MAXN", "0"}}).small_maxn == 32);
  CHECK(parse({{"CVM_SMALL_MAXN", "999"}}).small_maxn == 128 && parse({{"CVM_SMALL_MAXN", "48"}}).small_maxn == 48);
  CHECK(parse({{"CVM_SMALL_MAXN", "x"}}).small_maxn == 32);
  CHECK(parse({{"CVM_FORCE_FALLBACK", "1"}}).force_fallback && !parse({{"CVM_FORCE_FALLBACK", "0"}}).force_fallback);
  CHECK(parse({{"CVM_MID_TILE", "0"}}).mid_off && !parse({{"CVM_MID_TILE", "1"}}).mid_off);
  CHECK(parse({{"CVM_MID_MINN", "9"}, {"CVM_MID_MAXN", "77"}}).mid_minn == 9 && parse({{"CVM_MID_MAXN", "77"}}).mid_maxn == 77);
  CHECK(parse({{"CVM_NO_FUSED", "1"}}).no_fused && parse({{"CVM_FUSED_PREPASS", "1"}}).prepass);
  CHECK(parse({{"CVM_FUSED_ORDER", "1"}}).fused_order == 1 && parse({{"CVM_FUSED_ORDER", "3"}}).fused_order == 2);
  CHECK(parse({{"CVM_FUSED_TEST_TIMEOUT", "3"}}).fused_test == 3);
  // (these four count as set whatever their text)
  CHECK(parse({{"CVM_NO_DIRECT", "0"}}).no_direct && parse({{"CVM_NO_COMPACT", ""}}).no_compact);
  CHECK(parse({{"CVM_NO_INLINE_STATS", "1"}}).no_inline_stats && parse({{"CVM_NO_SWEEP_MERGE", "1"}}).no_sweep_merge);
  CHECK(!parse({{"CVM_NO_DIRECT", "1"}}).no_compact);

  CHECK(esize_of(CVM_F64) == 8 && esize_of(CVM_F32) == 4);
  printf("fold plan ok\n");
  return 0;
}
