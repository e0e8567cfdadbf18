// Host-only check of cvmatrix_amd/csrc/fit_plan.hpp (built and run by tests/test_fit_plan_host.py):
// the slot-to-problem map, the slot plan, the chunk plan and the dtype dispatch against their definitions.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../cvmatrix_amd/csrc/fit_plan.hpp"

static char g_err[128];
int fail(int code, const char *fmt, const char *detail) { snprintf(g_err, sizeof(g_err), fmt, detail); return code; }

#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  // slot_first: a permutation of 0 .. G-1; the blocks of one residue b & 7 in increasing b take consecutive values,
  // the residue classes laid out in order
  for (int G = 1; G <= 600; ++G) {
    std::vector<int> seen(G, 0);
    int next = 0;
    for (int r = 0; r < 8; ++r)
      for (int b = r; b < G; b += 8) {
        const int t = slot_first(b, G);
        CHECK(t == next && t >= 0 && t < G && !seen[t]);
        seen[t] = 1;
        ++next;
      }
    CHECK(next == G);
  }
  // slot plan against the closed forms
  for (int cap : {1, 7, 512})
    for (size_t per : {(size_t)256, (size_t)4352, (size_t)1 << 33})
      for (int64_t P : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)cap, (int64_t)cap + 1, (int64_t)1 << 40}) {
        const int64_t full = P < 1 ? 1 : P > cap ? cap : P;
        CHECK(slot_workspace_bytes(P, per, cap) == (size_t)full * per);
        for (size_t ws : {(size_t)0, per - 1, per, 2 * per + 1, 6 * per, per * 10000}) {
          int64_t want = (int64_t)(ws / per);
          if (want > P) want = P;
          if (want > cap) want = cap;
          CHECK(slot_count(P, per, ws, cap) == want);
        }
      }
  // chunk plan against a linear scan, need(n) = a + b n; nothing fits: 1
  for (int64_t top = 1; top <= 40; ++top)
    for (size_t a : {(size_t)0, (size_t)100})
      for (size_t b : {(size_t)1, (size_t)37})
        for (size_t ws = 0; ws <= a + b * 41; ws += 7) {
          auto need = [&](int64_t n) { return a + b * (size_t)n; };
          int64_t want = 1;
          for (int64_t n = 1; n <= top; ++n)
            if (need(n) <= ws) want = n;
          CHECK(folds_per_chunk(top, ws, need) == want);
          if (ws < need(1)) CHECK(folds_per_chunk(top, ws, need) == 1);
        }
  // dtype dispatch: the element type by value, the message for anything else
  auto size = [](auto t) { return (int)sizeof(t); };
  CHECK(by_dtype(CVM_F64, "x", size) == 8 && by_dtype(CVM_F32, "x", size) == 4);
  CHECK(by_dtype(7, "cvm_x_fit", size) == CVM_EINVAL && !strcmp(g_err, "cvm_x_fit: dtype must be CVM_F32 or CVM_F64"));
  printf("fit plan ok\n");
  return 0;
}
