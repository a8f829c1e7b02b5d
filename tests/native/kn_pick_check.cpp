// Host check of csrc/kn_pick.h, the dispatcher of the assembly launchers: plain C++17, no HIP.  Prints one line per
// failed property and returns their number (tests/test_kn_pick_host.py builds and runs it, once more under ASan + UBSan).
#include <cstdio>
#include <vector>

#include "../../knp-emi-fenics-x_amd/csrc/kn_pick.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, int a = 0, int b = 0, int c = 0) {
  if (ok) return;
  ++failures;
  std::printf("FAILED: %s (%d, %d, %d)\n", what, a, b, c);
}

// a table with holes, shaped as the row kernels' (lanes, solved ions, membrane path)
constexpr bool built(int L, int KS, int MEM) {
  return (L == 2 || L == 4) ? KS >= 1 && KS <= 3 && MEM >= 0 && MEM <= 2 : (L == 1 || L == 8) && KS == 2 && MEM == 0;
}

// the launcher idiom: nested picks, the innermost body under the predicate; 1: the body ran (once), 0: refused
int launch(int l, int ks, int mem, int* seen) {
  int ran = 0;
  kn_pick<1, 2, 4, 8>(l, [&](auto l_) {
    constexpr int L = decltype(l_)::value;
    kn_pick<1, 2, 3>(ks, [&](auto ks_) {
      constexpr int KS = decltype(ks_)::value;
      kn_pick<0, 1, 2>(mem, [&](auto mem_) {
        constexpr int MEM = decltype(mem_)::value;
        if constexpr (built(L, KS, MEM)) {
          ++ran;
          seen[0] = L, seen[1] = KS, seen[2] = MEM;
        }
      });
    });
  });
  return ran;
}

}  // namespace

int main() {
  // each listed value reaches f with that constant, exactly once; an unlisted one returns false and never calls f
  for (int v = -3; v <= 12; ++v) {
    std::vector<int> got;
    const bool hit = kn_pick<1, 2, 4, 8>(v, [&](auto c) {
      static_assert(std::is_same_v<typename decltype(c)::value_type, int>);
      got.push_back(decltype(c)::value);
    });
    const bool listed = v == 1 || v == 2 || v == 4 || v == 8;
    expect(hit == listed, "return value says whether the value is listed", v);
    expect(listed ? got.size() == 1 && got[0] == v : got.empty(), "f sees the listed value once, an unlisted one never", v);
  }
  // a value listed twice is still one call; an empty list matches nothing; negative values and zero are values like any other
  int calls = 0;
  expect(kn_pick<3, 3, 5>(3, [&](auto) { ++calls; }) && calls == 1, "a value listed twice is picked once");
  expect(!kn_pick<>(0, [&](auto) { ++calls; }) && calls == 1, "an empty list matches nothing");
  expect(kn_pick<-1, 0>(-1, [&](auto c) { calls += decltype(c)::value; }) && calls == 0, "negative constants");
  // the constant is usable where a template argument is needed, and the result of f is not what kn_pick returns
  expect(kn_pick<7>(7, [](auto c) { return std::integral_constant<bool, decltype(c)::value == 8>{}; }), "true whatever f returns");

  // nested picks under a constexpr predicate reach exactly the predicate's set: over the full product of run-time values
  int n_ran = 0, n_built = 0;
  for (int l = 0; l <= 9; ++l)
    for (int ks = 0; ks <= 4; ++ks)
      for (int mem = -1; mem <= 3; ++mem) {
        int seen[3] = {-9, -9, -9};
        const int ran = launch(l, ks, mem, seen);
        const bool want = built(l, ks, mem);
        n_ran += ran;
        n_built += want;
        expect(ran == (want ? 1 : 0), "the body runs once for a built combination and never for another", l, ks, mem);
        if (ran) expect(seen[0] == l && seen[1] == ks && seen[2] == mem, "the body sees the run-time values as constants", l, ks, mem);
      }
  expect(n_ran == n_built && n_built == 20, "20 combinations of the table are built and reached", n_ran, n_built);
  std::printf("kn_pick_check: %d combinations reached, %d failure(s)\n", n_ran, failures);
  return failures;
}
