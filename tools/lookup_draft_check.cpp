// lookup_draft_check — host-only exercise of the drafter of speculative greedy decode (csrc/kh_lookup.h): the named
// cases of tests/test_lookup.py, empty and one-token inputs, and random sequences over small alphabets against a naive
// restatement of the three rules.  Every array holds exactly the entries the call may touch, so a read or write past
// an end is the sanitizer's to catch.  No GPU, no library: build with a host compiler under sanitizers and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I kuiperllama_amd/csrc tools/lookup_draft_check.cpp -o lookup_draft_check
#include <cstdio>
#include <vector>

#include "kh_lookup.h"

using Toks = std::vector<int32_t>;

static Toks run(const Toks& seq, const Toks& hint, int hi, int lo, int cap) {
  Toks out((size_t)cap);  // exactly cap entries
  const int n = kh_lookup_draft_core(seq.empty() ? nullptr : seq.data(), (int)seq.size(), hint.empty() ? nullptr : hint.data(),
                                     (int)hint.size(), hi, lo, out.empty() ? nullptr : out.data(), cap);
  if (n < 0 || n > cap) return std::printf("draft length %d outside [0, %d]\n", n, cap), Toks{-1};
  out.resize((size_t)n);
  return out;
}
// the rules, word for word
static Toks naive(const Toks& seq, const Toks& hint, int hi, int lo, int cap) {
  const int ns = (int)seq.size(), nh = (int)hint.size();
  for (int g = hi < ns ? hi : ns; g >= lo; --g) {
    auto eq = [&](const Toks& a, int j) {
      for (int i = 0; i < g; ++i)
        if (a[(size_t)(j + i)] != seq[(size_t)(ns - g + i)]) return false;
      return true;
    };
    const Toks* src = nullptr;
    int at = -1;
    for (int j = 0; j + g < nh && at < 0; ++j)
      if (eq(hint, j)) src = &hint, at = j + g;
    for (int j = ns - 1 - g; j >= 0 && at < 0; --j)
      if (eq(seq, j)) src = &seq, at = j + g;
    if (at >= 0) {
      Toks d(src->begin() + at, src->end());
      if ((int)d.size() > cap) d.resize((size_t)cap);
      return d;
    }
  }
  return {};
}

int main() {
  long checked = 0;
  auto expect = [&](const Toks& seq, const Toks& hint, int hi, int lo, int cap, const Toks& want) {
    const Toks got = run(seq, hint, hi, lo, cap);
    ++checked;
    if (got == want && naive(seq, hint, hi, lo, cap) == want) return true;
    std::printf("case %ld: %zu tokens drafted, %zu expected\n", checked, got.size(), want.size());
    return false;
  };
  bool ok = true;
  // the named cases of tests/test_lookup.py
  ok &= expect({7, 8}, {1, 7, 8, 9, 4}, 6, 1, 7, {9, 4});
  ok &= expect({7}, {}, 6, 1, 7, {});
  ok &= expect({7, 7}, {}, 6, 1, 7, {7});
  ok &= expect({3, 4, 5}, {}, 4, 4, 7, {});
  ok &= expect({1, 2, 1, 2}, {1, 2, 3}, 4, 1, 0, {});
  ok &= expect({1, 2}, {0, 1, 2}, 4, 2, 7, {});
  ok &= expect({0, 1, 2}, {}, 4, 2, 7, {});
  ok &= expect({1, 2}, {0, 1, 2}, 4, 1, 7, {});
  ok &= expect({1, 2, 5, 1, 2}, {9, 1, 2, 6}, 4, 1, 7, {6});
  ok &= expect({4, 1, 2, 5, 4, 1, 2}, {9, 1, 2, 6}, 3, 1, 7, {5, 4, 1, 2});
  ok &= expect({1, 2}, {1, 2, 3, 1, 2, 4}, 4, 1, 7, {3, 1, 2, 4});
  ok &= expect({1, 2, 3, 1, 2, 4, 1, 2}, {}, 4, 1, 7, {4, 1, 2});
  ok &= expect({1, 2}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, 4, 1, 7, {3, 4, 5, 6, 7, 8, 9});
  ok &= expect({1, 2}, {1, 2, 3}, 4, 1, 7, {3});
  // empty and one-token inputs
  ok &= expect({}, {}, 4, 1, 7, {});
  ok &= expect({}, {1, 2, 3}, 4, 1, 7, {});
  ok &= expect({1}, {}, 4, 1, 7, {});
  ok &= expect({1}, {1}, 4, 1, 7, {});
  ok &= expect({1}, {1, 2}, 4, 1, 1, {2});
  ok &= expect({1}, {2}, 1, 1, 7, {});
  // the defaults of kh_lookup_opts
  KhLookupCfg cfg;
  ok &= kh_lookup_resolve(0, 0, 0, &cfg) && cfg.ngram_max == 4 && cfg.ngram_min == 1 && cfg.miss_steps == 8;
  ok &= kh_lookup_resolve(6, 6, 8, &cfg) && cfg.ngram_max == 6 && cfg.ngram_min == 6 && cfg.miss_steps == 8;
  ok &= !kh_lookup_resolve(2, 3, 1, &cfg) && !kh_lookup_resolve(0, 5, 1, &cfg) && !kh_lookup_resolve(4, 1, 9, &cfg) &&
        !kh_lookup_resolve(-1, 1, 1, &cfg) && !kh_lookup_resolve(4, -1, 1, &cfg) && !kh_lookup_resolve(4, 1, -1, &cfg);
  // random sequences over 3 .. 5 symbols, with and without a hint
  uint32_t x = 12345u;
  auto rnd = [&](uint32_t n) { return (x = x * 1664525u + 1013904223u, (x >> 8) % n); };
  for (int it = 0; it < 4000 && ok; ++it) {
    const uint32_t k = 3 + rnd(3);
    Toks seq(1 + rnd(40)), hint(it % 2 ? 1 + rnd(30) : 0);
    for (auto& t : seq) t = (int32_t)rnd(k);
    for (auto& t : hint) t = (int32_t)rnd(k);
    const int lo = 1 + (int)rnd(3), hi = lo + (int)rnd(5), cap = (int)rnd(9);
    ok &= expect(seq, hint, hi, lo, cap, naive(seq, hint, hi, lo, cap));
  }
  if (!ok) return 1;
  std::printf("lookup_draft_check: %ld drafts ok\n", checked);
  return 0;
}
