// score_plan_check — host-only exercise of the index arithmetic of sequence scoring (csrc/kh_score_plan.h): the
// target of every token of every chunk, for all lengths and chunk sizes around the chunk boundaries.  No GPU, no
// library: build with a host compiler, optionally under sanitizers, and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I kuiperllama_amd/csrc tools/score_plan_check.cpp -o score_plan_check
#include <cstdio>
#include <vector>

#include "kh_score_plan.h"

int main() {
  long checked = 0;
  for (int B : {2, 4, 8}) {
    for (int n = 1; n <= 4 * B + 3; ++n) {
      std::vector<int32_t> toks((size_t)n);  // exactly n entries: a read past the end is the sanitizer's to catch
      for (int i = 0; i < n; ++i) toks[(size_t)i] = 1000 + i;
      std::vector<int32_t> seen;
      for (int t0 = 0; t0 < n; t0 += B) {
        const int nv = n - t0 < B ? n - t0 : B;
        std::vector<int32_t> target((size_t)nv);  // exactly nv entries
        kh_score_targets(toks.data(), n, t0, nv, target.data());
        seen.insert(seen.end(), target.begin(), target.end());
      }
      if ((int)seen.size() != n) return std::printf("B %d n %d: %zu targets\n", B, n, seen.size()), 1;
      for (int i = 0; i < n; ++i) {
        const int32_t want = i + 1 < n ? 1000 + i + 1 : -1;
        if (seen[(size_t)i] != want) return std::printf("B %d n %d token %d: %d, not %d\n", B, n, i, seen[(size_t)i], want), 1;
        ++checked;
      }
    }
  }
  std::printf("score_plan_check: %ld targets ok\n", checked);
  return 0;
}
