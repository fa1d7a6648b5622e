// seq_plan_check — host-only exercise of the bookkeeping of sequence slots (csrc/kh_seq_plan.h): the partition of the
// cache rows and the lane grouping of kh_model_generate_batch, with sequences that finish and stop at different
// steps.  No GPU, no library: build with a host compiler, optionally under sanitizers, and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I kuiperllama_amd/csrc tools/seq_plan_check.cpp -o seq_plan_check
#include <cstdio>
#include <vector>

#include "kh_seq_plan.h"

int main() {
  long checked = 0;
  for (int cache : {8, 63, 64, 320, 1280, 131072})
    for (int n = -1; n <= 66; ++n) {
      const int len = kh_seq_slot_len(cache, n);
      const bool ok = n >= 1 && n <= KH_SEQ_SLOTS_MAX && cache / n >= KH_SEQ_SLOT_MIN_ROWS;
      if (len != (ok ? cache / n : 0)) return std::printf("cache %d slots %d: slot_len %d\n", cache, n, len), 1;
      if (ok && (long)n * len > cache) return std::printf("cache %d slots %d: slots past the cache\n", cache, n), 1;
      ++checked;
    }
  for (int width : {4, 8})
    for (int n_seq : {1, width, width + 1, 2 * width + 3, KH_SEQ_SLOTS_MAX}) {
      // exactly n_seq / width entries: a read or write past the end is the sanitizer's to catch
      std::vector<int32_t> pos((size_t)n_seq), total((size_t)n_seq), fed((size_t)n_seq, 0), lanes((size_t)width);
      std::vector<uint8_t> stopped((size_t)n_seq, 0);
      for (int s = 0; s < n_seq; ++s) {
        pos[(size_t)s] = (3 * s) % 5;
        total[(size_t)s] = pos[(size_t)s] + (s % 4 == 3 ? 0 : 1 + (7 * s + 2) % 9);  // every fourth: nothing to sample
      }
      const std::vector<int32_t> first = pos;
      int cursor = 0, passes = 0;
      for (int n; (n = kh_seq_next_pass(n_seq, width, pos.data(), total.data(), stopped.data(), &cursor, lanes.data())) > 0;
           ++passes) {
        if (n > width) return std::printf("width %d n_seq %d: a pass of %d lanes\n", width, n_seq, n), 1;
        for (int i = 0; i < n; ++i) {
          const int s = lanes[(size_t)i];
          if (s < 0 || s >= n_seq || (i > 0 && s <= lanes[(size_t)i - 1]) || stopped[(size_t)s] ||
              pos[(size_t)s] >= total[(size_t)s])
            return std::printf("width %d n_seq %d pass %d: lane %d holds sequence %d\n", width, n_seq, passes, i, s), 1;
          pos[(size_t)s] += 1;
          fed[(size_t)s] += 1;
          ++checked;
        }
        if (passes == 5 && n_seq > 2) stopped[2] = 1;  // a stop seen by the host: the sequence leaves here
        if (passes > 100000) return std::printf("width %d n_seq %d: the plan does not end\n", width, n_seq), 1;
      }
      for (int s = 0; s < n_seq; ++s) {
        const int want = total[(size_t)s] - first[(size_t)s];
        if (stopped[(size_t)s] ? fed[(size_t)s] > want : fed[(size_t)s] != want)
          return std::printf("width %d n_seq %d: sequence %d was fed %d times, not %d\n", width, n_seq, s, fed[(size_t)s], want), 1;
      }
    }
  std::printf("seq_plan_check: %ld checks ok\n", checked);
  return 0;
}
