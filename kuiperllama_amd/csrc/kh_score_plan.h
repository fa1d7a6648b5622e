// kh_score_plan.h — host-side index arithmetic of sequence scoring (kh_model_score), free of HIP so that a plain
// host program can exercise it (tools/score_plan_check.cpp).
//   The call feeds tokens[0..n) in chunks of B; the chunk at offset t0 holds nv tokens.  The record of the token at
//   offset t0 + b reports the token that FOLLOWED it: tokens[t0 + b + 1] - which lives in the next chunk for the
//   chunk's last token - and -1 behind the last token of the call.
#pragma once
#include <stdint.h>

static inline void kh_score_targets(const int32_t* tokens, int n, int t0, int nv, int32_t* target /*[nv]*/) {
  for (int b = 0; b < nv; ++b) {
    const int64_t nxt = (int64_t)t0 + b + 1;
    target[b] = nxt < n ? tokens[nxt] : -1;
  }
}
