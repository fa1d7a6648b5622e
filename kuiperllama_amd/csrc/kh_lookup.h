// kh_lookup.h — the drafter of speculative greedy decode (kh_model_generate_lookup, kh_lookup_draft): a guess of the
// next tokens from text that is already there, free of HIP so that a plain host program can exercise it
// (tools/lookup_draft_check.cpp).  Stateless: every call scans; microseconds against a verify pass of milliseconds.
//   seq  = the tokens of the sequence so far, the one to be fed next included (prompt, then words)
//   hint = optional text the caller expects ("predicted output")
//   For g = min(ngram_max, n_seq) down to ngram_min, key = the last g tokens of seq:
//     1. hint: the EARLIEST j with hint[j .. j+g) == key and a follower (j + g < n_hint); draft = hint[j+g ..]
//     2. else seq itself: the MOST RECENT j with j + g <= n_seq - 1 and seq[j .. j+g) == key; draft = seq[j+g ..]
//     3. the draft is cut to cap; the first g that matches wins; no match: 0 tokens
#pragma once
#include <stdint.h>

#include "kh_fsm.h"  // (host part: kh_fsm, kh_fsm_edge_host - the drafter under a constraint, below)

struct KhLookupCfg {
  int ngram_max, ngram_min, miss_steps;
};
// kh_lookup_opts' defaults (0 -> 4 / 1 / 8) and ranges; false: not a configuration.  miss_steps 8: the host round trip
// per miss_steps steps is what text without repeats pays unasked - +2.3-2.5 % at 1, +0.2-0.4 % at 8
static inline bool kh_lookup_resolve(int32_t ngram_max, int32_t ngram_min, int32_t miss_steps, KhLookupCfg* out) {
  if (ngram_max < 0 || ngram_min < 0 || miss_steps < 0 || miss_steps > 8) return false;
  out->ngram_max = ngram_max ? ngram_max : 4;
  out->ngram_min = ngram_min ? ngram_min : 1;
  out->miss_steps = miss_steps ? miss_steps : 8;
  return out->ngram_max >= out->ngram_min;
}

static inline bool kh_lookup_match(const int32_t* a, const int32_t* key, int g) {
  for (int i = 0; i < g; ++i)
    if (a[i] != key[i]) return false;
  return true;
}
static inline int kh_lookup_copy(const int32_t* from, int avail, int32_t* out, int cap) {
  const int n = avail < cap ? avail : cap;
  for (int i = 0; i < n; ++i) out[i] = from[i];
  return n;
}
// ngram_max >= ngram_min >= 1 (resolved); returns the draft length, 0 .. cap
static inline int kh_lookup_draft_core(const int32_t* seq, int n_seq, const int32_t* hint, int n_hint, int ngram_max,
                                       int ngram_min, int32_t* out, int cap) {
  if (cap <= 0 || n_seq <= 0) return 0;
  for (int g = ngram_max < n_seq ? ngram_max : n_seq; g >= ngram_min; --g) {
    const int32_t* key = seq + (n_seq - g);
    for (int j = 0; j + g < n_hint; ++j)
      if (kh_lookup_match(hint + j, key, g)) return kh_lookup_copy(hint + j + g, n_hint - (j + g), out, cap);
    for (int j = n_seq - 1 - g; j >= 0; --j)
      if (kh_lookup_match(seq + j, key, g)) return kh_lookup_copy(seq + j + g, n_seq - (j + g), out, cap);
  }
  return 0;
}

// ---- the drafter under a constraint (kh_model_generate_lookup_fsm, kh_lookup_draft_fsm): the automaton drafts.  From
// `state`, until cap tokens are out or neither rule adds one:
//   (a) while the row of the current state has exactly ONE edge: that token is the pick of every sampler (a raw logit
//       of -inf or NaN aside) - emit it, move along it; *n_forced counts these;
//   (b) otherwise kh_lookup_draft_core on seq + what is out so far, for the remaining room; of its proposal the longest
//       prefix the automaton can follow from the current state is kept and followed; nothing kept: stop.
// Every drafted token is followable, so a verify pass never feeds a token the mask would ban.  The automaton and the
// state are checked by the caller (kh_fsm_check_host; 0 <= state < n_states), the bounds resolved.  `work` holds
// n_seq + cap entries: seq, then the draft (rule (b) searches the text as it would stand).
static inline int kh_lookup_draft_fsm_core(const kh_fsm* a, int32_t state, const int32_t* seq, int n_seq,
                                           const int32_t* hint, int n_hint, int ngram_max, int ngram_min, int32_t* out,
                                           int cap, int32_t* work, int32_t* n_forced) {
  int n = 0, forced = 0;
  for (int i = 0; i < n_seq; ++i) work[i] = seq[i];
  while (n < cap) {
    const int before = n;
    while (n < cap && a->row_ptr[state + 1] - a->row_ptr[state] == 1) {  // (a)
      const int64_t e = a->row_ptr[state];
      out[n] = work[n_seq + n] = a->tokens[e];
      state = a->next[e];
      ++n;
      ++forced;
    }
    if (n < cap) {  // (b)
      const int d = kh_lookup_draft_core(work, n_seq + n, hint, n_hint, ngram_max, ngram_min, out + n, cap - n);
      for (int i = 0; i < d; ++i) {
        const int64_t e = kh_fsm_edge_host(a, state, out[n]);
        if (e < 0) break;
        work[n_seq + n] = out[n];
        state = a->next[e];
        ++n;
      }
    }
    if (n == before) break;
  }
  if (n_forced) *n_forced = forced;
  return n;
}
