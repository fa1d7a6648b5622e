// kh_seq_plan.h — host-only bookkeeping of sequence slots (kh_model_seq.hip): the partition of the cache rows and the
// order in which kh_model_generate_batch puts its live sequences into passes.  No device code; the CPU suite reaches
// both through kh_plan_seq_slots / kh_plan_seq_batch.
#pragma once
#include <stdint.h>

#define KH_SEQ_SLOTS_MAX 64    // sequence slots of a model's cache (kh_model_seq_slots), entries of the per-slot tables
#define KH_SEQ_SLOT_MIN_ROWS 8

// slot s = rows [s * slot_len, (s + 1) * slot_len); 0 = not a partition this library makes
static inline int kh_seq_slot_len(int cache_len, int n_slots) {
  if (cache_len <= 0 || n_slots < 1 || n_slots > KH_SEQ_SLOTS_MAX) return 0;
  const int len = cache_len / n_slots;
  return len >= KH_SEQ_SLOT_MIN_ROWS ? len : 0;
}

// The lanes of the next pass.  Sequence s is live while pos[s] < total[s] and it has not been seen to stop.  Rounds
// walk the sequences in slot order; a pass takes the next up to `width` live ones from the cursor on and never wraps
// (a sequence sits in at most one lane of a pass), the cursor goes back to 0 behind the last sequence.  More than
// `width` live sequences thus take several passes per round, and a sequence that leaves makes room at once.  Returns
// the lane count (0: nobody is live) and advances *cursor; the caller advances pos[] of the lanes.
static inline int kh_seq_next_pass(int n_seq, int width, const int32_t* pos, const int32_t* total,
                                   const uint8_t* stopped, int* cursor, int32_t* lanes) {
  for (int attempt = 0; attempt < 2; ++attempt) {
    int n = 0, s = *cursor;
    for (; s < n_seq && n < width; ++s)
      if (pos[s] < total[s] && !(stopped && stopped[s])) lanes[n++] = s;
    *cursor = s >= n_seq ? 0 : s;
    if (n > 0) return n;
    // nothing from the cursor on: a new round (once)
  }
  return 0;
}
