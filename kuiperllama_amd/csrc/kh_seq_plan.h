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

// slots of unequal length: slot s = rows [row0[s], row0[s] + len[s]), slot 0 from row 0 (the batch-1 sequence's rows),
// the others behind it without gaps.  Returns false for what is not such a partition of the cache (fewer than
// KH_SEQ_SLOT_MIN_ROWS rows in a slot, more rows than the cache holds); row0 may be null.
static inline bool kh_seq_slots_var(int cache_len, int n_slots, const int32_t* len, int32_t* row0) {
  if (cache_len <= 0 || n_slots < 1 || n_slots > KH_SEQ_SLOTS_MAX || !len) return false;
  int64_t at = 0;
  for (int s = 0; s < n_slots; ++s) {
    if (len[s] < KH_SEQ_SLOT_MIN_ROWS) return false;
    at += len[s];
  }
  if (at > cache_len) return false;
  at = 0;
  for (int s = 0; s < n_slots; ++s) {
    if (row0) row0[s] = (int32_t)at;
    at += len[s];
  }
  return true;
}

// A slot may read its positions [0, pfx) from the rows of another slot, its parent (kh_model_seq_share); it then owns
// only what follows them: position p >= pfx lives at row0 + (p - pfx), and the slot holds pfx + len positions.
struct KhSeqSlot {
  int32_t row0 = 0, len = 0;  // the rows the slot owns
  int32_t parent = -1;        // the slot whose rows [0, pfx) hold this slot's positions [0, pfx); -1: none
  int32_t pfx = 0;            // shared positions (0: the slot shares nothing)
  int32_t pmax = 0;           // as a parent: the largest pfx one of its dependants holds (rows below are immutable)
};
static inline int kh_seq_capacity(const KhSeqSlot& t) { return t.pfx + t.len; }
// the row of position p >= t.pfx is kh_seq_own_base(t) + p; negative for a sharer near the start of the cache
static inline int kh_seq_own_base(const KhSeqSlot& t) { return t.row0 - t.pfx; }

// The passes of the GEMM prefill into slots (kh_seq_prefill.h; kh_plan_seq_prefill_gemm).  A pass has KH_RG_TILES token
// tiles of 16; a segment of n tokens takes ceil(n / 16) of them.  Segments are walked in call order: one that fits in
// what is left of the pass is placed whole, else its first 16 x free tokens fill the pass (if a tile is free) and the
// rest continues in the next - the split of the batch-1 GEMM prefill's 512-token chunks.
// f(pass, segment, first token offset, count) per placed run; returns the number of passes.
#define KH_RG_TILES 32
template <class F>
static inline int kh_rg_plan(int n_seq, const int32_t* n_tokens, F&& f) {
  int pass = 0, used = 0;  // tiles taken in the current pass
  for (int s = 0; s < n_seq; ++s) {
    int off = 0, left = n_tokens[s];
    while (left > 0) {
      if (used == KH_RG_TILES) {
        ++pass;
        used = 0;
      }
      const int room = 16 * (KH_RG_TILES - used);
      const int n = left <= room ? left : room;
      f(pass, s, off, n);
      used += (n + 15) / 16;
      off += n;
      left -= n;
    }
  }
  return used > 0 ? pass + 1 : pass;
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
