// kh_fsm.h — constrained decoding: a deterministic automaton over token ids, on the host (its checks and its walk) and
// on the device (the mask of a state's row over a logit vector, the transition behind a pick).  gfx950.
//
// Semantics (include/kuiper_hip.h, "Constrained decoding"; tests/constraint_ref.py is the numpy statement of the same):
//   the automaton is in CSR form - row s holds the token ids allowed in state s, ascending and distinct, and the state
//   behind each; at a sampled position every logit whose id is NOT in row s becomes -inf ahead of the processors, the
//   pick and the record, and with pick t the state becomes next(s, t).
//
// Device form (KhFsmDev, one struct in device memory that the captured step tails read through a pointer, so that a new
// automaton of any size needs no graph recapture):
//   mask     [n_states][stride] words, stride = ceil(V / 32): bit v & 31 of word v >> 5 of row s set = v is in row s;
//   row_ptr / tokens / next   the CSR arrays as the caller gave them.
// The state itself is one more device word beside d_pos and d_token - or, for sequences in slots
// (kh_model_seq_set_constraint, kh_seq.h: k_seq_tail_fsm), one word per slot of a table: one automaton serves all slots,
// sequences with different constraints share a union and start at different states, -1 = unconstrained.
//
//   kh_fsm_mask_span    the mask pass of `nthr` threads over one vector: float4 q covers ids 4q .. 4q + 3, which are the
//                       four bits (q & 7) * 4 .. of mask word q >> 3 - eight neighbouring lanes share a word, a wave
//                       reads 8 consecutive words and 1 KiB of consecutive logits.  A float4 whose four bits are set is
//                       neither loaded nor stored; one whose bits are all clear is stored without being loaded.
//   kh_fsm_mask_core    ... by the one 1024-thread workgroup of a step tail; ends with a barrier.
//   kh_fsm_advance_core the transition, found by the whole workgroup: every thread compares a strided share of row s
//                       with the pick.  The ids of a row are distinct, so at most one thread matches and writes the
//                       state word.  (One thread bisecting the row would chain up to 17 dependent global loads - more
//                       than the whole mask pass takes; the row of V ids is 128 compares per thread, all in flight.)
//                       A pick that the row does not hold cannot follow the mask; it leaves the state as it is.
// Plain C++, vector stores, no scratch, no inline assembly, no LDS.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#include "kh_common.h"
#else
#include "../../include/kuiper_hip.h"  // a plain host build (kh_lookup.h's drafter over an automaton): kh_fsm, KH_ERR_*
#endif

#define KH_FSM_THREADS 1024

struct KhFsmDev {
  const uint32_t* mask;    // [n_states][stride]
  const int64_t* row_ptr;  // [n_states + 1]
  const int32_t* tokens;   // [n_edges]
  const int32_t* next;     // [n_edges]
  int32_t n_states;
  int32_t stride;          // mask words per state
};
// what a step tail is given: the descriptor and the state word (both null: no constraint)
struct KhFsmRef {
  const KhFsmDev* desc;
  int32_t* state;
};

// ---- host: the checks of kh_fsm_check and the walk of kh_fsm_walk (no device call)
static inline int kh_fsm_check_host(const kh_fsm* a, int64_t vocab) {
  if (!a || !a->row_ptr || !a->tokens || !a->next || a->n_states <= 0 || vocab <= 0) return KH_ERR_INVALID_ARG;
  if (a->start < 0 || a->start >= a->n_states) return KH_ERR_INVALID_ARG;
  if (a->row_ptr[0] != 0) return KH_ERR_INVALID_ARG;
  for (int32_t s = 0; s < a->n_states; ++s)
    if (a->row_ptr[s + 1] <= a->row_ptr[s]) return KH_ERR_INVALID_ARG;  // decreasing, or a row with no edge
  bool range = false;
  for (int32_t s = 0; s < a->n_states; ++s)
    for (int64_t e = a->row_ptr[s]; e < a->row_ptr[s + 1]; ++e) {
      if (e > a->row_ptr[s] && a->tokens[e] <= a->tokens[e - 1]) return KH_ERR_INVALID_ARG;
      if (a->next[e] < 0 || a->next[e] >= a->n_states) return KH_ERR_INVALID_ARG;
      if (a->tokens[e] < 0 || a->tokens[e] >= vocab) range = true;
    }
  return range ? KH_ERR_RANGE : KH_OK;
}
// the edge of row s on token t, or -1 (host; the row is ascending)
static inline int64_t kh_fsm_edge_host(const kh_fsm* a, int32_t s, int32_t t) {
  int64_t lo = a->row_ptr[s], hi = a->row_ptr[s + 1];
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (a->tokens[mid] < t) lo = mid + 1;
    else hi = mid;
  }
  return lo < a->row_ptr[s + 1] && a->tokens[lo] == t ? lo : -1;
}

// ---- host: which rows a -inf bias list could empty, decided without a device read (kh_model_seq_set_constraint: one
// automaton serves every slot and the device moves a slot's state, so the host knows the state it last SET, not the one
// the slot is in).  A state can only reach states of its weakly connected component - label[s] = the smallest state of
// the component of s -, and a list of at most max_edges ids can only empty a row of at most max_edges edges: `small`
// holds those rows, ascending.  Built once per automaton.
struct KhFsmReach {
  std::vector<int32_t> label;  // [n_states]
  std::vector<int32_t> small;  // states whose row has at most max_edges edges
};
static inline KhFsmReach kh_fsm_reach_host(const kh_fsm* a, int64_t max_edges) {
  KhFsmReach r;
  r.label.resize((size_t)a->n_states);
  std::vector<int32_t>& p = r.label;  // union-find, the smaller root wins: a root is the smallest state of its set
  for (int32_t s = 0; s < a->n_states; ++s) p[s] = s;
  auto root = [&](int32_t s) {
    while (p[s] != s) s = p[s] = p[p[s]];
    return s;
  };
  for (int32_t s = 0; s < a->n_states; ++s) {
    for (int64_t e = a->row_ptr[s]; e < a->row_ptr[s + 1]; ++e) {
      const int32_t x = root(s), y = root(a->next[e]);
      if (x < y) p[y] = x;
      else p[x] = y;
    }
    if (a->row_ptr[s + 1] - a->row_ptr[s] <= max_edges) r.small.push_back(s);
  }
  for (int32_t s = 0; s < a->n_states; ++s) p[s] = root(s);
  return r;
}
// does the ascending list `banned` hold every token of some small row in the component of `state`?
static inline bool kh_fsm_reach_emptied_host(const int64_t* row_ptr, const int32_t* tokens, const KhFsmReach& r,
                                             int32_t state, const std::vector<int32_t>& banned) {
  if (banned.empty() || state < 0 || (size_t)state >= r.label.size()) return false;
  for (const int32_t s : r.small) {
    if (r.label[s] != r.label[state] || row_ptr[s + 1] - row_ptr[s] > (int64_t)banned.size()) continue;
    bool all = true;
    for (int64_t e = row_ptr[s]; e < row_ptr[s + 1] && all; ++e)
      all = std::binary_search(banned.begin(), banned.end(), tokens[e]);
    if (all) return true;
  }
  return false;
}

#if defined(__HIPCC__)
// ---- device
// lg[v] = -inf for every v < n whose bit in mrow is clear; thread tid of nthr.  Bits past n are never looked at.
__device__ __forceinline__ void kh_fsm_mask_span(float* lg, int n, const uint32_t* mrow, int tid, int nthr) {
  const float ninf = -INFINITY;
  int done = 0;
  if ((((uintptr_t)lg) & 15u) == 0) {
    const int n4 = n >> 2;
    f32x4* l4 = (f32x4*)lg;
#pragma unroll 4
    for (int q = tid; q < n4; q += nthr) {
      const uint32_t bits = (mrow[q >> 3] >> ((q & 7) * 4)) & 15u;
      if (bits == 15u) continue;
      f32x4 v;
      if (bits == 0u) {
        v.x = v.y = v.z = v.w = ninf;
      } else {
        v = l4[q];
        if (!(bits & 1u)) v.x = ninf;
        if (!(bits & 2u)) v.y = ninf;
        if (!(bits & 4u)) v.z = ninf;
        if (!(bits & 8u)) v.w = ninf;
      }
      l4[q] = v;
    }
    done = 4 * n4;
  }
  for (int64_t i = (int64_t)done + tid; i < n; i += nthr)  // (64-bit: n + nthr may pass 2^31)
    if (!((mrow[i >> 5] >> (i & 31)) & 1u)) lg[i] = ninf;
}
// All KH_FSM_THREADS threads of the workgroup, uniform arguments; ends with a barrier, so every thread may read the
// masked logits afterwards.
__device__ __forceinline__ void kh_fsm_mask_core(float* lg, int n, const uint32_t* mrow) {
  kh_fsm_mask_span(lg, n, mrow, (int)threadIdx.x, KH_FSM_THREADS);
  __syncthreads();
}
// All KH_FSM_THREADS threads, uniform arguments: s is the state the step's mask was made from (read by every thread
// ahead of a barrier, so no thread reads the word behind this write).
__device__ __forceinline__ void kh_fsm_advance_core(const KhFsmDev& d, int s, int pick, int32_t* state) {
  if ((unsigned)s >= (unsigned)d.n_states) return;  // uniform
  const int64_t lo = d.row_ptr[s], hi = d.row_ptr[s + 1];
  int64_t e = lo + (int64_t)threadIdx.x;
  // eight loads in flight per thread, each a contiguous 256 bytes per wave (one load per trip waits out the latency of
  // every one of the 126 trips a row of 128k ids takes)
  for (; e + 7 * KH_FSM_THREADS < hi; e += 8 * KH_FSM_THREADS) {
    int32_t t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = d.tokens[e + k * KH_FSM_THREADS];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (t[k] == pick) *state = d.next[e + k * KH_FSM_THREADS];
  }
  for (; e < hi; e += KH_FSM_THREADS)
    if (d.tokens[e] == pick) *state = d.next[e];
}

// ---- operator (kh_token_mask_f32) and the unfused step's mask: a grid over the vocabulary.  desc non-null: the row of
// state *state of that automaton (nothing where the state is out of range), else `mask` itself.
static __global__ __launch_bounds__(KH_WG) void k_token_mask(float* logits, int n, const uint32_t* mask,
                                                             const KhFsmDev* desc, const int32_t* state) {
  const uint32_t* mrow = mask;
  if (desc) {
    const int s = *state;
    if ((unsigned)s >= (unsigned)desc->n_states) return;
    mrow = desc->mask + (size_t)s * (size_t)desc->stride;
  }
  kh_fsm_mask_span(logits, n, mrow, (int)(blockIdx.x * KH_WG + threadIdx.x), (int)(gridDim.x * KH_WG));
}
// ---- the unfused step's transition behind its pick: one workgroup
static __global__ __launch_bounds__(KH_FSM_THREADS) void k_fsm_advance(const KhFsmDev* desc, int32_t* state,
                                                                       const int32_t* d_pick) {
  const int s = *state;
  const int pick = *d_pick;
  __syncthreads();
  kh_fsm_advance_core(*desc, s, pick, state);
}
#endif
