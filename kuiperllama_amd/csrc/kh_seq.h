// kh_seq.h — one full-depth B-token pass (kh_prefill.h) over lanes that belong to DIFFERENT sequences
// (kh_model_seq_step, kh_model_generate_batch).  The reference decodes one sequence per process; here up to 8 (fp32) or
// 4 (int8, wide fp32) independent sequences share every sweep of the weights.  wo, ffn13, w2 and the classifier do not
// care where a token sits and are the prefill kernels themselves, and the layer loop is the prefill pass's own
// (kh_model_prefill.hip::launch_pf_pass with a lane table); four kernels do:
//   k_seq_embed   k_pf_embed with the lanes' tokens read from a device array (one entry per sequence slot), so that
//                 the picks of one pass feed a later one without a host round trip, whichever lanes share it
//   k_seq_qkv     k_pf_qkv's body (pf_qkv_body) under the lane table's addressing: RoPE row pos[b], cache row row[b]
//   k_seq_attn    kh_attn.h: k_attn_decode's slice body (attn_slice_body) with position and K/V base per lane
//   k_seq_pick    one workgroup per lane: the first maximum of the lane's logits row (kh_samp_row_amax) or, with the
//                 lane's temperature > 0, the sampler core's draw with counter = position and the lane's own seed -
//                 what k_sample / k_sample_topp pick from the same logits
// and, in place of k_seq_pick when a call states penalties, a logit bias or log-probs per sequence
// (kh_model_seq_step_ex, kh_model_generate_batch_ex):
//   k_seq_tail    one workgroup per lane: the step tails' pick chain (kh_logprobs.h: kh_tail_chain) on the lane's row -
//                 the processing core on the slot's parameters and history, the maximum, the greedy or sampled pick,
//                 the record of the lane's cache row
// and, in place of either while the sequence-level constraint is set (kh_model_seq_set_constraint) and a lane of the
// pass sits in a constrained slot:
//   k_seq_tail_fsm  k_seq_tail's twin whose chain is given the automaton (kh_fsm.h) and the slot's word of the state
//                 table: the row of the slot's state masks the lane's logits ahead of the processing core, the word
//                 moves along the pick; a slot at -1 is neither masked nor moved.  A twin, not an argument: k_seq_tail
//                 keeps its code and registers (both: 107 VGPR, 104 SGPR, 57928 B LDS, no scratch)
// gfx950 only.
#pragma once
#include "kh_logprobs.h"
#include "kh_prefill.h"
#include "kh_sample.h"
#include "kh_seq_plan.h"  // KH_SEQ_SLOTS_MAX

// embedding rows of the lanes' tokens -> X[B][dim]; lanes >= nvalid repeat the last valid lane (as k_pf_embed's
// caller pads).  A token outside the vocabulary (the pick of a row without a maximum) copies nothing.
static __global__ __launch_bounds__(KH_WG) void k_seq_embed(const int32_t* __restrict__ tok, const KhSeqLanes lanes,
                                                            int nvalid, int vocab, const float* __restrict__ emb,
                                                            float* __restrict__ X, int dim) {
  const int b = blockIdx.x;
  const int t = tok[lanes.slot[b < nvalid ? b : nvalid - 1]];
  if (t < 0 || t >= vocab) return;
  const f32x4* src = (const f32x4*)(emb + (size_t)t * dim);
  f32x4* dst = (f32x4*)(X + (size_t)b * dim);
  for (int i = threadIdx.x; i < (dim >> 2); i += KH_WG) dst[i] = src[i];
}

// lane addressing of pf_qkv_body: the host fills pos[] of the padding lanes with the last valid lane's
struct KhSeqQkvArgs {
  KhPfQkvArgs a;  // pos0 unused
  KhSeqLanes lanes;
};
struct PfLaneAddr {
  const KhSeqLanes& l;
  __device__ __forceinline__ int pos(int b) const { return l.pos[b]; }
  __device__ __forceinline__ int row(int b) const { return l.row[b]; }
};
template <bool QUANT, int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_seq_qkv(const KhSeqQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_qkv_body<Gemv<QUANT, KH_PF_U(QUANT)>, SPLIT, B>(a.a, PfLaneAddr{a.lanes}, smem_raw);
}

// The tail of a pass.  Workgroup b: the maximum of row b of the logits and its first index (kh_samp_row_amax, as
// k_spec_pick); the sampling parameters of the lane's slot from the device table; the pick;
// tok[slot[b]] = pick (the sequence's next pass reads it in k_seq_embed) and words[row[b]] = pick (may be null), the
// sequence's word of position pos[b] - a sequence's words sit at its slot's rows, like its K/V.
struct KhSeqPickArgs {
  const float* logits;  // [B][vstride]
  int vocab, vstride;
  KhSeqLanes lanes;
  const KhSampParams* params;  // [KH_SEQ_SLOTS_MAX] device table, temperature <= 0: greedy
  int32_t* tok;                // [KH_SEQ_SLOTS_MAX]
  int32_t* words;              // [cache_len] or null
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_seq_pick(const KhSeqPickArgs a) {
  __shared__ KhSampSmem s;
  __shared__ float s_max;
  __shared__ int s_idx;
  const int b = blockIdx.x;
  const float* lg = a.logits + (size_t)b * (size_t)a.vstride;
  float v;
  int idx;
  kh_samp_row_amax(lg, a.vocab, s.red, s.red_i, v, idx);
  if (threadIdx.x == 0) {
    s_max = v;
    s_idx = idx;
  }
  __syncthreads();
  const KhSampParams p = a.params[a.lanes.slot[b]];
  int pick = s_idx;
  if (p.temperature > 0.f) pick = kh_sample_core(s, lg, a.vocab, s_max, p, (uint32_t)a.lanes.pos[b]);  // uniform
  if (threadIdx.x == 0) {
    a.tok[a.lanes.slot[b]] = pick;
    if (a.words) a.words[a.lanes.row[b]] = pick;
  }
}

// The tail of a pass with per-sequence processors or log-probs: steps 1 - 4 are kh_logprobs.h: kh_tail_chain, the one
// chain of k_sample_proc, k_sample_lp and kh_spec.h: k_spec_tail, here one workgroup per lane on per-slot state.
// Workgroup b, slot = slot[b], pos = pos[b], row = row[b]:
//   1. proc[slot] says anything: kh_logit_process_core in place on row b of the logits, over the slot's history -
//      hist is addressed by cache row like K/V, position p of the slot is hist[row - pos + p] - with the slot's bias
//      list and the LANE's counters (lanes run side by side; cnt is zero before and after);
//   2. the first maximum of the processed row; 3. the pick: the sampler core (counter = pos) where the slot's
//   temperature > 0, else that maximum;
//   4. top_n >= 0: the record of cache row `row` - the pick, its log-prob and the top top_n of the logits the pick was
//      made from; entries from top_n on are "none" (kh_rec_none);
//   5. tok[slot] = words[row] = pick, and hist[row + 1] = pick unless pos is the slot's last position (cap[b] = the
//      positions the lane's slot holds; slots differ in length): row + 1 is then a row of the next slot.
// LDS: KhSampSmem + KhLpSmem, as k_sample_lp.  No scratch, plain vector stores.
struct KhSeqTailArgs {
  float* logits;  // [B][vstride], processed in place
  int vocab, vstride;
  KhSeqLanes lanes;
  const KhSampParams* params;  // [KH_SEQ_SLOTS_MAX] device table, temperature <= 0: greedy
  const KhProcParams* proc;    // [KH_SEQ_SLOTS_MAX] device table, neutral: nothing is processed
  const int32_t* bias_ids;     // [KH_SEQ_SLOTS_MAX][KH_SEQ_BIAS_MAX]
  const float* bias;           // [KH_SEQ_SLOTS_MAX][KH_SEQ_BIAS_MAX]
  int32_t* hist;               // [cache_len + 1] token fed at every cache row
  int32_t cap[KH_PF_BMAX];     // positions the lane's slot holds
  int32_t* cnt;                // [KH_PF_BMAX][vocab] counters, zero between launches
  int top_n;                   // -1: no record
  KhTailRecs recs;             // [cache_len]
  int32_t* tok;                // [KH_SEQ_SLOTS_MAX]
  int32_t* words;              // [cache_len] or null
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_seq_tail(const KhSeqTailArgs a) {
  const int b = blockIdx.x;
  const int slot = a.lanes.slot[b], pos = a.lanes.pos[b], row = a.lanes.row[b];
  const KhProcParams pp = a.proc[slot];
  const KhSampParams p = a.params[slot];
  const int pick = kh_tail_chain(a.logits + (size_t)b * (size_t)a.vstride, a.vocab, a.hist + (row - pos), pos, pp,
                                 a.bias_ids + (size_t)slot * KH_SEQ_BIAS_MAX, a.bias + (size_t)slot * KH_SEQ_BIAS_MAX,
                                 a.cnt + (size_t)b * (size_t)a.vocab, p, a.top_n, a.recs, row);
  if (threadIdx.x == 0) {
    a.tok[slot] = pick;
    if (a.words) a.words[row] = pick;
    if (pos + 1 < a.cap[b]) a.hist[row + 1] = pick;
  }
}

// ... and while the sequence-level constraint is set and a lane of the pass sits in a constrained slot
// (kh_model_seq_set_constraint): a twin of k_seq_tail whose chain is given the automaton, so that k_seq_tail keeps its
// code and registers - the rule of k_sample_proc_fsm.  One automaton serves every slot (sequences with different
// constraints share a union, each from its own start state) and state[slot] is the slot's state word: the chain reads
// it ahead of its first barrier, masks row b outside the state's row ahead of step 1 and moves the word along the pick
// behind step 4.  A slot whose word is -1 (any word outside [0, n_states)) is unconstrained: the chain's out-of-range
// path, no mask and no advance.  Lanes sit in distinct slots, so no two workgroups touch one word.
struct KhSeqTailFsmArgs {
  KhFsmRef fsm;  // the descriptor, and the state table [KH_SEQ_SLOTS_MAX]
  KhSeqTailArgs t;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_seq_tail_fsm(const KhSeqTailFsmArgs a) {
  const int b = blockIdx.x;
  const int slot = a.t.lanes.slot[b], pos = a.t.lanes.pos[b], row = a.t.lanes.row[b];
  const KhProcParams pp = a.t.proc[slot];
  const KhSampParams p = a.t.params[slot];
  const int pick =
      kh_tail_chain(a.t.logits + (size_t)b * (size_t)a.t.vstride, a.t.vocab, a.t.hist + (row - pos), pos, pp,
                    a.t.bias_ids + (size_t)slot * KH_SEQ_BIAS_MAX, a.t.bias + (size_t)slot * KH_SEQ_BIAS_MAX,
                    a.t.cnt + (size_t)b * (size_t)a.t.vocab, p, a.t.top_n, a.t.recs, row,
                    KhAmaxParts{nullptr, nullptr, 0}, KhFsmRef{a.fsm.desc, a.fsm.state + slot});
  if (threadIdx.x == 0) {
    a.t.tok[slot] = pick;
    if (a.t.words) a.t.words[row] = pick;
    if (pos + 1 < a.t.cap[b]) a.t.hist[row + 1] = pick;
  }
}
