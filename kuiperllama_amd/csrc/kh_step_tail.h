// kh_step_tail.h — what the last launch of a batch-1 decode step leaves behind, written once.  The five tails -
// k_sample (kh_fused.h), k_sample_screen (kh_cls_screen.h), k_sample_topp (kh_sample.h), k_sample_proc and
// k_sample_lp (kh_logprobs.h) - differ in how they come to a pick; the state they read and write, the forced-token
// rule, the commit and the embedding gather of the token fed next are these:
//   KhStepState      the twelve fields, the LAST member of each tail's argument struct (khm::fill_step_tail fills it)
//   kh_step_forced   the token the caller feeds behind `pos` whatever the logits say, or -1
//   kh_step_commit   d_next / words / hist / d_token / d_pos (one thread)
//   kh_embed_gather  the embedding row of the token fed next into the residual stream (the whole workgroup; the verify
//                    pass's accept, kh_spec.h, gathers with it too), on kh_embed_row, the copy itself (k_set_state)
//   kh_step_commit_pick                the rule and the commit of the 256-thread tails, in thread 0 behind the pick
//   kh_step_begin / kh_step_end        the same for the 1024-thread tails: the rule first, broadcast
//   KhTailRecs / kh_rec_none           the log-prob record arrays and their "none" entries
// Plain C++ stores, no scratch.  gfx950 only.
#pragma once
#include "kh_common.h"

struct KhStepState {
  const int32_t* forced;  // [n_forced] token to feed at position i, or -1 => picked
  int n_forced;
  int32_t* words;         // [words_cap] the reference's `words` vector (main.cpp:14,36-41); may be null
  int words_cap;
  int32_t* d_next;        // the pick (-1 while in the prompt, like post_processing)
  int32_t* d_token;       // token fed at the NEXT position
  int32_t* d_pos;
  const float* tok_emb;   // [vocab, dim]
  float* x;               // residual stream: receives the next token's embedding row
  int dim, vocab;
  int advance;            // 1: generate loop (feed next token, ++pos); 0: predict() only
};

// Prompt phase: next = tokens[pos + 1] (main.cpp:36-38) - the token forced behind position pos, or -1 where the step's
// own pick is fed.  A forced step reports -1 (post_processing while is_prompt, llama3.cpp:738).
__device__ __forceinline__ int kh_step_forced(const KhStepState& st, int pos) {
  if (st.forced && pos + 1 < st.n_forced && st.forced[pos + 1] >= 0) return st.forced[pos + 1];
  return -1;
}

// One thread.  hist / hist_cap: the fed-token record of the tails that keep one (kh_logit_proc.h), else null.
__device__ __forceinline__ void kh_step_commit(const KhStepState& st, int pos, int feed, int reported, int32_t* hist,
                                               int hist_cap) {
  *st.d_next = reported;
  if (st.advance) {
    if (st.words && pos < st.words_cap) st.words[pos] = feed;
    if (hist && pos + 1 < hist_cap) hist[pos + 1] = feed;
    *st.d_token = feed;
    *st.d_pos = pos + 1;
  }
}

// One thread, behind a pick that cost nothing to wait for (k_sample, k_sample_screen: thread 0 holds the argmax): the
// forced-token rule, then the commit.  Returns the token whose row the workgroup gathers, -1 where none is fed.
__device__ __forceinline__ int kh_step_commit_pick(const KhStepState& st, int pick) {
  const int pos = *st.d_pos;
  const int forced = kh_step_forced(st, pos);
  int feed = pick, reported = pick;
  if (forced >= 0) {
    feed = forced;
    reported = -1;
  }
  kh_step_commit(st, pos, feed, reported, nullptr, 0);
  return st.advance ? feed : -1;
}

// x[0 .. dim) = row `tok` of tok_emb.  Every thread of a workgroup of `stride` threads, tok uniform and in range.
__device__ __forceinline__ void kh_embed_row(const float* tok_emb, float* x, int dim, int tok, int stride) {
  const f32x4* src = (const f32x4*)(tok_emb + (size_t)tok * dim);
  f32x4* dst = (f32x4*)x;
  for (int i = threadIdx.x; i < (dim >> 2); i += stride) dst[i] = src[i];
}
// The same behind a pick: a token outside the vocabulary (-1: nothing is fed; 0x7fffffff: the pick of a row without a
// maximum) copies nothing.
__device__ __forceinline__ void kh_embed_gather(const float* tok_emb, float* x, int dim, int vocab, int tok, int stride) {
  if (tok >= 0 && tok < vocab) kh_embed_row(tok_emb, x, dim, tok, stride);
}

// The three 1024-thread tails evaluate the rule FIRST and broadcast it, so a forced step reads no logit.  Begin: the
// step's position and the forced token (or -1) in every thread.
__device__ __forceinline__ void kh_step_begin(const KhStepState& st, int& pos, int& forced) {
  __shared__ int s_pos, s_forced;
  if (threadIdx.x == 0) {
    s_pos = *st.d_pos;
    s_forced = kh_step_forced(st, s_pos);
  }
  __syncthreads();
  pos = s_pos;
  forced = s_forced;
}
// End: `pick` (uniform; anything where a token was forced) - thread 0 commits, the workgroup of `stride` threads gathers.
__device__ __forceinline__ void kh_step_end(const KhStepState& st, int pos, int forced, int pick, int32_t* hist,
                                            int hist_cap, int stride) {
  const int feed = forced >= 0 ? forced : pick;
  if (threadIdx.x == 0) kh_step_commit(st, pos, feed, forced >= 0 ? -1 : pick, hist, hist_cap);
  kh_embed_gather(st.tok_emb, st.x, st.dim, st.vocab, st.advance ? feed : -1, stride);
}

// ---- the log-prob records a tail leaves (kh_logprobs.h; the rows of the B-token passes leave them too: kh_seq.h,
// kh_spec.h, k_score_lp).  A record has a fixed stride of KH_LOGPROBS_MAX_TOP top entries.
struct KhTailRecs {
  int32_t* token;    // [rows]
  float* lp;         // [rows]
  int32_t* top_ids;  // [rows][KH_LOGPROBS_MAX_TOP]
  float* top_lp;     // [rows][KH_LOGPROBS_MAX_TOP]
};
// "None" (-1, NaN) over record `rec`: its top entries from `from` on, or with from < 0 the whole record, the token and
// its log-prob too.  Called by a workgroup of at least KH_LOGPROBS_MAX_TOP threads.
__device__ __forceinline__ void kh_rec_none(const KhTailRecs& r, int rec, int from) {
  const float none = __uint_as_float(0xffffffffu);
  if (from < 0 && threadIdx.x == 0) {
    r.token[rec] = -1;
    r.lp[rec] = none;
  }
  if ((int)threadIdx.x >= from && threadIdx.x < KH_LOGPROBS_MAX_TOP) {
    r.top_ids[(size_t)rec * KH_LOGPROBS_MAX_TOP + threadIdx.x] = -1;
    r.top_lp[(size_t)rec * KH_LOGPROBS_MAX_TOP + threadIdx.x] = none;
  }
}
