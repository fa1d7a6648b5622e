// kh_spec.h — the tail of a verify pass of speculative greedy decode (kh_model_verify, kh_model_generate_lookup).
// A full-depth B-token pass (kh_prefill.h) and k_pf_cls leave the logits of up to 8 consecutive positions, bit-identical
// to the token-by-token path.  Two launches turn them into accepted tokens:
//   k_spec_pick    one workgroup per position: the FIRST maximum of its row (kh_sample.h: kh_samp_row_amax).  No
//                  arithmetic enters a maximum, so the pick is k_sample's pick on the same logits.
//   k_spec_accept  one workgroup: how many drafts the picks confirm, the words, the fed-token record and the decode
//                  state of the step that follows - what k_sample leaves behind an advancing step.
// A dependent launch, not a ticket and a last arriver: 1.55 us against a hand-over inside a launch.
// Under the model's settings (kh_model_verify_as_set, kh_model_generate_lookup_as_set: a sampler, penalties, a logit
// bias or log-probs on) three launches take their place:
//   k_spec_hist        the pass's fed tokens into the fed-token record, ahead of the rows that read them
//   k_spec_tail        one workgroup per position: the step tails' pick chain on its row (kh_logprobs.h: kh_tail_chain) - the
//                      processors over the record up to its own position, the maximum, the greedy pick or the seeded
//                      draw with counter = position, the log-prob record.  What a batch-1 step picks on the same logits.
//   k_spec_accept_set  k_spec_accept's duties on those picks, the record entry the next step's window reads and "none"
//                      (kh_rec_none) over the log-prob records of the rejected positions
// Under the model's constraint (kh_model_verify_fsm, kh_model_generate_lookup_fsm; kh_fsm.h) the three have twins:
//   k_spec_fsm_rows    k_spec_hist's duty, and the automaton state AHEAD of every row: rows[0] = the model's state word,
//                      rows[b] = next(rows[b - 1], fed[b]), -1 from the first fed token its row does not hold.  A draft is
//                      accepted only where it equals the pick, so the only state row b can be accepted in is the walk
//                      of the state word over fed[1 .. b] - known before the pass.
//   k_spec_tail_fsm    k_spec_tail with the chain given the automaton and rows[b]: mask ahead of the processors, the
//                      transition behind the pick - rows[b] then holds the state BEHIND row b's pick.  A row at -1
//                      cannot be accepted: it leaves at once with pick -1.
//   k_spec_accept_fsm  k_spec_accept_set, and the model's state word = rows[a]: behind the last owned pick, where a
//                      batch-1 step leaves it.
// The accept gathers the next token's embedding row with the step tails' kh_embed_gather (kh_step_tail.h).
// gfx950 only.
#pragma once
#include "kh_logprobs.h"  // kh_tail_chain, KhTailRecs, kh_rec_none
#include "kh_sample.h"    // KH_SAMP_THREADS, kh_samp_row_amax

// pick[b] = first maximum of logits[b * stride .. + n), b = blockIdx.x (kh_samp_row_amax).  A row without a maximum
// (every entry NaN) leaves 0x7fffffff, as k_sample does.
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_spec_pick(const float* logits, int n, long long stride,
                                                                      int32_t* pick) {
  __shared__ float sv[KH_SAMP_THREADS / KH_WAVE];
  __shared__ int si[KH_SAMP_THREADS / KH_WAVE];
  float v;
  int idx;
  kh_samp_row_amax(logits + (size_t)blockIdx.x * (size_t)stride, n, sv, si, v, idx);
  if (threadIdx.x == 0) pick[blockIdx.x] = idx;
}

// The pass fed fed[0 .. n) at positions pos0 .. pos0 + n - 1: fed[0] was known, fed[1 .. n) are drafts.  pick[i] is the
// greedy token behind fed[0 .. i].  a = the largest value in [0, n - 1] with pick[i] == fed[i + 1] for all i < a: the
// caller owns pick[0 .. a].
struct KhSpecAcceptArgs {
  int32_t* res;            // [1 + KH_PF_BMAX]: res[1 + i] = pick[i] (k_spec_pick); res[0] = a, written here
  int32_t fed[KH_PF_BMAX];
  int pos0, n;
  int32_t* words;          // [words_cap] words[pos0 + i] = pick[i], i <= a (may be null)
  int words_cap;
  int32_t* hist;           // [hist_cap] the token fed at every position: fed[i] up to pos0 + a, -1 behind (rejected)
  int hist_cap;
  int32_t *d_next, *d_token, *d_pos;
  const float* tok_emb;    // [vocab, dim]
  float* x;                // residual stream: receives the embedding row of pick[a]
  int dim, vocab;
};
// returns a in thread 0 (every other thread: 0); the embedding gather is the whole workgroup's
static __device__ __forceinline__ int kh_spec_accept_body(const KhSpecAcceptArgs& t) {
  __shared__ int s_next;
  int a = 0;
  if (threadIdx.x == 0) {
    const int n = t.n < KH_PF_BMAX ? t.n : KH_PF_BMAX;
    const int32_t* pick = t.res + 1;
    while (a < n - 1 && pick[a] == t.fed[a + 1]) ++a;
    t.res[0] = a;
    for (int i = 0; i < n; ++i) {
      const int pos = t.pos0 + i;
      if (i <= a && t.words && pos < t.words_cap) t.words[pos] = pick[i];
      if (pos < t.hist_cap) t.hist[pos] = i <= a ? t.fed[i] : -1;
    }
    const int nxt = pick[a];
    *t.d_next = nxt;
    *t.d_token = nxt;
    *t.d_pos = t.pos0 + a + 1;
    s_next = nxt;
  }
  __syncthreads();
  kh_embed_gather(t.tok_emb, t.x, t.dim, t.vocab, s_next, KH_WG);
  return a;
}
static __global__ __launch_bounds__(KH_WG) void k_spec_accept(const KhSpecAcceptArgs t) { kh_spec_accept_body(t); }

// ---- the same pass under the model's settings ------------------------------------------------------------------------
// hist[pos0 + i] = fed[i], i < n: every row of k_spec_tail reads the record up to its own position, and one workgroup
// cannot wait for another, so the entries are there before that launch
static __global__ __launch_bounds__(KH_WAVE) void k_spec_hist(const KhSpecAcceptArgs t) {
  const int i = threadIdx.x, pos = t.pos0 + i;
  if (i < t.n && i < KH_PF_BMAX && pos >= 0 && pos < t.hist_cap) t.hist[pos] = t.fed[i];
}

// Workgroup b: kh_tail_chain on row b of the pass's logits, in place, as the batch-1 step at position pos0 + b runs it
// on its own logits - history = the fed-token record (k_spec_hist wrote this pass's entries), counter = pos0 + b,
// counters cnt[b][vocab] (rows run side by side; zero before and after), record = position pos0 + b.  The parameters
// are the model's device copies (a null pointer: that setting was never made - neutral / greedy / no record).
struct KhSpecTailArgs {
  float* logits;               // [n][vstride], processed in place
  int vocab, vstride;
  int pos0;
  const KhSampParams* params;  // kh_model_set_sampling's device copy, or null
  const KhProcParams* proc;    // kh_model_set_penalties / _logit_bias's device copy, or null
  const int32_t* bias_ids;
  const float* bias;
  const int32_t* hist;         // [hist_cap >= pos0 + n]
  int32_t* cnt;                // [KH_PF_BMAX][vocab] (null while proc is)
  const int32_t* top_n;        // kh_model_set_logprobs's device word, or null while log-probs are off
  KhTailRecs recs;             // [rec_cap >= pos0 + n]
  int32_t* res;                // res[1 + b] = pick
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_spec_tail(const KhSpecTailArgs a) {
  const int b = blockIdx.x;
  if (b >= KH_PF_BMAX) return;  // uniform
  const int pos = a.pos0 + b;
  const KhProcParams pp = a.proc ? *a.proc : KhProcParams{1.f, 0.f, 0.f, 0, 0};
  const KhSampParams p = a.params ? *a.params : KhSampParams{};
  const int top_n = a.top_n ? max(*a.top_n, 0) : -1;
  const int pick = kh_tail_chain(a.logits + (size_t)b * (size_t)a.vstride, a.vocab, a.hist, pos, pp, a.bias_ids, a.bias,
                                 a.cnt + (size_t)b * (size_t)a.vocab, p, top_n, a.recs, pos);
  if (threadIdx.x == 0) a.res[1 + b] = pick;
}

// k_spec_accept, then what a batch-1 step leaves besides: hist[pos0 + a + 1] = pick[a] (the token the next step feeds;
// its penalty window reads it) and the records of the rejected positions pos0 + a + 1 .. pos0 + n - 1 back to "none"
struct KhSpecAcceptSetArgs {
  KhSpecAcceptArgs t;
  KhTailRecs recs;  // token == null: log-probs are off
  int rec_cap;
};
static __global__ __launch_bounds__(KH_WG) void k_spec_accept_set(const KhSpecAcceptSetArgs s) {
  __shared__ int s_a;
  const int a0 = kh_spec_accept_body(s.t);
  if (threadIdx.x == 0) {
    const int at = s.t.pos0 + a0 + 1;
    if (at < s.t.hist_cap) s.t.hist[at] = s.t.res[1 + a0];
    s_a = a0;
  }
  __syncthreads();
  if (!s.recs.token) return;  // uniform
  const int n = s.t.n < KH_PF_BMAX ? s.t.n : KH_PF_BMAX;
  for (int i = s_a + 1; i < n; ++i) {
    const int pos = s.t.pos0 + i;
    if (pos >= s.rec_cap) break;
    kh_rec_none(s.recs, pos, -1);
  }
}

// ---- the same pass under the model's settings AND its constraint (kh_fsm.h) ------------------------------------------
// One workgroup of KH_FSM_THREADS, ahead of the pass: k_spec_hist's entries, then rows[b] = the state ahead of row b.
// Each transition is kh_fsm_advance_core's strided search by the whole workgroup (no thread bisects: a row of V ids is
// 128 compares per thread, all in flight), handed on through one LDS word with barriers between the steps.
static __global__ __launch_bounds__(KH_FSM_THREADS) void k_spec_fsm_rows(const KhSpecAcceptArgs t, const KhFsmDev* desc,
                                                                         const int32_t* state, int32_t* rows) {
  __shared__ int32_t s_cur;
  const int i = threadIdx.x, pos = t.pos0 + i;
  const int n = t.n < KH_PF_BMAX ? t.n : KH_PF_BMAX;
  if (i < n && pos >= 0 && pos < t.hist_cap) t.hist[pos] = t.fed[i];
  if (i == 0) s_cur = *state;
  for (int b = 0; b < KH_PF_BMAX; ++b) {  // uniform
    __syncthreads();
    const int cur = b < n ? s_cur : -1;
    if (i == 0) rows[b] = cur;
    if (b + 1 >= n) continue;
    __syncthreads();  // every thread holds cur: the word may change
    if (i == 0) s_cur = -1;
    __syncthreads();
    kh_fsm_advance_core(*desc, cur, t.fed[b + 1], &s_cur);  // (cur == -1: nothing; no edge: the word stays -1)
  }
}

struct KhSpecTailFsmArgs {
  KhFsmRef fsm;  // the descriptor, and rows [KH_PF_BMAX] (k_spec_fsm_rows)
  KhSpecTailArgs t;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_spec_tail_fsm(const KhSpecTailFsmArgs f) {
  const KhSpecTailArgs& a = f.t;
  const int b = blockIdx.x;
  if (b >= KH_PF_BMAX) return;  // uniform
  int32_t* const word = f.fsm.state + b;
  if (*word < 0) {  // uniform: behind a fed token that cannot be followed
    if (threadIdx.x == 0) a.res[1 + b] = -1;
    return;
  }
  const int pos = a.pos0 + b;
  const KhProcParams pp = a.proc ? *a.proc : KhProcParams{1.f, 0.f, 0.f, 0, 0};
  const KhSampParams p = a.params ? *a.params : KhSampParams{};
  const int top_n = a.top_n ? max(*a.top_n, 0) : -1;
  const int pick = kh_tail_chain(a.logits + (size_t)b * (size_t)a.vstride, a.vocab, a.hist, pos, pp, a.bias_ids, a.bias,
                                 a.cnt + (size_t)b * (size_t)a.vocab, p, top_n, a.recs, pos,
                                 KhAmaxParts{nullptr, nullptr, 0}, KhFsmRef{f.fsm.desc, word});
  if (threadIdx.x == 0) a.res[1 + b] = pick;
}

struct KhSpecAcceptFsmArgs {
  KhSpecAcceptSetArgs s;
  const int32_t* rows;  // [KH_PF_BMAX] behind k_spec_tail_fsm: the state behind every row's pick
  int32_t* state;       // the model's state word
};
static __global__ __launch_bounds__(KH_WG) void k_spec_accept_fsm(const KhSpecAcceptFsmArgs f) {
  const KhSpecAcceptSetArgs& s = f.s;
  __shared__ int s_a;
  const int a0 = kh_spec_accept_body(s.t);
  if (threadIdx.x == 0) {
    const int at = s.t.pos0 + a0 + 1;
    if (at < s.t.hist_cap) s.t.hist[at] = s.t.res[1 + a0];
    *f.state = f.rows[a0];
    s_a = a0;
  }
  __syncthreads();
  if (!s.recs.token) return;  // uniform
  const int n = s.t.n < KH_PF_BMAX ? s.t.n : KH_PF_BMAX;
  for (int i = s_a + 1; i < n; ++i) {
    const int pos = s.t.pos0 + i;
    if (pos >= s.rec_cap) break;
    kh_rec_none(s.recs, pos, -1);
  }
}
