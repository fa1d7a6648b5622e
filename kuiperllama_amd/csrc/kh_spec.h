// kh_spec.h — the tail of a verify pass of speculative greedy decode (kh_model_verify, kh_model_generate_lookup).
// A full-depth B-token pass (kh_prefill.h) and k_pf_cls leave the logits of up to 8 consecutive positions, bit-identical
// to the token-by-token path.  Two launches turn them into accepted tokens:
//   k_spec_pick    one workgroup per position: the FIRST maximum of its row (kh_sample.h: kh_samp_row_amax).  No
//                  arithmetic enters a maximum, so the pick is k_sample's pick on the same logits.
//   k_spec_accept  one workgroup: how many drafts the picks confirm, the words, the fed-token record and the decode
//                  state of the step that follows - what k_sample leaves behind an advancing step.
// A dependent launch, not a ticket and a last arriver: 1.55 us against a hand-over inside a launch.
// gfx950 only.
#pragma once
#include "kh_sample.h"  // KH_SAMP_THREADS, kh_samp_row_amax

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
static __global__ __launch_bounds__(KH_WG) void k_spec_accept(const KhSpecAcceptArgs t) {
  __shared__ int s_next;
  if (threadIdx.x == 0) {
    const int n = t.n < KH_PF_BMAX ? t.n : KH_PF_BMAX;
    const int32_t* pick = t.res + 1;
    int a = 0;
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
  const int nxt = s_next;
  if (nxt >= 0 && nxt < t.vocab) {
    const f32x4* src = (const f32x4*)(t.tok_emb + (size_t)nxt * t.dim);
    f32x4* dst = (f32x4*)t.x;
    for (int i = threadIdx.x; i < (t.dim >> 2); i += KH_WG) dst[i] = src[i];
  }
}
