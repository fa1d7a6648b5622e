// kh_logprobs.h — log-probability of a token and the top-N alternatives of a logit vector on the device (gfx950).
//
// Semantics (include/kuiper_hip.h, "Log-probabilities"; tests/logprobs_ref.py is the fp64 statement of the same):
//   m = max l, lse = m + log(sum exp(l_i - m)), lp(i) = l_i - lse (-inf where l_i = -inf); the top-N are the first N
//   tokens of the sampler's order (logit descending, index ascending), 0 <= N <= KH_LOGPROBS_MAX_TOP.
//
// One workgroup of 1024 threads per vector, given l_max, on the sampler's shared memory and machinery (kh_sample.h):
//   pass 1 (global)  every thread sums expf(l - l_max) of its float4 column (thread t owns float4 t, t + 1024, ...: four
//                    fp32 partials of at most ceil(V / 4096) adds each, two adds to join them, then a ten-level tree
//                    over the workgroup) and counts the token on the sampler's first-pass bins of l_max - l (32 per
//                    unit).  The bins up to the one where the running count reaches N hold every token the top-N can
//                    contain: the CANDIDATES.
//   pass 2 (global)  the candidates are compacted into LDS (at most KH_SAMP_CAP of them; more - flat logits, or fewer
//                    than N finite ones - leaves them in global memory and every step below re-reads the logits).
//   then             on the candidates: the sampler's exact radix descent to the order key of the N-th token, its
//                    index descent for the cut among equal logits at the boundary, the gather of the exactly N
//                    survivors into LDS and their ranks (N threads, N comparisons each).
// N = 0 stops after pass 1 and counts nothing.  The order involves no arithmetic, so the ids are exact; the floats
// carry the fp32 roundings of the sum, logf, l_max + log Z and l - lse.
// No scratch, no inline assembly; every result is written with plain C++ stores.
// Also here: kh_tail_chain, the one chain process -> first maximum -> pick -> record, and the two step tails that run it
// between kh_step_tail.h's begin and end (k_sample_proc, k_sample_lp); the rows of kh_seq.h and kh_spec.h run it too.
#pragma once
#include "kh_fsm.h"
#include "kh_sample.h"

#define KH_LOGPROBS_TOP KH_LOGPROBS_MAX_TOP  // (kuiper_hip.h) also the stride of a model's records

struct KhLpSmem {
  float l[KH_LOGPROBS_TOP];
  int32_t i[KH_LOGPROBS_TOP];
  int n;
};

// Called by all 1024 threads of the workgroup with uniform arguments.  id: the token whose log-prob goes to *o_lp
// (outside [0, n): NaN).  Any output pointer may be null; o_top_ids / o_top_lp receive top_n entries.  Inlined into
// each kernel: a call would save the callee's registers in scratch.
__device__ __forceinline__ void kh_logprobs_core(KhSampSmem& s, KhLpSmem& t, const float* logits, int n, float lmax,
                                                 int id, int top_n, float* o_lse, float* o_lp, int32_t* o_top_ids,
                                                 float* o_top_lp) {
  KhSampCtx c;
  c.logits = logits;
  c.n = n;
  c.lmax = lmax;
  c.T = 1.f;
  c.fx_scale = 0.0;  // the descents below count, they weigh nothing
  c.b_end = KH_SAMP_NB - 1;
  c.in_lds = false;
  const bool want_top = top_n > 0 && (o_top_ids || o_top_lp);
  __syncthreads();  // whatever the caller did with s is over
  for (int b = threadIdx.x; b < KH_SAMP_NB; b += KH_SAMP_THREADS) {
    s.cnt[b] = 0;
    s.wsum[b] = 0;
  }
  if (threadIdx.x == 0) {
    s.ncand = 0;
    t.n = 0;
  }
  __syncthreads();
  // ---- pass 1: sum of exp and the candidate histogram
  float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
  {
    KhSampRun run;
    auto one = [&](float l, float& z) __attribute__((always_inline)) {
      const float e = c.expo(l);
      z += expf(e);
      if (want_top) run.add(s.cnt, s.wsum, c.bin_of(e), 0ull);
    };
    int done = 0;
    if ((((uintptr_t)logits) & 15u) == 0) {
      const int n4 = n >> 2;
      const f32x4* l4 = (const f32x4*)logits;
      auto four = [&](const f32x4& v) __attribute__((always_inline)) {
        one(v.x, z0);
        one(v.y, z1);
        one(v.z, z2);
        one(v.w, z3);
      };
      // four loads in flight per thread, each a contiguous kilobyte per wave
      for (int q = threadIdx.x; q < n4; q += 4 * KH_SAMP_THREADS) {
        const int q1 = q + KH_SAMP_THREADS, q2 = q + 2 * KH_SAMP_THREADS, q3 = q + 3 * KH_SAMP_THREADS;
        const f32x4 v0 = l4[q];
        f32x4 v1 = v0, v2 = v0, v3 = v0;
        if (q1 < n4) v1 = l4[q1];
        if (q2 < n4) v2 = l4[q2];
        if (q3 < n4) v3 = l4[q3];
        four(v0);
        if (q1 < n4) four(v1);
        if (q2 < n4) four(v2);
        if (q3 < n4) four(v3);
      }
      done = 4 * n4;
    }
    for (int i = done + threadIdx.x; i < n; i += KH_SAMP_THREADS) one(logits[i], z0);
    run.flush(s.cnt, s.wsum);
  }
  float z = (z0 + z1) + (z2 + z3);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, KH_WAVE);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s.red[wave] = z;
  __syncthreads();
  z = lane < KH_SAMP_THREADS / KH_WAVE ? s.red[lane] : 0.f;
#pragma unroll
  for (int off = KH_SAMP_THREADS / KH_WAVE / 2; off > 0; off >>= 1) z += __shfl_xor(z, off, KH_WAVE);
  z = __shfl(z, 0, KH_WAVE);  // the same sixteen words in the same order in every wave
  const float lse = __fadd_rn(lmax, logf(z));
  if (threadIdx.x == 0) {
    if (o_lse) *o_lse = lse;
    if (o_lp) *o_lp = (unsigned)id < (unsigned)n ? __fsub_rn(logits[id], lse) : __uint_as_float(0x7fc00000u);
  }
  if (!want_top) return;  // uniform

  // ---- the candidate bins, pass 2: compaction
  kh_samp_walk(s, KH_SAMP_NB, false, false, false, (double)top_n, 0, 0);
  __syncthreads();
  c.b_end = s.r_digit >= 0 ? s.r_digit : KH_SAMP_NB - 1;
  const unsigned long long ncand = s.r_digit >= 0 ? s.r_cb + s.cnt[s.r_digit] : (unsigned long long)n;
  __syncthreads();
  if (ncand <= KH_SAMP_CAP) {
    kh_samp_for_global(logits, n, [&](float l, int i) __attribute__((always_inline)) {
      if (c.bin_of(c.expo(l)) <= c.b_end) {
        const int slot = atomicAdd(&s.ncand, 1);
        if (slot < KH_SAMP_CAP) {
          s.cl[slot] = l;
          s.ci[slot] = i;
        }
      }
    });
    c.in_lds = true;
    __syncthreads();
  }
  // ---- the key of the top_n-th token of the order, and the index cut among its equals
  const KhSampDesc dk = kh_samp_descend(
      c, s, [&](float l, int, uint32_t& v) __attribute__((always_inline)) { v = kh_okey(l); return true; }, 32,
      /*desc=*/true, /*by_w=*/false, /*strict=*/false, (double)top_n);
  const uint32_t t_key = dk.value;
  const unsigned long long m_key = (unsigned long long)top_n - dk.c_before;
  int i_cut = 0x7fffffff;
  if (m_key < dk.c_at) {
    const KhSampDesc di = kh_samp_descend(
        c, s,
        [&](float l, int i, uint32_t& v) __attribute__((always_inline)) {
          v = (uint32_t)i;
          return kh_okey(l) == t_key;
        },
        32 - __clz(n), /*desc=*/false, /*by_w=*/false, /*strict=*/false, (double)m_key, /*low8=*/true);
    if (di.found) i_cut = (int)di.value;
  }
  // ---- the survivors, ranked
  kh_samp_for_src(c, s, [&](float l, int i) __attribute__((always_inline)) {
    const uint32_t k = kh_okey(l);
    if (k > t_key || (k == t_key && i <= i_cut)) {
      const int slot = atomicAdd(&t.n, 1);
      if (slot < KH_LOGPROBS_TOP) {
        t.l[slot] = l;
        t.i[slot] = i;
      }
    }
  });
  __syncthreads();
  const int got = min(t.n, min(top_n, KH_LOGPROBS_TOP));
  if ((int)threadIdx.x < got) {
    const float l = t.l[threadIdx.x];
    const int i = t.i[threadIdx.x];
    const uint32_t k = kh_okey(l);
    int rank = 0;
    for (int j = 0; j < got; ++j) {
      const uint32_t kj = kh_okey(t.l[j]);
      rank += kj > k || (kj == k && t.i[j] < i);
    }
    if (o_top_ids) o_top_ids[rank] = i;
    if (o_top_lp) o_top_lp[rank] = __fsub_rn(l, lse);
  }
}

// ---- the pick chain of one row of logits: the batch-1 step's (k_sample_proc, k_sample_lp below) and that of one row of
// a B-token pass (kh_seq.h: k_seq_tail, kh_spec.h: k_spec_tail).  One workgroup of KH_SAMP_THREADS threads per row,
// every argument uniform.
//   1. pp says anything: kh_logit_process_core in place on lg[0 .. vocab) over hist[.. pos] (hist[j] = the token fed at
//      the sequence's position j) with the bias list and cnt[vocab] (zero before and after);
//   2. the first maximum of the row (kh_samp_row_amax) - from `parts`, the maxima a launch left of the RAW row, where
//      there are any and step 1 changed nothing;
//   3. the pick: the sampler core with counter pos where p.temperature > 0, else that maximum;
//   4. top_n >= 0: the record at index `rec` of the record arrays - the pick, its log-prob and the top top_n of the
//      logits the pick was made from (KhTailRecs, kh_step_tail.h); entries from top_n on are "none" (kh_rec_none).
// With a constraint (fsm.desc non-null: the batch-1 tails k_sample_proc_fsm / k_sample_lp_fsm and, on a slot's state word,
// kh_seq.h: k_seq_tail_fsm; the argument is a constant null in every other caller and the inlined chain is the one it was):
//   0. kh_fsm_mask_core: the logits outside the row of the automaton state become -inf, ahead of step 1;
//   5. kh_fsm_advance_core: the state behind the pick.
// Returns the pick in every thread.  LDS: KhSampSmem + KhLpSmem.  Inlined, like the cores.
__device__ __forceinline__ int kh_tail_chain(float* lg, int vocab, const int32_t* hist, int pos, const KhProcParams pp,
                                             const int32_t* bias_ids, const float* bias, int32_t* cnt,
                                             const KhSampParams p, int top_n, const KhTailRecs r, int rec,
                                             KhAmaxParts parts = {nullptr, nullptr, 0},
                                             const KhFsmRef fsm = {nullptr, nullptr}) {
  __shared__ KhSampSmem s;
  __shared__ KhLpSmem t;
  __shared__ float s_max;
  __shared__ int s_idx;
  int fsm_s = -1;
  if (fsm.desc) {  // uniform; every thread reads the state word ahead of the core's barrier, the write is step 5
    fsm_s = *fsm.state;
    if ((unsigned)fsm_s < (unsigned)fsm.desc->n_states)
      kh_fsm_mask_core(lg, vocab, fsm.desc->mask + (size_t)fsm_s * (size_t)fsm.desc->stride);
    parts.val = nullptr;  // the launch's maxima describe the raw row
  }
  if (pp.repetition != 1.f || pp.presence != 0.f || pp.frequency != 0.f || pp.n_bias > 0) {  // uniform
    kh_logit_process_core(lg, vocab, hist, pos, pp, bias_ids, bias, cnt);
    parts.val = nullptr;
  }
  float v;
  int idx;
  kh_samp_row_amax(lg, vocab, s.red, s.red_i, v, idx, parts);
  if (threadIdx.x == 0) {
    s_max = v;
    s_idx = idx;
  }
  __syncthreads();
  const float lmax = s_max;
  int pick = s_idx;
  if (p.temperature > 0.f) pick = kh_sample_core(s, lg, vocab, lmax, p, (uint32_t)pos);  // uniform
  if (top_n >= 0) {
    top_n = min(top_n, min(KH_LOGPROBS_TOP, vocab));
    const size_t r0 = (size_t)rec * KH_LOGPROBS_TOP;
    kh_logprobs_core(s, t, lg, vocab, lmax, pick, top_n, nullptr, r.lp + rec, r.top_ids + r0, r.top_lp + r0);
    if (threadIdx.x == 0) r.token[rec] = pick;
    kh_rec_none(r, rec, top_n);
  }
  if (fsm.desc) kh_fsm_advance_core(*fsm.desc, fsm_s, pick, fsm.state);
  return pick;
}

// ---- operator: one workgroup per row of logits[n_rows][n]
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_logprobs_op(const float* logits, int n, const int32_t* ids,
                                                                         int top_n, float* lse, float* lp,
                                                                         int32_t* top_ids, float* top_lp) {
  __shared__ KhSampSmem s;
  __shared__ KhLpSmem t;
  const size_t row = blockIdx.x;
  const float* lg = logits + row * (size_t)n;
  float m = -INFINITY;
  kh_samp_for_global(lg, n, [&](float l, int) __attribute__((always_inline)) { m = fmaxf(m, l); });
  const float lmax = kh_samp_block_max(s, m);
  kh_logprobs_core(s, t, lg, n, lmax, ids ? ids[row] : -1, top_n, lse ? lse + row : nullptr, lp ? lp + row : nullptr,
                   top_ids ? top_ids + row * (size_t)top_n : nullptr, top_lp ? top_lp + row * (size_t)top_n : nullptr);
}

// ---- the decode step's last launch while penalties or a logit bias are set (kh_logit_proc.h; k_sample_proc) or
// log-probs are on (kh_model_set_logprobs; k_sample_lp): kh_tail_chain on the step's logits between the begin and the end
// of kh_step_tail.h.  Forced steps leave before touching a logit.  Both record the token they feed next in hist[pos + 1]
// (the window of the steps that follow); the parameters are the model's device copies.
//   k_sample_proc  top_n = -1: no record.  k_cls's partials describe the raw logits and the processors are on: no parts.
//   k_sample_lp    the record of position pos < rec_cap with the top *top_n (fixed stride KH_LOGPROBS_TOP); the whole
//                  record of a forced step is "none".  k_cls's partials give the maximum while no processor is on,
//                  which saves the pass over the vocabulary.
struct KhSampleProcArgs {
  float* logits;
  const KhSampParams* params;  // device copy (kh_model_set_sampling; T <= 0 while the model is greedy)
  const KhProcParams* proc;    // device copy (kh_model_set_penalties / kh_model_set_logit_bias)
  const int32_t* bias_ids;
  const float* bias;
  int32_t* hist;               // [hist_cap] token fed at every position
  int hist_cap;
  int32_t* cnt;                // [vocab] counters, zero between launches
  KhStepState st;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_sample_proc(const KhSampleProcArgs a) {
  int pos, forced, pick = -1;
  kh_step_begin(a.st, pos, forced);
  if (forced < 0)
    pick = kh_tail_chain(a.logits, a.st.vocab, a.hist, pos, *a.proc, a.bias_ids, a.bias, a.cnt, *a.params,
                         /*top_n=*/-1, KhTailRecs{nullptr, nullptr, nullptr, nullptr}, 0);
  kh_step_end(a.st, pos, forced, pick, a.hist, a.hist_cap, KH_SAMP_THREADS);
}
struct KhSampleLpArgs {
  float* logits;
  const float* part_val;       // k_cls's per-workgroup maxima of the raw logits
  const int32_t* part_idx;
  int nparts;
  const KhSampParams* params;  // device copy (kh_model_set_sampling; T <= 0 while the model is greedy)
  const KhProcParams* proc;    // device copy (kh_model_set_penalties / kh_model_set_logit_bias; neutral while off)
  const int32_t* bias_ids;
  const float* bias;
  int32_t* hist;               // [hist_cap] token fed at every position
  int hist_cap;
  int32_t* cnt;                // [vocab] counters, zero between launches
  const int32_t* top_n;        // device word (kh_model_set_logprobs)
  KhTailRecs recs;             // [rec_cap]
  int rec_cap;
  KhStepState st;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_sample_lp(const KhSampleLpArgs a) {
  int pos, forced, pick = -1;
  kh_step_begin(a.st, pos, forced);
  const bool rec = pos >= 0 && pos < a.rec_cap;
  if (forced < 0)
    pick = kh_tail_chain(a.logits, a.st.vocab, a.hist, pos, *a.proc, a.bias_ids, a.bias, a.cnt, *a.params,
                         rec ? max(*a.top_n, 0) : -1, a.recs, pos, KhAmaxParts{a.part_val, a.part_idx, a.nparts});
  else if (rec)
    kh_rec_none(a.recs, pos, -1);
  kh_step_end(a.st, pos, forced, pick, a.hist, a.hist_cap, KH_SAMP_THREADS);
}

// ---- ... and while a constraint is set (kh_fsm.h, kh_model_set_constraint): twins of the two tails above whose chain
// masks ahead of the processors and moves the automaton state behind the pick.  Twins, not an argument of the tails
// above: the launches of a model without a constraint keep their code and their registers.  The descriptor and the state
// word are the model's (allocated once): a new automaton needs no recapture.  proc / params / cnt exist (neutral / greedy
// unless set), as for k_sample_lp.
struct KhSampleProcFsmArgs {
  KhFsmRef fsm;
  KhSampleProcArgs t;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_sample_proc_fsm(const KhSampleProcFsmArgs a) {
  int pos, forced, pick = -1;
  kh_step_begin(a.t.st, pos, forced);
  if (forced < 0)
    pick = kh_tail_chain(a.t.logits, a.t.st.vocab, a.t.hist, pos, *a.t.proc, a.t.bias_ids, a.t.bias, a.t.cnt, *a.t.params,
                         /*top_n=*/-1, KhTailRecs{nullptr, nullptr, nullptr, nullptr}, 0, KhAmaxParts{nullptr, nullptr, 0},
                         a.fsm);
  kh_step_end(a.t.st, pos, forced, pick, a.t.hist, a.t.hist_cap, KH_SAMP_THREADS);
}
struct KhSampleLpFsmArgs {
  KhFsmRef fsm;
  KhSampleLpArgs t;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_sample_lp_fsm(const KhSampleLpFsmArgs a) {
  int pos, forced, pick = -1;
  kh_step_begin(a.t.st, pos, forced);
  const bool rec = pos >= 0 && pos < a.t.rec_cap;
  if (forced < 0)
    pick = kh_tail_chain(a.t.logits, a.t.st.vocab, a.t.hist, pos, *a.t.proc, a.t.bias_ids, a.t.bias, a.t.cnt, *a.t.params,
                         rec ? max(*a.t.top_n, 0) : -1, a.t.recs, pos, KhAmaxParts{nullptr, nullptr, 0}, a.fsm);
  else if (rec)
    kh_rec_none(a.t.recs, pos, -1);
  kh_step_end(a.t.st, pos, forced, pick, a.t.hist, a.t.hist_cap, KH_SAMP_THREADS);
}

// ---- sequence scoring (kh_model_score): the records of the fed positions of one B-token pass.  One workgroup per
// valid token; the token at position pos0 + b reads row b of k_pf_cls's logits (kh_prefill.h) - the RAW logits: no
// processor, no sampler - finds its maximum as k_logprobs_op does, and leaves the record of the position: the token
// that FOLLOWED it (target[b]; -1 behind the last token of a call, whose log-prob is then NaN while its top list
// is the next-token distribution), that token's log-prob and the top *top_n.  Entries from *top_n on are "none" (kh_rec_none).
struct KhScoreLpArgs {
  const float* logits;         // [gridDim.x][vstride]
  int vstride, vocab;
  int32_t target[KH_PF_BMAX];
  int pos0;
  const int32_t* top_n;        // device word (kh_model_set_logprobs)
  KhTailRecs recs;             // [rec_cap]
  int rec_cap;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_score_lp(const KhScoreLpArgs a) {
  __shared__ KhSampSmem s;
  __shared__ KhLpSmem t;
  const int b = blockIdx.x;
  const int pos = a.pos0 + b;
  if (b >= KH_PF_BMAX || pos < 0 || pos >= a.rec_cap) return;  // uniform
  const float* lg = a.logits + (size_t)b * a.vstride;
  float m = -INFINITY;
  kh_samp_for_global(lg, a.vocab, [&](float l, int) __attribute__((always_inline)) { m = fmaxf(m, l); });
  const float lmax = kh_samp_block_max(s, m);
  const int id = a.target[b];
  const int top_n = min(max(*a.top_n, 0), min(KH_LOGPROBS_TOP, a.vocab));
  const size_t r0 = (size_t)pos * KH_LOGPROBS_TOP;
  kh_logprobs_core(s, t, lg, a.vocab, lmax, id, top_n, nullptr, a.recs.lp + pos, a.recs.top_ids + r0, a.recs.top_lp + r0);
  if (threadIdx.x == 0) a.recs.token[pos] = id;
  kh_rec_none(a.recs, pos, top_n);
}
