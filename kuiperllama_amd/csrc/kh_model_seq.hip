// kh_model_seq.hip — several independent sequences in one model: sequence slots of the K/V cache, the pass over lanes
// of different sequences as an entry point (kh_model_seq_step) and the batched generate loop on top of it
// (kh_model_generate_batch), and their _ex forms with per-sequence penalties, logit bias and log-probs (the pass then
// ends in k_seq_tail), and their _gemm forms: the same host text over the wide pass of up to KH_SEQ_SLOTS_MAX lanes
// (kh_model_gemm.hip: seq_pass_enqueue_gemm), and the sequence-level constraint (kh_model_seq_set_constraint: one
// automaton, one state word per slot; the passes of a call with a constrained lane end in k_seq_tail_fsm).  Host side only: what is launched lives in kh_model_prefill.hip (seq_prefill_enqueue,
// seq_pass_enqueue; kernels in kh_seq.h, kh_attn.h).  The reference decodes one sequence per process
// (demo/main.cpp:16-50); n samples of a prompt are n runs of that loop there.
// gfx950 only.
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "kh_logit_proc.h"
#include "kh_model_internal.h"
#include "kh_sample.h"
#include "kh_seq_plan.h"

using namespace khm;

static_assert(KH_SEQ_SLOTS_MAX >= KH_PF_BMAX, "a pass never has more lanes than there can be slots");

namespace {
// The slot table (kh_seq_plan.h): slot s owns rows [row0, row0 + len) and, as a sharer, reads its positions [0, pfx)
// from its parent's rows.  cap: the positions it holds; own_base + p: the row of position p >= pfx (the base itself
// may be negative); seq_row: the row of any position.
inline const KhSeqSlot& slot_of(const kh_model* m, int s) { return m->seq_tab[s]; }
inline int cap(const kh_model* m, int s) { return kh_seq_capacity(m->seq_tab[s]); }
inline int own_base(const kh_model* m, int s) { return kh_seq_own_base(m->seq_tab[s]); }
inline int pfx_row0(const kh_model* m, int s) {
  return m->seq_tab[s].pfx > 0 ? m->seq_tab[m->seq_tab[s].parent].row0 : 0;
}
inline int seq_row(const kh_model* m, int s, int p) {
  return p < m->seq_tab[s].pfx ? pfx_row0(m, s) + p : own_base(m, s) + p;
}
// would feeding position p of slot s write a row it may not write: a shared row of a parent, or (a sharer) a row of
// its parent's?
inline bool writes_shared(const kh_model* m, int s, int p) { return p < m->seq_tab[s].pmax || p < m->seq_tab[s].pfx; }
// the rows positions [p0, p1) of slot s touch, read or written: its own up to p1 and its parent's shared ones
int ensure_slot_rows(kh_model* m, int s, int p1) {
  const KhSeqSlot& t = m->seq_tab[s];
  int rc;
  if (t.pfx > 0 && (rc = kv_ensure_rows(m, pfx_row0(m, s), pfx_row0(m, s) + t.pfx)) != KH_OK) return rc;
  return p1 > t.pfx ? kv_ensure_rows(m, t.row0, t.row0 + p1 - t.pfx) : KH_OK;
}
void lane_set(const kh_model* m, KhSeqLanes& l, int i, int s, int p) {
  l.pos[i] = p;
  l.row[i] = own_base(m, s) + p;
  l.slot[i] = s;
  l.pfx_len[i] = m->seq_tab[s].pfx;
  l.pfx_row0[i] = pfx_row0(m, s);
}
void set_layout(kh_model* m, int n, const int32_t* len, const int32_t* row0) {
  m->seq_slots = n;
  for (int s = 0; s < KH_SEQ_SLOTS_MAX; ++s) m->seq_tab[s] = KhSeqSlot{};
  for (int s = 0; s < n; ++s) {
    m->seq_tab[s].row0 = row0[s];
    m->seq_tab[s].len = len[s];
  }
}
// the sequence-level constraint (kh_model_seq_set_constraint): every slot unconstrained again, on the model stream (a
// 32-bit fill: no host word to keep alive)
int seq_fsm_reset(kh_model* m) {
  if (!m->seq_fsm_on) return KH_OK;
  for (int s = 0; s < KH_SEQ_SLOTS_MAX; ++s) m->seq_fsm_state[s] = -1;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(int32_t*)m->seq_fsm.state, -1, KH_SEQ_SLOTS_MAX, m->stream));
  return KH_OK;
}
// does a lane of the call sit in a constrained slot?  By the states the host last set (the device only moves a state
// that is >= 0 to another that is): then the call's passes end in k_seq_tail_fsm
bool seq_fsm_lanes(const kh_model* m, int n, const int32_t* slots) {
  if (!m->seq_fsm_on) return false;
  for (int i = 0; i < n; ++i)
    if (m->seq_fsm_state[slots ? slots[i] : i] >= 0) return true;
  return false;
}
// a plain call on constrained slots runs as the _ex call with these
const kh_seq_opts* seq_neutral_opts(const kh_sampling* samplings, kh_seq_opts* store) {
  *store = kh_seq_opts{samplings, nullptr, nullptr, nullptr, nullptr, -1};
  return store;
}
bool penalties_on_sharer(const kh_model* m, const kh_seq_opts* o, int i, int s) {
  return o && o->penalties && m->seq_tab[s].pfx > 0 && !kh_penalties_neutral(&o->penalties[i]);
}
inline bool is_stop(int32_t t, const int32_t* stop, int n_stop) {
  for (int i = 0; i < n_stop; ++i)
    if (stop[i] == t) return true;
  return false;
}
// what the seq entry points do not cover, as kh_model_generate_lookup: refused, never rerouted
inline bool seq_unsupported(const kh_model* m) { return m->proc_on || m->lp_top_n >= 0 || !full_depth_supported(m); }
// the per-slot tables of a call: token to feed and sampling parameters (NULL / temperature <= 0: greedy), staged in
// pinned memory and uploaded on the model stream
int upload_slot_tables(kh_model* m) {
  KH_CHECK_HIP(hipMemcpyAsync(m->d_seq_tok, m->h_seq_tok_pin, sizeof(int32_t) * KH_SEQ_SLOTS_MAX, hipMemcpyHostToDevice,
                              m->stream));
  KH_CHECK_HIP(hipMemcpyAsync(m->d_seq_samp, m->h_seq_samp_pin, sizeof(KhSampParams) * KH_SEQ_SLOTS_MAX,
                              hipMemcpyHostToDevice, m->stream));
  return KH_OK;
}
void clear_slot_tables(kh_model* m) {
  for (int s = 0; s < KH_SEQ_SLOTS_MAX; ++s) {
    m->h_seq_tok_pin[s] = 0;
    m->h_seq_samp_pin[s] = KhSampParams{0.f, 0, 1.f, 0u, 0u};
  }
}
// What an _ex call asks of the tail of its passes, checked: on = k_seq_tail runs instead of k_seq_pick (a processor
// on at least one sequence, or log-probs); off[i] = where sequence i's bias entries start in the caller's arrays.
struct SeqEx {
  bool on = false;
  int top_n = -1;
  const kh_seq_opts* o = nullptr;
  int32_t off[KH_SEQ_SLOTS_MAX + 1] = {0};
};
// the checks of kh_model_set_penalties / kh_model_set_logit_bias / kh_model_set_logprobs per sequence; no device call
// slot_of_i: the slots of the call's entries (null: entry i is slot i) - a -inf bias may not empty a row that the
// entry's slot could reach under the sequence-level constraint (KhFsmReach)
int seq_ex_parse(const kh_model* m, int n, const kh_seq_opts* o, SeqEx* out, const int32_t* slot_of_i) {
  out->o = o;
  if (!o) return KH_OK;
  const int V = m->cfg.vocab_size;
  if (o->logprobs_top_n < -1 || o->logprobs_top_n > KH_LOGPROBS_MAX_TOP || o->logprobs_top_n > V)
    return KH_ERR_INVALID_ARG;
  out->top_n = o->logprobs_top_n;
  out->on = out->top_n >= 0;
  for (int i = 0; i < n; ++i) {
    if (o->penalties) {
      if (!kh_penalties_valid(&o->penalties[i])) return KH_ERR_INVALID_ARG;
      out->on = out->on || !kh_penalties_neutral(&o->penalties[i]);
    }
    const int nb = o->n_bias ? o->n_bias[i] : 0;
    if (nb < 0 || (nb > 0 && (!o->bias_ids || !o->bias))) return KH_ERR_INVALID_ARG;
    if (nb > KH_SEQ_BIAS_MAX) return KH_ERR_RANGE;
    const int32_t* ids = o->bias_ids + out->off[i];
    const float* bias = o->bias + out->off[i];
    int banned = 0;
    for (int j = 0; j < nb; ++j) {
      if (bias[j] != bias[j] || bias[j] == INFINITY) return KH_ERR_INVALID_ARG;
      banned += bias[j] == -INFINITY;
    }
    for (int j = 0; j < nb; ++j)
      if (ids[j] < 0 || ids[j] >= V) return KH_ERR_RANGE;
    for (int j = 0; j < nb; ++j)
      for (int k = 0; k < j; ++k)
        if (ids[k] == ids[j]) return KH_ERR_INVALID_ARG;
    if (nb > 0 && banned >= V) return KH_ERR_INVALID_ARG;  // nothing left to pick
    const int st = m->seq_fsm_on ? m->seq_fsm_state[slot_of_i ? slot_of_i[i] : i] : -1;
    if (banned > 0 && st >= 0) {
      std::vector<int32_t> b;
      for (int j = 0; j < nb; ++j)
        if (bias[j] == -INFINITY) b.push_back(ids[j]);
      std::sort(b.begin(), b.end());
      if (kh_fsm_reach_emptied_host(m->seq_fsm.h_row_ptr.data(), m->seq_fsm.h_tokens.data(), m->seq_fsm_reach, st, b))
        return KH_ERR_INVALID_ARG;
    }
    out->off[i + 1] = out->off[i] + nb;
    out->on = out->on || nb > 0;
  }
  return KH_OK;
}
// the per-slot processor tables of a call into pinned staging (entry i of the call is slot slot_of(i)), then uploaded
template <class SlotOf>
int upload_proc_tables(kh_model* m, int n, const SeqEx& ex, SlotOf slot_of) {
  for (int s = 0; s < KH_SEQ_SLOTS_MAX; ++s) m->h_seq_proc_pin[s] = KhProcParams{1.f, 0.f, 0.f, 0, 0};
  const kh_seq_opts* o = ex.o;
  for (int i = 0; i < n; ++i) {
    const int s = slot_of(i), nb = ex.off[i + 1] - ex.off[i];
    KhProcParams& pp = m->h_seq_proc_pin[s];
    if (o->penalties) pp = KhProcParams{o->penalties[i].repetition, o->penalties[i].presence, o->penalties[i].frequency,
                                        o->penalties[i].last_n, 0};
    pp.n_bias = nb;
    for (int j = 0; j < nb; ++j) {
      m->h_seq_bias_ids_pin[(size_t)s * KH_SEQ_BIAS_MAX + j] = o->bias_ids[ex.off[i] + j];
      m->h_seq_bias_pin[(size_t)s * KH_SEQ_BIAS_MAX + j] = o->bias[ex.off[i] + j];
    }
  }
  const size_t nb_all = (size_t)KH_SEQ_SLOTS_MAX * KH_SEQ_BIAS_MAX;
  KH_CHECK_HIP(hipMemcpyAsync(m->d_seq_proc, m->h_seq_proc_pin, sizeof(KhProcParams) * KH_SEQ_SLOTS_MAX,
                              hipMemcpyHostToDevice, m->stream));
  KH_CHECK_HIP(hipMemcpyAsync(m->d_seq_bias_ids, m->h_seq_bias_ids_pin, sizeof(int32_t) * nb_all, hipMemcpyHostToDevice,
                              m->stream));
  KH_CHECK_HIP(hipMemcpyAsync(m->d_seq_bias, m->h_seq_bias_pin, sizeof(float) * nb_all, hipMemcpyHostToDevice,
                              m->stream));
  return KH_OK;
}
}  // namespace

extern "C" int kh_plan_seq_slots(int32_t cache_len, int32_t n_slots, int32_t* slot_len_out) {
  const int len = kh_seq_slot_len(cache_len, n_slots);
  if (!len) return KH_ERR_INVALID_ARG;
  if (slot_len_out) *slot_len_out = len;
  return KH_OK;
}

namespace {
int plan_seq_batch(int32_t n_seq, int32_t width, int32_t width_max, const int32_t* first_pos,
                   const int32_t* total_steps, int32_t* out_lanes, int32_t cap_passes, int32_t* n_passes) {
  if (n_seq <= 0 || n_seq > KH_SEQ_SLOTS_MAX || width <= 0 || width > width_max || !first_pos || !total_steps ||
      !n_passes || cap_passes < 0 || (cap_passes > 0 && !out_lanes))
    return KH_ERR_INVALID_ARG;
  for (int s = 0; s < n_seq; ++s)
    if (first_pos[s] < 0 || total_steps[s] <= 0) return KH_ERR_INVALID_ARG;
  int32_t pos[KH_SEQ_SLOTS_MAX], lanes[KH_SEQ_SLOTS_MAX];
  memcpy(pos, first_pos, sizeof(int32_t) * (size_t)n_seq);
  int cursor = 0, passes = 0;
  for (int n; (n = kh_seq_next_pass(n_seq, width, pos, total_steps, nullptr, &cursor, lanes)) > 0; ++passes) {
    for (int i = 0; i < width; ++i) {
      if (passes < cap_passes) out_lanes[(size_t)passes * width + i] = i < n ? lanes[i] : -1;
      if (i < n) pos[lanes[i]] += 1;
    }
  }
  *n_passes = passes;
  return passes <= cap_passes ? KH_OK : KH_ERR_RANGE;
}
}  // namespace
extern "C" int kh_plan_seq_batch(int32_t n_seq, int32_t width, const int32_t* first_pos, const int32_t* total_steps,
                                 int32_t* out_lanes, int32_t cap_passes, int32_t* n_passes) {
  return plan_seq_batch(n_seq, width, KH_PF_BMAX, first_pos, total_steps, out_lanes, cap_passes, n_passes);
}
// ... for the passes of kh_model_generate_batch_gemm: width up to KH_SEQ_SLOTS_MAX
extern "C" int kh_plan_seq_batch_wide(int32_t n_seq, int32_t width, const int32_t* first_pos,
                                      const int32_t* total_steps, int32_t* out_lanes, int32_t cap_passes,
                                      int32_t* n_passes) {
  return plan_seq_batch(n_seq, width, KH_SEQ_SLOTS_MAX, first_pos, total_steps, out_lanes, cap_passes, n_passes);
}

extern "C" int kh_plan_seq_slots_var(int32_t cache_len, int32_t n_slots, const int32_t* h_len, int32_t* row0_out) {
  return kh_seq_slots_var(cache_len, n_slots, h_len, row0_out) ? KH_OK : KH_ERR_INVALID_ARG;
}

extern "C" int kh_model_seq_slots(kh_model* m, int32_t n_slots, int32_t* slot_len_out) {
  if (!m) return KH_ERR_INVALID_ARG;
  const int len = kh_seq_slot_len(m->cfg.cache_len, n_slots);
  if (!len) return KH_ERR_INVALID_ARG;
  int32_t lens[KH_SEQ_SLOTS_MAX], row0[KH_SEQ_SLOTS_MAX];
  for (int s = 0; s < n_slots; ++s) {
    lens[s] = len;
    row0[s] = s * len;
  }
  set_layout(m, n_slots, lens, row0);
  if (slot_len_out) *slot_len_out = len;
  return seq_fsm_reset(m);
}

extern "C" int kh_model_seq_slots_var(kh_model* m, int32_t n_slots, const int32_t* h_len) {
  if (!m) return KH_ERR_INVALID_ARG;
  int32_t row0[KH_SEQ_SLOTS_MAX];
  if (!kh_seq_slots_var(m->cfg.cache_len, n_slots, h_len, row0)) return KH_ERR_INVALID_ARG;
  set_layout(m, n_slots, h_len, row0);
  return seq_fsm_reset(m);
}

// Bookkeeping only: nothing is copied, nothing is launched.
extern "C" int kh_model_seq_share(kh_model* m, int32_t src_slot, int32_t dst_slot, int32_t n_rows) {
  if (!m || src_slot == dst_slot || n_rows < 0 || dst_slot == 0) return KH_ERR_INVALID_ARG;
  if (src_slot < 0 || src_slot >= m->seq_slots || dst_slot < 0 || dst_slot >= m->seq_slots ||
      n_rows > m->seq_tab[src_slot].len)
    return KH_ERR_RANGE;
  if (n_rows > 0 && m->seq_tab[src_slot].pfx > 0) return KH_ERR_UNSUPPORTED;  // one level only
  for (int s = 0; s < m->seq_slots; ++s)
    if (m->seq_tab[s].pfx > 0 && m->seq_tab[s].parent == dst_slot) return KH_ERR_UNSUPPORTED;  // dst has dependants
  KhSeqSlot& d = m->seq_tab[dst_slot];
  d.parent = n_rows > 0 ? src_slot : -1;
  d.pfx = n_rows;
  for (int s = 0; s < m->seq_slots; ++s) m->seq_tab[s].pmax = 0;
  for (int s = 0; s < m->seq_slots; ++s) {
    const KhSeqSlot& t = m->seq_tab[s];
    if (t.pfx > 0 && t.pfx > m->seq_tab[t.parent].pmax) m->seq_tab[t.parent].pmax = t.pfx;
  }
  return KH_OK;
}

extern "C" int kh_model_seq_row(const kh_model* m, int32_t slot, int32_t pos, int32_t* row) {
  if (!m || !row) return KH_ERR_INVALID_ARG;
  if (slot < 0 || slot >= m->seq_slots || pos < 0 || pos >= cap(m, slot)) return KH_ERR_RANGE;
  *row = seq_row(m, slot, pos);
  return KH_OK;
}

extern "C" int kh_model_seq_width(const kh_model* m, int32_t* width) {
  if (!m || !width) return KH_ERR_INVALID_ARG;
  if (!full_depth_supported(m)) return KH_ERR_UNSUPPORTED;
  *width = verify_width(m);
  return KH_OK;
}

extern "C" int kh_model_seq_width_gemm(const kh_model* m, int32_t* width) {
  if (!m || !width) return KH_ERR_INVALID_ARG;
  if (!seq_gemm_supported(m)) return KH_ERR_UNSUPPORTED;
  *width = KH_SEQ_SLOTS_MAX;
  return KH_OK;
}

extern "C" int kh_model_seq_prefill(kh_model* m, int32_t slot, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  if (!m || !h_tokens || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  if (slot < 0 || slot >= m->seq_slots || (int64_t)pos0 + n > cap(m, slot)) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  if (writes_shared(m, slot, pos0)) return KH_ERR_INVALID_ARG;  // a sharer below its shared length, a parent's shared rows
  if (m->fsm_on || !prefill_supported(m)) return KH_ERR_UNSUPPORTED;  // (a constraint: the slots are not for it)
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  const int row0 = own_base(m, slot);
  if ((rc = ensure_slot_rows(m, slot, pos0 + n)) != KH_OK) return rc;
  if ((rc = seq_prepare(m)) != KH_OK) return rc;
  if ((rc = seq_prefill_enqueue(m, row0, h_tokens, n, pos0, slot_of(m, slot).pfx, pfx_row0(m, slot))) != KH_OK)
    return rc;
  return hist_write(m, h_tokens, n, row0 + pos0);  // the slot's fed-token record, as kh_model_prefill from row 0
}

// Host only: the runs kh_model_seq_prefill_gemm's passes are made of (kh_seq_plan.h: kh_rg_plan)
extern "C" int kh_plan_seq_prefill_gemm(int32_t n_seq, const int32_t* n_tokens, int32_t* out_runs, int32_t cap_runs,
                                        int32_t* n_runs, int32_t* n_passes) {
  if (n_seq <= 0 || !n_tokens || !n_runs || cap_runs < 0 || (cap_runs > 0 && !out_runs)) return KH_ERR_INVALID_ARG;
  for (int s = 0; s < n_seq; ++s)
    if (n_tokens[s] <= 0) return KH_ERR_INVALID_ARG;
  int runs = 0;
  const int passes = kh_rg_plan(n_seq, n_tokens, [&](int pass, int s, int off, int n) {
    if (runs < cap_runs) {
      int32_t* r = out_runs + (size_t)4 * runs;
      r[0] = pass; r[1] = s; r[2] = off; r[3] = n;
    }
    ++runs;
  });
  *n_runs = runs;
  if (n_passes) *n_passes = passes;
  return runs <= cap_runs ? KH_OK : KH_ERR_RANGE;
}

// The GEMM prefill into slots (kh_seq_prefill.h).  Every check before the first launch.
extern "C" int kh_model_seq_prefill_gemm(kh_model* m, int32_t n_seq, const int32_t* slots, const int32_t* h_tokens,
                                         const int32_t* n_tokens, const int32_t* pos0) {
  if (!m || !slots || !h_tokens || !n_tokens || !pos0 || n_seq <= 0) return KH_ERR_INVALID_ARG;
  if (n_seq > KH_SEQ_SLOTS_MAX) return KH_ERR_RANGE;
  size_t total = 0;
  for (int i = 0; i < n_seq; ++i) {
    if (n_tokens[i] <= 0 || pos0[i] < 0) return KH_ERR_INVALID_ARG;
    if (slots[i] < 0 || slots[i] >= m->seq_slots || (int64_t)pos0[i] + n_tokens[i] > cap(m, slots[i])) return KH_ERR_RANGE;
    total += (size_t)n_tokens[i];
  }
  if (!tokens_in_vocab(m, h_tokens, total)) return KH_ERR_RANGE;
  for (int i = 0; i < n_seq; ++i) {
    // a sharer below its shared length, a parent's shared rows
    if (writes_shared(m, slots[i], pos0[i])) return KH_ERR_INVALID_ARG;
    for (int j = 0; j < n_seq; ++j) {
      if (j < i && slots[j] == slots[i]) return KH_ERR_INVALID_ARG;  // two segments of one slot cannot share a call
      // a sharer with its parent: the parent is fed by an earlier call
      if (slot_of(m, slots[i]).pfx > 0 && slot_of(m, slots[i]).parent == slots[j]) return KH_ERR_INVALID_ARG;
    }
  }
  int rc;
  if (m->fsm_on) return KH_ERR_UNSUPPORTED;
  if ((rc = seq_prefill_gemm_check(m)) != KH_OK) return rc;
  return kh_api_guard([&]() -> int {
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    for (int i = 0; i < n_seq; ++i)
      if ((rc = ensure_slot_rows(m, slots[i], pos0[i] + n_tokens[i])) != KH_OK) return rc;
    rc = seq_prefill_gemm_enqueue(m, n_seq, slots, h_tokens, n_tokens, pos0);
    // every segment's fed tokens at its slot's rows of the history, as kh_model_seq_prefill's hist_write; pageable
    // source: the sync keeps the caller's array alive for the uploads (and drains the passes on every way out)
    const int32_t* seg = h_tokens;
    for (int i = 0; i < n_seq && rc == KH_OK; ++i) {
      const int64_t at = (int64_t)own_base(m, slots[i]) + pos0[i];
      if (at < 0 || at + n_tokens[i] > m->hist_cap)
        rc = KH_ERR_RANGE;
      else
        rc = (int)hipMemcpyAsync(m->d_hist + at, seg, sizeof(int32_t) * (size_t)n_tokens[i], hipMemcpyHostToDevice,
                                 m->stream);
      seg += n_tokens[i];
    }
    const hipError_t e = hipStreamSynchronize(m->stream);
    if (rc != KH_OK) return rc;
    return e == hipSuccess ? KH_OK : (int)e;
  });
}

extern "C" int kh_model_seq_fork(kh_model* m, int32_t src_slot, int32_t dst_slot, int32_t n_rows) {
  if (!m || n_rows <= 0 || src_slot == dst_slot) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if (src_slot < 0 || src_slot >= m->seq_slots || dst_slot < 0 || dst_slot >= m->seq_slots ||
      n_rows > slot_of(m, src_slot).len || n_rows > slot_of(m, dst_slot).len)
    return KH_ERR_RANGE;
  if (m->fsm_on) return KH_ERR_UNSUPPORTED;
  if (slot_of(m, src_slot).pfx > 0 || slot_of(m, dst_slot).pfx > 0) return KH_ERR_UNSUPPORTED;  // a sharer's rows are not one run
  if (slot_of(m, dst_slot).pmax > 0) return KH_ERR_INVALID_ARG;  // a parent's shared rows are immutable
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  const size_t srow = (size_t)slot_of(m, src_slot).row0, drow = (size_t)slot_of(m, dst_slot).row0;
  if ((rc = kv_ensure_rows(m, (int)srow, (int)srow + n_rows)) != KH_OK) return rc;
  if ((rc = kv_ensure_rows(m, (int)drow, (int)drow + n_rows)) != KH_OK) return rc;
  const size_t nb = (size_t)n_rows * c.kv_dim * sizeof(float);
  for (int l = 0; l < c.layer_num; ++l) {
    const size_t so = ((size_t)l * c.cache_len + srow) * c.kv_dim;
    const size_t dof = ((size_t)l * c.cache_len + drow) * c.kv_dim;
    KH_CHECK_HIP(hipMemcpyAsync(m->kcache + dof, m->kcache + so, nb, hipMemcpyDeviceToDevice, m->stream));
    KH_CHECK_HIP(hipMemcpyAsync(m->vcache + dof, m->vcache + so, nb, hipMemcpyDeviceToDevice, m->stream));
  }
  KH_CHECK_HIP(hipMemcpyAsync(m->d_hist + drow, m->d_hist + srow,
                              sizeof(int32_t) * (size_t)n_rows, hipMemcpyDeviceToDevice, m->stream));
  if (m->seq_fsm_on) {  // the fork continues under the source's constraint, from the state the source is in
    KH_CHECK_HIP(hipMemcpyAsync(m->seq_fsm.state + dst_slot, m->seq_fsm.state + src_slot, sizeof(int32_t),
                                hipMemcpyDeviceToDevice, m->stream));
    m->seq_fsm_state[dst_slot] = m->seq_fsm_state[src_slot];
  }
  return KH_OK;
}

// One pass.  Eager launches on the model stream; every check before the first of them.  o: the _ex call's options
// (its samplings are `samplings` here), which replace the model's own settings - those refuse the plain call.
// wide: the pass is the wide one (kh_seq_gemm.h: up to KH_SEQ_SLOTS_MAX lanes, seq_pass_enqueue_gemm); an _ex call.
namespace {
int seq_step_run(kh_model* m, int32_t n, const int32_t* slots, const int32_t* h_tokens, const int32_t* pos,
                 const kh_sampling* samplings, const kh_seq_opts* o, bool ex_call, int32_t* h_next, bool wide = false) {
  if (!m || !slots || !h_tokens || !pos || !h_next || n <= 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if (m->fsm_on || (wide ? !seq_gemm_supported(m) : (ex_call ? !full_depth_supported(m) : seq_unsupported(m))))
    return KH_ERR_UNSUPPORTED;  // (a constraint: one automaton state, no lane has its own)
  if (n > (wide ? KH_SEQ_SLOTS_MAX : verify_width(m))) return KH_ERR_RANGE;
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= m->seq_slots || pos[i] < 0 || pos[i] >= cap(m, slots[i]) || h_tokens[i] < 0 ||
        h_tokens[i] >= c.vocab_size)
      return KH_ERR_RANGE;
    for (int j = 0; j < i; ++j)
      if (slots[j] == slots[i]) return KH_ERR_INVALID_ARG;  // two lanes of one sequence cannot share a pass
    if (samplings && !kh_sampling_valid(&samplings[i])) return KH_ERR_INVALID_ARG;
  }
  const bool fsm = seq_fsm_lanes(m, n, slots);
  kh_seq_opts neutral;
  if (fsm && !o) o = seq_neutral_opts(samplings, &neutral);
  SeqEx ex;
  int rc;
  if ((rc = seq_ex_parse(m, n, o, &ex, slots)) != KH_OK) return rc;
  ex.on = ex.on || fsm;
  for (int i = 0; i < n; ++i) {
    if (writes_shared(m, slots[i], pos[i])) return KH_ERR_INVALID_ARG;
    if (penalties_on_sharer(m, o, i, slots[i])) return KH_ERR_UNSUPPORTED;  // its history lies in two row ranges
  }
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  for (int i = 0; i < n; ++i)
    if ((rc = ensure_slot_rows(m, slots[i], pos[i] + 1)) != KH_OK) return rc;
  if ((rc = seq_prepare(m)) != KH_OK) return rc;
  if (ex.on && (rc = seq_prepare_ex(m, ex.top_n >= 0)) != KH_OK) return rc;
  if (wide && (rc = seq_gemm_prepare(m)) != KH_OK) return rc;
  clear_slot_tables(m);
  KhSeqLanes lanes;
  for (int i = 0; i < n; ++i) {
    if (!wide) lane_set(m, lanes, i, slots[i], pos[i]);
    m->h_seq_tok_pin[slots[i]] = h_tokens[i];
    if (samplings && !kh_sampling_greedy(&samplings[i])) m->h_seq_samp_pin[slots[i]] = kh_samp_params(&samplings[i]);
  }
  rc = upload_slot_tables(m);
  const KhSeqTail tail{ex.top_n, m->d_seq_proc, m->d_seq_bias_ids, m->d_seq_bias, m->d_seq_cnt,
                       fsm ? KhFsmRef{m->seq_fsm.desc, m->seq_fsm.state} : KhFsmRef{nullptr, nullptr}};
  if (rc == KH_OK && ex.on) {
    rc = upload_proc_tables(m, n, ex, [&](int i) { return slots[i]; });
    for (int i = 0; i < n && rc == KH_OK; ++i) {  // the lanes' fed tokens at their rows of the history
      m->h_seq_hist_pin[i] = h_tokens[i];
      rc = (int)hipMemcpyAsync(m->d_hist + own_base(m, slots[i]) + pos[i], m->h_seq_hist_pin + i, sizeof(int32_t), hipMemcpyHostToDevice,
                               m->stream);
    }
    if (rc == KH_OK && ex.top_n >= 0) m->seq_lp_top_n = ex.top_n;
  }
  if (rc == KH_OK)
    rc = wide ? seq_pass_enqueue_gemm(m, slots, pos, n, /*words=*/false, ex.on ? &tail : nullptr)
              : seq_pass_enqueue(m, lanes, n, /*words=*/false, ex.on ? &tail : nullptr);
  if (rc == KH_OK)
    rc = (int)hipMemcpyAsync(m->h_seq_tok_pin, m->d_seq_tok, sizeof(int32_t) * KH_SEQ_SLOTS_MAX, hipMemcpyDeviceToHost,
                             m->stream);
  const hipError_t e = hipStreamSynchronize(m->stream);  // drained on every way out
  if (rc != KH_OK) return rc;
  if (e != hipSuccess) return (int)e;
  for (int i = 0; i < n; ++i) h_next[i] = m->h_seq_tok_pin[slots[i]];
  return KH_OK;
}
}  // namespace
extern "C" int kh_model_seq_step(kh_model* m, int32_t n, const int32_t* slots, const int32_t* h_tokens,
                                 const int32_t* pos, const kh_sampling* samplings, int32_t* h_next) {
  return seq_step_run(m, n, slots, h_tokens, pos, samplings, nullptr, /*ex_call=*/false, h_next);
}
extern "C" int kh_model_seq_step_ex(kh_model* m, int32_t n, const int32_t* slots, const int32_t* h_tokens,
                                    const int32_t* pos, const kh_seq_opts* o, int32_t* h_next) {
  return seq_step_run(m, n, slots, h_tokens, pos, o ? o->samplings : nullptr, o, /*ex_call=*/true, h_next);
}
extern "C" int kh_model_seq_step_gemm(kh_model* m, int32_t n, const int32_t* slots, const int32_t* h_tokens,
                                      const int32_t* pos, const kh_seq_opts* o, int32_t* h_next) {
  return seq_step_run(m, n, slots, h_tokens, pos, o ? o->samplings : nullptr, o, /*ex_call=*/true, h_next,
                      /*wide=*/true);
}
extern "C" int kh_model_seq_gemm_logits(kh_model* m, int32_t lane, float* h_logits) {
  if (!m || !h_logits) return KH_ERR_INVALID_ARG;
  if (!m->sg_logits || m->sg_lanes == 0) return KH_ERR_UNSUPPORTED;  // no wide pass yet
  if (lane < 0 || lane >= m->sg_lanes) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemcpyAsync(h_logits, m->sg_logits + (size_t)lane * m->pf_vstride,
                              sizeof(float) * (size_t)m->cfg.vocab_size, hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}

// kh_model_generate_until for n_seq sequences at once, sequence s in slot s.  The fed-only part of every prompt runs
// as kh_model_seq_prefill's passes; the sampled part as passes of up to `width` lanes, enqueued eagerly (the picks
// feed the next pass on the device).  With a stop list the words of every 8 passes are mirrored into pinned memory
// behind them and inspected while the next 8 are queued: generate_until's check, with its contract that what ran
// past a stop is discarded.
extern "C" int kh_model_generate_batch(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                                       const int32_t* total_steps, const kh_sampling* samplings, const int32_t* h_stop,
                                       int32_t n_stop, int32_t* h_words, int32_t words_stride, int32_t* n_words,
                                       float* h_elapsed_ms) {
  return kh_model_generate_batch_from(m, n_seq, h_prompts, n_prompt, nullptr, total_steps, samplings, h_stop, n_stop,
                                      h_words, words_stride, n_words, h_elapsed_ms);
}
// ... with the first n_cached[s] positions of sequence s already in its slot's rows (kh_model_seq_prefill,
// kh_model_seq_fork): the call feeds the rest of the prompt
namespace {
int generate_batch_run(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                       const int32_t* n_cached, const int32_t* total_steps, const kh_sampling* samplings,
                       const kh_seq_opts* o, bool ex_call, const int32_t* h_stop, int32_t n_stop, int32_t* h_words,
                       int32_t words_stride, int32_t* n_words, float* h_elapsed_ms, bool wide = false);
}
extern "C" int kh_model_generate_batch_from(kh_model* m, int32_t n_seq, const int32_t* h_prompts,
                                            const int32_t* n_prompt, const int32_t* n_cached,
                                            const int32_t* total_steps, const kh_sampling* samplings,
                                            const int32_t* h_stop, int32_t n_stop, int32_t* h_words,
                                            int32_t words_stride, int32_t* n_words, float* h_elapsed_ms) {
  return generate_batch_run(m, n_seq, h_prompts, n_prompt, n_cached, total_steps, samplings, nullptr, /*ex_call=*/false,
                            h_stop, n_stop, h_words, words_stride, n_words, h_elapsed_ms);
}
// ... with per-sequence options in place of the model's own settings (see seq_step_run)
extern "C" int kh_model_generate_batch_ex(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                                          const int32_t* n_cached, const int32_t* total_steps, const kh_seq_opts* o,
                                          const int32_t* h_stop, int32_t n_stop, int32_t* h_words,
                                          int32_t words_stride, int32_t* n_words, float* h_elapsed_ms) {
  return generate_batch_run(m, n_seq, h_prompts, n_prompt, n_cached, total_steps, o ? o->samplings : nullptr, o,
                            /*ex_call=*/true, h_stop, n_stop, h_words, words_stride, n_words, h_elapsed_ms);
}
// ... with the sampled part as wide passes (kh_seq_gemm.h): the same loop at width KH_SEQ_SLOTS_MAX
extern "C" int kh_model_generate_batch_gemm(kh_model* m, int32_t n_seq, const int32_t* h_prompts,
                                            const int32_t* n_prompt, const int32_t* n_cached,
                                            const int32_t* total_steps, const kh_seq_opts* o, const int32_t* h_stop,
                                            int32_t n_stop, int32_t* h_words, int32_t words_stride, int32_t* n_words,
                                            float* h_elapsed_ms) {
  return generate_batch_run(m, n_seq, h_prompts, n_prompt, n_cached, total_steps, o ? o->samplings : nullptr, o,
                            /*ex_call=*/true, h_stop, n_stop, h_words, words_stride, n_words, h_elapsed_ms,
                            /*wide=*/true);
}
namespace {
int generate_batch_run(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                       const int32_t* n_cached, const int32_t* total_steps, const kh_sampling* samplings,
                       const kh_seq_opts* o, bool ex_call, const int32_t* h_stop, int32_t n_stop, int32_t* h_words,
                       int32_t words_stride, int32_t* n_words, float* h_elapsed_ms, bool wide) {
  if (!m || !h_prompts || !n_prompt || !total_steps || !h_words || !n_words || n_seq <= 0 || words_stride <= 0 ||
      n_stop < 0 || (n_stop > 0 && !h_stop))
    return KH_ERR_INVALID_ARG;
  if (n_seq > m->seq_slots) return KH_ERR_RANGE;
  size_t n_tok = 0;
  for (int s = 0; s < n_seq; ++s) {
    if (n_prompt[s] <= 0 || total_steps[s] <= 0 || total_steps[s] > words_stride) return KH_ERR_INVALID_ARG;
    if (total_steps[s] > cap(m, s)) return KH_ERR_RANGE;
    if (samplings && !kh_sampling_valid(&samplings[s])) return KH_ERR_INVALID_ARG;
    // only fed-only positions can be cached: the last prompt token's logits are the first pick's
    if (n_cached && (n_cached[s] < 0 || n_cached[s] > n_prompt[s] - 1 || n_cached[s] > total_steps[s]))
      return KH_ERR_INVALID_ARG;
    n_tok += (size_t)n_prompt[s];
  }
  if (!tokens_in_vocab(m, h_prompts, n_tok)) return KH_ERR_RANGE;
  if (m->fsm_on || (wide ? !seq_gemm_supported(m) : (ex_call ? !full_depth_supported(m) : seq_unsupported(m))))
    return KH_ERR_UNSUPPORTED;  // (a constraint: one automaton state, no lane has its own)
  const bool fsm = seq_fsm_lanes(m, n_seq, nullptr);
  kh_seq_opts neutral;
  if (fsm && !o) o = seq_neutral_opts(samplings, &neutral);
  SeqEx ex;
  {
    const int rc = seq_ex_parse(m, n_seq, o, &ex, nullptr);
    if (rc != KH_OK) return rc;
    ex.on = ex.on || fsm;
  }
  for (int s = 0; s < n_seq; ++s) {
    // the first position the call feeds: what is cached must cover a sharer's shared length and a parent's shared rows
    if (writes_shared(m, s, n_cached ? n_cached[s] : 0)) return KH_ERR_INVALID_ARG;
    if (penalties_on_sharer(m, o, s, s)) return KH_ERR_UNSUPPORTED;  // its history lies in two row ranges
  }
  return kh_api_guard([&]() -> int {
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    int rc;
    for (int s = 0; s < n_seq; ++s) {
      n_words[s] = 0;
      if ((rc = ensure_slot_rows(m, s, total_steps[s])) != KH_OK) return rc;
    }
    if ((rc = seq_prepare(m)) != KH_OK) return rc;
    if (ex.on && (rc = seq_prepare_ex(m, ex.top_n >= 0)) != KH_OK) return rc;
    if (wide && (rc = seq_gemm_prepare(m)) != KH_OK) return rc;
    const KhSeqTail tail{ex.top_n, m->d_seq_proc, m->d_seq_bias_ids, m->d_seq_bias, m->d_seq_cnt,
                         fsm ? KhFsmRef{m->seq_fsm.desc, m->seq_fsm.state} : KhFsmRef{nullptr, nullptr}};
    // every early return below may leave launches and copies into pinned memory in flight: drain first
    auto fail = [&](int code) -> int {
      (void)hipStreamSynchronize(m->stream);
      return code;
    };
    const int width = wide ? KH_SEQ_SLOTS_MAX : verify_width(m);
    std::vector<const int32_t*> prompt((size_t)n_seq);
    // pos[s]: the next position sequence s feeds in a pass; copied / checked: how far its words were mirrored / read
    std::vector<int32_t> pos((size_t)n_seq), copied((size_t)n_seq), checked((size_t)n_seq), stop_at((size_t)n_seq, -1);
    std::vector<uint8_t> stopped((size_t)n_seq, 0);
    clear_slot_tables(m);
    {
      const int32_t* p = h_prompts;
      for (int s = 0; s < n_seq; ++s) {
        prompt[s] = p;
        p += n_prompt[s];
        const int fed = n_prompt[s] - 1 < total_steps[s] ? n_prompt[s] - 1 : total_steps[s];  // fed-only positions
        pos[s] = copied[s] = checked[s] = fed;
        m->h_seq_tok_pin[s] = prompt[s][fed];  // fed <= n_prompt - 1
        if (samplings && !kh_sampling_greedy(&samplings[s])) m->h_seq_samp_pin[s] = kh_samp_params(&samplings[s]);
      }
    }
    if ((rc = upload_slot_tables(m)) != KH_OK) return fail(rc);
    if (ex.on) {
      if ((rc = upload_proc_tables(m, n_seq, ex, [](int i) { return i; })) != KH_OK) return fail(rc);
      // every sequence's whole prompt at its slot's entries of the history (its cached part too: the prompt is here
      // whoever fed it), staged in pinned memory; the records of its fed-only positions become "none"
      // (a sharer: from its shared length on - the rows below are its parent's, with the parent's history and records)
      for (int s = 0; s < n_seq; ++s) {
        const int np = n_prompt[s] < cap(m, s) ? n_prompt[s] : cap(m, s);
        const int p0 = slot_of(m, s).pfx;
        if (np > p0) {
          const size_t at = (size_t)(own_base(m, s) + p0);
          memcpy(m->h_seq_hist_pin + at, prompt[s] + p0, sizeof(int32_t) * (size_t)(np - p0));
          if (hipMemcpyAsync(m->d_hist + at, m->h_seq_hist_pin + at, sizeof(int32_t) * (size_t)(np - p0),
                             hipMemcpyHostToDevice, m->stream) != hipSuccess)
            return fail((int)hipErrorUnknown);
        }
        if (ex.top_n >= 0 && pos[s] > p0 && (rc = lp_fill_none(m, own_base(m, s) + p0, pos[s] - p0)) != KH_OK)
          return fail(rc);
      }
      if (ex.top_n >= 0) m->seq_lp_top_n = ex.top_n;
    }
    if (hipEventRecord(m->ev0, m->stream) != hipSuccess) return fail((int)hipErrorUnknown);
    for (int s = 0; s < n_seq; ++s) {
      const int have = n_cached ? n_cached[s] : 0;
      if (pos[s] > have && (rc = seq_prefill_enqueue(m, own_base(m, s), prompt[s] + have, pos[s] - have, have,
                                                     slot_of(m, s).pfx, pfx_row0(m, s))) != KH_OK)
        return fail(rc);
    }
    int32_t* const pin = m->h_seq_words_pin;
    struct Chunk {
      std::vector<int32_t> upto;
    };
    Chunk infl[2];
    int n_infl = 0, head = 0, cursor = 0;
    // the words the passes so far have written, into the pinned mirror; an event behind the copies
    auto mirror = [&]() -> int {
      for (int s = 0; s < n_seq; ++s)
        if (pos[s] > copied[s]) {
          const size_t at = (size_t)(own_base(m, s) + copied[s]);  // copied[s] >= the slot's shared length
          if (hipMemcpyAsync(pin + at, m->d_seq_words + at, sizeof(int32_t) * (size_t)(pos[s] - copied[s]),
                             hipMemcpyDeviceToHost, m->stream) != hipSuccess)
            return (int)hipErrorUnknown;
          copied[s] = pos[s];
        }
      const int slot = (head + n_infl) & 1;
      if (hipEventRecord(m->ev_chunk[slot], m->stream) != hipSuccess) return (int)hipErrorUnknown;
      infl[slot].upto = pos;
      ++n_infl;
      return KH_OK;
    };
    // wait for the oldest mirror and read it: a sequence whose word is a stop token leaves the lane table here
    auto retire = [&]() -> int {
      if (hipEventSynchronize(m->ev_chunk[head]) != hipSuccess) return (int)hipErrorUnknown;
      for (int s = 0; s < n_seq; ++s) {
        for (int p = checked[s]; p < infl[head].upto[s] && !stopped[s]; ++p)
          if (is_stop(pin[(size_t)(own_base(m, s) + p)], h_stop, n_stop)) {
            stop_at[s] = p;
            stopped[s] = 1;
          }
        checked[s] = infl[head].upto[s];
      }
      head ^= 1;
      --n_infl;
      return KH_OK;
    };
    const int per_check = n_stop > 0 ? KH_GRAPH_STEPS : INT_MAX;
    for (;;) {
      int k = 0;
      while (k < per_check) {
        int32_t who[KH_SEQ_SLOTS_MAX], at[KH_SEQ_SLOTS_MAX];
        const int n = kh_seq_next_pass(n_seq, width, pos.data(), total_steps, stopped.data(), &cursor, who);
        if (n == 0) break;
        KhSeqLanes lanes;
        for (int i = 0; i < n; ++i) {
          if (!wide) lane_set(m, lanes, i, who[i], pos[who[i]]);
          at[i] = pos[who[i]];
          pos[who[i]] += 1;
        }
        rc = wide ? seq_pass_enqueue_gemm(m, who, at, n, /*words=*/true, ex.on ? &tail : nullptr)
                  : seq_pass_enqueue(m, lanes, n, /*words=*/true, ex.on ? &tail : nullptr);
        if (rc != KH_OK) return fail(rc);
        ++k;
      }
      if (k > 0 && (rc = mirror()) != KH_OK) return fail(rc);
      if (n_infl == 2 || (k == 0 && n_infl > 0))
        if ((rc = retire()) != KH_OK) return fail(rc);
      if (k == 0 && n_infl == 0) break;
    }
    if (hipEventRecord(m->ev1, m->stream) != hipSuccess) return fail((int)hipErrorUnknown);
    if ((rc = kh_launch_status()) != KH_OK) return fail(rc);
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    for (int s = 0; s < n_seq; ++s) {
      const int n_out = stop_at[s] >= 0 ? stop_at[s] : total_steps[s];
      int32_t* w = h_words + (size_t)s * words_stride;
      for (int p = 0; p < n_out; ++p)
        w[p] = p < n_prompt[s] - 1 ? prompt[s][p + 1] : pin[(size_t)(own_base(m, s) + p)];  // forced, main.cpp:36-38
      n_words[s] = n_out;
    }
    if (h_elapsed_ms) KH_CHECK_HIP(hipEventElapsedTime(h_elapsed_ms, m->ev0, m->ev1));
    return KH_OK;
  });
}
}  // namespace

// ---- the sequence-level constraint: one automaton, one state word per slot (kh_fsm.h, kh_seq.h: k_seq_tail_fsm)
extern "C" int kh_model_seq_set_constraint(kh_model* m, const kh_fsm* a) {
  if (!m) return KH_ERR_INVALID_ARG;
  return kh_api_guard([&]() -> int {
    if (!a) {  // off: k_seq_pick / k_seq_tail again; the buffers stay for the next "on"
      m->seq_fsm_on = false;
      return KH_OK;
    }
    // every check before any device call
    int rc = kh_fsm_check_host(a, m->cfg.vocab_size);
    if (rc != KH_OK) return rc;
    if (m->fsm_on) return KH_ERR_UNSUPPORTED;  // one of the two constraints at a time
    FsmStage st;
    if ((rc = fsm_stage(m, a, m->seq_fsm, KH_SEQ_SLOTS_MAX, &st)) != KH_OK) return rc;
    KhFsmReach reach = kh_fsm_reach_host(a, KH_SEQ_BIAS_MAX);
    if (st.desc) {
      m->seq_fsm.desc = std::move(st.desc);
      m->seq_fsm.state = std::move(st.state);
    }
    m->seq_fsm_on = true;
    rc = seq_fsm_reset(m);
    const int rc2 = fsm_install(m, a, m->seq_fsm, st);
    if (rc != KH_OK || rc2 != KH_OK) {
      m->seq_fsm_on = false;
      return rc != KH_OK ? rc : rc2;
    }
    m->seq_fsm_reach = std::move(reach);
    return KH_OK;
  });
}
extern "C" int kh_model_seq_set_constraint_state(kh_model* m, int32_t slot, int32_t state) {
  if (!m) return KH_ERR_INVALID_ARG;
  if (!m->seq_fsm_on) return KH_ERR_UNSUPPORTED;
  if (slot < 0 || slot >= m->seq_slots || state < -1 || state >= m->seq_fsm.n_states) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(m->seq_fsm.state + slot), state, 1, m->stream));
  m->seq_fsm_state[slot] = state;
  return KH_OK;
}
extern "C" int kh_model_seq_get_constraint_state(kh_model* m, int32_t slot, int32_t* state) {
  if (!m || !state) return KH_ERR_INVALID_ARG;
  if (!m->seq_fsm_on) return KH_ERR_UNSUPPORTED;
  if (slot < 0 || slot >= m->seq_slots) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemcpyAsync(state, m->seq_fsm.state + slot, sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}
// host only, stateless: the two questions kh_model_seq_set_constraint and the launching calls ask of an automaton
// (kh_fsm.h: KhFsmReach), as entry points of their own - a caller can ask them before it submits a bias list
extern "C" int kh_fsm_components(const kh_fsm* a, int32_t* labels) {
  if (!labels) return KH_ERR_INVALID_ARG;
  const int rc = kh_fsm_check_host(a, INT64_MAX);
  if (rc != KH_OK) return rc;
  return kh_api_guard([&]() -> int {
    const KhFsmReach r = kh_fsm_reach_host(a, 0);
    memcpy(labels, r.label.data(), sizeof(int32_t) * r.label.size());
    return KH_OK;
  });
}
extern "C" int kh_fsm_bias_empties(const kh_fsm* a, int32_t state, const int32_t* h_ids, const float* h_bias, int32_t n,
                                   int32_t* emptied) {
  if (!emptied || n < 0 || (n > 0 && (!h_ids || !h_bias))) return KH_ERR_INVALID_ARG;
  const int rc = kh_fsm_check_host(a, INT64_MAX);
  if (rc != KH_OK) return rc;
  if (state < -1 || state >= a->n_states || n > KH_SEQ_BIAS_MAX) return KH_ERR_RANGE;
  return kh_api_guard([&]() -> int {
    std::vector<int32_t> banned;
    for (int i = 0; i < n; ++i)
      if (h_bias[i] == -INFINITY) banned.push_back(h_ids[i]);
    std::sort(banned.begin(), banned.end());
    const KhFsmReach r = kh_fsm_reach_host(a, KH_SEQ_BIAS_MAX);
    *emptied = kh_fsm_reach_emptied_host(a->row_ptr, a->tokens, r, state, banned) ? 1 : 0;
    return KH_OK;
  });
}

extern "C" int kh_model_seq_set_history(kh_model* m, int32_t slot, int32_t pos0, const int32_t* h_tokens, int32_t n) {
  if (!m || !h_tokens || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  if (slot < 0 || slot >= m->seq_slots || (int64_t)pos0 + n > cap(m, slot)) return KH_ERR_RANGE;
  if (writes_shared(m, slot, pos0)) return KH_ERR_INVALID_ARG;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  return hist_write(m, h_tokens, n, own_base(m, slot) + pos0);
}

extern "C" int kh_model_seq_get_logprobs(kh_model* m, int32_t slot, int32_t pos0, int32_t n, int32_t* h_token,
                                         float* h_lp, int32_t* h_top_ids, float* h_top_lp) {
  if (!m || n <= 0) return KH_ERR_INVALID_ARG;
  if (!m->d_lp_token || m->seq_lp_top_n < 0) return KH_ERR_UNSUPPORTED;
  if (slot < 0 || slot >= m->seq_slots || pos0 < 0 || (int64_t)pos0 + n > cap(m, slot)) return KH_ERR_RANGE;
  // a sharer has no records below its shared length (the rows there are its parent's, and so are the records): "none"
  const int w = m->seq_lp_top_n > 0 ? m->seq_lp_top_n : 0;
  const int skip = pos0 < slot_of(m, slot).pfx ? std::min(n, slot_of(m, slot).pfx - pos0) : 0;
  if (skip > 0) {
    if (h_token) memset(h_token, 0xFF, sizeof(int32_t) * (size_t)skip);
    if (h_lp) memset(h_lp, 0xFF, sizeof(float) * (size_t)skip);
    if (h_top_ids && w) memset(h_top_ids, 0xFF, sizeof(int32_t) * (size_t)skip * w);
    if (h_top_lp && w) memset(h_top_lp, 0xFF, sizeof(float) * (size_t)skip * w);
  }
  if (skip == n) return KH_OK;
  return lp_read(m, own_base(m, slot) + pos0 + skip, n - skip, m->seq_lp_top_n, h_token ? h_token + skip : nullptr,
                 h_lp ? h_lp + skip : nullptr, h_top_ids ? h_top_ids + (size_t)skip * w : nullptr,
                 h_top_lp ? h_top_lp + (size_t)skip * w : nullptr);
}

extern "C" int kh_seq_rank(int32_t n_seq, const float* h_lp, int32_t stride, const int32_t* first,
                           const int32_t* n_words, int32_t* order, double* mean_lp) {
  if (n_seq <= 0 || !h_lp || !first || !n_words || !order || stride < 0) return KH_ERR_INVALID_ARG;
  for (int s = 0; s < n_seq; ++s)
    if (first[s] < 0 || n_words[s] > stride) return KH_ERR_INVALID_ARG;
  return kh_api_guard([&]() -> int {
    std::vector<double> mean((size_t)n_seq);
    for (int s = 0; s < n_seq; ++s) {
      double sum = 0.0;
      for (int p = first[s]; p < n_words[s]; ++p) sum += (double)h_lp[(size_t)s * stride + p];
      mean[s] = n_words[s] > first[s] ? sum / (double)(n_words[s] - first[s]) : (double)NAN;
      if (mean_lp) mean_lp[s] = mean[s];
      order[s] = s;
    }
    std::stable_sort(order, order + n_seq, [&](int32_t a, int32_t b) {
      const bool na = std::isnan(mean[a]), nb = std::isnan(mean[b]);
      if (na || nb) return !na && nb;
      return mean[a] > mean[b];
    });
    return KH_OK;
  });
}
