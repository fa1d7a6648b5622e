// kh_model_internal.h — state and cross-unit helpers of the model level of the C-ABI.
// The model level is split into fourteen translation units:
//   kh_model_load.hip     .bin image -> HBM arena, weight table, buffers, create / destroy, cache I/O
//   kh_model_step.hip     launch shapes, the fused and unfused decode step, hipGraph capture,
//                         predict / generate (kh_fused.h kernels are instantiated here: one list of values per
//                         template parameter, picked from and launched through kh_dispatch.h)
//   kh_model_prefill.hip  the B-token VALU pass (kh_prefill.h kernels) and what runs on it: prefill, scoring, verify,
//                         the B-lane pass over different sequences (kh_seq.h kernels) and the twins of the B-token
//                         kernels on the 16-bit copy (kh_w16_pass.h)
//   kh_model_gemm.hip     what runs on the GEMM slabs (kh_gemm.h, kh_pattn.h, kh_seq_prefill.h, kh_seq_gemm.h kernels):
//                         the MFMA prompt prefill, its form into sequence slots and the wide sequence pass
//   kh_model_gemm_w16.hip the same GEMMs on the bf16 matrix cores from the 16-bit copy (KH_FLAG_GEMM16; kh_gemm_w16.h kernels)
//   kh_model_gemm_q16.hip the GEMMs of an int8 group-64 model on the bf16 matrix cores from the int8 image (KH_FLAG_GEMM16_Q8;
//                         kh_gemm_q16.h kernels)
//   kh_model_seq.hip      sequence slots of the K/V cache, kh_model_seq_step, kh_model_generate_batch and their _ex
//                         forms with per-sequence processors and log-probs (host side)
//   kh_model_profile.hip  per-kernel / per-step timing entry points
//   kh_model_screen.hip   the screened classifier of the greedy generate loop (kh_cls_screen.h kernels)
//   kh_model_selftest.hip creation-time checks of the ring kernels, the fence-free split merge, the screen and the
//                         weight copies (one check for W16 and Q4)
//   kh_model_w16.hip      the 16-bit copy of a bf16-exact fp32 model's matrices, and what every weight copy shares: its
//                         bytes, its build, its release and the routing of the decode GEMV launches that read a copy
//                         (kh_copy_launch.h: one launch text; the _w16 kernels of kh_w16.h are instantiated here)
//   kh_model_q4.hip       the 4-bit copy of a 4-bit-exact int8 model's matrices (the same launch text; the kh_q4.h
//                         kernels are instantiated here)
//   kh_model_q4_pass.hip  ... and its B-token passes (kh_pf_launch.h's launch text; the _q4 kernels of kh_q4_pass.h)
//   kh_model_h16.hip      the same launch text for a 16-bit copy in fp16 format (KH_FLAG_W16_F16; the _h16 kernels of kh_w16.h)
//   kh_model_h16_pass.hip ... and its B-token passes (the _h16 kernels of kh_w16_pass.h)
// gfx950 only.  No CPU fallback: every path launches HIP kernels.
//
// Ownership: every device or pinned-host buffer the library allocates is a KhDev<T> / KhPin<T> (kh_buf.h) - a field of
// kh_model or a local - and frees itself; kh_model_destroy has no list of them.  A function that needs several buffers
// together allocates into locals and moves them into the model once all of it succeeded, so a failed call leaves the
// model as it found it and emptiness of one member of a group says whether the group exists.  Not owned this way, and
// released by hand: the VMM-mapped KV cache (KvVmm, kv_release), the weight arena (borrowed in
// kh_model_create_from_device_weights), the stream, events and graphs.
#pragma once
#include <new>
#include <thread>
#include <stdint.h>

#include <utility>
#include <vector>

#include "kh_attn.h"
#include "kh_buf.h"
#include "kh_common.h"
#include "kh_fsm.h"
#include "kh_seq_plan.h"
#include "kh_step_tail.h"

namespace khm {
// the two places memory comes from (alloc: KH_OK or the HIP error code)
struct KhDevMem {
  static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
struct KhPinMem {
  static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};
static_assert(KH_BUF_OK == KH_OK && KH_BUF_OOM == (int)hipErrorOutOfMemory, "kh_buf.h speaks HIP's codes");
template <class T>
using KhDev = KhBuf<T, KhDevMem>;
template <class T>
using KhPin = KhBuf<T, KhPinMem>;
// No C++ exception crosses the C ABI: the entry points that allocate host containers or start threads run their
// body through this (std::bad_alloc -> hipErrorOutOfMemory, anything else -> KH_ERR_INTERNAL).
template <class F>
static inline int kh_api_guard(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return (int)hipErrorOutOfMemory;
  } catch (...) {
    return KH_ERR_INTERNAL;
  }
}
// joins a helper thread on every way out of a scope (an exception while it runs would otherwise terminate)
struct KhJoinOnExit {
  std::thread& t;
  ~KhJoinOnExit() {
    if (t.joinable()) t.join();
  }
};

struct LayerW {
  KhLin wq, wk, wv, wo, w1, w2, w3;
  const float* att_norm;
  const float* ffn_norm;
};

}  // namespace khm
using khm::KhDev;
using khm::KhPin;
using khm::LayerW;

#define KH_STEP_VARIANTS 3  // kh_model_step.hip::step_variant
struct KhSampParams;       // kh_sample.h
struct KhQkvArgs;          // kh_fused.h
struct KhGemvResArgs;
struct KhWoCombArgs;
struct KhFfn13Args;
struct KhClsArgs;
struct KhProcParams;       // kh_logit_proc.h
struct KhPgGemmArgs;       // kh_gemm.h
struct KhRgTiles;          // kh_seq_prefill.h
struct KhWideLanes;        // kh_seq_gemm.h
struct kh_model {
  kh_config cfg{};
  kh_model_opts opts{};
  hipStream_t stream = nullptr;
  // weights: one arena holding the .bin bytes after the header, in file order (a raw pointer: borrowed from the
  // caller by kh_model_create_from_device_weights, else freed by kh_model_destroy)
  char* arena = nullptr;
  bool owns_arena = false;
  size_t arena_bytes = 0;
  std::vector<LayerW> layers;
  const float* tok_emb = nullptr;
  const float* final_norm = nullptr;
  KhLin cls{};
  int gshift = 0;
  // activations / caches (llama3.cpp:425-500)
  KhDev<float> x, rms, q, att, h1, h3, w2o, logits, score, sin_cache, cos_cache;
  // the cache's addresses: reserved ranges of KvVmm (not owned here: kv_release), or kv_plain's two halves
  float *kcache = nullptr, *vcache = nullptr;
  KhDev<float> kv_plain[2];
  KhDev<float> part_val;
  KhDev<int32_t> part_idx;
  int nparts = 0;
  // KV cache on reserved addresses, physical memory mapped on demand (kh_model_load.hip::kv_ensure): the contiguous
  // [layer, cache_len, kv_dim] addressing of llama3.cpp:469-472 with HBM committed only for the rows a sequence reached
  struct KvVmm {
    bool on = false;
    size_t chunk = 0;      // mapping unit in bytes (a multiple of the allocation granularity)
    size_t reserved = 0;   // bytes reserved per cache (K and V each)
    size_t mapped = 0;     // bytes mapped, K + V
    std::vector<uint8_t> have[2];  // per chunk of the K / V reservation: mapped?
    struct Run {
      void* va;
      size_t len;
      hipMemGenericAllocationHandle_t h;
    };
    std::vector<Run> runs;
    int rows_all = 0;      // rows [0, rows_all) of EVERY layer are mapped
  };
  KvVmm kv;
  float load_ms = 0.f;      // host image -> HBM upload time (kh_model_get_load_ms)
  std::thread unmap_thread;  // kh_model_create_from_file: munmap of the file off the critical path, joined by destroy
  KhDev<char> attn_ws;  // split-T attention partials + tickets (kh_attn.h)
  int attn_ns = 1;
  int attn_ns_g = 0;        // GQA long-context path: splits per KV group (0 = path off)
  int attn_ws_stride = 1;   // split slots per head in attn_ws
  int attn_t_long = 1 << 30;
  int attn_wg = KH_WG;
  int attn_ts_shift = 8;     // log2 of the per-head split quantum (kh_attn.h::attn_ts_shift_for)
  bool attn_fenced = false;  // KH_FLAG_ATTN_MERGE_FENCED / KH_ATTN_FENCED: fences around the in-launch split merge
  bool attn_defer = false;  // variant 1 exists: split partials combined by kh_fused.h::k_wo_comb
  int attn_defer_max = 0;   // ... up to this many active splits (more: the in-launch merge is as fast or faster)
  KhDev<int32_t> d_pos, d_token, d_next, d_forced, d_words;
  int seq_cap = 0;  // capacity of d_forced / d_words
  // prefill (kh_prefill.h): residual / q / attention / hidden rows of up to KH_PF_BMAX prompt tokens
  // (one group, made by the first call that needs it: pf_x says whether it exists)
  KhDev<float> pf_x, pf_q, pf_att, pf_h;
  KhDev<char> pf_ws;            // KH_PF_BMAX attention split workspaces
  size_t pf_ws_tok_bytes = 0;
  // sequence scoring (kh_model_score): k_pf_cls's logits of one pass, [KH_PF_BMAX][pf_vstride], pf_vstride = the
  // vocabulary rounded up to 4 floats; made by the first call that needs it
  KhDev<float> pf_logits;
  int pf_vstride = 0;
  // speculative greedy decode (kh_model_verify, kh_spec.h): the result block of a verify pass {a, pick[0 .. 8)} on the
  // device and its pinned mirror; one group, made by the first verify pass
  KhDev<int32_t> d_spec;
  KhPin<int32_t> h_spec_pin;
  // ... under the model's settings (kh_model_verify_as_set; k_spec_tail): the processing core's counters per ROW of the
  // pass, [KH_PF_BMAX][vocab], zeroed once (the core re-arms them); made by the first such pass with processors on
  KhDev<int32_t> d_spec_cnt;
  // ... and under its constraint (kh_model_verify_fsm; k_spec_fsm_rows): the automaton state of every row of the pass,
  // [KH_PF_BMAX] - ahead of the row behind k_spec_fsm_rows, behind its pick behind k_spec_tail_fsm, -1: the row stands
  // behind a fed token that cannot be followed; made by the first such pass
  KhDev<int32_t> d_spec_fsm;
  // Sequence slots (kh_model_seq_slots, kh_model_seq.hip): the cache rows cut into seq_slots equal regions of
  // cache_len / seq_slots rows - bookkeeping, no kernel reads it.  Device tables with one entry per slot, one group
  // made by the first seq pass: the token the slot's sequence feeds next and its sampling parameters; the words of every
  // sequence at its slot's rows ([cache_len]); pinned mirrors / staging of the three.
  int seq_slots = 1;
  // ... or into slots of unequal length (kh_model_seq_slots_var), some of which read a prompt prefix from another
  // slot's rows (kh_model_seq_share): row0 / len / sharing of every slot; the equal partition is the same table
  KhSeqSlot seq_tab[KH_SEQ_SLOTS_MAX];
  bool seq_pfx_pad8 = false;  // hook KH_SEQ_PFX_PAD=1: k_seq_attn_pfx's grid.x padded to a multiple of 8
  KhDev<int32_t> d_seq_tok;
  KhDev<KhSampParams> d_seq_samp;
  KhDev<int32_t> d_seq_words;
  KhPin<int32_t> h_seq_tok_pin;
  KhPin<KhSampParams> h_seq_samp_pin;
  KhPin<int32_t> h_seq_words_pin;
  // ... with per-sequence processors or log-probs (kh_model_seq_step_ex, kh_model_generate_batch_ex; k_seq_tail):
  // per-slot KhProcParams and bias lists [KH_SEQ_SLOTS_MAX][KH_SEQ_BIAS_MAX], the processing core's counters per LANE
  // [KH_PF_BMAX][vocab] (zeroed once, the core re-arms them), pinned staging of the tables and of the history uploads
  // [cache_len]; one group, made by the first call that asks (seq_prepare_ex).  The history is d_hist and the records are
  // d_lp_* below, both addressed by cache row.  seq_lp_top_n: the record width of the last such call (-1: none yet)
  KhDev<KhProcParams> d_seq_proc;
  KhDev<int32_t> d_seq_bias_ids;
  KhDev<float> d_seq_bias;
  KhDev<int32_t> d_seq_cnt;
  KhPin<KhProcParams> h_seq_proc_pin;
  KhPin<int32_t> h_seq_bias_ids_pin;
  KhPin<float> h_seq_bias_pin;
  KhPin<int32_t> h_seq_hist_pin;
  int seq_lp_top_n = -1;
  // GEMM prefill (kh_gemm.h): slabs of KH_PG_TMAX token rows (one group: pg_x says whether it exists)
  KhDev<float> pg_x, pg_xn, pg_q, pg_att, pg_h;
  KhDev<float> pg_part;         // partial rows of residual GEMMs that split K across workgroups
  KhDev<char> pg_ws;            // KH_PG_TMAX attention split workspaces (the first pass that takes the fallback)
  size_t pg_ws_tok_bytes = 0;
  // the wide sequence pass (kh_seq_gemm.h): logits rows [KH_SEQ_SLOTS_MAX][pf_vstride] of its classifier GEMM, made by
  // the first wide call; sg_lanes: the lane count of the last wide pass (0: none yet)
  KhDev<float> sg_logits;
  int sg_lanes = 0;
  KhPin<int32_t> h_words_pin;   // pinned mirror of d_words (stop-token check, final copy-out)
  KhPin<int32_t> h_forced_pin;  // pinned staging of d_forced [seq_cap + 1]: the upload needs no host sync
  int forced_hwm = 0;              // entries of d_forced that may differ from -1 (the last generate's upload)
  bool forced_in_flight = false;   // a generate returned before its final stream sync: h_forced_pin may be under DMA
  // near-tie report (kh_model_first_sample): logits of the first sampled step of the last generate with a prefill
  KhDev<float> first_logits;      // [vocab], made on first use
  int first_pos = -1;             // -1: the last generate had no prefill phase
  int first_mode = 0;             // 1 = kh_model_prefill, 2 = kh_model_prefill_gemm
  hipEvent_t ev_chunk[2] = {nullptr, nullptr};
  // launch geometry
  struct Shape {
    int u = 2, split = 1, grid = 1, wg = KH_WG;
  };
  Shape sh_qkv, sh_wo, sh_ffn, sh_w2, sh_cls;
  // int8 ffn13 / cls on the LDS-DMA ring kernels (kh_fused_ring.h): ring slots per wave (0 = the register-tile
  // kernel of sh_ffn / sh_cls) and workgroups (256 threads each); chosen by plan_ring
  struct RingPlan {
    int ffn_r = 0, ffn_grid = 0, cls_r = 0, cls_grid = 0;
  };
  RingPlan ring;
  // graph
  // the decode step captured once as a 1-step graph and once as a KH_GRAPH_STEPS-step graph:
  // consecutive hipGraphLaunch calls leave the GPU idle for ~8 us (measured), so the long
  // graph amortises that gap over several tokens
  // ... each in three VARIANTS of the attention / wo pair (kh_model_step.hip::step_variant): 0 = the
  // attention launch merges its time splits itself (valid at every position; nothing to merge below
  // position 256), 1 = the splits are merged by k_wo_comb (positions on the per-head path only), 2 = as 0
  // with the per-head-only attention instantiation (positions below the group path, merge not deferrable)
  struct StepGraph {
    hipGraph_t g = nullptr;
    hipGraphExec_t e = nullptr;
  };
  // [StepTail][variant][log2 steps]: graphs of 1, 2, 4 and KH_GRAPH_STEPS = 8 steps per tail of the step
  StepGraph sg[8][KH_STEP_VARIANTS][4];
  // kh_model_set_sampling: the parameters (host copy), whether they sample (temperature > 0), and their device copy,
  // which the captured k_sample_topp launches read (a new seed or temperature needs no recapture)
  kh_sampling samp{0.f, 0, 1.f, 0};
  bool samp_on = false;
  KhDev<KhSampParams> d_samp;
  // Logit processors (kh_logit_proc.h).  d_hist[hist_cap = cache_len + 1]: the token fed at every position, -1 where
  // none was: written by set_state, by k_sample_proc for the token it feeds next, by the prompt upload of a generate
  // with processors on and by kh_model_prefill / kh_model_prefill_gemm - like the K/V rows, slots below a call's
  // position are whatever earlier calls left.  Sized by the cache, not by seq_cap: predict reaches every position.
  // kh_model_set_penalties / kh_model_set_logit_bias: host copies, whether anything is on, and the device copies the
  // captured k_sample_proc launches read (new values need no recapture; a bias list that outgrows d_bias does).
  KhDev<int32_t> d_hist;
  int hist_cap = 0;
  kh_penalties pen{1.f, 0.f, 0.f, 0};
  int n_bias = 0;
  bool proc_on = false;
  KhDev<KhProcParams> d_proc;
  KhDev<int32_t> d_bias_ids;
  KhDev<float> d_bias;
  KhDev<int32_t> d_cnt;  // [vocab] counters of the processing core, zero between launches
  // Log-probs (kh_logprobs.h, kh_model_set_logprobs).  lp_top_n: -1 off, else the width of a record's top list; its
  // device copy d_lp_top_n is what the captured k_sample_lp launches read (a new width needs no recapture).  Records of
  // every position, [lp_cap = cache_len] with a fixed stride of KH_LOGPROBS_MAX_TOP like d_hist: predict reaches every
  // position.  One group, made by the first call that needs records (lp_ensure_records), all bytes 0xff ("none": -1 / NaN) where no
  // sampled step wrote.  While on, d_proc / d_samp / d_cnt exist too (neutral / greedy unless set): k_sample_lp reads them.
  int lp_top_n = -1;
  int lp_cap = 0;
  KhDev<int32_t> d_lp_top_n;
  KhDev<int32_t> d_lp_token;
  KhDev<float> d_lp_lp;
  KhDev<int32_t> d_lp_top_ids;
  KhDev<float> d_lp_top_lp;
  // Constraint (kh_fsm.h, kh_model_set_constraint).  d_fsm: the descriptor the captured k_sample_*_fsm launches read,
  // d_fsm_state: the automaton state - both allocated once, by the first "on", so that a new automaton rewrites the
  // descriptor and swaps the buffers behind it without a recapture (the old buffers go once the stream has drained).
  // Host copies of what the checks need: the CSR rows (a -inf bias may not empty a row) and the -inf ids of the bias.
  struct Fsm {
    KhDev<KhFsmDev> desc;
    KhDev<int32_t> state;
    KhDev<uint32_t> mask;
    KhDev<int64_t> row_ptr;
    KhDev<int32_t> tokens, next;
    int n_states = 0, start = 0;
    std::vector<int64_t> h_row_ptr;
    std::vector<int32_t> h_tokens;
    std::vector<int32_t> h_next;  // (kh_model_generate_lookup_fsm walks the state on the host)
  };
  Fsm fsm;
  bool fsm_on = false;
  // The sequence-level constraint (kh_model_seq_set_constraint; k_seq_tail_fsm): one automaton for all slots, the same
  // buffers with a state table of KH_SEQ_SLOTS_MAX words, -1 = the slot is unconstrained.  One of the two constraints is
  // on at a time.  seq_fsm_state: the state the host last set per slot - it decides whether a pass ends in
  // k_seq_tail_fsm and which rows a lane's -inf bias is checked against (seq_fsm_reach; the host never walks
  // these).  The device moves the words; a word that was set >= 0 stays >= 0.
  Fsm seq_fsm;
  bool seq_fsm_on = false;
  int32_t seq_fsm_state[KH_SEQ_SLOTS_MAX];
  KhFsmReach seq_fsm_reach;
  std::vector<int32_t> bias_banned;  // ascending ids of the bias list's -inf entries
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // Screened classifier of the greedy generate loop (kh_cls_screen.h, kh_model_screen.hip): fp32 models only
  struct ClsScreen {
    bool on = false;        // the bf16 copy exists and the creation-time check passed (or was skipped)
    int selftest = 0;       // 0 not applicable / skipped, 1 passed, -1 failed -> screening off
    KhDev<uint16_t> wbf;       // [vocab, dim] bf16 copy of the classifier
    KhDev<float> err;          // [vocab] per-row error norm
    KhDev<float> x_save;       // [dim] input of the last screened step
    KhDev<float> p_lb, p_spill, p_ub;  // partials of k_cls_screen
    KhDev<int32_t> p_idx;
    KhDev<float> ov_val;       // argmax partials of an overflow step [sgrid]
    KhDev<int32_t> ov_idx;
    KhDev<uint32_t> ticket;
    KhDev<int32_t> stats;      // steps, candidate rows, overflow steps
    int u = 4, grid = 1, wg = KH_WG, sgrid = 1;  // launch of k_cls_screen; workgroups of k_sample_screen
    size_t bytes = 0;          // HBM the copy and its tables take
    float build_ms = 0.f;      // time of the conversion kernel
    bool stale = false;        // the logits buffer is older than the last step: refresh from x_save on demand
    // the int8 tier ahead of the bf16 screen (k_cls_q8_build, k_cls_screen_q8, k_cls_screen's survivor mode)
    struct Q8 {
      bool on = false;         // the int8 copy exists and its creation-time check passed (or was skipped)
      int selftest = 0;        // 0 not applicable / skipped, 1 passed, -1 failed -> tier off, the bf16 screen goes on
      KhDev<int8_t> q;         // [vocab, dim]
      KhDev<float> sc;         // [vocab, dim / 64]
      KhDev<float> e8;         // [vocab]
      KhDev<float> p_lb, p_spill, p_ub;  // partials of k_cls_screen_q8
      KhDev<int32_t> p_idx;
      KhDev<int32_t> stats;    // tier-1 steps, rows that survived it, steps in which it spilled
      int u = 2, grid = 1, wg = KH_WG;  // launch of k_cls_screen_q8
      size_t bytes = 0;
      float build_ms = 0.f;
    };
    Q8 q8;
  };
  ClsScreen scr;
  // A narrow exact copy of the model's matrices (kh_model_w16.hip: copy_build, copy_release): a second
  // arena that the batch-1 decode GEMVs of the adopted launch classes read instead of the image.  What W16 and Q4 share.
  struct WCopy {
    int state = 0;          // 0 off or not applicable, 1 on, -1 some matrix is not exact in the copy, -2 the self-check failed
    KhDev<char> alloc;      // the allocation; arena = its first 4-KiB boundary
    char* arena = nullptr;
    size_t bytes = 0;       // of the copy (every matrix padded to 256 bytes)
    float build_us = 0.f;   // the build kernel over all matrices
    int classes = 0;        // KH_W16_* bits: launch classes that run on the copy
    int first_inexact = -1; // tensor index 7 * layer + {wq, wk, wv, wo, w1, w2, w3}, 7 * layers = classifier
    struct Layer {
      const void *wq, *wk, *wv, *wo, *w1, *w2, *w3;
    };
    std::vector<Layer> layers;
    const void* cls = nullptr;
  };
  // W16 (kh_w16.h, kh_model_w16.hip; KH_FLAG_W16 / hook KH_W16): the upper halves of every matrix word of a bf16-exact
  // fp32 model (state -1: some matrix is not exact in a format asked for), read by the B-token passes of the adopted
  // classes as well.  With KH_FLAG_W16_F16 / hook KH_W16_F16 an image that is not bf16-exact but fp16-exact gets the
  // fp16 values instead.  classes: plan_w16.
  struct W16 : WCopy {
    int format = 0;         // of the live copy: KH_W16_BF16 (also: no copy) or KH_W16_F16 (kh_w16.h)
    int first_inexact_f16 = -1;  // as first_inexact, for the fp16 format (-1: not tried, or every tensor passed)
    int pass_classes = 0;   // classes whose B-token pass reads the copy too (kh_w16_pass.h; hook KH_W16_PASS): a subset of classes
    // KH_FLAG_GEMM16 / hook KH_GEMM16 (kh_gemm_w16.h): classes whose GEMMs of the GEMM pass (kh_model_gemm.hip:
    // pg_gemm) run on the bf16 matrix cores from the copy - a live bf16-format copy, the GEMM prefill's geometry, K a
    // multiple of 32 and the adoption mask (plan_gemm16, hook KH_GEMM16_CLASSES); 0 wherever the flag is inert, and
    // gemm_reason says why (KH_GEMM16_*: kh_model_gemm16_info)
    int gemm_classes = 0;
    int gemm_reason = 0;
    int gemm_plan = 0;      // plan_gemm16's mask for the geometry, whatever the hook says (0 unless the flag is live)
  };
  W16 w16;
  // Q4 (kh_q4.h, kh_model_q4.hip; KH_FLAG_Q4 / hook KH_Q4): the low nibbles of every int8 matrix value of a 4-bit-exact
  // int8 model, two per byte (state -1: some value lies outside [-8, 7]).  The group scales stay where they are.  The
  // decode launches of `classes` (plan_q4, hook KH_Q4_CLASSES) and the B-token passes of `pass_classes` read the copy;
  // the GEMM passes and whatever is in neither mask read the int8 image.
  struct Q4 : WCopy {
    int nparts_image = 0;   // m->nparts of the int8 launches (the ring classifier's grid), for a copy that is given up
    // classes whose B-token pass reads the copy (kh_q4_pass.h; hook KH_Q4_PASS): the copy holds every matrix, so the mask
    // does not depend on `classes`; 0 unless the copy is live
    int pass_classes = 0;
  };
  Q4 q4;
  // KH_FLAG_GEMM16_Q8 / hook KH_GEMM16_Q8 (kh_gemm_q16.h, kh_model_gemm_q16.hip): classes whose GEMMs of the
  // GEMM pass (kh_model_gemm.hip: pg_gemm) run on the bf16 matrix cores from the int8 image itself - an int8 group-64
  // model on the GEMM prefill's geometry and the adoption mask (plan_gemm16_q8, hook KH_GEMM16_Q8_CLASSES); 0 wherever
  // the flag is inert, and reason says why (KH_GEMM16_Q8_*: kh_model_gemm16_q8_info).  No copy, no memory.
  struct Gemm16Q8 {
    int classes = 0;
    int reason = 0;
    int plan = 0;           // plan_gemm16_q8's mask for the geometry, whatever the hook says (0 unless the flag is live)
  };
  Gemm16Q8 g16q8;
};

#define KH_GRAPH_STEPS 8
#define KH_PG_MIN_TOKENS 16  // prompts with fewer fed-only tokens stay on the bit-identical path

namespace khm {
// every token of a caller's array is a row of the embedding table (the entry points answer KH_ERR_RANGE otherwise)
inline bool tokens_in_vocab(const kh_model* m, const int32_t* toks, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (toks[i] < 0 || toks[i] >= m->cfg.vocab_size) return false;
  return true;
}

// ---- kh_model_step.hip ----------------------------------------------------------------------
kh_model::Shape pick_shape(bool quant, int pairs, int M, int max_split, const char* env, int wg = KH_WG,
                           int wg_max = KH_WG, bool many_waves = false, bool u3 = false);
// launch geometry of the five GEMV kernels of a decode step: qkv, wo, ffn13, w2, cls (host-only)
void plan_decode_shapes(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size, kh_model::Shape (&out)[5]);
// which int8 GEMVs of a decode step run on the LDS-DMA ring kernels, and their launch geometry (host-only)
void plan_ring(bool quant, int dim, int hidden_dim, int vocab_size, int group_size, kh_model::RingPlan* out);
int configure_step_kernels(kh_model* m);  // >64 KiB dynamic-LDS opt-in of the hidden-sized GEMVs
// What a launch helper does beyond the model's plan is an argument, never a field of *m changed around the call.
// variant (see kh_model::sg, step_variant): which attention / wo pair is launched; fenced: the form of the in-launch
// split merge (m->attn_fenced, but for the self-test that compares the two)
KhAttnArgs fill_attn(kh_model* m, int l, int variant, bool fenced);
// on: what the launch streams its matrices from - the image, the 16-bit copy (kh_model::w16) or the 4-bit copy
// (kh_model::q4); a kernel on a copy has the bits of the one on the image.  The forms without the argument follow the
// model's plan.  A launch on the 4-bit copy has no ring form: it takes the place of the ring launch.
// A type of its own: a bool or a class bit in its place does not compile.
enum KhOn { KH_ON_IMAGE = 0, KH_ON_W16 = 1, KH_ON_Q4 = 2 };
enum { KH_W16_QKV = 1, KH_W16_WO = 2, KH_W16_FFN13 = 4, KH_W16_W2 = 8, KH_W16_CLS = 16, KH_W16_ALL = 31 };
// classes whose B-token pass reads the copy unless KH_W16_PASS says otherwise: the ones 3.1c's adoption rule keeps on
// every geometry (profiles/w16_pass_ab.txt; qkv and wo fail it on Qwen2.5-0.5B, cls on TinyLlama)
enum { KH_W16_PASS_DEFAULT = KH_W16_FFN13 | KH_W16_W2 };
static inline bool w16_runs(const kh_model* m, int cls) { return (m->w16.classes & cls) != 0; }
static inline bool q4_runs(const kh_model* m, int cls) { return (m->q4.classes & cls) != 0; }  // same class bits
static inline KhOn runs_on(const kh_model* m, int cls) {
  return q4_runs(m, cls) ? KH_ON_Q4 : (w16_runs(m, cls) ? KH_ON_W16 : KH_ON_IMAGE);
}
// the GEMM pass of the class on the bf16 matrix cores (kh_model_gemm.hip: pg_gemm)
static inline bool gemm16_runs(const kh_model* m, int cls) { return m->w16.state == 1 && (m->w16.gemm_classes & cls) != 0; }
// why KH_FLAG_GEMM16 does nothing on a model (kh_model_gemm16_info, slot 2); KH_GEMM16_ON: it does something
enum { KH_GEMM16_ON = 0, KH_GEMM16_NO_FLAG = 1, KH_GEMM16_NO_W16 = 2, KH_GEMM16_QUANT = 3, KH_GEMM16_INEXACT = 4,
       KH_GEMM16_FP16_COPY = 5, KH_GEMM16_GEOMETRY = 6, KH_GEMM16_NO_CLASS = 7, KH_GEMM16_SELFCHECK = 8 };
// the GEMM pass of the class on the bf16 matrix cores from the int8 image (KH_FLAG_GEMM16_Q8; kh_model_gemm.hip: pg_gemm)
static inline bool gemm16_q8_runs(const kh_model* m, int cls) { return (m->g16q8.classes & cls) != 0; }
// why KH_FLAG_GEMM16_Q8 does nothing on a model (kh_model_gemm16_q8_info, slot 2); KH_GEMM16_Q8_ON: it does something
enum { KH_GEMM16_Q8_ON = 0, KH_GEMM16_Q8_NO_FLAG = 1, KH_GEMM16_Q8_FP32 = 2, KH_GEMM16_Q8_GROUP = 3,
       KH_GEMM16_Q8_GEOMETRY = 4, KH_GEMM16_Q8_NO_CLASS = 5 };
// the B-token pass of the class (kh_model_prefill.hip: launch_pf_pass, pf_gemv_res, launch_pf_cls)
static inline bool w16_pass_runs(const kh_model* m, int cls) { return (m->w16.pass_classes & cls) != 0; }
// classes whose B-token pass reads the 4-bit copy unless KH_Q4_PASS says otherwise: the ones 3.1c's adoption rule keeps
// on both geometries of the same-box A/B (tools/q4_pass_ab.py, profiles/q4_pass_ab.txt).  w2 alone: in
// both runs a prefill pass takes -0.8 % at Llama-2-7B int8 geometry (2.814 -> 2.791 ms) and -0.4 % at TinyLlama's
// (0.825 -> 0.822 ms), each beyond the range of the int8 runs; wo and qkv pass at TinyLlama's in one run of two, ffn13
// and cls in none (the pass is bound by its LDS reads and FMAs, not by the weight bytes)
enum { KH_Q4_PASS_DEFAULT = KH_W16_W2 };
static inline bool q4_pass_runs(const kh_model* m, int cls) { return (m->q4.pass_classes & cls) != 0; }
// what the B-token pass of the class streams its matrices from (an image is fp32 or int8, so at most one copy is live)
static inline KhOn pass_runs_on(const kh_model* m, int cls) {
  return q4_pass_runs(m, cls) ? KH_ON_Q4 : (w16_pass_runs(m, cls) ? KH_ON_W16 : KH_ON_IMAGE);
}
void launch_qkv(kh_model* m, int l, KhOn on);
void launch_attn(kh_model* m, int l, int variant, bool fenced);
void launch_wo(kh_model* m, int l, int variant, KhOn on);
// ring: the LDS-DMA ring kernel (m->ring.ffn_r), else register tiles
void launch_ffn13(kh_model* m, int l, bool ring, KhOn on);
void launch_w2(kh_model* m, int l, KhOn on);
static inline void launch_qkv(kh_model* m, int l) { launch_qkv(m, l, runs_on(m, KH_W16_QKV)); }
static inline void launch_wo(kh_model* m, int l, int variant) { launch_wo(m, l, variant, runs_on(m, KH_W16_WO)); }
static inline void launch_ffn13(kh_model* m, int l, bool ring) { launch_ffn13(m, l, ring, runs_on(m, KH_W16_FFN13)); }
static inline void launch_w2(kh_model* m, int l) { launch_w2(m, l, runs_on(m, KH_W16_W2)); }
// what a classifier launch reads and writes; the model's own buffers and plan: launch_cls(m)
struct ClsIo {
  const float* x;
  float *logits, *part_val;
  int32_t* part_idx;
};
void launch_cls(kh_model* m, const ClsIo& io, bool ring, KhOn on);
static inline void launch_cls(kh_model* m, const ClsIo& io, bool ring) {
  launch_cls(m, io, ring, runs_on(m, KH_W16_CLS));
}
static inline void launch_cls(kh_model* m) {
  launch_cls(m, {m->x, m->logits, m->part_val, m->part_idx}, m->ring.cls_r == 2);
}
// a classifier launch has written the model's own logits buffer (kh_model_get_logits need not re-run k_cls)
static inline void logits_fresh(kh_model* m) { m->scr.stale = false; }
// The last two launches of a fused step, and the index of kh_model::sg its graphs live in: k_cls + k_sample (argmax),
// k_cls + k_sample_topp, the screened pair k_cls_screen + k_sample_screen (greedy steps of a generate, see scr), or
// k_cls + k_sample_proc (penalties or a logit bias set: processing, then the greedy or sampled pick), or k_cls +
// k_sample_lp (log-probs on: k_sample_proc's duties, then the record of the position).  kScreenQ8: the screened pair
// behind its int8 tier, k_cls_screen_q8 + k_cls_screen (survivor mode) + k_sample_screen: 5L + 3 launches
// kProcessFsm / kLogprobFsm: a constraint is set (kh_fsm.h) - k_cls + k_sample_proc_fsm / k_sample_lp_fsm, the two
// tails above with the mask of the automaton state's row ahead of the chain and the transition behind the pick
enum StepTail { kGreedy = 0, kSample = 1, kScreen = 2, kProcess = 3, kLogprob = 4, kScreenQ8 = 5, kProcessFsm = 6,
                kLogprobFsm = 7 };
static inline bool tail_screens(StepTail t) { return t == kScreen || t == kScreenQ8; }
// log-probs, processing and sampling need every logit: they are stronger than a caller's wish to screen, and log-probs
// are stronger than the rest.  process = false: a step whose pick is discarded (kh_model_predict at a prompt position)
// leaves its logits as the classifier wrote them and writes no record
// screen: 0 no, 1 the bf16 screen, 2 the bf16 screen behind its int8 tier (cls_screen_level)
static inline StepTail step_tail(const kh_model* m, int screen, bool process = true) {
  return m->fsm_on && process        ? (m->lp_top_n >= 0 ? kLogprobFsm : kProcessFsm)
         : m->lp_top_n >= 0 && process ? kLogprob
         : m->proc_on && process     ? kProcess
         : m->samp_on                ? kSample
         : screen == 2               ? kScreenQ8
         : screen                    ? kScreen
                                     : kGreedy;
}
// what every step tail leaves behind (kh_step_tail.h): the last member of the five tails' arguments
static inline KhStepState fill_step_tail(const kh_model* m, int advance, int n_forced) {
  KhStepState st;
  st.forced = n_forced > 0 ? (const int32_t*)m->d_forced : nullptr;
  st.n_forced = n_forced;
  st.words = m->d_words;
  st.words_cap = m->seq_cap;
  st.d_next = m->d_next;
  st.d_token = m->d_token;
  st.d_pos = m->d_pos;
  st.tok_emb = m->tok_emb;
  st.x = m->x;
  st.dim = m->cfg.dim;
  st.vocab = m->cfg.vocab_size;
  st.advance = advance;
  return st;
}
// the model's log-prob record buffers as the kernels take them
static inline KhTailRecs lp_records(const kh_model* m) {
  return {m->d_lp_token, m->d_lp_lp, m->d_lp_top_ids, m->d_lp_top_lp};
}
// the step's last launch
void launch_sample(kh_model* m, int advance, int n_forced, StepTail tail);
// the variant of the steps at positions pos_lo .. pos_hi
int step_variant(const kh_model* m, int pos_lo, int pos_hi);
void launch_step_fused(kh_model* m, int advance, int n_forced, hipEvent_t* ev, int variant, StepTail tail);
int launch_step_unfused(kh_model* m, int pos, bool process);  // process: apply the model's logit processors
void set_state(kh_model* m, int token, int pos);
// d_hist[pos0 .. pos0 + n) = h_tokens (the public prefill entry points; a generate uploads its prompt itself)
int hist_write(kh_model* m, const int32_t* h_tokens, int n, int pos0);
// log-probs on: the records of positions [pos0, pos0 + n) become "none" (fed, not sampled), on the model stream
int lp_none(kh_model* m, int pos0, int n);
// the record buffers (d_lp_*, lp_cap), all "none", allocated by whoever needs them first: kh_model_set_logprobs and
// the sequence passes with log-probs (seq_prepare_ex); lp_top_n is the caller's to set
int lp_ensure_records(kh_model* m);
// records [pos0, pos0 + n) become "none" whatever the model's own setting says
int lp_fill_none(kh_model* m, int pos0, int n);
// records [pos0, pos0 + n) to the host with top lists of width w (kh_model_get_logprobs); synchronises
int lp_read(kh_model* m, int pos0, int n, int w, int32_t* h_token, float* h_lp, int32_t* h_top_ids, float* h_top_lp);
int ensure_pinned_words(kh_model* m, int n);
int ensure_chunk_events(kh_model* m);  // ev_chunk, made by whoever needs them first
int ensure_seq_cap(kh_model* m, int n);
void destroy_step_graphs(kh_model* m);
// the captured graph of `nsteps` in {1, 2, 4, 8} decode steps in `variant` ending in `tail`, captured on first use
int step_graph(kh_model* m, int n_forced, int variant, int nsteps, StepTail tail, hipGraphExec_t* out);
// Enqueue the steps at positions pos .. pos + nsteps - 1 behind whatever set the state: one replay of their captured
// graph (exec KH_EXEC_GRAPH) or eager launches (KH_EXEC_FUSED).  Picks the variant; records whether the logits buffer
// is left behind the steps (scr.stale).
int enqueue_steps(kh_model* m, int pos, int nsteps, int n_forced, StepTail tail, int exec);
// ---- kh_model_screen.hip --------------------------------------------------------------------
int cls_screen_create(kh_model* m);   // bf16 copy + tables, once the weights are resident (no-op where it does not apply)
void cls_screen_release(kh_model* m);  // frees the copies and tables; screening is off afterwards
bool cls_screen_wanted(const kh_model* m);  // may this generate screen? (sampler, hooks)
int cls_screen_level(const kh_model* m);    // 0 no screen, 1 the bf16 screen, 2 behind the int8 tier (hooks)
// dbg_lb / dbg_ub [vocab] (optional): receive every row's interval.  survivors: re-screen what the k_cls_screen_q8
// launch in front of this one left (kh_cls_screen.h) instead of scanning every row
void launch_cls_screen(kh_model* m, float* dbg_lb = nullptr, float* dbg_ub = nullptr, bool survivors = false);
void launch_cls_screen_q8(kh_model* m, float* dbg_lb = nullptr, float* dbg_ub = nullptr, int grid = 0);
int cls_screen_q8_selftest(kh_model* m, int32_t* d_flag, bool inject, int* result);
void launch_sample_screen(kh_model* m, int advance, int n_forced);
int cls_refresh_logits(kh_model* m);  // k_cls on the saved input if the logits buffer is stale
int cls_screen_selftest(kh_model* m, int32_t* d_flag, bool inject, int* result);
// ---- kh_model_w16.hip -----------------------------------------------------------------------
// Launch classes that run on the copy for a geometry (KH_W16_* bits, 0: not applicable) and the copy's bytes (host-only)
int plan_w16(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size, int layer_num, size_t* bytes);
// Launch classes whose GEMM-pass GEMMs run on the bf16 matrix cores for a geometry (KH_W16_* bits; host-only): the
// adoption mask among the classes whose contraction length is a multiple of 32; 0 for int8 and for geometries the
// GEMM prefill does not run on
int plan_gemm16(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size);
// the copy, once the weights are resident and ahead of the self-tests (no-op unless KH_FLAG_W16 / KH_W16=1 asks)
int w16_create(kh_model* m);
void w16_release(kh_model* m);  // frees the copy; no class runs on it afterwards
// The twins of the image's launches on a copy (on: KH_ON_W16 or KH_ON_Q4): `a` as the image's launch fills it, the
// matrices replaced by their copies.  One text for every source (kh_copy_launch.h); routed here to the translation
// unit that compiles the source's kernels - kh_model_w16.hip (bf16), kh_model_h16.hip (fp16), kh_model_q4.hip.
void copy_launch_qkv(kh_model* m, int l, KhOn on, const KhQkvArgs& a);
void copy_launch_wo(kh_model* m, int l, KhOn on, const KhGemvResArgs& a);
void copy_launch_wo_comb(kh_model* m, int l, KhOn on, const KhWoCombArgs& a);
void copy_launch_ffn13(kh_model* m, int l, KhOn on, const KhFfn13Args& a);
void copy_launch_w2(kh_model* m, int l, KhOn on, const KhGemvResArgs& a);
void copy_launch_cls(kh_model* m, KhOn on, const KhClsArgs& a);
// ---- kh_model_q4.hip ------------------------------------------------------------------------
// Launch classes that run on the 4-bit copy for a geometry (KH_W16_* bits, 0: not applicable) and the copy's bytes
// (host-only)
int plan_q4(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size, int layer_num, int group_size, size_t* bytes);
// the copy, once the weights are resident and ahead of the self-tests (no-op unless KH_FLAG_Q4 / KH_Q4=1 asks)
int q4_create(kh_model* m);
void q4_release(kh_model* m);  // frees the copy; every class is back on what a model without the flag launches
// ---- kh_model_load.hip ----------------------------------------------------------------------
// Make rows [0, rows) of the K / V cache usable before anything that touches them is enqueued: every layer, or one
// (layer >= 0).  No-op for rows that are mapped already and for caches that are plainly allocated.  Newly mapped
// memory is zeroed on the model's stream.
int kv_ensure(kh_model* m, int rows, int layer = -1);
int kv_ensure_rows(kh_model* m, int row0, int row_end);  // rows [row0, row_end) of every layer (a sequence slot's)
// ---- kh_model_selftest.hip ------------------------------------------------------------------
// ring kernels vs register tiles, fence-free vs fenced split merge: once at the end of kh_model_create_*
int run_selftests(kh_model* m);
// ---- kh_model_prefill.hip -------------------------------------------------------------------
bool prefill_supported(const kh_model* m);  // B-token VALU path
// kh_model_prefill without the token record (hist_write)
int prefill_run(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0);
// Full-depth passes (kh_model_score, kh_model_verify): the geometries they run on, and the tokens of one pass
bool full_depth_supported(const kh_model* m);
int verify_width(const kh_model* m);
// the buffers of a verify pass that reaches cache rows [0, rows): before the first verify_enqueue of a call.  as_set:
// of a pass under the model's settings - the row counters too, where the settings need them
// fsm (with as_set, while the constraint is on): the rows' state words as well
int verify_prepare(kh_model* m, int rows, bool as_set = false, bool fsm = false);
// One verify pass of toks[0 .. n), 1 <= n <= verify_width, at positions pos0 ..: the full-depth pass, k_pf_cls,
// k_spec_pick, k_spec_accept and the copy of the result block into m->h_spec_pin {a, pick[0 .. n)}, all enqueued on the
// model stream; the caller synchronises before it reads the block.  Arguments are the caller's to check.
// as_set: the picks are made under the model's sampler, penalties, logit bias and log-probs - where any of them is on,
// k_spec_hist, k_spec_tail and k_spec_accept_set take the place of the last two launches; where none is, nothing changes.
// fsm (with as_set, while the constraint is on): the pass under the constraint as well - k_spec_fsm_rows (k_spec_hist's
// duty is part of it), k_spec_tail_fsm and k_spec_accept_fsm, whatever else is set; the model's state word follows.
int verify_enqueue(kh_model* m, const int32_t* toks, int n, int pos0, bool as_set = false, bool fsm = false);
// Sequence slots (kh_model_seq.hip drives these; arguments are the caller's to check).  seq_prepare: the buffers of
// a pass, before the first enqueue of a call.  seq_prefill_enqueue: kh_model_prefill's passes for n tokens at
// positions pos0 .. of the sequence whose position 0 is cache row row0.  seq_pass_enqueue: one full-depth pass over
// lanes [0, n) (entries >= n are padded here) - k_seq_embed from d_seq_tok, k_seq_qkv, k_seq_attn, the prefill
// kernels, k_pf_cls, k_seq_pick; picks land in d_seq_tok[slot] and, with words, in d_seq_words[row].  With a tail
// description the pass ends in k_seq_tail instead of k_seq_pick: per-slot processing on the tables seq_prepare_ex
// made (uploaded by the caller), the pick, and with top_n >= 0 the record of every lane's row.
struct KhSeqTail {
  int top_n;                 // -1: no records
  const KhProcParams* proc;  // [KH_SEQ_SLOTS_MAX]
  const int32_t* bias_ids;   // [KH_SEQ_SLOTS_MAX][KH_SEQ_BIAS_MAX]
  const float* bias;
  int32_t* cnt;              // [KH_PF_BMAX][vocab]
  KhFsmRef fsm;              // a lane's slot is constrained: the pass ends in k_seq_tail_fsm (else both null)
};
// The device form of an automaton (kh_model_set_constraint, kh_model_seq_set_constraint): the mask-size check and the
// mask rows on the host, new buffers (and, the first time, the descriptor and n_state_words state words) - nothing of
// the model is touched, a failure leaves it as it was.  fsm_install: the uploads and the descriptor on the model
// stream, a sync, then the buffers replace f's; on an error they are kept alive in f too (the descriptor may name
// them) and the caller turns its constraint off.  The state words are the caller's to write, ahead of fsm_install.
struct FsmStage {
  KhDev<KhFsmDev> desc;
  KhDev<int32_t> state, tokens, next;
  KhDev<uint32_t> mask;
  KhDev<int64_t> row_ptr;
  std::vector<uint32_t> h_mask;
  std::vector<int64_t> h_row_ptr;
  std::vector<int32_t> h_tokens;
  size_t stride = 0;
};
int fsm_stage(kh_model* m, const kh_fsm* a, const kh_model::Fsm& f, size_t n_state_words, FsmStage* st);
int fsm_install(kh_model* m, const kh_fsm* a, kh_model::Fsm& f, FsmStage& st);
int seq_prepare(kh_model* m);
int seq_prepare_ex(kh_model* m, bool records);  // behind seq_prepare: the tables of k_seq_tail, the record buffers
int seq_prefill_enqueue(kh_model* m, int row0, const int32_t* toks, int n, int pos0, int pfx_len = 0, int pfx_row0 = 0);
int seq_pass_enqueue(kh_model* m, KhSeqLanes lanes, int n, bool words, const KhSeqTail* tail = nullptr);
// the two ends of a pass that do not care how its logits and q rows were made, for lanes [0, n) of a full table: the
// attention of layer l on q / out rows of dim floats per lane (k_seq_attn, k_seq_attn_pfx where a lane shares a
// prefix; the B-token pass's workspace), and the tail on logits rows [n][pf_vstride] (k_seq_pick, or k_seq_tail)
void seq_attn_enqueue(kh_model* m, int l, const float* q, float* out, const KhSeqLanes& lanes, int n);
int seq_tail_enqueue(kh_model* m, float* logits, const KhSeqLanes& lanes, int n, bool words, const KhSeqTail* tail);
// fill_attn(m, l, 0, m->attn_fenced) as the arguments of a multi-token slice (launch_attn_decode with tokens > 1,
// launch_seq_attn[_pfx]): token t's q / out rows at q / out + t * dim, its split workspace at ws + t * ws_tok_bytes
KhAttnArgs attn_slice_args(kh_model* m, int l, const float* q, float* out, void* ws, size_t ws_tok_bytes);
// ---- kh_model_gemm.hip ----------------------------------------------------------------------
bool pg_supported(const kh_model* m);  // MFMA GEMM path
// the >48 KiB dynamic-LDS opt-in of a GEMM-pass kernel, once per (device, kernel); false: refused
bool pg_lds_opt_in(const void* kern, size_t lds);
// ---- kh_model_gemm_w16.hip ------------------------------------------------------------------
struct PgW16Launch {  // one GEMM of a pass as pg_gemm planned it, on the k_*_gemm_w16 kernels (kh_gemm_w16.h)
  int epi, R, NT;     // KH_PG_*; a listed (R, NT) register tile
  dim3 grid;
  int wg;
  size_t lds;
};
// a: the image launch's arguments with KhLin::w of every matrix pointing into the 16-bit copy.  tiles / lanes: the
// token addressing (both null: a run).  false: the LDS opt-in was refused (nothing launched)
bool pg_gemm_w16_launch(const PgW16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
                        const KhWideLanes* lanes);
// ---- kh_model_gemm_q16.hip ------------------------------------------------------------------
// the same launch on the k_*_gemm_q16 kernels (kh_gemm_q16.h): a is the int8 image launch's own.  The stem has no (2,8)
// register tile: the caller plans without it
bool pg_gemm_q16_launch(const PgW16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
                        const KhWideLanes* lanes);
// classes that run on it by default for a geometry (0: not an int8 group-64 model the GEMM prefill takes)
int plan_gemm16_q8(bool quant, int group_size, int dim, int hidden_dim, int kv_dim, int vocab_size);
void gemm16_q8_configure(kh_model* m);  // at creation
// kh_model_prefill_gemm without the token record (hist_write); prefill_gemm_prepare: its slabs, made by the call
// itself or ahead of it by whoever times it
int prefill_gemm_run(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0);
int prefill_gemm_prepare(kh_model* m);
// The GEMM prefill into sequence slots (kh_seq_prefill.h; kh_model_seq_prefill_gemm).  _check: KH_OK where the pass
// runs - the GEMM prefill's geometries with an MFMA attention instantiation for the head size and KH_PG_ATTN not 0 -,
// else KH_ERR_UNSUPPORTED.  _enqueue: the planned passes (kh_rg_plan) for segment s = n_tokens[s] tokens of the
// concatenated toks at positions pos0[s] .. of slot slots[s]; it makes the slabs.  Arguments and the slots' rows
// (ensure_slot_rows) are the caller's to check.
int seq_prefill_gemm_check(const kh_model* m);
int seq_prefill_gemm_enqueue(kh_model* m, int n_seq, const int32_t* slots, const int32_t* toks, const int32_t* n_tokens,
                             const int32_t* pos0);
// The wide sequence pass (kh_seq_gemm.h): up to KH_SEQ_SLOTS_MAX lanes of distinct slots at full depth with the four
// weight GEMMs and the classifier on the matrix cores; lane i feeds d_seq_tok[slots[i]] at position pos[i].  Picks
// land as seq_pass_enqueue's.  seq_gemm_supported: the geometries it runs on; seq_gemm_prepare: its buffers, behind
// seq_prepare and before the first enqueue of a call.
bool seq_gemm_supported(const kh_model* m);
int seq_gemm_prepare(kh_model* m);
int seq_pass_enqueue_gemm(kh_model* m, const int32_t* slots, const int32_t* pos, int n, bool words,
                          const KhSeqTail* tail = nullptr);
}  // namespace khm
