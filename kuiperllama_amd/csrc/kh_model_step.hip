// kh_model_step.hip — the decode step of the model level: launch shapes, the fused (5L+2 launches)
// and unfused (the reference's own sequence) step, hipGraph capture, predict and the generate loop.
// Replaces, for the decode path,
//   LLama2Model::forward / predict                         kuiper/source/model/llama3.cpp:147-167, 642-650
//   generate()                                             demo/main.cpp:5-47
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "kh_dispatch.h"
#include "kh_fused.h"
#include "kh_fused_ring.h"
#include "kh_sample.h"
#include "kh_logprobs.h"
#include "kh_lookup.h"
#include "kh_model_internal.h"

namespace khm {

// (The instantiation lists of the kernels launched below - FusedU, GemvResU, FusedMV, ... - and pick_fused are in
// kh_dispatch.h: kh_model_w16.hip launches the W16 twins of these kernels from the same lists.)

// Launch shape of one GEMV: rows are processed as `pairs` work items of two M-long rows.
//  split: waves sharing a pair (1/2/4) — raised while the launch has < 4096 waves and each wave
//         would still stream >= 8 KiB (fp32) / 4 KiB (int8);
//  u    : 16-byte loads per row per lane in flight (covers the wave's column range when it can);
//  grid : workgroups, <= 1024 (4 per CU), chosen so every wave gets the same number of items.
kh_model::Shape pick_shape(bool quant, int pairs, int M, int max_split, const char* env, int wg,
                           int wg_max, bool many_waves, bool u3) {
  kh_model::Shape sh;
  sh.wg = wg;
  // tuning hook (tools/sweep_shapes.py): KH_SHAPE_<K>="split,u,grid[,wg]" overrides the heuristic
  if (const char* ov = env ? dbg(env) : nullptr) {
    int sp = 0, u = 0, g = 0, w = wg;
    const int nf = sscanf(ov, "%d,%d,%d,%d", &sp, &u, &g, &w);
    const bool u_ok = u3 ? (quant ? GemvResU<true>::has(u) : GemvResU<false>::has(u))
                         : (quant ? FusedU<true>::has(u) : FusedU<false>::has(u));
    if (nf >= 3 && GemvResSP::has(sp) && sp <= max_split && u_ok && g >= 1 && g <= 4096 &&
        (w == 256 || (w == 512 && wg_max >= 512))) {
      sh.split = sp;
      sh.u = u;
      sh.grid = g;
      sh.wg = w;
      return sh;
    }
    // not a launch this kernel has (e.g. split 4 for qkv, u 8 for int8, wg 512 where the kernel stays at 256):
    // say so rather than let a test believe it forced a shape
    fprintf(stderr, "[kh] %s=\"%s\" rejected (split <= %d, u 2/4%s%s, grid 1..4096, wg 256%s): heuristic shape\n",
            env, ov, max_split, quant ? "" : "/8", quant && u3 ? "/3" : "", wg_max >= 512 ? "/512" : "");
  }
  const int elem = quant ? 1 : 4;
  const int min_bytes = quant ? 4096 : 8192;  // bytes one wave must still stream per pair
  const long pair_bytes = 2L * M * elem;
  // waves to aim for before rows are split.  gemv_pairs walks a wave's tiles (pair, chunk) in ONE loop and
  // requests the next tile in a burst right after the current tile's FMAs (kh_fused.h: ROLL = false everywhere but
  // the int8 QKV kernel), so a wave that walks several chunks of a long row keeps loads in flight across them and
  // fewer, longer-lived waves beat many short ones (r3 sweeps, profiles/r3_shape_sweep.txt: Llama-2-7B w2 int8
  // split 4 -> 2: 12.6 -> 10.8 us, fp32 33.6 -> 31.4; wo int8 split 2 -> 1: 5.6 -> 5.25); rounds 1-2 aimed at
  // twice as many.
  const int target_waves = pair_bytes >= 16384 ? 4096 : 2048;
  while (sh.split < max_split && pairs * sh.split < target_waves &&
         pair_bytes / (sh.split * 2) >= min_bytes)
    sh.split *= 2;
  const int Mc = quant ? M / 16 : M / 4;
  const int per_lane = ((Mc + sh.split - 1) / sh.split + KH_WAVE - 1) / KH_WAVE;
  if (quant) {
    // one chunk when it covers the column range; ranges that need several chunks anyway take the
    // small one (less padding in the last chunk, finer refill: w2 int8 u4 -> u2 11.9 -> 10.8 us)
    sh.u = per_lane > 4 ? 2 : (per_lane >= 3 ? 4 : 2);
    // [r6] w2 only (u3): a column range of 5 or 6 loads per lane as TWO exact tiles of 3 instead of three tiles of
    // 2 - Llama-2-7B int8's w2 (5.4 loads per lane): 10.45 -> 10.25 us, +0.4 % tok/s, four alternations on one box
    // (profiles/r6_w2_u3_ab.txt); ONE tile of 6 is slower (10.95 us: the whole item requested in one burst)
    if (u3 && per_lane > 4 && per_lane <= 6) sh.u = 3;
  } else {
    sh.u = per_lane >= 8 ? 8 : (per_lane >= 3 ? 4 : 2);
  }
  const int ppw = (wg / KH_WAVE) / sh.split;  // pairs per workgroup per iteration
  const int need = (pairs + ppw - 1) / ppw;
  // every workgroup re-stages the M-float input vector from L2: keep that below ~75 % of the
  // weight bytes (matters for w2, whose input is the hidden-sized vector; sweep in
  // profiles/r1_shape_sweep.md), and never more than 4 workgroups per CU
  long cap = (long)(0.75 * (double)pairs * (double)pair_bytes / ((double)M * 4.0));
  const long cap_hi = 1024L * KH_WG / wg, cap_lo = 256L * KH_WG / wg;  // 4 .. 1 x 256 threads / CU
  if (cap > cap_hi) cap = cap_hi;
  if (cap < cap_lo) cap = cap_lo;
  if (need <= cap) {
    sh.grid = need;
  } else {
    // several iterations per workgroup: keep the grid a whole number of workgroups per CU (256
    // CUs; 384- or 688-wide grids measured 5-10 % slower than their balanced neighbours) and
    // minimise the per-CU critical path (g/256)*ceil(need/g).  Ties: the many-row matrices
    // (qkv, ffn13, cls) prefer 8 resident waves per CU, then 12, 16 -- fewer, longer-lived
    // workgroups re-stage x less often; the few-long-row matrices (wo, w2: one or two chunks
    // per wave) prefer 16 -- everything is in flight at once (profiles/r1_shape_sweep.md).
    const int wpw = wg / KH_WAVE;           // waves per workgroup
    // resident waves per CU, in order of preference
    const int pref_lo[4] = {8, 12, 16, 4}, pref_hi[4] = {16, 12, 8, 4};
    long best_cost = -1;
    for (int wv : (many_waves ? pref_hi : pref_lo)) {
      if (wv == 4 && best_cost >= 0) break;  // 4 waves per CU only when nothing else fits
      if (wv % wpw) continue;
      const long g = 256L * (wv / wpw);
      if (g > cap) continue;
      const long cost = g * ((need + g - 1) / g);
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        sh.grid = (int)g;
      }
    }
    if (best_cost < 0) sh.grid = (int)cap;
  }
  return sh;
}

// ---- fused launches -------------------------------------------------------------------------
KhQkvArgs fill_qkv(kh_model* m, int l) {
  const kh_config& c = m->cfg;
  const LayerW& W = m->layers[l];
  KhQkvArgs a;
  a.x = m->x;
  a.att_norm = W.att_norm;
  a.wq = W.wq;
  a.wk = W.wk;
  a.wv = W.wv;
  a.q_out = m->q;
  a.kcache_layer = m->kcache + (size_t)l * c.cache_len * c.kv_dim;
  a.vcache_layer = m->vcache + (size_t)l * c.cache_len * c.kv_dim;
  a.d_pos = m->d_pos;
  a.sin_cache = m->sin_cache;
  a.cos_cache = m->cos_cache;
  a.dim = c.dim;
  a.kv_dim = c.kv_dim;
  a.head_size = c.head_size;
  a.rope_mode = c.rope_mode;
  a.gshift = m->gshift;
  a.eps = c.rms_eps;
  return a;
}
void launch_qkv(kh_model* m, int l, KhOn on) {
  const kh_config& c = m->cfg;
  const KhQkvArgs a = fill_qkv(m, l);
  if (on != KH_ON_IMAGE) return copy_launch_qkv(m, l, on, a);  // the same shape on a weight copy (kh_model_w16.hip)
  const kh_model::Shape& sh = m->sh_qkv;
  pick_fused<FusedU, FusedMV, QkvSP>(c.is_quant, sh.u, kh_stage_maxv(c.dim, sh.wg), sh.split,
                                     [&](auto Q, auto U, auto MV, auto SP) {
    kh_launch(KH_KERNEL(k_qkv, Q, U, MV, SP), sh.grid, sh.wg, fused_lds_bytes(Q, c.dim), m->stream, a);
  });
}
KhAttnArgs fill_attn(kh_model* m, int l, int variant, bool fenced) {
  const kh_config& c = m->cfg;
  KhAttnArgs a;
  a.q = m->q;
  a.kcache_layer = m->kcache + (size_t)l * c.cache_len * c.kv_dim;
  a.vcache_layer = m->vcache + (size_t)l * c.cache_len * c.kv_dim;
  a.out = m->att;
  a.d_pos = m->d_pos;
  a.kv_dim = c.kv_dim;
  a.kv_mul = c.kv_mul;
  a.head_size = c.head_size;
  a.kv_heads = c.kv_head_num;
  a.nsplit = m->attn_ns;
  a.ws = m->attn_ws;
  a.ws_stride = m->attn_ws_stride;
  // step variants 1 and 2 cover positions below the group path's threshold only (step_variant): launch the
  // per-head-only instantiation, whose register count leaves room for two 512-thread workgroups per CU
  a.nsplit_g = variant != 0 ? 0 : m->attn_ns_g;
  a.t_long = m->attn_t_long;
  a.ts_shift = m->attn_ts_shift;
  a.defer = variant == 1 ? 1 : 0;
  a.fenced = fenced ? 1 : 0;
  a.tok_stride = 0;
  a.ws_tok_bytes = 0;
  return a;
}
int attn_group_lanes(const kh_config& c) {
  int G = 1;
  while (G < c.head_size / 4) G <<= 1;
  return G < 16 ? 16 : G;
}
void launch_attn(kh_model* m, int l, int variant, bool fenced) {
  const kh_config& c = m->cfg;
  const KhAttnArgs a = fill_attn(m, l, variant, fenced);
  const int wg = m->attn_wg;
  if (c.head_size > 32)
    launch_attn_decode(a, 0, wg, m->stream);
  else {  // head_size <= 32: generic LDS-score kernel (tiny test models)
    launch_log("k_attn_generic");
    hipLaunchKernelGGL(k_attn_generic, dim3(c.head_num), dim3(wg),
                       attn_lds_bytes(c.head_size, wg), m->stream, a);
  }
}
KhGemvResArgs fill_wo(kh_model* m, int l) {
  const kh_config& c = m->cfg;
  KhGemvResArgs a;
  a.vec = m->att;
  a.w = m->layers[l].wo;
  a.x = m->x;
  a.M = c.dim;
  a.K = c.dim;
  a.gshift = m->gshift;
  return a;
}
void launch_wo(kh_model* m, int l, int variant, KhOn on) {
  const kh_config& c = m->cfg;
  const kh_model::Shape& sh = m->sh_wo;
  if (variant == 1) {  // behind a deferring attention launch: in-register staging of 2 or 4 float4
    KhWoCombArgs a;
    a.g = fill_wo(m, l);
    const AttnSplitWs ws = attn_ws_carve(m->attn_ws, c.head_num, c.head_size, m->attn_ws_stride);
    a.cb.ml = ws.ml;
    a.cb.o = ws.o;
    a.cb.d_pos = m->d_pos;
    a.cb.ns = m->attn_ns;
    a.cb.ts_shift = m->attn_ts_shift;
    a.cb.nsw = m->attn_ws_stride;
    a.cb.heads = c.head_num;
    a.cb.hs = c.head_size;
    if (on != KH_ON_IMAGE) return copy_launch_wo_comb(m, l, on, a);
    pick_fused<FusedU, WoCombMV, GemvResSP>(c.is_quant, sh.u, c.dim <= 2 * 4 * sh.wg ? 2 : 4, sh.split,
                                            [&](auto Q, auto U, auto MV, auto SP) {
      kh_launch(KH_KERNEL(k_wo_comb, Q, U, MV, SP), sh.grid, sh.wg, comb_lds_bytes(Q, c.dim, c.head_num), m->stream, a);
    });
    return;
  }
  const KhGemvResArgs a = fill_wo(m, l);
  if (on != KH_ON_IMAGE) return copy_launch_wo(m, l, on, a);
  pick_fused<FusedU, FusedMV, GemvResSP>(c.is_quant, sh.u, kh_stage_maxv(c.dim, sh.wg), sh.split,
                                         [&](auto Q, auto U, auto MV, auto SP) {
    kh_launch(KH_KERNEL(k_gemv_res, Q, U, MV, SP), sh.grid, sh.wg, fused_lds_bytes(Q, c.dim), m->stream, a);
  });
}
void launch_ffn13(kh_model* m, int l, bool ring, KhOn on) {
  const kh_config& c = m->cfg;
  const LayerW& W = m->layers[l];
  KhFfn13Args a;
  a.x = m->x;
  a.ffn_norm = W.ffn_norm;
  a.w1 = W.w1;
  a.w3 = W.w3;
  a.h = m->h1;
  a.dim = c.dim;
  a.hidden = c.hidden_dim;
  a.gshift = m->gshift;
  a.eps = c.rms_eps;
  // Ahead of the ring branch: on the 4-bit copy the launch takes the ring launch's place (the copy has no ring form),
  // and a model with a 16-bit copy is fp32 and never has a ring plan (plan_ring returns an empty one unless quant)
  if (on != KH_ON_IMAGE) return copy_launch_ffn13(m, l, on, a);
  // the int8 LDS-DMA ring kernels (kh_fused_ring.h): 2 ring slots per wave, 4 float4 staged per thread, plain layout
  if (ring) {  // plan_ring: int8, dim a multiple of 256 floats and at most 16 per thread
    kh_launch(KH_KERNEL(k_ffn13_ring, 2, 4, false), m->ring.ffn_grid, KH_WG,
              ring_lds_bytes(c.dim, false, KH_WAVES_PER_WG, 2), m->stream, a);
    return;
  }
  const kh_model::Shape& sh = m->sh_ffn;
  pick_fused<FusedU, FusedMV, NoSP>(c.is_quant, sh.u, kh_stage_maxv(c.dim, sh.wg), 1, [&](auto Q, auto U, auto MV, auto) {
    kh_launch(KH_KERNEL(k_ffn13, Q, U, MV), sh.grid, sh.wg, fused_lds_bytes(Q, c.dim), m->stream, a);
  });
}
void launch_w2(kh_model* m, int l, KhOn on) {
  const kh_config& c = m->cfg;
  KhGemvResArgs a;
  a.vec = m->h1;
  a.w = m->layers[l].w2;
  a.x = m->x;
  a.M = c.hidden_dim;
  a.K = c.dim;
  a.gshift = m->gshift;
  if (on != KH_ON_IMAGE) return copy_launch_w2(m, l, on, a);
  const kh_model::Shape& sh = m->sh_w2;  // int8 u 3: two exact tiles of three loads per row (pick_shape, u3)
  pick_fused<GemvResU, GemvResMV, GemvResSP>(c.is_quant, sh.u, kh_stage_maxv(c.hidden_dim, sh.wg), sh.split,
                                             [&](auto Q, auto U, auto MV, auto SP) {
    kh_launch(KH_KERNEL(k_gemv_res, Q, U, MV, SP), sh.grid, sh.wg, fused_lds_bytes(Q, c.hidden_dim), m->stream, a);
  });
}
void launch_cls(kh_model* m, const ClsIo& io, bool ring, KhOn on) {
  const kh_config& c = m->cfg;
  if (io.logits == m->logits) logits_fresh(m);  // (enqueue_steps has the last word behind captured steps)
  KhClsArgs a;
  a.x = io.x;
  a.final_norm = m->final_norm;
  a.wcls = m->cls;
  a.logits = io.logits;
  a.part_val = io.part_val;
  a.part_idx = io.part_idx;
  a.dim = c.dim;
  a.vocab = c.vocab_size;
  a.gshift = m->gshift;
  a.eps = c.rms_eps;
  // ahead of the ring branch, as in launch_ffn13 (on the 4-bit copy m->nparts follows the launch: q4_create)
  if (on != KH_ON_IMAGE) return copy_launch_cls(m, on, a);
  // the classifier is int8 only when the model is quantised (untied; llama3.cpp:255-268)
  if (ring) {
    kh_launch(KH_KERNEL(k_cls_ring, 2, 4, false), m->ring.cls_grid, KH_WG,
              ring_lds_bytes(c.dim, false, KH_WAVES_PER_WG, 2), m->stream, a);
    return;
  }
  const kh_model::Shape& sh = m->sh_cls;
  pick_fused<FusedU, FusedMV, NoSP>(c.is_quant, sh.u, kh_stage_maxv(c.dim, sh.wg), 1, [&](auto Q, auto U, auto MV, auto) {
    kh_launch(KH_KERNEL(k_cls, Q, U, MV), sh.grid, sh.wg, cls_lds_bytes(Q, c.dim), m->stream, a);
  });
}
void launch_sample(kh_model* m, int advance, int n_forced, StepTail tail) {
  if (tail_screens(tail) && step_tail(m, 1) != kScreen) tail = step_tail(m, 1);  // processors or sampling on are stronger than "screen"
  const KhFsmRef fsm{m->fsm.desc, m->fsm.state};  // (the _fsm tails: both exist while a constraint is set)
  if (tail_screens(tail)) {
    launch_sample_screen(m, advance, n_forced);
  } else if (tail == kLogprob || tail == kLogprobFsm) {
    KhSampleLpArgs t;
    t.logits = m->logits;
    t.part_val = m->part_val;
    t.part_idx = m->part_idx;
    t.nparts = m->nparts;
    t.params = m->d_samp;
    t.proc = m->d_proc;
    t.bias_ids = m->d_bias_ids;
    t.bias = m->d_bias;
    t.hist = m->d_hist;
    t.hist_cap = m->hist_cap;
    t.cnt = m->d_cnt;
    t.top_n = m->d_lp_top_n;
    t.recs = lp_records(m);
    t.rec_cap = m->lp_cap;
    t.st = fill_step_tail(m, advance, n_forced);
    if (tail == kLogprobFsm) {
      launch_log("k_sample_lp_fsm");
      const KhSampleLpFsmArgs tf{fsm, t};
      hipLaunchKernelGGL(k_sample_lp_fsm, dim3(1), dim3(KH_SAMP_THREADS), 0, m->stream, tf);
      return;
    }
    launch_log("k_sample_lp");
    hipLaunchKernelGGL(k_sample_lp, dim3(1), dim3(KH_SAMP_THREADS), 0, m->stream, t);
  } else if (tail == kProcess || tail == kProcessFsm) {
    KhSampleProcArgs t;
    t.logits = m->logits;
    t.params = m->d_samp;
    t.proc = m->d_proc;
    t.bias_ids = m->d_bias_ids;
    t.bias = m->d_bias;
    t.hist = m->d_hist;
    t.hist_cap = m->hist_cap;
    t.cnt = m->d_cnt;
    t.st = fill_step_tail(m, advance, n_forced);
    if (tail == kProcessFsm) {
      launch_log("k_sample_proc_fsm");
      const KhSampleProcFsmArgs tf{fsm, t};
      hipLaunchKernelGGL(k_sample_proc_fsm, dim3(1), dim3(KH_SAMP_THREADS), 0, m->stream, tf);
      return;
    }
    launch_log("k_sample_proc");
    hipLaunchKernelGGL(k_sample_proc, dim3(1), dim3(KH_SAMP_THREADS), 0, m->stream, t);
  } else if (tail == kSample) {
    KhSampleTopArgs t;
    t.logits = m->logits;
    t.part_val = m->part_val;
    t.nparts = m->nparts;
    t.params = m->d_samp;
    t.st = fill_step_tail(m, advance, n_forced);
    launch_log("k_sample_topp");
    hipLaunchKernelGGL(k_sample_topp, dim3(1), dim3(KH_SAMP_THREADS), 0, m->stream, t);
  } else {
    KhSampleArgs a;
    a.part_val = m->part_val;
    a.part_idx = m->part_idx;
    a.nparts = m->nparts;
    a.st = fill_step_tail(m, advance, n_forced);
    hipLaunchKernelGGL(k_sample, dim3(1), dim3(KH_WG), 0, m->stream, a);
  }
}

// Which attention / wo pair the steps at positions pos_lo .. pos_hi launch (host decision, per captured
// graph or eager step).  Variant 1 (time splits merged by k_wo_comb) wherever the per-head path has more
// than one split to merge; variant 0 (the attention launch leaves the final vector) below position 256,
// where there is nothing to merge and wo keeps its plain staging, and from the first position of the GQA
// group path on, whose 32 splits per KV group are merged by their last arriver.  Every wo workgroup
// re-reads all nact partials (nact x dim floats from L2: 64 MB over the launch at 16 splits of a 2048-wide
// model, +3.3 us), so shapes whose staging cannot hide under wo's first weight tile (kh_fused.h:
// OVERLAP) defer only up to 4 splits (profiles/r4_attn_defer_ab.txt: Llama-2-7B int8 loses from 8 on).
int step_variant(const kh_model* m, int pos_lo, int pos_hi) {
  (void)pos_lo;
  if (pos_hi < KH_ATTN_MIN_TS) return 0;         // pos + 1 <= 256 everywhere: one split
  if (pos_hi + 1 >= m->attn_t_long) return 0;    // some step runs the group path
  if (m->attn_defer && attn_active_splits(pos_hi, m->attn_ns, m->attn_ts_shift) <= m->attn_defer_max) return 1;
  // Variant 2: the merge stays in the attention launch, but every step of the range is below the group path's
  // threshold, so the launch uses the per-head-only instantiation.  The one that also carries the group path needs
  // 138+ registers (two K/V batches in flight for kv_mul heads): one 512-thread workgroup per CU, which cost the 512
  // (head, split) workgroups at position 4094 +3.6 us per layer (profiles/r4_attn_pipe_ab.txt); per-head-only: 115.
  return m->attn_ns_g > 0 ? 2 : 0;
}
// one fused decode step = 5L + 2 launches.  ev (optional) receives an event after each launch.
void launch_step_fused(kh_model* m, int advance, int n_forced, hipEvent_t* ev, int variant, StepTail tail) {
  int e = 0;
  auto mark = [&]() {
    if (ev) (void)hipEventRecord(ev[e++], m->stream);
  };
  mark();
  for (int l = 0; l < m->cfg.layer_num; ++l) {
    launch_qkv(m, l);
    mark();
    launch_attn(m, l, variant, m->attn_fenced);
    mark();
    launch_wo(m, l, variant);
    mark();
    launch_ffn13(m, l, m->ring.ffn_r == 2);
    mark();
    launch_w2(m, l);
    mark();
  }
  if (tail == kScreenQ8) {
    launch_cls_screen_q8(m);  // the int8 tier, then the bf16 screen of what it left: 5L + 3 launches
    launch_cls_screen(m, nullptr, nullptr, /*survivors=*/true);
  } else if (tail == kScreen) {
    launch_cls_screen(m);  // k_cls's slot: still 5L + 2 launches
  } else {
    launch_cls(m);
  }
  mark();
  launch_sample(m, advance, n_forced, tail);
  mark();
}

// the reference's own launch sequence, one C-ABI op per reference kernel (llama3.cpp:147-167)
int launch_step_unfused(kh_model* m, int pos, bool process) {
  const kh_config& c = m->cfg;
  void* s = (void*)m->stream;
  int rc;
#define KH_TRY(x)          \
  if ((rc = (x)) != KH_OK) \
  return rc
  auto lin = [&](const KhLin& L, const float* in, float* out, int M, int K) -> int {
    int r = c.is_quant ? kh_matmul_q8(in, (const int8_t*)L.w, L.scales, c.group_size, out, M, K, s)
                       : kh_matmul_f32(in, (const float*)L.w, out, M, K, 1.f, s);
    if (r == KH_OK && L.bias) r = kh_add_f32(out, L.bias, out, K, s);  // matmul.cpp:74-77
    return r;
  };
  for (int l = 0; l < c.layer_num; ++l) {
    const LayerW& W = m->layers[l];
    float* krow = m->kcache + ((size_t)l * c.cache_len + pos) * c.kv_dim;
    float* vrow = m->vcache + ((size_t)l * c.cache_len + pos) * c.kv_dim;
    KH_TRY(kh_rmsnorm_f32(m->x, W.att_norm, m->rms, c.dim, c.rms_eps, s));
    KH_TRY(lin(W.wq, m->rms, m->q, c.dim, c.dim));
    KH_TRY(lin(W.wk, m->rms, krow, c.dim, c.kv_dim));
    KH_TRY(lin(W.wv, m->rms, vrow, c.dim, c.kv_dim));
    KH_TRY(kh_rope_f32(c.dim, c.kv_dim, c.head_size, m->q, krow, nullptr, pos, m->sin_cache,
                       m->cos_cache, c.rope_mode, s));
    KH_TRY(kh_mha_f32(nullptr, pos, c.head_num, l, c.cache_len, c.kv_dim, c.kv_mul, c.head_size,
                      m->att, m->q, m->score, m->kcache, m->vcache, s));
    KH_TRY(lin(W.wo, m->att, m->q /* kAttnOutput aliases kQuery, llama3.cpp:478-489 */, c.dim,
               c.dim));
    KH_TRY(kh_add_f32(m->x, m->q, m->x, c.dim, s));
    KH_TRY(kh_rmsnorm_f32(m->x, W.ffn_norm, m->rms, c.dim, c.rms_eps, s));
    KH_TRY(lin(W.w1, m->rms, m->h1, c.dim, c.hidden_dim));
    KH_TRY(lin(W.w3, m->rms, m->h3, c.dim, c.hidden_dim));
    KH_TRY(kh_swiglu_f32(m->h1, m->h3, m->h1, c.hidden_dim, s));
    KH_TRY(lin(W.w2, m->h1, m->w2o, c.hidden_dim, c.dim));
    KH_TRY(kh_add_f32(m->x, m->w2o, m->x, c.dim, s));
  }
  KH_TRY(kh_rmsnorm_f32(m->x, m->final_norm, m->x, c.dim, c.rms_eps, s));
  KH_TRY(lin(m->cls, m->x, m->logits, c.dim, c.vocab_size));
  logits_fresh(m);
  const bool fsm = process && m->fsm_on;
  if (fsm) {  // the row of the automaton state, ahead of the processors: k_token_mask reads the state word itself
    const int n4 = (c.vocab_size + 3) / 4, grid = (n4 + KH_WG - 1) / KH_WG;
    launch_log("k_token_mask");
    hipLaunchKernelGGL(k_token_mask, dim3(grid < 1024 ? grid : 1024), dim3(KH_WG), 0, m->stream, (float*)m->logits,
                       c.vocab_size, (const uint32_t*)nullptr, (const KhFsmDev*)m->fsm.desc, (const int32_t*)m->fsm.state);
    KH_TRY(kh_launch_status());
  }
  if (process && m->proc_on)  // d_hist[pos] is this step's own token (set_state)
    KH_TRY(kh_logit_process_f32(m->logits, c.vocab_size, m->d_hist, nullptr, pos, &m->pen, m->d_bias_ids, m->d_bias,
                                m->n_bias, m->d_cnt, s));
  if (m->samp_on) {  // the counter is the position whose logits are sampled, as in the fused step
    KH_TRY(kh_sample_f32(m->logits, c.vocab_size, &m->samp, pos, 1, m->d_next, s));
  } else {
    KH_TRY(kh_argmax_f32(m->logits, c.vocab_size, m->d_next, s));
  }
  if (fsm) {  // the state behind the pick
    launch_log("k_fsm_advance");
    hipLaunchKernelGGL(k_fsm_advance, dim3(1), dim3(KH_FSM_THREADS), 0, m->stream, (const KhFsmDev*)m->fsm.desc,
                       (int32_t*)m->fsm.state, (const int32_t*)m->d_next);
    KH_TRY(kh_launch_status());
  }
  if (process && m->lp_top_n >= 0) {  // the record of the position, from the logits the pick was made from
    KH_TRY(lp_none(m, pos, 1));       // (the entries behind top_n stay "none")
    KH_CHECK_HIP(hipMemcpyAsync(m->d_lp_token + pos, m->d_next, sizeof(int32_t), hipMemcpyDeviceToDevice, m->stream));
    KH_TRY(kh_logprobs_f32(m->logits, c.vocab_size, 1, m->d_next, m->lp_top_n, nullptr, m->d_lp_lp + pos,
                           m->d_lp_top_ids + (size_t)pos * KH_LOGPROBS_TOP, m->d_lp_top_lp + (size_t)pos * KH_LOGPROBS_TOP,
                           s));
  }
#undef KH_TRY
  return KH_OK;
}

void set_state(kh_model* m, int token, int pos) {
  hipLaunchKernelGGL(k_set_state, dim3(1), dim3(KH_WG), 0, m->stream, token, pos, m->d_token,
                     m->d_pos, m->tok_emb, m->x, m->cfg.dim, m->d_hist);
}
int hist_write(kh_model* m, const int32_t* h_tokens, int n, int pos0) {
  if (pos0 < 0 || n <= 0 || (int64_t)pos0 + n > m->hist_cap) return KH_ERR_RANGE;
  // pageable source: the sync keeps the caller's array alive for the upload
  KH_CHECK_HIP(hipMemcpyAsync(m->d_hist + pos0, h_tokens, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}

int lp_none(kh_model* m, int pos0, int n) { return m->lp_top_n < 0 ? KH_OK : lp_fill_none(m, pos0, n); }
int lp_fill_none(kh_model* m, int pos0, int n) {
  if (!m->d_lp_token || pos0 < 0 || pos0 >= m->lp_cap) return KH_OK;
  if (n > m->lp_cap - pos0) n = m->lp_cap - pos0;
  if (n <= 0) return KH_OK;
  const size_t k = KH_LOGPROBS_TOP;
  KH_CHECK_HIP(hipMemsetAsync(m->d_lp_token + pos0, 0xFF, sizeof(int32_t) * (size_t)n, m->stream));
  KH_CHECK_HIP(hipMemsetAsync(m->d_lp_lp + pos0, 0xFF, sizeof(float) * (size_t)n, m->stream));
  KH_CHECK_HIP(hipMemsetAsync(m->d_lp_top_ids + pos0 * k, 0xFF, sizeof(int32_t) * n * k, m->stream));
  KH_CHECK_HIP(hipMemsetAsync(m->d_lp_top_lp + pos0 * k, 0xFF, sizeof(float) * n * k, m->stream));
  return KH_OK;
}
int lp_ensure_records(kh_model* m) {
  if (m->d_lp_token) return KH_OK;
  const size_t cap = (size_t)m->cfg.cache_len, k = KH_LOGPROBS_TOP;
  KhDev<int32_t> w, tok, ids;
  KhDev<float> lp, tlp;
  int rc;
  if ((rc = w.alloc(1)) != KH_OK || (rc = tok.alloc(cap)) != KH_OK || (rc = lp.alloc(cap)) != KH_OK ||
      (rc = ids.alloc(cap * k)) != KH_OK || (rc = tlp.alloc(cap * k)) != KH_OK)
    return rc;
  // every record "none"
  KH_CHECK_HIP(hipMemsetAsync(tok, 0xFF, sizeof(int32_t) * cap, m->stream));
  KH_CHECK_HIP(hipMemsetAsync(lp, 0xFF, sizeof(float) * cap, m->stream));
  KH_CHECK_HIP(hipMemsetAsync(ids, 0xFF, sizeof(int32_t) * cap * k, m->stream));
  KH_CHECK_HIP(hipMemsetAsync(tlp, 0xFF, sizeof(float) * cap * k, m->stream));
  m->d_lp_top_n = std::move(w);
  m->d_lp_token = std::move(tok);
  m->d_lp_lp = std::move(lp);
  m->d_lp_top_ids = std::move(ids);
  m->d_lp_top_lp = std::move(tlp);
  m->lp_cap = (int)cap;
  return KH_OK;
}
int lp_read(kh_model* m, int pos0, int n, int top_w, int32_t* h_token, float* h_lp, int32_t* h_top_ids,
            float* h_top_lp) {
  return kh_api_guard([&]() -> int {
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    const size_t k = KH_LOGPROBS_TOP, w = top_w > 0 ? (size_t)top_w : 0;
    std::vector<int32_t> ids(h_top_ids && w ? (size_t)n * k : 0);
    std::vector<float> tlp(h_top_lp && w ? (size_t)n * k : 0);
    if (h_token)
      KH_CHECK_HIP(hipMemcpyAsync(h_token, m->d_lp_token + pos0, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, m->stream));
    if (h_lp)
      KH_CHECK_HIP(hipMemcpyAsync(h_lp, m->d_lp_lp + pos0, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, m->stream));
    if (!ids.empty())
      KH_CHECK_HIP(hipMemcpyAsync(ids.data(), m->d_lp_top_ids + pos0 * k, sizeof(int32_t) * ids.size(), hipMemcpyDeviceToHost, m->stream));
    if (!tlp.empty())
      KH_CHECK_HIP(hipMemcpyAsync(tlp.data(), m->d_lp_top_lp + pos0 * k, sizeof(float) * tlp.size(), hipMemcpyDeviceToHost, m->stream));
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    for (size_t r = 0; r < (size_t)n; ++r) {  // the records' stride -> the caller's
      if (!ids.empty()) memcpy(h_top_ids + r * w, ids.data() + r * k, sizeof(int32_t) * w);
      if (!tlp.empty()) memcpy(h_top_lp + r * w, tlp.data() + r * k, sizeof(float) * w);
    }
    return KH_OK;
  });
}

int ensure_chunk_events(kh_model* m) {
  for (auto& e : m->ev_chunk)
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return (int)hipErrorUnknown;
  return KH_OK;
}
int ensure_pinned_words(kh_model* m, int n) {
  int rc;
  if ((rc = ensure_chunk_events(m)) != KH_OK) return rc;
  if (n <= (int)m->h_words_pin.size()) return KH_OK;
  KhPin<int32_t> pin;  // the old mirror stays until the new one exists
  if ((rc = pin.alloc((size_t)n)) != KH_OK) return rc;
  m->h_words_pin = std::move(pin);
  return KH_OK;
}

int ensure_seq_cap(kh_model* m, int n) {
  if (n <= m->seq_cap) return KH_OK;
  KhPin<int32_t> pin;
  KhDev<int32_t> forced, words;
  int rc;
  if ((rc = pin.alloc((size_t)n + 1)) != KH_OK || (rc = forced.alloc((size_t)n + 1)) != KH_OK ||
      (rc = words.alloc((size_t)n + 1)) != KH_OK)
    return rc;
  // forced[i] = -1 (0xFFFFFFFF): every position sampled, until a generate uploads its prompt
  KH_CHECK_HIP(hipMemsetAsync(forced, 0xFF, sizeof(int32_t) * ((size_t)n + 1), m->stream));
  // the graphs captured the old pointers and capacity: they go first, then the buffers they read (nothing of the
  // model has changed on any way out above)
  destroy_step_graphs(m);
  m->h_forced_pin = std::move(pin);
  m->d_forced = std::move(forced);
  m->d_words = std::move(words);
  m->forced_hwm = 0;
  m->forced_in_flight = false;
  m->seq_cap = n;
  return KH_OK;
}
void destroy_step_graphs(kh_model* m) {
  for (auto& per_sampler : m->sg)
    for (int v = 0; v < KH_STEP_VARIANTS; ++v)
      for (int k = 0; k < 4; ++k) {
        kh_model::StepGraph& sg = per_sampler[v][k];
        if (sg.e) (void)hipGraphExecDestroy(sg.e);
        if (sg.g) (void)hipGraphDestroy(sg.g);
        sg = kh_model::StepGraph{};
      }
}

int capture_steps(kh_model* m, int n_forced, int steps, int variant, StepTail tail, hipGraph_t* g, hipGraphExec_t* ge) {
  KH_CHECK_HIP(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < steps; ++i) launch_step_fused(m, /*advance=*/1, n_forced, nullptr, variant, tail);
  hipError_t e = hipStreamEndCapture(m->stream, g);
  if (e != hipSuccess) return (int)e;
  KH_CHECK_HIP(hipGraphInstantiate(ge, *g, nullptr, nullptr, 0));
  return KH_OK;
}
int step_graph(kh_model* m, int n_forced, int variant, int nsteps, StepTail tail, hipGraphExec_t* out) {
  if (variant < 0 || variant >= KH_STEP_VARIANTS) return KH_ERR_INVALID_ARG;
  const int k = nsteps == 1 ? 0 : nsteps == 2 ? 1 : nsteps == 4 ? 2 : nsteps == KH_GRAPH_STEPS ? 3 : -1;
  if (k < 0) return KH_ERR_INVALID_ARG;
  kh_model::StepGraph& sg = m->sg[tail][variant][k];
  if (!sg.e) {
    const int rc = capture_steps(m, n_forced, nsteps, variant, tail, &sg.g, &sg.e);
    if (rc != KH_OK) return rc;
    // push the executable graph to the device now: otherwise its FIRST launch pays for it (a 20-step run behind a
    // 5-step warm-up launched its 8-step graph for the first time inside the timed region: 1037-1046 tok/s by wall
    // clock where repeated runs gave 1060)
    (void)hipGraphUpload(sg.e, m->stream);
  }
  *out = sg.e;
  return KH_OK;
}
int enqueue_steps(kh_model* m, int pos, int nsteps, int n_forced, StepTail tail, int exec) {
  const int variant = step_variant(m, pos, pos + nsteps - 1);
  if (exec == KH_EXEC_GRAPH) {
    hipGraphExec_t ge = nullptr;
    const int rc = step_graph(m, n_forced, variant, nsteps, tail, &ge);
    if (rc != KH_OK) return rc;
    KH_CHECK_HIP(hipGraphLaunch(ge, m->stream));
  } else {
    for (int i = 0; i < nsteps; ++i) launch_step_fused(m, /*advance=*/1, n_forced, nullptr, variant, tail);
  }
  // behind screened steps the logits buffer is as old as the last full classifier launch
  m->scr.stale = tail_screens(tail);
  return KH_OK;
}

void plan_decode_shapes(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size,
                        kh_model::Shape (&out)[5]) {
  out[0] = pick_shape(quant, (dim + 2 * kv_dim) / 2, dim, 2, "KH_SHAPE_QKV", KH_WG, KH_WG_MAX);
  out[1] = pick_shape(quant, dim / 2, dim, 4, "KH_SHAPE_WO", KH_WG, KH_WG_MAX, true);
  out[2] = pick_shape(quant, hidden_dim, dim, 1, "KH_SHAPE_FFN", KH_WG, KH_WG_MAX);
  // w2 re-stages the hidden-sized input in every workgroup: 512-thread workgroups halve that
  // L2 -> LDS traffic for the same number of waves (measured 14.1 -> 11.8 us on Llama-3.2-1B)
  out[3] = pick_shape(quant, dim / 2, hidden_dim, 4, "KH_SHAPE_W2", KH_WG_MAX, KH_WG_MAX, true, /*u3=*/true);
  out[4] = pick_shape(quant, (vocab_size + 1) / 2, dim, 1, "KH_SHAPE_CLS", quant ? KH_WG : KH_WG_MAX, KH_WG_MAX);
}

// The int8 ffn13 and classifier launches run on the LDS-DMA ring kernels (kh_fused_ring.h) when the geometry fits
// them: at most 16 floats of the input vector per staging thread (the MAXV = 4 staging of the 256-thread kernels,
// which the ring kernels reproduce bit for bit), a power-of-two group of at least 16 weights (one scale per lane and
// piece).  Same-box A/B on Llama-2-7B int8, 32 distinct slabs per
// graph (tools/mb_q8ring.hip, profiles/r5_int8_ring_ab.txt): ffn13 17.7-17.9 -> 16.6-16.7 us (-6...-7 %), cls
// 24.35 -> 23.5 (-3.5 %); qkv +0.7 %, w2 -1.3 %, wo +5.8 % - those three stay on the register-tile kernels.
// Two ring slots per wave and two 256-thread workgroups per CU measured best (deeper rings and more waves per CU
// are slower: 3 slots +1 %, 4 slots +5 %, three workgroups per CU +3 %).  KH_RING=0 turns the ring kernels off.
void plan_ring(bool quant, int dim, int hidden_dim, int vocab_size, int group_size, kh_model::RingPlan* out) {
  *out = kh_model::RingPlan();
  if (!quant || dbg_off("KH_RING")) return;
  if (dim % 16 != 0 || !kh_stage_fits4(dim, KH_WG)) return;
  if (group_size < 16 || (group_size & (group_size - 1)) != 0 || dim % group_size != 0) return;
  if (ring_lds_bytes(dim, false, KH_WAVES_PER_WG, 2) > 64 * 1024) return;  // no dynamic-LDS opt-in on this path
  auto grid_of = [](int items) {
    const int need = (items + KH_WAVES_PER_WG - 1) / KH_WAVES_PER_WG;
    return need < 512 ? need : 512;
  };
  // a KH_SHAPE_FFN / KH_SHAPE_CLS hook asks for a specific register-tile launch: honour it (the B-token prefill
  // follows the same hook, and its bit-identity with decode needs the same workgroup width on both sides)
  if (!dbg("KH_SHAPE_FFN")) {
    out->ffn_r = 2;
    out->ffn_grid = grid_of(hidden_dim);
  }
  if (!dbg("KH_SHAPE_CLS")) {
    out->cls_r = 2;
    out->cls_grid = grid_of((vocab_size + 1) / 2);
  }
}
extern "C" int kh_plan_decode_ring(int32_t dim, int32_t hidden_dim, int32_t vocab_size, int32_t is_quant,
                                   int32_t group_size, int32_t* out4) {
  if (!out4 || dim <= 0 || hidden_dim <= 0 || vocab_size <= 0) return KH_ERR_INVALID_ARG;
  kh_model::RingPlan r;
  plan_ring(is_quant != 0, dim, hidden_dim, vocab_size, group_size, &r);
  out4[0] = r.ffn_r;
  out4[1] = r.ffn_grid;
  out4[2] = r.cls_r;
  out4[3] = r.cls_grid;
  return KH_OK;
}

// Host-only view of that plan for tools and the CPU test-suite: out[5][4] = {split, u, grid, wg} of qkv, wo,
// ffn13, w2, cls for a geometry (no device is touched).
extern "C" int kh_plan_decode_shapes(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size,
                                     int32_t is_quant, int32_t* out20) {
  if (!out20 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0) return KH_ERR_INVALID_ARG;
  kh_model::Shape sh[5];
  plan_decode_shapes(is_quant != 0, dim, hidden_dim, kv_dim, vocab_size, sh);
  for (int i = 0; i < 5; ++i) {
    out20[4 * i] = sh[i].split;
    out20[4 * i + 1] = sh[i].u;
    out20[4 * i + 2] = sh[i].grid;
    out20[4 * i + 3] = sh[i].wg;
  }
  return KH_OK;
}

int configure_step_kernels(kh_model* m) {
  const kh_config& c = m->cfg;
  // big activation vectors (hidden > 16 K floats) need the >64 KiB dynamic-LDS opt-in
  const size_t lds_need = fused_lds_bytes(c.is_quant, c.hidden_dim);
  if (lds_need > 160 * 1024) return KH_ERR_UNSUPPORTED;
  if (lds_need > 64 * 1024) {
    auto opt_in = [&](auto Q) {  // every k_gemv_res that w2 can launch on such an input: MAXV 0 and 6
      GemvResU<decltype(Q)::value>::each([&](auto U) {
        GemvResSP::each([&](auto SP) {
          KhVals<0, 6>::each([&](auto MV) {
            (void)hipFuncSetAttribute(
                (const void*)k_gemv_res<decltype(Q)::value, decltype(U)::value, decltype(MV)::value, decltype(SP)::value>,
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_need);
          });
        });
      });
    };
    opt_in(std::false_type{});
    opt_in(std::true_type{});
  }
  return KH_OK;
}

}  // namespace khm
using namespace khm;

extern "C" int kh_model_predict(kh_model* m, int32_t token, int32_t pos, int32_t is_prompt,
                                int32_t exec, int32_t* h_next) {
  if (!m || !h_next) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if (token < 0 || token >= c.vocab_size || pos < 0 || pos >= c.cache_len) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc = kv_ensure(m, pos + 1);  // cache rows 0 .. pos backed by HBM before the step is enqueued
  if (rc != KH_OK) return rc;
  set_state(m, token, pos);  // embedding() + fill_input (llama3.cpp:578-598, model.cpp:245-263)
  if (is_prompt && (rc = lp_none(m, pos, 1)) != KH_OK) return rc;  // fed, not sampled
  // logit processors apply to the calls whose pick is returned: prompt positions are never processed
  if (exec == KH_EXEC_UNFUSED) {
    rc = launch_step_unfused(m, pos, !is_prompt);
  } else if (exec == KH_EXEC_FUSED || exec == KH_EXEC_GRAPH) {
    // a single step always runs the full classifier
    launch_step_fused(m, /*advance=*/0, /*n_forced=*/0, nullptr, step_variant(m, pos, pos),
                      step_tail(m, false, !is_prompt));
    rc = kh_launch_status();
  } else {
    return KH_ERR_INVALID_ARG;
  }
  if (rc != KH_OK) return rc;
  int32_t next = -1;
  KH_CHECK_HIP(hipMemcpyAsync(&next, m->d_next, sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  *h_next = is_prompt ? -1 : next;  // post_processing (llama3.cpp:733-745)
  return KH_OK;
}

extern "C" int kh_model_set_sampling(kh_model* m, const kh_sampling* p) {
  if (p && !kh_sampling_valid(p)) return KH_ERR_INVALID_ARG;
  if (!m) return KH_ERR_INVALID_ARG;
  const kh_sampling greedy{0.f, 0, 1.f, 0};
  const kh_sampling want = p ? *p : greedy;
  const bool on = !kh_sampling_greedy(&want);
  if (on || m->d_samp) {  // (k_sample_proc decides greedy or sampled from the device copy: it follows "off" too)
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    int rc;
    if ((rc = m->d_samp.ensure(1)) != KH_OK) return rc;
    // written on the model stream behind whatever is queued; the sync keeps the host copy alive for the upload
    const KhSampParams dp = kh_samp_params(&want);
    KH_CHECK_HIP(hipMemcpyAsync(m->d_samp, &dp, sizeof(dp), hipMemcpyHostToDevice, m->stream));
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  }
  m->samp = want;
  m->samp_on = on;
  return KH_OK;
}
extern "C" int kh_model_get_sampling(const kh_model* m, kh_sampling* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  *out = m->samp;
  return KH_OK;
}

// ---- logit processors (kh_logit_proc.h)
namespace {
// does the ascending list `banned` (the -inf ids of a bias list) hold every token of some row of a constraint?  Such a
// state would leave the sampler no finite logit.
bool fsm_row_emptied(const std::vector<int64_t>& row_ptr, const int32_t* tokens, const std::vector<int32_t>& banned) {
  if (banned.empty()) return false;
  for (size_t s = 0; s + 1 < row_ptr.size(); ++s) {
    if (row_ptr[s + 1] - row_ptr[s] > (int64_t)banned.size()) continue;
    bool all = true;
    for (int64_t e = row_ptr[s]; e < row_ptr[s + 1] && all; ++e)
      all = std::binary_search(banned.begin(), banned.end(), tokens[e]);
    if (all) return true;
  }
  return false;
}
// after a change of m->pen / the bias list: whether anything is on, the buffers of the first "on", the device copy of
// the parameters (on the model stream, behind whatever is queued)
int proc_commit(kh_model* m) {
  const bool on = !kh_penalties_neutral(&m->pen) || m->n_bias > 0;
  // (k_sample_lp reads the device copies while log-probs are on, k_sample_proc_fsm while a constraint is set)
  if (on || m->d_proc || m->lp_top_n >= 0 || m->fsm_on) {
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    if (!m->d_proc) {  // the first "on": d_proc and d_cnt together, and d_samp where no sampler call made it yet
      KhDev<KhProcParams> proc;
      KhDev<int32_t> cnt;
      KhDev<KhSampParams> samp;
      const size_t V = (size_t)m->cfg.vocab_size;
      int rc;
      if ((rc = proc.alloc(1)) != KH_OK || (rc = cnt.alloc(V)) != KH_OK || (!m->d_samp && (rc = samp.alloc(1)) != KH_OK))
        return rc;
      KH_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * V, m->stream));  // once
      if (samp) {  // k_sample_proc reads the sampler's device copy: greedy until kh_model_set_sampling says more
        const KhSampParams sp = kh_samp_params(&m->samp);
        KH_CHECK_HIP(hipMemcpyAsync(samp, &sp, sizeof(sp), hipMemcpyHostToDevice, m->stream));
        KH_CHECK_HIP(hipStreamSynchronize(m->stream));
        m->d_samp = std::move(samp);
      }
      m->d_proc = std::move(proc);
      m->d_cnt = std::move(cnt);
    }
    const KhProcParams dp{m->pen.repetition, m->pen.presence, m->pen.frequency, m->pen.last_n, m->n_bias};
    KH_CHECK_HIP(hipMemcpyAsync(m->d_proc, &dp, sizeof(dp), hipMemcpyHostToDevice, m->stream));
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  }
  m->proc_on = on;
  return KH_OK;
}
}  // namespace

extern "C" int kh_model_set_penalties(kh_model* m, const kh_penalties* p) {
  if (p && !kh_penalties_valid(p)) return KH_ERR_INVALID_ARG;
  if (!m) return KH_ERR_INVALID_ARG;
  const kh_penalties before = m->pen;
  m->pen = p ? *p : kh_penalties{1.f, 0.f, 0.f, 0};
  const int rc = proc_commit(m);
  if (rc != KH_OK) m->pen = before;
  return rc;
}
extern "C" int kh_model_get_penalties(const kh_model* m, kh_penalties* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  *out = m->pen;
  return KH_OK;
}
extern "C" int kh_model_set_logit_bias(kh_model* m, const int32_t* h_ids, const float* h_bias, int32_t n) {
  if (n < 0 || (n > 0 && (!h_ids || !h_bias))) return KH_ERR_INVALID_ARG;
  return kh_api_guard([&]() -> int {
    // every check before any device call: values, ids that no vocabulary has, duplicates; then what needs the model
    for (int i = 0; i < n; ++i)
      if (h_bias[i] != h_bias[i] || h_bias[i] == INFINITY) return KH_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i)
      if (h_ids[i] < 0) return KH_ERR_RANGE;
    std::vector<int32_t> ids(h_ids, h_ids + n);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return KH_ERR_INVALID_ARG;
    if (!m) return KH_ERR_INVALID_ARG;
    const int V = m->cfg.vocab_size;
    if (n > 0 && ids.back() >= V) return KH_ERR_RANGE;
    int banned = 0;
    for (int i = 0; i < n; ++i) banned += h_bias[i] == -INFINITY;
    if (banned >= V) return KH_ERR_INVALID_ARG;  // (ids are distinct and in range) nothing left to pick
    std::vector<int32_t> banned_ids;
    for (int i = 0; i < n; ++i)
      if (h_bias[i] == -INFINITY) banned_ids.push_back(h_ids[i]);
    std::sort(banned_ids.begin(), banned_ids.end());
    // ... nor in any state of the constraint
    if (m->fsm_on && fsm_row_emptied(m->fsm.h_row_ptr, m->fsm.h_tokens.data(), banned_ids)) return KH_ERR_INVALID_ARG;
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    if (n > (int)m->d_bias.size()) {
      // the captured k_sample_proc launches hold the old pointers: drain, drop the graphs (rebuilt on next use), then
      // replace the lists - once both new ones exist; until then the model and its graphs are as they were
      const int cap = n < 64 ? 64 : n;
      KhDev<int32_t> ids_new;
      KhDev<float> bias_new;
      int rc;
      if ((rc = ids_new.alloc((size_t)cap)) != KH_OK || (rc = bias_new.alloc((size_t)cap)) != KH_OK) return rc;
      KH_CHECK_HIP(hipStreamSynchronize(m->stream));
      destroy_step_graphs(m);
      m->d_bias_ids = std::move(ids_new);
      m->d_bias = std::move(bias_new);
      m->n_bias = 0;
    }
    if (n > 0) {
      KH_CHECK_HIP(hipMemcpyAsync(m->d_bias_ids, h_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, m->stream));
      KH_CHECK_HIP(hipMemcpyAsync(m->d_bias, h_bias, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, m->stream));
    }
    m->n_bias = n;
    m->bias_banned = std::move(banned_ids);
    return proc_commit(m);  // (its sync keeps the caller's arrays alive for the uploads)
  });
}

// ---- constraint (kh_fsm.h)
int khm::fsm_stage(kh_model* m, const kh_fsm* a, const kh_model::Fsm& f, size_t n_state_words, FsmStage* st) {
  const int64_t n_edges = a->row_ptr[a->n_states];
  // the mask rows, on the host
  st->stride = ((size_t)m->cfg.vocab_size + 31) / 32;
  // one mask row per state, on the host and again on the device: bounded (16 KiB per state at V = 128256)
  if (st->stride * sizeof(uint32_t) * (size_t)a->n_states > (size_t)KH_FSM_MAX_MASK_BYTES) return KH_ERR_UNSUPPORTED;
  st->h_row_ptr.assign(a->row_ptr, a->row_ptr + a->n_states + 1);
  st->h_tokens.assign(a->tokens, a->tokens + n_edges);
  st->h_mask.assign(st->stride * (size_t)a->n_states, 0u);
  for (int32_t s = 0; s < a->n_states; ++s)
    for (int64_t e = a->row_ptr[s]; e < a->row_ptr[s + 1]; ++e)
      st->h_mask[st->stride * (size_t)s + ((size_t)a->tokens[e] >> 5)] |= 1u << (a->tokens[e] & 31);
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  // new buffers first: a failed call leaves the model as it found it
  int rc;
  if ((!f.desc && ((rc = st->desc.alloc(1)) != KH_OK || (rc = st->state.alloc(n_state_words)) != KH_OK)) ||
      (rc = st->mask.alloc(st->h_mask.size())) != KH_OK || (rc = st->row_ptr.alloc(st->h_row_ptr.size())) != KH_OK ||
      (rc = st->tokens.alloc((size_t)n_edges)) != KH_OK || (rc = st->next.alloc((size_t)n_edges)) != KH_OK)
    return rc;
  return KH_OK;
}
int khm::fsm_install(kh_model* m, const kh_fsm* a, kh_model::Fsm& f, FsmStage& st) {
  const int64_t n_edges = a->row_ptr[a->n_states];
  // on the model stream, behind whatever is queued; the sync keeps the host copies alive for the uploads - and the
  // stream has drained before the old buffers, which launches ahead of the new descriptor read, are released
  const KhFsmDev d{st.mask, st.row_ptr, st.tokens, st.next, a->n_states, (int32_t)st.stride};
  hipError_t e =
      hipMemcpyAsync(st.mask, st.h_mask.data(), sizeof(uint32_t) * st.h_mask.size(), hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(st.row_ptr, st.h_row_ptr.data(), sizeof(int64_t) * st.h_row_ptr.size(), hipMemcpyHostToDevice,
                       m->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(st.tokens, a->tokens, sizeof(int32_t) * (size_t)n_edges, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(st.next, a->next, sizeof(int32_t) * (size_t)n_edges, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(f.desc, &d, sizeof(d), hipMemcpyHostToDevice, m->stream);
  const hipError_t es = hipStreamSynchronize(m->stream);
  // (on an error the descriptor may name the new buffers: they are kept alive in the model all the same)
  f.mask = std::move(st.mask);
  f.row_ptr = std::move(st.row_ptr);
  f.tokens = std::move(st.tokens);
  f.next = std::move(st.next);
  if (e != hipSuccess || es != hipSuccess) return e != hipSuccess ? (int)e : (int)es;
  f.n_states = a->n_states;
  f.start = a->start;
  f.h_row_ptr = std::move(st.h_row_ptr);
  f.h_tokens = std::move(st.h_tokens);
  f.h_next.assign(a->next, a->next + n_edges);
  return KH_OK;
}
extern "C" int kh_model_set_constraint(kh_model* m, const kh_fsm* a) {
  if (!m) return KH_ERR_INVALID_ARG;
  return kh_api_guard([&]() -> int {
    if (!a) {  // off: the tails of the other settings again; the buffers stay for the next "on"
      m->fsm_on = false;
      return KH_OK;
    }
    // every check before any device call
    int rc = kh_fsm_check_host(a, m->cfg.vocab_size);
    if (rc != KH_OK) return rc;
    if (m->seq_fsm_on) return KH_ERR_UNSUPPORTED;  // one of the two constraints at a time
    {
      const std::vector<int64_t> h_row_ptr(a->row_ptr, a->row_ptr + a->n_states + 1);
      if (fsm_row_emptied(h_row_ptr, a->tokens, m->bias_banned)) return KH_ERR_INVALID_ARG;
    }
    FsmStage st;
    if ((rc = fsm_stage(m, a, m->fsm, 1, &st)) != KH_OK) return rc;
    const bool was_on = m->fsm_on;
    m->fsm_on = true;
    rc = proc_commit(m);  // what the _fsm tails read beside the automaton: d_proc, d_cnt, d_samp
    if (rc != KH_OK) {
      m->fsm_on = was_on;
      return rc;
    }
    if (st.desc) {
      m->fsm.desc = std::move(st.desc);
      m->fsm.state = std::move(st.state);
    }
    rc = (int)hipMemsetD32Async((hipDeviceptr_t)(int32_t*)m->fsm.state, a->start, 1, m->stream);
    const int rc2 = fsm_install(m, a, m->fsm, st);
    if (rc != KH_OK || rc2 != KH_OK) {
      m->fsm_on = false;
      return rc != KH_OK ? rc : rc2;
    }
    return KH_OK;
  });
}
extern "C" int kh_model_get_constraint_state(kh_model* m, int32_t* state) {
  if (!m || !state) return KH_ERR_INVALID_ARG;
  if (!m->fsm_on) return KH_ERR_UNSUPPORTED;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemcpyAsync(state, m->fsm.state, sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}
extern "C" int kh_model_set_constraint_state(kh_model* m, int32_t state) {
  if (!m) return KH_ERR_INVALID_ARG;
  if (!m->fsm_on) return KH_ERR_UNSUPPORTED;
  if (state < 0 || state >= m->fsm.n_states) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemcpyAsync(m->fsm.state, &state, sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));  // (keeps the host word alive for the upload)
  return KH_OK;
}

// ---- log-probs (kh_logprobs.h)
extern "C" int kh_model_set_logprobs(kh_model* m, int32_t top_n) {
  if (top_n < -1 || top_n > KH_LOGPROBS_MAX_TOP || !m || top_n > m->cfg.vocab_size) return KH_ERR_INVALID_ARG;
  if (top_n < 0) {
    m->lp_top_n = -1;
    return KH_OK;
  }
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  const int before = m->lp_top_n;
  {  // the first "on": the records of every position, all "none"
    const int rc = lp_ensure_records(m);
    if (rc != KH_OK) return rc;
  }
  m->lp_top_n = top_n;
  const int rc = proc_commit(m);  // the device copies of the processors' and the sampler's parameters exist
  if (rc != KH_OK) {
    m->lp_top_n = before;
    return rc;
  }
  // written on the model stream behind whatever is queued; the sync keeps the host copy alive for the upload
  const int32_t word = top_n;
  hipError_t e = hipMemcpyAsync(m->d_lp_top_n, &word, sizeof(word), hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  if (e != hipSuccess) {
    m->lp_top_n = -1;
    return (int)e;
  }
  return KH_OK;
}
extern "C" int kh_model_get_logprobs_setting(const kh_model* m, int32_t* top_n) {
  if (!m || !top_n) return KH_ERR_INVALID_ARG;
  *top_n = m->lp_top_n;
  return KH_OK;
}
extern "C" int kh_model_get_logprobs(kh_model* m, int32_t pos0, int32_t n, int32_t* h_token, float* h_lp,
                                     int32_t* h_top_ids, float* h_top_lp) {
  if (!m || n <= 0) return KH_ERR_INVALID_ARG;
  if (!m->d_lp_token) return KH_ERR_UNSUPPORTED;
  if (pos0 < 0 || (int64_t)pos0 + n > m->lp_cap) return KH_ERR_RANGE;
  return lp_read(m, pos0, n, m->lp_top_n, h_token, h_lp, h_top_ids, h_top_lp);
}

extern "C" int kh_model_generate(kh_model* m, const int32_t* h_prompt, int32_t n_prompt,
                                 int32_t total_steps, int32_t exec, int32_t* h_words,
                                 int32_t* n_words, float* h_elapsed_ms) {
  return kh_model_generate_until(m, h_prompt, n_prompt, total_steps, exec, nullptr, 0, h_words,
                                 n_words, h_elapsed_ms);
}

namespace {
// constraint on: the automaton state = start, on the model stream (a 32-bit fill: no host word to keep alive)
int fsm_rearm(kh_model* m) {
  if (!m->fsm_on) return KH_OK;
  KH_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(int32_t*)m->fsm.state, m->fsm.start, 1, m->stream));
  return KH_OK;
}
inline bool is_stop(int32_t t, const int32_t* stop, int n_stop) {
  for (int i = 0; i < n_stop; ++i)
    if (stop[i] == t) return true;
  return false;
}
// What the graph / fused forms of kh_model_generate_until and kh_model_generate_lookup share: the setup and the
// prompt phase of a run (generate_begin), and the enqueue of its next steps (generate_chunk)
struct GenRun {
  int exec = KH_EXEC_GRAPH;
  int screen = 0;      // cls_screen_level: the tail of the greedy steps
  int n_forced = 0;
  int start = 0;       // first position the step loop feeds: n_prompt - 1 behind a prefill, else 0
  int total_steps = 0;
};
// Forced-token upload, step buffers, cache rows, step graphs and their dry launches, the event that opens the timed
// loop, the prompt phase by the model's mode, and the decode state at (h_prompt[start], start).  Arguments checked by
// the caller.
int generate_begin(kh_model* m, const int32_t* h_prompt, int n_prompt, int total_steps, int exec, GenRun* g) {
  const kh_config& c = m->cfg;
  int rc;
  // greedy steps run the screened classifier pair (kh_cls_screen.h) wherever the model has one
  const int screen = cls_screen_level(m);
  if ((rc = ensure_seq_cap(m, total_steps)) != KH_OK) return rc;
  // every cache row this call can reach is backed by HBM before its first launch (the dry launches of fresh graphs
  // below touch rows 0 .. 7); mapping happens here, on the host, outside the event bracket of the step loop
  if ((rc = kv_ensure(m, total_steps < KH_GRAPH_STEPS ? KH_GRAPH_STEPS : total_steps)) != KH_OK) return rc;
  // pinned mirror of the words, sized like the device buffers so that a longer run later does not re-allocate it (a
  // hipHostMalloc inside the step loop's event bracket stalled the first 20-step run behind a 5-step one by 0.3 ms)
  if ((rc = ensure_pinned_words(m, m->seq_cap)) != KH_OK) return rc;
  // forced[i] = token fed at position i while inside the prompt, -1 afterwards.  Staged in the model's pinned
  // buffer: the upload is ordered before the steps by the stream and needs no host-side wait.  A generate that
  // returned early on an error may have left its upload in flight: the buffer is refilled only behind a stream
  // sync in that case (forced_in_flight; free when the previous call ended normally - it synchronised itself).
  // Only the first total_steps + 1 entries are written; whatever an earlier, longer run left beyond them goes back
  // to -1 (time_step / profile_step at deeper positions must not feed a stale prompt token).
  {
    if (m->forced_in_flight) KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    const int nf = total_steps + 1 <= m->seq_cap + 1 ? total_steps + 1 : m->seq_cap + 1;
    for (int i = 0; i < nf; ++i) m->h_forced_pin[i] = i < n_prompt ? h_prompt[i] : -1;
    m->forced_in_flight = true;
    KH_CHECK_HIP(hipMemcpyAsync(m->d_forced, m->h_forced_pin, (size_t)nf * sizeof(int32_t), hipMemcpyHostToDevice,
                                m->stream));
    if (m->forced_hwm > nf)
      KH_CHECK_HIP(hipMemsetAsync(m->d_forced + nf, 0xFF, (size_t)(m->forced_hwm - nf) * sizeof(int32_t), m->stream));
    m->forced_hwm = nf;
  }
  const int n_forced = m->seq_cap + 1;
  if (exec == KH_EXEC_GRAPH) {
    // all four graphs of variant 0 (1 / 2 / 4 / 8 steps) exist after the first generate of a model, whatever its
    // length (a warm-up run of 5 steps must leave the 8-step graph behind: capturing 656 nodes costs ~0.8 ms, which a
    // 20-step run would otherwise pay inside its timed loop); the other variants are captured when a run first
    // reaches position 256
    // ... and each has been LAUNCHED once: the first launch of an instantiated graph costs ~0.1-0.3 ms on this
    // runtime even after hipGraphUpload (a 20-step run behind a 5-step warm-up: 1012 tok/s, every later one 1028 on
    // the same model instance).  Every dry launch starts at position 0 (set_state before each one), so together they
    // write cache rows / words 0 .. 7 and read forced[1 .. 8] - uploaded above, or -1 beyond this call's prompt:
    // rows this very call rewrites (generate always starts a new sequence at position 0) unless total_steps < 8, in
    // which case rows total_steps .. 7 hold the K/V of a throw-away continuation afterwards (kuiper_hip.h says so:
    // a generate owns rows [0, max(total_steps, 8)) of the cache).  Skipped when the cache is shorter than that.
    // (Launching only the graphs of at most total_steps steps - the first r5 form - left the 8-step graph's first
    // launch inside the timed loop of a 20-step run behind a 5-step warm-up: 1018 instead of 1036-1042 tok/s.)
    const StepTail tail = step_tail(m, screen);
    bool fresh[4] = {false, false, false, false};
    hipGraphExec_t ge = nullptr;
    for (int n = 1, k = 0; n <= KH_GRAPH_STEPS; n *= 2, ++k) {
      fresh[k] = m->sg[tail][0][k].e == nullptr;
      if ((rc = step_graph(m, n_forced, 0, n, tail, &ge)) != KH_OK) return rc;
    }
    bool dry = false;
    if (c.cache_len >= KH_GRAPH_STEPS && m->seq_cap >= KH_GRAPH_STEPS)
      for (int k = 3; k >= 0; --k)
        if (fresh[k]) {
          set_state(m, h_prompt[0], 0);
          if ((rc = enqueue_steps(m, 0, 1 << k, n_forced, tail, KH_EXEC_GRAPH)) != KH_OK) return rc;
          dry = true;
        }
    if (dry) KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  }

  // prompt phase: the tokens that are only fed (positions 0 .. n_prompt-2).  KH_PREFILL selects how:
  //   "0" / "token"  the reference's one forward pass per prompt token (demo/main.cpp:20-22)
  //   "gemv"         B-token VALU kernels: K/V rows bit-identical to the token-by-token ones
  //   "gemm"         fp32-MFMA GEMM prefill: rows equal to fp32 round-off (tolerance, NOT bit-identity:
  //                  greedy tokens can differ from the token-by-token path at near-ties)
  //   unset          KH_FLAG_PREFILL_EXACT: "gemv" always; otherwise "gemm" from KH_PG_MIN_TOKENS fed-only tokens
  //                  on, "gemv" below that
  // any other value is an error (KH_ERR_INVALID_ARG), not a silent choice.
  int start = 0;
  // the token record of the processors' window: the prompt, -1 behind it (the steps write what they feed; the dry
  // launches above left a throw-away continuation in slots 1 .. 8)
  if (m->proc_on)
    KH_CHECK_HIP(hipMemcpyAsync(m->d_hist, m->d_forced, sizeof(int32_t) * (size_t)m->forced_hwm, hipMemcpyDeviceToDevice,
                                m->stream));
  // log-probs: the prompt positions are fed, not sampled (whatever path feeds them; the dry launches above wrote the
  // records of a throw-away continuation at positions 0 .. 7)
  if ((rc = lp_none(m, 0, n_prompt - 1)) != KH_OK) return rc;
  // the constraint: every generate starts its automaton over (the dry launches above moved the state along a
  // throw-away continuation)
  if ((rc = fsm_rearm(m)) != KH_OK) return rc;
  KH_CHECK_HIP(hipEventRecord(m->ev0, m->stream));
  if (n_prompt - 1 >= 2 && n_prompt - 1 < total_steps) {
    const char* e = dbg("KH_PREFILL");
    bool want_gemm = n_prompt - 1 >= KH_PG_MIN_TOKENS && !(m->opts.flags & KH_FLAG_PREFILL_EXACT), want_gemv = true;
    if (e && *e) {
      if (!strcmp(e, "0") || !strcmp(e, "token")) want_gemm = want_gemv = false;
      else if (!strcmp(e, "gemv")) want_gemm = false;
      else if (!strcmp(e, "gemm")) want_gemm = true;
      else return KH_ERR_INVALID_ARG;
    }
    if (want_gemm && pg_supported(m)) {
      if ((rc = prefill_gemm_run(m, h_prompt, n_prompt - 1, 0)) != KH_OK) return rc;
      start = n_prompt - 1;
      m->first_mode = 2;
    } else if (want_gemv && prefill_supported(m)) {
      if ((rc = prefill_run(m, h_prompt, n_prompt - 1, 0)) != KH_OK) return rc;
      start = n_prompt - 1;
      m->first_mode = 1;
    }
  }
  // near-tie report (kh_model_first_sample): with a prefill the first sampled step runs on its own and its logits
  // are put aside before the next step overwrites them
  m->first_pos = -1;
  if (start > 0) {
    if ((rc = m->first_logits.ensure((size_t)c.vocab_size)) != KH_OK) return rc;
    m->first_pos = start;
  }
  set_state(m, h_prompt[start], start);
  g->exec = exec;
  g->screen = screen;
  g->n_forced = n_forced;
  g->start = start;
  g->total_steps = total_steps;
  return KH_OK;
}
// enqueue the next 1 or up to KH_GRAPH_STEPS steps (positions s ..), at most `limit` of them; returns how many, -1 on
// an error
int generate_chunk(kh_model* m, const GenRun& g, int s, int limit) {
  // graph exec: the largest of 8 / 4 / 2 / 1 steps that still fits (a single-step launch costs ~15 us of graph-launch
  // gap: the 20-step form of the bench ran 8 + 8 + 1 + 1 + 1 + 1 and lost 0.3 % to it; now 8 + 8 + 4)
  int n = g.exec == KH_EXEC_GRAPH ? KH_GRAPH_STEPS : 1;
  while (n > limit) n >>= 1;
  // first sampled step behind a prefill: alone, and it leaves its logits in the buffer (full classifier)
  const bool keep = s == g.start && g.start > 0;
  if (keep) n = 1;
  if (enqueue_steps(m, s, n, g.n_forced, step_tail(m, keep ? 0 : g.screen), g.exec) != KH_OK) return -1;
  if (keep && hipMemcpyAsync(m->first_logits, m->logits, sizeof(float) * (size_t)m->cfg.vocab_size,
                             hipMemcpyDeviceToDevice, m->stream) != hipSuccess)
    return -1;
  return n;
}
}  // namespace

extern "C" int kh_model_generate_until(kh_model* m, const int32_t* h_prompt, int32_t n_prompt,
                                       int32_t total_steps, int32_t exec, const int32_t* h_stop,
                                       int32_t n_stop, int32_t* h_words, int32_t* n_words,
                                       float* h_elapsed_ms) {
  if (!m || !h_prompt || n_prompt <= 0 || total_steps <= 0 || !h_words || !n_words ||
      n_stop < 0 || (n_stop > 0 && !h_stop))
    return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if (total_steps > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_prompt, n_prompt)) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  *n_words = 0;

  if (exec == KH_EXEC_UNFUSED) {
    // the reference loop verbatim: host drives every step and reads `next` back each time
    if ((rc = fsm_rearm(m)) != KH_OK) return rc;
    KH_CHECK_HIP(hipEventRecord(m->ev0, m->stream));
    int pos = 0, next = -1, nw = 0;
    while (pos < total_steps) {
      const bool is_prompt = pos < n_prompt - 1;
      const int tok = pos <= n_prompt - 1 ? h_prompt[pos] : next;
      int got = -1;
      if ((rc = kh_model_predict(m, tok, pos, is_prompt, KH_EXEC_UNFUSED, &got)) != KH_OK) return rc;
      // demo/main.cpp:30-32: only a sampled token can end the sentence (next == -1 in the prompt)
      if (!is_prompt && is_stop(got, h_stop, n_stop)) break;
      next = is_prompt ? h_prompt[pos + 1] : got;
      h_words[nw++] = next;
      pos += 1;
    }
    KH_CHECK_HIP(hipEventRecord(m->ev1, m->stream));
    KH_CHECK_HIP(hipEventSynchronize(m->ev1));
    if (h_elapsed_ms) KH_CHECK_HIP(hipEventElapsedTime(h_elapsed_ms, m->ev0, m->ev1));
    *n_words = nw;
    return KH_OK;
  }
  if (exec != KH_EXEC_GRAPH && exec != KH_EXEC_FUSED) return KH_ERR_INVALID_ARG;

  GenRun g;
  if ((rc = generate_begin(m, h_prompt, n_prompt, total_steps, exec, &g)) != KH_OK) return rc;
  const int start = g.start;
  auto launch_chunk = [&](int s) -> int { return generate_chunk(m, g, s, total_steps - s); };
  int n_out = total_steps;
  if (n_stop == 0) {
    for (int s = start; s < total_steps;) {
      const int n = launch_chunk(s);
      if (n < 0) return (int)hipErrorUnknown;
      s += n;
    }
    KH_CHECK_HIP(hipEventRecord(m->ev1, m->stream));
    if ((rc = kh_launch_status()) != KH_OK) return rc;
    // through the pinned mirror: a device-to-pageable copy is staged and synchronised by the runtime on top of ours
    KH_CHECK_HIP(hipMemcpyAsync(m->h_words_pin, m->d_words, sizeof(int32_t) * total_steps,
                                hipMemcpyDeviceToHost, m->stream));
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    memcpy(h_words, m->h_words_pin, sizeof(int32_t) * (size_t)total_steps);
    for (int i = 0; i < start; ++i) h_words[i] = h_prompt[i + 1];  // forced, main.cpp:36-38
  } else {
    // Stop-token check without a per-step host round trip: the words of every
    // chunk of steps are mirrored into pinned memory behind the chunk, and the host inspects
    // chunk k while chunk k+1 is already queued, so the GPU never waits for the check.  At
    // most two chunks of steps run past the stop token; their words are discarded.
    struct Chunk { int s0, n; };
    Chunk infl[2];
    int n_infl = 0, head = 0, launched = start, stop_at = -1;
    for (int i = 0; i < start; ++i) m->h_words_pin[i] = h_prompt[i + 1];
    // Once chunks are queued, an early return must not leave graph launches and their D2H copies
    // into h_words_pin in flight (the caller may destroy the model or start another generate that
    // reallocates those buffers): every error path below drains the stream first.
    auto fail = [&](int code) -> int {
      (void)hipStreamSynchronize(m->stream);
      return code;
    };
#define KH_CHECK_DRAIN(expr)                          \
  do {                                                \
    hipError_t _e = (expr);                           \
    if (_e != hipSuccess) return fail((int)_e);       \
  } while (0)
    while (stop_at < 0 && (launched < total_steps || n_infl > 0)) {
      while (launched < total_steps && n_infl < 2) {
        const int n = launch_chunk(launched);
        if (n < 0) return fail((int)hipErrorUnknown);
        const int slot = (head + n_infl) & 1;
        KH_CHECK_DRAIN(hipMemcpyAsync(m->h_words_pin + launched, m->d_words + launched,
                                      sizeof(int32_t) * n, hipMemcpyDeviceToHost, m->stream));
        KH_CHECK_DRAIN(hipEventRecord(m->ev_chunk[slot], m->stream));
        infl[slot] = {launched, n};
        launched += n;
        ++n_infl;
      }
      KH_CHECK_DRAIN(hipEventSynchronize(m->ev_chunk[head]));
      const Chunk c0 = infl[head];
      for (int s = c0.s0; s < c0.s0 + c0.n; ++s)
        if (s >= n_prompt - 1 && is_stop(m->h_words_pin[s], h_stop, n_stop)) {
          stop_at = s;
          break;
        }
      if (stop_at >= 0) {
        // elapsed_ms ends behind the chunks already queued when the stop token was seen: it
        // includes up to 2 x 8 discarded steps past the stop (the reference's timer ends with the
        // step that produced it)
        KH_CHECK_DRAIN(hipEventRecord(m->ev1, m->stream));
      }
      head ^= 1;
      --n_infl;
    }
    if (stop_at < 0) KH_CHECK_DRAIN(hipEventRecord(m->ev1, m->stream));
    if ((rc = kh_launch_status()) != KH_OK) return fail(rc);
#undef KH_CHECK_DRAIN
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    n_out = stop_at >= 0 ? stop_at : total_steps;
    memcpy(h_words, m->h_words_pin, sizeof(int32_t) * (size_t)n_out);
  }
  m->forced_in_flight = false;  // both branches above end with a stream sync
  if (h_elapsed_ms) KH_CHECK_HIP(hipEventElapsedTime(h_elapsed_ms, m->ev0, m->ev1));
  *n_words = n_out;
  return KH_OK;
}

// ---- speculative greedy decode (kh_lookup.h: the drafter; kh_model_prefill.hip: the verify pass) -------------------
extern "C" int kh_lookup_draft(const int32_t* seq, int32_t n_seq, const int32_t* hint, int32_t n_hint, int32_t ngram_max,
                               int32_t ngram_min, int32_t* out, int32_t cap) {
  KhLookupCfg cfg;
  if (n_seq < 0 || n_hint < 0 || cap < 0 || (n_seq > 0 && !seq) || (n_hint > 0 && !hint) || (cap > 0 && !out) ||
      !kh_lookup_resolve(ngram_max, ngram_min, 0, &cfg))
    return KH_ERR_INVALID_ARG;
  return kh_lookup_draft_core(seq, n_seq, hint, n_hint, cfg.ngram_max, cfg.ngram_min, out, cap);
}
extern "C" int kh_lookup_draft_fsm(const kh_fsm* a, int32_t state, const int32_t* seq, int32_t n_seq, const int32_t* hint,
                                   int32_t n_hint, int32_t ngram_max, int32_t ngram_min, int32_t* out, int32_t cap,
                                   int32_t* n_forced) {
  KhLookupCfg cfg;
  // every check before anything is touched: the automaton's (kh_fsm_check, any vocabulary), then the drafter's
  const int rc = kh_fsm_check_host(a, INT64_MAX);
  if (rc != KH_OK) return rc;
  if (state < 0 || state >= a->n_states) return KH_ERR_RANGE;
  if (n_seq < 0 || n_hint < 0 || cap < 0 || (n_seq > 0 && !seq) || (n_hint > 0 && !hint) || (cap > 0 && !out) ||
      !kh_lookup_resolve(ngram_max, ngram_min, 0, &cfg))
    return KH_ERR_INVALID_ARG;
  return kh_api_guard([&]() -> int {
    std::vector<int32_t> work((size_t)n_seq + (size_t)cap);
    return kh_lookup_draft_fsm_core(a, state, seq, n_seq, hint, n_hint, cfg.ngram_max, cfg.ngram_min, out, cap,
                                    work.data(), n_forced);
  });
}

// kh_model_generate_until's graph form with the sampled part driven by draft + verify: at position p a draft of d >= 1
// tokens costs one verify pass and yields a + 1 words, no draft costs miss_steps steps on the step graphs.  The host
// reads the words behind either (the next draft needs them), so every iteration ends in a stream sync.
// as_set = false: greedy on the raw logits, any setting is refused.  as_set = true: the pass picks under the model's
// settings (verify_enqueue) as the plain steps do (step_tail); a draft is accepted where it EQUALS that pick - the
// seeded draw depends on (seed, position) and the logits alone - so the words are generate_until's either way.
// fsm (with as_set): the call that runs under the model's constraint.  The host tracks the automaton state - `start` as
// generate_begin sets the device word, then along every sampled word it reads, on the model's host copy of the automaton -
// and drafts from it with kh_lookup_draft_fsm_core: forced tokens first, n-gram proposals cut to what the automaton can
// follow.  The passes are verify_enqueue's constrained form, the plain steps' tails are the _fsm ones already.  A stop
// among the owned picks: the device word is set behind it (the pass or the steps moved it further).
static int generate_lookup_run(kh_model* m, const int32_t* h_prompt, int32_t n_prompt, int32_t total_steps,
                               const int32_t* h_stop, int32_t n_stop, const kh_lookup_opts* opts, int32_t* h_words,
                               int32_t* n_words, float* h_elapsed_ms, kh_lookup_stats* stats, bool as_set,
                               bool fsm = false, int32_t* n_forced = nullptr) {
  if (!m || !h_prompt || n_prompt <= 0 || total_steps <= 0 || !h_words || !n_words || n_stop < 0 ||
      (n_stop > 0 && !h_stop))
    return KH_ERR_INVALID_ARG;
  const kh_lookup_opts o = opts ? *opts : kh_lookup_opts{0, 0, 0, nullptr, 0};
  KhLookupCfg cfg;
  if (!kh_lookup_resolve(o.ngram_max, o.ngram_min, o.miss_steps, &cfg) || o.n_hint < 0 || (o.n_hint > 0 && !o.h_hint))
    return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if (total_steps > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_prompt, n_prompt)) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, o.h_hint, o.n_hint)) return KH_ERR_RANGE;
  // only where the verify pass runs and, unless as_set, greedy on the raw logits only: no silent fallback to
  // generate_until
  if ((m->fsm_on && !fsm) || !full_depth_supported(m)) return KH_ERR_UNSUPPORTED;  // (a constraint: as kh_model_verify)
  if (!as_set && (m->samp_on || m->proc_on || m->lp_top_n >= 0)) return KH_ERR_UNSUPPORTED;
  return kh_api_guard([&]() -> int {
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    *n_words = 0;
    int rc;
    // every early return below may leave launches and copies into pinned memory in flight: drain first
    auto fail = [&](int code) -> int {
      (void)hipStreamSynchronize(m->stream);
      return code;
    };
    std::vector<int32_t> seq(h_prompt, h_prompt + n_prompt);  // seq[i] = the token of position i, as far as known
    seq.reserve((size_t)total_steps + KH_GRAPH_STEPS + 1);
    if ((rc = verify_prepare(m, total_steps, as_set, fsm)) != KH_OK) return rc;
    // the constraint, as the host sees it
    const bool fsm_run = fsm && m->fsm_on;
    const kh_fsm A{m->fsm.n_states, m->fsm.start, m->fsm.h_row_ptr.data(), m->fsm.h_tokens.data(), m->fsm.h_next.data()};
    int32_t hs = m->fsm.start;
    auto fsm_move = [&](int32_t w) {  // (a word its row does not hold leaves the state, as kh_fsm_advance_core does)
      const int64_t e = fsm_run ? kh_fsm_edge_host(&A, hs, w) : -1;
      if (e >= 0) hs = A.next[e];
    };
    std::vector<int32_t> work(fsm_run ? (size_t)total_steps + KH_GRAPH_STEPS + 1 : 0);
    int forced_total = 0;
    GenRun g;
    if ((rc = generate_begin(m, h_prompt, n_prompt, total_steps, KH_EXEC_GRAPH, &g)) != KH_OK) return fail(rc);
    const int width = verify_width(m);
    int32_t* const pin = m->h_words_pin;
    for (int i = 0; i < g.start; ++i) pin[i] = h_prompt[i + 1];  // forced, main.cpp:36-38
    kh_lookup_stats st{0, 0, 0, 0};
    int p = g.start, stop_at = -1;
    while (p < total_steps && stop_at < 0) {
      const bool sampled = p >= n_prompt - 1;
      // the first sampled position behind a prefill takes a plain step with the full classifier (kh_model_first_sample)
      const bool first = p == g.start && g.start > 0;
      int32_t fed[KH_GRAPH_STEPS];
      int d = 0;
      if (sampled && !first) {
        const int room = total_steps - 1 - p, cap = width - 1 < room ? width - 1 : room;
        if (fsm_run) {
          int32_t forced = 0;
          d = kh_lookup_draft_fsm_core(&A, hs, seq.data(), p + 1, o.h_hint, o.n_hint, cfg.ngram_max, cfg.ngram_min,
                                       fed + 1, cap, work.data(), &forced);
          forced_total += forced;
        } else {
          d = kh_lookup_draft_core(seq.data(), p + 1, o.h_hint, o.n_hint, cfg.ngram_max, cfg.ngram_min, fed + 1, cap);
        }
      }
      if (d > 0) {
        fed[0] = seq[(size_t)p];
        if ((rc = verify_enqueue(m, fed, d + 1, p, as_set, fsm)) != KH_OK) return fail(rc);
        if (hipStreamSynchronize(m->stream) != hipSuccess) return fail((int)hipErrorUnknown);
        const int a = m->h_spec_pin[0];
        for (int i = 0; i <= a && stop_at < 0; ++i) {
          const int32_t w = m->h_spec_pin[1 + i];
          fsm_move(w);
          if (is_stop(w, h_stop, n_stop)) {
            stop_at = p + i;
          } else {
            pin[p + i] = w;
            seq.push_back(w);
          }
        }
        st.passes += 1;
        st.drafted += d;
        st.accepted += a;
        p += a + 1;
      } else {
        // nothing drafted: steps on the step graphs, exactly as generate enqueues them (prompt positions that no
        // prefill covered run here too, up to the last fed-only one)
        int k = sampled ? cfg.miss_steps : n_prompt - 1 - p;
        if (k > total_steps - p) k = total_steps - p;
        if (k > KH_GRAPH_STEPS) k = KH_GRAPH_STEPS;
        if (first) k = 1;
        for (int s = p; s < p + k;) {
          const int n = generate_chunk(m, g, s, p + k - s);
          if (n < 0) return fail((int)hipErrorUnknown);
          s += n;
        }
        if (hipMemcpyAsync(pin + p, m->d_words + p, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, m->stream) !=
                hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess)
          return fail((int)hipErrorUnknown);
        for (int s = p; s < p + k && stop_at < 0; ++s) {
          if (s >= n_prompt - 1) fsm_move(pin[s]);
          if (s >= n_prompt - 1 && is_stop(pin[s], h_stop, n_stop))
            stop_at = s;
          else if (s + 1 >= (int)seq.size())
            seq.push_back(pin[s]);
        }
        if (sampled) st.plain_steps += k;
        p += k;
      }
    }
    if (hipEventRecord(m->ev1, m->stream) != hipSuccess) return fail((int)hipErrorUnknown);
    // the state behind the stop: the pass or the steps that met it moved the device word past it
    if (fsm_run && stop_at >= 0 &&
        hipMemsetD32Async((hipDeviceptr_t)(int32_t*)m->fsm.state, hs, 1, m->stream) != hipSuccess)
      return fail((int)hipErrorUnknown);
    if ((rc = kh_launch_status()) != KH_OK) return fail(rc);
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    m->forced_in_flight = false;
    const int n_out = stop_at >= 0 ? stop_at : total_steps;
    memcpy(h_words, pin, sizeof(int32_t) * (size_t)n_out);
    if (h_elapsed_ms) KH_CHECK_HIP(hipEventElapsedTime(h_elapsed_ms, m->ev0, m->ev1));
    if (stats) *stats = st;
    if (n_forced) *n_forced = forced_total;
    *n_words = n_out;
    return KH_OK;
  });
}
extern "C" int kh_model_generate_lookup(kh_model* m, const int32_t* h_prompt, int32_t n_prompt, int32_t total_steps,
                                        const int32_t* h_stop, int32_t n_stop, const kh_lookup_opts* opts,
                                        int32_t* h_words, int32_t* n_words, float* h_elapsed_ms,
                                        kh_lookup_stats* stats) {
  return generate_lookup_run(m, h_prompt, n_prompt, total_steps, h_stop, n_stop, opts, h_words, n_words, h_elapsed_ms,
                             stats, /*as_set=*/false);
}
extern "C" int kh_model_generate_lookup_as_set(kh_model* m, const int32_t* h_prompt, int32_t n_prompt,
                                               int32_t total_steps, const int32_t* h_stop, int32_t n_stop,
                                               const kh_lookup_opts* opts, int32_t* h_words, int32_t* n_words,
                                               float* h_elapsed_ms, kh_lookup_stats* stats) {
  return generate_lookup_run(m, h_prompt, n_prompt, total_steps, h_stop, n_stop, opts, h_words, n_words, h_elapsed_ms,
                             stats, /*as_set=*/true);
}
extern "C" int kh_model_generate_lookup_fsm(kh_model* m, const int32_t* h_prompt, int32_t n_prompt, int32_t total_steps,
                                            const int32_t* h_stop, int32_t n_stop, const kh_lookup_opts* opts,
                                            int32_t* h_words, int32_t* n_words, float* h_elapsed_ms,
                                            kh_lookup_stats* stats, int32_t* n_forced) {
  return generate_lookup_run(m, h_prompt, n_prompt, total_steps, h_stop, n_stop, opts, h_words, n_words, h_elapsed_ms,
                             stats, /*as_set=*/true, /*fsm=*/true, n_forced);
}
