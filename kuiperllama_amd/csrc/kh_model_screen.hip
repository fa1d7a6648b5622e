// kh_model_screen.hip — host side of the screened classifier (kh_cls_screen.h): the bf16 copy made at model
// creation, the two launches that take k_cls's and k_sample's slots in the greedy steps of kh_model_generate*,
// logits on demand behind such steps, the creation-time check, kh_model_cls_screen_info.
// Replaces nothing in the reference (kuiper/source/model/llama3.cpp:722-745 streams the fp32 classifier every step).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kh_cls_screen.h"
#include "kh_dispatch.h"
#include "kh_model_internal.h"

namespace khm {

namespace {
// The instantiations of the two kernels, <U, MAXV>.  k_cls_screen has no U 8: a tile of 8 loads per row, 64 registers
// of packed weights beside their unpacked halves, does not fit 128 registers.  k_sample_screen takes k_cls's U.  A
// vector staged deeper than 4 float4 per thread is not screened (cls_screen_create), so MAXV is one of these; the
// lists end in the value an unlisted one takes (kh_dispatch.h).
using ScreenU = KhVals<4, 2>;
using SampleScreenU = KhVals<8, 4, 2>;
using ScreenMV = KhVals<4, 2, 1>;
template <class US, class F>
void pick_screen(int u, int mv, F&& f) {
  kh_pick_ge(US{}, u, [&](auto U) { kh_pick(ScreenMV{}, mv, [&](auto MV) { f(U, MV); }); });
}

// Launch of k_cls_screen.  u: 16-byte loads per row and lane in flight, one tile per row where it fits (a lane
// covers 8 weights per load: dim 2048 is 4 loads; longer rows walk several tiles of 4).  A bf16 row pair is half
// the bytes of k_cls's, so twice the workgroups of k_cls's plan keep the same bytes in flight per CU (measured on
// Llama-3.2-1B: 83.8 us for 525.8 MB, profiles/cls_screen_ab.txt).  Hook KH_SHAPE_SCREEN="u,grid,wg" overrides.
void plan_screen(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::ClsScreen& s = m->scr;
  const int per_lane = (c.dim / 8 + KH_WAVE - 1) / KH_WAVE;
  s.u = per_lane >= 3 ? 4 : 2;
  s.wg = m->sh_cls.wg;
  const int pairs = (c.vocab_size + 1) / 2, wpw = s.wg / KH_WAVE;
  const int need = (pairs + wpw - 1) / wpw;
  const int cap = 1024 * KH_WG / s.wg;  // 16 waves per CU
  s.grid = 2 * m->sh_cls.grid;
  if (s.grid > cap) s.grid = cap;
  if (s.grid > need) s.grid = need;
  if (const char* ov = dbg("KH_SHAPE_SCREEN")) {
    int u = 0, g = 0, w = 0;
    if (sscanf(ov, "%d,%d,%d", &u, &g, &w) == 3 && ScreenU::has(u) && g >= 1 && g <= 4096 &&
        (w == 256 || w == 512) && ScreenMV::has(kh_stage_maxv(c.dim, w))) {
      s.u = u;
      s.grid = g;
      s.wg = w;
    } else {
      fprintf(stderr, "[kh] KH_SHAPE_SCREEN=\"%s\" rejected (u 2/4, grid 1..4096, wg 256/512): planned shape\n", ov);
    }
  }
}

// Launch of k_cls_screen_q8: Gemv<true, U>, a lane covers 16 weights per load (dim 2048 is 2 loads).  256-thread
// workgroups, three per CU: 12 waves per CU, all resident at once (the kernel's 85 registers would allow 20; more
// workgroups measured slower), an int8 row pair is 4 KB and a wave streams about twenty of them behind one
// staging of the vector.  The sweep of this shape on Llama-3.2-1B is the last section of
// profiles/cls_screen_q8_ab.txt (tools/cls_screen_q8_ab.py --sweep): step loop per token against the two-launch
// tail.  512-thread workgroups where the vector is too long to stage from 256.  Hook
// KH_SHAPE_SCREEN_Q8="u,grid,wg" overrides (tests reach every instantiation and the one-workgroup spill this way).
using ScreenQ8U = KhVals<4, 2>;
void plan_screen_q8(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::ClsScreen::Q8& t = m->scr.q8;
  const int per_lane = (c.dim / 16 + KH_WAVE - 1) / KH_WAVE;
  t.u = per_lane >= 3 ? 4 : 2;
  t.wg = ScreenMV::has(kh_stage_maxv(c.dim, KH_WG)) ? KH_WG : KH_WG_MAX;
  const int pairs = (c.vocab_size + 1) / 2, wpw = t.wg / KH_WAVE;
  const int need = (pairs + wpw - 1) / wpw;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->opts.device) != hipSuccess || cus <= 0)
    cus = 256;
  t.grid = 3 * cus * KH_WG / t.wg;
  if (t.grid > 4096) t.grid = 4096;
  if (t.grid > need) t.grid = need;
  if (const char* ov = dbg("KH_SHAPE_SCREEN_Q8")) {
    int u = 0, g = 0, w = 0;
    if (sscanf(ov, "%d,%d,%d", &u, &g, &w) == 3 && ScreenQ8U::has(u) && g >= 1 && g <= 4096 &&
        (w == 256 || w == 512) && ScreenMV::has(kh_stage_maxv(c.dim, w))) {
      t.u = u;
      t.grid = g;
      t.wg = w;
    } else {
      fprintf(stderr, "[kh] KH_SHAPE_SCREEN_Q8=\"%s\" rejected (u 2/4, grid 1..4096, wg 256/512): planned shape\n", ov);
    }
  }
}
// The tier steps aside - the tail is the two-launch one - where a hook asks for a specific k_cls_screen or k_cls
// launch, and under KH_CLS_SCREEN_Q8=0.
bool q8_hooks_bar() { return dbg_off("KH_CLS_SCREEN_Q8") || dbg("KH_SHAPE_SCREEN") || dbg("KH_SHAPE_CLS"); }
}  // namespace

namespace {
// A KH_SHAPE_CLS hook asks for a specific k_cls launch (the rule of plan_ring): screening steps aside - unless
// KH_CLS_SCREEN=force asks for both (tests: k_sample_screen re-scores with k_cls's U, staging depth and width, and
// away from the heuristic those change only through that hook).
bool cls_hook_bars_screen() {
  if (!dbg("KH_SHAPE_CLS")) return false;
  const char* v = dbg("KH_CLS_SCREEN");
  return !(v && strcmp(v, "force") == 0);
}
}  // namespace

bool cls_screen_wanted(const kh_model* m) {
  // the sampling kernel needs every logit
  return m->scr.on && !m->samp_on && !dbg_off("KH_CLS_SCREEN") && !cls_hook_bars_screen();
}

int cls_screen_level(const kh_model* m) {
  if (!cls_screen_wanted(m)) return 0;
  return m->scr.q8.on && !q8_hooks_bar() ? 2 : 1;
}

static void cls_screen_q8_release(kh_model* m) { m->scr.q8 = kh_model::ClsScreen::Q8(); }

// The int8 copy behind a bf16 screen that is on: fp32 model, dim a multiple of the group, no hook in the way.  Where
// the copy cannot be had - no room for it - the tier is off and nothing else changes: KH_OK, the bf16 screen goes on.
// A failing stream operation or launch is an error of the model (its stream is not usable); nothing stays allocated.
static int cls_screen_q8_create(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::ClsScreen::Q8& t = m->scr.q8;
  if (!m->scr.on || c.dim % KH_SCR8_G != 0 || q8_hooks_bar()) return KH_OK;
  plan_screen_q8(m);
  if (!ScreenMV::has(kh_stage_maxv(c.dim, t.wg))) return KH_OK;
  const size_t V = (size_t)c.vocab_size, gpr = (size_t)(c.dim / KH_SCR8_G);
  // partials: every grid a KH_SHAPE_SCREEN_Q8 hook may ask for
  // (eight allocations: the ones whose failure a creation survives)
  if (t.q.alloc(V * (size_t)c.dim) != KH_OK || t.sc.alloc(V * gpr) != KH_OK || t.e8.alloc(V) != KH_OK ||
      t.p_lb.alloc(4096) != KH_OK || t.p_spill.alloc(4096) != KH_OK || t.p_ub.alloc(4096 * KH_SCR8_C) != KH_OK ||
      t.p_idx.alloc(4096 * KH_SCR8_C) != KH_OK || t.stats.alloc(4) != KH_OK) {
    (void)hipGetLastError();  // the failed allocation is not the model's error
    cls_screen_q8_release(m);
    if (dbg("KH_LOAD_DEBUG") || dbg("KH_SHAPE_DEBUG"))
      fprintf(stderr, "[kh] classifier screen, int8 tier: no room for the copy, the tier is off\n");
    return KH_OK;
  }
  hipStream_t st = m->stream;
  const int n = (c.dim + KH_WAVE - 1) / KH_WAVE + 24;  // roundings a term passes through (kh_cls_screen.h)
  const double u = 1.0 / 16777216.0;
  const double gam2 = 2.0 * (n * u) / (1.0 - n * u);
  float ms = 0.f;
  auto build = [&]() -> int {
    KH_CHECK_HIP(hipMemsetAsync(t.stats, 0, 4 * sizeof(int32_t), st));
    KH_CHECK_HIP(hipEventRecord(m->ev0, st));
    hipLaunchKernelGGL(k_cls_q8_build, dim3(2048), dim3(KH_WG), 0, st, (const float*)m->cls.w, (uint32_t*)t.q.get(),
                       t.sc.get(), t.e8.get(), c.dim, c.vocab_size, gam2);
    KH_CHECK_HIP(hipEventRecord(m->ev1, st));
    KH_CHECK_HIP(hipEventSynchronize(m->ev1));
    const int rc = kh_launch_status();
    if (rc != KH_OK) return rc;
    KH_CHECK_HIP(hipEventElapsedTime(&ms, m->ev0, m->ev1));
    return KH_OK;
  };
  const int rc = build();
  if (rc != KH_OK) {
    cls_screen_q8_release(m);
    return rc;
  }
  t.bytes = V * (size_t)c.dim + V * gpr * sizeof(float) + V * sizeof(float);
  t.build_ms = ms;
  t.on = true;
  if (dbg("KH_LOAD_DEBUG") || dbg("KH_SHAPE_DEBUG"))
    fprintf(stderr, "[kh] classifier screen, int8 tier: copy %.1f MB in %.2f ms; k_cls_screen_q8 u %d grid %d wg %d\n",
            (double)t.bytes / 1e6, t.build_ms, t.u, t.grid, t.wg);
  return KH_OK;
}

void cls_screen_release(kh_model* m) { m->scr = kh_model::ClsScreen(); }

int cls_screen_create(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::ClsScreen& s = m->scr;
  s = kh_model::ClsScreen();
  // fp32 models whose rows keep 16-byte alignment as bf16 and whose vector k_cls stages in registers; int8
  // classifiers are a fiftieth of their token and stay as they are
  if (c.is_quant || (m->opts.flags & KH_FLAG_NO_CLS_SCREEN) || dbg_off("KH_CLS_SCREEN") || cls_hook_bars_screen()) return KH_OK;
  if (c.dim % 8 != 0 || c.vocab_size < 2) return KH_OK;
  if (!ScreenMV::has(kh_stage_maxv(c.dim, m->sh_cls.wg))) return KH_OK;
  plan_screen(m);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->opts.device) != hipSuccess || cus <= 0)
      cus = 256;
    const int wpw = m->sh_cls.wg / KH_WAVE, need = ((c.vocab_size + 1) / 2 + wpw - 1) / wpw;
    s.sgrid = cus < need ? cus : need;
  }
  int rc;
  const size_t V = (size_t)c.vocab_size;
  // (partials: sized for every grid a KH_SHAPE_SCREEN hook may ask for)
  if ((rc = s.wbf.alloc(V * (size_t)c.dim)) != KH_OK || (rc = s.err.alloc(V)) != KH_OK ||
      (rc = s.x_save.alloc((size_t)c.dim)) != KH_OK || (rc = s.p_lb.alloc(4096)) != KH_OK ||
      (rc = s.p_spill.alloc(4096)) != KH_OK || (rc = s.p_ub.alloc(4096 * KH_SCR_C)) != KH_OK ||
      (rc = s.p_idx.alloc(4096 * KH_SCR_C)) != KH_OK || (rc = s.ov_val.alloc((size_t)s.sgrid)) != KH_OK ||
      (rc = s.ov_idx.alloc((size_t)s.sgrid)) != KH_OK || (rc = s.ticket.alloc(1)) != KH_OK ||
      (rc = s.stats.alloc(4)) != KH_OK) {
    cls_screen_release(m);
    return rc;
  }
  s.bytes = V * (size_t)c.dim * sizeof(uint16_t) + V * sizeof(float);
  hipStream_t st = m->stream;
  KH_CHECK_HIP(hipMemsetAsync(s.ticket, 0, sizeof(uint32_t), st));
  KH_CHECK_HIP(hipMemsetAsync(s.stats, 0, 4 * sizeof(int32_t), st));
  KH_CHECK_HIP(hipMemsetAsync(s.x_save, 0, sizeof(float) * (size_t)c.dim, st));
  const int n = (c.dim + KH_WAVE - 1) / KH_WAVE + 8;  // roundings a term passes through (kh_cls_screen.h)
  const double u = 1.0 / 16777216.0;
  const double gam2 = 2.0 * (n * u) / (1.0 - n * u);
  KH_CHECK_HIP(hipEventRecord(m->ev0, st));
  hipLaunchKernelGGL(k_cls_bf16_build, dim3(2048), dim3(KH_WG), 0, st, (const float*)m->cls.w, (uint32_t*)s.wbf.get(),
                     s.err.get(), c.dim, c.vocab_size, gam2);
  KH_CHECK_HIP(hipEventRecord(m->ev1, st));
  KH_CHECK_HIP(hipEventSynchronize(m->ev1));
  if ((rc = kh_launch_status()) != KH_OK) return rc;
  KH_CHECK_HIP(hipEventElapsedTime(&s.build_ms, m->ev0, m->ev1));
  s.on = true;
  if ((rc = cls_screen_q8_create(m)) != KH_OK) return rc;
  if (dbg("KH_LOAD_DEBUG") || dbg("KH_SHAPE_DEBUG"))
    fprintf(stderr, "[kh] classifier screen: bf16 copy %.1f MB in %.2f ms; k_cls_screen u %d grid %d wg %d, "
                    "k_sample_screen grid %d wg %d\n", (double)s.bytes / 1e6, s.build_ms, s.u, s.grid, s.wg, s.sgrid,
            m->sh_cls.wg);
  return KH_OK;
}

void launch_cls_screen_q8(kh_model* m, float* dbg_lb, float* dbg_ub, int grid) {
  const kh_config& c = m->cfg;
  const kh_model::ClsScreen::Q8& t = m->scr.q8;
  KhClsScreenQ8Args a;
  a.x = m->x;
  a.final_norm = m->final_norm;
  a.q = t.q;
  a.sc = t.sc;
  a.e8 = t.e8;
  a.p_lb = t.p_lb;
  a.p_spill = t.p_spill;
  a.p_ub = t.p_ub;
  a.p_idx = t.p_idx;
  a.dbg_lb = dbg_lb;
  a.dbg_ub = dbg_ub;
  a.dim = c.dim;
  a.vocab = c.vocab_size;
  a.eps = c.rms_eps;
  pick_screen<ScreenQ8U>(t.u, kh_stage_maxv(c.dim, t.wg), [&](auto U, auto MV) {
    kh_launch(KH_KERNEL(k_cls_screen_q8, U, MV), grid > 0 ? grid : t.grid, t.wg, cls_screen_q8_lds_bytes(c.dim), m->stream, a);
  });
}

// nq > 0: survivor mode behind a k_cls_screen_q8 launch of nq workgroups; 0: the full scan
static void launch_cls_screen_behind(kh_model* m, float* dbg_lb, float* dbg_ub, int nq) {
  const kh_config& c = m->cfg;
  const kh_model::ClsScreen& s = m->scr;
  KhClsScreenArgs a;
  a.q_lb = nq > 0 ? s.q8.p_lb : nullptr;
  a.q_spill = s.q8.p_spill;
  a.q_ub = s.q8.p_ub;
  a.q_idx = s.q8.p_idx;
  a.q_stats = s.q8.stats;
  a.nq = nq;
  a.x = m->x;
  a.final_norm = m->final_norm;
  a.wbf = s.wbf;
  a.err = s.err;
  a.x_save = s.x_save;
  a.p_lb = s.p_lb;
  a.p_spill = s.p_spill;
  a.p_ub = s.p_ub;
  a.p_idx = s.p_idx;
  a.dbg_lb = dbg_lb;
  a.dbg_ub = dbg_ub;
  a.dim = c.dim;
  a.vocab = c.vocab_size;
  a.eps = c.rms_eps;
  pick_screen<ScreenU>(s.u, kh_stage_maxv(c.dim, s.wg), [&](auto U, auto MV) {
    kh_launch(KH_KERNEL(k_cls_screen, U, MV), s.grid, s.wg, cls_screen_lds_bytes(c.dim), m->stream, a);
  });
}

void launch_cls_screen(kh_model* m, float* dbg_lb, float* dbg_ub, bool survivors) {
  launch_cls_screen_behind(m, dbg_lb, dbg_ub, survivors ? m->scr.q8.grid : 0);
}

void launch_sample_screen(kh_model* m, int advance, int n_forced) {
  const kh_config& c = m->cfg;
  const kh_model::ClsScreen& s = m->scr;
  KhSampleScreenArgs a;
  a.p_lb = s.p_lb;
  a.p_spill = s.p_spill;
  a.p_ub = s.p_ub;
  a.p_idx = s.p_idx;
  a.nsp = s.grid;
  a.x_save = s.x_save;
  a.final_norm = m->final_norm;
  a.wcls = (const float*)m->cls.w;
  a.eps = c.rms_eps;
  a.ov_val = s.ov_val;
  a.ov_idx = s.ov_idx;
  a.ticket = s.ticket;
  a.stats = s.stats;
  a.st = fill_step_tail(m, advance, n_forced);
  // k_cls's own U, staging depth and workgroup width: the re-scored values are then k_cls's, bit for bit
  const int wg = m->sh_cls.wg;
  pick_screen<SampleScreenU>(m->sh_cls.u, kh_stage_maxv(c.dim, wg), [&](auto U, auto MV) {
    kh_launch(KH_KERNEL(k_sample_screen, U, MV), s.sgrid, wg, cls_lds_bytes(false, c.dim), m->stream, a);
  });
}

int cls_refresh_logits(kh_model* m) {
  if (!m->scr.stale) return KH_OK;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  // the input the last screened step saw; today's k_cls instantiation on the same bytes (clears scr.stale)
  launch_cls(m, {m->scr.x_save, m->logits, m->part_val, m->part_idx}, m->ring.cls_r == 2);
  return kh_launch_status();
}

namespace {
// *flag |= some logit outside its interval (a NaN logit has the interval (-inf, +inf))
__global__ __launch_bounds__(KH_WG) void k_st_interval(const float* lg, const float* lb, const float* ub, size_t n,
                                                      int32_t* flag) {
  bool d = false;
  for (size_t i = (size_t)blockIdx.x * KH_WG + threadIdx.x; i < n; i += (size_t)gridDim.x * KH_WG) {
    const float v = lg[i];
    d |= v == v ? !(lb[i] <= v && v <= ub[i]) : !(lb[i] == -INFINITY && ub[i] == INFINITY);
  }
  if (d) *flag = 1;
}
}  // namespace

// One screened pair, then one full pair, on the vector now in m->x, without advancing: tok[0] / tok[1] receive the two
// tokens, and the model's logits buffer holds k_cls's logits of that vector afterwards.  Every row's interval goes to
// two arrays that live for this call: then(lb, ub) enqueues the caller's reads of them behind the pairs and ahead of
// the stream sync that ends the body.
template <class F>
static int cls_screen_pairs(kh_model* m, int32_t* tok, F&& then) {
  hipStream_t st = m->stream;
  const size_t V = (size_t)m->cfg.vocab_size;
  KhDev<float> lb, ub;
  int rc;
  if ((rc = lb.alloc(V)) != KH_OK || (rc = ub.alloc(V)) != KH_OK) return rc;
  launch_cls_screen(m, lb, ub);
  launch_sample(m, /*advance=*/0, /*n_forced=*/0, kScreen);
  hipError_t e = hipMemcpyAsync(&tok[0], m->d_next, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  launch_cls(m);
  launch_sample(m, 0, 0, kGreedy);
  if (e == hipSuccess) e = hipMemcpyAsync(&tok[1], m->d_next, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = then(lb.get(), ub.get());
  // whatever was enqueued reads lb / ub: the stream drains before they go, on the failure paths too
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? KH_OK : (int)e;
}

// One screened step against one full step on a fixed vector (the embedding row of token 1): the same token, every
// full logit inside the interval the screen gave its row.  *result: 0 not applicable, 1 passed, -1 failed ->
// screening off for this model.
int cls_screen_selftest(kh_model* m, int32_t* d_flag, bool inject, int* result) {
  const kh_config& c = m->cfg;
  kh_model::ClsScreen& s = m->scr;
  *result = 0;
  if (!s.on) return KH_OK;
  hipStream_t st = m->stream;
  const size_t V = (size_t)c.vocab_size;
  int32_t tok[2] = {-1, -2}, flag = 0;
  set_state(m, 1 % c.vocab_size, 0);
  int rc = cls_screen_pairs(m, tok, [&](const float* lb, const float* ub) {
    const size_t g = (V + KH_WG - 1) / KH_WG;
    hipLaunchKernelGGL(k_st_interval, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(KH_WG), 0, st, m->logits, lb, ub, V,
                       d_flag);
    return hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, st);
  });
  if (rc == KH_OK) rc = kh_launch_status();
  if (rc != KH_OK) return rc;
  *result = (flag || tok[0] != tok[1] || inject) ? -1 : 1;
  KH_CHECK_HIP(hipMemsetAsync(s.stats, 0, 4 * sizeof(int32_t), st));  // the counters describe the user's steps
  if (*result < 0) {
    fprintf(stderr, "[kh] classifier screen self-test failed (tokens %d / %d): screening is off for this model\n",
            tok[0], tok[1]);
    cls_screen_release(m);  // the copy's HBM goes back
    s.selftest = -1;
  } else {
    s.selftest = 1;
  }
  return KH_OK;
}

// One three-launch tail - tier 1 on grid1 workgroups (0: the planned grid), the bf16 screen of what it left, the
// re-score - then one full pair, on the vector now in m->x, without advancing.  tok[0] / tok[1]: the two tokens; the
// logits buffer holds k_cls's logits afterwards.  then(lb8, ub8): see cls_screen_pairs.
template <class F>
static int cls_screen_q8_pairs(kh_model* m, int grid1, int32_t* tok, F&& then) {
  hipStream_t st = m->stream;
  const size_t V = (size_t)m->cfg.vocab_size;
  KhDev<float> lb, ub;
  int rc;
  if ((rc = lb.alloc(V)) != KH_OK || (rc = ub.alloc(V)) != KH_OK) return rc;
  launch_cls_screen_q8(m, lb, ub, grid1);
  launch_cls_screen_behind(m, nullptr, nullptr, grid1 > 0 ? grid1 : m->scr.q8.grid);
  launch_sample(m, /*advance=*/0, /*n_forced=*/0, kScreen);
  hipError_t e = hipMemcpyAsync(&tok[0], m->d_next, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  launch_cls(m);
  launch_sample(m, 0, 0, kGreedy);
  if (e == hipSuccess) e = hipMemcpyAsync(&tok[1], m->d_next, sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = then(lb.get(), ub.get());
  // whatever was enqueued reads lb / ub: the stream drains before they go, on the failure paths too
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? KH_OK : (int)e;
}

// The tier's creation-time check: the embedding row of token 1 through the three-launch tail and through a full step.
// *result: 0 not applicable, 1 passed, -1 failed -> the tier is off for this model, the bf16 screen goes on.
int cls_screen_q8_selftest(kh_model* m, int32_t* d_flag, bool inject, int* result) {
  const kh_config& c = m->cfg;
  kh_model::ClsScreen& s = m->scr;
  *result = 0;
  if (!s.on || !s.q8.on) return KH_OK;
  hipStream_t st = m->stream;
  const size_t V = (size_t)c.vocab_size;
  int32_t tok[2] = {-1, -2}, flag = 0;
  set_state(m, 1 % c.vocab_size, 0);
  int rc = cls_screen_q8_pairs(m, 0, tok, [&](const float* lb, const float* ub) {
    const size_t g = (V + KH_WG - 1) / KH_WG;
    hipLaunchKernelGGL(k_st_interval, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(KH_WG), 0, st, m->logits, lb, ub, V,
                       d_flag);
    return hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, st);
  });
  if (rc == KH_OK) rc = kh_launch_status();
  if (rc != KH_OK) return rc;
  *result = (flag || tok[0] != tok[1] || inject) ? -1 : 1;
  KH_CHECK_HIP(hipMemsetAsync(s.stats, 0, 4 * sizeof(int32_t), st));  // the counters describe the user's steps
  KH_CHECK_HIP(hipMemsetAsync(s.q8.stats, 0, 4 * sizeof(int32_t), st));
  if (*result < 0) {
    fprintf(stderr, "[kh] classifier screen, int8 tier: self-test failed (tokens %d / %d): the tier is off for this "
                    "model\n", tok[0], tok[1]);
    KH_CHECK_HIP(hipStreamSynchronize(st));
    cls_screen_q8_release(m);  // the copy's HBM goes back
    s.q8.selftest = -1;
  } else {
    s.q8.selftest = 1;
  }
  return KH_OK;
}

}  // namespace khm
using namespace khm;

// One screened step and one full step on the caller's residual vector, without advancing (tests): the body of
// cls_screen_selftest above, through the same two launch functions a generate uses.  out[4]: screened token | full
// classifier's token | candidate rows re-scored | 1 if the step overflowed.  h_lb / h_ub: every row's interval.  The
// logits buffer is left holding k_cls's logits of that vector; the residual vector (m->x), the screen's saved input
// and d_next are overwritten (the next generate or step sets its own state).  The counters of
// kh_model_cls_screen_info are put back on every path that got as far as reading them.
extern "C" int kh_model_cls_screen_probe(kh_model* m, const float* h_x, float* h_lb, float* h_ub, int64_t* out) {
  if (!m || !h_x || !h_lb || !h_ub || !out) return KH_ERR_INVALID_ARG;
  const kh_model::ClsScreen& s = m->scr;
  if (!s.on || m->samp_on) return KH_ERR_UNSUPPORTED;
  const kh_config& c = m->cfg;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  hipStream_t st = m->stream;
  const size_t V = (size_t)c.vocab_size;
  int32_t tok[2] = {-1, -2}, h0[4] = {0, 0, 0, 0}, h1[4] = {0, 0, 0, 0};
  KH_CHECK_HIP(hipMemcpyAsync(h0, s.stats, sizeof(h0), hipMemcpyDeviceToHost, st));
  KH_CHECK_HIP(hipStreamSynchronize(st));
  hipError_t e = hipMemcpyAsync(m->x, h_x, sizeof(float) * (size_t)c.dim, hipMemcpyHostToDevice, st);
  int rc = e != hipSuccess ? (int)e : cls_screen_pairs(m, tok, [&](const float* lb, const float* ub) {
    hipError_t r = hipMemcpyAsync(h_lb, lb, sizeof(float) * V, hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipMemcpyAsync(h_ub, ub, sizeof(float) * V, hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipMemcpyAsync(h1, s.stats, sizeof(h1), hipMemcpyDeviceToHost, st);
    return r;
  });
  // the user's steps: also behind a failed copy or launch (h0 is pageable, so the copy has left it on return)
  e = hipMemcpyAsync(s.stats, h0, sizeof(h0), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (rc == KH_OK && e != hipSuccess) rc = (int)e;
  if (rc == KH_OK) rc = kh_launch_status();
  if (rc != KH_OK) return rc;
  out[0] = tok[0];
  out[1] = tok[1];
  out[2] = h1[1] - h0[1];
  out[3] = h1[2] - h0[2];
  return KH_OK;
}

// the bf16 copy [vocab x dim] and the per-row error table [vocab] (tests)
extern "C" int kh_model_cls_screen_read(kh_model* m, uint16_t* h_wbf, float* h_err) {
  if (!m || !h_wbf || !h_err) return KH_ERR_INVALID_ARG;
  const kh_model::ClsScreen& s = m->scr;
  if (!s.on) return KH_ERR_UNSUPPORTED;
  const size_t V = (size_t)m->cfg.vocab_size;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemcpyAsync(h_wbf, s.wbf, sizeof(uint16_t) * V * (size_t)m->cfg.dim, hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipMemcpyAsync(h_err, s.err, sizeof(float) * V, hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}

// out[8]: 0 screening on | 1 self-test (0 / 1 / -1) | 2 HBM bytes of the bf16 copy and its row table |
// 3 microseconds the conversion took | 4 screened steps so far | 5 candidate rows re-scored in them |
// 6 steps that overflowed into the full classifier | 7 candidate capacity of a step
extern "C" int kh_model_cls_screen_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  const kh_model::ClsScreen& s = m->scr;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = s.on ? 1 : 0;
  out[1] = s.selftest;
  out[2] = (int64_t)s.bytes;
  out[3] = (int64_t)(s.build_ms * 1000.f);
  out[7] = KH_SCR_CAND;
  if (s.on) {
    int32_t h[4] = {0, 0, 0, 0};
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    KH_CHECK_HIP(hipMemcpyAsync(h, s.stats, sizeof(h), hipMemcpyDeviceToHost, m->stream));
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    out[4] = h[0];
    out[5] = h[1];
    out[6] = h[2];
  }
  return KH_OK;
}

// The int8 tier (tests).  One non-advancing three-launch tail - k_cls_screen_q8 on `grid` workgroups (0: the planned
// grid), k_cls_screen in survivor mode, k_sample_screen - and one full step on the caller's residual vector.
// h_lb8 / h_ub8 [vocab]: tier 1's interval of every row.  out[6]: the tail's token | the full classifier's token | rows
// that survived tier 1 | 1 if tier 1 spilled (the bf16 launch then scanned every row) | candidate rows re-scored | 1 if
// the step overflowed.  The counters of both info calls are put back; the logits buffer holds k_cls's logits of h_x.
extern "C" int kh_model_cls_screen_q8_probe(kh_model* m, const float* h_x, int32_t grid, float* h_lb8, float* h_ub8,
                                            int64_t* out) {
  if (!m || !h_x || !h_lb8 || !h_ub8 || !out || grid < 0 || grid > 4096) return KH_ERR_INVALID_ARG;
  const kh_model::ClsScreen& s = m->scr;
  if (!s.on || !s.q8.on || m->samp_on) return KH_ERR_UNSUPPORTED;
  const kh_config& c = m->cfg;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  hipStream_t st = m->stream;
  const size_t V = (size_t)c.vocab_size;
  int32_t tok[2] = {-1, -2}, h0[8] = {0}, h1[8] = {0};
  KH_CHECK_HIP(hipMemcpyAsync(h0, s.stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  KH_CHECK_HIP(hipMemcpyAsync(h0 + 4, s.q8.stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  KH_CHECK_HIP(hipStreamSynchronize(st));
  hipError_t e = hipMemcpyAsync(m->x, h_x, sizeof(float) * (size_t)c.dim, hipMemcpyHostToDevice, st);
  int rc = e != hipSuccess ? (int)e : cls_screen_q8_pairs(m, grid, tok, [&](const float* lb, const float* ub) {
    hipError_t r = hipMemcpyAsync(h_lb8, lb, sizeof(float) * V, hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipMemcpyAsync(h_ub8, ub, sizeof(float) * V, hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipMemcpyAsync(h1, s.stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (r == hipSuccess) r = hipMemcpyAsync(h1 + 4, s.q8.stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    return r;
  });
  e = hipMemcpyAsync(s.stats, h0, 4 * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(s.q8.stats, h0 + 4, 4 * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (rc == KH_OK && e != hipSuccess) rc = (int)e;
  if (rc == KH_OK) rc = kh_launch_status();
  if (rc != KH_OK) return rc;
  out[0] = tok[0];
  out[1] = tok[1];
  out[2] = h1[5] - h0[5];
  out[3] = h1[6] - h0[6];
  out[4] = h1[1] - h0[1];
  out[5] = h1[2] - h0[2];
  return KH_OK;
}

// the int8 copy [vocab x dim], its scales [vocab x dim / 64] and its per-row error table [vocab] (tests)
extern "C" int kh_model_cls_screen_q8_read(kh_model* m, int8_t* h_q, float* h_sc, float* h_e8) {
  if (!m || !h_q || !h_sc || !h_e8) return KH_ERR_INVALID_ARG;
  const kh_model::ClsScreen::Q8& t = m->scr.q8;
  if (!t.on) return KH_ERR_UNSUPPORTED;
  const size_t V = (size_t)m->cfg.vocab_size, D = (size_t)m->cfg.dim;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  KH_CHECK_HIP(hipMemcpyAsync(h_q, t.q, V * D, hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipMemcpyAsync(h_sc, t.sc, sizeof(float) * V * (D / KH_SCR8_G), hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipMemcpyAsync(h_e8, t.e8, sizeof(float) * V, hipMemcpyDeviceToHost, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  return KH_OK;
}

// out[8]: 0 the tier is on | 1 self-test (0 / 1 / -1) | 2 HBM bytes of the int8 copy, its scales and its row table |
// 3 microseconds the conversion took | 4 tier-1 steps so far | 5 rows that survived tier 1 in them | 6 steps in which
// tier 1 spilled (the bf16 launch scanned every row) | 7 rows a tier-1 workgroup hands over
extern "C" int kh_model_cls_screen_q8_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  const kh_model::ClsScreen::Q8& t = m->scr.q8;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = t.on ? 1 : 0;
  out[1] = t.selftest;
  out[2] = (int64_t)t.bytes;
  out[3] = (int64_t)(t.build_ms * 1000.f);
  out[7] = KH_SCR8_C;
  if (t.on) {
    int32_t h[4] = {0, 0, 0, 0};
    KH_CHECK_HIP(hipSetDevice(m->opts.device));
    KH_CHECK_HIP(hipMemcpyAsync(h, t.stats, sizeof(h), hipMemcpyDeviceToHost, m->stream));
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    out[4] = h[0];
    out[5] = h[1];
    out[6] = h[2];
  }
  return KH_OK;
}
