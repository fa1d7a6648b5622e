// kh_model_selftest.hip — run-time self-checks of the two fast paths that are correct by test rather than by
// construction, executed once at the end of kh_model_create_* on the model's own device, weights and geometry:
//
//  (a) the int8 LDS-DMA ring kernels (kh_q8ring.h): their input-vector staging uses asm loads whose destination
//      registers the compiler believes written at the asm statement.  One launch of every adopted
//      ring kernel (ffn13 on the first layer's w1 / w3, the classifier) against the register-tile kernel of the same
//      launch on the same input, outputs compared word for word.  A mismatch turns the ring off for this model
//      (kh_config.ring_selftest = -1; the register-tile kernels are bit-identical by design, so nothing else changes).
//  (b) the fence-free in-launch merge of the decode-attention time splits (kh_attn.h::attn_publish_barrier, default
//      form): it leans on gfx950 behaviour the HIP memory model does not spell out.  One fenced launch gives the
//      reference, KH_SELFTEST_ATTN_LAUNCHES back-to-back fence-free launches of the same merge (per-head path and,
//      where the geometry has one, the GQA group path) must reproduce it word for word.  A mismatch makes this
//      model use the fenced form (kh_config.attn_merge_selftest = -1).
//  (c) the screened classifier of the greedy generate loop (kh_cls_screen.h; kh_model_screen.hip::cls_screen_selftest):
//      one screened step against one full step on a fixed vector - the same token, every full logit inside the
//      interval the screen gave its row.  A failure turns screening off for this model, frees the bf16 copy and says
//      so on stderr (kh_model_cls_screen_info reports -1).
//  (d) the int8 tier ahead of that screen (kh_model_screen.hip::cls_screen_q8_selftest): one three-launch tail against
//      one full step on the same vector - the same token, every full logit inside the interval tier 1 gave its row.
//      A failure turns the tier off and frees the int8 copy; the bf16 screen goes on (kh_model_cls_screen_q8_info: -1).
//  (e) W16 (kh_w16.h, kh_model_w16.hip): every launch class that runs on the 16-bit copy, once against the fp32 kernel
//      of the same launch - layer 0 or the classifier, a real embedding row as the residual stream - outputs compared
//      word for word.  A mismatch frees the copy and the model streams fp32 (kh_model_w16_info: state -2).  The
//      launches go by the copy's format, so an fp16-format copy (KH_FLAG_W16_F16) is checked through its _h16 kernels.
//  (f) Q4 (kh_q4.h, kh_model_q4.hip): every launch class that runs on the 4-bit copy, once against the int8 register-tile
//      kernel of the same launch - layer 0 or the classifier, a real embedding row as the residual stream - outputs
//      compared word for word.  A mismatch frees the copy and the model launches what it launches without the flag
//      (kh_model_q4_info: state -2).  (e) and (f) are one procedure, copy_selftest, told which copy to check.
//
// Both run on scratch state the model owns at that moment (activation buffers, rows of layer 0 of the still
// empty KV cache, which are zeroed again) in about a millisecond.  This is a tripwire for a part, a compiler or a
// partition mode on which the suite never ran - a race that shows once in a million launches will not trip it.
// Hooks (kh_debug_set / KH_* environment at load): KH_SELFTEST=0 skips both; KH_SELFTEST_FAIL="ring", "attn" or
// "ring,attn" (also "screen", "w16", "q4") reports the named comparison as failed (fault injection: tests/test_model_gpu.py checks that the
// fallbacks engage and that decode still matches the oracle).
// Replaces nothing in the reference (it has neither path); cf. kuiper/source/op/kernels/cuda/matmul_kernel.cu:56-87,
// mha_kernel.cu:47-130 for the kernels these paths stand in for.
#include <chrono>
#include <string.h>

#include "kh_model_internal.h"

#define KH_SELFTEST_ATTN_LAUNCHES 24

namespace {

__global__ __launch_bounds__(KH_WG) void k_st_fill(float* p, size_t n, uint32_t seed, float scale) {
  for (size_t i = (size_t)blockIdx.x * KH_WG + threadIdx.x; i < n; i += (size_t)gridDim.x * KH_WG) {
    uint32_t h = (uint32_t)i * 2654435761u ^ seed;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    p[i] = scale * ((float)(h & 0xffffu) / 32768.0f - 1.0f);
  }
}
// *flag |= (a[i] != b[i] for some i), compared as words (NaN == NaN when the bits agree)
__global__ __launch_bounds__(KH_WG) void k_st_diff(const uint32_t* a, const uint32_t* b, size_t n, int32_t* flag) {
  bool d = false;
  for (size_t i = (size_t)blockIdx.x * KH_WG + threadIdx.x; i < n; i += (size_t)gridDim.x * KH_WG) d |= a[i] != b[i];
  if (d) *flag = 1;
}
inline int grid_for(size_t n) {
  const size_t g = (n + KH_WG - 1) / KH_WG;
  return (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}
inline bool hook_has(const char* v, const char* word) { return v && strstr(v, word) != nullptr; }
// "screen" names the bf16 screen, "screen8" its int8 tier: the shorter word does not match inside the longer one
inline bool hook_has_screen(const char* v) {
  for (const char* p = v; p && (p = strstr(p, "screen")) != nullptr; p += 6)
    if (p[6] != '8') return true;
  return false;
}

}  // namespace

namespace khm {

// *result: 0 not applicable, 1 passed, -1 failed (fallback engaged); the return value is a KH / HIP status
static int ring_selftest(kh_model* m, int32_t* d_flag, bool inject, int* result) {
  const kh_config& c = m->cfg;
  *result = 0;
  if (!m->ring.ffn_r && !m->ring.cls_r) return KH_OK;  // no ring kernel planned for this model
  const kh_model::RingPlan plan = m->ring;
  hipStream_t s = m->stream;
  int rc = KH_OK;
  set_state(m, 1 % c.vocab_size, 0);  // x = a real embedding row
  // (a class on the 4-bit copy launches no ring kernel: kh_model_internal.h, KH_ON_Q4)
  if (plan.ffn_r && !q4_runs(m, KH_W16_FFN13)) {
    launch_ffn13(m, 0, /*ring=*/true);  // -> h1
    KH_CHECK_HIP(hipMemcpyAsync(m->h3, m->h1, sizeof(float) * (size_t)c.hidden_dim, hipMemcpyDeviceToDevice, s));
    launch_ffn13(m, 0, /*ring=*/false);  // register tiles -> h1
    hipLaunchKernelGGL(k_st_diff, dim3(grid_for((size_t)c.hidden_dim)), dim3(KH_WG), 0, s, (const uint32_t*)m->h1.get(),
                       (const uint32_t*)m->h3.get(), (size_t)c.hidden_dim, d_flag);
  }
  // scratch of the register-tile classifier; whatever is enqueued on it has run when a return below frees it (the
  // returns behind a launch follow a stream sync, and a device free waits for the device)
  KhDev<float> tmp_logits, tmp_pv;
  KhDev<int32_t> tmp_pi;
  if (plan.cls_r && !q4_runs(m, KH_W16_CLS)) {
    const size_t np = (size_t)(m->sh_cls.grid > plan.cls_grid ? m->sh_cls.grid : plan.cls_grid);
    if ((rc = tmp_logits.alloc((size_t)c.vocab_size)) != KH_OK || (rc = tmp_pv.alloc(np)) != KH_OK ||
        (rc = tmp_pi.alloc(np)) != KH_OK)
      return rc;
    launch_cls(m);  // ring -> logits
    launch_cls(m, {m->x, tmp_logits, tmp_pv, tmp_pi}, /*ring=*/false);  // register tiles -> tmp
    hipLaunchKernelGGL(k_st_diff, dim3(grid_for((size_t)c.vocab_size)), dim3(KH_WG), 0, s,
                       (const uint32_t*)m->logits.get(), (const uint32_t*)tmp_logits.get(), (size_t)c.vocab_size, d_flag);
  }
  int32_t flag = 0;
  KH_CHECK_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, s));
  KH_CHECK_HIP(hipStreamSynchronize(s));
  if ((rc = kh_launch_status()) != KH_OK) return rc;
  *result = 1;
  if (!flag && !inject) return KH_OK;
  // fall back: register-tile kernels for this model; the argmax partials follow the register-tile grid
  if (m->sh_cls.grid != m->nparts) {
    KhDev<float> pv;
    KhDev<int32_t> pi;
    if ((rc = pv.alloc((size_t)m->sh_cls.grid)) != KH_OK || (rc = pi.alloc((size_t)m->sh_cls.grid)) != KH_OK) return rc;
    m->part_val = std::move(pv);
    m->part_idx = std::move(pi);
    m->nparts = m->sh_cls.grid;
  }
  *result = -1;
  m->ring = kh_model::RingPlan();
  return KH_OK;
}

// one in-launch merge configuration: reference by the fenced form, then back-to-back fence-free launches
static int attn_merge_case(kh_model* m, int pos, int variant, int32_t* d_flag) {
  const kh_config& c = m->cfg;
  hipStream_t s = m->stream;
  set_state(m, 1 % c.vocab_size, pos);
  launch_attn(m, 0, variant, /*fenced=*/true);
  KH_CHECK_HIP(hipMemcpyAsync(m->rms, m->att, sizeof(float) * (size_t)c.dim, hipMemcpyDeviceToDevice, s));
  for (int i = 0; i < KH_SELFTEST_ATTN_LAUNCHES; ++i) {
    launch_attn(m, 0, variant, /*fenced=*/false);
    hipLaunchKernelGGL(k_st_diff, dim3(grid_for((size_t)c.dim)), dim3(KH_WG), 0, s, (const uint32_t*)m->att.get(),
                       (const uint32_t*)m->rms.get(), (size_t)c.dim, d_flag);
  }
  return kh_launch_status();
}

// *result: 0 not applicable, 1 passed, -1 failed (fenced form engaged), 2 the fenced form was requested
static int attn_selftest(kh_model* m, int32_t* d_flag, bool inject, int* result) {
  const kh_config& c = m->cfg;
  *result = 2;
  if (m->attn_fenced) return KH_OK;  // the caller asked for the fenced form (flag / hook): nothing to decide
  *result = 0;
  if (c.head_size <= 32 || m->attn_ns <= 1) return KH_OK;  // generic kernel / no time splits in this cache
  // per-head path, merge in the launch (what a step takes when it cannot defer the merge to wo)
  int pos1 = (c.cache_len < 1024 ? c.cache_len : 1024) - 1;
  if (pos1 + 1 >= m->attn_t_long) pos1 = m->attn_t_long - 2;
  const bool head_case = pos1 >= 1 && attn_active_splits(pos1, m->attn_ns, m->attn_ts_shift) >= 2;
  // GQA group path (always merged by its last arriver)
  int pos2 = -1;
  if (m->attn_ns_g > 0 && m->attn_t_long < c.cache_len) {
    pos2 = m->attn_t_long + 255 < c.cache_len ? m->attn_t_long + 255 : c.cache_len - 1;
    if (attn_active_splits(pos2, m->attn_ns_g, KH_ATTN_TSG_SHIFT) < 2) pos2 = -1;
  }
  if (!head_case && pos2 < 0) return KH_OK;
  const size_t rows = (size_t)((head_case ? pos1 : 0) > pos2 ? (head_case ? pos1 : 0) : pos2) + 1;
  const size_t n = rows * (size_t)c.kv_dim;
  hipStream_t s = m->stream;
  int rc = kv_ensure(m, (int)rows, /*layer=*/0);  // layer 0 only: the rows the check borrows
  if (rc != KH_OK) return rc;
  hipLaunchKernelGGL(k_st_fill, dim3(grid_for(n)), dim3(KH_WG), 0, s, m->kcache, n, 0x9e3779b9u, 1.0f);
  hipLaunchKernelGGL(k_st_fill, dim3(grid_for(n)), dim3(KH_WG), 0, s, m->vcache, n, 0x85ebca6bu, 1.0f);
  hipLaunchKernelGGL(k_st_fill, dim3(grid_for((size_t)c.dim)), dim3(KH_WG), 0, s, m->q, (size_t)c.dim, 0xc2b2ae35u, 1.0f);
  if (head_case) rc = attn_merge_case(m, pos1, m->attn_ns_g > 0 ? 2 : 0, d_flag);
  if (rc == KH_OK && pos2 >= 0) rc = attn_merge_case(m, pos2, 0, d_flag);
  int32_t flag = 0;
  hipError_t e = hipMemsetAsync(m->kcache, 0, n * sizeof(float), s);  // the cache is empty again
  if (e == hipSuccess) e = hipMemsetAsync(m->vcache, 0, n * sizeof(float), s);
  if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (rc != KH_OK) return rc;
  if (e != hipSuccess) return (int)e;
  *result = 1;
  if (!flag && !inject) return KH_OK;
  *result = -1;
  m->attn_fenced = true;
  return KH_OK;
}

// The weight copy `on` (KH_ON_W16 or KH_ON_Q4) against the image, class by class.
// *result: 0 not applicable, 1 passed, -1 failed (the copy is freed, every class back on the image's launch)
static int copy_selftest(kh_model* m, KhOn on, int32_t* d_flag, bool inject, int* result) {
  const kh_config& c = m->cfg;
  const bool q4 = on == KH_ON_Q4;
  kh_model::WCopy& w = q4 ? static_cast<kh_model::WCopy&>(m->q4) : m->w16;
  *result = 0;
  if (w.state != 1) return KH_OK;
  auto runs = [&](int cls) { return (w.classes & cls) != 0; };
  hipStream_t s = m->stream;
  const size_t dim = (size_t)c.dim, kv = (size_t)c.kv_dim, hid = (size_t)c.hidden_dim, voc = (size_t)c.vocab_size;
  // Both classifier launches below are register-tile launches.  (An fp32 model's m->nparts is this grid too: only a
  // ring plan makes the two differ - kh_model_load.hip -, and plan_ring has none for fp32.)
  const size_t np = (size_t)m->sh_cls.grid;
  // scratch: x as the check found it | outputs of the copy's launch (q, K row, V row | x | h | logits) | the image's
  // classifier outputs
  size_t tmp_n = dim + 2 * kv;
  if (hid > tmp_n) tmp_n = hid;
  if (voc > tmp_n) tmp_n = voc;
  KhDev<float> x0, tmp, ref, tmp_pv, ref_pv;
  KhDev<int32_t> tmp_pi, ref_pi;
  int rc = kv_ensure(m, 1, /*layer=*/0);  // the qkv launch writes row 0 of layer 0
  if (rc != KH_OK || (rc = x0.alloc(dim)) != KH_OK || (rc = tmp.alloc(tmp_n)) != KH_OK) return rc;
  if (runs(KH_W16_CLS) && ((rc = tmp_pv.alloc(np)) != KH_OK || (rc = tmp_pi.alloc(np)) != KH_OK)) return rc;
  // The image's classifier launch of a W16 model writes the model's own buffers: they hold these logits until the first
  // step (kh_model_get_logits of a fresh model).  A Q4 model's stay as they are.
  ClsIo ref_io{m->x, m->logits, m->part_val, m->part_idx};
  if (q4 && runs(KH_W16_CLS)) {
    if ((rc = ref.alloc(voc)) != KH_OK || (rc = ref_pv.alloc(np)) != KH_OK || (rc = ref_pi.alloc(np)) != KH_OK) return rc;
    ref_io = ClsIo{m->x, ref, ref_pv, ref_pi};
  }
  auto diff = [&](const void* a, const void* b, size_t n) {  // words, whatever they hold
    hipLaunchKernelGGL(k_st_diff, dim3(grid_for(n)), dim3(KH_WG), 0, s, (const uint32_t*)a, (const uint32_t*)b, n, d_flag);
  };
  auto copy = [&](float* dst, const float* src, size_t n) {
    return hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, s);
  };
  set_state(m, 1 % c.vocab_size, 0);  // x = a real embedding row
  hipError_t e = copy(x0, m->x, dim);
  if (runs(KH_W16_QKV) && e == hipSuccess) {
    launch_qkv(m, 0, on);  // -> q, row 0 of layer 0's K and V
    e = copy(tmp, m->q, dim);
    if (e == hipSuccess) e = copy(tmp + dim, m->kcache, kv);
    if (e == hipSuccess) e = copy(tmp + dim + kv, m->vcache, kv);
    launch_qkv(m, 0, KH_ON_IMAGE);
    diff(m->q, tmp, dim);
    diff(m->kcache, tmp + dim, kv);
    diff(m->vcache, tmp + dim + kv, kv);
    if (e == hipSuccess) e = hipMemsetAsync(m->kcache, 0, sizeof(float) * kv, s);  // the cache is empty again
    if (e == hipSuccess) e = hipMemsetAsync(m->vcache, 0, sizeof(float) * kv, s);
  } else if (runs(KH_W16_WO) && e == hipSuccess) {
    launch_qkv(m, 0, KH_ON_IMAGE);  // wo's vector below
    e = hipMemsetAsync(m->kcache, 0, sizeof(float) * kv, s);
    if (e == hipSuccess) e = hipMemsetAsync(m->vcache, 0, sizeof(float) * kv, s);
  }
  if (runs(KH_W16_WO) && e == hipSuccess) {  // x += wo . att, on the projected query as the vector
    e = copy(m->att, m->q, dim);
    launch_wo(m, 0, /*variant=*/0, on);
    if (e == hipSuccess) e = copy(tmp, m->x, dim);
    if (e == hipSuccess) e = copy(m->x, x0, dim);
    launch_wo(m, 0, /*variant=*/0, KH_ON_IMAGE);
    diff(m->x, tmp, dim);
  }
  if (runs(KH_W16_FFN13) && e == hipSuccess) {
    launch_ffn13(m, 0, /*ring=*/false, on);  // -> h1
    e = copy(tmp, m->h1, hid);
    launch_ffn13(m, 0, /*ring=*/false, KH_ON_IMAGE);
    diff(m->h1, tmp, hid);
  }
  if (runs(KH_W16_W2) && e == hipSuccess) {  // x += w2 . h1 (h1: what ffn13 left, or computed here)
    if (!runs(KH_W16_FFN13)) launch_ffn13(m, 0, /*ring=*/false, KH_ON_IMAGE);
    e = copy(x0, m->x, dim);
    launch_w2(m, 0, on);
    if (e == hipSuccess) e = copy(tmp, m->x, dim);
    if (e == hipSuccess) e = copy(m->x, x0, dim);
    launch_w2(m, 0, KH_ON_IMAGE);
    diff(m->x, tmp, dim);
  }
  if (runs(KH_W16_CLS) && e == hipSuccess) {
    launch_cls(m, {m->x, tmp, tmp_pv, tmp_pi}, /*ring=*/false, on);
    launch_cls(m, ref_io, /*ring=*/false, KH_ON_IMAGE);
    diff(ref_io.logits, tmp, voc);
    diff(ref_io.part_val, tmp_pv, np);
    diff(ref_io.part_idx, tmp_pi, np);
  }
  int32_t flag = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return (int)e;
  if ((rc = kh_launch_status()) != KH_OK) return rc;
  *result = 1;
  if (!flag && !inject) return KH_OK;
  *result = -1;
  q4 ? q4_release(m) : w16_release(m);
  w.state = -2;
  fprintf(stderr, "[kh] %s self-check %s: the model streams its %s matrices\n", q4 ? "Q4" : "W16",
          inject ? "reported as failed (hook)" : "FAILED", q4 ? "int8" : "fp32");
  return KH_OK;
}

// -> KH_OK, or a HIP / KH error when a launch itself failed (the model is then not usable).  Results in
// m->cfg.ring_selftest / attn_merge_selftest: 0 not applicable (or skipped), 1 passed, -1 failed -> fallback
// engaged, 2 (attention only) the fenced form was requested.
int run_selftests(kh_model* m) {
  m->cfg.ring_selftest = 0;
  m->cfg.attn_merge_selftest = m->attn_fenced ? 2 : 0;
  if (dbg_off("KH_SELFTEST")) return KH_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const char* inj = dbg("KH_SELFTEST_FAIL");
  KhDev<int32_t> d_flag;
  int rc;
  if ((rc = d_flag.alloc(6)) != KH_OK) return rc;
  int r = 0, a = 0, sc = 0, s8 = 0, w = 0, q4 = 0;
  KH_CHECK_HIP(hipMemsetAsync(d_flag, 0, 6 * sizeof(int32_t), m->stream));
  // W16 first: the checks behind it then run on the kernels the model will launch
  if ((rc = copy_selftest(m, KH_ON_W16, d_flag + 4, hook_has(inj, "w16"), &w)) != KH_OK) return rc;
  if ((rc = copy_selftest(m, KH_ON_Q4, d_flag + 5, hook_has(inj, "q4"), &q4)) != KH_OK) return rc;
  if ((rc = ring_selftest(m, d_flag, hook_has(inj, "ring"), &r)) != KH_OK) return rc;
  if ((rc = attn_selftest(m, d_flag + 1, hook_has(inj, "attn"), &a)) != KH_OK) return rc;
  if ((rc = cls_screen_selftest(m, d_flag + 2, hook_has_screen(inj), &sc)) != KH_OK) return rc;
  if ((rc = cls_screen_q8_selftest(m, d_flag + 3, hook_has(inj, "screen8"), &s8)) != KH_OK) return rc;
  m->cfg.ring_selftest = r;
  m->cfg.attn_merge_selftest = a;
  if (dbg("KH_LOAD_DEBUG") || dbg("KH_SHAPE_DEBUG"))
    fprintf(stderr, "[kh] self-tests: ring %d, attention merge %d, classifier screen %d, its int8 tier %d, W16 %d, Q4 %d (%.2f ms)\n", r, a, sc, s8, w, q4,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return KH_OK;
}

}  // namespace khm
