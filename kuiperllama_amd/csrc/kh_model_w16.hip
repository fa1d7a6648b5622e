// kh_model_w16.hip — W16 at the model level: the 16-bit copy of a bf16-exact (or, with KH_FLAG_W16_F16, fp16-exact)
// fp32 model's matrices (plan, exactness check, release, the class masks of decode and of the B-token passes) and
// kh_model_w16_info - and what W16 shares with the 4-bit copy of an int8 model (kh_model_q4.hip): the bytes of a copy,
// its build (arena, one build kernel over every matrix, per-tensor exactness flags), its release, and the routing of the
// decode GEMV launches on a copy to the translation unit of their source (the launch text: kh_copy_launch.h; the
// passes' launches: kh_model_prefill.hip, kh_model_h16_pass.hip).  The kernels here are kh_w16.h's _w16 ones; each
// launch is the image's launch of kh_model_step.hip with the same shape (split, u, grid, wg - a shape forced through
// KH_SHAPE_* included) on the twin of its kernel, so the bits do not change.
// Replaces nothing in the reference (it streams fp32 weights: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kh_copy_launch.h"

namespace khm {

// ---- what every weight copy shares (W16 in both formats, Q4: kh_model_q4.hip) -----------------------------------
namespace {
inline size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }
// the matrices a copy covers, in tensor-index order: {rows K, columns M} of wq, wk, wv, wo, w1, w2, w3
inline void layer_dims(int dim, int hidden, int kv_dim, size_t (&K)[7], size_t (&M)[7]) {
  const size_t d = (size_t)dim, h = (size_t)hidden, kv = (size_t)kv_dim;
  const size_t k[7] = {d, kv, kv, d, h, d, h}, mm[7] = {d, d, d, d, d, h, d};
  for (int i = 0; i < 7; ++i) {
    K[i] = k[i];
    M[i] = mm[i];
  }
}
}  // namespace

size_t copy_bytes(int dim, int hidden_dim, int kv_dim, int vocab_size, int layer_num, KhCopyMatBytes mat_bytes) {
  size_t K[7], M[7], total = 0;
  layer_dims(dim, hidden_dim, kv_dim, K, M);
  for (int i = 0; i < 7; ++i) total += pad256(mat_bytes(K[i] * M[i]));
  return total * (size_t)layer_num + pad256(mat_bytes((size_t)vocab_size * (size_t)dim));
}

void copy_release(kh_model::WCopy& w) {
  w.alloc.reset();
  w.arena = nullptr;
  w.classes = 0;
  w.bytes = 0;
  w.layers.clear();
  w.cls = nullptr;
}

int copy_build(kh_model* m, kh_model::WCopy& w, KhCopyBuildKernel kernel, KhCopyMatBytes mat_bytes, int per_item,
               size_t bytes, int* first) {
  const kh_config& c = m->cfg;
  const int nt = 7 * c.layer_num + 1;
  int rc;
  if (!w.arena) {
    if ((rc = w.alloc.alloc(bytes + 4096)) != KH_OK) return rc;
    w.arena = (char*)(((uintptr_t)w.alloc.get() + 4095) & ~(uintptr_t)4095);
    w.layers.resize((size_t)c.layer_num);
  }
  KhDev<uint32_t> d_flags;  // per tensor: some value is not exact in the copy being built
  if ((rc = d_flags.alloc((size_t)nt)) != KH_OK) return rc;
  hipStream_t s = m->stream;
  size_t K[7], M[7], off = 0;
  layer_dims(c.dim, c.hidden_dim, c.kv_dim, K, M);
  hipError_t e = hipMemsetAsync(d_flags, 0, sizeof(uint32_t) * (size_t)nt, s);
  if (e == hipSuccess) e = hipEventRecord(m->ev0, s);
  auto build = [&](const void* src, size_t elems, int tensor) -> const void* {
    char* dst = w.arena + off;
    off += pad256(mat_bytes(elems));
    const size_t n = elems / (size_t)per_item, need = (n + KH_WG - 1) / KH_WG;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(need < 4096 ? (need ? need : 1) : 4096)), dim3(KH_WG), 0, s,
                       (const u32x4*)src, (u32x2*)dst, n, d_flags + tensor);
    return dst;
  };
  for (int l = 0; l < c.layer_num && e == hipSuccess; ++l) {
    const LayerW& W = m->layers[(size_t)l];
    const void* src[7] = {W.wq.w, W.wk.w, W.wv.w, W.wo.w, W.w1.w, W.w2.w, W.w3.w};
    const void* dst[7];
    for (int i = 0; i < 7; ++i) dst[i] = build(src[i], K[i] * M[i], 7 * l + i);
    w.layers[(size_t)l] = kh_model::WCopy::Layer{dst[0], dst[1], dst[2], dst[3], dst[4], dst[5], dst[6]};
  }
  w.cls = build(m->cls.w, (size_t)c.vocab_size * (size_t)c.dim, nt - 1);  // tok_emb when the classifier is tied
  std::vector<uint32_t> flags((size_t)nt, 0);
  if (e == hipSuccess) e = hipEventRecord(m->ev1, s);
  if (e == hipSuccess) e = hipMemcpyAsync(flags.data(), d_flags, sizeof(uint32_t) * (size_t)nt, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  rc = e == hipSuccess ? kh_launch_status() : (int)e;
  if (rc == KH_OK && off != bytes) rc = KH_ERR_INTERNAL;
  if (rc != KH_OK) return rc;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, m->ev0, m->ev1) == hipSuccess) w.build_us += ms * 1000.f;
  *first = -1;
  for (int t = 0; t < nt && *first < 0; ++t)
    if (flags[(size_t)t]) *first = t;
  return KH_OK;
}

// ---- W16 ------------------------------------------------------------------------------------------
static size_t w16_mat_bytes(size_t elems) { return 2 * elems; }  // either format

// Which launch classes run on the copy.  Every class does: in the same-box A/B (tools/w16_ab.py, profiles/w16_ab.txt)
// each class's W16 median lies below its fp32 median by more than the range of the fp32 runs on all four geometries
// (smallest margin: Qwen2.5-0.5B's qkv, 2.90 -> 2.85 us).  A class that one takes out here keeps its fp32 kernel and
// costs nothing but its bytes in the copy.
int plan_w16(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size, int layer_num, size_t* bytes) {
  if (bytes) *bytes = 0;
  if (quant || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0 || layer_num <= 0) return 0;
  if (dim % 4 != 0 || hidden_dim % 4 != 0) return 0;  // a lane's unit is four columns
  if (bytes) *bytes = copy_bytes(dim, hidden_dim, kv_dim, vocab_size, layer_num, w16_mat_bytes);
  return KH_W16_ALL;
}

void w16_release(kh_model* m) {
  copy_release(m->w16);
  m->w16.pass_classes = 0;
  if (m->w16.gemm_classes) m->w16.gemm_reason = KH_GEMM16_SELFCHECK;  // a live copy given up: the self-check's verdict
  m->w16.gemm_classes = 0;
  m->w16.format = KH_W16_BF16;
}

// Which classes run their B-token pass (kh_w16_pass.h) on the copy as well: those of KH_W16_PASS_DEFAULT that decode
// adopted.  Hook KH_W16_PASS, read at creation: unset or 1 - that default; 0 - none (the passes stream fp32 while decode
// reads the copy); any other number (strtol, base 0: 0x1f, 12, 0x1 for qkv alone) - a mask of KH_W16_* bits.
static int w16_pass_mask() {
  const char* hook = dbg("KH_W16_PASS");
  if (!hook || strcmp(hook, "1") == 0) return KH_W16_PASS_DEFAULT;
  return (int)strtol(hook, nullptr, 0) & KH_W16_ALL;
}

// ---- KH_FLAG_GEMM16: the GEMM pass on the bf16 matrix cores (kh_gemm_w16.h) ------------------------------------
// Classes that run their GEMMs of the GEMM pass on the copy unless KH_GEMM16_CLASSES says otherwise: 3.1e's adoption
// rule - the class's time with the flag on lies below its flag-off time by more than the run-to-run range, at 512
// tokens, on Llama-3.2-1B and on Llama-2-7B geometry (profiles/gemm16_ab.txt: qkv -2.4 / -8.1 %, wo -1.2 / -2.4 %,
// ffn13 -14.3 / -13.1 %, w2 -4.9 / -6.0 % of the whole 512-token prefill; cls -3.2 % of a 64-lane batch on the 1B
// geometry but -0.1 %, inside the range, on the 7B one: left out) - among the classes whose contraction length K is a multiple of the
// 32-column block: qkv, wo, ffn13 and cls contract over dim, w2 over hidden_dim.
enum { KH_GEMM16_DEFAULT = KH_W16_QKV | KH_W16_WO | KH_W16_FFN13 | KH_W16_W2 };
static int gemm16_k32_classes(int dim, int hidden_dim) {
  return (dim % 32 == 0 ? KH_W16_QKV | KH_W16_WO | KH_W16_FFN13 | KH_W16_CLS : 0) | (hidden_dim % 32 == 0 ? KH_W16_W2 : 0);
}
int plan_gemm16(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size) {
  if (quant || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0) return 0;
  if (dim % 16 || hidden_dim % 16 || kv_dim % 16) return 0;  // pg_supported's granules of an fp32 model
  return KH_GEMM16_DEFAULT & gemm16_k32_classes(dim, hidden_dim);
}
// Read at creation, behind the copy's build.  Hooks: KH_GEMM16=1 / 0 overrides the flag; KH_GEMM16_CLASSES=<number>
// (strtol, base 0) replaces the adoption mask - the K % 32 rule still holds.
static void gemm16_configure(kh_model* m, bool w16_wanted) {
  const kh_config& c = m->cfg;
  kh_model::W16& w = m->w16;
  w.gemm_classes = w.gemm_plan = 0;
  const char* hook = dbg("KH_GEMM16");
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_GEMM16) != 0;
  if (!want) { w.gemm_reason = KH_GEMM16_NO_FLAG; return; }
  if (c.is_quant) { w.gemm_reason = KH_GEMM16_QUANT; return; }
  if (!w16_wanted) { w.gemm_reason = KH_GEMM16_NO_W16; return; }
  if (w.state != 1) { w.gemm_reason = w.state == -1 ? KH_GEMM16_INEXACT : KH_GEMM16_GEOMETRY; return; }
  if (w.format != KH_W16_BF16) { w.gemm_reason = KH_GEMM16_FP16_COPY; return; }
  if (!pg_supported(m)) { w.gemm_reason = KH_GEMM16_GEOMETRY; return; }
  w.gemm_plan = plan_gemm16(false, c.dim, c.hidden_dim, c.kv_dim, c.vocab_size);
  int mask = w.gemm_plan;
  if (const char* cl = dbg("KH_GEMM16_CLASSES"))
    mask = (int)strtol(cl, nullptr, 0) & gemm16_k32_classes(c.dim, c.hidden_dim);
  w.gemm_classes = mask & w.classes;
  w.gemm_reason = w.gemm_classes ? KH_GEMM16_ON : KH_GEMM16_NO_CLASS;
}

// The copy in the first format the image is exact in: bf16 (KH_FLAG_W16 or KH_FLAG_W16_F16), else fp16 (only
// KH_FLAG_W16_F16; into the same arena - plan_w16's layout holds for both), else none.  All or nothing per format.
static int w16_create_copy(kh_model* m, bool* wanted);
int w16_create(kh_model* m) {
  bool wanted = false;
  const int rc = w16_create_copy(m, &wanted);
  if (rc == KH_OK) gemm16_configure(m, wanted);
  return rc;
}
static int w16_create_copy(kh_model* m, bool* wanted) {
  const kh_config& c = m->cfg;
  kh_model::W16& w = m->w16;
  w = kh_model::W16();
  const char* hook = dbg("KH_W16");
  const char* hook_f16 = dbg("KH_W16_F16");
  const bool try_f16 = hook_f16 ? hook_f16[0] == '1' : (m->opts.flags & KH_FLAG_W16_F16) != 0;
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_W16) != 0 || try_f16;
  *wanted = want;
  if (!want) return KH_OK;
  size_t bytes = 0;
  const int classes = plan_w16(c.is_quant != 0, c.dim, c.hidden_dim, c.kv_dim, c.vocab_size, c.layer_num, &bytes);
  if (!classes) return KH_OK;  // int8, or a geometry the view does not cover: nothing changes
  int first = -1, first_f16 = -1, format = KH_W16_BF16;
  int rc = copy_build(m, w, k_w16_build, w16_mat_bytes, 4, bytes, &first);
  if (rc == KH_OK && first >= 0 && try_f16) {
    format = KH_W16_F16;
    rc = copy_build(m, w, k_h16_build, w16_mat_bytes, 4, bytes, &first_f16);
  }
  if (rc != KH_OK) {
    w16_release(m);
    return rc;
  }
  w.first_inexact = first;
  w.first_inexact_f16 = first_f16;
  if (format == KH_W16_BF16 ? first >= 0 : first_f16 >= 0) {  // all or nothing: the model streams fp32 as if no flag were set
    w16_release(m);
    w.state = -1;
    return KH_OK;
  }
  w.bytes = bytes;
  w.format = format;
  format == KH_W16_F16 ? copy_configure<KH_SRC_F16>(m) : copy_configure<KH_SRC_BF16>(m);
  w.classes = classes;
  w.pass_classes = classes & w16_pass_mask();
  w.state = 1;
  if (dbg("KH_LOAD_DEBUG") || dbg("KH_SHAPE_DEBUG"))
    fprintf(stderr, "[kh] W16: %.1f MiB %s copy of %d matrices in %.0f us, classes 0x%x, passes 0x%x\n",
            (double)bytes / (1 << 20), format == KH_W16_F16 ? "fp16" : "bf16", 7 * c.layer_num + 1, (double)w.build_us,
            (unsigned)classes, (unsigned)w.pass_classes);
  return KH_OK;
}

// ---- the launches on a copy (kh_copy_launch.h) -------------------------------------------------------
// This translation unit compiles the _w16 kernels; an fp16-format copy goes to kh_model_h16.hip and the 4-bit copy to
// kh_model_q4.hip, which compile the _h16 and _q4 kernels from the same launch text.
KH_COPY_LAUNCHES(, KH_SRC_BF16);
// fn<source>(...): the 4-bit copy where the launch is on it, else the 16-bit copy in its format
#define KH_COPY_ROUTE(fn, m, on, ...)                             \
  ((on) == KH_ON_Q4                ? fn<KH_SRC_Q4>(__VA_ARGS__)   \
   : (m)->w16.format == KH_W16_F16 ? fn<KH_SRC_F16>(__VA_ARGS__)  \
                                   : fn<KH_SRC_BF16>(__VA_ARGS__))
void copy_launch_qkv(kh_model* m, int l, KhOn on, const KhQkvArgs& a) { KH_COPY_ROUTE(copy_qkv, m, on, m, l, a); }
void copy_launch_wo(kh_model* m, int l, KhOn on, const KhGemvResArgs& a) { KH_COPY_ROUTE(copy_wo, m, on, m, l, a); }
void copy_launch_wo_comb(kh_model* m, int l, KhOn on, const KhWoCombArgs& a) { KH_COPY_ROUTE(copy_wo_comb, m, on, m, l, a); }
void copy_launch_ffn13(kh_model* m, int l, KhOn on, const KhFfn13Args& a) { KH_COPY_ROUTE(copy_ffn13, m, on, m, l, a); }
void copy_launch_w2(kh_model* m, int l, KhOn on, const KhGemvResArgs& a) { KH_COPY_ROUTE(copy_w2, m, on, m, l, a); }
void copy_launch_cls(kh_model* m, KhOn on, const KhClsArgs& a) { KH_COPY_ROUTE(copy_cls, m, on, m, a); }

}  // namespace khm
using namespace khm;

// out2 = {KH_W16_* bits of the launch classes that run on the copy (0: not applicable), bytes of the copy}
extern "C" int kh_plan_w16(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t layer_num,
                           int32_t is_quant, int64_t* out2) {
  if (!out2 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0 || layer_num <= 0) return KH_ERR_INVALID_ARG;
  size_t bytes = 0;
  out2[0] = plan_w16(is_quant != 0, dim, hidden_dim, kv_dim, vocab_size, layer_num, &bytes);
  out2[1] = (int64_t)bytes;
  return KH_OK;
}

extern "C" int kh_model_w16_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  memset(out, 0, 8 * sizeof(int64_t));
  out[0] = m->w16.state;
  out[1] = (int64_t)m->w16.bytes;
  out[2] = (int64_t)m->w16.build_us;
  out[3] = m->w16.classes;
  out[4] = m->w16.first_inexact;
  out[5] = m->w16.pass_classes;
  out[6] = m->w16.format == KH_W16_F16;
  out[7] = m->w16.first_inexact_f16 + 1;
  return KH_OK;
}

// out2 = {KH_W16_* bits of the launch classes whose GEMM-pass GEMMs run on the bf16 matrix cores under KH_FLAG_GEMM16
// (0: not applicable), the columns of a K block}
extern "C" int kh_plan_gemm16(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t is_quant,
                              int64_t* out2) {
  if (!out2 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0) return KH_ERR_INVALID_ARG;
  out2[0] = plan_gemm16(is_quant != 0, dim, hidden_dim, kv_dim, vocab_size);
  out2[1] = 32;
  return KH_OK;
}

extern "C" int kh_model_gemm16_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  memset(out, 0, 8 * sizeof(int64_t));
  const bool on = m->w16.state == 1 && m->w16.gemm_classes != 0;
  out[0] = on;
  out[1] = on ? m->w16.gemm_classes : 0;
  out[2] = on ? KH_GEMM16_ON : m->w16.gemm_reason;
  out[3] = m->w16.gemm_plan;
  return KH_OK;
}
