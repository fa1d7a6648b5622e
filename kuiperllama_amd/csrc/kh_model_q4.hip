// kh_model_q4.hip — Q4 at the model level: the packed 4-bit copy of a 4-bit-exact int8 model's matrices (plan, build,
// range check, release, the class mask), the decode GEMV launches that read it and kh_model_q4_info.  The kernels are
// kh_q4.h's; each launch is the int8 launch of kh_model_step.hip with the same shape (split, u, grid, wg - a shape
// forced through KH_SHAPE_* included) on the Q4 twin of its kernel, so the bits do not change.
// Replaces nothing in the reference (it streams int8 weights: kuiper/source/op/kernels/cuda/matmul_kernel.cu:56-87).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kh_dispatch.h"
#include "kh_q4.h"
#include "kh_model_internal.h"

namespace khm {

namespace {
inline size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }
// the matrices the copy covers, in tensor-index order: {rows K, columns M} of wq, wk, wv, wo, w1, w2, w3
inline void layer_dims(int dim, int hidden, int kv_dim, size_t (&K)[7], size_t (&M)[7]) {
  const size_t d = (size_t)dim, h = (size_t)hidden, kv = (size_t)kv_dim;
  const size_t k[7] = {d, kv, kv, d, h, d, h}, mm[7] = {d, d, d, d, d, h, d};
  for (int i = 0; i < 7; ++i) {
    K[i] = k[i];
    M[i] = mm[i];
  }
}
// Launch classes that run on the copy unless KH_Q4_CLASSES says otherwise: those that pass 3.1c's adoption rule - the Q4
// median below the flag-off median by more than the range of the flag-off runs - on both geometries of the same-box
// A/B (tools/q4_ab.py, profiles/q4_ab.txt).  qkv and wo are out: both pass at Llama-2-7B geometry (10.91
// -> 9.45 us, 5.09 -> 4.61 us) and lose at TinyLlama's (3.36 -> 3.54 us, 2.82 -> 2.84 us); KH_Q4_CLASSES=0x1f puts them
// back.  A class that is out keeps its int8 launch and costs nothing but its bytes in the copy.
enum { KH_Q4_DEFAULT = KH_W16_FFN13 | KH_W16_W2 | KH_W16_CLS };
}  // namespace

int plan_q4(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size, int layer_num, int group_size,
            size_t* bytes) {
  if (bytes) *bytes = 0;
  if (!quant || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0 || layer_num <= 0) return 0;
  // a lane's unit is sixteen columns of one group (the int8 view's own premise)
  if (group_size < 16 || (group_size & (group_size - 1)) != 0 || dim % group_size != 0 || hidden_dim % group_size != 0)
    return 0;
  size_t K[7], M[7], total = 0;
  layer_dims(dim, hidden_dim, kv_dim, K, M);
  for (int i = 0; i < 7; ++i) total += pad256(K[i] * M[i] / 2);
  total *= (size_t)layer_num;
  total += pad256((size_t)vocab_size * (size_t)dim / 2);
  if (bytes) *bytes = total;
  return KH_Q4_DEFAULT;
}

void q4_release(kh_model* m) {
  kh_model::Q4& q = m->q4;
  if (q.classes & KH_W16_CLS) m->nparts = q.nparts_image;  // the int8 classifier launch's partials again
  q.alloc.reset();
  q.arena = nullptr;
  q.classes = 0;
  q.bytes = 0;
  q.layers.clear();
  q.cls = nullptr;
}

// Hook KH_Q4_CLASSES, read at creation: unset - the plan's classes; a number (strtol, base 0: 0x1f, 12, 0x1 for qkv
// alone, 0 for none) - a mask of KH_W16_* bits, whatever the plan says (the tests reach every kernel through it)
static int q4_class_mask(int planned) {
  const char* hook = dbg("KH_Q4_CLASSES");
  return hook ? (int)strtol(hook, nullptr, 0) & KH_W16_ALL : planned;
}

// >64 KiB dynamic-LDS opt-in of the gemv_res twin as w2 (configure_step_kernels does it for k_gemv_res)
static void q4_configure(const kh_model* m) {
  const size_t lds_need = fused_lds_bytes(true, m->cfg.hidden_dim);
  if (lds_need <= 64 * 1024) return;
  GemvResU<true>::each([&](auto U) {
    GemvResSP::each([&](auto SP) {
      KhVals<0, 6>::each([&](auto MV) {
        (void)hipFuncSetAttribute(
            (const void*)k_gemv_res_q4<decltype(U)::value, decltype(MV)::value, decltype(SP)::value>,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_need);
      });
    });
  });
}

// All or nothing: one value outside [-8, 7] anywhere and the model launches what it launches without the flag.
int q4_create(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::Q4& q = m->q4;
  q = kh_model::Q4();
  const char* hook = dbg("KH_Q4");
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_Q4) != 0;
  if (!want) return KH_OK;
  size_t bytes = 0;
  const int planned =
      plan_q4(c.is_quant != 0, c.dim, c.hidden_dim, c.kv_dim, c.vocab_size, c.layer_num, c.group_size, &bytes);
  if (!bytes) return KH_OK;  // fp32, or a geometry the view does not cover: nothing changes
  const int nt = 7 * c.layer_num + 1;
  KhDev<uint32_t> d_flags;  // per tensor: some value lies outside [-8, 7]
  int rc;
  if ((rc = q.alloc.alloc(bytes + 4096)) != KH_OK || (rc = d_flags.alloc((size_t)nt)) != KH_OK) {
    q4_release(m);
    return rc;
  }
  q.arena = (char*)(((uintptr_t)q.alloc.get() + 4095) & ~(uintptr_t)4095);
  q.layers.resize((size_t)c.layer_num);
  hipStream_t s = m->stream;
  size_t K[7], M[7], off = 0;
  layer_dims(c.dim, c.hidden_dim, c.kv_dim, K, M);
  hipError_t e = hipMemsetAsync(d_flags, 0, sizeof(uint32_t) * (size_t)nt, s);
  if (e == hipSuccess) e = hipEventRecord(m->ev0, s);
  auto build = [&](const void* src, size_t elems, int tensor) -> const void* {
    char* dst = q.arena + off;
    off += pad256(elems / 2);
    const size_t n16 = elems / 16, need = (n16 + KH_WG - 1) / KH_WG;
    hipLaunchKernelGGL(k_q4_build, dim3((unsigned)(need < 4096 ? (need ? need : 1) : 4096)), dim3(KH_WG), 0, s,
                       (const u32x4*)src, (u32x2*)dst, n16, d_flags + tensor);
    return dst;
  };
  for (int l = 0; l < c.layer_num && e == hipSuccess; ++l) {
    const LayerW& W = m->layers[(size_t)l];
    const void* src[7] = {W.wq.w, W.wk.w, W.wv.w, W.wo.w, W.w1.w, W.w2.w, W.w3.w};
    const void* dst[7];
    for (int i = 0; i < 7; ++i) dst[i] = build(src[i], K[i] * M[i], 7 * l + i);
    q.layers[(size_t)l] = kh_model::W16::Layer{dst[0], dst[1], dst[2], dst[3], dst[4], dst[5], dst[6]};
  }
  q.cls = build(m->cls.w, (size_t)c.vocab_size * (size_t)c.dim, nt - 1);
  std::vector<uint32_t> flags((size_t)nt, 0);
  if (e == hipSuccess) e = hipEventRecord(m->ev1, s);
  if (e == hipSuccess) e = hipMemcpyAsync(flags.data(), d_flags, sizeof(uint32_t) * (size_t)nt, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  rc = e == hipSuccess ? kh_launch_status() : (int)e;
  if (rc == KH_OK && off != bytes) rc = KH_ERR_INTERNAL;
  if (rc != KH_OK) {
    q4_release(m);
    return rc;
  }
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, m->ev0, m->ev1) == hipSuccess) q.build_us = ms * 1000.f;
  for (int t = 0; t < nt && q.first_inexact < 0; ++t)
    if (flags[(size_t)t]) q.first_inexact = t;
  if (q.first_inexact >= 0) {  // the model streams int8 as if no flag were set
    q4_release(m);
    q.state = -1;
    return KH_OK;
  }
  const int classes = q4_class_mask(planned);
  // A classifier on the copy launches the register-tile grid where the model planned the ring kernel's: the argmax
  // partials follow it (room for the larger of the two, so that a copy given up later needs no allocation)
  q.nparts_image = m->nparts;
  if ((classes & KH_W16_CLS) && m->sh_cls.grid != m->nparts) {
    if (m->sh_cls.grid > m->nparts) {
      KhDev<float> pv;
      KhDev<int32_t> pi;
      if ((rc = pv.alloc((size_t)m->sh_cls.grid)) != KH_OK || (rc = pi.alloc((size_t)m->sh_cls.grid)) != KH_OK) {
        q4_release(m);
        return rc;
      }
      m->part_val = std::move(pv);
      m->part_idx = std::move(pi);
    }
    m->nparts = m->sh_cls.grid;
  }
  q.bytes = bytes;
  q4_configure(m);
  q.classes = classes;
  q.state = 1;
  if (dbg("KH_LOAD_DEBUG") || dbg("KH_SHAPE_DEBUG"))
    fprintf(stderr, "[kh] Q4: %.1f MiB 4-bit copy of %d matrices in %.0f us, classes 0x%x\n", (double)bytes / (1 << 20),
            nt, (double)q.build_us, (unsigned)classes);
  return KH_OK;
}

// ---- the launches ----------------------------------------------------------------------------
namespace {
// f(U, MV, SP) from the int8 lists of a kernel (pick_fused without its QUANT level: a Q4 kernel has no fp32 form)
template <class US, class MVS, class SPS, class F>
void pick_q4(int u, int mv, int sp, F&& f) {
  kh_pick_ge(US{}, u, [&](auto U) {
    kh_pick(MVS{}, mv, [&](auto MV) { kh_pick(SPS{}, sp, [&](auto SP) { f(U, MV, SP); }); });
  });
}
}  // namespace

void q4_launch_qkv(kh_model* m, int l, const KhQkvArgs& int8) {
  const kh_config& c = m->cfg;
  KhQkvArgs a = int8;
  const kh_model::W16::Layer& W = m->q4.layers[(size_t)l];
  a.wq.w = W.wq;
  a.wk.w = W.wk;
  a.wv.w = W.wv;
  const kh_model::Shape& sh = m->sh_qkv;
  pick_q4<FusedU<true>, FusedMV, QkvSP>(sh.u, kh_stage_maxv(c.dim, sh.wg), sh.split, [&](auto U, auto MV, auto SP) {
    kh_launch(KH_KERNEL(k_qkv_q4, U, MV, SP), sh.grid, sh.wg, fused_lds_bytes(true, c.dim), m->stream, a);
  });
}
void q4_launch_wo(kh_model* m, int l, const KhGemvResArgs& int8) {
  const kh_config& c = m->cfg;
  KhGemvResArgs a = int8;
  a.w.w = m->q4.layers[(size_t)l].wo;
  const kh_model::Shape& sh = m->sh_wo;
  pick_q4<FusedU<true>, FusedMV, GemvResSP>(sh.u, kh_stage_maxv(c.dim, sh.wg), sh.split, [&](auto U, auto MV, auto SP) {
    kh_launch(KH_KERNEL(k_gemv_res_q4, U, MV, SP), sh.grid, sh.wg, fused_lds_bytes(true, c.dim), m->stream, a);
  });
}
void q4_launch_wo_comb(kh_model* m, int l, const KhWoCombArgs& int8) {
  const kh_config& c = m->cfg;
  KhWoCombArgs a = int8;
  a.g.w.w = m->q4.layers[(size_t)l].wo;
  const kh_model::Shape& sh = m->sh_wo;
  pick_q4<FusedU<true>, WoCombMV, GemvResSP>(sh.u, c.dim <= 2 * 4 * sh.wg ? 2 : 4, sh.split, [&](auto U, auto MV, auto SP) {
    kh_launch(KH_KERNEL(k_wo_comb_q4, U, MV, SP), sh.grid, sh.wg, comb_lds_bytes(true, c.dim, c.head_num), m->stream, a);
  });
}
void q4_launch_ffn13(kh_model* m, int l, const KhFfn13Args& int8) {
  const kh_config& c = m->cfg;
  KhFfn13Args a = int8;
  a.w1.w = m->q4.layers[(size_t)l].w1;
  a.w3.w = m->q4.layers[(size_t)l].w3;
  const kh_model::Shape& sh = m->sh_ffn;
  pick_q4<FusedU<true>, FusedMV, NoSP>(sh.u, kh_stage_maxv(c.dim, sh.wg), 1, [&](auto U, auto MV, auto) {
    kh_launch(KH_KERNEL(k_ffn13_q4, U, MV), sh.grid, sh.wg, fused_lds_bytes(true, c.dim), m->stream, a);
  });
}
void q4_launch_w2(kh_model* m, int l, const KhGemvResArgs& int8) {
  const kh_config& c = m->cfg;
  KhGemvResArgs a = int8;
  a.w.w = m->q4.layers[(size_t)l].w2;
  const kh_model::Shape& sh = m->sh_w2;
  pick_q4<GemvResU<true>, GemvResMV, GemvResSP>(sh.u, kh_stage_maxv(c.hidden_dim, sh.wg), sh.split,
                                                [&](auto U, auto MV, auto SP) {
    kh_launch(KH_KERNEL(k_gemv_res_q4, U, MV, SP), sh.grid, sh.wg, fused_lds_bytes(true, c.hidden_dim), m->stream, a);
  });
}
void q4_launch_cls(kh_model* m, const KhClsArgs& int8) {
  const kh_config& c = m->cfg;
  KhClsArgs a = int8;
  a.wcls.w = m->q4.cls;
  const kh_model::Shape& sh = m->sh_cls;
  pick_q4<FusedU<true>, FusedMV, NoSP>(sh.u, kh_stage_maxv(c.dim, sh.wg), 1, [&](auto U, auto MV, auto) {
    kh_launch(KH_KERNEL(k_cls_q4, U, MV), sh.grid, sh.wg, cls_lds_bytes(true, c.dim), m->stream, a);
  });
}

}  // namespace khm
using namespace khm;

// out2 = {KH_W16_* bits of the launch classes that run on the 4-bit copy (0: not applicable), bytes of the copy}
extern "C" int kh_plan_q4(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t layer_num,
                          int32_t is_quant, int32_t group_size, int64_t* out2) {
  if (!out2 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0 || layer_num <= 0) return KH_ERR_INVALID_ARG;
  size_t bytes = 0;
  out2[0] = plan_q4(is_quant != 0, dim, hidden_dim, kv_dim, vocab_size, layer_num, group_size, &bytes);
  out2[1] = (int64_t)bytes;
  return KH_OK;
}

// out[0..4] = state, bytes, build us, class mask, first inexact tensor
extern "C" int kh_model_q4_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  memset(out, 0, 8 * sizeof(int64_t));
  out[0] = m->q4.state;
  out[1] = (int64_t)m->q4.bytes;
  out[2] = (int64_t)m->q4.build_us;
  out[3] = m->q4.classes;
  out[4] = m->q4.first_inexact;
  return KH_OK;
}
