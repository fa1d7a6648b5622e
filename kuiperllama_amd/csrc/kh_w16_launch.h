// kh_w16_launch.h — the decode GEMV launches on the 16-bit copy, written once for both formats of the copy (kh_w16.h:
// KH_W16_BF16 -> the _w16 kernels, KH_W16_F16 -> the _h16 kernels).  Host code only.  Each launch is the fp32 launch
// of kh_model_step.hip with the same shape (split, u, grid, wg - a shape forced through KH_SHAPE_* included) on the
// twin of its kernel, so the bits do not change.  A translation unit instantiates ONE format
// (kh_model_w16.hip bf16, kh_model_h16.hip fp16): the kernels of the other are named here and compiled there.
// Replaces nothing in the reference (it streams fp32 weights: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
#pragma once
#include "kh_dispatch.h"
#include "kh_w16.h"
#include "kh_model_internal.h"

namespace khm {

// go(KH_KERNEL(<stem>_w16 or <stem>_h16, ...)) by the format: one spelling of the stem and of the template arguments
#define KH_W16_TWIN(FMT, go, K, ...)          \
  do {                                        \
    if constexpr (FMT == KH_W16_F16)          \
      go(KH_KERNEL(K##_h16, __VA_ARGS__));    \
    else                                      \
      go(KH_KERNEL(K##_w16, __VA_ARGS__));    \
  } while (0)

// f(U, MV, SP) from the fp32 lists of a kernel (pick_fused without its QUANT level: a W16 kernel has no int8 form, and
// walking both levels would compile it for the int8 values of U as well)
template <class US, class MVS, class SPS, class F>
static void pick_w16(int u, int mv, int sp, F&& f) {
  kh_pick_ge(US{}, u, [&](auto U) {
    kh_pick(MVS{}, mv, [&](auto MV) { kh_pick(SPS{}, sp, [&](auto SP) { f(U, MV, SP); }); });
  });
}
// the logged launch of one twin on a decode shape
template <class A>
struct W16Go {
  const kh_model::Shape& sh;
  size_t lds;
  hipStream_t stream;
  const A& a;
  template <class K>
  void operator()(K kernel, const char* stem, std::initializer_list<KhTArg> targs) const {
    kh_launch(kernel, stem, targs, sh.grid, sh.wg, lds, stream, a);
  }
};

// >64 KiB dynamic-LDS opt-in of the gemv_res twin as w2 (configure_step_kernels does it for k_gemv_res)
template <int FMT>
static void w16_configure_fmt(const kh_model* m) {
  const size_t lds_need = fused_lds_bytes(false, m->cfg.hidden_dim);
  if (lds_need <= 64 * 1024) return;
  auto opt_in = [&](auto kernel, const char*, std::initializer_list<KhTArg>) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_need);
  };
  GemvResU<false>::each([&](auto U) {
    GemvResSP::each([&](auto SP) {
      KhVals<0, 6>::each([&](auto MV) { KH_W16_TWIN(FMT, opt_in, k_gemv_res, U, MV, SP); });
    });
  });
}

template <int FMT>
static void w16_qkv_fmt(kh_model* m, int l, const KhQkvArgs& fp32) {
  const kh_config& c = m->cfg;
  KhQkvArgs a = fp32;
  const kh_model::W16::Layer& W = m->w16.layers[(size_t)l];
  a.wq.w = W.wq;
  a.wk.w = W.wk;
  a.wv.w = W.wv;
  const W16Go<KhQkvArgs> go{m->sh_qkv, fused_lds_bytes(false, c.dim), m->stream, a};
  pick_w16<FusedU<false>, FusedMV, QkvSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), go.sh.split,
                                          [&](auto U, auto MV, auto SP) { KH_W16_TWIN(FMT, go, k_qkv, U, MV, SP); });
}
template <int FMT>
static void w16_wo_fmt(kh_model* m, int l, const KhGemvResArgs& fp32) {
  const kh_config& c = m->cfg;
  KhGemvResArgs a = fp32;
  a.w.w = m->w16.layers[(size_t)l].wo;
  const W16Go<KhGemvResArgs> go{m->sh_wo, fused_lds_bytes(false, c.dim), m->stream, a};
  pick_w16<FusedU<false>, FusedMV, GemvResSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), go.sh.split,
                                              [&](auto U, auto MV, auto SP) { KH_W16_TWIN(FMT, go, k_gemv_res, U, MV, SP); });
}
template <int FMT>
static void w16_wo_comb_fmt(kh_model* m, int l, const KhWoCombArgs& fp32) {
  const kh_config& c = m->cfg;
  KhWoCombArgs a = fp32;
  a.g.w.w = m->w16.layers[(size_t)l].wo;
  const W16Go<KhWoCombArgs> go{m->sh_wo, comb_lds_bytes(false, c.dim, c.head_num), m->stream, a};
  pick_w16<FusedU<false>, WoCombMV, GemvResSP>(go.sh.u, c.dim <= 2 * 4 * go.sh.wg ? 2 : 4, go.sh.split,
                                               [&](auto U, auto MV, auto SP) { KH_W16_TWIN(FMT, go, k_wo_comb, U, MV, SP); });
}
template <int FMT>
static void w16_ffn13_fmt(kh_model* m, int l, const KhFfn13Args& fp32) {
  const kh_config& c = m->cfg;
  KhFfn13Args a = fp32;
  a.w1.w = m->w16.layers[(size_t)l].w1;
  a.w3.w = m->w16.layers[(size_t)l].w3;
  const W16Go<KhFfn13Args> go{m->sh_ffn, fused_lds_bytes(false, c.dim), m->stream, a};
  pick_w16<FusedU<false>, FusedMV, NoSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), 1,
                                         [&](auto U, auto MV, auto) { KH_W16_TWIN(FMT, go, k_ffn13, U, MV); });
}
template <int FMT>
static void w16_w2_fmt(kh_model* m, int l, const KhGemvResArgs& fp32) {
  const kh_config& c = m->cfg;
  KhGemvResArgs a = fp32;
  a.w.w = m->w16.layers[(size_t)l].w2;
  const W16Go<KhGemvResArgs> go{m->sh_w2, fused_lds_bytes(false, c.hidden_dim), m->stream, a};
  pick_w16<GemvResU<false>, GemvResMV, GemvResSP>(go.sh.u, kh_stage_maxv(c.hidden_dim, go.sh.wg), go.sh.split,
                                                  [&](auto U, auto MV, auto SP) { KH_W16_TWIN(FMT, go, k_gemv_res, U, MV, SP); });
}
template <int FMT>
static void w16_cls_fmt(kh_model* m, const KhClsArgs& fp32) {
  const kh_config& c = m->cfg;
  KhClsArgs a = fp32;
  a.wcls.w = m->w16.cls;
  const W16Go<KhClsArgs> go{m->sh_cls, cls_lds_bytes(false, c.dim), m->stream, a};
  pick_w16<FusedU<false>, FusedMV, NoSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), 1,
                                         [&](auto U, auto MV, auto) { KH_W16_TWIN(FMT, go, k_cls, U, MV); });
}

}  // namespace khm
