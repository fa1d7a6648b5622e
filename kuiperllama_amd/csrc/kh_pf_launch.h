// kh_pf_launch.h — how a B-token kernel (kh_prefill.h, kh_seq.h, kh_w16_pass.h) is launched: the grid clipped to one
// resident round, the instantiation lists, and the launches of the twins on the 16-bit copy, written once for both
// formats of the copy (kh_w16.h: KH_W16_BF16 -> the _w16 kernels, compiled by kh_model_prefill.hip; KH_W16_F16 -> the
// _h16 kernels, compiled by kh_model_h16_pass.hip).  Host code only.
// Replaces nothing in the reference (it feeds the prompt one token per forward pass: demo/main.cpp:20-22).
#pragma once
#include <vector>

#include "kh_dispatch.h"
#include "kh_model_internal.h"
#include "kh_copy_launch.h"
#include "kh_w16_pass.h"

namespace khm {

// The B-token kernels are register- and LDS-heavy: a grid larger than what is resident at once
// runs in rounds and every round re-stages the B activation vectors, so the decode shape's grid
// is clipped to one resident round (the result does not depend on the grid).
template <class K>
void pf_clip_grid(K kernel, dim3& grid, int wg, size_t lds) {
  // resident-workgroup count and the >64 KiB LDS opt-in are per (device, kernel, shape): a thread
  // that drives models on several GPUs must not reuse device A's answer (or skip the attribute)
  // on device B
  struct Cached {
    int dev;
    const void* fn;
    int wg;
    size_t lds;
    int resident;
  };
  static thread_local std::vector<Cached> cache;
  int dev = 0;
  (void)hipGetDevice(&dev);
  int resident = 0;
  for (const auto& c : cache)
    if (c.dev == dev && c.fn == (const void*)kernel && c.wg == wg && c.lds == lds) resident = c.resident;
  if (!resident) {
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
    int per_cu = 0, cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, wg, lds) != hipSuccess ||
        per_cu < 1)
      per_cu = 1;
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
      cus = v;
    resident = per_cu * cus;
    cache.push_back({dev, (const void*)kernel, wg, lds, resident});
  }
  if ((int)grid.x > resident) grid.x = resident;
}
// pf_launch(KH_KERNEL(k_pf_qkv, Q, SP, B), ...): the logged launch of kh_dispatch.h on the clipped grid
template <class K, class A>
void pf_launch(K kernel, const char* stem, std::initializer_list<KhTArg> targs, const kh_model::Shape& sh, size_t lds,
               hipStream_t s, const A& args) {
  (void)kh_launch_prep([&](K k, dim3& grid) { return pf_clip_grid(k, grid, sh.wg, lds), true; }, kernel, stem, targs,
                       sh.grid, sh.wg, lds, s, args);
}
// The instantiations of the B-token kernels: SP = the decode shape's split (prefill_supported: qkv's at most 2), B =
// tokens per pass - 8, 4 or 2 by construction (prefill_batch, pf_gemv_res), int8 at most 4.
template <bool Q>
using PfB = std::conditional_t<Q, KhVals<4>, KhVals<8, 4>>;  // k_pf_qkv, k_pf_ffn13
template <bool Q>
using PfGemvResB = std::conditional_t<Q, KhVals<4, 2>, KhVals<8, 4, 2>>;
using PfQkvSP = KhVals<2, 1>;
using PfGemvResSP = KhVals<4, 2, 1>;
using PfNoSP = KhVals<1>;  // k_pf_ffn13
// f(Q, SP, B) with the compile-time values of a launch
template <template <bool> class BS, class SPS, class F>
void pick_pf(bool quant, int sp, int b, F&& f) {
  kh_pick_bool(quant, [&](auto Q) {
    kh_pick(SPS{}, sp, [&](auto SP) { kh_pick_ge(BS<decltype(Q)::value>{}, b, [&](auto B) { f(Q, SP, B); }); });
  });
}
// ---- the twins on the 16-bit copy (kh_w16_pass.h): `fp32` as the fp32 launch fills it, the matrices of layer l
// replaced by their 16-bit copies, on the fp32 launch's shape, LDS bytes (the plain layout) and clipped grid - the fp32
// lists without their int8 level, as pick_copy of kh_copy_launch.h
template <class SPS, class BS, class F>
void pick_pf_w16(int sp, int b, F&& f) {
  kh_pick(SPS{}, sp, [&](auto SP) { kh_pick_ge(BS{}, b, [&](auto B) { f(SP, B); }); });
}
// the logged, clipped launch of one twin
template <class A>
struct PfW16Go {
  const kh_model::Shape& sh;
  size_t lds;
  hipStream_t stream;
  const A& a;
  template <class K>
  void operator()(K kernel, const char* stem, std::initializer_list<KhTArg> targs) const {
    pf_launch(kernel, stem, targs, sh, lds, stream, a);
  }
};
template <int FMT>
void w16_pf_qkv_fmt(kh_model* m, int l, const KhPfQkvArgs& fp32, const KhSeqLanes* lanes, int B) {
  KhPfQkvArgs a = fp32;
  const kh_model::W16::Layer& W = m->w16.layers[(size_t)l];
  a.wq.w = W.wq;
  a.wk.w = W.wk;
  a.wv.w = W.wv;
  pick_pf_w16<PfQkvSP, PfB<false>>(m->sh_qkv.split, B, [&](auto SP, auto BB) {
    const size_t lds = pf_lds_bytes(false, a.dim, BB);
    if (lanes) {
      const KhSeqQkvArgs sa{a, *lanes};
      const PfW16Go<KhSeqQkvArgs> go{m->sh_qkv, lds, m->stream, sa};
      KH_W16_TWIN(FMT, go, k_seq_qkv, SP, BB);
    } else {
      const PfW16Go<KhPfQkvArgs> go{m->sh_qkv, lds, m->stream, a};
      KH_W16_TWIN(FMT, go, k_pf_qkv, SP, BB);
    }
  });
}
template <int FMT>
void w16_pf_ffn13_fmt(kh_model* m, int l, const KhPfFfn13Args& fp32, int B) {
  KhPfFfn13Args a = fp32;
  a.w1.w = m->w16.layers[(size_t)l].w1;
  a.w3.w = m->w16.layers[(size_t)l].w3;
  pick_pf_w16<PfNoSP, PfB<false>>(1, B, [&](auto, auto BB) {
    const PfW16Go<KhPfFfn13Args> go{m->sh_ffn, pf_lds_bytes(false, a.dim, BB), m->stream, a};
    KH_W16_TWIN(FMT, go, k_pf_ffn13, BB);
  });
}
// cls: KH_W16_WO or KH_W16_W2; bs: the sub-batch pf_gemv_res chose
template <int FMT>
void w16_pf_gemv_res_fmt(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& fp32, int bs) {
  KhPfGemvResArgs a = fp32;
  a.w.w = cls == KH_W16_WO ? m->w16.layers[(size_t)l].wo : m->w16.layers[(size_t)l].w2;
  pick_pf_w16<PfGemvResSP, PfGemvResB<false>>(sh.split, bs, [&](auto SP, auto B) {
    const PfW16Go<KhPfGemvResArgs> go{sh, pf_lds_bytes(false, a.M, B), m->stream, a};
    KH_W16_TWIN(FMT, go, k_pf_gemv_res, SP, B);
  });
}
template <int FMT>
void w16_pf_cls_fmt(kh_model* m, const KhPfClsArgs& fp32, int B) {
  KhPfClsArgs a = fp32;
  a.wcls.w = m->w16.cls;
  pick_pf_w16<PfNoSP, PfB<false>>(1, B, [&](auto, auto BB) {
    const PfW16Go<KhPfClsArgs> go{m->sh_cls, pf_lds_bytes(false, a.dim, BB), m->stream, a};
    KH_W16_TWIN(FMT, go, k_pf_cls, BB);
  });
}
// kh_model_h16_pass.hip: the four above for KH_W16_F16
void h16_pf_qkv(kh_model* m, int l, const KhPfQkvArgs& fp32, const KhSeqLanes* lanes, int B);
void h16_pf_ffn13(kh_model* m, int l, const KhPfFfn13Args& fp32, int B);
void h16_pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& fp32, int bs);
void h16_pf_cls(kh_model* m, const KhPfClsArgs& fp32, int B);

}  // namespace khm
