// kh_pf_launch.h — how a B-token kernel (kh_prefill.h, kh_seq.h, kh_w16_pass.h, kh_q4_pass.h) is launched: the grid
// clipped to one resident round, the instantiation lists, and the launches of the twins on a narrow exact copy, written
// once over the source of kh_copy_launch.h (KH_SRC_BF16 -> the _w16 kernels, compiled by kh_model_prefill.hip;
// KH_SRC_F16 -> the _h16 kernels, compiled by kh_model_h16_pass.hip; KH_SRC_Q4 -> the _q4 kernels of kh_q4_pass.h,
// compiled by kh_model_q4_pass.hip).  Host code only.
// Replaces nothing in the reference (it feeds the prompt one token per forward pass: demo/main.cpp:20-22).
#pragma once
#include <vector>

#include "kh_dispatch.h"
#include "kh_model_internal.h"
#include "kh_copy_launch.h"
#include "kh_w16_pass.h"

// The _q4 pass kernels by name only (kh_q4_pass.h, which kh_model_q4_pass.hip includes: the unit that compiles them)
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_qkv_q4(const KhPfQkvArgs a);
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_seq_qkv_q4(const KhSeqQkvArgs a);
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_ffn13_q4(const KhPfFfn13Args a);
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_gemv_res_q4(const KhPfGemvResArgs a);
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_cls_q4(const KhPfClsArgs a);

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
// ---- the twins on a copy (kh_w16_pass.h, kh_q4_pass.h): `img` as the image's launch fills it, the matrices of layer l
// replaced by their copies (copy_of<SRC>: the 16-bit or the 4-bit arena), on the image's launch shape, LDS bytes (the
// layout of the image's kind: kh_src_quant<SRC>) and clipped grid - the lists at the ONE level of QUANT the source has,
// as pick_copy of kh_copy_launch.h
template <class SPS, class BS, class F>
void pick_pf_copy(int sp, int b, F&& f) {
  kh_pick(SPS{}, sp, [&](auto SP) { kh_pick_ge(BS{}, b, [&](auto B) { f(SP, B); }); });
}
// the logged, clipped launch of one twin
template <class A>
struct PfCopyGo {
  const kh_model::Shape& sh;
  size_t lds;
  hipStream_t stream;
  const A& a;
  template <class K>
  void operator()(K kernel, const char* stem, std::initializer_list<KhTArg> targs) const {
    pf_launch(kernel, stem, targs, sh, lds, stream, a);
  }
};
template <int SRC>
void copy_pf_qkv(kh_model* m, int l, const KhPfQkvArgs& img, const KhSeqLanes* lanes, int B) {
  constexpr bool Q = kh_src_quant<SRC>;
  KhPfQkvArgs a = img;
  const kh_model::WCopy::Layer& W = copy_of<SRC>(m).layers[(size_t)l];
  a.wq.w = W.wq;
  a.wk.w = W.wk;
  a.wv.w = W.wv;
  pick_pf_copy<PfQkvSP, PfB<Q>>(m->sh_qkv.split, B, [&](auto SP, auto BB) {
    const size_t lds = pf_lds_bytes(Q, a.dim, BB);
    if (lanes) {
      const KhSeqQkvArgs sa{a, *lanes};
      const PfCopyGo<KhSeqQkvArgs> go{m->sh_qkv, lds, m->stream, sa};
      KH_COPY_TWIN(SRC, go, k_seq_qkv, SP, BB);
    } else {
      const PfCopyGo<KhPfQkvArgs> go{m->sh_qkv, lds, m->stream, a};
      KH_COPY_TWIN(SRC, go, k_pf_qkv, SP, BB);
    }
  });
}
template <int SRC>
void copy_pf_ffn13(kh_model* m, int l, const KhPfFfn13Args& img, int B) {
  constexpr bool Q = kh_src_quant<SRC>;
  KhPfFfn13Args a = img;
  a.w1.w = copy_of<SRC>(m).layers[(size_t)l].w1;
  a.w3.w = copy_of<SRC>(m).layers[(size_t)l].w3;
  pick_pf_copy<PfNoSP, PfB<Q>>(1, B, [&](auto, auto BB) {
    const PfCopyGo<KhPfFfn13Args> go{m->sh_ffn, pf_lds_bytes(Q, a.dim, BB), m->stream, a};
    KH_COPY_TWIN(SRC, go, k_pf_ffn13, BB);
  });
}
// cls: KH_W16_WO or KH_W16_W2; bs: the sub-batch pf_gemv_res chose
template <int SRC>
void copy_pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& img, int bs) {
  constexpr bool Q = kh_src_quant<SRC>;
  KhPfGemvResArgs a = img;
  const kh_model::WCopy::Layer& W = copy_of<SRC>(m).layers[(size_t)l];
  a.w.w = cls == KH_W16_WO ? W.wo : W.w2;
  pick_pf_copy<PfGemvResSP, PfGemvResB<Q>>(sh.split, bs, [&](auto SP, auto B) {
    const PfCopyGo<KhPfGemvResArgs> go{sh, pf_lds_bytes(Q, a.M, B), m->stream, a};
    KH_COPY_TWIN(SRC, go, k_pf_gemv_res, SP, B);
  });
}
template <int SRC>
void copy_pf_cls(kh_model* m, const KhPfClsArgs& img, int B) {
  constexpr bool Q = kh_src_quant<SRC>;
  KhPfClsArgs a = img;
  a.wcls.w = copy_of<SRC>(m).cls;
  pick_pf_copy<PfNoSP, PfB<Q>>(1, B, [&](auto, auto BB) {
    const PfCopyGo<KhPfClsArgs> go{m->sh_cls, pf_lds_bytes(Q, a.dim, BB), m->stream, a};
    KH_COPY_TWIN(SRC, go, k_pf_cls, BB);
  });
}
// kh_model_h16_pass.hip: the four above for KH_SRC_F16 ...
void h16_pf_qkv(kh_model* m, int l, const KhPfQkvArgs& img, const KhSeqLanes* lanes, int B);
void h16_pf_ffn13(kh_model* m, int l, const KhPfFfn13Args& img, int B);
void h16_pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& img, int bs);
void h16_pf_cls(kh_model* m, const KhPfClsArgs& img, int B);
// ... and kh_model_q4_pass.hip: for KH_SRC_Q4
void q4_pf_qkv(kh_model* m, int l, const KhPfQkvArgs& img, const KhSeqLanes* lanes, int B);
void q4_pf_ffn13(kh_model* m, int l, const KhPfFfn13Args& img, int B);
void q4_pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& img, int bs);
void q4_pf_cls(kh_model* m, const KhPfClsArgs& img, int B);

}  // namespace khm
