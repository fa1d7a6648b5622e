// kh_model_h16_pass.hip — the B-token pass launches of a model whose 16-bit copy holds fp16 values (KH_FLAG_W16_F16,
// DESIGN 3.1c): the launch text of kh_pf_launch.h instantiated for KH_SRC_F16, which compiles the five _h16 pass
// kernels of kh_w16_pass.h here and nowhere else (a translation unit of its own: the parallel build is as long as its
// longest unit).  kh_model_prefill.hip fills the arguments and hands the launch over by the copy's format.
// Replaces nothing in the reference (it feeds the prompt one token per forward pass: demo/main.cpp:20-22).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include "kh_pf_launch.h"

namespace khm {

void h16_pf_qkv(kh_model* m, int l, const KhPfQkvArgs& img, const KhSeqLanes* lanes, int B) {
  copy_pf_qkv<KH_SRC_F16>(m, l, img, lanes, B);
}
void h16_pf_ffn13(kh_model* m, int l, const KhPfFfn13Args& img, int B) { copy_pf_ffn13<KH_SRC_F16>(m, l, img, B); }
void h16_pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& img, int bs) {
  copy_pf_gemv_res<KH_SRC_F16>(m, l, cls, sh, img, bs);
}
void h16_pf_cls(kh_model* m, const KhPfClsArgs& img, int B) { copy_pf_cls<KH_SRC_F16>(m, img, B); }

}  // namespace khm
