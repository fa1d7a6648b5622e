// kh_model_q4_pass.hip — the B-token pass launches of a Q4 model on its packed 4-bit copy (KH_FLAG_Q4, hook
// KH_Q4_PASS): the launch text of kh_pf_launch.h instantiated for KH_SRC_Q4, which compiles the five _q4
// pass kernels of kh_q4_pass.h here and nowhere else (a translation unit of its own: the parallel build is as long as
// its longest unit).  kh_model_prefill.hip fills the arguments as the int8 launch takes them and hands the launch over
// for the classes of the pass mask.
// Replaces nothing in the reference (it feeds the prompt one token per forward pass: demo/main.cpp:20-22).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include "kh_q4_pass.h"
#include "kh_pf_launch.h"

namespace khm {

void q4_pf_qkv(kh_model* m, int l, const KhPfQkvArgs& img, const KhSeqLanes* lanes, int B) {
  copy_pf_qkv<KH_SRC_Q4>(m, l, img, lanes, B);
}
void q4_pf_ffn13(kh_model* m, int l, const KhPfFfn13Args& img, int B) { copy_pf_ffn13<KH_SRC_Q4>(m, l, img, B); }
void q4_pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& img, int bs) {
  copy_pf_gemv_res<KH_SRC_Q4>(m, l, cls, sh, img, bs);
}
void q4_pf_cls(kh_model* m, const KhPfClsArgs& img, int B) { copy_pf_cls<KH_SRC_Q4>(m, img, B); }

}  // namespace khm
