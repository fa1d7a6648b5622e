// kh_model_h16.hip — the decode GEMV launches of a model whose 16-bit copy holds fp16 values (KH_FLAG_W16_F16, DESIGN
// 3.1c): the launch text of kh_w16_launch.h instantiated for KH_W16_F16, which compiles the five _h16 kernels of
// kh_w16.h here and nowhere else (a translation unit of its own: the parallel build is as long as its longest unit).
// kh_model_w16.hip builds the copy and hands its launches over by the copy's format.
// Replaces nothing in the reference (it streams fp32 weights: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include "kh_w16_launch.h"

namespace khm {

void h16_configure(const kh_model* m) { w16_configure_fmt<KH_W16_F16>(m); }
void h16_launch_qkv(kh_model* m, int l, const KhQkvArgs& fp32) { w16_qkv_fmt<KH_W16_F16>(m, l, fp32); }
void h16_launch_wo(kh_model* m, int l, const KhGemvResArgs& fp32) { w16_wo_fmt<KH_W16_F16>(m, l, fp32); }
void h16_launch_wo_comb(kh_model* m, int l, const KhWoCombArgs& fp32) { w16_wo_comb_fmt<KH_W16_F16>(m, l, fp32); }
void h16_launch_ffn13(kh_model* m, int l, const KhFfn13Args& fp32) { w16_ffn13_fmt<KH_W16_F16>(m, l, fp32); }
void h16_launch_w2(kh_model* m, int l, const KhGemvResArgs& fp32) { w16_w2_fmt<KH_W16_F16>(m, l, fp32); }
void h16_launch_cls(kh_model* m, const KhClsArgs& fp32) { w16_cls_fmt<KH_W16_F16>(m, fp32); }

}  // namespace khm
