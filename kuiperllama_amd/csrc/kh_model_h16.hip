// kh_model_h16.hip — the decode GEMV launches of a model whose 16-bit copy holds fp16 values (KH_FLAG_W16_F16, DESIGN
// 3.1c): the launch text of kh_copy_launch.h instantiated for KH_SRC_F16, which compiles the five _h16 kernels of
// kh_w16.h here and nowhere else (a translation unit of its own: the parallel build is as long as its longest unit).
// kh_model_w16.hip builds the copy and hands its launches over by the copy's format.
// Replaces nothing in the reference (it streams fp32 weights: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
// gfx950 only.  No CPU fallback: every path below launches HIP kernels.
#include "kh_copy_launch.h"

namespace khm {

KH_COPY_LAUNCHES(, KH_SRC_F16);

}  // namespace khm
