// kh_model_score_gemm_w16.hip — the scoring classifier on the bf16 matrix cores (kh_score_gemm_w16.h):
// this translation unit compiles the two k_pg_cls_lse_w16 instantiations and holds their launch, which
// kh_model_score_gemm.hip::launch_cls_lse takes where the classifier is the bf16-format 16-bit copy.  A unit of its own
// so that the kernels compile beside k_pg_cls_lse's and the GEMM16 family's, with the epilogue text
// (kh_score_gemm_epilogue.h) under the flags of kh_model_score_gemm.hip (build.py).
// The reference has no scoring call.  gfx950 only.  No CPU fallback.
#include "kh_dispatch.h"
#include "kh_score_gemm_w16.h"

namespace khm {
// a.w.w: bf16 bits, row-major [vocab][K], K % 32 == 0; NT = cl_nt(a.T), grid = cl_blocks(a.vocab) * a.slices
void launch_cls_lse_w16(hipStream_t stream, dim3 grid, int NT, const KhClsLseArgs& a) {
  kh_pick(KhVals<8, 4>{}, NT, [&](auto N) { kh_launch(KH_KERNEL(k_pg_cls_lse_w16, N), grid, KH_CL_WAVES * 64, 0, stream, a); });
}
}  // namespace khm
