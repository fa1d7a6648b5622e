// kh_model_gemm_w16.hip — the GEMM pass on the bf16 matrix cores (KH_FLAG_GEMM16; kh_gemm_w16.h): this
// translation unit compiles the k_pg_gemm_w16 / k_rg_gemm_w16 / k_sg_gemm_w16 instantiations behind the family's launch
// text (kh_gemm16_launch.h: the one kh_model_gemm.hip::pg_gemm planned, with the tiles, grid, workgroup and LDS of the
// fp32 stem it replaces), and holds the operator-level entry kh_gemm_w16_f32.  A unit of its own so that its 28 kernels
// compile beside the fp32 / int8 ones.
// Replaces nothing in the reference (it multiplies fp32 by fp32: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
// gfx950 only.  No CPU fallback.
#include "kh_gemm_w16.h"
#include "kh_gemm16_launch.h"

namespace khm {
KH_GEMM16_LAUNCH(PG_W16, w16)
}  // namespace khm
using namespace khm;

// y[T][ldy] (first M columns of each row) = x[T][K] . w16[M][K]^T: gemm16_op on pg_kloop_w16.  w16: bf16 bits, row-major.
// M % 16 == 0, K % 32 == 0, 1 <= T <= KH_PG_TMAX, ldy >= M and a multiple of 4, pointers 16-byte aligned; else
// KH_ERR_UNSUPPORTED / KH_ERR_INVALID_ARG.
extern "C" int kh_gemm_w16_f32(const float* x, const uint16_t* w16, float* y, int32_t T, int32_t M, int32_t K,
                               int32_t ldy, void* stream) {
  if (!x || !w16 || !y || T <= 0 || M <= 0 || K <= 0 || ldy < M) return KH_ERR_INVALID_ARG;
  if (((uintptr_t)x | (uintptr_t)w16 | (uintptr_t)y) & 15 || ldy % 4) return KH_ERR_INVALID_ARG;
  if (M % 16 || K % 32 || T > KH_PG_TMAX) return KH_ERR_UNSUPPORTED;
  return gemm16_op(pg_gemm_w16_launch, 32, x, w16, nullptr, 0, y, T, M, K, ldy, (hipStream_t)stream);
}
