// kh_model_gemm_w16.hip — the GEMM pass on the bf16 matrix cores (KH_FLAG_GEMM16; kh_gemm_w16.h): this
// translation unit compiles the k_pg_gemm_w16 / k_rg_gemm_w16 / k_sg_gemm_w16 instantiations, launches the one
// kh_model_gemm.hip::pg_gemm planned (the same tiles, grid, workgroup and LDS as the fp32 stem it replaces), and holds the
// operator-level entry kh_gemm_w16_f32.  A unit of its own so that its 28 kernels compile beside the fp32 / int8 ones.
// Replaces nothing in the reference (it multiplies fp32 by fp32: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
// gfx950 only.  No CPU fallback.
#include "kh_dispatch.h"
#include "kh_gemm_w16.h"
#include "kh_model_internal.h"

namespace khm {
namespace {
// the register tiles of kh_model_gemm.hip::kPgTiles, in its order; the wide pass has no (2,8)
constexpr int kTiles[4][2] = {{2, 8}, {2, 4}, {2, 2}, {1, 4}};
}  // namespace

bool pg_gemm_w16_launch(const PgW16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
                        const KhWideLanes* lanes) {
  int tile = 3;
  for (int i = 0; i < 4; ++i)
    if (kTiles[i][0] == L.R && kTiles[i][1] == L.NT) tile = i;
  auto opt_in = [&](auto kern, dim3&) { return pg_lds_opt_in((const void*)kern, L.lds); };
  bool launched = false;
  kh_pick(KhVals<KH_PG_QKV, KH_PG_RESID, KH_PG_SWIGLU, KH_PG_STORE>{}, L.epi, [&](auto E) {
    kh_pick(KhVals<0, 1, 2, 3>{}, tile, [&](auto I) {
      constexpr int EPI = decltype(E)::value, R = kTiles[I][0], NT = kTiles[I][1];
      if (lanes) {
        if constexpr (NT <= 4)
          launched = kh_launch_prep(opt_in, KH_KERNEL(k_sg_gemm_w16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a, *lanes);
        return;
      }
      if constexpr (EPI == KH_PG_QKV) {
        if (tiles) {
          launched = kh_launch_prep(opt_in, KH_KERNEL(k_rg_gemm_w16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a, *tiles);
          return;
        }
      }
      if constexpr (EPI != KH_PG_STORE)
        launched = kh_launch_prep(opt_in, KH_KERNEL(k_pg_gemm_w16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a);
    });
  });
  return launched;
}
}  // namespace khm
using namespace khm;

// y[T][ldy] (first M columns of each row) = x[T][K] . w16[M][K]^T: the STORE epilogue on pg_kloop_w16 with a row-major B
// operand.  w16: bf16 bits, row-major.  M % 16 == 0, K % 32 == 0, 1 <= T <= KH_PG_TMAX, ldy >= M and a multiple of 4,
// pointers 16-byte aligned; else KH_ERR_UNSUPPORTED / KH_ERR_INVALID_ARG.  The token tiles of the kernel are whole: x is
// staged into a zero-padded copy, so the call allocates, synchronises the stream and frees.  The register tile
// follows M and T ((2,4) for more than 32 tokens, (2,2) below, (1,4) where 32 rows do not divide M), the K split the
// number of 32-column blocks (4 waves from 32 blocks, 2 from 8): together the shapes a test reaches by its sizes.
extern "C" int kh_gemm_w16_f32(const float* x, const uint16_t* w16, float* y, int32_t T, int32_t M, int32_t K,
                               int32_t ldy, void* stream) {
  if (!x || !w16 || !y || T <= 0 || M <= 0 || K <= 0 || ldy < M) return KH_ERR_INVALID_ARG;
  if (((uintptr_t)x | (uintptr_t)w16 | (uintptr_t)y) & 15 || ldy % 4) return KH_ERR_INVALID_ARG;
  if (M % 16 || K % 32 || T > KH_PG_TMAX) return KH_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int R = M % 32 == 0 ? 2 : 1, NT = R == 2 ? (T > 32 ? 4 : 2) : 4;
  const int slices = ((T + 15) / 16 + NT - 1) / NT, rows = slices * NT * 16, nb = K / 32;
  const int ks = nb >= 32 ? 4 : (nb >= 8 ? 2 : 1);
  KhDev<float> xs;  // [rows][K], the padding rows zero
  int rc;
  if ((rc = xs.alloc((size_t)rows * K)) != KH_OK) return rc;
  KH_CHECK_HIP(hipMemsetAsync(xs, 0, (size_t)rows * K * sizeof(float), s));
  KH_CHECK_HIP(hipMemcpyAsync(xs, x, (size_t)T * K * sizeof(float), hipMemcpyDeviceToDevice, s));
  KhPgGemmArgs a{};
  a.w[0].w = w16;
  a.B = xs; a.b_tiled = 0; a.tcap = rows; a.out = y;
  a.rows0 = M; a.ldo = ldy; a.K = K; a.T = T;
  const KhWideLanes none{};  // (the STORE epilogue reads no lane)
  const bool ok = pg_gemm_w16_launch(PgW16Launch{KH_PG_STORE, R, NT, dim3(M / (16 * R), slices, 1), ks * 64,
                                                 pg_lds_bytes(ks, NT)},
                                     s, a, nullptr, &none);
  rc = ok ? kh_launch_status() : KH_ERR_UNSUPPORTED;
  const hipError_t e = hipStreamSynchronize(s);  // xs is freed on return
  return rc != KH_OK ? rc : (int)e;
}
