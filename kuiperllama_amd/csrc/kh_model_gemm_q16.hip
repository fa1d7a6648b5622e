// kh_model_gemm_q16.hip — the GEMM pass of an int8 group-64 model on the bf16 matrix cores from the int8 image itself
// (KH_FLAG_GEMM16_Q8; kh_gemm_q16.h): this translation unit compiles the k_pg_gemm_q16 / k_rg_gemm_q16 /
// k_sg_gemm_q16 instantiations, launches the one kh_model_gemm.hip::pg_gemm planned (the grid, workgroup and LDS of the
// int8 stem it replaces), configures the flag at creation and holds the operator-level entry kh_gemm_q8_bf16_f32.  A
// unit of its own so that its 24 kernels compile beside the fp32 / int8 / W16 ones.
// Replaces nothing in the reference (it dequantises per element on CUDA cores: kuiper/source/op/kernels/cuda/matmul_kernel.cu:50-96).
// gfx950 only.  No CPU fallback.
#include <stdlib.h>
#include <string.h>

#include "kh_dispatch.h"
#include "kh_gemm_q16.h"
#include "kh_model_internal.h"

namespace khm {
namespace {
// the register tiles of kh_model_gemm.hip::kPgTiles without (2,8) (kh_gemm_q16.h: it does not fit 256 registers)
constexpr int kTiles[3][2] = {{2, 4}, {2, 2}, {1, 4}};
}  // namespace

bool pg_gemm_q16_launch(const PgW16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
                        const KhWideLanes* lanes) {
  int tile = -1;
  for (int i = 0; i < 3; ++i)
    if (kTiles[i][0] == L.R && kTiles[i][1] == L.NT) tile = i;
  if (tile < 0) return false;  // (pg_gemm plans among the three)
  auto opt_in = [&](auto kern, dim3&) { return pg_lds_opt_in((const void*)kern, L.lds); };
  bool launched = false;
  kh_pick(KhVals<KH_PG_QKV, KH_PG_RESID, KH_PG_SWIGLU, KH_PG_STORE>{}, L.epi, [&](auto E) {
    kh_pick(KhVals<0, 1, 2>{}, tile, [&](auto I) {
      constexpr int EPI = decltype(E)::value, R = kTiles[I][0], NT = kTiles[I][1];
      if (lanes) {
        launched = kh_launch_prep(opt_in, KH_KERNEL(k_sg_gemm_q16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a, *lanes);
        return;
      }
      if constexpr (EPI == KH_PG_QKV) {
        if (tiles) {
          launched = kh_launch_prep(opt_in, KH_KERNEL(k_rg_gemm_q16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a, *tiles);
          return;
        }
      }
      if constexpr (EPI != KH_PG_STORE)
        launched = kh_launch_prep(opt_in, KH_KERNEL(k_pg_gemm_q16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a);
    });
  });
  return launched;
}

// Classes that run on the new stem unless KH_GEMM16_Q8_CLASSES says otherwise: 3.1f's adoption rule - a class is in only
// if its time with the flag on lies below its flag-off time by more than the run-to-run range on BOTH measured int8
// geometries (profiles/gemm16_q8_ab.txt).
enum { KH_GEMM16_Q8_DEFAULT = KH_W16_QKV | KH_W16_WO | KH_W16_FFN13 | KH_W16_W2 };
int plan_gemm16_q8(bool quant, int group_size, int dim, int hidden_dim, int kv_dim, int vocab_size) {
  if (!quant || group_size != 64 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0) return 0;
  if (dim % 64 || hidden_dim % 64 || kv_dim % 16) return 0;  // pg_supported's granules of an int8 model
  return KH_GEMM16_Q8_DEFAULT;
}
// Read at creation.  Hooks: KH_GEMM16_Q8=1 / 0 overrides the flag; KH_GEMM16_Q8_CLASSES=<number> (strtol, base 0)
// replaces the adoption mask.  Independent of KH_FLAG_Q4: the GEMM passes of a Q4 model read the int8 image.
void gemm16_q8_configure(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::Gemm16Q8& g = m->g16q8;
  g = kh_model::Gemm16Q8();
  const char* hook = dbg("KH_GEMM16_Q8");
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_GEMM16_Q8) != 0;
  if (!want) { g.reason = KH_GEMM16_Q8_NO_FLAG; return; }
  if (!c.is_quant) { g.reason = KH_GEMM16_Q8_FP32; return; }
  if (c.group_size != 64) { g.reason = KH_GEMM16_Q8_GROUP; return; }
  if (!pg_supported(m)) { g.reason = KH_GEMM16_Q8_GEOMETRY; return; }
  g.plan = plan_gemm16_q8(true, c.group_size, c.dim, c.hidden_dim, c.kv_dim, c.vocab_size);
  int mask = g.plan;
  if (const char* cl = dbg("KH_GEMM16_Q8_CLASSES")) mask = (int)strtol(cl, nullptr, 0) & KH_W16_ALL;
  g.classes = mask;
  g.reason = g.classes ? KH_GEMM16_Q8_ON : KH_GEMM16_Q8_NO_CLASS;
}
}  // namespace khm
using namespace khm;

// out2 = {KH_W16_* bits of the launch classes whose GEMM-pass GEMMs run on the bf16 matrix cores under
// KH_FLAG_GEMM16_Q8 by default (0: not applicable), the columns of a K block}
extern "C" int kh_plan_gemm16_q8(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t is_quant,
                                 int32_t group_size, int64_t* out2) {
  if (!out2 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0 || group_size < 0) return KH_ERR_INVALID_ARG;
  out2[0] = plan_gemm16_q8(is_quant != 0, group_size, dim, hidden_dim, kv_dim, vocab_size);
  out2[1] = 64;
  return KH_OK;
}

extern "C" int kh_model_gemm16_q8_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  memset(out, 0, 8 * sizeof(int64_t));
  out[0] = m->g16q8.classes != 0;
  out[1] = m->g16q8.classes;
  out[2] = m->g16q8.reason;
  out[3] = m->g16q8.plan;
  return KH_OK;
}

// y[T][ldy] (first M columns of each row) = x[T][K] . (scales * w8)[M][K]^T: the STORE epilogue on pg_kloop_q16 with a
// row-major B operand.  w8: int8, row-major; scales[M][K / 64].  M % 16 == 0, K % 64 == 0, 1 <= T <= KH_PG_TMAX, ldy >= M
// and a multiple of 4, pointers 16-byte aligned; else KH_ERR_UNSUPPORTED / KH_ERR_INVALID_ARG.  The token tiles of the
// kernel are whole: x is staged into a zero-padded copy, so the call allocates, synchronises the stream and frees.  The
// register tile follows M and T ((2,4) for more than 32 tokens, (2,2) below, (1,4) where 32 rows do not divide M), the
// K split the number of 64-column blocks (4 waves from 32 blocks, 2 from 8): together the shapes a test reaches by its
// sizes.
extern "C" int kh_gemm_q8_bf16_f32(const float* x, const int8_t* w8, const float* scales, float* y, int32_t T, int32_t M,
                                   int32_t K, int32_t ldy, void* stream) {
  if (!x || !w8 || !scales || !y || T <= 0 || M <= 0 || K <= 0 || ldy < M) return KH_ERR_INVALID_ARG;
  if (((uintptr_t)x | (uintptr_t)w8 | (uintptr_t)y) & 15 || (uintptr_t)scales & 3 || ldy % 4) return KH_ERR_INVALID_ARG;
  if (M % 16 || K % 64 || T > KH_PG_TMAX) return KH_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int R = M % 32 == 0 ? 2 : 1, NT = R == 2 ? (T > 32 ? 4 : 2) : 4;
  const int slices = ((T + 15) / 16 + NT - 1) / NT, rows = slices * NT * 16, nb = K / 64;
  const int ks = nb >= 32 ? 4 : (nb >= 8 ? 2 : 1);
  KhDev<float> xs;  // [rows][K], the padding rows zero
  int rc;
  if ((rc = xs.alloc((size_t)rows * K)) != KH_OK) return rc;
  KH_CHECK_HIP(hipMemsetAsync(xs, 0, (size_t)rows * K * sizeof(float), s));
  KH_CHECK_HIP(hipMemcpyAsync(xs, x, (size_t)T * K * sizeof(float), hipMemcpyDeviceToDevice, s));
  KhPgGemmArgs a{};
  a.w[0].w = w8;
  a.w[0].scales = scales;
  a.B = xs; a.b_tiled = 0; a.tcap = rows; a.out = y;
  a.rows0 = M; a.ldo = ldy; a.K = K; a.T = T; a.gshift = 6;
  const KhWideLanes none{};  // (the STORE epilogue reads no lane)
  const bool ok = pg_gemm_q16_launch(PgW16Launch{KH_PG_STORE, R, NT, dim3(M / (16 * R), slices, 1), ks * 64,
                                                 pg_lds_bytes(ks, NT)},
                                     s, a, nullptr, &none);
  rc = ok ? kh_launch_status() : KH_ERR_UNSUPPORTED;
  const hipError_t e = hipStreamSynchronize(s);  // xs is freed on return
  return rc != KH_OK ? rc : (int)e;
}
