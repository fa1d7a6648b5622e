// kh_model_gemm_q16.hip — the GEMM pass of an int8 group-64 model on the bf16 matrix cores from the int8 image itself
// (KH_FLAG_GEMM16_Q8; kh_gemm_q16.h): this translation unit compiles the k_pg_gemm_q16 / k_rg_gemm_q16 /
// k_sg_gemm_q16 instantiations behind the family's launch text (kh_gemm16_launch.h: the grid, workgroup and LDS of the
// int8 stem it replaces), configures the flag at creation and holds the operator-level entry kh_gemm_q8_bf16_f32.  A
// unit of its own so that its 24 kernels compile beside the fp32 / int8 / W16 ones.
// Replaces nothing in the reference (it dequantises per element on CUDA cores: kuiper/source/op/kernels/cuda/matmul_kernel.cu:50-96).
// gfx950 only.  No CPU fallback.
#include <string.h>

#include "kh_gemm_q16.h"
#include "kh_gemm16_launch.h"

namespace khm {
KH_GEMM16_LAUNCH(PG_Q16, q16)

// Classes that run on the new stem unless KH_GEMM16_Q8_CLASSES says otherwise: 3.1f's adoption rule - a class is in only
// if its time with the flag on lies below its flag-off time by more than the run-to-run range on BOTH measured int8
// geometries (profiles/gemm16_q8_ab.txt).
enum { KH_GEMM16_Q8_DEFAULT = KH_W16_QKV | KH_W16_WO | KH_W16_FFN13 | KH_W16_W2 };
int plan_gemm16_q8(bool quant, int group_size, int dim, int hidden_dim, int kv_dim, int vocab_size) {
  if (!quant || group_size != 64 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0) return 0;
  if (dim % 64 || hidden_dim % 64 || kv_dim % 16) return 0;  // pg_supported's granules of an int8 model
  return KH_GEMM16_Q8_DEFAULT;
}
// Read at creation.  Hooks: KH_GEMM16_Q8=1 / 0 overrides the flag; KH_GEMM16_Q8_CLASSES replaces the adoption mask
// (gemm16_hook_mask).  Independent of KH_FLAG_Q4: the GEMM passes of a Q4 model read the int8 image.
void gemm16_q8_configure(kh_model* m) {
  const kh_config& c = m->cfg;
  kh_model::Gemm16& g = m->g16q8;
  g = kh_model::Gemm16();
  const char* hook = dbg("KH_GEMM16_Q8");
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_GEMM16_Q8) != 0;
  if (!want) { g.reason = KH_GEMM16_Q8_NO_FLAG; return; }
  if (!c.is_quant) { g.reason = KH_GEMM16_Q8_FP32; return; }
  if (c.group_size != 64) { g.reason = KH_GEMM16_Q8_GROUP; return; }
  if (!pg_supported(m)) { g.reason = KH_GEMM16_Q8_GEOMETRY; return; }
  g.plan = plan_gemm16_q8(true, c.group_size, c.dim, c.hidden_dim, c.kv_dim, c.vocab_size);
  g.classes = gemm16_hook_mask(dbg("KH_GEMM16_Q8_CLASSES"), g.plan, KH_W16_ALL);
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

// y[T][ldy] (first M columns of each row) = x[T][K] . (scales * w8)[M][K]^T: gemm16_op on pg_kloop_q16.  w8: int8,
// row-major; scales[M][K / 64].  M % 16 == 0, K % 64 == 0, 1 <= T <= KH_PG_TMAX, ldy >= M and a multiple of 4, pointers
// 16-byte aligned (scales: 4); else KH_ERR_UNSUPPORTED / KH_ERR_INVALID_ARG.
extern "C" int kh_gemm_q8_bf16_f32(const float* x, const int8_t* w8, const float* scales, float* y, int32_t T, int32_t M,
                                   int32_t K, int32_t ldy, void* stream) {
  if (!x || !w8 || !scales || !y || T <= 0 || M <= 0 || K <= 0 || ldy < M) return KH_ERR_INVALID_ARG;
  if (((uintptr_t)x | (uintptr_t)w8 | (uintptr_t)y) & 15 || (uintptr_t)scales & 3 || ldy % 4) return KH_ERR_INVALID_ARG;
  if (M % 16 || K % 64 || T > KH_PG_TMAX) return KH_ERR_UNSUPPORTED;
  return gemm16_op(pg_gemm_q16_launch, 64, x, w8, scales, 6, y, T, M, K, ldy, (hipStream_t)stream);
}
