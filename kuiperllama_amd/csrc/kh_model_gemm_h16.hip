// kh_model_gemm_h16.hip — the GEMM pass of an fp16-origin fp32 model on the bf16 matrix cores from the fp16-format 16-bit
// copy (KH_FLAG_GEMM16_F16; kh_gemm_h16.h): this translation unit compiles the k_pg_gemm_h16 /
// k_rg_gemm_h16 / k_sg_gemm_h16 instantiations, launches the one kh_model_gemm.hip::pg_gemm planned (the grid, workgroup
// and LDS of the _w16 launch of the same shape), configures the flag at creation and holds the operator-level entry
// kh_gemm_h16_f32.  A unit of its own so that its 24 kernels compile beside the fp32 / int8 / W16 ones.
// Replaces nothing in the reference (it multiplies fp32 by fp32: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
// gfx950 only.  No CPU fallback.
#include <stdlib.h>
#include <string.h>

#include "kh_dispatch.h"
#include "kh_gemm_h16.h"
#include "kh_model_internal.h"
#include "kh_w16.h"  // KH_W16_F16: the copy's format

namespace khm {
namespace {
// the register tiles of kh_model_gemm.hip::kPgTiles without (2,8) (kh_gemm_h16.h: it does not fit 256 registers)
constexpr int kTiles[3][2] = {{2, 4}, {2, 2}, {1, 4}};
}  // namespace

bool pg_gemm_h16_launch(const PgW16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
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
        launched = kh_launch_prep(opt_in, KH_KERNEL(k_sg_gemm_h16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a, *lanes);
        return;
      }
      if constexpr (EPI == KH_PG_QKV) {
        if (tiles) {
          launched = kh_launch_prep(opt_in, KH_KERNEL(k_rg_gemm_h16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a, *tiles);
          return;
        }
      }
      if constexpr (EPI != KH_PG_STORE)
        launched = kh_launch_prep(opt_in, KH_KERNEL(k_pg_gemm_h16, R, NT, EPI), L.grid, L.wg, L.lds, stream, a);
    });
  });
  return launched;
}

// Classes that run on the new stem unless KH_GEMM16_F16_CLASSES says otherwise: 3.1c's adoption rule - a class is in only
// if its time with the flag on lies below its flag-off time by more than the flag-off range on BOTH the Llama-3.2-1B
// and the Llama-2-7B geometry at 512 tokens (profiles/gemm16_f16_ab.txt) - among the classes whose contraction length
// is a multiple of the 32-column block.  On the 1B geometry qkv, wo and w2 stay inside the range and ffn13 loses 18 %; cls
// gains 2.7 % of a 64-sequence batch there but the 7B geometry is not measured.  The rule keeps nothing:
// the flag acts only through the hook.
enum { KH_GEMM16_F16_DEFAULT = 0 };
static int gemm16_f16_k32_classes(int dim, int hidden_dim) {
  return (dim % 32 == 0 ? KH_W16_QKV | KH_W16_WO | KH_W16_FFN13 | KH_W16_CLS : 0) | (hidden_dim % 32 == 0 ? KH_W16_W2 : 0);
}
int plan_gemm16_f16(bool quant, int dim, int hidden_dim, int kv_dim, int vocab_size) {
  if (quant || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0) return 0;
  if (dim % 16 || hidden_dim % 16 || kv_dim % 16) return 0;  // pg_supported's granules of an fp32 model
  return KH_GEMM16_F16_DEFAULT & gemm16_f16_k32_classes(dim, hidden_dim);
}
// Read at creation, behind the copy's build (w16_create).  Hooks: KH_GEMM16_F16=1 / 0 overrides the flag;
// KH_GEMM16_F16_CLASSES=<number> (strtol, base 0) replaces the adoption mask - the K % 32 rule still holds.
void gemm16_f16_configure(kh_model* m) {
  const kh_config& c = m->cfg;
  const kh_model::W16& w = m->w16;
  kh_model::Gemm16F16& g = m->g16f16;
  g = kh_model::Gemm16F16();
  const char* hook = dbg("KH_GEMM16_F16");
  const bool want = hook ? hook[0] == '1' : (m->opts.flags & KH_FLAG_GEMM16_F16) != 0;
  if (!want) { g.reason = KH_GEMM16_F16_NO_FLAG; return; }
  if (c.is_quant) { g.reason = KH_GEMM16_F16_QUANT; return; }
  const char* hook_f16 = dbg("KH_W16_F16");  // (as w16_create reads it)
  if (!(hook_f16 ? hook_f16[0] == '1' : (m->opts.flags & KH_FLAG_W16_F16) != 0)) { g.reason = KH_GEMM16_F16_NO_W16_F16; return; }
  if (w.state != 1) { g.reason = w.state == -1 ? KH_GEMM16_F16_INEXACT : KH_GEMM16_F16_GEOMETRY; return; }
  if (w.format != KH_W16_F16) { g.reason = KH_GEMM16_F16_BF16_COPY; return; }
  if (!pg_supported(m)) { g.reason = KH_GEMM16_F16_GEOMETRY; return; }
  g.plan = plan_gemm16_f16(false, c.dim, c.hidden_dim, c.kv_dim, c.vocab_size);
  int mask = g.plan;
  if (const char* cl = dbg("KH_GEMM16_F16_CLASSES"))
    mask = (int)strtol(cl, nullptr, 0) & gemm16_f16_k32_classes(c.dim, c.hidden_dim);
  g.classes = mask & w.classes;
  g.reason = g.classes ? KH_GEMM16_F16_ON : KH_GEMM16_F16_NO_CLASS;
}
}  // namespace khm
using namespace khm;

// out2 = {KH_W16_* bits of the launch classes whose GEMM-pass GEMMs run on the bf16 matrix cores under
// KH_FLAG_GEMM16_F16 by default (0: not applicable, or the adoption rule keeps none), the columns of a K block}
extern "C" int kh_plan_gemm16_f16(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t is_quant,
                                  int64_t* out2) {
  if (!out2 || dim <= 0 || hidden_dim <= 0 || kv_dim <= 0 || vocab_size <= 0) return KH_ERR_INVALID_ARG;
  out2[0] = plan_gemm16_f16(is_quant != 0, dim, hidden_dim, kv_dim, vocab_size);
  out2[1] = 32;
  return KH_OK;
}

extern "C" int kh_model_gemm16_f16_info(kh_model* m, int64_t* out) {
  if (!m || !out) return KH_ERR_INVALID_ARG;
  memset(out, 0, 8 * sizeof(int64_t));
  const bool live = m->w16.state == 1 && m->w16.format == KH_W16_F16;  // (a copy given up by its self-check: state -2)
  const bool on = live && m->g16f16.classes != 0;
  out[0] = on;
  out[1] = on ? m->g16f16.classes : 0;
  out[2] = on ? KH_GEMM16_F16_ON : (m->g16f16.classes ? KH_GEMM16_F16_SELFCHECK : m->g16f16.reason);
  out[3] = m->g16f16.plan;
  return KH_OK;
}

// y[T][ldy] (first M columns of each row) = x[T][K] . w16[M][K]^T: the STORE epilogue on pg_kloop_h16 with a row-major B
// operand.  w16: fp16 bits, row-major.  M % 16 == 0, K % 32 == 0, 1 <= T <= KH_PG_TMAX, ldy >= M and a multiple of 4,
// pointers 16-byte aligned; else KH_ERR_UNSUPPORTED / KH_ERR_INVALID_ARG.  The token tiles of the kernel are whole: x is
// staged into a zero-padded copy, so the call allocates, synchronises the stream and frees.  The register tile
// follows M and T ((2,4) for more than 32 tokens, (2,2) below, (1,4) where 32 rows do not divide M), the K split the
// number of 32-column blocks (4 waves from 32 blocks, 2 from 8): together the shapes a test reaches by its sizes.
extern "C" int kh_gemm_h16_f32(const float* x, const uint16_t* w16, float* y, int32_t T, int32_t M, int32_t K,
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
  const bool ok = pg_gemm_h16_launch(PgW16Launch{KH_PG_STORE, R, NT, dim3(M / (16 * R), slices, 1), ks * 64,
                                                 pg_lds_bytes(ks, NT)},
                                     s, a, nullptr, &none);
  rc = ok ? kh_launch_status() : KH_ERR_UNSUPPORTED;
  const hipError_t e = hipStreamSynchronize(s);  // xs is freed on return
  return rc != KH_OK ? rc : (int)e;
}
