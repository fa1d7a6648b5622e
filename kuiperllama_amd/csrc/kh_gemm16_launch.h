// kh_gemm16_launch.h — one GEMM of a GEMM pass on the bf16 matrix cores, written once for the three cores that run there:
// PG_W16 (the 16-bit copy in bf16 format -> the _w16 stems of kh_gemm_w16.h), PG_H16 (the copy in fp16 format -> the _h16
// stems of kh_gemm_h16.h) and PG_Q16 (the int8 image -> the _q16 stems of kh_gemm_q16.h).  Host code only: the register
// tiles of each core, which core runs a launch class, the launch description kh_model_gemm.hip::pg_gemm hands over, and
// the launch text (the tile pick, the kh_pick over epilogue and tile, the three token addressings).  A translation unit
// instantiates ONE core behind its kernel header (KH_GEMM16_LAUNCH at the end: kh_model_gemm_w16.hip, _h16.hip,
// _q16.hip - units of their own so that the 24 - 28 kernels of each compile side by side, kh_model_gemm_h16.hip with flags
// of its own); kh_model_gemm.hip names the three launches and compiles none of their kernels.
// Replaces nothing in the reference (it multiplies fp32 by fp32, or dequantises per element, on CUDA cores:
// kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-96).
#pragma once
#include "kh_dispatch.h"
#include "kh_gemm.h"
#include "kh_model_internal.h"
#include "kh_seq_gemm.h"
#include "kh_seq_prefill.h"

namespace khm {

// The (R, NT) register tiles of the family in the order of kh_model_gemm.hip::kPgTiles.  PG_W16 is compiled for all four;
// the other two without (2,8), which does not fit their 256 registers (kh_gemm_h16.h, kh_gemm_q16.h) - the plan runs
// (2,4) in its place (pg_plan).  The wide pass has no (2,8) under any core.
constexpr int kPg16Tiles[4][2] = {{2, 8}, {2, 4}, {2, 2}, {1, 4}};
constexpr int pg16_tile(PgCore core, int R, int NT) {  // index in kPg16Tiles, -1: the core has no such tile
  for (int i = core == PG_W16 ? 0 : 1; i < 4; ++i)
    if (kPg16Tiles[i][0] == R && kPg16Tiles[i][1] == NT) return i;
  return -1;
}

// The core that runs the GEMMs of a launch class (KH_W16_*) in the GEMM pass: the image's own loop, or - where a GEMM16*
// flag adopted the class (kh_model::Gemm16) - one on the bf16 matrix cores.  The two that read the 16-bit copy need it
// live: a copy its self-check gave up (w16.state -2) takes their launches with it.  An int8 model has no copy.
inline PgCore pg_core_of(const kh_model* m, int cls) {
  const bool f16 = m->w16.format == 1 /* KH_W16_F16 (kh_w16.h) */;
  if (m->w16.state == 1 && ((f16 ? m->g16f16 : m->g16).classes & cls) != 0) return f16 ? PG_H16 : PG_W16;
  if ((m->g16q8.classes & cls) != 0) return PG_Q16;
  return m->cfg.is_quant ? PG_Q8 : PG_F32;
}

struct PgGemm16Launch {  // one GEMM of a pass as pg_gemm planned it, on the stems of one core
  int epi, R, NT;        // KH_PG_*; an (R, NT) register tile of the core (pg16_tile)
  dim3 grid;
  int wg;
  size_t lds;
};
// a: the image launch's arguments - under PG_W16 / PG_H16 with KhLin::w of every matrix pointing into the 16-bit copy,
// under PG_Q16 the int8 image's own.  tiles / lanes: the token addressing (both null: a run).  false: nothing launched -
// the LDS opt-in was refused, or the core has no such tile (pg_gemm and gemm16_op pass listed tiles only)
typedef bool (*PgGemm16LaunchFn)(const PgGemm16Launch& L, hipStream_t stream, const KhPgGemmArgs& a,
                                 const KhRgTiles* tiles, const KhWideLanes* lanes);
bool pg_gemm_w16_launch(const PgGemm16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
                        const KhWideLanes* lanes);
bool pg_gemm_h16_launch(const PgGemm16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
                        const KhWideLanes* lanes);
bool pg_gemm_q16_launch(const PgGemm16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles,
                        const KhWideLanes* lanes);
inline PgGemm16LaunchFn pg_gemm16_launch_of(PgCore core) {
  return core == PG_W16 ? pg_gemm_w16_launch : (core == PG_H16 ? pg_gemm_h16_launch : pg_gemm_q16_launch);
}

// The body of the three operator-level entries (kh_model_gemm.hip), behind their argument checks:
// y[T][ldy] (first M columns of each row) = x[T][K] . w[M][K]^T through the STORE epilogue of `launch`'s stems with a
// row-major B operand.  kcols: the columns of the core's K block; scales / gshift: an int8 w's group scales (else null,
// 0).  The token tiles of the kernel are whole: x is staged into a zero-padded copy, so the call allocates, synchronises
// the stream and frees.  The register tile follows M and T ((2,4) for more than 32 tokens, (2,2) below, (1,4) where 32
// rows do not divide M), the K split the number of blocks (4 waves from 32 blocks, 2 from 8): together the shapes a test
// reaches by its sizes.
int gemm16_op(PgGemm16LaunchFn launch, int kcols, const float* x, const void* w, const float* scales, int gshift, float* y,
              int T, int M, int K, int ldy, hipStream_t s);

// pg_gemm_<SFX>_launch for the core whose stems k_{pg,rg,sg}_gemm_<SFX> the unit compiled
#define KH_GEMM16_LAUNCH(CORE, SFX)                                                                                      \
  bool pg_gemm_##SFX##_launch(const PgGemm16Launch& L, hipStream_t stream, const KhPgGemmArgs& a, const KhRgTiles* tiles, \
                              const KhWideLanes* lanes) {                                                                \
    const int tile = pg16_tile(CORE, L.R, L.NT);                                                                         \
    if (tile < 0) return false;                                                                                          \
    auto opt_in = [&](auto kern, dim3&) { return pg_lds_opt_in((const void*)kern, L.lds); };                             \
    bool launched = false;                                                                                               \
    kh_pick(KhVals<KH_PG_QKV, KH_PG_RESID, KH_PG_SWIGLU, KH_PG_STORE>{}, L.epi, [&](auto E) {                            \
      kh_pick(KhVals<0, 1, 2, 3>{}, tile, [&](auto I) {                                                                  \
        constexpr int EPI = decltype(E)::value, R = kPg16Tiles[I][0], NT = kPg16Tiles[I][1];                             \
        if constexpr (pg16_tile(CORE, R, NT) >= 0) {                                                                     \
          if (lanes) {                                                                                                   \
            if constexpr (NT <= 4)                                                                                       \
              launched = kh_launch_prep(opt_in, KH_KERNEL(k_sg_gemm_##SFX, R, NT, EPI), L.grid, L.wg, L.lds, stream, a,  \
                                        *lanes);                                                                         \
            return;                                                                                                      \
          }                                                                                                              \
          if constexpr (EPI == KH_PG_QKV) { /* the other GEMMs do not care where a token sits */                         \
            if (tiles) {                                                                                                 \
              launched = kh_launch_prep(opt_in, KH_KERNEL(k_rg_gemm_##SFX, R, NT, EPI), L.grid, L.wg, L.lds, stream, a,  \
                                        *tiles);                                                                         \
              return;                                                                                                    \
            }                                                                                                            \
          }                                                                                                              \
          if constexpr (EPI != KH_PG_STORE) /* the classifier epilogue is the lanes' alone */                            \
            launched = kh_launch_prep(opt_in, KH_KERNEL(k_pg_gemm_##SFX, R, NT, EPI), L.grid, L.wg, L.lds, stream, a);   \
        }                                                                                                                \
      });                                                                                                                \
    });                                                                                                                  \
    return launched;                                                                                                     \
  }

}  // namespace khm
