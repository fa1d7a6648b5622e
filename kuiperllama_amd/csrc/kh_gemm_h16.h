// kh_gemm_h16.h — the GEMM pass of an fp16-origin fp32 model on the bf16 matrix cores, fp32-accurate, from the
// fp16-format 16-bit copy (KH_FLAG_GEMM16_F16).  No second copy, no rounding.
//
// Every finite fp16 value w has 11 significand bits and an exponent far inside bf16's range, so - on the fp32 word the
// exact widening GemvW16<KH_W16_F16>::widen (kh_w16.h) gives - it splits EXACTLY into two bf16 numbers by truncation:
//     w_hi = f32(w) & 0xffff0000      (the sign, the exponent and the upper 8 significand bits)
//     w_lo = f32(w) - w_hi            (exact: at most 3 significant bits; zero, or at least 2^-34 in magnitude - a bf16
//                                      normal; fp16 subnormals and +-0 split exactly too)
// w_hi + w_lo == w.  The activation side is pg_split3 of kh_gemm_w16.h unchanged (x == hi + mid + lo, exact).  A
// bf16 x bf16 product is exact in fp32, so the six v_mfma_f32_16x16x32_bf16
//     {w_hi, w_lo} x {x_hi, x_mid, x_lo}
// accumulate the fp32 dot product of 32 columns in fp32: what the eight v_mfma_f32_16x16x4_f32 of pg_kloop_f32 compute,
// in another summation order - kh_model_prefill_gemm's contract.  All six terms are kept (w_lo * x_lo is not dropped:
// without it a single product would no longer be exact).
// Issue order of the six terms of a (row tile, token tile, block), fixed, onto TWO fp32 accumulators kept over the whole
// K range of the wave:
//     acc  += w_hi*x_hi                                                  (the leading term: 16 of the 24 + 11 product bits)
//     accl += w_lo*x_hi, w_hi*x_mid, w_lo*x_mid, w_hi*x_lo, w_lo*x_lo    (all at most 2^-8 of the leading term)
// and acc += accl once behind the loop.  Every MFMA rounds its accumulator once; with all six on one accumulator a block
// costs six roundings at the magnitude of the sum (measured on the operator's general case: 2.4e-6 against the fp32
// GEMV's 6.6e-7), with the split one, plus five at 2^-8 of it - and the two chains are independent, so neither waits
// for the other's result.  The one-hot and integer cases stay exact: every partial sum of either chain and their sum
// are multiples of the product's last place bounded by the product.
//
// Operand map and ring: pg_kloop_w16's.  Lane (i = l & 15, h = l >> 4) holds A[row i][k = 8h .. 8h + 7] and
// B[k = 8h .. 8h + 7][column i]; blocks are 32 columns; the lane's eight fp16 weights of a block are ONE 16-byte
// non-temporal load from the row-major copy, the activations the 32 bytes the fp32 loops read; weights AND activations
// of block b + D are requested together when block b has been consumed; a range shorter than the ring repeats its last
// block, and nothing is requested past the range.
// Slot order inside one block: the weight split of the R row tiles first (8 conversions, 8 masks, 8 exact
// subtractions, 8 v_perm_b32 packs per tile; once per (row tile, block), shared by the wave's NT token tiles), then per
// token tile its pg_split3 (once per (token tile, block), shared by the R row tiles) followed by its 6 R MFMAs, the R
// independent chains interleaved term by term.  So a wave alternates a VALU stretch of ~44 instructions with a stretch
// of 6 R MFMAs (R leading, 5 R small) NT times per block; its partner wave on the SIMD runs out of phase and finds the matrix pipe free
// while this one splits - the launch plan never goes solo on the 16-bit copy.
// The split uses no rounding mode and no convert on the way back: the conversion fp16 -> fp32 is exact, the rest is a
// mask, an exact subtraction and packs of upper halves.
// Register tiles: (2,4), (2,2), (1,4).  (2,8) is not compiled: its 128 accumulators, the ring and both splits do not fit
// 256 registers; the plan runs (2,4) (as for kh_gemm_q16.h).  Resource numbers: DESIGN 3.1g.
// Replaces nothing in the reference (it multiplies fp32 by fp32 on CUDA cores: cuda/matmul_kernel.cu:8-44).
// gfx950 only.
#pragma once
#include "kh_gemm_w16.h"

// eight fp16 values (four dwords, the low half first) -> their two bf16x8 terms (see the head of the file)
struct PgSplitH16 {
  bf16x8 hi, lo;
};
__device__ __forceinline__ PgSplitH16 pg_split_h16(const pg_u32x4& q) {
  const uint32_t d[4] = {q.x, q.y, q.z, q.w};
  float f[8], g[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = (float)__builtin_bit_cast(_Float16, (uint16_t)(d[e] & 0xffffu));  // exact (kh_w16.h: widen)
    f[2 * e + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(d[e] >> 16));
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] = f[e] - pg_trunc16(f[e]);  // exact: the lower 3 significand bits
  pg_u32x4 hi, lo;
  hi.x = pg_pack_hi16(f[0], f[1]); hi.y = pg_pack_hi16(f[2], f[3]); hi.z = pg_pack_hi16(f[4], f[5]); hi.w = pg_pack_hi16(f[6], f[7]);
  lo.x = pg_pack_hi16(g[0], g[1]); lo.y = pg_pack_hi16(g[2], g[3]); lo.z = pg_pack_hi16(g[4], g[5]); lo.w = pg_pack_hi16(g[6], g[7]);
  return PgSplitH16{__builtin_bit_cast(bf16x8, hi), __builtin_bit_cast(bf16x8, lo)};
}

// ring depth per register tile: D * (R + 2 NT) float4 of ring registers beside the 2 R * NT accumulators, 2 R float4 of
// split weights and one split activation tile, within the 256 registers of two waves per SIMD
template <int R, int NT>
struct PgH16Ring {
  static_assert(R * NT <= 8, "the (2,8) tile does not fit (see the head of the file)");
  static constexpr int D = R * NT >= 8 ? 3 : 4;
};

// fp16 weights: pg_kloop_w16's ring (pg_ring16); a slot splits the weights and issues six MFMAs on two accumulators
template <int R, int NT>
__device__ __forceinline__ void pg_kloop_h16(const uint16_t* const (&wrow)[R], const PgBAddr& B, int b0, int b1,
                                             f32x4 (&acc)[R][NT]) {
  f32x4 accl[R][NT];  // the five small terms (see the head of the file)
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) accl[r][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  pg_ring16<PgH16Ring<R, NT>::D, R, NT>(wrow, B, b0, b1, [&](const pg_u32x4 (&a)[R], const f32x4 (&xb)[NT][2])
                                                             __attribute__((always_inline)) {
    PgSplitH16 w[R];
#pragma unroll
    for (int r = 0; r < R; ++r) w[r] = pg_split_h16(a[r]);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const PgSplit3 x = pg_split3(xb[nt][0], xb[nt][1]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r].hi, x.hi, acc[r][nt], 0, 0, 0);
        accl[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r].lo, x.hi, accl[r][nt], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        accl[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r].hi, x.mid, accl[r][nt], 0, 0, 0);
        accl[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r].lo, x.mid, accl[r][nt], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        accl[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r].hi, x.lo, accl[r][nt], 0, 0, 0);
        accl[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r].lo, x.lo, accl[r][nt], 0, 0, 0);
      }
    }
  });
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      acc[r][nt].x += accl[r][nt].x; acc[r][nt].y += accl[r][nt].y;
      acc[r][nt].z += accl[r][nt].z; acc[r][nt].w += accl[r][nt].w;
    }
}
KH_PG_KLOOP(PG_H16, pg_kloop_h16);

// The kernels: kh_gemm_body.h with the K loop above (CORE = PG_H16), under the three token addressings of the GEMM pass.
// KhLin::w of every matrix points into the fp16-format copy.  Launch geometry, LDS and arguments are k_pg_gemm's.
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_F32) void k_pg_gemm_h16(const KhPgGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  static_assert(EPI != KH_PG_STORE, "the classifier epilogue is the wide sequence pass's (k_sg_gemm_h16)");
  constexpr PgCore CORE = PG_H16;
  const PgRunAddr addr{a.pos0};
#include "kh_gemm_body.h"
}
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_F32) void k_rg_gemm_h16(const KhPgGemmArgs a, const KhRgTiles tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  static_assert(EPI == KH_PG_QKV, "the other GEMMs of the pass are k_pg_gemm_h16's");
  constexpr PgCore CORE = PG_H16;
  const RgTileAddr addr{tiles};
#include "kh_gemm_body.h"
}
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_F32) void k_sg_gemm_h16(const KhPgGemmArgs a, const KhWideLanes lanes) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr PgCore CORE = PG_H16;
  const SgLaneAddr addr{lanes};
#include "kh_gemm_body.h"
}
