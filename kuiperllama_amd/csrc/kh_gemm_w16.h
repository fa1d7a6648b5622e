// kh_gemm_w16.h — the GEMM pass of kh_gemm.h on the bf16 matrix cores, fp32-accurate (KH_FLAG_GEMM16).
//
// A W16 model (kh_w16.h) holds every matrix as exact bf16.  An fp32 activation x splits EXACTLY into three bf16 terms by
// truncation:
//     hi  = x & 0xffff0000            (the sign, the exponent and the upper 8 significand bits of x)
//     mid = (x - hi) & 0xffff0000     (x - hi is exact: the lower 16 significand bits; mid takes the upper 8 of them)
//     lo  = x - hi - mid              (exact; at most 8 significant bits, so lo is a bf16 value itself)
// hi + mid + lo == x for every finite x; lo is bf16-exact unless it falls into the fp32 subnormals (|x| < 2^-100 or
// so), where its low bits are dropped - an error below 2^-149 * 2^16 per term.  A bf16 x bf16 product is exact in
// fp32, so
//     acc = mfma_bf16(w, hi, acc);  acc = mfma_bf16(w, mid, acc);  acc = mfma_bf16(w, lo, acc)
// with v_mfma_f32_16x16x32_bf16 accumulates the fp32 dot product of 32 columns in fp32: what the eight
// v_mfma_f32_16x16x4_f32 of pg_kloop_f32 compute, in another summation order - kh_model_prefill_gemm's contract.  Two
// terms are not enough (16 significand bits).
//
// Operand map (MI355X guide §3, 16x16x32): lane (i = l & 15, h = l >> 4) holds A[row i][k = 8h .. 8h + 7] and
// B[k = 8h .. 8h + 7][column i].  Blocks are 32 columns:
//   * weights: the lane's eight bf16 W16[row i][32b + 8h .. +8] are ONE 16-byte non-temporal load from the row-major
//     16-bit copy;
//   * activations: the eight fp32 Xn[token i][32b + 8h .. +8] are 32 contiguous bytes of the slabs the fp32 loops read -
//     tiled [K/16][tcap][16]: 16-column block 2b + (h >> 1), half h & 1; row-major [T][K]: as they lie - so the
//     producers (k_pg_rmsnorm, the SwiGLU epilogue, the attention kernels) write what they always wrote.  The split
//     runs in registers on bit masks, exact subtractions and v_perm_b32 packs; no convert instruction, no rounding mode;
//   * C/D: that of 16x16x4 f32 (the C/D map does not depend on the input type), so everything below the K loop in
//     kh_gemm_body.h - the ks reduction, kz partials, bias, both RoPE epilogues, residual, SwiGLU, STORE - is unchanged.
// Operand feeding: a uniform ring as pg_kloop_f32_ring's - weights AND activations of block b + D requested together
// when block b has been consumed - that takes any block count: a range shorter than the ring fills the spare slots
// with its last block, and nothing is requested past the range.
// The split costs ~44 VALU instructions per token tile and block, shared by the R row tiles of the wave.
// Replaces nothing in the reference (it multiplies fp32 by fp32 on CUDA cores: cuda/matmul_kernel.cu:8-44).
// gfx950 only.
#pragma once
#include "kh_gemm.h"
#include "kh_seq_gemm.h"
#include "kh_seq_prefill.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t pg_u32x4 __attribute__((ext_vector_type(4)));

// the upper halves of two words as a bf16 pair: element 0 = e0's, element 1 = e1's (one v_perm_b32)
__device__ __forceinline__ uint32_t pg_pack_hi16(float e0, float e1) {
  return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, e1), __builtin_bit_cast(uint32_t, e0), 0x07060302u);
}
__device__ __forceinline__ float pg_trunc16(float v) {
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) & 0xffff0000u);
}
// eight fp32 values -> their three bf16x8 terms (see the head of the file)
struct PgSplit3 {
  bf16x8 hi, mid, lo;
};
__device__ __forceinline__ PgSplit3 pg_split3(const f32x4& u, const f32x4& v) {
  const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
  float r[8], s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    r[e] = x[e] - pg_trunc16(x[e]);  // exact: the lower 16 significand bits
    s[e] = r[e] - pg_trunc16(r[e]);  // exact: the lowest 8
  }
  pg_u32x4 hi, mid, lo;
  hi.x = pg_pack_hi16(x[0], x[1]); hi.y = pg_pack_hi16(x[2], x[3]); hi.z = pg_pack_hi16(x[4], x[5]); hi.w = pg_pack_hi16(x[6], x[7]);
  mid.x = pg_pack_hi16(r[0], r[1]); mid.y = pg_pack_hi16(r[2], r[3]); mid.z = pg_pack_hi16(r[4], r[5]); mid.w = pg_pack_hi16(r[6], r[7]);
  lo.x = pg_pack_hi16(s[0], s[1]); lo.y = pg_pack_hi16(s[2], s[3]); lo.z = pg_pack_hi16(s[4], s[5]); lo.w = pg_pack_hi16(s[6], s[7]);
  return PgSplit3{__builtin_bit_cast(bf16x8, hi), __builtin_bit_cast(bf16x8, mid), __builtin_bit_cast(bf16x8, lo)};
}

// ring depth per register tile: D * (R + 2 NT) float4 of ring registers beside the R * NT accumulators, within the 256
// registers of two waves per SIMD
template <int R, int NT>
struct PgW16Ring {
  static constexpr int D = R * NT >= 16 ? 2 : (R * NT >= 8 ? 3 : 4);
};

// bf16 weights: blocks of 32 columns [b0, b1), b1 > b0; lane (i, h) owns W16[i][32b + 8h .. +8] of each of its R tiles
// (wrow[r] points at the lane's eight columns of block 0) and Xn[token][32b + 8h .. +8] of each of its NT token tiles
// (B.base likewise; s_nt / s_b in floats per token tile / per block of 32)
template <int R, int NT>
__device__ __forceinline__ void pg_kloop_w16(const uint16_t* const (&wrow)[R], const PgBAddr& B, int b0, int b1,
                                             f32x4 (&acc)[R][NT]) {
  constexpr int D = PgW16Ring<R, NT>::D;
  pg_u32x4 a[D][R];
  f32x4 xb[D][NT][2];
  const int last = b1 - 1;
  auto load = [&](int slot, int bb) __attribute__((always_inline)) {
    bb = bb < last ? bb : last;  // (wave-uniform)
#pragma unroll
    for (int r = 0; r < R; ++r) a[slot][r] = ld_nt((const pg_u32x4*)(wrow[r] + (size_t)bb * 32));
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float* p = B.base + nt * B.s_nt + (size_t)bb * B.s_b;
      xb[slot][nt][0] = *(const f32x4*)p;
      xb[slot][nt][1] = *(const f32x4*)(p + 4);
    }
    __builtin_amdgcn_sched_barrier(0);  // slots stay in issue order (vmcnt retires in order)
  };
  auto mfma = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const PgSplit3 x = pg_split3(xb[slot][nt][0], xb[slot][nt][1]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, a[slot][r]);
        acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x.hi, acc[r][nt], 0, 0, 0);
        acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x.mid, acc[r][nt], 0, 0, 0);
        acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x.lo, acc[r][nt], 0, 0, 0);
      }
    }
  };
#pragma unroll
  for (int d = 0; d < D; ++d) load(d, b0 + d);
  for (int b = b0; b < b1; b += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (b + d < b1) {  // wave-uniform (b0, b1 are scalars)
        mfma(d);
        if (b + d + D < b1) load(d, b + d + D);
      }
    }
  }
}

// The kernels: kh_gemm_body.h with the K loop above (KH_GEMM_W16), under the three token addressings of the GEMM pass.
// KhLin::w of every matrix points into the 16-bit copy.  Launch geometry, LDS and arguments are k_pg_gemm's.
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_F32) void k_pg_gemm_w16(const KhPgGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  static_assert(EPI != KH_PG_STORE, "the classifier epilogue is the wide sequence pass's (k_sg_gemm_w16)");
  constexpr bool QUANT = false, KH_GEMM_W16 = true, KH_GEMM_Q16 = false;
  const PgRunAddr addr{a.pos0};
#include "kh_gemm_body.h"
}
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_F32) void k_rg_gemm_w16(const KhPgGemmArgs a, const KhRgTiles tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  static_assert(EPI == KH_PG_QKV, "the other GEMMs of the pass are k_pg_gemm_w16's");
  constexpr bool QUANT = false, KH_GEMM_W16 = true, KH_GEMM_Q16 = false;
  const RgTileAddr addr{tiles};
#include "kh_gemm_body.h"
}
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_F32) void k_sg_gemm_w16(const KhPgGemmArgs a, const KhWideLanes lanes) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr bool QUANT = false, KH_GEMM_W16 = true, KH_GEMM_Q16 = false;
  const SgLaneAddr addr{lanes};
#include "kh_gemm_body.h"
}
