// kh_gemm_q16.h — the GEMM pass of an int8 group-64 model on the bf16 matrix cores, fp32-accurate, from the int8 image
// itself (KH_FLAG_GEMM16_Q8).  No weight copy.
//
// Every int8 value -128 .. 127 is an exact bf16 number (at most 8 significant bits), and an fp32 activation splits
// exactly into three bf16 terms (kh_gemm_w16.h: pg_split3).  A bf16 x bf16 product is exact in fp32, so for one group of
// 64 columns
//     t = sum over the group of q * (hi + mid + lo)          six v_mfma_f32_16x16x32_bf16, fp32 accumulation from zero
//     acc += s * t                                            the group scale, ONCE per partial sum (fmaf)
// is the int8 GEMM prefill's contract - exact products, fp32 accumulation - in another summation order, without the
// per-weight rounding of s * q that pg_kloop_q8 (and the reference: cuda/matmul_kernel.cu:73) performs.  pg_kloop_q8
// spends sixteen v_mfma_f32_16x16x4_f32 on the same group, an instruction that runs at 1/16 of the bf16 rate.
//
// Operand map: the int8 loop's lane map is kept.  Lane (i = l & 15, h = l >> 4) loads W8[row i][64b + 16h .. +16] as ONE
// non-temporal dwordx4; its bytes 8s .. 8s + 7 are the A operand of MFMA step s (s = 0, 1) and pair with
// Xn[token i][64b + 16h + 8s .. +8]: quarters 2s and 2s + 1 of the int8 tiled slab (pg_tiled_index(true, ...)), or 32
// contiguous bytes of a row-major slab.  A and B use the same column permutation inside the group (MFMA k index
// 8h + e <-> column 16h + 8s + e), so the two steps together contract all 64 columns and the producers (k_pg_rmsnorm<true>,
// the SwiGLU epilogue, the attention kernels) write what they always wrote.
//   * weights: int8 -> fp32 (exact) -> upper 16 bits (exact: 8 significant bits) packed by v_perm_b32; no rounding mode
//     is involved.  Done once per step and row tile, shared by the NT token tiles.
//   * activations: pg_split3, shared by the R row tiles.
//   * scale: in the C/D map a lane holds rows 4h .. 4h + 3 of the tile for token i - not row i, whose weights it loaded.
//     The lane loads the scale of row 4h + (i & 3); the four lanes of a quad hold the four scales every lane of the
//     quad needs, and a quad-permute DPP move broadcasts each.
//   * each step's three MFMAs accumulate into a partial of their own that starts from zero (two token tiles at a time:
//     2 R independent chains of three), and acc = fmaf(s, t, acc) follows - explicitly fmaf: the library is built with
//     -ffp-contract=off.  So a group adds two scaled partials of 32 columns each.
// Operand feeding: a uniform ring as pg_kloop_w16's, with the activations counted in steps of 32 columns: when step u
// has been consumed the activations of step u + DX are requested (DX = 2 or 4), and when block b has been consumed the
// weights and scales of block b + 2 (two weight slots).  Any block count is taken: a range shorter than the ring fills
// the spare slots with its last block, and nothing is requested past the range.  The (2,8) register tile is not
// compiled: its 64 accumulators, 128 activation registers per block and the partials do not fit 256 registers; the plan
// runs (2,4).  Compiled: (2,4) 254, (2,2) 202, (1,4) 250 VGPRs, no scratch.
// Replaces nothing in the reference (it dequantises per element on CUDA cores: cuda/matmul_kernel.cu:50-96).
// gfx950 only.
#pragma once
#include "kh_gemm_w16.h"

// eight int8 values (two dwords, byte 0 first) as eight bf16: exact
__device__ __forceinline__ bf16x8 pg_q8_to_bf16x8(int d0, int d1) {
  float f[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = (float)(int8_t)((d0 >> (8 * e)) & 0xff);
    f[4 + e] = (float)(int8_t)((d1 >> (8 * e)) & 0xff);
  }
  pg_u32x4 p;
  p.x = pg_pack_hi16(f[0], f[1]); p.y = pg_pack_hi16(f[2], f[3]); p.z = pg_pack_hi16(f[4], f[5]); p.w = pg_pack_hi16(f[6], f[7]);
  return __builtin_bit_cast(bf16x8, p);
}
// the value lane J of the caller's quad holds (v_mov_b32 quad_perm:[J,J,J,J])
template <int J>
__device__ __forceinline__ float pg_quad_bcast(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), J * 0x55, 0xf, 0xf, true));
}

// activation steps in flight per register tile: DX * 8 NT ring registers beside 2 * 5 R of the weight ring, the 4 R NT
// accumulators, 24 of two splits and 8 R of partials - within the 256 registers of two waves per SIMD
template <int R, int NT>
struct PgQ16Ring {
  static_assert(R * NT <= 8 && NT % 2 == 0, "the (2,8) tile does not fit (see the head of the file)");
  static constexpr int DX = R * NT >= 8 ? 2 : 4;
};

// int8 group-64 weights: blocks of 64 columns [b0, b1), b1 > b0.  wrow[r]: the lane's sixteen columns of block 0 of row
// i of tile r; srow[r]: the scales of row 4h + (i & 3) of tile r; B: the int8 loop's addressing (s_q: floats per quarter)
template <int R, int NT>
__device__ __forceinline__ void pg_kloop_q16(const int8_t* const (&wrow)[R], const float* const (&srow)[R],
                                             const PgBAddr& B, int b0, int b1, f32x4 (&acc)[R][NT]) {
  constexpr int DX = PgQ16Ring<R, NT>::DX;
  i32x4 qw[2][R];
  float sc[2][R];
  f32x4 xb[DX][NT][2];
  const int last = b1 - 1;
  auto load_w = [&](int slot, int bb) __attribute__((always_inline)) {
    bb = bb < last ? bb : last;  // (wave-uniform)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      qw[slot][r] = ld_nt((const i32x4*)(wrow[r] + (size_t)bb * 64));
      sc[slot][r] = srow[r][bb];
    }
    __builtin_amdgcn_sched_barrier(0);  // slots stay in issue order (vmcnt retires in order)
  };
  auto load_x = [&](int slot, int bb, int s) __attribute__((always_inline)) {
    bb = bb < last ? bb : last;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float* p = B.base + nt * B.s_nt + (size_t)bb * B.s_b + (size_t)(2 * s) * B.s_q;
      xb[slot][nt][0] = *(const f32x4*)p;
      xb[slot][nt][1] = *(const f32x4*)(p + B.s_q);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto step = [&](int xs, int ws, int s) __attribute__((always_inline)) {
    bf16x8 w[R];
    float sj[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const i32x4 qv = qw[ws][r];
      w[r] = s == 0 ? pg_q8_to_bf16x8(qv.x, qv.y) : pg_q8_to_bf16x8(qv.z, qv.w);
      sj[r][0] = pg_quad_bcast<0>(sc[ws][r]);
      sj[r][1] = pg_quad_bcast<1>(sc[ws][r]);
      sj[r][2] = pg_quad_bcast<2>(sc[ws][r]);
      sj[r][3] = pg_quad_bcast<3>(sc[ws][r]);
    }
#pragma unroll
    for (int nt = 0; nt < NT; nt += 2) {
      const PgSplit3 x0 = pg_split3(xb[xs][nt][0], xb[xs][nt][1]);
      const PgSplit3 x1 = pg_split3(xb[xs][nt + 1][0], xb[xs][nt + 1][1]);
      f32x4 t[R][2];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        t[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r], x0.hi, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        t[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r], x1.hi, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        t[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r], x0.mid, t[r][0], 0, 0, 0);
        t[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r], x1.mid, t[r][1], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        t[r][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r], x0.lo, t[r][0], 0, 0, 0);
        t[r][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[r], x1.lo, t[r][1], 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          f32x4& c = acc[r][nt + p];
          c.x = fmaf(sj[r][0], t[r][p].x, c.x);
          c.y = fmaf(sj[r][1], t[r][p].y, c.y);
          c.z = fmaf(sj[r][2], t[r][p].z, c.z);
          c.w = fmaf(sj[r][3], t[r][p].w, c.w);
        }
    }
  };
  // prologue, in the order of use: block b0 and its steps, block b0 + 1 and (DX = 4) its steps
  load_w(0, b0);
  load_x(0, b0, 0);
  load_x(1, b0, 1);
  load_w(1, b0 + 1);
  if constexpr (DX == 4) {
    load_x(2, b0 + 1, 0);
    load_x(3, b0 + 1, 1);
  }
  for (int b = b0; b < b1; b += 2) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {  // step d & 1 of block b + (d >> 1)
      const int bb = b + (d >> 1);
      if (bb < b1) {  // wave-uniform (b0, b1 are scalars)
        step(d % DX, d >> 1, d & 1);
        if (bb + DX / 2 < b1) load_x(d % DX, bb + DX / 2, d & 1);
        if ((d & 1) == 1 && bb + 2 < b1) load_w(d >> 1, bb + 2);  // the block's weight slot is free
      }
    }
  }
}

// The kernels: kh_gemm_body.h with the K loop above (KH_GEMM_Q16), under the three token addressings of the GEMM pass.
// KhLin::w / scales of every matrix are the image's own.  Launch geometry, LDS and arguments are k_pg_gemm's.
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_Q8) void k_pg_gemm_q16(const KhPgGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  static_assert(EPI != KH_PG_STORE, "the classifier epilogue is the wide sequence pass's (k_sg_gemm_q16)");
  constexpr bool QUANT = true, KH_GEMM_W16 = false, KH_GEMM_Q16 = true;
  const PgRunAddr addr{a.pos0};
#include "kh_gemm_body.h"
}
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_Q8) void k_rg_gemm_q16(const KhPgGemmArgs a, const KhRgTiles tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  static_assert(EPI == KH_PG_QKV, "the other GEMMs of the pass are k_pg_gemm_q16's");
  constexpr bool QUANT = true, KH_GEMM_W16 = false, KH_GEMM_Q16 = true;
  const RgTileAddr addr{tiles};
#include "kh_gemm_body.h"
}
template <int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX_Q8) void k_sg_gemm_q16(const KhPgGemmArgs a, const KhWideLanes lanes) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr bool QUANT = true, KH_GEMM_W16 = false, KH_GEMM_Q16 = true;
  const SgLaneAddr addr{lanes};
#include "kh_gemm_body.h"
}
