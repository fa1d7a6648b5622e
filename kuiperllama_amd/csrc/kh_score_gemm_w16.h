// kh_score_gemm_w16.h — the scoring classifier of kh_score_gemm.h on the bf16 matrix cores, from the bf16-format 16-bit
// copy, with the activations split ONCE per workgroup in LDS (KH_FLAG_GEMM16 with the cls class).
//
//   k_pg_cls_lse_w16<NT>   k_pg_cls_lse's work split - 4 waves = KH_CL_ROWS vocabulary rows x one slice of 16 NT tokens,
//                          every wave two 16-row tiles over the whole K, blockIdx.x = block * slices + slice, the
//                          accumulators in registers to the end - and its epilogue (kh_score_gemm_epilogue.h), on
//                          v_mfma_f32_16x16x32_bf16 with kh_gemm_w16.h's three-term split of the fp32 activations.
// The loops of kh_gemm_w16.h split in registers: every wave splits the activations it multiplies, ~44 VALU instructions
// per token tile and block of 32 columns, shared by its R = 2 row tiles - and the four waves of a workgroup here would
// split the SAME token slice four times.  Here the workgroup splits each (token, 8-column octet) once:
//   * staging: block b of the slice is 16 NT tokens x 4 octets; thread t takes the octets (token 16 nt + (t & 15),
//     octet 2 c + ((t >> 4) & 1)) with nt + NT c = (t >> 5) + 8 j, j < NT / 4 - two octets a thread for NT = 8, one for
//     NT = 4.  An octet is 32 contiguous bytes of the tiled slab k_pg_rmsnorm leaves ([K/16][tcap][16]: 16-column block
//     2 b + c, half (t >> 4) & 1), a wave's loads cover 2 KB of it without a gap.  pg_split3 makes the three bf16x8
//     terms, each ONE 16-byte LDS store;
//   * LDS: s_x[buffer][term][token tile][64] x 16 bytes, slot 16 h + i = the B operand of lane (i, h) (token i of the
//     tile, k = 8 h .. 8 h + 7): a wave fetches a term of a token tile as 64 consecutive 16-byte words - one
//     ds_read_b128, no bank conflict - and the 16 lanes t & 15 of a staging store write 256 consecutive bytes;
//   * two buffers (2 x 3 x NT KB: 48 KB for NT = 8): block b + 1 is split and stored and block b + 2 requested ahead of
//     the MFMAs of block b, ONE barrier per block behind them.  A single block is the prologue alone, in buffer 0;
//   * weights: lane (i, h) loads W16[row i][32 b + 8 h .. +8] of its two tiles as one 16-byte non-temporal load each,
//     through a register ring KH_CL16_RING_D blocks deep, filled and refilled as pg_ring16's weight half (any block
//     count: a range shorter than the ring fills the spare slots with its last block);
//   * three MFMAs per (row tile, token tile, block) on one accumulator, hi, mid, lo, token tiles outside the row tiles:
//     pg_kloop_w16's order, so a logit is the value k_sg_gemm_w16's STORE epilogue would write.
// Numerics: kh_gemm_w16.h's - the fp32 dot product in another summation order; weights must be finite (a -inf weight
// times a zero term of the split is NaN).  Activations of padding tokens (finite, or whatever the slab holds) meet only
// their own columns, which leave no record.
// Static LDS 48 + 12 KB (NT = 8), 24 + 6 KB (NT = 4).  No scratch, no inline assembly; gfx950 only.
// The reference has no scoring call and multiplies fp32 by fp32 (cuda/matmul_kernel.cu:8-44).
#pragma once
#include "kh_gemm_w16.h"
#include "kh_score_gemm.h"

#define KH_CL16_RING_D 4  // blocks of weights in flight per wave: 4 x 2 KB

template <int NT>
__global__ __launch_bounds__(KH_CL_WAVES * 64) void k_pg_cls_lse_w16(const KhClsLseArgs a) {
  constexpr int R = KH_CL_R, TW = 16 * NT, D = KH_CL16_RING_D, ITEMS = NT / 4;
  static_assert(NT % 4 == 0 && D % 2 == 0, "whole octets per thread; the buffer of a ring slot is its parity");
  __shared__ pg_u32x4 s_x[2][3][NT][64];
  __shared__ float s_red[2][KH_CL_WAVES][TW];
  __shared__ float s_cv[2][KH_CL_WAVES][TW];
  __shared__ int s_ci[2][KH_CL_WAVES][TW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 15, h = lane >> 4;
  const int blk = (int)blockIdx.x / a.slices, slice = (int)blockIdx.x - blk * a.slices;
  const int tok0 = slice * TW;
  const int K = a.K, nb = K >> 5;
  int trow[R];
  bool valid[R];  // wave-uniform
  const uint16_t* wrow[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    trow[r] = blk * KH_CL_ROWS + (wave * R + r) * 16;
    valid[r] = trow[r] < a.vocab;
    wrow[r] = (const uint16_t*)a.w.w + (size_t)((valid[r] ? trow[r] : a.vocab - 16) + i) * K + 8 * h;
  }
  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- the thread's octets of a block: where they lie in the slab (block 0) and where their terms go in a buffer
  const size_t xstride = (size_t)2 * a.tcap * 16;  // floats between two blocks of 32 columns
  const float* xsrc[ITEMS];
  int xnt[ITEMS], xslot[ITEMS];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const int rest = (tid >> 5) + 8 * j, c = rest / NT, half = (tid >> 4) & 1;
    xnt[j] = rest % NT;
    xslot[j] = (2 * c + half) * 16 + i;
    xsrc[j] = a.B + ((size_t)c * a.tcap + tok0 + 16 * xnt[j] + i) * 16 + 8 * half;
  }
  f32x4 xr[ITEMS][2];
  auto fetch = [&](int bb) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      const float* p = xsrc[j] + (size_t)bb * xstride;
      xr[j][0] = *(const f32x4*)p;
      xr[j][1] = *(const f32x4*)(p + 4);
    }
  };
  auto stage = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      const PgSplit3 x = pg_split3(xr[j][0], xr[j][1]);
      s_x[buf][0][xnt[j]][xslot[j]] = __builtin_bit_cast(pg_u32x4, x.hi);
      s_x[buf][1][xnt[j]][xslot[j]] = __builtin_bit_cast(pg_u32x4, x.mid);
      s_x[buf][2][xnt[j]][xslot[j]] = __builtin_bit_cast(pg_u32x4, x.lo);
    }
  };

  // ---- the weight ring (pg_ring16's weight half)
  pg_u32x4 wr[D][R];
  const int last = nb - 1;
  auto load = [&](int d, int bb) __attribute__((always_inline)) {
    bb = bb < last ? bb : last;  // (uniform)
#pragma unroll
    for (int r = 0; r < R; ++r) wr[d][r] = ld_nt((const pg_u32x4*)(wrow[r] + (size_t)bb * 32));
    __builtin_amdgcn_sched_barrier(0);  // slots stay in issue order (vmcnt retires in order)
  };
#pragma unroll
  for (int d = 0; d < D; ++d) load(d, d);

  // ---- prologue: block 0 into buffer 0, block 1 requested
  fetch(0);
  stage(0);
  if (nb > 1) fetch(1);
  __syncthreads();
  for (int b = 0; b < nb; b += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int bb = b + d;  // its buffer is d & 1: b is a multiple of the even D
      if (bb < nb) {         // uniform
        if (bb + 1 < nb) {
          stage((d + 1) & 1);  // (its readers, block bb - 1's MFMAs, are behind the last barrier)
          if (bb + 2 < nb) fetch(bb + 2);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const bf16x8 hi = __builtin_bit_cast(bf16x8, s_x[d & 1][0][nt][lane]);
          const bf16x8 mid = __builtin_bit_cast(bf16x8, s_x[d & 1][1][nt][lane]);
          const bf16x8 lo = __builtin_bit_cast(bf16x8, s_x[d & 1][2][nt][lane]);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bf16x8 w = __builtin_bit_cast(bf16x8, wr[d][r]);
            acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, hi, acc[r][nt], 0, 0, 0);
            acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, mid, acc[r][nt], 0, 0, 0);
            acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, lo, acc[r][nt], 0, 0, 0);
          }
        }
        if (bb + D < nb) load(d, bb + D);
        if (bb + 1 < nb) __syncthreads();  // block bb + 1 is whole, block bb's buffer free
      }
    }
  }
#include "kh_score_gemm_epilogue.h"
}
