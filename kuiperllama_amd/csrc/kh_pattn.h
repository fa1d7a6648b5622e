// kh_pattn.h — causal attention of a prompt slice on the matrix cores (GEMM prefill).
//
// The reference computes attention one query token at a time (cpu/mha_kernel.cpp:5-61,
// cuda/mha_kernel.cu:47-110: score = q.k * 1/sqrt(hs), softmax over 0..pos, out = sum p_t v_t).
// With T prompt tokens in flight, q.K^T and P.V are real GEMMs: here one workgroup owns (head h,
// 16 query tokens) and its four or eight waves split the key/value timesteps in 16-position tiles; both
// contractions run on v_mfma_f32_16x16x4_f32 (exact fp32 fmaf chains), the softmax is the online
// form the decode kernel already uses (running max m, running sum l, rescale by exp(m - m')).
//
// The transposed products make the operands fall out of the registers without any shuffle:
//   S^T[pos, tok] = K[pos, :] . Q[tok, :]      A = K rows (lane i = l&15 -> position), B = Q rows
//       D layout: lane holds column tok = l&15, rows pos = 4*(l>>4) + reg            (reg 0..3)
//   O^T[d, tok]  += V^T[d, pos] . P^T[pos, tok]
//       MFMA #s contracts the position quad {s, 4+s, 8+s, 12+s}: its B operand for k = l>>4 is the
//       lane's OWN register s of P^T - the D layout of the first product IS the B layout of the
//       second.  A = V[pos = 4*(l>>4)+s][d]: the lane loads a float4 V[pos][64c + 4i .. +4] and feeds
//       component a to the accumulator tile (c, a), whose row i stands for d = 64c + 4i + a; in the
//       D layout a lane then holds d = 64c + 16*(l>>4) + 4*reg + a, i.e. 16 consecutive outputs of
//       its token - four float4 stores.
// As in kh_gemm.h the K-side contraction visits the head dimension in the order of the lanes'
// float4 loads (k-quad {16b+s, 16b+4+s, ...}); any order is a valid dot product.
//
// Row statistics: a token's scores sit in 4 registers x 4 lane groups (l>>4); the tile maximum is
// combined across the groups with two ds_bpermute, so every lane of a token uses the same m and
// the P values fed to the matrix core are consistently scaled.  The row sum is kept per lane and
// combined once at the end.  The waves' (m, l, O) partials merge through LDS in fixed order.
//
// Output goes straight into the tiled activation slab the wo GEMM reads (pg_tiled_index).
#pragma once
#include "kh_gemm.h"

struct KhPgAttnArgs {
  const float* q;   // [T][dim] row-major, RoPE applied
  const float* kc;  // this layer's K cache rows [cache_len][kv_dim]; rows pos0 .. pos0+T-1 just written
  const float* vc;
  float* out;       // layout 0 / 1: tiled slab [dim x tcap] of an fp32 / int8 model
                    // (pg_tiled_index, T <= tcap); layout 2: row-major [T][dim]
  int dim, kv_dim, kv_heads, kv_mul, T, pos0, layout, tcap;
};
enum { KH_PA_TILED_F32 = 0, KH_PA_TILED_Q8 = 1, KH_PA_ROWS = 2 };

// The statements of the kernel live in kh_pattn_body.h, included by the two kernels that differ in where the query
// columns and the timesteps sit: k_pg_attn below takes T consecutive positions of one sequence whose position p is
// cache row p (PaRunAddr), kh_seq_prefill.h: k_rg_attn one segment of a sequence slot per query tile (a tile table).
struct PaRunAddr {
  int pos0, T;
  __device__ __forceinline__ int tiles(int qt) const { return (T + 16 * qt - 1) / (16 * qt); }
  __device__ __forceinline__ int last_pos(int t0, int qt) const {
    return pos0 + (t0 + 16 * qt - 1 < T - 1 ? t0 + 16 * qt - 1 : T - 1);
  }
  __device__ __forceinline__ int col(int t) const { return t < T ? t : T - 1; }
  __device__ __forceinline__ int pos(int t) const { return pos0 + col(t); }
  __device__ __forceinline__ int tile_pos0(int t) const { return pos0 + t; }
  __device__ __forceinline__ int row(int, int p) const { return p; }
  __device__ __forceinline__ bool stores(int t) const { return t < T; }
};
template <int HB /* head_size / 16 */, int NW /* waves that split the timesteps: 4 or 8 */,
          int QT /* 16-token query tiles per workgroup: every K/V fragment a wave loads feeds QT tiles */>
__global__ __launch_bounds__(64 * NW) void k_pg_attn(const KhPgAttnArgs a) {
  const PaRunAddr addr{a.pos0, a.T};
#include "kh_pattn_body.h"
}

static inline bool pg_attn_supported(int head_size) {
  return head_size == 48 || head_size == 64 || head_size == 128;
}
// Query tiles per workgroup: every doubling halves the K/V bytes a workgroup pulls through L2 per MFMA
// (256 B per MFMA with one tile).  Measured (profiles/r3_pattn_qt.txt, Llama-3.2-1B, 512-token pass): the
// kernel is closer to MFMA-bound than to L2-bound - 4 tiles take a pass at start position 32256 from 31.95
// to 28.9 ms (attention 1.42 -> 1.23 ms per layer = 111 TFLOP/s of the ~135 the matrix cores deliver in
// fp32), 2 % at position 4096, and LOSE 2 % at position 0 (fewer, longer workgroups on the causal
// triangle); with fewer than 256 workgroups they lose outright (128-token pass at 32256: 8.8 -> 13.8 ms).
// So: more than one tile only from start position 2048 on and only while the launch keeps >= 256
// workgroups.  Head size 128 stops at 2 (registers).  KH_PG_ATTN_QT forces a value.
static inline int pg_attn_qt(const KhPgAttnArgs& a, int head_size) {
  const int heads = a.kv_heads * a.kv_mul, maxqt = head_size == 128 ? 2 : 4;
  const char* e = khm::dbg("KH_PG_ATTN_QT");
  const int forced = e ? atoi(e) : 0;
  if (forced == 1 || forced == 2 || forced == 4) return forced < maxqt ? forced : maxqt;
  if (a.pos0 < 2048) return 1;
  int qt = 1;
  while (qt < maxqt && heads * ((a.T + 32 * qt - 1) / (32 * qt)) >= 256) qt *= 2;
  return qt;
}
static inline void launch_pg_attn(const KhPgAttnArgs& a, int head_size, hipStream_t s) {
  const int qt = pg_attn_qt(a, head_size);
  const int grid = a.kv_heads * a.kv_mul * ((a.T + 16 * qt - 1) / (16 * qt));
  // 8 waves (two per SIMD: one wave's softmax fills the other's MFMA shadow) where the registers
  // allow it; head size 128 keeps 4
#define KH_PA_GO(HB, NW, QT)                                                          \
  do {                                                                                \
    khm::launch_log("k_pg_attn<" #HB "," #NW "," #QT ">");                            \
    hipLaunchKernelGGL((k_pg_attn<HB, NW, QT>), dim3(grid), dim3(64 * NW), 0, s, a);  \
  } while (0)
  switch (head_size) {
    case 48: if (qt == 4) KH_PA_GO(3, 8, 4); else if (qt == 2) KH_PA_GO(3, 8, 2); else KH_PA_GO(3, 8, 1); break;
    case 64: if (qt == 4) KH_PA_GO(4, 8, 4); else if (qt == 2) KH_PA_GO(4, 8, 2); else KH_PA_GO(4, 8, 1); break;
    case 128: if (qt >= 2) KH_PA_GO(8, 4, 2); else KH_PA_GO(8, 4, 1); break;
    default: break;
  }
#undef KH_PA_GO
}
