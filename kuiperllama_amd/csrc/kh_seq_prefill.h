// kh_seq_prefill.h — the MFMA prompt prefill into sequence slots (kh_model_seq_prefill_gemm): prompt segments of
// SEVERAL slots packed into one GEMM pass of up to KH_PG_TMAX = 512 tokens.  kh_model_prefill_gemm (kh_gemm.h,
// kh_pattn.h) fills rows pos0 + t of the batch-1 layout only; kh_model_seq_prefill is the bit-exact VALU pass, 8 (fp32)
// or 4 (int8) tokens per sweep of the weights.  The reference feeds a prompt one token per forward pass
// (demo/main.cpp:20-22) and knows one sequence per process.
//
// A pass holds up to KH_RG_TILES = 32 TOKEN TILES of 16 slab tokens.  A tile belongs to exactly one segment - a run of
// consecutive positions of one slot; a segment of n tokens takes ceil(n / 16) tiles, and the 1 .. 15 padding tokens of
// its last tile REPEAT THE TILE'S LAST VALID TOKEN: same token id, same position, same cache row.  This is the padding
// idiom of the 8-lane and wide passes (kh_seq.h, kh_seq_gemm.h): every slab column is defined and finite, a padding
// column computes the bits of the column it repeats in every launch of every layer, so its duplicate K/V store writes
// identical bits to the same address, and kh_gemm_body.h needs no "valid" test.  T of a pass = 16 x its tiles.
//   k_rg_gemm     k_pg_gemm's statements (kh_gemm_body.h) under the tile address - the QKV epilogue only
//   k_rg_rope     k_pg_rope over the tile table, for the shapes whose epilogue cannot rotate
//   k_rg_attn     k_pg_attn's statements (kh_pattn_body.h) with one query tile per workgroup: position, valid count, row
//                 base and shared prefix of the tile from the table (the row translation of k_seq_attn_pfx)
// wo, the SwiGLU pair, w2 and the RMSNorm are k_pg_gemm and k_pg_rmsnorm themselves: they do not care where a token
// sits.  Numerics: kh_model_prefill_gemm's contract, and its very arithmetic per slab column.
// gfx950 only.
#pragma once
#include "kh_gemm.h"
#include "kh_pattn.h"

#include "kh_seq_plan.h"  // KH_RG_TILES, kh_rg_plan

static_assert(KH_RG_TILES * 16 == KH_PG_TMAX, "a pass of full tiles is one chunk of the GEMM prefill");

// Tile k of a pass: slab tokens 16 k .. 16 k + 15 are positions pos0[k] .. pos0[k] + nvalid[k] - 1 of a slot whose
// position p >= its shared length lives at cache row base[k] + p (kh_seq_own_base: negative for a sharer near the start
// of the cache); the attention alone reads positions [0, pfx_len[k]) from rows pfx_row0[k] .. of the slot's parent.
// By value, as KhWideLanes.
struct KhRgTiles {
  int32_t pos0[KH_RG_TILES], nvalid[KH_RG_TILES], base[KH_RG_TILES];
  int32_t pfx_len[KH_RG_TILES], pfx_row0[KH_RG_TILES];
};
static_assert(sizeof(KhPgGemmArgs) + sizeof(KhRgTiles) <= 4096, "kernel arguments");

struct RgTileAddr {
  const KhRgTiles& t;
  __device__ __forceinline__ int pos(int tok) const {
    const int k = tok >> 4, i = tok & 15, nv = t.nvalid[k];
    return t.pos0[k] + (i < nv ? i : nv - 1);
  }
  __device__ __forceinline__ int row(int tok) const { return t.base[tok >> 4] + pos(tok); }
};
// k_pg_gemm's launch geometry; a.T = 16 x tiles of the pass (the epilogue reads the table at tok < a.T only)
template <bool QUANT, int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX(QUANT)) void k_rg_gemm(const KhPgGemmArgs a, const KhRgTiles tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  static_assert(EPI == KH_PG_QKV, "the other GEMMs of the pass are k_pg_gemm's");
  constexpr bool KH_GEMM_W16 = false, KH_GEMM_Q16 = false;
  const RgTileAddr addr{tiles};
#include "kh_gemm_body.h"
}

// RoPE of the pass's query rows and fresh key rows, in place: k_pg_rope with the tile's position and cache row.  A
// padding token returns at entry: its key row is the one the valid token it repeats rotates - a repeated row must not
// be rotated twice - and its own query row is read by nobody (RgAttnAddr::col takes a padding column's query from the
// slab row of the token it repeats).  blockIdx.x = slab token.
static __global__ __launch_bounds__(KH_WG) void k_rg_rope(float* __restrict__ Q, float* __restrict__ kc,
                                                          const float* __restrict__ sin_cache,
                                                          const float* __restrict__ cos_cache, int dim, int kv_dim,
                                                          int hs, const KhRgTiles tiles, int mode) {
  const int t = blockIdx.x, tk = t >> 4, i = t & 15;
  if (i >= tiles.nvalid[tk]) return;
  const int pos = tiles.pos0[tk] + i;
  pg_rope_token(Q + (size_t)t * dim, kc + (size_t)(tiles.base[tk] + pos) * kv_dim, sin_cache + (size_t)pos * hs,
                cos_cache + (size_t)pos * hs, dim, kv_dim, hs, mode);
}

// Query columns by tile (QT = 1: a workgroup's columns are one tile, of one slot).  Every column's output is kept: a
// padding column is the twin of the one it repeats in the slab the wo GEMM reads.
struct RgAttnAddr {
  const KhRgTiles& t;
  int T;
  __device__ __forceinline__ int tiles(int) const { return T >> 4; }
  __device__ __forceinline__ int last_pos(int t0, int) const { return t.pos0[t0 >> 4] + t.nvalid[t0 >> 4] - 1; }
  __device__ __forceinline__ int off(int tok) const {
    const int i = tok & 15, nv = t.nvalid[tok >> 4];
    return i < nv ? i : nv - 1;
  }
  __device__ __forceinline__ int col(int tok) const { return (tok & ~15) + off(tok); }
  __device__ __forceinline__ int pos(int tok) const { return t.pos0[tok >> 4] + off(tok); }
  __device__ __forceinline__ int tile_pos0(int tok) const { return t.pos0[tok >> 4]; }
  // k_seq_attn_pfx's translation: timesteps below the shared length are the parent's rows
  __device__ __forceinline__ int row(int t0, int p) const {
    const int k = t0 >> 4;
    return p < t.pfx_len[k] ? t.pfx_row0[k] + p : t.base[k] + p;
  }
  __device__ __forceinline__ bool stores(int) const { return true; }
};
// k_pg_attn's launch geometry at QT = 1: heads x (a.T / 16) workgroups of 64 NW threads; a.pos0 is not read.
// The 8-wave forms ask for four waves per SIMD (two workgroups per CU), as k_pg_attn<HB, 8, 1> has at its 128 VGPRs:
// the table look-ups cost two registers more, and 130 leave one workgroup per CU (measured without the bound: 27.5
// against k_pg_attn's 21.2 us per layer on Llama-3.2-1B at 512 tokens).
template <int HB /* head_size / 16 */, int NW /* waves that split the timesteps, as k_pg_attn's for the head size */>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 4 : 1) void k_rg_attn(const KhPgAttnArgs a, const KhRgTiles tiles) {
  constexpr int QT = 1;
  const RgAttnAddr addr{tiles, a.T};
#include "kh_pattn_body.h"
}
