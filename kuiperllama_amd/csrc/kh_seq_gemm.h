// kh_seq_gemm.h — the wide sequence pass: up to KH_SEQ_SLOTS_MAX = 64 lanes of DIFFERENT sequences at unrelated
// positions share one sweep of the weights, with the four weight GEMMs and the classifier on the matrix cores
// (kh_model_seq_step_gemm, kh_model_generate_batch_gemm).  The 8-lane pass of kh_seq.h runs its matrices on the VALU
// and is bound by LDS reads and FMAs at 8 lanes; here the lanes sit on the MFMA N dimension of
// kh_gemm.h's GEMM, whose text this header instantiates unchanged under a lane address.  The reference decodes one
// sequence per process (demo/main.cpp:16-50).
//   k_sg_embed    k_seq_embed over the wide table: lane b gathers row tok[slot[b]] into X[b]
//   k_sg_gemm     k_pg_gemm's statements (kh_gemm_body.h) with "RoPE row pos[tok], cache row row[tok]" - the QKV epilogue
//                 on lanes - and the epilogue KH_PG_STORE (row-major logits rows) for the classifier
//   k_sg_rope     k_pg_rope over the lane table, for the shapes whose epilogue cannot rotate
// Attention and the tail are the 8-lane pass's own launches, once per group of KH_PF_BMAX lanes.
// Numerics: kh_model_prefill_gemm's contract - fp32 round-off from another summation order than the decode GEMVs.
// gfx950 only.
#pragma once
#include "kh_gemm.h"
#include "kh_seq_plan.h"  // KH_SEQ_SLOTS_MAX

// Lane b: a token at position pos[b] of the sequence in slot slot[b], cache row row[b].  By value; the host fills the
// padding lanes with the last valid lane's entries, as the 8-lane table's.
struct KhWideLanes {
  int32_t pos[KH_SEQ_SLOTS_MAX], row[KH_SEQ_SLOTS_MAX], slot[KH_SEQ_SLOTS_MAX];
};
static_assert(sizeof(KhPgGemmArgs) + sizeof(KhWideLanes) <= 4096, "kernel arguments");

struct SgLaneAddr {
  const KhWideLanes& l;
  __device__ __forceinline__ int pos(int tok) const { return l.pos[tok]; }
  __device__ __forceinline__ int row(int tok) const { return l.row[tok]; }
};
// k_pg_gemm's launch geometry; a.T <= KH_SEQ_SLOTS_MAX (the epilogue reads the table at tok < a.T only)
template <bool QUANT, int R, int NT, int EPI>
__global__ __launch_bounds__(KH_PG_WG_MAX(QUANT)) void k_sg_gemm(const KhPgGemmArgs a, const KhWideLanes lanes) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr bool KH_GEMM_W16 = false, KH_GEMM_Q16 = false;
  const SgLaneAddr addr{lanes};
#include "kh_gemm_body.h"
}

// embedding rows of the lanes' tokens -> X[n][dim], blockIdx.x = lane < n.  A token outside the vocabulary (the pick
// of a row without a maximum) copies nothing, as k_seq_embed.
static __global__ __launch_bounds__(KH_WG) void k_sg_embed(const int32_t* __restrict__ tok, const KhWideLanes lanes,
                                                           int vocab, const float* __restrict__ emb,
                                                           float* __restrict__ X, int dim) {
  const int b = blockIdx.x;
  const int t = tok[lanes.slot[b]];
  if (t < 0 || t >= vocab) return;
  const f32x4* src = (const f32x4*)(emb + (size_t)t * dim);
  f32x4* dst = (f32x4*)(X + (size_t)b * dim);
  for (int i = threadIdx.x; i < (dim >> 2); i += KH_WG) dst[i] = src[i];
}

// RoPE of the lanes' query rows and fresh key rows, in place: k_pg_rope with position pos[b] and cache row row[b].
static __global__ __launch_bounds__(KH_WG) void k_sg_rope(float* __restrict__ Q, float* __restrict__ kc,
                                                          const float* __restrict__ sin_cache,
                                                          const float* __restrict__ cos_cache, int dim, int kv_dim,
                                                          int hs, const KhWideLanes lanes, int mode) {
  const int t = blockIdx.x, pos = lanes.pos[t];
  pg_rope_token(Q + (size_t)t * dim, kc + (size_t)lanes.row[t] * kv_dim, sin_cache + (size_t)pos * hs,
                cos_cache + (size_t)pos * hs, dim, kv_dim, hs, mode);
}
