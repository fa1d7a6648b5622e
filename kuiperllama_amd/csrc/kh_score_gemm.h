// kh_score_gemm.h — sequence scoring on the matrix cores: the classifier GEMM with the log-softmax in its epilogue
// (kh_model_score_gemm, kh_cls_logprobs_f32).  No logits row ever reaches memory.
//
// kh_model_score (kh_prefill.h: k_pf_cls, kh_logprobs.h: k_score_lp) is the bit-exact VALU pass, 8 or 4 tokens per sweep
// of the weights; its classifier writes the logits of a pass and k_score_lp reads them back.  A 512-token GEMM pass on
// a 128 256-word vocabulary would make 262 MB of logits per pass - as much traffic again, both ways, as the classifier
// matrix itself - and a scorer needs none of them: per token the log-sum-exp, the logit of the token that followed and
// the top-N.  The reference has neither call (it computes the logits of one position per forward pass, llama3.cpp:738).
//
//   k_pg_cls_lse    C[vocab rows, T] = Wcls . Xn^T on v_mfma_f32_16x16x4_f32 with kh_gemm.h's operand arrangement and
//                   rings (pg_kloop_f32 / pg_kloop_f32_ring / pg_kloop_q8, the activation slab tiled as k_pg_rmsnorm
//                   leaves it).  A workgroup = 4 waves = KH_CL_ROWS (128) vocabulary rows x one slice of 16 NT tokens
//                   (NT = 4 up to 64 tokens, else 8); every wave owns two 16-row tiles over the WHOLE K, so no partial
//                   sum crosses a wave and the accumulators stay in registers to the end.  blockIdx.x = vocabulary
//                   block * slices + slice: the slices of one block are neighbours in launch order, so that they can
//                   share its rows in L2 (the intent; no counter run has shown it).
//                   Epilogue, per token column (lane (j, hq) holds rows 4 hq .. 4 hq + 3 of both tiles for token j):
//                     max       8 values in the lane, v_permlane16/32_swap across the four lane groups, LDS across the
//                               four waves;
//                     sum       expf(l - max) pairwise in the lane (depth 3), the same two swaps, ((w0 + w1) + (w2 + w3));
//                     target    the one lane that holds row target[tok] stores its logit;
//                     top-N     top_n rounds of "the first element behind the last one taken" in the order (value
//                               descending, id ascending): 8 compares in the lane, two swaps, one LDS exchange and ONE
//                               barrier per round (two exchange buffers by round parity).  Nothing is sorted, nothing
//                               is removed: a round only remembers the (value, id) it took.  top_n = 0 runs no round.
//                   One record per (vocabulary block, token) goes to the workspace: {max, sum, target logit, -,
//                   (value, id) x top_n}, KH_CL_STRIDE words apart.  A tile past the vocabulary's end (vocab % 128 != 0)
//                   loads the last tile's rows and is never counted.
//   k_pg_lse_merge  one workgroup of 256 threads per token folds the blocks' records: thread t owns blocks t, t + 256, ..
//                   in ascending order - maximum, then sum_b exp(max_b - max) in fp32, joined by the xor butterfly and
//                   ((w0 + w1) + (w2 + w3)) -, lse = max + log(sum), lp = target logit - lse, and the same rounds over
//                   the blocks' lists (each is sorted, so a block's candidate is the first entry behind the last one
//                   taken).  It writes the record of the token's cache row in exactly k_score_lp's layout (KhTailRecs,
//                   "none" from top_n on), or an operator's plain arrays.
// Numerics: the logits are kh_model_prefill_gemm's (a k-ordered fmaf chain per row, NOT the decode classifier's order),
// so the records are not bit-identical to kh_model_score's; the ids are exact on the pass's own logits (the order
// involves no arithmetic), lse and lp carry expf, logf and at most 3 + 2 + 2 + ceil(blocks / 256) + 6 + 2 fp32 adds per
// term and one multiply by exp(max_b - max).
// The epilogue is kh_score_gemm_epilogue.h, text included at the end of the kernel body: k_pg_cls_lse_w16
// (kh_score_gemm_w16.h) ends in the same text.  That kernel is the classifier on the bf16 matrix cores from the
// bf16-format 16-bit copy, which score_gemm_tail takes where KH_FLAG_GEMM16 adopted the cls class (not by default) and
// kh_cls_logprobs_w16_f32 always.  Outside both files: the fp16-format copy, the 4-bit copy and the int8 image on the
// bf16 matrix cores - there the classifier reads the fp32 or int8 image.
// No scratch, no inline assembly; every result is written with plain C++ stores.  gfx950 only.
#pragma once
#include "kh_gemm.h"
#include "kh_step_tail.h"

#define KH_CL_WAVES 4
#define KH_CL_R 2
#define KH_CL_ROWS (KH_CL_WAVES * KH_CL_R * 16)  // vocabulary rows per workgroup
#define KH_CL_HDR 4                              // max, sum, target logit, (unused)
#define KH_CL_STRIDE (KH_CL_HDR + 2 * KH_LOGPROBS_MAX_TOP)  // words between two records
#define KH_CL_MERGE_WG 256
#define KH_CL_NO_ID 0x7fffffff  // a list entry that holds no row

static inline int cl_blocks(int vocab) { return (vocab + KH_CL_ROWS - 1) / KH_CL_ROWS; }
static inline int cl_nt(int T) { return T > 64 ? 8 : 4; }
static inline int cl_slices(int T) { return ((T + 15) / 16 + cl_nt(T) - 1) / cl_nt(T); }

struct KhClsLseArgs {
  KhLin w;                // the classifier [vocab][K], fp32 or int8 group 64
  const float* B;         // tiled slab (pg_tiled_index) of tcap >= 16 NT slices token rows, rows >= T finite
  int vocab, K, T, tcap, slices;
  const int32_t* target;  // [T] device; outside [0, vocab): none
  int top_n;              // 0 .. min(KH_LOGPROBS_MAX_TOP, vocab)
  float* ws;              // [blocks][ws_tokens][KH_CL_STRIDE]
  int ws_tokens;
};

// (value descending, id ascending): is a ahead of b?
__device__ __forceinline__ bool cl_ahead(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
// the better of the lane's pair and that of the lanes 16 and 32 further on: every lane of a column ends with the same
template <bool HALVES>
__device__ __forceinline__ void cl_best_swap(float& v, int& id) {
  const int vi = __builtin_bit_cast(int, v);
  const auto rv = HALVES ? __builtin_amdgcn_permlane32_swap(vi, vi, false, false)
                         : __builtin_amdgcn_permlane16_swap(vi, vi, false, false);
  const auto ri = HALVES ? __builtin_amdgcn_permlane32_swap(id, id, false, false)
                         : __builtin_amdgcn_permlane16_swap(id, id, false, false);
  const float v0 = __builtin_bit_cast(float, (int)rv[0]), v1 = __builtin_bit_cast(float, (int)rv[1]);
  const int i0 = (int)ri[0], i1 = (int)ri[1];
  const bool first = cl_ahead(v0, i0, v1, i1);
  v = first ? v0 : v1;
  id = first ? i0 : i1;
}

template <bool QUANT, int NT>
__global__ __launch_bounds__(KH_CL_WAVES * 64) void k_pg_cls_lse(const KhClsLseArgs a) {
  constexpr int R = KH_CL_R, TW = 16 * NT;
  __shared__ float s_red[2][KH_CL_WAVES][TW];  // [0] maxima, [1] sums
  __shared__ float s_cv[2][KH_CL_WAVES][TW];   // the waves' candidates of a round, by round parity
  __shared__ int s_ci[2][KH_CL_WAVES][TW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, h = lane >> 4;
  const int blk = (int)blockIdx.x / a.slices, slice = (int)blockIdx.x - blk * a.slices;
  const int tok0 = slice * TW;
  const int K = a.K;
  int trow[R];
  bool valid[R];  // wave-uniform
#pragma unroll
  for (int r = 0; r < R; ++r) {
    trow[r] = blk * KH_CL_ROWS + (wave * R + r) * 16;
    valid[r] = trow[r] < a.vocab;
  }
  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (!QUANT) {
    const int nb = K >> 4;
    const float* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      wrow[r] = (const float*)a.w.w + (size_t)((valid[r] ? trow[r] : a.vocab - 16) + i) * K + 4 * h;
    const PgBAddr B{a.B + (size_t)(tok0 + i) * 16 + 4 * h, 256, (size_t)a.tcap * 16, 0};
    constexpr int RING_D = R * NT <= 8 ? 8 : KH_PG_RING_D16;  // k_pg_gemm's choice of loop
    if constexpr (RING_D > 0) {
      if (nb >= 2 * RING_D && nb % RING_D == 0)
        pg_kloop_f32_ring<R, NT, RING_D>(wrow, B, 0, nb, acc);
      else
        pg_kloop_f32<R, NT>(wrow, B, 0, nb, acc);
    } else {
      pg_kloop_f32<R, NT>(wrow, B, 0, nb, acc);
    }
  } else {
    const int nb = K >> 6;
    const int8_t* wrow[R];
    const float* srow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const size_t row = (size_t)((valid[r] ? trow[r] : a.vocab - 16) + i);
      wrow[r] = (const int8_t*)a.w.w + row * K + 16 * h;
      srow[r] = a.w.scales + row * nb;
    }
    const PgBAddr B{a.B + (size_t)(tok0 + i) * 16 + 4 * h, 256, (size_t)4 * a.tcap * 16, (size_t)a.tcap * 16};
    pg_kloop_q8<R, NT>(wrow, srow, B, 0, nb, acc);
  }
#include "kh_score_gemm_epilogue.h"
}

struct KhLseMergeArgs {
  const float* ws;        // k_pg_cls_lse's records
  int ws_tokens, nblk, vocab, top_n;
  const int32_t* target;  // [gridDim.x] device, as k_pg_cls_lse's
  int rec0, rec_cap;      // token t writes record rec0 + t < rec_cap
  int top_stride;         // entries per record of top_ids / top_lp; [top_n, top_stride) become "none"
  KhTailRecs recs;        // any pointer may be null
  float* o_lse;           // operator only, [rec_cap], may be null: lse, the maximum, the target's logit
  float* o_max;
  float* o_tlogit;
};
static __global__ __launch_bounds__(KH_CL_MERGE_WG) void k_pg_lse_merge(const KhLseMergeArgs a) {
  constexpr int NW = KH_CL_MERGE_WG / 64;
  __shared__ float s_f[2][NW];
  __shared__ float s_v[2][NW];
  __shared__ int s_i[2][NW];
  const int tok = blockIdx.x, rec = a.rec0 + tok;
  if (rec < 0 || rec >= a.rec_cap) return;  // uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = a.ws + (size_t)tok * KH_CL_STRIDE;
  const size_t bs = (size_t)a.ws_tokens * KH_CL_STRIDE;
  float m = -INFINITY;
  for (int b = tid; b < a.nblk; b += KH_CL_MERGE_WG) m = fmaxf(m, base[b * bs]);
  m = group_max<64>(m);
  if (lane == 0) s_f[0][wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_f[0][0], s_f[0][1]), fmaxf(s_f[0][2], s_f[0][3]));
  float z = 0.f;
  for (int b = tid; b < a.nblk; b += KH_CL_MERGE_WG) {
    const float mb = base[b * bs];
    if (mb > -INFINITY) z += base[b * bs + 1] * expf(mb - m);
  }
  z = group_sum<64>(z);
  if (lane == 0) s_f[1][wave] = z;
  __syncthreads();
  z = (s_f[1][0] + s_f[1][1]) + (s_f[1][2] + s_f[1][3]);
  const float lse = __fadd_rn(m, logf(z));
  const int tgt = a.target ? a.target[tok] : -1;
  if (tid == 0) {
    const bool has = (unsigned)tgt < (unsigned)a.vocab;
    const float tl = has ? base[(size_t)(tgt / KH_CL_ROWS) * bs + 2] : __uint_as_float(0x7fc00000u);
    if (a.recs.token) a.recs.token[rec] = tgt;
    if (a.recs.lp) a.recs.lp[rec] = has ? __fsub_rn(tl, lse) : __uint_as_float(0x7fc00000u);
    if (a.o_lse) a.o_lse[rec] = lse;
    if (a.o_max) a.o_max[rec] = m;
    if (a.o_tlogit) a.o_tlogit[rec] = tl;
  }
  if (!a.recs.top_ids && !a.recs.top_lp) return;  // uniform
  const size_t r0 = (size_t)rec * a.top_stride;
  if (tid >= a.top_n && tid < a.top_stride) {  // "none" behind the list (kh_rec_none)
    if (a.recs.top_ids) a.recs.top_ids[r0 + tid] = -1;
    if (a.recs.top_lp) a.recs.top_lp[r0 + tid] = __uint_as_float(0xffffffffu);
  }
  float lv = INFINITY;
  int li = -1;
  for (int k = 0; k < a.top_n; ++k) {
    const int par = k & 1;
    float bv = -INFINITY;
    int bi = KH_CL_NO_ID;
    for (int b = tid; b < a.nblk; b += KH_CL_MERGE_WG) {
      const float* e = base + b * bs + KH_CL_HDR;
      for (int j = 0; j < a.top_n; ++j) {  // a sorted list: its first entry behind the last one taken is its best
        const float v = e[2 * j];
        const int id = __float_as_int(e[2 * j + 1]);
        if (id == KH_CL_NO_ID) break;
        if (cl_ahead(lv, li, v, id)) {
          if (cl_ahead(v, id, bv, bi)) {
            bv = v;
            bi = id;
          }
          break;
        }
      }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float v = __shfl_xor(bv, off, 64);
      const int id = __shfl_xor(bi, off, 64);
      if (cl_ahead(v, id, bv, bi)) {
        bv = v;
        bi = id;
      }
    }
    if (lane == 0) {
      s_v[par][wave] = bv;
      s_i[par][wave] = bi;
    }
    __syncthreads();
    bv = s_v[par][0];
    bi = s_i[par][0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
      if (cl_ahead(s_v[par][w], s_i[par][w], bv, bi)) {
        bv = s_v[par][w];
        bi = s_i[par][w];
      }
    lv = bv;
    li = bi;
    if (tid == 0) {
      const bool none = bi == KH_CL_NO_ID;  // (top_n <= vocab: never)
      if (a.recs.top_ids) a.recs.top_ids[r0 + k] = none ? -1 : bi;
      if (a.recs.top_lp) a.recs.top_lp[r0 + k] = none ? __uint_as_float(0xffffffffu) : __fsub_rn(bv, lse);
    }
  }
}

// the operator's activations: row-major X[T][K] as the tiled slab k_pg_cls_lse reads, rows T .. tcap zero
static __global__ __launch_bounds__(KH_WG) void k_cls_pack(const float* __restrict__ X, float* __restrict__ slab, int T,
                                                           int K, int tcap) {
  const int t = blockIdx.x;
  for (int k = threadIdx.x; k < K; k += KH_WG)
    slab[pg_tiled_index(false, k, t, tcap)] = t < T ? X[(size_t)t * K + k] : 0.f;
}
