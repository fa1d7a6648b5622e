// kh_cls_screen.h — exact greedy argmax without streaming the fp32 classifier: a bf16 copy of the classifier
// screens the rows, the few rows that can still be the argmax are re-scored from their fp32 rows.
//
// A greedy step uses one fact about its 128 k logits: which is largest.  k_cls streams vocab x dim fp32 weights to
// find it; here
//
//   k_cls_bf16_build  (model creation) writes the classifier once more as bf16, round to nearest even, and per row
//                     e[r] >= |w_r - bf16(w_r)|_2 + 2 gamma_n (|w_r|_2 + |bf16(w_r)|_2)            (fp64, rounded up)
//   k_cls_screen      (k_cls's slot in the step) streams the bf16 rows - half the bytes - against the same staged
//                     g = w_norm o x and leaves, per workgroup, the best LOWER bound of a logit and its few best
//                     rows by UPPER bound
//   k_sample_screen   (k_sample's slot) merges the partials, re-scores the candidate rows from the fp32 classifier
//                     with k_cls's own per-lane order and reduction (the same device functions: Stager,
//                     Gemv<false, U>::load / fma, wave_sum), and takes the argmax of those exact values; what it
//                     then leaves behind is k_sample's, through the same helpers (kh_step_tail.h).
//
// The interval.  Let g be the staged vector (fp32 words, the same in both kernels), rs the RMS scale, S and A the
// exact sums  sum_i w_i g_i  and  sum_i bf16(w_i) g_i, S32 and A32 what the fp32 kernels accumulate for them.  k_cls
// stores l = fl(rs S32); the screen forms a = fl(rs A32).
//   |S - A|     <= |w - bf16(w)|_2 |g|_2                                          (Cauchy-Schwarz, exact reals)
//   |S32 - S|   <= gamma_n sum_i |w_i g_i| <= gamma_n |w|_2 |g|_2 ,  gamma_n = n u / (1 - n u),  u = 2^-24
//   |A32 - A|   <= gamma_n |bf16(w)|_2 |g|_2
// n is the number of roundings a term passes through: a lane's chain of dim/64 FMAs (both kernels: 64 lanes, one
// FMA per weight) plus six butterfly additions, n = ceil(dim / 64) + 8; e[r] carries 2 gamma_n, twice what the
// analysis needs (at dim 2048 the rounding part is well under 1 % of e; the bf16 part is everything).  So
//   |rs S32 - rs A32| <= rs |g|_2 e[r] .
// What is left is relative to the values themselves: the two multiplications by rs (1 u each), an rs that a launch
// of another workgroup width sums in another order (a few u), |g|_2 formed in fp32 (sum of non-negative terms,
// < 32 u, and one square root), the products and the sums that form b, a - b and a + b.  They are covered by
//   b = fl(rs |g|_2 (1 + 2^-17)) e[r] + |a| 2^-18 + 1e-30
// (64 u on |a| against fewer than 8; 128 u on the main term against fewer than 40; 1e-30 stands for products that
// underflow: dim x 2^-126 x rs stays below 1e-31 for every dim up to 64 k).  Claim: l lies in [a - b, a + b].  A
// row whose a or b is not finite gets (-inf, +inf): always a candidate, never raises the lower bound.
//
// Exactness of the token.  L = max over rows of (a - b) is a lower bound of the largest logit, so a row with
// a + b < L is not the argmax, nor tied with it.  Every other row is re-scored exactly; the argmax over them, ties to
// the lowest index, is the argmax over all rows.  A workgroup hands over its KH_SCR_C best rows by upper bound and
// the largest upper bound it dropped; if a dropped bound reaches L, or more than KH_SCR_CAND rows qualify, the step
// OVERFLOWS: every workgroup of k_sample_screen (one per CU; all but the first leave at once otherwise) then runs
// the full fp32 classifier and the last one to arrive merges - the arithmetic of k_cls + k_sample, inside the same
// launch, no host decision.
//
// The int8 tier ahead of the bf16 screen.  The bf16 pass is at the stream ceiling, so only fewer bytes make the tail
// shorter: an int8 copy with one fp32 scale per KH_SCR8_G = 64 weights is 0.53 of the bf16 copy's bytes.  Its interval
// is 3-4 times wider, too wide to feed k_sample_screen's KH_SCR_CAND rows directly, so it only thins the vocabulary:
//
//   k_cls_q8_build     (model creation) per group G: sc_G = max |w_i| / 127, q_i = rint(w_i / sc_G) clamped to +-127
//                      (an all-zero group, or one with a NaN / Inf weight: sc_G = 0, q = 0), and per row
//                      e8[r] >= |w_r - sc o q_r|_2 + 2 gamma_n (|w_r|_2 + |sc o q_r|_2)               (fp64, rounded up)
//                      with e8[r] = +inf for a row that holds a NaN or an Inf
//   k_cls_screen_q8    (first launch of the tail) streams q and sc against g staged in the int8 kernels' four-plane
//                      layout and leaves, per workgroup, the best lower bound, its KH_SCR8_C best rows by upper bound
//                      and the largest upper bound it dropped.  No logits, no x_save.
//   k_cls_screen       (survivor mode: KhClsScreenArgs::q_lb set) reads those partials: L8 = max lower bound, S8 = max
//                      dropped bound.  S8 >= L8: tier 1 spilled, every workgroup runs the full bf16 scan as if there
//                      were no tier 1.  Otherwise workgroup b re-screens the slots b, b + grid, ... of tier 1's partials
//                      whose upper bound reaches L8 (neighbouring slots - the rows of one tier-1 workgroup - go to
//                      different workgroups: each hands on KH_SCR_C rows, a tier-1 workgroup twice as many) - one wave
//                      per row, the row's chunks in gemv_pairs' order, so the interval is the full scan's bit for bit -
//                      and hands over the usual partials.
//
// Its interval.  A = sum_G sc_G sum_{i in G} q_i g_i in exact reals; A32 what the kernel accumulates: a lane owns 16
// consecutive weights of one group per load, t = a chain of 16 FMAs q_i g_i from 0 (q_i exact in fp32), then
// a = fma(sc_G, t, a) along the lane's ceil(dim / 1024) loads, then the six butterfly additions.
//   |S - A|     <= |w - sc o q|_2 |g|_2                                          (Cauchy-Schwarz, exact reals)
//   |A32 - A|   <= gamma_n8 sum |sc q_i g_i| <= gamma_n8 |sc o q|_2 |g|_2 ,  n8 = 16 + 1 + ceil(dim / 1024) + 6
//   |S32 - S|   <= gamma_n' |w|_2 |g|_2 ,                                     n' = ceil(dim / 64) + 8  (k_cls, above)
// e8[r] carries 2 gamma_n for both with the one n = ceil(dim / 64) + 24 >= max(n8, n') (at dim 2048 the rounding
// part is 2e-3 of e8; the quantisation part is everything).  So |rs S32 - rs A32| <= rs |g|_2 e8[r], and with
// a8 = fl(rs A32) the terms relative to the values are the bf16 interval's, covered by the same slack:
//   b8 = fl(rs |g|_2 (1 + 2^-17)) e8[r] + |a8| 2^-18 + 1e-30 ,     l in [a8 - b8, a8 + b8].
// (rs and |g|_2 are formed as in the bf16 kernel, thread for thread; a launch of another workgroup width sums them in
// another order: a few u, inside the 128 u of the main term.)  A row whose a8 or b8 is not finite gets (-inf, +inf).
// Exactness.  L8 = max (a8 - b8) is a lower bound of the largest logit: a row with a8 + b8 < L8 is neither the argmax
// nor tied with it.  The bf16 screen of the remaining rows is the screen above on a smaller vocabulary that still
// holds every row that can win: its L is a lower bound of the largest logit, its candidates hold the argmax.
// Which workgroup re-screens which slot is a function of the slot's position alone: no scheduling order enters.
// The survivor pass could raise its lower bounds to L8 and does not: the row that sets L8 is a survivor itself, and
// its bf16 half-width is about a quarter of its int8 one, so L would hardly ever move; k_sample_screen sees the
// partials it always saw.
//
// Replaces nothing in the reference (it streams the fp32 classifier and runs an argmax kernel,
// kuiper/source/model/llama3.cpp:722-745).
#pragma once
#include "kh_fused.h"

#define KH_SCR_C 4      // rows a workgroup of k_cls_screen hands over
#define KH_SCR_CAND 32  // rows k_sample_screen re-scores before the step counts as an overflow
#define KH_SCR_MERGE_WORDS (2 + 2 * KH_SCR_C)
#define KH_SCR8_C 8     // rows a workgroup of k_cls_screen_q8 hands over
#define KH_SCR8_G 64    // weights per scale of the int8 copy
#define KH_SCR8_GSHIFT 6
#define KH_SCR8_MERGE_WORDS (2 + 2 * KH_SCR8_C)

// LDS layout of the staged vector for the bf16 rows: a lane owns 8 consecutive weights (one dwordx4), i.e. the
// float4 f = 2j and 2j + 1 of its 8-chunk j.  Two planes, slot(f) = (f & 1) * (M8 + 1) + (f >> 1): for either half
// consecutive lanes read consecutive 16-byte slots (the int8 kernels' q8_slot with two planes instead of four).
__device__ __forceinline__ int bf_slot(int f, int M8) { return (f & 1) * (M8 + 1) + (f >> 1); }
static inline size_t kh_bf_lds_bytes(int M) { return (size_t)2 * (size_t)(M / 8 + 1) * 16; }
// xs (two planes) | ss[KH_WAVES_MAX] | gg[KH_WAVES_MAX] | per-wave partials
static inline size_t cls_screen_lds_bytes(int M) {
  return kh_bf_lds_bytes(M) + (size_t)(2 * KH_WAVES_MAX + KH_WAVES_MAX * KH_SCR_MERGE_WORDS) * sizeof(float);
}

__device__ __forceinline__ float bf_lo(int d) { return __builtin_bit_cast(float, d << 16); }
__device__ __forceinline__ float bf_hi(int d) { return __builtin_bit_cast(float, d & (int)0xffff0000u); }
// 8 packed bf16 (one dwordx4, element 2k in the low half of dword k) . 8 floats
__device__ __forceinline__ float dot8_bf16(i32x4 q, f32x4 xa, f32x4 xb, float acc) {
  acc = __builtin_fmaf(bf_lo(q.x), xa.x, acc);
  acc = __builtin_fmaf(bf_hi(q.x), xa.y, acc);
  acc = __builtin_fmaf(bf_lo(q.y), xa.z, acc);
  acc = __builtin_fmaf(bf_hi(q.y), xa.w, acc);
  acc = __builtin_fmaf(bf_lo(q.z), xb.x, acc);
  acc = __builtin_fmaf(bf_hi(q.z), xb.y, acc);
  acc = __builtin_fmaf(bf_lo(q.w), xb.z, acc);
  acc = __builtin_fmaf(bf_hi(q.w), xb.w, acc);
  return acc;
}

// The matrix view gemv_pairs needs (kh_gemv.h: kU, Regs, Rows, Mc, load, fma), over bf16 rows of M weights.
template <int U>
struct RegsBf16 {
  i32x4 v0[U], v1[U];
};
struct RowsBf16 {
  const i32x4* w0;
  const i32x4* w1;
};
template <int U>
struct GemvBf16 {
  static constexpr int kU = U;
  using Regs = RegsBf16<U>;
  using Rows = RowsBf16;
  int Mc;  // 16-byte units per row: M / 8
  __device__ __forceinline__ explicit GemvBf16(int M) : Mc(M >> 3) {}
  __device__ __forceinline__ Rows rows(const uint16_t* base, int r0, int r1, int M) const {
    return Rows{(const i32x4*)(base + (size_t)r0 * M), (const i32x4*)(base + (size_t)r1 * M)};
  }
  __device__ __forceinline__ void load(Regs& r, const Rows& rw, int c0, int lim, int lane) const {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = c0 + u * KH_WAVE + lane;
      const int cidx = idx < lim ? idx : 0;  // clamped address; masked in fma (kh_gemv.h::fma_u)
      r.v0[u] = ld_nt(rw.w0 + cidx);
      r.v1[u] = ld_nt(rw.w1 + cidx);
      __builtin_amdgcn_sched_barrier(0);  // slots stay in issue order (kh_gemv.h::load_u)
    }
  }
  __device__ __forceinline__ void fma(const Regs& r, const f32x4* xs, int c0, int lim, int lane, float& a0,
                                      float& a1) const {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = c0 + u * KH_WAVE + lane;
      const bool in = idx < lim;
      const int ci = in ? idx : 0;
      f32x4 xa = xs[ci], xb = xs[Mc + 1 + ci];
      xa.x = in ? xa.x : 0.f;
      xa.y = in ? xa.y : 0.f;
      xa.z = in ? xa.z : 0.f;
      xa.w = in ? xa.w : 0.f;
      xb.x = in ? xb.x : 0.f;
      xb.y = in ? xb.y : 0.f;
      xb.z = in ? xb.z : 0.f;
      xb.w = in ? xb.w : 0.f;
      a0 = dot8_bf16(r.v0[u], xa, xb, a0);
      a1 = dot8_bf16(r.v1[u], xa, xb, a1);
    }
  }
};

// ---------------------------------------------------------------------------------------------
// Model creation: bf16 copy of the classifier + per-row error norm.  One wave per row, fp64 accumulation.
__device__ __forceinline__ uint32_t bf16_rne(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // NaN stays a (quiet) NaN
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, KH_WAVE);
  return v;
}
// gam2 = 2 gamma_n (see the head of this file).  dim is even (the caller requires a multiple of 8).
static __global__ __launch_bounds__(KH_WG) void k_cls_bf16_build(const float* __restrict__ w, uint32_t* __restrict__ out,
                                                                 float* __restrict__ err, int dim, int vocab,
                                                                 double gam2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = dim >> 1;
  for (int row = blockIdx.x * KH_WAVES_PER_WG + wave; row < vocab; row += gridDim.x * KH_WAVES_PER_WG) {
    const float2* src = (const float2*)(w + (size_t)row * dim);
    uint32_t* dst = out + (size_t)row * half;
    double d2 = 0.0, w2 = 0.0, b2 = 0.0;
    for (int i = lane; i < half; i += KH_WAVE) {
      const float2 v = src[i];
      const uint32_t lo = bf16_rne(v.x), hi = bf16_rne(v.y);
      dst[i] = lo | (hi << 16);
      const float bx = __builtin_bit_cast(float, lo << 16), by = __builtin_bit_cast(float, hi << 16);
      const double ex = (double)v.x - (double)bx, ey = (double)v.y - (double)by;
      d2 += ex * ex + ey * ey;
      w2 += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
      b2 += (double)bx * (double)bx + (double)by * (double)by;
    }
    d2 = wave_sum_f64(d2);
    w2 = wave_sum_f64(w2);
    b2 = wave_sum_f64(b2);
    if (lane == 0) {
      // the fp64 sums carry a relative error below dim x 2^-52: (1 + 1e-9) is far above it
      const double e = (sqrt(d2) + gam2 * (sqrt(w2) + sqrt(b2))) * (1.0 + 1e-9);
      float f = (float)e;
      if ((double)f < e) f = nextafterf(f, INFINITY);
      if (!(e < (double)INFINITY)) f = INFINITY;  // NaN / Inf weights: the row is always a candidate
      err[row] = f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// keep the C largest upper bounds (descending) and the largest one that fell out
template <int C>
struct ScrTopN {
  float lb, spill;
  float u[C];
  int i[C];
  __device__ __forceinline__ void init() {
    lb = -INFINITY;
    spill = -INFINITY;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      u[k] = -INFINITY;
      i[k] = -1;
    }
  }
  __device__ __forceinline__ void insert(float ub, int idx) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const bool sw = ub > u[k];
      const float tu = sw ? u[k] : ub;
      const int ti = sw ? i[k] : idx;
      u[k] = sw ? ub : u[k];
      i[k] = sw ? idx : i[k];
      ub = tu;
      idx = ti;
    }
    spill = fmaxf(spill, idx >= 0 ? ub : -INFINITY);  // an empty slot that fell out is not a row
  }
  // insert() for a bound every lane of the wave holds alike: one that does not beat the last kept bound falls straight
  // out (what the walk above comes to for it), decided by a scalar branch - most rows of a vocabulary take it
  __device__ __forceinline__ void offer(float ub, int idx) {
    if (__builtin_amdgcn_readfirstlane((int)(ub > u[C - 1])))
      insert(ub, idx);
    else
      spill = fmaxf(spill, idx >= 0 ? ub : -INFINITY);
  }
};
using ScrTop = ScrTopN<KH_SCR_C>;

// The end of both screening kernels: the waves' lists merged by thread 0 (mg: nwaves x (2 + 2 C) words of LDS), one
// partial per workgroup.
template <int C>
__device__ __forceinline__ void scr_handover(ScrTopN<C>& top, float* mg, int lane, int wave, float* p_lb, float* p_spill,
                                             float* p_ub, int32_t* p_idx) {
  constexpr int W = 2 + 2 * C;
  if (lane == 0) {
    float* q = mg + wave * W;
    q[0] = top.lb;
    q[1] = top.spill;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      q[2 + k] = top.u[k];
      q[2 + C + k] = __builtin_bit_cast(float, top.i[k]);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1, nw = kh_nwaves(); w < nw; ++w) {
      const float* q = mg + w * W;
      top.lb = fmaxf(top.lb, q[0]);
      top.spill = fmaxf(top.spill, q[1]);
      // a wave's list is in descending order: behind the first bound that falls out, all of them do
      for (int k = 0; k < C; ++k) {
        const float ub = q[2 + k];
        const int idx = __builtin_bit_cast(int, q[2 + C + k]);
        if (!(ub > top.u[C - 1])) {
          top.spill = fmaxf(top.spill, idx >= 0 ? ub : -INFINITY);
          break;
        }
        top.insert(ub, idx);
      }
    }
    p_lb[blockIdx.x] = top.lb;
    p_spill[blockIdx.x] = top.spill;
#pragma unroll
    for (int k = 0; k < C; ++k) {
      p_ub[blockIdx.x * C + k] = top.u[k];
      p_idx[blockIdx.x * C + k] = top.i[k];
    }
  }
}

struct KhClsScreenArgs {
  const float* x;
  const float* final_norm;
  const uint16_t* wbf;  // [vocab, dim] bf16
  const float* err;     // [vocab]
  float* x_save;        // [dim]: the pre-norm input, for logits on demand and for the re-scoring
  float* p_lb;          // [grid]
  float* p_spill;       // [grid]
  float* p_ub;          // [grid, KH_SCR_C]
  int32_t* p_idx;       // [grid, KH_SCR_C], -1 = empty
  float* dbg_lb;        // [vocab] or nullptr: every row's interval (creation-time self-test)
  float* dbg_ub;
  int dim, vocab;
  float eps;
  // survivor mode (q_lb set): the partials of the k_cls_screen_q8 launch in front of this one, nq workgroups of it
  const float* q_lb;
  const float* q_spill;
  const float* q_ub;     // [nq, KH_SCR8_C]
  const int32_t* q_idx;  // [nq, KH_SCR8_C], -1 = empty
  int32_t* q_stats;      // [0] tier-1 steps, [1] rows that survived tier 1, [2] steps in which tier 1 spilled
  int nq;
};
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_cls_screen(const KhClsScreenArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  f32x4* xs = (f32x4*)smem_raw;
  const int dim = a.dim, vocab = a.vocab, M8 = dim >> 3;
  float* red = (float*)(xs + 2 * (M8 + 1));
  float* mg = red + 2 * KH_WAVES_MAX;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint16_t* const wbf = a.wbf;
  const float* const err = a.err;
  float* const dbg_lb = a.dbg_lb;
  float* const dbg_ub = a.dbg_ub;
  float* const x_save = a.x_save;
  const float eps = a.eps;
  const GemvBf16<U> g(dim);
  Stager<true, false, MAXV> st(a.x, a.final_norm, dim);
  ScrTop top;
  top.init();
  auto r1_of = [&](int p) __attribute__((always_inline)) { return 2 * p + 1 < vocab ? 2 * p + 1 : 2 * p; };
  auto pair = [&](int p) __attribute__((always_inline)) { return g.rows(wbf, 2 * p, r1_of(p), dim); };
  struct Aux {
    float e0, e1;
  };
  auto pre = [&](int p) __attribute__((always_inline)) { return Aux{err[2 * p], err[r1_of(p)]}; };
  float rs = 1.f, cb = 0.f;  // RMS scale; rs |g|_2 (1 + 2^-17)
  auto track = [&](float s, float e, int r) __attribute__((always_inline)) {
    const float av = s * rs;
    const float b = __builtin_fmaf(cb, e, fabsf(av) * 0x1p-18f) + 1e-30f;
    const bool ok = fabsf(av) < INFINITY && b < INFINITY;  // false for NaN as well
    const float lb = ok ? av - b : -INFINITY, ub = ok ? av + b : INFINITY;
    top.lb = fmaxf(top.lb, lb);
    top.insert(ub, r);
    if (dbg_lb && lane == 0) {
      dbg_lb[r] = lb;
      dbg_ub[r] = ub;
    }
  };
  // every lane holds the same sums behind the butterfly: the bookkeeping runs unmasked, lane 0 hands it over
  auto epi = [&](int p, float s0, float s1, const Aux& x) __attribute__((always_inline)) {
    const int r0 = 2 * p, r1 = r1_of(p);
    track(s0, x.e0, r0);
    if (r1 != r0) track(s1, x.e1, r1);
  };
  auto finish = [&]() __attribute__((always_inline)) {
    // Stager::finish with the two-plane layout, the sum of g^2 beside the sum of x^2, and the input put aside
    const int M4 = dim >> 2;
    float ss = 0.f, gg = 0.f;
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
      const int i = threadIdx.x + v * kh_wg();
      const bool in = i < M4;
      const float t = fma4(st.xv[v], st.xv[v], 0.f);
      ss += in ? t : 0.f;
      f32x4 gv = st.xv[v];
      gv.x = st.wv[v].x * gv.x;
      gv.y = st.wv[v].y * gv.y;
      gv.z = st.wv[v].z * gv.z;
      gv.w = st.wv[v].w * gv.w;
      const float t2 = fma4(gv, gv, 0.f);
      gg += in ? t2 : 0.f;
      if (in) {
        xs[bf_slot(i, M8)] = gv;
        if (blockIdx.x == 0) ((f32x4*)x_save)[i] = st.xv[v];
      }
    }
    gg = wave_sum(gg);
    if (lane == 0) red[KH_WAVES_MAX + wave] = gg;
    rs = stage_rs(ss, dim, eps, red);  // its barrier publishes xs and both sets of wave sums
    const int n = kh_nwaves();
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < KH_WAVES_MAX; ++w) r += w < n ? red[KH_WAVES_MAX + (w < n ? w : 0)] : 0.f;
    cb = rs * sqrtf(r) * (1.f + 0x1p-17f);
  };
  // survivor mode: what tier 1 left.  Every workgroup comes to the same decision from the same words.
  bool survivors = false;
  float L8 = -INFINITY;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  // Slots of this workgroup: j = b, b + grid, ... of tier 1's nq x KH_SCR8_C slots, so the rows one tier-1 workgroup
  // hands over go to as many workgroups here (each hands on KH_SCR_C rows only); wave w takes its slots w, w + nwaves, ...
  const int mine = a.q_lb ? (a.nq * KH_SCR8_C - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
  auto slot_of = [&](int s) __attribute__((always_inline)) { return (int)blockIdx.x + s * (int)gridDim.x; };
  int r_first = -1;
  float ub_first = -INFINITY;
  if (a.q_lb) {
    // what does not depend on L8 leaves first: the vector and the wave's first slot.  (A spilled step requests the
    // vector once more through gemv_pairs below: its ISSUE stays unconditional, the issue order of the full scan is
    // the one every other step of the kernel has; a spill is rare and the words come from L2.)
    st.issue();
    if (wv < mine) {
      r_first = a.q_idx[slot_of(wv)];
      ub_first = a.q_ub[slot_of(wv)];
    }
    float l = -INFINITY, sp = -INFINITY;
    for (int i = threadIdx.x; i < a.nq; i += kh_wg()) {
      l = fmaxf(l, a.q_lb[i]);
      sp = fmaxf(sp, a.q_spill[i]);
    }
    l = wave_max(l);
    sp = wave_max(sp);
    if (lane == 0) {
      red[wave] = l;
      red[KH_WAVES_MAX + wave] = sp;
    }
    __syncthreads();
    float S8 = -INFINITY;
    const int n = kh_nwaves();
#pragma unroll
    for (int w = 0; w < KH_WAVES_MAX; ++w) {
      L8 = fmaxf(L8, red[w < n ? w : 0]);
      S8 = fmaxf(S8, red[KH_WAVES_MAX + (w < n ? w : 0)]);
    }
    __syncthreads();  // red is the staging's from here on
    survivors = !(S8 >= L8);  // a dropped bound that reaches L8 (or no finite bound at all): the full scan below
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the tier's counters
      atomicAdd(a.q_stats + 0, 1);
      if (!survivors) atomicAdd(a.q_stats + 2, 1);
    }
  }
  if (survivors) {
    // One wave per surviving row, the chunks of the row in gemv_pairs' order (SPLIT 1: c0 = 0, step, ...; a row's sum
    // does not depend on the row it is paired with), the same staging, reduction and interval as the full scan.  The
    // first row's first tile is requested ahead of the staging barrier (row 0 where the wave has nothing to take).
    typename GemvBf16<U>::Regs regs;
    const int step = KH_WAVE * U;
    int r = __builtin_amdgcn_readfirstlane(r_first);
    bool take = r >= 0 && __builtin_amdgcn_readfirstlane((int)(ub_first >= L8));
    r = take ? r : 0;
    RowsBf16 rw = g.rows(wbf, r, r, dim);
    g.load(regs, rw, 0, g.Mc, lane);
    float e_r = err[r];
    finish();
    for (int s = wv; s < mine; s += kh_nwaves()) {
      if (s != wv) {
        r = __builtin_amdgcn_readfirstlane(a.q_idx[slot_of(s)]);
        take = r >= 0 && __builtin_amdgcn_readfirstlane((int)(a.q_ub[slot_of(s)] >= L8));
        if (take) {
          rw = g.rows(wbf, r, r, dim);
          g.load(regs, rw, 0, g.Mc, lane);
          e_r = err[r];
        }
      }
      if (!take) continue;
      float a0 = 0.f, a1 = 0.f;
      for (int c0 = 0;;) {
        g.fma(regs, xs, c0, g.Mc, lane, a0, a1);
        c0 += step;
        if (c0 >= g.Mc) break;
        g.load(regs, rw, c0, g.Mc, lane);
      }
      track(wave_sum(a0), e_r, r);
    }
    if (blockIdx.x == 0) {  // rows that survived tier 1, over all of its workgroups
      int n = 0;
      for (int i = threadIdx.x; i < a.nq * KH_SCR8_C; i += kh_wg()) n += a.q_idx[i] >= 0 && a.q_ub[i] >= L8 ? 1 : 0;
      if (n) atomicAdd(a.q_stats + 1, n);
    }
  } else {
    gemv_pairs<1, /*ROLL=*/false>(g, xs, (vocab + 1) >> 1, lane, nullptr, pair, pre,
                                  [&]() __attribute__((always_inline)) { st.issue(); }, finish, epi);
  }
  // one partial per workgroup
  scr_handover(top, mg, lane, wave, a.p_lb, a.p_spill, a.p_ub, a.p_idx);
}

// ---------------------------------------------------------------------------------------------
// Model creation: the int8 copy (see the head of this file).  One wave per row, a lane converts 4 consecutive weights
// (16 lanes = one group of 64, four groups per pass), fp64 accumulation.  dim is a multiple of 64.
static __global__ __launch_bounds__(KH_WG) void k_cls_q8_build(const float* __restrict__ w, uint32_t* __restrict__ q,
                                                               float* __restrict__ sc, float* __restrict__ err, int dim,
                                                               int vocab, double gam2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gpr = dim >> KH_SCR8_GSHIFT;
  for (int row = blockIdx.x * KH_WAVES_PER_WG + wave; row < vocab; row += gridDim.x * KH_WAVES_PER_WG) {
    const f32x4* src = (const f32x4*)(w + (size_t)row * dim);
    uint32_t* dst = q + (size_t)row * (dim >> 2);
    double d2 = 0.0, w2 = 0.0, q2 = 0.0;
    for (int base = 0; base < dim; base += 4 * KH_WAVE) {
      const int i4 = (base >> 2) + lane;  // float4 index in the row; a group's 16 lanes are inside the row together
      const bool in = i4 < (dim >> 2);
      const f32x4 v = src[in ? i4 : 0];
      const float wv[4] = {v.x, v.y, v.z, v.w};
      float am = fmaxf(fmaxf(fabsf(wv[0]), fabsf(wv[1])), fmaxf(fabsf(wv[2]), fabsf(wv[3])));
      bool bad = !(fabsf(wv[0]) < INFINITY && fabsf(wv[1]) < INFINITY && fabsf(wv[2]) < INFINITY && fabsf(wv[3]) < INFINITY);
      am = group_max<16>(am);  // fmaxf drops a NaN: `bad` carries it
      bad = group_max<16>(bad ? 1.f : 0.f) != 0.f;
      const float s = bad ? 0.f : am / 127.f;
      uint32_t packed = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float t = s > 0.f ? rintf(wv[k] / s) : 0.f;
        t = fminf(fmaxf(t, -127.f), 127.f);
        if (!(t == t)) t = 0.f;
        const int qi = (int)t;
        packed |= (uint32_t)(qi & 0xff) << (8 * k);
        const double dq = (double)s * (double)qi, e = (double)wv[k] - dq;  // fp32 x 8-bit integer: exact in fp64
        if (in) {
          d2 += e * e;
          w2 += (double)wv[k] * (double)wv[k];
          q2 += dq * dq;
        }
      }
      if (in) {
        dst[i4] = packed;
        if ((lane & 15) == 0) sc[(size_t)row * gpr + (i4 >> 4)] = s;
      }
    }
    d2 = wave_sum_f64(d2);
    w2 = wave_sum_f64(w2);
    q2 = wave_sum_f64(q2);
    if (lane == 0) {
      const double e = (sqrt(d2) + gam2 * (sqrt(w2) + sqrt(q2))) * (1.0 + 1e-9);
      float f = (float)e;
      if ((double)f < e) f = nextafterf(f, INFINITY);
      if (!(e < (double)INFINITY)) f = INFINITY;  // NaN / Inf weights: the row always survives
      err[row] = f;
    }
  }
}

// xs (four planes) | ss[KH_WAVES_MAX] | gg[KH_WAVES_MAX] | per-wave partials
static inline size_t cls_screen_q8_lds_bytes(int M) {
  return kh_q8_lds_bytes(M) + (size_t)(2 * KH_WAVES_MAX + KH_WAVES_MAX * KH_SCR8_MERGE_WORDS) * sizeof(float);
}
struct KhClsScreenQ8Args {
  const float* x;
  const float* final_norm;
  const int8_t* q;   // [vocab, dim]
  const float* sc;   // [vocab, dim / KH_SCR8_G]
  const float* e8;   // [vocab]
  float* p_lb;       // [grid]
  float* p_spill;    // [grid]
  float* p_ub;       // [grid, KH_SCR8_C]
  int32_t* p_idx;    // [grid, KH_SCR8_C], -1 = empty
  float* dbg_lb;     // [vocab] or nullptr: every row's interval (self-test, probe)
  float* dbg_ub;
  int dim, vocab;
  float eps;
};
// Tier 1: k_cls_screen over the int8 copy - Gemv<true, U> with one scale per 64 weights as the matrix view, the
// vector staged in its four-plane layout.  Writes neither logits nor x_save.
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_cls_screen_q8(const KhClsScreenQ8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  f32x4* xs = (f32x4*)smem_raw;
  const int dim = a.dim, vocab = a.vocab, M16 = dim >> 4;
  float* red = (float*)(xs + 4 * (M16 + 1));
  float* mg = red + 2 * KH_WAVES_MAX;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* const e8 = a.e8;
  float* const dbg_lb = a.dbg_lb;
  float* const dbg_ub = a.dbg_ub;
  const float eps = a.eps;
  const Gemv<true, U> g(dim, KH_SCR8_GSHIFT);
  Stager<true, true, MAXV> st(a.x, a.final_norm, dim);
  ScrTopN<KH_SCR8_C> top;
  top.init();
  auto r1_of = [&](int p) __attribute__((always_inline)) { return 2 * p + 1 < vocab ? 2 * p + 1 : 2 * p; };
  auto pair = [&](int p) __attribute__((always_inline)) { return g.rows(a.q, 2 * p, a.q, r1_of(p), a.sc, a.sc, dim); };
  struct Aux {
    float e0, e1;
  };
  auto pre = [&](int p) __attribute__((always_inline)) { return Aux{e8[2 * p], e8[r1_of(p)]}; };
  float rs = 1.f, cb = 0.f;  // RMS scale; rs |g|_2 (1 + 2^-17)
  auto track = [&](float s, float e, int r) __attribute__((always_inline)) {
    const float av = s * rs;
    const float b = __builtin_fmaf(cb, e, fabsf(av) * 0x1p-18f) + 1e-30f;
    const bool ok = fabsf(av) < INFINITY && b < INFINITY;  // false for NaN as well
    const float lb = ok ? av - b : -INFINITY, ub = ok ? av + b : INFINITY;
    top.lb = fmaxf(top.lb, lb);
    top.offer(ub, r);
    if (dbg_lb && lane == 0) {
      dbg_lb[r] = lb;
      dbg_ub[r] = ub;
    }
  };
  auto epi = [&](int p, float s0, float s1, const Aux& x) __attribute__((always_inline)) {
    const int r0 = 2 * p, r1 = r1_of(p);
    track(s0, x.e0, r0);
    if (r1 != r0) track(s1, x.e1, r1);
  };
  auto finish = [&]() __attribute__((always_inline)) {
    // k_cls_screen's staging with the four-plane layout; x_save is the bf16 kernel's to write
    const int M4 = dim >> 2;
    float ss = 0.f, gg = 0.f;
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
      const int i = threadIdx.x + v * kh_wg();
      const bool in = i < M4;
      const float t = fma4(st.xv[v], st.xv[v], 0.f);
      ss += in ? t : 0.f;
      f32x4 gv = st.xv[v];
      gv.x = st.wv[v].x * gv.x;
      gv.y = st.wv[v].y * gv.y;
      gv.z = st.wv[v].z * gv.z;
      gv.w = st.wv[v].w * gv.w;
      const float t2 = fma4(gv, gv, 0.f);
      gg += in ? t2 : 0.f;
      if (in) xs[q8_slot(i, M16)] = gv;
    }
    gg = wave_sum(gg);
    if (lane == 0) red[KH_WAVES_MAX + wave] = gg;
    rs = stage_rs(ss, dim, eps, red);  // its barrier publishes xs and both sets of wave sums
    const int n = kh_nwaves();
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < KH_WAVES_MAX; ++w) r += w < n ? red[KH_WAVES_MAX + (w < n ? w : 0)] : 0.f;
    cb = rs * sqrtf(r) * (1.f + 0x1p-17f);
  };
  gemv_pairs<1, /*ROLL=*/false>(g, xs, (vocab + 1) >> 1, lane, nullptr, pair, pre,
                                [&]() __attribute__((always_inline)) { st.issue(); }, finish, epi);
  scr_handover(top, mg, lane, wave, a.p_lb, a.p_spill, a.p_ub, a.p_idx);
}

// ---------------------------------------------------------------------------------------------
struct KhSampleScreenArgs {
  // the screen's partials
  const float* p_lb;
  const float* p_spill;
  const float* p_ub;
  const int32_t* p_idx;
  int nsp;
  // the exact classifier (re-scoring, overflow)
  const float* x_save;
  const float* final_norm;
  const float* wcls;  // fp32 [vocab, dim]
  float eps;
  float* ov_val;      // [gridDim.x] argmax partials of an overflow step
  int32_t* ov_idx;
  uint32_t* ticket;   // 0 between launches
  int32_t* stats;     // [0] steps, [1] candidate rows re-scored, [2] overflow steps
  KhStepState st;     // what the step leaves behind (kh_step_tail.h)
};
// k_sample's last steps on the helpers of kh_step_tail.h: thread 0 holds the argmax and evaluates the forced-token rule
// behind it, commits, and the workgroup (k_cls's width) gathers the row of the token fed next
__device__ __forceinline__ void screen_tail(const KhStepState& st, int idx, int* s_next) {
  if (threadIdx.x == 0) *s_next = kh_step_commit_pick(st, idx);
  __syncthreads();
  kh_embed_gather(st.tok_emb, st.x, st.dim, st.vocab, *s_next, kh_wg());
}
// U, MAXV and the workgroup width are those of the model's k_cls launch: the staging (and with it rs) and the
// per-lane order of a row's sum are then k_cls's, bit for bit.  Dynamic LDS: cls_lds_bytes(false, dim).
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_sample_screen(const KhSampleScreenArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ float s_cv[KH_SCR_CAND];
  __shared__ int s_ci[KH_SCR_CAND];
  __shared__ int s_n, s_last, s_next;
  f32x4* xs = (f32x4*)smem_raw;
  const int dim = a.st.dim, vocab = a.st.vocab;
  float* red = lds_red_ptr<false>(xs, dim);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const float* const wcls = a.wcls;
  const float eps = a.eps;
  // ---- merge the screen's partials: L, the largest dropped bound, the candidate rows (every workgroup: all of
  // them must come to the same decision without talking to each other)
  float l = -INFINITY, sp = -INFINITY;
  for (int i = threadIdx.x; i < a.nsp; i += kh_wg()) {
    l = fmaxf(l, a.p_lb[i]);
    sp = fmaxf(sp, a.p_spill[i]);
  }
  if (threadIdx.x == 0) s_n = 0;
  const float L = block_max(l, red);
  const float S = block_max(sp, red);
  for (int i = threadIdx.x; i < a.nsp * KH_SCR_C; i += kh_wg()) {
    const int idx = a.p_idx[i];
    if (idx >= 0 && a.p_ub[i] >= L) {
      const int slot = atomicAdd(&s_n, 1);
      if (slot < KH_SCR_CAND) s_ci[slot] = idx;  // order is free: the argmax below breaks ties by index
    }
  }
  __syncthreads();
  const int n = s_n;
  const bool overflow = S >= L || n > KH_SCR_CAND || n == 0;
  const Gemv<false, U> g(dim, 0);
  Stager<true, false, MAXV> st(a.x_save, a.final_norm, dim);
  if (!overflow) {
    if (blockIdx.x != 0) return;
    // ---- re-score: one wave per candidate row, the row requested before the vector is staged
    typename Gemv<false, U>::Regs regs;
    st.issue();
    __builtin_amdgcn_sched_barrier(0);
    const int step = KH_WAVE * U;
    int r = s_ci[wave < n ? wave : 0];
    typename Gemv<false, U>::Rows rw = g.rows(wcls, r, wcls, r, nullptr, nullptr, dim);
    g.load(regs, rw, 0, g.Mc, lane);
    const float rs = st.finish(xs, eps, red);
    for (int j = wave; j < n; j += kh_nwaves()) {
      if (j != wave) {
        r = s_ci[j];
        rw = g.rows(wcls, r, wcls, r, nullptr, nullptr, dim);
        g.load(regs, rw, 0, g.Mc, lane);
      }
      float a0 = 0.f, a1 = 0.f;
      for (int c0 = 0;;) {  // gemv_pairs' walk over a row's chunks (SPLIT = 1, no rolling refill)
        g.fma(regs, xs, c0, g.Mc, lane, a0, a1);
        c0 += step;
        if (c0 >= g.Mc) break;
        g.load(regs, rw, c0, g.Mc, lane);
      }
      float s0 = wave_sum(a0);
      s0 *= rs;
      if (lane == 0) s_cv[j] = s0;
    }
    __syncthreads();
    int idx = 0x7fffffff;
    if (threadIdx.x == 0) {
      float v = -INFINITY;
      for (int k = 0; k < n; ++k) amax_merge(v, idx, s_cv[k], s_ci[k]);
      a.stats[0] += 1;
      a.stats[1] += n;
    }
    screen_tail(a.st, idx, &s_next);
    return;
  }
  // ---- overflow: k_cls's classifier in every workgroup, argmax partials, last arriver merges
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  auto r1_of = [&](int p) __attribute__((always_inline)) { return 2 * p + 1 < vocab ? 2 * p + 1 : 2 * p; };
  auto pair = [&](int p) __attribute__((always_inline)) {
    return g.rows(wcls, 2 * p, wcls, r1_of(p), nullptr, nullptr, dim);
  };
  float rs = 1.f;
  auto epi = [&](int p, float s0, float s1, const NoAux&) __attribute__((always_inline)) {
    if (lane != 0) return;
    const int r0 = 2 * p, r1 = r1_of(p);
    s0 *= rs;
    s1 *= rs;
    amax_merge(bv, bi, s0, r0);
    if (r1 != r0) amax_merge(bv, bi, s1, r1);
  };
  gemv_pairs<1, /*ROLL=*/false>(g, xs, (vocab + 1) >> 1, lane, nullptr, pair,
                                [](int) __attribute__((always_inline)) { return NoAux{}; },
                                [&]() __attribute__((always_inline)) { st.issue(); },
                                [&]() __attribute__((always_inline)) { rs = st.finish(xs, eps, red); }, epi);
  int* redi = (int*)(red + 3 * KH_WAVES_MAX);
  __syncthreads();
  if (lane == 0) {
    red[wave] = bv;
    redi[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = red[0];
    int i = redi[0];
    for (int w = 1, nw = kh_nwaves(); w < nw; ++w) amax_merge(v, i, red[w], redi[w]);
    // agent-scope stores + a release in front of the ticket: the partial is visible to whoever draws the last one
    __hip_atomic_store(a.ov_val + blockIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.ov_idx + blockIdx.x, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  float v = -INFINITY;
  int idx = 0x7fffffff;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += kh_wg())
    amax_merge(v, idx, __hip_atomic_load(a.ov_val + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
               __hip_atomic_load(a.ov_idx + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  wave_amax(v, idx);
  __syncthreads();  // red / redi were read by thread 0 above
  if (lane == 0) {
    red[wave] = v;
    redi[wave] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    v = red[0];
    idx = redi[0];
    for (int w = 1, nw = kh_nwaves(); w < nw; ++w) amax_merge(v, idx, red[w], redi[w]);
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.stats[0] += 1;
    a.stats[2] += 1;
  }
  screen_tail(a.st, idx, &s_next);
}
