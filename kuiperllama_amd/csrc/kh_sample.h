// kh_sample.h — seeded temperature / top-k / top-p sampling on the device (gfx950).
//
// Semantics (include/kuiper_hip.h, kh_sampling; tests/sampling_ref.py is the fp64 statement of the same):
//   order the tokens by (logit descending, index ascending); keep the first K (0 < K < V); weights
//   w_i = exp((l_i - l_max) / T); keep the shortest prefix of that order whose weight reaches P times the kept total
//   (P < 1) = S; u = ((x >> 8) + 0.5) * 2^-24 with x = Philox4x32-10(counter (c, 0, 0, 0), key (seed lo, seed hi))[0];
//   the pick is the smallest index j in S whose index-order prefix sum of w over S exceeds u * Z_S.
//
// One workgroup of 1024 threads per draw, no sort:
//   pass 1 (global)  (count, weight) histogram of every token on 2048 bins of (l_max - l) / T (32 bins per unit;
//                    the last bin takes everything from 64 on).  Bins are monotone in the logit, so the bins up to
//                    the one where the top-k count (or, without top-k, the top-p weight) is reached hold every token
//                    S can contain: the CANDIDATES.
//   pass 2 (global)  when there are at most KH_SAMP_CAP of them (peaked logits), the candidates are compacted into
//                    LDS; otherwise (flat logits) every later step re-reads the logits from global memory and
//                    filters them by bin.  Both sources give bit-identical results.
//   then             exact MSD radix descents (11-bit digits; index digits cut at bits 8 / 19 / 30) over the candidates: the 32-bit order key of the
//                    K-th token, the key at which the top-p weight is reached, the index cut among equal logits at
//                    the boundary, and finally the pick itself as a weighted descent over the index bits.
// Every sum is an integer sum of fixed-point weights (round(w * 2^sb), sb = min(52, 63 - bitlen(V))): LDS atomics in
// any order give the same totals, so draws are bit-reproducible.  The fixed point costs at most V * 2^-sb-1 of
// absolute weight against Z >= 1 (the top token has w = 1): below 1e-8 relative for V < 2^20.
// No scratch, no inline assembly; every result is written with plain C++ stores.
// The step tail built on it, k_sample_topp (end of this file), shares the forced-token rule, the commit and the
// embedding gather with the other step tails: kh_step_tail.h (kh_step_begin / kh_step_end).
#pragma once
#include <cmath>

#include "kh_common.h"
#include "kh_logit_proc.h"
#include "kh_step_tail.h"

#define KH_SAMP_THREADS 1024
#define KH_SAMP_NB 2048   // histogram bins = 2^11 (one 11-bit digit of a radix descent)
#define KH_SAMP_BPU 32    // first-pass bins per unit of (l_max - l) / T
#define KH_SAMP_CAP 4096  // candidates compacted into LDS

// the sampling parameters as the kernels read them (the model keeps one copy on the device)
struct KhSampParams {
  float temperature;
  int32_t top_k;
  float top_p;
  uint32_t seed_lo, seed_hi;
};

// host: parameters valid (a non-finite temperature, K < 0, P NaN or outside (0, 1] are not)
static inline bool kh_sampling_valid(const kh_sampling* p) {
  return p && std::isfinite(p->temperature) && p->top_k >= 0 && p->top_p > 0.f && p->top_p <= 1.f;
}
static inline bool kh_sampling_greedy(const kh_sampling* p) { return !p || p->temperature <= 0.f; }
static inline KhSampParams kh_samp_params(const kh_sampling* p) {
  return KhSampParams{p->temperature, p->top_k, p->top_p, (uint32_t)(p->seed & 0xffffffffu), (uint32_t)(p->seed >> 32)};
}

struct KhU4 {
  uint32_t x, y, z, w;
};
// Philox4x32-10 (Salmon et al., SC'11): 10 rounds, key bumped by the Weyl constants between rounds
__host__ __device__ inline KhU4 kh_philox4x32_10(KhU4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    c = KhU4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
  }
  return c;
}
// u in (0, 1) of a draw
__host__ __device__ inline double kh_samp_uniform(uint32_t counter, uint32_t seed_lo, uint32_t seed_hi) {
  const KhU4 r = kh_philox4x32_10(KhU4{counter, 0u, 0u, 0u}, seed_lo, seed_hi);
  return ((double)(r.x >> 8) + 0.5) * (1.0 / 16777216.0);
}

// order-preserving 32-bit key of a logit (larger logit -> larger key; -0 and +0 share one key) and its inverse
__device__ __forceinline__ uint32_t kh_okey(float l) {
  const uint32_t b = __float_as_uint(l == 0.f ? 0.f : l);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float kh_okey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct KhSampSmem {
  uint32_t cnt[KH_SAMP_NB];
  unsigned long long wsum[KH_SAMP_NB];
  float cl[KH_SAMP_CAP];    // candidate logits
  int32_t ci[KH_SAMP_CAP];  // candidate indices
  float red[KH_SAMP_THREADS / KH_WAVE];
  int red_i[KH_SAMP_THREADS / KH_WAVE];
  unsigned long long wt_c[KH_SAMP_THREADS / KH_WAVE], wt_w[KH_SAMP_THREADS / KH_WAVE];  // walk: per-wave totals
  unsigned long long r_wb, r_cb;  // descent step: weight / count of the included values walked before the digit
  int r_digit;                    // -1: the target was not reached
  int ncand;
};

// Per-draw state: the logits, the constants of the weight function and the candidate source.
struct KhSampCtx {
  const float* logits;
  int n;
  float lmax, T;
  double fx_scale;  // 2^sb
  int b_end;        // candidates: first-pass bin <= b_end
  bool in_lds;      // candidates compacted into KhSampSmem::cl / ci
  __device__ __forceinline__ float expo(float l) const { return (l - lmax) / T; }
  __device__ __forceinline__ int bin_of(float e) const {
    return e > -(float)(KH_SAMP_NB / KH_SAMP_BPU) ? min((int)(-e * (float)KH_SAMP_BPU), KH_SAMP_NB - 1)
                                                  : KH_SAMP_NB - 1;
  }
  __device__ __forceinline__ unsigned long long fx_of_e(float e) const {
    const float w = e > -104.f ? expf(e) : 0.f;  // expf underflows to 0 below about -103.97
    return (unsigned long long)((double)w * fx_scale + 0.5);
  }
  __device__ __forceinline__ unsigned long long fx(float l) const { return fx_of_e(expo(l)); }
};

// f(logit, index) for every element of the logits.  Each thread takes 16 consecutive elements per step (four float4
// loads in flight when the vector is 16-byte aligned): more bytes in flight for the single workgroup, and runs of
// consecutive indices per thread, which the histogram updates below merge before their LDS atomics.
template <class F>
__device__ __forceinline__ void kh_samp_for_global(const float* lg, int n, F&& f) {
  int done = 0;
  if ((((uintptr_t)lg) & 15u) == 0) {
    const int n16 = n >> 4;
    const f32x4* l4 = (const f32x4*)lg;
    for (int q = threadIdx.x; q < n16; q += KH_SAMP_THREADS) {
      const f32x4 v0 = l4[4 * q], v1 = l4[4 * q + 1], v2 = l4[4 * q + 2], v3 = l4[4 * q + 3];
      const int i = 16 * q;
      f(v0.x, i); f(v0.y, i + 1); f(v0.z, i + 2); f(v0.w, i + 3);
      f(v1.x, i + 4); f(v1.y, i + 5); f(v1.z, i + 6); f(v1.w, i + 7);
      f(v2.x, i + 8); f(v2.y, i + 9); f(v2.z, i + 10); f(v2.w, i + 11);
      f(v3.x, i + 12); f(v3.y, i + 13); f(v3.z, i + 14); f(v3.w, i + 15);
    }
    done = 16 * n16;
  }
  for (int i = done + threadIdx.x; i < n; i += KH_SAMP_THREADS) f(lg[i], i);
}
// Histogram update with the thread's current run merged: consecutive adds to one bin become one pair of atomics.
struct KhSampRun {
  int d = -1;
  uint32_t c = 0;
  unsigned long long w = 0;
  __device__ __forceinline__ void flush(uint32_t* cnt, unsigned long long* wsum) {
    if (d >= 0) {
      atomicAdd(&cnt[d], c);
      if (w) atomicAdd(&wsum[d], w);
    }
    d = -1;
    c = 0;
    w = 0;
  }
  __device__ __forceinline__ void add(uint32_t* cnt, unsigned long long* wsum, int bin, unsigned long long wt) {
    if (bin != d) {
      flush(cnt, wsum);
      d = bin;
    }
    c += 1;
    w += wt;
  }
};
// f(logit, index) for every candidate
template <class F>
__device__ __forceinline__ void kh_samp_for_src(const KhSampCtx& c, KhSampSmem& s, F&& f) {
  if (c.in_lds) {
    for (int i = threadIdx.x; i < s.ncand; i += KH_SAMP_THREADS) f(s.cl[i], s.ci[i]);
  } else {
    kh_samp_for_global(c.logits, c.n, [&](float l, int i) __attribute__((always_inline)) {
      if (c.bin_of(c.expo(l)) <= c.b_end) f(l, i);
    });
  }
}

// The workgroup walks bins 0 .. nb-1 (desc: nb-1 .. 0) of s.cnt / s.wsum and finds the first bin at which the
// running total of the primary quantity (counts, or weights when by_w) plus its base satisfies  total >= target
// (total > target when strict).  Leaves the bin in s.r_digit (-1: never reached) and the count / weight walked BEFORE
// it in s.r_cb / s.r_wb.  Thread t owns walk positions 2t and 2t+1; one workgroup scan.  Called by all threads; the
// caller synchronises before and after.
__device__ inline void kh_samp_walk(KhSampSmem& s, int nb, bool desc, bool by_w, bool strict, double target,
                                    unsigned long long cbase, unsigned long long wbase) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned long long c0 = 0, w0 = 0, c1 = 0, w1 = 0;
  int b0 = -1, b1 = -1;
  if (2 * t < nb) {
    b0 = desc ? nb - 1 - 2 * t : 2 * t;
    c0 = s.cnt[b0];
    w0 = s.wsum[b0];
  }
  if (2 * t + 1 < nb) {
    b1 = desc ? nb - 2 - 2 * t : 2 * t + 1;
    c1 = s.cnt[b1];
    w1 = s.wsum[b1];
  }
  unsigned long long ci = c0 + c1, wi = w0 + w1;
#pragma unroll
  for (int off = 1; off < KH_WAVE; off <<= 1) {
    const unsigned long long co = __shfl_up(ci, off, KH_WAVE);
    const unsigned long long wo = __shfl_up(wi, off, KH_WAVE);
    if (lane >= off) {
      ci += co;
      wi += wo;
    }
  }
  if (lane == KH_WAVE - 1) {
    s.wt_c[wave] = ci;
    s.wt_w[wave] = wi;
  }
  if (t == 0) s.r_digit = -1;
  __syncthreads();
  for (int w = 0; w < wave; ++w) {
    ci += s.wt_c[w];
    wi += s.wt_w[w];
  }
  auto reached = [&](unsigned long long c, unsigned long long w) __attribute__((always_inline)) {
    const double v = by_w ? (double)(wbase + w) : (double)(cbase + c);
    return strict ? v > target : v >= target;
  };
  const unsigned long long ce = ci - c0 - c1, we = wi - w0 - w1;  // walked before this thread's bins
  if (reached(ci, wi) && !reached(ce, we)) {  // the running total is monotone: exactly one thread
    if (reached(ce + c0, we + w0)) {
      s.r_digit = b0;
      s.r_cb = ce;
      s.r_wb = we;
    } else {
      s.r_digit = b1;
      s.r_cb = ce + c0;
      s.r_wb = we + w0;
    }
  }
}

struct KhSampDesc {
  uint32_t value;              // the value found
  unsigned long long c_before; // count / weight of the included elements ordered before it
  unsigned long long w_before;
  unsigned long long c_at;     // count / weight of the included elements with exactly that value
  unsigned long long w_at;
  bool found;
};
// MSD radix descent over a B-bit value of the candidates (11-bit digits): sel(l, i, &v) says whether the element
// takes part and gives its value.  desc walks values from the largest down.  Called by the whole workgroup.
template <class Sel>
__device__ inline KhSampDesc kh_samp_descend(const KhSampCtx& c, KhSampSmem& s, Sel sel, int B, bool desc,
                                             bool by_w, bool strict, double target, bool low8 = false) {
  KhSampDesc r{0u, 0ull, 0ull, 0ull, 0ull, false};
  uint32_t prefix = 0;
  for (int hi = B; hi > 0;) {
    // order keys: 11-bit digits from the top; indices: digit boundaries at bits 8, 19 and 30, so that the 16
    // consecutive indices of a thread share their upper digit (one merged atomic) and the lowest level spans 256
    const int lo = !low8 ? (hi > 11 ? hi - 11 : 0) : hi <= 8 ? 0 : hi <= 19 ? 8 : hi <= 30 ? 19 : 30;
    const int nb = 1 << (hi - lo);
    for (int b = threadIdx.x; b < nb; b += KH_SAMP_THREADS) {
      s.cnt[b] = 0;
      s.wsum[b] = 0;
    }
    __syncthreads();
    KhSampRun run;
    kh_samp_for_src(c, s, [&](float l, int i) __attribute__((always_inline)) {
      uint32_t v;
      if (!sel(l, i, v)) return;
      if (hi < 32 && (v >> hi) != prefix) return;
      run.add(s.cnt, s.wsum, (int)((v >> lo) & (uint32_t)(nb - 1)), c.fx(l));
    });
    run.flush(s.cnt, s.wsum);
    __syncthreads();
    kh_samp_walk(s, nb, desc, by_w, strict, target, r.c_before, r.w_before);
    __syncthreads();
    const int d = s.r_digit;
    if (d < 0) return r;  // uniform: every thread read the same word
    r.c_before += s.r_cb;
    r.w_before += s.r_wb;
    r.c_at = s.cnt[d];
    r.w_at = s.wsum[d];
    prefix = (prefix << (hi - lo)) | (uint32_t)d;
    hi = lo;
    __syncthreads();  // s.r_* and the bins are rewritten by the next level
  }
  r.value = prefix;
  r.found = true;
  return r;
}

// workgroup max of one float per thread (all threads get it)
__device__ inline float kh_samp_block_max(KhSampSmem& s, float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, KH_WAVE));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s.red[wave] = v;
  __syncthreads();
  float m = s.red[0];
  for (int w = 1; w < KH_SAMP_THREADS / KH_WAVE; ++w) m = fmaxf(m, s.red[w]);
  return m;
}
__device__ inline int kh_samp_block_max_i(KhSampSmem& s, int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, KH_WAVE));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s.red_i[wave] = v;
  __syncthreads();
  int m = s.red_i[0];
  for (int w = 1; w < KH_SAMP_THREADS / KH_WAVE; ++w) m = max(m, s.red_i[w]);
  return m;
}
// Per-workgroup first maxima of a row that another launch left (k_cls: part_val / part_idx); val == null: none
struct KhAmaxParts {
  const float* val;
  const int32_t* idx;
  int n;
};
// The FIRST maximum of the row lg[0 .. n) and its index (ties -> lowest index: amax_merge; a row without a maximum,
// every entry NaN, gives 0x7fffffff).  Called by all threads with one slot per wave in red / red_i; THREAD 0 returns
// with the row's (v, idx), the other threads with partial results.  Rows on 16-byte boundaries take the walker's
// vector path.  No arithmetic enters a maximum, so the index is k_sample's pick on the same logits - and `parts`, where
// a launch left them for this row, give the same (v, idx) without the pass over the row.
__device__ __forceinline__ void kh_samp_row_amax(const float* lg, int n, float* red, int* red_i, float& v, int& idx,
                                                 const KhAmaxParts parts = {nullptr, nullptr, 0}) {
  v = -INFINITY;
  idx = 0x7fffffff;
  if (parts.val) {  // uniform
    for (int i = threadIdx.x; i < parts.n; i += KH_SAMP_THREADS) amax_merge(v, idx, parts.val[i], parts.idx[i]);
  } else {
    kh_samp_for_global(lg, n, [&](float l, int i) __attribute__((always_inline)) { amax_merge(v, idx, l, i); });
  }
  wave_amax(v, idx);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave] = v;
    red_i[wave] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    v = red[0];
    idx = red_i[0];
#pragma unroll
    for (int w = 1; w < KH_SAMP_THREADS / KH_WAVE; ++w) amax_merge(v, idx, red[w], red_i[w]);
  }
}

// The sampler core: one draw from logits[0..n) with temperature T > 0, given l_max.  Called by all 1024 threads of
// the workgroup; every thread returns the sampled index.
__device__ inline int kh_sample_core(KhSampSmem& s, const float* logits, int n, float lmax, const KhSampParams& p,
                                     uint32_t counter) {
  if (n <= 1) return 0;
  KhSampCtx c;
  c.logits = logits;
  c.n = n;
  c.lmax = lmax;
  c.T = p.temperature;
  const int vbits = 32 - __clz(n);
  c.fx_scale = (double)(1ull << min(52, 63 - vbits));
  c.b_end = KH_SAMP_NB - 1;
  c.in_lds = false;
  const bool use_k = p.top_k > 0 && p.top_k < n;
  const bool use_p = p.top_p < 1.f;

  // ---- pass 1: (count, weight) per bin of (l_max - l) / T
  for (int b = threadIdx.x; b < KH_SAMP_NB; b += KH_SAMP_THREADS) {
    s.cnt[b] = 0;
    s.wsum[b] = 0;
  }
  if (threadIdx.x == 0) s.ncand = 0;
  __syncthreads();
  {
    KhSampRun run;
    kh_samp_for_global(logits, n, [&](float l, int) __attribute__((always_inline)) {
      const float e = c.expo(l);
      run.add(s.cnt, s.wsum, c.bin_of(e), c.fx_of_e(e));
    });
    run.flush(s.cnt, s.wsum);
  }
  __syncthreads();
  // total weight and the candidate bins
  kh_samp_walk(s, KH_SAMP_NB, false, false, false, (double)n, 0, 0);  // reaches the last non-empty bin: totals
  __syncthreads();
  const unsigned long long ztot = s.r_wb + s.wsum[s.r_digit];
  const int n_total = n;
  __syncthreads();
  if (use_k || use_p) {
    kh_samp_walk(s, KH_SAMP_NB, false, use_k ? false : true, false,
                 use_k ? (double)p.top_k : (double)p.top_p * (double)ztot, 0, 0);
    __syncthreads();
    c.b_end = s.r_digit >= 0 ? s.r_digit : KH_SAMP_NB - 1;
    const unsigned long long ncand = s.r_digit >= 0 ? s.r_cb + s.cnt[s.r_digit] : (unsigned long long)n_total;
    __syncthreads();
    // ---- pass 2: compact the candidates into LDS when they fit
    if (ncand <= KH_SAMP_CAP) {
      kh_samp_for_global(logits, n, [&](float l, int i) __attribute__((always_inline)) {
        if (c.bin_of(c.expo(l)) <= c.b_end) {
          const int slot = atomicAdd(&s.ncand, 1);
          s.cl[slot] = l;
          s.ci[slot] = i;
        }
      });
      c.in_lds = true;
      __syncthreads();
    }
  } else if (n <= KH_SAMP_CAP) {
    kh_samp_for_global(logits, n, [&](float l, int i) __attribute__((always_inline)) {
      s.cl[i] = l;
      s.ci[i] = i;
    });
    if (threadIdx.x == 0) s.ncand = n;
    c.in_lds = true;
    __syncthreads();
  }

  // ---- the boundary of S in the order: keys > t_key, and the first m_key of the keys == t_key by index
  bool bounded = false;
  uint32_t t_key = 0;
  unsigned long long m_key = 0, ties = 0, z_s = ztot;
  if (use_k) {
    const KhSampDesc d = kh_samp_descend(
        c, s, [&](float l, int, uint32_t& v) __attribute__((always_inline)) { v = kh_okey(l); return true; }, 32,
        /*desc=*/true, /*by_w=*/false, /*strict=*/false, (double)p.top_k);
    bounded = true;
    t_key = d.value;
    m_key = (unsigned long long)p.top_k - d.c_before;
    ties = d.c_at;
    z_s = d.w_before + m_key * c.fx(kh_okey_inv(t_key));
  }
  if (use_p) {
    const double target = (double)p.top_p * (double)z_s;
    const uint32_t t_k = t_key;
    const unsigned long long m_k = m_key;
    const bool had_k = bounded;
    const KhSampDesc d = kh_samp_descend(
        c, s,
        [&](float l, int, uint32_t& v) __attribute__((always_inline)) {
          v = kh_okey(l);
          return v >= t_k;
        },
        32, /*desc=*/true, /*by_w=*/true, /*strict=*/false, target);
    if (d.found) {
      const unsigned long long wt = c.fx(kh_okey_inv(d.value));
      unsigned long long cap = d.c_at;
      if (had_k && d.value == t_k && m_k < cap) cap = m_k;
      unsigned long long m = 1;
      if (wt > 0) {
        const double need = (target - (double)d.w_before) / (double)wt;
        m = need > 1.0 ? (unsigned long long)ceil(need) : 1ull;
        if (m > cap) m = cap;
        while (m > 1 && (double)(d.w_before + (m - 1) * wt) >= target) --m;
        while (m < cap && (double)(d.w_before + m * wt) < target) ++m;
      }
      bounded = true;
      t_key = d.value;
      m_key = m;
      ties = d.c_at;
      z_s = d.w_before + m * wt;
    }
  }
  // index cut among the ties at the boundary: the m_key-th smallest index with key == t_key
  int i_cut = 0x7fffffff;
  if (bounded && m_key < ties) {
    const uint32_t t = t_key;
    const KhSampDesc d = kh_samp_descend(
        c, s,
        [&](float l, int i, uint32_t& v) __attribute__((always_inline)) {
          v = (uint32_t)i;
          return kh_okey(l) == t;
        },
        vbits, /*desc=*/false, /*by_w=*/false, /*strict=*/false, (double)m_key, /*low8=*/true);
    if (d.found) i_cut = (int)d.value;
  }
  const uint32_t tb = t_key;
  const bool bnd = bounded;
  auto in_s = [&](float l, int i) __attribute__((always_inline)) {
    if (!bnd) return true;
    const uint32_t k = kh_okey(l);
    return k > tb || (k == tb && i <= i_cut);
  };
  // ---- the pick: smallest index whose index-order prefix weight over S exceeds u * Z_S
  const double thr = kh_samp_uniform(counter, p.seed_lo, p.seed_hi) * (double)z_s;
  const KhSampDesc d = kh_samp_descend(
      c, s,
      [&](float l, int i, uint32_t& v) __attribute__((always_inline)) {
        v = (uint32_t)i;
        return in_s(l, i);
      },
      vbits, /*desc=*/false, /*by_w=*/true, /*strict=*/true, thr, /*low8=*/true);
  if (d.found) return (int)d.value;
  // rounding left no index past the threshold: the largest index of S
  int best = -1;
  kh_samp_for_src(c, s, [&](float l, int i) __attribute__((always_inline)) {
    if (in_s(l, i)) best = max(best, i);
  });
  return kh_samp_block_max_i(s, best);
}

// ---- operator: n_draws draws (one workgroup each) on one logit vector, counters counter0 + draw
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_sample_op(const float* logits, int n, KhSampParams p,
                                                                       uint32_t counter0, int32_t* out) {
  __shared__ KhSampSmem s;
  float m = -INFINITY;
  kh_samp_for_global(logits, n, [&](float l, int) __attribute__((always_inline)) { m = fmaxf(m, l); });
  const float lmax = kh_samp_block_max(s, m);
  const int r = kh_sample_core(s, logits, n, lmax, p, counter0 + (uint32_t)blockIdx.x);
  if (threadIdx.x == 0) out[blockIdx.x] = r;
}
// out[1 .. n) = out[0] (greedy draws: one argmax, copied)
static __global__ __launch_bounds__(KH_WG) void k_sample_bcast(int32_t* out, int n) {
  const int v = out[0];
  for (int i = 1 + blockIdx.x * KH_WG + threadIdx.x; i < n; i += gridDim.x * KH_WG) out[i] = v;
}

// ---- the decode step's sampler: k_sample's duties on the helpers of kh_step_tail.h (the forced-token rule, the commit,
// the embedding gather of the token fed next) with a sampled token instead of the argmax merge.  l_max comes from
// k_cls's per-workgroup partials; the counter is the step's position.  The rule is evaluated first and broadcast:
// forced steps leave before reading any logit.
// (The step's last launch while penalties, a logit bias or log-probs are on - k_sample_proc, k_sample_lp - runs
// kh_tail_chain between the same begin and commit: kh_logprobs.h.)
struct KhSampleTopArgs {
  const float* logits;
  const float* part_val;
  int nparts;
  const KhSampParams* params;  // device copy (kh_model_set_sampling)
  KhStepState st;
};
static __global__ __launch_bounds__(KH_SAMP_THREADS) void k_sample_topp(const KhSampleTopArgs a) {
  __shared__ KhSampSmem s;
  int pos, forced, pick = -1;
  kh_step_begin(a.st, pos, forced);
  if (forced < 0) {
    float m = -INFINITY;
    for (int i = threadIdx.x; i < a.nparts; i += KH_SAMP_THREADS) m = fmaxf(m, a.part_val[i]);
    const float lmax = kh_samp_block_max(s, m);
    const KhSampParams p = *a.params;
    pick = kh_sample_core(s, a.logits, a.st.vocab, lmax, p, (uint32_t)pos);
  }
  kh_step_end(a.st, pos, forced, pick, nullptr, 0, KH_SAMP_THREADS);
}
