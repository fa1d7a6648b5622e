// kh_w16.h — batch-1 decode of bf16-exact fp32 models from a 16-bit copy of their matrices.
//
// Every fp32 .bin this library meets in practice was widened from a bf16 checkpoint by the exporter
// (tools/export.py:79-131 writes float32 whatever the source held), so the low 16 bits of every matrix word are
// zero and the upper 16 bits ARE the weight.  k_w16_build writes those upper halves, row-major, into a second arena
// and proves the premise while it does (it ORs every low half it drops into a flag word); GemvW16 is the view of
// such a matrix for kh_gemv.h::gemv_pairs.  A lane owns the same four columns per slot as in the fp32 view, the
// weights come back by a shift or a mask (no conversion, no rounding, no denormal mode), and the FMAs run in the
// same order, so a W16 kernel produces the bits of its fp32 twin from half the weight bytes.
// A second format (KH_W16_F16, flag KH_FLAG_W16_F16) serves fp32 images widened from an fp16 checkpoint: k_h16_build
// stores the IEEE binary16 value of every word, the view's widen converts it back (exactly), and the _h16 kernels at
// the end of this file are the _w16 kernels on that view.
// The five decode GEMV kernels exist once: their bodies (kh_fused.h: qkv_body, gemv_res_body, wo_comb_body,
// ffn13_body, cls_body) are templates over the view, and the kernels below instantiate them with GemvW16.
// Replaces nothing in the reference (it streams fp32: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
#pragma once
#include "kh_fused.h"

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// dst[i] = upper halves of the four words src[i]; *flag |= their lower halves (non-zero: the matrix is not
// bf16-exact and the copy must not be used).  n4 = elements / 4.  16-byte loads, 8-byte stores.
static __global__ __launch_bounds__(KH_WG) void k_w16_build(const u32x4* __restrict__ src, u32x2* __restrict__ dst,
                                                            size_t n4, uint32_t* flag) {
  uint32_t low = 0;
  for (size_t i = (size_t)blockIdx.x * KH_WG + threadIdx.x; i < n4; i += (size_t)gridDim.x * KH_WG) {
    const u32x4 w = src[i];
    low |= w.x | w.y | w.z | w.w;
    u32x2 o;
    o.x = (w.x >> 16) | (w.y & 0xffff0000u);  // element j in the low half, j + 1 in the high half: uint16 row-major
    o.y = (w.z >> 16) | (w.w & 0xffff0000u);
    dst[i] = o;
  }
  low &= 0xffffu;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) low |= (uint32_t)__shfl_xor((int)low, off, KH_WAVE);
  if ((threadIdx.x & 63) == 0 && low) atomicOr(flag, low);
}

// The copy's format.  KH_W16_BF16: a 16-bit field is the upper half of its fp32 word.  KH_W16_F16: it is the IEEE
// binary16 value equal to the fp32 word (an fp32 image widened from an fp16 checkpoint: 13 zero mantissa bits, an
// exponent inside fp16's normal or subnormal range).  Either way the field widens back to the very fp32 word.
enum { KH_W16_BF16 = 0, KH_W16_F16 = 1 };

// The fp16 field of one fp32 word, by integer arithmetic alone (no convert instruction, no float mode); *bad |= 1 when
// the word is not fp16-representable.  With a = |w| as a word and e its exponent field a word is exact iff a == 0, or
// 113 <= e <= 142 and its low 13 bits are zero (fp16 normals 2^-14 .. 65504), or 103 <= e <= 112 and its low 126 - e
// bits are zero (fp16 subnormals, multiples of 2^-24).  Inf and NaN are inexact: a NaN's payload would not come back.
static __device__ __forceinline__ uint32_t h16_field(uint32_t w, uint32_t& bad) {
  const uint32_t a = w & 0x7fffffffu, e = a >> 23;
  const bool norm = e >= 113 && e <= 142, sub = e >= 103 && e <= 112;
  const uint32_t drop = sub ? 126 - e : 13;  // low bits of the word that the field has no room for
  // normal: rebias the exponent (127 -> 15); subnormal: the significand with its leading one, in units of 2^-24
  const uint32_t v = sub ? (a & 0x007fffffu) | 0x00800000u : a - (112u << 23);
  bad |= (uint32_t)(a != 0 && !norm && !sub) | (uint32_t)((norm || sub) && (a & ((1u << drop) - 1)) != 0);
  return ((w >> 16) & 0x8000u) | (norm || sub ? v >> drop : 0u);
}
// k_w16_build for the fp16 format: dst[i] = the fp16 fields of the four words src[i]; *flag becomes non-zero when a
// word is not fp16-representable (the copy must not be used).  n4 = elements / 4.  16-byte loads, 8-byte stores.
static __global__ __launch_bounds__(KH_WG) void k_h16_build(const u32x4* __restrict__ src, u32x2* __restrict__ dst,
                                                            size_t n4, uint32_t* flag) {
  uint32_t bad = 0;
  for (size_t i = (size_t)blockIdx.x * KH_WG + threadIdx.x; i < n4; i += (size_t)gridDim.x * KH_WG) {
    const u32x4 w = src[i];
    u32x2 o;
    o.x = h16_field(w.x, bad) | (h16_field(w.y, bad) << 16);  // element j in the low half, j + 1 in the high half
    o.y = h16_field(w.z, bad) | (h16_field(w.w, bad) << 16);
    dst[i] = o;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= (uint32_t)__shfl_xor((int)bad, off, KH_WAVE);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(flag, bad);
}

// Register tile: one chunk (U x 512 B) of two rows, two 32-bit words = four weights per slot.  The format is part of
// the type: the B-token overload of fma_chunk_b (kh_w16_pass.h) is found through the tile alone.
template <int U, int FMT = KH_W16_BF16>
struct RegsW16 {
  u32x2 v0[U], v1[U];
};
struct RowsW16 {
  const u32x2* w0;
  const u32x2* w1;
};

// The matrix view (interface: kh_gemv.h::gemv_pairs, G).  Units are 8 bytes = the four columns of the fp32 view's
// 16-byte unit, so Mc, the split partition and every index below are those of Gemv<false, U>.
template <int U, int FMT = KH_W16_BF16>
struct GemvW16 {
  static constexpr int kU = U;
  static constexpr bool kLayoutQ8 = false;
  using Regs = RegsW16<U, FMT>;
  using Rows = RowsW16;
  int Mc;  // units per row: M/4
  __device__ __forceinline__ GemvW16(int M, int /*gshift*/) : Mc(M >> 2) {}
  __device__ __forceinline__ Rows rows(const void* w0_base, int r0, const void* w1_base, int r1, const float*,
                                       const float*, int M) const {
    return Rows{(const u32x2*)((const uint16_t*)w0_base + (size_t)r0 * M),
                (const u32x2*)((const uint16_t*)w1_base + (size_t)r1 * M)};
  }
  __device__ __forceinline__ void load1(Regs& r, const Rows& rw, int c0, int lim, int lane, int u) const {
    const int idx = c0 + u * KH_WAVE + lane;
    const int cidx = idx < lim ? idx : 0;  // clamped address; masked in fma1 (kh_gemv.h::load_u)
    r.v0[u] = ld_nt(rw.w0 + cidx);
    r.v1[u] = ld_nt(rw.w1 + cidx);
    __builtin_amdgcn_sched_barrier(0);  // see the fp32 load_u
  }
  // the four fp32 words of a slot.  bf16: bit operations only.  fp16: four conversions, each exact (every finite fp16
  // value, subnormals included, is an fp32 normal or zero), which the compiler is free to fold into the FMA's operand
  static __device__ __forceinline__ f32x4 widen(u32x2 d) {
    f32x4 w;
    if constexpr (FMT == KH_W16_F16) {
      w.x = (float)__builtin_bit_cast(_Float16, (uint16_t)(d.x & 0xffffu));
      w.y = (float)__builtin_bit_cast(_Float16, (uint16_t)(d.x >> 16));
      w.z = (float)__builtin_bit_cast(_Float16, (uint16_t)(d.y & 0xffffu));
      w.w = (float)__builtin_bit_cast(_Float16, (uint16_t)(d.y >> 16));
    } else {
      w.x = __builtin_bit_cast(float, d.x << 16);
      w.y = __builtin_bit_cast(float, d.x & 0xffff0000u);
      w.z = __builtin_bit_cast(float, d.y << 16);
      w.w = __builtin_bit_cast(float, d.y & 0xffff0000u);
    }
    return w;
  }
  __device__ __forceinline__ void fma1(const Regs& r, const f32x4* xs, int c0, int lim, int lane, int u, float& a0,
                                       float& a1) const {
    // lanes past the end: clamped address, zeroed x (kh_gemv.h::fma_u, same proviso on the row's first four weights)
    const int idx = c0 + u * KH_WAVE + lane;
    const bool in = idx < lim;
    f32x4 xv = xs[in ? idx : 0];
    xv.x = in ? xv.x : 0.f;
    xv.y = in ? xv.y : 0.f;
    xv.z = in ? xv.z : 0.f;
    xv.w = in ? xv.w : 0.f;
    a0 = fma4(widen(r.v0[u]), xv, a0);
    a1 = fma4(widen(r.v1[u]), xv, a1);
  }
  __device__ __forceinline__ void load(Regs& r, const Rows& rw, int c0, int lim, int lane) const {
#pragma unroll
    for (int u = 0; u < U; ++u) load1(r, rw, c0, lim, lane, u);
  }
  __device__ __forceinline__ void fma(const Regs& r, const f32x4* xs, int c0, int lim, int lane, float& a0,
                                      float& a1) const {
#pragma unroll
    for (int u = 0; u < U; ++u) fma1(r, xs, c0, lim, lane, u, a0, a1);
  }
};

// The decode GEMV kernels on the copy: KhLin::w of their arguments points into the 16-bit arena, everything else
// (norm weights, biases, sin/cos, vectors) is what the fp32 launch passes.  Plain LDS layout, the fp32 refill policy.
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_qkv_w16(const KhQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  qkv_body<GemvW16<U>, false, MAXV, SPLIT>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_gemv_res_w16(const KhGemvResArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  f32x4* xs = (f32x4*)smem_raw;
  Stager<false, false, MAXV> st(a.vec, nullptr, a.M);
  gemv_res_body<GemvW16<U>, SPLIT>(a, st, xs, lds_red_ptr<false>(xs, a.M));
  KH_STAMP_FLUSH();
}
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_wo_comb_w16(const KhWoCombArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  wo_comb_body<GemvW16<U>, false, MAXV, SPLIT>(a, (f32x4*)smem_raw);
}
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_ffn13_w16(const KhFfn13Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  ffn13_body<GemvW16<U>, false, MAXV>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_cls_w16(const KhClsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  cls_body<GemvW16<U>, false, MAXV>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}

// The same five on an fp16-format copy (KH_FLAG_W16_F16): the bodies, instantiation lists, launch bounds and LDS layout
// of the kernels above; only GemvW16::widen differs.  Stems of their own, so the _w16 names and sets stay what they were.
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_qkv_h16(const KhQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  qkv_body<GemvW16<U, KH_W16_F16>, false, MAXV, SPLIT>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_gemv_res_h16(const KhGemvResArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  f32x4* xs = (f32x4*)smem_raw;
  Stager<false, false, MAXV> st(a.vec, nullptr, a.M);
  gemv_res_body<GemvW16<U, KH_W16_F16>, SPLIT>(a, st, xs, lds_red_ptr<false>(xs, a.M));
  KH_STAMP_FLUSH();
}
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_wo_comb_h16(const KhWoCombArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  wo_comb_body<GemvW16<U, KH_W16_F16>, false, MAXV, SPLIT>(a, (f32x4*)smem_raw);
}
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_ffn13_h16(const KhFfn13Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  ffn13_body<GemvW16<U, KH_W16_F16>, false, MAXV>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_cls_h16(const KhClsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  cls_body<GemvW16<U, KH_W16_F16>, false, MAXV>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
