// kh_q4.h — batch-1 decode of 4-bit-exact int8 models from a packed 4-bit copy of their matrices.
//
// An int8 .bin whose quantised values all lie in [-8, 7] is a legal int8 checkpoint (tools/export.py:134-210 writes
// int8 whatever range the quantiser used), and for such an image the low nibble of every byte IS the weight.
// k_q4_build writes those nibbles, two per byte and row-major, into a second arena and proves the premise while it does
// (it ORs an "outside [-8, 7]" bit per tensor); GemvQ4 is the view of such a matrix for kh_gemv.h::gemv_pairs.  A lane
// owns the same sixteen columns per slot as in the int8 view, reads the same fp32 group scales where the image keeps
// them, and runs dot4_i8's chain - sixteen FMAs into t in ascending column order, then fma(scale, t, a) - on weights
// that come back by a sign-extending bit-field extract and an (exact) integer -> float conversion.  So a Q4 kernel
// produces the bits of its int8 twin from half the weight bytes.
// The five decode GEMV kernels exist once: their bodies (kh_fused.h) are templates over the view, and the kernels
// below instantiate them with GemvQ4, the q8_slot LDS layout and the int8 refill policy (LQ8 = true).
// Replaces nothing in the reference (it streams int8: kuiper/source/op/kernels/cuda/matmul_kernel.cu:56-87).
#pragma once
#include "kh_fused.h"
#include "kh_w16.h"  // u32x2

// dst[i] = the low nibbles of the sixteen int8 values src[i], value 2j in the low and 2j + 1 in the high half of byte
// j; *flag becomes non-zero when a value lies outside [-8, 7] (the copy must not be used).  n16 = elements / 16.
// 16-byte loads, 8-byte stores.
static __device__ __forceinline__ uint32_t q4_pack4(uint32_t w, uint32_t& bad) {
  // bits 3..7 of a byte in range are all equal: s = 0 or 0x1f, s + 1 = 1 or 0x20, neither has a bit of 0x1e; every
  // other s (1 .. 0x1e) gives 2 .. 0x1f, which has one.  No carry leaves a byte.
  const uint32_t s = (w >> 3) & 0x1f1f1f1fu;
  bad |= (s + 0x01010101u) & 0x1e1e1e1eu;
  return (w & 0xfu) | ((w >> 4) & 0xf0u) | ((w >> 8) & 0xf00u) | ((w >> 12) & 0xf000u);
}
static __global__ __launch_bounds__(KH_WG) void k_q4_build(const u32x4* __restrict__ src, u32x2* __restrict__ dst,
                                                           size_t n16, uint32_t* flag) {
  uint32_t bad = 0;
  for (size_t i = (size_t)blockIdx.x * KH_WG + threadIdx.x; i < n16; i += (size_t)gridDim.x * KH_WG) {
    const u32x4 w = src[i];
    u32x2 o;
    o.x = q4_pack4(w.x, bad) | (q4_pack4(w.y, bad) << 16);
    o.y = q4_pack4(w.z, bad) | (q4_pack4(w.w, bad) << 16);
    dst[i] = o;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= (uint32_t)__shfl_xor((int)bad, off, KH_WAVE);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(flag, 1u);
}

// Register tile: one chunk (U x 512 B) of two rows, two 32-bit words = sixteen weights per slot, and the group scale
// of each (the int8 tile's)
template <int U>
struct RegsQ4 {
  u32x2 q0[U], q1[U];
  float g0[U], g1[U];
};
struct RowsQ4 {
  const u32x2* w0;
  const u32x2* w1;
  const float* sc0;  // scale of the row's first group, in the int8 image
  const float* sc1;
};

// nibble k (0 .. 7) of a word as the float of its signed value: v_bfe_i32 + v_cvt_f32_i32, both exact
template <int K>
static __device__ __forceinline__ float q4_val(uint32_t w) {
  return (float)((int32_t)(w << (28 - 4 * K)) >> 28);
}
// dot4_i8 (kh_common.h) on nibbles 4H .. 4H + 3 of a word: the same four FMAs in the same order
template <int H>
static __device__ __forceinline__ float dot4_q4(uint32_t w, f32x4 x, float acc) {
  acc = __builtin_fmaf(q4_val<4 * H>(w), x.x, acc);
  acc = __builtin_fmaf(q4_val<4 * H + 1>(w), x.y, acc);
  acc = __builtin_fmaf(q4_val<4 * H + 2>(w), x.z, acc);
  acc = __builtin_fmaf(q4_val<4 * H + 3>(w), x.w, acc);
  return acc;
}

// The matrix view (interface: kh_gemv.h::gemv_pairs, G).  Units are 8 bytes = the sixteen columns of the int8 view's
// 16-byte unit, so Mc, the split partition, the group index and every index below are those of Gemv<true, U>.
template <int U>
struct GemvQ4 {
  static constexpr int kU = U;
  static constexpr bool kLayoutQ8 = true;  // the int8 view's staged vector
  using Regs = RegsQ4<U>;
  using Rows = RowsQ4;
  int Mc;  // units per row: M/16
  int gshift;
  __device__ __forceinline__ GemvQ4(int M, int gs) : Mc(M >> 4), gshift(gs) {}
  __device__ __forceinline__ Rows rows(const void* w0_base, int r0, const void* w1_base, int r1, const float* s0_base,
                                       const float* s1_base, int M) const {
    const int gpr = M >> gshift;  // groups per row
    return Rows{(const u32x2*)((const uint8_t*)w0_base + (size_t)r0 * (M >> 1)),
                (const u32x2*)((const uint8_t*)w1_base + (size_t)r1 * (M >> 1)), s0_base + (size_t)r0 * gpr,
                s1_base + (size_t)r1 * gpr};
  }
  // issue order per slot: q0, q1, s0, s1 (kh_gemv.h: the int8 load_u)
  __device__ __forceinline__ void load1(Regs& r, const Rows& rw, int c0, int lim, int lane, int u) const {
    const int idx = c0 + u * KH_WAVE + lane;
    const int cidx = idx < lim ? idx : 0;  // clamped address; masked in fma1
    r.q0[u] = ld_nt(rw.w0 + cidx);
    r.q1[u] = ld_nt(rw.w1 + cidx);
    const int gi = (cidx << 4) >> gshift;
    r.g0[u] = rw.sc0[gi];
    r.g1[u] = rw.sc1[gi];
    __builtin_amdgcn_sched_barrier(0);  // see the fp32 load_u
  }
  __device__ __forceinline__ void fma1(const Regs& r, const f32x4* xs, int c0, int lim, int lane, int u, float& a0,
                                       float& a1) const {
    // lanes past the end: unit 0 and a zeroed group scale (kh_gemv.h: the int8 fma_u)
    const int idx = c0 + u * KH_WAVE + lane;
    const bool in = idx < lim;
    const int ci = in ? idx : 0;
    const int plane = Mc + 1;
    const f32x4 x0 = xs[ci], x1 = xs[plane + ci], x2 = xs[2 * plane + ci], x3 = xs[3 * plane + ci];
    float t0 = 0.f, t1 = 0.f;
    t0 = dot4_q4<0>(r.q0[u].x, x0, t0);
    t0 = dot4_q4<1>(r.q0[u].x, x1, t0);
    t0 = dot4_q4<0>(r.q0[u].y, x2, t0);
    t0 = dot4_q4<1>(r.q0[u].y, x3, t0);
    t1 = dot4_q4<0>(r.q1[u].x, x0, t1);
    t1 = dot4_q4<1>(r.q1[u].x, x1, t1);
    t1 = dot4_q4<0>(r.q1[u].y, x2, t1);
    t1 = dot4_q4<1>(r.q1[u].y, x3, t1);
    a0 = __builtin_fmaf(in ? r.g0[u] : 0.f, t0, a0);
    a1 = __builtin_fmaf(in ? r.g1[u] : 0.f, t1, a1);
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

// The decode GEMV kernels on the copy: KhLin::w of their arguments points into the 4-bit arena, everything else (the
// group scales in the image, norm weights, sin/cos, vectors) is what the int8 launch passes.  The int8 kernels' LDS
// layout, refill policy and launch bounds.
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_qkv_q4(const KhQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  qkv_body<GemvQ4<U>, true, MAXV, SPLIT>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_gemv_res_q4(const KhGemvResArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  f32x4* xs = (f32x4*)smem_raw;
  Stager<false, true, MAXV> st(a.vec, nullptr, a.M);
  gemv_res_body<GemvQ4<U>, SPLIT>(a, st, xs, lds_red_ptr<true>(xs, a.M));
  KH_STAMP_FLUSH();
}
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_wo_comb_q4(const KhWoCombArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  wo_comb_body<GemvQ4<U>, true, MAXV, SPLIT>(a, (f32x4*)smem_raw);
}
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_ffn13_q4(const KhFfn13Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  ffn13_body<GemvQ4<U>, true, MAXV>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_cls_q4(const KhClsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  KH_STAMP_INIT();
  cls_body<GemvQ4<U>, true, MAXV>(a, (f32x4*)smem_raw);
  KH_STAMP_FLUSH();
}
