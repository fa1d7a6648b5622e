// kh_q4_pass.h — the B-token passes (kh_prefill.h, kh_seq.h) of a Q4 model on the packed 4-bit copy of its matrices
// (DESIGN 3.1d): prefill, scoring, verify and the sequence-slot passes of the classes in the pass mask read half the
// weight bytes and leave the bits of the int8 pass.  The bodies are kh_prefill.h's own text over the view GemvQ4<U>
// (kh_q4.h): a lane owns the columns it owns in Gemv<true, U>, reads the group scales where the image keeps them, the
// nibbles come back by two exact instructions and the FMAs run in the int8 overload's order.  The staged vectors use
// the int8 view's four-plane LDS layout (GemvQ4::kLayoutQ8), so pf_lds_bytes(true, ...) holds.
// Replaces nothing in the reference (it streams int8: kuiper/source/op/kernels/cuda/matmul_kernel.cu:56-87).
#pragma once
#include "kh_prefill.h"
#include "kh_q4.h"
#include "kh_seq.h"

// 8-byte loads per row in flight per lane.  A lane's columns and its accumulation order do not depend on U, so the
// value changes no bit: 2 keeps the int8 pass's instruction count at half the bytes in flight, 4 keeps its bytes in
// flight (the raw tile is still smaller than the int8 one).
#ifndef KH_PF_U_Q4  // build.py --variant: the A/B of the two values (tools/q4_pass_ab.py)
#define KH_PF_U_Q4 2
#endif

// the sixteen nibbles of a slot's two words as floats, in column order (cvt16_i8's place in the int8 overload)
__device__ __forceinline__ void cvt16_q4(const u32x2& q, float (&w)[16]) {
  w[0] = q4_val<0>(q.x);
  w[1] = q4_val<1>(q.x);
  w[2] = q4_val<2>(q.x);
  w[3] = q4_val<3>(q.x);
  w[4] = q4_val<4>(q.x);
  w[5] = q4_val<5>(q.x);
  w[6] = q4_val<6>(q.x);
  w[7] = q4_val<7>(q.x);
  w[8] = q4_val<0>(q.y);
  w[9] = q4_val<1>(q.y);
  w[10] = q4_val<2>(q.y);
  w[11] = q4_val<3>(q.y);
  w[12] = q4_val<4>(q.y);
  w[13] = q4_val<5>(q.y);
  w[14] = q4_val<6>(q.y);
  w[15] = q4_val<7>(q.y);
}

// B-token FMA of one Q4 register chunk: the int8 overload's text with the conversion replaced - the two rows' nibbles
// of a slot become floats ONCE and are reused by all B tokens; per token dot16 over the token's four planes, then
// fma(scale, t, a), under the int8 overload's guard and with its sched_barriers (GemvQ4::load clamps the address of
// the lanes it skips).
template <int U, int B>
__device__ __forceinline__ void fma_chunk_b(const RegsQ4<U>& r, const f32x4* xs, int xstride, int c0, int M16,
                                            int plane, int lane, float (&a0)[B], float (&a1)[B]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int idx = c0 + u * KH_WAVE + lane;
    if (idx < M16) {
      float w0[16], w1[16];
      cvt16_q4(r.q0[u], w0);
      cvt16_q4(r.q1[u], w1);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const f32x4* xb = xs + (size_t)b * xstride;
        const f32x4 x0 = xb[idx], x1 = xb[plane + idx], x2 = xb[2 * plane + idx], x3 = xb[3 * plane + idx];
        a0[b] = __builtin_fmaf(r.g0[u], dot16(w0, x0, x1, x2, x3), a0[b]);
        a1[b] = __builtin_fmaf(r.g1[u], dot16(w1, x0, x1, x2, x3), a1[b]);
        // keep the next token's LDS reads below this token's FMAs (bounds the live operands)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The twins of k_pf_qkv, k_seq_qkv, k_pf_ffn13, k_pf_gemv_res and k_pf_cls: KhLin::w of their arguments points into
// the 4-bit arena, everything else (the group scales in the image included) is what the int8 launch passes.  The int8
// kernels' launch bounds and instantiation lists (kh_pf_launch.h).
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_qkv_q4(const KhPfQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_qkv_body<GemvQ4<KH_PF_U_Q4>, SPLIT, B>(a, PfRunAddr{a.pos0, a.nvalid}, smem_raw);
}
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_seq_qkv_q4(const KhSeqQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_qkv_body<GemvQ4<KH_PF_U_Q4>, SPLIT, B>(a.a, PfLaneAddr{a.lanes}, smem_raw);
}
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_ffn13_q4(const KhPfFfn13Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_ffn13_body<GemvQ4<KH_PF_U_Q4>, B>(a, smem_raw);
}
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_gemv_res_q4(const KhPfGemvResArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_gemv_res_body<GemvQ4<KH_PF_U_Q4>, SPLIT, B>(a, smem_raw);
}
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_cls_q4(const KhPfClsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_cls_body<GemvQ4<KH_PF_U_Q4>, B>(a, smem_raw);
}
