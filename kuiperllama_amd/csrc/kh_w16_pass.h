// kh_w16_pass.h — the B-token passes (kh_prefill.h, kh_seq.h) of a W16 model on the 16-bit copy of its matrices
// (DESIGN 3.1c): prefill, scoring, verify and the sequence-slot passes read half the weight bytes and leave the bits
// of the fp32 pass.  The bodies are kh_prefill.h's own text over the view GemvW16<U> (kh_w16.h): a lane owns the
// columns it owns in Gemv<false, U>, the weights come back by a shift or a mask and the FMAs run in the fp32
// overload's order.  The staged vectors use the plain fp32 LDS layout, so pf_lds_bytes(false, ...) holds.
// Replaces nothing in the reference (it streams fp32: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-44).
#pragma once
#include "kh_prefill.h"
#include "kh_seq.h"
#include "kh_w16.h"

// 8-byte loads per row in flight per lane.  A lane's columns do not depend on U, so the value changes no bit: 4 keeps
// the fp32 pass's instruction count at half the bytes in flight, 8 would keep the bytes in flight at RegsF32<4>'s
// register cost.
#ifndef KH_PF_U_W16  // build.py --variant: the A/B of the two values (tools/w16_pass_ab.py)
#define KH_PF_U_W16 4
#endif

// B-token FMA of one W16 register chunk: the two rows' words of a slot are widened ONCE (bit operations, no convert
// instruction) and reused by all B tokens, as the int8 overload reuses its converted tile; per token the two fma4 of
// the fp32 overload, in its order and under its guard (GemvW16::load clamps the address of the lanes it skips).
// (FMT is deduced from the tile; for KH_W16_F16 the widening is four exact conversions per row, once per slot as well.)
template <int U, int B, int FMT>
__device__ __forceinline__ void fma_chunk_b(const RegsW16<U, FMT>& r, const f32x4* xs, int xstride, int c0, int M4,
                                            int lane, float (&a0)[B], float (&a1)[B]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int idx = c0 + u * KH_WAVE + lane;
    if (idx < M4) {
      const f32x4 w0 = GemvW16<U, FMT>::widen(r.v0[u]);
      const f32x4 w1 = GemvW16<U, FMT>::widen(r.v1[u]);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const f32x4 xv = xs[(size_t)b * xstride + idx];
        a0[b] = fma4(w0, xv, a0[b]);
        a1[b] = fma4(w1, xv, a1[b]);
      }
    }
  }
}

// The twins of k_pf_qkv, k_seq_qkv, k_pf_ffn13, k_pf_gemv_res and k_pf_cls: KhLin::w of their arguments points into
// the 16-bit arena, everything else is what the fp32 launch passes.
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_qkv_w16(const KhPfQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_qkv_body<GemvW16<KH_PF_U_W16>, SPLIT, B>(a, PfRunAddr{a.pos0, a.nvalid}, smem_raw);
}
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_seq_qkv_w16(const KhSeqQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_qkv_body<GemvW16<KH_PF_U_W16>, SPLIT, B>(a.a, PfLaneAddr{a.lanes}, smem_raw);
}
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_ffn13_w16(const KhPfFfn13Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_ffn13_body<GemvW16<KH_PF_U_W16>, B>(a, smem_raw);
}
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_gemv_res_w16(const KhPfGemvResArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_gemv_res_body<GemvW16<KH_PF_U_W16>, SPLIT, B>(a, smem_raw);
}
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_cls_w16(const KhPfClsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_cls_body<GemvW16<KH_PF_U_W16>, B>(a, smem_raw);
}

// The same five on an fp16-format copy (KH_FLAG_W16_F16): the bodies and instantiation lists of the twins above on
// GemvW16<KH_PF_U_W16, KH_W16_F16>.  Stems of their own, so the _w16 names and sets stay what they were.
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_qkv_h16(const KhPfQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_qkv_body<GemvW16<KH_PF_U_W16, KH_W16_F16>, SPLIT, B>(a, PfRunAddr{a.pos0, a.nvalid}, smem_raw);
}
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_seq_qkv_h16(const KhSeqQkvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_qkv_body<GemvW16<KH_PF_U_W16, KH_W16_F16>, SPLIT, B>(a.a, PfLaneAddr{a.lanes}, smem_raw);
}
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_ffn13_h16(const KhPfFfn13Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_ffn13_body<GemvW16<KH_PF_U_W16, KH_W16_F16>, B>(a, smem_raw);
}
template <int SPLIT, int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_gemv_res_h16(const KhPfGemvResArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_gemv_res_body<GemvW16<KH_PF_U_W16, KH_W16_F16>, SPLIT, B>(a, smem_raw);
}
template <int B>
__global__ __launch_bounds__(KH_WG_MAX) void k_pf_cls_h16(const KhPfClsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  pf_cls_body<GemvW16<KH_PF_U_W16, KH_W16_F16>, B>(a, smem_raw);
}
