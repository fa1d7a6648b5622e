// kh_copy_launch.h — the decode GEMV launches on a narrow exact copy of the matrices, written once for the three sources
// a launch can stream from: the 16-bit copy in bf16 format (KH_SRC_BF16 -> the _w16 kernels of kh_w16.h), the same copy
// in fp16 format (KH_SRC_F16 -> the _h16 kernels) and the 4-bit copy of an int8 model (KH_SRC_Q4 -> the _q4 kernels of
// kh_q4.h).  Host code only.  Each launch is the image's launch of kh_model_step.hip with the same shape (split, u, grid,
// wg - a shape forced through KH_SHAPE_* included) on the twin of its kernel, so the bits do not change (DESIGN 3.1c,
// 3.1d).  A translation unit instantiates ONE source (kh_model_w16.hip bf16, kh_model_h16.hip fp16, kh_model_q4.hip
// q4: KH_COPY_LAUNCHES at the end); the kernels of the others are named here and compiled there.
// Replaces nothing in the reference (it streams the image's weights: kuiper/source/op/kernels/cuda/matmul_kernel.cu:8-87).
#pragma once
#include "kh_dispatch.h"
#include "kh_w16.h"
#include "kh_model_internal.h"

// The _q4 kernels by name only (kh_q4.h: a unit that includes it compiles its k_q4_build, and only the two units that
// instantiate kernels on the view - kh_model_q4.hip, kh_model_q4_pass.hip - are to)
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_qkv_q4(const KhQkvArgs a);
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_gemv_res_q4(const KhGemvResArgs a);
template <int U, int MAXV, int SPLIT>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_wo_comb_q4(const KhWoCombArgs a);
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_ffn13_q4(const KhFfn13Args a);
template <int U, int MAXV>
__global__ __launch_bounds__(KH_WG_MAX, 4) void k_cls_q4(const KhClsArgs a);

namespace khm {

// What a twin streams: a format of the 16-bit copy (kh_w16.h's numbers), or the 4-bit copy
enum { KH_SRC_BF16 = KH_W16_BF16, KH_SRC_F16 = KH_W16_F16, KH_SRC_Q4 = 2 };
// the image under a source is int8: the QUANT argument of the instantiation lists and of the LDS layouts
template <int SRC>
inline constexpr bool kh_src_quant = SRC == KH_SRC_Q4;

// ---- kh_model_w16.hip: what the copies share besides their launches ------------------------------------
// k_w16_build, k_h16_build, k_q4_build: n work items of a matrix, *flag set where a value is not exact in the copy
typedef void (*KhCopyBuildKernel)(const u32x4* src, u32x2* dst, size_t n, uint32_t* flag);
typedef size_t (*KhCopyMatBytes)(size_t elems);  // bytes of a matrix of `elems` elements in the copy, unpadded
// bytes of a copy of the 7 * layers + 1 matrices, each padded to 256 bytes
size_t copy_bytes(int dim, int hidden_dim, int kv_dim, int vocab_size, int layer_num, KhCopyMatBytes mat_bytes);
// One pass of a build kernel (per_item elements per work item) over every matrix into w's arena of `bytes` bytes, made
// here by the first pass: w.layers, w.cls, w.build_us += its time; *first = the first inexact tensor (-1: none).
// -> KH_OK or a HIP / KH error, w left for the caller to release
int copy_build(kh_model* m, kh_model::WCopy& w, KhCopyBuildKernel kernel, KhCopyMatBytes mat_bytes, int per_item,
               size_t bytes, int* first);
void copy_release(kh_model::WCopy& w);  // frees the arena; no class runs on the copy afterwards

// go(KH_KERNEL(<stem>_w16 or <stem>_h16, ...)) by the format: one spelling of the stem and of the template arguments
#define KH_W16_TWIN(FMT, go, K, ...)          \
  do {                                        \
    if constexpr (FMT == KH_W16_F16)          \
      go(KH_KERNEL(K##_h16, __VA_ARGS__));    \
    else                                      \
      go(KH_KERNEL(K##_w16, __VA_ARGS__));    \
  } while (0)
// ... or <stem>_q4, by the source (the decode launches below and the B-token pass launches of kh_pf_launch.h)
#define KH_COPY_TWIN(SRC, go, K, ...)         \
  do {                                        \
    if constexpr (SRC == KH_SRC_Q4)           \
      go(KH_KERNEL(K##_q4, __VA_ARGS__));     \
    else                                      \
      KH_W16_TWIN(SRC, go, K, __VA_ARGS__);   \
  } while (0)

// f(U, MV, SP) from the lists of a kernel at ONE level of QUANT (pick_fused without that level: a twin has no form for
// the other kind of image, and walking both levels would compile it for the other's values of U as well)
template <class US, class MVS, class SPS, class F>
static void pick_copy(int u, int mv, int sp, F&& f) {
  kh_pick_ge(US{}, u, [&](auto U) {
    kh_pick(MVS{}, mv, [&](auto MV) { kh_pick(SPS{}, sp, [&](auto SP) { f(U, MV, SP); }); });
  });
}
// the logged launch of one twin on a decode shape
template <class A>
struct CopyGo {
  const kh_model::Shape& sh;
  size_t lds;
  hipStream_t stream;
  const A& a;
  template <class K>
  void operator()(K kernel, const char* stem, std::initializer_list<KhTArg> targs) const {
    kh_launch(kernel, stem, targs, sh.grid, sh.wg, lds, stream, a);
  }
};
// the copy a source's launches read: its per-layer table and its classifier
template <int SRC>
static const kh_model::WCopy& copy_of(const kh_model* m) {
  if constexpr (kh_src_quant<SRC>)
    return m->q4;
  else
    return m->w16;
}

// >64 KiB dynamic-LDS opt-in of the gemv_res twin as w2 (configure_step_kernels does it for k_gemv_res)
template <int SRC>
void copy_configure(const kh_model* m) {
  constexpr bool Q = kh_src_quant<SRC>;
  const size_t lds_need = fused_lds_bytes(Q, m->cfg.hidden_dim);
  if (lds_need <= 64 * 1024) return;
  auto opt_in = [&](auto kernel, const char*, std::initializer_list<KhTArg>) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_need);
  };
  GemvResU<Q>::each([&](auto U) {
    GemvResSP::each([&](auto SP) {
      KhVals<0, 6>::each([&](auto MV) { KH_COPY_TWIN(SRC, opt_in, k_gemv_res, U, MV, SP); });
    });
  });
}

// `img`: the arguments as the image's launch fills them; the matrices are replaced by their copies here
template <int SRC>
void copy_qkv(kh_model* m, int l, const KhQkvArgs& img) {
  constexpr bool Q = kh_src_quant<SRC>;
  const kh_config& c = m->cfg;
  KhQkvArgs a = img;
  const kh_model::WCopy::Layer& W = copy_of<SRC>(m).layers[(size_t)l];
  a.wq.w = W.wq;
  a.wk.w = W.wk;
  a.wv.w = W.wv;
  const CopyGo<KhQkvArgs> go{m->sh_qkv, fused_lds_bytes(Q, c.dim), m->stream, a};
  pick_copy<FusedU<Q>, FusedMV, QkvSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), go.sh.split,
                                       [&](auto U, auto MV, auto SP) { KH_COPY_TWIN(SRC, go, k_qkv, U, MV, SP); });
}
template <int SRC>
void copy_wo(kh_model* m, int l, const KhGemvResArgs& img) {
  constexpr bool Q = kh_src_quant<SRC>;
  const kh_config& c = m->cfg;
  KhGemvResArgs a = img;
  a.w.w = copy_of<SRC>(m).layers[(size_t)l].wo;
  const CopyGo<KhGemvResArgs> go{m->sh_wo, fused_lds_bytes(Q, c.dim), m->stream, a};
  pick_copy<FusedU<Q>, FusedMV, GemvResSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), go.sh.split,
                                           [&](auto U, auto MV, auto SP) { KH_COPY_TWIN(SRC, go, k_gemv_res, U, MV, SP); });
}
template <int SRC>
void copy_wo_comb(kh_model* m, int l, const KhWoCombArgs& img) {
  constexpr bool Q = kh_src_quant<SRC>;
  const kh_config& c = m->cfg;
  KhWoCombArgs a = img;
  a.g.w.w = copy_of<SRC>(m).layers[(size_t)l].wo;
  const CopyGo<KhWoCombArgs> go{m->sh_wo, comb_lds_bytes(Q, c.dim, c.head_num), m->stream, a};
  pick_copy<FusedU<Q>, WoCombMV, GemvResSP>(go.sh.u, c.dim <= 2 * 4 * go.sh.wg ? 2 : 4, go.sh.split,
                                            [&](auto U, auto MV, auto SP) { KH_COPY_TWIN(SRC, go, k_wo_comb, U, MV, SP); });
}
template <int SRC>
void copy_ffn13(kh_model* m, int l, const KhFfn13Args& img) {
  constexpr bool Q = kh_src_quant<SRC>;
  const kh_config& c = m->cfg;
  KhFfn13Args a = img;
  a.w1.w = copy_of<SRC>(m).layers[(size_t)l].w1;
  a.w3.w = copy_of<SRC>(m).layers[(size_t)l].w3;
  const CopyGo<KhFfn13Args> go{m->sh_ffn, fused_lds_bytes(Q, c.dim), m->stream, a};
  pick_copy<FusedU<Q>, FusedMV, NoSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), 1,
                                      [&](auto U, auto MV, auto) { KH_COPY_TWIN(SRC, go, k_ffn13, U, MV); });
}
template <int SRC>
void copy_w2(kh_model* m, int l, const KhGemvResArgs& img) {
  constexpr bool Q = kh_src_quant<SRC>;
  const kh_config& c = m->cfg;
  KhGemvResArgs a = img;
  a.w.w = copy_of<SRC>(m).layers[(size_t)l].w2;
  const CopyGo<KhGemvResArgs> go{m->sh_w2, fused_lds_bytes(Q, c.hidden_dim), m->stream, a};
  pick_copy<GemvResU<Q>, GemvResMV, GemvResSP>(go.sh.u, kh_stage_maxv(c.hidden_dim, go.sh.wg), go.sh.split,
                                               [&](auto U, auto MV, auto SP) { KH_COPY_TWIN(SRC, go, k_gemv_res, U, MV, SP); });
}
template <int SRC>
void copy_cls(kh_model* m, const KhClsArgs& img) {
  constexpr bool Q = kh_src_quant<SRC>;
  const kh_config& c = m->cfg;
  KhClsArgs a = img;
  a.wcls.w = copy_of<SRC>(m).cls;
  const CopyGo<KhClsArgs> go{m->sh_cls, cls_lds_bytes(Q, c.dim), m->stream, a};
  pick_copy<FusedU<Q>, FusedMV, NoSP>(go.sh.u, kh_stage_maxv(c.dim, go.sh.wg), 1,
                                      [&](auto U, auto MV, auto) { KH_COPY_TWIN(SRC, go, k_cls, U, MV); });
}

// The seven above for one source: `KH_COPY_LAUNCHES(, SRC)` in the unit that compiles the source's kernels.  Every unit
// sees the other sources as `extern`, so that naming their launches (kh_model_w16.hip routes to all three) compiles none.
#define KH_COPY_LAUNCHES(EXTERN, SRC)                                                   \
  EXTERN template void copy_configure<SRC>(const kh_model*);                            \
  EXTERN template void copy_qkv<SRC>(kh_model*, int, const KhQkvArgs&);                 \
  EXTERN template void copy_wo<SRC>(kh_model*, int, const KhGemvResArgs&);              \
  EXTERN template void copy_wo_comb<SRC>(kh_model*, int, const KhWoCombArgs&);          \
  EXTERN template void copy_ffn13<SRC>(kh_model*, int, const KhFfn13Args&);             \
  EXTERN template void copy_w2<SRC>(kh_model*, int, const KhGemvResArgs&);              \
  EXTERN template void copy_cls<SRC>(kh_model*, const KhClsArgs&)
KH_COPY_LAUNCHES(extern, KH_SRC_BF16);
KH_COPY_LAUNCHES(extern, KH_SRC_F16);
KH_COPY_LAUNCHES(extern, KH_SRC_Q4);

}  // namespace khm
