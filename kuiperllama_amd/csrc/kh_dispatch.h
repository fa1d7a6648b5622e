// kh_dispatch.h — from a run-time launch shape to one compiled kernel instantiation, and the one helper that
// launches it.  Host code only.
//   KhVals<4, 2, 1, 0>   the values one template parameter of a kernel is compiled for: each kernel's launch site
//                        states its lists once, and the dispatch, the LDS opt-in walk and the shape-hook validators
//                        all read them (has / each / kh_pick)
//   kh_pick(list, v, f)  calls f(std::integral_constant<int, V>) for the listed V that equals v, the LAST listed one
//                        when none does (the instantiation an unlisted value falls back to); kh_pick_ge takes the
//                        first listed V <= v instead (lists in descending order: "u >= 8 -> 8, >= 4 -> 4, else 2")
//   kh_launch(KH_KERNEL(k_gemv_res, Q, U, MV, SP), grid, wg, lds, stream, args...)
//                        names the instantiation in the launch log (hook KH_LAUNCH_LOG, kh_common.h) and launches it
// Replaces nothing in the reference (its kernels are not templated on the launch shape).
#pragma once
#include <initializer_list>
#include <string>
#include <type_traits>

#include "kh_common.h"

namespace khm {

template <int... Vs>
struct KhVals {
  static constexpr bool has(int v) { return ((v == Vs) || ...); }
  template <class F>
  static void each(F&& f) {
    (f(std::integral_constant<int, Vs>{}), ...);
  }
};

template <int V0, int... Vs, class F>
void kh_pick(KhVals<V0, Vs...>, int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0)
    f(std::integral_constant<int, V0>{});
  else if (v == V0)
    f(std::integral_constant<int, V0>{});
  else
    kh_pick(KhVals<Vs...>{}, v, f);
}
template <int V0, int... Vs, class F>
void kh_pick_ge(KhVals<V0, Vs...>, int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0)
    f(std::integral_constant<int, V0>{});
  else if (v >= V0)
    f(std::integral_constant<int, V0>{});
  else
    kh_pick_ge(KhVals<Vs...>{}, v, f);
}
template <class F>
void kh_pick_bool(bool b, F&& f) {
  if (b)
    f(std::true_type{});
  else
    f(std::false_type{});
}

// The instantiations each decode GEMV kernel is compiled for, stated once: the dispatch of kh_model_step.hip and
// kh_model_w16.hip, the LDS opt-in of configure_step_kernels and the KH_SHAPE_* validator of pick_shape all read these
// lists.  U: 16-byte loads per row in flight per lane (kh_pick_ge: u >= 8 -> 8, >= 4 -> 4, else 2); MV: in-register
// staging depth (kh_stage_maxv of the input length) and SP: waves sharing one row pair (kh_pick: an unlisted value
// takes the last one listed).
template <bool Q>
using FusedU = std::conditional_t<Q, KhVals<4, 2>, KhVals<8, 4, 2>>;  // k_qkv, k_gemv_res as wo, k_wo_comb, k_ffn13, k_cls
template <bool Q>
using GemvResU = std::conditional_t<Q, KhVals<4, 3, 2>, KhVals<8, 4, 2>>;  // k_gemv_res as w2 (pick_shape, u3)
using FusedMV = KhVals<4, 2, 1, 0>;
using GemvResMV = KhVals<6, 4, 2, 1, 0>;  // w2 only: the 6-deep staging for hidden-sized inputs (wo's 6 runs as 0)
using WoCombMV = KhVals<2, 4>;
using QkvSP = KhVals<2, 1>;  // k_qkv's shape is split at most twice (plan_decode_shapes: max_split 2)
using GemvResSP = KhVals<4, 2, 1>;  // k_gemv_res, k_wo_comb
using NoSP = KhVals<1>;             // k_ffn13, k_cls
// f(Q, U, MV, SP) with the compile-time values a launch shape selects from a kernel's lists
template <template <bool> class US, class MVS, class SPS, class F>
void pick_fused(bool quant, int u, int mv, int sp, F&& f) {
  kh_pick_bool(quant, [&](auto Q) {
    kh_pick_ge(US<decltype(Q)::value>{}, u, [&](auto U) {
      kh_pick(MVS{}, mv, [&](auto MV) { kh_pick(SPS{}, sp, [&](auto SP) { f(Q, U, MV, SP); }); });
    });
  });
}

// one template argument of a launched kernel as the launch log spells it: "true" / "false" or a decimal number
struct KhTArg {
  int v;
  bool is_bool;
  KhTArg(bool b) : v(b), is_bool(true) {}
  KhTArg(int i) : v(i), is_bool(false) {}
  template <class T, T V>
  KhTArg(std::integral_constant<T, V>) : KhTArg(V) {}
};
// The kernel, its name and its template arguments for kh_launch, from ONE spelling of each: the log cannot name
// another instantiation than the one launched.
#define KH_KERNEL(K, ...) K<__VA_ARGS__>, #K, {__VA_ARGS__}

// Log off: one relaxed flag read, no string is built.  prep(kernel, grid) runs between the log entry and the launch -
// what a launch site keeps per (device, kernel), such as an LDS opt-in or a grid clipped to one resident round - and
// may refuse the launch (false).
template <class P, class K, class... A>
bool kh_launch_prep(P&& prep, K kernel, const char* stem, std::initializer_list<KhTArg> targs, dim3 grid, int wg,
                    size_t lds, hipStream_t stream, const A&... args) {
  if (g_launch_log_on.load(std::memory_order_relaxed)) {
    std::string n = stem;
    char sep = '<';
    for (const KhTArg& t : targs) {
      n += sep;
      n += t.is_bool ? (t.v ? "true" : "false") : std::to_string(t.v);
      sep = ',';
    }
    launch_log_add((n + '>').c_str());
  }
  if (!prep(kernel, grid)) return false;
  hipLaunchKernelGGL(kernel, grid, dim3(wg), lds, stream, args...);
  return true;
}
template <class K, class... A>
void kh_launch(K kernel, const char* stem, std::initializer_list<KhTArg> targs, dim3 grid, int wg, size_t lds,
               hipStream_t stream, const A&... args) {
  (void)kh_launch_prep([](K, dim3&) { return true; }, kernel, stem, targs, grid, wg, lds, stream, args...);
}

}  // namespace khm
