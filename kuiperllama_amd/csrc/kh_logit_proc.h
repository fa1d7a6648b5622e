// kh_logit_proc.h — repetition / presence / frequency penalties and logit bias on the device (gfx950).
//
// Semantics (include/kuiper_hip.h, kh_penalties; tests/logit_proc_ref.py is the numpy float32 statement of the same):
//   window = positions [max(0, p + 1 - last_n), p] (last_n = 0: [0, p]); c(v) = window positions whose fed token is v
//   (tokens outside [0, V) are ignored; a never-written slot holds -1).  For every v with c(v) > 0, once, in fp32,
//   every operation rounded once:  l = l > 0 ? l / r : l * r  (r != 1), then  l = l - (float(c) * frequency + presence)
//   (unless both are 0).  Then l[id] += b for every bias entry.
//
// One workgroup of 1024 threads, time proportional to the window (never to the vocabulary), on a table of V int32
// counters in global memory that is zero before and after:
//   phase 1  every window entry: atomicAdd(&cnt[t], 1)
//   barrier
//   phase 2  every window entry: c = atomicExch(&cnt[t], 0); the one thread that gets c > 0 owns token t and rewrites
//            logits[t] with the full count - which thread that is does not matter, and the table is re-armed
//   barrier, then the bias entries (ids are distinct: one thread each).
// __syncthreads() is the workgroup-scope fence that orders the global atomics and stores of one phase before the
// reads of the next.  The core needs no LDS of its own, so the step's last launch (kh_logprobs.h: k_sample_proc) calls
// it ahead of the pick on whatever shared memory it has.  No scratch, no inline assembly, plain vector stores.
#pragma once
#include <cmath>

#include "kh_common.h"

#define KH_PROC_THREADS 1024

// the parameters as the kernels read them (the model keeps one copy on the device)
struct KhProcParams {
  float repetition, presence, frequency;
  int32_t last_n;
  int32_t n_bias;
};

// host: parameters valid (repetition finite and > 0, presence / frequency finite, last_n >= 0)
static inline bool kh_penalties_valid(const kh_penalties* p) {
  return p && std::isfinite(p->repetition) && p->repetition > 0.f && std::isfinite(p->presence) &&
         std::isfinite(p->frequency) && p->last_n >= 0;
}
static inline bool kh_penalties_neutral(const kh_penalties* p) {
  return !p || (p->repetition == 1.f && p->presence == 0.f && p->frequency == 0.f);
}

// one penalised logit: c > 0 occurrences in the window
__device__ __forceinline__ float kh_proc_penalise(float l, int c, const KhProcParams& p) {
  if (p.repetition != 1.f) l = l > 0.f ? __fdiv_rn(l, p.repetition) : __fmul_rn(l, p.repetition);
  if (p.presence != 0.f || p.frequency != 0.f)
    l = __fsub_rn(l, __fadd_rn(__fmul_rn((float)c, p.frequency), p.presence));
  return l;
}

// The processing core, in place on logits[0..n): tokens[j] = token fed at position j (read for the window that ends at
// `pos`), cnt[n] all zero (and all zero again afterwards).  Called by all KH_PROC_THREADS threads of the workgroup
// with uniform arguments; ends with a barrier, so every thread may read the processed logits afterwards.
__device__ inline void kh_logit_process_core(float* logits, int n, const int32_t* tokens, int pos,
                                             const KhProcParams& p, const int32_t* bias_ids, const float* bias,
                                             int32_t* cnt) {
  if (p.repetition != 1.f || p.presence != 0.f || p.frequency != 0.f) {
    const int lo = p.last_n > 0 && pos + 1 > p.last_n ? pos + 1 - p.last_n : 0;
    for (int j = lo + (int)threadIdx.x; j <= pos; j += KH_PROC_THREADS) {
      const int t = tokens[j];
      if ((unsigned)t < (unsigned)n) atomicAdd(&cnt[t], 1);
    }
    __syncthreads();
    for (int j = lo + (int)threadIdx.x; j <= pos; j += KH_PROC_THREADS) {
      const int t = tokens[j];
      if ((unsigned)t < (unsigned)n) {
        const int c = atomicExch(&cnt[t], 0);
        if (c > 0) logits[t] = kh_proc_penalise(logits[t], c, p);
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < p.n_bias; i += KH_PROC_THREADS) {
    const int id = bias_ids[i];
    if ((unsigned)id < (unsigned)n) logits[id] = __fadd_rn(logits[id], bias[i]);
  }
  __syncthreads();
}

// ---- operator
static __global__ __launch_bounds__(KH_PROC_THREADS) void k_logit_process(float* logits, int n, const int32_t* tokens,
                                                                           const int32_t* d_pos, int pos, KhProcParams p,
                                                                           const int32_t* bias_ids, const float* bias,
                                                                           int32_t* cnt) {
  kh_logit_process_core(logits, n, tokens, d_pos ? *d_pos : pos, p, bias_ids, bias, cnt);
}
