// mb_engine.hip — go / no-go prototype: ONE persistent launch per decoder layer
// (qkv -> attention -> wo -> ffn13 -> w2, batch 1, fp32) built as the MI355X guide describes its only
// measured persistent-kernel win (cdna_hip_programming.md §5.6; MI355X_MICROARCH.md price-list rows
// engine-vs-launches, prefetch-credit, ldsdma-fill, nt-weights, polling-cost, gather-pass), against the
// product's five hipGraph-captured launches per layer on the SAME weights, same box, outputs compared.
//
// Engine, per CU (256 workgroups x 256 threads, one per CU, ~156 KiB LDS):
//   wave 0      LOADER: walks this CU's share of the layer's weight rows in op order and pulls them into a
//               104 KiB LDS ring with global_load_lds_dwordx4 ... nt (1 KiB per instruction, no VGPRs),
//               up to 3 batches of 16 pieces in flight (vmcnt is 6 bits).  Weights do not depend on
//               activations, so it keeps running ACROSS the dependency edges until the ring is full:
//               while the consumers wait for a hand-off, the next op's rows arrive (prefetch-credit).
//   waves 1-3   CONSUMERS: take row pairs from the ring (ds_read_b128) against the activation vector in
//               LDS with the product's own per-lane order (lane l owns float4 idx0 + 64 k + l, the split
//               parts of pick_shape reduced separately with the same DPP butterfly and added in the same
//               order), so every GEMV stage is bit-identical to its product kernel.
//   hand-offs   8-byte {tag, value} granules, one agent-scope relaxed store each (global_store sc1), swept by
//               consumer waves with agent-scope relaxed loads until every tag carries this (token, layer,
//               edge); no flag, no fence, no atomic RMW, no grid barrier.  Tags derive from a device
//               counter bumped once per token, so graph replay needs no memset.
//   intra-CU    LDS words polled with s_sleep: pieces landed (loader -> consumers), first unreleased piece
//               per consumer (consumers -> loader), staged-vector epoch, per-op done marks.
// Every spin is bounded: on give-up a code lands in dbg[] and all waves of the workgroup leave.
// Attention runs inside the launch on (heads) CUs, three waves per head, positions < 256 only and head size
// 64 only in this prototype; its summation order is its own (compared with tolerance, the GEMV stages
// bit for bit).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/mb_engine.hip -o kuiperllama_amd/lib/mb_engine
//   mb_engine [1b|qwen|tiny] [pos] [reps]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../kuiperllama_amd/csrc/kh_fused.h"

namespace khm {
const char* dbg(const char*) { return nullptr; }
std::atomic<bool> g_launch_log_on{false};  // the launch log of launch_attn_decode stays off here
void launch_log_add(const char*) {}
}  // namespace khm

#define CK(x)                                                                       \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

// ------------------------------------------------------------------------------------------------
#define EN_NCU 256
#define EN_RING 104            // ring pieces of 1 KiB (104 + 32 + 16 + 4 KiB = 156 KiB of the 160)
#define EN_POLL_SLEEP 1        // s_sleep argument of the consumers' LDS polls (x 64 clocks)
#define EN_ACT_BYTES 32768     // staged activation vector (<= 8192 floats)
#define EN_XRAW_BYTES 16384    // residual stream after wo (<= 4096 floats)
#define EN_MISC_BYTES 4096
#define EN_LDS_BYTES (EN_RING * 1024 + EN_ACT_BYTES + EN_XRAW_BYTES + EN_MISC_BYTES)
#define EN_NCONS 3
#define EN_DEPTH 3             // loader batches (16 pieces) in flight

typedef unsigned long long u64;
// LDS through address-space-3 pointers ONLY: through a generic pointer every access is a flat_load that counts in
// vmcnt as well - the loader's polls would then wait for its own LDS-DMA queue
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) volatile uint32_t lds_vu32;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

enum { OP_QKV = 0, OP_WO = 1, OP_FFN = 2, OP_W2 = 3, N_WOPS = 4 };
enum { EDGE_QKV = 1, EDGE_ATT = 2, EDGE_X2 = 3, EDGE_H = 4 };
// misc words (u32)
enum {
  MW_FILLED = 0, MW_CUR0 = 1, /* 1..3 */ MW_ABORT = 4, MW_ACT = 5, MW_DONE0 = 6, /* 6..8 */
  MW_GATH = 9, MW_THIN = 10, MW_ATTQ = 11, MW_APART0 = 12, /* 12..14 */
  MW_F_AQ = 64,            // floats: q[64] k[64] v[64]
  MW_F_APART = 64 + 192,   // floats: 3 x 80: o[64] | M | L | pad   (16-byte aligned partials)
  MW_OPD = 512,            // words: OpD[N_WOPS]
};
// profile slots per CU (ticks of the 100 MHz real-time counter)
enum {
  PF_START = 0, PF_LD_OPEND0 = 1 /* 1..4: loader issued the op's last piece */, PF_LD_END = 5,
  PF_LD_SPACE = 6 /* accumulated: waiting for ring space */, PF_LD_VM = 7 /* accumulated: vmcnt waits */,
  PF_STAGE0 = 8 /* 8..11: consumer 0 begins staging op */, PF_READY0 = 12 /* 12..15: vector staged */,
  PF_ITEMS0 = 16 /* 16..19: consumer 0 finished its items of op */, PF_ATT_Q = 20, PF_ATT_DONE = 21, PF_END = 22,
  PF_FILLWAIT = 23 /* accumulated by consumer 0: waiting for pieces */, PF_N = 32
};
#define EN_TICK() __builtin_amdgcn_s_memrealtime()
// give-up codes
enum { GU_LOADER_SPACE = 1, GU_FILLED = 2, GU_ACT = 3, GU_DONE = 4, GU_GATHER = 5, GU_ATTQ = 6, GU_APART = 7 };

struct EngArgs {
  const float *wq, *wk, *wv, *wo, *w1, *w3, *w2;
  const float *bq, *bk, *bv;
  const float *att_norm, *ffn_norm;
  float* x;  // residual stream, in place
  float *kc, *vc;  // this layer's cache rows [cache_len, kv_dim]
  const float *sin_cache, *cos_cache;
  const int32_t* d_pos;
  const uint32_t* d_epoch;
  u64 *g_qkv, *g_att, *g_x2, *g_h;
  uint32_t* dbg;
  u64* prof;  // optional: [EN_NCU][32] s_memrealtime ticks (10 ns), see PF_*
  int dim, kv_dim, hidden, hs, heads, kv_heads, rope_mode, layer, n_layers;
  int split_qkv, split_wo, split_ffn, split_w2;
  float eps;
  int mode;  // ablations (timing only, results are garbage): 1 = loader alone, ignoring ring space; 2 = consumers only wait
             // for their pieces and release them; 3 = + the dot products, still no staging / hand-offs
};

struct OpD {
  int lo, n;      // this CU's items [lo, lo + n) of the op's global item list
  int ppr;        // 1 KiB pieces per weight row
  int M;          // floats per row
  int split;      // column parts reduced separately (pick_shape of the product kernel)
  uint32_t start; // first stream piece of the op in this CU's stream
};

__device__ __forceinline__ int ceil_div(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ void en_ops(const EngArgs& a, int cu, __attribute__((address_space(3))) OpD* d) {
  const int tot[N_WOPS] = {(a.dim + 2 * a.kv_dim) >> 1, a.dim >> 1, a.hidden, a.dim >> 1};
  const int Ms[N_WOPS] = {a.dim, a.dim, a.dim, a.hidden};
  const int sp[N_WOPS] = {a.split_qkv, a.split_wo, a.split_ffn, a.split_w2};
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < N_WOPS; ++k) {
    const int lo = (int)(((long)cu * tot[k]) >> 8), hi = (int)(((long)(cu + 1) * tot[k]) >> 8);  // EN_NCU == 256
    d[k].lo = lo;
    d[k].n = hi - lo;
    d[k].M = Ms[k];
    d[k].ppr = ceil_div(Ms[k] * 4, 1024);
    d[k].split = sp[k];
    d[k].start = s;
    s += (uint32_t)(hi - lo) * 2u * (uint32_t)d[k].ppr;
  }
}

// qkv work item -> (projection, rows, sin/cos column): the product's pairing (kh_fused.h::k_qkv)
__device__ __forceinline__ void qkv_decode(const EngArgs& a, int p, int& which, int& r0, int& r1, int& cidx) {
  const int npq = a.dim >> 1, npk = a.kv_dim >> 1, half = a.hs >> 1;
  int pp;
  if (p < npq) { which = 0; pp = p; }
  else if (p < npq + npk) { which = 1; pp = p - npq; }
  else { which = 2; pp = p - npq - npk; }
  if (which < 2 && a.rope_mode == KH_ROPE_HALF) {
    const int head = pp / half, j = pp - head * half;
    r0 = head * a.hs + j;
    r1 = r0 + half;
    cidx = 2 * j;
  } else {
    r0 = 2 * pp;
    r1 = r0 + 1;
    cidx = r0 % a.hs;
  }
}
__device__ __forceinline__ const float* row_ptr(const EngArgs& a, int op, int p, int sel) {
  if (op == OP_QKV) {
    int which, r0, r1, cidx;
    qkv_decode(a, p, which, r0, r1, cidx);
    const float* w = sel3(which, a.wq, a.wk, a.wv);  // select on VALUES (kh_fused.h::sel3)
    return w + (size_t)(sel ? r1 : r0) * a.dim;
  }
  if (op == OP_WO) return a.wo + (size_t)(2 * p + sel) * a.dim;
  if (op == OP_FFN) return sel3(sel, a.w1, a.w3, a.w3) + (size_t)p * a.dim;
  return a.w2 + (size_t)(2 * p + sel) * a.hidden;
}

// ---- LDS-DMA: 64 lanes x 16 B -> 1 KiB at lds_dst (wave-uniform byte address), non-temporal --------
__device__ __forceinline__ void dma_piece(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}

// n pieces of one row in ONE asm statement (tools/mb_dma.hip: 27.7 GB/s per CU from one wave, against 21.9 with a
// statement per piece): uniform row pointer in SGPRs + 32-bit lane offset, M0 bumped inside the loop, ring wrap
// by scalar select.  voff advances by 1 KiB per piece; dst is the ring byte address, updated.
__device__ __forceinline__ void dma_row(const void* base, unsigned voff, unsigned& dst, unsigned rbeg, unsigned rend,
                                        int n) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %[keep], m0\n"
      ".Lrow%=:\n\t"
      "s_mov_b32 m0, %[dst]\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %[voff], %[base] nt\n\t"
      "v_add_u32 %[voff], 0x400, %[voff]\n\t"
      "s_add_u32 %[dst], %[dst], 0x400\n\t"
      "s_cmp_eq_u32 %[dst], %[rend]\n\t"
      "s_cselect_b32 %[dst], %[rbeg], %[dst]\n\t"
      "s_sub_u32 %[n], %[n], 1\n\t"
      "s_cmp_lg_u32 %[n], 0\n\t"
      "s_cbranch_scc1 .Lrow%=\n\t"
      "s_mov_b32 m0, %[keep]"
      : [keep] "=&s"(keep), [voff] "+v"(voff), [dst] "+s"(dst), [n] "+s"(n)
      : [base] "s"(base), [rend] "s"(rend), [rbeg] "s"(rbeg)
      : "memory", "scc");
}

struct Ctx {
  lds_vu32* mw;  // misc words
  uint32_t* dbg;
  u64* prof;     // this CU's slots or null
  int lane, cu;
};
__device__ __forceinline__ void pf_set(const Ctx& c, int slot) {
  if (c.prof && c.lane == 0) c.prof[slot] = EN_TICK();
}
__device__ __forceinline__ void pf_add(const Ctx& c, int slot, u64 t0) {
  if (c.prof && c.lane == 0) c.prof[slot] += EN_TICK() - t0;
}
// a polled LDS word as a wave-uniform (scalar) value: conditions on it become s_cbranch, and whatever the loops
// carry stays in SGPRs
__device__ __forceinline__ uint32_t uword(const Ctx& c, int w) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)c.mw[w]);
}
__device__ __forceinline__ bool aborted(const Ctx& c) { return uword(c, MW_ABORT) != 0; }
__device__ __forceinline__ void give_up(const Ctx& c, uint32_t code, uint32_t info) {
  if (c.lane == 0) {
    c.mw[MW_ABORT] = 1;
    if (atomicCAS(&c.dbg[0], 0u, code | ((uint32_t)c.cu << 8)) == 0u) c.dbg[1] = info;
  }
}
#define EN_SPIN_MAX (1u << 22)
// wait until word w >= target (monotonic counters); false on abort / give-up
__device__ __forceinline__ bool wait_ge(const Ctx& c, int w, uint32_t target, uint32_t code) {
  for (uint32_t spins = 0;; ++spins) {
    if (uword(c, w) >= target) break;
    if ((spins & 15) == 15 && aborted(c)) return false;
    if (spins > EN_SPIN_MAX) {
      give_up(c, code, target);
      return false;
    }
    __builtin_amdgcn_s_sleep(EN_POLL_SLEEP);
  }
  asm volatile("" ::: "memory");  // data guarded by the word is re-read from LDS, not from registers
  return true;
}

// ================================= LOADER =======================================================
__device__ void en_loader(const EngArgs& a, const Ctx& c, const __attribute__((address_space(3))) OpD* d, unsigned ring_lds) {
  // every counter here is wave-uniform (SGPRs, s_cbranch)
  uint32_t q = 0, landed = 0, tail = 0;
  unsigned dst = ring_lds;
  const unsigned rbeg = ring_lds, rend = ring_lds + EN_RING * 1024u;
  int out = 0;  // pieces issued and not known landed
  u64 acc_space = 0, acc_vm = 0;  // profile: ticks blocked on ring space / in vmcnt waits (written once, at the end:
                                  // a read-modify-write of global memory here would drain the DMA queue)
  auto publish = [&](uint32_t upto) {
    landed = upto;
    if (c.lane == 0) c.mw[MW_FILLED] = upto;
  };
  auto drain = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    publish(q);
    out = 0;
  };
  for (int op = 0; op < N_WOPS; ++op) {
    const int ppr = __builtin_amdgcn_readfirstlane(d[op].ppr), rowb = __builtin_amdgcn_readfirstlane(d[op].M) * 4;
    const int n = __builtin_amdgcn_readfirstlane(d[op].n), lo = __builtin_amdgcn_readfirstlane(d[op].lo);
    const int full = rowb >> 10, rem = rowb & 1023;  // whole pieces of a row; bytes of the partial last piece
    for (int it = 0; it < n; ++it) {
      for (int sel = 0; sel < 2; ++sel) {
        const char* base = (const char*)row_ptr(a, op, lo + it, sel);
        const uint64_t bu = (uint64_t)base;
        base = (const char*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(bu >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((int)bu));
        // ring space for the whole row: piece q + ppr - 1 overwrites piece q + ppr - 1 - EN_RING
        if (a.mode != 1 && q + (uint32_t)ppr - tail > EN_RING) {
          u64 t_sp = 0;
          for (uint32_t spins = 0;; ++spins) {
            const uint32_t t0 = uword(c, MW_CUR0), t1 = uword(c, MW_CUR0 + 1), t2 = uword(c, MW_CUR0 + 2);
            tail = t0 < t1 ? (t0 < t2 ? t0 : t2) : (t1 < t2 ? t1 : t2);
            if (q + (uint32_t)ppr - tail <= EN_RING) break;
            if (spins == 0 && c.prof) t_sp = EN_TICK();
            if (landed != q) drain();  // blocked: everything issued so far becomes visible now
            if ((spins & 15) == 15 && aborted(c)) return;
            if (spins > EN_SPIN_MAX) {
              give_up(c, GU_LOADER_SPACE, q);
              return;
            }
            __builtin_amdgcn_s_sleep(4);
          }
          if (t_sp) acc_space += EN_TICK() - t_sp;
        }
        if (full) dma_row(base, (unsigned)c.lane * 16u, dst, rbeg, rend, full);
        if (rem) {  // lanes past the row end re-read its start; never consumed
          const unsigned vo = (unsigned)c.lane * 16u < (unsigned)rem ? (unsigned)full * 1024u + (unsigned)c.lane * 16u : 0u;
          dma_row(base, vo, dst, rbeg, rend, 1);
        }
        q += (uint32_t)ppr;
        out += ppr;
        // at most 32 pieces stay in flight (vmcnt counts 63; two batches of 16 reach the chip rate,
        // tools/mb_dma.hip): everything older has landed and is published row by row
        if (out > 32) {
          const u64 t_vm = c.prof ? EN_TICK() : 0;
          asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
          if (c.prof) acc_vm += EN_TICK() - t_vm;
          out = 32;
          publish(q - 32u);
        } else if (uword(c, MW_THIN)) {
          drain();  // a consumer wave of this CU is sweeping granules: nothing outstanding beside it
        }
      }
    }
    pf_set(c, PF_LD_OPEND0 + op);
  }
  drain();
  pf_set(c, PF_LD_END);
  if (c.prof && c.lane == 0) {
    c.prof[PF_LD_SPACE] = acc_space;
    c.prof[PF_LD_VM] = acc_vm;
  }
}

// ================================= CONSUMERS ====================================================
// sweep n granules (n <= EN_CHUNK) starting at g until every tag == tag; values -> dst[0..n) (LDS floats)
#define EN_CHUNK 2048
__device__ __forceinline__ bool gather_chunk(const Ctx& c, const u64* g, int n, uint32_t tag, lds_f32* dst) {
  for (uint32_t spins = 0;; ++spins) {
    u64 v[32];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const int i = k * 64 + c.lane;
      const int ci = i < n ? i : 0;
      v[k] = __hip_atomic_load(g + ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) ok &= (uint32_t)(v[k] >> 32) == tag;
    if (__all(ok)) {
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const int i = k * 64 + c.lane;
        if (i < n) dst[i] = __builtin_bit_cast(float, (uint32_t)v[k]);
      }
      return true;
    }
    if ((spins & 7) == 7 && aborted(c)) return false;
    if (spins > (EN_SPIN_MAX >> 4)) {
      give_up(c, GU_GATHER, tag);
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}
// the three 64-granule vectors an attention worker needs (q of its head, k and v of its kv head): ONE sweep
__device__ __forceinline__ bool gather_qkv(const Ctx& c, const u64* gq, const u64* gk, const u64* gv, uint32_t tag,
                                           lds_f32* dst /* q | k | v, 64 floats each */) {
  for (uint32_t spins = 0;; ++spins) {
    const u64 a = __hip_atomic_load(gq + c.lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 b = __hip_atomic_load(gk + c.lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 d = __hip_atomic_load(gv + c.lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool ok = (uint32_t)(a >> 32) == tag && (uint32_t)(b >> 32) == tag && (uint32_t)(d >> 32) == tag;
    if (__all(ok)) {
      dst[c.lane] = __builtin_bit_cast(float, (uint32_t)a);
      dst[64 + c.lane] = __builtin_bit_cast(float, (uint32_t)b);
      dst[128 + c.lane] = __builtin_bit_cast(float, (uint32_t)d);
      return true;
    }
    if ((spins & 7) == 7 && aborted(c)) return false;
    if (spins > (EN_SPIN_MAX >> 2)) {
      give_up(c, GU_GATHER, tag);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}
__device__ __forceinline__ void put_granule(u64* g, uint32_t tag, float v) {
  __hip_atomic_store(g, ((u64)tag << 32) | (u64)__builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// RMS-normalise xr (float4 j = lane + 64 j of the vector) into act exactly as the product's 256-thread
// Stager<true, false, 4> does: thread t = lane + 64 vw sums its float4s t + 256 v in ascending v, one DPP
// butterfly per wave, the four wave sums added in wave order.
__device__ __forceinline__ void norm_stage(const f32x4 (&xr)[16], const float* wnorm, int M, float eps, lds_f32x4* act,
                                           int lane) {
  const int M4 = M >> 2;
  float ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = lane + 64 * j;
    const float t = fma4(xr[j], xr[j], 0.f);
    ss[j & 3] += i < M4 ? t : 0.f;
  }
  float r = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) r += wave_sum(ss[w]);
  const float rs = 1.0f / sqrtf(r / (float)M + eps);
  const f32x4* w4 = (const f32x4*)wnorm;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = lane + 64 * j;
    if (i < M4) {
      const f32x4 w = w4[i];
      f32x4 t = xr[j];
      t.x = w.x * (rs * t.x);
      t.y = w.y * (rs * t.y);
      t.z = w.z * (rs * t.z);
      t.w = w.w * (rs * t.w);
      act[i] = t;
    }
  }
}

// one row pair out of the ring against xs: the product's per-lane order and split structure.  Four 64-float4
// blocks (12 ds_read_b128) are requested before the first FMA: a block at a time the loop ran at LDS latency
// (1.8 us per 16 KiB item, profiles/r4_engine_profile.txt), as slow as the whole weight stream.
__device__ __forceinline__ void item_dot(const lds_char* ring, uint32_t sp /* start piece, mod ring */, int ppr, int Mc,
                                         int split, const lds_f32x4* xs, int lane, float& s0, float& s1) {
  const int Q = (((Mc + split - 1) / split) + 3) & ~3;
  s0 = 0.f;
  s1 = 0.f;
  for (int part = 0; part < split; ++part) {
    const int cb = part * Q, ce = cb + Q < Mc ? cb + Q : Mc;
    float a0 = 0.f, a1 = 0.f;
    for (int i0 = cb; i0 < ce; i0 += 256) {
      f32x4 w0[4], w1[4], xv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int idx = i0 + 64 * k + lane;
        const int ci = idx < ce ? idx : 0;
        uint32_t p0 = sp + (uint32_t)(ci >> 6), p1 = p0 + (uint32_t)ppr;
        p0 = p0 >= EN_RING ? p0 - EN_RING : p0;
        p1 = p1 >= EN_RING ? p1 - EN_RING : p1;
        w0[k] = *(const lds_f32x4*)(ring + p0 * 1024u + (uint32_t)(ci & 63) * 16u);
        w1[k] = *(const lds_f32x4*)(ring + p1 * 1024u + (uint32_t)(ci & 63) * 16u);
        xv[k] = xs[ci];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (i0 + 64 * k < ce) {  // uniform: blocks wholly past the part's end are not part of the product's sum
          const bool in = i0 + 64 * k + lane < ce;
          f32x4 x = xv[k];
          x.x = in ? x.x : 0.f;
          x.y = in ? x.y : 0.f;
          x.z = in ? x.z : 0.f;
          x.w = in ? x.w : 0.f;
          a0 = fma4(w0[k], x, a0);
          a1 = fma4(w1[k], x, a1);
        }
      }
    }
    const float q0 = wave_sum(a0), q1 = wave_sum(a1);
    if (part == 0) {
      s0 = q0;
      s1 = q1;
    } else {
      s0 += q0;
      s1 += q1;
    }
  }
}

__device__ void en_consumer(const EngArgs& a, const Ctx& c, const __attribute__((address_space(3))) OpD* d,
                            lds_char* smem, int cons) {
  const lds_char* ring = smem;
  lds_f32x4* act = (lds_f32x4*)(smem + EN_RING * 1024);
  lds_f32* actf = (lds_f32*)act;
  lds_f32* xraw = (lds_f32*)(smem + EN_RING * 1024 + EN_ACT_BYTES);
  lds_f32* mf = (lds_f32*)(smem + EN_RING * 1024 + EN_ACT_BYTES + EN_XRAW_BYTES);  // misc as floats
  const int lane = c.lane;
  const int pos = *a.d_pos;
  const uint32_t tagbase = ((*a.d_epoch) * (uint32_t)a.n_layers + (uint32_t)a.layer) << 3;
  // this consumer's items: the running item sequence of the CU, round robin
  u64 acc_fw = 0;  // profile: ticks waiting for pieces
  int seq = 0;  // items of earlier ops
  auto first_mine = [&](int op, int seq0) {  // local index of my first item in op, or d[op].n
    int i = (cons - (seq0 % EN_NCONS) + EN_NCONS) % EN_NCONS;
    return i < d[op].n ? i : d[op].n;
  };
  // next item of mine at or after (op, i): sets cur_start so the loader knows what is released
  auto set_cur = [&](int op, int i, int seq0) {
    uint32_t s = 0xFFFFFFFFu;
    int sq = seq0;
    for (int k = op; k < N_WOPS; ++k) {
      const int f = k == op ? i : first_mine(k, sq);
      if (f < d[k].n) {
        s = d[k].start + (uint32_t)f * 2u * (uint32_t)d[k].ppr;
        break;
      }
      sq += d[k].n;
    }
    if (lane == 0) c.mw[MW_CUR0 + cons] = s;
  };
  auto wait_others_done = [&](uint32_t k) -> bool {  // the act region is free for op k's vector
    for (int w = 0; w < EN_NCONS; ++w)
      if (!wait_ge(c, MW_DONE0 + w, k, GU_DONE)) return false;
    return true;
  };

  if (a.mode == 1) return;
  if (a.mode >= 2) {  // ablation: no staging, no hand-offs
    int sq = 0;
    for (int op = 0; op < N_WOPS; ++op) {
      const int ppr = d[op].ppr, Mc = d[op].M >> 2;
      for (int i = first_mine(op, sq); i < d[op].n; i += EN_NCONS) {
        const uint32_t st = d[op].start + (uint32_t)i * 2u * (uint32_t)ppr;
        if (!wait_ge(c, MW_FILLED, st + 2u * (uint32_t)ppr, GU_FILLED)) return;
        float s0 = 0.f, s1 = 0.f;
        if (a.mode == 3) item_dot(ring, st % EN_RING, ppr, Mc, d[op].split, act, lane, s0, s1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        set_cur(op, i + EN_NCONS, sq);
        if (a.mode == 3 && lane == 0 && s0 == 123.4f) a.x[0] = s1;
      }
      sq += d[op].n;
    }
    return;
  }
  for (int op = 0; op < N_WOPS; ++op) {
    const uint32_t stage_id = (uint32_t)op + 1;  // MW_ACT value when op's vector is staged
    if (lane == 0) c.mw[MW_DONE0 + cons] = (uint32_t)op;  // finished every item of ops < op
    if (cons == 0) pf_set(c, PF_STAGE0 + op);
    // ---------------- stage the activation vector of `op` ----------------
    if (op == OP_QKV) {
      if (cons == 0) {
        f32x4 xr[16];
        const f32x4* x4 = (const f32x4*)a.x;
        const int M4 = a.dim >> 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int i = lane + 64 * j;
          xr[j] = x4[i < M4 ? i : 0];
        }
        norm_stage(xr, a.att_norm, a.dim, a.eps, act, lane);
        if (lane == 0) c.mw[MW_ACT] = stage_id;
      }
    } else if (op == OP_WO) {
      // ---- attention first (worker CUs), then the gather of its output by every CU ----
      const int h = (c.cu * a.heads) / EN_NCU;
      const bool worker = c.cu == (h * EN_NCU + a.heads - 1) / a.heads && h < a.heads;
      if (worker) {
        const int kvm = a.heads / a.kv_heads, g = h / kvm, hs = a.hs;
        lds_f32* aq = mf + MW_F_AQ;
        if (cons == 0) {
          c.mw[MW_THIN] = 1;
          const bool ok = gather_qkv(c, a.g_qkv + (size_t)h * hs, a.g_qkv + a.dim + (size_t)g * hs,
                                     a.g_qkv + a.dim + a.kv_dim + (size_t)g * hs, tagbase + EDGE_QKV + 1, aq);
          c.mw[MW_THIN] = 0;
          if (!ok) return;
          pf_set(c, PF_ATT_Q);
          if (lane == 0) c.mw[MW_ATTQ] = 1;
        }
        if (!wait_ge(c, MW_ATTQ, 1, GU_ATTQ)) return;
        // 16 lanes per timestep, each a float4 of the head (hs == 64); 12 lane groups per CU
        const int dl = lane & 15, vg = cons * 4 + (lane >> 4);
        const f32x4 q4 = ((const lds_f32x4*)aq)[dl];
        const f32x4 kcur = ((const lds_f32x4*)(aq + 64))[dl], vcur = ((const lds_f32x4*)(aq + 128))[dl];
        const int stride4 = a.kv_dim >> 2;
        const f32x4* K4 = (const f32x4*)(a.kc + (size_t)g * hs);
        const f32x4* V4 = (const f32x4*)(a.vc + (size_t)g * hs);
        const float scale = 1.0f / sqrtf((float)hs);
        float m = -INFINITY, l = 0.f;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        for (int tb = vg; tb <= pos; tb += 12 * 8) {
          f32x4 kv[8], vv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int t = tb + 12 * u;
            const int tt = t < pos ? t : 0;  // row `pos` itself comes from the hand-off, not from the cache
            kv[u] = K4[(size_t)tt * stride4 + dl];
            vv[u] = V4[(size_t)tt * stride4 + dl];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int t = tb + 12 * u;
            const f32x4 kk = t == pos ? kcur : kv[u], vx = t == pos ? vcur : vv[u];
            const float s = group_sum<16>(fma4(q4, kk, 0.f)) * scale;
            if (t <= pos) {
              const float mn = fmaxf(m, s);
              const float al = expf(m - mn), p = expf(s - mn);
              l = l * al + p;
              o.x = __builtin_fmaf(p, vx.x, o.x * al);
              o.y = __builtin_fmaf(p, vx.y, o.y * al);
              o.z = __builtin_fmaf(p, vx.z, o.z * al);
              o.w = __builtin_fmaf(p, vx.w, o.w * al);
              m = mn;
            }
          }
        }
        // lane groups of the wave -> wave partial
        const float Mw = across_groups_max<16>(m);
        const float f = m == -INFINITY ? 0.f : expf(m - Mw);
        const float Lw = across_groups_sum<16>(l * f);
        f32x4 ow;
        ow.x = across_groups_sum<16>(o.x * f);
        ow.y = across_groups_sum<16>(o.y * f);
        ow.z = across_groups_sum<16>(o.z * f);
        ow.w = across_groups_sum<16>(o.w * f);
        lds_f32* ap = mf + MW_F_APART + cons * 80;
        if (lane < 16) ((lds_f32x4*)ap)[dl] = ow;
        if (lane == 0) {
          ap[64] = Mw;
          ap[65] = Lw;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) c.mw[MW_APART0 + cons] = 1;
        if (cons == 0) {
          for (int w = 1; w < EN_NCONS; ++w)
            if (!wait_ge(c, MW_APART0 + w, 1, GU_APART)) return;
          const lds_f32* p0 = mf + MW_F_APART;
          float Mx = fmaxf(p0[64], fmaxf(p0[80 + 64], p0[160 + 64]));
          float num = 0.f, den = 0.f;
#pragma unroll
          for (int w = 0; w < EN_NCONS; ++w) {
            const float mw_ = p0[w * 80 + 64];
            const float fw = mw_ == -INFINITY ? 0.f : expf(mw_ - Mx);
            num = __builtin_fmaf(p0[w * 80 + lane], fw, num);
            den = __builtin_fmaf(p0[w * 80 + 65], fw, den);
          }
          put_granule(a.g_att + (size_t)h * hs + lane, tagbase + EDGE_ATT + 1, num / den);
          pf_set(c, PF_ATT_DONE);
        }
      }
      // gather the attention output (dim granules) into act: consumers share the 8 KB chunks
      if (!wait_others_done((uint32_t)op)) return;
      if (cons == 0) c.mw[MW_THIN] = 1;
      const int nch = ceil_div(a.dim, EN_CHUNK);
      for (int ch = cons; ch < nch; ch += EN_NCONS) {
        const int n = a.dim - ch * EN_CHUNK < EN_CHUNK ? a.dim - ch * EN_CHUNK : EN_CHUNK;
        if (!gather_chunk(c, a.g_att + (size_t)ch * EN_CHUNK, n, tagbase + EDGE_ATT + 1, actf + ch * EN_CHUNK)) return;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add((lds_u32*)&c.mw[MW_GATH], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (!wait_ge(c, MW_GATH, (uint32_t)EN_NCONS * 1u, GU_GATHER)) return;
      if (cons == 0) {
        c.mw[MW_THIN] = 0;
        c.mw[MW_ACT] = stage_id;
      }
    } else if (op == OP_FFN) {
      if (!wait_others_done((uint32_t)op)) return;
      if (cons == 0) c.mw[MW_THIN] = 1;
      const int nch = ceil_div(a.dim, EN_CHUNK);
      for (int ch = cons; ch < nch; ch += EN_NCONS) {
        const int n = a.dim - ch * EN_CHUNK < EN_CHUNK ? a.dim - ch * EN_CHUNK : EN_CHUNK;
        if (!gather_chunk(c, a.g_x2 + (size_t)ch * EN_CHUNK, n, tagbase + EDGE_X2 + 1, xraw + ch * EN_CHUNK)) return;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add((lds_u32*)&c.mw[MW_GATH], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (!wait_ge(c, MW_GATH, (uint32_t)EN_NCONS * 2u, GU_GATHER)) return;
      if (cons == 0) {
        c.mw[MW_THIN] = 0;
        f32x4 xr[16];
        const lds_f32x4* x4 = (const lds_f32x4*)xraw;
        const int M4 = a.dim >> 2;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int i = lane + 64 * j;
          xr[j] = x4[i < M4 ? i : 0];
        }
        norm_stage(xr, a.ffn_norm, a.dim, a.eps, act, lane);
        if (lane == 0) c.mw[MW_ACT] = stage_id;
      }
    } else {  // OP_W2: hidden granules straight into act
      if (!wait_others_done((uint32_t)op)) return;
      if (cons == 0) c.mw[MW_THIN] = 1;
      const int nch = ceil_div(a.hidden, EN_CHUNK);
      for (int ch = cons; ch < nch; ch += EN_NCONS) {
        const int n = a.hidden - ch * EN_CHUNK < EN_CHUNK ? a.hidden - ch * EN_CHUNK : EN_CHUNK;
        if (!gather_chunk(c, a.g_h + (size_t)ch * EN_CHUNK, n, tagbase + EDGE_H + 1, actf + ch * EN_CHUNK)) return;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add((lds_u32*)&c.mw[MW_GATH], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (!wait_ge(c, MW_GATH, (uint32_t)EN_NCONS * 3u, GU_GATHER)) return;
      if (cons == 0) {
        c.mw[MW_THIN] = 0;
        c.mw[MW_ACT] = stage_id;
      }
    }
    if (!wait_ge(c, MW_ACT, stage_id, GU_ACT)) return;
    if (cons == 0) pf_set(c, PF_READY0 + op);

    // ---------------- my items of `op` ----------------
    const int ppr = d[op].ppr, Mc = d[op].M >> 2;
    for (int i = first_mine(op, seq); i < d[op].n; i += EN_NCONS) {
      const uint32_t st = d[op].start + (uint32_t)i * 2u * (uint32_t)ppr;
      // epilogue operands (bias, sin / cos, residual) requested BEFORE the wait for the item's pieces: behind it
      // each item paid a dependent global round trip in its epilogue (2.5 us per wo item in the first profile)
      const int p = d[op].lo + i;
      float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
      int which = 0, r0 = 2 * p, r1 = 2 * p + 1, cidx = 0;
      if (op == OP_QKV) {
        qkv_decode(a, p, which, r0, r1, cidx);
        const float* bias = sel3(which, a.bq, a.bk, a.bv);
        e0 = bias ? bias[r0] : 0.f;
        e1 = bias ? bias[r1] : 0.f;
        e2 = a.sin_cache[(size_t)pos * a.hs + cidx];
        e3 = a.cos_cache[(size_t)pos * a.hs + cidx];
      } else if (op == OP_WO) {
        e0 = a.x[r0];
        e1 = a.x[r1];
      }
      const u64 t_fw = (c.prof && cons == 0) ? EN_TICK() : 0;
      if (!wait_ge(c, MW_FILLED, st + 2u * (uint32_t)ppr, GU_FILLED)) return;
      if (c.prof && cons == 0) acc_fw += EN_TICK() - t_fw;
      float s0, s1;
      item_dot(ring, st % EN_RING, ppr, Mc, d[op].split, act, lane, s0, s1);
      // released: my next item (this op or a later one)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      set_cur(op, i + EN_NCONS, seq);
      if (lane == 0) {
        if (op == OP_QKV) {
          s0 = s0 + e0;
          s1 = s1 + e1;
          if (which < 2) {
            const float v0 = s0, v1 = s1;
            s0 = v0 * e3 - v1 * e2;
            s1 = v0 * e2 + v1 * e3;
          }
          u64* gq = a.g_qkv + sel3(which, 0, a.dim, a.dim + a.kv_dim);
          put_granule(gq + r0, tagbase + EDGE_QKV + 1, s0);
          put_granule(gq + r1, tagbase + EDGE_QKV + 1, s1);
          if (which > 0) {  // the cache row for the following tokens
            float* row = sel3(which, (float*)nullptr, a.kc, a.vc) + (size_t)pos * a.kv_dim;
            row[r0] = s0;
            row[r1] = s1;
          }
        } else if (op == OP_WO) {
          put_granule(a.g_x2 + r0, tagbase + EDGE_X2 + 1, e0 + s0);
          put_granule(a.g_x2 + r1, tagbase + EDGE_X2 + 1, e1 + s1);
        } else if (op == OP_FFN) {
          put_granule(a.g_h + p, tagbase + EDGE_H + 1, swiglu1(s0, s1));
        } else {
          a.x[r0] = xraw[r0] + s0;
          a.x[r1] = xraw[r1] + s1;
        }
      }
    }
    if (cons == 0) pf_set(c, PF_ITEMS0 + op);
    // nothing of mine left in this op: cur_start already points at my next item (set_cur above), or was
    // set at kernel start when I own no item of this op
    seq += d[op].n;
  }
  if (cons == 0) {
    pf_set(c, PF_END);
    if (c.prof && lane == 0) c.prof[PF_FILLWAIT] = acc_fw;
  }
}

__global__ __launch_bounds__(256, 1) void k_engine_layer(const EngArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_generic[];
  if (a.mode == 4) return;  // ablation: the launch itself
  lds_char* smem = (lds_char*)smem_generic;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  Ctx c;
  c.mw = (lds_vu32*)(smem + EN_RING * 1024 + EN_ACT_BYTES + EN_XRAW_BYTES);
  c.dbg = a.dbg;
  c.lane = threadIdx.x & 63;
  c.cu = (int)blockIdx.x;
  c.prof = a.prof ? a.prof + (size_t)blockIdx.x * PF_N : nullptr;
  if (c.prof && threadIdx.x == 0) {
    for (int i = 0; i < PF_N; ++i) c.prof[i] = 0;
    c.prof[PF_START] = EN_TICK();
  }
  __attribute__((address_space(3))) OpD* d = (__attribute__((address_space(3))) OpD*)(c.mw + MW_OPD);  // in LDS: indexed by a runtime op everywhere (a register array would go to scratch)
  if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(a.dbg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
    return;  // an earlier launch gave up: do not spin through every bounded wait again
  // initial state: nothing landed, no abort; cur_start = 0 until a consumer writes its first item (conservative:
  // the loader merely sees less free space for a moment), so ONE barrier is enough
  if (threadIdx.x < 64) c.mw[threadIdx.x] = 0;
  if (threadIdx.x == 64) en_ops(a, c.cu, d);
  __syncthreads();
  if (wave >= 1 && c.lane == 0) {
    // first item of consumer (wave - 1) over the whole op list
    const int cons = wave - 1;
    uint32_t s = 0xFFFFFFFFu;
    int sq = 0;
    for (int k = 0; k < N_WOPS; ++k) {
      int i = (cons - (sq % EN_NCONS) + EN_NCONS) % EN_NCONS;
      if (i < d[k].n) {
        s = d[k].start + (uint32_t)i * 2u * (uint32_t)d[k].ppr;
        break;
      }
      sq += d[k].n;
    }
    c.mw[MW_CUR0 + cons] = s;
  }
  if (a.mode == 5) return;  // ablation: launch + prologue
  if (wave == 0) {
    en_loader(a, c, d, (unsigned)(size_t)smem);
  } else {
    en_consumer(a, c, d, smem, wave - 1);
  }
}

__global__ void k_bump(uint32_t* e) { *e += 1; }
__global__ void k_ungran(const u64* g, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = __builtin_bit_cast(float, (uint32_t)g[i]);
}

// ================================= host ==========================================================
struct Cfg {
  const char* name;
  int dim, hidden, heads, kv_heads, layers, rope_mode;
  bool bias;
  // product launch plan (kh_plan_decode_shapes of the preset): split, u, grid, wg
  int qkv[4], wo[4], ffn[4], w2[4];
};
static const Cfg CFGS[] = {
    {"1b", 2048, 8192, 32, 8, 16, KH_ROPE_HALF, false, {2, 4, 768, 256}, {2, 4, 512, 256}, {1, 8, 512, 256}, {4, 8, 512, 512}},
    {"qwen", 896, 4864, 14, 2, 24, KH_ROPE_HALF, true, {1, 4, 144, 256}, {1, 4, 112, 256}, {1, 4, 512, 256}, {4, 4, 224, 512}},
    {"tiny", 2048, 5632, 32, 4, 22, KH_ROPE_INTERLEAVED, false, {2, 4, 640, 256}, {2, 4, 512, 256}, {1, 8, 512, 256}, {4, 4, 512, 512}},
};

struct LayerBuf {
  float *wq, *wk, *wv, *wo, *w1, *w3, *w2, *bq, *bk, *bv, *an, *fn, *kc, *vc;
};

static void fill_rand(float* d, size_t n, float std, uint32_t seed) {
  std::vector<float> h(n);
  uint32_t s = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    const float u = (float)(s >> 8) * (1.0f / 16777216.0f) - 0.5f;
    h[i] = u * 3.4641f * std;  // uniform with that std
  }
  CK(hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
}
static float* dalloc_f(size_t n) {
  float* p;
  CK(hipMalloc(&p, n * sizeof(float)));
  return p;
}

template <int U, int SP>
static void launch_qkv_t(const KhQkvArgs& a, int grid, int wg, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((k_qkv<false, U, 4, SP>), dim3(grid), dim3(wg), lds, s, a);
}
template <int U, int SP>
static void launch_res_t(const KhGemvResArgs& a, int grid, int wg, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((k_gemv_res<false, U, 4, SP>), dim3(grid), dim3(wg), lds, s, a);
}
template <int U>
static void launch_ffn_t(const KhFfn13Args& a, int grid, int wg, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((k_ffn13<false, U, 4>), dim3(grid), dim3(wg), lds, s, a);
}
#define SEL_U(FN, U, ...) \
  do { if ((U) >= 8) FN<8>(__VA_ARGS__); else if ((U) >= 4) FN<4>(__VA_ARGS__); else FN<2>(__VA_ARGS__); } while (0)
static void launch_qkv(const KhQkvArgs& a, const int* sh, size_t lds, hipStream_t s) {
  const int u = sh[1], sp = sh[0];
#define GO(UU) do { if (sp == 2) launch_qkv_t<UU, 2>(a, sh[2], sh[3], lds, s); else launch_qkv_t<UU, 1>(a, sh[2], sh[3], lds, s); } while (0)
  if (u >= 8) GO(8); else if (u >= 4) GO(4); else GO(2);
#undef GO
}
static void launch_res(const KhGemvResArgs& a, const int* sh, size_t lds, hipStream_t s) {
  const int u = sh[1], sp = sh[0];
#define GO(UU) do { if (sp == 4) launch_res_t<UU, 4>(a, sh[2], sh[3], lds, s); else if (sp == 2) launch_res_t<UU, 2>(a, sh[2], sh[3], lds, s); else launch_res_t<UU, 1>(a, sh[2], sh[3], lds, s); } while (0)
  if (u >= 8) GO(8); else if (u >= 4) GO(4); else GO(2);
#undef GO
}
static void launch_ffn(const KhFfn13Args& a, const int* sh, size_t lds, hipStream_t s) {
  if (sh[1] >= 8) launch_ffn_t<8>(a, sh[2], sh[3], lds, s);
  else if (sh[1] >= 4) launch_ffn_t<4>(a, sh[2], sh[3], lds, s);
  else launch_ffn_t<2>(a, sh[2], sh[3], lds, s);
}

int main(int argc, char** argv) {
  const char* which = argc > 1 ? argv[1] : "1b";
  const int pos = argc > 2 ? atoi(argv[2]) : 64;
  const int reps = argc > 3 ? atoi(argv[3]) : 20;
  const Cfg* cf = nullptr;
  for (const Cfg& c : CFGS)
    if (!strcmp(c.name, which)) cf = &c;
  if (!cf || pos < 0 || pos > 255) {
    printf("usage: mb_engine [1b|qwen|tiny] [pos 0..255] [reps]\n");
    return 2;
  }
  const int dim = cf->dim, hidden = cf->hidden, hs = 64, heads = cf->heads, kvh = cf->kv_heads, kv_dim = kvh * hs;
  const int L = cf->layers, cache_len = 256;
  hipStream_t st;
  CK(hipStreamCreate(&st));
  std::vector<LayerBuf> lb(L);
  const float wstd = 0.02f;
  for (int l = 0; l < L; ++l) {
    LayerBuf& b = lb[l];
    b.wq = dalloc_f((size_t)dim * dim); b.wk = dalloc_f((size_t)kv_dim * dim); b.wv = dalloc_f((size_t)kv_dim * dim);
    b.wo = dalloc_f((size_t)dim * dim); b.w1 = dalloc_f((size_t)hidden * dim); b.w3 = dalloc_f((size_t)hidden * dim);
    b.w2 = dalloc_f((size_t)dim * hidden);
    b.an = dalloc_f(dim); b.fn = dalloc_f(dim);
    b.kc = dalloc_f((size_t)cache_len * kv_dim); b.vc = dalloc_f((size_t)cache_len * kv_dim);
    b.bq = b.bk = b.bv = nullptr;
    uint32_t sd = 100 * l;
    fill_rand(b.wq, (size_t)dim * dim, wstd, sd + 1); fill_rand(b.wk, (size_t)kv_dim * dim, wstd, sd + 2);
    fill_rand(b.wv, (size_t)kv_dim * dim, wstd, sd + 3); fill_rand(b.wo, (size_t)dim * dim, wstd, sd + 4);
    fill_rand(b.w1, (size_t)hidden * dim, wstd, sd + 5); fill_rand(b.w3, (size_t)hidden * dim, wstd, sd + 6);
    fill_rand(b.w2, (size_t)dim * hidden, wstd, sd + 7);
    fill_rand(b.an, dim, 0.05f, sd + 8); fill_rand(b.fn, dim, 0.05f, sd + 9);
    {  // norm weights 1 + jitter
      std::vector<float> h(dim);
      for (float** p : {&b.an, &b.fn}) {
        CK(hipMemcpy(h.data(), *p, dim * 4, hipMemcpyDeviceToHost));
        for (float& v : h) v += 1.0f;
        CK(hipMemcpy(*p, h.data(), dim * 4, hipMemcpyHostToDevice));
      }
    }
    if (cf->bias) {
      b.bq = dalloc_f(dim); b.bk = dalloc_f(kv_dim); b.bv = dalloc_f(kv_dim);
      fill_rand(b.bq, dim, wstd, sd + 10); fill_rand(b.bk, kv_dim, wstd, sd + 11); fill_rand(b.bv, kv_dim, wstd, sd + 12);
    }
    fill_rand(b.kc, (size_t)cache_len * kv_dim, 1.0f, sd + 13);
    fill_rand(b.vc, (size_t)cache_len * kv_dim, 1.0f, sd + 14);
  }
  // two copies of the mutable state: chain (c) and engine (e)
  float *x0 = dalloc_f(dim), *xc = dalloc_f(dim), *xe = dalloc_f(dim), *qc = dalloc_f(dim), *attc = dalloc_f(dim), *hc = dalloc_f(hidden);
  fill_rand(x0, dim, 1.0f, 999);
  std::vector<float*> kce(L), vce(L);
  for (int l = 0; l < L; ++l) {
    kce[l] = dalloc_f((size_t)cache_len * kv_dim);
    vce[l] = dalloc_f((size_t)cache_len * kv_dim);
    CK(hipMemcpy(kce[l], lb[l].kc, (size_t)cache_len * kv_dim * 4, hipMemcpyDeviceToDevice));
    CK(hipMemcpy(vce[l], lb[l].vc, (size_t)cache_len * kv_dim * 4, hipMemcpyDeviceToDevice));
  }
  float *sinc = dalloc_f((size_t)cache_len * hs), *cosc = dalloc_f((size_t)cache_len * hs);
  {
    std::vector<float> hsn((size_t)cache_len * hs), hcs((size_t)cache_len * hs);
    for (int p = 0; p < cache_len; ++p)
      for (int dd = 0; dd < hs; ++dd) {
        const float fr = 1.0f / powf(10000.f, (float)dd / (float)hs), v = (float)p * fr;
        hsn[(size_t)p * hs + dd] = sinf(v);
        hcs[(size_t)p * hs + dd] = cosf(v);
      }
    CK(hipMemcpy(sinc, hsn.data(), hsn.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(cosc, hcs.data(), hcs.size() * 4, hipMemcpyHostToDevice));
  }
  int32_t* d_pos;
  CK(hipMalloc(&d_pos, 4));
  CK(hipMemcpy(d_pos, &pos, 4, hipMemcpyHostToDevice));
  uint32_t *d_epoch, *d_dbg;
  CK(hipMalloc(&d_epoch, 4));
  CK(hipMalloc(&d_dbg, 64));
  CK(hipMemset(d_epoch, 0, 4));
  CK(hipMemset(d_dbg, 0, 64));
  u64 *g_qkv, *g_att, *g_x2, *g_h;
  CK(hipMalloc(&g_qkv, (size_t)(dim + 2 * kv_dim) * 8)); CK(hipMalloc(&g_att, (size_t)dim * 8));
  CK(hipMalloc(&g_x2, (size_t)dim * 8)); CK(hipMalloc(&g_h, (size_t)hidden * 8));
  CK(hipMemset(g_qkv, 0, (size_t)(dim + 2 * kv_dim) * 8)); CK(hipMemset(g_att, 0, (size_t)dim * 8));
  CK(hipMemset(g_x2, 0, (size_t)dim * 8)); CK(hipMemset(g_h, 0, (size_t)hidden * 8));
  // attention workspace of the product launch (positions < 256: one split, unused)
  const int attn_wg = 512;
  CK(hipFuncSetAttribute((const void*)k_engine_layer, hipFuncAttributeMaxDynamicSharedMemorySize, EN_LDS_BYTES));

  u64* g_prof = nullptr;
  int g_mode = 0;
  auto chain_layer = [&](int l, hipStream_t s) {
    const LayerBuf& b = lb[l];
    KhQkvArgs q{};
    q.x = xc; q.att_norm = b.an;
    q.wq = KhLin{b.wq, nullptr, b.bq}; q.wk = KhLin{b.wk, nullptr, b.bk}; q.wv = KhLin{b.wv, nullptr, b.bv};
    q.q_out = qc; q.kcache_layer = b.kc; q.vcache_layer = b.vc; q.d_pos = d_pos; q.sin_cache = sinc; q.cos_cache = cosc;
    q.dim = dim; q.kv_dim = kv_dim; q.head_size = hs; q.rope_mode = cf->rope_mode; q.gshift = 0; q.eps = 1e-5f;
    launch_qkv(q, cf->qkv, fused_lds_bytes(false, dim), s);
    KhAttnArgs at{};
    at.q = qc; at.kcache_layer = b.kc; at.vcache_layer = b.vc; at.out = attc; at.d_pos = d_pos;
    at.kv_dim = kv_dim; at.kv_mul = heads / kvh; at.head_size = hs; at.kv_heads = kvh; at.nsplit = 1; at.ws = nullptr;
    at.ws_stride = 1; at.nsplit_g = 0; at.t_long = 1 << 30; at.defer = 0; at.tok_stride = 0; at.ws_tok_bytes = 0;
    launch_attn_decode(at, 0, attn_wg, s);
    KhGemvResArgs w{};
    w.vec = attc; w.w = KhLin{b.wo, nullptr, nullptr}; w.x = xc; w.M = dim; w.K = dim; w.gshift = 0;
    launch_res(w, cf->wo, fused_lds_bytes(false, dim), s);
    KhFfn13Args f{};
    f.x = xc; f.ffn_norm = b.fn; f.w1 = KhLin{b.w1, nullptr, nullptr}; f.w3 = KhLin{b.w3, nullptr, nullptr}; f.h = hc;
    f.dim = dim; f.hidden = hidden; f.gshift = 0; f.eps = 1e-5f;
    launch_ffn(f, cf->ffn, fused_lds_bytes(false, dim), s);
    KhGemvResArgs w2{};
    w2.vec = hc; w2.w = KhLin{b.w2, nullptr, nullptr}; w2.x = xc; w2.M = hidden; w2.K = dim; w2.gshift = 0;
    launch_res(w2, cf->w2, fused_lds_bytes(false, hidden), s);
  };
  auto engine_layer = [&](int l, hipStream_t s) {
    const LayerBuf& b = lb[l];
    EngArgs a{};
    a.wq = b.wq; a.wk = b.wk; a.wv = b.wv; a.wo = b.wo; a.w1 = b.w1; a.w3 = b.w3; a.w2 = b.w2;
    a.bq = b.bq; a.bk = b.bk; a.bv = b.bv; a.att_norm = b.an; a.ffn_norm = b.fn;
    a.x = xe; a.kc = kce[l]; a.vc = vce[l]; a.sin_cache = sinc; a.cos_cache = cosc; a.d_pos = d_pos; a.d_epoch = d_epoch;
    a.g_qkv = g_qkv; a.g_att = g_att; a.g_x2 = g_x2; a.g_h = g_h; a.dbg = d_dbg; a.prof = g_prof; a.mode = g_mode;
    a.dim = dim; a.kv_dim = kv_dim; a.hidden = hidden; a.hs = hs; a.heads = heads; a.kv_heads = kvh;
    a.rope_mode = cf->rope_mode; a.layer = l; a.n_layers = L;
    a.split_qkv = cf->qkv[0]; a.split_wo = cf->wo[0]; a.split_ffn = cf->ffn[0]; a.split_w2 = cf->w2[0];
    a.eps = 1e-5f;
    hipLaunchKernelGGL(k_engine_layer, dim3(EN_NCU), dim3(256), EN_LDS_BYTES, s, a);
  };
  // >64 KiB LDS opt-in of the product's w2 kernel where needed
  if (fused_lds_bytes(false, hidden) > 64 * 1024) { printf("hidden too large for this harness\n"); return 2; }

  // ---------------- correctness: ONE layer at a time from identical inputs ----------------
  int bad = 0;
  std::vector<float> ha(dim), hb(dim);
  for (int l = 0; l < (L < 3 ? L : 3); ++l) {
    CK(hipMemcpy(xc, x0, dim * 4, hipMemcpyDeviceToDevice));
    CK(hipMemcpy(xe, x0, dim * 4, hipMemcpyDeviceToDevice));
    chain_layer(l, st);
    engine_layer(l, st);
    hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, st, d_epoch);
    hipError_t e = hipStreamSynchronize(st);
    uint32_t dbg[4];
    CK(hipMemcpy(dbg, d_dbg, 16, hipMemcpyDeviceToHost));
    if (e != hipSuccess || dbg[0]) {
      printf("layer %d: engine gave up: code %u cu %u info %u (%s)\n", l, dbg[0] & 255, dbg[0] >> 8, dbg[1], hipGetErrorString(e));
      return 1;
    }
    // stage outputs: q / k / v rows, attention output, hidden, final x
    auto cmp_gran = [&](const char* what, const u64* g, const float* ref, int n, bool exact) {
      std::vector<u64> hg(n);
      std::vector<float> hr(n);
      CK(hipMemcpy(hg.data(), g, (size_t)n * 8, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hr.data(), ref, (size_t)n * 4, hipMemcpyDeviceToHost));
      int ndiff = 0;
      float worst = 0.f;
      for (int i = 0; i < n; ++i) {
        float v;
        uint32_t bits = (uint32_t)hg[i];
        memcpy(&v, &bits, 4);
        if (memcmp(&v, &hr[i], 4)) ++ndiff;
        const float dlt = fabsf(v - hr[i]);
        if (!(dlt <= worst)) worst = dlt;
      }
      const bool ok = exact ? ndiff == 0 : worst <= 2e-5f;
      printf("  layer %d %-10s %s: %d / %d values differ, max |diff| %.3e\n", l, what, ok ? "ok " : "BAD", ndiff, n, worst);
      if (!ok) ++bad;
    };
    cmp_gran("q", g_qkv, qc, dim, true);
    cmp_gran("k-row", g_qkv + dim, lb[l].kc + (size_t)pos * kv_dim, kv_dim, true);
    cmp_gran("v-row", g_qkv + dim + kv_dim, lb[l].vc + (size_t)pos * kv_dim, kv_dim, true);
    cmp_gran("attention", g_att, attc, dim, false);
    cmp_gran("hidden", g_h, hc, hidden, false);
    CK(hipMemcpy(ha.data(), xc, dim * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hb.data(), xe, dim * 4, hipMemcpyDeviceToHost));
    float worst = 0.f;
    int ndiff = 0;
    for (int i = 0; i < dim; ++i) {
      if (memcmp(&ha[i], &hb[i], 4)) ++ndiff;
      const float dlt = fabsf(ha[i] - hb[i]);
      if (!(dlt <= worst)) worst = dlt;
    }
    printf("  layer %d x out      %s: %d / %d differ, max |diff| %.3e\n", l, worst <= 2e-5f ? "ok " : "BAD", ndiff, dim, worst);
    if (!(worst <= 2e-5f)) ++bad;
    // GEMV stages bit for bit: the product's wo / ffn13 / w2 kernels re-run on the ENGINE's own attention
    // output (the two attention kernels differ in summation order, so the chain's later stages see slightly
    // different inputs): every stage output of the engine must then equal the product kernel's exactly.
    {
      const LayerBuf& b = lb[l];
      CK(hipMemcpy(xc, x0, dim * 4, hipMemcpyDeviceToDevice));
      hipLaunchKernelGGL(k_ungran, dim3((dim + 255) / 256), dim3(256), 0, st, g_att, attc, dim);
      KhGemvResArgs w{};
      w.vec = attc; w.w = KhLin{b.wo, nullptr, nullptr}; w.x = xc; w.M = dim; w.K = dim; w.gshift = 0;
      launch_res(w, cf->wo, fused_lds_bytes(false, dim), st);
      CK(hipStreamSynchronize(st));
      cmp_gran("x after wo", g_x2, xc, dim, true);
      KhFfn13Args f{};
      f.x = xc; f.ffn_norm = b.fn; f.w1 = KhLin{b.w1, nullptr, nullptr}; f.w3 = KhLin{b.w3, nullptr, nullptr}; f.h = hc;
      f.dim = dim; f.hidden = hidden; f.gshift = 0; f.eps = 1e-5f;
      launch_ffn(f, cf->ffn, fused_lds_bytes(false, dim), st);
      CK(hipStreamSynchronize(st));
      cmp_gran("hidden*", g_h, hc, hidden, true);
      KhGemvResArgs w2{};
      w2.vec = hc; w2.w = KhLin{b.w2, nullptr, nullptr}; w2.x = xc; w2.M = hidden; w2.K = dim; w2.gshift = 0;
      launch_res(w2, cf->w2, fused_lds_bytes(false, hidden), st);
      CK(hipStreamSynchronize(st));
      CK(hipMemcpy(ha.data(), xc, dim * 4, hipMemcpyDeviceToHost));
      int nd = 0;
      for (int i = 0; i < dim; ++i) nd += memcmp(&ha[i], &hb[i], 4) != 0;
      printf("  layer %d x out*     %s: %d / %d differ from the product kernels run on the engine's attention output\n", l,
             nd ? "BAD" : "ok ", nd, dim);
      if (nd) ++bad;
    }
  }
  // ---------------- one profiled engine launch (layer 1): where the time goes inside the launch ----------------
  {
    u64* d_prof;
    CK(hipMalloc(&d_prof, (size_t)EN_NCU * PF_N * 8));
    CK(hipMemset(d_prof, 0, (size_t)EN_NCU * PF_N * 8));
    g_prof = d_prof;
    CK(hipMemcpy(xe, x0, dim * 4, hipMemcpyDeviceToDevice));
    engine_layer(0, st);  // warm
    hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, st, d_epoch);
    engine_layer(1 % L, st);
    hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, st, d_epoch);
    CK(hipStreamSynchronize(st));
    g_prof = nullptr;
    std::vector<u64> hp((size_t)EN_NCU * PF_N);
    CK(hipMemcpy(hp.data(), d_prof, hp.size() * 8, hipMemcpyDeviceToHost));
    u64 t0 = ~0ull, tend = 0;
    for (int cu = 0; cu < EN_NCU; ++cu) {
      if (hp[(size_t)cu * PF_N + PF_START] < t0) t0 = hp[(size_t)cu * PF_N + PF_START];
      if (hp[(size_t)cu * PF_N + PF_END] > tend) tend = hp[(size_t)cu * PF_N + PF_END];
    }
    printf("profiled launch (layer 1): %.2f us from the first workgroup's start to the last consumer's end\n",
           (double)(tend - t0) * 0.01);
    auto rel = [&](int cu, int slot) { const u64 v = hp[(size_t)cu * PF_N + slot]; return v ? (double)(v - t0) * 0.01 : -1.0; };
    auto acc = [&](int cu, int slot) { return (double)hp[(size_t)cu * PF_N + slot] * 0.01; };
    const char* opn[4] = {"qkv", "wo", "ffn13", "w2"};
    for (int cu : {0, 1, 100, 255}) {
      printf("  cu %3d: start %.2f | loader: issued", cu, rel(cu, PF_START));
      for (int k = 0; k < 4; ++k) printf(" %s %.2f", opn[k], rel(cu, PF_LD_OPEND0 + k));
      printf(" end %.2f, waited for space %.2f, in vmcnt %.2f\n", rel(cu, PF_LD_END), acc(cu, PF_LD_SPACE), acc(cu, PF_LD_VM));
      printf("           consumer 0:");
      for (int k = 0; k < 4; ++k)
        printf(" %s[stage %.2f ready %.2f items %.2f]", opn[k], rel(cu, PF_STAGE0 + k), rel(cu, PF_READY0 + k), rel(cu, PF_ITEMS0 + k));
      printf(" end %.2f, waited for pieces %.2f; attention q %.2f done %.2f\n", rel(cu, PF_END), acc(cu, PF_FILLWAIT),
             rel(cu, PF_ATT_Q), rel(cu, PF_ATT_DONE));
    }
    // chip-wide averages
    double a_space = 0, a_vm = 0, a_fw = 0, a_ldend = 0;
    for (int cu = 0; cu < EN_NCU; ++cu) {
      a_space += acc(cu, PF_LD_SPACE); a_vm += acc(cu, PF_LD_VM); a_fw += acc(cu, PF_FILLWAIT); a_ldend += rel(cu, PF_LD_END);
    }
    printf("  mean over CUs: loader end %.2f, waited for space %.2f, in vmcnt %.2f; consumer 0 waited for pieces %.2f\n",
           a_ldend / EN_NCU, a_space / EN_NCU, a_vm / EN_NCU, a_fw / EN_NCU);
    CK(hipFree(d_prof));
  }
  // ---------------- timing: L layers per token, graph replay ----------------
  hipGraph_t gc, ge;
  hipGraphExec_t gec, gee;
  CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  for (int l = 0; l < L; ++l) chain_layer(l, st);
  CK(hipStreamEndCapture(st, &gc));
  CK(hipGraphInstantiate(&gec, gc, nullptr, nullptr, 0));
  CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  for (int l = 0; l < L; ++l) engine_layer(l, st);
  hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, st, d_epoch);
  CK(hipStreamEndCapture(st, &ge));
  CK(hipGraphInstantiate(&gee, ge, nullptr, nullptr, 0));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto time_graph = [&](hipGraphExec_t g) {
    CK(hipMemcpy(xc, x0, dim * 4, hipMemcpyDeviceToDevice));
    CK(hipMemcpy(xe, x0, dim * 4, hipMemcpyDeviceToDevice));
    CK(hipGraphLaunch(g, st));
    CK(hipStreamSynchronize(st));
    CK(hipEventRecord(e0, st));
    for (int r = 0; r < reps; ++r) CK(hipGraphLaunch(g, st));
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1e3f / (float)(reps * L);
  };
  for (int round = 0; round < 3; ++round) {
    const float tc = time_graph(gec);
    const float te = time_graph(gee);
    uint32_t dbg[4];
    CK(hipMemcpy(dbg, d_dbg, 16, hipMemcpyDeviceToHost));
    printf("%s pos %d: chain %.2f us/layer   engine %.2f us/layer   ratio %.3f%s\n", cf->name, pos, tc, te, te / tc,
           dbg[0] ? "   ENGINE GAVE UP" : "");
    if (dbg[0]) {
      printf("  give-up code %u cu %u info %u\n", dbg[0] & 255, dbg[0] >> 8, dbg[1]);
      return 1;
    }
  }
  // ablations of the engine launch (results are garbage, timing only)
  for (int mode = 1; mode <= 5; ++mode) {
    g_mode = mode;
    hipGraph_t gm;
    hipGraphExec_t gem;
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    for (int l = 0; l < L; ++l) engine_layer(l, st);
    hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, st, d_epoch);
    CK(hipStreamEndCapture(st, &gm));
    CK(hipGraphInstantiate(&gem, gm, nullptr, nullptr, 0));
    const float t = time_graph(gem);
    const char* what[6] = {"", "loader alone (no ring back-pressure, no consumers)", "loader + consumers that only take and release pieces",
                           "loader + consumers with the dot products (no staging, no hand-offs)", "empty launch (immediate return)",
                           "launch + prologue only"};
    printf("%s ablation %d: %.2f us/layer   %s\n", cf->name, mode, t, what[mode]);
    uint32_t dbg[4];
    CK(hipMemcpy(dbg, d_dbg, 16, hipMemcpyDeviceToHost));
    if (dbg[0]) { printf("  give-up code %u cu %u info %u\n", dbg[0] & 255, dbg[0] >> 8, dbg[1]); return 1; }
    CK(hipGraphExecDestroy(gem));
    CK(hipGraphDestroy(gm));
  }
  g_mode = 0;
  const double mb = ((double)(2.0 * dim * dim + 2.0 * kv_dim * dim + 3.0 * hidden * dim)) * 4.0 / 1e6;
  printf("%s: %.1f MB of weights per layer; mismatching stages: %d\n", cf->name, mb, bad);
  return bad ? 1 : 0;
}
