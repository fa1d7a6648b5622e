// kh_seq_attn_wide.h — attention of the wide sequence pass in ONE launch for all lanes, shared prefixes read once
// (KH_FLAG_WIDE_ATTN; the plan is kh_wide_attn_plan.h).  The reference attends one query token of one sequence at a time
// (cuda/mha_kernel.cu:47-110); the wide pass without the flag launches the 8-lane pass's k_seq_attn / k_seq_attn_pfx once
// per group of 8 lanes, and every lane that shares a prompt streams the parent's rows itself.
//
//   k_sg_attn        a workgroup owns (item, kv head, chunk of the item's rows, up to QT tiles of 16 query columns).  The
//                    columns are query rows of DIFFERENT lanes and heads that all attend to the SAME rows, so there is no
//                    causal mask: the only bound is the end of the item.  Its waves take the chunk's 16-position tiles in
//                    turn; every K/V fragment a wave pulls into registers feeds all QT column tiles (16 QT columns per
//                    row read: 64 at head sizes 48 and 64, 32 at 128).  Both products run on v_mfma_f32_16x16x4_f32 in
//                    the operand arrangement of kh_pattn.h - S^T = K.Q^T, whose D layout is the B layout of
//                    O^T += V^T.P^T - with the online softmax in the log2 domain.  The waves' partials merge through LDS
//                    in fixed order; the workgroup stores UNNORMALISED (m, l, O[head_size]) per (lane, head, kind, chunk).
//   k_sg_attn_merge  one wave per (lane, head) folds that row's partials - the share item's chunks, then the own item's,
//                    at most 2 x KH_WA_NSPLIT_MAX - and writes head_size outputs row-major where the grouped launches
//                    write.  A launch of its own: stream order makes it correct without tickets or fences.
//
// Rows outside an item are never loaded (the cache is a reserved range whose rows past a slot's last position may be
// unmapped): a ragged last tile clamps its row index into the item and nulls the scores.  A ragged last column tile
// repeats its last valid column and does not store the copies (kh_seq_prefill.h's padding twins).
// Numerics: kh_model_prefill_gemm's tolerance contract (another summation order than k_seq_attn), nothing bit-exact.
// gfx950 only.
#pragma once
#include "kh_gemm.h"  // f32x4, mfma16, pg_comp
#include "kh_wide_attn_plan.h"

struct KhSgAttnArgs {
  const float* q;   // [n_lanes][dim] row-major, RoPE applied
  const float* kc;  // this layer's K cache rows [cache_len][kv_dim]; the lanes' own rows just written
  const float* vc;
  float* ws;        // partials: [n_lanes][heads][2 kinds][KH_WA_NSPLIT_MAX][KH_WA_HDR + head_size]
  float* out;       // [n_lanes][dim] row-major
  int dim, kv_dim, kv_heads, kv_mul;
};
static_assert(sizeof(KhSgAttnArgs) + sizeof(KhWaTable) <= 4096, "kernel arguments");
#define KH_WA_HDR 4  // floats ahead of a partial's O: m (log2 domain), l, two unused - O stays 16-byte aligned

__host__ __device__ static inline size_t kh_wa_slot(int lane, int heads, int h, int kind, int chunk, int hs) {
  return ((((size_t)lane * heads + h) * 2 + kind) * KH_WA_NSPLIT_MAX + chunk) * (size_t)(KH_WA_HDR + hs);
}
static inline size_t kh_wa_ws_floats(int n_lanes, int heads, int hs) { return kh_wa_slot(n_lanes, heads, 0, 0, 0, hs); }

template <int HB /* head_size / 16 */, int NW /* waves that split the chunk's position tiles */,
          int QT /* 16-column query tiles per workgroup */>
__global__ __launch_bounds__(64 * NW) void k_sg_attn(const KhSgAttnArgs a, const KhWaTable t) {
  constexpr int HS = 16 * HB;
  constexpr int NC = (HS + 63) / 64;  // 64-wide chunks of the head dimension on the P.V side
  constexpr int LDO = HS + 4;         // LDS row stride (floats): float4 rows of 16 columns hit distinct banks
  __shared__ __attribute__((aligned(16))) float o_lds[NW][16][LDO];
  __shared__ float m_lds[NW][16], l_lds[NW][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lj = lane >> 4;
  // workgroup -> (kv head g, work unit u): b % 8 is the XCD, so with 8 kv heads every workgroup that reads the rows of
  // kv head g shares one XCD's L2.  The table lists the share items - the long ones - first.
  const int b = (int)blockIdx.x;
  const int g = b % a.kv_heads;
  const int u = b / a.kv_heads;
  int it = 0;
  while (t.unit0[it + 1] <= u) ++it;  // uniform: the grid is unit0[n_items] x kv_heads
  const int ncols = (int)t.nlanes[it] * a.kv_mul;
  const int groups = ((ncols + 15) / 16 + QT - 1) / QT;
  const int ur = u - t.unit0[it];
  const int grp = ur % groups, chunk = ur / groups;
  const int row0 = t.row0[it], len = t.len[it];
  const int pt0 = chunk * t.ctiles[it];  // the chunk's 16-position tiles, counted from the item's first row
  const int n_pt = (len + 15) >> 4;
  const int pt1 = pt0 + t.ctiles[it] < n_pt ? pt0 + t.ctiles[it] : n_pt;
  const int col0 = grp * QT * 16;
  const int nq = (ncols - col0 + 15) / 16 < QT ? (ncols - col0 + 15) / 16 : QT;  // column tiles this workgroup holds
  const int heads = a.kv_heads * a.kv_mul;
  // scores in the log2 domain (score * 1/sqrt(hs) * log2(e)): the softmax runs on v_exp_f32, as kh_pattn_body.h
  const float scale = (1.0f / sqrtf((float)HS)) * 1.4426950408889634f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const float* kbase = a.kc + (size_t)g * HS + 4 * lj;
  const float* vbase = a.vc + (size_t)g * HS + 4 * li;
  auto load_k = [&](f32x4(&kf)[HB], int pt) __attribute__((always_inline)) {
    int p = pt * 16 + li;
    p = p < len - 1 ? p : len - 1;  // rows past the item are not this item's (maybe nobody's): clamp, nulled below
    const float* r = kbase + (size_t)(row0 + p) * a.kv_dim;
#pragma unroll
    for (int bb = 0; bb < HB; ++bb) kf[bb] = *(const f32x4*)(r + 16 * bb);
  };
  auto load_v = [&](f32x4(&vf)[NC][4], int pt) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int p = pt * 16 + lj * 4 + s;
      p = p < len - 1 ? p : len - 1;
      const float* r = vbase + (size_t)(row0 + p) * a.kv_dim;
#pragma unroll
      for (int c = 0; c < NC; ++c) vf[c][s] = (64 * c + 4 * li < HS) ? *(const f32x4*)(r + 64 * c) : zero4;
    }
  };

  f32x4 kf[2][HB], vf[2][NC][4];
  if (pt0 + wave < pt1) {  // wave-uniform
    load_k(kf[0], pt0 + wave);
    load_v(vf[0], pt0 + wave);
  }
  // column tile qi: this lane's query column = (lane of the item, head of the kv group); a padding column repeats the
  // item's last one
  f32x4 qf[QT][HB];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    int c = col0 + 16 * qi + li;
    c = c < ncols ? c : ncols - 1;
    const int ln = t.order[t.lane0[it] + c / a.kv_mul];
    const int h = g * a.kv_mul + c % a.kv_mul;
    const float* qrow = a.q + (size_t)ln * a.dim + (size_t)h * HS + 4 * lj;
#pragma unroll
    for (int bb = 0; bb < HB; ++bb) qf[qi][bb] = *(const f32x4*)(qrow + 16 * bb);
  }
  float m[QT], l[QT];
  f32x4 oacc[QT][NC][4];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    m[qi] = -INFINITY;
    l[qi] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) oacc[qi][c][e] = zero4;
  }

  auto tile = [&](const f32x4(&kc_)[HB], const f32x4(&vc_)[NC][4], int pt) __attribute__((always_inline)) {
    const int pb = pt * 16 + lj * 4;
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
      if (QT > 1 && qi >= nq) continue;  // a column tile beyond the item's columns (uniform)
      f32x4 sacc = zero4;
#pragma unroll
      for (int bb = 0; bb < HB; ++bb)
#pragma unroll
        for (int s = 0; s < 4; ++s) sacc = mfma16(pg_comp(kc_[bb], s), pg_comp(qf[qi][bb], s), sacc);
      float sv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) sv[r] = (pb + r < len) ? pg_comp(sacc, r) * scale : -INFINITY;
      float tm = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
      tm = fmaxf(tm, __shfl_xor(tm, 16));
      tm = fmaxf(tm, __shfl_xor(tm, 32));
      // finite: every tile below pt1 holds a row of the item
      const float m_new = fmaxf(m[qi], tm);
      const float alpha = __builtin_amdgcn_exp2f(m[qi] - m_new);  // exp2(-inf) = 0 on the wave's first tile
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(sv[r] - m_new);
      l[qi] = l[qi] * alpha + ((p[0] + p[1]) + (p[2] + p[3]));
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f32x4 o = oacc[qi][c][e];
          o.x *= alpha; o.y *= alpha; o.z *= alpha; o.w *= alpha;
#pragma unroll
          for (int s = 0; s < 4; ++s) o = mfma16(pg_comp(vc_[c][s], e), p[s], o);
          oacc[qi][c][e] = o;
        }
      m[qi] = m_new;
    }
  };

  for (int pt = pt0 + wave; pt < pt1; pt += 2 * NW) {
    const int p1 = pt + NW, p2 = pt + 2 * NW;
    if (p1 < pt1) {
      load_k(kf[1], p1);
      load_v(vf[1], p1);
    }
    __builtin_amdgcn_sched_barrier(0);
    tile(kf[0], vf[0], pt);
    if (p1 < pt1) {
      if (p2 < pt1) {
        load_k(kf[0], p2);
        load_v(vf[0], p2);
      }
      __builtin_amdgcn_sched_barrier(0);
      tile(kf[1], vf[1], p1);
    }
  }

  // ---- merge the waves' partials (fixed order), one column tile at a time through the same LDS area; the chunk's
  // partial goes out unnormalised --------------------------------------------------------------------------------------
  const int kind = it < t.n_share ? 0 : 1;
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    if (qi > 0) __syncthreads();
    float lq = l[qi];
    lq += __shfl_xor(lq, 16);
    lq += __shfl_xor(lq, 32);
    if (lj == 0) {
      m_lds[wave][li] = m[qi];
      l_lds[wave][li] = lq;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int d0 = 64 * c + 16 * lj;
      if (d0 < HS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          f32x4 v = {pg_comp(oacc[qi][c][0], r), pg_comp(oacc[qi][c][1], r), pg_comp(oacc[qi][c][2], r),
                     pg_comp(oacc[qi][c][3], r)};
          *(f32x4*)&o_lds[wave][li][d0 + 4 * r] = v;
        }
      }
    }
    __syncthreads();
    const int tok = tid & 15;
    const int c = col0 + 16 * qi + tok;
    if (c < ncols) {  // (a column tile beyond nq stores nothing either)
      float M = m_lds[0][tok];
#pragma unroll
      for (int w = 1; w < NW; ++w) M = fmaxf(M, m_lds[w][tok]);  // finite: wave 0 had the chunk's first tile
      float f[NW], L = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        f[w] = __builtin_amdgcn_exp2f(m_lds[w][tok] - M);  // waves without a tile: m = -inf -> 0
        L += f[w] * l_lds[w][tok];
      }
      const int ln = t.order[t.lane0[it] + c / a.kv_mul];
      const int h = g * a.kv_mul + c % a.kv_mul;
      float* dst = a.ws + kh_wa_slot(ln, heads, h, kind, chunk, HS);
      if ((tid >> 4) == 0) {
        dst[0] = M;
        dst[1] = L;
      }
      for (int grp4 = tid >> 4; grp4 < HS / 4; grp4 += 4 * NW) {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const f32x4 o = *(const f32x4*)&o_lds[w][tok][4 * grp4];
          r.x += f[w] * o.x; r.y += f[w] * o.y; r.z += f[w] * o.z; r.w += f[w] * o.w;
        }
        *(f32x4*)(dst + KH_WA_HDR + 4 * grp4) = r;
      }
    }
  }
}

// blockIdx.x = lane * heads + head; one wave.  Partials in fixed order: the share item's chunks, then the own item's.
template <int HB>
__global__ __launch_bounds__(64) void k_sg_attn_merge(const KhSgAttnArgs a, const KhWaTable t) {
  constexpr int HS = 16 * HB;
  const int heads = a.kv_heads * a.kv_mul;
  const int ln = (int)blockIdx.x / heads, h = (int)blockIdx.x % heads;
  const int sh = t.share_of[ln];
  const int n0 = sh == 255 ? 0 : (int)t.nsplit[sh];  // chunks of the share item
  const int n1 = t.nsplit[t.n_share + ln];           // ... of the own item (>= 1)
  const float* p0 = a.ws + kh_wa_slot(ln, heads, h, 0, 0, HS);
  const float* p1 = a.ws + kh_wa_slot(ln, heads, h, 1, 0, HS);
  constexpr int S = KH_WA_HDR + HS;
  float M = -INFINITY;
  for (int k = 0; k < n0; ++k) M = fmaxf(M, p0[k * S]);
  for (int k = 0; k < n1; ++k) M = fmaxf(M, p1[k * S]);  // finite: the own item holds the lane's own row
  float L = 0.f;
  float acc[(HS + 63) / 64];
#pragma unroll
  for (int i = 0; i < (HS + 63) / 64; ++i) acc[i] = 0.f;
  auto fold = [&](const float* p) __attribute__((always_inline)) {
    const float f = __builtin_amdgcn_exp2f(p[0] - M);
    L += f * p[1];
#pragma unroll
    for (int i = 0; i < (HS + 63) / 64; ++i) {
      const int d = (int)threadIdx.x + 64 * i;
      if (d < HS) acc[i] += f * p[KH_WA_HDR + d];
    }
  };
  for (int k = 0; k < n0; ++k) fold(p0 + k * S);
  for (int k = 0; k < n1; ++k) fold(p1 + k * S);
  float* out = a.out + (size_t)ln * a.dim + (size_t)h * HS;
#pragma unroll
  for (int i = 0; i < (HS + 63) / 64; ++i) {
    const int d = (int)threadIdx.x + 64 * i;
    if (d < HS) out[d] = acc[i] / L;
  }
}
