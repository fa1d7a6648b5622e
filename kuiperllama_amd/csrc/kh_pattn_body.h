// kh_pattn_body.h — the statements of the prompt-slice attention kernel of kh_pattn.h, included INSIDE a kernel
// definition (no include guard), as kh_gemm_body.h is: ONE text for k_pg_attn (kh_pattn.h: the query tokens of a run of
// consecutive positions of one sequence whose position p is cache row p) and k_rg_attn (kh_seq_prefill.h: every
// 16-token query tile a segment of some sequence slot, which may read a shared prefix from its parent's rows).  The
// including kernel has in scope
//   HB, NW, QT              compile-time: head_size / 16, waves that split the timesteps, query tiles per workgroup
//   const KhPgAttnArgs a    its first kernel argument
//   addr                    where the query columns sit:
//     addr.tiles(QT)          workgroups per head: groups of QT query tiles in the slab
//     addr.last_pos(t0, QT)   the last timestep any column of the group that starts at slab token t0 attends to
//     addr.col(t)             the slab row column t reads its query from (a padding column repeats the last valid one)
//     addr.pos(t)             the position of column t: the last timestep it attends to
//     addr.tile_pos0(t)       the position of the first column of the query tile that starts at slab token t
//     addr.row(t0, p)         the cache row of timestep p for the group that starts at slab token t0
//     addr.stores(t)          is column t's output kept
  constexpr int HS = 16 * HB;
  constexpr int NC = (HS + 63) / 64;  // 64-wide chunks of the head dimension on the P.V side
  constexpr int LDO = HS + 4;         // LDS row stride (floats): float4 rows of 16 tokens hit distinct banks
  __shared__ __attribute__((aligned(16))) float o_lds[NW][16][LDO];
  __shared__ float m_lds[NW][16], l_lds[NW][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lj = lane >> 4;
  // workgroup -> (kv group g, head-in-group j, token tile tt); b % 8 is the XCD: the kv_mul heads
  // (and all token tiles) that share K/V rows share an XCD's L2.  Long tiles are dispatched first.
  const int b = (int)blockIdx.x;
  const int g = b % a.kv_heads;
  const int rest = b / a.kv_heads;
  const int j = rest % a.kv_mul;
  const int n_tt = addr.tiles(QT);
  const int tt = n_tt - 1 - rest / a.kv_mul;
  const int h = g * a.kv_mul + j;
  const int t0 = tt * 16 * QT;
  const int p_last = addr.last_pos(t0, QT);  // last timestep any token of this workgroup attends to
  const int n_pt = (p_last >> 4) + 1;  // 16-position tiles, aligned at timestep 0
  // scores are kept in the log2 domain (score * 1/sqrt(hs) * log2(e)) so that the softmax runs on the
  // hardware exp2 (v_exp_f32), like the GQA decode path of kh_attn.h: exp(s - m) == exp2(s2 - m2)
  const float scale = (1.0f / sqrtf((float)HS)) * 1.4426950408889634f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  const float* kbase = a.kc + (size_t)g * HS + 4 * lj;
  const float* vbase = a.vc + (size_t)g * HS + 4 * li;
  auto load_k = [&](f32x4(&kf)[HB], int pt) __attribute__((always_inline)) {
    int p = pt * 16 + li;
    p = p < p_last ? p : p_last;  // rows past the slice are not written yet: clamp, masked below
    const float* r = kbase + (size_t)addr.row(t0, p) * a.kv_dim;
#pragma unroll
    for (int bb = 0; bb < HB; ++bb) kf[bb] = *(const f32x4*)(r + 16 * bb);
  };
  auto load_v = [&](f32x4(&vf)[NC][4], int pt) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int p = pt * 16 + lj * 4 + s;
      p = p < p_last ? p : p_last;
      const float* r = vbase + (size_t)addr.row(t0, p) * a.kv_dim;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        vf[c][s] = (64 * c + 4 * li < HS) ? *(const f32x4*)(r + 64 * c) : zero4;
    }
  };

  f32x4 kf[2][HB], vf[2][NC][4];
  if (wave < n_pt) {  // wave-uniform
    load_k(kf[0], wave);
    load_v(vf[0], wave);
  }
  // query tile qi: this lane's query token (column of both products; padding columns repeat the last
  // token) and the last timestep it attends to
  f32x4 qf[QT][HB];
  int my_pos[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    const int t = t0 + 16 * qi + li;
    const int tq = addr.col(t);
    my_pos[qi] = addr.pos(t);
    const float* qrow = a.q + (size_t)tq * a.dim + (size_t)h * HS + 4 * lj;
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
      // position tiles wholly above the diagonal of this query tile: nothing to add (wave-uniform)
      if (QT > 1 && pt * 16 > addr.tile_pos0(t0 + 16 * qi) + 15) continue;
      f32x4 sacc = zero4;
#pragma unroll
      for (int bb = 0; bb < HB; ++bb)
#pragma unroll
        for (int s = 0; s < 4; ++s) sacc = mfma16(pg_comp(kc_[bb], s), pg_comp(qf[qi][bb], s), sacc);
      float sv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) sv[r] = (pb + r <= my_pos[qi]) ? pg_comp(sacc, r) * scale : -INFINITY;
      float tm = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
      tm = fmaxf(tm, __shfl_xor(tm, 16));
      tm = fmaxf(tm, __shfl_xor(tm, 32));
      const float m_new = fmaxf(m[qi], tm);
      const float m_ref = m_new == -INFINITY ? 0.f : m_new;  // a token that has seen no timestep yet
      const float alpha = __builtin_amdgcn_exp2f(m[qi] - m_ref);  // exp2(-inf) = 0 on its first timestep
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(sv[r] - m_ref);
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

  for (int pt = wave; pt < n_pt; pt += 2 * NW) {
    const int p1 = pt + NW, p2 = pt + 2 * NW;
    if (p1 < n_pt) {
      load_k(kf[1], p1);
      load_v(vf[1], p1);
    }
    __builtin_amdgcn_sched_barrier(0);
    tile(kf[0], vf[0], pt);
    if (p1 < n_pt) {
      if (p2 < n_pt) {
        load_k(kf[0], p2);
        load_v(vf[0], p2);
      }
      __builtin_amdgcn_sched_barrier(0);
      tile(kf[1], vf[1], p1);
    }
  }

  // ---- merge the waves' partials (fixed order), one query tile at a time through the same LDS area -----
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
    const int t = t0 + 16 * qi + tok;
    if (addr.stores(t)) {
      float M = m_lds[0][tok];
#pragma unroll
      for (int w = 1; w < NW; ++w) M = fmaxf(M, m_lds[w][tok]);  // finite: a token sees its own timestep
      float f[NW], L = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        f[w] = __builtin_amdgcn_exp2f(m_lds[w][tok] - M);  // waves without a timestep: m = -inf -> 0
        L += f[w] * l_lds[w][tok];
      }
      for (int grp = tid >> 4; grp < HS / 4; grp += 4 * NW) {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const f32x4 o = *(const f32x4*)&o_lds[w][tok][4 * grp];
          r.x += f[w] * o.x; r.y += f[w] * o.y; r.z += f[w] * o.z; r.w += f[w] * o.w;
        }
        r.x /= L; r.y /= L; r.z /= L; r.w /= L;
        const int k = h * HS + 4 * grp;
        const size_t at = a.layout == KH_PA_ROWS ? (size_t)t * a.dim + k
                                                 : pg_tiled_index(a.layout == KH_PA_TILED_Q8, k, t, a.tcap);
        *(f32x4*)(a.out + at) = r;
      }
    }
  }
