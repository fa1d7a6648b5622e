// kh_gemm_body.h — the statements of the GEMM kernel of kh_gemm.h, included INSIDE a kernel definition (no include
// guard): ONE text for k_pg_gemm (kh_gemm.h: tokens of a run of consecutive positions) and k_sg_gemm (kh_seq_gemm.h:
// lanes of different sequences).  The including kernel is a template <bool QUANT, int R, int NT, int EPI> - or <int R, int NT,
// EPI> with QUANT a constant - and has in scope
//   constexpr bool KH_GEMM_W16   the K loop: false - pg_kloop_f32 / pg_kloop_q8 on the image; true - pg_kloop_w16
//                           (kh_gemm_w16.h) on the 16-bit copy
//   constexpr bool KH_GEMM_Q16   with QUANT: pg_kloop_q16 (kh_gemm_q16.h) on the int8 image in place of pg_kloop_q8
//   const KhPgGemmArgs a    its first kernel argument
//   addr                    the token addressing of the QKV epilogue: addr.pos(tok) = the RoPE row, addr.row(tok) = the
//                           cache row of token tok (PgRunAddr, SgLaneAddr)
//   char smem_raw[]         the dynamic LDS
// Textual, not a device function template (the way pf_qkv_body is): the arguments would reach a function through a
// generic-address-space reference, the compiler then no longer reads them straight from the kernel-argument segment,
// and the run-time indexed a.w[] leaves a 176-byte copy of them in scratch (every QKV instantiation: 184 bytes per
// lane; tests/test_code_objects.py allows none).
  static_assert(EPI == KH_PG_QKV || EPI == KH_PG_RESID || EPI == KH_PG_SWIGLU || EPI == KH_PG_STORE, "epilogue");
  constexpr int NM = EPI == KH_PG_SWIGLU ? 2 : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = kh_nwaves();
  const int ks = nw / NM;
  const int mat = wave / ks, kpart = wave - mat * ks;
  const int i = lane & 15, h = lane >> 4;
  const int K = a.K;
  // first row of the wave's tile r in the stacked output: neighbours, or (half-mode fused RoPE) the
  // tile and its rotation partner hs/2 rows further down the same head
  int row0 = (int)blockIdx.x * (16 * R), rstep = 16;
  if (EPI == KH_PG_QKV && R == 2 && NT <= 4 && a.rope == KH_PG_ROPE_TILES) {
    const int nb = a.head_size >> 5;  // workgroups per head
    const int g = (int)blockIdx.x / nb;
    row0 = g * a.head_size + ((int)blockIdx.x - g * nb) * 16;
    rstep = a.head_size >> 1;
  }
  const int tok0 = (int)blockIdx.y * (16 * NT);
  // weight matrix of this workgroup (its tiles never straddle two matrices: row counts are multiples
  // of 16 * R - of the head size with paired tiles -, checked by the host)
  KhLin W = a.w[mat];
  int wr0 = row0;
  if (EPI == KH_PG_QKV) {
    if (row0 >= a.rows0 + a.rows1) {
      W = a.w[2];
      wr0 = row0 - a.rows0 - a.rows1;
    } else if (row0 >= a.rows0) {
      W = a.w[1];
      wr0 = row0 - a.rows0;
    }
  }
  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (the K range depends on the wave index only: keep it in scalar registers so the block guards
  // of the K loop are scalar branches)
  PgBAddr B;
  if constexpr (KH_GEMM_W16) {
    // the 16-bit copy on the bf16 matrix cores (kh_gemm_w16.h): blocks of 32 columns; the activation slabs are the fp32
    // loops' - the lane's eight columns 32b + 8h .. are half h & 1 of the tiled slab's 16-column block 2b + (h >> 1)
    const int nb = K >> 5;
    const int z0 = (int)((long)blockIdx.z * nb / gridDim.z), z1 = (int)((long)(blockIdx.z + 1) * nb / gridDim.z);
    const int b0 = __builtin_amdgcn_readfirstlane(z0 + (int)((long)kpart * (z1 - z0) / ks));
    const int b1 = __builtin_amdgcn_readfirstlane(z0 + (int)((long)(kpart + 1) * (z1 - z0) / ks));
    const uint16_t* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wrow[r] = (const uint16_t*)W.w + (size_t)(wr0 + rstep * r + i) * K + 8 * h;
    if (a.b_tiled) {
      B = PgBAddr{a.B + ((size_t)(h >> 1) * a.tcap + (size_t)(tok0 + i)) * 16 + 8 * (h & 1), 256, (size_t)a.tcap * 32, 0};
    } else {
      B = PgBAddr{a.B + (size_t)(tok0 + i) * K + 8 * h, (size_t)16 * K, 32, 0};
    }
    if (b1 > b0) pg_kloop_w16<R, NT>(wrow, B, b0, b1, acc);
  } else if (!QUANT) {
    const int nb = K >> 4;
    const int z0 = (int)((long)blockIdx.z * nb / gridDim.z), z1 = (int)((long)(blockIdx.z + 1) * nb / gridDim.z);
    const int b0 = __builtin_amdgcn_readfirstlane(z0 + (int)((long)kpart * (z1 - z0) / ks));
    const int b1 = __builtin_amdgcn_readfirstlane(z0 + (int)((long)(kpart + 1) * (z1 - z0) / ks));
    const float* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wrow[r] = (const float*)W.w + (size_t)(wr0 + rstep * r + i) * K + 4 * h;
    if (a.b_tiled) {
      B = PgBAddr{a.B + (size_t)(tok0 + i) * 16 + 4 * h, 256, (size_t)a.tcap * 16, 0};
    } else {
      B = PgBAddr{a.B + (size_t)(tok0 + i) * K + 4 * h, (size_t)16 * K, 16, 0};
    }
    // the uniform ring (both operands D blocks ahead) when the wave's block count allows it: 8 blocks
    // deep for the small register tiles, KH_PG_RING_D16 for the big (2, 8) tile; else the phase scheme
    constexpr int RING_D = R * NT <= 8 ? 8 : KH_PG_RING_D16;
    if constexpr (RING_D > 0) {
      if (b1 - b0 >= 2 * RING_D && (b1 - b0) % RING_D == 0)
        pg_kloop_f32_ring<R, NT, RING_D>(wrow, B, b0, b1, acc);
      else if (b1 > b0)
        pg_kloop_f32<R, NT>(wrow, B, b0, b1, acc);
    } else if (b1 > b0) {
      pg_kloop_f32<R, NT>(wrow, B, b0, b1, acc);
    }
  } else {
    const int nb = K >> 6;
    const int z0 = (int)((long)blockIdx.z * nb / gridDim.z), z1 = (int)((long)(blockIdx.z + 1) * nb / gridDim.z);
    const int b0 = __builtin_amdgcn_readfirstlane(z0 + (int)((long)kpart * (z1 - z0) / ks));
    const int b1 = __builtin_amdgcn_readfirstlane(z0 + (int)((long)(kpart + 1) * (z1 - z0) / ks));
    const int8_t* wrow[R];
    const float* srow[R];
    // the scale a lane loads: pg_kloop_q8 scales the weights of row i; pg_kloop_q16 (kh_gemm_q16.h) scales the partial
    // sums, and the lane's quad shares the scales of the rows 4h .. 4h + 3 its accumulators hold
    const int si = KH_GEMM_Q16 ? 4 * h + (i & 3) : i;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      wrow[r] = (const int8_t*)W.w + (size_t)(wr0 + rstep * r + i) * K + 16 * h;
      srow[r] = W.scales + (size_t)(wr0 + rstep * r + si) * nb;
    }
    if (a.b_tiled) {
      B = PgBAddr{a.B + (size_t)(tok0 + i) * 16 + 4 * h, 256, (size_t)4 * a.tcap * 16,
                  (size_t)a.tcap * 16};
    } else {
      B = PgBAddr{a.B + (size_t)(tok0 + i) * K + 16 * h, (size_t)16 * K, 64, 4};
    }
    if constexpr (KH_GEMM_Q16) {
      if (b1 > b0) pg_kloop_q16<R, NT>(wrow, srow, B, b0, b1, acc);
    } else {
      if (b1 > b0) pg_kloop_q8<R, NT>(wrow, srow, B, b0, b1, acc);
    }
  }
  // ---- combine the K slices (fixed order) and run the epilogue on float4 = 4 rows x 1 token,
  //      one 16-row tile at a time (the LDS area holds one tile row of partials) -------------------
  f32x4* red = (f32x4*)smem_raw;
  const bool direct = nw == 1;
  // fused half-mode RoPE: tile 0's rows wait here for their partners in tile 1 (NT <= 4 only: with
  // eight token tiles the 32 extra registers push the epilogue into scratch; the host then keeps k_pg_rope)
  constexpr bool TILE_ROPE = EPI == KH_PG_QKV && R == 2 && NT <= 4;
  f32x4 keep[TILE_ROPE ? NT : 1];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!direct) {
      if (r > 0) __syncthreads();
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) red[((size_t)wave * NT + nt) * 64 + lane] = acc[r][nt];
      __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < NT; ++it) {  // NT * 64 elements over >= 64 threads (static trip count: keep[])
      const int e = (int)threadIdx.x + it * kh_wg();
      if (e >= NT * 64) break;
      const int nt = e >> 6, ln = e & 63;
      f32x4 v0, v1 = f32x4{0.f, 0.f, 0.f, 0.f};
      if (direct) {
        v0 = acc[r][0];
#pragma unroll
        for (int t = 1; t < NT; ++t)
          if (t == nt) v0 = acc[r][t];
      } else {
        v0 = red[((size_t)0 * NT + nt) * 64 + ln];
        for (int kp = 1; kp < ks; ++kp) {
          const f32x4 p = red[((size_t)kp * NT + nt) * 64 + ln];
          v0.x += p.x; v0.y += p.y; v0.z += p.z; v0.w += p.w;
        }
        if (NM == 2) {
          v1 = red[((size_t)ks * NT + nt) * 64 + ln];
          for (int kp = 1; kp < ks; ++kp) {
            const f32x4 p = red[((size_t)(ks + kp) * NT + nt) * 64 + ln];
            v1.x += p.x; v1.y += p.y; v1.z += p.z; v1.w += p.w;
          }
        }
      }
      const int tok = tok0 + 16 * nt + (ln & 15);
      if (tok >= a.T) continue;  // (padding tokens: nothing kept, nothing stored)
      const int orow = row0 + rstep * r + 4 * (ln >> 4);  // first of the 4 output rows
      if (EPI == KH_PG_QKV) {
        // bias after the matmul, before RoPE (matmul.cpp:74-77)
        int which = 0, rr = orow;
        if (rr >= a.rows0 + a.rows1) {
          which = 2;
          rr -= a.rows0 + a.rows1;
        } else if (rr >= a.rows0) {
          which = 1;
          rr -= a.rows0;
        }
        const float* bias = a.w[which].bias;
        if (bias) {
          const f32x4 bv = *(const f32x4*)(bias + rr);
          v0.x += bv.x; v0.y += bv.y; v0.z += bv.z; v0.w += bv.w;
        }
        float* dst = which == 0 ? a.out + (size_t)tok * a.ldo
                                : (which == 1 ? a.kc : a.vc) + (size_t)addr.row(tok) * a.rows1;
        const int hs = a.head_size;
        const float* sn = a.sin_cache + (size_t)addr.pos(tok) * hs;
        const float* cs = a.cos_cache + (size_t)addr.pos(tok) * hs;
        if (which < 2 && a.rope == KH_PG_ROPE_PAIRS) {
          // interleaved: the float4 holds pairs (rr, rr+1), (rr+2, rr+3); cache column = row in head
          const int c = rr % hs;
          const float s0 = sn[c], c0 = cs[c], s1 = sn[c + 2], c1 = cs[c + 2];
          f32x4 o;
          o.x = v0.x * c0 - v0.y * s0;
          o.y = v0.x * s0 + v0.y * c0;
          o.z = v0.z * c1 - v0.w * s1;
          o.w = v0.z * s1 + v0.w * c1;
          *(f32x4*)(dst + rr) = o;
        } else if (TILE_ROPE && which < 2 && a.rope == KH_PG_ROPE_TILES) {
          if (r == 0) {
            keep[TILE_ROPE ? it : 0] = v0;  // rows head*hs + j .. + 3 (j < hs/2): rotated when tile 1 arrives
          } else {
            // this tile holds the partners, rows head*hs + hs/2 + j .. + 3; cache column 2 * j
            const int half = hs >> 1, j = (rr - half) % hs;
            const f32x4 lo = keep[TILE_ROPE ? it : 0];
            f32x4 olo, ohi;
            const float s0 = sn[2 * j], c0 = cs[2 * j], s1 = sn[2 * j + 2], c1 = cs[2 * j + 2];
            const float s2 = sn[2 * j + 4], c2 = cs[2 * j + 4], s3 = sn[2 * j + 6], c3 = cs[2 * j + 6];
            olo.x = lo.x * c0 - v0.x * s0; ohi.x = lo.x * s0 + v0.x * c0;
            olo.y = lo.y * c1 - v0.y * s1; ohi.y = lo.y * s1 + v0.y * c1;
            olo.z = lo.z * c2 - v0.z * s2; ohi.z = lo.z * s2 + v0.z * c2;
            olo.w = lo.w * c3 - v0.w * s3; ohi.w = lo.w * s3 + v0.w * c3;
            *(f32x4*)(dst + rr - half) = olo;
            *(f32x4*)(dst + rr) = ohi;
          }
        } else {
          *(f32x4*)(dst + rr) = v0;
        }
      } else if (EPI == KH_PG_RESID) {
        if (gridDim.z > 1) {  // K slice of a cross-workgroup split: the following k_pg_rmsnorm adds it
          *(f32x4*)(a.part + ((size_t)blockIdx.z * a.tcap + tok) * a.ldo + orow) = v0;
        } else {
          f32x4* dst = (f32x4*)(a.out + (size_t)tok * a.ldo + orow);
          f32x4 x = *dst;
          x.x += v0.x; x.y += v0.y; x.z += v0.z; x.w += v0.w;  // residual add (llama3.cpp:686,719)
          *dst = x;
        }
      } else if (EPI == KH_PG_STORE) {
        *(f32x4*)(a.out + (size_t)tok * a.ldo + orow) = v0;  // row-major [T][ldo]: the classifier's logits rows
      } else {
        f32x4 o;
        o.x = swiglu1(v0.x, v1.x);
        o.y = swiglu1(v0.y, v1.y);
        o.z = swiglu1(v0.z, v1.z);
        o.w = swiglu1(v0.w, v1.w);
        *(f32x4*)(a.out + pg_tiled_index(QUANT, orow, tok, a.tcap)) = o;  // H feeds the w2 GEMM: tiled slab
      }
    }
  }
