// kh_score_gemm_epilogue.h — the epilogue of the classifier kernels of sequence scoring, written once: the text is
// included at the END of a kernel's body (as kh_gemm_body.h is), in k_pg_cls_lse (kh_score_gemm.h) and k_pg_cls_lse_w16
// (kh_score_gemm_w16.h).  The C/D map of v_mfma_f32_16x16x32_bf16 is that of v_mfma_f32_16x16x4_f32, so both kernels hand
// over the same accumulators.  Included text and not a function: as a __forceinline__ function the same statements cost
// k_pg_cls_lse<false,8> 6 - 8 % of its time (another register assignment in its K loop).
// Expects in scope: KhClsLseArgs a; constexpr R, NT; f32x4 acc[R][NT]; int trow[R]; bool valid[R] (wave-uniform); blk,
// tok0; wave, i = lane & 15, h = lane >> 4; and the LDS arrays the four waves exchange per token column through:
//   __shared__ float s_red[2][KH_CL_WAVES][16 * NT];  // [0] maxima, [1] sums
//   __shared__ float s_cv[2][KH_CL_WAVES][16 * NT];   // the waves' candidates of a round, by round parity
//   __shared__ int s_ci[2][KH_CL_WAVES][16 * NT];
// No include guard: a kernel body includes it.
  // ---- epilogue: lane (i, h) holds rows trow[r] + 4 h + c of token tok0 + 16 nt + i in acc[r][nt] component c
  const bool writer = wave == 0 && h == 0;  // the lane that stores column 16 nt + i of the records
  float mx[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (valid[r]) m = fmaxf(fmaxf(m, fmaxf(acc[r][nt].x, acc[r][nt].y)), fmaxf(acc[r][nt].z, acc[r][nt].w));
    m = xor32_max(xor16_max(m));
    if (h == 0) s_red[0][wave][16 * nt + i] = m;
  }
  __syncthreads();
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = 16 * nt + i;
    mx[nt] = fmaxf(fmaxf(s_red[0][0][col], s_red[0][1][col]), fmaxf(s_red[0][2][col], s_red[0][3][col]));
    float s = 0.f;
    if (mx[nt] > -INFINITY) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (valid[r]) {
          const float e = (expf(acc[r][nt].x - mx[nt]) + expf(acc[r][nt].y - mx[nt])) +
                          (expf(acc[r][nt].z - mx[nt]) + expf(acc[r][nt].w - mx[nt]));
          s = r == 0 ? e : s + e;
        }
    }
    s = xor32_sum(xor16_sum(s));
    if (h == 0) s_red[1][wave][col] = s;
  }
  __syncthreads();
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = 16 * nt + i, tok = tok0 + col;
    if (tok >= a.T) continue;  // padding tokens leave no record
    float* rec = a.ws + ((size_t)blk * a.ws_tokens + tok) * KH_CL_STRIDE;
    if (writer) {
      rec[0] = mx[nt];
      rec[1] = (s_red[1][0][col] + s_red[1][1][col]) + (s_red[1][2][col] + s_red[1][3][col]);
    }
    const int tgt = a.target ? a.target[tok] : -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int lr = tgt - trow[r] - 4 * h;
      if (valid[r] && (unsigned)lr < 4u) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (lr == c) rec[2] = pg_comp(acc[r][nt], c);
      }
    }
  }
  if (a.top_n <= 0) return;  // uniform (the epilogue is the end of its kernel)
  float lv[NT];
  int li[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    lv[nt] = INFINITY;
    li[nt] = -1;
  }
  for (int k = 0; k < a.top_n; ++k) {
    const int par = k & 1;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float bv = -INFINITY;
      int bi = KH_CL_NO_ID;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (valid[r]) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float v = pg_comp(acc[r][nt], c);
            const int id = trow[r] + 4 * h + c;
            if (cl_ahead(lv[nt], li[nt], v, id) && cl_ahead(v, id, bv, bi)) {  // behind the last one taken, ahead of the rest
              bv = v;
              bi = id;
            }
          }
        }
      cl_best_swap<false>(bv, bi);
      cl_best_swap<true>(bv, bi);
      if (h == 0) {
        s_cv[par][wave][16 * nt + i] = bv;
        s_ci[par][wave][16 * nt + i] = bi;
      }
    }
    __syncthreads();  // (the buffer of round k + 1 is the other one; that of round k + 2 is written behind the next barrier)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int col = 16 * nt + i, tok = tok0 + col;
      float bv = s_cv[par][0][col];
      int bi = s_ci[par][0][col];
#pragma unroll
      for (int w = 1; w < KH_CL_WAVES; ++w) {
        const float v = s_cv[par][w][col];
        const int id = s_ci[par][w][col];
        if (cl_ahead(v, id, bv, bi)) {
          bv = v;
          bi = id;
        }
      }
      lv[nt] = bv;
      li[nt] = bi;
      if (writer && tok < a.T) {
        float* rec = a.ws + ((size_t)blk * a.ws_tokens + tok) * KH_CL_STRIDE + KH_CL_HDR + 2 * k;
        rec[0] = bv;
        rec[1] = __int_as_float(bi);
      }
    }
  }
