// kh_model_seq_gemm.hip — the wide sequence pass (kh_seq_gemm.h): what kh_model_seq_step_gemm and
// kh_model_generate_batch_gemm (kh_model_seq.hip) enqueue.  One pass = up to KH_SEQ_SLOTS_MAX lanes of distinct slots at
// full depth: k_sg_embed; per layer k_pg_rmsnorm, the QKV GEMM on lanes (k_sg_rope behind it where its epilogue cannot
// rotate), the 8-lane pass's attention once per group of KH_PF_BMAX lanes, the wo GEMM, k_pg_rmsnorm, the SwiGLU GEMM,
// the w2 GEMM; the final k_pg_rmsnorm, the classifier GEMM (KH_PG_STORE) and the 8-lane pass's tail once per group.
// Slabs, launch shapes and hooks are the GEMM prefill's (ensure_pg_buffers, pg_plan).  The reference decodes one
// sequence per process (demo/main.cpp:16-50).
// gfx950 only.
#include "kh_dispatch.h"
#include "kh_model_internal.h"
#include "kh_seq_gemm.h"

using namespace khm;

namespace {
// the (R, NT) register tiles pg_plan can return for <= 64 tokens (no 128-token tile: NT = 8 runs as NT = 4)
constexpr int kSgTiles[3][2] = {{2, 4}, {2, 2}, {1, 4}};
constexpr int sg_tile(int R, int NT) {
  for (int i = 0; i < 3; ++i)
    if (kSgTiles[i][0] == R && kSgTiles[i][1] == NT) return i;
  return -1;
}
// One GEMM of the pass; returns what pg_launch returns: QKV - did the epilogue rotate; RESID - the K slices whose
// partial rows the next RMSNorm adds.  ok: cleared when the LDS opt-in of the shape is refused.
template <int EPI>
int sg_launch(kh_model* m, int rows_total, bool r2_ok, KhPgGemmArgs a, const KhWideLanes& lanes, bool* ok) {
  const bool q = m->cfg.is_quant;
  const int nm = EPI == KH_PG_SWIGLU ? 2 : 1;
  PgShape sh = pg_plan(m, EPI, a.T, rows_total, r2_ok, a.K);
  if (sh.NT > 4) {  // a hook asked for the 128-token tile
    sh.NT = 4;
    sh.slices = ((a.T + 15) / 16 + 3) / 4;
  }
  if (EPI == KH_PG_QKV && a.rope == KH_PG_ROPE_TILES && sh.R != 2) a.rope = KH_PG_ROPE_OFF;  // no partner tile in the wave
  const int tiles = rows_total / (16 * sh.R), wg = nm * sh.ks * 64;
  size_t lds = pg_lds_bytes(wg / 64, sh.NT);
  if (sh.solo && lds < KH_PG_SOLO_LDS) lds = KH_PG_SOLO_LDS;
  auto opt_in = [&](auto kern, dim3&) { return pg_lds_opt_in((const void*)kern, lds); };
  const int tile = sg_tile(sh.R, sh.NT);
  kh_pick_bool(q, [&](auto Q) {
    kh_pick(KhVals<0, 1, 2>{}, tile >= 0 ? tile : (sh.R == 2 ? 1 : 2), [&](auto I) {
      constexpr int R = kSgTiles[I][0], NT = kSgTiles[I][1];
      if (!kh_launch_prep(opt_in, KH_KERNEL(k_sg_gemm, Q, R, NT, EPI), dim3(tiles, sh.slices, sh.kz), wg, lds,
                          m->stream, a, lanes))
        *ok = false;
    });
  });
  if (EPI == KH_PG_RESID) return sh.kz > 1 ? sh.kz : 0;
  return EPI == KH_PG_QKV && a.rope != KH_PG_ROPE_OFF;
}
}  // namespace

bool khm::seq_gemm_supported(const kh_model* m) {
  // the 8-lane pass's attention and tail (full_depth_supported: their buffers are seq_prepare's), the GEMMs' K and row
  // granules, and a classifier of whole 16-row tiles
  return full_depth_supported(m) && pg_supported(m) && m->cfg.vocab_size % 16 == 0;
}

int khm::seq_gemm_prepare(kh_model* m) {
  int rc;
  if ((rc = ensure_pg_buffers(m)) != KH_OK) return rc;
  if (m->sg_logits) return KH_OK;
  KhDev<float> lg;
  const size_t n = (size_t)KH_SEQ_SLOTS_MAX * (size_t)m->pf_vstride;  // pf_vstride: seq_prepare ran
  if ((rc = lg.alloc(n)) != KH_OK) return rc;
  KH_CHECK_HIP(hipMemsetAsync(lg, 0, n * sizeof(float), m->stream));
  m->sg_logits = std::move(lg);
  return KH_OK;
}

int khm::seq_pass_enqueue_gemm(kh_model* m, const int32_t* slots, const int32_t* pos, int n, bool words,
                               const KhSeqTail* tail) {
  const kh_config& c = m->cfg;
  const bool q = c.is_quant;
  const int T = n, tcap = pg_tcap(T);
  if (n <= 0 || n > KH_SEQ_SLOTS_MAX) return KH_ERR_RANGE;
  KhWideLanes wide;
  for (int b = 0; b < KH_SEQ_SLOTS_MAX; ++b) {  // padding lanes repeat the last valid lane
    const int i = b < n ? b : n - 1;
    wide.pos[b] = pos[i];
    wide.row[b] = kh_seq_own_base(m->seq_tab[slots[i]]) + pos[i];
    wide.slot[b] = slots[i];
  }
  // lanes [g * KH_PF_BMAX ..) as the 8-lane table the attention and the tail read
  auto group = [&](int g, int* ng) {
    KhSeqLanes l;
    *ng = n - g * KH_PF_BMAX < KH_PF_BMAX ? n - g * KH_PF_BMAX : KH_PF_BMAX;
    for (int b = 0; b < KH_PF_BMAX; ++b) {
      const int i = g * KH_PF_BMAX + (b < *ng ? b : *ng - 1);
      const KhSeqSlot& t = m->seq_tab[slots[i]];
      l.pos[b] = wide.pos[i];
      l.row[b] = wide.row[i];
      l.slot[b] = wide.slot[i];
      l.pfx_len[b] = t.pfx;
      l.pfx_row0[b] = t.pfx > 0 ? m->seq_tab[t.parent].row0 : 0;
    }
    return l;
  };
  const int groups = (n + KH_PF_BMAX - 1) / KH_PF_BMAX;
  bool ok = true;
  launch_log("k_sg_embed");
  hipLaunchKernelGGL(k_sg_embed, dim3(T), dim3(KH_WG), 0, m->stream, (const int32_t*)m->d_seq_tok, wide, c.vocab_size,
                     (const float*)m->tok_emb, (float*)m->pg_x, c.dim);
  int pending_kz = 0;  // K slices of the last residual GEMM still to be added to pg_x (by the next RMSNorm)
  auto rmsnorm = [&](const float* w) {
    kh_pick_bool(q, [&](auto Q) {
      kh_launch(KH_KERNEL(k_pg_rmsnorm, Q), T, KH_WG, 0, m->stream, (float*)m->pg_x, w, (float*)m->pg_xn, c.dim,
                c.rms_eps, tcap, (const float*)m->pg_part, pending_kz);
    });
    pending_kz = 0;
  };
  const bool rope_fuse_env = !dbg_off("KH_PG_ROPE_FUSE");
  for (int l = 0; l < c.layer_num; ++l) {
    const LayerW& W = m->layers[l];
    float* kc = m->kcache + (size_t)l * c.cache_len * c.kv_dim;
    float* vc = m->vcache + (size_t)l * c.cache_len * c.kv_dim;
    rmsnorm(W.att_norm);
    bool rope_fused = false;
    {
      KhPgGemmArgs a{};
      a.w[0] = W.wq; a.w[1] = W.wk; a.w[2] = W.wv;
      a.B = m->pg_xn; a.b_tiled = 1; a.tcap = tcap; a.out = m->pg_q; a.kc = kc; a.vc = vc;
      a.rows0 = c.dim; a.rows1 = c.kv_dim; a.ldo = c.dim; a.K = c.dim; a.T = T; a.pos0 = 0;
      a.gshift = m->gshift;
      a.head_size = c.head_size; a.sin_cache = m->sin_cache; a.cos_cache = m->cos_cache;
      a.rope = !rope_fuse_env ? KH_PG_ROPE_OFF
               : (c.rope_mode == KH_ROPE_HALF ? (c.head_size % 32 == 0 ? KH_PG_ROPE_TILES : KH_PG_ROPE_OFF)
                                              : KH_PG_ROPE_PAIRS);
      rope_fused = sg_launch<KH_PG_QKV>(m, c.dim + 2 * c.kv_dim, c.dim % 32 == 0 && c.kv_dim % 32 == 0, a, wide, &ok) != 0;
    }
    if (!rope_fused) {
      launch_log("k_sg_rope");
      hipLaunchKernelGGL(k_sg_rope, dim3(T), dim3(KH_WG), 0, m->stream, (float*)m->pg_q, kc,
                         (const float*)m->sin_cache, (const float*)m->cos_cache, c.dim, c.kv_dim, c.head_size, wide,
                         (int)c.rope_mode);
    }
    for (int g = 0; g < groups; ++g) {
      int ng;
      const KhSeqLanes lg = group(g, &ng);
      const size_t at = (size_t)g * KH_PF_BMAX * c.dim;
      seq_attn_enqueue(m, l, m->pg_q + at, m->pg_att + at, lg, ng);
    }
    {
      KhPgGemmArgs a{};
      a.w[0] = W.wo;
      a.B = m->pg_att; a.b_tiled = 0; a.tcap = tcap; a.out = m->pg_x;  // the decode attention leaves row-major rows
      a.rows0 = c.dim; a.ldo = c.dim; a.K = c.dim; a.T = T; a.gshift = m->gshift; a.part = m->pg_part;
      pending_kz = sg_launch<KH_PG_RESID>(m, c.dim, c.dim % 32 == 0, a, wide, &ok);
    }
    rmsnorm(W.ffn_norm);
    {
      KhPgGemmArgs a{};
      a.w[0] = W.w1; a.w[1] = W.w3;
      a.B = m->pg_xn; a.b_tiled = 1; a.tcap = tcap; a.out = m->pg_h;
      a.rows0 = c.hidden_dim; a.ldo = c.hidden_dim; a.K = c.dim; a.T = T; a.gshift = m->gshift;
      sg_launch<KH_PG_SWIGLU>(m, c.hidden_dim, c.hidden_dim % 32 == 0, a, wide, &ok);
    }
    {
      KhPgGemmArgs a{};
      a.w[0] = W.w2;
      a.B = m->pg_h; a.b_tiled = 1; a.tcap = tcap; a.out = m->pg_x;
      a.rows0 = c.dim; a.ldo = c.dim; a.K = c.hidden_dim; a.T = T; a.gshift = m->gshift; a.part = m->pg_part;
      pending_kz = sg_launch<KH_PG_RESID>(m, c.dim, c.dim % 32 == 0, a, wide, &ok);
    }
  }
  rmsnorm(m->final_norm);  // adds the last w2 GEMM's pending partials too
  {
    KhPgGemmArgs a{};
    a.w[0] = m->cls;
    a.B = m->pg_xn; a.b_tiled = 1; a.tcap = tcap; a.out = m->sg_logits;
    a.rows0 = c.vocab_size; a.ldo = m->pf_vstride; a.K = c.dim; a.T = T; a.gshift = m->gshift;
    sg_launch<KH_PG_STORE>(m, c.vocab_size, c.vocab_size % 32 == 0, a, wide, &ok);
  }
  m->sg_lanes = n;
  for (int g = 0; g < groups; ++g) {
    int ng, rc;
    const KhSeqLanes lg = group(g, &ng);
    if ((rc = seq_tail_enqueue(m, m->sg_logits + (size_t)g * KH_PF_BMAX * m->pf_vstride, lg, ng, words, tail)) != KH_OK)
      return rc;
  }
  if (!ok) return KH_ERR_UNSUPPORTED;  // a GEMM shape's LDS opt-in was refused
  return kh_launch_status();
}
