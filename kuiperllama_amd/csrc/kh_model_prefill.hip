// kh_model_prefill.hip — prompt phase of the model level: the B-token VALU pass (kh_prefill.h, bit-identical to
// token-by-token; ONE layer driver, launch_pf_pass) and what runs on it - the prompt prefill, sequence scoring
// (kh_model_score: k_pf_cls, k_score_lp), the verify pass of speculative decode (kh_model_verify[_as_set]: k_pf_cls,
// kh_spec.h) and the pass over lanes of different sequences (kh_seq.h; kh_model_seq.hip drives it); for a W16 model
// the launch classes of its pass mask run on the 16-bit copy (kh_w16_pass.h, the w16_pf_* launchers) - and the
// fp32-MFMA GEMM prefill (kh_gemm.h, kh_pattn.h), which always reads fp32.  The
// reference feeds the prompt one token per forward pass (demo/main.cpp:20-22).
// gfx950 only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kh_dispatch.h"
#include "kh_gemm.h"
#include "kh_logprobs.h"
#include "kh_model_internal.h"
#include "kh_pattn.h"
#include "kh_pf_launch.h"
#include "kh_prefill.h"
#include "kh_score_plan.h"
#include "kh_seq.h"
#include "kh_seq_prefill.h"
#include "kh_spec.h"
#include "kh_w16_pass.h"

using namespace khm;

namespace khm {
// The B-token kernels mirror the decode kernels' arithmetic only for the staging variant the
// decode path uses at these sizes (in-register, at most 4 float4 per thread) and for the fast attention core.
bool prefill_supported(const kh_model* m) {
  const kh_config& c = m->cfg;
  if (c.head_size <= 32) return false;
  if (!kh_stage_fits4(c.dim, m->sh_qkv.wg) || !kh_stage_fits4(c.dim, m->sh_ffn.wg)) return false;
  if (m->sh_qkv.split > 2 || m->sh_ffn.split != 1) return false;
  if (pf_lds_bytes(c.is_quant, c.dim, 4) > 160 * 1024) return false;
  if (pf_lds_bytes(c.is_quant, c.hidden_dim, 2) > 160 * 1024) return false;
  return true;
}
// the full-depth pass ends in k_pf_cls, which stages like k_cls at the classifier's workgroup width
bool full_depth_supported(const kh_model* m) {
  return prefill_supported(m) && kh_stage_fits4(m->cfg.dim, m->sh_cls.wg);
}
bool pg_supported(const kh_model* m) {
  const kh_config& c = m->cfg;
  if (c.head_size <= 32) return false;  // attention: the fast multi-token decode kernel
  const int kq = c.is_quant ? 64 : 16;  // K granule of one MFMA operand load
  if (c.dim % kq || c.hidden_dim % kq || c.dim % 16 || c.kv_dim % 16 || c.hidden_dim % 16) return false;
  if (c.is_quant && m->gshift != 6) return false;
  return true;
}
}  // namespace khm

// ---- prompt prefill (kh_prefill.h) ---------------------------------------------------------------
namespace {
// tokens per pass of the dim-input matrices (qkv, wo, ffn13)
int prefill_batch(const kh_model* m) {
  const kh_config& c = m->cfg;
  if (!c.is_quant && pf_lds_bytes(false, c.dim, 8) <= 80 * 1024) return 8;
  return 4;
}
int ensure_prefill_buffers(kh_model* m) {
  if (m->pf_x) return KH_OK;
  const kh_config& c = m->cfg;
  KhDev<float> x, q, att, h;
  KhDev<char> ws;
  int rc;
  if ((rc = x.alloc((size_t)KH_PF_BMAX * c.dim)) != KH_OK || (rc = q.alloc((size_t)KH_PF_BMAX * c.dim)) != KH_OK ||
      (rc = att.alloc((size_t)KH_PF_BMAX * c.dim)) != KH_OK || (rc = h.alloc((size_t)KH_PF_BMAX * c.hidden_dim)) != KH_OK)
    return rc;
  const size_t tok_bytes = (attn_ws_bytes(c.head_num, c.head_size, m->attn_ws_stride) + 255) & ~(size_t)255;
  if (tok_bytes) {
    if ((rc = ws.alloc(tok_bytes * KH_PF_BMAX)) != KH_OK) return rc;
    KH_CHECK_HIP(hipMemsetAsync(ws, 0, tok_bytes * KH_PF_BMAX, m->stream));
  }
  m->pf_ws_tok_bytes = tok_bytes;
  m->pf_x = std::move(x);
  m->pf_q = std::move(q);
  m->pf_att = std::move(att);
  m->pf_h = std::move(h);
  m->pf_ws = std::move(ws);
  return KH_OK;
}
// ---- the twins on the 16-bit copy (kh_pf_launch.h): this translation unit compiles the _w16 kernels; an fp16-format
// copy goes to kh_model_h16_pass.hip, which compiles the _h16 kernels from the same launch text
inline bool f16_copy(const kh_model* m) { return m->w16.format == KH_W16_F16; }
void w16_pf_qkv(kh_model* m, int l, const KhPfQkvArgs& fp32, const KhSeqLanes* lanes, int B) {
  f16_copy(m) ? h16_pf_qkv(m, l, fp32, lanes, B) : w16_pf_qkv_fmt<KH_W16_BF16>(m, l, fp32, lanes, B);
}
void w16_pf_ffn13(kh_model* m, int l, const KhPfFfn13Args& fp32, int B) {
  f16_copy(m) ? h16_pf_ffn13(m, l, fp32, B) : w16_pf_ffn13_fmt<KH_W16_BF16>(m, l, fp32, B);
}
void w16_pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& fp32, int bs) {
  f16_copy(m) ? h16_pf_gemv_res(m, l, cls, sh, fp32, bs) : w16_pf_gemv_res_fmt<KH_W16_BF16>(m, l, cls, sh, fp32, bs);
}
void w16_pf_cls(kh_model* m, const KhPfClsArgs& fp32, int B) {
  f16_copy(m) ? h16_pf_cls(m, fp32, B) : w16_pf_cls_fmt<KH_W16_BF16>(m, fp32, B);
}
// y = W.v ; X += y for the nvalid tokens of the chunk, in sub-batches of the largest of 8/4/2
// tokens (<= bmax) whose input vectors fit LDS.  w: layer l's wo (cls = KH_W16_WO) or w2 (KH_W16_W2)
void pf_gemv_res(kh_model* m, int l, int cls, const kh_model::Shape& sh, const KhLin& w, const float* V, float* X,
                 int M, int K, int nvalid, int bmax) {
  const bool q = m->cfg.is_quant;
  int bs = bmax;
  while (bs > 2 && pf_lds_bytes(q, M, bs) > 160 * 1024) bs >>= 1;
  KhPfGemvResArgs a;
  a.w = w;
  a.M = M;
  a.K = K;
  a.gshift = m->gshift;
  for (int t0 = 0; t0 < nvalid; t0 += bs) {
    a.V = V + (size_t)t0 * M;
    a.X = X + (size_t)t0 * K;
    a.nvalid = nvalid - t0 < bs ? nvalid - t0 : bs;
    if (w16_pass_runs(m, cls)) {  // the same shape on the 16-bit copy
      w16_pf_gemv_res(m, l, cls, sh, a, bs);
      continue;
    }
    pick_pf<PfGemvResB, PfGemvResSP>(q, sh.split, bs, [&](auto Q, auto SP, auto B) {
      pf_launch(KH_KERNEL(k_pf_gemv_res, Q, SP, B), sh, pf_lds_bytes(Q, M, B), m->stream, a);
    });
  }
}
// One pass of nvalid (<= B) tokens through the B-token kernels.  Where a token's id, its RoPE row and its cache row
// come from is the only thing the callers differ in:
//   a run (lanes = null)  toks[b] sits at position pos0 + b of the sequence whose position 0 is cache row row0 (a
//                         sequence slot's first row; 0 for the batch-1 entry points): k_pf_embed, k_pf_qkv,
//                         k_attn_decode.  Without full_depth the pass fills the tokens' K/V cache rows and stops
//                         behind the last layer's; with it (scoring, verify) the last layer's attention, wo and FFN
//                         run too and pf_x holds the tokens' final residual vectors
//   a lane table          lane b feeds d_seq_tok[slot[b]] at position pos[b], cache row row[b] (kh_seq.h): k_seq_embed,
//                         k_seq_qkv, k_seq_attn.  Always full depth
//   a run into a slot that shares a prefix (pfx_len > 0, kh_model_seq_share): row0 is the slot's own base (the row of
//                         its first own position minus pfx_len; it may be negative, rows below pos0 >= pfx_len are
//                         never touched through it), positions [0, pfx_len) are the parent's rows pfx_row0 ..:
//                         k_pf_embed and k_pf_qkv as any run, the attention as k_seq_attn_pfx over a lane table of
//                         the run's positions - the same slices in the same launch order
// wo, ffn13 and w2 do not care where a token sits.
struct PfPass {
  int nvalid, B;
  bool full_depth;
  const int32_t* toks;
  int pos0, row0;
  const KhSeqLanes* lanes;
  int pfx_len = 0, pfx_row0 = 0;
};
PfPass pf_run(const int32_t* toks, int nvalid, int pos0, int B, bool full_depth, int row0 = 0, int pfx_len = 0,
              int pfx_row0 = 0) {
  return PfPass{nvalid, B, full_depth, toks, pos0, row0, nullptr, pfx_len, pfx_row0};
}
PfPass pf_lanes(const KhSeqLanes& lanes, int nvalid, int B) { return PfPass{nvalid, B, true, nullptr, 0, 0, &lanes}; }
// layer l's k_pf_qkv / k_seq_qkv arguments: cache rows counted from row0, RoPE rows from pos0 (a lane table brings
// its own of both: 0, 0)
KhPfQkvArgs pf_qkv_args(const kh_model* m, int l, const PfPass& p) {
  const kh_config& c = m->cfg;
  const LayerW& W = m->layers[l];
  KhPfQkvArgs a;
  a.X = m->pf_x;
  a.att_norm = W.att_norm;
  a.wq = W.wq;
  a.wk = W.wk;
  a.wv = W.wv;
  a.Q = m->pf_q;
  const ptrdiff_t row = (ptrdiff_t)l * c.cache_len + p.row0;  // signed: a sharer's own base may lie below row 0
  a.kcache_layer = m->kcache + row * c.kv_dim;
  a.vcache_layer = m->vcache + row * c.kv_dim;
  a.sin_cache = m->sin_cache;
  a.cos_cache = m->cos_cache;
  a.dim = c.dim;
  a.kv_dim = c.kv_dim;
  a.head_size = c.head_size;
  a.rope_mode = c.rope_mode;
  a.gshift = m->gshift;
  a.pos0 = p.pos0;
  a.nvalid = p.nvalid;
  a.eps = c.rms_eps;
  return a;
}
void launch_pf_pass(kh_model* m, const PfPass& p) {
  const kh_config& c = m->cfg;
  const bool q = c.is_quant;
  const int nvalid = p.nvalid, B = p.B;
  if (p.lanes) {
    launch_log("k_seq_embed");
    hipLaunchKernelGGL(k_seq_embed, dim3(B), dim3(KH_WG), 0, m->stream, (const int32_t*)m->d_seq_tok, *p.lanes, nvalid,
                       c.vocab_size, m->tok_emb, m->pf_x, c.dim);
  } else {
    KhPfTokens tk;
    for (int b = 0; b < KH_PF_BMAX; ++b) tk.t[b] = p.toks[b < nvalid ? b : nvalid - 1];
    hipLaunchKernelGGL(k_pf_embed, dim3(B), dim3(KH_WG), 0, m->stream, tk, m->tok_emb, m->pf_x, c.dim);
  }
  for (int l = 0; l < c.layer_num; ++l) {
    const LayerW& W = m->layers[l];
    // the instantiations of k_seq_qkv are k_pf_qkv's (PfB x PfQkvSP)
    if (w16_pass_runs(m, KH_W16_QKV)) {  // the same shape on the 16-bit copy
      w16_pf_qkv(m, l, pf_qkv_args(m, l, p), p.lanes, B);
    } else {
      pick_pf<PfB, PfQkvSP>(q, m->sh_qkv.split, B, [&](auto Q, auto SP, auto BB) {
        const size_t lds = pf_lds_bytes(Q, c.dim, BB);
        if (p.lanes)
          pf_launch(KH_KERNEL(k_seq_qkv, Q, SP, BB), m->sh_qkv, lds, m->stream,
                    KhSeqQkvArgs{pf_qkv_args(m, l, p), *p.lanes});
        else
          pf_launch(KH_KERNEL(k_pf_qkv, Q, SP, BB), m->sh_qkv, lds, m->stream, pf_qkv_args(m, l, p));
      });
    }
    // the prompt phase leaves K/V rows and nothing else (no logits): the last layer's K/V rows are
    // written, its attention, wo and FFN feed nothing - unless the classifier follows (full_depth)
    if (l == c.layer_num - 1 && !p.full_depth) break;
    {
      KhAttnArgs a = fill_attn(m, l, /*variant=*/0, m->attn_fenced);
      a.defer = 0;  // multi-token slices merge in the launch
      a.nsplit_g = m->attn_ns_g;  // not the decode step's variant: the launch plan decides from the slices' positions
      a.q = m->pf_q;
      a.out = m->pf_att;
      a.d_pos = nullptr;
      a.ws = m->pf_ws;
      a.tok_stride = c.dim;
      a.ws_tok_bytes = m->pf_ws_tok_bytes;
      if (p.lanes) {
        if (seq_lanes_share(*p.lanes, nvalid))
          launch_seq_attn_pfx(a, *p.lanes, nvalid, m->attn_wg, m->stream, m->seq_pfx_pad8);
        else
          launch_seq_attn(a, *p.lanes, nvalid, m->attn_wg, m->stream);
      } else if (p.pfx_len > 0) {
        KhSeqLanes run;
        for (int b = 0; b < KH_PF_BMAX; ++b) {
          const int bb = b < nvalid ? b : nvalid - 1;
          run.pos[b] = p.pos0 + bb;
          run.row[b] = p.row0 + p.pos0 + bb;
          run.slot[b] = 0;
          run.pfx_len[b] = p.pfx_len;
          run.pfx_row0[b] = p.pfx_row0;
        }
        launch_seq_attn_pfx(a, run, nvalid, m->attn_wg, m->stream, m->seq_pfx_pad8);
      } else {
        a.kcache_layer += (size_t)p.row0 * c.kv_dim;
        a.vcache_layer += (size_t)p.row0 * c.kv_dim;
        launch_attn_decode(a, p.pos0, m->attn_wg, m->stream, nvalid, p.pos0 + nvalid - 1);
      }
    }
    pf_gemv_res(m, l, KH_W16_WO, m->sh_wo, W.wo, m->pf_att, m->pf_x, c.dim, c.dim, nvalid, B);
    {
      KhPfFfn13Args a;
      a.X = m->pf_x;
      a.ffn_norm = W.ffn_norm;
      a.w1 = W.w1;
      a.w3 = W.w3;
      a.H = m->pf_h;
      a.dim = c.dim;
      a.hidden = c.hidden_dim;
      a.gshift = m->gshift;
      a.nvalid = nvalid;
      a.eps = c.rms_eps;
      if (w16_pass_runs(m, KH_W16_FFN13))
        w16_pf_ffn13(m, l, a, B);
      else
        pick_pf<PfB, PfNoSP>(q, 1, B, [&](auto Q, auto, auto BB) {
          pf_launch(KH_KERNEL(k_pf_ffn13, Q, BB), m->sh_ffn, pf_lds_bytes(Q, c.dim, BB), m->stream, a);
        });
    }
    pf_gemv_res(m, l, KH_W16_W2, m->sh_w2, W.w2, m->pf_h, m->pf_x, c.hidden_dim, c.dim, nvalid, B);
  }
}
// ---- sequence scoring: the classifier and the records behind a full-depth chunk -------------------
int ensure_score_buffers(kh_model* m) {
  if (m->pf_logits) return KH_OK;
  m->pf_vstride = (m->cfg.vocab_size + 3) & ~3;
  return m->pf_logits.alloc((size_t)KH_PF_BMAX * m->pf_vstride);
}
// logits of the chunk's tokens behind a full-depth pass (k_cls's arithmetic on pf_x, the decode classifier's workgroup
// width): rows 0 .. nvalid - 1 of pf_logits
void launch_pf_cls(kh_model* m, int nvalid, int B) {
  const kh_config& c = m->cfg;
  KhPfClsArgs a;
  a.X = m->pf_x;
  a.final_norm = m->final_norm;
  a.wcls = m->cls;
  a.logits = m->pf_logits;
  a.dim = c.dim;
  a.vocab = c.vocab_size;
  a.vstride = m->pf_vstride;
  a.gshift = m->gshift;
  a.nvalid = nvalid;
  a.eps = c.rms_eps;
  if (w16_pass_runs(m, KH_W16_CLS)) return w16_pf_cls(m, a, B);
  pick_pf<PfB, PfNoSP>(c.is_quant, 1, B, [&](auto Q, auto, auto BB) {
    pf_launch(KH_KERNEL(k_pf_cls, Q, BB), m->sh_cls, pf_lds_bytes(Q, c.dim, BB), m->stream, a);
  });
}
// the classifier, then the record of every position: target[b] = the token fed behind token b, -1 behind the last
// token of the call
void launch_score_tail(kh_model* m, const int32_t* target, int nvalid, int pos0, int B) {
  const kh_config& c = m->cfg;
  launch_pf_cls(m, nvalid, B);
  KhScoreLpArgs t;
  t.logits = m->pf_logits;
  t.vstride = m->pf_vstride;
  t.vocab = c.vocab_size;
  for (int b = 0; b < KH_PF_BMAX; ++b) t.target[b] = b < nvalid ? target[b] : -1;
  t.pos0 = pos0;
  t.top_n = m->d_lp_top_n;
  t.rec_token = m->d_lp_token;
  t.rec_lp = m->d_lp_lp;
  t.rec_top_ids = m->d_lp_top_ids;
  t.rec_top_lp = m->d_lp_top_lp;
  t.rec_cap = m->lp_cap;
  launch_log("k_score_lp");
  hipLaunchKernelGGL(k_score_lp, dim3(nvalid), dim3(KH_SAMP_THREADS), 0, m->stream, t);
}
}  // namespace

// ---- GEMM prefill (kh_gemm.h) ------------------------------------------------------------------
int khm::ensure_pg_buffers(kh_model* m) {
  if (m->pg_x) return KH_OK;
  const kh_config& c = m->cfg;
  const size_t T = KH_PG_TMAX;
  int rc;
  auto zalloc = [&](KhDev<float>& b, size_t n) -> int {
    if ((rc = b.alloc(n)) != KH_OK) return rc;
    // rows beyond the valid tokens are read as MFMA operands (their columns are discarded):
    // they must hold finite numbers
    return (int)hipMemsetAsync(b, 0, n * sizeof(float), m->stream);
  };
  // a failure half-way leaves the model without any slab: a later call starts over
  KhDev<float> x, xn, q, att, h, part;
  if ((rc = zalloc(x, T * c.dim)) != KH_OK || (rc = zalloc(xn, T * c.dim)) != KH_OK ||
      (rc = zalloc(q, T * c.dim)) != KH_OK || (rc = zalloc(att, T * c.dim)) != KH_OK ||
      (rc = zalloc(h, T * c.hidden_dim)) != KH_OK ||
      (rc = zalloc(part, (size_t)KH_PG_KZ_MAX * T * c.dim)) != KH_OK)  // K-slice partial rows
    return rc;
  m->pg_x = std::move(x);
  m->pg_xn = std::move(xn);
  m->pg_q = std::move(q);
  m->pg_att = std::move(att);
  m->pg_h = std::move(h);
  m->pg_part = std::move(part);
  return KH_OK;
}
namespace {
// does the prompt-slice attention run on the MFMA kernel (kh_pattn.h)?  KH_PG_ATTN=0 forces the fallback.
bool pg_mfma_attn(const kh_model* m) { return !dbg_off("KH_PG_ATTN") && pg_attn_supported(m->cfg.head_size); }
// The split workspace of the decode-attention FALLBACK (one per token of a pass, ~270 KB per token at
// Llama-3.2-1B geometry: 136 MB for a 512-token pass).  Every BASELINE head size has an MFMA
// instantiation, so it is allocated on the first pass that actually takes the fallback.
int ensure_pg_ws(kh_model* m) {
  if (m->pg_ws || pg_mfma_attn(m)) return KH_OK;
  m->pg_ws_tok_bytes = (attn_ws_bytes(m->cfg.head_num, m->cfg.head_size, m->attn_ws_stride) + 255) & ~(size_t)255;
  if (!m->pg_ws_tok_bytes) return KH_OK;
  KhDev<char> ws;
  int rc;
  if ((rc = ws.alloc(m->pg_ws_tok_bytes * (size_t)KH_PG_TMAX)) != KH_OK) return rc;
  KH_CHECK_HIP(hipMemsetAsync(ws, 0, m->pg_ws_tok_bytes * (size_t)KH_PG_TMAX, m->stream));
  m->pg_ws = std::move(ws);
  return KH_OK;
}
// the (R, NT) register tiles k_pg_gemm is compiled for, and the waves per SIMD that fit with each
constexpr int kPgTiles[4][3] = {{2, 8, 2}, {2, 4, 3}, {2, 2, 4}, {1, 4, 4}};
constexpr int pg_tile(int R, int NT) {  // index in kPgTiles, -1: no such tile
  for (int i = 0; i < 4; ++i)
    if (kPgTiles[i][0] == R && kPgTiles[i][1] == NT) return i;
  return -1;
}
// Launch shape of one prefill GEMM (kh_gemm.h): R 16-row tiles and NT 16-token tiles per wave,
// ks waves splitting K per workgroup, grid.y token slices.  Picked by a small cost model of the
// busiest SIMD, fitted to a sweep on Llama-3.2-1B (profiles/r2_gemm_shape_sweep.txt):
//   * a workgroup lives on ONE CU: fewer than 256 workgroups leave CUs idle (the model prices the
//     busiest CU, so such shapes simply show their long per-wave work);
//   * fp32: ONE wave per SIMD is the sweet spot: two MFMA-bound waves on a SIMD cost ~1.6x the
//     time of the same work in one wave (the (w1,w3) GEMM went 140 -> 84 us per launch from 8 to 4
//     waves per CU), three or more ~1.8x;  int8: the opposite - its waves spend VALU time on the
//     dequant between MFMAs, so a second and third wave per SIMD fill the matrix pipe
//     (profiles/r2_gemm_shape_sweep_7b.txt: (w1,w3) 2 -> 4 waves per workgroup 30.4 -> 23.3 ms per
//     prefill), up to what the register file admits;
//     (these penalties were fitted with the phase scheme in every fp32 loop; since the uniform
//     operand rings of kh_gemm.h a second wave per SIMD costs less - (w1,w3) with 8 instead of 4
//     waves per workgroup: 3.01 vs 2.75 ms per 128-token pass - but still loses, and a re-sweep of
//     13 forced shapes leaves every choice of the model in place, profiles/r3_prefill_shapes512.txt);
//   * bigger register tiles need fewer operand bytes per MFMA (small factor), more token slices
//     re-read the weights from L2 (small factor), padding tokens are wasted MFMAs;
//   * fp32 passes of more than 128 tokens launch several times 256 workgroups, which would sit two
//     or more to a CU - two or more MFMA-bound waves per SIMD.  `solo` keeps ONE workgroup per CU at
//     a time (a dynamic-LDS request above half the CU's 160 KiB; the workgroups of a CU then run back
//     to back at the one-wave-per-SIMD rate) and is priced as such: Llama-3.2-1B, 512-token pass,
//     56.4 k prompt tok/s with it, 38.0 k without (profiles/r3_prefill_wide.txt).  Passes of <= 128
//     tokens use it for the MFMA-bound (2,8) tile only (Llama-2-7B fp32: 344 / 384 workgroups); their
//     small latency-bound tiles gain from a partner wave, and whole rounds of 256 cost more than
//     they save (Qwen2.5, (1,4) tile in 608 workgroups: 45.9 k shared, 41.8 k solo).
//   * the residual GEMMs (wo, w2) may split K across `kz` workgroups as well (blockIdx.z): with 2048
//     rows x 128 tokens there are only 64 (2,8) tiles, so a chip-filling launch either takes small
//     tiles or more K slices than a workgroup has waves.  The slices store partial rows and the
//     RMSNorm kernel that follows adds them in fixed order (kh_gemm.h) - no ticket, no second launch.
// hooks read per call (kh_debug_set takes effect on the next launch plan)
static inline bool pg_solo_on() { return !dbg_off("KH_PG_SOLO"); }
static inline bool pg_kz_on() { return !dbg_off("KH_PG_KZ"); }
}  // namespace
PgShape khm::pg_shape(int T, int rows_total, bool r2_ok, int nm, int kblocks, int min_blocks, bool quant,
                      bool allow_kz) {
  const int nt_all = (T + 15) / 16;
  const bool wide = nt_all > 8;  // a pass of more than 128 tokens
  PgShape best{1, 4, 1, (nt_all + 3) / 4, false, 1};
  double best_cost = -1.0;
  for (const auto& c : kPgTiles) {
    const int R = c[0], NT = c[1], occ = c[2];
    if (R == 2 && !r2_ok) continue;
    if (R == 1 && quant && r2_ok) continue;  // int8: the 32-row tile measured better wherever it fits
    if (NT > 4 && nt_all <= 4) continue;     // no 128-token tile for <= 64 tokens
    const int slices = (nt_all + NT - 1) / NT;
    for (int kz = 1; kz <= (allow_kz && pg_kz_on() ? KH_PG_KZ_MAX : 1); kz *= 2)
    for (int ks = 1; ks * nm * 64 <= KH_PG_WG_MAX(quant); ks *= 2) {
      const long wgs = (long)(rows_total / (16 * R)) * slices * kz;
      if (ks * kz > 1 && kblocks / (ks * kz) < min_blocks) break;  // keep a useful K range per wave
      // waves per SIMD on the busiest CU.  A workgroup counts as one wave on EACH SIMD it touches:
      // two 2-wave workgroups on a CU were measured on the same two SIMDs (Llama-3.2-1B, 256 tokens:
      // the (2,8) SwiGLU tile with 2-wave workgroups 255 us against 2 x 83 us for two 128-token
      // launches of 4-wave workgroups)
      const long cu_wgs = (wgs + 255) / 256;
      long wps = cu_wgs * ((nm * ks + 3) / 4);
      const long rounds = (wps + occ - 1) / occ;                    // beyond the register file: queued
      if (wps > occ) wps = occ;
      const double pen = quant ? (wps <= 1 ? 1.0 : (wps == 2 ? 0.72 : 0.62))
                               : (wps <= 1 ? 1.0 : (wps == 2 ? 1.6 : 1.8));
      const double per_wave = (double)((kblocks + ks * kz - 1) / (ks * kz)) * R * NT;
      double cost = per_wave * (double)(wps * rounds) * pen;
      cost *= 1.0 + 0.04 * (double)(kz - 1);  // partial rows written, and read back by the RMSNorm
      cost *= 1.0 + 0.15 * (double)(R + NT) / (double)(R * NT);
      // every token slice re-reads the weights from L2 - and, int8, dequantises them again
      cost *= 1.0 + (quant ? 0.15 : 0.05) * (double)(slices - 1);
      cost *= (double)(slices * NT) / (double)nt_all;
      bool solo = false;
      if (!quant && (wide || R * NT >= 16) && pg_solo_on() && wgs > 256) {
        const long wg_wps = (nm * ks + 3) / 4;
        const double c1 = per_wave * (double)(((wgs + 255) / 256) * wg_wps) * (wg_wps <= 1 ? 1.0 : (wg_wps == 2 ? 1.6 : 1.8));
        if (c1 < per_wave * (double)(wps * rounds) * pen) {
          cost *= c1 / (per_wave * (double)(wps * rounds) * pen);
          solo = true;
        }
      }
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost;
        best = PgShape{R, NT, ks, slices, solo, kz};
      }
    }
  }
  return best;
}
bool khm::pg_lds_opt_in(const void* kern, size_t lds) {
  if (lds > 48 * 1024) {
    // the >48 KiB dynamic-LDS opt-in is per (device, kernel): set once, not on every launch of
    // the prefill hot path; a refusal is reported here, not as a generic launch error later
    struct Done { int dev; const void* fn; size_t lds; };
    static thread_local std::vector<Done> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    bool hit = false;
    for (const auto& d : done) hit = hit || (d.dev == dev && d.fn == kern && d.lds >= lds);
    if (!hit) {
      if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
      done.push_back({dev, kern, lds});
    }
  }
  return true;
}
// The launch shape of one GEMM of a pass: the cost model, the KH_PG_SHAPE_<QKV|RESID|SWIGLU|STORE> hook, KH_PG_DEBUG.
// epi: KH_PG_*; STORE (the classifier GEMM of the wide sequence pass) plans as a residual GEMM without a K split
// across workgroups.
PgShape khm::pg_plan(const kh_model* m, int EPI, int T, int rows_total, bool r2_ok, int K) {
  const bool q = m->cfg.is_quant;
  const int nm = EPI == KH_PG_SWIGLU ? 2 : 1;
  PgShape sh = pg_shape(T, rows_total, r2_ok, nm, K / (q ? 64 : 16), q ? 4 : 16, q, EPI == KH_PG_RESID);
  {  // tuning hook: KH_PG_SHAPE_<QKV|RESID|SWIGLU|STORE>="R,NT,ks[,kz]" overrides the heuristic
    static const char* const names[4] = {"KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU",
                                         "KH_PG_SHAPE_STORE"};
    const char* const ov = dbg(names[EPI]);
    if (ov) {
      int R = 0, NT = 0, ks = 0, kz = 1;
      if (sscanf(ov, "%d,%d,%d,%d", &R, &NT, &ks, &kz) >= 3 && pg_tile(R, NT) >= 0 && (R != 2 || r2_ok) &&
          (ks == 1 || ks == 2 || ks == 4 || ks == 8) && ks * nm * 64 <= KH_PG_WG_MAX(q) &&
          (kz == 1 || (EPI == KH_PG_RESID && (kz == 2 || kz == 4))))
      {
        const int slices = ((T + 15) / 16 + NT - 1) / NT;
        sh = PgShape{R, NT, ks, slices,
                     !q && (T > 128 || R * NT >= 16) && pg_solo_on() && (long)(rows_total / (16 * R)) * slices * kz > 256, kz};
      } else {
        // not a launch this GEMM has (e.g. R = 2 where 32 rows do not divide the matrices): say so rather than
        // let a test believe it forced a shape
        fprintf(stderr, "[kh] %s=\"%s\" rejected (R,NT 1,4%s, ks 1/2/4/8 up to %d waves%s): heuristic shape\n",
                names[EPI], ov, r2_ok ? " or 2,2/4/8" : "", KH_PG_WG_MAX(q) / 64 / nm,
                EPI == KH_PG_RESID ? ", kz 1/2/4" : "");
      }
    }
  }
  if (dbg("KH_PG_DEBUG"))
    fprintf(stderr, "[pg] epi %d rows %d K %d T %d -> R %d NT %d slices %d ks %d kz %d (%d wgs x %d waves%s)\n", EPI,
            rows_total, K, T, sh.R, sh.NT, sh.slices, sh.ks, sh.kz, rows_total / (16 * sh.R) * sh.slices * sh.kz,
            nm * sh.ks, sh.solo ? ", solo" : "");
  return sh;
}
namespace {
// rg: the tokens are the tiles of a pass into sequence slots (kh_seq_prefill.h) - the QKV GEMM is then k_rg_gemm, the
// same statements under the tile address, in the same launch geometry
template <bool Q, int EPI>
bool pg_launch_cfg(const PgShape& sh, int tiles, int wg, hipStream_t s, const KhPgGemmArgs& a, const KhRgTiles* rg) {
  size_t lds = pg_lds_bytes(wg / 64, sh.NT);
  if (sh.solo && lds < KH_PG_SOLO_LDS) lds = KH_PG_SOLO_LDS;  // one workgroup per CU at a time
  auto opt_in = [&](auto kern, dim3&) { return pg_lds_opt_in((const void*)kern, lds); };
  const int tile = pg_tile(sh.R, sh.NT);  // one that is not listed runs as (2,2) where R is 2, else as (1,4)
  bool ok = false;
  kh_pick(KhVals<0, 1, 2, 3>{}, tile >= 0 ? tile : (sh.R == 2 ? 2 : 3), [&](auto I) {
    constexpr int R = kPgTiles[I][0], NT = kPgTiles[I][1];
    if constexpr (EPI == KH_PG_QKV) {
      if (rg) {
        ok = kh_launch_prep(opt_in, KH_KERNEL(k_rg_gemm, Q, R, NT, EPI), dim3(tiles, sh.slices, sh.kz), wg, lds, s, a, *rg);
        return;
      }
    }
    ok = kh_launch_prep(opt_in, KH_KERNEL(k_pg_gemm, Q, R, NT, EPI), dim3(tiles, sh.slices, sh.kz), wg, lds, s, a);
  });
  return ok;
}
// returns whether the QKV epilogue rotates q / k itself (else k_pg_rope has to follow); RESID: the
// number of K slices whose partial rows the next RMSNorm has to add (0 = the epilogue added itself)
template <int EPI>
int pg_launch(kh_model* m, int rows_total, bool r2_ok, KhPgGemmArgs a, const KhRgTiles* rg = nullptr) {
  const bool q = m->cfg.is_quant;
  const int nm = EPI == KH_PG_SWIGLU ? 2 : 1;
  const PgShape sh = pg_plan(m, EPI, a.T, rows_total, r2_ok, a.K);
  if (EPI == KH_PG_QKV && a.rope == KH_PG_ROPE_TILES && (sh.R != 2 || sh.NT > 4))
    a.rope = KH_PG_ROPE_OFF;  // no partner tile in the wave / no registers to hold it: k_pg_rope follows
  const int tiles = rows_total / (16 * sh.R);
  const bool ok = q ? pg_launch_cfg<true, EPI>(sh, tiles, nm * sh.ks * 64, m->stream, a, rg)
                    : pg_launch_cfg<false, EPI>(sh, tiles, nm * sh.ks * 64, m->stream, a, rg);
  if (!ok) m->pg_launch_failed = true;  // reported by kh_model_prefill_gemm
  if (EPI == KH_PG_RESID) return sh.kz > 1 ? sh.kz : 0;
  return EPI == KH_PG_QKV && a.rope != KH_PG_ROPE_OFF;
}
// k_rg_attn (kh_seq_prefill.h) in k_pg_attn's launch geometry at one query tile per workgroup, with k_pg_attn's waves
// per head size; pg_attn_supported(head_size) is the caller's to check
void launch_rg_attn(const KhPgAttnArgs& a, const KhRgTiles& tiles, int head_size, hipStream_t s) {
  const int grid = a.kv_heads * a.kv_mul * (a.T / 16);
  switch (head_size) {
    case 48: kh_launch(KH_KERNEL(k_rg_attn, 3, 8), grid, 64 * 8, 0, s, a, tiles); break;
    case 64: kh_launch(KH_KERNEL(k_rg_attn, 4, 8), grid, 64 * 8, 0, s, a, tiles); break;
    case 128: kh_launch(KH_KERNEL(k_rg_attn, 8, 4), grid, 64 * 4, 0, s, a, tiles); break;
    default: break;
  }
}
// forward of T (<= KH_PG_TMAX) prompt tokens at positions pos0..: fills their K/V cache rows.
// rg (kh_seq_prefill.h): the T = 16 x tiles slab tokens are the tiles of a pass into sequence slots instead - toks is
// the padded token list, pos0 is not read; the QKV GEMM, the RoPE fallback and the attention take the tile table
// (k_rg_gemm, k_rg_rope, k_rg_attn: MFMA attention only, the caller checked), every other launch is the run's own
void launch_prefill_gemm_chunk(kh_model* m, const int32_t* toks, int T, int pos0, const KhRgTiles* rg = nullptr) {
  const kh_config& c = m->cfg;
  const bool q = c.is_quant;
  const int tcap = pg_tcap(T);  // token stride of this chunk's tiled slabs
  (void)kh_embedding_f32_host(toks, T, m->tok_emb, m->pg_x, c.dim, c.vocab_size, (void*)m->stream);
  int pending_kz = 0;  // K slices of the last residual GEMM still to be added to pg_x (by the next RMSNorm)
  auto rmsnorm = [&](const float* w) {
    kh_pick_bool(q, [&](auto Q) {
      kh_launch(KH_KERNEL(k_pg_rmsnorm, Q), T, KH_WG, 0, m->stream, m->pg_x, w, m->pg_xn, c.dim, c.rms_eps, tcap,
                (const float*)m->pg_part, pending_kz);
    });
    pending_kz = 0;
  };
  // attention of the slice: MFMA kernel (kh_pattn.h) unless KH_PG_ATTN=0 or an odd head size
  const bool mfma_attn = pg_mfma_attn(m);
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
      a.rows0 = c.dim; a.rows1 = c.kv_dim; a.ldo = c.dim; a.K = c.dim; a.T = T; a.pos0 = pos0;
      a.gshift = m->gshift;
      // RoPE in the epilogue: interleaved pairs sit in one lane's float4; half-mode partners need the
      // paired-tile mapping (R = 2, head size a multiple of 32).  KH_PG_ROPE_FUSE=0: separate kernel.
      a.head_size = c.head_size; a.sin_cache = m->sin_cache; a.cos_cache = m->cos_cache;
      a.rope = !rope_fuse_env ? KH_PG_ROPE_OFF
               : (c.rope_mode == KH_ROPE_HALF ? (c.head_size % 32 == 0 ? KH_PG_ROPE_TILES : KH_PG_ROPE_OFF)
                                              : KH_PG_ROPE_PAIRS);
      rope_fused = pg_launch<KH_PG_QKV>(m, c.dim + 2 * c.kv_dim, c.dim % 32 == 0 && c.kv_dim % 32 == 0, a, rg) != 0;
    }
    if (!rope_fused && rg) {
      launch_log("k_rg_rope");
      hipLaunchKernelGGL(k_rg_rope, dim3(T), dim3(KH_WG), 0, m->stream, m->pg_q, kc, m->sin_cache,
                         m->cos_cache, c.dim, c.kv_dim, c.head_size, *rg, c.rope_mode);
    } else if (!rope_fused) {
      launch_log("k_pg_rope");
      hipLaunchKernelGGL(k_pg_rope, dim3(T), dim3(KH_WG), 0, m->stream, m->pg_q, kc, m->sin_cache,
                         m->cos_cache, c.dim, c.kv_dim, c.head_size, pos0, c.rope_mode);
    }
    // the prompt phase leaves K/V rows and nothing else (no logits): the last layer's K/V rows are
    // written, its attention, wo and FFN feed nothing (1/L of the pass minus one QKV GEMM)
    if (l == c.layer_num - 1) break;
    if (mfma_attn) {
      KhPgAttnArgs a{};
      a.q = m->pg_q; a.kc = kc; a.vc = vc; a.out = m->pg_att;
      a.dim = c.dim; a.kv_dim = c.kv_dim; a.kv_heads = c.kv_head_num; a.kv_mul = c.kv_mul;
      a.T = T; a.pos0 = pos0; a.layout = q ? KH_PA_TILED_Q8 : KH_PA_TILED_F32; a.tcap = tcap;
      if (rg)
        launch_rg_attn(a, *rg, c.head_size, m->stream);
      else
        launch_pg_attn(a, c.head_size, m->stream);
    } else {
      KhAttnArgs a = fill_attn(m, l, /*variant=*/0, m->attn_fenced);
      a.defer = 0;  // multi-token slices merge in the launch
      a.nsplit_g = m->attn_ns_g;  // not the decode step's variant: the launch plan decides from the slice's positions
      a.q = m->pg_q;
      a.out = m->pg_att;
      a.d_pos = nullptr;
      a.ws = m->pg_ws;
      a.tok_stride = c.dim;
      a.ws_tok_bytes = m->pg_ws_tok_bytes;
      // head sizes without an MFMA instantiation (and KH_PG_ATTN=0): the decode kernel, one grid
      // slice per token, 256-thread workgroups (4096 latency-bound (head, token) workgroups: twice
      // as many fit a CU as with the decode width, 28.7 -> 19.6 us per layer)
      launch_attn_decode(a, pos0, KH_WG, m->stream, T, pos0 + T - 1);
    }
    {
      KhPgGemmArgs a{};
      a.w[0] = W.wo;
      a.B = m->pg_att; a.b_tiled = mfma_attn ? 1 : 0; a.tcap = tcap; a.out = m->pg_x;  // decode kernel: row-major rows
      a.rows0 = c.dim; a.ldo = c.dim; a.K = c.dim; a.T = T; a.gshift = m->gshift; a.part = m->pg_part;
      pending_kz = pg_launch<KH_PG_RESID>(m, c.dim, c.dim % 32 == 0, a);
    }
    rmsnorm(W.ffn_norm);
    {
      KhPgGemmArgs a{};
      a.w[0] = W.w1; a.w[1] = W.w3;
      a.B = m->pg_xn; a.b_tiled = 1; a.tcap = tcap; a.out = m->pg_h;
      a.rows0 = c.hidden_dim; a.ldo = c.hidden_dim; a.K = c.dim; a.T = T; a.gshift = m->gshift;
      pg_launch<KH_PG_SWIGLU>(m, c.hidden_dim, c.hidden_dim % 32 == 0, a);
    }
    {
      KhPgGemmArgs a{};
      a.w[0] = W.w2;
      a.B = m->pg_h; a.b_tiled = 1; a.tcap = tcap; a.out = m->pg_x;
      a.rows0 = c.dim; a.ldo = c.dim; a.K = c.hidden_dim; a.T = T; a.gshift = m->gshift; a.part = m->pg_part;
      pending_kz = pg_launch<KH_PG_RESID>(m, c.dim, c.dim % 32 == 0, a);  // (the next layer's RMSNorm adds them)
    }
  }
}
}  // namespace

// Host-only view of the prefill GEMM launch plan (pg_shape) for tools and the CPU test-suite: epi 0 = QKV
// (rows = dim + 2 kv_dim), 1 = residual GEMM (wo / w2: rows = dim), 2 = SwiGLU pair (rows = hidden_dim); K =
// contraction length; r2_ok = the 32-row register tile divides the row blocks.  out[7] = {R, NT, ks, token
// slices, solo, kz, workgroups}.  No device is touched; the KH_PG_SHAPE_* overrides are not applied.
extern "C" int kh_plan_prefill_shape(int32_t epi, int32_t T, int32_t rows, int32_t K, int32_t is_quant,
                                     int32_t r2_ok, int32_t* out7) {
  if (!out7 || epi < 0 || epi > 2 || T <= 0 || T > KH_PG_TMAX || rows <= 0 || K <= 0) return KH_ERR_INVALID_ARG;
  const bool q = is_quant != 0;
  if (rows % 16 || K % (q ? 64 : 16)) return KH_ERR_UNSUPPORTED;
  const PgShape sh = pg_shape(T, rows, r2_ok != 0, epi == KH_PG_SWIGLU ? 2 : 1, K / (q ? 64 : 16), q ? 4 : 16, q,
                              epi == KH_PG_RESID);
  out7[0] = sh.R; out7[1] = sh.NT; out7[2] = sh.ks; out7[3] = sh.slices; out7[4] = sh.solo ? 1 : 0; out7[5] = sh.kz;
  out7[6] = rows / (16 * sh.R) * sh.slices * sh.kz;
  return KH_OK;
}

extern "C" int kh_model_prefill_gemm(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  int rc = khm::prefill_gemm_run(m, h_tokens, n, pos0);
  if (rc == KH_OK) rc = khm::lp_none(m, pos0, n);
  return rc == KH_OK ? khm::hist_write(m, h_tokens, n, pos0) : rc;
}
int khm::prefill_gemm_run(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  if (!m || !h_tokens || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if ((int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  if (!pg_supported(m)) return KH_ERR_UNSUPPORTED;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if ((rc = kv_ensure(m, pos0 + n)) != KH_OK) return rc;
  if ((rc = ensure_pg_buffers(m)) != KH_OK) return rc;
  if ((rc = ensure_pg_ws(m)) != KH_OK) return rc;
  m->pg_launch_failed = false;
  // tuning / test hook: KH_PG_CHUNK=<tokens per weight pass> (16 .. KH_PG_TMAX), read per call
  int chunk = KH_PG_TMAX;
  if (const char* e = dbg("KH_PG_CHUNK")) {
    const int v = atoi(e);
    chunk = v < 16 ? 16 : (v > KH_PG_TMAX ? KH_PG_TMAX : v);
  }
  for (int t0 = 0; t0 < n; t0 += chunk)
    launch_prefill_gemm_chunk(m, h_tokens + t0, n - t0 < chunk ? n - t0 : chunk, pos0 + t0);
  if (m->pg_launch_failed) return KH_ERR_UNSUPPORTED;  // a GEMM shape's LDS opt-in was refused
  return kh_launch_status();
}

// ---- the GEMM prefill into sequence slots (kh_seq_prefill.h; kh_model_seq.hip checks the call and drives this) -------
int khm::seq_prefill_gemm_check(const kh_model* m) {
  // no fallback to the VALU pass, none to the decode-attention slices (KH_PG_ATTN=0 refuses the call)
  return pg_supported(m) && pg_mfma_attn(m) ? KH_OK : KH_ERR_UNSUPPORTED;
}
int khm::seq_prefill_gemm_enqueue(kh_model* m, int n_seq, const int32_t* slots, const int32_t* toks,
                                  const int32_t* n_tokens, const int32_t* pos0) {
  int rc;
  if ((rc = ensure_pg_buffers(m)) != KH_OK) return rc;
  m->pg_launch_failed = false;
  std::vector<size_t> seg_at((size_t)n_seq);  // where segment s starts in toks
  size_t at = 0;
  for (int s = 0; s < n_seq; ++s) {
    seg_at[s] = at;
    at += (size_t)n_tokens[s];
  }
  KhRgTiles tiles;
  int32_t slab_tok[KH_PG_TMAX];
  int ntiles = 0, cur_pass = 0;
  auto flush = [&]() {
    if (ntiles == 0) return;
    for (int k = ntiles; k < KH_RG_TILES; ++k) {  // entries no slab token reads: the last tile's, as the lane tables pad
      tiles.pos0[k] = tiles.pos0[ntiles - 1];
      tiles.nvalid[k] = tiles.nvalid[ntiles - 1];
      tiles.base[k] = tiles.base[ntiles - 1];
      tiles.pfx_len[k] = tiles.pfx_len[ntiles - 1];
      tiles.pfx_row0[k] = tiles.pfx_row0[ntiles - 1];
    }
    launch_prefill_gemm_chunk(m, slab_tok, 16 * ntiles, 0, &tiles);
    ntiles = 0;
  };
  kh_rg_plan(n_seq, n_tokens, [&](int pass, int s, int off, int n) {
    if (pass != cur_pass) {
      flush();
      cur_pass = pass;
    }
    const KhSeqSlot& t = m->seq_tab[slots[s]];
    for (int o = 0; o < n; o += 16) {
      const int k = ntiles++, nv = n - o < 16 ? n - o : 16;
      tiles.pos0[k] = pos0[s] + off + o;
      tiles.nvalid[k] = nv;
      tiles.base[k] = kh_seq_own_base(t);
      tiles.pfx_len[k] = t.pfx;
      tiles.pfx_row0[k] = t.pfx > 0 ? m->seq_tab[t.parent].row0 : 0;
      // the padding tokens of a segment's last tile repeat its last valid token
      for (int i = 0; i < 16; ++i) slab_tok[16 * k + i] = toks[seg_at[s] + (size_t)(off + o + (i < nv ? i : nv - 1))];
    }
  });
  flush();
  if (m->pg_launch_failed) return KH_ERR_UNSUPPORTED;  // a GEMM shape's LDS opt-in was refused
  return kh_launch_status();
}

// Operator-level entry of the MFMA slice attention (kh_pattn.h): the multi-token form of MHAKernel.
extern "C" int kh_mha_prefill_f32(int32_t pos0, int32_t n_tokens, int32_t head_num, int32_t layer_index,
                                  int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                                  float* mha_out, const float* q, const float* key_cache,
                                  const float* value_cache, void* stream) {
  if (!mha_out || !q || !key_cache || !value_cache) return KH_ERR_INVALID_ARG;
  if (n_tokens <= 0 || pos0 < 0 || head_num <= 0 || layer_index < 0 || seq_len <= 0 || kv_mul <= 0 ||
      head_size <= 0 || kv_dim <= 0)
    return KH_ERR_INVALID_ARG;
  if (head_num % kv_mul || kv_dim != (head_num / kv_mul) * head_size) return KH_ERR_INVALID_ARG;
  if ((int64_t)pos0 + n_tokens > seq_len) return KH_ERR_RANGE;
  if (!pg_attn_supported(head_size)) return KH_ERR_UNSUPPORTED;
  if (((uintptr_t)mha_out | (uintptr_t)q | (uintptr_t)key_cache | (uintptr_t)value_cache) & 15)
    return KH_ERR_INVALID_ARG;  // 16-byte loads / stores
  KhPgAttnArgs a{};
  const size_t layer_off = (size_t)layer_index * seq_len * kv_dim;
  a.q = q; a.kc = key_cache + layer_off; a.vc = value_cache + layer_off; a.out = mha_out;
  a.dim = head_num * head_size; a.kv_dim = kv_dim; a.kv_heads = head_num / kv_mul; a.kv_mul = kv_mul;
  a.T = n_tokens; a.pos0 = pos0; a.layout = KH_PA_ROWS;
  launch_pg_attn(a, head_size, (hipStream_t)stream);
  return kh_launch_status();
}

extern "C" int kh_model_prefill(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  int rc = khm::prefill_run(m, h_tokens, n, pos0);
  if (rc == KH_OK) rc = khm::lp_none(m, pos0, n);
  return rc == KH_OK ? khm::hist_write(m, h_tokens, n, pos0) : rc;
}
int khm::prefill_run(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  if (!m || !h_tokens || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if ((int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  if (!prefill_supported(m)) return KH_ERR_UNSUPPORTED;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if ((rc = kv_ensure(m, pos0 + n)) != KH_OK) return rc;
  if ((rc = ensure_prefill_buffers(m)) != KH_OK) return rc;
  const int B = prefill_batch(m);
  for (int t0 = 0; t0 < n; t0 += B)
    launch_pf_pass(m, pf_run(h_tokens + t0, n - t0 < B ? n - t0 : B, pos0 + t0, B, /*full_depth=*/false));
  return kh_launch_status();
}

// Sequence scoring: kh_model_prefill's pass at full depth, k_pf_cls and k_score_lp per chunk of B tokens.  Eager
// launches on the model stream; every check before the first of them.
extern "C" int kh_model_score(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  if (!m || !h_tokens || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if ((int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  if (m->lp_top_n < 0 || !full_depth_supported(m)) return KH_ERR_UNSUPPORTED;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if ((rc = kv_ensure(m, pos0 + n)) != KH_OK) return rc;
  if ((rc = ensure_prefill_buffers(m)) != KH_OK) return rc;
  if ((rc = ensure_score_buffers(m)) != KH_OK) return rc;
  const int B = prefill_batch(m);
  for (int t0 = 0; t0 < n; t0 += B) {
    const int nv = n - t0 < B ? n - t0 : B;
    int32_t target[KH_PF_BMAX];
    kh_score_targets(h_tokens, n, t0, nv, target);
    launch_pf_pass(m, pf_run(h_tokens + t0, nv, pos0 + t0, B, /*full_depth=*/true));
    launch_score_tail(m, target, nv, pos0 + t0, B);
  }
  if ((rc = kh_launch_status()) != KH_OK) return rc;
  return khm::hist_write(m, h_tokens, n, pos0);
}

// ---- speculative greedy decode: the verify pass (kh_spec.h) ---------------------------------------------------------
int khm::verify_width(const kh_model* m) { return prefill_batch(m); }
int khm::verify_prepare(kh_model* m, int rows, bool as_set) {
  int rc;
  if ((rc = kv_ensure(m, rows)) != KH_OK) return rc;
  if ((rc = ensure_prefill_buffers(m)) != KH_OK) return rc;
  if ((rc = ensure_score_buffers(m)) != KH_OK) return rc;
  if (as_set && m->proc_on && !m->d_spec_cnt) {
    const size_t n = (size_t)KH_PF_BMAX * (size_t)m->cfg.vocab_size;
    KhDev<int32_t> cnt;
    if ((rc = cnt.alloc(n)) != KH_OK) return rc;
    KH_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * n, m->stream));  // once: the core re-arms them
    m->d_spec_cnt = std::move(cnt);
  }
  if (m->d_spec) return KH_OK;
  KhDev<int32_t> spec;
  KhPin<int32_t> pin;
  if ((rc = spec.alloc((size_t)1 + KH_PF_BMAX)) != KH_OK || (rc = pin.alloc((size_t)1 + KH_PF_BMAX)) != KH_OK) return rc;
  m->d_spec = std::move(spec);
  m->h_spec_pin = std::move(pin);
  return KH_OK;
}
int khm::verify_enqueue(kh_model* m, const int32_t* toks, int n, int pos0, bool as_set) {
  const kh_config& c = m->cfg;
  const int B = prefill_batch(m);
  // the tail of the pass under the settings; with none of them on the greedy pair below is that tail
  const bool tail = as_set && (m->samp_on || m->proc_on || m->lp_top_n >= 0);
  KhSpecAcceptArgs t;
  t.hist = m->d_hist;
  t.hist_cap = m->hist_cap;
  for (int b = 0; b < KH_PF_BMAX; ++b) t.fed[b] = b < n ? toks[b] : -1;
  t.pos0 = pos0;
  t.n = n;
  if (tail && m->proc_on) {  // the record the rows' windows read, ahead of them on the stream
    launch_log("k_spec_hist");
    hipLaunchKernelGGL(k_spec_hist, dim3(1), dim3(KH_WAVE), 0, m->stream, t);
  }
  launch_pf_pass(m, pf_run(toks, n, pos0, B, /*full_depth=*/true));
  launch_pf_cls(m, n, B);
  const bool records = tail && m->lp_top_n >= 0;
  const KhTailRecs recs{m->d_lp_token, m->d_lp_lp, m->d_lp_top_ids, m->d_lp_top_lp};
  if (tail) {
    KhSpecTailArgs a;
    a.logits = m->pf_logits;
    a.vocab = c.vocab_size;
    a.vstride = m->pf_vstride;
    a.pos0 = pos0;
    a.params = m->d_samp;
    a.proc = m->proc_on ? (const KhProcParams*)m->d_proc : nullptr;
    a.bias_ids = m->d_bias_ids;
    a.bias = m->d_bias;
    a.hist = m->d_hist;
    a.cnt = m->d_spec_cnt;
    a.top_n = records ? (const int32_t*)m->d_lp_top_n : nullptr;
    a.recs = recs;
    a.res = m->d_spec;
    launch_log("k_spec_tail");
    hipLaunchKernelGGL(k_spec_tail, dim3(n), dim3(KH_SAMP_THREADS), 0, m->stream, a);
  } else {
    launch_log("k_spec_pick");
    hipLaunchKernelGGL(k_spec_pick, dim3(n), dim3(KH_SAMP_THREADS), 0, m->stream, (const float*)m->pf_logits,
                       c.vocab_size, (long long)m->pf_vstride, m->d_spec + 1);
  }
  t.res = m->d_spec;
  t.words = m->d_words;
  t.words_cap = m->seq_cap;
  t.d_next = m->d_next;
  t.d_token = m->d_token;
  t.d_pos = m->d_pos;
  t.tok_emb = m->tok_emb;
  t.x = m->x;
  t.dim = c.dim;
  t.vocab = c.vocab_size;
  if (tail) {
    launch_log("k_spec_accept_set");
    hipLaunchKernelGGL(k_spec_accept_set, dim3(1), dim3(KH_WG), 0, m->stream,
                       KhSpecAcceptSetArgs{t, records ? recs : KhTailRecs{nullptr, nullptr, nullptr, nullptr}, m->lp_cap});
  } else {
    launch_log("k_spec_accept");
    hipLaunchKernelGGL(k_spec_accept, dim3(1), dim3(KH_WG), 0, m->stream, t);
  }
  KH_CHECK_HIP(hipMemcpyAsync(m->h_spec_pin, m->d_spec, sizeof(int32_t) * (size_t)(1 + n), hipMemcpyDeviceToHost,
                              m->stream));
  return kh_launch_status();
}

// ---- sequence slots: what kh_model_seq.hip enqueues (kh_seq.h) -----------------------------------------------------
int khm::seq_prepare(kh_model* m) {
  int rc;
  if ((rc = ensure_prefill_buffers(m)) != KH_OK) return rc;
  if ((rc = ensure_score_buffers(m)) != KH_OK) return rc;
  if ((rc = ensure_chunk_events(m)) != KH_OK) return rc;  // the stop check's events
  if (m->d_seq_tok) return KH_OK;
  const size_t rows = (size_t)m->cfg.cache_len, slots = KH_SEQ_SLOTS_MAX;
  KhDev<int32_t> tok, words;
  KhDev<KhSampParams> samp;
  KhPin<int32_t> tok_pin, words_pin;
  KhPin<KhSampParams> samp_pin;
  if ((rc = tok.alloc(slots)) != KH_OK || (rc = samp.alloc(slots)) != KH_OK || (rc = words.alloc(rows)) != KH_OK ||
      (rc = tok_pin.alloc(slots)) != KH_OK || (rc = samp_pin.alloc(slots)) != KH_OK ||
      (rc = words_pin.alloc(rows)) != KH_OK)
    return rc;
  m->d_seq_tok = std::move(tok);
  m->d_seq_samp = std::move(samp);
  m->d_seq_words = std::move(words);
  m->h_seq_tok_pin = std::move(tok_pin);
  m->h_seq_samp_pin = std::move(samp_pin);
  m->h_seq_words_pin = std::move(words_pin);
  return KH_OK;
}
int khm::seq_prepare_ex(kh_model* m, bool records) {
  int rc;
  if (!m->d_seq_proc) {
    const size_t slots = KH_SEQ_SLOTS_MAX, nb = (size_t)KH_SEQ_SLOTS_MAX * KH_SEQ_BIAS_MAX;
    const size_t n = (size_t)KH_PF_BMAX * (size_t)m->cfg.vocab_size;
    KhDev<KhProcParams> proc;
    KhDev<int32_t> bias_ids, cnt;
    KhDev<float> bias;
    KhPin<KhProcParams> proc_pin;
    KhPin<int32_t> bias_ids_pin, hist_pin;
    KhPin<float> bias_pin;
    if ((rc = proc.alloc(slots)) != KH_OK || (rc = bias_ids.alloc(nb)) != KH_OK || (rc = bias.alloc(nb)) != KH_OK ||
        (rc = cnt.alloc(n)) != KH_OK || (rc = proc_pin.alloc(slots)) != KH_OK || (rc = bias_ids_pin.alloc(nb)) != KH_OK ||
        (rc = bias_pin.alloc(nb)) != KH_OK || (rc = hist_pin.alloc((size_t)m->cfg.cache_len)) != KH_OK)
      return rc;
    KH_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * n, m->stream));  // once: the core re-arms them
    m->d_seq_proc = std::move(proc);
    m->d_seq_bias_ids = std::move(bias_ids);
    m->d_seq_bias = std::move(bias);
    m->d_seq_cnt = std::move(cnt);
    m->h_seq_proc_pin = std::move(proc_pin);
    m->h_seq_bias_ids_pin = std::move(bias_ids_pin);
    m->h_seq_bias_pin = std::move(bias_pin);
    m->h_seq_hist_pin = std::move(hist_pin);
  }
  return records ? lp_ensure_records(m) : KH_OK;
}
int khm::seq_prefill_enqueue(kh_model* m, int row0, const int32_t* toks, int n, int pos0, int pfx_len, int pfx_row0) {
  const int B = prefill_batch(m);
  for (int t0 = 0; t0 < n; t0 += B)
    launch_pf_pass(m, pf_run(toks + t0, n - t0 < B ? n - t0 : B, pos0 + t0, B, /*full_depth=*/false, row0, pfx_len,
                             pfx_row0));
  return kh_launch_status();
}
int khm::seq_pass_enqueue(kh_model* m, KhSeqLanes lanes, int n, bool words, const KhSeqTail* tail) {
  const int B = prefill_batch(m);
  for (int b = n; b < KH_PF_BMAX; ++b) {  // padding lanes rotate by the last valid lane's row; nothing of them is kept
    lanes.pos[b] = lanes.pos[n - 1];
    lanes.row[b] = lanes.row[n - 1];
    lanes.slot[b] = lanes.slot[n - 1];
    lanes.pfx_len[b] = lanes.pfx_len[n - 1];
    lanes.pfx_row0[b] = lanes.pfx_row0[n - 1];
  }
  launch_pf_pass(m, pf_lanes(lanes, n, B));
  launch_pf_cls(m, n, B);
  return seq_tail_enqueue(m, m->pf_logits, lanes, n, words, tail);
}
// the attention of lanes [0, n) of layer l (entries >= n padded by the caller): q / out rows of c.dim floats per lane
void khm::seq_attn_enqueue(kh_model* m, int l, const float* q, float* out, const KhSeqLanes& lanes, int n) {
  KhAttnArgs a = fill_attn(m, l, /*variant=*/0, m->attn_fenced);
  a.defer = 0;  // multi-token slices merge in the launch
  a.nsplit_g = m->attn_ns_g;
  a.q = q;
  a.out = out;
  a.d_pos = nullptr;
  a.ws = m->pf_ws;
  a.tok_stride = m->cfg.dim;
  a.ws_tok_bytes = m->pf_ws_tok_bytes;
  if (seq_lanes_share(lanes, n))
    launch_seq_attn_pfx(a, lanes, n, m->attn_wg, m->stream, m->seq_pfx_pad8);
  else
    launch_seq_attn(a, lanes, n, m->attn_wg, m->stream);
}
// the tail of lanes [0, n) on their logits rows [n][pf_vstride]: k_seq_pick, or k_seq_tail with a tail description
int khm::seq_tail_enqueue(kh_model* m, float* logits, const KhSeqLanes& lanes, int n, bool words,
                          const KhSeqTail* tail) {
  const kh_config& c = m->cfg;
  if (tail) {
    KhSeqTailArgs t;
    t.logits = logits;
    t.vocab = c.vocab_size;
    t.vstride = m->pf_vstride;
    t.lanes = lanes;
    t.params = m->d_seq_samp;
    t.proc = tail->proc;
    t.bias_ids = tail->bias_ids;
    t.bias = tail->bias;
    t.hist = m->d_hist;
    for (int b = 0; b < KH_PF_BMAX; ++b) t.cap[b] = kh_seq_capacity(m->seq_tab[lanes.slot[b]]);
    t.cnt = tail->cnt;
    t.top_n = tail->top_n;
    t.rec_token = m->d_lp_token;
    t.rec_lp = m->d_lp_lp;
    t.rec_top_ids = m->d_lp_top_ids;
    t.rec_top_lp = m->d_lp_top_lp;
    t.tok = m->d_seq_tok;
    t.words = words ? m->d_seq_words : nullptr;
    launch_log("k_seq_tail");
    hipLaunchKernelGGL(k_seq_tail, dim3(n), dim3(KH_SAMP_THREADS), 0, m->stream, t);
    return kh_launch_status();
  }
  KhSeqPickArgs t;
  t.logits = logits;
  t.vocab = c.vocab_size;
  t.vstride = m->pf_vstride;
  t.lanes = lanes;
  t.params = m->d_seq_samp;
  t.tok = m->d_seq_tok;
  t.words = words ? m->d_seq_words : nullptr;
  launch_log("k_seq_pick");
  hipLaunchKernelGGL(k_seq_pick, dim3(n), dim3(KH_SAMP_THREADS), 0, m->stream, t);
  return kh_launch_status();
}

extern "C" int kh_model_verify_width(const kh_model* m, int32_t* width) {
  if (!m || !width) return KH_ERR_INVALID_ARG;
  if (!full_depth_supported(m)) return KH_ERR_UNSUPPORTED;
  *width = verify_width(m);
  return KH_OK;
}
// One verify pass.  Eager launches on the model stream; every check before the first of them.
static int verify_call(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0, int32_t* h_next,
                       int32_t* n_accept, bool as_set) {
  if (!m || !h_tokens || !h_next || !n_accept || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if (!full_depth_supported(m)) return KH_ERR_UNSUPPORTED;
  if (n > verify_width(m) || (int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if ((rc = verify_prepare(m, pos0 + n, as_set)) != KH_OK) return rc;
  rc = verify_enqueue(m, h_tokens, n, pos0, as_set);
  const hipError_t e = hipStreamSynchronize(m->stream);  // drained on every way out
  if (rc != KH_OK) return rc;
  if (e != hipSuccess) return (int)e;
  *n_accept = m->h_spec_pin[0];
  memcpy(h_next, m->h_spec_pin + 1, sizeof(int32_t) * (size_t)n);
  return KH_OK;
}
extern "C" int kh_model_verify(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0, int32_t* h_next,
                               int32_t* n_accept) {
  return verify_call(m, h_tokens, n, pos0, h_next, n_accept, /*as_set=*/false);
}
extern "C" int kh_model_verify_as_set(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0, int32_t* h_next,
                                      int32_t* n_accept) {
  return verify_call(m, h_tokens, n, pos0, h_next, n_accept, /*as_set=*/true);
}

// Time the prompt phase alone: n fed-only tokens at positions pos0.., HIP events on the model
// stream around exactly that work (no decode step, no set_state).  mode KH_PREFILL_TOKEN = the
// reference's one forward pass per prompt token (demo/main.cpp:20-22), replayed from the hipGraph;
// KH_PREFILL_GEMV = kh_model_prefill's B-token VALU kernels; KH_PREFILL_GEMM = the MFMA GEMM path.
extern "C" int kh_model_time_prefill(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0,
                                     int32_t mode, float* h_ms) {
  if (!m || !h_tokens || !h_ms || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if ((int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if ((rc = kv_ensure(m, pos0 + n + 1)) != KH_OK) return rc;
  if (mode == KH_PREFILL_TOKEN) {
    if ((rc = ensure_seq_cap(m, pos0 + n + 1)) != KH_OK) return rc;
    std::vector<int32_t> forced((size_t)m->seq_cap + 1, -1);
    for (int i = 0; i < n; ++i) forced[pos0 + i] = h_tokens[i];
    forced[pos0 + n] = h_tokens[n - 1];  // keeps the last timed step in the prompt phase
    KH_CHECK_HIP(hipMemcpyAsync(m->d_forced, forced.data(), forced.size() * sizeof(int32_t),
                                hipMemcpyHostToDevice, m->stream));
    KH_CHECK_HIP(hipStreamSynchronize(m->stream));
    const int n_forced = m->seq_cap + 1;
    const StepTail tail = step_tail(m, false);
    // capture (first use) outside the timed region
    hipGraphExec_t ge = nullptr;
    for (int s = 0; s < n;) {
      const int k = n - s >= KH_GRAPH_STEPS ? KH_GRAPH_STEPS : 1;
      if ((rc = step_graph(m, n_forced, step_variant(m, pos0 + s, pos0 + s + k - 1), k, tail, &ge)) != KH_OK) return rc;
      s += k;
    }
    set_state(m, h_tokens[0], pos0);
    KH_CHECK_HIP(hipEventRecord(m->ev0, m->stream));
    for (int s = 0; s < n;) {
      const int k = n - s >= KH_GRAPH_STEPS ? KH_GRAPH_STEPS : 1;
      if ((rc = enqueue_steps(m, pos0 + s, k, n_forced, tail, KH_EXEC_GRAPH)) != KH_OK) return rc;
      s += k;
    }
    KH_CHECK_HIP(hipEventRecord(m->ev1, m->stream));
  } else if (mode == KH_PREFILL_GEMV) {
    if (!prefill_supported(m)) return KH_ERR_UNSUPPORTED;
    if ((rc = ensure_prefill_buffers(m)) != KH_OK) return rc;
    KH_CHECK_HIP(hipEventRecord(m->ev0, m->stream));
    if ((rc = prefill_run(m, h_tokens, n, pos0)) != KH_OK) return rc;
    KH_CHECK_HIP(hipEventRecord(m->ev1, m->stream));
  } else if (mode == KH_PREFILL_GEMM) {
    if (!pg_supported(m)) return KH_ERR_UNSUPPORTED;
    if ((rc = ensure_pg_buffers(m)) != KH_OK) return rc;
    if ((rc = ensure_pg_ws(m)) != KH_OK) return rc;
    KH_CHECK_HIP(hipEventRecord(m->ev0, m->stream));
    if ((rc = prefill_gemm_run(m, h_tokens, n, pos0)) != KH_OK) return rc;
    KH_CHECK_HIP(hipEventRecord(m->ev1, m->stream));
  } else {
    return KH_ERR_INVALID_ARG;
  }
  KH_CHECK_HIP(hipEventSynchronize(m->ev1));
  KH_CHECK_HIP(hipEventElapsedTime(h_ms, m->ev0, m->ev1));
  if ((rc = kh_launch_status()) != KH_OK) return rc;
  return KH_OK;
}
