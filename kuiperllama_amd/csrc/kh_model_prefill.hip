// kh_model_prefill.hip — prompt phase of the model level: the B-token VALU pass (kh_prefill.h, bit-identical to
// token-by-token; ONE layer driver, launch_pf_pass) and what runs on it - the prompt prefill, sequence scoring
// (kh_model_score: k_pf_cls, k_score_lp), the verify pass of speculative decode (kh_model_verify[_as_set]: k_pf_cls,
// kh_spec.h) and the pass over lanes of different sequences (kh_seq.h; kh_model_seq.hip drives it); for a W16 or a Q4
// model the launch classes of its pass mask run on the 16-bit / 4-bit copy (kh_w16_pass.h, kh_q4_pass.h; the
// pf_*_on launchers below).  What runs on the GEMM slabs lives in kh_model_gemm.hip.  The reference feeds the prompt
// one token per forward pass (demo/main.cpp:20-22).
// gfx950 only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kh_dispatch.h"
#include "kh_logprobs.h"
#include "kh_model_internal.h"
#include "kh_pf_launch.h"
#include "kh_prefill.h"
#include "kh_score_plan.h"
#include "kh_seq.h"
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
// fill_attn's decode arguments as those of a multi-token slice: q / out rows of dim floats per token, one split
// workspace of ws_tok_bytes per token
KhAttnArgs attn_slice_args(kh_model* m, int l, const float* q, float* out, void* ws, size_t ws_tok_bytes) {
  KhAttnArgs a = fill_attn(m, l, /*variant=*/0, m->attn_fenced);
  a.defer = 0;  // multi-token slices merge in the launch
  a.nsplit_g = m->attn_ns_g;  // not the decode step's variant: the launch plan decides from the slices' positions
  a.q = q;
  a.out = out;
  a.d_pos = nullptr;
  a.ws = ws;
  a.tok_stride = m->cfg.dim;
  a.ws_tok_bytes = ws_tok_bytes;
  return a;
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
// ---- the twins on a copy (kh_pf_launch.h; on: KH_ON_W16 or KH_ON_Q4, `img`: the image's arguments): this translation
// unit compiles the _w16 kernels; an fp16-format copy goes to kh_model_h16_pass.hip and the 4-bit copy to
// kh_model_q4_pass.hip, which compile the _h16 and the _q4 kernels from the same launch text
inline bool f16_copy(const kh_model* m) { return m->w16.format == KH_W16_F16; }
void pf_qkv_on(kh_model* m, KhOn on, int l, const KhPfQkvArgs& img, const KhSeqLanes* lanes, int B) {
  if (on == KH_ON_Q4) return q4_pf_qkv(m, l, img, lanes, B);
  f16_copy(m) ? h16_pf_qkv(m, l, img, lanes, B) : copy_pf_qkv<KH_SRC_BF16>(m, l, img, lanes, B);
}
void pf_ffn13_on(kh_model* m, KhOn on, int l, const KhPfFfn13Args& img, int B) {
  if (on == KH_ON_Q4) return q4_pf_ffn13(m, l, img, B);
  f16_copy(m) ? h16_pf_ffn13(m, l, img, B) : copy_pf_ffn13<KH_SRC_BF16>(m, l, img, B);
}
void pf_gemv_res_on(kh_model* m, KhOn on, int l, int cls, const kh_model::Shape& sh, const KhPfGemvResArgs& img,
                    int bs) {
  if (on == KH_ON_Q4) return q4_pf_gemv_res(m, l, cls, sh, img, bs);
  f16_copy(m) ? h16_pf_gemv_res(m, l, cls, sh, img, bs) : copy_pf_gemv_res<KH_SRC_BF16>(m, l, cls, sh, img, bs);
}
void pf_cls_on(kh_model* m, KhOn on, const KhPfClsArgs& img, int B) {
  if (on == KH_ON_Q4) return q4_pf_cls(m, img, B);
  f16_copy(m) ? h16_pf_cls(m, img, B) : copy_pf_cls<KH_SRC_BF16>(m, img, B);
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
  const KhOn on = pass_runs_on(m, cls);  // the image, the 16-bit copy or the 4-bit copy
  for (int t0 = 0; t0 < nvalid; t0 += bs) {
    a.V = V + (size_t)t0 * M;
    a.X = X + (size_t)t0 * K;
    a.nvalid = nvalid - t0 < bs ? nvalid - t0 : bs;
    if (on != KH_ON_IMAGE) {  // the same shape on the copy
      pf_gemv_res_on(m, on, l, cls, sh, a, bs);
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
    if (const KhOn on = pass_runs_on(m, KH_W16_QKV); on != KH_ON_IMAGE) {  // the same shape on the copy
      pf_qkv_on(m, on, l, pf_qkv_args(m, l, p), p.lanes, B);
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
    if (p.lanes) {
      seq_attn_enqueue(m, l, m->pf_q, m->pf_att, *p.lanes, nvalid);
    } else {
      KhAttnArgs a = attn_slice_args(m, l, m->pf_q, m->pf_att, m->pf_ws, m->pf_ws_tok_bytes);
      if (p.pfx_len > 0) {
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
      if (const KhOn on = pass_runs_on(m, KH_W16_FFN13); on != KH_ON_IMAGE)
        pf_ffn13_on(m, on, l, a, B);
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
  if (const KhOn on = pass_runs_on(m, KH_W16_CLS); on != KH_ON_IMAGE) return pf_cls_on(m, on, a, B);
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
  t.recs = lp_records(m);
  t.rec_cap = m->lp_cap;
  launch_log("k_score_lp");
  hipLaunchKernelGGL(k_score_lp, dim3(nvalid), dim3(KH_SAMP_THREADS), 0, m->stream, t);
}
}  // namespace

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
int khm::verify_prepare(kh_model* m, int rows, bool as_set, bool fsm) {
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
  if (as_set && fsm && m->fsm_on && !m->d_spec_fsm) {
    KhDev<int32_t> words;
    if ((rc = words.alloc(KH_PF_BMAX)) != KH_OK) return rc;
    m->d_spec_fsm = std::move(words);
  }
  if (m->d_spec) return KH_OK;
  KhDev<int32_t> spec;
  KhPin<int32_t> pin;
  if ((rc = spec.alloc((size_t)1 + KH_PF_BMAX)) != KH_OK || (rc = pin.alloc((size_t)1 + KH_PF_BMAX)) != KH_OK) return rc;
  m->d_spec = std::move(spec);
  m->h_spec_pin = std::move(pin);
  return KH_OK;
}
int khm::verify_enqueue(kh_model* m, const int32_t* toks, int n, int pos0, bool as_set, bool fsm) {
  const kh_config& c = m->cfg;
  const int B = prefill_batch(m);
  // the constrained form: the tail's twins with the automaton, whatever else is set (the chain is the greedy pick then)
  fsm = fsm && as_set && m->fsm_on;
  // the tail of the pass under the settings; with none of them on the greedy pair below is that tail
  const bool tail = fsm || (as_set && (m->samp_on || m->proc_on || m->lp_top_n >= 0));
  KhSpecAcceptArgs t;
  t.hist = m->d_hist;
  t.hist_cap = m->hist_cap;
  for (int b = 0; b < KH_PF_BMAX; ++b) t.fed[b] = b < n ? toks[b] : -1;
  t.pos0 = pos0;
  t.n = n;
  if (fsm) {  // the state ahead of every row - and the record, k_spec_hist's duty
    launch_log("k_spec_fsm_rows");
    hipLaunchKernelGGL(k_spec_fsm_rows, dim3(1), dim3(KH_FSM_THREADS), 0, m->stream, t, (const KhFsmDev*)m->fsm.desc,
                       (const int32_t*)m->fsm.state, (int32_t*)m->d_spec_fsm);
  } else if (tail && m->proc_on) {  // the record the rows' windows read, ahead of them on the stream
    launch_log("k_spec_hist");
    hipLaunchKernelGGL(k_spec_hist, dim3(1), dim3(KH_WAVE), 0, m->stream, t);
  }
  launch_pf_pass(m, pf_run(toks, n, pos0, B, /*full_depth=*/true));
  launch_pf_cls(m, n, B);
  const bool records = tail && m->lp_top_n >= 0;
  const KhTailRecs recs = lp_records(m);
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
    if (fsm) {
      const KhSpecTailFsmArgs af{KhFsmRef{m->fsm.desc, m->d_spec_fsm}, a};
      launch_log("k_spec_tail_fsm");
      hipLaunchKernelGGL(k_spec_tail_fsm, dim3(n), dim3(KH_SAMP_THREADS), 0, m->stream, af);
    } else {
      launch_log("k_spec_tail");
      hipLaunchKernelGGL(k_spec_tail, dim3(n), dim3(KH_SAMP_THREADS), 0, m->stream, a);
    }
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
    const KhSpecAcceptSetArgs s{t, records ? recs : KhTailRecs{nullptr, nullptr, nullptr, nullptr}, m->lp_cap};
    if (fsm) {
      launch_log("k_spec_accept_fsm");
      hipLaunchKernelGGL(k_spec_accept_fsm, dim3(1), dim3(KH_WG), 0, m->stream,
                         KhSpecAcceptFsmArgs{s, (const int32_t*)m->d_spec_fsm, (int32_t*)m->fsm.state});
    } else {
      launch_log("k_spec_accept_set");
      hipLaunchKernelGGL(k_spec_accept_set, dim3(1), dim3(KH_WG), 0, m->stream, s);
    }
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
  const KhAttnArgs a = attn_slice_args(m, l, q, out, m->pf_ws, m->pf_ws_tok_bytes);
  if (seq_lanes_share(lanes, n))
    launch_seq_attn_pfx(a, lanes, n, m->attn_wg, m->stream, m->seq_pfx_pad8);
  else
    launch_seq_attn(a, lanes, n, m->attn_wg, m->stream);
}
// the tail of lanes [0, n) on their logits rows [n][pf_vstride]: k_seq_pick, or k_seq_tail with a tail description
// (k_seq_tail_fsm where the description names an automaton)
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
    t.recs = lp_records(m);
    t.tok = m->d_seq_tok;
    t.words = words ? m->d_seq_words : nullptr;
    if (tail->fsm.desc) {  // a lane's slot is constrained: the twin with the automaton, for all lanes of the pass
      const KhSeqTailFsmArgs tf{tail->fsm, t};
      launch_log("k_seq_tail_fsm");
      hipLaunchKernelGGL(k_seq_tail_fsm, dim3(n), dim3(KH_SAMP_THREADS), 0, m->stream, tf);
      return kh_launch_status();
    }
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
                       int32_t* n_accept, bool as_set, bool fsm = false) {
  if (!m || !h_tokens || !h_next || !n_accept || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  // (a constraint: kh_model_verify_fsm is the call for it - its rows take their states from k_spec_fsm_rows)
  if ((m->fsm_on && !fsm) || !full_depth_supported(m)) return KH_ERR_UNSUPPORTED;
  if (n > verify_width(m) || (int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if ((rc = verify_prepare(m, pos0 + n, as_set, fsm)) != KH_OK) return rc;
  rc = verify_enqueue(m, h_tokens, n, pos0, as_set, fsm);
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
extern "C" int kh_model_verify_fsm(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0, int32_t* h_next,
                                   int32_t* n_accept) {
  return verify_call(m, h_tokens, n, pos0, h_next, n_accept, /*as_set=*/true, /*fsm=*/true);
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
    if ((rc = prefill_gemm_prepare(m)) != KH_OK) return rc;
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
