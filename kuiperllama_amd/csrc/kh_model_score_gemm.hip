// kh_model_score_gemm.hip — sequence scoring on the matrix cores (kh_score_gemm.h): the launch of k_pg_cls_lse and
// k_pg_lse_merge, the tail the GEMM pass of kh_model_gemm.hip ends in where it scores (score_gemm_tail), the public
// call kh_model_score_gemm and the operators kh_cls_logprobs_f32 / kh_cls_logprobs_w16_f32.  The classifier reads the
// fp32 or int8 image, or - KH_FLAG_GEMM16 with the cls class, and the bf16 operator - the bf16-format 16-bit copy
// through k_pg_cls_lse_w16 (kh_score_gemm_w16.h, compiled in kh_model_score_gemm_w16.hip).  The reference has no scoring
// call.  gfx950 only.
#include <vector>

#include "kh_dispatch.h"
#include "kh_gemm16_launch.h"
#include "kh_model_internal.h"
#include "kh_score_gemm.h"
#include "kh_score_plan.h"

using namespace khm;

namespace khm {
void launch_cls_lse_w16(hipStream_t stream, dim3 grid, int NT, const KhClsLseArgs& a);  // kh_model_score_gemm_w16.hip
}

namespace {
// the two launches on a tiled slab of T tokens.  No one-workgroup-per-CU request (pg_shape's `solo`): on a 128 256 x 2048
// fp32 classifier at 512 tokens it measured 2.72 / 2.98 ms with against 2.65 / 2.98 ms without (profiles/score_gemm_ab.txt)
// core: what a.w holds - PG_F32 / PG_Q8 the image's classifier, PG_W16 its bf16 copy (k_pg_cls_lse_w16: the same grid)
void launch_cls_lse(hipStream_t stream, PgCore core, KhClsLseArgs a, KhLseMergeArgs mg) {
  const int NT = cl_nt(a.T), nblk = cl_blocks(a.vocab);
  a.slices = cl_slices(a.T);
  const dim3 grid(nblk * a.slices);
  if (core == PG_W16)
    launch_cls_lse_w16(stream, grid, NT, a);
  else
    kh_pick_bool(core == PG_Q8, [&](auto Q) {
      kh_pick(KhVals<8, 4>{}, NT, [&](auto N) { kh_launch(KH_KERNEL(k_pg_cls_lse, Q, N), grid, KH_CL_WAVES * 64, 0, stream, a); });
    });
  mg.ws = a.ws;
  mg.ws_tokens = a.ws_tokens;
  mg.nblk = nblk;
  mg.vocab = a.vocab;
  mg.top_n = a.top_n;
  mg.target = a.target;
  launch_log("k_pg_lse_merge");
  hipLaunchKernelGGL(k_pg_lse_merge, dim3(a.T), dim3(KH_CL_MERGE_WG), 0, stream, mg);
}
}  // namespace

// the records of one record-less GEMM pass at full depth: pg_xn holds the final RMSNorm's rows of T tokens at positions
// pos0 ..; d_target[t] = the token that followed token t
void khm::score_gemm_tail(kh_model* m, int T, int pos0, const int32_t* d_target) {
  const kh_config& c = m->cfg;
  // the bf16 matrix cores where KH_FLAG_GEMM16 adopted the cls class on a live bf16-format copy; the fp16-format copy
  // and the int8 image on the bf16 matrix cores (PG_H16, PG_Q16) have no such kernel: the image's
  const bool w16 = pg_core_of(m, KH_W16_CLS) == PG_W16;
  KhClsLseArgs a{};
  a.w = w16 ? KhLin{m->w16.cls, nullptr, nullptr} : m->cls;
  a.B = m->pg_xn;
  a.vocab = c.vocab_size; a.K = c.dim; a.T = T; a.tcap = pg_tcap(T);
  a.target = d_target;
  a.top_n = m->lp_top_n < c.vocab_size ? m->lp_top_n : c.vocab_size;  // (<= KH_LOGPROBS_MAX_TOP: kh_model_set_logprobs)
  a.ws = m->cl_ws; a.ws_tokens = KH_PG_TMAX;
  KhLseMergeArgs mg{};
  mg.rec0 = pos0; mg.rec_cap = m->lp_cap; mg.top_stride = KH_LOGPROBS_MAX_TOP;
  mg.recs = lp_records(m);
  launch_cls_lse(m->stream, w16 ? PG_W16 : (c.is_quant ? PG_Q8 : PG_F32), a, mg);
}

// Sequence scoring on the GEMM pass: kh_model_prefill_gemm's passes at full depth, each ending in k_pg_cls_lse and
// k_pg_lse_merge.  Eager launches on the model stream; every check before the first of them.
extern "C" int kh_model_score_gemm(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0) {
  if (!m || !h_tokens || n <= 0 || pos0 < 0) return KH_ERR_INVALID_ARG;
  const kh_config& c = m->cfg;
  if ((int64_t)pos0 + n > c.cache_len) return KH_ERR_RANGE;
  if (!tokens_in_vocab(m, h_tokens, n)) return KH_ERR_RANGE;
  if (m->lp_top_n < 0 || m->fsm_on || !pg_supported(m) || c.vocab_size % 16) return KH_ERR_UNSUPPORTED;
  KH_CHECK_HIP(hipSetDevice(m->opts.device));
  int rc;
  if (!m->cl_ws) {  // the first call: the partial records of one pass, the targets of one call
    KhDev<float> ws;
    KhDev<int32_t> tg;
    if ((rc = ws.alloc((size_t)cl_blocks(c.vocab_size) * KH_PG_TMAX * KH_CL_STRIDE)) != KH_OK ||
        (rc = tg.alloc((size_t)c.cache_len)) != KH_OK)
      return rc;
    m->cl_ws = std::move(ws);
    m->cl_target = std::move(tg);
  }
  std::vector<int32_t> target((size_t)n);
  kh_score_targets(h_tokens, n, 0, n, target.data());
  // pageable source: the sync keeps the array alive for the upload (hist_write)
  KH_CHECK_HIP(hipMemcpyAsync(m->cl_target, target.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, m->stream));
  KH_CHECK_HIP(hipStreamSynchronize(m->stream));
  if ((rc = prefill_gemm_run(m, h_tokens, n, pos0, m->cl_target)) != KH_OK) return rc;
  return hist_write(m, h_tokens, n, pos0);
}

// ---- operators: the two kernels on caller buffers, fp32 or bf16 weights ---------------------------------------------
extern "C" int64_t kh_cls_logprobs_workspace_bytes(int32_t T, int32_t vocab, int32_t dim) {
  if (T <= 0 || T > KH_PG_TMAX || vocab <= 0 || dim <= 0) return 0;
  return (int64_t)sizeof(float) * ((int64_t)dim * pg_tcap(T) + (int64_t)cl_blocks(vocab) * T * KH_CL_STRIDE);
}
// core: PG_F32 - W fp32 [vocab][dim], dim % 16 == 0; PG_W16 - W bf16 bits [vocab][dim], dim % 32 == 0
static int cls_logprobs_op(PgCore core, const void* W, const float* X, int32_t T, int32_t vocab, int32_t dim,
                           const int32_t* d_targets, int32_t top_n, float* d_lse, float* d_lp, int32_t* d_top_ids,
                           float* d_top_lp, float* d_max, float* d_target_logit, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  if (!W || !X || !workspace || T <= 0 || vocab <= 0 || dim <= 0 || top_n < 0 || top_n > KH_LOGPROBS_MAX_TOP ||
      top_n > vocab)
    return KH_ERR_INVALID_ARG;
  if (T > KH_PG_TMAX) return KH_ERR_RANGE;
  if (vocab % 16 || dim % (core == PG_W16 ? 32 : 16)) return KH_ERR_UNSUPPORTED;
  if (!kh_aligned16(W) || !kh_aligned16(X) || !kh_aligned16(workspace) ||
      workspace_bytes < kh_cls_logprobs_workspace_bytes(T, vocab, dim))
    return KH_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int tcap = pg_tcap(T);
  float* slab = (float*)workspace;
  launch_log("k_cls_pack");
  hipLaunchKernelGGL(k_cls_pack, dim3(tcap), dim3(KH_WG), 0, s, X, slab, (int)T, (int)dim, tcap);
  KhClsLseArgs a{};
  a.w = KhLin{W, nullptr, nullptr};
  a.B = slab;
  a.vocab = vocab; a.K = dim; a.T = T; a.tcap = tcap;
  a.target = d_targets;
  a.top_n = top_n;
  a.ws = slab + (size_t)dim * tcap; a.ws_tokens = T;
  KhLseMergeArgs mg{};
  mg.rec0 = 0; mg.rec_cap = T; mg.top_stride = top_n;
  mg.recs = KhTailRecs{nullptr, d_lp, d_top_ids, d_top_lp};
  mg.o_lse = d_lse; mg.o_max = d_max; mg.o_tlogit = d_target_logit;
  launch_cls_lse(s, core, a, mg);
  return kh_launch_status();
}
extern "C" int kh_cls_logprobs_f32(const float* W, const float* X, int32_t T, int32_t vocab, int32_t dim,
                                   const int32_t* d_targets, int32_t top_n, float* d_lse, float* d_lp, int32_t* d_top_ids,
                                   float* d_top_lp, float* d_max, float* d_target_logit, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  return cls_logprobs_op(PG_F32, W, X, T, vocab, dim, d_targets, top_n, d_lse, d_lp, d_top_ids, d_top_lp, d_max,
                         d_target_logit, workspace, workspace_bytes, stream);
}
// the same on the bf16 matrix cores (k_pg_cls_lse_w16): W16 holds the bf16 bits of finite weights
extern "C" int kh_cls_logprobs_w16_f32(const uint16_t* W16, const float* X, int32_t T, int32_t vocab, int32_t dim,
                                       const int32_t* d_targets, int32_t top_n, float* d_lse, float* d_lp,
                                       int32_t* d_top_ids, float* d_top_lp, float* d_max, float* d_target_logit,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  return cls_logprobs_op(PG_W16, W16, X, T, vocab, dim, d_targets, top_n, d_lse, d_lp, d_top_ids, d_top_lp, d_max,
                         d_target_logit, workspace, workspace_bytes, stream);
}
