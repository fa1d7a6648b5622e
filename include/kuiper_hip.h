/*
 * kuiper_hip.h — C-ABI of libkuiper_hip.so: the MI355X (gfx950) decode path that drops in
 * behind KuiperLLama's kernel-function-pointer interface
 *     kuiper/source/op/kernels/kernels_interface.h:6-68   (typedefs + get_*_kernel getters)
 * and, one level up, behind model::LLama2Model / model::Qwen2Model
 *     kuiper/include/model/model.h:20-56, kuiper/source/model/llama3.cpp:107-167,733-745.
 *
 * Conventions
 *   - every function returns int: 0 = success, >0 = a hipError_t, <0 = KH_ERR_* below.
 *     Nothing aborts (the reference CHECK/LOG(FATAL)s; a C-ABI must not).
 *   - all tensor pointers are DEVICE pointers unless a parameter is named h_* / host.
 *   - tensors are dense row-major fp32 (int8 for quantised weights), exactly the layouts of
 *     the reference (weights [K rows, M cols]; KV cache [layer, seq_len, kv_dim]).
 *   - `stream` is a hipStream_t passed as void* (the reference passes `void* stream` /
 *     CudaConfig::stream the same way, kuiper/include/base/cuda_config.h:6-13).
 *     Launches are asynchronous on that stream, never allocate, never synchronise, and are
 *     hipGraph-capturable — which is why positions/tokens can be given as DEVICE scalars
 *     (the reference reads `pos` on the host: cuda/rope_kernel.cu:157, op/mha.cpp:33).
 *   - callee never takes ownership of caller memory.
 */
#ifndef KUIPER_HIP_H
#define KUIPER_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_VERSION 100 /* 0.1.0 */

enum {
  KH_OK = 0,
  KH_ERR_INVALID_ARG = -1, /* null pointer, non-positive size, size mismatch */
  KH_ERR_UNSUPPORTED = -2, /* e.g. int8 + tied classifier (broken in the reference too) */
  KH_ERR_IO = -3,          /* file open/map failure (reference: error::PathNotValid) */
  KH_ERR_FORMAT = -4,      /* malformed .bin (reference: error::ModelParseError) */
  KH_ERR_NO_DEVICE = -5,
  KH_ERR_RANGE = -6,       /* token / position out of range */
  KH_ERR_INTERNAL = -7     /* a C++ exception inside the library (host allocation, thread creation): caught at the
                              boundary, everything the call had built is released; host out-of-memory is reported as
                              hipErrorOutOfMemory (2) */
};
const char* kh_error_string(int code);
int kh_version(void);
/* number of HIP devices visible; <0 on error */
int kh_device_count(void);

enum { KH_ROPE_INTERLEAVED = 0, KH_ROPE_HALF = 1 };
enum { KH_FAMILY_LLAMA = 0, KH_FAMILY_QWEN2 = 1 };

/* ============================ operator level ==========================================
 * One entry point per reference kernel typedef (kernels_interface.h). */

/* AddKernel (kernels_interface.h:6-7; cuda/add_kernel.cu:14-32): out = in1 + in2 */
int kh_add_f32(const float* in1, const float* in2, float* out, int32_t n, void* stream);

/* MatmulKernel (kernels_interface.h:9-10; cuda/matmul_kernel.cu:89-109,
 * cpu/matmul_kernel.cpp:5-41): y[K] = (W[K,M] . x[M]) * scale.
 * (The reference CUDA path ignores `scale`, the CPU path honours it; honoured here.) */
/* y[t][0 .. M) = w16[M][K] . x[t][0 .. K) for t < T on the bf16 matrix cores, fp32-accurate (csrc/kh_gemm_w16.h: the
 * K loop of KH_FLAG_GEMM16 under its STORE epilogue): w16 holds bf16 bits, row-major; every x splits exactly into
 * three bf16 terms, products are exact, accumulation is fp32.  y has row stride ldy >= M.  M % 16 == 0, K % 32 == 0 and
 * T <= 512, else KH_ERR_UNSUPPORTED; 16-byte aligned pointers, ldy % 4 == 0.  Allocates a staging copy of x and
 * synchronises the stream. */
int kh_gemm_w16_f32(const float* x, const uint16_t* w16, float* y, int32_t T, int32_t M, int32_t K, int32_t ldy,
                    void* stream);
int kh_matmul_f32(const float* x, const float* w, float* y, int32_t M, int32_t K, float scale,
                  void* stream);
/* y[t][0 .. M) = sum over groups g of scales[m][g] * (w8[m][64g .. 64g + 64) . x[t][64g .. 64g + 64)) for t < T, on the
 * bf16 matrix cores, fp32-accurate (csrc/kh_gemm_q16.h: the K loop of KH_FLAG_GEMM16_Q8 under its STORE epilogue): w8 is
 * int8, row-major [M][K], group size 64, scales[M][K / 64]; every int8 value is an exact bf16, every x splits exactly into
 * three bf16 terms, products are exact, accumulation is fp32 and the group scale multiplies the group's partial sum.  y
 * has row stride ldy >= M.  M % 16 == 0, K % 64 == 0 and T <= 512, else KH_ERR_UNSUPPORTED; 16-byte aligned pointers,
 * ldy % 4 == 0.  Allocates a staging copy of x and synchronises the stream. */
int kh_gemm_q8_bf16_f32(const float* x, const int8_t* w8, const float* scales, float* y, int32_t T, int32_t M, int32_t K,
                        int32_t ldy, void* stream);

/* MatmulKernelQuant (kernels_interface.h:12-14; cuda/matmul_kernel.cu:56-87,111-134):
 * y[p] = sum_i x[i] * scales[(p*M+i)/group_size] * float(w8[p*M+i]) */
int kh_matmul_q8(const float* x, const int8_t* w8, const float* scales, int32_t group_size,
                 float* y, int32_t M, int32_t K, void* stream);

/* EmbeddingKernel (kernels_interface.h:16-17; cuda/emb_kernel.cu:3-48):
 * out[t,:] = W[tokens[t],:].  tokens is a DEVICE int32 array (for callers that already hold the
 * ids on the device; the reference hands over a HOST tensor and uploads it per call,
 * emb_kernel.cu:25-29 - that form is kh_embedding_f32_host below, which the adapter uses).  Rows
 * whose token is outside [0, vocab) are left untouched. */
int kh_embedding_f32(const int32_t* tokens, int32_t n_tokens, const float* w, float* out,
                     int32_t dim, int32_t vocab, void* stream);

/* The same with the token ids in HOST memory, which is what the reference's EmbeddingKernel
 * receives (the input tensor is a CPU tensor, op/embedding.cpp; emb_kernel.cu:25-29 uploads it per
 * call).  The ids travel in the kernel arguments, 64 per launch: no staging buffer, no copy. */
int kh_embedding_f32_host(const int32_t* h_tokens, int32_t n_tokens, const float* w, float* out,
                          int32_t dim, int32_t vocab, void* stream);

/* SwigluKernel (kernels_interface.h:19-20; cuda/swiglu_kernel.cu:4-47):
 * out = a*sigmoid(a) * b ; out may alias a (llama3.cpp:708). */
int kh_swiglu_f32(const float* a, const float* b, float* out, int32_t n, void* stream);

/* RMSNormKernel (kernels_interface.h:30-31; cuda/rmsnorm_kernel.cu:5-78,
 * cpu/rmsnorm_kernel.cpp:4-33): out = w * (x / sqrt(mean(x^2)+eps)); out may alias x.
 * eps is a compile-time #ifdef in the reference (1e-5 / 1e-6 QWEN2). */
int kh_rmsnorm_f32(const float* x, const float* w, float* out, int32_t n, float eps,
                   void* stream);

/* RoPEKernel (kernels_interface.h:33-36; cuda/rope_kernel.cu:5-36,51-82,104-122,153-170):
 * in-place rotation of q[dim] and k[kv_dim] with cached sin/cos row `pos`.
 * mode selects what the reference picks with LLAMA3_SUPPORT/QWEN2_SUPPORT (half) or
 * neither (interleaved).  Position = *d_pos if d_pos != NULL else pos. */
int kh_rope_f32(int32_t dim, int32_t kv_dim, int32_t head_size, float* q, float* k,
                const int32_t* d_pos, int32_t pos, const float* sin_cache,
                const float* cos_cache, int32_t mode, void* stream);

/* sin_cos_cache_calc_cu (cuda/rope_kernel.cuh:9-10; cpu/rope_kernel.cpp:4-16):
 * cache[pos*hs + d] = sin/cos(float(pos) * (1/pow(theta, d/hs))) for d < head_size. */
int kh_sincos_cache_f32(int32_t head_size, int32_t max_seq_len, float theta, float* sin_cache,
                        float* cos_cache, void* stream);

/* MHAKernel (kernels_interface.h:22-28; cuda/mha_kernel.cu:47-130, cpu/mha_kernel.cpp:5-61).
 * Decode attention for one query token over the contiguous KV cache; softmax probabilities
 * are left in score[head, 0..pos] like the reference.  Position = *d_pos or pos.
 * score may be NULL: probabilities are then not materialised and the launch uses the fused
 * decode path's low-latency kernel (per-lane-group online softmax, one memory round trip). */
int kh_mha_f32(const int32_t* d_pos, int32_t pos, int32_t head_num, int32_t layer_index,
               int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
               float* mha_out, const float* q, float* score, const float* kcache,
               const float* vcache, void* stream);

/* Multi-token form of MHAKernel for the prompt phase (no reference counterpart: demo/main.cpp:20-22
 * feeds the prompt one token per forward pass, so mha.cpp:19-38 only ever sees one query).  Causal
 * attention of n_tokens consecutive queries at positions pos0 .. pos0+n_tokens-1 against one layer's
 * contiguous cache, whose rows up to pos0+n_tokens-1 are already written; q and mha_out are
 * row-major [n_tokens][head_num*head_size].  Both contractions (q.K^T, P.V) run on
 * v_mfma_f32_16x16x4_f32 with an online softmax; per token the result equals kh_mha_f32 at
 * pos = pos0 + t within the fp32 tolerance.  head_size 48, 64 or 128, else KH_ERR_UNSUPPORTED. */
int kh_mha_prefill_f32(int32_t pos0, int32_t n_tokens, int32_t head_num, int32_t layer_index,
                       int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                       float* mha_out, const float* q, const float* key_cache,
                       const float* value_cache, void* stream);
/* The same launch in the output layout a model pass asks for: layout 0 / 1 = the tiled activation slab of an fp32 /
 * int8 model that the wo GEMM reads (mha_out holds dim * tcap floats; element (token t, column k) of the fp32 slab
 * sits at ((k / 16) * tcap + t) * 16 + k % 16), layout 2 = row-major as above.  n_tokens <= tcap <= 512 and
 * tcap % 16 == 0, else KH_ERR_INVALID_ARG; tcap is not read for layout 2 but checked all the same.  Layout 1
 * interleaves the quarters of 64-column blocks and needs dim % 64 == 0 (KH_ERR_INVALID_ARG). */
int kh_mha_prefill_layout_f32(int32_t pos0, int32_t n_tokens, int32_t head_num, int32_t layer_index,
                              int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                              int32_t layout, int32_t tcap, float* mha_out, const float* q,
                              const float* key_cache, const float* value_cache, void* stream);
/* The attention of the prompt prefill into sequence slots (kh_model_seq_prefill_gemm) as an operator: n_tiles
 * (1 .. 32) query tiles of 16 slab tokens, q is [16 * n_tiles][dim].  h_tiles is a HOST table of 5 x n_tiles int32:
 * pos0[], nvalid[], base[], pfx_len[], pfx_row0[].  The tokens of tile k are positions pos0[k] .. pos0[k] +
 * nvalid[k] - 1 (1 <= nvalid <= 16; the other columns of the tile repeat its last valid token and are stored too);
 * position p of its sequence is cache row pfx_row0[k] + p for p < pfx_len[k] (0 <= pfx_len <= pos0) and row
 * base[k] + p from there on (base may be negative).  Every such row up to position pos0 + nvalid - 1 must lie in
 * [0, seq_len), else KH_ERR_RANGE; 16 * n_tiles <= tcap <= 512, tcap % 16 == 0.  Layouts as above (row-major:
 * [16 * n_tiles][dim]). */
int kh_mha_prefill_tiles_f32(int32_t n_tiles, const int32_t* h_tiles, int32_t head_num, int32_t layer_index,
                             int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                             int32_t layout, int32_t tcap, float* mha_out, const float* q,
                             const float* key_cache, const float* value_cache, void* stream);

/* The decode-path attention kernel with its long-context machinery.  Per-head path: the grid
 * carries ceil(seq_len/256) (<= 16) workgroups per head; positions < 256 use one of them, longer
 * contexts split the timesteps and the last workgroup to finish merges the partial
 * (max, sum, o) triples.  GQA models (kv_mul 2/4/7/8) switch, from pos + 1 >= 4096 on
 * (env KH_ATTN_TLONG; 0 = never), to one workgroup per (kv group, time split) that computes the
 * group's kv_mul heads from ONE pass over the K/V rows.  `workspace` =
 * kh_mha_decode_workspace_bytes(...) bytes, 16-byte aligned, ZEROED once before first use (the
 * kernel re-arms it); may be NULL when that is 0. */
int64_t kh_mha_decode_workspace_bytes(int32_t head_num, int32_t head_size, int32_t seq_len);
int kh_mha_decode_f32(const int32_t* d_pos, int32_t pos, int32_t head_num, int32_t layer_index,
                      int32_t seq_len, int32_t kv_dim, int32_t kv_mul, int32_t head_size,
                      float* mha_out, const float* q, const float* kcache, const float* vcache,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* argmax_kernel_cu (cuda/argmax_kernel.cuh:4; argmax_sampler.cpp:5-13): index of the first
 * maximum.  Device-result form (graph-capturable) and host-result form (synchronises the
 * stream, like the reference's D2H copy at argmax_kernel.cu:84). */
int kh_argmax_f32(const float* logits, int64_t n, int32_t* d_out_index, void* stream);
int kh_argmax_f32_host(const float* logits, int64_t n, int64_t* h_out_index, void* stream);
/* The row form: d_out[r] = index of the first maximum of logits[r * row_stride .. + n), r < n_rows - the pick of a
 * verify pass (kh_model_verify) as an operator.  One workgroup per row, grids of at most 8 rows; asynchronous and
 * graph-capturable.  KH_ERR_INVALID_ARG for NULL pointers, n <= 0, n_rows <= 0, row_stride < n or row_stride not a
 * multiple of 4 (rows of a 16-byte aligned buffer then take 16-byte loads). */
int kh_argmax_rows_f32(const float* logits, int64_t n, int64_t row_stride, int32_t n_rows, int32_t* d_out,
                       void* stream);

/* Seeded sampling (the reference's sampler::Sampler interface, kuiper/include/sampler/sampler.h, has only the
 * argmax; these are further samplers behind it).  With temperature T, top_k K, top_p P, seed and a 64-bit counter c:
 *   1. T <= 0: greedy - exactly kh_argmax_f32 (ties -> lowest index), on the argmax kernels;
 *   2. order the tokens by (logit descending, index ascending);
 *   3. 0 < K < n: keep the first K of that order (K = 0 or K >= n: no top-k);
 *   4. weights w_i = exp((l_i - l_max) / T) of the kept tokens;
 *   5. P < 1: keep the shortest prefix of that order whose weight is >= P times the kept total (at least one
 *      token; P = 1: no top-p) = the set S;
 *   6. x = Philox4x32-10(counter = (c mod 2^32, 0, 0, 0), key = (seed & 0xffffffff, seed >> 32)) word 0,
 *      u = ((x >> 8) + 0.5) * 2^-24;
 *   7. the result is the smallest index j in S whose index-order prefix sum of w over S exceeds u * Z_S
 *      (Z_S = the weight of S); the largest index of S if rounding leaves none.
 * K = 1 is the argmax.  Logits must be finite or -inf.  KH_ERR_INVALID_ARG, before any device call, for a
 * non-finite T, K < 0, or P NaN or outside (0, 1].  One 1024-thread workgroup per draw: a histogram pass of
 * (l_max - l) / T, the candidates compacted into LDS when at most 4096 of them can be in S, exact radix descents
 * over them (csrc/kh_sample.h; DESIGN.md "Sampling" has the measured cost). */
typedef struct kh_sampling {
  float temperature; /* <= 0: greedy */
  int32_t top_k;     /* 0: off */
  float top_p;       /* 1: off */
  uint64_t seed;
} kh_sampling;
/* n_draws draws on one logit vector with counters counter0 .. counter0 + n_draws - 1 -> d_out[n_draws] (DEVICE;
 * graph-capturable, asynchronous) */
int kh_sample_f32(const float* logits, int64_t n, const kh_sampling* p, int64_t counter0, int32_t n_draws,
                  int32_t* d_out, void* stream);
/* one draw with the index in HOST memory: the twin of kh_argmax_f32_host (synchronises the stream) */
int kh_sample_f32_host(const float* logits, int64_t n, const kh_sampling* p, int64_t counter, int64_t* h_out,
                       void* stream);

/* Logit processors: repetition / presence / frequency penalties over a window of the fed tokens, and a logit bias,
 * applied IN PLACE to a logit vector ahead of the pick (the controls of llama.cpp's repeat_penalty / repeat_last_n /
 * presence_penalty / frequency_penalty / logit_bias and HF's repetition_penalty / bad_words_ids).  Let p be the
 * position whose logits are processed, V = n, N = last_n:
 *   1. the window is the positions j in [max(0, p + 1 - N), p]; N = 0: [0, p];
 *   2. t_j = the token FED at position j (prompt tokens count, as in llama.cpp); c(v) = the number of window
 *      positions with t_j == v; entries outside [0, V) are ignored (a never-written slot of a model's record is -1);
 *   3. for every v with c(v) > 0, once, in fp32, each operation rounded once and never contracted, in this order:
 *        l = l > 0 ? l / repetition : l * repetition            (skipped when repetition == 1)
 *        l = l - (float(c) * frequency + presence)              (skipped when both are 0)
 *   4. then for every bias entry (id, b): l[id] = l[id] + b.  A bias of -inf bans a token; -inf logits stay -inf
 *      through all three steps.
 * The caller keeps the processed logits finite or -inf with at least one finite entry (kh_sample_f32's
 * precondition).  The processed logits are bit-identical to the numpy float32 twin tests/logit_proc_ref.py.
 * KH_ERR_INVALID_ARG, before any device call, for repetition non-finite or <= 0, presence or frequency non-finite,
 * last_n < 0.  One 1024-thread workgroup, time proportional to the window, not to V (csrc/kh_logit_proc.h; DESIGN.md
 * 3.3c has the measured cost). */
typedef struct kh_penalties {
  float repetition;  /* 1: off; finite, > 0 */
  float presence;    /* 0: off; finite */
  float frequency;   /* 0: off; finite */
  int32_t last_n;    /* window length in positions; 0: the whole sequence; >= 0 */
} kh_penalties;
/* bytes of the operator's workspace: n int32 counters, zeroed ONCE by the caller; the kernel re-arms them */
int64_t kh_logit_process_workspace_bytes(int64_t n);
/* d_tokens[j] = token fed at position j, j <= position (DEVICE); the position is *d_pos (DEVICE, graph-capturable
 * form) or, when d_pos is NULL, pos; d_bias_ids / d_bias [n_bias] (DEVICE): distinct ids in [0, n), no NaN, no +inf -
 * an id outside [0, n) is skipped.  p NULL or (1, 0, 0, *) with n_bias 0: nothing is launched.  Asynchronous. */
int kh_logit_process_f32(float* logits, int64_t n, const int32_t* d_tokens, const int32_t* d_pos, int32_t pos,
                         const kh_penalties* p, const int32_t* d_bias_ids, const float* d_bias, int32_t n_bias,
                         void* workspace, void* stream);

/* Log-probabilities: what a pick was worth and which tokens it beat (the logprobs / top_logprobs of the inference
 * APIs).  The input is a logit vector l[0..V) with entries finite or -inf, at least one finite:
 *   1. m = max l;  lse = m + log(sum_i exp(l_i - m));
 *   2. lp(i) = l_i - lse;  lp(i) = -inf where l_i = -inf;
 *   3. the top-N, 0 <= N <= KH_LOGPROBS_MAX_TOP, are the first N tokens of the sampler's order (logit descending, index
 *      ascending): ties at the cut go to the lower index; if fewer than N logits are finite, -inf entries follow in
 *      index order with lp = -inf.
 * These are the log-probs of the softmax of l itself - inside a model, of the PROCESSED logits (after penalties and
 * bias, before temperature, top-k and top-p).  The ids are exact (ordering fp32 values involves no arithmetic); lse
 * and lp are fp32: the sum of exp is accumulated in fp32 (four strided partials per thread of a 1024-thread workgroup,
 * then a tree), within 2^-24 (ceil(V / 1024) + 16) + 2^-23 (|lse| + |lp|) of the fp64 values
 * (tests/logprobs_ref.py is the fp64 statement).  One 1024-thread workgroup per row; with the maximum known, one pass
 * over the logits for the sum and the candidate histogram and one for the gather of the candidates (csrc/kh_logprobs.h;
 * DESIGN.md 3.3d has the pass count and the cost). */
#define KH_LOGPROBS_MAX_TOP 20
/* logits [n_rows][n] row-major (DEVICE); d_ids[n_rows]: the token whose log-prob each row reports (an id outside
 * [0, n), or d_ids NULL, gives NaN) -> d_lse[n_rows], d_lp[n_rows], d_top_ids[n_rows][top_n], d_top_lp[n_rows][top_n]
 * (DEVICE; any of them may be NULL).  Asynchronous, graph-capturable, never allocates.  KH_ERR_INVALID_ARG, before any
 * device call, for top_n < 0, top_n > KH_LOGPROBS_MAX_TOP, top_n > n, n_rows <= 0 or a NULL logits. */
int kh_logprobs_f32(const float* logits, int64_t n, int32_t n_rows, const int32_t* d_ids, int32_t top_n, float* d_lse,
                    float* d_lp, int32_t* d_top_ids, float* d_top_lp, void* stream);

/* Constrained decoding: a TOKEN AUTOMATON is a deterministic automaton over token ids in CSR form.  Row s =
 * tokens[row_ptr[s] .. row_ptr[s + 1]) holds the ids allowed in state s, strictly ascending, and next[] the state behind
 * each.  With a state s and a logit vector l[0..V):
 *   1. every l[v] with v NOT in row s becomes -inf - a logit bias of -inf on exactly those ids;
 *   2. with t the token picked from the masked vector, s = next(s, t).
 * -inf stays -inf through all three steps of kh_logit_process_f32 and a bias may not be +inf, so masking AHEAD of the
 * processors and biasing by -inf BEHIND them leave the same bits in every entry: a constrained step equals an
 * unconstrained one whose bias list bans the ids outside the row.  The end of the output is part of the automaton:
 * accepting states carry an edge on the stop token into a sink whose only edge is that token onto itself, so steps
 * that run past a stop stay legal.
 * kh_fsm_check, host only, the checks every call that takes an automaton makes before any device call:
 * KH_ERR_INVALID_ARG for NULL arrays, n_states <= 0, start or any next outside [0, n_states), row_ptr not non-decreasing
 * from 0, a row that is not strictly ascending, a row with NO edge (the sampler needs one finite logit); KH_ERR_RANGE
 * for a token outside [0, vocab).
 * kh_fsm_walk, host only: from `state`, follows tokens[0..n) as far as every token is in the row of the state reached;
 * *out_state = the state behind the *n_ok tokens it could follow (the state behind words a model returned). */
typedef struct kh_fsm {
  int32_t n_states, start;
  const int64_t* row_ptr;  /* [n_states + 1] */
  const int32_t* tokens;   /* [n_edges] ascending and distinct within a row, in [0, vocab) */
  const int32_t* next;     /* [n_edges] state after that token */
} kh_fsm;
int kh_fsm_check(const kh_fsm* a, int64_t vocab);
int kh_fsm_walk(const kh_fsm* a, int32_t state, const int32_t* tokens, int64_t n, int32_t* out_state, int64_t* n_ok);
/* The mask as an operator, in place: bit v & 31 of word v >> 5 of d_mask (DEVICE, ceil(n / 32) words) clear means
 * logits[v] = -inf; every other entry keeps its bits; bits past n in the last word are ignored.  Asynchronous,
 * graph-capturable, never allocates.  KH_ERR_INVALID_ARG for NULL pointers or n <= 0. */
int kh_token_mask_f32(float* logits, int64_t n, const uint32_t* d_mask, void* stream);

/* CPU-only helpers of the reference (kernels_interface.h:38-46), provided on device so the
 * op set is closed: softmax in place, x *= scale, out += sum_t scale[t]*value[t*stride..] */
int kh_softmax_f32(float* x, int32_t n, void* stream);
int kh_scale_f32(float scale, float* x, int32_t n, void* stream);
int kh_scale_sum_f32(const float* value, const float* scale, float* out, int32_t pos,
                     int32_t size, int32_t stride, void* stream);

/* ============================ model level ==============================================
 * Replaces model::LLama2Model / Qwen2Model for the decode path: .bin image -> HBM arena,
 * per-token forward, greedy generate loop captured in a hipGraph. */
typedef struct kh_model kh_model;

typedef struct kh_model_opts {
  int32_t family;      /* KH_FAMILY_* : weight layout (llama3.cpp:290-423 / qwen2.cpp) */
  int32_t is_quant;    /* int8 group-quantised image (tools/export.py version 3) */
  int32_t rope_mode;   /* KH_ROPE_* */
  float rope_theta;    /* 10000 / 500000 (LLAMA3) / 1000000 (QWEN2) in the reference */
  float rms_eps;       /* 1e-5 / 1e-6 (QWEN2) */
  int32_t max_seq_len; /* rows of KV cache + sin/cos to allocate; 0 = header seq_len */
  int32_t device;      /* HIP device ordinal (reference: cudaSetDevice(0)) */
  int32_t flags;       /* KH_FLAG_* bits, 0 = defaults */
} kh_model_opts;
/* decode attention at positions that need several time splits: merge the split partials inside the
 * attention launch (ticket + last arriver) instead of in the wo kernel that follows (the default) */
#define KH_FLAG_ATTN_MERGE_IN_LAUNCH 1
/* the in-launch merge of time splits (operator entry points, prompt slices, the GQA group path, and everything
 * under KH_FLAG_ATTN_MERGE_IN_LAUNCH) orders its hand-over with agent-scope release / acquire FENCES instead of the
 * default write-through stores + drained vmcnt + sc1 loads (csrc/kh_attn.h: attn_publish_barrier).  Same
 * results; 1-2 us slower per layer at positions that need several splits.  Hook KH_ATTN_FENCED=1 does the same
 * for models created while it is set and for kh_mha_decode_f32 / kh_mha_f32. */
#define KH_FLAG_ATTN_MERGE_FENCED 2
/* The prompt phase of kh_model_generate*.  The reference feeds the prompt one token per forward pass
 * (demo/main.cpp:20-22), so its prompt phase is, bit for bit, its decode path.  Two batched prompt paths exist here:
 *  - default: prompts with >= 16 fed-only tokens run as fp32-MFMA GEMMs (kh_model_prefill_gemm, 45-60 k prompt
 *    tokens/s on Llama-3.2-1B): K/V rows equal to fp32 round-off, i.e. the greedy continuation can differ from the
 *    reference's at near-ties (kh_model_first_sample reports the margin of the first sampled step);
 *  - KH_FLAG_PREFILL_EXACT: every prompt runs on the B-token VALU kernels (kh_model_prefill, 5.9 k prompt
 *    tokens/s): K/V rows and every later logit are bit-identical to the token-by-token prompt phase - what a
 *    drop-in user who needs token identity with the reference's own prompt phase sets.
 * kh_first_sample.prefill_mode says which one the last generate took.  The test hook KH_PREFILL overrides both. */
#define KH_FLAG_PREFILL_EXACT 4
/* fp32 models keep a bf16 copy of the classifier (vocab x dim x 2 bytes of HBM, made at creation) with which the
 * greedy steps of kh_model_generate* (graph and fused exec) find the argmax without streaming the fp32 classifier:
 * the copy screens the rows, the rows that can still win are re-scored from their fp32 rows, the tokens are
 * bit for bit those of the full classifier, and kh_model_get_logits behind such a run computes the last step's
 * logits on demand (csrc/kh_cls_screen.h).  This flag - or hook KH_CLS_SCREEN=0 at creation - leaves the copy out;
 * the hook set later turns screening off for the generates that follow.  A KH_SHAPE_CLS hook (a specific k_cls
 * launch was asked for) does the same, unless KH_CLS_SCREEN=force is set beside it: screening stays on and
 * re-scores with the hooked U, staging depth and workgroup width (tests reach every k_sample_screen instantiation
 * this way).  kh_model_cls_screen_info reports; kh_model_cls_screen_probe / _read expose one screened step on a
 * caller-supplied vector, every row's interval, the bf16 copy and its error table to the tests. */
#define KH_FLAG_NO_CLS_SCREEN 8
/* W16: a bf16-exact fp32 model runs from a 16-bit copy of its matrices, bit for bit.  An fp32 .bin that was
 * exported from a bf16 checkpoint holds zeros in the low 16 bits of every matrix word; with this flag the model keeps a
 * second arena with the upper halves of wq, wk, wv, wo, w1, w2, w3 of every layer and of the classifier matrix (half
 * their bytes on top of the fp32 image) and the decode GEMVs stream that copy: the same tokens, logits, K/V rows and
 * log-prob records as without the flag, compared as raw bits, from half the weight bytes per token.  The B-token
 * passes - kh_model_prefill, kh_model_score, kh_model_verify / kh_model_generate_lookup, kh_model_seq_prefill,
 * kh_model_seq_step[_ex], kh_model_generate_batch[_ex] - read the copy too, with the same bits, for the launch classes
 * of the pass mask: by default ffn13 and w2, the two that gain on every measured geometry; hook KH_W16_PASS at
 * creation: 0 none (the passes stream fp32), 0x1f all five, any other number a mask of the class bits below, 1 or
 * unset the default.  Still reading the fp32 image whatever the masks say: the MFMA GEMM prefill
 * (kh_model_prefill_gemm, long prompts of kh_model_generate without KH_FLAG_PREFILL_EXACT; KH_FLAG_GEMM16 below puts its
 * GEMMs on the copy), the operator level, the
 * exact re-score of the screened greedy tails and the embedding gather.  Nothing is ever rounded: if one matrix word
 * of the image has a non-zero low half the copy is freed and the model behaves as if the flag were not set; likewise
 * on int8 images.  Hook KH_W16=1 / 0 at creation overrides the flag.  kh_model_w16_info reports. */
#define KH_FLAG_W16 16
/* W16 for fp16-origin checkpoints (Llama-2): keep the 16-bit copy in whichever format the image is exact in.  First
 * bf16, exactly as KH_FLAG_W16 (its kernels, all or nothing); if some matrix word is not bf16-exact, fp16: a word
 * qualifies when it is +-0, an fp16 normal (2^-14 .. 65504, low 13 mantissa bits zero) or an fp16 subnormal (a multiple
 * of 2^-24 below 2^-14); Inf and NaN do not.  The copy then holds the IEEE binary16 value of every matrix word (same
 * layout and bytes), the kernels convert each back - exactly - and run the FMAs of the fp32 kernels in their order, so
 * the bits are again those of the fp32 run; the creation-time self-check covers this copy as it covers a bf16 one.  If
 * the image is exact in neither format there is no copy (state -1).  Implies KH_FLAG_W16; everything said there about
 * the passes, KH_W16_PASS and what still reads fp32 holds.  Hook KH_W16_F16=1 / 0 at creation overrides this bit;
 * KH_W16=0 still means no copy at all.  kh_model_w16_info slots 6 and 7 report. */
#define KH_FLAG_W16_F16 32
/* Q4: a 4-bit-exact int8 model runs its batch-1 decode GEMVs from a packed 4-bit copy of its matrices, bit for bit.  An
 * int8 .bin whose quantised values all lie in [-8, 7] is a legal int8 checkpoint; with this flag the model keeps a
 * second arena with the low nibbles of wq, wk, wv, wo, w1, w2, w3 of every layer and of wcls, two values per byte
 * (half the int8 matrix bytes more HBM; the fp32 group scales are read where the image keeps them), and the decode
 * GEMVs of the adopted launch classes (kh_plan_q4) stream it through kernels that run the int8 kernels' FMAs in their
 * order.  The B-token passes (prefill, score, verify, the sequence-slot calls) of the classes in the pass mask stream
 * the copy as well, through twins that leave the int8 pass's bits; the mask is KH_Q4_PASS's, independent of the decode
 * classes, and by default w2 alone (the one class that passed the adoption rule on every measured geometry: DESIGN
 * 3.1d).  The int8
 * image stays and everything else reads it: the MFMA GEMM prefill, the wide pass, the operator level and the embedding
 * gather.  Nothing is ever rounded: one value outside [-8, 7] and the copy is
 * freed and the model behaves as if the flag were not set; likewise on fp32 images (KH_FLAG_W16* on an int8 image
 * does nothing either).  Hooks at creation: KH_Q4=1 / 0 overrides the flag, KH_Q4_CLASSES=<mask> the adopted
 * classes, KH_Q4_PASS=<mask> the classes whose B-token pass reads the copy (0x1f: all five; unset or 1: the default;
 * no effect without a live copy).  kh_model_q4_info reports. */
#define KH_FLAG_Q4 64
/* GEMM16: the GEMM pass of a W16 model on the bf16 matrix cores, fp32-accurate (csrc/kh_gemm_w16.h).  Takes effect only
 * where the model holds a live 16-bit copy in bf16 format (KH_FLAG_W16, or KH_FLAG_W16_F16 on a bf16-exact image) and
 * the GEMM prefill runs on its geometry.  The GEMMs of kh_model_prefill_gemm (and the default prompt path of
 * kh_model_generate), kh_model_seq_prefill_gemm, kh_model_seq_step_gemm and kh_model_generate_batch_gemm then read the
 * bf16 weights of the copy and split every fp32 activation exactly into three bf16 terms (hi + mid + lo == x), so three
 * v_mfma_f32_16x16x32_bf16 per 32 columns accumulate the fp32 dot product in fp32: kh_model_prefill_gemm's contract
 * (fp32 round-off from another summation order), not the bits of the fp32 kernels.  Per launch class (1 qkv, 2 wo,
 * 4 ffn13, 8 w2, 16 cls): a class whose contraction length is no multiple of 32, or that the adoption mask leaves out
 * (kh_plan_gemm16; hook KH_GEMM16_CLASSES=<mask> at creation), keeps its fp32 kernel.  Inert - the launches and bits of
 * the same model without the flag - on an fp16-format copy, an int8 model, an image that is not bf16-exact, and without
 * a W16 flag.  Hook KH_GEMM16=1 / 0 at creation overrides the flag.  kh_model_gemm16_info reports. */
#define KH_FLAG_GEMM16 128
/* GEMM16_Q8: the GEMM pass of an int8 group-64 model on the bf16 matrix cores, fp32-accurate, from the int8 image itself
 * (csrc/kh_gemm_q16.h): no weight copy, no extra memory.  The GEMMs of kh_model_prefill_gemm (and the default prompt path
 * of kh_model_generate), kh_model_seq_prefill_gemm, kh_model_seq_step_gemm and kh_model_generate_batch_gemm convert the
 * int8 weights exactly to bf16 in registers, split every fp32 activation exactly into three bf16 terms and multiply the
 * fp32 partial sum of each group of 64 columns by the group's scale: six v_mfma_f32_16x16x32_bf16 per group instead of
 * sixteen v_mfma_f32_16x16x4_f32.  kh_model_prefill_gemm's int8 contract (exact products, fp32 accumulation) in another
 * summation order and without the per-weight rounding of scale * q: not the bits of the int8 kernels.  Per launch class
 * (1 qkv, 2 wo, 4 ffn13, 8 w2, 16 cls): a class the adoption mask leaves out (kh_plan_gemm16_q8; hook
 * KH_GEMM16_Q8_CLASSES=<mask> at creation) keeps its int8 kernel.  Inert - the launches and bits of the same model
 * without the flag - on an fp32 model, a group size other than 64 and a geometry the GEMM prefill does not take.
 * Independent of KH_FLAG_Q4 (the GEMM passes of a Q4 model read the int8 image) and of KH_FLAG_GEMM16 (inert on int8).
 * Hook KH_GEMM16_Q8=1 / 0 at creation overrides the flag.  kh_model_gemm16_q8_info reports. */
#define KH_FLAG_GEMM16_Q8 256

typedef struct kh_config {
  int32_t dim, hidden_dim, layer_num, head_num, kv_head_num, vocab_size, seq_len;
  int32_t kv_dim, kv_mul, head_size, is_shared_weight, is_quant, group_size;
  int32_t family, rope_mode, cache_len;
  float rope_theta, rms_eps;
  int64_t weight_bytes; /* bytes of the weight arena resident in HBM */
  int32_t launches_per_token; /* 5 per layer + classifier + sampler */
  /* Self-checks run once at the end of kh_model_create_* (csrc/kh_model_selftest.hip), about a millisecond:
   *   ring_selftest        the int8 LDS-DMA ring kernels against the register-tile kernels of the same launches on
   *                        this model's own weights: 0 = no ring kernel planned (fp32, geometry, KH_RING=0) or skipped,
   *                        1 = outputs identical, -1 = mismatch: this model runs the register-tile kernels;
   *   attn_merge_selftest  the fence-free in-launch merge of the decode-attention time splits against the fenced
   *                        form: 0 = not applicable (no time splits in this cache) or skipped, 1 = identical,
   *                        -1 = mismatch: this model uses the fenced form, 2 = the fenced form was requested
   *                        (KH_FLAG_ATTN_MERGE_FENCED / KH_ATTN_FENCED=1).
   * Hook KH_SELFTEST=0 skips both, KH_SELFTEST_FAIL="ring,attn" injects a failure (tests). */
  int32_t ring_selftest, attn_merge_selftest;
} kh_config;

/* Model::read_model_file + init (model.cpp:41-123, llama3.cpp:107-145) */
int kh_model_create_from_file(const char* path, const kh_model_opts* opts, kh_model** out);
/* same, from the bytes of a .bin file already in host memory (header included) */
int kh_model_create_from_host_image(const void* h_image, size_t nbytes,
                                    const kh_model_opts* opts, kh_model** out);
/* weights already resident in HBM: h_header = the 7 (fp32) or 8 (int8) header ints,
 * d_weight_data = the file bytes AFTER the header, 16-byte aligned, not owned
 * (the reference's "external buffer", layer.cpp:190-202). */
int kh_model_create_from_device_weights(const int32_t* h_header, const void* d_weight_data,
                                        size_t weight_nbytes, const kh_model_opts* opts,
                                        kh_model** out);
void kh_model_destroy(kh_model* m);
int kh_model_get_config(const kh_model* m, kh_config* out);
void* kh_model_stream(kh_model* m); /* the model's hipStream_t */
/* milliseconds the host-image -> HBM upload took (0 for device-resident weights) */
float kh_model_get_load_ms(const kh_model* m);

enum {
  KH_EXEC_GRAPH = 0,   /* fused kernels, whole step replayed as one hipGraph */
  KH_EXEC_FUSED = 1,   /* fused kernels, eager launches */
  KH_EXEC_UNFUSED = 2  /* one launch per reference kernel, in the reference's order
                          (llama3.cpp:147-167): the literal drop-in sequence */
};

/* Model::predict (llama3.cpp:642-650): embedding of `token` -> forward at `pos` ->
 * argmax (or the kh_model_set_sampling draw) unless is_prompt.  *h_next receives the token (or -1 when is_prompt).
 * Synchronises the stream. exec: KH_EXEC_FUSED or KH_EXEC_UNFUSED. */
int kh_model_predict(kh_model* m, int32_t token, int32_t pos, int32_t is_prompt, int32_t exec,
                     int32_t* h_next);
/* copy the last logits (kForwardOutput) to host; behind a step that ran the model's logit processors
 * (kh_model_set_penalties / kh_model_set_logit_bias) these are the PROCESSED logits: processing is in place */
int kh_model_get_logits(kh_model* m, float* h_logits);
/* the screened classifier (KH_FLAG_NO_CLS_SCREEN): out[8] = on (0 / 1), creation-time self-test (0 not run, 1 passed,
 * -1 failed: screening off), HBM bytes of the bf16 copy and its row table, microseconds its conversion took, screened
 * steps so far, candidate rows re-scored in them, steps that overflowed into the full classifier, candidate
 * capacity of a step */
int kh_model_cls_screen_info(kh_model* m, int64_t* out8);
/* W16 (KH_FLAG_W16): out[8] = state (0 off or not applicable, 1 on, -1 a matrix is not bf16-exact, -2 the creation-time
 * self-check failed - in both cases the model streams fp32), bytes of the 16-bit copy, its build time in us, bit mask of
 * the launch classes that run on it (1 qkv, 2 wo, 4 ffn13, 8 w2, 16 cls), index of the first inexact tensor (7 * layer
 * + {wq, wk, wv, wo, w1, w2, w3}, 7 * layers: the classifier; -1 none), bit mask of the launch classes whose B-token
 * passes (prefill, score, verify, sequence slots) run on it as well - a subset of the first mask, 0 unless state is 1 -
 * then the format of the live copy (0 bf16 or no copy, 1 fp16: KH_FLAG_W16_F16) and 1 + the index of the first tensor
 * that is not fp16-exact (0: fp16 was not tried, or every tensor passed).  With KH_FLAG_W16_F16 state -1 means exact
 * in neither format, and slot 4 keeps the first tensor that is not bf16-exact. */
int kh_model_w16_info(kh_model* m, int64_t* out8);
/* Q4 (KH_FLAG_Q4): out[8] = state (0 off or not applicable, 1 on, -1 a value lies outside [-8, 7], -2 the creation-time
 * self-check failed - in both cases the model launches what it launches without the flag), bytes of the 4-bit copy,
 * its build time in us, bit mask of the launch classes that run on it (1 qkv, 2 wo, 4 ffn13, 8 w2, 16 cls), index of
 * the first inexact tensor (7 * layer + {wq, wk, wv, wo, w1, w2, w3}, 7 * layers: wcls; -1 none), bit mask of the launch
 * classes whose B-token passes (prefill, score, verify, sequence slots) run on the copy - hook KH_Q4_PASS, whatever the
 * first mask says, 0 unless state is 1; slots 6 and 7 are 0. */
int kh_model_q4_info(kh_model* m, int64_t* out8);
/* GEMM16 (KH_FLAG_GEMM16): out[8] = state (1: some class of the GEMM pass runs on the bf16 matrix cores, 0: inert), bit
 * mask of those classes (1 qkv, 2 wo, 4 ffn13, 8 w2, 16 cls), the reason where inert (0 none, 1 flag not set, 2 no W16
 * flag, 3 int8 model, 4 image not bf16-exact, 5 the copy is in fp16 format, 6 geometry off the GEMM prefill or the W16
 * view, 7 no class left by the mask and the K % 32 rule, 8 the copy's creation-time self-check failed), kh_plan_gemm16's
 * mask for the geometry (0 where inert before the plan); slots 4 - 7 are 0. */
int kh_model_gemm16_info(kh_model* m, int64_t* out8);
/* GEMM16_Q8 (KH_FLAG_GEMM16_Q8): out[8] = state (1: some class of the GEMM pass runs on the bf16 matrix cores from the
 * int8 image, 0: inert), bit mask of those classes (1 qkv, 2 wo, 4 ffn13, 8 w2, 16 cls), the reason where inert (0 none,
 * 1 flag not set, 2 fp32 model, 3 group size is not 64, 4 geometry off the GEMM prefill, 5 no class left by the mask),
 * kh_plan_gemm16_q8's mask for the geometry (0 where inert before the plan); slots 4 - 7 are 0. */
int kh_model_gemm16_q8_info(kh_model* m, int64_t* out8);
/* tests: one screened step (k_cls_screen + k_sample_screen, as a generate launches them) and one full step (k_cls +
 * k_sample) on the residual vector h_x[dim], without advancing.  h_lb / h_ub [vocab]: the interval the screen gave
 * every row.  out4 = screened token, full classifier's token, candidate rows re-scored, 1 if the step overflowed.
 * Afterwards kh_model_get_logits returns k_cls's logits of h_x and the counters of kh_model_cls_screen_info are as
 * before, also behind a failed copy or launch.  Clobbers the model's residual vector, the screen's saved input and
 * the next-token word: the generate or step that follows sets its own.  KH_ERR_UNSUPPORTED where the model does
 * not screen. */
int kh_model_cls_screen_probe(kh_model* m, const float* h_x, float* h_lb, float* h_ub, int64_t* out4);
/* tests: the bf16 copy of the classifier [vocab x dim] and its per-row error table [vocab] */
int kh_model_cls_screen_read(kh_model* m, uint16_t* h_wbf, float* h_err);
/* The int8 tier ahead of the bf16 screen (csrc/kh_cls_screen.h): fp32 models with the bf16 screen on and dim a multiple
 * of 64 also keep an int8 copy of the classifier with one fp32 scale per 64 weights (about 0.27 of the classifier's
 * bytes).  Screened greedy steps then run three launches behind the layers (5 L + 3 in all): k_cls_screen_q8 thins the
 * vocabulary to the few rows whose int8 interval reaches the best lower bound, k_cls_screen screens those from the
 * bf16 copy, k_sample_screen re-scores.  Tokens and logits are unchanged.  The tier steps aside - the tail is the
 * two-launch one - under hook KH_CLS_SCREEN_Q8=0 (at creation: no copy; later: for the generates that follow), under
 * a KH_SHAPE_SCREEN or KH_SHAPE_CLS hook, and when its creation-time self-test fails (hook KH_SELFTEST_FAIL=screen8
 * injects that).  Hook KH_SHAPE_SCREEN_Q8="u,grid,wg" shapes its launch.
 * out8 = on, self-test (0 / 1 / -1), HBM bytes of the copy with its scales and row table, microseconds its conversion
 * took, tier-1 steps so far, rows that survived tier 1 in them, steps in which tier 1 spilled (a workgroup dropped a
 * row that could still win: the bf16 launch then scans every row), rows a tier-1 workgroup hands over */
int kh_model_cls_screen_q8_info(kh_model* m, int64_t* out8);
/* tests: one three-launch tail, tier 1 on `grid` workgroups (0: as planned), and one full step on h_x[dim], without
 * advancing.  h_lb8 / h_ub8 [vocab]: tier 1's interval of every row.  out6 = the tail's token, the full classifier's
 * token, rows that survived tier 1, 1 if tier 1 spilled, candidate rows re-scored, 1 if the step overflowed.  Counters
 * and clobbered state as kh_model_cls_screen_probe.  KH_ERR_UNSUPPORTED where the tier is off. */
int kh_model_cls_screen_q8_probe(kh_model* m, const float* h_x, int32_t grid, float* h_lb8, float* h_ub8, int64_t* out6);
/* tests: the int8 copy [vocab x dim], its scales [vocab x dim / 64] and its per-row error table [vocab] */
int kh_model_cls_screen_q8_read(kh_model* m, int8_t* h_q, float* h_sc, float* h_e8);
/* device pointers of the KV cache [layer, cache_len, kv_dim] (tests) */
int kh_model_get_kv(kh_model* m, float** d_kcache, float** d_vcache);
/* bytes of the KV cache: *reserved = the address range of [layer, cache_len, kv_dim] floats x 2 (the reference's
 * up-front allocation, llama3.cpp:469-472), *committed = HBM actually backing it now.  The range is reserved at
 * creation and memory is mapped in 8-MiB chunks as generate / predict / prefill / kh_model_write_kv first reach
 * rows (hook KH_KV_VMM=0: one plain allocation, committed == reserved).  kh_model_get_kv commits everything.
 * kh_model_destroy releases the memory but keeps the two address ranges in a process-wide list for the next model
 * with caches of the same size (hipMemAddressFree is never called: it crashes inside the runtime after 1000-2000
 * create / destroy cycles, profiles/r6_vmm_destroy_crash.txt). */
int kh_model_kv_bytes(const kh_model* m, int64_t* reserved, int64_t* committed);
/* copy rows [row0, row0+nrows) of one layer's K and V cache to host (tests) */
int kh_model_read_kv(kh_model* m, int32_t layer, int32_t row0, int32_t nrows, float* h_k,
                     float* h_v);
/* the inverse: overwrite rows [row0, row0+nrows) of one layer's K and V cache from host memory or
 * from memory of the model's device (restoring a saved context; tests and the long-context probes
 * of bench.py place rows at deep positions without decoding up to them).  Rows hold what the
 * forward pass stores: RoPE-rotated keys, raw values. */
int kh_model_write_kv(kh_model* m, int32_t layer, int32_t row0, int32_t nrows, const float* h_k,
                      const float* h_v);

/* demo/main.cpp:5-47 generate(): prompt fed one token per step without sampling, then
 * greedy decode, `total_steps` forward passes in total; h_words receives the reference's
 * `words` vector.  No stop-token check (see kh_model_generate_until).  *h_elapsed_ms = wall
 * time of the step loop measured with HIP events on the model stream.
 * A generate starts a NEW sequence at position 0 and owns the cache rows [0, max(total_steps, 8)): with
 * KH_EXEC_GRAPH, the first call after model creation (or after a longer run than any before grew the step
 * buffers) launches each freshly captured step graph once from position 0 before the timed loop - rows and words
 * 0 .. 7 - so that no later run pays a graph's first launch; rows beyond that range are never touched. */
int kh_model_generate(kh_model* m, const int32_t* h_prompt, int32_t n_prompt,
                      int32_t total_steps, int32_t exec, int32_t* h_words, int32_t* n_words,
                      float* h_elapsed_ms);
/* The same loop with the reference's stop check (demo/main.cpp:30-32, Model::is_sentence_ending
 * model.cpp:211-214): generation ends at the first SAMPLED token that is in h_stop[0..n_stop)
 * (SentencePiece: eos_id, encode.cpp:48-51; BPE: two stop tokens, encode.cpp:133-139); that token
 * is not appended to `words`, *n_words = the reference's return value min(pos, total_steps).
 * Graph mode checks chunk k's words from pinned memory while chunk k+1 is already queued, so
 * there is no per-token host round trip; at most 2*8 steps run past the stop and are discarded. */
int kh_model_generate_until(kh_model* m, const int32_t* h_prompt, int32_t n_prompt,
                            int32_t total_steps, int32_t exec, const int32_t* h_stop,
                            int32_t n_stop, int32_t* h_words, int32_t* n_words,
                            float* h_elapsed_ms);

/* Prompt prefill (extends the reference, which feeds prompt tokens one forward pass at a time,
 * demo/main.cpp:20-22): forward of tokens[0..n) at positions pos0.., 8 (fp32) or 4 (int8)
 * tokens per pass over the weights, no logits.  Leaves the K/V cache rows pos0..pos0+n-1 BIT-IDENTICAL to n calls of
 * kh_model_predict(.., is_prompt = 1, KH_EXEC_FUSED).  kh_model_generate* use it for the
 * fed-only part of prompts of 3+ tokens (env KH_PREFILL=0 disables).  KH_ERR_UNSUPPORTED for
 * geometries outside the mirrored kernels (head_size <= 32, dim > 4096). */
int kh_model_prefill(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0);

/* The same contract with the contractions as fp32-MFMA GEMMs (csrc/kh_gemm.h): up to 512 prompt
 * tokens share one pass over the weights (a longer prompt is cut into 512-token passes plus a
 * remainder; env KH_PG_CHUNK = 16..512 sets another pass size) (v_mfma_f32_16x16x4_f32, exact fp32 arithmetic, tokens on
 * the MFMA N dimension; int8 weights dequantised per element in registers).  The K/V rows agree
 * with the token-by-token path to fp32 round-off (different summation order), not bit for bit.
 * kh_model_generate* use it for prompts with >= 16 fed-only tokens unless the model was created with
 * KH_FLAG_PREFILL_EXACT - so for such prompts the greedy tokens carry this tolerance too and can differ from the
 * token-by-token prompt phase at near-ties;
 * hook KH_PREFILL = 0 | token | gemv | gemm overrides (gemv = the bit-identical path; any other
 * value makes generate return KH_ERR_INVALID_ARG).  KH_ERR_UNSUPPORTED: head_size <= 32, dim/hidden not a multiple of 16 (fp32) /
 * 64 (int8), int8 group size != 64. */
int kh_model_prefill_gemm(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0);

/* Near-tie report for prompts that went through a prefill.  The token-by-token prompt phase and kh_model_prefill
 * leave bit-identical K/V rows; kh_model_prefill_gemm (the default of kh_model_generate* from 16 fed-only tokens on)
 * leaves them within fp32 round-off, so the greedy continuation is the token-by-token one unless two logits of a
 * sampled step lie closer together than that round-off.  After every kh_model_generate* call whose prompt phase ran
 * as a prefill, the logits of the FIRST sampled step (the one the whole prompt feeds; later steps inherit its choice)
 * are kept on the device; this call returns their two largest entries.  top1_id is the token that step sampled;
 * top1 - top2 is the margin to compare with the tolerance the caller cares about (the parity tests use 4e-5 for
 * fp32, 1e-4 for int8 weights: tests/test_model_gpu.py).  prefill_mode: 1 = kh_model_prefill (bit-identical rows),
 * 2 = kh_model_prefill_gemm.  KH_ERR_UNSUPPORTED when the last generate had no prefill phase (prompts of fewer than
 * 3 tokens, KH_PREFILL=0, unsupported geometry): its tokens are the token-by-token ones by construction. */
typedef struct kh_first_sample {
  int32_t pos;           /* position of the first sampled step = n_prompt - 1 */
  int32_t prefill_mode;  /* 1 = B-token VALU prefill (bit-identical), 2 = MFMA GEMM prefill (fp32 tolerance) */
  int32_t top1_id, top2_id;
  float top1, top2;      /* the two largest logits of that step; ties -> lowest index first, like the sampler */
} kh_first_sample;
int kh_model_first_sample(kh_model* m, kh_first_sample* out);

/* The model's sampler (NULL = greedy, the default of every model).  Applies to kh_model_predict (fused and unfused),
 * kh_model_generate and kh_model_generate_until; the semantics are kh_sample_f32's with the counter = the position
 * whose logits are sampled, so the tokens depend only on (seed, prompt, parameters, logits): not on the exec mode,
 * on how steps are cut into graph chunks, or on whether generate or a loop of predict calls produced them.  Prompt
 * positions are never sampled.  The parameters live in a small device buffer written on the model stream, so a new
 * seed or temperature needs no graph recapture; greedy and sampled steps are captured as separate graphs, and the
 * sampled step replaces only the last launch (k_sample -> k_sample_topp: launches_per_token is unchanged).
 * KH_ERR_INVALID_ARG as kh_sample_f32.  kh_model_first_sample keeps reporting the two largest logits. */
int kh_model_set_sampling(kh_model* m, const kh_sampling* p);
int kh_model_get_sampling(const kh_model* m, kh_sampling* out);

/* The model's logit processors (NULL / n = 0 = off, the default of every model): kh_logit_process_f32's semantics
 * on the logits of every SAMPLED position of kh_model_predict (fused and unfused), kh_model_generate and
 * kh_model_generate_until, ahead of the pick - the first maximum (lowest index) of the processed logits, or, with a
 * sampler set, kh_sample_f32's draw on them with counter = position.  Prompt positions are never processed.  The
 * window runs over the model's record of the token fed at every position, which kh_model_predict, the generate
 * loops, kh_model_prefill and kh_model_prefill_gemm keep; like the K/V rows, slots below the position of a call are
 * whatever earlier calls left (generate steps that run with processors off do not record).  While anything is on, the
 * step's last launch is k_sample_proc (processing, one max pass, the pick: launches_per_token is unchanged) and the
 * screened classifier is not used; all-neutral penalties (1, 0, 0, *) and no bias entries are "off": the model then
 * runs exactly the launches it runs without this feature.  Parameters and the bias list live in device buffers
 * written on the model stream: new values need no graph recapture (a list longer than any before - 64 entries at
 * least fit - rebuilds the graphs).  kh_model_get_logits and kh_model_first_sample report the processed logits, so
 * top1_id stays the greedy pick.
 * kh_model_set_logit_bias, before any device call: KH_ERR_INVALID_ARG for a NaN or +inf bias, a duplicate id, -inf on
 * all vocab_size ids; KH_ERR_RANGE for an id outside [0, vocab_size). */
int kh_model_set_penalties(kh_model* m, const kh_penalties* p);
int kh_model_get_penalties(const kh_model* m, kh_penalties* out);
int kh_model_set_logit_bias(kh_model* m, const int32_t* h_ids, const float* h_bias, int32_t n);

/* Per-token log-probabilities of the model's picks (top_n = -1: off, the default of every model; 0: the picked token
 * only; 1 .. KH_LOGPROBS_MAX_TOP: and that many alternatives).  While on, every SAMPLED position p of kh_model_predict
 * (fused and unfused), kh_model_generate and kh_model_generate_until leaves a record: the picked token (= words[p]),
 * its log-prob, top_id[top_n] and top_lp[top_n] - kh_logprobs_f32's semantics on the logits the pick was made from
 * (the processed logits when processors are on; never the tempered or truncated sampling distribution).  Asking for
 * log-probs changes no token: the pick is the first maximum, or kh_sample_f32's draw with counter = position, exactly
 * as without them.  A position that predict, generate or a prefill fed but did not sample - prompt positions, rows a
 * prefill covered - holds the "none" record: token -1, ids -1, NaN floats (kh_model_score, below, is the call that
 * leaves records at fed positions).  A generate resets the records of its prompt positions [0, n_prompt - 1)
 * to "none"; like the K/V rows, records of other positions are whatever earlier calls left.  Records live in device
 * buffers sized by the cache, allocated by the first call that turns the feature on.  While on, the step's last launch
 * is k_sample_lp (k_sample_proc's duties, then the record: launches_per_token is unchanged) and the screened classifier
 * is not used; while off the model runs exactly the launches it runs without this feature.  top_n lives in a device
 * word written on the model stream and records have a fixed stride: a new top_n needs no graph recapture.
 * kh_model_set_logprobs: KH_ERR_INVALID_ARG for top_n < -1, top_n > KH_LOGPROBS_MAX_TOP or top_n > vocab_size.
 * kh_model_get_logprobs copies the records of positions [pos0, pos0 + n) to the host - h_token[n], h_lp[n],
 * h_top_ids[n][top_n], h_top_lp[n][top_n] with top_n the setting in force at the call (none while off); any of them may
 * be NULL - and synchronises the stream.  KH_ERR_UNSUPPORTED when log-probs were never turned on, KH_ERR_RANGE for a
 * range outside [0, cache_len).  After kh_model_generate_until the records of positions n_prompt - 1 .. *n_words - 1
 * are the returned words' records; records past the stop are whatever the discarded steps left. */
int kh_model_set_logprobs(kh_model* m, int32_t top_n);
int kh_model_get_logprobs_setting(const kh_model* m, int32_t* top_n);
int kh_model_get_logprobs(kh_model* m, int32_t pos0, int32_t n, int32_t* h_token, float* h_lp, int32_t* h_top_ids,
                          float* h_top_lp);

/* The model's constraint (NULL = off, the default of every model): a token automaton (kh_fsm, above) inside the decode
 * loop - "answer with one of these strings", "emit text that matches this pattern".  The model holds one automaton
 * state s, a device word: kh_model_set_constraint sets it to `start`, so does the beginning of every kh_model_generate*
 * call, and kh_model_set_constraint_state sets it to any state.  At every SAMPLED position of kh_model_predict (fused and
 * unfused), kh_model_generate and kh_model_generate_until the logits outside row s become -inf ahead of the penalties,
 * the bias, the pick and the log-prob record, and the pick t moves s to next(s, t); forced (prompt) steps and is_prompt
 * predicts neither mask nor advance.  In every exec mode, with and without a sampler, penalties, a bias and log-probs, the
 * tokens, logits and records are bit for bit those of a host loop of kh_model_predict on an unconstrained model whose
 * logit bias is re-set at every step to -inf on the ids outside the row (see kh_fsm for why the order does not matter).
 * Records come from the masked logits: a banned token has log-prob -inf; kh_model_get_logits and kh_model_first_sample
 * report the masked logits.  The up to 16 steps kh_model_generate_until runs past a stop move s further: read the state
 * behind returned words with kh_fsm_walk.
 * While a constraint is set the step's last launch is k_sample_proc_fsm or, with log-probs on, k_sample_lp_fsm - the
 * tails of the processors with the mask pass in front and the transition behind the pick: launches_per_token is
 * unchanged, nothing returns to the host - and the screened classifier is not used; while off the model runs exactly
 * the launches it runs without this feature.  The automaton lives in device buffers behind one descriptor that the
 * captured launches read: a new automaton of any size needs no graph recapture.
 * kh_model_set_constraint copies the automaton; before any device call it makes kh_fsm_check's checks against
 * vocab_size and returns KH_ERR_INVALID_ARG where some row has every one of its tokens banned by a -inf entry of the
 * model's logit bias; kh_model_set_logit_bias refuses such a list the same way while a constraint is set.
 * Memory: beside the CSR arrays the model keeps one mask row of ceil(vocab_size / 32) words per state, on the device and
 * while the call runs on the host - 16 KiB per state at a vocabulary of 128256; an automaton whose mask table would
 * exceed KH_FSM_MAX_MASK_BYTES (256 MiB: 16743 states at that vocabulary) is refused with KH_ERR_UNSUPPORTED before any
 * device call.
 * kh_model_get_constraint_state synchronises the stream; both state calls return KH_ERR_UNSUPPORTED while the
 * constraint is off, the setter KH_ERR_RANGE for a state outside [0, n_states).
 * While a constraint is set kh_model_verify, kh_model_verify_as_set, kh_model_generate_lookup and
 * kh_model_generate_lookup_as_set return KH_ERR_UNSUPPORTED before any launch: they know no automaton, and
 * kh_model_verify_fsm / kh_model_generate_lookup_fsm ("Constrained lookup decode" below) are the calls that verify and
 * draft under it.  Every kh_model_seq_* call that launches (prefill, prefill_gemm, fork, step*) and
 * kh_model_generate_batch* refuse the same way (the slots have a constraint of their own).  kh_model_score and the
 * prefills are untouched.  Sequences in slots are constrained by kh_model_seq_set_constraint ("Per-sequence constrained decoding"
 * below), a setting of its own with one state per slot; one of the two is on at a time, and kh_model_set_constraint
 * returns KH_ERR_UNSUPPORTED while that one is. */
#define KH_FSM_MAX_MASK_BYTES (256 * 1024 * 1024)
int kh_model_set_constraint(kh_model* m, const kh_fsm* a);
int kh_model_get_constraint_state(kh_model* m, int32_t* state);
int kh_model_set_constraint_state(kh_model* m, int32_t state);

/* Sequence scoring: log P(token | prefix) at every FED position (perplexity, loglikelihood evaluation, reranking, the
 * "echo" log-probs of a prompt).  Feeds h_tokens[0..n) at positions pos0 .. pos0 + n - 1 - rows below pos0 must exist,
 * as for kh_model_prefill - and leaves what kh_model_prefill leaves: the K/V rows of those positions in every layer,
 * bit-identical to the token-by-token path, and the fed-token record.  The decode state, the sampler and the
 * processors are not touched.  In addition every position p of the range receives its log-prob record: token =
 * h_tokens[p - pos0 + 1], the token that FOLLOWED; logprob = the log-softmax of the RAW logits of position p at that
 * token; top_ids / top_logprobs = the first top_n tokens of the sampler's order - kh_logprobs_f32's semantics.  The
 * last position, pos0 + n - 1, has no successor in the call: token -1, logprob NaN, and a FILLED top list (the
 * next-token distribution).  Entries from top_n on are "none"; records outside the range are untouched.  Penalties,
 * bias, temperature, top-k and top-p never enter: these are the model's own probabilities of given text.  Read the
 * records with kh_model_get_logprobs (which synchronises).
 * The records are BIT-IDENTICAL to kh_logprobs_f32 on the logits n calls of kh_model_predict(.., KH_EXEC_FUSED) leave:
 * the logits come from k_pf_cls, the B-token twin of the decode classifier (8 tokens per pass over the weights for
 * fp32, 4 for int8 and wide fp32 models), the records from the routine behind kh_logprobs_f32.  Eager launches on the
 * model stream, no graph; a model that never calls this launches exactly what it launched before.
 * Before any launch: KH_ERR_INVALID_ARG for NULL pointers, n <= 0, pos0 < 0; KH_ERR_RANGE for pos0 + n > cache_len or
 * a token outside [0, vocab_size); KH_ERR_UNSUPPORTED while log-probs are off (kh_model_set_logprobs never called, or
 * -1) and for geometries outside the mirrored kernels (kh_model_prefill's limits; dim > 16 x the classifier's
 * workgroup width).  There is no token-by-token fallback and no MFMA variant. */
int kh_model_score(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0);

/* Speculative greedy decode: up to `width` consecutive positions verified by ONE pass over the weights (llama.cpp's
 * lookup / --draft, vLLM's ngram speculator, the "predicted outputs" of hosted APIs, in their exact greedy form).
 * kh_model_verify_width: tokens per verify pass of this model - 8 for fp32, 4 for int8 and wide fp32 models (the
 * batch of kh_model_prefill); KH_ERR_UNSUPPORTED for the geometries kh_model_score refuses.
 * kh_model_verify feeds h_tokens[0..n), 1 <= n <= width, at positions pos0 .. pos0 + n - 1 (rows below pos0 must exist)
 * in one full-depth pass: h_tokens[0] is the token known to be fed at pos0, h_tokens[1..n) are drafts.  h_next[i] = the
 * greedy pick - the first maximum of the RAW logits - at position pos0 + i given h_tokens[0..i]; *n_accept = a, the
 * largest value in [0, n - 1] with h_next[i] == h_tokens[i + 1] for all i < a.  The caller owns a + 1 new tokens,
 * h_next[0..a]; h_next[a + 1 .. n) are the picks behind a rejected draft (what the model would say after the wrong
 * token), of use to tests only.
 * The logits are those of kh_model_score's pass - bit-identical to n calls of kh_model_predict(.., KH_EXEC_FUSED) - and a
 * maximum involves no arithmetic, so h_next[0..a] are exactly the tokens a loop of predict calls returns: a rejected
 * draft costs time, never a different word.  Afterwards the K/V rows pos0 .. pos0 + a are bit-identical to the
 * token-by-token path; the rows above hold the rejected drafts' K/V and are stale - no step reads a row above its own
 * position, and the step that reaches one rewrites it first.  The decode state stands at (token h_next[a], position
 * pos0 + a + 1), as behind an advancing step: graph steps may follow at once.  The fed-token record holds h_tokens[0..a]
 * at pos0 .. pos0 + a and -1 above; the logits buffer of kh_model_get_logits is not written.  Sampler, processors and
 * log-prob settings are neither consulted nor touched.  Eager launches on the model stream (the pass, k_pf_cls,
 * k_spec_pick, k_spec_accept); synchronises.  A model that never calls this launches exactly what it launched before.
 * Before any launch: KH_ERR_INVALID_ARG for NULL pointers, n <= 0, pos0 < 0; KH_ERR_UNSUPPORTED for the geometries
 * kh_model_score refuses (the same predicate) and while kh_model_set_constraint is on - this call, kh_model_verify_as_set,
 * kh_model_generate_lookup and kh_model_generate_lookup_as_set refuse there, kh_model_verify_fsm and
 * kh_model_generate_lookup_fsm are the way; KH_ERR_RANGE for n > width, pos0 + n > cache_len or a token outside
 * [0, vocab_size). */
int kh_model_verify_width(const kh_model* m, int32_t* width);
int kh_model_verify(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0, int32_t* h_next, int32_t* n_accept);

/* Prompt-lookup generation.  kh_model_generate_until's contract in its graph form - the same prompt phase, the same
 * words, the same *n_words, the same stop rule, *h_elapsed_ms around the loop - with the sampled part driven by
 * draft + verify.  At position p with token t to feed, kh_lookup_draft proposes up to min(width - 1, total_steps - 1
 * - p) tokens from the sequence so far (prompt, then words) and the optional hint; a draft of d >= 1 tokens costs one
 * kh_model_verify pass of [t, draft] and advances by a + 1 positions; no draft runs min(miss_steps, remaining) steps on
 * the step graphs, exactly as kh_model_generate enqueues them (screened classifier included).  The host reads the words
 * behind either, so unlike generate there is one host round trip per pass or per miss_steps steps: on text without
 * repeats that is the price of asking (DESIGN 3.3f has the figures).  The first sampled position behind a prefill
 * takes a plain step with the full classifier, so kh_model_first_sample keeps working.  A stop token among the accepted
 * picks ends the call there.  stats (may be NULL): verify passes, tokens drafted, drafts accepted, sampled steps run
 * on the step graphs; without a stop, accepted + passes + plain_steps = total_steps - (n_prompt - 1).
 * kh_lookup_opts (NULL = all defaults): ngram_max 0 -> 4, ngram_min 0 -> 1, miss_steps 0 -> 8 (the measured price of
 * the round trip on text that never drafts: +2.3-2.5 % of the token loop at 1, +0.2-0.4 % at 8).
 * Before any launch: KH_ERR_INVALID_ARG as kh_model_generate_until, and for negative options, ngram_max < ngram_min,
 * miss_steps > 8 or a hint without a pointer; KH_ERR_RANGE as there, and for a hint token outside [0, vocab_size);
 * KH_ERR_UNSUPPORTED while a sampler (temperature > 0), a penalty, a bias entry or log-probs are on, and for the
 * geometries kh_model_verify refuses.  There is no silent fallback: kh_model_generate_until is the caller's to call. */
typedef struct kh_lookup_opts {
  int32_t ngram_max;   /* longest suffix searched, >= ngram_min; 0 -> 4 */
  int32_t ngram_min;   /* >= 1; 0 -> 1 */
  int32_t miss_steps;  /* decode steps run on the step graphs when nothing is drafted, 1..8; 0 -> 8 */
  const int32_t* h_hint; int32_t n_hint;  /* optional expected text ("predicted output"), token ids in range */
} kh_lookup_opts;
typedef struct kh_lookup_stats { int32_t passes, drafted, accepted, plain_steps; } kh_lookup_stats;
int kh_model_generate_lookup(kh_model* m, const int32_t* h_prompt, int32_t n_prompt, int32_t total_steps,
                             const int32_t* h_stop, int32_t n_stop, const kh_lookup_opts* opts,
                             int32_t* h_words, int32_t* n_words, float* h_elapsed_ms, kh_lookup_stats* stats);

/* The two calls above under the model's own settings: kh_model_set_sampling, _penalties, _logit_bias and _logprobs.
 * kh_model_verify_as_set is kh_model_verify's pass with h_next[i] = what a loop of kh_model_predict(.., KH_EXEC_FUSED)
 * under the same settings returns at position pos0 + i after feeding h_tokens[0..i]: row i of the pass's logits is
 * processed (penalties, bias) over the fed-token record up to pos0 + i, with this pass's own tokens at pos0 .. pos0 + i;
 * then the first maximum of the processed row; then, where temperature > 0, the draw with counter pos0 + i.  *n_accept
 * is defined as above, on these picks: a draft is accepted where it EQUALS the pick.  The draw depends on (seed,
 * position) and the logits only, and the logits are bit-identical to the token loop's, so h_next[0..a] are exactly that
 * loop's tokens - no rejection sampling, no tolerance; a wrong draft costs time, never a word.
 * Afterwards: K/V rows and decode state as behind kh_model_verify.  The fed-token record holds h_tokens[0..a] at pos0 ..
 * pos0 + a, h_next[a] at pos0 + a + 1 (the next step's penalty window reads it, as behind a batch-1 step) and -1 above.
 * With log-probs on, the records of pos0 .. pos0 + a are bit for bit those of the token loop - the pick, its log-prob
 * under the processed logits, the top-N - and those of pos0 + a + 1 .. pos0 + n - 1 are "none".  The logits buffer of
 * kh_model_get_logits is not written.  Launches: the pass, k_pf_cls, then k_spec_tail and k_spec_accept_set (behind
 * k_spec_hist with a penalty or bias on); with NOTHING on - greedy, neutral penalties, no bias, log-probs off - exactly
 * kh_model_verify's launches and results, and nothing more is allocated.  Error codes: kh_model_verify's.
 * kh_model_generate_lookup_as_set is kh_model_generate_lookup's loop and contract with that pass in place of
 * kh_model_verify's and without the greedy-only refusal (KH_ERR_UNSUPPORTED is left for the geometries): the words, the
 * log-prob records of the sampled positions and the K/V rows are kh_model_generate_until's under the same settings.  The
 * plain steps of a miss run on the step graphs with the tail the settings select. */
int kh_model_verify_as_set(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0, int32_t* h_next,
                           int32_t* n_accept);
int kh_model_generate_lookup_as_set(kh_model* m, const int32_t* h_prompt, int32_t n_prompt, int32_t total_steps,
                                    const int32_t* h_stop, int32_t n_stop, const kh_lookup_opts* opts,
                                    int32_t* h_words, int32_t* n_words, float* h_elapsed_ms, kh_lookup_stats* stats);
/* The drafter itself (host only, no device; csrc/kh_lookup.h), stateless.  For g = min(ngram_max, n_seq) down to
 * ngram_min, with key = the last g tokens of seq: (1) the EARLIEST j with hint[j .. j+g) == key and j + g < n_hint
 * drafts hint[j+g ..]; (2) else the MOST RECENT j with j + g <= n_seq - 1 and seq[j .. j+g) == key drafts seq[j+g ..];
 * the first g that matches wins, the draft is cut to cap, no match gives 0.  Returns the draft length written to
 * out[0 .. cap), or KH_ERR_INVALID_ARG (negative sizes or options, ngram_max < ngram_min, a size without a pointer);
 * ngram_max 0 -> 4, ngram_min 0 -> 1. */
int kh_lookup_draft(const int32_t* seq, int32_t n_seq, const int32_t* hint, int32_t n_hint,
                    int32_t ngram_max, int32_t ngram_min, int32_t* out, int32_t cap);
/* The drafter under a constraint (host only, stateless): the automaton drafts.  From `state` of `a`, until cap tokens
 * are out or neither rule adds one: (a) while the row of the current state has exactly ONE edge, that token is emitted
 * and the state moves along it - such a token is the pick under greedy and under every sampler, a raw logit of -inf or
 * NaN aside; *n_forced (may be NULL) counts them; (b) otherwise kh_lookup_draft's proposal for seq + the tokens out so
 * far, with the same hint and bounds and the remaining room, is cut to the longest prefix the automaton can follow from
 * the current state, and the state moves along it; nothing kept: stop.  Every drafted token is followable: a loop built
 * on this never feeds a token the mask would ban.  Returns the count, or before touching anything kh_fsm_check's codes
 * for the automaton (any vocabulary), KH_ERR_RANGE for a state outside [0, n_states), kh_lookup_draft's
 * KH_ERR_INVALID_ARG. */
int kh_lookup_draft_fsm(const kh_fsm* a, int32_t state, const int32_t* seq, int32_t n_seq, const int32_t* hint,
                        int32_t n_hint, int32_t ngram_max, int32_t ngram_min, int32_t* out, int32_t cap,
                        int32_t* n_forced);

/* Constrained lookup decode: the two _as_set calls under the model's constraint (kh_model_set_constraint).  A draft is
 * accepted only where it equals the pick, so the only automaton state row b of a pass can be accepted in is the walk of
 * the state word s over the fed tokens h_tokens[1..b] - known before the pass.  Row b is masked to the row of that state
 * ahead of the penalties, the bias, the pick and the record, as a batch-1 step masks.
 * kh_model_verify_fsm is kh_model_verify_as_set - its checks, its codes, its results - and runs while the constraint is
 * on: h_next[i] = what a loop of kh_model_predict(.., KH_EXEC_FUSED) under the same constraint and settings returns at
 * pos0 + i, from the state word as the call finds it; h_next[i] = -1 for every row behind a token h_tokens[k], 1 <= k
 * <= i, that the automaton cannot follow (such a row cannot be accepted: the pick ahead of it lies in a row that does
 * not hold the token).  Afterwards, beside what kh_model_verify_as_set leaves, the state word stands behind the last
 * owned pick h_next[a] - kh_fsm_walk from the state at entry over h_next[0..a] - exactly where a batch-1 step leaves
 * it: graph steps follow without a host-side reset.  Launches: k_spec_fsm_rows ahead of the pass (the state of every
 * row; k_spec_hist's duty is part of it), the pass, k_pf_cls, k_spec_tail_fsm, k_spec_accept_fsm - with every
 * combination of sampler, penalties, bias and log-probs, none included: the _as_set pass's launches plus at most one.
 * With the constraint off it IS kh_model_verify_as_set.  The per-sequence constraint is not read.
 * kh_model_generate_lookup_fsm is kh_model_generate_lookup_as_set with that pass and kh_lookup_draft_fsm as its
 * drafter: the host tracks the state - `start`, then along every sampled word it reads - and drafts from it, forced
 * tokens first; *n_forced (may be NULL) = drafted tokens that came from rule (a).  Words, *n_words, log-prob records
 * and K/V rows are kh_model_generate_until's under the same constraint and settings.  After the call the state word
 * stands behind the last pick the call owned, the stop token included where one ended it - unlike
 * kh_model_generate_until, whose up to 16 steps past a stop move the state further. */
int kh_model_verify_fsm(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0, int32_t* h_next,
                        int32_t* n_accept);
int kh_model_generate_lookup_fsm(kh_model* m, const int32_t* h_prompt, int32_t n_prompt, int32_t total_steps,
                                 const int32_t* h_stop, int32_t n_stop, const kh_lookup_opts* opts, int32_t* h_words,
                                 int32_t* n_words, float* h_elapsed_ms, kh_lookup_stats* stats, int32_t* n_forced);

/* Sequence slots: several independent sequences in one model, decoded `width` per pass over the weights (best-of-n,
 * self-consistency, a handful of prompts at once).  The reference runs one sequence per process (demo/main.cpp).
 * kh_model_seq_slots cuts the cache rows into n_slots equal regions: *slot_len (may be NULL) = cache_len / n_slots,
 * rounded down; slot s is rows [s * slot_len, (s + 1) * slot_len) of every layer, position p of its sequence is row
 * s * slot_len + p of the unchanged [layer, cache_len, kv_dim] layout (kh_model_read_kv reads it there).  One slot is
 * the state at creation.  Bookkeeping only: no kernel reads it, nothing is moved, and every batch-1 entry point keeps
 * addressing rows from 0 - slot 0 IS the batch-1 sequence's rows.  KH_ERR_INVALID_ARG unless 1 <= n_slots <= 64 and
 * slot_len >= 8.  kh_plan_seq_slots is the host-only twin.
 * kh_model_seq_width: lanes per pass - kh_model_verify_width's value, refused alike.
 * kh_model_seq_prefill: kh_model_prefill on the rows of `slot` - n tokens at positions pos0 .. of that sequence, rows
 * bit-identical to the token-by-token path; the fed tokens are recorded at the slot's entries of the fed-token
 * history (see kh_seq_opts below), the log-prob records are not written.  KH_ERR_RANGE for a slot outside [0, n_slots), pos0 + n > slot_len or a token outside the
 * vocabulary, otherwise kh_model_prefill's codes.  Synchronises (the record is uploaded from the caller's array).
 * kh_model_seq_fork copies K/V rows [0, n_rows) of every layer, and the n_rows entries of the fed-token history, from
 * src_slot to dst_slot on the model stream: with the
 * prefill call, how n samples share one prefilled prompt (they hold copies; nothing reads a shared prefix once).
 * KH_ERR_INVALID_ARG for src == dst or n_rows <= 0, KH_ERR_RANGE for a slot outside the partition or n_rows >
 * slot_len.  Does not synchronise.
 * kh_model_seq_step: ONE full-depth pass over n <= width lanes in distinct slots.  Lane i feeds h_tokens[i] at
 * position pos[i] of slot slots[i] (rows below pos[i] of that slot must exist); h_next[i] = the pick at that position:
 * the first maximum of the raw logits, or, with samplings != NULL and samplings[i].temperature > 0, kh_sample_f32's
 * draw with counter = pos[i] and the lane's own seed.  The logits are kh_model_score's - bit-identical to
 * kh_model_predict(.., KH_EXEC_FUSED) after the same history - so h_next[i] is exactly what a predict loop on a batch-1
 * model with kh_model_set_sampling(samplings[i]) returns, and row slot * slot_len + pos[i] of every layer is
 * bit-identical to that loop's row pos[i]; no other row is written.  The model's own sampler setting is not
 * consulted; the decode state, the logits buffer of kh_model_get_logits and the fed-token record are not touched.
 * Eager launches (k_seq_embed, per layer k_seq_qkv, k_seq_attn and the prefill pass's kernels, k_pf_cls, k_seq_pick);
 * synchronises.  Before any launch: KH_ERR_INVALID_ARG for NULL pointers, n <= 0, two lanes in one slot or invalid
 * sampling parameters; KH_ERR_UNSUPPORTED while a penalty, a bias entry or log-probs are on and for the geometries
 * kh_model_score refuses; KH_ERR_RANGE for n > width, a slot outside the partition, pos[i] outside [0, slot_len) or a
 * token outside the vocabulary.
 * kh_model_generate_batch: kh_model_generate_until for n_seq <= n_slots sequences at once, sequence s in slot s.
 * h_prompts holds the prompts back to back (n_prompt[s] tokens each); row s of h_words ([n_seq][words_stride],
 * words_stride >= every total_steps[s]) and n_words[s] are EXACTLY what kh_model_generate_until returns for prompt s,
 * total_steps[s], the stop list and kh_model_set_sampling(samplings[s]) (NULL: greedy) on a batch-1 model whose
 * prompt phase is bit-identical (KH_FLAG_PREFILL_EXACT, or fewer than 17 prompt tokens), and rows [0, n_words[s]) of
 * slot s are that model's rows.  The fed-only part of each prompt runs as kh_model_seq_prefill's passes, then passes of
 * up to `width` lanes: more live sequences than that take several passes per step, lanes grouped in slot order
 * (kh_plan_seq_batch is the grouping, host-only: out_lanes[pass * width + i] = the sequence in lane i or -1; first_pos[s]
 * = n_prompt[s] - 1; KH_ERR_RANGE with *n_passes set when cap_passes is too small).  Passes are enqueued eagerly, the
 * picks feed the next pass on the device; with a stop list the host reads the words of every 8 passes from pinned
 * memory while the next 8 are queued, and a sequence that stopped or reached its total leaves the lane table there -
 * what ran past a stop is discarded, as in kh_model_generate_until.  *h_elapsed_ms (may be NULL) spans the prompt passes
 * and the loop.  Leaves the decode state, the logits buffer and the records alone.  Before any launch:
 * KH_ERR_INVALID_ARG for NULL pointers, n_seq <= 0, a prompt or total of no tokens, words_stride below a total, invalid
 * sampling parameters; KH_ERR_RANGE for n_seq > n_slots, total_steps[s] > slot_len or a token outside the vocabulary;
 * KH_ERR_UNSUPPORTED as kh_model_seq_step.  There is no fallback to a token loop.
 * kh_model_generate_batch_from is the same call for prompts whose first n_cached[s] positions already sit in slot s
 * (kh_model_seq_prefill, kh_model_seq_fork; NULL = none): it feeds the rest and returns the words of the WHOLE prompt's
 * kh_model_generate_until.  KH_ERR_INVALID_ARG unless 0 <= n_cached[s] <= min(n_prompt[s] - 1, total_steps[s]).
 *
 * Slots of unequal length and a shared prompt prefix (n samples of one long prompt, one system prompt for several
 * users: ONE copy of the prompt's K/V rows).
 * kh_model_seq_slots_var: slot s owns h_len[s] consecutive rows, slot 0 from row 0 (it stays the batch-1 sequence's
 * rows), the others behind it without gaps.  KH_ERR_INVALID_ARG unless 1 <= n_slots <= 64, every h_len[s] >= 8 and
 * their sum <= cache_len.  kh_plan_seq_slots_var is the host-only twin (row0_out[s] = slot s's first row, may be NULL).
 * kh_model_seq_slots is the equal layout in the same tables; both calls reset every sharing relation.  Wherever the
 * text above says slot_len, read "the positions the slot holds" (its capacity), and row s * slot_len + p is
 * kh_model_seq_row(s, p).
 * kh_model_seq_share(src, dst, n_rows): from now on positions [0, n_rows) of dst ARE src's rows [0, n_rows); position
 * p >= n_rows of dst lives at dst's own row (p - n_rows), so dst holds n_rows + h_len[dst] positions.  Bookkeeping:
 * nothing is copied or launched, dst's previous content is discarded, n_rows == 0 detaches dst.  A sharer's words,
 * K/V rows and log-prob records are bit for bit those of a forked copy and of a batch-1 model: the attention of its
 * lanes is k_seq_attn's with the row of a timestep below n_rows taken from the parent (k_seq_attn_pfx, launched only
 * by a pass that has such a lane).  KH_ERR_INVALID_ARG for src == dst, n_rows < 0 or dst == 0 (slot 0 is what the
 * batch-1 entry points address: a parent, never a sharer); KH_ERR_RANGE for a slot outside the partition or n_rows >
 * h_len[src]; KH_ERR_UNSUPPORTED when src is itself a sharer (one level only) or dst has dependants.
 * While shared, a parent's rows below Pmax (the largest n_rows a dependant holds) are immutable: kh_model_seq_prefill,
 * kh_model_seq_step[_ex], kh_model_generate_batch* (by n_cached[s]) and kh_model_seq_set_history that would write
 * such a position, and kh_model_seq_fork INTO the parent, return KH_ERR_INVALID_ARG before any launch; the parent
 * keeps decoding at positions >= Pmax.  The batch-1 entry points ignore the bookkeeping, as ever: a caller that
 * shares slot 0's rows does not run them below Pmax.
 * A sharer is fed from its shared length on: kh_model_seq_prefill with pos0 below it, a lane position below it and
 * n_cached[s] below it are KH_ERR_INVALID_ARG; lanes of sharers and non-sharers mix in one pass.  It never writes
 * K/V, history or records at rows it does not own: kh_model_seq_get_logprobs returns "none" records below its shared
 * length, kh_model_generate_batch_ex resets and uploads only from there on.  Penalties on a sharer are refused
 * (KH_ERR_UNSUPPORTED from the _ex calls: its fed-token history would lie in two row ranges); sampling, logit bias and
 * log-probs work.  kh_model_seq_fork: the source may be a parent; KH_ERR_UNSUPPORTED if either side is a sharer.
 * kh_model_seq_row: the cache row that holds position pos of slot (the parent's below the shared length), for
 * kh_model_read_kv; KH_ERR_RANGE outside the slot's capacity. */
int kh_model_seq_slots(kh_model* m, int32_t n_slots, int32_t* slot_len);
int kh_model_seq_slots_var(kh_model* m, int32_t n_slots, const int32_t* h_len);
int kh_plan_seq_slots_var(int32_t cache_len, int32_t n_slots, const int32_t* h_len, int32_t* row0_out);
int kh_model_seq_share(kh_model* m, int32_t src_slot, int32_t dst_slot, int32_t n_rows);
int kh_model_seq_row(const kh_model* m, int32_t slot, int32_t pos, int32_t* row);
int kh_plan_seq_slots(int32_t cache_len, int32_t n_slots, int32_t* slot_len);
int kh_model_seq_width(const kh_model* m, int32_t* width);
int kh_model_seq_prefill(kh_model* m, int32_t slot, const int32_t* h_tokens, int32_t n, int32_t pos0);
int kh_model_seq_fork(kh_model* m, int32_t src_slot, int32_t dst_slot, int32_t n_rows);
int kh_model_seq_step(kh_model* m, int32_t n, const int32_t* slots, const int32_t* h_tokens, const int32_t* pos,
                      const kh_sampling* samplings, int32_t* h_next);
int kh_model_generate_batch(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                            const int32_t* total_steps, const kh_sampling* samplings, const int32_t* h_stop,
                            int32_t n_stop, int32_t* h_words, int32_t words_stride, int32_t* n_words,
                            float* h_elapsed_ms);
int kh_model_generate_batch_from(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                                 const int32_t* n_cached, const int32_t* total_steps, const kh_sampling* samplings,
                                 const int32_t* h_stop, int32_t n_stop, int32_t* h_words, int32_t words_stride,
                                 int32_t* n_words, float* h_elapsed_ms);
int kh_plan_seq_batch(int32_t n_seq, int32_t width, const int32_t* first_pos, const int32_t* total_steps,
                      int32_t* out_lanes, int32_t cap_passes, int32_t* n_passes);

/* Sequence slots with per-sequence penalties, logit bias and log-probs: the `_ex` forms of kh_model_seq_step and
 * kh_model_generate_batch_from.  Everything is stated per sequence IN THE CALL, as `samplings` already is: the model's
 * own kh_model_set_sampling / _penalties / _logit_bias / _logprobs values are NOT consulted by the _ex calls (the plain
 * entry points keep refusing while those are on).  kh_seq_opts, entry i for lane i (seq_step_ex) or sequence i
 * (generate_batch_ex); a NULL array is the neutral value for everyone:
 *   samplings       kh_sampling per sequence (temperature <= 0: greedy);
 *   penalties       kh_penalties per sequence, kh_model_set_penalties' semantics over the SLOT's fed-token history;
 *   n_bias          entries of sequence i's logit-bias list, 0 .. KH_SEQ_BIAS_MAX; the entries of sequence i follow
 *                   those of sequence i - 1 in bias_ids / bias (kh_model_set_logit_bias' semantics);
 *   logprobs_top_n  -1 off, else 0 .. KH_LOGPROBS_MAX_TOP for every sequence of the call: kh_model_set_logprobs'
 *                   records, kept per CACHE ROW - the record of position p of slot s is entry s * slot_len + p.
 * o == NULL, or everything in it neutral / off, is exactly the plain call: the same launches ending in k_seq_pick,
 * nothing allocated, no history or record written.  Otherwise the pass ends in k_seq_tail (csrc/kh_seq.h), one
 * workgroup per lane that chains the bit-exact cores of the batch-1 tail in its order - processing, maximum, greedy or
 * sampled pick (counter = position), record - so lane i's pick and record are EXACTLY those of a batch-1 model with
 * kh_model_set_penalties / _logit_bias / _sampling / _logprobs set to sequence i's values after the same history.
 * The fed-token history is addressed by cache row like K/V (position p of slot s is entry s * slot_len + p; slot 0's
 * is the batch-1 record).  It is written by kh_model_seq_prefill (the fed tokens; that call now synchronises), copied
 * by kh_model_seq_fork (n_rows entries), set by kh_model_seq_set_history (any int32; entries outside the vocabulary
 * count for nothing), and by the _ex calls while anything is on: seq_step_ex records each lane's fed token at its row
 * ahead of the pass - entries below it are whatever earlier calls left, the contract of the K/V rows - and
 * generate_batch_ex uploads every sequence's WHOLE prompt (also its n_cached part) to its slot's entries; k_seq_tail
 * records each pick as the token fed next, except behind a slot's last position.  generate_batch_ex also resets the
 * records of every sequence's fed-only positions to "none", as kh_model_generate_until does.
 * Tables (per-slot parameters and bias lists, KH_PF_BMAX x vocab_size counters, pinned staging) and the records are
 * allocated by the first call that needs them; a model that never asks allocates and launches nothing new.
 * Before any launch or copy: the plain calls' codes (KH_ERR_UNSUPPORTED only for the geometries kh_model_score
 * refuses), and KH_ERR_INVALID_ARG for invalid penalties (kh_model_set_penalties), a NaN or +inf bias, a duplicate id
 * within one sequence's list, a negative n_bias, n_bias without bias_ids / bias, logprobs_top_n outside
 * [-1, min(KH_LOGPROBS_MAX_TOP, vocab_size)]; KH_ERR_RANGE for a bias id outside the vocabulary or more than
 * KH_SEQ_BIAS_MAX entries for one sequence.
 * kh_model_seq_get_logprobs: kh_model_get_logprobs on the rows of `slot` - positions [pos0, pos0 + n) of its sequence;
 * h_top_ids / h_top_lp are [n][w] with w = the logprobs_top_n of the last _ex call that had log-probs on.
 * KH_ERR_UNSUPPORTED before any such call, KH_ERR_RANGE for a slot outside the partition or pos0 + n > slot_len.
 * kh_seq_rank (host only, stateless; the ONE definition of "best" of best-of-n): sequence s's log-probs are
 * h_lp[s * stride + p] for p in [first[s], n_words[s]); mean_lp[s] (may be NULL) = their sum in fp64, in index order,
 * over their number - NaN where the range is empty or an entry is NaN; order[0 .. n_seq) = the sequences by that mean,
 * descending, ties by ascending index, NaN last (by ascending index).  KH_ERR_INVALID_ARG for NULL pointers, n_seq <= 0,
 * first[s] < 0 or n_words[s] > stride. */
#define KH_SEQ_BIAS_MAX 64
typedef struct kh_seq_opts {
  const kh_sampling* samplings;   /* [n] or NULL: greedy */
  const kh_penalties* penalties;  /* [n] or NULL: neutral */
  const int32_t* n_bias;          /* [n] or NULL: none; entries of sequence i follow those of i - 1 in bias_ids / bias */
  const int32_t* bias_ids;
  const float* bias;
  int32_t logprobs_top_n;         /* -1 off, 0 .. KH_LOGPROBS_MAX_TOP */
} kh_seq_opts;
int kh_model_seq_step_ex(kh_model* m, int32_t n, const int32_t* slots, const int32_t* h_tokens, const int32_t* pos,
                         const kh_seq_opts* o, int32_t* h_next);
int kh_model_generate_batch_ex(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                               const int32_t* n_cached, const int32_t* total_steps, const kh_seq_opts* o,
                               const int32_t* h_stop, int32_t n_stop, int32_t* h_words, int32_t words_stride,
                               int32_t* n_words, float* h_elapsed_ms);
int kh_model_seq_set_history(kh_model* m, int32_t slot, int32_t pos0, const int32_t* h_tokens, int32_t n);
int kh_model_seq_get_logprobs(kh_model* m, int32_t slot, int32_t pos0, int32_t n, int32_t* h_token, float* h_lp,
                              int32_t* h_top_ids, float* h_top_lp);
int kh_seq_rank(int32_t n_seq, const float* h_lp, int32_t stride, const int32_t* first, const int32_t* n_words,
                int32_t* order, double* mean_lp);

/* Batched decode on the matrix cores: up to 64 sequences per weight pass (csrc/kh_seq_gemm.h).  The passes above share
 * a sweep of the weights between 8 (4) lanes on the VALU; the `_gemm` forms put the lanes on the MFMA token dimension
 * of kh_model_prefill_gemm's GEMMs - QKV with the lane's RoPE row and cache row, wo, the SwiGLU pair, w2 and the
 * classifier - and run the attention and the tail of the 8-lane pass once per group of 8 lanes.  Opt-in: no other
 * entry point routes here, and a model that never calls these allocates and launches nothing new.
 * Contract: kh_model_prefill_gemm's, NOT the bit-exact one of the calls above - fp32 round-off from another summation
 * order.  K/V rows and logits agree with the token-by-token path within the project's tolerances; every pick is an
 * exact function of the pass's own logits (kh_model_seq_gemm_logits): the first maximum, kh_sample_f32's draw with
 * counter = position, or the k_seq_tail chain; greedy words can differ from the batch-1 loop at near-ties only.
 * kh_model_seq_width_gemm: *width = 64, or KH_ERR_UNSUPPORTED: a geometry kh_model_seq_width or kh_model_prefill_gemm
 * refuses, or vocab_size % 16 != 0.  There is no fallback to the 8-lane pass.
 * kh_model_seq_step_gemm: kh_model_seq_step_ex with n <= 64 lanes; o == NULL: greedy and neutral.  The same refusals in
 * the same order, all before any launch, and the same rules for sharers and parents.  Eager launches (k_sg_embed, per
 * layer k_pg_rmsnorm, k_sg_gemm, k_sg_rope where the epilogue cannot rotate, k_seq_attn / k_seq_attn_pfx per group,
 * k_sg_gemm x 3 with k_pg_rmsnorm between; k_pg_rmsnorm, the classifier k_sg_gemm, k_seq_pick / k_seq_tail per group);
 * synchronises.
 * kh_model_generate_batch_gemm: kh_model_generate_batch_ex's parameters and host loop - lanes grouped in slot order
 * (kh_plan_seq_batch_wide is kh_plan_seq_batch for width <= 64), picks fed on the device, the stop check every 8
 * passes - at width 64 over the wide pass.  The fed-only part of every prompt runs as kh_model_seq_prefill's passes,
 * bit-exact as ever.
 * kh_model_seq_gemm_logits: the logits row [vocab_size] of lane `lane` of the last wide pass - after the tail's
 * in-place processing when the call had an option on; the near-tie probe of a caller that compares against the
 * batch-1 loop.  KH_ERR_UNSUPPORTED before any wide pass, KH_ERR_RANGE for a lane that pass did not have.
 * Synchronises. */
int kh_model_seq_width_gemm(const kh_model* m, int32_t* width);
int kh_model_seq_step_gemm(kh_model* m, int32_t n, const int32_t* slots, const int32_t* h_tokens, const int32_t* pos,
                           const kh_seq_opts* o, int32_t* h_next);
int kh_model_generate_batch_gemm(kh_model* m, int32_t n_seq, const int32_t* h_prompts, const int32_t* n_prompt,
                                 const int32_t* n_cached, const int32_t* total_steps, const kh_seq_opts* o,
                                 const int32_t* h_stop, int32_t n_stop, int32_t* h_words, int32_t words_stride,
                                 int32_t* n_words, float* h_elapsed_ms);
int kh_model_seq_gemm_logits(kh_model* m, int32_t lane, float* h_logits);
int kh_plan_seq_batch_wide(int32_t n_seq, int32_t width, const int32_t* first_pos, const int32_t* total_steps,
                           int32_t* out_lanes, int32_t cap_passes, int32_t* n_passes);

/* Per-sequence constrained decoding: the token automaton (kh_fsm, kh_model_set_constraint above) for sequences in slots -
 * a server whose users each bring a schema, n constrained samples of a best-of-n, structured output from the wide pass.
 * ONE automaton serves all slots and every slot has its own state word on the device.  Sequences with different
 * constraints share a UNION: the automata laid side by side with their states renumbered, each sequence at its own
 * start state (kuiperllama_amd.constraint.union builds it); KH_FSM_MAX_MASK_BYTES bounds the union as it bounds a
 * single automaton.  A slot whose state is -1 is unconstrained: its row is not masked, nothing advances.
 * At a lane's pass in kh_model_seq_step, _ex, _gemm and kh_model_generate_batch, _from, _ex, _gemm the row of the
 * slot's state masks the lane's logits ahead of the penalties, the bias, the pick and the record, and the slot's state
 * moves along the pick.  Fed-only positions (kh_model_seq_prefill, _prefill_gemm, the prompt part of generate_batch)
 * neither mask nor advance: the caller moves a state along forced text with kh_fsm_walk and the setter.
 * generate_batch* does not reset states; it samples from the state each slot holds.
 * Contract: for sequence s with sub-automaton A_s the words, log-prob records, K/V rows and masked logits are bit for
 * bit those of a batch-1 model under kh_model_set_constraint(A_s) with the same sampling, penalties, bias and log-probs
 * through kh_model_generate; for the wide pass its own contract: every pick is exact on the pass's own logits, and
 * kh_model_seq_gemm_logits returns the masked row.
 * Launches: while some lane of a call sits in a slot whose state is >= 0 every pass of the call ends in k_seq_tail_fsm
 * (csrc/kh_seq.h: k_seq_tail's twin with the automaton in its chain) for all its lanes, and a plain call runs as its
 * _ex form with neutral options (the plain calls' refusals about the MODEL's own penalties, bias and log-probs stay).
 * While no lane does - the constraint off, or every slot of the call at -1 - the calls launch exactly what they launch
 * without this feature.  "Sits in" is decided on the host, by the state last SET for the slot (the device only moves
 * a state >= 0 to another one).
 * kh_model_seq_set_constraint (NULL: off) copies the automaton and sets every slot's state to -1.  Before any device
 * call: kh_fsm_check's codes against vocab_size; KH_ERR_UNSUPPORTED while the model's batch-1 constraint is on
 * (kh_model_set_constraint refuses the same way while this one is) and for a mask table above KH_FSM_MAX_MASK_BYTES.  The
 * descriptor and the 64 state words (one per possible slot) are allocated once; a new automaton rewrites the descriptor.
 * kh_model_seq_set_constraint_state / _get_constraint_state: state -1 or [0, n_states) of slot [0, n_slots), else
 * KH_ERR_RANGE; KH_ERR_UNSUPPORTED while off.  The setter is stream-ordered; the getter synchronises.
 * kh_model_seq_slots / _slots_var reset every state to -1, as they reset sharing.  kh_model_seq_fork copies the source
 * slot's state to the destination on the stream (and the host's record of it): a fork in mid-generation continues
 * under the same constraint.  kh_model_seq_share leaves states alone; a sharer may be constrained.
 * A -inf bias may not leave a state without a token: a launching call returns KH_ERR_INVALID_ARG before any launch
 * where the -inf entries of a lane's bias list hold every token of a row the lane's slot COULD reach - decided
 * without a device read: the rows of the weakly connected component of the state last set for the slot.  Component
 * labels and the rows of at most KH_SEQ_BIAS_MAX edges (no other row can be emptied) are computed once per automaton.
 * kh_fsm_components / kh_fsm_bias_empties (host only, stateless) answer the two questions for any automaton:
 * labels[s] = the smallest state of the weakly connected component of s; *emptied = 1 where the -inf entries of the
 * list (n <= KH_SEQ_BIAS_MAX, else KH_ERR_RANGE) empty a row of state's component (state -1: never).  Both return
 * kh_fsm_check's KH_ERR_INVALID_ARG codes for a malformed automaton.
 * Speculative verify and lookup do not read this constraint: kh_model_verify*, kh_model_generate_lookup* and the two
 * _fsm calls run under it as they run without any.  Under the batch-1 constraint the four calls without _fsm refuse;
 * kh_model_verify_fsm and kh_model_generate_lookup_fsm are the way. */
int kh_model_seq_set_constraint(kh_model* m, const kh_fsm* a);
int kh_model_seq_set_constraint_state(kh_model* m, int32_t slot, int32_t state);
int kh_model_seq_get_constraint_state(kh_model* m, int32_t slot, int32_t* state);
int kh_fsm_components(const kh_fsm* a, int32_t* labels);
int kh_fsm_bias_empties(const kh_fsm* a, int32_t state, const int32_t* h_ids, const float* h_bias, int32_t n,
                        int32_t* emptied);

/* MFMA prompt prefill into sequence slots: many prompts per weight pass (csrc/kh_seq_prefill.h).  kh_model_seq_prefill
 * is the bit-exact VALU pass, 8 (fp32) or 4 (int8) tokens per sweep of the weights; kh_model_prefill_gemm writes rows
 * pos0 + t of the batch-1 layout only.  Here prompt SEGMENTS of several slots - segment i = n_tokens[i] tokens of the
 * concatenated h_tokens at positions pos0[i] .. of slot slots[i] - are packed into GEMM passes of 32 token tiles of 16
 * (a tile belongs to one segment; the padding tokens of a segment's last tile repeat its last valid token).  One prompt
 * into one slot is the one-segment call.  Opt-in: no other entry point routes here, and a model that never calls it
 * allocates and launches nothing new.  It reads the fp32 weights, also under KH_FLAG_W16.
 * Contract: kh_model_prefill_gemm's, NOT the bit-exact one of kh_model_seq_prefill - the call leaves K/V rows (and the
 * slots' fed-token record, as kh_model_seq_prefill) and no logits.  A lone segment leaves the very bytes
 * kh_model_prefill_gemm(tokens, n, pos0) leaves in rows [pos0, pos0 + n) of a batch-1 model below position 2048 (from
 * there on that call may share K/V fragments between query tiles, which regroups nothing but is not promised here).
 * kh_plan_seq_prefill_gemm: host only.  Segments are walked in call order; one that fits in what is left of the pass is
 * placed whole, else its first 16 x free tokens fill the pass and the rest continues in the next.  out_runs[r] = {pass,
 * segment, first token offset, count}; *n_runs = the runs there are (KH_ERR_RANGE when cap_runs holds fewer: call with
 * cap_runs 0 to size the array), *n_passes (optional) the passes.
 * kh_model_seq_prefill_gemm: every check before the first launch - per segment kh_model_seq_prefill's (the slot and its
 * capacity: KH_ERR_RANGE; the vocabulary: KH_ERR_RANGE; a sharer below its shared length or a parent's shared rows:
 * KH_ERR_INVALID_ARG); n_seq > 64: KH_ERR_RANGE; a slot twice, or a sharer together with its parent (feed the parent in
 * an earlier call): KH_ERR_INVALID_ARG; a geometry kh_model_prefill_gemm refuses, a head size other than 48 / 64 / 128,
 * or KH_PG_ATTN=0: KH_ERR_UNSUPPORTED - there is no fallback to the VALU pass or to the decode attention.  Launches per
 * pass: the embedding, per layer k_pg_rmsnorm, k_rg_gemm (QKV under the tile address), k_rg_rope where the epilogue
 * cannot rotate, k_rg_attn, k_pg_gemm x 3 with k_pg_rmsnorm between; the last layer stops behind its QKV GEMM.  The
 * KH_PG_SHAPE_* hooks apply, KH_PG_CHUNK does not.  Synchronises. */
int kh_plan_seq_prefill_gemm(int32_t n_seq, const int32_t* n_tokens, int32_t* out_runs, int32_t cap_runs,
                             int32_t* n_runs, int32_t* n_passes);
int kh_model_seq_prefill_gemm(kh_model* m, int32_t n_seq, const int32_t* slots, const int32_t* h_tokens,
                              const int32_t* n_tokens, const int32_t* pos0);

/* Launch plans, host-only (no device is touched; for tools and the CPU test-suite).
 * kh_plan_decode_shapes: {split, u, grid, wg} of the five GEMV kernels of a decode step (qkv, wo, ffn13, w2,
 * cls) for a geometry - what kh_model_create_* configures (env KH_SHAPE_* overrides included).
 * kh_plan_prefill_shape: {R, NT, ks, token slices, solo, kz, workgroups} of one GEMM of a T-token prefill
 * pass (epi 0 = QKV, 1 = residual GEMM wo / w2, 2 = SwiGLU pair; csrc/kh_model_gemm.hip::pg_shape). */
int kh_plan_decode_shapes(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size,
                          int32_t is_quant, int32_t* out20);
/* kh_plan_decode_ring: out4 = {ffn13 ring slots per wave, ffn13 workgroups, cls ring slots, cls workgroups} - which
 * int8 GEMVs of a decode step run on the LDS-DMA ring kernels (csrc/kh_fused_ring.h; 0 slots = the register-tile
 * kernel of kh_plan_decode_shapes) and with how many 256-thread workgroups.  Hook KH_RING=0 turns them off. */
int kh_plan_decode_ring(int32_t dim, int32_t hidden_dim, int32_t vocab_size, int32_t is_quant, int32_t group_size,
                        int32_t* out4);
/* kh_plan_w16: out2 = {bit mask of the decode launch classes that run on the 16-bit copy of KH_FLAG_W16 for this
 * geometry (kh_model_w16_info; 0: not applicable - int8, or dims that are no multiple of 4), bytes of the copy}. */
int kh_plan_w16(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t layer_num, int32_t is_quant,
                int64_t* out2);
/* kh_plan_q4: out2 = {bit mask of the decode launch classes that run on the 4-bit copy of KH_FLAG_Q4 for this geometry
 * (kh_model_q4_info; 0: not applicable - fp32, or dims that are no multiple of the group size - or no class adopted),
 * bytes of the copy (0: not applicable)}. */
int kh_plan_q4(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t layer_num, int32_t is_quant,
               int32_t group_size, int64_t* out2);
/* kh_plan_attention: the decode-attention geometry of kh_mha_decode_f32 / the fused step for a cache of seq_len rows:
 * out8 = {time splits per head, splits per KV group (0: no group path), workspace slot stride, first pos + 1 of the
 * group path, path taken at `pos` (0 per-head, 1 group), active splits at `pos`, timesteps per split at `pos`,
 * workgroups that own timesteps at `pos`} (KH_ATTN_TLONG, KH_ATTN_TS and KH_ATTN_WG honoured). */
/* kh_plan_gemm16: out2 = {bit mask of the launch classes whose GEMMs of the GEMM pass run on the bf16 matrix cores under
 * KH_FLAG_GEMM16 for this geometry (0: int8, or dims the GEMM prefill does not take): the adoption mask among the
 * classes whose contraction length (dim; w2: hidden_dim) is a multiple of 32, columns of a K block (32)}. */
int kh_plan_gemm16(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t is_quant, int64_t* out2);
/* kh_plan_gemm16_q8: out2 = {bit mask of the launch classes whose GEMMs of the GEMM pass run on the bf16 matrix cores
 * from the int8 image under KH_FLAG_GEMM16_Q8 for this geometry by default (0: fp32, a group size other than 64, or dims
 * the int8 GEMM prefill does not take), columns of a K block (64)}. */
int kh_plan_gemm16_q8(int32_t dim, int32_t hidden_dim, int32_t kv_dim, int32_t vocab_size, int32_t is_quant,
                      int32_t group_size, int64_t* out2);
int kh_plan_attention(int32_t head_num, int32_t kv_mul, int32_t head_size, int32_t seq_len, int32_t pos,
                      int32_t* out8);
/* kh_plan_attention_launch: ONE decode-attention launch over the tokens at positions pos[0 .. n) of that geometry (a
 * prefill slice, the lanes of a pass over sequence slots); n = 0: the position is a device word (a decode step).
 * out6 = {lanes per timestep G, heads per KV-group workgroup KVM (0 = per-head only) of the kernel instantiation,
 * grid.x, dynamic LDS bytes, per-head splits, group splits the grid carries} (same hooks). */
int kh_plan_attention_launch(int32_t head_num, int32_t kv_mul, int32_t head_size, int32_t seq_len,
                             const int32_t* pos, int32_t n, int32_t* out6);
int kh_plan_prefill_shape(int32_t epi, int32_t T, int32_t rows, int32_t K, int32_t is_quant,
                          int32_t r2_ok, int32_t* out7);

/* Tuning / test hooks.  Every hook the library honours (KH_SHAPE_<QKV|WO|FFN|W2|CLS>, KH_RING, KH_ATTN_WG, KH_ATTN_FENCED,
 * KH_ATTN_TLONG, KH_ATTN_DEFER (0 = never merge time splits in the wo kernel), KH_ATTN_DEFER_MAX (active splits up to
 * which it does), KH_PREFILL, KH_PG_<CHUNK|SHAPE_*|SOLO|KZ|ATTN|ATTN_QT|ROPE_FUSE|DEBUG>,
 * KH_SHAPE_DEBUG, KH_LAUNCH_LOG) lives in ONE process-wide key -> value table, seeded once from the KH_* variables of
 * the environment when the library is first used and changed afterwards only through kh_debug_set
 * (value NULL = unset).  No launch path reads the environment.  Hooks that shape a model (KH_SHAPE_*,
 * KH_ATTN_*) are read by kh_model_create_*; the others by the call they affect.  Keys must start with "KH_". */
int kh_debug_set(const char* key, const char* value);
const char* kh_debug_get(const char* key); /* NULL when unset */
int64_t kh_debug_list(char* buf, int64_t cap); /* '\n'-separated names; returns bytes needed */
/* Launch log.  While hook KH_LAUNCH_LOG is set (to anything but "0"), every fused decode-step, B-token prefill and
 * GEMM prefill launch adds the name of the kernel instantiation it launches ("k_gemv_res<true,3,6,2>",
 * "k_pg_gemm<false,2,8,1>", "k_pg_rope") to a process-wide set.  Decode attention adds "k_attn_decode<16,7>" (lanes
 * per timestep, heads per KV-group workgroup; 0 = per-head only) and one record of the launch's host-side variant,
 * "attn_launch<wg,ts_shift,defer,fenced,ntok>1?,group_grid?>" (workgroup width - hook KH_ATTN_WG = 256 | 512, which
 * kh_mha_decode_f32, kh_mha_decode_workspace_bytes and kh_plan_attention honour like kh_model_create_* -, log2 of the
 * split quantum, partials left to the wo kernel, fenced merge, several tokens per launch, grid carries the GQA group
 * path); a pass over sequence slots adds "k_seq_attn<16,2>" and "seq_attn_launch<wg,ts_shift,fenced,group_grid?>"
 * instead; the small-head kernel and kh_mha_f32's score kernel add "k_attn_generic" / "k_mha";
 * setting, resetting or unsetting the hook (kh_debug_set) empties it.  kh_debug_launch_log: the names,
 * '\n'-separated and sorted, into buf (always NUL-terminated); returns the bytes needed. */
int64_t kh_debug_launch_log(char* buf, int64_t cap);
/* Allocation accounting.  Every device and pinned-host buffer the library allocates is counted, process-wide.
 * out4 = {live buffers, live bytes, allocations since hook KH_ALLOC_FAIL was last set or cleared, failures injected
 * since then}.  Test hook KH_ALLOC_FAIL=k: the k-th such allocation after the hook was set answers
 * hipErrorOutOfMemory (2) without reaching the runtime; setting, resetting or unsetting it restarts the count.  (Not
 * counted: the weight arena and the mapped-on-demand KV cache.) */
int kh_debug_alloc_stats(int64_t* out4);

/* Duration (ms, HIP events on the model stream) of the prompt phase alone for n fed-only tokens:
 * KH_PREFILL_TOKEN = the reference's prompt phase, one forward pass per token (demo/main.cpp:20-22)
 * replayed from the decode hipGraph; KH_PREFILL_GEMV = kh_model_prefill's bit-identical B-token
 * kernels; KH_PREFILL_GEMM = the fp32-MFMA GEMM prefill.  Leaves the K/V rows of those positions. */
enum { KH_PREFILL_TOKEN = 0, KH_PREFILL_GEMV = 1, KH_PREFILL_GEMM = 2 };
int kh_model_time_prefill(kh_model* m, const int32_t* h_tokens, int32_t n, int32_t pos0,
                          int32_t mode, float* h_ms);

/* Average duration of ONE kernel class launched back to back (no event between launches, so
 * no event overhead in the figure): the kernel is captured for layers 0..L-1 `reps` times into
 * a hipGraph that is replayed between two HIP events on the model stream (cls / sample: `reps`
 * launches; a graph because a 3-4 us kernel outruns eager host enqueues); consecutive
 * launches read different layers' weights, so nothing is served from cache.  This is the
 * number bench.py's roofline uses and the one rocprofv3's per-kernel average must agree with.
 * Destroys the activation state and KV row `pos` (a later generate/predict resets both). */
int kh_model_profile_kernel(kh_model* m, int32_t kclass, int32_t pos, int32_t reps,
                            float* h_avg_us);

/* Latency of ONE decode step at position `pos` (per-token latency at pos 0/64/127):
 * the 1-step hipGraph replayed `reps` times with the device state reset to `pos` before each,
 * HIP events around each replay; h_us[reps] in microseconds.  KV rows below pos must exist and
 * a graph-mode generate of more than `pos` steps must have run on this model. */
int kh_model_time_step(kh_model* m, int32_t pos, int32_t reps, float* h_us);

/* Per-kernel-class timing of the fused step with HIP events (eager launches, one event
 * between every kernel).  n_steps decode steps starting at position start_pos (KV rows
 * below start_pos must already exist).  Writes avg microseconds per launch for each
 * class into h_avg_us[KH_NUM_KCLASS] and launches-per-step into h_count. */
enum {
  KH_K_QKV = 0, KH_K_ATTN = 1, KH_K_WO = 2, KH_K_FFN13 = 3, KH_K_W2 = 4, KH_K_CLS = 5,
  KH_K_SAMPLE = 6, KH_NUM_KCLASS = 7
};
int kh_model_profile_step(kh_model* m, int32_t start_pos, int32_t n_steps, float* h_avg_us,
                          int32_t* h_count);
const char* kh_kclass_name(int kclass);

/* ---- Tokenizer: SentencePiece BPE (host only) -------------------------------------------------
 * Replaces op::SpeEncodeLayer (kuiper/source/op/encode.cpp:10-57), the reference's wrapper over
 * the external sentencepiece library: Load -> create, Encode (+bos/eos like encode.cpp:37-44),
 * Decode, eos_id (is_sentence_ending, encode.cpp:48-51), GetPieceSize.  BPE model files with the
 * identity character map (Llama-2's tokenizer.model); anything else -> KH_ERR_UNSUPPORTED.
 * encode/decode return KH_ERR_RANGE when the output does not fit and store the needed size. */
typedef struct kh_spm kh_spm;
int kh_spm_create_from_file(const char* tokenizer_model_path, kh_spm** out);
int kh_spm_create_from_memory(const void* model_proto, int64_t nbytes, kh_spm** out);
void kh_spm_destroy(kh_spm* t);
int32_t kh_spm_vocab_size(const kh_spm* t);
int32_t kh_spm_bos_id(const kh_spm* t);
int32_t kh_spm_eos_id(const kh_spm* t);
int32_t kh_spm_unk_id(const kh_spm* t);
int kh_spm_encode(const kh_spm* t, const char* utf8, int64_t len, int32_t add_bos, int32_t add_eos,
                  int32_t* out_ids, int32_t cap, int32_t* n_ids);
int kh_spm_decode(const kh_spm* t, const int32_t* ids, int32_t n, char* out_utf8, int64_t cap,
                  int64_t* out_len);

/* ---- Tokenizer: byte-level BPE over a HuggingFace tokenizer.json (host only) ---------------------
 * Replaces op::BpeEncodeLayer (Llama-3.x) and op::QwenEncodeLayer (Qwen2.5)
 * (kuiper/source/op/encode.cpp:59-183) together with what they link: nlohmann::json, the vendored
 * tiktoken.h (kuiper/include/base/tiktoken.h:17-268), RE2 (the pre-split pattern PAT_STR,
 * encode.cpp:59-60), abseil and the vendored Unicode tables.  `flavor` selects which added_tokens
 * are BOS / EOS / second stop id (encode.cpp:97-103: <|begin_of_text|>, <|end_of_text|>, <|eot_id|>;
 * :170-176: <|im_start|>, <|im_end|>, <|endoftext|>); a name the file lacks is reported as -1.
 * KH_BPE_REF_SPACES reproduces the reference's " " -> "Ġ" replacement before encoding and its
 * inverse after decoding (encode.cpp:108-111, 124-126); without it the text is encoded as it is,
 * which is what HF `tokenizers` produces for the same pattern.  Model::encode adds BOS for Llama and
 * not for Qwen (model.cpp:158-165): that is the caller's add_bos.  Return codes as kh_spm_*. */
typedef struct kh_bpe kh_bpe;
enum { KH_BPE_LLAMA3 = 0, KH_BPE_QWEN2 = 1 };
enum { KH_BPE_REF_SPACES = 1 };
int kh_bpe_create_from_file(const char* tokenizer_json_path, int32_t flavor, kh_bpe** out);
int kh_bpe_create_from_memory(const void* tokenizer_json, int64_t nbytes, int32_t flavor, kh_bpe** out);
void kh_bpe_destroy(kh_bpe* t);
int32_t kh_bpe_vocab_size(const kh_bpe* t); /* |model.vocab| + |added_tokens| (encode.cpp:105) */
int32_t kh_bpe_bos_id(const kh_bpe* t);
int32_t kh_bpe_eos_id(const kh_bpe* t);
int32_t kh_bpe_stop_id(const kh_bpe* t, int32_t which); /* 0, 1: is_sentence_ending (encode.cpp:130-136) */
int kh_bpe_encode(const kh_bpe* t, const char* utf8, int64_t len, int32_t add_bos, int32_t add_eos,
                  int32_t flags, int32_t* out_ids, int32_t cap, int32_t* n_ids);
int kh_bpe_decode(const kh_bpe* t, const int32_t* ids, int32_t n, int32_t flags, char* out_utf8,
                  int64_t cap, int64_t* out_len);

#ifdef __cplusplus
}
#endif
#endif /* KUIPER_HIP_H */
