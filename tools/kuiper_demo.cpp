// kuiper_demo — command-line twin of the reference's demo/main.cpp / demo/main_qwen.cpp on top of
// the C-ABI (include/kuiper_hip.h).  The reference hard-codes tokenizer type, quantisation,
// device and prompt in the source; here they are flags.  The prompt is given as
// token ids (--prompt) or as text (--text) with the tokenizer file the reference takes as its second
// argument (main.cpp:56): a SentencePiece-BPE tokenizer.model (--tokenizer: BOS + encode like
// SpeEncodeLayer, stop at eos_id) or a HuggingFace tokenizer.json (--tokenizer-json: the byte-level BPE
// of the LLAMA3_SUPPORT / QWEN2_SUPPORT builds, encode.cpp:59-183 - BOS for Llama-3 and not for Qwen2,
// the reference's space -> "Ġ" replacement unless --hf-spaces, two stop ids); the decoded text is
// printed like main.cpp:43-45.
//
//   kuiper_demo model.bin [--family llama|qwen2] [--quant] [--rope interleaved|half]
//               [--theta 10000] [--eps 1e-5] [--steps 128] [--prompt 1,263] [--stop 2]
//               [--exec graph|fused|unfused] [--max-seq-len N] [--device 0]
//               [--tokenizer tokenizer.model | --tokenizer-json tokenizer.json [--hf-spaces]] [--text "a"]
//               [--exact-prefill] [--fenced-merge] [--w16] [--w16-f16] [--q4] [--gemm16] [--gemm16-q8]
//               [--temperature T] [--top-k K] [--top-p P] [--seed S]
//               [--repeat-penalty R] [--presence-penalty A] [--frequency-penalty B] [--repeat-last-n N]
//               [--logit-bias id=value]... [--logprobs N] [--score]
//               [--lookup [ngram_max]] [--lookup-as-set [ngram_max]] [--lookup-constrained [ngram_max]] [--hint id,id,...]
//               [--parallel N [--gemm-batch]] [--best-of N] [--share-prefix] [--gemm-prefill]
//
// --exact-prefill = KH_FLAG_PREFILL_EXACT: the prompt phase bit for bit the reference's one-token-per-pass prompt
// phase (demo/main.cpp:20-22); without it prompts of 17+ tokens run as fp32-MFMA GEMMs (tolerance parity, 8-10 x the
// prompt tokens/s).  --fenced-merge = KH_FLAG_ATTN_MERGE_FENCED.  The self-checks of kh_model_create_* are printed.
// --w16 = KH_FLAG_W16: decode a bf16-exact fp32 image from a 16-bit copy of its matrices, bit for bit (an image that is
// not bf16-exact decodes as without the flag); prints kh_model_w16_info, the pass class mask included.
// --w16-f16 = KH_FLAG_W16_F16: the same for an image that is bf16-exact OR fp16-exact (Llama-2's fp16 checkpoints); the
// format of the copy is printed.
// --q4 = KH_FLAG_Q4: decode an int8 image whose values all lie in [-8, 7] from a packed 4-bit copy of its matrices, bit
// for bit (any other image decodes as without the flag); prints kh_model_q4_info, the pass class mask included.
// --gemm16 = KH_FLAG_GEMM16 (with --w16 or --w16-f16 on a bf16-exact image): the GEMM prompt phase and the wide batch
// passes run on the bf16 matrix cores from the 16-bit copy, fp32-accurate (three exact bf16 terms per activation);
// prints kh_model_gemm16_info.  Inert - and says why - on any other model.
// --gemm16-q8 = KH_FLAG_GEMM16_Q8 (an int8 group-64 image): the GEMM prompt phase and the wide batch passes run on the bf16
// matrix cores from the int8 image itself, fp32-accurate; prints kh_model_gemm16_q8_info.  Inert - and says why - on any
// other model.
// --temperature / --top-k / --top-p / --seed: seeded sampling instead of the argmax (kh_model_set_sampling; the
// reference's demo is greedy, which stays the default).
// --repeat-penalty / --presence-penalty / --frequency-penalty over the last --repeat-last-n fed tokens (0: all of
// them; llama.cpp's flags of the same names) and --logit-bias id=value (repeatable; value -inf bans the token):
// kh_model_set_penalties / kh_model_set_logit_bias, applied to the logits ahead of the greedy or sampled pick.
// --logprobs N (0 .. 20): kh_model_set_logprobs; after the words and the timing, one line per generated token,
// "pos token lp | id:lp ..." with the N most likely tokens of that position (no token changes).
// --score (needs --logprobs N): scores the prompt instead of generating (kh_model_score): one line per prompt
// position in the same form - the token is the one that FOLLOWED, "-1 nan" at the last position, whose list is the
// next-token distribution - then "sum_logprob:" and "perplexity:" over the prompt's n - 1 predicted tokens.
// --lookup [ngram_max]: speculative greedy decode (kh_model_generate_lookup): the same words, several per pass over
// the weights wherever the text so far - or --hint id,id,..., the expected output - predicts the next tokens (n-grams
// of up to ngram_max tokens, default 4).  Greedy only.  A line "lookup: passes P drafted D accepted A plain_steps S"
// follows the words.
// --lookup-as-set [ngram_max]: the same loop under --temperature / --seed, the penalties, --logit-bias and --logprobs
// (kh_model_generate_lookup_as_set): a draft is accepted where it equals the pick the settings make, so the words and
// the log-prob lines are those of the same run without lookup.
// --lookup-constrained [ngram_max]: that loop under --choices as well (kh_model_generate_lookup_fsm): the automaton
// drafts - the tokens of a choice behind its branching prefix are forced - and the words are those of the same run
// without lookup.  The stats line gains "forced F", the drafted tokens that were forced ones.
// --parallel N: N samples of the one prompt, decoded together (kh_model_seq_slots / _seq_prefill / _seq_fork /
// kh_model_generate_batch_from): the cache is cut into N slots, the prompt is prefilled once and forked, the seeds are
// --seed, --seed + 1, ...; each sequence's ids are printed on a line of their own, then the aggregate "steps/s".
// Greedy without --temperature (N equal lines).  Penalties, bias and log-probs are refused, as by the library.
// --gemm-batch (beside --parallel): the samples decode as wide passes on the matrix cores, up to 64 per pass over the
// weights (kh_model_seq_width_gemm / kh_model_generate_batch_gemm): equal to the plain run to fp32 round-off, greedy ids
// can differ at near-ties.  Refused where the library refuses it; there is no fallback.
// --best-of N: --parallel's N samples (seeds --seed, --seed + 1, ...) through kh_model_generate_batch_ex, which takes
// the sampler, penalty, bias and --logprobs flags per sequence (the model's own settings are not consulted), ranked by
// kh_seq_rank on the mean log-prob of each sample's generated tokens: one line per sample, best first,
// "mean_logprob seed | id id ...", then the aggregate "steps/s".  --logprobs defaults to 0 here.
// --share-prefix (beside --parallel / --best-of): the samples read the prompt's rows from slot 0 instead of holding
// copies (kh_model_seq_slots_var / kh_model_seq_share): prompt + N x generated rows of cache, not N x (prompt +
// generated).  Same ids; penalties are refused on the sharing slots, as by the library.
// --gemm-prefill (beside --parallel / --best-of): the one prefill of the prompt into slot 0 is the GEMM pass on the
// matrix cores (kh_model_seq_prefill_gemm, one segment): its rows equal the plain run's to fp32 round-off.  Refused
// where the library refuses it; there is no fallback.
// Prints the generated ids and "steps/s" like demo/main.cpp:70-72.
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kuiper_hip.h"

// The slots of --parallel / --best-of: N equal ones whose samples hold copies of the prompt's rows (kh_model_seq_fork),
// or with --share-prefix one parent that owns all `steps` positions and N - 1 slots that read the prompt's `have` rows
// from it and own only what follows (kh_model_seq_slots_var, kh_model_seq_share).  *rows: rows of a sample's slot.
static int seq_layout(kh_model* m, int n, int have, int steps, bool share, int32_t* rows) {
  if (!share || have <= 0 || n < 2) return kh_model_seq_slots(m, n, rows);
  std::vector<int32_t> len((size_t)n, steps - have > 8 ? steps - have : 8);
  len[0] = steps > 8 ? steps : 8;
  *rows = len[1];
  return kh_model_seq_slots_var(m, n, len.data());
}
static int seq_attach(kh_model* m, int s, int have, bool share) {
  return share ? kh_model_seq_share(m, 0, s, have) : kh_model_seq_fork(m, 0, s, have);
}

// the prompt's fed-only part into slot 0: kh_model_seq_prefill, or with --gemm-prefill the one-segment GEMM call
static int seq_feed_prompt(kh_model* m, const std::vector<int32_t>& prompt, int have, bool gemm) {
  if (!gemm) return kh_model_seq_prefill(m, 0, prompt.data(), have, 0);
  const int32_t slot = 0, n = have, pos0 = 0;
  return kh_model_seq_prefill_gemm(m, 1, &slot, prompt.data(), &n, &pos0);
}

// --choices "id,id,..;id,id,..": the token automaton of "answer with one of these" (kh_fsm) - the trie of the
// sequences, each followed by `eos` into a sink whose only edge is `eos` onto itself (what the Python package's
// constraint.from_choices builds).  State 0 is the root.  The arrays back the returned kh_fsm.
struct ChoiceFsm {
  std::vector<int64_t> row_ptr;
  std::vector<int32_t> tokens, next;
  kh_fsm a{0, 0, nullptr, nullptr, nullptr};
};
static bool build_choices(const std::vector<std::vector<int32_t>>& seqs, int32_t eos, ChoiceFsm* out) {
  std::vector<std::map<int32_t, int32_t>> rows(1);
  std::vector<int32_t> accepting;
  for (const auto& seq : seqs) {
    int32_t s = 0;
    for (const int32_t t : seq) {
      if (t == eos) return false;
      auto it = rows[(size_t)s].find(t);
      if (it == rows[(size_t)s].end()) {
        rows.emplace_back();
        it = rows[(size_t)s].emplace(t, (int32_t)rows.size() - 1).first;
      }
      s = it->second;
    }
    accepting.push_back(s);
  }
  const int32_t sink = (int32_t)rows.size();
  rows.emplace_back();
  rows[(size_t)sink][eos] = sink;
  for (const int32_t s : accepting) rows[(size_t)s][eos] = sink;
  out->row_ptr.assign(1, 0);
  for (const auto& r : rows) {
    for (const auto& e : r) {
      out->tokens.push_back(e.first);
      out->next.push_back(e.second);
    }
    out->row_ptr.push_back((int64_t)out->tokens.size());
  }
  out->a = kh_fsm{(int32_t)rows.size(), 0, out->row_ptr.data(), out->tokens.data(), out->next.data()};
  return true;
}
// the sequence-level constraint of --parallel / --best-of: one automaton, every sample's slot at its start state
static int seq_constrain(kh_model* m, const kh_fsm* a, int n) {
  int rc = kh_model_seq_set_constraint(m, a);
  for (int s = 0; s < n && rc == KH_OK; ++s) rc = kh_model_seq_set_constraint_state(m, s, a->start);
  return rc;
}

static void usage() {
  std::fprintf(stderr,
               "usage: kuiper_demo model.bin [--family llama|qwen2] [--quant] [--rope interleaved|half]\n"
               "       [--theta F] [--eps F] [--steps N] [--prompt id,id,...] [--stop id,id] [--exec graph|fused|unfused]\n"
               "       [--max-seq-len N] [--device D] [--tokenizer tokenizer.model | --tokenizer-json tokenizer.json\n"
               "       [--hf-spaces]] [--text \"...\"] [--exact-prefill] [--fenced-merge] [--w16] [--w16-f16]\n"
               "       [--q4] [--gemm16] [--gemm16-q8]\n"
               "       [--temperature T] [--top-k K] [--top-p P] [--seed S]\n"
               "       [--repeat-penalty R] [--presence-penalty A] [--frequency-penalty B] [--repeat-last-n N]\n"
               "       [--logit-bias id=value]... [--logprobs N] [--score]\n"
               "       [--lookup [ngram_max]] [--lookup-as-set [ngram_max]] [--lookup-constrained [ngram_max]] [--hint id,id,...]\n"
               "       [--parallel N [--gemm-batch]] [--best-of N] [--share-prefix] [--gemm-prefill]\n"
               "       [--choices \"id,id,..;id,id,..\"]  (answer with one of these, then the first --stop id; also\n"
               "       beside --parallel / --best-of: every sample is constrained)\n");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    usage();
    return 2;
  }
  const char* path = argv[1];
  kh_model_opts o{KH_FAMILY_LLAMA, 0, KH_ROPE_INTERLEAVED, 10000.f, 1e-5f, 0, 0, 0};
  kh_sampling samp{0.f, 0, 1.f, 0};  // greedy unless --temperature > 0 (kh_model_set_sampling)
  kh_penalties pen{1.f, 0.f, 0.f, 0};  // off unless one of the penalty flags says more (kh_model_set_penalties)
  std::vector<int32_t> bias_ids;       // --logit-bias id=value (kh_model_set_logit_bias)
  std::vector<float> bias_vals;
  int steps = 128, exec = KH_EXEC_GRAPH;
  int logprobs = -1;  // --logprobs N (kh_model_set_logprobs)
  bool score = false;  // --score (kh_model_score)
  bool lookup = false;  // --lookup [ngram_max] (kh_model_generate_lookup)
  bool lookup_as_set = false;  // --lookup-as-set [ngram_max] (kh_model_generate_lookup_as_set)
  bool lookup_fsm = false;  // --lookup-constrained [ngram_max] (kh_model_generate_lookup_fsm)
  kh_lookup_opts lk{0, 0, 0, nullptr, 0};
  int parallel = 0;  // --parallel N (kh_model_generate_batch)
  bool gemm_batch = false;  // --gemm-batch (kh_model_generate_batch_gemm)
  bool gemm_prefill = false;  // --gemm-prefill (kh_model_seq_prefill_gemm)
  int best_of = 0;   // --best-of N (kh_model_generate_batch_ex, kh_seq_rank)
  bool share_prefix = false;  // --share-prefix: the samples read the prompt's rows from slot 0 (kh_model_seq_share)
  std::vector<std::vector<int32_t>> choices;  // --choices (kh_model_set_constraint / kh_model_seq_set_constraint)
  std::vector<int32_t> hint;  // --hint
  std::vector<int32_t> stop;  // is_sentence_ending ids (main.cpp:30): eos / <|eot_id|> / ...
  std::vector<int32_t> prompt{1, 263};  // BOS + "a": the reference demo's prompt (main.cpp:64)
  const char* tok_path = nullptr;
  const char* bpe_path = nullptr;
  int bpe_flags = KH_BPE_REF_SPACES;  // the reference's behaviour (encode.cpp:108-111)
  std::string text;
  bool have_text = false;
  for (int i = 2; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) {
        usage();
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "--family") o.family = std::string(next()) == "qwen2" ? KH_FAMILY_QWEN2 : KH_FAMILY_LLAMA;
    else if (a == "--quant") o.is_quant = 1;
    else if (a == "--rope") o.rope_mode = std::string(next()) == "half" ? KH_ROPE_HALF : KH_ROPE_INTERLEAVED;
    else if (a == "--theta") o.rope_theta = (float)std::atof(next());
    else if (a == "--eps") o.rms_eps = (float)std::atof(next());
    else if (a == "--steps") steps = std::atoi(next());
    else if (a == "--tokenizer") tok_path = next();
    else if (a == "--tokenizer-json") bpe_path = next();
    else if (a == "--hf-spaces") bpe_flags = 0;
    else if (a == "--exact-prefill") o.flags |= KH_FLAG_PREFILL_EXACT;
    else if (a == "--fenced-merge") o.flags |= KH_FLAG_ATTN_MERGE_FENCED;
    else if (a == "--w16") o.flags |= KH_FLAG_W16;
    else if (a == "--w16-f16") o.flags |= KH_FLAG_W16_F16;
    else if (a == "--q4") o.flags |= KH_FLAG_Q4;
    else if (a == "--gemm16") o.flags |= KH_FLAG_GEMM16;
    else if (a == "--gemm16-q8") o.flags |= KH_FLAG_GEMM16_Q8;
    else if (a == "--temperature") samp.temperature = (float)std::atof(next());
    else if (a == "--top-k") samp.top_k = std::atoi(next());
    else if (a == "--top-p") samp.top_p = (float)std::atof(next());
    else if (a == "--seed") samp.seed = std::strtoull(next(), nullptr, 0);
    else if (a == "--repeat-penalty") pen.repetition = (float)std::atof(next());
    else if (a == "--presence-penalty") pen.presence = (float)std::atof(next());
    else if (a == "--frequency-penalty") pen.frequency = (float)std::atof(next());
    else if (a == "--repeat-last-n") pen.last_n = std::atoi(next());
    else if (a == "--logprobs") logprobs = std::atoi(next());
    else if (a == "--score") score = true;
    else if (a == "--parallel") parallel = std::atoi(next());
    else if (a == "--gemm-batch") gemm_batch = true;
    else if (a == "--gemm-prefill") gemm_prefill = true;
    else if (a == "--best-of") best_of = std::atoi(next());
    else if (a == "--share-prefix") share_prefix = true;
    else if (a == "--lookup" || a == "--lookup-as-set" || a == "--lookup-constrained") {
      lookup = true;
      if (a == "--lookup-as-set") lookup_as_set = true;
      if (a == "--lookup-constrained") lookup_fsm = true;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') lk.ngram_max = std::atoi(argv[++i]);
    }
    else if (a == "--logit-bias") {
      const std::string e = next();
      const size_t eq = e.find('=');
      if (eq == std::string::npos || eq == 0 || eq + 1 >= e.size()) {
        usage();
        return 2;
      }
      bias_ids.push_back(std::atoi(e.substr(0, eq).c_str()));
      bias_vals.push_back(std::strtof(e.c_str() + eq + 1, nullptr));  // "-inf" parses
    }
    else if (a == "--choices") {
      const std::string e = next();
      choices.clear();
      for (size_t p = 0; p <= e.size();) {  // sequences between ';', ids between ','
        size_t q = e.find(';', p);
        if (q == std::string::npos) q = e.size();
        choices.emplace_back();
        for (size_t i = p; i < q;) {
          size_t j = e.find(',', i);
          if (j == std::string::npos || j > q) j = q;
          choices.back().push_back(std::atoi(e.substr(i, j - i).c_str()));
          i = j + 1;
        }
        p = q + 1;
      }
    }
    else if (a == "--text") {
      text = next();
      have_text = true;
    }
    else if (a == "--max-seq-len") o.max_seq_len = std::atoi(next());
    else if (a == "--device") o.device = std::atoi(next());
    else if (a == "--exec") {
      std::string e = next();
      exec = e == "unfused" ? KH_EXEC_UNFUSED : (e == "fused" ? KH_EXEC_FUSED : KH_EXEC_GRAPH);
    } else if (a == "--prompt" || a == "--stop" || a == "--hint") {
      std::vector<int32_t>& dst = a == "--prompt" ? prompt : (a == "--stop" ? stop : hint);
      dst.clear();
      std::string s = next();
      size_t p = 0;
      while (p < s.size()) {
        size_t q = s.find(',', p);
        if (q == std::string::npos) q = s.size();
        dst.push_back(std::atoi(s.substr(p, q - p).c_str()));
        p = q + 1;
      }
    } else {
      usage();
      return 2;
    }
  }
  if (gemm_prefill && parallel <= 0 && best_of <= 0) {  // it is the prefill of the slots of those two runs
    std::fprintf(stderr, "--gemm-prefill goes beside --parallel N or --best-of N\n");
    usage();
    return 2;
  }
  kh_spm* tok = nullptr;
  if (tok_path) {
    const int trc = kh_spm_create_from_file(tok_path, &tok);
    if (trc != KH_OK) {
      std::fprintf(stderr, "tokenizer load failed: %d (%s)\n", trc, kh_error_string(trc));
      return 1;
    }
    if (have_text) {  // model.cpp:158-165: BOS on for the Llama family; encode.cpp:37-41
      int32_t n = 0;
      prompt.assign(text.size() * 4 + 8, 0);
      if (kh_spm_encode(tok, text.data(), (int64_t)text.size(), 1, 0, prompt.data(), (int32_t)prompt.size(),
                        &n) != KH_OK) {
        std::fprintf(stderr, "encode failed\n");
        return 1;
      }
      prompt.resize((size_t)n);
    }
    if (stop.empty()) stop.push_back(kh_spm_eos_id(tok));  // is_sentence_ending, encode.cpp:48-51
  }
  kh_bpe* bpe = nullptr;
  if (bpe_path) {
    const int flavor = o.family == KH_FAMILY_QWEN2 ? KH_BPE_QWEN2 : KH_BPE_LLAMA3;
    const int trc = kh_bpe_create_from_file(bpe_path, flavor, &bpe);
    if (trc != KH_OK) {
      std::fprintf(stderr, "tokenizer.json load failed: %d (%s) - expected a byte-level BPE tokenizer.json "
                           "(Llama-3.x / Qwen2.5); SentencePiece models go to --tokenizer\n",
                   trc, kh_error_string(trc));
      return 1;
    }
    if (have_text) {  // model.cpp:158-165: BOS for Llama, none for Qwen
      int32_t n = 0;
      prompt.assign(text.size() * 2 + 8, 0);
      if (kh_bpe_encode(bpe, text.data(), (int64_t)text.size(), flavor == KH_BPE_LLAMA3, 0, bpe_flags,
                        prompt.data(), (int32_t)prompt.size(), &n) != KH_OK) {
        std::fprintf(stderr, "encode failed\n");
        return 1;
      }
      prompt.resize((size_t)n);
    }
    if (stop.empty()) {  // is_sentence_ending, encode.cpp:130-136
      stop.push_back(kh_bpe_stop_id(bpe, 0));
      stop.push_back(kh_bpe_stop_id(bpe, 1));
    }
  }
  if (have_text && !tok && !bpe) {
    std::fprintf(stderr, "--text needs --tokenizer (SentencePiece tokenizer.model) or --tokenizer-json "
                         "(HuggingFace byte-level BPE tokenizer.json)\n");
    return 2;
  }
  kh_model* m = nullptr;
  int rc = kh_model_create_from_file(path, &o, &m);
  if (rc != KH_OK) {
    std::fprintf(stderr, "The model init failed: %d (%s)\n", rc, kh_error_string(rc));
    return 1;
  }
  kh_config c;
  kh_model_get_config(m, &c);
  std::fprintf(stderr, "dim %d hidden %d layers %d heads %d kv_heads %d vocab %d seq_len %d%s\n", c.dim,
               c.hidden_dim, c.layer_num, c.head_num, c.kv_head_num, c.vocab_size, c.seq_len,
               c.is_quant ? " int8" : "");
  std::fprintf(stderr, "weights: %.2f GB uploaded in %.1f ms (%.1f GB/s)\n", c.weight_bytes / 1e9,
               kh_model_get_load_ms(m), c.weight_bytes / 1e6 / (kh_model_get_load_ms(m) + 1e-9));
  // kh_config: 0 n/a, 1 passed, -1 failed -> fallback in use, 2 (merge) fenced form requested
  std::fprintf(stderr, "self-checks: int8 ring kernels %d, attention split merge %d; prompt phase: %s\n", c.ring_selftest,
               c.attn_merge_selftest, (o.flags & KH_FLAG_PREFILL_EXACT) ? "exact (bit-identical to token-by-token)"
                                                                        : "GEMM for 17+ tokens (fp32 round-off)");
  if (o.flags & (KH_FLAG_W16 | KH_FLAG_W16_F16)) {
    int64_t w[8] = {0};
    kh_model_w16_info(m, w);
    // state: 0 not applicable (int8), 1 on, -1 the image is not exact in a format asked for, -2 self-check failed (both:
    // fp32 decode); format: of the live copy; w[7]: 1 + the first tensor that is not fp16-exact (0: not tried / none)
    // pass classes: whose B-token passes (prefill, score, verify, sequence slots) read the copy too (hook KH_W16_PASS)
    std::fprintf(stderr, "W16: state %lld, format %s, copy %.2f GB built in %.2f ms, launch classes 0x%llx, pass classes "
                 "0x%llx, first inexact tensor %lld (bf16) %lld (fp16)\n",
                 (long long)w[0], w[0] != 1 ? "none" : (w[6] ? "fp16" : "bf16"), (double)w[1] / 1e9, (double)w[2] / 1e3,
                 (unsigned long long)w[3], (unsigned long long)w[5], (long long)w[4], (long long)w[7] - 1);
  }
  if (o.flags & KH_FLAG_Q4) {
    int64_t w[8] = {0};
    kh_model_q4_info(m, w);
    // state: 0 not applicable (fp32), 1 on, -1 a value lies outside [-8, 7], -2 self-check failed (both: int8 decode)
    // pass classes: whose B-token passes (prefill, score, verify, sequence slots) read the copy too (hook KH_Q4_PASS)
    std::fprintf(stderr,
                 "Q4: state %lld, copy %.2f GB built in %.2f ms, launch classes 0x%llx, pass classes 0x%llx, first inexact "
                 "tensor %lld\n",
                 (long long)w[0], (double)w[1] / 1e9, (double)w[2] / 1e3, (unsigned long long)w[3], (unsigned long long)w[5],
                 (long long)w[4]);
  }
  if (o.flags & KH_FLAG_GEMM16) {
    int64_t w[8] = {0};
    kh_model_gemm16_info(m, w);
    // reason: 0 on, 1 flag not set, 2 no W16 flag, 3 int8, 4 image not bf16-exact, 5 fp16-format copy, 6 geometry,
    // 7 no class, 8 self-check failed
    std::fprintf(stderr, "GEMM16: state %lld, classes on the bf16 matrix cores 0x%llx (plan 0x%llx), reason %lld\n",
                 (long long)w[0], (unsigned long long)w[1], (unsigned long long)w[3], (long long)w[2]);
  }
  if (o.flags & KH_FLAG_GEMM16_Q8) {
    int64_t w[8] = {0};
    kh_model_gemm16_q8_info(m, w);
    // reason: 0 on, 1 flag not set, 2 fp32 model, 3 group size not 64, 4 geometry, 5 no class
    std::fprintf(stderr, "GEMM16_Q8: state %lld, classes on the bf16 matrix cores 0x%llx (plan 0x%llx), reason %lld\n",
                 (long long)w[0], (unsigned long long)w[1], (unsigned long long)w[3], (long long)w[2]);
  }
  rc = kh_model_set_sampling(m, &samp);
  if (rc != KH_OK) {
    std::fprintf(stderr, "invalid sampling parameters: %d (%s)\n", rc, kh_error_string(rc));
    kh_model_destroy(m);
    return 1;
  }
  if (samp.temperature > 0.f)
    std::fprintf(stderr, "sampling: temperature %g, top-k %d, top-p %g, seed %llu\n", samp.temperature, samp.top_k,
                 samp.top_p, (unsigned long long)samp.seed);
  rc = kh_model_set_penalties(m, &pen);
  if (rc == KH_OK) rc = kh_model_set_logit_bias(m, bias_ids.data(), bias_vals.data(), (int32_t)bias_ids.size());
  if (rc != KH_OK) {
    std::fprintf(stderr, "invalid penalties or logit bias: %d (%s)\n", rc, kh_error_string(rc));
    kh_model_destroy(m);
    return 1;
  }
  if (pen.repetition != 1.f || pen.presence != 0.f || pen.frequency != 0.f || !bias_ids.empty())
    std::fprintf(stderr, "logit processors: repeat %g, presence %g, frequency %g over the last %d tokens (0: all), %zu bias entries\n",
                 pen.repetition, pen.presence, pen.frequency, pen.last_n, bias_ids.size());
  if (logprobs != -1 && (rc = kh_model_set_logprobs(m, logprobs)) != KH_OK) {
    std::fprintf(stderr, "invalid --logprobs %d: %d (%s)\n", logprobs, rc, kh_error_string(rc));
    kh_model_destroy(m);
    return 1;
  }
  ChoiceFsm cfsm;
  if (!choices.empty()) {
    // the end of an answer is the first stop id (is_sentence_ending): the runs below stop there
    if (stop.empty() || !build_choices(choices, stop[0], &cfsm) || (rc = kh_fsm_check(&cfsm.a, c.vocab_size)) != KH_OK) {
      std::fprintf(stderr, "--choices needs --stop (or a tokenizer), ids of the vocabulary and no stop id inside a choice\n");
      kh_model_destroy(m);
      return 2;
    }
    if ((lookup && !lookup_fsm) || score) {
      std::fprintf(stderr, "--choices does not go with --lookup, --lookup-as-set or --score (--lookup-constrained is the one)\n");
      kh_model_destroy(m);
      return 2;
    }
    // --parallel / --best-of constrain their slots below (kh_model_seq_set_constraint); one of the two at a time
    if (parallel <= 0 && best_of <= 0 && (rc = kh_model_set_constraint(m, &cfsm.a)) != KH_OK) {
      std::fprintf(stderr, "--choices failed: %d (%s)\n", rc, kh_error_string(rc));
      kh_model_destroy(m);
      return 1;
    }
    std::fprintf(stderr, "constraint: %zu choices, %d states, ends on token %d\n", choices.size(), cfsm.a.n_states, stop[0]);
  }
  if (score) {
    if (logprobs < 0) {
      std::fprintf(stderr, "--score needs --logprobs N\n");
      kh_model_destroy(m);
      return 2;
    }
    const int cnt = (int)prompt.size();
    if ((rc = kh_model_score(m, prompt.data(), cnt, 0)) != KH_OK) {
      std::fprintf(stderr, "kh_model_score failed: %d (%s)\n", rc, kh_error_string(rc));
      kh_model_destroy(m);
      return 1;
    }
    std::vector<int32_t> tok_id((size_t)cnt), top_id((size_t)cnt * logprobs + 1);
    std::vector<float> lp((size_t)cnt), top_lp((size_t)cnt * logprobs + 1);
    if ((rc = kh_model_get_logprobs(m, 0, cnt, tok_id.data(), lp.data(), top_id.data(), top_lp.data())) != KH_OK) {
      std::fprintf(stderr, "kh_model_get_logprobs failed: %d (%s)\n", rc, kh_error_string(rc));
      kh_model_destroy(m);
      return 1;
    }
    double sum = 0.0;
    for (int i = 0; i < cnt; ++i) {
      if (tok_id[i] >= 0) sum += (double)lp[i];
      std::printf("%d %d %.6f |", i, tok_id[i], lp[i]);
      for (int k = 0; k < logprobs; ++k)
        std::printf(" %d:%.6f", top_id[(size_t)i * logprobs + k], top_lp[(size_t)i * logprobs + k]);
      std::printf("\n");
    }
    std::printf("sum_logprob:%.6f\nperplexity:%.6f\n", sum, cnt > 1 ? std::exp(-sum / (cnt - 1)) : std::nan(""));
    if (tok) kh_spm_destroy(tok);
    if (bpe) kh_bpe_destroy(bpe);
    kh_model_destroy(m);
    return 0;
  }
  if (best_of > 0) {
    // --parallel's samples with everything stated per sequence, then ranked
    const int N = best_of, top_n = logprobs < 0 ? 0 : logprobs;
    int32_t slot_len = 0;
    const int32_t np = (int32_t)prompt.size();
    const int32_t have = np - 1 < steps ? np - 1 : steps;
    const size_t stride = (size_t)(steps > 0 ? steps : 1);
    std::vector<int32_t> prompts, n_prompt((size_t)N, np), cached((size_t)N, have), totals((size_t)N, steps),
        n_out((size_t)N, 0), out((size_t)N * stride), nb((size_t)N, (int32_t)bias_ids.size()), ids, first((size_t)N, 0),
        order((size_t)N, 0);
    std::vector<float> vals, lp((size_t)N * stride, std::nanf(""));
    std::vector<double> mean((size_t)N, 0.0);
    std::vector<kh_sampling> samps((size_t)N, samp);
    std::vector<kh_penalties> pens((size_t)N, pen);
    for (int s = 0; s < N; ++s) {
      prompts.insert(prompts.end(), prompt.begin(), prompt.end());
      ids.insert(ids.end(), bias_ids.begin(), bias_ids.end());
      vals.insert(vals.end(), bias_vals.begin(), bias_vals.end());
      samps[(size_t)s].seed = samp.seed + (uint64_t)s;
    }
    const kh_seq_opts so{samps.data(), pens.data(), nb.data(), ids.data(), vals.data(), top_n};
    float ms = 0.f;
    std::printf("Generating...\n");
    const auto t0 = std::chrono::steady_clock::now();
    rc = seq_layout(m, N, have, steps, share_prefix, &slot_len);
    if (rc == KH_OK && !choices.empty()) rc = seq_constrain(m, &cfsm.a, N);
    if (rc == KH_OK && have > 0) rc = seq_feed_prompt(m, prompt, have, gemm_prefill);
    for (int s = 1; s < N && rc == KH_OK && have > 0; ++s) rc = seq_attach(m, s, have, share_prefix);
    if (rc == KH_OK)
      rc = kh_model_generate_batch_ex(m, N, prompts.data(), n_prompt.data(), cached.data(), totals.data(), &so,
                                      stop.data(), (int32_t)stop.size(), out.data(), steps, n_out.data(), &ms);
    const auto t1 = std::chrono::steady_clock::now();
    for (int s = 0; s < N && rc == KH_OK; ++s) {
      first[(size_t)s] = have < n_out[(size_t)s] ? have : n_out[(size_t)s];
      if (n_out[(size_t)s] > 0)
        rc = kh_model_seq_get_logprobs(m, s, 0, n_out[(size_t)s], nullptr, lp.data() + (size_t)s * stride, nullptr, nullptr);
    }
    if (rc == KH_OK)
      rc = kh_seq_rank(N, lp.data(), (int32_t)stride, first.data(), n_out.data(), order.data(), mean.data());
    if (rc != KH_OK) {
      std::fprintf(stderr, "--best-of %d failed: %d (%s)\n", N, rc, kh_error_string(rc));
      kh_model_destroy(m);
      return 1;
    }
    std::fprintf(stderr, "best-of: %d slots of %d rows\n", N, slot_len);
    long total = 0;
    for (int r = 0; r < N; ++r) {
      const size_t s = (size_t)order[(size_t)r];
      std::printf("%.6f %llu |", mean[s], (unsigned long long)samps[s].seed);
      for (int i = 0; i < n_out[s]; ++i) std::printf(" %d", out[s * stride + i]);
      std::printf("\n");
      total += n_out[s];
    }
    std::printf("steps/s:%lf\n", (double)total / std::chrono::duration<double>(t1 - t0).count());
    std::fprintf(stderr, "(device time of the passes: %.3f ms)\n", ms);
    if (tok) kh_spm_destroy(tok);
    if (bpe) kh_bpe_destroy(bpe);
    kh_model_destroy(m);
    return 0;
  }
  if (parallel > 0) {
    // N samples of the prompt: one prefill, N - 1 forks, then all sequences share every pass over the weights
    int32_t slot_len = 0, width = 0;
    const int32_t np = (int32_t)prompt.size();
    const int32_t have = np - 1 < steps ? np - 1 : steps;  // fed-only positions: prefilled once, forked
    std::vector<int32_t> prompts, n_prompt((size_t)parallel, np), cached((size_t)parallel, have),
        totals((size_t)parallel, steps), n_out((size_t)parallel, 0), out((size_t)parallel * (size_t)(steps > 0 ? steps : 1));
    std::vector<kh_sampling> samps((size_t)parallel, samp);
    for (int s = 0; s < parallel; ++s) {
      prompts.insert(prompts.end(), prompt.begin(), prompt.end());
      samps[(size_t)s].seed = samp.seed + (uint64_t)s;
    }
    float ms = 0.f;
    std::printf("Generating...\n");
    const auto t0 = std::chrono::steady_clock::now();
    rc = seq_layout(m, parallel, have, steps, share_prefix, &slot_len);
    if (rc == KH_OK && !choices.empty()) rc = seq_constrain(m, &cfsm.a, parallel);
    if (rc == KH_OK) rc = gemm_batch ? kh_model_seq_width_gemm(m, &width) : kh_model_seq_width(m, &width);
    if (rc == KH_OK && have > 0) rc = seq_feed_prompt(m, prompt, have, gemm_prefill);
    for (int s = 1; s < parallel && rc == KH_OK && have > 0; ++s) rc = seq_attach(m, s, have, share_prefix);
    if (rc == KH_OK && gemm_batch) {
      kh_seq_opts so{};
      so.samplings = samps.data();
      so.logprobs_top_n = -1;
      rc = kh_model_generate_batch_gemm(m, parallel, prompts.data(), n_prompt.data(), cached.data(), totals.data(), &so,
                                        stop.data(), (int32_t)stop.size(), out.data(), steps, n_out.data(), &ms);
    } else if (rc == KH_OK) {
      rc = kh_model_generate_batch_from(m, parallel, prompts.data(), n_prompt.data(), cached.data(), totals.data(),
                                        samps.data(), stop.data(), (int32_t)stop.size(), out.data(), steps,
                                        n_out.data(), &ms);
    }
    const auto t1 = std::chrono::steady_clock::now();
    if (rc != KH_OK) {
      std::fprintf(stderr, "--parallel %d failed: %d (%s)\n", parallel, rc, kh_error_string(rc));
      kh_model_destroy(m);
      return 1;
    }
    std::fprintf(stderr, "parallel: %d slots of %d rows, %d lanes per pass\n", parallel, slot_len, width);
    long total = 0;
    for (int s = 0; s < parallel; ++s) {
      for (int i = 0; i < n_out[(size_t)s]; ++i) std::printf("%d ", out[(size_t)s * steps + i]);
      std::printf("\n");
      total += n_out[(size_t)s];
    }
    std::printf("steps/s:%lf\n", (double)total / std::chrono::duration<double>(t1 - t0).count());
    std::fprintf(stderr, "(device time of the passes: %.3f ms)\n", ms);
    if (tok) kh_spm_destroy(tok);
    if (bpe) kh_bpe_destroy(bpe);
    kh_model_destroy(m);
    return 0;
  }
  std::vector<int32_t> words((size_t)steps);
  int32_t n = 0;
  float gpu_ms = 0.f;
  std::printf("Generating...\n");
  const auto t0 = std::chrono::steady_clock::now();  // timer excludes init (main.cpp:66)
  kh_lookup_stats lks{0, 0, 0, 0};
  int32_t lk_forced = 0;
  if (lookup) {
    lk.h_hint = hint.empty() ? nullptr : hint.data();
    lk.n_hint = (int32_t)hint.size();
  }
  if (lookup_fsm) {
    rc = kh_model_generate_lookup_fsm(m, prompt.data(), (int32_t)prompt.size(), steps, stop.data(), (int32_t)stop.size(),
                                      &lk, words.data(), &n, &gpu_ms, &lks, &lk_forced);
  } else if (lookup) {
    rc = (lookup_as_set ? kh_model_generate_lookup_as_set : kh_model_generate_lookup)(
        m, prompt.data(), (int32_t)prompt.size(), steps, stop.data(), (int32_t)stop.size(), &lk, words.data(), &n,
        &gpu_ms, &lks);
  } else {
    rc = kh_model_generate_until(m, prompt.data(), (int32_t)prompt.size(), steps, exec, stop.data(),
                                 (int32_t)stop.size(), words.data(), &n, &gpu_ms);
  }
  const auto t1 = std::chrono::steady_clock::now();
  if (rc != KH_OK) {
    std::fprintf(stderr, "generate failed: %d (%s)\n", rc, kh_error_string(rc));
    kh_model_destroy(m);
    return 1;
  }
  const int n_gen = n;  // positions 0 .. n_gen - 1 produced words; those from prompt.size() - 1 on were sampled
  if (o.family == KH_FAMILY_QWEN2 && !prompt.empty()) {
    // demo/main_qwen.cpp:12,18 seeds `next` with the first prompt token and pushes it into `words`
    // before the loop (main.cpp starts from next = -1): the Qwen demo's output begins with it
    words.insert(words.begin(), prompt[0]);
    ++n;
  }
  if (tok) {  // main.cpp:43-45: printf("%s ", model.decode(words))
    std::vector<char> buf((size_t)n * 16 + 16);
    int64_t len = 0;
    if (kh_spm_decode(tok, words.data(), n, buf.data(), (int64_t)buf.size(), &len) == KH_OK)
      std::printf("%.*s \n", (int)len, buf.data());
    kh_spm_destroy(tok);
  }
  if (bpe) {
    std::vector<char> buf((size_t)n * 32 + 16);
    int64_t len = 0;
    if (kh_bpe_decode(bpe, words.data(), n, bpe_flags, buf.data(), (int64_t)buf.size(), &len) == KH_OK)
      std::printf("%.*s \n", (int)len, buf.data());
    kh_bpe_destroy(bpe);
  }
  for (int i = 0; i < n; ++i) std::printf("%d ", words[i]);
  const double dur = std::chrono::duration<double>(t1 - t0).count();
  const int steps_done = n - (o.family == KH_FAMILY_QWEN2 && !prompt.empty() ? 1 : 0);
  if (lookup)
    std::printf("\nlookup: passes %d drafted %d accepted %d plain_steps %d", lks.passes, lks.drafted, lks.accepted,
                lks.plain_steps);
  if (lookup_fsm) std::printf(" forced %d", lk_forced);
  std::printf("\nsteps/s:%lf\n", (double)steps_done / dur);
  if (o.family == KH_FAMILY_QWEN2) std::printf("\nsteps:%d\n\nduration:%lf\n", steps_done, dur);  // main_qwen.cpp:73-74
  const int p0 = (int)prompt.size() - 1;
  if (logprobs >= 0 && n_gen > p0) {
    const int cnt = n_gen - p0;
    std::vector<int32_t> tok_id((size_t)cnt), top_id((size_t)cnt * logprobs + 1);
    std::vector<float> lp((size_t)cnt), top_lp((size_t)cnt * logprobs + 1);
    rc = kh_model_get_logprobs(m, p0, cnt, tok_id.data(), lp.data(), top_id.data(), top_lp.data());
    if (rc != KH_OK) {
      std::fprintf(stderr, "kh_model_get_logprobs failed: %d (%s)\n", rc, kh_error_string(rc));
      kh_model_destroy(m);
      return 1;
    }
    for (int i = 0; i < cnt; ++i) {
      std::printf("%d %d %.6f |", p0 + i, tok_id[i], lp[i]);
      for (int k = 0; k < logprobs; ++k)
        std::printf(" %d:%.6f", top_id[(size_t)i * logprobs + k], top_lp[(size_t)i * logprobs + k]);
      std::printf("\n");
    }
  }
  std::fprintf(stderr, "(device time of the step loop: %.3f ms)\n", gpu_ms);
  kh_model_destroy(m);
  return 0;
}
