"""Shared by test_seq_gemm.py (CPU) and test_seq_gemm_gpu.py: the geometries, the slot layout and the batched-loop
case of the wide sequence pass (csrc/kh_seq_gemm.h).  The images are synthesised on the CPU (binfmt.synth_image,
device "cpu") so that the CPU suite can check, with the oracle, the very weights the GPU suite runs."""
import numpy as np

from kuiperllama_amd import binfmt

LOGIT_ATOL_F32 = 2e-5  # test_model_gpu.py: LOGIT_ATOL_F32 / LOGIT_ATOL_Q8 / KV_ATOL_GEMM (int8: 4x)
LOGIT_ATOL_Q8 = 5e-5
KV_ATOL_GEMM = 5e-6
CACHE = 2048
LONG, SHORT = 300, 8
LENS = [LONG] * 3 + [SHORT] * 61  # seq_slots_var: three slots of 300 rows and 61 of 8

L, Q2 = binfmt.FAMILY_LLAMA, binfmt.FAMILY_QWEN2
HALF, INTER = binfmt.ROPE_HALF, binfmt.ROPE_INTERLEAVED
# 2 layers, as the tiny specs of test_model_gpu.py; vocabularies are multiples of 16
SPECS = {
    # interleaved RoPE with MHA (head size 128): the pair epilogue
    "mha-inter": binfmt.ModelSpec(512, 1408, 2, 4, 4, 512, CACHE, False, L, False, 64, INTER, 10000.0, 1e-5, "sg-mha"),
    # half-mode GQA, head size 64: the fused tile RoPE (R = 2 tiles), tied classifier
    "gqa-half": binfmt.ModelSpec(512, 1536, 2, 8, 2, 640, CACHE, True, L, False, 64, HALF, 500000.0, 1e-5, "sg-gqa"),
    # half mode with head size 48 (no multiple of 32): the epilogue cannot rotate, k_sg_rope follows
    "half-hs48": binfmt.ModelSpec(384, 1024, 2, 8, 2, 512, CACHE, False, L, False, 64, HALF, 10000.0, 1e-5, "sg-hs48"),
    # Qwen2 bias, kv_mul 7
    "qwen-bias": binfmt.ModelSpec(448, 1216, 2, 7, 1, 704, CACHE, True, Q2, False, 64, HALF, 1000000.0, 1e-6,
                                  "sg-qwen"),
    # int8 group 64
    "int8": binfmt.ModelSpec(512, 1408, 2, 4, 4, 512, CACHE, False, L, True, 64, INTER, 10000.0, 1e-5, "sg-int8"),
}
# refused: a vocabulary that is no multiple of 16; a head size <= 32
ODD_VOCAB = binfmt.ModelSpec(512, 1408, 2, 4, 4, 500, 64, False, L, False, 64, INTER, 10000.0, 1e-5, "sg-v500")
SMALL_HEAD = binfmt.ModelSpec(256, 704, 2, 8, 8, 512, 64, False, L, False, 64, INTER, 10000.0, 1e-5, "sg-hs32")
SEED = 4242


def logit_atol(spec):
    return LOGIT_ATOL_Q8 if spec.quant else LOGIT_ATOL_F32


def kv_atol(spec):
    return KV_ATOL_GEMM * (4 if spec.quant else 1)


_IMG = {}


def host_image(spec, seed=SEED, wander=False):
    """the image as host bytes (numpy uint8); wander: a zero-mean final norm (binfmt.synth_image) so that a tied
    classifier's greedy text is no fixed point"""
    key = (spec.name, spec.seq_len, seed, wander)
    if key not in _IMG:
        img = binfmt.synth_image(spec, seed=seed, device="cpu", final_norm_std=1.0 if wander else None)
        _IMG[key] = np.ascontiguousarray(img.numpy())
    return _IMG[key]


def lane_pos(slot):
    """the position a pass feeds in `slot`: 255 / 256 / 257 in the long slots (below, on and behind the attention
    time-split quantum), 0 .. 7 in the short ones (slot 3 and every eighth after it at position 0)"""
    return 255 + slot if slot < 3 else (slot - 3) % SHORT


def texts(spec, seed=7):
    """per slot the tokens of positions 0 .. lane_pos(slot)"""
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, spec.vocab_size, lane_pos(s) + 1)] for s in range(len(LENS))]


def plan_twin(first_pos, totals, width):
    """kh_seq_plan.h: kh_seq_next_pass, in Python: rounds walk the sequences in slot order, a pass takes the next up to
    `width` live ones from the cursor on and never wraps"""
    pos, passes, cursor = list(first_pos), [], 0
    while True:
        lanes = []
        for _ in range(2):
            s = cursor
            while s < len(pos) and len(lanes) < width:
                if pos[s] < totals[s]:
                    lanes.append(s)
                s += 1
            cursor = 0 if s >= len(pos) else s
            if lanes:
                break
        if not lanes:
            return passes
        for s in lanes:
            pos[s] += 1
        passes.append(lanes)


# ---- the batched loop: 20 sequences (a full tile of 16 and a partial one), prompts of 1 .. 12 tokens, unequal totals
LOOP_SPEC = "gqa-half"
LOOP_SEED = 31
LOOP_N = 20


def loop_case(spec):
    rng = np.random.default_rng(LOOP_SEED)
    prompts = [[int(t) for t in rng.integers(0, spec.vocab_size, 1 + (5 * s) % 12)] for s in range(LOOP_N)]
    totals = [len(p) - 1 + 6 + (7 * s) % 13 for s, p in enumerate(prompts)]
    return prompts, totals


def greedy_loop(step, prompt, total, stop, atol):
    """generate_until's loop over step(token, pos) -> logits: (words, near, clean) with near = the index of the first
    word whose pick had a top-1 minus top-2 gap below 4 * atol (len(words) if none, and then clean): the words from
    there on, and where the sequence ends, need not agree"""
    words, near = [], None
    for p in range(total):
        lg = step(prompt[p] if p < len(prompt) else words[p - 1], p)
        if p + 1 < len(prompt):
            words.append(prompt[p + 1])
            continue
        top2 = np.sort(lg)[-2:]
        if near is None and top2[1] - top2[0] < 4 * atol:
            near = len(words)
        w = int(np.argmax(lg))
        if w in stop:
            break
        words.append(w)
    return words, len(words) if near is None else near, near is None
