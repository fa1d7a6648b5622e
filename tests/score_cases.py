"""Shared cases of the sequence-scoring tests (tests/test_score.py, tests/test_score_gpu.py): the four synthetic
models, their token sequences, and the oracle side of the independent check - which needs no GPU, so the CPU suite
verifies that the chosen seed keeps enough positions checkable."""
import numpy as np

from kuiperllama_amd import binfmt

# (a) fp32 GQA shaped like the log-prob tests' flat model, with a cache long enough for the 300-token run; (b) int8,
# group 64 (untied classifier); (c) Qwen2: QKV bias, rotate-half RoPE; (d) fp32 wide enough that a prefill pass takes
# 4 tokens (8 vectors of dim floats need more than 80 KiB of LDS from dim 2560 on), one layer, small hidden size, an
# ODD vocabulary: the classifier's last pair is clamped and the rows of the logits scratch are padded.
SPECS = {
    "a": binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 320, True, binfmt.FAMILY_LLAMA, False, 64,
                          binfmt.ROPE_HALF, 500000.0, 1e-5, "score-a"),
    "b": binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 64, False, binfmt.FAMILY_LLAMA, True, 64,
                          binfmt.ROPE_HALF, 500000.0, 1e-5, "score-b"),
    "c": binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 64, True, binfmt.FAMILY_QWEN2, False, 64,
                          binfmt.ROPE_HALF, 1000000.0, 1e-6, "score-c"),
    "d": binfmt.ModelSpec(3072, 512, 1, 24, 8, 2051, 64, True, binfmt.FAMILY_LLAMA, False, 64,
                          binfmt.ROPE_HALF, 500000.0, 1e-5, "score-d"),
}
BATCH = {"a": 8, "b": 4, "c": 8, "d": 4}  # tokens per pass (csrc/kh_model_prefill.hip::prefill_batch)
SEEDS = {"a": 3, "b": 5, "c": 7, "d": 11}
LONG_N = 300  # model (a): positions cross 256, where decode attention starts its time splits


def tokens(name, n):
    """the model's token sequence: distinct ids where the vocabulary has enough, seeded by the model"""
    V = SPECS[name].vocab_size
    rng = np.random.default_rng(100 + SEEDS[name])
    return [int(t) for t in (rng.choice(V, n, replace=False) if n <= V else rng.integers(0, V, n))]


def lengths(name):
    """n of a score call: one token, a partial chunk, an exact chunk, a chunk and one token - the target of the first
    chunk's last token lives in the second - and three chunks"""
    B = BATCH[name]
    return [1, B - 1, B, B + 1, 2 * B + 3]


# ---- the independent check against the oracle (model (a), image made on the CPU so both sides read the same bytes)
ORACLE_SEED = 3
ORACLE_T = 24
ORACLE_TOP = 5
LOGIT_PARITY = 4e-5  # the project's fp32 logit parity bound (README, tests/test_model_gpu.py)


def oracle_image():
    return np.ascontiguousarray(binfmt.synth_image(SPECS["a"], seed=ORACLE_SEED, device="cpu").numpy())


def oracle_rows(O, img):
    """fp32 logits of the oracle at every position of the sequence, [ORACLE_T, V]"""
    om = O.OracleModel.from_spec(img, SPECS["a"])
    toks = tokens("a", ORACLE_T)
    rows = np.stack([np.array(om.forward(t, p), np.float32) for p, t in enumerate(toks)])
    om.close()
    return toks, rows


def oracle_expectation(rows):
    """-> (lp64 [T, V], order [T, ORACLE_TOP], checkable [T]): the fp64 log-softmax of the oracle's logits, its top
    list, and whether every boundary of that list - each gap between neighbours of the first ORACLE_TOP + 1 logits of
    the order - is wider than twice the parity bound, so that no logit within the bound can reorder it"""
    l = rows.astype(np.float64)
    m = l.max(axis=1, keepdims=True)
    lp = l - (m + np.log(np.exp(l - m).sum(axis=1, keepdims=True)))
    order = np.stack([np.lexsort((np.arange(l.shape[1]), -r)) for r in l])[:, :ORACLE_TOP + 1]
    top = np.take_along_axis(l, order, axis=1)
    checkable = (top[:, :-1] - top[:, 1:] > 2 * LOGIT_PARITY).all(axis=1)
    return lp, order[:, :ORACLE_TOP], checkable
