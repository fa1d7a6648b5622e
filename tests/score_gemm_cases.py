"""Shared by test_score_gemm.py (CPU) and test_score_gemm_gpu.py: the models, the token strings of every run and the
near-tie rule.  Images are synthesised on the CPU so that the oracle reads the bytes the GPU runs."""
import numpy as np

import score_cases as S
import seq_gemm_cases as G
from kuiperllama_amd import binfmt

TOP = 5
N = 64      # one pass, the whole 64-token tile
CHUNK = 16  # hook KH_PG_CHUNK: a pass boundary behind 16 tokens; CHUNK + 3 tokens cross it
LONG = 65   # "q8": the int8 128-token tile (model (b)'s cache ends at 64 rows)
# model (d) of score_cases has an odd vocabulary: it is the refusal
CASES = {"a": (S.SPECS["a"], 3), "b": (S.SPECS["b"], 5), "c": (S.SPECS["c"], 7), "q8": (G.SPECS["int8"], G.SEED)}


def image(name):
    spec, seed = CASES[name]
    return np.ascontiguousarray(binfmt.synth_image(spec, seed=seed, device="cpu").numpy())


def runs(name):
    """[(KH_PG_CHUNK or None, tokens)]: two strings without a common position; the second crosses a pass boundary"""
    spec = CASES[name][0]
    if name == "q8":
        return [(None, [int(t) for t in np.random.default_rng(9).integers(0, spec.vocab_size, LONG)])]
    toks = S.tokens(name, N + CHUNK + 3)
    return [(None, toks[:N]), (str(CHUNK), toks[N:])]


def tol(name):
    return 2 * G.logit_atol(CASES[name][0])  # a log-prob is a difference of two quantities within the logit tolerance


def clear(top, name):
    """top [n, TOP + 1] descending: positions where no two neighbours lie within tol - there the ids must agree"""
    return (top[:, :-1] - top[:, 1:] > tol(name)).all(axis=1)
