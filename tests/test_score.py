"""Sequence scoring, CPU side: the exported symbol, argument validation before any device call, the arithmetic of
KuiperModel.score's totals, and the seed of the GPU suite's oracle check.  The last two tests (the case table and the
oracle seed) guard the fixtures of tests/test_score_gpu.py and do not exercise the feature: they pass without it.  The
first three need kh_model_score / KuiperModel.score_totals."""
import ctypes as C

import numpy as np
import pytest

import score_cases as S
from kuiperllama_amd import _ffi, build
from kuiperllama_amd.model import KuiperModel


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def test_symbol_is_exported(lib):
    assert "kh_model_score" in _ffi.EXPORTS
    assert hasattr(lib, "kh_model_score")


def test_invalid_arguments_are_rejected_without_touching_the_device(lib):
    fake = C.c_void_p(0x1000)  # never dereferenced: validation comes first
    toks = (C.c_int32 * 4)(1, 2, 3, 4)
    none = C.POINTER(C.c_int32)()
    f = lib.kh_model_score
    assert f(None, toks, 4, 0) == _ffi.KH_ERR_INVALID_ARG   # no model
    assert f(fake, none, 4, 0) == _ffi.KH_ERR_INVALID_ARG   # no tokens
    assert f(fake, toks, 0, 0) == _ffi.KH_ERR_INVALID_ARG   # n <= 0
    assert f(fake, toks, -4, 0) == _ffi.KH_ERR_INVALID_ARG
    assert f(fake, toks, 4, -1) == _ffi.KH_ERR_INVALID_ARG  # pos0 < 0


def test_totals_of_a_hand_made_record():
    lp = np.array([-0.5, -2.25, -1.0, np.nan], np.float32)
    rec = {"token": np.array([7, 9, 4, -1], np.int32), "logprob": lp,
           "top_ids": np.zeros((4, 0), np.int32), "top_logprobs": np.zeros((4, 0), np.float32)}
    out = KuiperModel.score_totals(rec)
    assert set(out) == {"token", "logprob", "top_ids", "top_logprobs", "sum_logprob", "perplexity"}
    assert out["logprob"] is lp  # the records themselves are handed through
    assert isinstance(out["sum_logprob"], float) and out["sum_logprob"] == -3.75  # exact in binary
    assert out["perplexity"] == pytest.approx(np.exp(3.75 / 3), rel=1e-15)
    # the sum runs in float64: 2^24 + 1 terms of one float32 value do not stall
    many = {"token": np.zeros(2 ** 24 + 2, np.int32), "logprob": np.full(2 ** 24 + 2, -1.0, np.float32)}
    many["token"][-1] = -1
    many["logprob"][-1] = np.nan
    assert KuiperModel.score_totals(many)["sum_logprob"] == -(2.0 ** 24 + 1)
    # one token predicts nothing inside the call
    one = KuiperModel.score_totals({"token": np.array([-1], np.int32), "logprob": np.array([np.nan], np.float32)})
    assert one["sum_logprob"] == 0.0 and np.isnan(one["perplexity"])
    # a certain text has perplexity one; an impossible token makes it infinite
    sure = KuiperModel.score_totals({"token": np.array([3, -1], np.int32), "logprob": np.array([0.0, np.nan], np.float32)})
    assert sure["perplexity"] == 1.0
    never = KuiperModel.score_totals({"token": np.array([3, -1], np.int32), "logprob": np.array([-np.inf, np.nan], np.float32)})
    assert never["sum_logprob"] == -np.inf and never["perplexity"] == np.inf


def test_case_table():
    for name, spec in S.SPECS.items():
        B = S.BATCH[name]
        assert S.lengths(name) == [1, B - 1, B, B + 1, 2 * B + 3]
        assert spec.head_size > 32 and spec.dim <= 4096 and 5 + max(S.lengths(name)) <= spec.seq_len
        # tokens per pass as prefill_batch decides: 8 vectors of dim floats and the reduction slots within 80 KiB
        assert B == (8 if not spec.quant and 8 * spec.dim * 4 + 3 * 8 * 8 * 4 <= 80 * 1024 else 4), name
    assert S.SPECS["d"].vocab_size % 2 == 1 and S.SPECS["d"].dim > 2560
    assert S.LONG_N + 1 <= S.SPECS["a"].seq_len and S.LONG_N > 256 + 8
    assert len(set(S.tokens("a", S.LONG_N))) == S.LONG_N


def test_oracle_seed_keeps_the_top_lists_checkable(oracle):
    """The GPU suite compares top ids with the oracle's only where no boundary of the list lies within twice the logit
    parity bound, and asserts that this covers 90 % of the positions: with the oracle alone, the seed does."""
    toks, rows = S.oracle_rows(oracle, S.oracle_image())
    lp, order, checkable = S.oracle_expectation(rows)
    assert rows.shape == (S.ORACLE_T, S.SPECS["a"].vocab_size) and np.isfinite(rows).all()
    assert np.allclose(np.exp(lp).sum(axis=1), 1.0, atol=1e-12)
    assert checkable.mean() >= 0.9, checkable
    print(f"checkable positions: {int(checkable.sum())} of {S.ORACLE_T}")
