"""Logit processors, CPU side: the numpy float32 twin of the semantics (tests/logit_proc_ref.py) on hand-computed
cases, the exported symbols, and argument validation before any device call."""
import ctypes as C

import numpy as np
import pytest

import logit_proc_ref as R
from kuiperllama_amd import _ffi, build

F = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def test_positive_zero_negative_and_minus_inf_logits():
    lg = np.array([2.0, 0.0, -3.0, -INF, 5.0], F)
    hist = [0, 1, 2, 3]  # token 4 is not in the window
    out = R.process(lg, hist, 3, repetition=1.5)
    assert out.dtype == F
    assert out[0] == F(2.0) / F(1.5)      # positive: divided
    assert out[1] == 0.0                  # zero: 0 * r
    assert out[2] == F(-3.0) * F(1.5)     # negative: multiplied
    assert out[3] == -INF                 # -inf stays
    assert out[4] == 5.0                  # untouched
    out = R.process(lg, hist, 3, repetition=1.5, presence=0.25, frequency=0.5)
    assert out[0] == F(2.0) / F(1.5) - (F(1) * F(0.5) + F(0.25))
    assert out[1] == F(-0.75)
    assert out[2] == F(-4.5) - F(0.75)
    assert out[3] == -INF and out[4] == 5.0
    # repetition 1 and zero penalties are skipped: the very bits of the input
    assert R.process(lg, hist, 3).tobytes() == lg.tobytes()


def test_counts_one_and_three_apply_once():
    lg = np.array([1.0, 4.0, -2.0], F)
    hist = [1, 0, 1, 1]  # c(1) = 3, c(0) = 1, c(2) = 0
    out = R.process(lg, hist, 3, repetition=2.0, presence=0.5, frequency=0.1)
    assert out[0] == F(0.5) - (F(1) * F(0.1) + F(0.5))
    assert out[1] == F(2.0) - (F(3) * F(0.1) + F(0.5))  # divided ONCE, the count enters the frequency term only
    assert out[2] == -2.0
    assert list(R.counts(hist, 3, 0, 3)) == [1, 3, 0]


def test_window_cuts_a_run_and_ignores_foreign_entries():
    hist = [7, 7, 7, 7, 7, 2, -1, 9 + 7]  # V = 9: -1 (never written) and V + 7 are ignored
    assert list(R.window(hist, 7, 5)) == [7, 7, 2, -1, 16]
    c = R.counts(hist, 7, 5, 9)
    assert c[7] == 2 and c[2] == 1 and c.sum() == 3
    assert R.counts(hist, 7, 0, 9)[7] == 5          # last_n 0: the whole sequence
    assert R.counts(hist, 4, 1, 9)[7] == 1          # a window of one position
    assert R.counts(hist, 7, 100, 9)[7] == 5        # longer than the sequence
    assert R.counts(hist, 3, 0, 9).sum() == 4       # positions beyond pos are not read
    lg = np.arange(9, dtype=F)
    out = R.process(lg, hist, 7, frequency=1.0, last_n=5)
    assert out[7] == 5.0 and out[2] == 1.0 and out[8] == 8.0


def test_bias_comes_last_and_bans():
    lg = np.array([1.0, 3.0, 2.0, -INF], F)
    out = R.process(lg, [1], 0, repetition=2.0, bias={1: 0.25, 2: -INF, 3: 5.0})
    assert out[1] == F(1.5) + F(0.25)     # penalised, then biased
    assert out[2] == -INF and out[3] == -INF
    assert R.greedy(out) == 1
    assert R.greedy(np.array([1.0, 7.0, 7.0], F)) == 1  # first maximum


def test_symbols_are_exported(lib):
    for n in ("kh_logit_process_workspace_bytes", "kh_logit_process_f32", "kh_model_set_penalties",
              "kh_model_get_penalties", "kh_model_set_logit_bias"):
        assert n in _ffi.EXPORTS
        assert hasattr(lib, n)
    assert C.sizeof(_ffi.Penalties) == 16
    assert lib.kh_logit_process_workspace_bytes(128256) == 4 * 128256
    assert lib.kh_logit_process_workspace_bytes(0) == -1


BAD = [(float("nan"), 0.0, 0.0, 0), (INF, 0.0, 0.0, 0), (0.0, 0.0, 0.0, 0), (-1.5, 0.0, 0.0, 0),
       (1.0, float("nan"), 0.0, 0), (1.0, INF, 0.0, 0), (1.0, 0.0, float("nan"), 0), (1.0, 0.0, -INF, 0),
       (1.3, 0.5, 0.2, -1)]


@pytest.mark.parametrize("r,pres,freq,n", BAD)
def test_invalid_penalties_are_rejected_without_touching_the_device(lib, r, pres, freq, n):
    p = _ffi.Penalties(r, pres, freq, n)
    fake = C.c_void_p(0x1000)  # never dereferenced: validation comes first
    assert lib.kh_logit_process_f32(fake, 100, fake, None, 5, p, None, None, 0, fake, None) == -1
    assert lib.kh_logit_process_f32(None, 100, None, None, 5, p, None, None, 0, None, None) == -1
    assert lib.kh_model_set_penalties(None, p) == -1


def test_null_arguments_are_rejected(lib):
    p = _ffi.penalties(1.3, 0.5, 0.2, 16)
    fake = C.c_void_p(0x1000)
    assert lib.kh_model_set_penalties(None, p) == -1
    assert lib.kh_model_set_penalties(None, None) == -1
    assert lib.kh_model_get_penalties(None, C.byref(_ffi.Penalties())) == -1
    assert lib.kh_logit_process_f32(None, 100, fake, None, 5, p, None, None, 0, fake, None) == -1   # logits
    assert lib.kh_logit_process_f32(fake, 0, fake, None, 5, p, None, None, 0, fake, None) == -1     # n
    assert lib.kh_logit_process_f32(fake, 100, None, None, 5, p, None, None, 0, fake, None) == -1   # tokens
    assert lib.kh_logit_process_f32(fake, 100, fake, None, 5, p, None, None, 0, None, None) == -1   # workspace
    assert lib.kh_logit_process_f32(fake, 100, fake, None, -1, p, None, None, 0, fake, None) == -1  # position
    assert lib.kh_logit_process_f32(fake, 100, fake, None, 5, p, None, None, 2, fake, None) == -1   # bias arrays
    assert lib.kh_logit_process_f32(fake, 100, fake, None, 5, p, fake, fake, -1, fake, None) == -1
    # all neutral and no bias entries: off - nothing is launched, no pointer is needed beyond the logits
    assert lib.kh_logit_process_f32(fake, 100, None, None, 5, None, None, None, 0, None, None) == 0
    assert lib.kh_logit_process_f32(fake, 100, None, None, 5, _ffi.penalties(1.0, 0.0, 0.0, 7), None, None, 0, None,
                                    None) == 0


def _bias(lib, ids, vals, m=None):
    a = (C.c_int32 * max(len(ids), 1))(*ids)
    b = (C.c_float * max(len(vals), 1))(*vals)
    return lib.kh_model_set_logit_bias(m, a, b, len(ids))


def test_invalid_bias_lists_are_rejected_without_touching_the_device(lib):
    assert _bias(lib, [1, 2], [0.5, float("nan")]) == -1
    assert _bias(lib, [1, 2], [INF, 0.0]) == -1
    assert _bias(lib, [3, 5, 3], [0.5, 0.25, -INF]) == -1        # duplicate id
    assert _bias(lib, [1, -4], [0.5, 0.5]) == _ffi.KH_ERR_RANGE  # below every vocabulary
    assert _bias(lib, [1, 2], [0.5, -INF]) == -1                 # a valid list, no model
    assert _bias(lib, [], []) == -1
    assert lib.kh_model_set_logit_bias(None, None, None, 2) == -1
    assert lib.kh_model_set_logit_bias(None, None, None, -1) == -1
