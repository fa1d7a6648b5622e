"""Log-probabilities, CPU side: the fp64 twin of the semantics (tests/logprobs_ref.py) on hand-computed cases, the
exported symbols, and argument validation before any device call."""
import ctypes as C

import numpy as np
import pytest

import logprobs_ref as L
from kuiperllama_amd import _ffi, build

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def test_probabilities_sum_to_one():
    rng = np.random.default_rng(0)
    lg = rng.normal(0.0, 2.0, 1000).astype(np.float32)
    lg[::9] = -INF
    lse, lp, ids, tlp = L.logprobs(lg, 5)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-12
    assert np.isneginf(lp[::9]).all() and np.isfinite(np.delete(lp, np.s_[::9])).all()
    assert list(ids) == sorted(range(1000), key=lambda i: (-float(lg[i]), i))[:5]
    assert (tlp == lp[ids]).all() and (np.diff(tlp) <= 0).all()
    # two tokens: log of one half each
    lse, lp, _, _ = L.logprobs(np.array([3.0, 3.0], np.float32))
    assert lse == pytest.approx(3.0 + np.log(2.0), abs=1e-15) and lp[0] == lp[1] == pytest.approx(-np.log(2.0), abs=1e-15)
    # a large offset does not overflow: the maximum is taken out first
    assert L.logprobs(np.array([1000.0, 999.0], np.float32))[1][0] == pytest.approx(-np.log1p(np.exp(-1.0)), abs=1e-12)


def test_ties_at_the_cut_go_to_the_lower_index():
    lg = np.array([1.0, 5.0, 2.0, 5.0, 2.0, 2.0, -0.0, 0.0], np.float32)
    assert list(L.logprobs(lg, 1)[2]) == [1]
    assert list(L.logprobs(lg, 2)[2]) == [1, 3]
    assert list(L.logprobs(lg, 3)[2]) == [1, 3, 2]       # three 2.0s, one place: the lowest index
    assert list(L.logprobs(lg, 4)[2]) == [1, 3, 2, 4]
    assert list(L.logprobs(lg, 8)[2]) == [1, 3, 2, 4, 5, 0, 6, 7]  # -0 and +0 are one value: index order
    assert list(L.logprobs(np.full(50, 0.25, np.float32), 20)[2]) == list(range(20))


def test_fewer_finite_logits_than_asked_for():
    lg = np.full(12, -INF, np.float32)
    lg[7], lg[3] = 1.5, -2.0
    lse, lp, ids, tlp = L.logprobs(lg, 5)
    assert list(ids) == [7, 3, 0, 1, 2]  # then the -inf entries in index order
    assert np.isfinite(tlp[:2]).all() and np.isneginf(tlp[2:]).all()
    lg = np.full(30, -INF, np.float32)
    lg[11] = 4.0
    lse, lp, ids, tlp = L.logprobs(lg, 3)
    assert lse == 4.0 and lp[11] == 0.0 and list(ids) == [11, 0, 1]


def test_no_alternatives_asked_for():
    lse, lp, ids, tlp = L.logprobs(np.array([0.5, -1.0, 2.0], np.float32), 0)
    assert ids.shape == (0,) and tlp.shape == (0,) and lp.shape == (3,) and np.isfinite(lse)
    with pytest.raises(AssertionError):
        L.logprobs(np.array([0.5, -1.0, 2.0], np.float32), 4)  # more than the vocabulary has
    with pytest.raises(AssertionError):
        L.logprobs(np.zeros(100, np.float32), 21)


def test_tolerance_of_the_shapes_the_gpu_test_uses():
    assert L.tol(501, 0.0) == 2.0 ** -24 * 17
    assert L.tol(128256, 10.0, -2.0) == 2.0 ** -24 * (126 + 16) + 2.0 ** -23 * 12.0


def test_symbols_are_exported(lib):
    for n in ("kh_logprobs_f32", "kh_model_set_logprobs", "kh_model_get_logprobs_setting", "kh_model_get_logprobs"):
        assert n in _ffi.EXPORTS
        assert hasattr(lib, n)
    assert _ffi.KH_LOGPROBS_MAX_TOP == L.MAX_TOP == 20


def test_invalid_arguments_are_rejected_without_touching_the_device(lib):
    fake = C.c_void_p(0x1000)  # never dereferenced: validation comes first
    f = lib.kh_logprobs_f32
    assert f(fake, 100, 1, fake, -1, fake, fake, fake, fake, None) == _ffi.KH_ERR_INVALID_ARG   # top_n < 0
    assert f(fake, 100, 1, fake, 21, fake, fake, fake, fake, None) == _ffi.KH_ERR_INVALID_ARG   # top_n > 20
    assert f(fake, 7, 1, fake, 8, fake, fake, fake, fake, None) == _ffi.KH_ERR_INVALID_ARG      # top_n > n
    assert f(fake, 100, 0, fake, 5, fake, fake, fake, fake, None) == _ffi.KH_ERR_INVALID_ARG    # no rows
    assert f(fake, 100, -3, fake, 5, fake, fake, fake, fake, None) == _ffi.KH_ERR_INVALID_ARG
    assert f(None, 100, 1, fake, 5, fake, fake, fake, fake, None) == _ffi.KH_ERR_INVALID_ARG    # logits
    assert f(fake, 0, 1, fake, 0, fake, fake, fake, fake, None) == _ffi.KH_ERR_INVALID_ARG      # n
    # the model entry points
    n = C.c_int32(0)
    assert lib.kh_model_set_logprobs(None, 5) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_model_set_logprobs(None, 21) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_model_set_logprobs(None, -2) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_model_get_logprobs_setting(None, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_model_get_logprobs(None, 0, 1, None, None, None, None) == _ffi.KH_ERR_INVALID_ARG
