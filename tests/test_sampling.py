"""Seeded sampling, CPU side: the fp64 reference of the semantics (tests/sampling_ref.py) on hand-made cases, the
Philox4x32-10 known-answer vectors, the exported symbols and argument validation before any device call."""
import ctypes as C

import numpy as np
import pytest

import sampling_ref as R
from kuiperllama_amd import _ffi, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    assert R.philox4x32_10(ctr, key) == want


def test_uniform_is_open_interval_and_keyed_by_seed_halves():
    us = [R.uniform(s, c) for s in (0, 1, 1 << 32, 2 ** 64 - 1) for c in range(64)]
    assert all(0.0 < u < 1.0 for u in us)
    assert R.uniform(1, 5) != R.uniform(1 << 32, 5)  # the high word of the seed is the second key word
    x = R.philox4x32_10((7, 0, 0, 0), (3, 0))[0]
    assert R.uniform(3, 7) == ((x >> 8) + 0.5) / 2 ** 24


def test_ties_at_the_top_k_edge_keep_the_lowest_indices():
    lg = np.array([1.0, 3.0, 3.0, 2.0, 3.0], np.float32)
    S, w, _ = R.kept_set(lg, 1.0, 2, 1.0)
    assert list(S) == [1, 2]
    S, _, _ = R.kept_set(lg, 1.0, 4, 1.0)
    assert list(S) == [1, 2, 4, 3]
    np.testing.assert_allclose(R.kept_set(lg, 1.0, 4, 1.0)[1], [1, 1, 1, np.exp(-1)])


def test_k1_is_argmax_and_k_at_least_v_is_off():
    rng = np.random.default_rng(3)
    for _ in range(20):
        lg = rng.normal(size=37).astype(np.float32)
        lg[rng.integers(0, 37)] = lg.max()  # a tie for the maximum: the lower index wins
        for c in range(8):
            assert R.pick(lg, 0.7, 1, 1.0, 11, c) == int(np.argmax(lg))
            assert R.pick(lg, 0.7, 37, 1.0, 11, c) == R.pick(lg, 0.7, 0, 1.0, 11, c)
            assert R.pick(lg, 0.7, 99, 1.0, 11, c) == R.pick(lg, 0.7, 0, 1.0, 11, c)
        assert R.pick(lg, 0.0, 0, 1.0, 11, 0) == int(np.argmax(lg))
        assert R.pick(lg, -1.0, 5, 0.5, 11, 0) == int(np.argmax(lg))


def test_top_p_tiny_keeps_one_token_and_one_keeps_all():
    lg = np.array([0.5, 2.0, 2.0, -1.0, 1.5], np.float32)
    S, _, _ = R.kept_set(lg, 1.0, 0, 1e-6)
    assert list(S) == [1]
    S, _, _ = R.kept_set(lg, 1.0, 0, 1.0)
    assert sorted(S) == list(range(5))
    # P exactly reached by a prefix: that prefix, not one more
    lg2 = np.log(np.array([0.5, 0.25, 0.25])).astype(np.float64)
    S, _, _ = R.kept_set(lg2, 1.0, 0, 0.75)
    assert list(S) == [0, 1]


def test_one_token_vocabulary():
    lg = np.array([-3.0], np.float32)
    for c in range(4):
        assert R.pick(lg, 1.3, 0, 0.9, 5, c) == 0


def test_pick_walks_index_order_and_checker_tolerance():
    lg = np.zeros(4, np.float32)  # uniform: the pick is floor(4u)
    for c in range(32):
        u = R.uniform(9, c)
        assert R.pick(lg, 1.0, 0, 1.0, 9, c) == int(4 * u)
    ch = R.Checker(lg)
    picks = [R.pick(lg, 1.0, 0, 1.0, 9, c) for c in range(32)]
    assert ch.accepts(1.0, 0, 1.0, 9, range(32), picks).all()
    assert not ch.accepts(1.0, 0, 1.0, 9, range(32), [(p + 2) % 4 for p in picks]).any()
    # a token outside S is never accepted
    assert not R.Checker(np.array([5.0, 0.0, 0.0], np.float32)).accepts(1.0, 1, 1.0, 1, [0], [2]).any()


def test_sampling_symbols_are_exported(lib):
    for n in ("kh_sample_f32", "kh_sample_f32_host", "kh_model_set_sampling", "kh_model_get_sampling"):
        assert n in _ffi.EXPORTS
        assert hasattr(lib, n)
    assert C.sizeof(_ffi.Sampling) == 24


BAD = [(float("nan"), 0, 1.0), (float("inf"), 0, 1.0), (float("-inf"), 0, 1.0), (1.0, -1, 1.0),
       (1.0, 0, float("nan")), (1.0, 0, 0.0), (1.0, 0, -0.5), (1.0, 0, 1.5)]


@pytest.mark.parametrize("t,k,p", BAD)
def test_invalid_sampling_arguments_are_rejected_without_touching_the_device(lib, t, k, p):
    s = _ffi.Sampling(t, k, p, 1)
    fake = C.c_void_p(0x1000)  # never dereferenced: validation comes first
    out = C.c_int64(0)
    assert lib.kh_sample_f32(fake, 100, s, 0, 4, fake, None) == -1
    assert lib.kh_sample_f32_host(fake, 100, s, 0, C.byref(out), None) == -1
    assert lib.kh_model_set_sampling(None, s) == -1


def test_null_arguments_are_rejected(lib):
    s = _ffi.sampling(0.8, 50, 0.95, 7)
    fake = C.c_void_p(0x1000)
    assert lib.kh_sample_f32(None, 100, s, 0, 1, fake, None) == -1
    assert lib.kh_sample_f32(fake, 0, s, 0, 1, fake, None) == -1
    assert lib.kh_sample_f32(fake, 100, None, 0, 1, fake, None) == -1
    assert lib.kh_sample_f32(fake, 100, s, 0, 0, fake, None) == -1
    assert lib.kh_sample_f32_host(fake, 100, s, 0, None, None) == -1
    assert lib.kh_model_set_sampling(None, None) == -1
    assert lib.kh_model_get_sampling(None, C.byref(_ffi.Sampling())) == -1
