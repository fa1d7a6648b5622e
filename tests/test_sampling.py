"""Seeded sampling, CPU side: the fp64 reference of the semantics (tests/sampling_ref.py) on hand-made cases, the
Philox4x32-10 known-answer vectors (scalar and vectorised), the integer statement of two-level rows against the fp64
one, the exported symbols and argument validation before any device call."""
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


def test_vectorised_philox_is_the_scalar_one():
    rng = np.random.default_rng(1)
    counters = np.concatenate([np.arange(3000), rng.integers(0, 2 ** 32, 1000), [2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1]])
    for seed in (0, 1, 0x1234_5678_9ABC, 1 << 32, 2 ** 64 - 1):
        key = (seed & R.MASK, seed >> 32)
        want = [R.philox4x32_10((int(c), 0, 0, 0), key)[0] >> 8 for c in counters]
        got = R.philox_u24(seed, counters)
        assert got.dtype == np.uint64 and got.tolist() == want
        lo, hi = R.extreme_counters(seed, 3000)
        assert (lo, hi) == (int(np.argmin(want[:3000])), int(np.argmax(want[:3000])))
        assert R.uniform(seed, lo) == (want[lo] + 0.5) / 2 ** 24


def _two_level_row(rng, V, nA, T, low_inf, third):
    """(fp32 row, ascending indices of the maximum): the rest at 3 - 128 T (e = -128: weight zero on the device) or
    -inf, and - `third` - up to three of them at 3 - 3 T instead (a weighted level)"""
    A = np.sort(rng.choice(V, nA, replace=False))
    lg = np.full(V, -np.inf if low_inf else 3.0 - 128.0 * T, np.float32)
    lg[A] = 3.0
    rest = np.setdiff1d(np.arange(V), A)
    if third and rest.size:
        lg[rng.choice(rest, min(3, rest.size), replace=False)] = 3.0 - 3.0 * T
    return lg, A


def test_two_level_pick_is_the_fp64_pick():
    """The integer statement of a two-level row against the fp64 semantics on 400 small random rows.  Both are exact
    here - fp64 sums of ones, P32 * n and u * m carry no rounding, and a weight of exp(-128) vanishes against Z >= 1 -
    so any disagreement would have to come from a threshold within 1e-12 relative of a boundary: there is none."""
    rng = np.random.default_rng(20241020)
    n_rows = n_draws = 0
    for r in range(400):
        V = int(rng.integers(2, 601))
        nA = int(rng.choice([1, 2, V, int(rng.integers(1, V + 1))]))
        T = float(np.float32(rng.choice([1.0, 0.02, 50.0])))
        K = int(rng.choice([0, 1, nA - 1, nA, nA + 1, V - 1, V, int(rng.integers(0, V + 2))]))
        third = 0 < K <= nA and K < V and r % 3 == 0
        lg, A = _two_level_row(rng, V, nA, T, bool(r % 2), third)
        n = R.two_level_kept(nA, V, K, 1.0)[0]
        P = float(np.float32(rng.choice([1.0, 0.5, 0.75, 0.999, 1e-6, (n - 1) / n if n > 1 else 0.25, rng.random()])))
        seed = int(rng.integers(0, 2 ** 63))
        for c in range(r, r + 6):
            got, want = R.two_level_pick(A, V, K, P, seed, c), R.pick(lg, T, K, P, seed, c)
            if got != want:  # how close the fp64 threshold is to a boundary of its walk
                S, w, _ = R.kept_set(lg, T, K, P)
                cum = np.cumsum(w[np.argsort(S, kind="stable")])
                gap = np.abs(cum - R.uniform(seed, c) * cum[-1]).min() / cum[-1]
                raise AssertionError((V, nA, T, K, P, seed, c, got, want, f"boundary distance {gap:.3e} of Z"))
            n_draws += 1
        n_rows += 1
    assert (n_rows, n_draws) == (400, 2400)


def test_predict_path_on_hand_made_rows():
    def row(V, nA, low=-np.inf):
        lg = np.full(V, low, np.float32)
        lg[:nA] = 3.0
        return lg
    p = R.predict_path(row(4097, 4097), 1.0, 0, 1.0)  # no top-k, no top-p: the row itself is the candidate list
    assert (p["mode"], p["ncand"], p["in_lds"], p["descents"], p["levels"]) == ("neither", 4097, False, ("pick",), 2)
    assert R.predict_path(row(4096, 7), 1.0, 4096, 1.0)["in_lds"]  # K = V is off
    p = R.predict_path(row(300, 100, -200.0), 1.0, 100, 1.0)  # m_key == ties: no index cut
    assert (p["mode"], p["ncand"], p["descents"], p["m_key"], p["ties"]) == ("top-k only", 100, ("top-k key", "pick"), 100, 100)
    p = R.predict_path(row(300, 100, -200.0), 1.0, 99, 0.5)  # cap = m_k = 99: m = 50 < ties
    assert (p["mode"], p["descents"], p["m_key"]) == ("both", ("top-k key", "top-p key", "index cut", "pick"), 50)
    p = R.predict_path(row(5000, 100), 0.02, 101, 1.0)  # K beyond the weighted tokens: every token is a candidate
    assert (p["ncand"], p["in_lds"], p["m_key"], p["ties"], p["index_cut"]) == (5000, False, 1, 4900, True)
    p = R.predict_path(row((1 << 19) + 19, 4097), 50.0, 0, 0.5)
    assert (p["mode"], p["ncand"], p["in_lds"], p["m_key"], p["levels"]) == ("top-p only", 4097, False, 2049, 3)
    assert R.predict_path(row(255, 3), 1.0, 2, 1.0)["levels"] == 1 and R.predict_path(row(256, 3), 1.0, 2, 1.0)["levels"] == 2
    assert R.predict_path(row(1, 1), 1.0, 0, 1.0) == {"trivial": True}
    with pytest.raises(AssertionError):  # a weighted third level that top-k does not cut off is no two-level row
        R.predict_path(np.array([3.0, 3.0, 1.0, -np.inf], np.float32), 1.0, 0, 0.5)


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
