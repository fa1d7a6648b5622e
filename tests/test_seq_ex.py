"""Per-sequence penalties, logit bias and log-probs in batched decode, CPU side: the new symbols, kh_seq_rank - the one
definition of "best" of best-of-n - against a Python statement of it, argument validation of the _ex entry points and
the slot accessors before any device call, and the Python wrappers' own checks.  Every test needs symbols the feature
adds."""
import ctypes as C
import math

import numpy as np
import pytest

import score_cases as S
from kuiperllama_amd import _ffi, build
from kuiperllama_amd.model import KuiperModel, seq_rank

NEW = ["kh_model_seq_step_ex", "kh_model_generate_batch_ex", "kh_model_seq_set_history", "kh_model_seq_get_logprobs",
       "kh_seq_rank"]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def test_symbols_are_exported_and_bound(lib):
    for name in NEW:
        assert name in _ffi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert _ffi.KH_SEQ_BIAS_MAX == 64
    assert [f for f, _ in _ffi.SeqOpts._fields_] == ["samplings", "penalties", "n_bias", "bias_ids", "bias",
                                                     "logprobs_top_n"]


# ---- kh_seq_rank ------------------------------------------------------------------------------------------------------
def _rank(lp, first, n_words):
    """the header's statement: the fp64 sum in index order over the count (NaN: empty range, or a NaN entry); order by
    that mean descending, ties and NaN by ascending index, NaN last"""
    mean = []
    for s in range(len(first)):
        acc = 0.0
        for p in range(first[s], n_words[s]):
            acc += float(np.float64(lp[s][p]))
        mean.append(acc / (n_words[s] - first[s]) if n_words[s] > first[s] else math.nan)
    ok = sorted((s for s in range(len(mean)) if not math.isnan(mean[s])), key=lambda s: (-mean[s], s))
    return ok + [s for s in range(len(mean)) if math.isnan(mean[s])], mean


def _call(lib, lp, first, n_words):
    lp = np.ascontiguousarray(lp, np.float32)
    n, stride = lp.shape
    order = (C.c_int32 * n)(*([-7] * n))
    mean = np.full(n, -7.0, np.float64)
    rc = lib.kh_seq_rank(n, lp.ctypes.data_as(C.POINTER(C.c_float)), stride, (C.c_int32 * n)(*first),
                         (C.c_int32 * n)(*n_words), order, mean.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, list(order), mean


def _same_means(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (math.isnan(g) and math.isnan(w)) or np.float64(g).tobytes() == np.float64(w).tobytes(), (got, want)


@pytest.mark.parametrize("n_seq", [1, 3, 8, 64])
def test_seq_rank_is_the_stated_order(lib, n_seq):
    rng = np.random.default_rng(n_seq)
    stride = 37
    lp = -rng.random((n_seq, stride), np.float32) * 9
    first = [int(t) for t in rng.integers(0, 5, n_seq)]
    n_words = [int(t) for t in rng.integers(5, stride + 1, n_seq)]
    rc, order, mean = _call(lib, lp, first, n_words)
    want_order, want_mean = _rank(lp, first, n_words)
    assert rc == 0 and order == want_order
    _same_means(mean, want_mean)
    assert sorted(order) == list(range(n_seq))
    # the wrapper: rows of unequal length, the same answer
    o2, m2 = seq_rank([lp[s, :n_words[s]] for s in range(n_seq)], first, n_words)
    assert o2 == want_order
    _same_means(m2, want_mean)


def test_seq_rank_ties_empty_ranges_and_nan(lib):
    lp = np.array([[-1.0, -2.0, -3.0, -4.0],    # mean of [1, 3): -2.5
                   [-2.5, -2.5, -2.5, -2.5],    # the same mean: a tie, the lower index first
                   [-0.5, -0.5, -0.5, -0.5],    # an empty range: NaN
                   [-0.1, np.nan, -0.1, -0.1],  # a NaN entry inside the range: NaN
                   [np.nan, -0.25, -0.25, 9.0], # NaN and junk outside the range do not count: the best
                   [-2.5, -2.5, -2.5, -2.5]], np.float32)
    first = [1, 0, 2, 0, 1, 2]
    n_words = [3, 4, 2, 4, 3, 4]
    rc, order, mean = _call(lib, lp, first, n_words)
    assert rc == 0
    assert order == [4, 0, 1, 5, 2, 3]
    _same_means(mean, [-2.5, -2.5, math.nan, math.nan, -0.25, -2.5])
    assert _rank(lp, first, n_words)[0] == order
    # first beyond n_words is an empty range too; -inf is a value, not NaN, and sorts below every finite mean
    rc, order, mean = _call(lib, np.array([[-np.inf, -1.0], [-3.0, -3.0], [-1.0, -1.0]], np.float32), [0, 0, 2], [2, 2, 1])
    assert rc == 0 and order == [1, 0, 2] and mean[0] == -np.inf and math.isnan(mean[2])
    # mean_lp is optional
    o = (C.c_int32 * 2)()
    two = np.array([[-2.0], [-1.0]], np.float32)
    assert lib.kh_seq_rank(2, two.ctypes.data_as(C.POINTER(C.c_float)), 1, (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(1, 1),
                           o, None) == 0
    assert list(o) == [1, 0]


def test_seq_rank_rejects_bad_arguments(lib):
    lp = np.zeros((2, 4), np.float32)
    p = lp.ctypes.data_as(C.POINTER(C.c_float))
    z, f, o = (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(4, 4), (C.c_int32 * 2)()
    mean = (C.c_double * 2)()
    bad = _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_seq_rank(0, p, 4, z, f, o, mean) == bad
    assert lib.kh_seq_rank(-1, p, 4, z, f, o, mean) == bad
    assert lib.kh_seq_rank(2, None, 4, z, f, o, mean) == bad
    assert lib.kh_seq_rank(2, p, 4, None, f, o, mean) == bad
    assert lib.kh_seq_rank(2, p, 4, z, None, o, mean) == bad
    assert lib.kh_seq_rank(2, p, 4, z, f, None, mean) == bad
    assert lib.kh_seq_rank(2, p, 3, z, f, o, mean) == bad                        # n_words past the row
    assert lib.kh_seq_rank(2, p, 4, (C.c_int32 * 2)(0, -1), f, o, mean) == bad   # a negative first
    assert lib.kh_seq_rank(2, p, 4, z, f, o, mean) == 0
    with pytest.raises(ValueError):
        seq_rank([[0.0, 0.0], [0.0]], [0], [2, 1])
    with pytest.raises(ValueError):
        seq_rank([[0.0, 0.0], [0.0]], [0, 0], [2, 2])  # row 1 holds one log-prob


# ---- validation before any device call ------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected_without_touching_the_device(lib):
    fake = C.c_void_p(0x1000)  # never dereferenced: these checks come first
    four = (C.c_int32 * 4)(1, 2, 3, 4)
    none = C.POINTER(C.c_int32)()
    bad = _ffi.KH_ERR_INVALID_ARG
    o = _ffi.SeqOpts()
    o.logprobs_top_n = 0
    for opts in (None, C.byref(o)):
        assert lib.kh_model_seq_step_ex(None, 4, four, four, four, opts, four) == bad
        assert lib.kh_model_seq_step_ex(fake, 0, four, four, four, opts, four) == bad
        assert lib.kh_model_seq_step_ex(fake, 4, none, four, four, opts, four) == bad
        assert lib.kh_model_seq_step_ex(fake, 4, four, none, four, opts, four) == bad
        assert lib.kh_model_seq_step_ex(fake, 4, four, four, none, opts, four) == bad
        assert lib.kh_model_seq_step_ex(fake, 4, four, four, four, opts, none) == bad
        ms = C.c_float(0)
        g = lib.kh_model_generate_batch_ex
        assert g(None, 1, four, four, None, four, opts, None, 0, four, 4, four, C.byref(ms)) == bad
        assert g(fake, 0, four, four, None, four, opts, None, 0, four, 4, four, C.byref(ms)) == bad
        assert g(fake, 1, none, four, None, four, opts, None, 0, four, 4, four, C.byref(ms)) == bad
        assert g(fake, 1, four, none, None, four, opts, None, 0, four, 4, four, C.byref(ms)) == bad
        assert g(fake, 1, four, four, None, none, opts, None, 0, four, 4, four, C.byref(ms)) == bad
        assert g(fake, 1, four, four, None, four, opts, None, 0, none, 4, four, C.byref(ms)) == bad
        assert g(fake, 1, four, four, None, four, opts, None, 0, four, 4, none, C.byref(ms)) == bad
        assert g(fake, 1, four, four, None, four, opts, None, 0, four, 0, four, C.byref(ms)) == bad  # no room for words
        assert g(fake, 1, four, four, None, four, opts, None, 2, four, 4, four, C.byref(ms)) == bad  # stops without a list
    assert lib.kh_model_seq_set_history(None, 0, 0, four, 4) == bad
    assert lib.kh_model_seq_set_history(fake, 0, 0, none, 4) == bad
    assert lib.kh_model_seq_set_history(fake, 0, 0, four, 0) == bad
    assert lib.kh_model_seq_set_history(fake, 0, -1, four, 4) == bad
    buf = (C.c_float * 4)()
    assert lib.kh_model_seq_get_logprobs(None, 0, 0, 4, None, buf, None, None) == bad
    assert lib.kh_model_seq_get_logprobs(fake, 0, 0, 0, None, buf, None, None) == bad
    assert lib.kh_model_seq_get_logprobs(fake, 0, 0, -3, None, buf, None, None) == bad


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def test_wrappers_reject_ragged_arguments_before_the_library():
    m = KuiperModel.__new__(KuiperModel)  # a null handle: the library would refuse it, the wrappers never get there
    m._h, m._keep, m.spec, m._seq_slots, m._seq_top_n = C.c_void_p(), None, S.SPECS["a"], 1, None
    pen = {"repetition": 1.3}
    try:
        with pytest.raises(ValueError):
            m.seq_step([0, 1], [5, 6], [0, 0], penalties=[pen])
        with pytest.raises(ValueError):
            m.seq_step([0, 1], [5, 6], [0, 0], logit_bias=[{3: 1.0}, None, None])
        with pytest.raises(ValueError):
            m.seq_step([0, 1], [5, 6], [0, 0], samplings=[None], logprobs=0)
        with pytest.raises(ValueError):
            m.seq_step([0, 1], [5], [0, 0], logprobs=0)
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], 8, penalties=[pen, pen, pen])
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], 8, logit_bias=[{3: 1.0}])
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], 8, samplings=[{"temperature": 0.8}], logprobs=5)
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], [8], logprobs=5)
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], 8, cached=[1], logprobs=5)
        with pytest.raises(TypeError):
            m.generate_batch([[1, 2], [3]], 8, penalties=[pen, {"repeat": 1.3}])  # not a key of set_penalties
        with pytest.raises(ValueError):
            m.seq_logprobs(0, 0, 4)  # no call with logprobs= yet: no width to read with
        with pytest.raises(ValueError):
            m.best_of([], 3, 8, {"temperature": 0.8})
        with pytest.raises(ValueError):
            m.best_of([1, 2], 0, 8, {"temperature": 0.8})
        # well-formed arguments do reach the library, which refuses the null model
        for call in (lambda: m.seq_step([0, 1], [5, 6], [0, 0], penalties=[pen, None], logit_bias=[None, {3: -np.inf}]),
                     lambda: m.generate_batch([[1, 2], [3]], 8, penalties=[None, pen], logprobs=20),
                     lambda: m.seq_set_history(0, [1, 2, 3])):
            with pytest.raises(_ffi.KhError) as ei:
                call()
            assert ei.value.code == _ffi.KH_ERR_INVALID_ARG
        assert m._seq_top_n is None  # a refused call leaves seq_logprobs' width alone
    finally:
        m.close()  # nothing to destroy
