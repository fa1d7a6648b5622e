"""Sequence slots, CPU side: the partition of the cache rows (kh_plan_seq_slots) against a Python statement of it, the
lane grouping of generate_batch (kh_plan_seq_batch) against a Python twin of the rule, argument validation before any
device call, and the Python wrappers' own checks.  Every test needs symbols the feature adds."""
import ctypes as C

import pytest

import score_cases as S
from kuiperllama_amd import _ffi, build
from kuiperllama_amd.model import KuiperModel, plan_seq_batch, plan_seq_slots

NEW = ["kh_model_seq_slots", "kh_plan_seq_slots", "kh_model_seq_width", "kh_model_seq_prefill", "kh_model_seq_fork",
       "kh_model_seq_step", "kh_model_generate_batch", "kh_model_generate_batch_from", "kh_plan_seq_batch"]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def test_symbols_are_exported(lib):
    for name in NEW:
        assert name in _ffi.EXPORTS and hasattr(lib, name), name


# ---- the partition ----------------------------------------------------------------------------------------------------
def _partition(cache_len, n_slots):
    """the issue's statement: 1 <= n_slots <= 64, slot_len = cache_len // n_slots >= 8, else refused (None)"""
    if not 1 <= n_slots <= 64:
        return None
    slot_len = cache_len // n_slots
    return slot_len if slot_len >= 8 else None


def test_plan_seq_slots_is_the_stated_partition(lib):
    out = C.c_int32(-5)
    for cache_len in (8, 15, 16, 64, 320, 511, 512, 1280, 4096, 131072):
        for n_slots in (-1, 0, 1, 2, 3, 4, 7, 8, 9, 40, 63, 64, 65, 1000):
            want = _partition(cache_len, n_slots)
            rc = lib.kh_plan_seq_slots(cache_len, n_slots, C.byref(out))
            if want is None:
                assert rc == _ffi.KH_ERR_INVALID_ARG, (cache_len, n_slots)
                with pytest.raises(_ffi.KhError):
                    plan_seq_slots(cache_len, n_slots)
            else:
                assert rc == 0 and out.value == want, (cache_len, n_slots)
                assert plan_seq_slots(cache_len, n_slots) == want
                # the slots are disjoint and inside the cache; what is left over is less than one row per slot
                rows = [(s * want, (s + 1) * want) for s in range(n_slots)]
                assert rows[0][0] == 0 and rows[-1][1] <= cache_len < rows[-1][1] + n_slots
                assert all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
    # the rejections the issue names, and the cases of the GPU suite
    assert lib.kh_plan_seq_slots(320, 0, C.byref(out)) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_slots(4096, 65, C.byref(out)) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_slots(64, 9, C.byref(out)) == _ffi.KH_ERR_INVALID_ARG  # slot_len 7
    assert lib.kh_plan_seq_slots(64, 8, None) == 0                                 # slot_len 8, no out pointer
    assert plan_seq_slots(S.SPECS["a"].seq_len, 8) == 40 and plan_seq_slots(S.SPECS["b"].seq_len, 4) == 16
    assert plan_seq_slots(1280, 4) == 320


# ---- the lane grouping --------------------------------------------------------------------------------------------------
def _passes(first_pos, totals, width):
    """Python twin of the rule: rounds over the sequences in slot order, every round cut into passes of up to `width`
    live sequences; a sequence is live while its position is below its total"""
    pos, out = list(first_pos), []
    while True:
        live = [s for s in range(len(pos)) if pos[s] < totals[s]]
        if not live:
            return out
        for i in range(0, len(live), width):
            out.append(live[i:i + width])
        for s in live:
            pos[s] += 1


@pytest.mark.parametrize("width", [4, 8])
def test_plan_seq_batch_groups_the_live_sequences_in_slot_order(lib, width):
    for n_seq in (1, width, width + 1, 2 * width + 3):
        first = [(3 * s) % 5 for s in range(n_seq)]                     # prompts of 1 .. 5 tokens
        totals = [first[s] + 1 + (7 * s + 2) % 9 for s in range(n_seq)]  # 1 .. 9 sampled steps: they finish apart
        got = plan_seq_batch(first, totals, width)
        assert got == _passes(first, totals, width), (n_seq, width)
        # every sequence is fed at each of its positions exactly once, in order, never twice in one pass
        fed = {s: 0 for s in range(n_seq)}
        for lanes in got:
            assert 1 <= len(lanes) <= width and lanes == sorted(set(lanes))
            for s in lanes:
                fed[s] += 1
        assert [fed[s] for s in range(n_seq)] == [totals[s] - first[s] for s in range(n_seq)]
        # while more than `width` sequences are live a step takes ceil(live / width) passes; a sequence that
        # finished has left the lane table
        if n_seq == width + 1:
            assert got[0] == list(range(width)) and got[1] == [width]
        done_at = min(totals[s] - first[s] for s in range(n_seq))
        per_round = -(-n_seq // width)
        assert all(len(set(sum(got[r * per_round:(r + 1) * per_round], []))) == n_seq for r in range(done_at))
    # equal sequences, one pass each step
    assert plan_seq_batch([0] * width, [3] * width, width) == [list(range(width))] * 3
    # a sequence whose prompt already fills its total never enters a lane
    assert plan_seq_batch([5, 0], [5, 2], width) == [[1], [1]]


def test_plan_seq_batch_rejects_bad_arguments(lib):
    n = C.c_int32(0)
    one = (C.c_int32 * 1)(0)
    tot = (C.c_int32 * 1)(4)
    out = (C.c_int32 * 64)()
    f = lib.kh_plan_seq_batch
    assert f(0, 8, one, tot, out, 8, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert f(65, 8, one, tot, out, 8, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert f(1, 0, one, tot, out, 8, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert f(1, 9, one, tot, out, 8, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert f(1, 8, None, tot, out, 8, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert f(1, 8, one, tot, out, 8, None) == _ffi.KH_ERR_INVALID_ARG
    assert f(1, 8, one, tot, out, 2, C.byref(n)) == _ffi.KH_ERR_RANGE and n.value == 4  # too small: the need
    assert f(1, 8, one, tot, out, 4, C.byref(n)) == 0 and n.value == 4
    assert list(out[:32:8]) == [0, 0, 0, 0] and out[1] == -1


# ---- validation before any device call ------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected_without_touching_the_device(lib):
    fake = C.c_void_p(0x1000)  # never dereferenced: these checks come first
    four = (C.c_int32 * 4)(1, 2, 3, 4)
    none = C.POINTER(C.c_int32)()
    w = C.c_int32(0)
    bad = _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_model_seq_slots(None, 2, C.byref(w)) == bad
    assert lib.kh_model_seq_width(None, C.byref(w)) == bad
    assert lib.kh_model_seq_width(fake, None) == bad
    assert lib.kh_model_seq_prefill(None, 0, four, 4, 0) == bad
    assert lib.kh_model_seq_prefill(fake, 0, none, 4, 0) == bad
    assert lib.kh_model_seq_prefill(fake, 0, four, 0, 0) == bad
    assert lib.kh_model_seq_prefill(fake, 0, four, 4, -1) == bad
    assert lib.kh_model_seq_fork(None, 0, 1, 4) == bad
    assert lib.kh_model_seq_fork(fake, 1, 1, 4) == bad   # onto itself
    assert lib.kh_model_seq_fork(fake, 0, 1, 0) == bad
    assert lib.kh_model_seq_step(None, 4, four, four, four, None, four) == bad
    assert lib.kh_model_seq_step(fake, 0, four, four, four, None, four) == bad
    assert lib.kh_model_seq_step(fake, 4, none, four, four, None, four) == bad
    assert lib.kh_model_seq_step(fake, 4, four, four, four, None, none) == bad
    ms = C.c_float(0)
    g = lib.kh_model_generate_batch
    assert g(None, 1, four, four, four, None, None, 0, four, 4, four, C.byref(ms)) == bad
    assert g(fake, 0, four, four, four, None, None, 0, four, 4, four, C.byref(ms)) == bad
    assert g(fake, 1, none, four, four, None, None, 0, four, 4, four, C.byref(ms)) == bad
    assert g(fake, 1, four, four, four, None, None, 0, none, 4, four, C.byref(ms)) == bad
    assert g(fake, 1, four, four, four, None, None, 0, four, 0, four, C.byref(ms)) == bad   # no room for words
    assert g(fake, 1, four, four, four, None, None, 2, four, 4, four, C.byref(ms)) == bad   # stops without a list


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
def test_wrappers_reject_ragged_arguments_before_the_library():
    m = KuiperModel.__new__(KuiperModel)  # a null handle: the library would refuse it, the wrappers never get there
    m._h, m._keep, m.spec = C.c_void_p(), None, S.SPECS["a"]
    try:
        with pytest.raises(ValueError):
            m.seq_step([0, 1], [5], [0, 0])
        with pytest.raises(ValueError):
            m.seq_step([0, 1], [5, 6], [0])
        with pytest.raises(ValueError):
            m.seq_step([0, 1], [5, 6], [0, 0], samplings=[None])
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], [8])
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], [8, 8, 8])
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], []], 8)
        with pytest.raises(ValueError):
            m.generate_batch([], 8)
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], 8, samplings=[{"temperature": 0.8}])
        with pytest.raises(ValueError):
            m.generate_batch([[1, 2], [3]], 8, cached=[1])
        with pytest.raises(ValueError):
            plan_seq_batch([0, 0], [4], 8)
        # well-formed arguments do reach the library, which refuses the null model
        with pytest.raises(_ffi.KhError) as ei:
            m.generate_batch([[1, 2], [3]], 8, samplings=[{"temperature": 0.8, "seed": 3}, None])
        assert ei.value.code == _ffi.KH_ERR_INVALID_ARG
    finally:
        m.close()  # nothing to destroy
