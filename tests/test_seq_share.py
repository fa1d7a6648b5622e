"""Slots of unequal length and a shared prompt prefix, CPU side: the partition (kh_plan_seq_slots_var) against a Python
statement of it, the layout planner of best_of(share=True), the equal partition unchanged, and argument validation
before any device call.  The symbol test needs what the feature adds."""
import ctypes as C

import pytest

from kuiperllama_amd import _ffi, build
from kuiperllama_amd.model import plan_seq_slots, plan_seq_slots_var, plan_shared_layout

NEW = ["kh_model_seq_slots_var", "kh_plan_seq_slots_var", "kh_model_seq_share", "kh_model_seq_row"]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def test_symbols_are_exported(lib):
    for name in NEW:
        assert name in _ffi.EXPORTS and hasattr(lib, name), name


def _i32(v):
    return (C.c_int32 * max(len(v), 1))(*v)


def _partition(cache_len, lens):
    """the stated rule: 1 <= n <= 64 slots of at least 8 rows whose sum fits the cache, slot 0 from row 0, no gaps"""
    if not 1 <= len(lens) <= 64 or any(n < 8 for n in lens) or sum(lens) > cache_len:
        return None
    return [sum(lens[:s]) for s in range(len(lens))]


CASES = [
    (64, [64]), (64, [8] * 8), (64, [8] * 9), (64, [7, 8]), (64, [8, 7]), (64, [56, 8]), (64, [57, 8]), (64, [0]),
    (64, [-8, 80]), (4096, [3000 + 128] + [128] * 7), (4096, [3128] + [139] * 7), (4096, [8] * 64), (4096, [8] * 65),
    (640, [330, 8, 8, 31, 8, 100]), (320, [40] * 8), (8, [8]), (7, [8]), (2 ** 31 - 1, [2 ** 30, 2 ** 30 - 1]),
    (2 ** 31 - 1, [2 ** 30, 2 ** 30]),  # a sum past int32 is refused, not wrapped
]


def test_plan_seq_slots_var_is_the_stated_partition(lib):
    for cache_len, lens in CASES:
        want = _partition(cache_len, lens)
        row0 = (C.c_int32 * 65)(*([-5] * 65))
        rc = lib.kh_plan_seq_slots_var(cache_len, len(lens), _i32(lens), row0)
        if want is None:
            assert rc == _ffi.KH_ERR_INVALID_ARG, (cache_len, lens)
            assert all(r == -5 for r in row0), "a refused call writes nothing"
            with pytest.raises(_ffi.KhError):
                plan_seq_slots_var(cache_len, lens)
        else:
            assert rc == 0 and list(row0[:len(lens)]) == want, (cache_len, lens)
            assert row0[len(lens)] == -5
            assert plan_seq_slots_var(cache_len, lens) == want
            assert want[0] == 0 and want[-1] + lens[-1] <= cache_len
    assert lib.kh_plan_seq_slots_var(64, 0, _i32([]), None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_slots_var(64, 2, None, None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_slots_var(64, 2, _i32([8, 8]), None) == 0  # no out pointer
    assert lib.kh_plan_seq_slots_var(0, 1, _i32([8]), None) == _ffi.KH_ERR_INVALID_ARG


def test_the_equal_partition_is_a_case_of_it(lib):
    out = C.c_int32(0)
    for cache_len, n in ((320, 8), (64, 4), (1280, 4), (4096, 8), (131072, 64), (65, 8)):
        assert lib.kh_plan_seq_slots(cache_len, n, C.byref(out)) == 0 and out.value == cache_len // n
        assert plan_seq_slots_var(cache_len, [out.value] * n) == [s * out.value for s in range(n)]
    assert plan_seq_slots(320, 8) == 40 and plan_seq_slots(64, 4) == 16  # unchanged
    for cache_len, n in ((64, 9), (64, 0), (64, 65)):
        assert lib.kh_plan_seq_slots(cache_len, n, C.byref(out)) == _ffi.KH_ERR_INVALID_ARG


def test_plan_shared_layout():
    # the issue's example: 3000 prompt positions sampled 8 times, 128 more positions each, in 4096 rows
    lens = plan_shared_layout(4096, 8, 3000, 3128)
    assert lens == [3128] + [128] * 7 and sum(lens) == 3000 + 8 * 128
    assert plan_seq_slots_var(4096, lens)[1] == 3128
    assert plan_seq_slots(4096, 8) == 512 < 3128  # no equal partition into 8 holds one such sequence
    # unequal totals; a sharer that adds fewer than 8 positions still owns 8 rows
    assert plan_shared_layout(640, 4, 200, [230, 201, 330, 208]) == [230, 8, 130, 8]
    assert plan_shared_layout(64, 1, 0, 20) == [20]
    assert plan_shared_layout(64, 2, 0, 3) == [8, 8]
    for bad in ((640, 4, 200, 400), (640, 4, 200, [230, 201, 330]), (640, 0, 0, 8), (640, 2, 30, 20),
                (640, 2, -1, 20), (4096, 65, 1, 9)):
        with pytest.raises(ValueError):
            plan_shared_layout(*bad)
    # 4 x 310 positions: 1240 rows as copies (an equal slot of this cache holds 160), 640 with the prefix shared
    assert sum(plan_shared_layout(640, 4, 200, 310)) == 310 + 3 * 110 == 640 and plan_seq_slots(640, 4) == 160 < 310


def test_invalid_arguments_are_rejected_without_touching_the_device(lib):
    fake = C.c_void_p(0x1000)  # never dereferenced: these checks come first
    bad = _ffi.KH_ERR_INVALID_ARG
    row = C.c_int32(0)
    assert lib.kh_model_seq_slots_var(None, 1, _i32([8])) == bad
    assert lib.kh_model_seq_share(None, 0, 1, 4) == bad
    assert lib.kh_model_seq_share(fake, 1, 1, 4) == bad   # onto itself
    assert lib.kh_model_seq_share(fake, 0, 1, -1) == bad
    assert lib.kh_model_seq_share(fake, 1, 0, 4) == bad   # slot 0 never shares
    assert lib.kh_model_seq_row(None, 0, 0, C.byref(row)) == bad
    assert lib.kh_model_seq_row(fake, 0, 0, None) == bad
