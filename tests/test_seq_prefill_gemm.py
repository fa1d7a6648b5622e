"""The GEMM prefill into sequence slots on the CPU (csrc/kh_seq_prefill.h, kh_model_seq_prefill_gemm): the host plan
against a Python twin, the binding, and the argument checks that need no device.  The GPU half is
test_seq_prefill_gemm_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from kuiperllama_amd import _ffi, build, model
from kuiperllama_amd.model import KuiperModel

TILES = 32  # KH_RG_TILES: token tiles of 16 per pass


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def plan_twin(n_tokens):
    """kh_seq_plan.h: kh_rg_plan, in Python.  Segments in call order; one that fits in what is left of the pass is
    placed whole, else its first 16 x free tokens fill the pass (if a tile is free) and the rest continues."""
    runs, p, used = [], 0, 0
    for s, n in enumerate(n_tokens):
        off = 0
        while off < n:
            if used == TILES:
                p, used = p + 1, 0
            take = min(n - off, 16 * (TILES - used))
            runs.append((p, s, off, take))
            used += -(-take // 16)
            off += take
    return runs


HAND = {
    (1,): [(0, 0, 0, 1)],
    (16,): [(0, 0, 0, 16)],
    (17,): [(0, 0, 0, 17)],
    (512,): [(0, 0, 0, 512)],
    (513,): [(0, 0, 0, 512), (1, 0, 512, 1)],
    # pass 0: segment 0 whole (19 tiles) and 13 tiles = 208 tokens of segment 1; pass 1: its other 92 and segment 2
    (300, 300, 300): [(0, 0, 0, 300), (0, 1, 0, 208), (1, 1, 208, 92), (1, 2, 0, 300)],
}


@pytest.mark.parametrize("lens", sorted(HAND))
def test_plan_hand_cases(lib, lens):
    assert model.plan_seq_prefill_gemm(lens) == HAND[lens] == plan_twin(lens)


def test_plan_64_prompts_of_8(lib):
    """a tile belongs to one segment: 64 segments of 8 tokens are 64 tiles, two passes of 32"""
    got = model.plan_seq_prefill_gemm([8] * 64)
    assert got == [(s // 32, s, 0, 8) for s in range(64)] == plan_twin([8] * 64)
    assert KuiperModel.plan_seq_prefill_gemm([8] * 64) == got  # the model's name for it


def test_plan_random_lists(lib):
    """the runs cover every token of every segment once, in order, with at most 32 tiles per pass, passes in order"""
    rng = np.random.default_rng(11)
    for _ in range(200):
        lens = [int(n) for n in rng.integers(1, rng.choice([9, 40, 700]), rng.integers(1, 65))]
        runs = model.plan_seq_prefill_gemm(lens)
        assert runs == plan_twin(lens), lens
        at, tiles = [0] * len(lens), {}
        last = (0, 0)
        for p, s, off, n in runs:
            assert n > 0 and off == at[s] and (p, s) >= last, (lens, p, s, off, n)
            last = (p, s)
            at[s] += n
            tiles[p] = tiles.get(p, 0) + -(-n // 16)
            # a run that does not end its segment fills its pass with whole tiles
            assert at[s] == lens[s] or (n % 16 == 0 and tiles[p] == TILES), (lens, p, s, off, n)
        assert at == lens and max(tiles.values()) <= TILES, lens
        assert sorted(tiles) == list(range(len(tiles))), lens
        n_runs, n_passes = C.c_int32(0), C.c_int32(0)
        assert lib.kh_plan_seq_prefill_gemm(len(lens), model._i32_array(lens), None, 0, C.byref(n_runs),
                                            C.byref(n_passes)) == _ffi.KH_ERR_RANGE
        assert (n_runs.value, n_passes.value) == (len(runs), len(tiles))


def test_symbols_and_signatures(lib):
    i32, p32 = C.c_int32, C.POINTER(C.c_int32)
    assert {"kh_plan_seq_prefill_gemm", "kh_model_seq_prefill_gemm"} <= set(_ffi.EXPORTS)
    assert lib.kh_plan_seq_prefill_gemm.argtypes == [i32, p32, p32, i32, p32, p32]
    assert lib.kh_model_seq_prefill_gemm.argtypes == [C.c_void_p, i32, p32, p32, p32, p32]


def test_argument_checks_that_need_no_device(lib):
    n = C.c_int32(0)
    one = model._i32_array([4])
    out = (C.c_int32 * 4)()
    assert lib.kh_plan_seq_prefill_gemm(0, one, out, 1, C.byref(n), None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_prefill_gemm(1, None, out, 1, C.byref(n), None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_prefill_gemm(1, one, out, 1, None, None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_prefill_gemm(1, one, None, 1, C.byref(n), None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_prefill_gemm(1, model._i32_array([0]), out, 1, C.byref(n), None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_plan_seq_prefill_gemm(1, one, out, 1, C.byref(n), None) == 0 and list(out) == [0, 0, 0, 4]
    assert lib.kh_model_seq_prefill_gemm(None, 1, one, one, one, one) == _ffi.KH_ERR_INVALID_ARG
    with pytest.raises(_ffi.KhError):
        model.plan_seq_prefill_gemm([])
    m = KuiperModel.__new__(KuiperModel)  # the wrapper refuses these before it touches its handle
    for bad in (dict(slots=[0, 1], prompts=[[1]]), dict(slots=[0], prompts=[[1]], pos0=[0, 0]),
                dict(slots=[], prompts=[]), dict(slots=[0], prompts=[[]])):
        with pytest.raises(ValueError):
            m.seq_prefill_many(**bad)
    with pytest.raises(ValueError):
        m.seq_prefill(0, [], gemm=True)
