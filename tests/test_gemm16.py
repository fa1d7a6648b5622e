"""GEMM16 (KH_FLAG_GEMM16), host side: the three-term bf16 split of the activations (tests/split3_ref.py states what
csrc/kh_gemm_w16.h::pg_split3 computes), the class plan of a geometry (kh_plan_gemm16) and the ABI.  No GPU.
Every test here fails on a library without the feature."""
import numpy as np
import pytest

import gemm16_cases as g16
import split3_ref as s3
from kuiperllama_amd import _ffi, build

# the classes kh_plan_gemm16 / kh_plan_gemm16_f16 adopt where their contraction length is a multiple of 32
# (csrc/kh_model_w16.hip: KH_GEMM16_DEFAULT, from profiles/gemm16_ab.txt; KH_GEMM16_F16_DEFAULT = 0, from
# profiles/gemm16_f16_ab.txt: the adoption rule keeps no class)
DEFAULT = {g16.W16: ("qkv", "wo", "ffn13", "w2"), g16.H16: ()}


def _values(rng, n, lo_exp, hi_exp):
    """n fp32 values with full 24-bit significands and exponents uniform in [lo_exp, hi_exp], both signs."""
    m = rng.integers(1 << 23, 1 << 24, n).astype(np.float64)
    e = rng.integers(lo_exp, hi_exp + 1, n).astype(np.float64)
    s = rng.choice([-1.0, 1.0], n)
    return (s * m * np.exp2(e - 23)).astype(np.float32)


def test_split3_reconstructs_and_is_bf16_exact():
    rng = np.random.default_rng(5)
    x = np.concatenate([_values(rng, 1 << 20, -100, 100),
                        np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0, -1.0, 2.0 ** -100,
                                  1.0 + 2.0 ** -23, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -16, 3.0 - 2.0 ** -22], np.float32)])
    assert np.all(np.abs(x) >= np.float32(2.0 ** -100))
    hi, mid, lo = s3.split3(x)
    # exact reconstruction, in fp32 and in either order of the additions
    assert np.array_equal((hi + mid) + lo, x) and np.array_equal(hi + (mid + lo), x)
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))
    for name, part in (("hi", hi), ("mid", mid), ("lo", lo)):
        assert s3.is_bf16(part).all(), name
    # the parts do not overlap: each is below one unit of the last bf16 place of the one before
    assert np.all(np.abs(mid) < np.abs(hi) * np.float32(2.0 ** -7))
    assert np.all(np.abs(lo) <= np.abs(hi) * np.float32(2.0 ** -15))
    # what the kernel packs is the three parts
    for part, bits in zip((hi, mid, lo), s3.packed_upper_halves(x)):
        assert np.array_equal((bits.astype(np.uint32) << np.uint32(16)).view(np.float32), part)
    # two terms are not enough: hi + mid keeps 16 significand bits
    assert np.any(hi + mid != x)


def test_split3_zeros_and_subnormal_neighbourhood():
    z = np.array([0.0, -0.0], np.float32)
    hi, mid, lo = s3.split3(z)
    assert hi.view(np.uint32).tolist() == [0, 0x80000000]  # hi keeps the sign of a zero
    assert mid.view(np.uint32).tolist() == [0, 0] and lo.view(np.uint32).tolist() == [0, 0]  # x - x = +0
    # below 2^-100 the sum still reconstructs (fp32 subtraction is exact down to the subnormals); only lo's
    # bf16-exactness can fail, once it is an fp32 subnormal
    rng = np.random.default_rng(6)
    x = _values(rng, 1 << 16, -149 + 23, -101)
    hi, mid, lo = s3.split3(x)
    assert np.array_equal((hi + mid) + lo, x)
    assert s3.is_bf16(hi).all() and s3.is_bf16(mid[np.abs(mid) >= np.float32(2.0 ** -126)]).all()


def _check_plan_masks(core):
    """kh_plan_gemm16 / kh_plan_gemm16_f16 (csrc/kh_model_w16.hip: plan_gemm16_copy): the core's adoption mask among the
    classes whose contraction length 32 divides - qkv, wo, ffn13 and cls contract over dim, w2 over hidden_dim - on an
    fp32 geometry whose dim, hidden_dim and kv_dim 16 divides; nothing elsewhere."""
    build.build_lib()
    default, fn = DEFAULT[core], getattr(_ffi, core.plan)

    def want(dim, hidden):
        ok = {"qkv": dim % 32 == 0, "wo": dim % 32 == 0, "ffn13": dim % 32 == 0, "w2": hidden % 32 == 0,
              "cls": dim % 32 == 0}
        return [c for c in _ffi.KH_W16_CLASSES if c in default and ok[c]]

    # (dim, hidden, kv_dim, vocab): the geometries of tests/test_gemm16_gpu.py, then ones the flag does nothing on
    for dim, hidden, kv, vocab in ((1024, 2816, 256, 1008), (1024, 1536, 1024, 784), (960, 1600, 160, 1536),
                                   (512, 912, 128, 1008), (2048, 8192, 512, 128256), (4096, 11008, 4096, 32000)):
        p = fn(dim, hidden, kv, vocab, False)
        assert p == {"classes": want(dim, hidden), "kblock": 32}, (dim, hidden, p)
    # hidden 912 = 28.5 blocks of 32: w2 alone keeps its fp32 kernel
    assert "w2" not in fn(512, 912, 128, 1008, False)["classes"]
    assert set(fn(512, 912, 128, 1008, False)["classes"]) == set(default) - {"w2"}
    # dim 336 = 10.5 blocks: only w2 could run (hidden 928 = 29 blocks)
    assert fn(336, 928, 48, 1008, False)["classes"] == [c for c in ("w2",) if c in default]
    assert fn(336, 912, 48, 1008, False)["classes"] == []
    assert fn(1024, 2816, 256, 1008, True)["classes"] == []   # int8
    assert fn(1000, 2816, 250, 1008, False)["classes"] == []  # not a GEMM-prefill geometry
    out = (_ffi._i64 * 2)()
    entry = getattr(_ffi.lib(), "kh_" + core.plan)
    assert entry(0, 128, 64, 37, 0, out) == _ffi.KH_ERR_INVALID_ARG
    assert entry(64, 128, 64, 37, 0, None) == _ffi.KH_ERR_INVALID_ARG


def test_plan_gemm16_masks():
    _check_plan_masks(g16.W16)


def test_plan_gemm16_f16_masks():
    _check_plan_masks(g16.H16)
    assert all(not DEFAULT[g16.H16] and _ffi.plan_gemm16_f16(d, h, kv, 1008, False)["classes"] == []
               for d, h, kv in ((1024, 2816, 256), (512, 912, 128), (336, 928, 48)))  # the flag acts through the hook alone


def test_gemm16_symbols_are_in_the_abi():
    g16.check_abi(g16.W16, 128, 9)
    assert not _ffi.KH_FLAG_GEMM16 & (_ffi.KH_FLAG_W16 | _ffi.KH_FLAG_W16_F16 | _ffi.KH_FLAG_Q4)
    assert _ffi.lib().kh_gemm_w16_f32(None, None, None, 1, 16, 32, 16, None) == _ffi.KH_ERR_INVALID_ARG


def test_gemm16_f16_symbols_are_in_the_abi():
    g16.check_abi(g16.H16, 1024, 9)
    assert _ffi.lib().kh_gemm_h16_f32(None, None, None, 1, 16, 32, 16, None) == _ffi.KH_ERR_INVALID_ARG


def test_gemm16_kernels_in_the_code_objects():
    """The three stems are compiled for exactly the register tiles and epilogues of the stems they stand in for, and
    none of them uses scratch."""
    g16.check_code_objects(g16.W16)


def test_gemm16_f16_kernels_in_the_code_objects():
    """... without the (2,8) register tile: 9 k_pg_gemm_h16, 3 k_rg_gemm_h16, 12 k_sg_gemm_h16."""
    assert [len(v) for v in g16.compiled_kernels(g16.H16).values()] == [9, 3, 12]
    g16.check_code_objects(g16.H16)


# ---- the harness's own gates (tests/gemm16_cases.py), on made-up launch logs ----------------------------------------
def _log(core, classes):
    """what a prefill of a model whose classes are `classes` launches, at tile (2,4)"""
    return {(core.stems[0] if c in classes else "k_pg_gemm") + "<%s2,4,%d>" % ("" if c in classes else "false,", g16.EPI_OF[c])
            for c in ("qkv", "wo", "ffn13", "w2")} | {"k_pg_attn<64,4,1>"}


def test_check_stems_rejects_the_wrong_stem():
    for core in (g16.W16, g16.H16, g16.Q16):
        g16.check_stems(core, "as planned", _log(core, ["qkv", "ffn13"]), ["qkv", "ffn13"])
        g16.check_stems(core, "all", _log(core, g16.ALL), g16.ALL)
        with pytest.raises(AssertionError):  # an old stem for an adopted class
            g16.check_stems(core, "old stem", _log(core, ["qkv"]), ["qkv", "ffn13"])
        with pytest.raises(AssertionError):  # a new stem for a class outside the mask
            g16.check_stems(core, "new stem", _log(core, ["qkv", "wo", "ffn13"]), ["qkv", "ffn13"])
    for core in (g16.H16, g16.Q16):
        with pytest.raises(AssertionError):  # a W16 kernel under another core
            g16.check_stems(core, "w16 name", _log(core, g16.ALL) | {"k_pg_gemm_w16<2,4,0>"}, g16.ALL)
    g16.check_stems(g16.W16, "w16 name", _log(g16.W16, g16.ALL) | {"k_pg_gemm_w16<2,4,0>"}, g16.ALL)


def test_coverage_reports_a_kernel_never_launched():
    pg, rg, sg = g16.H16.stems
    compiled = {f"{pg}<2,4,0>", f"{pg}<2,2,0>", f"{rg}<2,4,0>", f"{sg}<1,4,3>"}
    (_, comp, got), *rest = g16.coverage(g16.H16.stems, compiled, compiled - {f"{pg}<2,2,0>"})
    assert comp - got == {f"{pg}<2,2,0>"} and all(c == g for _, c, g in rest)
    with pytest.raises(AssertionError):  # a launched name the library does not hold
        g16.coverage(g16.H16.stems, compiled, compiled | {f"{sg}<2,8,3>"})
    with pytest.raises(AssertionError):  # a stem the library does not hold at all
        g16.coverage(g16.H16.stems, compiled - {f"{rg}<2,4,0>"}, set())


def test_check_lane_bounds_and_first_maximum():
    floor = 2e-5
    g64 = np.array([0.0, 1.0, 3.0, 3.0, -2.0])  # two equal maxima: the first one is the pick
    g32 = g64 + np.array([0, 0, 0, 0, 4e-6])    # e32 = 4e-6: the bound is floor + e32 (3 e32 is below it)
    lim = max(floor + 4e-6, 3 * 4e-6)
    lg = (g64 + np.array([0, 0.9 * lim, 0, 0, 0])).astype(np.float64)
    assert g16.check_lane(lg, 2, g64, g32, floor, "inside") == pytest.approx(0.9 * lim)
    with pytest.raises(AssertionError):  # just above max(floor + e32, 3 e32)
        g16.check_lane(g64 + np.array([0, 1.01 * lim, 0, 0, 0]), 2, g64, g32, floor, "error")
    with pytest.raises(AssertionError):  # the second of two equal maxima
        g16.check_lane(lg, 3, g64, g32, floor, "pick")
    e32 = 2e-5  # where 3 e32 = 6e-5 exceeds floor + e32 = 4e-5 it is the bound
    g32 = g64 + np.array([0, 0, 0, 0, e32])
    g16.check_lane(g64 + np.array([0, 5.9e-5, 0, 0, 0]), 2, g64, g32, floor, "3 e32")
    with pytest.raises(AssertionError):
        g16.check_lane(g64 + np.array([0, 6.1e-5, 0, 0, 0]), 2, g64, g32, floor, "3 e32")
    with pytest.raises(AssertionError):  # a pick that is no maximum of the row at all
        g16.check_lane(g64, 1, g64, g32, floor, "pick")
