"""GEMM16 (KH_FLAG_GEMM16), host side: the three-term bf16 split of the activations (tests/split3_ref.py states what
csrc/kh_gemm_w16.h::pg_split3 computes), the class plan of a geometry (kh_plan_gemm16) and the ABI.  No GPU.
Every test here fails on a library without the feature."""
import os

import numpy as np

import code_objects as co
import split3_ref as s3
from kuiperllama_amd import _ffi, build

# the classes kh_plan_gemm16 adopts where their contraction length is a multiple of 32 (csrc/kh_model_w16.hip:
# KH_GEMM16_DEFAULT, from profiles/gemm16_ab.txt)
DEFAULT = ("qkv", "wo", "ffn13", "w2")


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


def test_plan_gemm16_masks():
    build.build_lib()

    def want(dim, hidden):
        ok = {"qkv": dim % 32 == 0, "wo": dim % 32 == 0, "ffn13": dim % 32 == 0, "w2": hidden % 32 == 0,
              "cls": dim % 32 == 0}
        return [c for c in _ffi.KH_W16_CLASSES if c in DEFAULT and ok[c]]

    # (dim, hidden, kv_dim, vocab): the geometries of tests/test_gemm16_gpu.py, then ones the flag does nothing on
    for dim, hidden, kv, vocab in ((1024, 2816, 256, 1008), (1024, 1536, 1024, 784), (960, 1600, 160, 1536),
                                   (512, 912, 128, 1008), (2048, 8192, 512, 128256), (4096, 11008, 4096, 32000)):
        p = _ffi.plan_gemm16(dim, hidden, kv, vocab, False)
        assert p == {"classes": want(dim, hidden), "kblock": 32}, (dim, hidden, p)
    # hidden 912 = 28.5 blocks of 32: w2 alone keeps its fp32 kernel
    assert "w2" not in _ffi.plan_gemm16(512, 912, 128, 1008, False)["classes"]
    assert set(_ffi.plan_gemm16(512, 912, 128, 1008, False)["classes"]) == set(DEFAULT) - {"w2"}
    # dim 336 = 10.5 blocks: only w2 could run (hidden 928 = 29 blocks)
    assert _ffi.plan_gemm16(336, 928, 48, 1008, False)["classes"] == [c for c in ("w2",) if c in DEFAULT]
    assert _ffi.plan_gemm16(336, 912, 48, 1008, False)["classes"] == []
    assert _ffi.plan_gemm16(1024, 2816, 256, 1008, True)["classes"] == []   # int8
    assert _ffi.plan_gemm16(1000, 2816, 250, 1008, False)["classes"] == []  # not a GEMM-prefill geometry
    out = (_ffi._i64 * 2)()
    assert _ffi.lib().kh_plan_gemm16(0, 128, 64, 37, 0, out) == _ffi.KH_ERR_INVALID_ARG
    assert _ffi.lib().kh_plan_gemm16(64, 128, 64, 37, 0, None) == _ffi.KH_ERR_INVALID_ARG


def test_gemm16_symbols_are_in_the_abi():
    build.build_lib()
    L = _ffi.lib()
    for n in ("kh_model_gemm16_info", "kh_plan_gemm16", "kh_gemm_w16_f32"):
        assert n in _ffi.EXPORTS and hasattr(L, n)
    assert _ffi.KH_FLAG_GEMM16 == 128
    assert not _ffi.KH_FLAG_GEMM16 & (_ffi.KH_FLAG_W16 | _ffi.KH_FLAG_W16_F16 | _ffi.KH_FLAG_Q4)
    src = open(os.path.join(build.CSRC, "..", "..", "include", "kuiper_hip.h")).read()
    assert "#define KH_FLAG_GEMM16 128" in src
    for decl in ("int kh_model_gemm16_info(", "int kh_plan_gemm16(", "int kh_gemm_w16_f32("):
        assert decl in src, decl
    assert L.kh_model_gemm16_info(None, None) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_gemm_w16_f32(None, None, None, 1, 16, 32, 16, None) == _ffi.KH_ERR_INVALID_ARG
    for hook in ("KH_GEMM16", "KH_GEMM16_CLASSES"):
        assert hook.startswith(_ffi._HOOK_PREFIXES)  # sync_env mirrors it from the environment
        assert _ffi.debug_get(hook) is None
        try:
            _ffi.debug_set(hook, "1")
            assert _ffi.debug_get(hook) == "1"
        finally:
            _ffi.debug_set(hook, None)
    from kuiperllama_amd import ops
    from kuiperllama_amd.model import KuiperModel
    assert callable(KuiperModel.gemm16_info) and callable(ops.gemm_w16)
    assert len(_ffi.KH_GEMM16_REASONS) == 9
    assert "kh_model_gemm_w16.hip" in build.SOURCES and "kh_gemm_w16.h" in build.HEADERS


def test_gemm16_kernels_in_the_code_objects():
    """The three stems are compiled for exactly the register tiles and epilogues of the stems they stand in for, and
    none of them uses scratch."""
    if not co.tools_present():
        import pytest
        pytest.skip("LLVM tools of the ROCm install not found")
    notes = co.code_object_notes(build.build_lib())
    tiles = ((2, 8), (2, 4), (2, 2), (1, 4))
    want = {
        "k_pg_gemm_w16": {f"k_pg_gemm_w16<{r},{nt},{e}>" for r, nt in tiles for e in (0, 1, 2)},
        "k_rg_gemm_w16": {f"k_rg_gemm_w16<{r},{nt},0>" for r, nt in tiles},
        "k_sg_gemm_w16": {f"k_sg_gemm_w16<{r},{nt},{e}>" for r, nt in tiles[1:] for e in (0, 1, 2, 3)},
    }
    for stem, w in want.items():
        got = co.instantiations(notes, {stem})
        assert got == w, (stem, sorted(got - w), sorted(w - got))
    scratch = {k: v for k, v in co.kernel_scratch(notes).items() if "_gemm_w16" in k and v}
    assert not scratch, scratch
