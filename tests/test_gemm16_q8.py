"""GEMM16_Q8 (KH_FLAG_GEMM16_Q8), host side: the arithmetic csrc/kh_gemm_q16.h::pg_kloop_q16 relies on (stated in
tests/gemm_q16_ref.py), the class plan of a geometry (kh_plan_gemm16_q8) and the ABI.  No GPU.
The plan, ABI and code-object tests fail on a library without the feature; the first three state the arithmetic in numpy
alone."""
import os

import numpy as np

import code_objects as co
import gemm_q16_ref as ref
import split3_ref as s3
from kuiperllama_amd import _ffi, build

# the classes kh_plan_gemm16_q8 adopts (csrc/kh_model_gemm_q16.hip: KH_GEMM16_Q8_DEFAULT, from profiles/gemm16_q8_ab.txt)
DEFAULT = ["qkv", "wo", "ffn13", "w2"]


def test_every_int8_value_is_its_own_bf16():
    q = np.arange(-128, 128).astype(np.int8)
    f = q.astype(np.float32)
    assert s3.is_bf16(f).all()  # nothing below the upper 16 bits: taking them rounds nothing
    back = ref.bf16_bits_to_f32(ref.int8_to_bf16_bits(q))
    assert np.array_equal(back, f) and np.array_equal(back.astype(np.int64), np.arange(-128, 128))
    assert len(set(ref.int8_to_bf16_bits(q).tolist())) == 256


def test_the_two_steps_cover_each_column_of_a_group_once():
    a = [ref.a_columns(s) for s in (0, 1)]
    for i in range(16):  # the four lanes i, 16 + i, 32 + i, 48 + i of a weight row (a token) share out its group
        allc = np.concatenate([c[i::16].ravel() for c in a])
        assert sorted(allc.tolist()) == list(range(64)), i
    for s in (0, 1):
        # the activation the B operand holds at a k index is the one of the weight's column, from the tiled slab
        assert np.array_equal(ref.b_columns(s), a[s]), s
        assert np.array_equal(ref.b_columns(s, tcap=512, token=300, block=0), a[s]), s
        # the lanes of one quarter h share the k range 8h .. 8h + 7 of the MFMA; a lane's bytes are 8s .. 8s + 7 of its 16
        lane = np.arange(64)
        assert np.array_equal(a[s][:, 0], 16 * (lane >> 4) + 8 * s)
        assert np.all(np.diff(a[s], axis=1) == 1)


def test_split3_terms_times_int8_are_exact_in_fp32():
    rng = np.random.default_rng(7)
    m = rng.integers(1 << 23, 1 << 24, 1 << 16).astype(np.float64)
    x = (rng.choice([-1.0, 1.0], m.size) * m * np.exp2(rng.integers(-40, 41, m.size) - 23.0)).astype(np.float32)
    q = rng.integers(-128, 128, m.size).astype(np.int8)
    q[:4] = (-128, 127, -127, 1)
    w = ref.bf16_bits_to_f32(ref.int8_to_bf16_bits(q))
    total = np.zeros(m.size, np.float64)
    for part in s3.split3(x):
        p32 = part * w  # fp32 product
        assert np.array_equal(p32.astype(np.float64), part.astype(np.float64) * w.astype(np.float64))
        total += p32.astype(np.float64)
    assert np.array_equal(total, x.astype(np.float64) * q.astype(np.float64))  # the three terms carry all of q * x


def test_plan_gemm16_q8_masks():
    build.build_lib()
    # (dim, hidden, kv_dim, vocab): the geometries of tests/test_gemm16_q8_gpu.py, then full-size ones
    for dim, hidden, kv, vocab in ((1024, 2816, 256, 1008), (1024, 1536, 256, 784), (384, 1024, 48, 1008),
                                   (2048, 5632, 256, 32000), (4096, 11008, 4096, 32000)):
        p = _ffi.plan_gemm16_q8(dim, hidden, kv, vocab, True)
        assert p == {"classes": DEFAULT, "kblock": 64}, (dim, hidden, p)
        assert _ffi.plan_gemm16_q8(dim, hidden, kv, vocab, True, 64) == p
    assert _ffi.plan_gemm16_q8(1024, 2816, 256, 1008, False)["classes"] == []       # fp32
    assert _ffi.plan_gemm16_q8(1024, 2816, 256, 1008, True, 128)["classes"] == []   # group 128
    assert _ffi.plan_gemm16_q8(1024, 2816, 256, 1008, True, 32)["classes"] == []
    assert _ffi.plan_gemm16_q8(1000, 2816, 250, 1008, True)["classes"] == []        # not a GEMM-prefill geometry
    assert _ffi.plan_gemm16_q8(1024, 2800, 256, 1008, True)["classes"] == []        # hidden is no multiple of 64
    # KH_FLAG_GEMM16's own plan is untouched: empty on int8
    assert _ffi.plan_gemm16(1024, 2816, 256, 1008, True)["classes"] == []
    out = (_ffi._i64 * 2)()
    assert _ffi.lib().kh_plan_gemm16_q8(0, 128, 64, 37, 1, 64, out) == _ffi.KH_ERR_INVALID_ARG
    assert _ffi.lib().kh_plan_gemm16_q8(64, 128, 64, 0, 1, 64, out) == _ffi.KH_ERR_INVALID_ARG
    assert _ffi.lib().kh_plan_gemm16_q8(64, 128, 64, 37, 1, -1, out) == _ffi.KH_ERR_INVALID_ARG
    assert _ffi.lib().kh_plan_gemm16_q8(64, 128, 64, 37, 1, 64, None) == _ffi.KH_ERR_INVALID_ARG


def test_gemm16_q8_symbols_are_in_the_abi():
    build.build_lib()
    L = _ffi.lib()
    for n in ("kh_model_gemm16_q8_info", "kh_plan_gemm16_q8", "kh_gemm_q8_bf16_f32"):
        assert n in _ffi.EXPORTS and hasattr(L, n)
    assert _ffi.KH_FLAG_GEMM16_Q8 == 256
    others = [v for k, v in vars(_ffi).items() if k.startswith("KH_FLAG_") and k != "KH_FLAG_GEMM16_Q8"]
    assert len(others) >= 8 and not any(_ffi.KH_FLAG_GEMM16_Q8 & v for v in others), others
    src = open(os.path.join(build.CSRC, "..", "..", "include", "kuiper_hip.h")).read()
    assert "#define KH_FLAG_GEMM16_Q8 256" in src
    for decl in ("int kh_model_gemm16_q8_info(", "int kh_plan_gemm16_q8(", "int kh_gemm_q8_bf16_f32("):
        assert decl in src, decl
    assert L.kh_model_gemm16_q8_info(None, None) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_gemm_q8_bf16_f32(None, None, None, None, 1, 16, 64, 16, None) == _ffi.KH_ERR_INVALID_ARG
    for hook in ("KH_GEMM16_Q8", "KH_GEMM16_Q8_CLASSES"):
        assert hook.startswith(_ffi._HOOK_PREFIXES)  # sync_env mirrors it from the environment
        assert _ffi.debug_get(hook) is None
        try:
            _ffi.debug_set(hook, "1")
            assert _ffi.debug_get(hook) == "1"
        finally:
            _ffi.debug_set(hook, None)
    lib_src = open(os.path.join(build.CSRC, "kh_model_gemm_q16.hip")).read()
    assert 'dbg("KH_GEMM16_Q8")' in lib_src and 'dbg("KH_GEMM16_Q8_CLASSES")' in lib_src
    from kuiperllama_amd import ops
    from kuiperllama_amd.model import KuiperModel
    assert callable(KuiperModel.gemm16_q8_info) and callable(ops.gemm_q8_bf16)
    assert len(_ffi.KH_GEMM16_Q8_REASONS) == 6 and len(_ffi.KH_GEMM16_REASONS) == 9
    assert "kh_model_gemm_q16.hip" in build.SOURCES and "kh_gemm_q16.h" in build.HEADERS


def test_gemm16_q8_kernels_in_the_code_objects():
    """The three stems are compiled for the register tiles they take - the int8 stem's without (2,8) - and the
    epilogues of the stems they stand in for, and none of them uses scratch."""
    if not co.tools_present():
        import pytest
        pytest.skip("LLVM tools of the ROCm install not found")
    notes = co.code_object_notes(build.build_lib())
    tiles = ((2, 4), (2, 2), (1, 4))
    want = {
        "k_pg_gemm_q16": {f"k_pg_gemm_q16<{r},{nt},{e}>" for r, nt in tiles for e in (0, 1, 2)},
        "k_rg_gemm_q16": {f"k_rg_gemm_q16<{r},{nt},0>" for r, nt in tiles},
        "k_sg_gemm_q16": {f"k_sg_gemm_q16<{r},{nt},{e}>" for r, nt in tiles for e in (0, 1, 2, 3)},
    }
    for stem, w in want.items():
        got = co.instantiations(notes, {stem})
        assert got == w, (stem, sorted(got - w), sorted(w - got))
    scratch = {k: v for k, v in co.kernel_scratch(notes).items() if "_gemm_q16" in k and v}
    assert not scratch, scratch
