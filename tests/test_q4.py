"""Q4 (KH_FLAG_Q4), host side: the helpers that make and recognise a 4-bit-exact int8 image, the plan of the packed
4-bit weight copy, the ABI and the compiled kernel set.  CPU only.

binfmt.requantize_matrices_q4 is checked against a numpy float32 restatement of its rule (per group w = q * s,
s' = max|w| / 7, q' = rint(w / s'); a zero group keeps scale and zeros).
"""
import os

import numpy as np
import torch

import code_objects as co
import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt, build

TINY = dict(dim=64, hidden_dim=128, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=37, seq_len=16)
MATS = wc.MATRICES


def _spec(group=64, **kw):
    return binfmt.ModelSpec(**{**TINY, **kw}, shared_classifier=False, quant=True, group_size=group)


def _i8(img, e):
    return img[e.offset: e.offset + e.nbytes].view(np.int8)


def _f32(img, e):
    return img[e.offset: e.offset + e.nbytes].view(np.float32)


def test_covered_tensors():
    spec = _spec()
    ents = binfmt.q4_tensors(spec)
    assert [e.name for e, _ in ents] == [f"{n}.{l}" for l in range(2) for n in MATS] + ["wcls"]  # tensor-index order
    for e, s in ents:
        assert e.dtype == "i8" and s.name == e.name + ".scales" and s.shape == (e.nbytes // spec.group_size,)
    assert binfmt.q4_tensors(binfmt.ModelSpec(**TINY)) == []


def test_requantize_matches_the_numpy_statement_and_touches_nothing_else():
    for group in (64, 32):
        spec = _spec(group)
        img = binfmt.synth_image(spec, seed=3).numpy().copy()
        first, first_s = binfmt.q4_tensors(spec)[0]
        _i8(img, first)[group: 2 * group] = 0          # a zero group by its values ...
        _f32(img, first_s)[3] = 0.0                    # ... and one by its scale
        before = img.copy()
        got = binfmt.requantize_matrices_q4(img, spec)
        assert got is img
        covered = np.zeros(img.size, bool)
        for e, s in binfmt.q4_tensors(spec):
            covered[e.offset: e.offset + e.nbytes] = True
            covered[s.offset: s.offset + s.nbytes] = True
            q0 = _i8(before, e).reshape(-1, group).astype(np.float32)
            s0 = _f32(before, s)
            w = q0 * s0[:, None]
            wmax = np.abs(w).max(axis=1)
            live = wmax > 0
            s1 = np.where(live, wmax / np.float32(7), s0).astype(np.float32)
            q1 = np.rint(w / np.where(live, s1, np.float32(1))[:, None]).astype(np.int8)
            q, sc = _i8(img, e).reshape(-1, group), _f32(img, s)
            assert np.array_equal(sc.view(np.uint32), s1.view(np.uint32)), e.name
            assert np.array_equal(q, q1), e.name
            assert q.min() >= -7 and q.max() <= 7, e.name
            assert (np.abs(q).max(axis=1)[live] == 7).all(), e.name  # every live group uses the full range
        q, sc = _i8(img, first).reshape(-1, group), _f32(img, first_s)
        assert not q[1].any() and sc[1] == _f32(before, first_s)[1] != 0  # the zero group: its zeros, its scale
        assert not q[3].any() and sc[3] == 0
        assert np.array_equal(img[~covered], before[~covered]), "bytes outside the covered tensors changed"
        assert binfmt.matrices_q4_exact(img, spec)
        again = binfmt.requantize_matrices_q4(img.copy(), spec)
        assert binfmt.matrices_q4_exact(again, spec)


def test_requantize_on_a_torch_image():
    spec = _spec()
    img = binfmt.synth_image(spec, seed=3)
    want = binfmt.requantize_matrices_q4(img.numpy().copy(), spec)
    binfmt.requantize_matrices_q4(img, spec)
    assert np.array_equal(img.numpy(), want)
    assert binfmt.matrices_q4_exact(img, spec)


def test_matrices_q4_exact():
    spec = _spec()
    plain = binfmt.synth_image(spec, seed=3).numpy().copy()
    for e, _ in binfmt.q4_tensors(spec):  # the quantiser's scale is max|w| / 127: every non-zero group holds +-127
        assert (np.abs(_i8(plain, e).reshape(-1, 64).astype(np.int32)).max(axis=1) == 127).all()
    assert not binfmt.matrices_q4_exact(plain, spec)
    img = binfmt.requantize_matrices_q4(plain.copy(), spec)
    assert binfmt.matrices_q4_exact(img, spec)
    for e, _ in binfmt.q4_tensors(spec):  # -8 is a 4-bit value the requantiser never writes
        _i8(img, e)[[0, 1, e.nbytes - 2, e.nbytes - 1]] = -8
    assert binfmt.matrices_q4_exact(img, spec) and binfmt.matrices_q4_exact(torch.from_numpy(img), spec)
    last = binfmt.q4_tensors(spec)[-1][0]
    assert last.name == "wcls"
    for v in (8, -9, 127, -128):
        bad = img.copy()
        _i8(bad, last)[last.nbytes - 1] = v
        assert not binfmt.matrices_q4_exact(bad, spec), v
    # bytes outside the covered tensors do not matter: scales and tok_emb hold anything
    other = [e for e in binfmt.layout(spec)[0] if e.name == "tok_emb"][0]
    img[other.offset: other.offset + 64] = 0x7F
    assert binfmt.matrices_q4_exact(img, spec)
    fp32 = binfmt.ModelSpec(**TINY)
    assert not binfmt.matrices_q4_exact(binfmt.synth_image(fp32, seed=3).numpy(), fp32)


def test_plan_q4_bytes_and_classes():
    build.build_lib()

    def pad(n):
        return (n + 255) & ~255
    geoms = list(binfmt.PRESETS.values()) + [_spec(), _spec(32), _spec(dim=448, hidden_dim=1216, n_heads=7, n_kv_heads=7,
                                                                     vocab_size=999)]
    for spec in geoms:
        p = _ffi.plan_q4(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, spec.n_layers, spec.quant,
                         spec.group_size)
        if not spec.quant:
            assert p == {"classes": [], "bytes": 0}, spec.name  # nothing for fp32
            continue
        want = sum(pad(e.shape[0] * e.shape[1] // 2) for e, _ in binfmt.q4_tensors(spec))
        assert p["bytes"] == want > 0, (spec.name, p, want)
        assert set(p["classes"]) <= set(_ffi.KH_Q4_CLASSES), spec.name
    # a vocabulary that leaves wcls no multiple of 256 bytes: 999 * 448 / 2 = 223776 = 874 * 256 + 32
    assert pad(999 * 448 // 2) != 999 * 448 // 2
    llama = binfmt.PRESETS["llama2-7b-int8"]
    p = _ffi.plan_q4(llama.dim, llama.hidden_dim, llama.kv_dim, llama.vocab_size, llama.n_layers, True, 64)
    assert p["bytes"] * 2 == sum(e.nbytes for e, _ in binfmt.q4_tensors(llama))  # half the int8 matrix bytes
    # totals and the default classes of the library before W16 and Q4 shared their byte count (copy_bytes)
    assert _ffi.plan_q4(64, 64, 64, 1, 1, True, 64) == {"classes": ["ffn13", "w2", "cls"], "bytes": 14592}
    assert p == {"classes": ["ffn13", "w2", "cls"], "bytes": 3303538688}
    assert _ffi.plan_q4(72, 128, 72, 37, 2, True, 64) == {"classes": [], "bytes": 0}  # dim no multiple of the group
    assert _ffi.plan_q4(64, 128, 64, 37, 2, True, 8) == {"classes": [], "bytes": 0}   # a group below a lane's unit
    out = (_ffi._i64 * 2)()
    assert _ffi.lib().kh_plan_q4(0, 128, 64, 37, 2, 1, 64, out) == _ffi.KH_ERR_INVALID_ARG
    assert _ffi.lib().kh_plan_q4(64, 128, 64, 37, 2, 1, 64, None) == _ffi.KH_ERR_INVALID_ARG


def test_q4_symbols_are_in_the_abi():
    """Fails on a library without the feature: no such entry points."""
    build.build_lib()
    L = _ffi.lib()
    for n in ("kh_model_q4_info", "kh_plan_q4"):
        assert n in _ffi.EXPORTS and hasattr(L, n)
    assert _ffi.KH_FLAG_Q4 == 64
    assert _ffi.KH_Q4_CLASSES == ("qkv", "wo", "ffn13", "w2", "cls")
    src = open(os.path.join(build.CSRC, "..", "..", "include", "kuiper_hip.h")).read()
    assert "#define KH_FLAG_Q4 64" in src and "int kh_model_q4_info(" in src and "int kh_plan_q4(" in src
    assert L.kh_model_q4_info(None, None) == _ffi.KH_ERR_INVALID_ARG
    for hook in ("KH_Q4", "KH_Q4_CLASSES"):
        assert hook.startswith(_ffi._HOOK_PREFIXES)  # sync_env mirrors it from the environment
        assert _ffi.debug_get(hook) is None
        with wc.hook(hook, "1"):
            assert _ffi.debug_get(hook) == "1"
    from kuiperllama_amd.model import KuiperModel
    assert callable(KuiperModel.q4_info)
    assert "kh_model_q4.hip" in build.SOURCES and "kh_q4.h" in build.HEADERS


def test_q4_kernels_in_the_code_objects():
    """The five _q4 stems are compiled for exactly the int8 lists of their twins - 89 instantiations, none with
    scratch - and the int8 / fp32 / W16 sets are what they were."""
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    notes = co.code_object_notes(build.build_lib())
    Q = (("false", (8, 4, 2)), ("true", (4, 2)))
    base = {
        "k_qkv": {f"k_qkv<{q},{u},{mv},{sp}>" for q, us in Q for u in us for mv in (4, 2, 1, 0) for sp in (1, 2)},
        "k_gemv_res": {f"k_gemv_res<{q},{u},{mv},{sp}>" for q, us in (("false", (8, 4, 2)), ("true", (4, 3, 2)))
                       for u in us for mv in (6, 4, 2, 1, 0) for sp in (1, 2, 4)},
        "k_wo_comb": {f"k_wo_comb<{q},{u},{mv},{sp}>" for q, us in Q for u in us for mv in (2, 4) for sp in (1, 2, 4)},
        "k_ffn13": {f"k_ffn13<{q},{u},{mv}>" for q, us in Q for u in us for mv in (4, 2, 1, 0)},
        "k_cls": {f"k_cls<{q},{u},{mv}>" for q, us in Q for u in us for mv in (4, 2, 1, 0)},
    }
    assert set(base) == wc.DECODE_F32
    counts = {"k_qkv": 16, "k_gemv_res": 45, "k_wo_comb": 12, "k_ffn13": 8, "k_cls": 8}
    total = 0
    for stem, want in base.items():
        assert co.instantiations(notes, {stem}) == want, stem  # fp32 and int8: unchanged
        for q, twin in (("true", "_q4"), ("false", "_w16"), ("false", "_h16")):
            assert stem + twin in wc.DECODE[twin[1:]]
            w = {k.replace(f"{stem}<{q},", f"{stem}{twin}<") for k in want if k.startswith(f"{stem}<{q},")}
            got = co.instantiations(notes, {stem + twin})
            assert got == w and got, (stem + twin, sorted(got - w), sorted(w - got))
        n = len(co.instantiations(notes, {stem + "_q4"}))
        assert n == counts[stem], (stem, n)
        total += n
    assert total == 89
    for ring in sorted(wc.DECODE_INT8 - wc.DECODE_F32):  # no ring form on the copy, the int8 one as it was
        assert co.instantiations(notes, {ring}) == {ring + "<2,4,false>"}
        assert not co.instantiations(notes, {ring + "_q4"})
    stems = wc.DECODE["q4"]
    scratch = {co.template_name(k): v for k, v in co.kernel_scratch(notes).items()
               if (co.template_name(k) or "").split("<")[0] in stems}
    assert len(scratch) == 89, len(scratch)
    assert not any(scratch.values()), {k: v for k, v in scratch.items() if v}
    assert "k_q4_build" in co.kernels(notes, {"k_q4_build"})
