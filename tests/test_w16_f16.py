"""W16 for fp16-exact images (KH_FLAG_W16_F16), host side: the helpers that make and recognise an fp16-exact image,
the ABI and the _h16 kernels in the library's gfx950 code objects.  CPU only.

binfmt.round_matrices_fp16 is checked word for word against numpy's float32 -> float16 -> float32 conversion (IEEE
round-to-nearest-even, subnormals produced, overflow to Inf) on a synthetic image and on hand-picked values;
binfmt.matrices_fp16_exact against the integer rule of the header (a = |w|, e = a >> 23: a == 0, or 113 <= e <= 142 with
13 zero low bits, or 103 <= e <= 112 with 126 - e zero low bits) restated in numpy.
"""
import os

import numpy as np

import code_objects as co
import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt, build

TINY = dict(dim=64, hidden_dim=96, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=37, seq_len=16)

DECODE_W16, PASS_W16 = wc.DECODE["w16"], wc.PASS["w16"]


def _spec(tied, **kw):
    return binfmt.ModelSpec(**{**TINY, **kw}, shared_classifier=tied)


def _np_round(words):
    with np.errstate(over="ignore", invalid="ignore"):
        return words.view(np.float32).astype(np.float16).astype(np.float32).view(np.uint32)


def _rule(words):
    """the exactness rule of include/kuiper_hip.h (KH_FLAG_W16_F16) on uint32 words"""
    a = words.astype(np.uint64) & 0x7FFFFFFF
    e = a >> 23
    norm = (e >= 113) & (e <= 142) & ((a & 0x1FFF) == 0)
    low = a & ((np.uint64(1) << np.clip(126 - e.astype(np.int64), 0, 63).astype(np.uint64)) - np.uint64(1))
    sub = (e >= 103) & (e <= 112) & (low == 0)
    return (a == 0) | norm | sub


EDGE = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25,
                 1023 * 2.0 ** -24, -1023 * 2.0 ** -24,  # the largest subnormal
                 2.0 ** -14, 65504.0, -65504.0, 65520.0, -65520.0, np.nan,
                 # beyond the issue's list: just around the ties, the subnormal / normal border, fp32 subnormals, Inf
                 2.0 ** -25 * (1 + 2.0 ** -23), 5 * 2.0 ** -26, 1023.5 * 2.0 ** -24, 2.0 ** -14 * (1 - 2.0 ** -12),
                 65519.996, 1e-40, 3e38, np.inf, -np.inf, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=np.float32)


def test_round_matrices_fp16_is_numpys_conversion_and_touches_nothing_else():
    for tied in (True, False):
        spec = _spec(tied, family=binfmt.FAMILY_QWEN2)
        img = binfmt.synth_image(spec, seed=11).numpy().copy()
        for e in binfmt.w16_tensors(spec):  # every covered tensor starts with the edge values
            img[e.offset: e.offset + EDGE.nbytes] = EDGE.view(np.uint8)
        before = img.copy()
        assert binfmt.round_matrices_fp16(img, spec) is img
        covered = np.zeros(img.size, bool)
        for e in binfmt.w16_tensors(spec):
            covered[e.offset: e.offset + e.nbytes] = True
            w = before[e.offset: e.offset + e.nbytes].view(np.uint32)
            r = img[e.offset: e.offset + e.nbytes].view(np.uint32)
            want = _np_round(w)
            bad = np.flatnonzero(r != want)
            assert bad.size == 0, (e.name, [(hex(w[i]), hex(r[i]), hex(want[i])) for i in bad[:4]])
        assert np.array_equal(img[~covered], before[~covered]), "bytes outside the covered tensors changed"
        again = binfmt.round_matrices_fp16(img.copy(), spec)
        assert np.array_equal(again, img), "not idempotent"
    # what the edge values become, spelled out
    spec = _spec(True)
    img = binfmt.synth_image(spec, seed=11).numpy().copy()
    e = binfmt.w16_tensors(spec)[0]
    img[e.offset: e.offset + EDGE.nbytes] = EDGE.view(np.uint8)
    binfmt.round_matrices_fp16(img, spec)
    got = img[e.offset: e.offset + EDGE.nbytes].view(np.float32)
    want = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 0.0, -0.0, 2.0 ** -23, -2.0 ** -23, 1023 * 2.0 ** -24, -1023 * 2.0 ** -24,
            2.0 ** -14, 65504.0, -65504.0, np.inf, -np.inf]
    assert np.array_equal(got[:15].view(np.uint32), np.array(want, np.float32).view(np.uint32))
    assert np.isnan(got[15])
    # random words near and inside fp16's range, every sign
    rng = np.random.default_rng(5)
    w = ((rng.integers(95, 150, 1 << 18, dtype=np.uint64) << 23) | rng.integers(0, 1 << 23, 1 << 18, dtype=np.uint64)
         | (rng.integers(0, 2, 1 << 18, dtype=np.uint64) << 31)).astype(np.uint32)
    spec = _spec(False, dim=512, hidden_dim=64, vocab_size=512)  # wcls: 512 x 512 words
    img = binfmt.synth_image(spec, seed=1).numpy().copy()
    e = [t for t in binfmt.w16_tensors(spec) if t.name == "wcls"][0]
    img[e.offset: e.offset + e.nbytes] = w.view(np.uint8)
    binfmt.round_matrices_fp16(img, spec)
    assert np.array_equal(img[e.offset: e.offset + e.nbytes].view(np.uint32), _np_round(w))


def test_round_matrices_fp16_on_a_torch_image():
    spec = _spec(True)
    img = binfmt.synth_image(spec, seed=3)
    want = binfmt.round_matrices_fp16(img.numpy().copy(), spec)
    binfmt.round_matrices_fp16(img, spec)
    assert np.array_equal(img.numpy(), want)


def test_matrices_fp16_exact():
    import torch
    for tied in (True, False):
        spec = _spec(tied)
        img = binfmt.synth_image(spec, seed=3).numpy().copy()
        assert not binfmt.matrices_fp16_exact(img, spec)  # a plain synthetic image
        binfmt.round_matrices_fp16(img, spec)
        assert binfmt.matrices_fp16_exact(img, spec)
        assert binfmt.matrices_fp16_exact(torch.from_numpy(img), spec)
        assert not binfmt.matrices_bf16_exact(img, spec)  # 10 mantissa bits do not fit bf16's 7
        for e in binfmt.w16_tensors(spec):
            words = img[e.offset: e.offset + e.nbytes].view(np.uint32)
            i = int(np.flatnonzero((words & 0x7FFFFFFF) >= (113 << 23))[0])  # an fp16 normal
            bad = img.copy()
            bad[e.offset: e.offset + e.nbytes].view(np.uint32)[i] |= 1 << 12  # mantissa bit 12 of one word
            assert not binfmt.matrices_fp16_exact(bad, spec), e.name
            inf = img.copy()
            inf[e.offset: e.offset + e.nbytes].view(np.float32)[i] = np.inf
            assert not binfmt.matrices_fp16_exact(inf, spec), e.name
            nan = img.copy()
            nan[e.offset: e.offset + e.nbytes].view(np.uint32)[i] = 0x7FC00000  # an fp16-representable quiet NaN
            assert not binfmt.matrices_fp16_exact(nan, spec), e.name
        # bits outside the covered tensors do not matter
        other = [e for e in binfmt.layout(spec)[0] if e.name == "final_norm"][0]
        img[other.offset] |= 1
        assert binfmt.matrices_fp16_exact(img, spec)
    assert not binfmt.matrices_fp16_exact(np.zeros(1 << 16, np.uint8), _spec(False, quant=True))


def test_matrices_fp16_exact_agrees_with_the_integer_rule():
    rng = np.random.default_rng(9)
    n = 1 << 20
    # a third each: any word; exponents around fp16's range; fp16 values with a few low bits set or not
    k = n // 3
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    w[k: 2 * k] = ((rng.integers(98, 148, k, dtype=np.uint64) << 23)
                   | (rng.integers(0, 1 << 11, k, dtype=np.uint64) << rng.integers(0, 14, k, dtype=np.uint64))
                   | (rng.integers(0, 2, k, dtype=np.uint64) << 31)).astype(np.uint32)
    h = rng.integers(0, 1 << 16, n - 2 * k, dtype=np.uint64).astype(np.uint16)
    w[2 * k:] = h.view(np.float16).astype(np.float32).view(np.uint32)
    rule = _rule(w)
    # the rule is "the numpy round trip gives the word back, and the value is finite"
    assert np.array_equal(rule, (_np_round(w) == w) & np.isfinite(w.view(np.float32)))
    assert 0.3 < rule.mean() < 0.7  # both answers are well represented
    # matrices_fp16_exact word by word: one word in an otherwise exact tensor
    spec = _spec(False, dim=1024, hidden_dim=64, vocab_size=1024)  # wcls: 1024 x 1024 = 1 M words
    img = binfmt.synth_image(spec, seed=1).numpy().copy()
    binfmt.round_matrices_fp16(img, spec)
    e = [t for t in binfmt.w16_tensors(spec) if t.name == "wcls"][0]
    import torch
    got = binfmt._fp16_exact_words(torch.from_numpy(w.copy()).view(torch.int32)).numpy()
    assert np.array_equal(got, rule)
    img[e.offset: e.offset + e.nbytes] = np.where(rule, w, 0).astype(np.uint32).view(np.uint8)
    assert binfmt.matrices_fp16_exact(img, spec)
    first_bad = int(np.flatnonzero(~rule)[0])
    img[e.offset + 4 * first_bad: e.offset + 4 * first_bad + 4] = w[first_bad: first_bad + 1].view(np.uint8)
    assert not binfmt.matrices_fp16_exact(img, spec)


def test_flag_hook_and_entry_points():
    build.build_lib()
    assert _ffi.KH_FLAG_W16_F16 == 32
    src = open(os.path.join(build.CSRC, "..", "..", "include", "kuiper_hip.h")).read()
    assert "#define KH_FLAG_W16_F16 32" in src and "#define KH_FLAG_W16 16" in src
    assert "KH_W16_F16".startswith(_ffi._HOOK_PREFIXES)  # sync_env mirrors it from the environment
    assert _ffi.debug_get("KH_W16_F16") is None
    with wc.hook("KH_W16_F16", "1"):
        assert _ffi.debug_get("KH_W16_F16") == "1"
    assert _ffi.debug_get("KH_W16_F16") is None
    from kuiperllama_amd.model import KuiperModel
    assert callable(KuiperModel.w16_format)
    for unit in ("kh_model_h16.hip", "kh_model_h16_pass.hip"):  # the twins compile in translation units of their own
        assert unit in build.SOURCES and os.path.exists(os.path.join(build.CSRC, unit))


def test_h16_kernels_in_the_code_objects():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    notes = co.code_object_notes(build.build_lib())
    n = {}
    for stems, total in ((DECODE_W16, 111), (PASS_W16, 21)):
        n[total] = 0
        for stem in sorted(stems):
            twin = stem[:-4] + "_h16"
            want = {k.replace(stem, twin) for k in co.instantiations(notes, {stem})}
            got = co.instantiations(notes, {twin})
            assert got == want and got, (twin, sorted(got - want), sorted(want - got))
            n[total] += len(got)
        assert n[total] == total, n
    # the _w16 pass sets and the fp32 / int8 sets are what they were
    for table in (wc.PASS_W16_COMPILED, wc.PASS_COMPILED_BEFORE):
        for stem, want in table.items():
            got = co.instantiations(notes, {stem})
            assert got == want, (stem, sorted(got - want), sorted(want - got))
    twins = wc.DECODE["h16"] | wc.PASS["h16"]
    scratch = {co.template_name(k): v for k, v in co.kernel_scratch(notes).items()
               if (co.template_name(k) or "").split("<")[0] in twins}
    assert len(scratch) == 132, len(scratch)
    assert not any(scratch.values()), {k: v for k, v in scratch.items() if v}
    assert "k_h16_build" in co.kernels(notes, {"k_h16_build"})
