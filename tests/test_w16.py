"""W16 (KH_FLAG_W16), host side: the helpers that make and recognise a bf16-exact image, the plan of the 16-bit weight
copy and the ABI.  CPU only.

binfmt.round_matrices_bf16 is checked against a numpy integer restatement of IEEE round-to-nearest-even from fp32 to
bf16 (drop 16 bits; up when the dropped half is above 0x8000, or equal to it and the kept part is odd; NaN stays a
quiet NaN) on hand-picked words - ties both ways, +-0, denormals, the largest finite value, Inf, NaN - and random ones.
"""
import os

import numpy as np
import torch

import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt, build

TINY = dict(dim=64, hidden_dim=96, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=37, seq_len=16)


def _spec(tied, **kw):
    return binfmt.ModelSpec(**{**TINY, **kw}, shared_classifier=tied)


def _rne_bf16_words(w):
    """uint32 fp32 words -> the fp32 words of their nearest bf16 values, by integer arithmetic on uint64."""
    w = w.astype(np.uint64)
    keep, drop = w >> 16, w & 0xFFFF
    up = (drop > 0x8000) | ((drop == 0x8000) & ((keep & 1) == 1))
    out = ((keep + up.astype(np.uint64)) << 16) & 0xFFFFFFFF
    nan = (w & 0x7FFFFFFF) > 0x7F800000
    out = np.where(nan, (w | 0x00400000) & 0xFFFF0000, out)
    return out.astype(np.uint32)


EDGE_WORDS = np.array([
    0x00000000, 0x80000000,              # +-0
    0x3F808000, 0x3F818000,              # ties: kept part even (stays), odd (goes up)
    0x3F807FFF, 0x3F808001,              # just below / above a tie
    0xBF808000, 0xBF818000, 0xBF818001,  # the same, negative
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,  # denormals (ties, largest)
    0x3F7FFFFF,                          # carries into the exponent: 1.0
    0x7F7FFFFF, 0xFF7FFFFF,              # largest finite: rounds to Inf
    0x7F7F0000, 0x7F7F7FFF,              # largest bf16, and just below its tie
    0x7F800000, 0xFF800000,              # Inf
    0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF, 0x7FBF8000,  # NaN: quiet, signalling, low-half payload only
], dtype=np.uint32)


def _image_with_words(spec, rng):
    """A synthetic image whose every covered tensor starts with the edge words followed by random words."""
    img = binfmt.synth_image(spec, seed=11).numpy().copy()
    for e in binfmt.w16_tensors(spec):
        v = img[e.offset: e.offset + e.nbytes].view(np.uint32)
        v[:] = rng.integers(0, 1 << 32, v.size, dtype=np.uint64).astype(np.uint32)
        v[: EDGE_WORDS.size] = EDGE_WORDS
    return img


def test_covered_tensors_follow_the_classifier():
    mats = {f"{n}.{l}" for n in wc.MATRICES for l in range(2)}
    assert {e.name for e in binfmt.w16_tensors(_spec(True))} == mats | {"tok_emb"}
    assert {e.name for e in binfmt.w16_tensors(_spec(False))} == mats | {"wcls"}
    q = _spec(True, family=binfmt.FAMILY_QWEN2)  # biases are not matrices
    assert {e.name for e in binfmt.w16_tensors(q)} == mats | {"tok_emb"}
    assert binfmt.w16_tensors(_spec(False, quant=True)) == []


def test_round_matrices_bf16_is_round_to_nearest_even_and_touches_nothing_else():
    rng = np.random.default_rng(5)
    for tied in (True, False):
        spec = _spec(tied, family=binfmt.FAMILY_QWEN2)
        img = _image_with_words(spec, rng)
        before = img.copy()
        got = binfmt.round_matrices_bf16(img, spec)
        assert got is img
        covered = np.zeros(img.size, bool)
        for e in binfmt.w16_tensors(spec):
            covered[e.offset: e.offset + e.nbytes] = True
            w = before[e.offset: e.offset + e.nbytes].view(np.uint32)
            r = img[e.offset: e.offset + e.nbytes].view(np.uint32)
            want = _rne_bf16_words(w)
            bad = np.flatnonzero(r != want)
            assert bad.size == 0, (e.name, [(hex(w[i]), hex(r[i]), hex(want[i])) for i in bad[:4]])
        assert np.array_equal(img[~covered], before[~covered]), "bytes outside the covered tensors changed"
        names = {e.name for e in binfmt.w16_tensors(spec)}
        assert ("tok_emb" in names) == tied  # the embedding is covered only as the tied classifier
        again = binfmt.round_matrices_bf16(img.copy(), spec)
        assert np.array_equal(again, img), "not idempotent"
    # the numpy restatement agrees with torch's own float32 -> bfloat16 conversion on random finite words
    w = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)
    w = w[(w & 0x7FFFFFFF) < 0x7F800000]
    t = torch.from_numpy(w.view(np.float32).copy()).to(torch.bfloat16).to(torch.float32).numpy().view(np.uint32)
    assert np.array_equal(_rne_bf16_words(w), t)


def test_round_matrices_bf16_on_a_torch_image():
    spec = _spec(True)
    img = binfmt.synth_image(spec, seed=3)
    want = binfmt.round_matrices_bf16(img.numpy().copy(), spec)
    binfmt.round_matrices_bf16(img, spec)
    assert np.array_equal(img.numpy(), want)


def test_matrices_bf16_exact():
    for tied in (True, False):
        spec = _spec(tied)
        img = binfmt.synth_image(spec, seed=3).numpy().copy()
        assert not binfmt.matrices_bf16_exact(img, spec)
        binfmt.round_matrices_bf16(img, spec)
        assert binfmt.matrices_bf16_exact(img, spec)
        assert binfmt.matrices_bf16_exact(torch.from_numpy(img), spec)
        for e in binfmt.w16_tensors(spec):  # one low bit in one element of one tensor
            bad = img.copy()
            bad[e.offset + 4 * (e.nbytes // 8)] |= 1
            assert not binfmt.matrices_bf16_exact(bad, spec), e.name
        # bits outside the covered tensors do not matter
        other = [e for e in binfmt.layout(spec)[0] if e.name == "final_norm"][0]
        img[other.offset] |= 1
        assert binfmt.matrices_bf16_exact(img, spec)
    assert not binfmt.matrices_bf16_exact(np.zeros(1 << 16, np.uint8), _spec(False, quant=True))


def test_plan_w16_bytes_and_classes():
    build.build_lib()
    for name, spec in binfmt.PRESETS.items():
        p = _ffi.plan_w16(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, spec.n_layers, spec.quant)
        if spec.quant:
            assert p == {"classes": [], "bytes": 0}, name  # not applicable
            continue
        want = sum(2 * e.shape[0] * e.shape[1] for e in binfmt.w16_tensors(spec))
        assert p["bytes"] == want, (name, p, want)  # every BASELINE matrix is a multiple of 256 bytes: no padding
        assert p["bytes"] * 2 == sum(e.nbytes for e in binfmt.w16_tensors(spec))  # half the matrix bytes
        assert set(p["classes"]) <= set(_ffi.KH_W16_CLASSES) and p["classes"], name
    # matrices that are no multiple of 256 bytes: each is padded on its own (the copy's byte count is one function for
    # W16 and Q4, kh_model_w16.hip::copy_bytes; the totals are those of the library before the two were merged)
    def pad(n):
        return (n + 255) & ~255
    dim, hid, kv, voc = 132, 356, 68, 1001
    want = 2 * pad(2 * dim * dim) + 2 * pad(2 * kv * dim) + 3 * pad(2 * hid * dim) + pad(2 * voc * dim)
    assert want == 653568 != 2 * (2 * dim * dim + 2 * kv * dim + 3 * hid * dim + voc * dim)
    assert _ffi.plan_w16(dim, hid, kv, voc, 1, False) == {"classes": list(_ffi.KH_W16_CLASSES), "bytes": want}
    assert _ffi.plan_w16(64, 64, 64, 1, 1, False)["bytes"] == 57600
    assert _ffi.plan_w16(256, 688, 128, 2048, 2, False)["bytes"] == 3948544
    assert _ffi.plan_w16(66, 96, 66, 37, 2, False) == {"classes": [], "bytes": 0}  # dim no multiple of 4
    out = (_ffi._i64 * 2)()
    assert _ffi.lib().kh_plan_w16(0, 96, 64, 37, 2, 0, out) == _ffi.KH_ERR_INVALID_ARG
    assert _ffi.lib().kh_plan_w16(64, 96, 64, 37, 2, 0, None) == _ffi.KH_ERR_INVALID_ARG


def test_w16_symbols_are_in_the_abi():
    build.build_lib()
    L = _ffi.lib()
    for n in ("kh_model_w16_info", "kh_plan_w16"):
        assert n in _ffi.EXPORTS and hasattr(L, n)
    assert _ffi.KH_FLAG_W16 == 16
    src = open(os.path.join(build.CSRC, "..", "..", "include", "kuiper_hip.h")).read()
    assert "#define KH_FLAG_W16 16" in src
    assert L.kh_model_w16_info(None, None) == _ffi.KH_ERR_INVALID_ARG
