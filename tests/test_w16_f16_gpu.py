"""W16 for fp16-exact images (KH_FLAG_W16_F16) on the GPU: a model that streams the fp16-format 16-bit copy of an
fp16-exact image computes the BITS of the same image streamed as fp32 - logits, K/V rows, tokens and log-prob records,
compared with np.array_equal / as bytes, never with a tolerance.

Models and helpers are those of wcopy_cases.py (2 layers, 1024 cache rows, its four fp32 geometries); the image is
synth_image(seed fixed, final_norm_std=1.0) with its matrices rounded to fp16 (binfmt.round_matrices_fp16): 87 % of its
matrix words are not bf16-exact and some thousand per geometry are fp16 subnormals.  The two models of a comparison
share one device image.

  1. state: fp16-rounded image + new flag -> state 1, format fp16, the planned bytes, a step logs the _h16 kernels and
     no fp32 or _w16 GEMV, the flag-off logits; the same image + KH_FLAG_W16 alone -> state -1 and today's launches; a
     bf16-rounded image + new flag -> format bf16, _w16 kernels; a plain image -> state -1, first inexact fp16 tensor 0;
     int8 -> state 0; the hook KH_W16_F16 overrides the bit both ways.
  2. bit identity under forced shapes: the loop of test_w16_gpu.py (every (u, split, wg) the KH_SHAPE_* hooks accept,
     two small odd grids; positions 0, 1, 2 and 300 behind random rows; NaN-filled cache rows).
  3. the copy is what is read: NaN over layer 1's fp32 matrices.
  4. edges: (a) layer 0's wk made of +-2^-24, the largest fp16 subnormal, 2^-14, 65504 and -0; (b) an untied geometry
     whose embedding row 5 is scaled down until the flag-OFF model's layer-0 K row holds fp32 subnormals (asserted), so
     the FMAs of the _h16 kernels meet subnormal products, accumulators and results.
  5. loops: greedy and sampled generate with penalties, a bias and log-probs, graph and fused, across position 256; 32
     greedy words against the CPU oracle on the fp16-rounded image.
  6. KH_SELFTEST_FAIL=w16 -> state -2, fp32 launches, the same logits.
  7. coverage gate: every compiled instantiation of the five _h16 stems was launched by (2).
"""
import numpy as np
import pytest
import torch

import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

W16 = _ffi.KH_FLAG_W16
F16 = _ffi.KH_FLAG_W16_F16  # fails on a library without the feature
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
GEOMETRIES, TIED = wc.GEOMETRIES_F32, wc.TIED
UNTIED = wc.spec(448, 1216, 7, 7, 999, False, 64, wc.INTER, wc.L, "h16-untied")  # tok_emb is not in the copy
STEMS = wc.DECODE["h16"]
GEMV = STEMS | wc.DECODE["w16"] | wc.DECODE_F32  # the launches a logged step keeps
# one fused step at position 0
TIED_STEP_FP32, TIED_STEP_W16, TIED_STEP_H16 = wc.TIED_STEP_F32, wc.TIED_STEP["w16"], wc.TIED_STEP["h16"]
NO_COPY = {"state": 0, "bytes": 0, "build_us": 0, "classes": [], "first_inexact": -1}

_LAUNCHED = {}  # geometry -> _h16 instantiations its shapes launched (test_bit_identity -> test_coverage_gate)
_model = wc.model


@pytest.fixture(scope="module")
def tied_img(gpu):
    return wc.exact_image("h16", TIED, gpu)


def _logged_step(m):
    return wc.logged_step(m, GEMV)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. state ---------------------------------------------------------------------------------
def test_state_and_launches(gpu, tied_img):
    assert binfmt.matrices_fp16_exact(tied_img, TIED) and not binfmt.matrices_bf16_exact(tied_img, TIED)
    m0, m1, mb = _model(tied_img, TIED), _model(tied_img, TIED, F16), _model(tied_img, TIED, W16)
    try:
        assert m0.w16_info() == NO_COPY and m0.w16_format() == {"format": None, "first_inexact_fp16": -1}
        info = m1.w16_info()
        assert info["state"] == 1 and info["first_inexact"] == 0, info  # wq of layer 0 is not bf16-exact
        assert info["bytes"] == wc.planned_w16_bytes(TIED) > 0, info
        assert info["classes"] == list(_ffi.KH_W16_CLASSES), info
        assert m1.w16_format() == {"format": "fp16", "first_inexact_fp16": -1}
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == TIED_STEP_FP32, sorted(log0)
        assert log1 == TIED_STEP_H16, sorted(log1)
        assert np.isfinite(lg0).all() and _same_bits(lg0, lg1)
        # KH_FLAG_W16 alone stays bf16-only: what it reported and launched before the fp16 format existed
        info = mb.w16_info()
        assert info["state"] == -1 and info["bytes"] == 0 and info["classes"] == [] and info["first_inexact"] == 0, info
        assert mb.w16_format() == {"format": None, "first_inexact_fp16": -1}  # fp16 was not tried
        logb, lgb = _logged_step(mb)
        assert logb == TIED_STEP_FP32 and _same_bits(lg0, lgb), sorted(logb)
    finally:
        m0.close()
        m1.close()
        mb.close()


def test_bf16_plain_and_int8_images(gpu):
    img = wc.exact_image("w16", TIED, gpu)  # bf16-exact: the bf16 format wins, the fp16 build never runs
    m0, m1 = _model(img, TIED), _model(img, TIED, F16)
    try:
        assert m1.w16_info()["state"] == 1 and m1.w16_format() == {"format": "bf16", "first_inexact_fp16": -1}
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log1 == TIED_STEP_W16 and _same_bits(lg0, lg1), sorted(log1)
    finally:
        m0.close()
        m1.close()
    plain = binfmt.synth_image(TIED, seed=4242, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    m0, m1 = _model(plain, TIED), _model(plain, TIED, F16)
    try:
        info = m1.w16_info()
        assert info["state"] == -1 and info["bytes"] == 0 and info["classes"] == [] and info["first_inexact"] == 0, info
        assert m1.w16_format() == {"format": None, "first_inexact_fp16": 0}  # slot 7 = 1: wq of layer 0
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 == TIED_STEP_FP32 and _same_bits(lg0, lg1), (sorted(log0), sorted(log1))
    finally:
        m0.close()
        m1.close()
    # one mantissa bit too many in the LAST covered tensor (the tied classifier = tok_emb is tensor 7 * layers)
    img = wc.exact_image("h16", TIED, gpu)
    e = [t for t in binfmt.layout(TIED)[0] if t.name == "tok_emb"][0]
    img[e.offset + e.nbytes - 4] |= 1
    torch.cuda.synchronize()
    m = _model(img, TIED, F16)
    try:
        assert m.w16_info()["state"] == -1
        assert m.w16_format() == {"format": None, "first_inexact_fp16": 7 * TIED.n_layers}
    finally:
        m.close()
    q8 = wc.spec(512, 1408, 8, 8, 501, True, 64, wc.INTER, wc.L, "h16-q8")
    qimg = binfmt.synth_image(q8, seed=7, device=gpu)
    torch.cuda.synchronize()
    m0, m1 = _model(qimg, q8), _model(qimg, q8, F16)
    try:
        assert m1.w16_info() == NO_COPY and m1.w16_format() == {"format": None, "first_inexact_fp16": -1}
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 and log0 and not wc.stems(log1) & (STEMS | wc.DECODE["w16"]), sorted(log1)
        assert _same_bits(lg0, lg1)
    finally:
        m0.close()
        m1.close()


def test_hook_overrides_the_flag(gpu, tied_img):
    with wc.hook("KH_W16_F16", "1"):
        for flags in (0, W16):  # the hook alone asks for a copy, as the flag alone does
            m = _model(tied_img, TIED, flags)
            try:
                assert m.w16_info()["state"] == 1 and m.w16_format()["format"] == "fp16", flags
                assert _logged_step(m)[0] == TIED_STEP_H16
            finally:
                m.close()
        with wc.hook("KH_W16", "0"):  # no copy at all, whatever else is set
            m = _model(tied_img, TIED, F16)
            try:
                assert m.w16_info() == NO_COPY and _logged_step(m)[0] == TIED_STEP_FP32
            finally:
                m.close()
    with wc.hook("KH_W16_F16", "0"):
        m = _model(tied_img, TIED, F16 | W16)  # bf16 only
        try:
            assert m.w16_info()["state"] == -1 and m.w16_format() == {"format": None, "first_inexact_fp16": -1}
            assert _logged_step(m)[0] == TIED_STEP_FP32
        finally:
            m.close()
        m = _model(tied_img, TIED, F16)  # the bit is off and nothing else asks
        try:
            assert m.w16_info() == NO_COPY
        finally:
            m.close()


# ---- 2. bit identity under forced shapes ------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes(gpu, name):
    spec = GEOMETRIES[name]
    img = wc.exact_image("h16", spec, gpu)
    assert binfmt.matrices_fp16_exact(img, spec) and not binfmt.matrices_bf16_exact(img, spec)
    rng = np.random.default_rng(7)
    steps = wc.steps(spec, rng)
    rows = wc.deep_rows(spec, rng)
    shapes = wc.decode_shapes(spec)
    launched = set()
    try:
        for i, sh in enumerate(shapes):
            what = f"{name} shape {i} {sh}"
            wc.set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _model(img, spec, F16)
            try:
                assert m1.w16_info()["state"] == 1 and m1.w16_format()["format"] == "fp16", what
                launched |= wc.compare_steps(m0, m1, spec, steps, rows, what, STEMS, GEMV)[0]
            finally:
                m0.close()
                m1.close()
    finally:
        wc.set_shape_hooks({})
    _LAUNCHED[name] = launched
    print(f"{name}: {len(shapes)} shapes, {len(launched)} _h16 instantiations launched")


# ---- 3. the copy is what is read --------------------------------------------------------------
def test_the_copy_is_what_is_read(gpu):
    for flags in (F16, 0):
        img = wc.exact_image("h16", TIED, gpu)
        assert (img.data_ptr() + TIED.header_bytes()) % 16 == 0  # from_device_image uses the image in place
        m = _model(img, TIED, flags)
        try:
            m.set_sampling(temperature=0.8, top_k=50, top_p=0.95, seed=3)  # no screened tail: nothing re-scores fp32 rows
            t0 = m.predict(5, 0, exec="fused")
            before = m.logits()
            assert np.isfinite(before).all()
            wc.poison_layer1(img, TIED, wc.LAYER1, float("nan"))
            t1 = m.predict(5, 0, exec="fused")
            after = m.logits()
            if flags:
                assert m.w16_format()["format"] == "fp16"
                assert t0 == t1 and _same_bits(before, after)
            else:  # the check of this test: the poison is in what a flag-off model streams
                assert np.isnan(after).all()
        finally:
            m.close()


# ---- 4. edges ---------------------------------------------------------------------------------
def _subnormal_words(words):
    return int((((words >> 23) & 0xFF) == 0).sum() - ((words & 0x7FFFFFFF) == 0).sum())


def test_edge_weights(gpu):
    """(a) every fp16 edge value as a weight: rows of one value each, then rows that hold all six"""
    img = wc.exact_image("h16", TIED, gpu)
    vals = torch.tensor([2.0 ** -24, -2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, -0.0], dtype=torch.float32)
    e = [t for t in binfmt.layout(TIED)[0] if t.name == "wk.0"][0]
    wk = binfmt.tensor_from_image(img, e)
    r = torch.arange(wk.shape[0]).unsqueeze(1)
    c = torch.arange(wk.shape[1]).unsqueeze(0)
    idx = torch.where(r < wk.shape[0] // 2, r + 0 * c, r + c) % len(vals)
    wk.copy_(vals[idx].to(wk.device))
    torch.cuda.synchronize()
    assert binfmt.matrices_fp16_exact(img, TIED)
    words = wk.cpu().numpy().view(np.uint32)
    assert _subnormal_words(words) == 0 and (words == 0x80000000).sum() > 0  # fp16 subnormals are fp32 normals
    m0, m1 = _model(img, TIED), _model(img, TIED, F16)
    try:
        assert m1.w16_format()["format"] == "fp16"
        steps = [(5, 0), (17, 1), (900, 2)]
        _, want, _ = wc.compare_steps(m0, m1, TIED, steps, None, "edge weights", STEMS, GEMV)
        assert np.isfinite(want[0][0].view(np.float32)).all()  # position 0: one key, whatever its size
        k0 = np.abs(want[0][1][0].view(np.float32))  # layer 0's K row is made of these weights: 2^-24 .. 65504 times a sum
        assert np.isfinite(k0).all() and (k0 > 1e3).any() and ((k0 > 0) & (k0 < 1e-3)).any(), (k0.min(), k0.max())
    finally:
        m0.close()
        m1.close()


def test_fp32_subnormal_products_and_sums(gpu):
    """(b) an embedding row so small that the norm leaves it tiny (x^2 underflows: x * rsqrt(eps)): layer 0's K row
    is a sum of fp32-subnormal products.  tok_emb is not in the copy of an untied model, so the image stays fp16-exact."""
    img = wc.exact_image("h16", UNTIED, gpu)
    e = [t for t in binfmt.layout(UNTIED)[0] if t.name == "tok_emb"][0]
    # |emb| ~ 0.02, rsqrt(eps) = 316, a K entry ~ 0.02 sqrt(448) |x rsqrt(eps)|: 2^-130 puts it near 2^-129
    row = binfmt.tensor_from_image(img, e)[5]
    small = np.ldexp(row.cpu().numpy(), -130)  # on the host: no device flush mode has a say in the test's input
    assert _subnormal_words(small.view(np.uint32)) > row.numel() // 2
    row.copy_(torch.from_numpy(small))
    torch.cuda.synchronize()
    assert binfmt.matrices_fp16_exact(img, UNTIED)
    m0, m1 = _model(img, UNTIED), _model(img, UNTIED, F16)
    try:
        assert m1.w16_info()["state"] == 1 and m1.w16_format()["format"] == "fp16"
        steps = [(5, 0), (5, 1)]
        _, want, got = wc.compare_steps(m0, m1, UNTIED, steps, None, "subnormal K row", STEMS, GEMV)
        k0 = want[0][1][0]  # flag OFF: layer 0's K row at position 0
        n = _subnormal_words(k0)
        print(f"flag-off K row: {n} of {k0.size} words are non-zero fp32 subnormals")
        assert n > 0, "the case is vacuous: no fp32 subnormal in the flag-off K row"
        assert _subnormal_words(got[0][1][0]) == n
    finally:
        m0.close()
        m1.close()


# ---- 5. loops ---------------------------------------------------------------------------------
def test_generate_loops_match(gpu, oracle, tied_img):
    res = {}
    for flags in (EXACT, EXACT | F16):
        m = _model(tied_img, TIED, flags)
        try:
            assert m.w16_format()["format"] == ("fp16" if flags & F16 else None)
            greedy32 = m.generate(wc.loop_prompt(TIED)[:2], 32, exec="graph")[0]
            res[flags] = dict(wc.generate_loops(m), greedy32=greedy32)
        finally:
            m.close()
    a, b = res[EXACT], res[EXACT | F16]
    wc.assert_loops_equal(a, b)
    # anchor outside the library: the CPU oracle on the fp16-rounded image
    om = oracle.OracleModel.from_spec(tied_img.cpu().numpy(), TIED, cache_len=wc.CACHE)
    want = om.generate(wc.loop_prompt(TIED)[:2], 32)
    om.close()
    assert b["greedy32"] == want, (b["greedy32"], want)


# ---- 6. self-check ----------------------------------------------------------------------------
def test_selfcheck_failure_falls_back_to_fp32(gpu, tied_img):
    m0 = _model(tied_img, TIED)
    with wc.hook("KH_SELFTEST_FAIL", "w16"):
        m1 = _model(tied_img, TIED, F16)
    try:
        info = m1.w16_info()
        assert info["state"] == -2 and info["bytes"] == 0 and info["classes"] == [], info
        assert m1.w16_format()["format"] is None
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 == TIED_STEP_FP32, sorted(log1)
        assert _same_bits(lg0, lg1)
    finally:
        m0.close()
        m1.close()


# ---- 7. coverage gate -------------------------------------------------------------------------
def test_coverage_gate(gpu):
    wc.coverage_gate(STEMS, GEOMETRIES, _LAUNCHED, "_h16")
