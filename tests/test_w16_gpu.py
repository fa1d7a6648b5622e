"""W16 (KH_FLAG_W16) on the GPU: a model that streams the 16-bit copy of a bf16-exact image computes the BITS of the
same image streamed as fp32 - logits, K/V rows, tokens and log-prob records, compared with np.array_equal / as bytes,
never with a tolerance.

Models: 2 layers, 1024 cache rows, synth_image(seed fixed, final_norm_std=1.0) with its matrices rounded to bf16
(binfmt.round_matrices_bf16).  The two models of a comparison share one device image.  Geometries, shapes, the step
loop and the comparisons are those of wcopy_cases.py.

  1. state: a rounded image -> state 1, the planned bytes, the launch log of a step names the _w16 kernel of every
     adopted class and no fp32 twin of it; a plain synth_image -> state -1, an int8 image -> state 0, both with the
     launches (and logits) of a flag-off model; flag off -> the launches written down here.
  2. bit identity under forced shapes: four geometries (w2 staging depths 6 / 0 and 4 / 0, masked lanes in every row,
     the copy of a tied tok_emb), for workgroups of 256 and 512 threads every (u, split) each kernel accepts through
     KH_SHAPE_*, grids of one pair per wave, and two shapes with small odd grids; teacher-forced steps at positions 0,
     1, 2 and - after random K/V rows were written below it - 300 (k_wo_comb_w16), into K/V rows that hold NaN;
     m.prefill of the first three tokens (fp32 arena) leaves the token loop's rows.
  3. the copy is what is read: NaN over the fp32 matrices of layer 1 does not change a flag-on model's logits and
     turns a flag-off model's into NaN.
  4. loops: generate, greedy and sampled with penalties, a logit bias and log-probs, exec graph and fused, across
     positions 250 .. 270; 32 greedy words equal the CPU oracle's on the rounded image.
  5. KH_SELFTEST_FAIL=w16 -> state -2, fp32 launches, the same logits.
  6. coverage gate: every compiled instantiation of the five _w16 stems was launched by (2); a launched name exists
     in the code objects.
"""
import numpy as np
import pytest
import torch

import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

W16 = _ffi.KH_FLAG_W16
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
GEOMETRIES, TIED = wc.GEOMETRIES_F32, wc.TIED
STEMS = wc.DECODE["w16"]
GEMV = STEMS | wc.DECODE_F32  # the launches a logged step keeps
TIED_STEP_FP32, TIED_STEP_W16 = wc.TIED_STEP_F32, wc.TIED_STEP["w16"]  # one fused step at position 0

_LAUNCHED = {}  # geometry -> _w16 instantiations its shapes launched (test_bit_identity -> test_coverage_gate)
_model = wc.model


@pytest.fixture(scope="module")
def tied_img(gpu):
    return wc.exact_image("w16", TIED, gpu)


def _logged_step(m):
    return wc.logged_step(m, GEMV)


# ---- 1. state ---------------------------------------------------------------------------------
def test_state_and_launches(gpu, tied_img):
    m0 = _model(tied_img, TIED)
    m1 = _model(tied_img, TIED, W16)
    try:
        # fails on a library without the feature: no such entry point
        assert m0.w16_info() == {"state": 0, "bytes": 0, "build_us": 0, "classes": [], "first_inexact": -1}
        info = m1.w16_info()
        assert info["state"] == 1 and info["first_inexact"] == -1, info
        assert info["bytes"] == wc.planned_w16_bytes(TIED) > 0, info
        assert info["classes"] == list(_ffi.KH_W16_CLASSES), info  # the plan adopts every class
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == TIED_STEP_FP32, sorted(log0)
        assert log1 == TIED_STEP_W16, sorted(log1)
        assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    finally:
        m0.close()
        m1.close()


def test_inexact_and_int8_images_launch_what_they_launch_today(gpu):
    plain = binfmt.synth_image(TIED, seed=4242, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    m0, m1 = _model(plain, TIED), _model(plain, TIED, W16)
    try:
        info = m1.w16_info()
        assert info["state"] == -1 and info["bytes"] == 0 and info["classes"] == [], info
        assert info["first_inexact"] == 0, info  # wq of layer 0
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 == TIED_STEP_FP32, (sorted(log0), sorted(log1))
        assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    finally:
        m0.close()
        m1.close()
    # one low bit in the LAST covered tensor (the tied classifier = tok_emb is tensor 7 * layers)
    img = wc.exact_image("w16", TIED, gpu)
    e = [t for t in binfmt.layout(TIED)[0] if t.name == "tok_emb"][0]
    img[e.offset + e.nbytes - 4] |= 1
    torch.cuda.synchronize()
    m = _model(img, TIED, W16)
    try:
        info = m.w16_info()
        assert info["state"] == -1 and info["first_inexact"] == 7 * TIED.n_layers, info
    finally:
        m.close()
    q8 = wc.spec(512, 1408, 8, 8, 501, True, 64, wc.INTER, wc.L, "w16-q8")
    qimg = binfmt.synth_image(q8, seed=7, device=gpu)
    torch.cuda.synchronize()
    m0, m1 = _model(qimg, q8), _model(qimg, q8, W16)
    try:
        assert m1.w16_info() == {"state": 0, "bytes": 0, "build_us": 0, "classes": [], "first_inexact": -1}
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 and log0 and not any(k.split("<")[0] in STEMS for k in log1), sorted(log1)
        assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    finally:
        m0.close()
        m1.close()


def test_hook_overrides_the_flag(gpu, tied_img):
    with wc.hook("KH_W16", "1"):
        m = _model(tied_img, TIED)
        try:
            assert m.w16_info()["state"] == 1
        finally:
            m.close()
    with wc.hook("KH_W16", "0"):
        m = _model(tied_img, TIED, W16)
        try:
            assert m.w16_info()["state"] == 0 and _logged_step(m)[0] == TIED_STEP_FP32
        finally:
            m.close()


# ---- 2. bit identity under forced shapes ------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes(gpu, name):
    spec = GEOMETRIES[name]
    img = wc.exact_image("w16", spec, gpu)
    assert binfmt.matrices_bf16_exact(img, spec)
    rng = np.random.default_rng(7)
    steps = wc.steps(spec, rng)
    rows = wc.deep_rows(spec, rng)
    shapes = wc.decode_shapes(spec)
    launched, n_prefill = set(), 0
    try:
        for i, sh in enumerate(shapes):
            what = f"{name} shape {i} {sh}"
            wc.set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _model(img, spec, W16)
            try:
                assert m1.w16_info()["state"] == 1, what
                log, _, got = wc.compare_steps(m0, m1, spec, steps, rows, what, STEMS, GEMV)
                launched |= log
                toks = [t for t, _ in steps[:3]]
                try:
                    m1.prefill(toks, 0)  # B-token pass on the fp32 arena
                except _ffi.KhError as e:
                    assert e.code == _ffi.KH_ERR_UNSUPPORTED, e  # the shape is outside prefill_supported
                else:
                    n_prefill += 1
                    for layer in range(spec.n_layers):
                        k, v = m1.read_kv(layer, 0, 3)
                        kt = np.stack([r[1][layer] for r in got[:3]])
                        vt = np.stack([r[2][layer] for r in got[:3]])
                        assert np.array_equal(k.view(np.uint32), kt) and np.array_equal(v.view(np.uint32), vt), \
                            f"{what}: prefill K/V, layer {layer}"
            finally:
                m0.close()
                m1.close()
    finally:
        wc.set_shape_hooks({})
    assert n_prefill > 0, f"{name}: no shape ran the B-token prefill"
    _LAUNCHED[name] = launched
    print(f"{name}: {len(shapes)} shapes, {len(launched)} W16 instantiations launched, {n_prefill} prefills")


# ---- 3. the copy is what is read --------------------------------------------------------------
def test_the_copy_is_what_is_read(gpu):
    for flags in (W16, 0):
        img = wc.exact_image("w16", TIED, gpu)
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
                assert t0 == t1 and np.array_equal(before.view(np.uint32), after.view(np.uint32))
            else:  # the check of this test: the poison is in what a flag-off model streams
                assert np.isnan(after).all()
        finally:
            m.close()


# ---- 4. loops ---------------------------------------------------------------------------------
def test_generate_loops_match(gpu, oracle, tied_img):
    res = {}
    for flags in (EXACT, EXACT | W16):
        m = _model(tied_img, TIED, flags)
        try:
            assert m.w16_info()["state"] == (1 if flags & W16 else 0)
            greedy32 = m.generate(wc.loop_prompt(TIED)[:2], 32, exec="graph")[0]
            res[flags] = dict(wc.generate_loops(m), greedy32=greedy32)
        finally:
            m.close()
    a, b = res[EXACT], res[EXACT | W16]
    wc.assert_loops_equal(a, b)
    # anchor outside the library: the CPU oracle on the rounded image
    om = oracle.OracleModel.from_spec(tied_img.cpu().numpy(), TIED, cache_len=wc.CACHE)
    want = om.generate(wc.loop_prompt(TIED)[:2], 32)
    om.close()
    assert b["greedy32"] == want, (b["greedy32"], want)


# ---- 5. self-check ----------------------------------------------------------------------------
def test_selfcheck_failure_falls_back_to_fp32(gpu, tied_img):
    m0 = _model(tied_img, TIED)
    with wc.hook("KH_SELFTEST_FAIL", "w16"):
        m1 = _model(tied_img, TIED, W16)
    try:
        info = m1.w16_info()
        assert info["state"] == -2 and info["bytes"] == 0 and info["classes"] == [], info
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 == TIED_STEP_FP32, sorted(log1)
        assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    finally:
        m0.close()
        m1.close()


# ---- 6. coverage gate -------------------------------------------------------------------------
def test_coverage_gate(gpu):
    wc.coverage_gate(STEMS, GEOMETRIES, _LAUNCHED, "W16")
