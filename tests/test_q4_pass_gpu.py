"""The B-token passes of Q4 models on the GPU (kh_q4_pass.h): prefill, score, verify / generate_lookup and the
sequence-slot calls of a KH_FLAG_Q4 model whose pass mask (hook KH_Q4_PASS) names a class stream the packed 4-bit copy
and leave the BITS of the same image streamed as int8 - K/V rows, records, picks and words compared with
np.array_equal / as bytes, never with a tolerance.

Models: 2 layers, 1024 cache rows, wc.exact_image("q4", ..) (synth_image requantised to 4 bits), KH_FLAG_PREFILL_EXACT,
the four int8 geometries of test_q4_gpu.py, 4 tokens per pass (2 for w2 at hidden 10368: four int8-layout vectors of
10368 floats exceed the 160 KiB of pf_gemv_res).  The two models of a comparison share one device image.  Shapes, the
call sequence of (2) and the loops of (4) are those of wcopy_cases.py.

  1. state and launches: flag off -> the int8 pass stems alone; KH_Q4_PASS=0x1f -> exactly the five _q4 stems; 0 -> the
     int8 stems; 0x11 (qkv, cls) -> their _q4 stems beside the int8 k_pf_ffn13 and k_pf_gemv_res; hook unset -> the
     documented default; KH_Q4_CLASSES=0 with KH_Q4_PASS=0x1f -> every pass on the copy; the predict that follows launches
     what q4_info()["classes"] says whatever the pass hook is.
  2. bit identity under forced shapes: per geometry every shape of wc.pass_shapes, flag off against KH_Q4_PASS=0x1f,
     through wc.run_pass_shape; the dim-448 image carries the planted -8 / 7 / -1 nibbles.
  3. the copy is what is read: 0x55 over the int8 values of layer 1 leaves the K/V rows of a prefill and the records of
     a score of a 0x1f model as they were and changes a flag-off model's.
  4. loops: wc.pass_loops and a generate_lookup with the truth as hint, flag off against 0x1f.
  5. no copy, no change: a plain synth_image (state -1), an fp32 image (state 0) and KH_SELFTEST_FAIL=q4 (state -2) have
     pass mask [] under KH_Q4_PASS=0x1f and the launches and results of a flag-off model.
  6. coverage gate: every one of the 12 compiled _q4 pass instantiations was launched and compared by (2).
"""
import contextlib

import numpy as np
import pytest
import torch

import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

Q4 = _ffi.KH_FLAG_Q4
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
HALF, INTER, L = wc.HALF, wc.INTER, wc.L
WIDTH = 4  # tokens per int8 / Q4 pass

GEOMETRIES = {
    "1152-h10368": wc.spec(1152, 10368, 18, 6, 1001, True, 64, HALF, L, "q4p-1152"),  # w2: 2 tokens per pass
    "4224-h3072": wc.spec(4224, 3072, 33, 3, 777, True, 64, INTER, L, "q4p-4224"),    # hs 128 interleaved
    "960-g32-hs80": wc.spec(960, 1600, 12, 2, 1537, True, 32, HALF, L, "q4p-g32"),    # group 32, 60 units, odd vocabulary
    "448": wc.spec(448, 1216, 7, 7, 999, True, 64, INTER, L, "q4p-448"),              # 28 units: masked lanes; planted
}
SMALL = GEOMETRIES["448"]
INT8_STEMS = wc.PASS_F32  # the int8 pass kernels carry the fp32 stems
STEMS = {s + "_q4" for s in INT8_STEMS}
DECODE_Q4 = wc.DECODE["q4"]
ALL = list(_ffi.KH_Q4_CLASSES)
DEFAULT = ["w2"]  # KH_Q4_PASS_DEFAULT: the one class that passed the adoption rule on both measured geometries

_LAUNCHED = {}  # geometry -> _q4 pass instantiations its shapes launched (test_bit_identity -> test_coverage_gate)


def _model(img, spec, flags=0, passes=None, q4_classes=None):
    """passes: the value of the hook KH_Q4_PASS while the model is created (None: unset)"""
    with wc.hook("KH_Q4_PASS", passes) if passes is not None else contextlib.nullcontext():
        return wc.model(img, spec, flags | EXACT, q4_classes=q4_classes)


def _logged_passes(m, spec):
    return wc.logged_passes(m, spec, STEMS | INT8_STEMS)


def _pass_stems(classes):
    """the pass stems a model with this pass mask launches (wo and w2 share k_pf_gemv_res)"""
    on = lambda c: "_q4" if c in classes else ""  # noqa: E731
    return ({"k_pf_qkv" + on("qkv"), "k_seq_qkv" + on("qkv"), "k_pf_ffn13" + on("ffn13"), "k_pf_cls" + on("cls")}
            | {"k_pf_gemv_res" + on(c) for c in ("wo", "w2")})


def _decode_stems(classes):
    """the _q4 decode stems of a step at position 0 (wo and w2 share k_gemv_res_q4; no k_wo_comb_q4 that shallow)"""
    of = {"qkv": "k_qkv_q4", "wo": "k_gemv_res_q4", "ffn13": "k_ffn13_q4", "w2": "k_gemv_res_q4", "cls": "k_cls_q4"}
    return {of[c] for c in classes}


@pytest.fixture(scope="module")
def small_img(gpu):
    return wc.exact_image("q4", SMALL, gpu)


def _results(m, spec):
    """the K/V rows of a prefill and the records of a score, as bytes"""
    toks = [int(t) for t in np.random.default_rng(19).integers(0, spec.vocab_size, 9)]
    m.prefill(toks[:6], 0)
    kv = [m.read_kv(layer, 0, 6) for layer in range(spec.n_layers)]
    rows = b"".join(k.tobytes() + v.tobytes() for k, v in kv)
    m.set_logprobs(3)
    rec = m.score(toks, 0)
    m.set_logprobs(None)
    assert np.isfinite(rec["logprob"][:-1]).all()
    return rows, wc.rec_bytes(rec)


# ---- 1. state and launches --------------------------------------------------------------------
def test_state_and_launches(gpu, small_img):
    m0 = _model(small_img, SMALL)
    m1 = _model(small_img, SMALL, Q4, passes="0x1f")
    md = _model(small_img, SMALL, Q4)
    try:
        # fails on a library without the feature: no such method, and no _q4 pass kernel in the log
        assert m0.q4_pass_info() == {"classes": []}
        assert m1.q4_info()["state"] == 1 and m1.q4_pass_info() == {"classes": ALL}
        assert md.q4_info()["state"] == 1 and md.q4_pass_info() == {"classes": DEFAULT}
        assert m1.q4_info() == md.q4_info() | {"build_us": m1.q4_info()["build_us"]}  # the pass hook moves no decode class
        p0, d0 = _logged_passes(m0, SMALL)
        p1, d1 = _logged_passes(m1, SMALL)
        pd, dd = _logged_passes(md, SMALL)
        assert p0 == INT8_STEMS, sorted(p0)
        assert p1 == STEMS, sorted(p1)
        assert pd == _pass_stems(DEFAULT), sorted(pd)
        assert not d0 & DECODE_Q4, sorted(d0)
        want = _decode_stems(md.q4_info()["classes"])
        assert want and d1 & DECODE_Q4 == dd & DECODE_Q4 == want, (sorted(d1), sorted(dd))
    finally:
        m0.close()
        m1.close()
        md.close()


def test_hook_keeps_the_passes_on_int8_or_picks_classes(gpu, small_img):
    m = _model(small_img, SMALL, Q4, passes="0")
    try:
        assert m.q4_info()["state"] == 1 and m.q4_pass_info() == {"classes": []}
        p, d = _logged_passes(m, SMALL)
        assert p == INT8_STEMS, sorted(p)
        assert d & DECODE_Q4 == _decode_stems(m.q4_info()["classes"]) != set(), sorted(d)  # decode still reads the copy
    finally:
        m.close()
    m = _model(small_img, SMALL, Q4, passes="0x11")  # qkv and cls
    try:
        assert m.q4_pass_info() == {"classes": ["qkv", "cls"]}
        p, _ = _logged_passes(m, SMALL)
        assert p == {"k_pf_qkv_q4", "k_seq_qkv_q4", "k_pf_gemv_res", "k_pf_ffn13", "k_pf_cls_q4"}, sorted(p)
    finally:
        m.close()
    m = _model(small_img, SMALL, Q4, passes="1")
    try:
        assert m.q4_pass_info() == {"classes": DEFAULT}
    finally:
        m.close()
    # the pass mask does not depend on the decode classes: a copy no decode launch reads still serves every pass
    m = _model(small_img, SMALL, Q4, passes="0x1f", q4_classes="0")
    try:
        assert m.q4_info()["state"] == 1 and m.q4_info()["classes"] == [] and m.q4_pass_info() == {"classes": ALL}
        p, d = _logged_passes(m, SMALL)
        assert p == STEMS, sorted(p)
        assert not d & DECODE_Q4, sorted(d)
    finally:
        m.close()
    m = _model(small_img, SMALL, Q4, passes="0x2", q4_classes="0x1f")  # wo's pass alone; every decode class
    try:
        assert m.q4_info()["classes"] == ALL and m.q4_pass_info() == {"classes": ["wo"]}
        p, d = _logged_passes(m, SMALL)
        assert p == _pass_stems(["wo"]) and {"k_pf_gemv_res", "k_pf_gemv_res_q4"} <= p, sorted(p)
        assert d & DECODE_Q4 == _decode_stems(ALL), sorted(d)
    finally:
        m.close()
    m = _model(small_img, SMALL, passes="0x1f")  # the hook does not switch the copy on
    try:
        assert m.q4_info()["state"] == 0 and m.q4_pass_info() == {"classes": []}
        assert _logged_passes(m, SMALL)[0] == INT8_STEMS
    finally:
        m.close()


# ---- 2. bit identity under forced shapes ------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes(gpu, name):
    spec = GEOMETRIES[name]
    img = wc.exact_image("q4", spec, gpu, plant=spec is SMALL)
    assert binfmt.matrices_q4_exact(img, spec)
    shapes = wc.pass_shapes(spec)
    launched, n_ran = set(), 0
    try:
        for i, sh in enumerate(shapes):
            what = f"{name} shape {i} {sh}"
            wc.set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _model(img, spec, Q4, passes="0x1f")
            try:
                assert m1.q4_info()["state"] == 1 and m1.q4_pass_info() == {"classes": ALL}, what
                try:
                    assert m1.verify_width() == WIDTH == m0.verify_width(), what
                except _ffi.KhError as e:
                    assert e.code == _ffi.KH_ERR_UNSUPPORTED, e  # the shape is outside prefill_supported
                    continue
                with wc.launch_log() as read:  # after creation; m0 logs into it too: only _q4 names are kept
                    wc.run_pass_shape(m0, m1, spec, WIDTH, what, 7 + i)
                    launched |= {k for k in read() if wc.stem(k) in STEMS}
                n_ran += 1
            finally:
                m0.close()
                m1.close()
    finally:
        wc.set_shape_hooks({})
    assert n_ran >= 4, f"{name}: only {n_ran} shapes ran the B-token pass"
    if spec.hidden_dim == 10368:  # w2's four vectors do not fit: its passes take two tokens
        assert {k for k in launched if k.endswith(",2>")} == {f"k_pf_gemv_res_q4<{sp},2>" for sp in (4, 2, 1)}, sorted(launched)
    _LAUNCHED[name] = launched
    print(f"{name}: {n_ran} of {len(shapes)} shapes, {len(launched)} Q4 pass instantiations launched")


# ---- 3. the copy is what is read --------------------------------------------------------------
def test_the_copy_is_what_is_read(gpu):
    for on in (True, False):
        img = wc.exact_image("q4", SMALL, gpu)
        assert (img.data_ptr() + SMALL.header_bytes()) % 16 == 0  # from_device_image uses the image in place
        m = _model(img, SMALL, Q4, passes="0x1f") if on else _model(img, SMALL)
        try:
            rows0, rec0 = _results(m, SMALL)
            wc.poison_layer1(img, SMALL, wc.LAYER1, 0x55)  # the int8 values of layer 1; the scales stay
            rows1, rec1 = _results(m, SMALL)
            if on:
                assert rows0 == rows1 and rec0 == rec1
            else:  # the check of this test: the overwrite is in what a flag-off model streams
                assert rows0 != rows1 and rec0 != rec1
        finally:
            m.close()


# ---- 4. loops ---------------------------------------------------------------------------------
def test_loops_match(gpu, small_img):
    assert SMALL.vocab_size == wc.TIED.vocab_size  # pass_loops draws its tokens from that vocabulary
    res, logs = {}, {}
    for flags in (0, Q4):
        m = _model(small_img, SMALL, flags, passes="0x1f")
        try:
            assert m.q4_pass_info() == {"classes": ALL if flags else []}
            logs[flags] = set()
            res[flags] = wc.pass_loops(m, WIDTH, logs[flags])
        finally:
            m.close()
    a, b = res[0], res[Q4]
    for key in a:
        assert a[key] == b[key], f"{key}: flag off and on differ"
    assert len({tuple(w) for w in a["batch"]}) > WIDTH // 2  # the sequences wander apart
    assert "k_seq_attn_pfx" in logs[Q4] and "k_seq_qkv_q4" in logs[Q4], sorted(logs[Q4])  # best_of on the copy
    assert "k_seq_qkv" not in logs[Q4] and "k_seq_qkv" in logs[0]
    prompt = a["prompts"][3]
    total = len(prompt) + 40
    out = {}
    for flags in (0, Q4):
        m = _model(small_img, SMALL, flags, passes="0x1f")
        try:
            truth, _ = m.generate(prompt, total, exec="graph")
            with wc.launch_log() as read:
                words, _, stats = m.generate_lookup(prompt, total, hint=truth)
                log = wc.stems(read())
            assert words == truth and stats["accepted"] > 0, stats
            if flags:
                assert log & (STEMS | INT8_STEMS) == STEMS - {"k_seq_qkv_q4"}, sorted(log)
            out[flags] = (words, stats)
        finally:
            m.close()
    assert out[0] == out[Q4]


# ---- 5. no copy, no change --------------------------------------------------------------------
def test_no_copy_no_change(gpu, small_img):
    plain = binfmt.synth_image(SMALL, seed=4242, device=gpu, final_norm_std=1.0)  # +-127 in every group
    f32 = wc.spec(448, 1216, 7, 7, 999, False, 64, INTER, L, "q4p-f32")
    fimg = binfmt.synth_image(f32, seed=7, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    for img, spec, state, inject in ((plain, SMALL, -1, None), (fimg, f32, 0, None), (small_img, SMALL, -2, "q4")):
        m0 = _model(img, spec)
        with wc.hook("KH_SELFTEST_FAIL", inject) if inject else contextlib.nullcontext():
            m1 = _model(img, spec, Q4, passes="0x1f")
        try:
            assert m1.q4_info()["state"] == state and m1.q4_info()["classes"] == [], (state, m1.q4_info())
            assert m1.q4_pass_info() == {"classes": []}, state
            p0, d0 = _logged_passes(m0, spec)
            p1, d1 = _logged_passes(m1, spec)
            assert p0 == p1 == INT8_STEMS, (state, sorted(p0), sorted(p1))  # int8 or fp32: the same stems
            assert d0 == d1 and not d1 & DECODE_Q4, (state, sorted(d1))
            assert _results(m0, spec) == _results(m1, spec), state
        finally:
            m0.close()
            m1.close()


# ---- 6. coverage gate -------------------------------------------------------------------------
def test_coverage_gate(gpu):
    compiled = wc.coverage_gate(STEMS, GEOMETRIES, _LAUNCHED, "Q4 pass")
    assert len(compiled) == 12, sorted(compiled)
