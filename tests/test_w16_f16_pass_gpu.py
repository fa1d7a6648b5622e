"""The B-token passes of fp16-format W16 models (KH_FLAG_W16_F16) on the GPU: prefill, score, verify / generate_lookup
and the sequence-slot calls stream the fp16-format 16-bit copy and leave the BITS of the same image streamed as fp32 -
K/V rows, records, picks and words compared as raw words / bytes, never with a tolerance.

Mirrors test_w16_pass_gpu.py (the geometries, widths, shapes and call sequence of wcopy_cases.py, as there) on images
whose matrices are rounded to fp16 (binfmt.round_matrices_fp16).

  1. state and launches: every class's pass on the copy (KH_W16_PASS=0x1f) -> only _h16 pass stems; the default mask
     and a class mask -> exactly their classes; 0 -> the fp32 stems while a predict logs the decode _h16 kernels.
  2. bit identity: per geometry the forced shapes of test_w16_pass_gpu.py under KH_W16_PASS=0x1f, then the first of
     them that runs the B-token pass again under the default mask and under 0: prefills of 1, width and 2 width + 1 tokens, one across position 256, a
     verify with a wrong draft in the middle, a score with records, a seq_step over shuffled slots.  After every call
     the whole cache of both models is compared, and every row the call does not own against what it held before.
  3. the copy is what is read: NaN over the fp32 matrices of layer 1 and the classifier.
  4. loops: generate_batch, best_of(share=True) and generate_lookup, flag off against flag on.
  5. coverage gate: every compiled instantiation of the five _h16 pass stems was launched and compared by (2).
"""
import numpy as np
import pytest

import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

F16 = _ffi.KH_FLAG_W16_F16  # fails on a library without the feature
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
GEOMETRIES, WIDTH, TIED, QWEN = wc.GEOMETRIES_F32, wc.WIDTH, wc.TIED, wc.QWEN
ALL = list(_ffi.KH_W16_CLASSES)
DEFAULT = ["ffn13", "w2"]  # the classes whose pass reads the copy unless KH_W16_PASS says otherwise
STEMS, W16_STEMS, FP32_STEMS = wc.PASS["h16"], wc.PASS["w16"], wc.PASS_F32
DECODE_H16 = wc.DECODE["h16"]
DECODE_ANY = DECODE_H16 | wc.DECODE["w16"]

_LAUNCHED = {}  # geometry -> _h16 pass instantiations its shapes launched (test_bit_identity -> test_coverage_gate)
_model = wc.model


@pytest.fixture(scope="module")
def tied_img(gpu):
    return wc.exact_image("h16", TIED, gpu)


def _logged_passes(m, spec):
    return wc.logged_passes(m, spec, STEMS | W16_STEMS | FP32_STEMS)  # fp32, _w16 or _h16


# ---- 1. state and launches --------------------------------------------------------------------
def test_state_and_launches(gpu, tied_img):
    m1 = _model(tied_img, TIED, F16, passes="0x1f")
    md = _model(tied_img, TIED, F16)
    try:
        for m in (m1, md):
            assert m.w16_info()["state"] == 1 and m.w16_format()["format"] == "fp16"
        assert m1.w16_pass_info() == {"classes": ALL} and md.w16_pass_info() == {"classes": DEFAULT}
        p1, d1 = _logged_passes(m1, TIED)
        pd, dd = _logged_passes(md, TIED)
        assert p1 == STEMS, sorted(p1)
        # wo and w2 share a stem: the default mask launches both forms of it
        assert pd == {"k_pf_qkv", "k_seq_qkv", "k_pf_gemv_res", "k_pf_gemv_res_h16", "k_pf_ffn13_h16", "k_pf_cls"}, sorted(pd)
        assert d1 & DECODE_ANY == dd & DECODE_ANY == DECODE_H16 - {"k_wo_comb_h16"}, (sorted(d1), sorted(dd))
    finally:
        m1.close()
        md.close()
    m = _model(tied_img, TIED, F16, passes="0")
    try:
        assert m.w16_info()["classes"] == ALL and m.w16_pass_info() == {"classes": []}
        p, d = _logged_passes(m, TIED)
        assert p == FP32_STEMS, sorted(p)
        assert d & DECODE_ANY == DECODE_H16 - {"k_wo_comb_h16"}, sorted(d)  # decode still reads the copy
    finally:
        m.close()
    m = _model(tied_img, TIED, F16, passes="0x11")  # qkv and cls
    try:
        assert m.w16_pass_info() == {"classes": ["qkv", "cls"]}
        p, _ = _logged_passes(m, TIED)
        assert p == {"k_pf_qkv_h16", "k_seq_qkv_h16", "k_pf_gemv_res", "k_pf_ffn13", "k_pf_cls_h16"}, sorted(p)
    finally:
        m.close()


# ---- 2. bit identity --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes_and_masks(gpu, name):
    spec, width = GEOMETRIES[name], WIDTH[name]
    img = wc.exact_image("h16", spec, gpu)
    assert binfmt.matrices_fp16_exact(img, spec) and not binfmt.matrices_bf16_exact(img, spec)
    shapes = wc.pass_shapes(spec)
    # (shape hooks, KH_W16_PASS, the classes it leaves): every forced shape with all five classes on the copy, then the
    # first of them that prefill_supported admits under the default mask and with the passes on fp32
    runs = [(sh, "0x1f", ALL) for sh in shapes]
    launched, n_ran, i = set(), 0, -1
    try:
        while i + 1 < len(runs):
            i += 1
            sh, passes, classes = runs[i]
            what = f"{name} run {i} {sh} KH_W16_PASS={passes}"
            wc.set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _model(img, spec, F16, passes=passes)
            try:
                assert m1.w16_info()["state"] == 1 and m1.w16_format()["format"] == "fp16", what
                assert m1.w16_pass_info() == {"classes": classes}, what
                try:
                    assert m1.verify_width() == width == m0.verify_width(), what
                except _ffi.KhError as e:
                    assert e.code == _ffi.KH_ERR_UNSUPPORTED and passes == "0x1f", e  # outside prefill_supported
                    continue
                if n_ran == 0:
                    runs += [(sh, None, DEFAULT), (sh, "0", [])]
                with wc.launch_log() as read:  # after creation; m0 logs into it too: only _h16 names are kept
                    wc.run_pass_shape(m0, m1, spec, width, what, 7 + i)
                    log = read()
                assert not any(wc.stem(k) in W16_STEMS for k in log), f"{what}: a bf16 twin was launched"
                mine = {k for k in log if k.split("<")[0] in STEMS}
                assert bool(mine) == bool(classes), what
                launched |= mine
                n_ran += 1
            finally:
                m0.close()
                m1.close()
    finally:
        wc.set_shape_hooks({})
    assert n_ran >= 6, f"{name}: only {n_ran} runs reached the B-token pass"
    _LAUNCHED[name] = launched
    print(f"{name}: {n_ran} of {len(runs)} runs, {len(launched)} _h16 pass instantiations launched")


def test_a_flag_on_pass_launches_no_fp32_twin_under_forced_shapes(gpu, tied_img):
    """the log of test 2 is shared by its two models; here the flag-on model runs alone"""
    try:
        wc.set_shape_hooks(wc.pass_shapes(TIED)[1])
        m = _model(tied_img, TIED, F16, passes="0x1f")
        try:
            p, _ = _logged_passes(m, TIED)
            assert p == STEMS, sorted(p)
        finally:
            m.close()
    finally:
        wc.set_shape_hooks({})


# ---- 3. the copy is what is read --------------------------------------------------------------
def test_the_copy_is_what_is_read(gpu):
    spec = QWEN
    rng = np.random.default_rng(5)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, 9)]
    prompts = [toks[:1], toks[2:5], toks[4:9]]
    for flags in (F16, 0):
        img = wc.exact_image("h16", spec, gpu)
        assert (img.data_ptr() + spec.header_bytes()) % 16 == 0  # from_device_image uses the image in place
        m = _model(img, spec, flags, passes="0x1f")
        try:
            m.seq_slots(4)
            w0, _ = m.generate_batch(prompts, [12, 10, 14])
            m.set_logprobs(5)
            r0 = m.score(toks, 0)
            assert np.isfinite(r0["logprob"][:-1]).all()
            wc.poison_layer1(img, spec, wc.LAYER1 | {"wcls"}, float("nan"))
            r1 = m.score(toks, 0)
            if flags:
                assert m.w16_format()["format"] == "fp16"
                assert wc.rec_bytes(r0) == wc.rec_bytes(r1)
                m.set_logprobs(None)
                w1, _ = m.generate_batch(prompts, [12, 10, 14])
                assert w0 == w1 and all(w0)
            else:  # the check of this test: the poison is in what a flag-off model streams
                assert np.isnan(r1["logprob"][:-1]).all()
        finally:
            m.close()


# ---- 4. loops ---------------------------------------------------------------------------------
def test_loops_match(gpu, tied_img):
    width = WIDTH["448-tied"]
    res, logs = {}, {}
    for flags in (EXACT, EXACT | F16):
        m = _model(tied_img, TIED, flags, passes="0x1f")
        try:
            assert m.w16_pass_info() == {"classes": ALL if flags & F16 else []}
            logs[flags] = set()
            res[flags] = wc.pass_loops(m, width, logs[flags])  # generate_batch three ways, best_of(share=True)
        finally:
            m.close()
    a, b = res[EXACT], res[EXACT | F16]
    for key in a:
        assert a[key] == b[key], f"{key}: flag off and on differ"
    assert len({tuple(w) for w in a["batch"]}) > width // 2  # the sequences wander apart
    assert "k_seq_attn_pfx" in logs[EXACT | F16] and "k_seq_qkv_h16" in logs[EXACT | F16], sorted(logs[EXACT | F16])
    assert "k_seq_qkv" not in logs[EXACT | F16] and "k_seq_qkv" in logs[EXACT]
    # generate_lookup with the truth as hint, and one sequence of the batch against a flag-on batch-1 model
    prompt = a["prompts"][3]
    total = len(prompt) + 40
    out = {}
    for flags in (EXACT, EXACT | F16):
        m = _model(tied_img, TIED, flags, passes="0x1f")
        try:
            truth, _ = m.generate(prompt, total, exec="graph")
            with wc.launch_log() as read:
                words, _, stats = m.generate_lookup(prompt, total, hint=truth)
                log = wc.stems(read())
            assert words == truth and stats["accepted"] > 0, stats
            if flags & F16:
                assert log & (STEMS | W16_STEMS | FP32_STEMS) == STEMS - {"k_seq_qkv_h16"}, sorted(log)
                for s in (0, 2):
                    m.set_sampling(**a["samp"][s])
                    got, _ = m.generate(a["prompts"][s], a["totals"][s], exec="graph")
                    assert got == b["batch"][s], f"sequence {s} of the batch against generate"
                m.set_sampling()
            out[flags] = (words, stats)
        finally:
            m.close()
    assert out[EXACT] == out[EXACT | F16]


# ---- 5. coverage gate -------------------------------------------------------------------------
def test_coverage_gate(gpu):
    compiled = wc.coverage_gate(STEMS, GEOMETRIES, _LAUNCHED, "_h16 pass")
    assert len(compiled) == 21, sorted(compiled)
