"""The B-token passes of W16 models on the GPU (kh_w16_pass.h): prefill, score, verify / generate_lookup and the
sequence-slot calls of a KH_FLAG_W16 model stream the 16-bit copy and leave the BITS of the same image streamed as
fp32 - K/V rows, records, picks and words compared as raw words / bytes, never with a tolerance.

Models: 2 layers, 1024 cache rows, synth_image(seed fixed, final_norm_std=1.0) with its matrices rounded to bf16
(binfmt.round_matrices_bf16) at the four fp32 geometries of wcopy_cases.py: 8 tokens per pass at dim 448 / 960 / 1152,
4 at dim 4224 (eight vectors exceed 80 KiB), 2 for w2 at hidden 10368.  The two models of a comparison share one
device image.  Shapes, the call sequence of (2) and the loops of (4) are those of wcopy_cases.py.

  1. state and launches: flag on with every class's pass on the copy (KH_W16_PASS=0x1f) -> a prefill, a score and a
     seq_step log only _w16 stems for the five pass classes; the default mask (ffn13, w2: DESIGN 3.1c's adoption) and
     any other class mask -> exactly their classes; KH_W16_PASS=0 -> the fp32 stems while a predict still logs the
     decode _w16 kernels; an unrounded image (state -1) and int8 -> the flag-off launches.  w16_pass_info() agrees in
     each case.  Tests 2 - 4 run under KH_W16_PASS=0x1f: all five classes are compared, adopted by default or not.
  2. bit identity under forced shapes: per geometry every (split, workgroup width) KH_SHAPE_* accept and
     prefill_supported admits, plus a shape with small odd grids; prefill of 1, width and 2 width + 1 tokens, a
     prefill across position 256 over random rows, a verify whose first wrong draft sits in the middle, a score with
     top-5 records and a seq_step over lanes at unequal positions in shuffled slots.  After every call the whole
     cache of both models is compared, and every row the call does not own against what it held before.
  3. the copy is what is read: NaN over the fp32 matrices of layer 1 and the classifier leaves a flag-on model's
     score records and generate_batch words as they were and turns a flag-off model's log-probs into NaN.
  4. loops: generate_batch (width + 1 sequences, sampled, a stop token; penalties, bias and records), best_of over a
     shared prefix and generate_lookup with a truthful hint, flag off against flag on; one sequence against generate
     of a flag-on batch-1 model.
  5. coverage gate: every compiled instantiation of the five stems was launched and compared by (2).
"""
import numpy as np
import pytest
import torch

import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

W16 = _ffi.KH_FLAG_W16
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
GEOMETRIES, WIDTH, TIED, QWEN = wc.GEOMETRIES_F32, wc.WIDTH, wc.TIED, wc.QWEN
STEMS, FP32_STEMS, DECODE_W16 = wc.PASS["w16"], wc.PASS_F32, wc.DECODE["w16"]
ALL = list(_ffi.KH_W16_CLASSES)
DEFAULT = ["ffn13", "w2"]  # the classes whose pass reads the copy unless KH_W16_PASS says otherwise

_LAUNCHED = {}  # geometry -> _w16 pass instantiations its shapes launched (test_bit_identity -> test_coverage_gate)
_model = wc.model


@pytest.fixture(scope="module")
def tied_img(gpu):
    return wc.exact_image("w16", TIED, gpu)


def _logged_passes(m, spec):
    return wc.logged_passes(m, spec, STEMS | FP32_STEMS)


# ---- 1. state and launches --------------------------------------------------------------------
def test_state_and_launches(gpu, tied_img):
    m0 = _model(tied_img, TIED)
    m1 = _model(tied_img, TIED, W16, passes="0x1f")
    md = _model(tied_img, TIED, W16)
    try:
        # fails on a library without the feature: no such entry point
        assert m0.w16_pass_info() == {"classes": []}
        assert m1.w16_info()["state"] == 1 and m1.w16_pass_info() == {"classes": ALL}
        assert md.w16_info()["classes"] == ALL and md.w16_pass_info() == {"classes": DEFAULT}
        p0, d0 = _logged_passes(m0, TIED)
        p1, d1 = _logged_passes(m1, TIED)
        pd, dd = _logged_passes(md, TIED)
        assert p0 == FP32_STEMS, sorted(p0)
        assert p1 == STEMS, sorted(p1)
        # wo and w2 share a stem: the default mask launches both forms of it
        assert pd == {"k_pf_qkv", "k_seq_qkv", "k_pf_gemv_res", "k_pf_gemv_res_w16", "k_pf_ffn13_w16", "k_pf_cls"}, sorted(pd)
        assert not d0 & DECODE_W16, sorted(d0)
        assert d1 & DECODE_W16 == dd & DECODE_W16 == DECODE_W16 - {"k_wo_comb_w16"}, (sorted(d1), sorted(dd))
    finally:
        m0.close()
        m1.close()
        md.close()


def test_hook_keeps_the_passes_on_fp32_or_picks_classes(gpu, tied_img):
    m = _model(tied_img, TIED, W16, passes="0")
    try:
        assert m.w16_info()["classes"] == ALL and m.w16_pass_info() == {"classes": []}
        p, d = _logged_passes(m, TIED)
        assert p == FP32_STEMS, sorted(p)
        assert d & DECODE_W16 == DECODE_W16 - {"k_wo_comb_w16"}, sorted(d)  # decode still reads the copy
    finally:
        m.close()
    m = _model(tied_img, TIED, W16, passes="0x11")  # qkv and cls
    try:
        assert m.w16_pass_info() == {"classes": ["qkv", "cls"]}
        p, _ = _logged_passes(m, TIED)
        assert p == {"k_pf_qkv_w16", "k_seq_qkv_w16", "k_pf_gemv_res", "k_pf_ffn13", "k_pf_cls_w16"}, sorted(p)
    finally:
        m.close()
    m = _model(tied_img, TIED, W16, passes="1")
    try:
        assert m.w16_pass_info() == {"classes": DEFAULT}
    finally:
        m.close()
    m = _model(tied_img, TIED, passes="0x1f")  # the hook does not switch the copy on
    try:
        assert m.w16_info()["state"] == 0 and m.w16_pass_info() == {"classes": []}
    finally:
        m.close()


def test_inexact_and_int8_images_launch_what_they_launch_today(gpu):
    plain = binfmt.synth_image(TIED, seed=4242, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    q8 = wc.spec(512, 1408, 8, 8, 501, True, 64, wc.INTER, wc.L, "w16-q8")
    qimg = binfmt.synth_image(q8, seed=7, device=gpu)
    torch.cuda.synchronize()
    for img, spec, state in ((plain, TIED, -1), (qimg, q8, 0)):
        m0, m1 = _model(img, spec), _model(img, spec, W16, passes="0x1f")
        try:
            assert m1.w16_info()["state"] == state and m1.w16_pass_info() == {"classes": []}
            p0, d0 = _logged_passes(m0, spec)
            p1, d1 = _logged_passes(m1, spec)
            assert p0 == p1 == FP32_STEMS, (sorted(p0), sorted(p1))
            assert d0 == d1 and not d1 & DECODE_W16, sorted(d1)
        finally:
            m0.close()
            m1.close()


# ---- 2. bit identity under forced shapes ------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes(gpu, name):
    spec, width = GEOMETRIES[name], WIDTH[name]
    img = wc.exact_image("w16", spec, gpu)
    assert binfmt.matrices_bf16_exact(img, spec)
    shapes = wc.pass_shapes(spec)
    launched, n_ran = set(), 0
    try:
        for i, sh in enumerate(shapes):
            what = f"{name} shape {i} {sh}"
            wc.set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _model(img, spec, W16, passes="0x1f")
            try:
                assert m1.w16_info()["state"] == 1 and m1.w16_pass_info() == {"classes": ALL}, what
                try:
                    assert m1.verify_width() == width == m0.verify_width(), what
                except _ffi.KhError as e:
                    assert e.code == _ffi.KH_ERR_UNSUPPORTED, e  # the shape is outside prefill_supported
                    continue
                with wc.launch_log() as read:  # after creation; m0 logs into it too: only _w16 names are kept
                    wc.run_pass_shape(m0, m1, spec, width, what, 7 + i)
                    launched |= {k for k in read() if wc.stem(k) in STEMS}
                n_ran += 1
            finally:
                m0.close()
                m1.close()
    finally:
        wc.set_shape_hooks({})
    assert n_ran >= 4, f"{name}: only {n_ran} shapes ran the B-token pass"
    _LAUNCHED[name] = launched
    print(f"{name}: {n_ran} of {len(shapes)} shapes, {len(launched)} W16 pass instantiations launched")


def test_a_flag_on_pass_launches_no_fp32_twin_under_forced_shapes(gpu, tied_img):
    """the log of test 2 is shared by its two models; here the flag-on model runs alone"""
    try:
        wc.set_shape_hooks(wc.pass_shapes(TIED)[1])
        m = _model(tied_img, TIED, W16, passes="0x1f")
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
    for flags in (W16, 0):
        img = wc.exact_image("w16", spec, gpu)
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
    for flags in (EXACT, EXACT | W16):
        m = _model(tied_img, TIED, flags, passes="0x1f")
        try:
            assert m.w16_pass_info() == {"classes": ALL if flags & W16 else []}
            logs[flags] = set()
            res[flags] = wc.pass_loops(m, width, logs[flags])
        finally:
            m.close()
    a, b = res[EXACT], res[EXACT | W16]
    for key in a:
        assert a[key] == b[key], f"{key}: flag off and on differ"
    assert len({tuple(w) for w in a["batch"]}) > width // 2  # the sequences wander apart
    assert "k_seq_attn_pfx" in logs[EXACT | W16] and "k_seq_qkv_w16" in logs[EXACT | W16], sorted(logs[EXACT | W16])
    assert "k_seq_qkv" not in logs[EXACT | W16] and "k_seq_qkv" in logs[EXACT]
    # generate_lookup with the truth as hint, and one sequence of the batch against a flag-on batch-1 model
    prompt = a["prompts"][3]
    total = len(prompt) + 40
    out = {}
    for flags in (EXACT, EXACT | W16):
        m = _model(tied_img, TIED, flags, passes="0x1f")
        try:
            truth, _ = m.generate(prompt, total, exec="graph")
            with wc.launch_log() as read:
                words, _, stats = m.generate_lookup(prompt, total, hint=truth)
                log = wc.stems(read())
            assert words == truth and stats["accepted"] > 0, stats
            if flags & W16:
                assert log & (STEMS | FP32_STEMS) == STEMS - {"k_seq_qkv_w16"}, sorted(log)
                for s in (0, 2):
                    m.set_sampling(**a["samp"][s])
                    got, _ = m.generate(a["prompts"][s], a["totals"][s], exec="graph")
                    assert got == b["batch"][s], f"sequence {s} of the batch against generate"
                m.set_sampling()
            out[flags] = (words, stats)
        finally:
            m.close()
    assert out[EXACT] == out[EXACT | W16]


# ---- 5. coverage gate -------------------------------------------------------------------------
def test_coverage_gate(gpu):
    wc.coverage_gate(STEMS, GEOMETRIES, _LAUNCHED, "W16 pass")
