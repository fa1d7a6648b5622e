"""Q4 (KH_FLAG_Q4) on the GPU: a model that streams the packed 4-bit copy of a 4-bit-exact int8 image computes the BITS
of the same image streamed as int8 - logits, K/V rows, tokens and log-prob records, compared with np.array_equal / as
bytes, never with a tolerance.

Models: 2 layers, 1024 cache rows, synth_image(seed fixed, final_norm_std=1.0) requantised to 4 bits
(binfmt.requantize_matrices_q4).  The two models of a comparison share one device image.  Where a test is about the
kernels, every launch class runs on the copy (hook KH_Q4_CLASSES=0x1f), whatever the default plan adopts.  Shapes, the
step loop and the comparisons are those of wcopy_cases.py.

  1. state: a requantised image -> state 1, the planned bytes and classes, the launch log of a step names the _q4 kernel
     of every adopted class and neither its int8 twin nor the ring kernel (the names are derived here from the planned
     shapes); a plain synth_image (+-127 in every group) -> state -1, first_inexact 0, an fp32 image -> state 0, both
     with the launches (and logits) of a flag-off model.
  2. bit identity under forced shapes: four geometries (dim 448 and 1152: masked lanes in every row; hidden 10368: w2
     staging depth 6 and SPLIT 4; head size 128 with interleaved RoPE; group 32 beside 64), for workgroups of 256 and
     512 threads every (u, split) each kernel accepts through KH_SHAPE_*, grids of one pair per wave, and two shapes
     with small odd grids; teacher-forced steps at positions 0, 1, 2 and - after random K/V rows were written below it
     - 300 (k_wo_comb_q4), into K/V rows that hold NaN.  The dim-448 image has -8, 7 and -1 planted in low and high
     nibbles of the first and the last unit of rows of every tensor.
  3. the copy is what is read: 0x55 over the int8 values of layer 1 does not change a flag-on model's logits and
     changes a flag-off model's.
  4. loops: generate, greedy and sampled with penalties, a logit bias and log-probs, exec graph and fused, across
     positions 250 .. 270; teacher-forced logits within the int8 bound (1e-4, tests/test_model_gpu.py) of the CPU
     oracle's int8 path on the requantised image; prefill, score and seq_step (they read the int8 image) equal.
  5. KH_SELFTEST_FAIL=q4 -> state -2, the int8 launches, the same logits.
  6. coverage gate: every compiled instantiation of the five _q4 stems was launched by (2); a launched name exists in
     the code objects.
"""
import numpy as np
import pytest
import torch

import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

EXACT = _ffi.KH_FLAG_PREFILL_EXACT
HALF, INTER, L = wc.HALF, wc.INTER, wc.L
INT8_ATOL = 1e-4  # tests/test_model_gpu.py: FULL_LOGIT_ATOL_Q8

GEOMETRIES = {
    "1152-h10368": wc.spec(1152, 10368, 18, 6, 1001, True, 64, HALF, L, "q4-1152"),  # 72 units; w2 depth 6 / 0, SPLIT 4
    "4224-h3072": wc.spec(4224, 3072, 33, 3, 777, True, 64, INTER, L, "q4-4224"),    # hs 128 interleaved; depth 4 / 0
    "960-g32-hs80": wc.spec(960, 1600, 12, 2, 1537, True, 32, HALF, L, "q4-g32"),    # group 32, 60 units, odd vocabulary
    "448": wc.spec(448, 1216, 7, 7, 999, True, 64, INTER, L, "q4-448"),              # 28 units: masked lanes; planted
}
SMALL = GEOMETRIES["448"]
STEMS = wc.DECODE["q4"]
GEMV = STEMS | wc.DECODE_INT8  # the launches a logged step keeps

_LAUNCHED = {}  # geometry -> _q4 instantiations its shapes launched (test_bit_identity -> test_coverage_gate)
_model, _hook = wc.model, wc.hook


def _q4_model(img, spec, flags=0):
    """flag on, every class on the copy"""
    return wc.model(img, spec, flags | _ffi.KH_FLAG_Q4, q4_classes="0x1f")


def _requantised(spec, gpu, plant=False):
    return wc.exact_image("q4", spec, gpu, plant=plant)


@pytest.fixture(scope="module")
def small_img(gpu):
    return _requantised(SMALL, gpu)


def _logged_step(m):
    return wc.logged_step(m, GEMV)


def _plan(spec):
    return _ffi.plan_q4(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, spec.n_layers, spec.quant,
                        spec.group_size)


def _maxv(n, wg, listed=(4, 2, 1, 0)):
    """kh_gemv.h::kh_stage_maxv, then kh_dispatch.h::kh_pick over a kernel's list (an unlisted depth takes the last)"""
    mv = 1 if n <= 4 * wg else 2 if n <= 8 * wg else 4 if n <= 16 * wg else 6 if n <= 24 * wg else 0
    return mv if mv in listed else listed[-1]


def _expected_step(spec, on):
    """{class: launch name} of one fused step at position 0 under the heuristic shapes, from the host-side plans: the
    _q4 kernel for a class in `on`, else what an int8 model launches (the ring kernel where plan_decode_ring has one)"""
    sh = _ffi.plan_decode_shapes(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, True)
    ring = _ffi.plan_decode_ring(spec.dim, spec.hidden_dim, spec.vocab_size, True, spec.group_size)

    def u_of(k):
        u = sh[k]["u"]
        return 4 if u >= 4 else (3 if u >= 3 and k == "w2" else 2)

    def name(stem, k, on_copy, split, n, listed=(4, 2, 1, 0)):
        args = [str(u_of(k)), str(_maxv(n, sh[k]["wg"], listed))] + ([str(sh[k]["split"])] if split else [])
        return f"{stem}_q4<{','.join(args)}>" if on_copy else f"{stem}<true,{','.join(args)}>"
    out = {"qkv": name("k_qkv", "qkv", "qkv" in on, True, spec.dim),
           "wo": name("k_gemv_res", "wo", "wo" in on, True, spec.dim),
           "w2": name("k_gemv_res", "w2", "w2" in on, True, spec.hidden_dim, (6, 4, 2, 1, 0))}
    for k, stem in (("ffn13", "k_ffn13"), ("cls", "k_cls")):
        if k not in on and ring[k]["slots"]:
            out[k] = f"{stem}_ring<2,4,false>"
        else:
            out[k] = name(stem, k, k in on, False, spec.dim)
    return out


# ---- 1. state ---------------------------------------------------------------------------------
def test_state_and_launches(gpu, small_img):
    assert binfmt.matrices_q4_exact(small_img, SMALL)
    m0 = _model(small_img, SMALL)
    m1 = _model(small_img, SMALL, _ffi.KH_FLAG_Q4)
    mall = _q4_model(small_img, SMALL)
    try:
        # fails on a library without the feature: no such entry point
        assert m0.q4_info() == {"state": 0, "bytes": 0, "build_us": 0, "classes": [], "first_inexact": -1}
        plan = _plan(SMALL)
        for m, classes in ((m1, plan["classes"]), (mall, list(_ffi.KH_Q4_CLASSES))):
            info = m.q4_info()
            assert info["state"] == 1 and info["first_inexact"] == -1, info
            assert info["bytes"] == plan["bytes"] > 0, info
            assert info["classes"] == classes, info
        log0, lg0 = _logged_step(m0)
        assert log0 == set(_expected_step(SMALL, ()).values()), sorted(log0)
        for m in (m1, mall):
            on = m.q4_info()["classes"]
            log1, lg1 = _logged_step(m)
            want = _expected_step(SMALL, on)
            assert log1 == set(want.values()), (on, sorted(log1), want)
            assert all(want[k].split("<")[0] in STEMS for k in on), want  # the _q4 kernel of every adopted class
            assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32)), on
        log_all = _logged_step(mall)[0]
        assert all(k.split("<")[0] in STEMS for k in log_all) and len(log_all) >= 4, sorted(log_all)
    finally:
        m0.close()
        m1.close()
        mall.close()


def test_inexact_and_fp32_images_launch_what_they_launch_today(gpu):
    plain = binfmt.synth_image(SMALL, seed=4242, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    m0, m1 = _model(plain, SMALL), _q4_model(plain, SMALL)
    try:
        info = m1.q4_info()
        assert info["state"] == -1 and info["bytes"] == 0 and info["classes"] == [], info
        assert info["first_inexact"] == 0, info  # wq of layer 0
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 == set(_expected_step(SMALL, ()).values()), (sorted(log0), sorted(log1))
        assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    finally:
        m0.close()
        m1.close()
    # one value of 8 at the very end of the LAST covered tensor (wcls is tensor 7 * layers); -8 elsewhere is exact
    img = _requantised(SMALL, gpu)
    last = binfmt.q4_tensors(SMALL)[-1][0]
    binfmt.tensor_from_image(img, binfmt.q4_tensors(SMALL)[0][0])[0, 0] = -8
    binfmt.tensor_from_image(img, last)[-1, -1] = 8
    torch.cuda.synchronize()
    m = _q4_model(img, SMALL)
    try:
        info = m.q4_info()
        assert info["state"] == -1 and info["first_inexact"] == 7 * SMALL.n_layers, info
    finally:
        m.close()
    f32 = wc.spec(448, 1216, 7, 7, 999, False, 64, INTER, L, "q4-f32")
    fimg = binfmt.synth_image(f32, seed=7, device=gpu)
    torch.cuda.synchronize()
    m0, m1 = _model(fimg, f32), _q4_model(fimg, f32)
    try:
        assert m1.q4_info() == {"state": 0, "bytes": 0, "build_us": 0, "classes": [], "first_inexact": -1}
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 and log0 and not any(k.split("<")[0] in STEMS for k in log1), sorted(log1)
        assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    finally:
        m0.close()
        m1.close()
    # KH_FLAG_W16* on an int8 image stays state 0
    m = _model(_requantised(SMALL, gpu), SMALL, _ffi.KH_FLAG_W16 | _ffi.KH_FLAG_W16_F16)
    try:
        assert m.w16_info()["state"] == 0 and m.q4_info()["state"] == 0
    finally:
        m.close()


def test_hooks_override_the_flag_and_the_plan(gpu, small_img):
    int8 = set(_expected_step(SMALL, ()).values())
    with _hook("KH_Q4", "1"):
        m = _model(small_img, SMALL)
    try:
        assert m.q4_info()["state"] == 1
    finally:
        m.close()
    with _hook("KH_Q4", "0"):
        m = _model(small_img, SMALL, _ffi.KH_FLAG_Q4)
    try:
        assert m.q4_info()["state"] == 0 and _logged_step(m)[0] == int8
    finally:
        m.close()
    with _hook("KH_Q4_CLASSES", "0x9"):  # qkv and w2 alone: the other classes keep their int8 launches
        m = _model(small_img, SMALL, _ffi.KH_FLAG_Q4)
    try:
        assert m.q4_info()["classes"] == ["qkv", "w2"]
        assert _logged_step(m)[0] == set(_expected_step(SMALL, ("qkv", "w2")).values())
    finally:
        m.close()
    with _hook("KH_Q4_CLASSES", "0"):  # a copy nobody reads
        m = _model(small_img, SMALL, _ffi.KH_FLAG_Q4)
    try:
        assert m.q4_info()["state"] == 1 and m.q4_info()["classes"] == [] and _logged_step(m)[0] == int8
    finally:
        m.close()


# ---- 2. bit identity under forced shapes ------------------------------------------------------
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes(gpu, name):
    spec = GEOMETRIES[name]
    img = _requantised(spec, gpu, plant=spec is SMALL)
    assert binfmt.matrices_q4_exact(img, spec)
    rng = np.random.default_rng(7)
    steps = wc.steps(spec, rng)
    rows = wc.deep_rows(spec, rng)
    shapes = wc.decode_shapes(spec)
    launched = set()
    try:
        for i, sh in enumerate(shapes):
            what = f"{name} shape {i} {sh}"
            wc.set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _q4_model(img, spec)
            try:
                info = m1.q4_info()
                assert info["state"] == 1 and info["classes"] == list(_ffi.KH_Q4_CLASSES), (what, info)
                launched |= wc.compare_steps(m0, m1, spec, steps, rows, what, STEMS, GEMV)[0]
            finally:
                m0.close()
                m1.close()
    finally:
        wc.set_shape_hooks({})
    _LAUNCHED[name] = launched
    print(f"{name}: {len(shapes)} shapes, {len(launched)} Q4 instantiations launched")


# ---- 3. the copy is what is read --------------------------------------------------------------
def test_the_copy_is_what_is_read(gpu):
    for on in (True, False):
        img = _requantised(SMALL, gpu)
        assert (img.data_ptr() + SMALL.header_bytes()) % 16 == 0  # from_device_image uses the image in place
        m = _q4_model(img, SMALL) if on else _model(img, SMALL)
        try:
            t0 = m.predict(5, 0, exec="fused")
            before = m.logits()
            assert np.isfinite(before).all()
            wc.poison_layer1(img, SMALL, wc.LAYER1, 0x55)  # the int8 values of layer 1; the scales stay
            t1 = m.predict(5, 0, exec="fused")  # a batch-1 step: no B-token call follows the overwrite
            after = m.logits()
            if on:
                assert t0 == t1 and np.array_equal(before.view(np.uint32), after.view(np.uint32))
            else:  # the check of this test: the overwrite is in what a flag-off model streams
                assert not np.array_equal(before.view(np.uint32), after.view(np.uint32))
        finally:
            m.close()


# ---- 4. loops ---------------------------------------------------------------------------------
def test_generate_loops_match(gpu, small_img):
    res = {}
    for on in (False, True):
        m = _q4_model(small_img, SMALL, EXACT) if on else _model(small_img, SMALL, EXACT)
        try:
            assert m.q4_info()["state"] == (1 if on else 0)
            res[on] = wc.generate_loops(m)
        finally:
            m.close()
    wc.assert_loops_equal(res[False], res[True])


def test_requantised_image_is_an_ordinary_int8_checkpoint(gpu, oracle, small_img):
    """anchor outside the library: the CPU oracle's int8 path on the requantised image, teacher-forced"""
    om = oracle.OracleModel.from_spec(small_img.cpu().numpy(), SMALL, cache_len=wc.CACHE)
    m = _q4_model(small_img, SMALL)
    try:
        rng = np.random.default_rng(3)
        worst = 0.0
        for pos, tok in enumerate(int(t) for t in rng.integers(0, SMALL.vocab_size, 8)):
            m.predict(tok, pos, exec="fused")
            d = float(np.abs(m.logits() - om.forward(tok, pos)).max())
            worst = max(worst, d)
            print(f"pos {pos}: |logit - oracle| {d:.3e}")
        assert worst <= INT8_ATOL, worst
    finally:
        m.close()
        om.close()


def test_b_token_passes_are_the_int8_models(gpu, small_img):
    rng = np.random.default_rng(19)
    toks = [int(t) for t in rng.integers(0, SMALL.vocab_size, 9)]
    res = []
    for on in (False, True):
        m = _q4_model(small_img, SMALL, EXACT) if on else _model(small_img, SMALL, EXACT)
        try:
            r = {}
            m.prefill(toks[:6], 0)
            kv = [m.read_kv(layer, 0, 6) for layer in range(SMALL.n_layers)]
            r["prefill"] = b"".join(k.tobytes() + v.tobytes() for k, v in kv)
            m.set_logprobs(3)
            sc = m.score(toks, 0)
            r["score"] = wc.rec_bytes(sc)
            m.set_logprobs(None)
            slot_len = m.seq_slots(2)
            m.seq_prefill(0, toks[:3], 0)
            m.seq_prefill(1, toks[3:6], 0)
            r["seq_step"] = tuple(m.seq_step([0, 1], [toks[6], toks[7]], [3, 3]))
            rows = [m.read_kv(layer, s * slot_len, 4) for layer in range(SMALL.n_layers) for s in (0, 1)]
            r["seq_rows"] = b"".join(k.tobytes() + v.tobytes() for k, v in rows)
            res.append(r)
        finally:
            m.close()
    for key in res[0]:
        assert res[0][key] == res[1][key], f"{key}: flag off and on differ"


# ---- 5. self-check ----------------------------------------------------------------------------
def test_selfcheck_failure_falls_back_to_int8(gpu, small_img):
    m0 = _model(small_img, SMALL)
    with _hook("KH_SELFTEST_FAIL", "q4"):
        m1 = _q4_model(small_img, SMALL)
    try:
        info = m1.q4_info()
        assert info["state"] == -2 and info["bytes"] == 0 and info["classes"] == [], info
        log0, lg0 = _logged_step(m0)
        log1, lg1 = _logged_step(m1)
        assert log0 == log1 == set(_expected_step(SMALL, ()).values()), sorted(log1)
        assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
        t0, t1 = m0.generate([1, 7], 24, exec="graph")[0], m1.generate([1, 7], 24, exec="graph")[0]
        assert t0 == t1
    finally:
        m0.close()
        m1.close()


# ---- 6. coverage gate -------------------------------------------------------------------------
def test_coverage_gate(gpu):
    wc.coverage_gate(STEMS, GEOMETRIES, _LAUNCHED, "Q4")
