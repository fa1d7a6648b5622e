"""W16 (KH_FLAG_W16) on the GPU: a model that streams the 16-bit copy of a bf16-exact image computes the BITS of the
same image streamed as fp32 - logits, K/V rows, tokens and log-prob records, compared with np.array_equal / as bytes,
never with a tolerance.

Models: 2 layers, 1024 cache rows, synth_image(seed fixed, final_norm_std=1.0) with its matrices rounded to bf16
(binfmt.round_matrices_bf16).  The two models of a comparison share one device image.

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
import itertools

import numpy as np
import pytest
import torch

import code_objects as co
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

CACHE = 1024
DEEP_POS = 300
W16 = _ffi.KH_FLAG_W16
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
L, Q2 = binfmt.FAMILY_LLAMA, binfmt.FAMILY_QWEN2
HALF, INTER = binfmt.ROPE_HALF, binfmt.ROPE_INTERLEAVED


def _spec(dim, hidden, heads, kv_heads, vocab, rope, family, name, tied=False, quant=False):
    q = family == Q2
    return binfmt.ModelSpec(dim, hidden, 2, heads, kv_heads, vocab, CACHE, tied, family, quant, 64, rope,
                            1000000.0 if q else 10000.0, 1e-6 if q else 1e-5, name)


GEOMETRIES = {
    "1152-h10368": _spec(1152, 10368, 18, 6, 1001, HALF, L, "w16-1152"),          # w2 depth 6 / 0
    "4224-h3072": _spec(4224, 3072, 33, 3, 777, INTER, L, "w16-4224"),            # hs 128, depth 4 / 0
    "qwen-960-hs80": _spec(960, 1600, 12, 2, 1537, HALF, Q2, "w16-qwen"),         # bias, 240 units: masked lanes
    "448-tied": _spec(448, 1216, 7, 7, 999, INTER, L, "w16-tied", tied=True),     # the copy of tok_emb
}
TIED = GEOMETRIES["448-tied"]
STEMS = {"k_qkv_w16", "k_gemv_res_w16", "k_wo_comb_w16", "k_ffn13_w16", "k_cls_w16"}
FP32_STEMS = {"k_qkv", "k_gemv_res", "k_wo_comb", "k_ffn13", "k_cls"}
# the decode GEMV launches of one fused step at position 0 of the 448-tied geometry under its heuristic shapes
# (qkv / wo / ffn13: u 2, 256 threads, staging depth 1; w2: u 4, 512 threads; cls: u 2, 512 threads; no split)
TIED_STEP_FP32 = {"k_qkv<false,2,1,1>", "k_gemv_res<false,2,1,1>", "k_ffn13<false,2,1>", "k_gemv_res<false,4,1,1>",
                  "k_cls<false,2,1>"}
TIED_STEP_W16 = {"k_qkv_w16<2,1,1>", "k_gemv_res_w16<2,1,1>", "k_ffn13_w16<2,1>", "k_gemv_res_w16<4,1,1>",
                 "k_cls_w16<2,1>"}

_LAUNCHED = {}  # geometry -> _w16 instantiations its shapes launched (test_bit_identity -> test_coverage_gate)


def _model(img, spec, flags=0):
    from kuiperllama_amd.model import KuiperModel
    return KuiperModel.from_device_image(img, spec, flags=flags)


def _rounded(spec, gpu, seed=4242):
    img = binfmt.synth_image(spec, seed=seed, device=gpu, final_norm_std=1.0)
    binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()
    return img


@pytest.fixture(scope="module")
def tied_img(gpu):
    return _rounded(TIED, gpu)


def _gemv_log(log):
    return {k for k in log if k.split("<")[0] in STEMS | FP32_STEMS}


def _logged_step(m, tok=5, pos=0):
    """(GEMV launches, logits) of one fused step"""
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        m.predict(tok, pos, exec="fused")
        lg = m.logits()
        return _gemv_log(_ffi.launch_log()), lg
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)


def _planned_bytes(spec):
    return _ffi.plan_w16(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, spec.n_layers, spec.quant)["bytes"]


# ---- 1. state ---------------------------------------------------------------------------------
def test_state_and_launches(gpu, tied_img):
    m0 = _model(tied_img, TIED)
    m1 = _model(tied_img, TIED, W16)
    try:
        # fails on a library without the feature: no such entry point
        assert m0.w16_info() == {"state": 0, "bytes": 0, "build_us": 0, "classes": [], "first_inexact": -1}
        info = m1.w16_info()
        assert info["state"] == 1 and info["first_inexact"] == -1, info
        assert info["bytes"] == _planned_bytes(TIED) > 0, info
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
    img = _rounded(TIED, gpu)
    e = [t for t in binfmt.layout(TIED)[0] if t.name == "tok_emb"][0]
    img[e.offset + e.nbytes - 4] |= 1
    torch.cuda.synchronize()
    m = _model(img, TIED, W16)
    try:
        info = m.w16_info()
        assert info["state"] == -1 and info["first_inexact"] == 7 * TIED.n_layers, info
    finally:
        m.close()
    q8 = _spec(512, 1408, 8, 8, 501, INTER, L, "w16-q8", quant=True)
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
    try:
        _ffi.debug_set("KH_W16", "1")
        m = _model(tied_img, TIED)
        try:
            assert m.w16_info()["state"] == 1
        finally:
            m.close()
        _ffi.debug_set("KH_W16", "0")
        m = _model(tied_img, TIED, W16)
        try:
            assert m.w16_info()["state"] == 0 and _logged_step(m)[0] == TIED_STEP_FP32
        finally:
            m.close()
    finally:
        _ffi.debug_set("KH_W16", None)


# ---- 2. bit identity under forced shapes ------------------------------------------------------
def _shapes(spec):
    """{hook suffix: (split, u, grid, wg)}: per workgroup width nine shapes that walk every (u, split) each kernel
    accepts (qkv: split <= 2, ffn13 / cls: 1), grids of one pair per wave; then two of them with small odd grids."""
    us = (2, 4, 8)
    combos = {"QKV": list(itertools.product(us, (1, 2))), "WO": list(itertools.product(us, (1, 2, 4))),
              "FFN": list(itertools.product(us, (1,))), "CLS": list(itertools.product(us, (1,))),
              "W2": list(itertools.product(us, (1, 2, 4)))}
    pairs = {"QKV": (spec.dim + 2 * spec.kv_dim) // 2, "WO": spec.dim // 2, "FFN": spec.hidden_dim,
             "W2": spec.dim // 2, "CLS": (spec.vocab_size + 1) // 2}
    out = []
    for wg in (256, 512):
        for i in range(9):
            sh = {}
            for k, c in combos.items():
                u, sp = c[i % len(c)]
                sh[k] = (sp, u, min(1024, -(-pairs[k] // ((wg // 64) // sp))), wg)
            out.append(sh)
    for base in (0, 13):
        out.append({k: (s[0], s[1], g, s[3]) for (k, s), g in zip(out[base].items(), (3, 5, 2, 7, 1))})
    return out


def _set_shape_hooks(sh):
    for k in ("QKV", "WO", "FFN", "W2", "CLS"):
        _ffi.debug_set(f"KH_SHAPE_{k}", ",".join(map(str, sh[k])) if k in sh else None)


def _run_steps(m, spec, steps, rows):
    """teacher-forced steps into NaN rows -> [(logits, K rows [layers, kv], V rows)] as raw words"""
    nan = np.full((1, spec.kv_dim), np.nan, np.float32)
    res = []
    for tok, pos in steps:
        if pos == DEEP_POS:
            for layer in range(spec.n_layers):
                m.write_kv(layer, 0, rows[0][layer], rows[1][layer])
        for layer in range(spec.n_layers):
            m.write_kv(layer, pos, nan, nan)
        m.predict(tok, pos, exec="fused")
        lg = m.logits()
        kv = [m.read_kv(layer, pos, 1) for layer in range(spec.n_layers)]
        res.append((lg.view(np.uint32), np.stack([k[0] for k, _ in kv]).view(np.uint32),
                    np.stack([v[0] for _, v in kv]).view(np.uint32)))
    return res


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes(gpu, name):
    spec = GEOMETRIES[name]
    img = _rounded(spec, gpu)
    assert binfmt.matrices_bf16_exact(img, spec)
    rng = np.random.default_rng(7)
    steps = list(zip([int(t) for t in rng.integers(0, spec.vocab_size, 4)], (0, 1, 2, DEEP_POS)))
    rows = (rng.standard_normal((spec.n_layers, DEEP_POS, spec.kv_dim), dtype=np.float32),
            rng.standard_normal((spec.n_layers, DEEP_POS, spec.kv_dim), dtype=np.float32))
    rows[0][:, rng.integers(0, DEEP_POS, 8)] *= 6.0  # a few dominant keys: the splits' maxima differ
    launched, n_prefill = set(), 0
    try:
        for i, sh in enumerate(_shapes(spec)):
            what = f"{name} shape {i} {sh}"
            _set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _model(img, spec, W16)
            try:
                assert m1.w16_info()["state"] == 1, what
                want = _run_steps(m0, spec, steps, rows)
                _ffi.debug_set("KH_LAUNCH_LOG", "1")  # after creation: the self-check's launches are not compared ones
                got = _run_steps(m1, spec, steps, rows)
                log = _gemv_log(_ffi.launch_log())
                _ffi.debug_set("KH_LAUNCH_LOG", None)
                assert log and all(k.split("<")[0] in STEMS for k in log), f"{what}: fp32 GEMV launched: {sorted(log)}"
                launched |= log
                for (tok, pos), (la, ka, va), (lb, kb, vb) in zip(steps, want, got):
                    assert not np.isnan(la.view(np.float32)).any(), f"{what} pos {pos}: NaN logits"
                    assert np.array_equal(la, lb), f"{what} pos {pos}: logits differ in {int((la != lb).sum())} words"
                    assert np.array_equal(ka, kb) and np.array_equal(va, vb), f"{what} pos {pos}: K/V rows differ"
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
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _set_shape_hooks({})
    assert n_prefill > 0, f"{name}: no shape ran the B-token prefill"
    _LAUNCHED[name] = launched
    print(f"{name}: {len(_shapes(spec))} shapes, {len(launched)} W16 instantiations launched, {n_prefill} prefills")


# ---- 3. the copy is what is read --------------------------------------------------------------
def test_the_copy_is_what_is_read(gpu):
    def poison(img):
        for e in binfmt.layout(TIED)[0]:
            if e.name in {f"{n}.1" for n in ("wq", "wk", "wv", "wo", "w1", "w2", "w3")}:
                binfmt.tensor_from_image(img, e).fill_(float("nan"))
        torch.cuda.synchronize()

    for flags in (W16, 0):
        img = _rounded(TIED, gpu)
        assert (img.data_ptr() + TIED.header_bytes()) % 16 == 0  # from_device_image uses the image in place
        m = _model(img, TIED, flags)
        try:
            m.set_sampling(temperature=0.8, top_k=50, top_p=0.95, seed=3)  # no screened tail: nothing re-scores fp32 rows
            t0 = m.predict(5, 0, exec="fused")
            before = m.logits()
            assert np.isfinite(before).all()
            poison(img)
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
    rng = np.random.default_rng(11)
    prompt = [int(t) for t in rng.integers(0, TIED.vocab_size, 250)]  # sampled steps at positions 249 .. 270
    total = 272
    bias = {int(t): float(v) for t, v in zip(rng.integers(0, TIED.vocab_size, 6), (-3.0, 2.5, -np.inf, 1.0, -1.5, 4.0))}
    res = {}
    for flags in (EXACT, EXACT | W16):
        m = _model(tied_img, TIED, flags)
        try:
            assert m.w16_info()["state"] == (1 if flags & W16 else 0)
            r = {}
            for ex in ("graph", "fused"):
                r["greedy", ex] = m.generate(prompt, total, exec=ex)[0]  # the screened tail, as it is
            r["greedy32"] = m.generate(prompt[:2], 32, exec="graph")[0]
            m.set_sampling(temperature=0.8, top_k=50, top_p=0.95, seed=17)
            m.set_penalties(repetition=1.3, presence=0.2, frequency=0.1, last_n=64)
            m.set_logit_bias(bias)
            m.set_logprobs(5)
            for ex in ("graph", "fused"):
                r["sampled", ex] = m.generate(prompt, total, exec=ex)[0]
                lp = m.logprobs(248, 24)
                r["records", ex] = b"".join(lp[k].tobytes() for k in ("token", "logprob", "top_ids", "top_logprobs"))
            res[flags] = r
        finally:
            m.close()
    a, b = res[EXACT], res[EXACT | W16]
    assert len(a["greedy", "graph"]) > 256 and len(a["sampled", "graph"]) > 256  # the runs cross position 256
    for key in a:
        assert a[key] == b[key], f"{key}: flag off and on differ"
    assert a["sampled", "graph"] == a["sampled", "fused"] and a["records", "graph"] == a["records", "fused"]
    assert len(set(a["sampled", "graph"][-20:])) > 4  # the run wanders: equality is not that of one repeated token
    # anchor outside the library: the CPU oracle on the rounded image
    om = oracle.OracleModel.from_spec(tied_img.cpu().numpy(), TIED, cache_len=CACHE)
    want = om.generate(prompt[:2], 32)
    om.close()
    assert b["greedy32"] == want, (b["greedy32"], want)


# ---- 5. self-check ----------------------------------------------------------------------------
def test_selfcheck_failure_falls_back_to_fp32(gpu, tied_img):
    m0 = _model(tied_img, TIED)
    try:
        _ffi.debug_set("KH_SELFTEST_FAIL", "w16")
        m1 = _model(tied_img, TIED, W16)
    finally:
        _ffi.debug_set("KH_SELFTEST_FAIL", None)
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
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    compiled = co.instantiations(co.code_object_notes(_ffi.LIB_PATH), STEMS)
    missing = [g for g in GEOMETRIES if g not in _LAUNCHED]
    assert not missing, f"geometries that did not run to the end (run the whole module): {missing}"
    seen = set().union(*_LAUNCHED.values())
    for stem in sorted(STEMS):
        assert any(k.split("<")[0] == stem for k in compiled), f"no {stem} instantiation in the library"
    assert seen <= compiled, f"launched but not found in the code objects: {sorted(seen - compiled)}"
    gap = compiled - seen
    print(f"{len(seen)} of {len(compiled)} compiled W16 instantiations launched and compared")
    assert not gap, f"compiled and never launched: {sorted(gap)}"
