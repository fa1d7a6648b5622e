"""KH_FLAG_GEMM16_F16 at the model level (csrc/kh_gemm_h16.h: k_pg_gemm_h16 / k_rg_gemm_h16 / k_sg_gemm_h16), by the
procedure of test_gemm16_gpu.py and test_prefill_gemm_instantiations_gpu.py (helpers imported): seeded 2-layer geometries
rounded to fp16 (not bf16-exact), KH_FLAG_W16_F16 | KH_FLAG_GEMM16_F16 under KH_GEMM16_F16_CLASSES=0x1f, the gold
OracleModel.forward(..., ACC_F64).  Shallow scenario - [0, 37), [37, 337), predict at 337 - under the default shapes and,
on the first geometry, each compiled (R, NT); bounds KV_ATOL_GEMM and LOGIT_ATOL_F32 as max(floor + e32, 3 e32) and the
argmax rule (pgi._call / pgi._next apply them)."""
import numpy as np
import pytest
import torch

import test_gemm16_gpu as g16
import test_prefill_gemm_instantiations_gpu as pgi
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

LOGIT_ATOL_F32 = pgi.LOGIT_ATOL_F32
FLAGS = _ffi.KH_FLAG_W16_F16 | _ffi.KH_FLAG_GEMM16_F16
ALL = g16.ALL
STEMS = ("k_pg_gemm_h16", "k_rg_gemm_h16", "k_sg_gemm_h16")
TILES = ((2, 4), (2, 2), (1, 4))  # the compiled register tiles
L, HALF, INTER = pgi.L, pgi.HALF, pgi.INTER

GEOMETRIES = {  # name -> (spec, classes on the new kernels under KH_GEMM16_F16_CLASSES=0x1f)
    "f32-hs128-mha-inter": (pgi._spec(1024, 1536, 8, 8, 784, False, 64, INTER, L, "g16f-hs128"), ALL),
    "f32-hs64-gqa-half": (pgi._spec(1024, 2816, 16, 4, 1024, False, 64, HALF, L, "g16f-hs64"), ALL),
    "f32-hs64-h912": (pgi._spec(512, 912, 8, 2, 1008, False, 64, HALF, L, "g16f-h912"), ["qkv", "wo", "ffn13", "cls"]),
}
FIRST = "f32-hs128-mha-inter"


def _image(spec, gpu, how="fp16"):
    img = binfmt.synth_image(spec, seed=4343, device=gpu, final_norm_std=1.0)
    if how == "fp16":
        img = binfmt.round_matrices_fp16(img, spec)
    elif how == "bf16":
        binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()
    return img


def _model(img, spec, mask="0x1f", flags=FLAGS):
    """A model of the image; mask: hook KH_GEMM16_F16_CLASSES at creation (None: the default adoption mask)."""
    from kuiperllama_amd.model import KuiperModel
    _ffi.debug_set("KH_GEMM16_F16_CLASSES", mask)
    try:
        return KuiperModel.from_device_image(img, spec, flags=flags)
    finally:
        _ffi.debug_set("KH_GEMM16_F16_CLASSES", None)


def _h16_stems(log):
    return {k for k in log if k.split("<")[0] in STEMS}


def _check_stems(name, log, classes):
    """The new stems for `classes`, the fp32 stem for the rest (by epilogue: 0 qkv, 1 wo and w2, 2 ffn13, 3 cls)."""
    epi = {"qkv": 0, "wo": 1, "w2": 1, "ffn13": 2, "cls": 3}
    new = {int(k[:-1].split(",")[-1]) for k in _h16_stems(log)}
    old = {int(k[:-1].split(",")[-1]) for k in g16._fp32_gemm_stems(log)}
    assert new - {3} == {epi[c] for c in classes} - {3}, (name, sorted(log))
    assert old - {3} == {epi[c] for c in ALL if c not in classes} - {3}, (name, sorted(log))
    assert not [k for k in log if "_gemm_w16" in k], (name, sorted(log))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name, capfd):
    spec, classes = GEOMETRIES[name]
    img_d = _image(spec, gpu)
    img_h = img_d.cpu().numpy()
    assert binfmt.matrices_fp16_exact(img_h, spec) and not binfmt.matrices_bf16_exact(img_h, spec)
    toks = [int(t) for t in np.random.default_rng(11).integers(0, spec.vocab_size, pgi.CACHE)]
    p2 = pgi.SHALLOW[2]
    sc = {"name": "shallow", "gold": pgi._gold(oracle, img_h, spec, toks, 0, p2 + 1, p2)}
    m = _model(img_d, spec)
    _ffi.debug_set("KH_PG_DEBUG", "1")
    try:
        info = m.gemm16_f16_info()
        assert info["on"] is True and info["classes"] == classes and info["reason"] == "on", info
        assert info["plan"] == _ffi.plan_gemm16_f16(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, False)["classes"]
        assert m.gemm16_info()["on"] is False and m.w16_format()["format"] == "fp16"
        prefill = [c for c in classes if c != "cls"]  # (a prefill runs no classifier)

        def run(hooks, what, mm=m, on=prefill, **kw):
            res, lg, _ = pgi._run(mm, spec, toks, sc, hooks, LOGIT_ATOL_F32, capfd, f"{name} {what}", **kw)
            _check_stems(f"{name} {what}", lg - {k for k in lg if k.startswith("k_sg_")}, on)
            return res, lg

        base, _ = run({}, "default shapes")
        pgi._same(base, run({}, "default shapes again")[0], f"{name} second run")
        for r, nt in (TILES if name == FIRST else ()):
            sh = {"QKV": (r, nt, 2), "RESID": (r, nt, 2, 2), "SWIGLU": (r, nt, 2)}
            _, lg = run(pgi._shape_hooks(sh), f"tile ({r},{nt})", forced=sh)
            want = {f"k_pg_gemm_h16<{r},{nt},{e}>" for e in (0, 1, 2)}
            assert want <= lg, (r, nt, sorted(_h16_stems(lg)))
        if name == FIRST:  # KH_FLAG_W16_F16 alone: the fp32 stems, as before the flag existed
            m0 = _model(img_d, spec, flags=_ffi.KH_FLAG_W16_F16)
            try:
                assert m0.gemm16_f16_info()["reason"] == "flag not set"
                run({}, "flag off", mm=m0, on=[])
            finally:
                m0.close()
    finally:
        _ffi.debug_set("KH_PG_DEBUG", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
        m.close()


def test_lone_segment_slot_prefill_has_the_bits_of_prefill_gemm(gpu):
    """seq_prefill(gemm=True) of one segment at slot 0 against prefill_gemm of the same tokens (k_rg_gemm_h16 against
    k_pg_gemm_h16 in the QKV GEMM; every other launch is shared)."""
    spec, _ = GEOMETRIES[FIRST]
    m = _model(_image(spec, gpu), spec)
    toks = [int(t) for t in np.random.default_rng(21).integers(0, spec.vocab_size, 300)]
    try:
        m.seq_slots(1)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        m.prefill_gemm(toks, 0)
        want = g16._kv(m, spec, 0, 300)
        nan = np.full((300, spec.kv_dim), np.nan, np.float32)
        for layer in range(spec.n_layers):
            m.write_kv(layer, 0, nan, nan)
        m.seq_prefill(0, toks, gemm=True)
        log = set(_ffi.launch_log())
        got = g16._kv(m, spec, m.seq_row(0, 0), 300)
        for (k0, v0), (k1, v1) in zip(want, got):
            assert np.array_equal(k0, k1) and np.array_equal(v0, v1)
        assert any(k.startswith("k_rg_gemm_h16<") for k in log) and any(k.startswith("k_pg_gemm_h16<") for k in log), sorted(log)
        assert not g16._fp32_gemm_stems(log), sorted(log)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()


def test_wide_pass(gpu, oracle):
    """One seq_step(gemm=True) at 16 lanes of different lengths: picks are the first maxima of seq_gemm_logits, the rows
    are within the logit bound of the fp64 gold; every GEMM of the pass, the classifier's included, is a k_sg_gemm_h16."""
    spec, classes = GEOMETRIES[FIRST]
    img_d = _image(spec, gpu)
    img_h = img_d.cpu().numpy()
    rng = np.random.default_rng(31)
    n = 16
    seqs = [[int(t) for t in rng.integers(0, spec.vocab_size, 2 + s % 7)] for s in range(n)]  # the last is stepped
    m = _model(img_d, spec)
    try:
        m.seq_slots(64)
        slots = list(range(n))
        m.seq_prefill_many(slots, [s[:-1] for s in seqs])
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        picks = m.seq_step(slots, [s[-1] for s in seqs], [len(s) - 1 for s in seqs], gemm=True)
        sg = {k for k in _ffi.launch_log() if k.startswith("k_sg_gemm")}
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _check_stems("wide 16", sg, classes)
        assert {int(k[:-1].split(",")[-1]) for k in _h16_stems(sg)} == {0, 1, 2, 3}, sorted(sg)
        for i, s in enumerate(seqs):
            gold = {}
            for tag, acc in (("64", oracle.ACC_F64), ("32", oracle.ACC_F32)):
                om = oracle.OracleModel.from_spec(img_h, spec, cache_len=16)
                for p, t in enumerate(s):
                    gold[tag] = om.forward(t, p, acc).copy()
                om.close()
            lg = m.seq_gemm_logits(i)
            assert picks[i] == int(np.argmax(lg)), i
            e32 = float(np.abs(gold["32"] - gold["64"]).max())
            err = float(np.abs(lg - gold["64"]).max())
            assert err <= max(LOGIT_ATOL_F32 + e32, 3.0 * e32), (i, err, e32)
            top2 = np.sort(gold["64"])[-2:]
            if top2[1] - top2[0] > 2 * LOGIT_ATOL_F32:
                assert picks[i] == int(np.argmax(gold["64"])), i
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()


def _inert_case(gpu, case):
    """(spec, image, flags beside KH_FLAG_GEMM16_F16, the reason gemm16_f16_info() gives)"""
    spec, _ = GEOMETRIES[FIRST]
    if case == "bf16-exact image":
        return spec, _image(spec, gpu, "bf16"), _ffi.KH_FLAG_W16_F16, "bf16-format copy"
    if case == "unrounded image":
        return spec, _image(spec, gpu, None), _ffi.KH_FLAG_W16_F16, "image not fp16-exact"
    if case == "int8 model":
        q8 = pgi._spec(1024, 2816, 16, 4, 1008, True, 64, INTER, L, "g16f-q8")
        return q8, _image(q8, gpu, None), _ffi.KH_FLAG_W16_F16, "int8 model"
    return spec, _image(spec, gpu), 0, "no W16_F16 flag"


@pytest.mark.parametrize("case", ["bf16-exact image", "unrounded image", "int8 model", "no W16_F16 flag"])
def test_inert(gpu, case):
    """Where the flag cannot take effect the model launches what it launches without it and leaves the same bits."""
    spec, img, flags, reason = _inert_case(gpu, case)
    toks = [int(t) for t in np.random.default_rng(41).integers(0, spec.vocab_size, 101)]
    out = []
    for fl in (flags, flags | _ffi.KH_FLAG_GEMM16_F16):
        m = _model(img, spec, flags=fl)
        try:
            info = m.gemm16_f16_info()
            want = reason if fl & _ffi.KH_FLAG_GEMM16_F16 else "flag not set"
            assert info["on"] is False and info["classes"] == [] and info["reason"] == want, (case, info)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            m.prefill_gemm(toks[:100], 0)
            m.predict(toks[100], 100, exec="fused")
            m.seq_slots(4)
            picks = m.seq_step([0, 1, 2], toks[:3], [0, 0, 0], gemm=True)
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            out.append((log, g16._kv(m, spec, 0, 100), m.logits(), picks, [m.seq_gemm_logits(i) for i in range(3)]))
        finally:
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            m.close()
    (log0, kv0, lg0, pk0, sg0), (log1, kv1, lg1, pk1, sg1) = out
    assert not [k for k in log1 if "_gemm_h16" in k], sorted(log1)
    assert log0 == log1, sorted(log0 ^ log1)
    assert np.array_equal(lg0, lg1) and pk0 == pk1 and all(np.array_equal(a, b) for a, b in zip(sg0, sg1))
    for (k0, v0), (k1, v1) in zip(kv0, kv1):
        assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes(), case
