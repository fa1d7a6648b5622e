"""KH_FLAG_GEMM16_F16 at the model level (csrc/kh_gemm_h16.h: k_pg_gemm_h16 / k_rg_gemm_h16 / k_sg_gemm_h16), every
compiled instantiation launched and compared, by the procedure of test_prefill_gemm_instantiations_gpu.py and the
harness gemm16_cases.py: seeded 2-layer geometries rounded to fp16 (not bf16-exact), KH_FLAG_W16_F16 |
KH_FLAG_GEMM16_F16 under KH_GEMM16_F16_CLASSES=0x1f (the default adoption mask is empty), the gold
OracleModel.forward(..., ACC_F64).  Shallow scenario - [0, 37), [37, 337), predict at 337 - under the default shapes and,
on the first geometry, each compiled (R, NT); bounds KV_ATOL_GEMM and LOGIT_ATOL_F32 as max(floor + e32, 3 e32) and the
argmax rule (pgi._call / pgi._next apply them).  The lone-segment slot prefill at the default shape and at each QKV tile;
the wide pass at 16 lanes on the first geometry and over the harness's run list on f32-hs64-gqa-half, whose vocabulary
and hidden size 32 divides: the 32-row tiles of every epilogue."""
import numpy as np
import pytest

import gemm16_cases as g16
import test_prefill_gemm_instantiations_gpu as pgi
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

CORE = g16.H16
ALL = g16.ALL
L, HALF, INTER = pgi.L, pgi.HALF, pgi.INTER

GEOMETRIES = {  # name -> (spec, classes on the new kernels under KH_GEMM16_F16_CLASSES=0x1f)
    "f32-hs128-mha-inter": (pgi._spec(1024, 1536, 8, 8, 784, False, 64, INTER, L, "g16f-hs128"), ALL),
    "f32-hs64-gqa-half": (pgi._spec(1024, 2816, 16, 4, 1024, False, 64, HALF, L, "g16f-hs64"), ALL),
    "f32-hs64-h912": (pgi._spec(512, 912, 8, 2, 1008, False, 64, HALF, L, "g16f-h912"), ["qkv", "wo", "ffn13", "cls"]),
}
FIRST = "f32-hs128-mha-inter"
WIDE = "f32-hs64-gqa-half"
_LAUNCHED = {}  # test -> _h16 GEMM instantiations its compared runs launched
_WORST = {"kv": 0.0, "logit": 0.0}


def _image(spec, gpu):
    return g16.image(spec, gpu, CORE.make_exact)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name, capfd):
    spec, classes = GEOMETRIES[name]
    img_d = _image(spec, gpu)
    img_h = img_d.cpu().numpy()
    assert binfmt.matrices_fp16_exact(img_h, spec) and not binfmt.matrices_bf16_exact(img_h, spec)
    toks = [int(t) for t in np.random.default_rng(11).integers(0, spec.vocab_size, pgi.CACHE)]
    p2 = pgi.SHALLOW[2]
    sc = {"name": "shallow", "gold": pgi._gold(oracle, img_h, spec, toks, 0, p2 + 1, p2)}
    launched = set()
    m = g16.model(CORE, img_d, spec, "0x1f")
    _ffi.debug_set("KH_PG_DEBUG", "1")
    try:
        info = m.gemm16_f16_info()
        assert info == {"on": True, "classes": classes, "reason": "on", "plan": g16.plan(CORE, spec)}, info
        assert m.gemm16_info()["on"] is False and m.w16_format()["format"] == "fp16"
        prefill = [c for c in classes if c != "cls"]  # (a prefill runs no classifier)

        def run(hooks, what, mm=m, on=prefill, **kw):
            res, lg, _ = pgi._run(mm, spec, toks, sc, hooks, CORE.floor, capfd, f"{name} {what}", **kw)
            g16.check_stems(CORE, f"{name} {what}", lg, on)
            launched.update(g16.new_stems(CORE, lg))
            g16.record(_WORST, res, sc)
            return res, lg

        base, _ = run({}, "default shapes")
        pgi._same(base, run({}, "default shapes again")[0], f"{name} second run")
        for r, nt in (CORE.tiles if name == FIRST else ()):
            sh = {"QKV": (r, nt, 2), "RESID": (r, nt, 2, 2), "SWIGLU": (r, nt, 2)}
            _, lg = run(pgi._shape_hooks(sh), f"tile ({r},{nt})", forced=sh)
            want = {f"k_pg_gemm_h16<{r},{nt},{e}>" for e in (0, 1, 2)}
            assert want <= lg, (r, nt, sorted(g16.new_stems(CORE, lg)))
        if name == FIRST:  # KH_FLAG_W16_F16 alone: the fp32 stems, as before the flag existed
            m0 = g16.model(CORE, img_d, spec, "0x1f", flags=_ffi.KH_FLAG_W16_F16)
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
    _LAUNCHED["geometry " + name] = launched


def test_lone_segment_slot_prefill_has_the_bits_of_prefill_gemm(gpu):
    """seq_prefill(gemm=True) of one segment at slot 0 against prefill_gemm of the same tokens, at the default shape and
    at each register tile of the QKV GEMM (k_rg_gemm_h16 against k_pg_gemm_h16; every other launch is shared)."""
    spec, _ = GEOMETRIES[FIRST]
    m = g16.model(CORE, _image(spec, gpu), spec, "0x1f")
    try:
        _LAUNCHED["slot prefill"] = g16.lone_segment_slot_prefill(CORE, m, spec, (None,) + CORE.tiles)
    finally:
        m.close()


def test_wide_pass(gpu, oracle):
    """One seq_step(gemm=True) at 16 lanes of different lengths: picks are the first maxima of seq_gemm_logits, the rows
    are within the logit bound of the fp64 gold; every GEMM of the pass, the classifier's included, is a k_sg_gemm_h16."""
    spec, classes = GEOMETRIES[FIRST]
    img_d = _image(spec, gpu)
    seqs = g16.wide_sequences(spec)[:16]
    gold = g16.wide_gold(oracle, img_d.cpu().numpy(), spec, seqs)
    m = g16.model(CORE, img_d, spec, "0x1f")
    try:
        g16.wide_16_lanes(CORE, m, spec, seqs, gold, classes, CORE.floor, FIRST, _WORST)
    finally:
        m.close()


def test_wide_pass_run_list(gpu, oracle):
    """seq_step(gemm=True) at 3, 16 and 40 lanes under the default shapes and under forced ones, every class on the new
    stem; then the default mask - no class: the fp32 stems - under the same bounds."""
    spec, classes = GEOMETRIES[WIDE]
    img_d = _image(spec, gpu)
    seqs = g16.wide_sequences(spec)
    gold = g16.wide_gold(oracle, img_d.cpu().numpy(), spec, seqs)
    m = g16.model(CORE, img_d, spec, "0x1f")
    try:
        assert m.gemm16_f16_info()["classes"] == classes and "cls" not in m.gemm16_f16_info()["plan"]
        _LAUNCHED["wide"] = g16.wide_pass(CORE, m, spec, seqs, gold, classes, CORE.floor, WIDE, _WORST)
    finally:
        m.close()
    m = g16.model(CORE, img_d, spec)
    try:
        g16.wide_16_lanes(CORE, m, spec, seqs, gold, g16.plan(CORE, spec), CORE.floor, WIDE, _WORST)
    finally:
        m.close()


def _inert_case(gpu, case):
    """(spec, image, flags beside KH_FLAG_GEMM16_F16, the reason gemm16_f16_info() gives)"""
    spec, _ = GEOMETRIES[FIRST]
    if case == "bf16-exact image":
        return spec, g16.image(spec, gpu, binfmt.round_matrices_bf16), _ffi.KH_FLAG_W16_F16, "bf16-format copy"
    if case == "unrounded image":
        return spec, g16.image(spec, gpu), _ffi.KH_FLAG_W16_F16, "image not fp16-exact"
    if case == "int8 model":
        q8 = pgi._spec(1024, 2816, 16, 4, 1008, True, 64, INTER, L, "g16f-q8")
        return q8, g16.image(q8, gpu), _ffi.KH_FLAG_W16_F16, "int8 model"
    return spec, _image(spec, gpu), 0, "no W16_F16 flag"


@pytest.mark.parametrize("case", ["bf16-exact image", "unrounded image", "int8 model", "no W16_F16 flag"])
def test_inert(gpu, case):
    """Where the flag cannot take effect the model launches what it launches without it and leaves the same bits."""
    spec, img, flags, reason = _inert_case(gpu, case)
    g16.inert(CORE, spec, lambda on: g16.model(CORE, img, spec, "0x1f", flags | (CORE.flag if on else 0)), reason, case)


def test_class_mask_hook(gpu):
    """KH_GEMM16_F16_CLASSES replaces the adoption mask at creation: the classes outside it keep the fp32 stem."""
    spec, _ = GEOMETRIES[FIRST]
    g16.class_mask_hook(CORE, _image(spec, gpu), spec)


def test_coverage_gate(gpu):
    """Every compiled instantiation of the three stems was launched by a run above whose results were compared."""
    need = ["geometry " + g for g in GEOMETRIES] + ["slot prefill", "wide"]
    g16.coverage_gate(CORE, need, _LAUNCHED, _WORST)
