"""KH_FLAG_GEMM16 at the model level: the GEMM pass of a W16 model on the bf16 matrix cores (csrc/kh_gemm_w16.h), every
compiled k_pg_gemm_w16 / k_rg_gemm_w16 / k_sg_gemm_w16 instantiation launched and compared.

The procedure is that of test_prefill_gemm_instantiations_gpu.py (its helpers are imported, not copied); the runs,
checks and gates the three GEMM16 cores share are gemm16_cases.py's.  Seeded 2-layer
geometries with 2613 cache rows whose matrices are rounded to bf16 (binfmt.round_matrices_bf16), models created with
KH_FLAG_W16 | KH_FLAG_GEMM16, the gold OracleModel.forward(..., ACC_F64) teacher-forced on the same rounded image.

  f32-hs64-gqa-half     paired-tile RoPE, MFMA attention, tiled B; also the deep scenario at 2085, the slot prefill and
                        the wide pass
  f32-hs128-mha-inter   RoPE pairs in the epilogue
  f32-qwen-hs80         Qwen2 bias; fallback attention: wo reads a row-major slab
  f32-hs64-h912         hidden 912 = 28.5 blocks of 32: w2 alone keeps the fp32 stem, the other classes log the new one

Scenarios: shallow - [0, 37), [37, 337), predict at 337 - and on the first geometry deep at 2085; under the heuristic
shapes, forced shapes through KH_PG_SHAPE_* (every accepted (R, NT) x ks 1/2/4/8 x kz 1/2/4 on the first geometry, the
first few elsewhere), KH_PG_SOLO=0, KH_PG_ROPE_FUSE=0 and KH_PG_CHUNK=100.  Bounds: the project's KV_ATOL_GEMM = 5e-6,
KV_ATOL_DEEP = 2e-5 and LOGIT_ATOL_F32 = 2e-5, each applied as max(floor + e32, 3 e32) against the gold (e32: the
oracle's fp32 run against its fp64 run); the argmax equals the gold's where the gold's top-2 margin exceeds 2 x floor;
the rows below and past a call keep their bits.  Bit-identical pairs: two runs of the same call, KH_PG_SOLO=0 at a
forced shape, KH_PG_ROPE_FUSE=0, and a lone-segment seq_prefill_gemm against prefill_gemm of the same tokens.
The wide pass (seq_step(gemm=True) at 3, 16 and 40 lanes): each pick is the first maximum of the lane's
seq_gemm_logits row, the rows within the logit bound.  Inert cases: an unrounded image, an fp16-exact image under
KH_FLAG_W16_F16, an int8 model and the flag without W16 launch no _w16 GEMM stem, leave the K/V bytes and logits of the
flag-off model, and gemm16_info() names the reason.  The worst measured errors are printed (DESIGN 3.1e quotes them).
"""
import numpy as np
import pytest

import gemm16_cases as g16
import test_prefill_gemm_instantiations_gpu as pgi
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

CORE = g16.W16
ALL = g16.ALL
L, Q2, HALF, INTER = pgi.L, pgi.Q2, pgi.HALF, pgi.INTER

GEOMETRIES = {  # name -> (spec, classes on the new kernels under KH_GEMM16_CLASSES=0x1f; the default mask leaves cls out)
    "f32-hs64-gqa-half": (pgi._spec(1024, 2816, 16, 4, 1024, False, 64, HALF, L, "g16-hs64"), ALL),
    "f32-hs128-mha-inter": (pgi._spec(1024, 1536, 8, 8, 784, False, 64, INTER, L, "g16-hs128"), ALL),
    "f32-qwen-hs80": (pgi._spec(960, 1600, 12, 2, 1536, False, 64, HALF, Q2, "g16-qwen-hs80"), ALL),
    "f32-hs64-h912": (pgi._spec(512, 912, 8, 2, 1008, False, 64, HALF, L, "g16-h912"), ["qkv", "wo", "ffn13", "cls"]),
}
FIRST = "f32-hs64-gqa-half"
WIDE = [FIRST, "f32-hs64-h912"]
_LAUNCHED = {}  # test -> _w16 GEMM instantiations its compared runs launched
_WORST = {"kv": 0.0, "kv_deep": 0.0, "logit": 0.0}


def _image(spec, gpu):
    return g16.image(spec, gpu, CORE.make_exact)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name, capfd):
    spec, classes = GEOMETRIES[name]
    img_d = _image(spec, gpu)
    img_h = img_d.cpu().numpy()
    assert binfmt.matrices_bf16_exact(img_h, spec)
    rng = np.random.default_rng(11)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, pgi.CACHE)]
    p2 = pgi.SHALLOW[2]
    scen = [{"name": "shallow", "gold": pgi._gold(oracle, img_h, spec, toks, 0, p2 + 1, p2)}]
    if name == FIRST:
        rows = pgi._deep_rows(spec, rng)
        scen.append({"name": "deep", "rows": rows,
                     "gold": pgi._gold(oracle, img_h, spec, toks, pgi.DEEP[0], pgi.DEEP[2], pgi.DEEP[1], rows)})
    launched = set()
    m = g16.model(CORE, img_d, spec)
    classes = [c for c in classes if c != "cls"]  # the default mask (a prefill runs no classifier either way)
    _ffi.debug_set("KH_PG_DEBUG", "1")
    try:
        info = m.gemm16_info()
        assert info == {"on": True, "classes": classes, "reason": "on", "plan": classes}, info
        assert m.w16_info()["state"] == 1
        for sc in scen:
            if sc["name"] == "deep":
                for layer in range(spec.n_layers):
                    m.write_kv(layer, 0, sc["rows"][0][layer], sc["rows"][1][layer])
            shapes = pgi._shapes(spec)
            if sc["name"] == "deep":
                shapes = shapes[:3] + shapes[-1:]
            elif name != FIRST:
                shapes = g16.one_shape_per_tile(shapes)
            g16.geometry_runs(CORE, m, spec, toks, sc, shapes, CORE.floor, classes, capfd, f"{name} {sc['name']}",
                              launched, _WORST)
    finally:
        _ffi.debug_set("KH_PG_DEBUG", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
        m.close()
    _LAUNCHED["geometry " + name] = launched
    print(f"{name}: {len(launched)} _w16 instantiations; worst so far: K/V {g16.kv_text(_WORST)},"
          f" logits {_WORST['logit']:.3e}")


def test_lone_segment_slot_prefill_has_the_bits_of_prefill_gemm(gpu):
    """seq_prefill(gemm=True) of one segment at slot 0 against prefill_gemm of the same tokens, under the flag, at each
    register tile of the QKV GEMM (k_rg_gemm_w16 against k_pg_gemm_w16; every other launch is shared)."""
    spec, _ = GEOMETRIES[FIRST]
    m = g16.model(CORE, _image(spec, gpu), spec)
    try:
        _LAUNCHED["slot prefill"] = g16.lone_segment_slot_prefill(CORE, m, spec, CORE.tiles)
    finally:
        m.close()


@pytest.mark.parametrize("name", WIDE)
def test_wide_pass(gpu, oracle, name):
    """seq_step(gemm=True) at 3, 16 and 40 lanes of different lengths, under the heuristic shapes and under forced
    ones: picks are the first maxima of seq_gemm_logits, the rows are within the logit bound of the fp64 gold."""
    spec, classes = GEOMETRIES[name]
    img_d = _image(spec, gpu)
    seqs = g16.wide_sequences(spec)
    gold = g16.wide_gold(oracle, img_d.cpu().numpy(), spec, seqs)
    m = g16.model(CORE, img_d, spec, "0x1f")  # the classifier GEMM too
    try:
        assert m.gemm16_info()["classes"] == classes and "cls" not in m.gemm16_info()["plan"]
        _LAUNCHED["wide " + name] = g16.wide_pass(CORE, m, spec, seqs, gold, classes, CORE.floor, name, _WORST)
    finally:
        m.close()
    # the default mask: the classifier GEMM stays on the fp32 stem, the pass holds the same bounds
    m = g16.model(CORE, img_d, spec)
    try:
        g16.wide_16_lanes(CORE, m, spec, seqs, gold, g16.plan(CORE, spec), CORE.floor, name, margin_rule=False)
    finally:
        m.close()
    print(f"{name} wide: worst logits so far {_WORST['logit']:.3e}")


def _inert_case(gpu, case):
    """(spec, image, flags beside KH_FLAG_GEMM16, the reason gemm16_info() gives)"""
    spec, _ = GEOMETRIES[FIRST]
    if case == "unrounded image":
        return spec, g16.image(spec, gpu), _ffi.KH_FLAG_W16, "image not bf16-exact"
    if case == "fp16-exact image":
        return spec, g16.image(spec, gpu, binfmt.round_matrices_fp16), _ffi.KH_FLAG_W16_F16, "fp16-format copy"
    if case == "int8 model":
        q8 = pgi._spec(1024, 2816, 16, 4, 1008, True, 64, INTER, L, "g16-q8")
        return q8, g16.image(q8, gpu), _ffi.KH_FLAG_W16, "int8 model"
    return spec, _image(spec, gpu), 0, "no W16 flag"


@pytest.mark.parametrize("case", ["unrounded image", "fp16-exact image", "int8 model", "no W16 flag"])
def test_inert(gpu, case):
    """Where the flag cannot take effect the model launches what it launches without it and leaves the same bits."""
    spec, img, flags, reason = _inert_case(gpu, case)
    if case == "fp16-exact image":
        assert not binfmt.matrices_bf16_exact(img.cpu().numpy(), spec)
    g16.inert(CORE, spec, lambda on: g16.model(CORE, img, spec, flags=flags | (CORE.flag if on else 0)), reason, case)


def test_class_mask_hook(gpu):
    """KH_GEMM16_CLASSES replaces the adoption mask at creation: the classes outside it keep the fp32 stem."""
    spec, _ = GEOMETRIES[FIRST]
    g16.class_mask_hook(CORE, _image(spec, gpu), spec)


def test_coverage_gate(gpu):
    """Every compiled instantiation of the three stems was launched by a run above whose results were compared."""
    need = ["geometry " + g for g in GEOMETRIES] + ["slot prefill"] + ["wide " + g for g in WIDE]
    g16.coverage_gate(CORE, need, _LAUNCHED, _WORST)
