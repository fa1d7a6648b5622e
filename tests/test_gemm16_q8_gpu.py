"""KH_FLAG_GEMM16_Q8 at the model level: the GEMM pass of an int8 group-64 model on the bf16 matrix cores from its int8
image (csrc/kh_gemm_q16.h), every compiled k_pg_gemm_q16 / k_rg_gemm_q16 / k_sg_gemm_q16 instantiation launched and
compared.

The procedure is that of test_prefill_gemm_instantiations_gpu.py (whose helpers are imported, not copied); the runs,
checks and gates the three GEMM16 cores share are gemm16_cases.py's.  Seeded 2-layer int8 group-64 geometries with 2613 cache rows, models created with KH_FLAG_GEMM16_Q8, the gold
OracleModel.forward(..., ACC_F64) teacher-forced on the same image.

  q8-hs64-inter    RoPE pairs in the epilogue, MFMA attention, tiled B; every class on the new stem (hook
                   KH_GEMM16_Q8_CLASSES=0x1f) and the whole walk of forced shapes; also the slot prefill and the wide pass
  q8-hs128-half    paired-tile RoPE; KH_PG_ATTN=0: wo reads a row-major slab; the default class mask
  q8-hs48-kv48     the QKV GEMM takes R = 1 (kv_dim 48); the default class mask

Scenario: shallow - [0, 37), [37, 337), predict at 337 - under the heuristic shapes, a second run (bit-identical),
KH_PG_ROPE_FUSE=0 (bit-identical), KH_PG_SOLO=0 at a forced shape (bit-identical), KH_PG_CHUNK=100 and forced shapes
through KH_PG_SHAPE_*: every register tile the new stem has - (2,4), (2,2), (1,4); a class that keeps the int8 stem also
(2,8) - x ks 1/2/4/8 x kz 1/2/4 on the first geometry, one shape per tile on the others.  Bounds: the project's int8
ones, LOGIT_ATOL_Q8 = 5e-5 and 4 x KV_ATOL_GEMM = 2e-5, each applied as max(floor + e32, 3 e32) against the gold (e32:
the oracle's fp32 run against its fp64 run); the argmax equals the gold's where the gold's top-2 margin exceeds
2 x floor; the rows below and past a call keep their bits.  The launch log: the classes in the mask launch the _q16
stem, the others the int8 stem.  A lone-segment seq_prefill(gemm=True) leaves the K/V bytes of prefill_gemm at each QKV
tile.  The wide pass (seq_step(gemm=True) at 3, 16 and 40 lanes, heuristic and forced tiles): each pick is the first
maximum of the lane's seq_gemm_logits row, the rows within the logit bound, the classifier GEMM on the new stem under
0x1f.  Inert cases: an fp32 model, an int8 group-128 model, a cleared flag (hook KH_GEMM16_Q8=0) and KH_FLAG_GEMM16 on
an int8 model launch no _q16 (and no _w16) stem and leave the K/V bytes, logits, picks and launch set of the flag-off
model; gemm16_q8_info() names the reason.  KH_FLAG_Q4 | KH_FLAG_GEMM16_Q8 on a 4-bit-exact image holds the same bounds
and its decode steps keep the Q4 bits.  The worst measured errors are printed (DESIGN 3.1f quotes them).
"""
import numpy as np
import pytest
import torch

import gemm16_cases as g16
import test_prefill_gemm_instantiations_gpu as pgi
from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

CORE = g16.Q16
FLAG = CORE.flag
ALL = g16.ALL
L, HALF, INTER = pgi.L, pgi.HALF, pgi.INTER

GEOMETRIES = {  # name -> (spec, hook KH_GEMM16_Q8_CLASSES at creation; None: the default adoption mask)
    "q8-hs64-inter": (pgi._spec(1024, 2816, 16, 4, 1008, True, 64, INTER, L, "g16q8-hs64"), "0x1f"),
    "q8-hs128-half": (pgi._spec(1024, 1536, 8, 2, 784, True, 64, HALF, L, "g16q8-hs128"), None),
    "q8-hs48-kv48": (pgi._spec(384, 1024, 8, 1, 1008, True, 64, HALF, L, "g16q8-hs48"), None),
}
FIRST = "q8-hs64-inter"
_LAUNCHED = {}  # test -> _q16 GEMM instantiations its compared runs launched
_WORST = {"kv": 0.0, "logit": 0.0}


def _shapes(spec, classes):
    """pgi._shapes over the tiles each GEMM accepts here: a GEMM with a class on the new stem has no (2,8) tile."""
    acc = pgi._accepted_tiles(spec)
    on = {"QKV": "qkv" in classes, "RESID": "wo" in classes or "w2" in classes, "SWIGLU": "ffn13" in classes}
    acc = {e: [t for t in ts if not (on[e] and t == (2, 8))] for e, ts in acc.items()}
    ks_max = {"QKV": 8, "RESID": 8, "SWIGLU": 4}
    combos = {e: [(r, nt, ks) for r, nt in acc[e] for ks in (1, 2, 4, 8) if ks <= ks_max[e]] for e in pgi.EPIS}
    n = max(len(c) for c in combos.values())
    out = []
    for i in range(n):
        sh = {e: c[i % len(c)] for e, c in combos.items()}
        sh["RESID"] = sh["RESID"] + ((1, 2, 4)[i % 3],)
        out.append(sh)
    out.append({"RESID": acc["RESID"][-1] + (8, 4)})
    return out


def _toks_and_gold(oracle, img_h, spec):
    rng = np.random.default_rng(11)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, pgi.CACHE)]
    p2 = pgi.SHALLOW[2]
    return toks, {"name": "shallow", "gold": pgi._gold(oracle, img_h, spec, toks, 0, p2 + 1, p2)}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name, capfd):
    spec, mask = GEOMETRIES[name]
    img_d = g16.image(spec, gpu)
    toks, sc = _toks_and_gold(oracle, img_d.cpu().numpy(), spec)
    launched = set()
    m = g16.model(CORE, img_d, spec, mask)
    plan = _ffi.plan_gemm16_q8(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, True, 64)["classes"]
    classes = ALL if mask == "0x1f" else plan
    _ffi.debug_set("KH_PG_DEBUG", "1")
    try:
        info = m.gemm16_q8_info()
        assert info == {"on": bool(classes), "classes": classes, "reason": "on" if classes else "no class", "plan": plan}, info
        classes = [c for c in classes if c != "cls"]  # (a prefill runs no classifier)
        shapes = _shapes(spec, classes)
        if name != FIRST:
            shapes = g16.one_shape_per_tile(shapes)
        run = g16.geometry_runs(CORE, m, spec, toks, sc, shapes, CORE.floor, classes, capfd, name, launched, _WORST)
        if name == "q8-hs128-half":
            run({"KH_PG_ATTN": "0"}, "KH_PG_ATTN=0")  # the wo GEMM reads a row-major slab
    finally:
        _ffi.debug_set("KH_PG_DEBUG", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
        m.close()
    _LAUNCHED["geometry " + name] = launched
    print(f"{name}: {len(launched)} _q16 instantiations; worst so far: K/V {g16.kv_text(_WORST)}, logits {_WORST['logit']:.3e}")


def test_lone_segment_slot_prefill_has_the_bits_of_prefill_gemm(gpu):
    """seq_prefill(gemm=True) of one segment at slot 0 against prefill_gemm of the same tokens, under the flag, at each
    register tile of the QKV GEMM (k_rg_gemm_q16 against k_pg_gemm_q16; every other launch is shared)."""
    spec, _ = GEOMETRIES[FIRST]
    m = g16.model(CORE, g16.image(spec, gpu), spec, "0x1f")
    try:
        _LAUNCHED["slot prefill"] = g16.lone_segment_slot_prefill(CORE, m, spec, CORE.tiles)
    finally:
        m.close()


def test_wide_pass(gpu, oracle):
    """seq_step(gemm=True) at 3, 16 and 40 lanes of different lengths, under the heuristic shapes and under forced
    ones, every class on the new stem: picks are the first maxima of seq_gemm_logits, the rows are within the logit
    bound of the fp64 gold, the classifier GEMM is on the new stem.  Then the default mask: the same bounds."""
    spec, _ = GEOMETRIES[FIRST]
    img_d = g16.image(spec, gpu)
    seqs = g16.wide_sequences(spec)
    gold = g16.wide_gold(oracle, img_d.cpu().numpy(), spec, seqs)
    m = g16.model(CORE, img_d, spec, "0x1f")
    try:
        assert m.gemm16_q8_info()["classes"] == ALL
        _LAUNCHED["wide"] = g16.wide_pass(CORE, m, spec, seqs, gold, ALL, CORE.floor, FIRST, _WORST)
    finally:
        m.close()
    # the default mask: the classes outside it stay on the int8 stem, the pass holds the same bounds
    m = g16.model(CORE, img_d, spec)
    try:
        g16.wide_16_lanes(CORE, m, spec, seqs, gold, g16.plan(CORE, spec), CORE.floor, FIRST, _WORST)
    finally:
        m.close()
    print(f"wide: worst logits so far {_WORST['logit']:.3e}")


def _inert_case(gpu, case):
    """(spec, image, flags of the model the flag cannot take effect on, hook KH_GEMM16_Q8 at its creation, the reason
    gemm16_q8_info() gives); the flag-off model has no flag"""
    q8 = GEOMETRIES[FIRST][0]
    if case == "fp32 model":
        spec = pgi._spec(1024, 2816, 16, 4, 1008, False, 64, INTER, L, "g16q8-f32")
        return spec, g16.image(spec, gpu), FLAG, None, "fp32 model"
    if case == "int8 group 128":
        spec = pgi._spec(512, 1024, 8, 2, 1008, True, 128, INTER, L, "g16q8-g128")
        return spec, g16.image(spec, gpu), FLAG, None, "group size not 64"
    if case == "cleared flag":
        return q8, g16.image(q8, gpu), FLAG, "0", "flag not set"
    # KH_FLAG_GEMM16 (with a W16 flag) on an int8 model: inert as ever, and it does not switch this flag on
    return q8, g16.image(q8, gpu), _ffi.KH_FLAG_W16 | _ffi.KH_FLAG_GEMM16, None, "flag not set"


def _rc(fn):
    try:
        return fn()
    except _ffi.KhError as e:
        return ("KhError", e.code)


def _inert_calls(m, spec, toks):
    """g16.inert_calls where a call may be refused (group 128: with or without the flag): the codes join the picks"""
    rc = _rc(lambda: m.prefill_gemm(toks[:100], 0))
    if rc is not None:
        m.generate(toks[:100], 101)  # the B-token prefill fills the rows
    m.predict(toks[100], 100, exec="fused")
    lg = m.logits()
    m.seq_slots(4)
    picks = _rc(lambda: m.seq_step([0, 1, 2], toks[:3], [0, 0, 0], gemm=True))
    return (rc, picks), lg, [m.seq_gemm_logits(i) for i in range(3)] if isinstance(picks, list) else []


@pytest.mark.parametrize("case", ["fp32 model", "int8 group 128", "cleared flag", "KH_FLAG_GEMM16 on int8"])
def test_inert(gpu, case):
    """Where the flag cannot take effect the model launches what it launches without it and leaves the same bits."""
    from kuiperllama_amd.model import KuiperModel
    spec, img, flags, hook, reason = _inert_case(gpu, case)

    def create(on):
        _ffi.debug_set("KH_GEMM16_Q8", hook if on else None)
        try:
            m = KuiperModel.from_device_image(img, spec, flags=flags if on else 0)
        finally:
            _ffi.debug_set("KH_GEMM16_Q8", None)
        if case == "KH_FLAG_GEMM16 on int8" and on:
            assert m.gemm16_info()["reason"] == "int8 model" and m.gemm16_info()["on"] is False
        return m

    g16.inert(CORE, spec, create, reason, case, _inert_calls)


def test_q4_and_gemm16_q8_together(gpu, oracle, capfd):
    """KH_FLAG_Q4 | KH_FLAG_GEMM16_Q8 on a 4-bit-exact image: the GEMM passes read the int8 image on the new stem within
    the bounds, the decode steps read the 4-bit copy and keep its bits (those of the int8 decode kernels)."""
    spec, _ = GEOMETRIES[FIRST]
    img_d = binfmt.requantize_matrices_q4(g16.image(spec, gpu), spec)
    torch.cuda.synchronize()
    toks, sc = _toks_and_gold(oracle, img_d.cpu().numpy(), spec)
    res = {}
    for tag, flags in (("both", _ffi.KH_FLAG_Q4 | FLAG), ("q16", FLAG)):
        m = g16.model(CORE, img_d, spec, "0x1f", flags=flags)
        _ffi.debug_set("KH_PG_DEBUG", "1")
        try:
            assert m.gemm16_q8_info()["classes"] == ALL
            assert m.q4_info()["state"] == (1 if tag == "both" else 0), m.q4_info()
            r, lg, _ = pgi._run(m, spec, toks, sc, {}, CORE.floor, capfd, f"q4 {tag}")
            g16.check_stems(CORE, f"q4 {tag}", {k for k in lg if "_gemm" in k}, ALL[:4])
            # the predict step's launches: on the 4-bit copy for the classes Q4 adopts
            assert bool([k for k in lg if "_q4" in k]) == (tag == "both" and bool(m.q4_info()["classes"])), sorted(lg)
            g16.record(_WORST, r, sc)
            res[tag] = r
        finally:
            _ffi.debug_set("KH_PG_DEBUG", None)
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            pgi._set_hooks({})
            m.close()
    pgi._same(res["both"], res["q16"], "Q4 | GEMM16_Q8 against GEMM16_Q8: K/V rows and the decode step's logits")


def test_store_epilogue_on_32_row_tiles(gpu):
    """The vocabularies above (1008, 784) are no multiples of 32, so their classifier GEMM runs the 16-row tile; the
    32-row STORE instantiations run under ops.gemm_q8_bf16, bit for bit against the fp64 gold on exact inputs
    (test_gemm16_q8_ops_gpu.py's, imported)."""
    import gemm_q16_ref as ref
    import test_gemm16_q8_ops_gpu as opsq
    launched = set()
    for (M, K, T), kern in (((32, 128, 17), "k_sg_gemm_q16<2,2,3>"), ((64, 512, 40), "k_sg_gemm_q16<2,4,3>")):
        x, q, s = opsq._exact_case(np.random.default_rng(M + K + T), M, K, T)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        try:
            got = opsq._run(gpu, x, q, s)
            log = set(_ffi.launch_log())
        finally:
            _ffi.debug_set("KH_LAUNCH_LOG", None)
        want = ref.gold(x, q, s)[0].astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (M, K, T)
        assert g16.new_stems(CORE, log) == {kern}, sorted(log)
        launched |= g16.new_stems(CORE, log)
    _LAUNCHED["store"] = launched


def test_class_mask_hook(gpu):
    """KH_GEMM16_Q8_CLASSES replaces the adoption mask at creation: the classes outside it keep the int8 stem."""
    spec, _ = GEOMETRIES[FIRST]
    g16.class_mask_hook(CORE, g16.image(spec, gpu), spec)


def test_coverage_gate(gpu):
    """Every compiled instantiation of the three stems was launched by a run above whose results were compared."""
    need = ["geometry " + g for g in GEOMETRIES] + ["slot prefill", "wide", "store"]
    g16.coverage_gate(CORE, need, _LAUNCHED, _WORST)
