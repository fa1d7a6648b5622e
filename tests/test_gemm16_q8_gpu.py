"""KH_FLAG_GEMM16_Q8 at the model level: the GEMM pass of an int8 group-64 model on the bf16 matrix cores from its int8
image (csrc/kh_gemm_q16.h), every compiled k_pg_gemm_q16 / k_rg_gemm_q16 / k_sg_gemm_q16 instantiation launched and
compared.

The procedure is that of test_gemm16_gpu.py and test_prefill_gemm_instantiations_gpu.py (whose helpers are imported, not
copied): seeded 2-layer int8 group-64 geometries with 2613 cache rows, models created with KH_FLAG_GEMM16_Q8, the gold
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
import re

import numpy as np
import pytest
import torch

import code_objects as co
import test_prefill_gemm_instantiations_gpu as pgi
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

LOGIT_ATOL_Q8, KV_ATOL_GEMM = pgi.LOGIT_ATOL_Q8, pgi.KV_ATOL_GEMM  # 5e-5; 5e-6, which pgi._call takes times 4 for int8
CACHE = pgi.CACHE
FLAG = _ffi.KH_FLAG_GEMM16_Q8
ALL = ["qkv", "wo", "ffn13", "w2", "cls"]
STEMS = ("k_pg_gemm_q16", "k_rg_gemm_q16", "k_sg_gemm_q16")
TILES = ((2, 4), (2, 2), (1, 4))  # the new stem has no (2,8) register tile
L, HALF, INTER = pgi.L, pgi.HALF, pgi.INTER
EPI_OF = {"qkv": 0, "wo": 1, "w2": 1, "ffn13": 2, "cls": 3}

GEOMETRIES = {  # name -> (spec, hook KH_GEMM16_Q8_CLASSES at creation; None: the default adoption mask)
    "q8-hs64-inter": (pgi._spec(1024, 2816, 16, 4, 1008, True, 64, INTER, L, "g16q8-hs64"), "0x1f"),
    "q8-hs128-half": (pgi._spec(1024, 1536, 8, 2, 784, True, 64, HALF, L, "g16q8-hs128"), None),
    "q8-hs48-kv48": (pgi._spec(384, 1024, 8, 1, 1008, True, 64, HALF, L, "g16q8-hs48"), None),
}
FIRST = "q8-hs64-inter"
_LAUNCHED = {}  # test -> _q16 GEMM instantiations its compared runs launched
_WORST = {"kv": 0.0, "logit": 0.0}


def _image(spec, gpu):
    img = binfmt.synth_image(spec, seed=4343, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    return img


def _model(img, spec, mask=None, flags=FLAG):
    """A model of the image; mask: hook KH_GEMM16_Q8_CLASSES at creation (None: the default adoption mask)."""
    from kuiperllama_amd.model import KuiperModel
    _ffi.debug_set("KH_GEMM16_Q8_CLASSES", mask)
    try:
        return KuiperModel.from_device_image(img, spec, flags=flags)
    finally:
        _ffi.debug_set("KH_GEMM16_Q8_CLASSES", None)


def _old_gemm_stems(log):
    """GEMM launches on the fp32 matrix cores (the int8 / fp32 stems)"""
    return {k for k in log if re.match(r"k_(pg|rg|sg)_gemm<", k)}


def _q16_stems(log):
    return {k for k in log if k.split("<")[0] in STEMS}


def _check_stems(name, log, classes):
    """Which GEMM stems a run launched: the new ones for `classes`, the int8 stem for the rest (epilogue 1 = residual
    GEMMs: wo and w2 share it).  No fp32-MFMA GEMM for an adopted class, none of the new stem for the others."""
    new = {int(k[:-1].split(",")[-1]) for k in _q16_stems(log)}
    old = {int(k[:-1].split(",")[-1]) for k in _old_gemm_stems(log)}
    want_new = {EPI_OF[c] for c in classes}
    want_old = {EPI_OF[c] for c in ALL if c not in classes}
    assert new - {3} == want_new - {3} and old - {3} == want_old - {3}, (name, classes, sorted(log))
    assert not [k for k in log if "_gemm_w16" in k], sorted(log)


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


def _record(res, sc):
    """worst |K/V - gold| and |logit - gold| of a run that passed its bounds"""
    calls, lg = res
    g, at = sc["gold"], 0
    for rows in calls:
        n = rows[0][0].shape[0]
        for layer, (k, v) in enumerate(rows):
            for nm, got in (("k", k), ("v", v)):
                _WORST["kv"] = max(_WORST["kv"], float(np.abs(got - g[nm + "64"][layer, at:at + n]).max()))
        at += n
    _WORST["logit"] = max(_WORST["logit"], float(np.abs(lg - g["lg64"]).max()))


def _toks_and_gold(oracle, img_h, spec):
    rng = np.random.default_rng(11)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, CACHE)]
    p2 = pgi.SHALLOW[2]
    return toks, {"name": "shallow", "gold": pgi._gold(oracle, img_h, spec, toks, 0, p2 + 1, p2)}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name, capfd):
    spec, mask = GEOMETRIES[name]
    img_d = _image(spec, gpu)
    toks, sc = _toks_and_gold(oracle, img_d.cpu().numpy(), spec)
    launched = set()
    m = _model(img_d, spec, mask)
    plan = _ffi.plan_gemm16_q8(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, True, 64)["classes"]
    classes = ALL if mask == "0x1f" else plan
    _ffi.debug_set("KH_PG_DEBUG", "1")
    try:
        info = m.gemm16_q8_info()
        assert info == {"on": bool(classes), "classes": classes, "reason": "on" if classes else "no class", "plan": plan}, info
        classes = [c for c in classes if c != "cls"]  # (a prefill runs no classifier)

        def run(hooks, what, **kw):
            res, lg, _ = pgi._run(m, spec, toks, sc, hooks, LOGIT_ATOL_Q8, capfd, f"{name} {what}", **kw)
            _check_stems(f"{name} {what}", lg, classes)
            launched.update(_q16_stems(lg))
            _record(res, sc)
            return res

        base = run({}, "heuristic")
        pgi._same(base, run({}, "heuristic again"), f"{name} second run")
        pgi._same(base, run({"KH_PG_ROPE_FUSE": "0"}, "KH_PG_ROPE_FUSE=0"), f"{name} KH_PG_ROPE_FUSE=0")
        shapes = _shapes(spec, classes)
        solo = run(pgi._shape_hooks(shapes[0]), f"shape 0 {shapes[0]}", forced=shapes[0])
        pgi._same(solo, run({**pgi._shape_hooks(shapes[0]), "KH_PG_SOLO": "0"}, "shape 0 KH_PG_SOLO=0", forced=shapes[0]),
                  f"{name} shape 0 KH_PG_SOLO=0")
        run({"KH_PG_CHUNK": "100"}, "KH_PG_CHUNK=100")
        if name == "q8-hs128-half":
            run({"KH_PG_ATTN": "0"}, "KH_PG_ATTN=0")  # the wo GEMM reads a row-major slab
        if name != FIRST:
            # one shape per accepted register tile of every GEMM (the walk puts ks in the inner loop), and the last
            shapes = shapes[:1] + shapes[4::4] + shapes[-1:]
        for i, sh in enumerate(shapes[1:], 1):
            run(pgi._shape_hooks(sh), f"shape {i} {sh}", forced=sh)
    finally:
        _ffi.debug_set("KH_PG_DEBUG", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
        m.close()
    _LAUNCHED["geometry " + name] = launched
    print(f"{name}: {len(launched)} _q16 instantiations; worst so far: K/V {_WORST['kv']:.3e}, logits {_WORST['logit']:.3e}")


def _kv(m, spec, row0, n):
    return [m.read_kv(layer, row0, n) for layer in range(spec.n_layers)]


def test_lone_segment_slot_prefill_has_the_bits_of_prefill_gemm(gpu):
    """seq_prefill(gemm=True) of one segment at slot 0 against prefill_gemm of the same tokens, under the flag, at each
    register tile of the QKV GEMM (k_rg_gemm_q16 against k_pg_gemm_q16; every other launch is shared)."""
    spec, _ = GEOMETRIES[FIRST]
    m = _model(_image(spec, gpu), spec, "0x1f")
    toks = [int(t) for t in np.random.default_rng(21).integers(0, spec.vocab_size, 300)]
    launched = set()
    try:
        m.seq_slots(1)
        for tile in TILES:
            pgi._set_hooks({"KH_PG_SHAPE_QKV": f"{tile[0]},{tile[1]},2"})
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            m.prefill_gemm(toks, 0)
            want = _kv(m, spec, 0, 300)
            nan = np.full((300, spec.kv_dim), np.nan, np.float32)
            for layer in range(spec.n_layers):
                m.write_kv(layer, 0, nan, nan)
            m.seq_prefill(0, toks, gemm=True)
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            got = _kv(m, spec, m.seq_row(0, 0), 300)
            for (k0, v0), (k1, v1) in zip(want, got):
                assert np.array_equal(k0, k1) and np.array_equal(v0, v1), tile
            assert f"k_rg_gemm_q16<{tile[0]},{tile[1]},0>" in log and f"k_pg_gemm_q16<{tile[0]},{tile[1]},0>" in log, \
                (tile, sorted(log))
            assert not _old_gemm_stems(log), sorted(log)
            launched |= _q16_stems(log)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
        m.close()
    _LAUNCHED["slot prefill"] = launched


def test_wide_pass(gpu, oracle):
    """seq_step(gemm=True) at 3, 16 and 40 lanes of different lengths, under the heuristic shapes and under forced
    ones, every class on the new stem: picks are the first maxima of seq_gemm_logits, the rows are within the logit
    bound of the fp64 gold, the classifier GEMM is on the new stem.  Then the default mask: the same bounds."""
    spec, _ = GEOMETRIES[FIRST]
    img_d = _image(spec, gpu)
    img_h = img_d.cpu().numpy()
    rng = np.random.default_rng(31)
    n_all = 40
    seqs = [[int(t) for t in rng.integers(0, spec.vocab_size, 2 + s % 7)] for s in range(n_all)]  # the last is stepped
    gold = []
    for s in range(n_all):
        row = {}
        for tag, acc in (("64", oracle.ACC_F64), ("32", oracle.ACC_F32)):
            om = oracle.OracleModel.from_spec(img_h, spec, cache_len=16)
            for p, t in enumerate(seqs[s]):
                lg = om.forward(t, p, acc)
            row[tag] = lg.copy()
            om.close()
        gold.append(row)

    def check(m, slots, picks, what):
        for i, s in enumerate(slots):
            lg = m.seq_gemm_logits(i)
            assert picks[i] == int(np.argmax(lg)), (what, i)
            g64, g32 = gold[s]["64"], gold[s]["32"]
            e32 = float(np.abs(g32 - g64).max())
            err = float(np.abs(lg - g64).max())
            assert err <= max(LOGIT_ATOL_Q8 + e32, 3.0 * e32), (what, i, err, e32)
            _WORST["logit"] = max(_WORST["logit"], err)
            top2 = np.sort(g64)[-2:]
            if top2[1] - top2[0] > 2 * LOGIT_ATOL_Q8:
                assert picks[i] == int(np.argmax(g64)), (what, i)

    m = _model(img_d, spec, "0x1f")
    assert m.gemm16_q8_info()["classes"] == ALL
    launched = set()
    hooks = ("KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU", "KH_PG_SHAPE_STORE")
    try:
        m.seq_slots(64)
        for lo in (0, 32):  # 32 tiles per call
            ss = list(range(lo, min(lo + 32, n_all)))
            m.seq_prefill_many(ss, [seqs[s][:-1] for s in ss])
        runs = [(n, None) for n in (3, 16, 40)]
        runs += [(n, (tile, ks, kz)) for n, (tile, ks, kz) in zip((3, 16, 40, 16, 40, 3),
                 ((TILES[0], 1, 1), (TILES[1], 2, 2), (TILES[2], 4, 4), (TILES[0], 8, 1), (TILES[1], 4, 1), (TILES[2], 2, 2)))]
        for n, forced in runs:
            slots = [int(s) for s in np.random.default_rng(n).permutation(n_all)[:n]]
            tile_of = {}
            if forced:
                (R, NT), ks, kz = forced
                for h in hooks:
                    e = h.rsplit("_", 1)[1]
                    # the classifier has no 32-row tile where 32 rows do not divide the vocabulary
                    tile_of[e] = (R, NT) if R == 1 or e != "STORE" or spec.vocab_size % 32 == 0 else (1, 4)
                    _ffi.debug_set(h, "%d,%d,%d" % (tile_of[e] + (min(ks, 4) if e == "SWIGLU" else ks,))
                                   + (f",{kz}" if e == "RESID" else ""))
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            picks = m.seq_step(slots, [seqs[s][-1] for s in slots], [len(seqs[s]) - 1 for s in slots], gemm=True)
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            for h in hooks:
                _ffi.debug_set(h, None)
            check(m, slots, picks, f"wide {n} {forced}")
            sg = {k for k in log if k.startswith("k_sg_gemm")}
            _check_stems(f"wide {n} {forced}", sg, ALL)
            assert {int(k[:-1].split(",")[-1]) for k in _q16_stems(sg)} >= {3} and not _old_gemm_stems(sg), sorted(sg)
            if forced:
                want = {"k_sg_gemm_q16<%d,%d,%d>" % (tile_of[e] + (i,)) for i, e in enumerate(("QKV", "RESID", "SWIGLU", "STORE"))}
                assert want <= sg, (forced, sorted(want - sg), sorted(sg))
            launched |= _q16_stems(log)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        for h in hooks:
            _ffi.debug_set(h, None)
        m.close()
    # the default mask: the classes outside it stay on the int8 stem, the pass holds the same bounds
    m = _model(img_d, spec)
    try:
        classes = m.gemm16_q8_info()["classes"]
        m.seq_slots(64)
        slots = list(range(16))
        m.seq_prefill_many(slots, [seqs[s][:-1] for s in slots])
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        picks = m.seq_step(slots, [seqs[s][-1] for s in slots], [len(seqs[s]) - 1 for s in slots], gemm=True)
        sg = {k for k in _ffi.launch_log() if k.startswith("k_sg_gemm")}
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _check_stems("wide, default mask", sg, classes)
        cls_new = {int(k[:-1].split(",")[-1]) for k in _q16_stems(sg)} >= {3}
        assert cls_new == ("cls" in classes), (classes, sorted(sg))
        check(m, slots, picks, "wide, default mask")
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()
    _LAUNCHED["wide"] = launched
    print(f"wide: worst logits so far {_WORST['logit']:.3e}")


def _inert_case(gpu, case):
    """(spec, image, flags of the flag-off model, flags of the other, hook KH_GEMM16_Q8, the reason gemm16_q8_info() gives)"""
    q8 = GEOMETRIES[FIRST][0]
    if case == "fp32 model":
        spec = pgi._spec(1024, 2816, 16, 4, 1008, False, 64, INTER, L, "g16q8-f32")
        return spec, _image(spec, gpu), 0, FLAG, None, "fp32 model"
    if case == "int8 group 128":
        spec = pgi._spec(512, 1024, 8, 2, 1008, True, 128, INTER, L, "g16q8-g128")
        return spec, _image(spec, gpu), 0, FLAG, None, "group size not 64"
    if case == "cleared flag":
        return q8, _image(q8, gpu), 0, FLAG, "0", "flag not set"
    # KH_FLAG_GEMM16 (with a W16 flag) on an int8 model: inert as ever, and it does not switch this flag on
    return q8, _image(q8, gpu), 0, _ffi.KH_FLAG_W16 | _ffi.KH_FLAG_GEMM16, None, "flag not set"


def _rc(fn):
    try:
        return fn()
    except _ffi.KhError as e:
        return ("KhError", e.code)


@pytest.mark.parametrize("case", ["fp32 model", "int8 group 128", "cleared flag", "KH_FLAG_GEMM16 on int8"])
def test_inert(gpu, case):
    """Where the flag cannot take effect the model launches what it launches without it and leaves the same bits."""
    from kuiperllama_amd.model import KuiperModel
    spec, img, flags0, flags1, hook, reason = _inert_case(gpu, case)
    toks = [int(t) for t in np.random.default_rng(41).integers(0, spec.vocab_size, 101)]
    out = []
    for fl in (flags0, flags1):
        _ffi.debug_set("KH_GEMM16_Q8", hook if fl == flags1 else None)
        try:
            m = KuiperModel.from_device_image(img, spec, flags=fl)
        finally:
            _ffi.debug_set("KH_GEMM16_Q8", None)
        try:
            info = m.gemm16_q8_info()
            assert info["on"] is False and info["classes"] == [] and info["plan"] == [], (case, info)
            assert info["reason"] == (reason if fl == flags1 else "flag not set"), (case, info)
            if case == "KH_FLAG_GEMM16 on int8" and fl == flags1:
                assert m.gemm16_info()["reason"] == "int8 model" and m.gemm16_info()["on"] is False
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            rc = _rc(lambda: m.prefill_gemm(toks[:100], 0))  # (group 128: refused, with or without the flag)
            if rc is not None:
                m.generate(toks[:100], 101)  # the B-token prefill fills the rows
            m.predict(toks[100], 100, exec="fused")
            lg = m.logits()
            m.seq_slots(4)
            picks = _rc(lambda: m.seq_step([0, 1, 2], toks[:3], [0, 0, 0], gemm=True))
            sg = [m.seq_gemm_logits(i) for i in range(3)] if isinstance(picks, list) else []
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            out.append((log, _kv(m, spec, 0, 100), lg, (rc, picks), sg))
        finally:
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            m.close()
    (log0, kv0, lg0, pk0, sg0), (log1, kv1, lg1, pk1, sg1) = out
    assert not [k for k in log1 if "_gemm_q16" in k or "_gemm_w16" in k], sorted(log1)
    assert log0 == log1, sorted(log0 ^ log1)
    assert np.array_equal(lg0, lg1) and pk0 == pk1 and len(sg0) == len(sg1)
    assert all(np.array_equal(a, b) for a, b in zip(sg0, sg1))
    for (k0, v0), (k1, v1) in zip(kv0, kv1):
        assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes(), case


def test_q4_and_gemm16_q8_together(gpu, oracle, capfd):
    """KH_FLAG_Q4 | KH_FLAG_GEMM16_Q8 on a 4-bit-exact image: the GEMM passes read the int8 image on the new stem within
    the bounds, the decode steps read the 4-bit copy and keep its bits (those of the int8 decode kernels)."""
    spec, _ = GEOMETRIES[FIRST]
    img_d = binfmt.requantize_matrices_q4(_image(spec, gpu), spec)
    torch.cuda.synchronize()
    toks, sc = _toks_and_gold(oracle, img_d.cpu().numpy(), spec)
    res = {}
    for tag, flags in (("both", _ffi.KH_FLAG_Q4 | FLAG), ("q16", FLAG)):
        m = _model(img_d, spec, "0x1f", flags=flags)
        _ffi.debug_set("KH_PG_DEBUG", "1")
        try:
            assert m.gemm16_q8_info()["classes"] == ALL
            assert m.q4_info()["state"] == (1 if tag == "both" else 0), m.q4_info()
            r, lg, _ = pgi._run(m, spec, toks, sc, {}, LOGIT_ATOL_Q8, capfd, f"q4 {tag}")
            _check_stems(f"q4 {tag}", {k for k in lg if "_gemm" in k}, ALL[:4])
            # the predict step's launches: on the 4-bit copy for the classes Q4 adopts
            assert bool([k for k in lg if "_q4" in k]) == (tag == "both" and bool(m.q4_info()["classes"])), sorted(lg)
            _record(r, sc)
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
        assert _q16_stems(log) == {kern}, sorted(log)
        launched |= _q16_stems(log)
    _LAUNCHED["store"] = launched


def test_class_mask_hook(gpu):
    """KH_GEMM16_Q8_CLASSES replaces the adoption mask at creation: the classes outside it keep the int8 stem."""
    spec, _ = GEOMETRIES[FIRST]
    m = _model(_image(spec, gpu), spec, "0x5")
    try:
        assert m.gemm16_q8_info()["classes"] == ["qkv", "ffn13"]
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        m.prefill_gemm(list(range(40)), 0)
        log = set(_ffi.launch_log())
        _check_stems("mask 0x5", log, ["qkv", "ffn13"])
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()


def test_coverage_gate(gpu):
    """Every compiled instantiation of the three stems was launched by a run above whose results were compared."""
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    need = ["geometry " + g for g in GEOMETRIES] + ["slot prefill", "wide", "store"]
    missing = [t for t in need if t not in _LAUNCHED]
    assert not missing, f"tests that did not run to the end (run the whole module): {missing}"
    build.build_lib()
    compiled = co.kernels(co.code_object_notes(_ffi.LIB_PATH), set(STEMS))
    seen = set().union(*_LAUNCHED.values())
    for stem in STEMS:
        comp = {k for k in compiled if k.split("<")[0] == stem}
        got = {k for k in seen if k.split("<")[0] == stem}
        assert comp and got <= comp, (stem, sorted(got - comp))
        print(f"{stem}: {len(got)} of {len(comp)} compiled instantiations launched and compared")
        assert not comp - got, f"{stem}: compiled and never launched: {sorted(comp - got)}"
    print(f"worst |K/V - gold| {_WORST['kv']:.3e}, worst |logit - gold| {_WORST['logit']:.3e}")
