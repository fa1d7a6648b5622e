"""KH_FLAG_GEMM16 at the model level: the GEMM pass of a W16 model on the bf16 matrix cores (csrc/kh_gemm_w16.h), every
compiled k_pg_gemm_w16 / k_rg_gemm_w16 / k_sg_gemm_w16 instantiation launched and compared.

The procedure is that of test_prefill_gemm_instantiations_gpu.py (its helpers are imported, not copied): seeded 2-layer
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
import re

import numpy as np
import pytest
import torch

import code_objects as co
import test_prefill_gemm_instantiations_gpu as pgi
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

LOGIT_ATOL_F32, KV_ATOL_GEMM, KV_ATOL_DEEP = pgi.LOGIT_ATOL_F32, pgi.KV_ATOL_GEMM, pgi.KV_ATOL_DEEP  # 2e-5, 5e-6, 2e-5
CACHE = pgi.CACHE
FLAGS = _ffi.KH_FLAG_W16 | _ffi.KH_FLAG_GEMM16
ALL = ["qkv", "wo", "ffn13", "w2", "cls"]
STEMS = ("k_pg_gemm_w16", "k_rg_gemm_w16", "k_sg_gemm_w16")
L, Q2, HALF, INTER = pgi.L, pgi.Q2, pgi.HALF, pgi.INTER

GEOMETRIES = {  # name -> (spec, classes on the new kernels under KH_GEMM16_CLASSES=0x1f; the default mask leaves cls out)
    "f32-hs64-gqa-half": (pgi._spec(1024, 2816, 16, 4, 1024, False, 64, HALF, L, "g16-hs64"), ALL),
    "f32-hs128-mha-inter": (pgi._spec(1024, 1536, 8, 8, 784, False, 64, INTER, L, "g16-hs128"), ALL),
    "f32-qwen-hs80": (pgi._spec(960, 1600, 12, 2, 1536, False, 64, HALF, Q2, "g16-qwen-hs80"), ALL),
    "f32-hs64-h912": (pgi._spec(512, 912, 8, 2, 1008, False, 64, HALF, L, "g16-h912"), ["qkv", "wo", "ffn13", "cls"]),
}
FIRST = "f32-hs64-gqa-half"
_LAUNCHED = {}  # test -> _w16 GEMM instantiations its compared runs launched
_WORST = {"kv": 0.0, "kv_deep": 0.0, "logit": 0.0}


def _image(spec, gpu, rounded=True):
    img = binfmt.synth_image(spec, seed=4343, device=gpu, final_norm_std=1.0)
    if rounded:
        binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()
    return img


def _model(img, spec, mask=None, flags=FLAGS):
    """A model of the image; mask: hook KH_GEMM16_CLASSES at creation (None: the default adoption mask)."""
    from kuiperllama_amd.model import KuiperModel
    _ffi.debug_set("KH_GEMM16_CLASSES", mask)
    try:
        return KuiperModel.from_device_image(img, spec, flags=flags)
    finally:
        _ffi.debug_set("KH_GEMM16_CLASSES", None)


def _fp32_gemm_stems(log):
    return {k for k in log if re.match(r"k_(pg|rg|sg)_gemm<", k)}


def _w16_stems(log):
    return {k for k in log if k.split("<")[0] in STEMS}


def _check_stems(name, log, classes):
    """Which GEMM stems a run launched: the new ones for `classes`, the fp32 stem for the rest (epilogue 1 = residual
    GEMMs: wo and w2 share it; 0 qkv, 2 ffn13, 3 cls)."""
    epi = {"qkv": 0, "wo": 1, "w2": 1, "ffn13": 2, "cls": 3}
    new = {int(k[:-1].split(",")[-1]) for k in _w16_stems(log)}
    old = {int(k[:-1].split(",")[-1]) for k in _fp32_gemm_stems(log)}
    want_new = {epi[c] for c in classes}
    want_old = {epi[c] for c in ALL if c not in classes}
    assert new - {3} == want_new - {3} and old - {3} == want_old - {3}, (name, sorted(log))


def _record(res, sc, spec):
    """worst |K/V - gold| and |logit - gold| of a run that passed its bounds"""
    calls, lg = res
    g, first = sc["gold"], (0 if sc["name"] == "shallow" else pgi.DEEP[0])
    at = first
    for rows in calls:
        n = rows[0][0].shape[0]
        for layer, (k, v) in enumerate(rows):
            for nm, got in (("k", k), ("v", v)):
                e = float(np.abs(got - g[nm + "64"][layer, at - first:at - first + n]).max())
                key = "kv" if sc["name"] == "shallow" else "kv_deep"
                _WORST[key] = max(_WORST[key], e)
        at += n
    _WORST["logit"] = max(_WORST["logit"], float(np.abs(lg - g["lg64"]).max()))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name, capfd):
    spec, classes = GEOMETRIES[name]
    img_d = _image(spec, gpu)
    img_h = img_d.cpu().numpy()
    assert binfmt.matrices_bf16_exact(img_h, spec)
    rng = np.random.default_rng(11)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, CACHE)]
    p2 = pgi.SHALLOW[2]
    scen = [{"name": "shallow", "gold": pgi._gold(oracle, img_h, spec, toks, 0, p2 + 1, p2)}]
    if name == FIRST:
        rows = pgi._deep_rows(spec, rng)
        scen.append({"name": "deep", "rows": rows,
                     "gold": pgi._gold(oracle, img_h, spec, toks, pgi.DEEP[0], pgi.DEEP[2], pgi.DEEP[1], rows)})
    launched = set()
    m = _model(img_d, spec)
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
            tag = f"{name} {sc['name']}"

            def run(hooks, what, **kw):
                res, lg, _ = pgi._run(m, spec, toks, sc, hooks, LOGIT_ATOL_F32, capfd, f"{tag} {what}", **kw)
                _check_stems(f"{tag} {what}", lg - {k for k in lg if k.startswith("k_sg_")}, classes)
                launched.update(_w16_stems(lg))
                _record(res, sc, spec)
                return res

            base = run({}, "heuristic")
            pgi._same(base, run({}, "heuristic again"), f"{tag} second run")
            pgi._same(base, run({"KH_PG_ROPE_FUSE": "0"}, "KH_PG_ROPE_FUSE=0"), f"{tag} KH_PG_ROPE_FUSE=0")
            shapes = pgi._shapes(spec)
            solo = run(pgi._shape_hooks(shapes[0]), f"shape 0 {shapes[0]}", forced=shapes[0])
            pgi._same(solo, run({**pgi._shape_hooks(shapes[0]), "KH_PG_SOLO": "0"}, "shape 0 KH_PG_SOLO=0",
                                forced=shapes[0]), f"{tag} shape 0 KH_PG_SOLO=0")
            run({"KH_PG_CHUNK": "100"}, "KH_PG_CHUNK=100")
            if sc["name"] == "deep":
                shapes = shapes[:3] + shapes[-1:]
            elif name != FIRST:
                # one shape per accepted register tile of every GEMM (the walk puts ks in the inner loop), and the last
                n_ks = 4
                shapes = shapes[:1] + shapes[n_ks::n_ks] + shapes[-1:]
            for i, sh in enumerate(shapes[1:], 1):
                run(pgi._shape_hooks(sh), f"shape {i} {sh}", forced=sh)
    finally:
        _ffi.debug_set("KH_PG_DEBUG", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
        m.close()
    _LAUNCHED["geometry " + name] = launched
    print(f"{name}: {len(launched)} _w16 instantiations; worst so far: K/V {_WORST['kv']:.3e} (deep {_WORST['kv_deep']:.3e}),"
          f" logits {_WORST['logit']:.3e}")


def _kv(m, spec, row0, n):
    return [m.read_kv(layer, row0, n) for layer in range(spec.n_layers)]


def test_lone_segment_slot_prefill_has_the_bits_of_prefill_gemm(gpu):
    """seq_prefill(gemm=True) of one segment at slot 0 against prefill_gemm of the same tokens, under the flag, at each
    register tile of the QKV GEMM (k_rg_gemm_w16 against k_pg_gemm_w16; every other launch is shared)."""
    spec, _ = GEOMETRIES[FIRST]
    m = _model(_image(spec, gpu), spec)
    toks = [int(t) for t in np.random.default_rng(21).integers(0, spec.vocab_size, 300)]
    launched = set()
    try:
        m.seq_slots(1)
        for tile in pgi.TILES:
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
            assert f"k_rg_gemm_w16<{tile[0]},{tile[1]},0>" in log and f"k_pg_gemm_w16<{tile[0]},{tile[1]},0>" in log, \
                (tile, sorted(log))
            assert not _fp32_gemm_stems(log), sorted(log)
            launched |= _w16_stems(log)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
        m.close()
    _LAUNCHED["slot prefill"] = launched


WIDE_TILES = ((2, 4), (2, 2), (1, 4))


@pytest.mark.parametrize("name", [FIRST, "f32-hs64-h912"])
def test_wide_pass(gpu, oracle, name):
    """seq_step(gemm=True) at 3, 16 and 40 lanes of different lengths, under the heuristic shapes and under forced
    ones: picks are the first maxima of seq_gemm_logits, the rows are within the logit bound of the fp64 gold."""
    spec, classes = GEOMETRIES[name]
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
    m = _model(img_d, spec, "0x1f")  # the classifier GEMM too
    assert m.gemm16_info()["classes"] == classes and "cls" not in m.gemm16_info()["plan"]
    launched = set()
    hooks = ("KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU", "KH_PG_SHAPE_STORE")
    r2 = {"QKV": True, "RESID": True, "SWIGLU": spec.hidden_dim % 32 == 0, "STORE": spec.vocab_size % 32 == 0}
    try:
        m.seq_slots(64)
        for lo in (0, 32):  # 32 tiles per call
            ss = list(range(lo, min(lo + 32, n_all)))
            m.seq_prefill_many(ss, [seqs[s][:-1] for s in ss])
        runs = [(n, None) for n in (3, 16, 40)]
        runs += [(n, (tile, ks, kz)) for n, (tile, ks, kz) in zip((3, 16, 40, 16, 40, 3),
                 ((WIDE_TILES[0], 1, 1), (WIDE_TILES[1], 2, 2), (WIDE_TILES[2], 4, 4), (WIDE_TILES[0], 8, 1),
                  (WIDE_TILES[1], 4, 1), (WIDE_TILES[2], 2, 2)))]
        for n, forced in runs:
            slots = [int(s) for s in np.random.default_rng(n).permutation(n_all)[:n]]
            tile_of = {}
            if forced:
                (R, NT), ks, kz = forced
                for h in hooks:
                    e = h.rsplit("_", 1)[1]
                    tile_of[e] = (R, NT) if R == 1 or r2[e] else (1, 4)  # no 32-row tile where 32 rows do not divide
                    v = "%d,%d,%d" % (tile_of[e] + (min(ks, 4) if e == "SWIGLU" else ks,)) + (f",{kz}" if e == "RESID" else "")
                    _ffi.debug_set(h, v)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            picks = m.seq_step(slots, [seqs[s][-1] for s in slots], [len(seqs[s]) - 1 for s in slots], gemm=True)
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            for h in hooks:
                _ffi.debug_set(h, None)
            for i, s in enumerate(slots):
                lg = m.seq_gemm_logits(i)
                assert picks[i] == int(np.argmax(lg)), (name, n, forced, i)
                g64, g32 = gold[s]["64"], gold[s]["32"]
                e32 = float(np.abs(g32 - g64).max())
                err = float(np.abs(lg - g64).max())
                assert err <= max(LOGIT_ATOL_F32 + e32, 3.0 * e32), (name, n, forced, i, err, e32)
                _WORST["logit"] = max(_WORST["logit"], err)
                top2 = np.sort(g64)[-2:]
                if top2[1] - top2[0] > 2 * LOGIT_ATOL_F32:
                    assert picks[i] == int(np.argmax(g64)), (name, n, forced, i)
            sg = {k for k in log if k.startswith("k_sg_gemm")}
            _check_stems(f"{name} wide {n} {forced}", sg, classes)
            assert {int(k[:-1].split(",")[-1]) for k in _w16_stems(sg)} >= {3}, sorted(sg)  # the classifier GEMM
            if forced:
                want = {"k_sg_gemm_w16<%d,%d,%d>" % (tile_of[e] + (i,))
                        for i, e in enumerate(("QKV", "RESID", "SWIGLU", "STORE")) if ("qkv", "wo", "ffn13", "cls")[i] in classes}
                assert want <= sg, (forced, sorted(want - sg), sorted(sg))
            launched |= _w16_stems(log)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        for h in hooks:
            _ffi.debug_set(h, None)
        m.close()
    # the default mask: the classifier GEMM stays on the fp32 stem, the pass holds the same bounds
    m = _model(img_d, spec)
    try:
        m.seq_slots(64)
        slots = list(range(16))
        m.seq_prefill_many(slots, [seqs[s][:-1] for s in slots])
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        picks = m.seq_step(slots, [seqs[s][-1] for s in slots], [len(seqs[s]) - 1 for s in slots], gemm=True)
        sg = {k for k in _ffi.launch_log() if k.startswith("k_sg_gemm")}
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _check_stems(f"{name} wide, default mask", sg, [c for c in classes if c != "cls"])
        assert {int(k[:-1].split(",")[-1]) for k in _fp32_gemm_stems(sg)} >= {3}, sorted(sg)
        for i, s in enumerate(slots):
            lg = m.seq_gemm_logits(i)
            e32 = float(np.abs(gold[s]["32"] - gold[s]["64"]).max())
            assert picks[i] == int(np.argmax(lg)) and \
                float(np.abs(lg - gold[s]["64"]).max()) <= max(LOGIT_ATOL_F32 + e32, 3.0 * e32), (name, i)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()
    _LAUNCHED["wide " + name] = launched
    print(f"{name} wide: worst logits so far {_WORST['logit']:.3e}")


def _inert_case(gpu, case):
    """(spec, image, flags beside KH_FLAG_GEMM16, the reason gemm16_info() gives)"""
    spec, _ = GEOMETRIES[FIRST]
    if case == "unrounded image":
        return spec, _image(spec, gpu, rounded=False), _ffi.KH_FLAG_W16, "image not bf16-exact"
    if case == "fp16-exact image":
        half = binfmt.round_matrices_fp16(_image(spec, gpu, rounded=False), spec)
        torch.cuda.synchronize()
        return spec, half, _ffi.KH_FLAG_W16_F16, "fp16-format copy"
    if case == "int8 model":
        q8 = pgi._spec(1024, 2816, 16, 4, 1008, True, 64, INTER, L, "g16-q8")
        return q8, _image(q8, gpu, rounded=False), _ffi.KH_FLAG_W16, "int8 model"
    return spec, _image(spec, gpu), 0, "no W16 flag"


@pytest.mark.parametrize("case", ["unrounded image", "fp16-exact image", "int8 model", "no W16 flag"])
def test_inert(gpu, case):
    """Where the flag cannot take effect the model launches what it launches without it and leaves the same bits."""
    from kuiperllama_amd.model import KuiperModel
    spec, img, flags, reason = _inert_case(gpu, case)
    if case == "fp16-exact image":
        assert not binfmt.matrices_bf16_exact(img.cpu().numpy(), spec)
    toks = [int(t) for t in np.random.default_rng(41).integers(0, spec.vocab_size, 101)]
    out = []
    for fl in (flags, flags | _ffi.KH_FLAG_GEMM16):
        m = KuiperModel.from_device_image(img, spec, flags=fl)
        try:
            info = m.gemm16_info()
            if fl & _ffi.KH_FLAG_GEMM16:
                assert info["on"] is False and info["classes"] == [] and info["reason"] == reason, (case, info)
            else:
                assert info["on"] is False and info["reason"] == "flag not set", (case, info)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            m.prefill_gemm(toks[:100], 0)
            m.predict(toks[100], 100, exec="fused")
            m.seq_slots(4)
            picks = m.seq_step([0, 1, 2], toks[:3], [0, 0, 0], gemm=True)
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            out.append((log, _kv(m, spec, 0, 100), m.logits(), picks, [m.seq_gemm_logits(i) for i in range(3)]))
        finally:
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            m.close()
    (log0, kv0, lg0, pk0, sg0), (log1, kv1, lg1, pk1, sg1) = out
    assert not [k for k in log1 if "_gemm_w16" in k], sorted(log1)
    assert log0 == log1, sorted(log0 ^ log1)
    assert np.array_equal(lg0, lg1) and pk0 == pk1 and all(np.array_equal(a, b) for a, b in zip(sg0, sg1))
    for (k0, v0), (k1, v1) in zip(kv0, kv1):
        assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes(), case


def test_class_mask_hook(gpu):
    """KH_GEMM16_CLASSES replaces the adoption mask at creation: the classes outside it keep the fp32 stem."""
    spec, _ = GEOMETRIES[FIRST]
    m = _model(_image(spec, gpu), spec, "0x5")
    try:
        assert m.gemm16_info()["classes"] == ["qkv", "ffn13"]
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
    need = ["geometry " + g for g in GEOMETRIES] + ["slot prefill", "wide " + FIRST, "wide f32-hs64-h912"]
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
    print(f"worst |K/V - gold| {_WORST['kv']:.3e} (deep {_WORST['kv_deep']:.3e}), worst |logit - gold| {_WORST['logit']:.3e}")
