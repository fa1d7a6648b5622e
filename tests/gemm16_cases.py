"""Shared by the tests of the three GEMM cores on the bf16 matrix cores - W16 (KH_FLAG_GEMM16, the bf16-format copy),
H16 (KH_FLAG_GEMM16_F16, the fp16-format copy) and Q16 (KH_FLAG_GEMM16_Q8, the int8 image): the model-level modules
test_gemm16_gpu.py, test_gemm16_f16_gpu.py and test_gemm16_q8_gpu.py, the operator-level modules test_gemm16_ops_gpu.py,
test_gemm16_f16_ops_gpu.py and test_gemm16_q8_ops_gpu.py, and the CPU modules test_gemm16.py and test_gemm16_q8.py.

Plain functions with explicit arguments over one record per core: images and models, the launch-log rules, the
worst-error recorder, the run list of a geometry, the lone-segment slot prefill, the wide pass, the inert comparison,
the class-mask check and the coverage gate; then the operator-level comparisons and the host-side ABI, plan and
code-object checks.  The procedure of a run is test_prefill_gemm_instantiations_gpu.py's (imported, not copied).  What
only one core needs stays in its module."""
import dataclasses
import os
import re
from typing import Callable, Optional

import numpy as np
import torch

import code_objects as co
import test_prefill_gemm_instantiations_gpu as pgi
from kuiperllama_amd import _ffi, binfmt, build, ops

ALL = ["qkv", "wo", "ffn13", "w2", "cls"]
EPI_OF = {"qkv": 0, "wo": 1, "w2": 1, "ffn13": 2, "cls": 3}  # the residual GEMMs wo and w2 share an epilogue
WIDE_HOOKS = ("KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU", "KH_PG_SHAPE_STORE")


# ---- the cores --------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Core:
    suffix: str      # of the kernel stems and of csrc/kh_gemm_<suffix>.h, csrc/kh_model_gemm_<suffix>.hip
    flag_name: str   # in _ffi and include/kuiper_hip.h; the hooks are KH_<rest> and KH_<rest>_CLASSES
    copy_flags: int  # the flags a model needs beside the core's own
    info: str        # the KuiperModel method over kh_model_<info>
    plan: str        # the _ffi function over kh_<plan>
    op: str          # the ops function over `entry`, the K loop under the STORE epilogue
    entry: str
    tiles: tuple     # the register tiles (R, NT) of the prefill stems; the wide pass has no (2,8) under any core
    make_exact: Optional[Callable]  # (image, spec) -> the image the core takes effect on (None: as synthesised)
    floor: float     # the logit floor of the model kind

    @property
    def flag(self):
        return getattr(_ffi, self.flag_name)

    @property
    def flags(self):
        return self.copy_flags | self.flag

    @property
    def hook(self):
        return self.flag_name.replace("KH_FLAG_", "KH_")

    @property
    def classes_hook(self):
        return self.hook + "_CLASSES"

    @property
    def stems(self):
        return tuple(f"k_{s}_gemm_{self.suffix}" for s in ("pg", "rg", "sg"))

    @property
    def wide_tiles(self):
        return tuple(t for t in self.tiles if t != (2, 8))


_TILES3 = ((2, 4), (2, 2), (1, 4))
W16 = Core("w16", "KH_FLAG_GEMM16", _ffi.KH_FLAG_W16, "gemm16_info", "plan_gemm16", "gemm_w16", "kh_gemm_w16_f32",
           ((2, 8),) + _TILES3, binfmt.round_matrices_bf16, pgi.LOGIT_ATOL_F32)
H16 = Core("h16", "KH_FLAG_GEMM16_F16", _ffi.KH_FLAG_W16_F16, "gemm16_f16_info", "plan_gemm16_f16", "gemm_h16",
           "kh_gemm_h16_f32", _TILES3, binfmt.round_matrices_fp16, pgi.LOGIT_ATOL_F32)
Q16 = Core("q16", "KH_FLAG_GEMM16_Q8", 0, "gemm16_q8_info", "plan_gemm16_q8", "gemm_q8_bf16", "kh_gemm_q8_bf16_f32",
           _TILES3, None, pgi.LOGIT_ATOL_Q8)


# ---- images and models ------------------------------------------------------------------------
def image(spec, gpu, make_exact=None):
    img = binfmt.synth_image(spec, seed=4343, device=gpu, final_norm_std=1.0)
    if make_exact:
        img = make_exact(img, spec)
    torch.cuda.synchronize()
    return img


def model(core, img, spec, mask=None, flags=None):
    """A model of the image; mask: the core's class-mask hook while it is created (None: the default adoption mask);
    flags: the core's own and its copy's unless given."""
    from kuiperllama_amd.model import KuiperModel
    _ffi.debug_set(core.classes_hook, mask)
    try:
        return KuiperModel.from_device_image(img, spec, flags=core.flags if flags is None else flags)
    finally:
        _ffi.debug_set(core.classes_hook, None)


def info(core, m):
    return getattr(m, core.info)()


def plan(core, spec):
    """the classes of the core's default adoption mask on the geometry"""
    group = (spec.group_size,) if core is Q16 else ()
    return getattr(_ffi, core.plan)(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, spec.quant, *group)["classes"]


def kv(m, spec, row0, n):
    return [m.read_kv(layer, row0, n) for layer in range(spec.n_layers)]


# ---- the launch log ---------------------------------------------------------------------------
def new_stems(core, log):
    return {k for k in log if k.split("<")[0] in core.stems}


def old_gemm_stems(log):
    """GEMM launches on the fp32 matrix cores (the fp32 / int8 stems)"""
    return {k for k in log if re.match(r"k_(pg|rg|sg)_gemm<", k)}


def epilogues(kernels):
    return {int(k[:-1].split(",")[-1]) for k in kernels}


def check_stems(core, name, log, classes):
    """Which GEMM stems a run launched: the core's for `classes`, the fp32 / int8 stem for the rest, by epilogue (the
    classifier's apart: a prefill runs none, the wide pass checks it itself); and no _gemm_w16 name under another core."""
    new, old = epilogues(new_stems(core, log)), epilogues(old_gemm_stems(log))
    want_new = {EPI_OF[c] for c in classes}
    want_old = {EPI_OF[c] for c in ALL if c not in classes}
    assert new - {3} == want_new - {3} and old - {3} == want_old - {3}, (name, classes, sorted(log))
    if core is not W16:
        assert not [k for k in log if "_gemm_w16" in k], (name, sorted(log))


# ---- worst errors -----------------------------------------------------------------------------
def record(worst, res, sc):
    """worst |K/V - gold| (key "kv"; the deep scenario's under "kv_deep") and |logit - gold| of a run that passed its
    bounds into the module's dict `worst`"""
    calls, lg = res
    g, first = sc["gold"], (0 if sc["name"] == "shallow" else pgi.DEEP[0])
    key = "kv" if sc["name"] == "shallow" else "kv_deep"
    at = first
    for rows in calls:
        n = rows[0][0].shape[0]
        for layer, (k, v) in enumerate(rows):
            for nm, got in (("k", k), ("v", v)):
                e = float(np.abs(got - g[nm + "64"][layer, at - first:at - first + n]).max())
                worst[key] = max(worst[key], e)
        at += n
    worst["logit"] = max(worst["logit"], float(np.abs(lg - g["lg64"]).max()))


def kv_text(worst):
    return f"{worst['kv']:.3e}" + (f" (deep {worst['kv_deep']:.3e})" if "kv_deep" in worst else "")


# ---- one geometry -----------------------------------------------------------------------------
def geometry_runs(core, m, spec, toks, sc, shapes, floor, classes, capfd, tag, launched, worst):
    """The runs of one scenario on a model whose prefill classes are `classes`: default shapes; again (same bits);
    KH_PG_ROPE_FUSE=0 (same bits); shapes[0]; shapes[0] with KH_PG_SOLO=0 (same bits); KH_PG_CHUNK=100; then
    shapes[1:].  Every run holds pgi's bounds under `floor` and check_stems, adds to `launched` and `worst`.  Returns
    run(hooks, what, **kw) for the runs only one module has."""
    def run(hooks, what, **kw):
        res, lg, _ = pgi._run(m, spec, toks, sc, hooks, floor, capfd, f"{tag} {what}", **kw)
        check_stems(core, f"{tag} {what}", lg, classes)
        launched.update(new_stems(core, lg))
        record(worst, res, sc)
        return res

    base = run({}, "heuristic")
    pgi._same(base, run({}, "heuristic again"), f"{tag} second run")
    pgi._same(base, run({"KH_PG_ROPE_FUSE": "0"}, "KH_PG_ROPE_FUSE=0"), f"{tag} KH_PG_ROPE_FUSE=0")
    solo = run(pgi._shape_hooks(shapes[0]), f"shape 0 {shapes[0]}", forced=shapes[0])
    pgi._same(solo, run({**pgi._shape_hooks(shapes[0]), "KH_PG_SOLO": "0"}, "shape 0 KH_PG_SOLO=0", forced=shapes[0]),
              f"{tag} shape 0 KH_PG_SOLO=0")
    run({"KH_PG_CHUNK": "100"}, "KH_PG_CHUNK=100")
    for i, sh in enumerate(shapes[1:], 1):
        run(pgi._shape_hooks(sh), f"shape {i} {sh}", forced=sh)
    return run


def one_shape_per_tile(shapes):
    """of pgi._shapes' walk (ks, four values, in the inner loop): the first shape of every register tile, and the last"""
    return shapes[:1] + shapes[4::4] + shapes[-1:]


# ---- slot prefill -----------------------------------------------------------------------------
def lone_segment_slot_prefill(core, m, spec, tiles):
    """seq_prefill(gemm=True) of one 300-token segment at slot 0 against prefill_gemm of the same tokens at each QKV
    register tile of `tiles` (None: the tile of the default shape): the K/V bytes are equal, the QKV GEMMs are
    k_rg_gemm_* and k_pg_gemm_* of that tile, no GEMM is on the old stem.  -> the launches on the core's stems"""
    toks = [int(t) for t in np.random.default_rng(21).integers(0, spec.vocab_size, 300)]
    launched = set()
    pg, rg, _ = core.stems
    try:
        m.seq_slots(1)
        for tile in tiles:
            pgi._set_hooks({"KH_PG_SHAPE_QKV": f"{tile[0]},{tile[1]},2"} if tile else {})
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            m.prefill_gemm(toks, 0)
            want = kv(m, spec, 0, 300)
            nan = np.full((300, spec.kv_dim), np.nan, np.float32)
            for layer in range(spec.n_layers):
                m.write_kv(layer, 0, nan, nan)
            m.seq_prefill(0, toks, gemm=True)
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            got = kv(m, spec, m.seq_row(0, 0), 300)
            for (k0, v0), (k1, v1) in zip(want, got):
                assert np.array_equal(k0, k1) and np.array_equal(v0, v1), tile
            qkv = "<%d,%d,0>" % tile if tile else "<"
            assert any(k.startswith(rg + qkv) for k in log) and any(k.startswith(pg + qkv) for k in log), (tile, sorted(log))
            assert not old_gemm_stems(log), sorted(log)
            launched |= new_stems(core, log)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        pgi._set_hooks({})
    return launched


# ---- the wide pass ----------------------------------------------------------------------------
N_WIDE = 40


def wide_sequences(spec):
    rng = np.random.default_rng(31)
    return [[int(t) for t in rng.integers(0, spec.vocab_size, 2 + s % 7)] for s in range(N_WIDE)]  # the last is stepped


def wide_gold(oracle, img_h, spec, seqs):
    """[{"64": the fp64 gold's logits behind the sequence's last token, "32": the fp32 oracle's}]"""
    gold = []
    for s in seqs:
        row = {}
        for tag, acc in (("64", oracle.ACC_F64), ("32", oracle.ACC_F32)):
            om = oracle.OracleModel.from_spec(img_h, spec, cache_len=16)
            for p, t in enumerate(s):
                lg = om.forward(t, p, acc)
            row[tag] = lg.copy()
            om.close()
        gold.append(row)
    return gold


def wide_forced_hooks(spec, forced):
    """((R, NT), ks, kz) -> ({QKV / RESID / SWIGLU / STORE: the tile that GEMM runs}, {hook: value}): a GEMM whose row
    count 32 does not divide has no 32-row tile and takes (1,4); SwiGLU workgroups hold two matrices (ks <= 4); the
    residual GEMMs alone split K over the grid (kz)."""
    (R, NT), ks, kz = forced
    r2 = {"QKV": True, "RESID": True, "SWIGLU": spec.hidden_dim % 32 == 0, "STORE": spec.vocab_size % 32 == 0}
    tile_of, hooks = {}, {}
    for h in WIDE_HOOKS:
        e = h.rsplit("_", 1)[1]
        tile_of[e] = (R, NT) if R == 1 or r2[e] else (1, 4)
        hooks[h] = "%d,%d,%d" % (tile_of[e] + (min(ks, 4) if e == "SWIGLU" else ks,)) + (f",{kz}" if e == "RESID" else "")
    return tile_of, hooks


def check_lane(lg, pick, g64, g32, floor, what, margin_rule=True):
    """One lane of a wide pass: the pick is the first maximum of its logit row, the row within max(floor + e32, 3 e32)
    of the gold (e32: the fp32 oracle against it), and the pick the gold's where the gold's top-2 margin exceeds
    2 x floor.  -> |row - gold|"""
    assert pick == int(np.argmax(lg)), (what, pick)
    e32 = float(np.abs(g32 - g64).max())
    err = float(np.abs(lg - g64).max())
    assert err <= max(floor + e32, 3.0 * e32), (what, err, e32)
    top2 = np.sort(g64)[-2:]
    if margin_rule and top2[1] - top2[0] > 2 * floor:
        assert pick == int(np.argmax(g64)), (what, pick)
    return err


def wide_runs(tiles):
    """[(lanes, None or ((R, NT), ks, kz))]: 3, 16 and 40 lanes at the default shapes, then six forced runs"""
    return [(n, None) for n in (3, 16, 40)] + list(zip(
        (3, 16, 40, 16, 40, 3),
        ((tiles[0], 1, 1), (tiles[1], 2, 2), (tiles[2], 4, 4), (tiles[0], 8, 1), (tiles[1], 4, 1), (tiles[2], 2, 2))))


def _cls_stem(core, sg, classes, what):
    """the classifier GEMM of a wide pass is on the core's stem exactly where cls is among `classes`"""
    on = "cls" in classes
    assert (3 in epilogues(new_stems(core, sg))) == on and (3 in epilogues(old_gemm_stems(sg))) == (not on), \
        (what, classes, sorted(sg))


def _wide_step(m, seqs, slots):
    """-> (picks, the k_sg_gemm* launches, every launch)"""
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        picks = m.seq_step(slots, [seqs[s][-1] for s in slots], [len(seqs[s]) - 1 for s in slots], gemm=True)
        log = set(_ffi.launch_log())
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    return picks, {k for k in log if k.startswith("k_sg_gemm")}, log


def wide_pass(core, m, spec, seqs, gold, classes, floor, what, worst):
    """seq_step(gemm=True) over wide_runs on a model whose classes are `classes` (cls among them): every lane holds
    check_lane, the launches check_stems, the classifier GEMM is on the core's stem, a forced run launches the forced
    tiles.  -> the launches on the core's stems"""
    launched = set()
    try:
        m.seq_slots(64)
        for lo in (0, 32):  # 32 tiles per call
            ss = list(range(lo, min(lo + 32, N_WIDE)))
            m.seq_prefill_many(ss, [seqs[s][:-1] for s in ss])
        for n, forced in wide_runs(core.wide_tiles):
            slots = [int(s) for s in np.random.default_rng(n).permutation(N_WIDE)[:n]]
            tile_of, hooks = wide_forced_hooks(spec, forced) if forced else ({}, {})
            for h, v in hooks.items():
                _ffi.debug_set(h, v)
            picks, sg, log = _wide_step(m, seqs, slots)
            for h in WIDE_HOOKS:
                _ffi.debug_set(h, None)
            for i, s in enumerate(slots):
                err = check_lane(m.seq_gemm_logits(i), picks[i], gold[s]["64"], gold[s]["32"], floor, (what, n, forced, i))
                worst["logit"] = max(worst["logit"], err)
            check_stems(core, f"{what} wide {n} {forced}", sg, classes)
            _cls_stem(core, sg, classes, (what, n, forced))
            if forced:
                want = {"%s<%d,%d,%d>" % ((core.stems[2],) + tile_of[e] + (i,))
                        for i, e in enumerate(("QKV", "RESID", "SWIGLU", "STORE")) if ("qkv", "wo", "ffn13", "cls")[i] in classes}
                assert want <= sg, (forced, sorted(want - sg), sorted(sg))
            launched |= new_stems(core, log)
    finally:
        for h in WIDE_HOOKS:
            _ffi.debug_set(h, None)
    return launched


def wide_16_lanes(core, m, spec, seqs, gold, classes, floor, what, worst=None, margin_rule=True):
    """The first 16 sequences in one pass at the default shapes on a model whose classes are `classes` - the default
    adoption mask's, plan(core, spec), in the modules that ran wide_pass under 0x1f: the other classes stay on the old
    stem, the lanes hold check_lane."""
    assert info(core, m)["classes"] == classes, (what, info(core, m))
    m.seq_slots(64)
    slots = list(range(16))
    m.seq_prefill_many(slots, [seqs[s][:-1] for s in slots])
    picks, sg, _ = _wide_step(m, seqs, slots)
    check_stems(core, f"{what} wide 16", sg, classes)
    _cls_stem(core, sg, classes, what)
    for i, s in enumerate(slots):
        err = check_lane(m.seq_gemm_logits(i), picks[i], gold[s]["64"], gold[s]["32"], floor, (what, 16, i),
                         margin_rule)
        if worst is not None:
            worst["logit"] = max(worst["logit"], err)


# ---- inert ------------------------------------------------------------------------------------
def inert_calls(m, spec, toks):
    """-> (picks, logits, wide rows) of a 100-token prefill_gemm, a fused step behind it and a 3-lane wide pass"""
    m.prefill_gemm(toks[:100], 0)
    m.predict(toks[100], 100, exec="fused")
    m.seq_slots(4)
    picks = m.seq_step([0, 1, 2], toks[:3], [0, 0, 0], gemm=True)
    return picks, m.logits(), [m.seq_gemm_logits(i) for i in range(3)]


def inert(core, spec, create, reason, what, calls=inert_calls):
    """create(False) - the model without the flag - and create(True) - the model it cannot take effect on: the core's
    info names `reason` ("flag not set" without the flag) with no class and no plan; `calls` launches the same set
    on both, none of it on a _gemm_w16 or the core's stems, and leaves equal picks, logits, wide rows and K/V bytes."""
    toks = [int(t) for t in np.random.default_rng(41).integers(0, spec.vocab_size, 101)]
    out = []
    for on in (False, True):
        m = create(on)
        try:
            got = info(core, m)
            want = {"on": False, "classes": [], "reason": reason if on else "flag not set", "plan": []}
            assert got == want, (what, on, got)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            res = calls(m, spec, toks)
            log = set(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            out.append((log, kv(m, spec, 0, 100)) + tuple(res))
        finally:
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            m.close()
    (log0, kv0, pk0, lg0, sg0), (log1, kv1, pk1, lg1, sg1) = out
    assert not [k for k in log1 if f"_gemm_{core.suffix}" in k or "_gemm_w16" in k], sorted(log1)
    assert log0 == log1, sorted(log0 ^ log1)
    assert np.array_equal(lg0, lg1) and pk0 == pk1 and len(sg0) == len(sg1)
    assert all(np.array_equal(a, b) for a, b in zip(sg0, sg1))
    for (k0, v0), (k1, v1) in zip(kv0, kv1):
        assert k0.tobytes() == k1.tobytes() and v0.tobytes() == v1.tobytes(), what


# ---- the class mask and the coverage gate -----------------------------------------------------
def class_mask_hook(core, img, spec):
    """the hook replaces the adoption mask at creation: the classes outside 0x5 keep the old stem"""
    m = model(core, img, spec, "0x5")
    try:
        assert info(core, m)["classes"] == ["qkv", "ffn13"]
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        m.prefill_gemm(list(range(40)), 0)
        check_stems(core, "mask 0x5", set(_ffi.launch_log()), ["qkv", "ffn13"])
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()


def coverage(stems, compiled, seen):
    """[(stem, its compiled instantiations, the launched ones)], each launched name a compiled one and each stem
    compiled at all; compiled and never launched is the caller's to report"""
    out = []
    for stem in stems:
        comp = {k for k in compiled if k.split("<")[0] == stem}
        got = {k for k in seen if k.split("<")[0] == stem}
        assert comp and got <= comp, (stem, sorted(got - comp))
        out.append((stem, comp, got))
    return out


def coverage_gate(core, need, launched, worst=None):
    """Every compiled instantiation of the core's stems is in `launched` ({test: names}, filled by the tests `need`
    names as they end)."""
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    missing = [t for t in need if t not in launched]
    assert not missing, f"tests that did not run to the end (run the whole module): {missing}"
    build.build_lib()
    compiled = co.kernels(co.code_object_notes(_ffi.LIB_PATH), set(core.stems))
    for stem, comp, got in coverage(core.stems, compiled, set().union(*launched.values())):
        print(f"{stem}: {len(got)} of {len(comp)} compiled instantiations launched and compared")
        assert not comp - got, f"{stem}: compiled and never launched: {sorted(comp - got)}"
    if worst is not None:
        print(f"worst |K/V - gold| {kv_text(worst)}, worst |logit - gold| {worst['logit']:.3e}")


# ---- the operator entries ---------------------------------------------------------------------
FMAX = np.finfo(np.float32).max
SPECIAL = {0: 0.0, 1: -0.0, 2: FMAX, 3: -FMAX}  # column -> value, on every other token


def x_values(rng, T, K):
    """full 24-bit significands over 2^+-30, both signs; SPECIAL in columns 0 .. 3"""
    m = rng.integers(1 << 23, 1 << 24, (T, K)).astype(np.float64)
    e = rng.integers(-30, 31, (T, K)).astype(np.float64)
    x = (rng.choice([-1.0, 1.0], (T, K)) * m * np.exp2(e - 23)).astype(np.float32)
    for c, v in SPECIAL.items():
        x[(c & 1)::2, c] = np.float32(v)
    return x


def assert_same_bits(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), f"{what}: {len(bad)} of {got.size} differ, first (token, row) {bad[0]}: " \
                         f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def one_hot(run, gpu, x, wv, K, what):
    """Row r of W holds the single value wv[r] at column r mod K: y[t][r] is one product, an fp32 value, added to +0 -
    and must be it bit for bit."""
    M = len(wv)
    col = np.arange(M) % K
    w = np.zeros((M, K), np.float32)
    w[np.arange(M), col] = wv
    got = run(gpu, x, w)
    p64 = x[:, col].astype(np.float64) * wv[None, :].astype(np.float64)
    want = np.float32(0) + p64.astype(np.float32)
    assert np.isfinite(want).all() and np.array_equal(want.astype(np.float64), p64 + 0.0)
    assert_same_bits(got, want, what)


def general_case(core, run, gpu, round_w):
    """random x against random weights rounded to the core's 16-bit format (round_w): within twice the error of the
    fp32 GEMV (kh_matmul_f32, row by row) on the same operands against an fp64 matmul, plus one ulp of the largest |y|"""
    rng = np.random.default_rng(99)
    T, K, M = 64, 1024, 128
    w = round_w(rng.standard_normal((M, K), dtype=np.float32) * np.float32(0.05))
    x = rng.standard_normal((T, K), dtype=np.float32)
    y64 = x.astype(np.float64) @ w.astype(np.float64).T
    got = run(gpu, x, w)
    xd, wd = torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu)
    y32 = torch.empty((T, M), dtype=torch.float32, device=gpu)
    for t in range(T):  # the fp32 yardstick: the GEMV kernel of kh_matmul_f32, one row of x at a time
        ops.matmul(xd[t], wd, y32[t])
    torch.cuda.synchronize()
    e16 = float(np.abs(got - y64).max())
    e32 = float(np.abs(y32.cpu().numpy() - y64).max())
    ulp = float(np.spacing(np.float32(np.abs(y64).max())))
    print(f"{core.op} vs fp64: {e16:.3e}; kh_matmul_f32 vs fp64: {e32:.3e}; 1 ulp of max |y|: {ulp:.3e}")
    assert e16 <= 2.0 * e32 + ulp


def preconditions(core, gpu):
    """the entry of a 16-bit core refuses M % 16, K % 32 and T > 512"""
    def rc(T, M, K):
        x = torch.zeros((T, K), dtype=torch.float32, device=gpu)
        w = torch.zeros((M, K), dtype=torch.int16, device=gpu)
        y = torch.zeros((T, (M + 3) // 4 * 4), dtype=torch.float32, device=gpu)
        return getattr(_ffi.lib(), core.entry)(x.data_ptr(), w.data_ptr(), y.data_ptr(), T, M, K, y.stride(0), None)
    assert rc(4, 24, 32) == _ffi.KH_ERR_UNSUPPORTED   # M % 16
    assert rc(4, 16, 48) == _ffi.KH_ERR_UNSUPPORTED   # K % 32
    assert rc(513, 16, 32) == _ffi.KH_ERR_UNSUPPORTED  # T > 512
    assert rc(512, 16, 32) == 0


# ---- host side --------------------------------------------------------------------------------
def check_abi(core, flag_value, n_reasons):
    """the core's entries, flag, hooks, Python names and sources are where a caller finds them"""
    build.build_lib()
    L = _ffi.lib()
    entries = ("kh_model_" + core.info, "kh_" + core.plan, core.entry)
    for n in entries:
        assert n in _ffi.EXPORTS and hasattr(L, n)
    assert core.flag == flag_value
    others = [v for k, v in vars(_ffi).items() if k.startswith("KH_FLAG_") and k != core.flag_name]
    assert len(others) >= 8 and not any(core.flag & v for v in others), others
    src = open(os.path.join(build.CSRC, "..", "..", "include", "kuiper_hip.h")).read()
    assert f"#define {core.flag_name} {flag_value}" in src
    for n in entries:
        assert f"int {n}(" in src, n
    assert getattr(L, "kh_model_" + core.info)(None, None) == _ffi.KH_ERR_INVALID_ARG
    for hook in (core.hook, core.classes_hook):
        assert hook.startswith(_ffi._HOOK_PREFIXES)  # sync_env mirrors it from the environment
        assert _ffi.debug_get(hook) is None
        try:
            _ffi.debug_set(hook, "1")
            assert _ffi.debug_get(hook) == "1"
        finally:
            _ffi.debug_set(hook, None)
    from kuiperllama_amd.model import KuiperModel
    assert callable(getattr(KuiperModel, core.info)) and callable(getattr(ops, core.op))
    assert len(getattr(_ffi, core.hook + "_REASONS")) == n_reasons
    assert f"kh_model_gemm_{core.suffix}.hip" in build.SOURCES and f"kh_gemm_{core.suffix}.h" in build.HEADERS


def compiled_kernels(core):
    """what the library is to hold of the core's stems: the prefill stems at every tile x the epilogues QKV, RESID and
    SWIGLU, the slot prefill's QKV GEMM at every tile, the wide pass at its tiles x the four epilogues"""
    pg, rg, sg = core.stems
    return {pg: {f"{pg}<{r},{nt},{e}>" for r, nt in core.tiles for e in (0, 1, 2)},
            rg: {f"{rg}<{r},{nt},0>" for r, nt in core.tiles},
            sg: {f"{sg}<{r},{nt},{e}>" for r, nt in core.wide_tiles for e in (0, 1, 2, 3)}}


def check_code_objects(core):
    """The three stems are compiled for exactly compiled_kernels(core), and none of them uses scratch."""
    if not co.tools_present():
        import pytest
        pytest.skip("LLVM tools of the ROCm install not found")
    notes = co.code_object_notes(build.build_lib())
    for stem, w in compiled_kernels(core).items():
        got = co.instantiations(notes, {stem})
        assert got == w, (stem, sorted(got - w), sorted(w - got))
    scratch = {k: v for k, v in co.kernel_scratch(notes).items() if f"_gemm_{core.suffix}" in k and v}
    assert not scratch, scratch
