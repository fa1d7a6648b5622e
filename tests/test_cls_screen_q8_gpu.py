"""The int8 tier ahead of the bf16 classifier screen (csrc/kh_cls_screen.h: k_cls_q8_build, k_cls_screen_q8 and the
survivor mode of k_cls_screen) on the GPU.

Tier 1 claims, per row, that the logit k_cls would store lies in [lb8, ub8]; the rows whose upper bound reaches the best
lower bound go on to the bf16 screen, every other row is dropped for the step.  A wrong bound drops the true argmax: it
does not crash, it picks a wrong token.  So, on the smallest shapes that can go wrong - dim 448 (seven groups, a partial
tile, odd vocabulary), 1152 and 2304 (two and three loads per lane), each under the planned launch and under the
KH_SHAPE_SCREEN_Q8 cells that reach every compiled <U, MAXV> - this file checks
  the copy     e8[r] >= |w_r - sc o q_r|_2 in fp64 from the read-back copy, |q| <= 127, sc >= 0, e8 = inf for NaN / Inf rows;
  containment  k_cls's stored logit and the fp64 gold inside [lb8, ub8] for every row, no tolerance, on a unit-normal
               vector, one with x50 outliers, all zeros, and vectors whose g is parallel to one row's quantisation error
               (built from the read-back copy; they use over 0.9 of b8, checked on the numpy twin first);
  survivors    every row that holds the largest logit survives; the tail's token is the full step's;
  grids        the same intervals bit for bit at tier-1 grids 1, 3, planned and 4096;
  spill        one tier-1 workgroup over thirteen qualifying rows spills, the bf16 launch scans every row, same token;
  generate     graph and fused exec, across position 256, behind both prefills, with a stop token: words and logits()
               bit-identical to KH_CLS_SCREEN_Q8=0 and to KH_CLS_SCREEN=0, three tail kernels in the launch log;
  off          every hook that makes the tier step aside, a failed tier self-test, dim % 64 != 0, int8 models,
               KH_FLAG_NO_CLS_SCREEN.
"""
import dataclasses

import numpy as np
import pytest
import torch

import cls_screen_q8_ref as Q
import cls_screen_ref as R
import code_objects as co
import test_cls_screen_gpu as T
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 1e-5
VOCAB = 3001
PROMPT = [1, 263]
HEADS = {448: (7, 7), 1152: (18, 6), 2304: (18, 6), 224: (7, 7)}
# special rows of the images
HUGE_ROW, ZERO_ROW, NAN_ROW, INF_ROW = 40, 41, 1500, 2999  # 2999 / 3000: the last full pair and the odd last row
RSTAR = 1601
CROWD_ROWS = tuple(33 + 230 * i for i in range(12))  # with r*: thirteen rows inside each other's int8 interval
ALIGNED_ROWS = (7, 3000)
# (dim, hook) -> the <U, MAXV> cell it launches; None: the planned launch.  Workgroup width 256 stages deeper.
CELLS = [(448, None), (448, "4,37,512"), (448, "2,37,512"), (1152, None), (1152, "4,37,256"), (1152, "2,37,256"),
         (2304, None), (2304, "4,37,256"), (2304, "2,37,256")]
_LAUNCHED = set()
_DONE = set()


def _spec(dim, layers=1, vocab=VOCAB, quant=False):
    h, kv = HEADS[dim]
    return binfmt.ModelSpec(dim, 512, layers, h, kv, vocab, 256, False, binfmt.FAMILY_LLAMA, quant, 64,
                            binfmt.ROPE_INTERLEAVED, 10000.0, EPS, f"scr8-{dim}")


def _maxv(dim, wg):
    return next(v for v in (1, 2, 4, 6) if dim <= v * 4 * wg)


def _view(spec, img, name):
    e = {e.name: e for e in binfmt.layout(spec)[0]}[name]
    return img[e.offset: e.offset + e.nbytes].view(F32).reshape(e.shape)


_IMG = {}


def _image(dim):
    """Host image of a dim with the special rows, its norm weight, the unit probe and g0 = w_norm o x0."""
    if dim not in _IMG:
        _IMG.clear()
        spec = _spec(dim)
        img = binfmt.synth_image(spec, seed=dim).numpy().copy()
        rng = np.random.default_rng(7000 + dim)
        wn = rng.normal(0.0, 1.0, dim).astype(F32)
        wn[np.abs(wn) < 0.05] = F32(0.05)  # the aligned probes divide by it
        _view(spec, img, "final_norm")[:] = wn
        x0 = rng.normal(0.0, 1.0, dim).astype(F32)
        g0 = (wn * x0).astype(F32)
        W = _view(spec, img, "wcls")
        W[HUGE_ROW] = (F32(-1e28) * g0).astype(F32)  # a huge row, far below every other logit on the unit probe
        W[ZERO_ROW] = 0
        W[NAN_ROW, dim // 5] = np.nan
        W[INF_ROW, 3] = -np.inf
        rstar = (F32(0.02) * g0).astype(F32)
        W[RSTAR] = rstar
        for j, r in enumerate(CROWD_ROWS, start=2):
            W[r] = (rstar * F32(1.0 - j * 2.0 ** -13)).astype(F32)
        _IMG[dim] = dict(spec=spec, img=img, wn=wn, x0=x0, W=W.copy(), W64=W.astype(np.float64))
    return _IMG[dim]


def _inside(v, lb, ub):
    nan = np.isnan(v)
    with np.errstate(all="ignore"):
        return np.where(nan, (lb == -np.inf) & (ub == np.inf), (lb <= v) & (v <= ub))


def _lowest_argmax(lg):
    return int(np.argmax(np.where(np.isnan(lg), -np.inf, lg)))


def _model(spec, img, hooks=None, flags=0):
    from kuiperllama_amd.model import KuiperModel
    hooks = hooks or {}
    try:
        for k, v in hooks.items():
            _ffi.debug_set(k, v)
        return KuiperModel.from_host_image(np.ascontiguousarray(img), spec, flags=flags)
    finally:
        for k in hooks:
            _ffi.debug_set(k, None)


def _probe(m, im, x, what, grid=0):
    """One probe vector: containment (k_cls's logit and the fp64 gold), the non-finite rows, survivors, tokens."""
    p = m.cls_screen_q8_probe(x, grid)
    lg = m.logits()
    lb, ub = p["lb"], p["ub"]
    bad = np.flatnonzero(~_inside(lg, lb, ub))
    assert bad.size == 0, f"{what}: k_cls logit outside [lb8, ub8], rows {bad[:5]}: {lg[bad[:5]]} not in " \
                          f"[{lb[bad[:5]]}, {ub[bad[:5]]}] ({bad.size} rows)"
    gold = R.gold_logits64(im["W"], x, im["wn"], F32(EPS))
    bad = np.flatnonzero(~_inside(gold, lb.astype(np.float64), ub.astype(np.float64)))
    assert bad.size == 0, f"{what}: fp64 gold outside [lb8, ub8], rows {bad[:5]}: {gold[bad[:5]]} not in " \
                          f"[{lb[bad[:5]]}, {ub[bad[:5]]}] ({bad.size} rows)"
    for r in (NAN_ROW, INF_ROW):
        assert lb[r] == -np.inf and ub[r] == np.inf, f"{what}: non-finite row {r} has [{lb[r]}, {ub[r]}]"
    want = _lowest_argmax(lg)
    assert p["token"] == p["full_token"] == want, f"{what}: tail {p['token']}, full step {p['full_token']}, argmax {want}"
    with np.errstate(all="ignore"):
        surv = ub >= lb.max()
    top = np.flatnonzero(lg == np.nanmax(lg))
    assert surv[top].all(), f"{what}: rows {top[~surv[top]]} hold the largest logit and did not survive tier 1"
    if not p["spill"]:
        assert p["survivors"] == int(surv.sum()), f"{what}: {p['survivors']} survivors counted, {int(surv.sum())} rows qualify"
    p["logits"] = lg
    return p


def _aligned_probe(im, q, sc, r, k=0.5):
    """x with w_norm o x (nearly) parallel to row r's quantisation error: Cauchy-Schwarz is tight for that row."""
    d = im["W64"][r] - Q.dequant64(q[r:r + 1], sc[r:r + 1])[0]
    return (k * d / np.linalg.norm(d) * np.sqrt(d.size) / im["wn"].astype(np.float64)).astype(F32)


@pytest.mark.parametrize("dim,hook", CELLS, ids=[f"{d}-{h or 'planned'}" for d, h in CELLS])
def test_copy_containment_survivors(gpu, dim, hook):
    im = _image(dim)
    spec = im["spec"]
    m = _model(spec, im["img"], {"KH_SHAPE_SCREEN_Q8": hook})
    what = f"dim {dim} {hook or 'planned'}"
    try:
        info = m.cls_screen_q8_info()
        assert info["on"] == 1 and info["selftest"] == 1 and m.cls_screen_info()["on"] == 1, f"{what}: {info}"
        assert info["bytes"] == VOCAB * dim + VOCAB * (dim // 64) * 4 + VOCAB * 4
        wg = int(hook.split(",")[2]) if hook else 256  # the planned launch: 256-thread workgroups
        # ---- the copy
        q, sc, e8 = m.cls_screen_q8_read()
        assert np.abs(q.astype(np.int32)).max() <= 127 and np.all(sc >= 0), what
        e64 = Q.quant_err64(im["W"], q, sc)
        fin = np.isfinite(e64)
        assert not fin[NAN_ROW] and not fin[INF_ROW] and fin.sum() == VOCAB - 2
        assert np.all(e8[~fin] == np.inf), f"{what}: NaN / Inf rows must carry e8 = +inf"
        low = np.flatnonzero(fin & ~(e8.astype(np.float64) >= e64))
        assert low.size == 0, f"{what}: e8 below the fp64 quantisation error in rows {low[:5]}"
        assert np.all(np.isfinite(e8[fin])), f"{what}: a finite row lost its bound"
        # ---- probes
        rng = np.random.default_rng(dim)
        y = im["x0"].copy()
        y[::61] *= 50.0
        _LOG_ON()
        out = _probe(m, im, im["x0"], f"{what} unit")
        assert out["token"] == RSTAR and out["spill"] == 0 and out["overflow"] == 0, out["token"]
        assert out["survivors"] >= 13  # r* and its twelve near copies
        _probe(m, im, y, f"{what} outliers")
        _probe(m, im, (im["x0"] * F32(1e-18)).astype(F32), f"{what} tiny")
        z = _probe(m, im, np.zeros(dim, F32), f"{what} zeros")
        # every logit equal: every row qualifies (a tier-1 workgroup with more than eight rows spills), the step overflows
        assert z["token"] == 0 and z["overflow"] == 1, f"{what}: all-zeros vector: {z['token']}, overflow {z['overflow']}"
        assert z["spill"] == 1 or z["survivors"] == VOCAB, f"{what}: all-zeros vector: {z['survivors']} survivors without a spill"
        for r in ALIGNED_ROWS:
            x = _aligned_probe(im, q, sc, r)
            # condition on the input, on the twin: row r uses more than 0.9 of its half-width
            g, rs, cb = R.stage(x, im["wn"], EPS, wg)
            a8, b8, _, _ = R.interval(Q.lane_dot_q8(q[r:r + 1], sc[r:r + 1], g), e8[r:r + 1], rs, cb)
            tl = (R.lane_dot(im["W"][r:r + 1], g, 4) * rs).astype(F32)
            use = float(abs(float(tl[0]) - float(a8[0])) / float(b8[0]))
            assert use > 0.9, f"{what}: aligned probe of row {r} uses {use:.4f} of b8 on the twin (condition on the input)"
            p = _probe(m, im, x, f"{what} aligned {r}")
            guse = abs(float(p["logits"][r]) - (float(p["lb"][r]) + float(p["ub"][r])) / 2) / ((float(p["ub"][r]) - float(p["lb"][r])) / 2)
            print(f"{what}: aligned row {r} uses {use:.4f} of b8 on the twin, {guse:.4f} on the GPU")
            assert guse > 0.9, f"{what}: the GPU's interval of row {r} is looser than the twin's ({guse:.4f})"
        after = m.cls_screen_q8_info()
        assert (after["steps"], after["survivors"], after["spill_steps"]) == (0, 0, 0), f"{what}: the probe moved the counters"
        assert m.cls_screen_info()["steps"] == 0
        # ---- the twin's interval of the unit probe: same finite set, close bounds (the order of the sums is the kernel's)
        a8, b8, lb8, ub8 = Q.intervals(q, sc, e8, im["x0"], im["wn"], EPS, wg)
        tf = np.isfinite(lb8) & np.isfinite(ub8)
        assert np.array_equal(tf, np.isfinite(out["lb"]) & np.isfinite(out["ub"])), f"{what}: finite intervals differ from the twin's"
        with np.errstate(all="ignore"):
            d = np.maximum(np.abs(out["lb"].astype(np.float64) - lb8), np.abs(out["ub"].astype(np.float64) - ub8))[tf]
        # both are fp32 sums of the same products in a valid order (each within gamma_n of the exact sum), rounded a -+ b
        g, rs, _ = R.stage(im["x0"], im["wn"], EPS, wg)
        with np.errstate(all="ignore"):
            tau = Q.gamma2(dim) * float(rs) * np.sqrt((Q.dequant64(q, sc) ** 2).sum(1)) * np.linalg.norm(g.astype(np.float64)) + \
                2.0 ** -5 * b8.astype(np.float64)
        assert np.all(d <= tau[tf]), f"{what}: bounds {float((d / tau[tf]).max()):.3g} tau from the twin's"
        if hook is None:
            # ---- grids: bit-identical intervals; one workgroup spills on the thirteen rows and the token stays
            for grid in (1, 3, 4096):
                p = _probe(m, im, im["x0"], f"{what} grid {grid}", grid)
                assert np.array_equal(p["lb"].view(np.uint32), out["lb"].view(np.uint32)) and \
                    np.array_equal(p["ub"].view(np.uint32), out["ub"].view(np.uint32)), f"{what}: grid {grid} changes the intervals"
                assert p["token"] == RSTAR
                assert p["spill"] == (1 if grid == 1 else 0), f"{what}: grid {grid}: spill {p['spill']}"
                # spilled (the full bf16 scan) or not (tier 1's slots spread over the bf16 workgroups, at most four of the
                # fifteen rows in one of them): k_sample_screen gets the same fifteen rows and does not overflow
                assert (p["overflow"], p["candidates"]) == (0, out["candidates"]), \
                    f"{what}: grid {grid}: overflow {p['overflow']}, {p['candidates']} candidates, planned {out['candidates']}"
        _LAUNCHED.update(k for k in _ffi.launch_log() if k.startswith("k_cls_screen_q8<"))
        u = int(hook.split(",")[0]) if hook else (4 if (dim // 16 + 63) // 64 >= 3 else 2)
        assert f"k_cls_screen_q8<{u},{_maxv(dim, wg)}>" in _LAUNCHED, (what, sorted(_LAUNCHED))
        _DONE.add((dim, hook))
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()


def _LOG_ON():
    _ffi.debug_set("KH_LAUNCH_LOG", "1")


def test_every_compiled_tier1_instantiation_was_launched(gpu):
    """The coverage gate: every compiled k_cls_screen_q8<U, MAXV> was launched (and checked) by the cells above."""
    missing = sorted(map(str, set(CELLS) - _DONE))
    assert not missing, f"cells that did not run to the end (run the whole module): {missing}"
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    have = co.instantiations(co.code_object_notes(_ffi.LIB_PATH), {"k_cls_screen_q8"})
    assert have == {f"k_cls_screen_q8<{u},{mv}>" for u in (4, 2) for mv in (4, 2, 1)}, sorted(have)
    assert _LAUNCHED <= have, f"launched but not found in the code objects: {sorted(_LAUNCHED - have)}"
    assert not have - _LAUNCHED, f"compiled and never launched: {sorted(have - _LAUNCHED)}"


# ---- generate ------------------------------------------------------------------------------------------------------
def _run(m, prompt, steps, **kw):
    words, _ = m.generate(prompt, steps, **kw)
    return words, m.logits()


def _three(m, fn, what, expect_overflow=False):
    """fn() with the tier, under KH_CLS_SCREEN_Q8=0 and under KH_CLS_SCREEN=0: identical; the tier's counters."""
    try:
        j0, i0 = m.cls_screen_q8_info(), m.cls_screen_info()
        a = fn()
        j1, i1 = m.cls_screen_q8_info(), m.cls_screen_info()
        _ffi.debug_set("KH_CLS_SCREEN_Q8", "0")
        b = fn()
        j2 = m.cls_screen_q8_info()
        _ffi.debug_set("KH_CLS_SCREEN_Q8", None)
        _ffi.debug_set("KH_CLS_SCREEN", "0")
        c = fn()
    finally:
        _ffi.debug_set("KH_CLS_SCREEN_Q8", None)
        _ffi.debug_set("KH_CLS_SCREEN", None)
    T._same(a, b, f"{what} vs KH_CLS_SCREEN_Q8=0")
    T._same(a, c, f"{what} vs KH_CLS_SCREEN=0")
    assert j2["steps"] == j1["steps"], f"{what}: KH_CLS_SCREEN_Q8=0 still ran tier-1 steps"
    d = {k: j1[k] - j0[k] for k in ("steps", "survivors", "spill_steps")}
    d["overflow_steps"] = i1["overflow_steps"] - i0["overflow_steps"]
    assert d["steps"] > 0 and d["steps"] == i1["steps"] - i0["steps"], f"{what}: {d}"
    if not expect_overflow:
        assert d["spill_steps"] == 0 and d["overflow_steps"] == 0, f"{what}: {d}"
    return a, d


def _check_generate(m, what, long_steps, expect_overflow=False):
    info = m.cls_screen_q8_info()
    assert info["on"] == 1 and info["selftest"] == 1, info
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        a, d = _three(m, lambda: _run(m, PROMPT, long_steps), f"{what} graph", expect_overflow)
        log = _ffi.launch_log()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    for stem in ("k_cls_screen_q8<", "k_cls_screen<", "k_sample_screen<"):
        assert any(k.startswith(stem) for k in log), (stem, log)
    print(f"{what}: {d['steps']} tier-1 steps, {d['survivors'] / d['steps']:.2f} survivors per step, {d['spill_steps']} spills, "
          f"{d['overflow_steps']} overflow steps")
    if expect_overflow:
        assert d["overflow_steps"] > 0, d
    words = a[0]
    f, _ = _three(m, lambda: _run(m, PROMPT, 48, exec="fused"), f"{what} fused", expect_overflow)
    assert f[0] == words[:48], f"{what}: fused and graph words differ"
    s, _ = _three(m, lambda: _run(m, PROMPT, 48, stop=[words[11]]), f"{what} stop", expect_overflow)
    assert len(s[0]) <= 11
    for n in (7, 21):  # 6 fed-only tokens: the B-token prefill; 20: the GEMM prefill
        prompt = [1] + [int(t) for t in words[:n - 1]]
        _three(m, lambda: _run(m, prompt, n + 24), f"{what} prefill {n}", expect_overflow)
    return words


def test_generate_llama_geometry_across_position_256(gpu):
    """Two layers of Llama-3.2-1B at its full width and vocabulary: the planned grids of both tiers, 300 steps."""
    from kuiperllama_amd.model import KuiperModel
    spec = dataclasses.replace(binfmt.PRESETS["llama3.2-1b"], n_layers=2, seq_len=512)
    img = binfmt.synth_image(spec, seed=77, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec)
    try:
        words = _check_generate(m, "llama3.2-1b x2", 300)
        assert len(set(words[2:])) > 8, "the sequence was meant to wander"
        info = m.cls_screen_q8_info()
        assert info["bytes"] == spec.vocab_size * (spec.dim + spec.dim // 64 * 4 + 4)
        assert m.cls_screen_info()["bytes"] == spec.vocab_size * spec.dim * 2 + spec.vocab_size * 4
    finally:
        m.close()


def test_generate_adv_geometry_and_the_crowd_still_overflows(gpu):
    img, view = T._adv_image()
    m = _model(T.ADV, img)
    try:
        base = _check_generate(m, "adv", 64)
    finally:
        m.close()
    w = base[1]
    W = view("wcls")
    src = W[w].copy()
    for i in range(300):  # test_cls_screen_gpu's crowd: copies of the best row with last-bit perturbations
        r = src.copy()
        r[i] = np.nextafter(r[i], F32(np.inf) if i % 2 else F32(-np.inf))
        W[(w + 1 + 13 * i) % T.ADV.vocab_size] = r
    m = _model(T.ADV, img)
    try:
        _check_generate(m, "adv crowd", 64, expect_overflow=True)
    finally:
        m.close()


# ---- the tier steps aside ------------------------------------------------------------------------------------------
def _no_tier(m, want, what, on):
    """The tier reports `on`, a generate launches no k_cls_screen_q8, decoding is `want` (None: what the same model
    decodes under KH_CLS_SCREEN=0 on top of the hooks that are set - a hooked k_cls sums in its own order)."""
    assert m.cls_screen_q8_info()["on"] == on, (what, m.cls_screen_q8_info())
    if want is None:
        was = _ffi.debug_get("KH_CLS_SCREEN") if hasattr(_ffi, "debug_get") else None
        try:
            _ffi.debug_set("KH_CLS_SCREEN", "0")
            want = _run(m, PROMPT, 32)
        finally:
            _ffi.debug_set("KH_CLS_SCREEN", was)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        got = _run(m, PROMPT, 32)
        log = _ffi.launch_log()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    assert not any(k.startswith("k_cls_screen_q8") for k in log), (what, log)
    T._same(got, want, what)
    j = m.cls_screen_q8_info()
    assert (j["steps"], j["survivors"], j["spill_steps"]) == (0, 0, 0), (what, j)
    return got


def test_tier_off(gpu):
    img, _ = T._adv_image()
    m = _model(T.ADV, img)
    try:
        assert m.cls_screen_q8_info()["on"] == 1
        want = _run(m, PROMPT, 32)
        assert m.cls_screen_q8_info()["steps"] >= 32
    finally:
        m.close()
    shape_cls = "1,2,64,256"  # split, u, grid, wg
    for what, hooks, on, screen_on in (
            ("KH_CLS_SCREEN_Q8=0 at creation", {"KH_CLS_SCREEN_Q8": "0"}, 0, 1),
            ("KH_SHAPE_SCREEN", {"KH_SHAPE_SCREEN": "2,37,256"}, 0, 1),
            ("KH_SHAPE_CLS", {"KH_SHAPE_CLS": shape_cls}, 0, 0),
            ("KH_SHAPE_CLS + force", {"KH_SHAPE_CLS": shape_cls, "KH_CLS_SCREEN": "force"}, 0, 1),
            ("failed tier self-test", {"KH_SELFTEST_FAIL": "screen8"}, 0, 1)):
        m = _model(T.ADV, img, hooks)
        try:
            assert m.cls_screen_info()["on"] == screen_on, (what, m.cls_screen_info())
            if what.startswith("failed"):
                j = m.cls_screen_q8_info()
                assert j["selftest"] == -1 and j["bytes"] == 0 and m.cls_screen_info()["selftest"] == 1, j
            for k, v in hooks.items():  # the shape hooks also bar the tier while they are set
                if k != "KH_SELFTEST_FAIL":
                    _ffi.debug_set(k, v)
            _no_tier(m, None if "KH_SHAPE_CLS" in hooks else want, what, on)
            if screen_on:
                assert m.cls_screen_info()["steps"] >= 32, what
        finally:
            for k in hooks:
                _ffi.debug_set(k, None)
            m.close()
    # a hook set later: a model with the tier steps aside for the generates that follow
    m = _model(T.ADV, img)
    try:
        for k, v in (("KH_CLS_SCREEN_Q8", "0"), ("KH_SHAPE_SCREEN", "2,37,256"), ("KH_SHAPE_CLS", shape_cls)):
            try:
                _ffi.debug_set(k, v)
                _no_tier(m, want, f"{k} per generate", 1)
            finally:
                _ffi.debug_set(k, None)
        T._same(_run(m, PROMPT, 32), want, "tier back on")
        assert m.cls_screen_q8_info()["steps"] >= 32
    finally:
        m.close()
    # the bf16 screen failing its own self-test takes the tier with it
    m = _model(T.ADV, img, {"KH_SELFTEST_FAIL": "screen"})
    try:
        assert m.cls_screen_info()["selftest"] == -1
        _no_tier(m, want, "failed bf16 self-test", 0)
    finally:
        m.close()


def test_dim_not_a_multiple_of_64_keeps_the_bf16_screen(gpu):
    spec = _spec(224, layers=2)
    img = binfmt.synth_image(spec, seed=9).numpy().copy()
    m = _model(spec, img, {"KH_CLS_SCREEN": "0"})
    try:
        want = _run(m, PROMPT, 32)
    finally:
        m.close()
    m = _model(spec, img)
    try:
        assert m.cls_screen_info()["on"] == 1
        _no_tier(m, want, "dim 224", 0)
        assert m.cls_screen_info()["steps"] >= 32
    finally:
        m.close()


def test_not_applicable(gpu):
    img, _ = T._adv_image()
    m = _model(T.ADV, img, flags=_ffi.KH_FLAG_NO_CLS_SCREEN)
    try:
        _no_tier(m, None, "KH_FLAG_NO_CLS_SCREEN", 0)
        assert m.cls_screen_info()["on"] == 0
        with pytest.raises(Exception):
            m.cls_screen_q8_probe(np.zeros(T.ADV.dim, F32))
    finally:
        m.close()
    qspec = dataclasses.replace(T.ADV, quant=True)
    qimg = binfmt.synth_image(qspec, seed=5).numpy().copy()
    m = _model(qspec, qimg)
    try:
        _no_tier(m, None, "int8 model", 0)
        assert m.cls_screen_info()["on"] == 0 and m.cls_screen_info()["steps"] == 0
    finally:
        m.close()
