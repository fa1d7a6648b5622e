"""Every compiled k_cls_screen / k_sample_screen instantiation, launched on the GPU and checked row by row against
fp64 and against the numpy twin of tests/cls_screen_ref.py.

The screened classifier (csrc/kh_cls_screen.h) claims, per row, that the logit k_cls would store lies in [lb, ub].  A
wrong bound does not crash: it picks a wrong token, and only when the true argmax falls just outside its interval.
Here one-layer models (untied classifier, vocabulary 3001, 256 cache rows) at dim 448, 1152, 2304 and 4224 - the
smallest dims that reach every (U, MAXV) cell: partial single tile / two partial tiles / two tiles with 32 live lanes
in the second and two re-score chunks / three tiles - are created under the planned launch, under every
KH_SHAPE_SCREEN (u, wg) cell and under KH_SHAPE_CLS + KH_CLS_SCREEN=force (k_sample_screen follows k_cls's U, staging
depth and width).  Final-norm weights are N(0, 1) x 0.25 and x 4, so |g| is far from |x|.  kh_model_cls_screen_probe
runs one screened and one full step on a given residual vector and returns every row's interval.

Classifier images per (dim, norm scale); g0 = w_norm o x of the unit-normal probe:
  special  random rows + the special rows of test_cls_screen.py::_rows + a NaN row + a row with an Inf weight + a row
           with a 3.4e38 weight (finite in fp32, +inf as bf16) + the
           aligned rows w = bf16(k g0) (1 + 0.9 2^-9), k = +-0.01, +-0.003 (bf16 error parallel to g0: Cauchy-Schwarz
           is tight, they use over 0.95 of their half-width b);
  spill    random rows + r* = bf16(0.02 g0) (exact in bf16: tiny b) + six rows r* (1 - j 2^-13), j = 2..7, which rank
           above r* by upper bound while r* is the argmax: one workgroup hands over four of them, not r*;
  crowd    the same with j = 2..13: more candidates than k_sample_screen has waves, all with distinct logits;
  cap32 / cap33   r* + 31 / 32 copies with one element moved by one fp32 ulp, 64 rows apart: the candidate cap.

Per configuration (on == 1 and selftest == 1 asserted first): the bf16 copy bit for bit, err[] against fp64 and
within one ulp of the twin's, and per probe vector (unit, x50 outliers, x1e-18, zeros, one non-zero element):
k_cls's stored logit and the fp64 gold inside [lb, ub] for every row with no tolerance, (-inf, +inf) for the
non-finite rows, lb / ub within tau_r of the twin's (cls_screen_ref.twin_tolerance), screened token == full
classifier's token == lowest-index argmax of the logits.  Then, in the planned, the KH_SHAPE_SCREEN and the forced
configurations alike, the spill path, the crowd, the cap and a 24-step generate in graph and fused exec against
KH_CLS_SCREEN=0; under the planned launch also the grids (1, 3, need, 4096: same intervals bit for bit) and the
refused hooks.  The gates at the end compare the launch log with the instantiations in the library's code objects
and print the run's figures (worst |d| / tau, bit-identical share, largest use of b, most candidates).
"""
import numpy as np
import pytest
import torch

import cls_screen_ref as R
import code_objects as co
from kuiperllama_amd import _ffi, binfmt, build
from test_cls_screen import _rows as _special_rows

pytestmark = pytest.mark.gpu

F32 = np.float32
VOCAB = 3001
DIMS = (448, 1152, 2304, 4224)
SCALES = (0.25, 4.0)
EPS = 1e-5
PROMPT = [1, 263]
STEPS = 24
STEMS = ("k_cls_screen", "k_sample_screen")
# dim -> (heads, kv heads)
HEADS = {448: (7, 7), 1152: (18, 6), 2304: (18, 6), 4224: (33, 3), 252: (7, 7)}

# row layout of the images
ALIGNED = {7: 0.01, 1203: -0.01, 2410: 0.003, 3000: -0.003}  # row 3000: the last pair is one row
SPECIAL0, SPECIAL_STRIDE = 100, 37
NAN_ROW, INF_ROW = 1500, 2999
BIG_ROW = 2000  # one weight of 3.4e38: finite in fp32, +inf as bf16 (the 3e38 of _rows stays finite: bf16 max is 3.39e38)
RSTAR = 1601
SPILL_ROWS = (90, 500, 950, 1400, 2100, 2800)  # j = 2..7
CROWD_ROWS = tuple(33 + 230 * i for i in range(12))  # j = 2..13
CAP0 = 5  # r* of the cap images; copy i at CAP0 + 64 i

_LAUNCHED = {}  # configuration -> instantiations launched
_DEPTH = {256: 0, 512: 0}  # k_sample_screen width -> most candidates re-scored in a non-overflow probe
_MIX = {d: set() for d in DIMS}  # dim -> {"overflow", "plain"}
_STAT = {"worst": 0.0, "rows": 0, "same": 0, "use": 0.0, "aligned": (np.inf, 0.0), "cand": 0}
_DONE = set()


def _spec(dim, vocab=VOCAB, quant=False):
    h, kv = HEADS[dim]
    return binfmt.ModelSpec(dim, 512, 1, h, kv, vocab, 256, False, binfmt.FAMILY_LLAMA, quant, 64,
                            binfmt.ROPE_INTERLEAVED, 10000.0, EPS, f"scr-{dim}")


def _need(wg, vocab=VOCAB):
    wpw = wg // 64
    return ((vocab + 1) // 2 + wpw - 1) // wpw


def _maxv(dim, wg):
    for v in (1, 2, 4, 6):
        if dim <= v * 4 * wg:
            return v
    return 0


def _screen_u(dim):
    return 4 if (dim // 8 + 63) // 64 >= 3 else 2


def _cls_u(dim):
    per_lane = (dim // 4 + 63) // 64
    return 8 if per_lane >= 8 else (4 if per_lane >= 3 else 2)


def _probes(dim, rng):
    x = rng.normal(0.0, 1.0, dim).astype(F32)
    out = [x.copy()]
    y = x.copy()
    y[::61] *= 50.0
    out.append(y)
    out.append((x * F32(1e-18)).astype(F32))
    out.append(np.zeros(dim, F32))
    z = np.zeros(dim, F32)
    z[dim // 3] = F32(-2.5)
    out.append(z)
    return out


class _Base:
    """What the two norm scales of one dim share: the seeded image, and the references of its random classifier
    rows (the images below change a few dozen rows of it; only those are computed again)."""

    def __init__(self, dim, vocab):
        self.spec = _spec(dim, vocab)
        self.img = binfmt.synth_image(self.spec, seed=dim).numpy().copy()
        self.ents = {e.name: e for e in binfmt.layout(self.spec)[0]}
        W = self.view(self.img, "wcls")
        self.bits = R.bf16_bits(W)
        self.e_twin = R.cls_err(W)[1]
        self.e64 = R.err_exact64(W)
        self.nb = R.bf16_row_norms(W)
        self.dot = R.LaneDot(R.bf16_rne(W), 8)
        self.W64 = W.astype(np.float64)

    def view(self, img, name):
        e = self.ents[name]
        return img[e.offset: e.offset + e.nbytes].view(F32).reshape(e.shape)


class _Images:
    """The host images of one (dim, norm scale), their device copies, and the references per (image, probe)."""

    def __init__(self, base, dim, scale, device, vocab=VOCAB):
        self.base, self.dim, self.scale, self.vocab = base, dim, scale, vocab
        self.spec = base.spec
        rng = np.random.default_rng(1000 * dim + int(scale * 100))
        self.wn = (rng.normal(0.0, 1.0, dim) * scale).astype(F32)
        self.probes = _probes(dim, rng)
        g0 = (self.wn * self.probes[0]).astype(F32)
        rstar = R.bf16_rne((F32(0.02) * g0).astype(F32))
        self.host, self.W, self.rows = {}, {}, {}
        kinds = ("special",) if vocab != VOCAB else ("special", "spill", "crowd", "cap32", "cap33")
        for kind in kinds:
            img = base.img.copy()
            base.view(img, "final_norm")[:] = self.wn
            W = base.view(img, "wcls")
            new = {}  # row -> weights
            if vocab != VOCAB:
                new[3] = np.zeros(dim, F32)
            elif kind == "special":
                sp = _special_rows(dim, rng, n_random=0)
                for i, row in enumerate(sp):
                    new[SPECIAL0 + SPECIAL_STRIDE * i] = row
                for r, e, v in ((NAN_ROW, dim // 5, np.nan), (INF_ROW, 3, -np.inf)):
                    new[r] = W[r].copy()
                    new[r][e] = v
                new[BIG_ROW] = np.zeros(dim, F32)
                new[BIG_ROW][dim // 2] = F32(3.4e38)
                for r, k in ALIGNED.items():
                    wh = R.bf16_rne((F32(k) * g0).astype(F32))
                    new[r] = (wh * F32(1.0 + 0.9 * 2.0 ** -9)).astype(F32)
            elif kind in ("spill", "crowd"):
                new[RSTAR] = rstar
                for j, r in enumerate(SPILL_ROWS if kind == "spill" else CROWD_ROWS, start=2):
                    new[r] = (rstar * F32(1.0 - j * 2.0 ** -13)).astype(F32)
            else:
                new[CAP0] = rstar
                big = np.argsort(-np.abs(rstar))
                for i in range(1, 32 if kind == "cap32" else 33):
                    c = rstar.copy()
                    e = int(big[i])
                    c[e] = np.nextafter(c[e], F32(np.inf) if i % 2 else F32(-np.inf))
                    new[CAP0 + 64 * i] = c
            self.rows[kind] = np.array(sorted(new))
            for r, w in new.items():
                W[r] = w
            self.host[kind] = img
            self.W[kind] = W
        self.dev = {k: torch.from_numpy(v).to(device) for k, v in self.host.items()}
        self._pref, self._ref, self._copy = {}, {}, {}

    def nonfinite_rows(self, kind):
        if kind != "special" or self.vocab != VOCAB:
            return []
        return [NAN_ROW, INF_ROW, BIG_ROW]

    def copy_ref(self, kind):
        """(bf16 bits, twin's e[], fp64 e without the safety factor, |bf16 w|) of an image's classifier."""
        if kind not in self._copy:
            rows = self.rows[kind]
            Wr = self.W[kind][rows]
            out = []
            for full, part in ((self.base.bits, R.bf16_bits(Wr)), (self.base.e_twin, R.cls_err(Wr)[1]),
                               (self.base.e64, R.err_exact64(Wr)), (self.base.nb, R.bf16_row_norms(Wr))):
                full = full.copy()
                full[rows] = part
                out.append(full)
            self._copy[kind] = tuple(out)
        return self._copy[kind]

    def ref(self, kind, pi, wg):
        """Twin intervals at screen width wg, the tolerance tau, the fp64 gold: computed once per (image, probe)."""
        x = self.probes[pi]
        if pi not in self._pref:  # the random rows: shared by the images
            g = (self.wn * x).astype(F32)
            x64 = x.astype(np.float64)
            with np.errstate(all="ignore"):
                gold = (self.base.W64 @ (self.wn.astype(np.float64) * x64)) / np.sqrt((x64 * x64).mean() + float(F32(EPS)))
            self._pref[pi] = (g, self.base.dot.dot(g), gold)
        g, sum0, gold0 = self._pref[pi]
        key = (kind, pi)
        if key not in self._ref:
            rows = self.rows[kind]
            Wr = self.W[kind][rows]
            s, gold = sum0.copy(), gold0.copy()
            s[rows] = R.lane_dot(R.bf16_rne(Wr), g, 8)
            gold[rows] = R.gold_logits64(Wr, x, self.wn, F32(EPS))
            self._ref[key] = {"sum": s, "gold": gold, "g": g, "wg": {}}
        ref = self._ref[key]
        if wg not in ref["wg"]:
            _, rs, cb = R.stage(x, self.wn, EPS, wg)
            _, e, _, nb = self.copy_ref(kind)
            a, b, lb, ub = R.interval(ref["sum"], e, rs, cb)
            ref["wg"][wg] = {"a": a, "b": b, "lb": lb, "ub": ub, "rs": rs,
                             "tau": R.twin_tolerance(nb, self.dim, g, rs, b)}
        return ref, ref["wg"][wg]

    def twin_logits(self, kind, pi, wg, rows):
        """k_cls's logits of a few rows on the twin (the fp32 order of a 4-weight load per lane)."""
        ref, rw = self.ref(kind, pi, wg)
        with np.errstate(all="ignore"):
            return (R.lane_dot(self.W[kind][rows], ref["g"], 4) * rw["rs"]).astype(F32)


_CACHE = {}


def _images(dim, scale, device, vocab=VOCAB):
    if ("base", dim, vocab) not in _CACHE:
        _CACHE.clear()  # one dim at a time: the images of dim 4224 are 100 MB each
        _CACHE["base", dim, vocab] = _Base(dim, vocab)
    if ("images", scale) not in _CACHE:
        for k in [k for k in _CACHE if k[0] == "images"]:
            del _CACHE[k]
        _CACHE["images", scale] = _Images(_CACHE["base", dim, vocab], dim, scale, device, vocab)
    return _CACHE["images", scale]


class _Hooks:
    """Hooks of one configuration, set for the creation and kept while its model lives."""

    def __init__(self, screen=None, cls=None, extra=None):
        self.h = {"KH_SHAPE_SCREEN": screen, "KH_SHAPE_CLS": cls, "KH_CLS_SCREEN": "force" if cls else None}
        self.h.update(extra or {})

    def __enter__(self):
        for k, v in self.h.items():
            _ffi.debug_set(k, v)

    def __exit__(self, *exc):
        for k in self.h:
            _ffi.debug_set(k, None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)


def _create(ims, kind, flags=0):
    from kuiperllama_amd.model import KuiperModel
    m = KuiperModel.from_device_image(ims.dev[kind], ims.spec, flags=flags)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")  # after creation: the self-test's launches are not checked launches
    return m


def _close(m, name):
    _LAUNCHED.setdefault(name, set()).update(k for k in _ffi.launch_log() if k.split("<")[0] in STEMS)
    _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


def _lowest_argmax(lg):
    return int(np.argmax(np.where(np.isnan(lg), -np.inf, lg)))


def _inside(v, lb, ub):
    """v inside [lb, ub] where v is a number; (-inf, +inf) where it is NaN."""
    nan = np.isnan(v)
    with np.errstate(all="ignore"):
        return np.where(nan, (lb == -np.inf) & (ub == np.inf), (lb <= v) & (v <= ub))


def _check_copy(m, ims, kind, what):
    bits, e_twin, e64, _ = ims.copy_ref(kind)
    wbf, err = m.cls_screen_read()
    assert np.array_equal(wbf, bits), f"{what}: bf16 copy differs in {int((wbf != bits).sum())} weights"
    fin = np.isfinite(e64)
    assert np.all(err[~fin] == np.inf), f"{what}: non-finite rows must carry err = +inf"
    assert np.all(err[fin].astype(np.float64) >= e64[fin]), \
        f"{what}: err below the fp64 bound in rows {np.flatnonzero(fin & (err.astype(np.float64) < e64))[:5]}"
    lo, hi = np.nextafter(e_twin, F32(-np.inf)), np.nextafter(e_twin, F32(np.inf))
    off = np.flatnonzero(fin & ~((lo <= err) & (err <= hi)))
    assert off.size == 0, f"{what}: err more than one ulp from the twin's in rows {off[:5]}: {err[off[:5]]} vs {e_twin[off[:5]]}"


def _probe(m, ims, kind, pi, swg, cwg, what):
    """One probe vector on model m (k_cls_screen at width swg, k_sample_screen at cwg): checks 3, 4 and 6."""
    what = f"{what} {kind} probe {pi}"
    r = m.cls_screen_probe(ims.probes[pi])
    lg = m.logits()
    lb, ub = r["lb"], r["ub"]
    ref, rw = ims.ref(kind, pi, swg)
    # soundness, no tolerance
    bad = np.flatnonzero(~_inside(lg, lb, ub))
    assert bad.size == 0, f"{what}: k_cls logit outside its interval, rows {bad[:5]}: {lg[bad[:5]]} not in " \
                          f"[{lb[bad[:5]]}, {ub[bad[:5]]}] ({bad.size} rows)"
    gold = ref["gold"]
    bad = np.flatnonzero(~_inside(gold, lb.astype(np.float64), ub.astype(np.float64)))
    assert bad.size == 0, f"{what}: fp64 gold outside its interval, rows {bad[:5]}: {gold[bad[:5]]} not in " \
                          f"[{lb[bad[:5]]}, {ub[bad[:5]]}] ({bad.size} rows)"
    for row in ims.nonfinite_rows(kind):
        assert lb[row] == -np.inf and ub[row] == np.inf, f"{what}: non-finite row {row} has [{lb[row]}, {ub[row]}]"
    # tightness against the twin
    tfin = np.isfinite(rw["lb"]) & np.isfinite(rw["ub"])
    assert np.array_equal(np.isfinite(lb) & np.isfinite(ub), tfin), f"{what}: finite intervals differ from the twin's"
    with np.errstate(all="ignore"):
        d = np.maximum(np.abs(lb.astype(np.float64) - rw["lb"]), np.abs(ub.astype(np.float64) - rw["ub"]))[tfin]
        ratio = np.where(d == 0, 0.0, d / rw["tau"][tfin])
    worst = float(ratio.max()) if ratio.size else 0.0
    _STAT["worst"] = max(_STAT["worst"], worst)
    _STAT["rows"] += int(tfin.sum())
    _STAT["same"] += int(((lb == rw["lb"]) & (ub == rw["ub"]))[tfin].sum())
    assert worst <= 1.0, f"{what}: lb / ub {worst:.3f} tau from the twin's (row {int(np.flatnonzero(tfin)[ratio.argmax()])})"
    # use of the half-width on the GPU: |logit - a| / b over all rows (the gate at the end reports the largest)
    fin = np.isfinite(lb) & np.isfinite(ub) & np.isfinite(lg)
    with np.errstate(all="ignore"):
        a64, b64 = (lb.astype(np.float64) + ub) / 2, (ub.astype(np.float64) - lb) / 2
        use = np.abs(lg - a64)[fin] / b64[fin]
    use = use[np.isfinite(use)]
    if use.size:
        _STAT["use"] = max(_STAT["use"], float(use.max()))
    # tokens
    want = _lowest_argmax(lg)
    assert r["token"] == r["full_token"] == want, \
        f"{what}: screened {r['token']}, full classifier {r['full_token']}, argmax of the logits {want}"
    if ims.vocab == VOCAB:
        _MIX[ims.dim].add("overflow" if r["overflow"] else "plain")
    if not r["overflow"]:
        _DEPTH[cwg] = max(_DEPTH[cwg], r["candidates"])
        _STAT["cand"] = max(_STAT["cand"], r["candidates"])
        with np.errstate(all="ignore"):
            n = int((ub >= lb.max()).sum())
        assert r["candidates"] == n, f"{what}: {r['candidates']} rows re-scored, {n} rows reach the best lower bound"
    r["logits"] = lg
    return r


def _check_special(m, ims, swg, cwg, what):
    """Checks 1 - 6 on the special image: copy, err, and every probe vector; the aligned rows use their bound."""
    info = m.cls_screen_info()
    assert info["on"] == 1 and info["selftest"] == 1, f"{what}: {info}"
    _check_copy(m, ims, "special", what)
    out = []
    for pi in range(len(ims.probes)):
        r = _probe(m, ims, "special", pi, swg, cwg, what)
        out.append(r)
        if pi == 3:
            assert r["token"] == 0 and r["overflow"] == 1, f"{what}: all-zeros vector: {r['token']}, {r['overflow']}"
    after = m.cls_screen_info()
    assert {k: after[k] for k in ("steps", "candidates", "overflow_steps")} == \
        {k: info[k] for k in ("steps", "candidates", "overflow_steps")}, f"{what}: the probe moved the user's counters"
    if ims.vocab == VOCAB:
        rows = np.array(sorted(ALIGNED))
        _, rw = ims.ref("special", 0, swg)
        tl = ims.twin_logits("special", 0, swg, rows)
        use = np.abs(tl.astype(np.float64) - rw["a"][rows]) / rw["b"][rows]
        assert np.all(use >= 0.95), f"{what}: the aligned rows use only {use} of b on the twin (condition on the inputs)"
        gl = out[0]["logits"][rows].astype(np.float64)
        guse = np.abs(gl - (out[0]["lb"][rows].astype(np.float64) + out[0]["ub"][rows]) / 2) / \
            ((out[0]["ub"][rows].astype(np.float64) - out[0]["lb"][rows]) / 2)
        _STAT["aligned"] = (min(_STAT["aligned"][0], float(guse.min())), max(_STAT["aligned"][1], float(guse.max())))
        print(f"{what}: aligned rows use {use.min():.4f}..{use.max():.4f} of b on the twin, "
              f"{guse.min():.4f}..{guse.max():.4f} on the GPU")
    return out


def _check_construction(m, ims, kind, swg, cwg, what, expect_overflow=None):
    """Spill / crowd / cap image on the unit probe: conditions on the twin, token, candidate count."""
    info = m.cls_screen_info()
    assert info["on"] == 1 and info["selftest"] == 1, f"{what}: {info}"
    ref, rw = ims.ref(kind, 0, swg)
    with np.errstate(all="ignore"):
        cand = np.flatnonzero(rw["ub"] >= rw["lb"].max())
    star = CAP0 if kind.startswith("cap") else RSTAR
    others = {"spill": SPILL_ROWS, "crowd": CROWD_ROWS}.get(kind)
    if others:
        assert sorted(cand) == sorted((star,) + tuple(others)), f"{what}: twin candidates {cand}"
        assert np.all(rw["ub"][list(others[:6])] > rw["ub"][star]), f"{what}: the rows do not outrank r* by upper bound"
        assert int(np.argmax(ref["gold"])) == star
    else:
        n = 32 if kind == "cap32" else 33
        assert cand.size == n and cand[0] == star, f"{what}: twin candidates {cand}"
    r = _probe(m, ims, kind, 0, swg, cwg, what)
    if others:
        assert r["token"] == star, f"{what}: token {r['token']}, r* is row {star}"
    if expect_overflow is not None:
        assert r["overflow"] == int(expect_overflow), f"{what}: overflow {r['overflow']}, {r['candidates']} candidates"
    if not r["overflow"]:
        assert r["candidates"] == cand.size, f"{what}: {r['candidates']} candidates, twin {cand.size}"
    return r


def _run(m, exec):
    words, _ = m.generate(PROMPT, STEPS, exec=exec)
    return words, m.logits()


def _check_generate(m, what, on_value):
    """Check 10: graph and fused generate, screened, against the same run under KH_CLS_SCREEN=0."""
    res = {}
    try:
        for mode in ("graph", "fused"):
            _ffi.debug_set("KH_CLS_SCREEN", on_value)
            i0 = m.cls_screen_info()
            a = _run(m, mode)
            i1 = m.cls_screen_info()
            _ffi.debug_set("KH_CLS_SCREEN", "0")
            b = _run(m, mode)
            i2 = m.cls_screen_info()
            assert i1["steps"] - i0["steps"] >= STEPS - len(PROMPT), f"{what} {mode}: {i1['steps'] - i0['steps']} screened steps"
            assert i2["steps"] == i1["steps"], f"{what} {mode}: KH_CLS_SCREEN=0 still ran screened steps"
            assert a[0] == b[0], f"{what} {mode}: words differ: {a[0]} vs {b[0]}"
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what} {mode}: logits() differ"
            res[mode] = a
    finally:
        _ffi.debug_set("KH_CLS_SCREEN", on_value)
    assert res["graph"][0] == res["fused"][0], f"{what}: graph {res['graph'][0]} vs fused {res['fused'][0]}"
    assert np.array_equal(res["graph"][1].view(np.uint32), res["fused"][1].view(np.uint32))


def _expect_log(name, dim, su, swg, cu, cwg):
    got = _LAUNCHED[name]
    want = {f"k_cls_screen<{su},{_maxv(dim, swg)}>", f"k_sample_screen<{cu},{_maxv(dim, cwg)}>"}
    assert got == want, f"{name}: launched {sorted(got)}, expected {sorted(want)}"


# ---- the planned launch: every image, the grids, generate --------------------------------------------------------
def _planned_launch(ims, dim, scale):
    su, cu, need = _screen_u(dim), _cls_u(dim), _need(512)
    name = f"planned-{dim}-{scale}"
    with _Hooks():
        m = _create(ims, "special")
        try:
            _check_special(m, ims, 512, 512, name)
        finally:
            _close(m, name)
        planned = {}
        for kind, over in (("spill", False), ("crowd", False), ("cap32", False), ("cap33", True)):
            m = _create(ims, kind)
            try:
                _check_copy(m, ims, kind, f"{name} {kind}")
                planned[kind] = _check_construction(m, ims, kind, 512, 512, name, expect_overflow=over)
                if kind == "spill":
                    assert planned[kind]["candidates"] == 7
                    _check_generate(m, name, None)
            finally:
                _close(m, name)
    _expect_log(name, dim, su, 512, cu, 512)
    # grids: the intervals do not depend on the grid; one workgroup must spill r* and overflow
    for grid in (1, 3, need, 4096):
        with _Hooks(screen=f"{su},{grid},512"):
            m = _create(ims, "spill")
            try:
                r = _check_construction(m, ims, "spill", 512, 512, f"{name} grid {grid}",
                                        expect_overflow=True if grid == 1 else None)
                assert r["token"] == planned["spill"]["token"]
                assert np.array_equal(r["lb"].view(np.uint32), planned["spill"]["lb"].view(np.uint32)) and \
                    np.array_equal(r["ub"].view(np.uint32), planned["spill"]["ub"].view(np.uint32)), \
                    f"{name}: the intervals depend on the grid ({grid})"
                if not r["overflow"]:
                    assert r["candidates"] == 7
            finally:
                _close(m, name)
    _expect_log(name, dim, su, 512, cu, 512)


# ---- every k_cls_screen cell: KH_SHAPE_SCREEN (u, wg) --------------------------------------------------------------
def _screen_cells(ims, dim, scale):
    cu = _cls_u(dim)
    for wg in (256, 512):
        if not 1 <= _maxv(dim, wg) <= 4:
            continue  # (refused: test_refused_hooks)
        for u in (2, 4):
            name = f"screen-{dim}-{scale}-u{u}-wg{wg}"
            with _Hooks(screen=f"{u},{_need(wg)},{wg}"):
                m = _create(ims, "special")
                try:
                    _check_special(m, ims, wg, 512, name)
                finally:
                    _close(m, name)
                for kind, over in (("spill", False), ("crowd", False), ("cap32", False), ("cap33", True)):
                    m = _create(ims, kind)
                    try:
                        r = _check_construction(m, ims, kind, wg, 512, name, expect_overflow=over)
                        if kind == "spill":
                            assert r["candidates"] == 7
                            _check_generate(m, name, None)  # this cell captured in a graph and in the fused loop
                    finally:
                        _close(m, name)
            with _Hooks(screen=f"{u},1,{wg}"):
                m = _create(ims, "spill")
                try:
                    _check_construction(m, ims, "spill", wg, 512, f"{name} grid 1", expect_overflow=True)
                finally:
                    _close(m, name)
            _expect_log(name, dim, u, wg, cu, 512)


# ---- every k_sample_screen cell the heuristic does not reach: KH_SHAPE_CLS + KH_CLS_SCREEN=force ------------------
FORCED = {1152: ((8, 512), (2, 256), (4, 256)), 2304: ((2, 256), (4, 256))}


def _forced_classifier_cells(ims, dim, scale):
    su = _screen_u(dim)
    for u, wg in FORCED.get(dim, ()):
        name = f"forced-{dim}-{scale}-u{u}-wg{wg}"
        with _Hooks(cls=f"1,{u},{_need(wg)},{wg}"):
            m = _create(ims, "special")
            try:
                _check_special(m, ims, wg, wg, name)
            finally:
                _close(m, name)
            for kind, over in (("spill", False), ("crowd", False), ("cap32", False), ("cap33", True)):
                m = _create(ims, kind)
                try:
                    r = _check_construction(m, ims, kind, wg, wg, name, expect_overflow=over)
                    if kind == "spill":
                        assert r["candidates"] == 7
                        # the re-scored values are k_cls's at the same forced shape: tokens and logits, bit for bit
                        _check_generate(m, name, "force")
                finally:
                    _close(m, name)
        _expect_log(name, dim, su, wg, u, wg)


# ---- one workgroup in both kernels ----------------------------------------------------------------------------------
def test_tiny_vocabulary_one_workgroup(gpu):
    ims = _images(448, 4.0, gpu, vocab=7)
    with _Hooks():
        m = _create(ims, "special")
        try:
            _check_special(m, ims, 512, 512, "tiny")
            words, _ = m.generate([1, 3], 12)
            _ffi.debug_set("KH_CLS_SCREEN", "0")
            assert m.generate([1, 3], 12)[0] == words
        finally:
            _close(m, "tiny")
    _expect_log("tiny", 448, 2, 512, 2, 512)
    _DONE.add("tiny")


# ---- refused hooks launch the planned shape, and say so -------------------------------------------------------------
REFUSED = {448: ("8,188,512", "2,188,384"), 4224: ("4,376,256",)}


def _refused_hooks(ims, dim, capfd):
    for hook in REFUSED.get(dim, ()):
        name = f"refused-{dim}-{hook}"
        capfd.readouterr()
        with _Hooks(screen=hook):
            m = _create(ims, "spill")
            try:
                err = capfd.readouterr().err
                assert f'KH_SHAPE_SCREEN="{hook}" rejected' in err, err
                r = _check_construction(m, ims, "spill", 512, 512, name, expect_overflow=False)
                assert r["candidates"] == 7
            finally:
                _close(m, name)
        _expect_log(name, dim, _screen_u(dim), 512, _cls_u(dim), 512)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dim", DIMS)
def test_configurations(gpu, capfd, dim, scale):
    """Every configuration of one (dim, norm scale): the planned launch with all images, the grids and generate; the
    KH_SHAPE_SCREEN cells; the KH_SHAPE_CLS + force cells; the refused hooks (module docstring)."""
    ims = _images(dim, scale, gpu)
    _planned_launch(ims, dim, scale)
    _screen_cells(ims, dim, scale)
    _forced_classifier_cells(ims, dim, scale)
    if scale == SCALES[-1]:
        _refused_hooks(ims, dim, capfd)
    _DONE.add((dim, scale))


# ---- the silent "screening not applicable" cases ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dim4224-cls256", "dim252", "int8"])
def test_not_applicable_reports_off_and_decodes_the_same(gpu, case):
    from kuiperllama_amd.model import KuiperModel
    hooks = _Hooks()
    if case == "dim4224-cls256":  # 24 floats per staging thread: the staging depth is outside 1..4
        spec = _spec(4224)
        hooks = _Hooks(cls=f"1,4,{_need(256)},256")
    elif case == "dim252":        # dim % 8 == 4: a bf16 row would lose its 16-byte alignment
        spec = _spec(252)
    else:
        spec = _spec(448, vocab=1001, quant=True)
    img = binfmt.synth_image(spec, seed=9, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    res = []
    with hooks:
        for flags in (0, _ffi.KH_FLAG_NO_CLS_SCREEN):
            m = KuiperModel.from_device_image(img, spec, flags=flags)
            try:
                info = m.cls_screen_info()
                assert info["on"] == 0 and info["bytes"] == 0, f"{case}: {info}"
                _ffi.debug_set("KH_LAUNCH_LOG", "1")
                res.append(_run(m, "graph"))
                assert not {k for k in _ffi.launch_log() if k.split("<")[0] in STEMS}
                assert m.cls_screen_info()["steps"] == 0
                with pytest.raises(_ffi.KhError):
                    m.cls_screen_probe(np.zeros(spec.dim, F32))
            finally:
                _ffi.debug_set("KH_LAUNCH_LOG", None)
                m.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))


# ---- gates -------------------------------------------------------------------------------------------------------------
def _whole_module():
    want = {(d, s) for d in DIMS for s in SCALES} | {"tiny"}
    missing = sorted(map(str, want - _DONE))
    assert not missing, f"tests that did not run to the end (run the whole module): {missing}"


@pytest.fixture(scope="module")
def compiled():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    return co.instantiations(co.code_object_notes(_ffi.LIB_PATH), set(STEMS))


@pytest.mark.parametrize("stem", STEMS)
def test_coverage_gate(gpu, compiled, stem):
    """Every compiled instantiation of the template was launched (and checked) by the tests above."""
    _whole_module()
    comp = {k for k in compiled if k.split("<")[0] == stem}
    seen = {k for s in _LAUNCHED.values() for k in s if k.split("<")[0] == stem}
    assert comp, f"no {stem} instantiation in the library"
    assert seen <= comp, f"launched but not found in the code objects: {sorted(seen - comp)}"
    print(f"{stem}: {len(seen)} of {len(comp)} compiled instantiations launched and checked")
    assert not comp - seen, f"{stem}: compiled and never launched: {sorted(comp - seen)}"


def test_rescore_depth_and_overflow_mix_gate(gpu):
    """The re-score loop ran its second iteration at both widths (more candidates than waves in a step that did not
    overflow); overflow and plain steps occurred at every dim."""
    _whole_module()
    assert _DEPTH[512] > 8 and _DEPTH[256] > 4, _DEPTH
    for d in DIMS:
        assert _MIX[d] == {"overflow", "plain"}, f"dim {d}: {_MIX[d]}"
    # soundness again, over every row of every probe: no logit used more than its half-width
    assert 0.0 < _STAT["use"] <= 1.0, _STAT
    print(f"worst |lb/ub - twin| / tau {_STAT['worst']:.4f}; {_STAT['same']} of {_STAT['rows']} rows bit-identical to "
          f"the twin ({100.0 * _STAT['same'] / max(1, _STAT['rows']):.2f} %); largest use of b on the GPU "
          f"{_STAT['use']:.4f} (aligned rows {_STAT['aligned'][0]:.4f}..{_STAT['aligned'][1]:.4f}); most candidates without overflow {_STAT['cand']}; re-score depth {_DEPTH}")
