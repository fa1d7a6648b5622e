"""Every GEMM-prefill kernel instantiation the library compiles, launched and checked against an fp64 gold.

kh_model_prefill_gemm (the default prompt path of generate() from 16 fed-only tokens on) picks, per GEMM, one of
k_pg_gemm<QUANT, R, NT, EPI> (tiles (2,8) (2,4) (2,2) (1,4); QKV, residual and SwiGLU epilogues) from the cost
model of pg_shape, runs attention on k_pg_attn<HB, NW, QT> (head sizes 48 / 64 / 128; 1, 2 or 4 query tiles) or on
the decode kernel (other head sizes, KH_PG_ATTN=0), and k_pg_rmsnorm<QUANT> / k_pg_rope between them.  The heuristic
shapes of the model geometries elsewhere in the suite reach only some of them.  Here nine seeded 2-layer geometries
(a small odd vocabulary, 2613 cache rows) run under forced shapes - hooks KH_PG_SHAPE_<QKV|RESID|SWIGLU> =
"R,NT,ks[,kz]" walking every tile the hook accepts with ks 1 / 2 / 4 / 8 and kz 1 / 2 / 4 - and under
KH_PG_SOLO=0, KH_PG_ROPE_FUSE=0, KH_PG_CHUNK=100, KH_PG_ATTN_QT=1/2/4 and KH_PG_ATTN=0:

  fp32 hs 64 GQA, half RoPE (16 heads)  paired-tile RoPE; at start position 2085 QT = 2 is picked by itself
  fp32 hs 128 MHA, interleaved           k_pg_attn<8,4,*>, RoPE pairs in the epilogue, k_pg_rope interleaved
  fp32 hs 48, dim 336, hidden 912       HB = 3; no 32-row tile fits any GEMM; k_pg_rope half mode; odd K blocks
  fp32 Qwen2 bias, hs 80                fallback attention (also at 2085: the pg_ws workspace at 512 tokens);
                                        the wo GEMM reads a row-major slab
  fp32 hs 96, half RoPE                 paired tiles 48 rows apart, three workgroups per head; fallback attention
  int8 g64, hs 64 / hs 128              every int8 tile through the hooks, R = 1 included; KH_PG_ATTN=0 (row-major B)
  int8 g64, hs 48, one KV head          the QKV GEMM takes R = 1 by itself (kv_dim 48)
  int8 g128                             not a GEMM-prefill model: prefill_gemm refuses it, generate() takes the
                                        B-token prefill (its words equal the token-by-token run's)

The int8 R = 1 residual and SwiGLU kernels, k_pg_gemm<true,1,4,1> and k_pg_gemm<true,1,4,2>, are reached through the
hooks only (the heuristic takes the 32-row tile wherever it fits, and it fits every int8 dim / hidden).

Per geometry the gold is computed once per scenario, OracleModel.forward(..., ACC_F64) teacher-forced; it does not
depend on the launch shape, so every shape reuses it:
  * shallow: prefill_gemm(toks[:37], 0), then prefill_gemm(toks[37:337], 37) (a start that is not a multiple of 16,
    three 128-token slab strides), then predict at 337;
  * deep (two geometries, MFMA and fallback attention): random K/V rows below 2085 in the model and the gold, a
    512-token prefill at 2085, predict at 2597, then a 16-token prefill that ends at the last cache row.
Per run:
  * the rows a call writes hold NaN before it; after it, the K/V rows of every layer are within
    max(KV floor + e32, 3 x e32) of the gold, e32 = |oracle fp32 - gold| of those rows (floor: the suite's
    GEMM-prefill bound against the oracle's fp32, int8 4x - carried over to the gold by the triangle inequality;
    4x that in the deep scenario, KV_ATOL_DEEP);
  * the rows below the call's start and the 8 rows past its end are bit-for-bit what they held before;
  * the next step's logits are within max(floor + e32, 3 x e32) (floor: the suite's fp32 / int8 logit
    tolerance), its argmax equal to the gold's wherever the gold's top-2 margin exceeds 2 x floor;
  * pairs that change nothing in the arithmetic are bit-identical: KH_PG_SOLO=0 at a forced shape (only the LDS
    request changes), KH_PG_ROPE_FUSE=0 (k_pg_rope evaluates the epilogue's rotation expression on the same stored
    GEMM output; the library is built with -ffp-contract=off, so neither side contracts it into an FMA) and a
    rejected shape hook (the heuristic shape runs).  Shapes that differ in ks, kz, the chunking or the query tiles
    change the order of sums and are held to the tolerances above;
  * hook KH_PG_DEBUG: the `[pg] ... -> R NT slices ks kz` line of every GEMM shows the shape that ran - a forced
    shape must be the one launched, and no `rejected` line may appear except where a test provokes one.
While the runs go, the launch log (hook KH_LAUNCH_LOG) records the instantiations launched.  The gates at the end
compare it with the instantiations compiled into the library (read from its code objects), and check that the runs
reached every variant inside the kernels: each RoPE path, kz 1 / 2 / 4, solo on and off, tiled and row-major B for
fp32 and int8, the ring and the phase K loop of every fp32 tile (each wave's K range computed as k_pg_gemm does),
waves with an empty K range, and QT > 1 writing both tiled slabs.
"""
import re

import numpy as np
import pytest
import torch

import code_objects as co
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

LOGIT_ATOL_F32 = 2e-5  # test_model_gpu.py: LOGIT_ATOL_F32 / LOGIT_ATOL_Q8
LOGIT_ATOL_Q8 = 5e-5
KV_ATOL_GEMM = 5e-6    # test_model_gpu.py: KV_ATOL_GEMM (int8: 4x)
# K/V rows written at start position 2085 over random unit-variance cache rows: the second layer's rows carry the
# error of 2600-term softmax sums (hardware exp2, log2-domain scores) - four times the shallow bound; measured on an
# MI355X: at most 1.63e-5 (fallback attention) and 1.05e-5 (MFMA attention), 3 to 5 x |oracle fp32 - gold|
KV_ATOL_DEEP = 2e-5
CACHE = 2613
SHALLOW = (0, 37, 337)             # two calls: [0, 37), [37, 337); the next step at 337
DEEP = (2085, 2597, CACHE)         # random rows below 2085; [2085, 2597), next step at 2597; [2597, CACHE)
PAST = 8                           # rows past a call's end that must keep their bits
RING_D16 = 2                       # kh_gemm.h: KH_PG_RING_D16, the ring depth of the (2,8) tile

L, Q2 = binfmt.FAMILY_LLAMA, binfmt.FAMILY_QWEN2
HALF, INTER = binfmt.ROPE_HALF, binfmt.ROPE_INTERLEAVED


def _spec(dim, hidden, heads, kv_heads, vocab, quant, group, rope, family, name):
    theta = 1000000.0 if family == Q2 else 10000.0
    return binfmt.ModelSpec(dim, hidden, 2, heads, kv_heads, vocab, CACHE, False, family, quant, group, rope, theta,
                            1e-6 if family == Q2 else 1e-5, name)


GEOMETRIES = {  # name -> (spec, runs the deep scenario)
    "f32-hs64-gqa-half": (_spec(1024, 2816, 16, 4, 1001, False, 64, HALF, L, "pg-f32-hs64"), True),
    "f32-hs128-mha-inter": (_spec(1024, 1536, 8, 8, 777, False, 64, INTER, L, "pg-f32-hs128"), False),
    "f32-hs48-d336": (_spec(336, 912, 7, 1, 999, False, 64, HALF, L, "pg-f32-hs48"), False),
    "f32-qwen-hs80": (_spec(960, 1600, 12, 2, 1537, False, 64, HALF, Q2, "pg-f32-qwen-hs80"), True),
    "f32-hs96-half": (_spec(768, 2080, 8, 2, 1003, False, 64, HALF, L, "pg-f32-hs96"), False),
    "q8-hs64-inter": (_spec(1024, 2816, 16, 4, 1001, True, 64, INTER, L, "pg-q8-hs64"), False),
    "q8-hs128-half": (_spec(1024, 1536, 8, 2, 777, True, 64, HALF, L, "pg-q8-hs128"), False),
    "q8-hs48-kv48": (_spec(384, 1024, 8, 1, 999, True, 64, HALF, L, "pg-q8-hs48"), False),
}

STEMS = ("k_pg_gemm", "k_pg_attn", "k_pg_rmsnorm", "k_pg_rope")
# compiled instantiations no prefill can launch, with the reason (none at present)
UNREACHABLE = {}

_LAUNCHED = {}  # geometry -> instantiations its runs launched (filled by test_geometry, read by the gates)
_VARIANTS = {}  # geometry -> variants its runs reached

TILES = ((2, 8), (2, 4), (2, 2), (1, 4))
EPIS = ("QKV", "RESID", "SWIGLU")
_PG_LINE = re.compile(r"\[pg\] epi (\d) rows (\d+) K (\d+) T (\d+) -> R (\d) NT (\d) slices (\d+) ks (\d) kz (\d) "
                      r"\((\d+) wgs x (\d+) waves(, solo)?\)")


def _mfma_attn(spec):
    return spec.head_size in (48, 64, 128)


def _accepted_tiles(spec):
    """(R, NT) the KH_PG_SHAPE_* hook accepts per GEMM: the 32-row tiles only where 32 rows divide the matrices."""
    r2 = {"QKV": spec.dim % 32 == 0 and spec.kv_dim % 32 == 0, "RESID": spec.dim % 32 == 0,
          "SWIGLU": spec.hidden_dim % 32 == 0}
    return {e: [t for t in TILES if t[0] == 1 or r2[e]] for e in EPIS}


def _shapes(spec):
    """Forced shapes of one geometry: [{QKV: (R, NT, ks), RESID: (R, NT, ks, kz), SWIGLU: (R, NT, ks)}].  Each GEMM
    walks every accepted (R, NT) x ks (ks 1 / 2 / 4 / 8 within 512 threads: SwiGLU workgroups hold two matrices),
    the residual GEMMs with kz 1 / 2 / 4 in turn; a last shape splits the residual K over 32 waves (8 x 4)."""
    acc = _accepted_tiles(spec)
    ks_max = {"QKV": 8, "RESID": 8, "SWIGLU": 4}
    combos = {e: [(r, nt, ks) for r, nt in acc[e] for ks in (1, 2, 4, 8) if ks <= ks_max[e]] for e in EPIS}
    n = max(len(c) for c in combos.values())
    out = []
    for i in range(n):
        sh = {e: c[i % len(c)] for e, c in combos.items()}
        sh["RESID"] = sh["RESID"] + ((1, 2, 4)[i % 3],)
        out.append(sh)
    out.append({"RESID": acc["RESID"][-1] + (8, 4)})
    return out


def _set_hooks(hooks):
    for k in ("KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU", "KH_PG_SOLO", "KH_PG_ROPE_FUSE",
              "KH_PG_CHUNK", "KH_PG_ATTN_QT", "KH_PG_ATTN"):
        _ffi.debug_set(k, hooks.get(k))


def _shape_hooks(sh):
    return {f"KH_PG_SHAPE_{e}": ",".join(map(str, s)) for e, s in sh.items()}


# ---- gold --------------------------------------------------------------------------------------------------------
def _deep_rows(spec, rng):
    n = DEEP[0]
    kr = rng.standard_normal((spec.n_layers, n, spec.kv_dim), dtype=np.float32)
    vr = rng.standard_normal((spec.n_layers, n, spec.kv_dim), dtype=np.float32)
    kr[:, rng.integers(0, n, 8)] *= 6.0  # a few dominant keys
    return kr, vr


def _gold(oracle, img_h, spec, toks, first, last, logit_pos, rows=None):
    """fp64 gold and fp32 oracle fed toks[first .. last) at their positions (rows: K/V rows below `first`):
    {k64, v64, k32, v32: [L, last - first, kv] ; lg64, lg32: logits at logit_pos}."""
    out = {}
    for tag, acc in (("64", oracle.ACC_F64), ("32", oracle.ACC_F32)):
        om = oracle.OracleModel.from_spec(img_h, spec, cache_len=CACHE)
        if rows is not None:
            ko, vo = om.kv_cache()
            ko[:, :first] = rows[0]
            vo[:, :first] = rows[1]
        for p in range(first, last):
            lg = om.forward(toks[p], p, acc)
            if p == logit_pos:
                out["lg" + tag] = lg.copy()
        ko, vo = om.kv_cache()
        out["k" + tag] = ko[:, first:last].copy()
        out["v" + tag] = vo[:, first:last].copy()
        om.close()
    return out


# ---- one run -----------------------------------------------------------------------------------------------------
def _call(m, spec, toks, pos0, end, gold, gfirst, below, what, kv_floor):
    """prefill_gemm(toks[pos0:end], pos0) with NaN in the rows it writes and a sentinel in the PAST rows after them;
    checks the written rows against the gold (rows gfirst.. of its arrays), `below` ([(K, V)] per layer, rows
    [0, pos0)) and the sentinel bit for bit.  Returns [(K, V)] of the written rows per layer."""
    kv_floor *= 4 if spec.quant else 1
    n, n_past = end - pos0, min(PAST, CACHE - end)
    nan = np.full((n, spec.kv_dim), np.nan, np.float32)
    sent = np.arange(n_past * spec.kv_dim, dtype=np.float32).reshape(n_past, spec.kv_dim) * 0.125 - 3.0
    for layer in range(spec.n_layers):
        m.write_kv(layer, pos0, nan, nan)
        if n_past:
            m.write_kv(layer, end, sent, -sent)
    m.prefill_gemm(toks[pos0:end], pos0)
    out = []
    a, b = pos0 - gfirst, end - gfirst
    for layer in range(spec.n_layers):
        k, v = m.read_kv(layer, pos0, n)
        for name, got in (("K", k), ("V", v)):
            g64 = gold[name.lower() + "64"][layer, a:b]
            g32 = gold[name.lower() + "32"][layer, a:b]
            e32 = float(np.abs(g32 - g64).max())
            lim = max(kv_floor + e32, 3.0 * e32)
            e = np.abs(got - g64)
            assert np.all(e <= lim), \
                f"{what} [{pos0},{end}) layer {layer}: {name} rows off by {np.nanmax(e) if np.isfinite(e).any() else e}" \
                f" > {lim:.3e} ({int(np.isnan(got).sum())} NaN, first bad row {pos0 + int(np.argwhere(~(e <= lim))[0][0])})"
        if below is not None and pos0:
            kb, vb = m.read_kv(layer, 0, pos0)
            assert np.array_equal(kb, below[layer][0]) and np.array_equal(vb, below[layer][1]), \
                f"{what} [{pos0},{end}) layer {layer}: rows below the call changed"
        if n_past:
            kp, vp = m.read_kv(layer, end, n_past)
            assert np.array_equal(kp, sent) and np.array_equal(vp, -sent), \
                f"{what} [{pos0},{end}) layer {layer}: rows past the call changed"
        out.append((k, v))
    return out


def _next(m, tok, pos, gold, floor, what):
    nxt = m.predict(tok, pos, exec="fused")
    got = m.logits()
    lg, lo = gold["lg64"], gold["lg32"]
    err = float(np.abs(got - lg).max())
    e32 = float(np.abs(lo - lg).max())
    lim = max(floor + e32, 3.0 * e32)
    assert err <= lim, f"{what} pos {pos}: |logit - gold| {err:.3e} > {lim:.3e}"
    top2 = np.sort(lg)[-2:]
    if top2[1] - top2[0] > 2 * floor:
        assert nxt == int(np.argmax(lg)), f"{what} pos {pos}: argmax {nxt} vs gold {int(np.argmax(lg))}"
    return got


def _scenario(m, spec, toks, sc, floor, what):
    """The calls and the next step of one scenario; returns (K/V rows per call, logits) for bit-identity checks."""
    if sc["name"] == "shallow":
        p0, p1, p2 = SHALLOW
        g = sc["gold"]
        r1 = _call(m, spec, toks, p0, p1, g, 0, None, what, KV_ATOL_GEMM)
        r2 = _call(m, spec, toks, p1, p2, g, 0, r1, what, KV_ATOL_GEMM)
        return [r1, r2], _next(m, toks[p2], p2, g, floor, what)
    p0, p1, p2 = DEEP
    g = sc["gold"]
    below = [(sc["rows"][0][layer], sc["rows"][1][layer]) for layer in range(spec.n_layers)]
    r1 = _call(m, spec, toks, p0, p1, g, p0, below, what, KV_ATOL_DEEP)
    lg = _next(m, toks[p1], p1, g, floor, what)
    # a call that ends at the last cache row: its K/V rows (no next step)
    below2 = [(np.concatenate([b[0], r[0]]), np.concatenate([b[1], r[1]])) for b, r in zip(below, r1)]
    r2 = _call(m, spec, toks, p1, p2, g, p0, below2, what, KV_ATOL_DEEP)
    return [r1, r2], lg


# ---- what ran ----------------------------------------------------------------------------------------------------
def _pg_lines(err):
    return [tuple(int(x) for x in mt.groups()[:11]) + (mt.group(12) is not None,)
            for mt in (_PG_LINE.search(ln) for ln in err.splitlines()) if mt]


def _wave_ranges(nb, ks, kz):
    """[b1 - b0] of every wave of a k_pg_gemm launch (each K slice z of gridDim.z = kz, each wave kpart of ks)."""
    out = []
    for z in range(kz):
        z0, z1 = z * nb // kz, (z + 1) * nb // kz
        out += [(z0 + (kp + 1) * (z1 - z0) // ks) - (z0 + kp * (z1 - z0) // ks) for kp in range(ks)]
    return out


def _variants(spec, lines, hooks, launched):
    """Variants a run reached, from its [pg] lines, the geometry and the hooks it ran under."""
    q = "q8" if spec.quant else "f32"
    fused = hooks.get("KH_PG_ROPE_FUSE") != "0"
    mfma_attn = _mfma_attn(spec) and hooks.get("KH_PG_ATTN") != "0"
    out = set()
    prev = None
    for epi, rows, K, T, R, NT, slices, ks, kz, wgs, waves, solo in lines:
        if epi == 0:
            if fused and spec.rope_mode == INTER:
                out.add(("rope", "pairs"))
            elif fused and spec.head_size % 32 == 0 and R == 2 and NT <= 4:
                out.add(("rope", "tiles", spec.head_size // 2))
            else:
                out.add(("rope", "k_pg_rope", "half" if spec.rope_mode == HALF else "interleaved"))
        if epi == 1:
            out.add(("kz", kz))
            wo = prev == 0  # the residual GEMM right after the QKV GEMM (and attention) is wo, else w2
            out.add(("B", q, "tiled" if (not wo or mfma_attn) else "rows"))
        if not spec.quant:
            out.add(("solo", solo))
        nb = K // (64 if spec.quant else 16)
        ring_d = 8 if R * NT <= 8 else RING_D16
        for n in _wave_ranges(nb, ks, kz):
            if n == 0:
                out.add(("empty K range", q))
            elif not spec.quant:
                out.add(("loop", R, NT, "ring" if n >= 2 * ring_d and n % ring_d == 0 else "phase"))
        prev = epi
    for k in launched:
        mt = re.match(r"k_pg_attn<\d+,\d+,(\d)>", k)
        if mt and int(mt.group(1)) > 1:
            out.add(("attn QT > 1, tiled", q))
    return out


def _run(m, spec, toks, sc, hooks, floor, capfd, what, forced=None, reject=False):
    """One scenario under `hooks`: launch log, [pg] lines (forced shapes checked) and variants recorded."""
    _set_hooks(hooks)
    capfd.readouterr()
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        res = _scenario(m, spec, toks, sc, floor, what)
        launched = _ffi.launch_log()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _set_hooks({})
    err = capfd.readouterr().err
    lines = _pg_lines(err)
    assert lines, f"{what}: no [pg] line (KH_PG_DEBUG)"
    if reject:
        for e in EPIS:
            assert f"[kh] KH_PG_SHAPE_{e}=" in err and "rejected" in err, f"{what}: KH_PG_SHAPE_{e} not reported"
    else:
        assert "rejected" not in err, f"{what}: {[ln for ln in err.splitlines() if 'rejected' in ln]}"
    for e, s in (forced or {}).items():
        ei = EPIS.index(e)
        got = {(ln[4], ln[5], ln[7], ln[8]) for ln in lines if ln[0] == ei}
        want = {tuple(s[:3]) + ((s[3] if len(s) > 3 else 1),)}
        assert got == want, f"{what}: {e} ran as {sorted(got)}, forced {want}"
    return res, launched, _variants(spec, lines, hooks, launched)


def _same(a, b, what):
    (ra, la), (rb, lb) = a, b
    assert np.array_equal(la, lb), f"{what}: logits differ"
    for ca, cb in zip(ra, rb):
        for layer, ((ka, va), (kb, vb)) in enumerate(zip(ca, cb)):
            assert np.array_equal(ka, kb) and np.array_equal(va, vb), f"{what}: K/V rows differ (layer {layer})"


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name, capfd):
    """All forced shapes and hook variants of one geometry against its fp64 gold (module docstring)."""
    from kuiperllama_amd.model import KuiperModel
    spec, deep = GEOMETRIES[name]
    floor = LOGIT_ATOL_Q8 if spec.quant else LOGIT_ATOL_F32
    img_d = binfmt.synth_image(spec, seed=4343, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    img_h = img_d.cpu().numpy()
    rng = np.random.default_rng(11)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, CACHE)]
    scen = [{"name": "shallow", "gold": _gold(oracle, img_h, spec, toks, 0, SHALLOW[2] + 1, SHALLOW[2])}]
    if deep:
        rows = _deep_rows(spec, rng)
        scen.append({"name": "deep", "rows": rows,
                     "gold": _gold(oracle, img_h, spec, toks, DEEP[0], DEEP[2], DEEP[1], rows)})
    mfma = _mfma_attn(spec)
    launched, variants = set(), set()
    m = KuiperModel.from_device_image(img_d, spec)
    _ffi.debug_set("KH_PG_DEBUG", "1")
    try:
        for sc in scen:
            if sc["name"] == "deep":
                for layer in range(spec.n_layers):
                    m.write_kv(layer, 0, sc["rows"][0][layer], sc["rows"][1][layer])
            tag = f"{name} {sc['name']}"

            def run(hooks, what, **kw):
                res, lg, var = _run(m, spec, toks, sc, hooks, floor, capfd, f"{tag} {what}", **kw)
                launched.update(lg)
                variants.update(var)
                return res, lg

            base, base_log = run({}, "heuristic")
            if sc["name"] == "deep" and mfma:
                # from start position 2048 on the attention takes more than one query tile by itself
                assert any(re.match(r"k_pg_attn<\d+,\d+,[24]>", k) for k in base_log), sorted(base_log)
            _same(base, run({"KH_PG_ROPE_FUSE": "0"}, "KH_PG_ROPE_FUSE=0")[0], f"{tag} KH_PG_ROPE_FUSE=0")
            shapes = _shapes(spec)
            # solo on and off at one forced shape (KH_PG_SOLO=0 also reprices the heuristic's candidates)
            solo = run(_shape_hooks(shapes[0]), f"shape 0 {shapes[0]}", forced=shapes[0])[0]
            _same(solo, run({**_shape_hooks(shapes[0]), "KH_PG_SOLO": "0"}, "shape 0 KH_PG_SOLO=0", forced=shapes[0])[0],
                  f"{tag} shape 0 KH_PG_SOLO=0")
            if sc["name"] == "deep":
                shapes = shapes[:3] + shapes[-1:]
                run({"KH_PG_ATTN": "0"} if mfma else {"KH_PG_CHUNK": "100"}, "variant")
            else:
                run({"KH_PG_CHUNK": "100"}, "KH_PG_CHUNK=100")
                # hook values no launch has: reported on stderr, the heuristic shape runs
                bad = {"KH_PG_SHAPE_QKV": "2,4,3", "KH_PG_SHAPE_RESID": "1,4,1,3", "KH_PG_SHAPE_SWIGLU": "1,4,8"}
                if spec.dim % 32:
                    bad["KH_PG_SHAPE_RESID"] = "2,2,1"  # no 32-row tile: dim is an odd multiple of 16
                _same(base, run(bad, "rejected hooks", reject=True)[0], f"{tag} rejected hooks")
                if mfma:
                    for qt in ("1", "2", "4"):
                        run({"KH_PG_ATTN_QT": qt}, f"KH_PG_ATTN_QT={qt}")
                if spec.quant and mfma and spec.head_size == 64:
                    run({"KH_PG_ATTN": "0"}, "KH_PG_ATTN=0")
            for i, sh in enumerate(shapes[1:], 1):
                run(_shape_hooks(sh), f"shape {i} {sh}", forced=sh)
    finally:
        _ffi.debug_set("KH_PG_DEBUG", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _set_hooks({})
        m.close()
    _LAUNCHED[name] = launched
    _VARIANTS[name] = variants
    print(f"{name}: {len(launched)} instantiations launched, {len(variants)} variants")


def test_int8_group128_takes_the_bit_exact_prefill(gpu):
    """int8 with 128-weight groups has no GEMM prefill (its MFMA operand load is one 64-group): prefill_gemm says
    KH_ERR_UNSUPPORTED, and generate() runs a long prompt through the B-token prefill - no k_pg_* kernel, words
    equal to the token-by-token prompt phase."""
    from kuiperllama_amd.model import KuiperModel
    spec = _spec(512, 1024, 8, 2, 999, True, 128, INTER, L, "pg-q8-g128")
    img_d = binfmt.synth_image(spec, seed=4343, device=gpu, final_norm_std=1.0)
    rng = np.random.default_rng(12)
    prompt = [int(t) for t in rng.integers(0, spec.vocab_size, 40)]
    m = KuiperModel.from_device_image(img_d, spec)
    try:
        with pytest.raises(_ffi.KhError) as ei:
            m.prefill_gemm(prompt, 0)
        assert ei.value.code == -2
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        got, _ = m.generate(prompt, 72)
        log = _ffi.launch_log()
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        assert not [k for k in log if k.startswith("k_pg_")], sorted(log)
        assert any(k.startswith("k_pf_") for k in log), sorted(log)
        fs = m.first_sample()
        assert fs is not None and fs["prefill_mode"] == "gemv", fs
        _ffi.debug_set("KH_PREFILL", "token")
        want, _ = m.generate(prompt, 72)
        assert m.first_sample() is None
        assert got == want
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _ffi.debug_set("KH_PREFILL", None)
        m.close()


@pytest.fixture(scope="module")
def compiled():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    return co.kernels(co.code_object_notes(_ffi.LIB_PATH), set(STEMS))


def _all_ran():
    missing = [g for g in GEOMETRIES if g not in _LAUNCHED]
    assert not missing, f"geometries that did not run to the end (run the whole module): {missing}"


@pytest.mark.parametrize("stem", STEMS)
def test_template_gate(gpu, compiled, stem):
    """Every compiled instantiation of the kernel was launched (and checked) by test_geometry, except the
    documented-unreachable ones."""
    _all_ran()
    comp = {k for k in compiled if k.split("<")[0] == stem}
    seen = {k for s in _LAUNCHED.values() for k in s if k.split("<")[0] == stem}
    unreach = {k for k in UNREACHABLE if k.split("<")[0] == stem}
    assert comp, f"no {stem} kernel in the library"
    assert seen <= comp, f"launched but not found in the code objects: {sorted(seen - comp)}"
    assert unreach <= comp, f"documented-unreachable but not compiled: {sorted(unreach - comp)}"
    assert not (seen & unreach), f"documented unreachable but launched: {sorted(seen & unreach)}"
    print(f"{stem}: {len(seen)} of {len(comp)} compiled instantiations launched and checked; "
          f"{len(unreach)} documented unreachable")
    assert not (comp - seen - unreach), f"{stem}: compiled, reachable and never launched: {sorted(comp - seen - unreach)}"


def _required_variants():
    req = {("rope", "pairs"), ("rope", "k_pg_rope", "half"), ("rope", "k_pg_rope", "interleaved")}
    req |= {("rope", "tiles", 32), ("rope", "tiles", 48), ("rope", "tiles", 64)}  # head sizes 64, 96, 128
    req |= {("kz", 1), ("kz", 2), ("kz", 4), ("solo", True), ("solo", False)}
    req |= {("B", q, b) for q in ("f32", "q8") for b in ("tiled", "rows")}
    req |= {("loop", r, nt, lp) for r, nt in TILES for lp in ("ring", "phase")}
    req |= {("empty K range", q) for q in ("f32", "q8")} | {("attn QT > 1, tiled", q) for q in ("f32", "q8")}
    return req


def test_variant_gate(gpu):
    """Every variant inside the kernels (module docstring) was reached by some run of test_geometry."""
    _all_ran()
    seen = set().union(*_VARIANTS.values())
    req = _required_variants()
    print(f"variants: {len(req & seen)} of {len(req)} reached")
    assert not (req - seen), f"never reached: {sorted(req - seen, key=str)}"
