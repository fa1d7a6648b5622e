"""Every decode-GEMV kernel instantiation the library compiles, launched and checked against an fp64 gold.

The fused decode step picks one instantiation of k_qkv / k_gemv_res (wo, w2) / k_wo_comb / k_ffn13 / k_cls
<QUANT, U, MAXV, SPLIT> per launch from the shape plan, the staging depth kh_stage_maxv(M, wg) and the value lists
of its launch site (kh_dispatch.h: kh_pick); the int8 ffn13 / classifier launches may run on the LDS-DMA ring kernels, and the B-token prefill has its own
k_pf_* family.  The heuristic shapes of the model geometries elsewhere in the suite reach only a few of them.  Here a
handful of seeded geometries - each 2 layers, a small odd vocabulary, 1024 cache rows - are run under forced shapes
(hooks KH_SHAPE_<QKV|WO|FFN|W2|CLS> = "split,u,grid,wg", workgroups of 256 and 512 threads) so that every staging
depth of every template is launched:

  MAXV 1 / 2 / 4 / 6 / 0 follow from M against 4, 8, 16 and 24 float4 per thread: dim 1152 (MAXV 2 at 256 threads,
  1 at 512), dim 4224 (0 at 256 threads - wo's depth 6 is launched as 0 -, 4 at 512), hidden 10368 (w2: 0 at 256
  threads, 6 at 512), hidden 3072 (4 / 2) and hidden <= 2048 (2 / 1).

and the edges where such kernels go wrong: M not a multiple of a wave's 256-float / 1-KiB piece, an odd vocabulary
(the last classifier pair is one row), grids of a few workgroups (every workgroup's pairs straddle the q/k/v
boundaries and the pair count is not a multiple of the grid's waves), both RoPE modes, head sizes 64, 128, 80 and 96,
Qwen2 biases, int8 groups of 16 ... 256 weights (ring geometries at 16 and 256).

Per geometry the gold is computed once: OracleModel.forward(..., ACC_F64) at teacher-forced steps 0, 1, 2 and, after
random K/V rows were written below it, at position 300 (two or three attention time splits, few enough that k_wo_comb
merges them wherever the geometry allows it).  It does not depend on the launch shape, so it serves every shape of
that geometry.  Per shape:
  * logits within max(floor, 3 x |oracle fp32 - gold|) of the gold (floor: the suite's fp32 / int8 logit tolerance),
    the argmax equal to the gold's wherever its top-2 margin exceeds 2 x floor;
  * the K/V rows each step wrote, in every layer, within 1e-5 of the gold's (the rows hold NaN before the step, so
    an element the kernel never writes fails);
  * grid invariance: a shape that differs only in the grids gives bit-identical logits and K/V rows;
  * the B-token prefill (where the shape allows it) writes K/V rows bit-identical to the token-by-token steps;
  * for two shapes per geometry, generate(exec="graph") equals exec="fused".
While the steps run, the launch log (hook KH_LAUNCH_LOG) records the instantiations launched.  The coverage gates at
the end compare it, per template, with the instantiations compiled into the library (read from its code objects):
a new template argument fails here until it is tested, and a shape hook the plan refused shows up as a gap.
"""
import itertools

import numpy as np
import pytest
import torch

import code_objects as co
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

LOGIT_ATOL_F32 = 2e-5  # test_model_gpu.py: LOGIT_ATOL_F32 / LOGIT_ATOL_Q8
LOGIT_ATOL_Q8 = 5e-5
KV_ATOL = 1e-5         # fused-path K/V bound of test_model_gpu.py::test_real_stride_deep_positions_vs_oracle
CACHE = 1024
DEEP_POS = 300         # 2 (head size 64) or 3 (128) attention time splits: k_wo_comb merges them where it can


def _spec(dim, hidden, heads, kv_heads, vocab, quant, group, rope, family, name):
    theta = 1000000.0 if family == binfmt.FAMILY_QWEN2 else 10000.0
    return binfmt.ModelSpec(dim, hidden, 2, heads, kv_heads, vocab, CACHE, False, family, quant, group, rope, theta,
                            1e-6 if family == binfmt.FAMILY_QWEN2 else 1e-5, name)


L, Q2 = binfmt.FAMILY_LLAMA, binfmt.FAMILY_QWEN2
HALF, INTER = binfmt.ROPE_HALF, binfmt.ROPE_INTERLEAVED
GEOMETRIES = {
    # fp32
    "f32-1152-h10368": _spec(1152, 10368, 18, 6, 1001, False, 64, HALF, L, "f32-1152"),       # hs 64, GQA 3:1
    "f32-4224-h3072": _spec(4224, 3072, 33, 3, 777, False, 64, INTER, L, "f32-4224"),         # hs 128, GQA 11:1
    "f32-qwen-960-hs80": _spec(960, 1600, 12, 2, 1537, False, 64, HALF, Q2, "f32-qwen-hs80"),  # bias, hs 80
    # int8
    "q8-1152-h10368-g128": _spec(1152, 10368, 9, 9, 1001, True, 128, INTER, L, "q8-1152"),     # hs 128, MHA
    "q8-4224-h3072-g64": _spec(4224, 3072, 66, 6, 777, True, 64, HALF, L, "q8-4224"),          # hs 64
    "q8-768-hs96-g32": _spec(768, 1536, 8, 2, 1537, True, 32, HALF, L, "q8-hs96"),             # hs 96
    "q8-640-g16": _spec(640, 1728, 10, 5, 999, True, 16, INTER, L, "q8-g16"),                  # ring at group 16
    "q8-1280-g256": _spec(1280, 2560, 10, 2, 1003, True, 256, INTER, L, "q8-g256"),            # ring at group 256
}

TEMPLATES = {  # coverage gate -> kernel name stems
    "k_qkv": {"k_qkv"}, "k_gemv_res": {"k_gemv_res"}, "k_wo_comb": {"k_wo_comb"}, "k_ffn13": {"k_ffn13"},
    "k_cls": {"k_cls"}, "ring": {"k_ffn13_ring", "k_cls_ring"}, "prefill": {"k_pf_qkv", "k_pf_gemv_res", "k_pf_ffn13"},
}
# compiled instantiations no decode step can launch, with the reason (none at present: k_qkv's SPLIT = 4 kernels,
# which the qkv plan never asked for, are no longer compiled)
UNREACHABLE = {}

_LAUNCHED = {}  # geometry -> instantiations its shapes launched (filled by test_geometry, read by the gates)


def _pairs(spec):
    """Work items (row pairs; ffn13: rows of w1/w3) of qkv, wo, ffn13, w2, cls: pick_shape's `pairs`."""
    return {"QKV": (spec.dim + 2 * spec.kv_dim) // 2, "WO": spec.dim // 2, "FFN": spec.hidden_dim,
            "W2": spec.dim // 2, "CLS": (spec.vocab_size + 1) // 2}


def _shapes(spec):
    """Forced shapes of one geometry: a list of {hook suffix: (split, u, grid, wg)}.  For each workgroup width, nine
    shapes walk every (u, split) each kernel accepts (qkv: split <= 2, ffn13 / cls: 1, int8 w2 also u = 3).  Grid:
    one pair per wave, at most 1024 workgroups.  Then two copies with only the grids changed, and for int8 one shape
    without the ffn13 / cls hooks (the ring kernels take those launches)."""
    us = (2, 4) if spec.quant else (2, 4, 8)
    combos = {"QKV": list(itertools.product(us, (1, 2))), "WO": list(itertools.product(us, (1, 2, 4))),
              "FFN": list(itertools.product(us, (1,))), "CLS": list(itertools.product(us, (1,))),
              "W2": list(itertools.product((2, 3, 4) if spec.quant else us, (1, 2, 4)))}
    pairs = _pairs(spec)
    out = []
    for wg in (256, 512):
        for i in range(9):
            sh = {}
            for k, c in combos.items():
                u, sp = c[i % len(c)]
                ppw = (wg // 64) // sp
                sh[k] = (sp, u, min(1024, -(-pairs[k] // ppw)), wg)
            out.append(sh)
    for base, grids in ((0, (3, 5, 2, 7, 1)), (13, (7, 61, 3, 13, 5))):
        out.append({k: (s[0], s[1], g, s[3]) for (k, s), g in zip(out[base].items(), grids)})
    if spec.quant:
        out.append({k: v for k, v in out[4].items() if k not in ("FFN", "CLS")})
    return out


def _steps(spec, rng):
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, 4)]
    return list(zip(toks, (0, 1, 2, DEEP_POS)))


def _deep_rows(spec, rng):
    kr = rng.standard_normal((spec.n_layers, DEEP_POS, spec.kv_dim), dtype=np.float32)
    vr = rng.standard_normal((spec.n_layers, DEEP_POS, spec.kv_dim), dtype=np.float32)
    kr[:, rng.integers(0, DEEP_POS, 8)] *= 6.0  # a few dominant keys: the splits' maxima differ
    return kr, vr


def _gold(oracle, img_h, spec, steps, rows):
    """fp64 gold and fp32 oracle of the teacher-forced steps: [(logits64, logits32, K rows [L, kv], V rows)]."""
    out = []
    g = oracle.OracleModel.from_spec(img_h, spec, cache_len=CACHE)
    o = oracle.OracleModel.from_spec(img_h, spec, cache_len=CACHE)
    for tok, pos in steps:
        if pos == DEEP_POS:
            for om in (g, o):
                ko, vo = om.kv_cache()
                ko[:, :DEEP_POS] = rows[0]
                vo[:, :DEEP_POS] = rows[1]
        lg = g.forward(tok, pos, oracle.ACC_F64)
        lo = o.forward(tok, pos)
        ko, vo = g.kv_cache()
        out.append((lg, lo, ko[:, pos].copy(), vo[:, pos].copy()))
    g.close()
    o.close()
    return out


def _set_shape_hooks(sh):
    for k in ("QKV", "WO", "FFN", "W2", "CLS"):
        _ffi.debug_set(f"KH_SHAPE_{k}", ",".join(map(str, sh[k])) if k in sh else None)


def _run_shape(m, spec, steps, rows, gold, floor, what):
    """The teacher-forced steps on model m; checks against the gold, returns (logits, K rows, V rows) per step."""
    nan = np.full((1, spec.kv_dim), np.nan, np.float32)
    res = []
    for (tok, pos), (lg, lo, kg, vg) in zip(steps, gold):
        if pos == DEEP_POS:
            for layer in range(spec.n_layers):
                m.write_kv(layer, 0, rows[0][layer], rows[1][layer])
        for layer in range(spec.n_layers):
            m.write_kv(layer, pos, nan, nan)
        nxt = m.predict(tok, pos, exec="fused")
        got = m.logits()
        err = float(np.abs(got - lg).max())
        lim = max(floor, 3.0 * float(np.abs(lo - lg).max()))
        assert err <= lim, f"{what} pos {pos}: |logit - gold| {err:.3e} > {lim:.3e}"
        top2 = np.sort(lg)[-2:]
        if top2[1] - top2[0] > 2 * floor:
            assert nxt == int(np.argmax(lg)), f"{what} pos {pos}: argmax {nxt} vs gold {int(np.argmax(lg))}"
        ks, vs = [], []
        for layer in range(spec.n_layers):
            k, v = m.read_kv(layer, pos, 1)
            for name, a, b in (("K", k[0], kg[layer]), ("V", v[0], vg[layer])):
                e = np.abs(a - b)
                assert np.all(e <= KV_ATOL), \
                    f"{what} pos {pos} layer {layer}: {name} row off by {np.nanmax(e) if np.isfinite(e).any() else e}" \
                    f" ({int(np.isnan(a).sum())} NaN)"
            ks.append(k[0])
            vs.append(v[0])
        res.append((got, np.stack(ks), np.stack(vs)))
    return res


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name):
    """All forced shapes of one geometry against its fp64 gold (module docstring), launch log recorded."""
    from kuiperllama_amd.model import KuiperModel
    spec = GEOMETRIES[name]
    floor = LOGIT_ATOL_Q8 if spec.quant else LOGIT_ATOL_F32
    img_d = binfmt.synth_image(spec, seed=4242, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    img_h = img_d.cpu().numpy()
    rng = np.random.default_rng(7)
    steps = _steps(spec, rng)
    rows = _deep_rows(spec, rng)
    gold = _gold(oracle, img_h, spec, steps, rows)
    launched = set()
    by_shape = {}  # (split, u, wg) of the five kernels -> results: grid invariance
    n_prefill = 0
    try:
        for i, sh in enumerate(_shapes(spec)):
            what = f"{name} shape {i} {sh}"
            _set_shape_hooks(sh)
            m = KuiperModel.from_device_image(img_d, spec)
            try:
                _ffi.debug_set("KH_LAUNCH_LOG", "1")  # after creation: its self-tests are not checked launches
                res = _run_shape(m, spec, steps, rows, gold, floor, what)
                key = tuple((k, s[0], s[1], s[3]) for k, s in sorted(sh.items()))
                if key in by_shape:
                    for (la, ka, va), (lb, kb, vb) in zip(by_shape[key], res):
                        assert np.array_equal(la, lb), f"{what}: logits depend on the grid"
                        assert np.array_equal(ka, kb) and np.array_equal(va, vb), f"{what}: K/V depend on the grid"
                by_shape.setdefault(key, res)
                # B-token prefill of the three first tokens: the K/V rows of the token-by-token steps, bit for bit
                toks = [t for t, _ in steps[:3]]
                try:
                    m.prefill(toks, 0)
                except _ffi.KhError as e:
                    assert e.code == -2, e  # KH_ERR_UNSUPPORTED: the shape is outside prefill_supported
                else:
                    n_prefill += 1
                    for layer in range(spec.n_layers):
                        k, v = m.read_kv(layer, 0, 3)
                        kt = np.stack([r[1][layer] for r in res[:3]])
                        vt = np.stack([r[2][layer] for r in res[:3]])
                        assert np.array_equal(k, kt) and np.array_equal(v, vt), f"{what}: prefill K/V, layer {layer}"
                launched |= _ffi.launch_log()
                _ffi.debug_set("KH_LAUNCH_LOG", None)
                if i in (0, 13):
                    prompt = [t for t, _ in steps[:2]]
                    ga, _ = m.generate(prompt, 10, exec="graph")
                    gf, _ = m.generate(prompt, 10, exec="fused")
                    assert ga == gf, f"{what}: graph replay {ga} vs fused {gf}"
            finally:
                m.close()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _set_shape_hooks({})
    assert n_prefill > 0, f"{name}: no shape ran the B-token prefill"
    _LAUNCHED[name] = launched
    print(f"{name}: {len(_shapes(spec))} shapes, {len(launched)} instantiations launched, {n_prefill} prefills")


@pytest.fixture(scope="module")
def compiled():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    return co.instantiations(co.code_object_notes(_ffi.LIB_PATH), set().union(*TEMPLATES.values()))


@pytest.mark.parametrize("template", list(TEMPLATES))
def test_coverage_gate(gpu, compiled, template):
    """Every compiled instantiation of the template was launched (and checked) by test_geometry, except the
    documented-unreachable ones."""
    missing_geo = [g for g in GEOMETRIES if g not in _LAUNCHED]
    assert not missing_geo, f"geometries that did not run to the end (run the whole module): {missing_geo}"
    stems = TEMPLATES[template]
    comp = {k for k in compiled if k.split("<")[0] in stems}
    seen = {k for s in _LAUNCHED.values() for k in s if k.split("<")[0] in stems}
    unreach = {k for k in UNREACHABLE if k.split("<")[0] in stems}
    assert comp, f"no {template} instantiation in the library"
    assert seen <= comp, f"launched but not found in the code objects: {sorted(seen - comp)}"
    assert unreach <= comp, f"documented-unreachable but not compiled: {sorted(unreach - comp)}"
    assert not (seen & unreach), f"documented unreachable but launched: {sorted(seen & unreach)}"
    gap = comp - seen - unreach
    print(f"{template}: {len(seen)} of {len(comp)} compiled instantiations launched and checked; "
          f"{len(unreach)} documented unreachable")
    assert not gap, f"{template}: compiled, reachable and never launched: {sorted(gap)}"
