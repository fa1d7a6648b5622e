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
The forced shapes, the teacher-forced step loop and the hooks are those of wcopy_cases.py, which the tests of the
weight copies share.
"""
import numpy as np
import pytest
import torch

import code_objects as co
import wcopy_cases as wc
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

LOGIT_ATOL_F32 = 2e-5  # test_model_gpu.py: LOGIT_ATOL_F32 / LOGIT_ATOL_Q8
LOGIT_ATOL_Q8 = 5e-5
KV_ATOL = 1e-5         # fused-path K/V bound of test_model_gpu.py::test_real_stride_deep_positions_vs_oracle
CACHE, DEEP_POS = wc.CACHE, wc.DEEP_POS  # 1024 rows; the deep step is at position 300
L, Q2, HALF, INTER = wc.L, wc.Q2, wc.HALF, wc.INTER
_spec = wc.spec

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


def _shapes(spec):
    """wcopy_cases.decode_shapes with a second odd-grid shape of its own and, for int8, the shape that leaves the
    ffn13 / cls launches to the ring kernels"""
    return wc.decode_shapes(spec, second_odd_grids=(7, 61, 3, 13, 5), ring_shape=spec.quant)


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


def _check_step(gold, floor, what):
    """run_steps' check of one step against the gold: logits, the argmax where the gold's margin allows, K/V rows"""
    def check(i, tok, pos, nxt, got, ks, vs):
        lg, lo, kg, vg = gold[i]
        err = float(np.abs(got - lg).max())
        lim = max(floor, 3.0 * float(np.abs(lo - lg).max()))
        assert err <= lim, f"{what} pos {pos}: |logit - gold| {err:.3e} > {lim:.3e}"
        top2 = np.sort(lg)[-2:]
        if top2[1] - top2[0] > 2 * floor:
            assert nxt == int(np.argmax(lg)), f"{what} pos {pos}: argmax {nxt} vs gold {int(np.argmax(lg))}"
        for layer in range(len(ks)):
            for name, a, b in (("K", ks[layer], kg[layer]), ("V", vs[layer], vg[layer])):
                e = np.abs(a - b)
                assert np.all(e <= KV_ATOL), \
                    f"{what} pos {pos} layer {layer}: {name} row off by {np.nanmax(e) if np.isfinite(e).any() else e}" \
                    f" ({int(np.isnan(a).sum())} NaN)"
    return check


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry(gpu, oracle, name):
    """All forced shapes of one geometry against its fp64 gold (module docstring), launch log recorded."""
    spec = GEOMETRIES[name]
    floor = LOGIT_ATOL_Q8 if spec.quant else LOGIT_ATOL_F32
    img_d = binfmt.synth_image(spec, seed=4242, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    img_h = img_d.cpu().numpy()
    rng = np.random.default_rng(7)
    steps = wc.steps(spec, rng)
    rows = wc.deep_rows(spec, rng)
    gold = _gold(oracle, img_h, spec, steps, rows)
    shapes = _shapes(spec)
    launched = set()
    by_shape = {}  # (split, u, wg) of the five kernels -> results: grid invariance
    n_prefill = 0
    try:
        for i, sh in enumerate(shapes):
            what = f"{name} shape {i} {sh}"
            wc.set_shape_hooks(sh)
            m = wc.model(img_d, spec)
            try:
                with wc.launch_log() as read:  # after creation: its self-tests are not checked launches
                    res = wc.run_steps(m, spec, steps, rows, _check_step(gold, floor, what))  # raw words
                    key = tuple((k, s[0], s[1], s[3]) for k, s in sorted(sh.items()))
                    if key in by_shape:
                        for (la, ka, va, _), (lb, kb, vb, _) in zip(by_shape[key], res):
                            assert np.array_equal(la, lb), f"{what}: logits depend on the grid"
                            assert np.array_equal(ka, kb) and np.array_equal(va, vb), f"{what}: K/V depend on the grid"
                    by_shape.setdefault(key, res)
                    # B-token prefill of the three first tokens: the K/V rows of the token-by-token steps, bit for bit
                    toks = [t for t, _ in steps[:3]]
                    try:
                        m.prefill(toks, 0)
                    except _ffi.KhError as e:
                        assert e.code == _ffi.KH_ERR_UNSUPPORTED, e  # the shape is outside prefill_supported
                    else:
                        n_prefill += 1
                        for layer in range(spec.n_layers):
                            k, v = m.read_kv(layer, 0, 3)
                            kt = np.stack([r[1][layer] for r in res[:3]])
                            vt = np.stack([r[2][layer] for r in res[:3]])
                            assert np.array_equal(k.view(np.uint32), kt) and np.array_equal(v.view(np.uint32), vt), \
                                f"{what}: prefill K/V, layer {layer}"
                    launched |= read()
                if i in (0, 13):
                    prompt = [t for t, _ in steps[:2]]
                    ga, _ = m.generate(prompt, 10, exec="graph")
                    gf, _ = m.generate(prompt, 10, exec="fused")
                    assert ga == gf, f"{what}: graph replay {ga} vs fused {gf}"
            finally:
                m.close()
    finally:
        wc.set_shape_hooks({})
    assert n_prefill > 0, f"{name}: no shape ran the B-token prefill"
    _LAUNCHED[name] = launched
    print(f"{name}: {len(shapes)} shapes, {len(launched)} instantiations launched, {n_prefill} prefills")


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
