"""The wide pass's one-launch attention on the GPU (KH_FLAG_WIDE_ATTN; csrc/kh_seq_attn_wide.h: k_sg_attn, k_sg_attn_merge).

The operator ops.mha_decode_lanes against an fp64 softmax attention (_gold) with every cache row outside the lanes' ranges
set to NaN, bound 3e-5 + 2e-5 |gold| (the attention gates'); its argument errors; one wide model pass per geometry of
seq_gemm_cases.SPECS under the flag against the CPU oracle within G.kv_atol / G.logit_atol, and the flag's inert cases.

Worst errors measured on an MI355X (the tests print them as "worst[...]"; DESIGN 3.3m repeats them):
    operator, |out - gold|:   8.2e-7 at head size 128, 9.9e-7 at 64, 7.5e-7 at 48 (bound 3e-5 + 2e-5 |gold|)
    model pass under the flag, K/V rows (bound) and logits (bound):
        mha-inter 1.25e-6 (5e-6) / 1.55e-6 (2e-5)      gqa-half 1.19e-6 (5e-6) / 1.64e-6 (2e-5), sharers included
        half-hs48 1.55e-6 (5e-6) / 1.25e-6 (2e-5)      qwen-bias 1.28e-6 (5e-6) / 1.55e-6 (2e-5)
        int8      1.67e-6 (2e-5) / 1.37e-6 (5e-5)"""
import numpy as np
import pytest
import torch

import seq_gemm_cases as G
from kuiperllama_amd import _ffi, ops
from kuiperllama_amd.model import KuiperModel

pytestmark = pytest.mark.gpu

SEQ = 4096    # cache rows of the operator tests
LONG = 1024   # a range long enough to split
GEOMS = [(4, 4, 128), (8, 2, 64), (7, 1, 64), (8, 2, 48)]  # heads, kv heads, head size


@pytest.fixture(autouse=True)
def _clean_log():
    yield
    _ffi.debug_set("KH_LAUNCH_LOG", None)


def _boundary(kv_mul, hs):  # the first chunk boundary of a range of LONG rows, from the plan
    (it,) = _ffi.plan_wide_attn(np.array([[LONG - 1], [0], [0], [0]], np.int32), kv_mul, hs, SEQ)
    assert it["chunks"] > 1
    return 16 * it["chunk_tiles"]


def _unrelated(positions, row=0):
    out = []
    for p in positions:
        out.append((p, row, 0, 0))
        row += p + 1
    return out, row


def _share_group(P, B):
    """a parent (rows from 0, own lane at P + 3), 5 sharers at positions P, P + 1 and far behind, 2 unrelated lanes"""
    row = P + 4
    lanes = [(P + 3, 0, 0, 0)]
    for pos in (P, P, P + 1, P + B + 40, P + 300):
        lanes.append((pos, row - P, P, 0))
        row += pos - P + 1
    more, _ = _unrelated([21, 0], row)
    return lanes + more


def lane_set(name, B):
    """rows of (pos, base, pfx_len, pfx_row0)"""
    if name == "one":
        return [(0, 5, 0, 0)]
    if name == "17":  # tile edges, one below / on / one behind the chunk boundary, a range that splits
        return _unrelated([0, 15, 16, 17, B - 1, B, B + 1, LONG - 1, 2 * B - 1, 2 * B, 3, 40, 7, 100, 1, 31, 32])[0]
    if name == "64":
        return _unrelated([(37 * i) % 60 for i in range(64)])[0]
    if name.startswith("share"):
        P = {"share1": 1, "share16": 16, "share17": 17, "shareB-1": B - 1, "shareB+1": B + 1, "share1000": 1000}[name]
        return _share_group(P, B)
    if name == "two parents":  # parents at rows 0 and 600; two sharers of the first with different P
        return [(50, 1500 - 33, 33, 0), (40, 1600 - 33, 33, 0), (90, 1700 - 20, 20, 0), (700, 1800 - 530, 530, 600),
                (531, 2100 - 530, 530, 600), (100, 0, 0, 0), (540, 600, 0, 0), (2, 3000, 0, 0)]
    assert name == "negative base"  # the sharer's own rows are rows 0 ..: base = -P
    return [(45, -40, 40, 500), (44, 100 - 40, 40, 500), (60, 500, 0, 0)]


SETS = ["one", "17", "64", "share1", "share16", "share17", "shareB-1", "shareB+1", "share1000", "two parents",
        "negative base"]


def _rows(lane):
    pos, base, pfx, prow = lane
    return np.concatenate([prow + np.arange(pfx), base + np.arange(pfx, pos + 1)])


def _gold(lanes, q, kc, vc, heads, kv_heads, hs):
    """fp64: per lane, gather its positions' rows through the prefix translation, then plain softmax attention"""
    out = np.zeros((len(lanes), heads * hs))
    for i, lane in enumerate(lanes):
        r = _rows(lane)
        for h in range(heads):
            g = h // (heads // kv_heads)
            s = kc[r, g * hs:(g + 1) * hs] @ q[i, h * hs:(h + 1) * hs] / np.sqrt(hs)
            p = np.exp(s - s.max())
            out[i, h * hs:(h + 1) * hs] = (p / p.sum()) @ vc[r, g * hs:(g + 1) * hs]
    return out


def _is_new(log):
    return (any(k.startswith("k_sg_attn<") for k in log) and any(k.startswith("k_sg_attn_merge") for k in log)
            and not any(k.startswith("k_seq_attn") for k in log))


_KV, _WORST = {}, {}


def _kv(kv_dim):
    if kv_dim not in _KV:
        rng = np.random.default_rng(kv_dim)
        _KV[kv_dim] = (rng.standard_normal((SEQ, kv_dim)).astype(np.float32),
                       rng.standard_normal((SEQ, kv_dim)).astype(np.float32))
    return _KV[kv_dim]


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("heads,kv_heads,hs", GEOMS)
def test_operator_against_fp64(gpu, heads, kv_heads, hs, name):
    kv_mul, kv_dim, dim = heads // kv_heads, kv_heads * hs, heads * hs
    lanes = lane_set(name, _boundary(kv_mul, hs))
    n = len(lanes)
    kc, vc = _kv(kv_dim)
    used = np.zeros(SEQ, bool)
    for lane in lanes:
        used[_rows(lane)] = True
    q = np.random.default_rng(n).standard_normal((n, dim)).astype(np.float32)
    gold = _gold(lanes, q.astype(np.float64), kc.astype(np.float64), vc.astype(np.float64), heads, kv_heads, hs)
    # every row that belongs to no lane's range is NaN, the rows just past each lane's pos included; layer 1 of 2
    poison = lambda a: torch.from_numpy(np.stack([np.full_like(a, np.nan), np.where(used[:, None], a, np.nan)])).to(gpu)
    out = torch.full((n, dim), float("nan"), device=gpu)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    ops.mha_decode_lanes(np.array(lanes, np.int32).T, heads, 1, SEQ, kv_dim, kv_mul, hs, out, torch.from_numpy(q).to(gpu),
                         poison(kc), poison(vc))
    log = _ffi.launch_log()
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), (name, np.argwhere(~np.isfinite(got))[:4])
    err = np.abs(got - gold)
    w = _WORST[hs] = max(_WORST.get(hs, 0.0), float(err.max()))
    print(f"worst[hs {hs}]: |out - gold| {w:.2e}")
    bad = err > 3e-5 + 2e-5 * np.abs(gold)
    assert not bad.any(), (name, float(err.max()), np.argwhere(bad)[:4])
    assert _is_new(log), log


@pytest.mark.parametrize("bad,code", [
    (dict(lanes=[(5, 0, 6, 100)]), _ffi.KH_ERR_INVALID_ARG),             # pos < pfx_len
    (dict(lanes=[(5, SEQ - 5, 0, 0)]), _ffi.KH_ERR_RANGE),               # its own row is row seq_len
    (dict(lanes=[(5, -1, 0, 0)]), _ffi.KH_ERR_RANGE),
    (dict(lanes=[(9, 100, 4, SEQ - 3)]), _ffi.KH_ERR_RANGE),             # the prefix runs past the cache
    (dict(lanes=[(0, i, 0, 0) for i in range(65)]), _ffi.KH_ERR_INVALID_ARG),
    (dict(lanes=[(0, 0, 0, 0)], hs=32), _ffi.KH_ERR_UNSUPPORTED),
])
def test_operator_argument_errors_leave_an_empty_launch_log(gpu, bad, code):
    hs, kv_mul, heads, n = bad.get("hs", 64), 4, 8, len(bad["lanes"])
    kv_dim = heads // kv_mul * hs
    z = lambda r, c: torch.zeros((r, c), device=gpu)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    with pytest.raises(_ffi.KhError) as e:
        ops.mha_decode_lanes(np.array(bad["lanes"], np.int32).T, heads, 0, SEQ, kv_dim, kv_mul, hs, z(n, heads * hs),
                             z(n, heads * hs), z(SEQ, kv_dim), z(SEQ, kv_dim))
    assert e.value.code == code and not _ffi.launch_log(), (e.value.code, _ffi.launch_log())


def _oracle_lane(om, text):
    """the oracle fed text token by token: logits and per-layer K/V row of its last position"""
    for p, t in enumerate(text):
        lg = om.forward(t, p)
    ko, vo = om.kv_cache()
    return lg.copy(), ko[:, len(text) - 1].copy(), vo[:, len(text) - 1].copy()


def _pass(m, spec, slots, toks, pos, want, what):
    """one wide pass; the lanes' K/V rows and logits against the oracle's; returns the launch log"""
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    got = m.seq_step(slots, toks, pos, gemm=True)
    log = set(_ffi.launch_log())
    _ffi.debug_set("KH_LAUNCH_LOG", None)
    worst_kv = worst_lg = 0.0
    for i, s in enumerate(slots):
        lg, k, v = want[i]
        row = m.seq_row(s, pos[i])
        for layer in range(spec.n_layers):
            kk, vv = m.read_kv(layer, row, 1)
            worst_kv = max(worst_kv, float(np.abs(kk[0] - k[layer]).max()), float(np.abs(vv[0] - v[layer]).max()))
        mine = m.seq_gemm_logits(i)
        worst_lg = max(worst_lg, float(np.abs(mine - lg).max()))
        assert got[i] == int(np.argmax(mine)), what + (i,)
    print(f"worst[{spec.name} {what[-1]}]: K/V {worst_kv:.2e} (bound {G.kv_atol(spec):.0e}), "
          f"logits {worst_lg:.2e} (bound {G.logit_atol(spec):.0e})")
    assert worst_kv <= G.kv_atol(spec) and worst_lg <= G.logit_atol(spec), what + (worst_kv, worst_lg)
    return log


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_a_wide_pass_under_the_flag(gpu, oracle, name):
    """17 lanes as lane_pos places them, on gqa-half also 3 sharers of slot 0 beside it; without the flag: as before"""
    spec = G.SPECS[name]
    T = G.texts(spec)
    om = oracle.OracleModel.from_spec(G.host_image(spec), spec, cache_len=G.LONG)
    slots = [int(s) for s in np.random.default_rng(17).permutation(17)]
    want = [_oracle_lane(om, T[s]) for s in slots]
    pos, toks = [G.lane_pos(s) for s in slots], [T[s][-1] for s in slots]
    for flags in (_ffi.KH_FLAG_WIDE_ATTN, 0):
        m = KuiperModel.from_host_image(G.host_image(spec), spec, max_seq_len=spec.seq_len, flags=flags)
        m.seq_slots_var(G.LENS)
        for s in slots:
            if G.lane_pos(s) > 0:
                m.seq_prefill(s, T[s][:G.lane_pos(s)])
        info = m.wide_attn_info()
        assert info["on"] == bool(flags) and info["reason"] == ("on" if flags else "flag not set"), info
        assert info["workspace_bytes"] == 0
        log = _pass(m, spec, slots, toks, pos, want, (name, "flag" if flags else "no flag"))
        assert _is_new(log) == bool(flags), sorted(log)
        assert (m.wide_attn_info()["workspace_bytes"] > 0) == bool(flags)
        if not flags:
            assert any(k.startswith("k_seq_attn<") for k in log), sorted(log)
        elif name == "gqa-half":
            # slots 3, 4, 5 share P = 200, 200 and 7 rows of slot 0 and continue with tokens of their own
            rng = np.random.default_rng(5)
            text = {s: T[0][:P] + [int(t) for t in rng.integers(0, spec.vocab_size, extra)]
                    for s, P, extra in ((3, 200, 1), (4, 200, 3), (5, 7, 4))}
            for s, P in ((3, 200), (4, 200), (5, 7)):
                m.seq_share(0, s, P)
                if len(text[s]) - 1 > P:
                    m.seq_prefill(s, text[s][P:-1], pos0=P)
            sl = [4, 0, 9, 3, 1, 5, 12]
            tx = [text.get(s, T[s]) for s in sl]
            log = _pass(m, spec, sl, [t[-1] for t in tx], [len(t) - 1 for t in tx], [_oracle_lane(om, t) for t in tx],
                        (name, "sharers"))
            assert _is_new(log), sorted(log)
        m.close()


def test_the_flag_is_inert_on_other_head_sizes(gpu):
    """head size 96 (no MFMA attention instantiation) under the flag: the grouped launches run, wide_attn_info says why"""
    spec = G.binfmt.ModelSpec(384, 1024, 2, 4, 2, 512, 256, False, G.L, False, 64, G.INTER, 10000.0, 1e-5, "sg-hs96")
    m = KuiperModel.from_host_image(G.host_image(spec), spec, flags=_ffi.KH_FLAG_WIDE_ATTN)
    info = m.wide_attn_info()
    assert not info["on"] and info["reason"] == "head size", info
    m.seq_slots(8)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    m.seq_step([0, 1, 2], [1, 2, 3], [0, 0, 0], gemm=True)
    log = _ffi.launch_log()
    assert any(k.startswith("k_seq_attn<") for k in log) and not any(k.startswith("k_sg_attn") for k in log), sorted(log)
    assert m.wide_attn_info()["workspace_bytes"] == 0
    m.close()
