"""Decode attention: every compiled k_attn_decode<G, KVM> instantiation, both workgroup widths, every split quantum
and every merge path, launched and checked against an fp64 gold.

The decode-attention launch (csrc/kh_attn.h::launch_attn_decode) picks k_attn_decode<G, KVM> from the head size
(G = 16 / 32 / 64 lanes per timestep) and the GQA ratio (KVM = kv_mul where the group path is instantiated and fits the
workgroup, else 0), runs 256- or 512-thread workgroups (hook KH_ATTN_WG), cuts the timesteps into splits of 64 / 128 /
256 (hook KH_ATTN_TS) or, past 16 quanta, of ceil(n / 16) rounded up to 64, switches to one workgroup per (KV group,
split) from pos + 1 >= t_long (hook KH_ATTN_TLONG), and merges the split partials in the last arriver (16 or 32 slots),
in the wo kernel (k_wo_comb, "deferred") or not at all (one split).  The model geometries elsewhere in the suite reach
a few of these.

Operator level (ops.mha_decode, the attention output itself): the geometries of GEOMETRIES - head sizes 36 ... 256, so
all three lane widths, masked lanes (36, 48, 72, 80, 96, 132, 160, 192), kv_mul 1, 2, 3 (not instantiated: stays
per-head), 4, 7, 8 - as layer 1 of a NaN-filled two-layer cache of 9000 rows, at both widths, under the default path
policy and KH_ATTN_TLONG = 64 / 300, one geometry per lane width also under KH_ATTN_TS = 64 / 128 / 256.  Where
the group path does not fit a width the plan (kh_plan_attention) must say so and the KVM = 0 kernel must run.  The
positions come from the plan: 0, 1, the kernel's batch size (wg / G) * 4 and its neighbours, both sides of pos + 1 =
256, of every change of the active-split count up to the cap, of t_long, the first position of the capped split
length, the last row.  Per position:
  * the output within atol 3e-5 + rtol 2e-5 of oracle.mha(..., ACC_F64) (the bound of
    test_ops_gpu.py::test_mha_decode_batch_pipeline_edges), device-position and host-position form, rows past the
    position NaN and the output finite; KH_ATTN_FENCED=1 bit-identical to the default;
  * seam probes - the under-read check.  A timestep dropped at position 9000 moves the output by 1e-4 of a V row,
    below any round-off bound, so one key is made dominant (score 20 against N(0, 1): the gold's largest probability
    must exceed 0.99) in turn at timestep 0, at pos, on both sides of every active split seam and at the first
    timestep of the last batch of the last split; different KV heads carry different probes in one launch.  The
    probed head's output is then that V row: a dropped or doubled timestep is an O(1) error.  The gold of a probed
    head is oracle.mha on that head alone (same arithmetic, 1 / heads of the cost);
  * the launch log holds exactly the instantiation and the variant record predicted from the plan.
After every configuration the ticket words of the workspace are zero.  ops.mha (k_mha with a score tensor, the
single-split decode kernel without) is checked at head sizes 132, 192 and 256, probabilities within 3e-6.

Model level (2-layer seeded models, scheme of test_decode_instantiations_gpu._run_shape): head size 256 fp32 and int8
(k_wo_comb at hsh = 6), head size 192 GQA (comb_supported false and, at 64 lanes, no group path: step variant 0 with
the in-launch merge of <64,0> at every position), head size 96 with kv_mul 4 and 80 with kv_mul 2 under
KH_ATTN_TLONG=300 (no deferral at these head sizes, so positions 256 ... 298 run step variant 2: the per-head-only
kernel although the group path is on - the `variant2` cell comes from these two), head size 32 (k_attn_generic).  Random K/V rows with a few x6 keys, then
teacher-forced steps at positions with 1, 2, 4, 5 and the maximum number of active splits: logits within max(floor,
3 x |oracle fp32 - gold|), K/V rows within 1e-5, argmax where the gold's margin allows (at most one step in ten may
skip it, asserted from the gold).  Whether a step defers its merge to k_wo_comb is predicted per step from the plan
(comb_supported, the flags, active splits against attn_defer_max: 16 where wo's staging hides the combine, else 4) and
must equal the launch record; a KH_ATTN_DEFER_MAX=4 twin moves the threshold between the 4- and the 5-split step.  The
KH_FLAG_ATTN_MERGE_IN_LAUNCH and KH_ATTN_DEFER_MAX=4 twins give bit-identical logits, a KH_ATTN_WG=256
twin stays within the bound, a 24-step graph run from position 250 equals the fused one, and multi-token KH_PREFILL
=gemv launches across position 256 and across t_long leave K/V rows bit-identical to token-by-token steps and within
1e-5 of the gold.

Gates: every k_attn_decode instantiation in the code objects was launched and checked (k_attn_generic and k_mha too),
and the variant table - per instantiation and width: single batch, several batches, 2-16 splits, capped split length,
fenced merge; for KVM > 0 the group path with 1, 2-16 and 17-32 splits and its fenced merge; quanta 64 / 128 / 256
per lane width; deferred, multi-token, variant 2 - has no missing cell.  UNREACHABLE lists the cells no geometry can
reach, with the reason.

Measured on an MI355X, worst |output - gold| of the operator-level checks per lane width (the largest are probed
heads, whose output is a V row of magnitude up to 4.5, so mostly the relative term): G = 16: 5.6e-5, G = 32: 5.5e-5,
G = 64: 5.0e-5 - all inside atol 3e-5 + rtol 2e-5 |gold|; no case needed a wider bound.  Module wall time: 17 s
(about 101 000 checked launches).
"""
import numpy as np
import pytest
import torch

import code_objects as co
from kuiperllama_amd import _ffi, binfmt, build
from test_decode_instantiations_gpu import KV_ATOL, LOGIT_ATOL_F32, LOGIT_ATOL_Q8

pytestmark = pytest.mark.gpu

SEQ = 9000          # beyond 16 quanta of 128 and 256 (capped split length), more than 16 group splits of 256
LAYER = 1           # the addressed layer of a two-layer cache; layer 0 holds NaN
ATOL, RTOL = 3e-5, 2e-5
PROB_ATOL = 3e-6
PROBE_SCORE = 20.0  # q.k / sqrt(hs) of a probe key; the other 9000 scores are N(0, 1): their mass is below 1e-4
BASE_SCORE = 6.0    # the base data's two dominant keys

GEOMETRIES = {  # lanes per timestep -> (heads, kv_heads, head size)
    16: [(6, 6, 48), (8, 4, 48), (8, 2, 48), (8, 8, 64), (8, 4, 64), (8, 2, 64), (14, 2, 64), (16, 2, 64), (9, 3, 64),
         (14, 2, 36)],  # 7 * 36 = 252: the one kv_mul-7 geometry whose group fits 256 threads
    32: [(4, 4, 128), (4, 2, 128), (8, 2, 128), (8, 4, 80), (8, 2, 96), (4, 2, 72)],
    64: [(4, 4, 256), (4, 2, 256), (4, 4, 192), (6, 2, 160), (3, 3, 132)],
}
ALL_GEOMETRIES = [g for G in GEOMETRIES for g in GEOMETRIES[G]]
POLICIES = (None, 64, 300)  # KH_ATTN_TLONG
TS_GEOMETRIES = {(8, 4, 64), (8, 4, 80), (4, 4, 256)}  # KH_ATTN_TS 64 / 128 / 256 (default policy: 4 KV heads)
# (KH_ATTN_TLONG, KH_ATTN_TS) on top: a KVM > 0 kernel runs the per-head path's capped split length only when t_long
# lies beyond 16 quanta, i.e. under the default threshold 4096 (>= 4 KV heads) or a hook pair like this one
EXTRA_CONFIGS = {(8, 2, 48): [(3000, 64)], (14, 2, 64): [(3000, 64)], (16, 2, 64): [(3000, 64)],
                 (8, 2, 128): [(3000, 64)], (14, 2, 36): [(3000, 64)]}
KVM_COMPILED = {16: (2, 4, 7, 8), 32: (2, 4), 64: ()}  # the test's own statement of attn_group_supported

_LAUNCHED = set()   # kernel names of checked launches
_CELLS = {}         # (instantiation | tag, width | None, cell) -> number of checked launches
_WORST = {}         # lanes per timestep -> worst |output - gold|
_DONE = set()       # tests that ran to the end (the gates need all of them)


def _lanes(hs):
    G = 1
    while G < hs // 4:
        G <<= 1
    return max(G, 16)


def _ts_shift(hs, ts):
    return {64: 6, 128: 7, 256: 8}[ts] if ts else (7 if hs >= 128 else 8)


def _group_on(heads, kvh, hs, wg, tlong):
    """Does the GQA group path run for this geometry, width and policy (csrc/kh_attn.h: attn_group_supported, attn_plan)?"""
    kv_mul = heads // kvh
    if kv_mul not in KVM_COMPILED[_lanes(hs)]:
        return False
    if kv_mul * hs > wg or kv_mul * 32 > wg:  # one thread per output element / per (head, merge slot)
        return False
    tl = tlong if tlong is not None else (4096 if kvh >= 4 else 0)
    return 0 < tl <= SEQ


def _close(got, gold):
    return np.abs(got - gold) <= ATOL + RTOL * np.abs(gold)


def _cell(inst, wg, cell):
    _CELLS[(inst, wg, cell)] = _CELLS.get((inst, wg, cell), 0) + 1


class _Geo:
    """One operator-level geometry: seeded data, device caches, golds (shared by all of its configurations)."""

    def __init__(self, gpu, oracle, heads, kvh, hs):
        self.gpu, self.oracle = gpu, oracle
        self.heads, self.kvh, self.hs = heads, kvh, hs
        self.kv_mul, self.kv_dim, self.dim, self.G = heads // kvh, kvh * hs, heads * hs, _lanes(hs)
        rng = np.random.default_rng(heads * 1000 + kvh * 100 + hs)
        self.k = rng.standard_normal((SEQ, self.kv_dim), dtype=np.float32)
        self.v = rng.standard_normal((SEQ, self.kv_dim), dtype=np.float32)
        self.q = rng.standard_normal(self.dim, dtype=np.float32)
        self.k[4500, :hs] = self.key(0, BASE_SCORE)                                # group 0, deep
        self.k[100, self.kv_dim - hs:] = self.key(heads - 1, BASE_SCORE)            # last group, shallow
        # per KV head: contiguous [SEQ, hs] copies for the single-head golds
        self.kg = [np.ascontiguousarray(self.k[:, g * hs:(g + 1) * hs]) for g in range(kvh)]
        self.vg = [np.ascontiguousarray(self.v[:, g * hs:(g + 1) * hs]) for g in range(kvh)]
        self.kbase = torch.from_numpy(self.k).to(gpu)
        self.vbase = torch.from_numpy(self.v).to(gpu)
        self.kw = torch.full((LAYER + 1, SEQ, self.kv_dim), float("nan"), device=gpu)
        self.vw = torch.full((LAYER + 1, SEQ, self.kv_dim), float("nan"), device=gpu)
        self.qd = torch.from_numpy(self.q).to(gpu)
        self.probe_keys = torch.from_numpy(np.stack([self.key(h, PROBE_SCORE) for h in range(heads)])).to(gpu)
        self._dpos, self._gold, self._gold_head, self._plan = {}, {}, {}, {}
        self.ws = None

    def key(self, h, score):
        """c * q_h / sqrt(hs / 64) with c such that q_h . key / sqrt(hs) = score."""
        qh = self.q[h * self.hs:(h + 1) * self.hs].astype(np.float64)
        return (qh * (score * np.sqrt(self.hs) / float(qh @ qh))).astype(np.float32)

    def dpos(self, pos):
        if pos not in self._dpos:
            self._dpos[pos] = torch.tensor([pos], dtype=torch.int32, device=self.gpu)
        return self._dpos[pos]

    def plan(self, pos):
        if pos not in self._plan:  # emptied when the hooks change (run_config)
            self._plan[pos] = _ffi.plan_attention(self.heads, self.kv_mul, self.hs, SEQ, pos)
        return self._plan[pos]

    def gold(self, pos):
        if pos not in self._gold:
            O = self.oracle
            self._gold[pos] = O.mha(pos, self.heads, 0, SEQ, self.kv_dim, self.kv_mul, self.hs, self.q, self.k[None],
                                    self.v[None], acc=O.ACC_F64)[0]
        return self._gold[pos]

    def gold_head(self, h, t, pos):
        """fp64 gold of head h alone with its probe key at timestep t: (output [hs], largest probability)."""
        if (h, t, pos) not in self._gold_head:
            O, hs, g = self.oracle, self.hs, h // self.kv_mul
            kg = self.kg[g]
            saved = kg[t].copy()
            kg[t] = self.key(h, PROBE_SCORE)
            out, score = O.mha(pos, 1, 0, SEQ, hs, 1, hs, self.q[h * hs:(h + 1) * hs], kg[None], self.vg[g][None],
                               acc=O.ACC_F64)
            kg[t] = saved
            self._gold_head[(h, t, pos)] = (out, float(score[0, :pos + 1].max()))
        return self._gold_head[(h, t, pos)]

    # ---- one configuration ---------------------------------------------------------------------------------------
    def positions(self, wg, ts_shift):
        """Tested positions of the current hook setting, from the plan (module docstring)."""
        step = (wg // self.G) * 4
        want = {0, 1, step - 1, step, step + 1, 254, 255, 256, SEQ - 1}
        key = lambda p: (p["group_path"], p["active_splits"])
        capped = lambda p, pos: pos + 1 > (p["ns_g"] << 8 if p["group_path"] else p["ns"] << ts_shift)
        p0 = self.plan(0)
        if p0["t_long"] <= SEQ:
            want |= {p0["t_long"] - 2, p0["t_long"] - 1}
        for NS, sh in ((p0["ns"], ts_shift), (p0["ns_g"], 8)):  # first position of the capped split length
            if 0 < (NS << sh) < SEQ:
                want.add(NS << sh)
        grid = list(range(0, SEQ, 32)) + [SEQ - 1]
        prev_pos, prev = 0, p0
        for pos in grid[1:]:
            cur = self.plan(pos)
            if key(cur) != key(prev):
                lo, hi = prev_pos, pos
                while hi - lo > 1:  # bisect to the change
                    mid = (lo + hi) // 2
                    if key(self.plan(mid)) == key(prev):
                        lo = mid
                    else:
                        hi = mid
                ph = self.plan(hi)
                if not capped(ph, hi) or ph["group_path"] != prev["group_path"]:
                    want |= {lo, hi}
            prev_pos, prev = pos, cur
        return sorted(p for p in want if 0 <= p < SEQ)

    def probes(self, pos, p, wg):
        step = (wg // self.G) * 4
        TS, nact = p["split_len"], p["active_splits"]
        ts = [0, pos]
        for s in range(1, nact):
            ts += [s * TS - 1, s * TS]
        t_begin = (nact - 1) * TS
        nb = -(-(pos + 1 - t_begin) // step)
        # first timestep of the last batch of the last split (its last is pos).  The group path's batch is the per-head
        # one today, TPI * KH_ATTN_UB = (wg / G) * 4 timesteps (attn_group_partial): revisit if that changes
        ts.append(t_begin + (nb - 1) * step)
        assert all(0 <= t <= pos for t in ts), (pos, p, ts)
        return list(dict.fromkeys(ts))

    def expect(self, pos, p, wg, ts_shift, form, group_on, fenced):
        """(instantiation, variant record) the launch must log."""
        grp = group_on and not (form == "host" and pos + 1 < p["t_long"])
        inst = f"k_attn_decode<{self.G},{self.kv_mul if grp else 0}>"
        return inst, f"attn_launch<{wg},{ts_shift},0,{int(fenced)},0,{int(grp)}>"

    def launch(self, pos, form, out, fenced=False):
        from kuiperllama_amd import ops
        if fenced:
            _ffi.debug_set("KH_ATTN_FENCED", "1")
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        try:
            ops.mha_decode(self.dpos(pos) if form == "dev" else pos, self.heads, LAYER, SEQ, self.kv_dim, self.kv_mul,
                           self.hs, out, self.qd, self.kw, self.vw, self.ws)
            return _ffi.launch_log()
        finally:
            if fenced:
                _ffi.debug_set("KH_ATTN_FENCED", None)

    def record(self, inst, pos, p, wg, ts_shift, fenced):
        step = (wg // self.G) * 4
        nT, nact, TS = pos + 1, p["active_splits"], p["split_len"]
        if p["group_path"]:
            _cell(inst, wg, "group:1" if nact == 1 else "group:2-16" if nact <= 16 else "group:17-32")
            if fenced and nact > 1:
                _cell(inst, wg, "group:fenced")
            return
        if nact == 1 and nT <= step:
            _cell(inst, wg, "head:single-batch")
        if min(TS, nT) > step:
            _cell(inst, wg, "head:multi-batch")
        if 2 <= nact <= 16:
            _cell(inst, wg, "head:splits2-16")
            if fenced:
                _cell(inst, wg, "head:fenced")
        if nT > (p["ns"] << ts_shift):
            _cell(inst, wg, "head:capped")
        elif nact >= 2:  # splits of one quantum each
            assert TS == 1 << ts_shift, (pos, p, ts_shift)
            _cell(f"G{self.G}", None, f"quantum{TS}")

    def run_config(self, wg, tlong, ts):
        from kuiperllama_amd import ops
        heads, kvh, hs, kv_mul = self.heads, self.kvh, self.hs, self.kv_mul
        what0 = f"({heads},{kvh},{hs}) wg {wg} t_long {tlong} ts {ts}"
        _ffi.debug_set("KH_ATTN_WG", str(wg))
        _ffi.debug_set("KH_ATTN_TLONG", None if tlong is None else str(tlong))
        _ffi.debug_set("KH_ATTN_TS", None if ts is None else str(ts))
        self._plan = {}
        ts_shift = _ts_shift(hs, ts)
        group_on = _group_on(heads, kvh, hs, wg, tlong)
        p0 = self.plan(0)
        assert (p0["ns_g"] > 0) == group_on, f"{what0}: plan {p0}, group path expected {group_on}"
        self.ws = ops.mha_decode_workspace(heads, hs, SEQ, self.gpu)
        assert self.ws is not None
        positions = self.positions(wg, ts_shift)
        if group_on:
            assert any(self.plan(pos)["group_path"] and self.plan(pos)["active_splits"] >= 17 for pos in positions), what0
        self.kw[LAYER].copy_(self.kbase)
        self.vw[LAYER].copy_(self.vbase)
        nan_from = SEQ
        n_launch = 0
        for pos in reversed(positions):
            self.kw[LAYER, pos + 1:nan_from] = float("nan")
            self.vw[LAYER, pos + 1:nan_from] = float("nan")
            nan_from = pos + 1
            p = self.plan(pos)
            what = f"{what0} pos {pos}"
            # ---- base data: device form, host form, fenced ----------------------------------------------------------
            outs = torch.full((3, self.dim), float("nan"), device=self.gpu)
            for i, (form, fenced) in enumerate((("dev", False), ("host", False), ("dev", True))):
                log = self.launch(pos, form, outs[i], fenced)
                inst, var = self.expect(pos, p, wg, ts_shift, form, group_on, fenced)
                assert log == {inst, var}, f"{what} {form}: log {sorted(log)}, predicted {[inst, var]}"
                if p["group_path"]:
                    assert inst.endswith(f",{kv_mul}>"), what
                _LAUNCHED.add(inst)
                self.record(inst, pos, p, wg, ts_shift, fenced)
            got = outs.cpu().numpy()
            gold = self.gold(pos)
            for i, form in enumerate(("dev", "host")):
                assert np.isfinite(got[i]).all(), f"{what} {form}: a row past the position reached the result"
                err = np.abs(got[i] - gold)
                _WORST[self.G] = max(_WORST.get(self.G, 0.0), float(err.max()))
                assert _close(got[i], gold).all(), f"{what} {form}: |out - gold| {err.max():.3e}"
            assert np.array_equal(got[2], got[0]), f"{what}: the fenced merge differs from the default"
            # ---- seam probes: kvh of them per launch, one per KV head -----------------------------------------------
            pr = self.probes(pos, p, wg)
            nl = -(-len(pr) // kvh)
            outs = torch.full((nl, self.dim), float("nan"), device=self.gpu)
            placed = []
            for i in range(nl):
                mine = [(g, (g + i) % kv_mul + g * kv_mul, t) for g, t in enumerate(pr[i * kvh:(i + 1) * kvh])]
                for g, h, t in mine:
                    self.kw[LAYER, t, g * hs:(g + 1) * hs] = self.probe_keys[h]
                form = "host" if i & 1 else "dev"
                log = self.launch(pos, form, outs[i])
                inst, var = self.expect(pos, p, wg, ts_shift, form, group_on, False)
                assert log == {inst, var}, f"{what} probe launch {i} {form}: log {sorted(log)}, predicted {[inst, var]}"
                for g, h, t in mine:
                    self.kw[LAYER, t, g * hs:(g + 1) * hs] = self.kbase[t, g * hs:(g + 1) * hs]
                placed.append(mine)
            got = outs.cpu().numpy()
            assert np.isfinite(got).all(), f"{what}: a probe launch read a row past the position"
            for i, mine in enumerate(placed):
                for g, h, t in mine:
                    gh, pmax = self.gold_head(h, t, pos)
                    assert pmax > 0.99, f"{what}: probe at {t} has probability {pmax} in the gold"
                    o = got[i, h * hs:(h + 1) * hs]
                    err = np.abs(o - gh)
                    _WORST[self.G] = max(_WORST.get(self.G, 0.0), float(err.max()))
                    assert _close(o, gh).all(), \
                        f"{what}: head {h} with the dominant key at timestep {t} (plan {p}): |out - gold| {err.max():.3e}"
            n_launch += 3 + nl
        tickets = self.ws[: ((heads + 3) & ~3) * 4].view(torch.int32)
        assert int(tickets.abs().sum().item()) == 0, f"{what0}: tickets not re-armed"
        return len(positions), n_launch


def _clear_hooks():
    for k in ("KH_ATTN_WG", "KH_ATTN_TLONG", "KH_ATTN_TS", "KH_ATTN_FENCED", "KH_LAUNCH_LOG", "KH_PREFILL",
              "KH_ATTN_DEFER_MAX"):
        _ffi.debug_set(k, None)


def _configs(geo):
    out = []
    for wg in (256, 512):
        for tlong in POLICIES:
            out.append((wg, tlong, None))
        if geo in TS_GEOMETRIES:
            out += [(wg, None, ts) for ts in (64, 128, 256)]
        out += [(wg, tl, ts) for tl, ts in EXTRA_CONFIGS.get(geo, [])]
    return out


@pytest.mark.parametrize("heads,kvh,hs", ALL_GEOMETRIES)
def test_operator_geometry(gpu, oracle, heads, kvh, hs):
    """ops.mha_decode of one geometry under every width, path policy and quantum against the fp64 gold, with seam
    probes, fenced twin, ticket and launch-log checks (module docstring)."""
    geo = _Geo(gpu, oracle, heads, kvh, hs)
    npos = nl = 0
    try:
        for wg, tlong, ts in _configs((heads, kvh, hs)):
            a, b = geo.run_config(wg, tlong, ts)
            npos, nl = npos + a, nl + b
    finally:
        _clear_hooks()
    _DONE.add(("operator", heads, kvh, hs))
    print(f"({heads},{kvh},{hs}): {len(_configs((heads, kvh, hs)))} configurations, {npos} positions, {nl} launches, "
          f"worst |out - gold| at G = {geo.G} so far {_WORST[geo.G]:.3e}")


@pytest.mark.parametrize("heads,kvh,hs", [(3, 3, 132), (4, 2, 192), (4, 4, 256)])
def test_mha_large_heads(gpu, oracle, heads, kvh, hs):
    """ops.mha at 64 lanes per timestep: k_mha (attn_head_decode, probabilities left in the score tensor, one and two
    LDS score chunks) and, without a score tensor, the single-split decode kernel."""
    from kuiperllama_amd import ops
    seq = 2500
    rng = np.random.default_rng(heads * 10 + hs)
    kv_dim, kv_mul, dim = kvh * hs, heads // kvh, heads * hs
    kc = rng.standard_normal((2, seq, kv_dim), dtype=np.float32)
    vc = rng.standard_normal((2, seq, kv_dim), dtype=np.float32)
    q = rng.standard_normal(dim, dtype=np.float32)
    kc[1, 2100, :hs] = q[:hs] * (BASE_SCORE * np.sqrt(hs) / float(q[:hs] @ q[:hs]))
    kcd, vcd, qd = (torch.from_numpy(a).to(gpu) for a in (kc, vc, q))
    try:
        for pos in (0, 1, 15, 16, 255, 256, 2047, 2048, 2100, seq - 1):
            kp, vp = kcd.clone(), vcd.clone()
            kp[:, pos + 1:] = float("nan")
            vp[:, pos + 1:] = float("nan")
            oo, so = oracle.mha(pos, heads, 1, seq, kv_dim, kv_mul, hs, q, kc, vc, acc=oracle.ACC_F64)
            for score in (torch.zeros(heads, seq, device=gpu), None):
                out = torch.full((dim,), float("nan"), device=gpu)
                _ffi.debug_set("KH_LAUNCH_LOG", "1")
                ops.mha(pos if pos & 1 else torch.tensor([pos], dtype=torch.int32, device=gpu), heads, 1, seq, kv_dim,
                        kv_mul, hs, out, qd, score, kp, vp)
                log = _ffi.launch_log()
                want = {"k_mha"} if score is not None else {"k_attn_decode<64,0>", "attn_launch<512,7,0,0,0,0>"}
                assert log == want, f"hs {hs} pos {pos}: log {sorted(log)}"
                got = out.cpu().numpy()
                what = f"({heads},{kvh},{hs}) pos {pos} {'k_mha' if score is not None else 'decode kernel'}"
                assert np.isfinite(got).all(), what
                assert _close(got, oo).all(), f"{what}: |out - gold| {np.abs(got - oo).max():.3e}"
                if score is not None:
                    pe = np.abs(score.cpu().numpy()[:, :pos + 1] - so[:, :pos + 1]).max()
                    assert pe <= PROB_ATOL, f"{what}: probabilities off by {pe:.3e}"
                _LAUNCHED.update(k for k in log if not k.startswith("attn_launch"))
    finally:
        _clear_hooks()
    _DONE.add(("mha", heads, kvh, hs))


# ---------------------------------------------------------------------------------------------------- model level
def _mspec(dim, hidden, heads, kv_heads, vocab, cache, quant, name):
    return binfmt.ModelSpec(dim, hidden, 2, heads, kv_heads, vocab, cache, False, binfmt.FAMILY_LLAMA, quant, 64,
                            binfmt.ROPE_HALF, 10000.0, 1e-5, name)


MODELS = {  # name -> (spec, KH_ATTN_TLONG, image seed)
    "f32-hs256": (_mspec(1024, 2048, 4, 4, 777, 2048, False, "attn-hs256"), None, 4242),        # k_wo_comb at hsh = 6
    "q8-hs256": (_mspec(1024, 2048, 4, 4, 777, 2048, True, "attn-q8-hs256"), None, 4242),
    "f32-hs192-gqa": (_mspec(768, 1536, 4, 2, 1001, 2048, False, "attn-hs192"), None, 4242),    # comb_supported false
    "f32-hs96-kvm4": (_mspec(768, 1536, 8, 2, 1001, 4096, False, "attn-hs96"), 300, 4242),      # masked lanes, <32,4>
    "f32-hs80-kvm2": (_mspec(640, 1280, 8, 4, 999, 4096, False, "attn-hs80"), 300, 4242),       # masked lanes, <32,2>
    "f32-hs32": (_mspec(256, 512, 8, 4, 501, 1024, False, "attn-hs32"), None, 4242),            # k_attn_generic
}
SPLIT_TARGETS = (1, 2, 3, 4, 5)  # active splits of the checked steps, plus the largest count of each path; 4 and 5
                                 # straddle the default attn_defer_max of 4 (quantum 128 has no position with 2)


def _model_plan(spec, pos):
    return _ffi.plan_attention(spec.n_heads, spec.kv_mul, spec.head_size, spec.seq_len, pos)


def _model_steps(spec, rng):
    """[(token, pos)]: the first position of every (path, active splits) in SPLIT_TARGETS and of each path's largest
    count, from the plan; plus position 0, both sides of pos + 1 = 257 and the last but one row."""
    first = {}
    for pos in range(spec.seq_len - 1):
        p = _model_plan(spec, pos)
        first.setdefault((p["group_path"], p["active_splits"]), pos)
    want = {0, 255, 256, spec.seq_len - 2}
    for path in (0, 1):
        counts = [n for (g, n) in first if g == path]
        for n in counts:
            if n in SPLIT_TARGETS or n == max(counts):
                want.add(first[(path, n)])
    return [(int(rng.integers(0, spec.vocab_size)), pos) for pos in sorted(want)]


def _rand_rows(spec, rng, n):
    kr = rng.standard_normal((spec.n_layers, n, spec.kv_dim), dtype=np.float32)
    vr = rng.standard_normal((spec.n_layers, n, spec.kv_dim), dtype=np.float32)
    kr[:, rng.integers(0, n, 12)] *= 6.0  # a few dominant keys: the splits' maxima differ
    return kr, vr


def _oracle_pair(oracle, img_h, spec, rows):
    out = []
    for _ in range(2):
        om = oracle.OracleModel.from_spec(img_h, spec, cache_len=spec.seq_len)
        ko, vo = om.kv_cache()
        ko[:, :rows[0].shape[1]] = rows[0]
        vo[:, :rows[0].shape[1]] = rows[1]
        out.append(om)
    return out


def _model_gold(oracle, img_h, spec, steps, rows):
    """[(logits fp64, logits fp32, K rows [L, kv], V rows)] of the steps, each over the random rows alone."""
    g, o = _oracle_pair(oracle, img_h, spec, rows)
    out = []
    for tok, pos in steps:
        lg = g.forward(tok, pos, oracle.ACC_F64)
        lo = o.forward(tok, pos)
        ko, vo = g.kv_cache()
        out.append((lg, lo, ko[:, pos].copy(), vo[:, pos].copy()))
        for om in (g, o):  # back to the random row: the steps do not depend on each other
            k2, v2 = om.kv_cache()
            k2[:, pos] = rows[0][:, pos]
            v2[:, pos] = rows[1][:, pos]
    g.close()
    o.close()
    return out


def _write_rows(m, spec, rows, r0=0, r1=None):
    for layer in range(spec.n_layers):
        m.write_kv(layer, r0, rows[0][layer, r0:r1], rows[1][layer, r0:r1])


def _attn_log():
    log = _ffi.launch_log()
    return ({k for k in log if k.startswith(("k_attn", "k_mha"))},
            [tuple(int(x) for x in k[len("attn_launch<"):-1].split(",")) for k in log if k.startswith("attn_launch<")])


def _defer_expected(spec, p, pos, flags, defer_max_hook):
    """Does the step at pos leave its split partials to k_wo_comb (kh_model_load.hip: attn_defer, attn_defer_max;
    kh_model_step.hip: step_variant)?  From the plans alone."""
    hs, dim, heads = spec.head_size, spec.dim, spec.n_heads
    wo = _ffi.plan_decode_shapes(dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, spec.quant)["wo"]
    comb = hs > 32 and hs & (hs - 1) == 0 and dim == heads * hs and dim <= 16 * wo["wg"] and heads * 16 <= 4 * wo["wg"]
    if not comb or p["ns"] <= 1 or flags & _ffi.KH_FLAG_ATTN_MERGE_IN_LAUNCH:
        return False
    if pos < 256 or pos + 1 >= p["t_long"]:
        return False
    mv = 2 if dim <= 8 * wo["wg"] else 4
    overlap = not (wo["u"] >= 8 or (spec.quant and wo["u"] >= 4 and mv >= 4))
    return p["active_splits"] <= (defer_max_hook or (16 if overlap else 4))


def _run_model_steps(m, spec, steps, rows, gold, floor, what, wg, flags=0, defer_max_hook=None):
    """Teacher-forced steps (scheme of test_decode_instantiations_gpu._run_shape); returns the logits per step."""
    G = _lanes(spec.head_size)
    nan = np.full((1, spec.kv_dim), np.nan, np.float32)
    res = []
    for (tok, pos), (lg, lo, kg, vg) in zip(steps, gold):
        for layer in range(spec.n_layers):
            m.write_kv(layer, pos, nan, nan)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        nxt = m.predict(tok, pos, exec="fused")
        kernels, variants = _attn_log()
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        got = m.logits()
        err = float(np.abs(got - lg).max())
        lim = max(floor, 3.0 * float(np.abs(lo - lg).max()))
        assert err <= lim, f"{what} pos {pos}: |logit - gold| {err:.3e} > {lim:.3e}"
        top2 = np.sort(lg)[-2:]
        if top2[1] - top2[0] > 2 * floor:
            assert nxt == int(np.argmax(lg)), f"{what} pos {pos}: argmax {nxt} vs gold {int(np.argmax(lg))}"
        for layer in range(spec.n_layers):
            k, v = m.read_kv(layer, pos, 1)
            for name, a, b in (("K", k[0], kg[layer]), ("V", v[0], vg[layer])):
                e = np.abs(a - b)
                assert np.all(e <= KV_ATOL), f"{what} pos {pos} layer {layer}: {name} row off ({int(np.isnan(a).sum())} NaN)"
        _write_rows(m, spec, rows, pos, pos + 1)
        # what the attention launch was, against the plan
        p = _model_plan(spec, pos)
        if spec.head_size <= 32:
            assert kernels == {"k_attn_generic"} and not variants, f"{what} pos {pos}: {kernels} {variants}"
        else:
            assert len(kernels) == 1 and len(variants) == 1, f"{what} pos {pos}: {kernels} {variants}"
            lwg, _, defer, _, ntok, grp = variants[0]
            inst = next(iter(kernels))
            between = pos >= 256 and pos + 1 < p["t_long"]  # step variants 1 / 2: per-head-only instantiation
            kvm = spec.kv_mul if p["ns_g"] > 0 and not between else 0
            assert inst == f"k_attn_decode<{G},{kvm}>" and lwg == wg and ntok == 0 and grp == int(kvm > 0), \
                f"{what} pos {pos}: {inst} {variants[0]}, plan {p}"
            want_defer = _defer_expected(spec, p, pos, flags, defer_max_hook)
            assert bool(defer) == want_defer, \
                f"{what} pos {pos}: deferred {defer}, predicted {want_defer} ({p['active_splits']} active splits)"
            if defer:
                _cell("model", None, f"deferred:hs{spec.head_size}")
            elif between and p["ns_g"] > 0:
                _cell("model", None, "variant2")
        _LAUNCHED.update(kernels)
        res.append((got, defer if spec.head_size > 32 else 0))
    return res


@pytest.mark.parametrize("name", list(MODELS))
def test_model(gpu, oracle, name):
    """Model-level paths no operator entry reaches (module docstring)."""
    from kuiperllama_amd.model import KuiperModel
    spec, tlong, seed = MODELS[name]
    floor = LOGIT_ATOL_Q8 if spec.quant else LOGIT_ATOL_F32
    hs = spec.head_size
    try:
        _ffi.debug_set("KH_ATTN_TLONG", None if tlong is None else str(tlong))
        img_d = binfmt.synth_image(spec, seed=seed, device=gpu, final_norm_std=1.0)
        torch.cuda.synchronize()
        img_h = img_d.cpu().numpy()
        rng = np.random.default_rng(11)
        steps = _model_steps(spec, rng)
        rows = _rand_rows(spec, rng, spec.seq_len)
        gold = _model_gold(oracle, img_h, spec, steps, rows)
        skipped = sum(1 for lg, _, _, _ in gold if np.sort(lg)[-1] - np.sort(lg)[-2] <= 2 * floor)
        assert skipped * 10 <= len(steps), f"{name}: {skipped} of {len(steps)} steps have no argmax margin in the gold"
        main = None
        for twin, flags, wg, dmax in (("default", 0, 512, None),
                                      ("merge-in-launch", _ffi.KH_FLAG_ATTN_MERGE_IN_LAUNCH, 512, None),
                                      ("defer-max-4", 0, 512, 4), ("wg256", 0, 256, None)):
            _ffi.debug_set("KH_ATTN_WG", str(wg) if wg != 512 else None)
            _ffi.debug_set("KH_ATTN_DEFER_MAX", None if dmax is None else str(dmax))
            m = KuiperModel.from_device_image(img_d, spec, flags=flags)
            try:
                _write_rows(m, spec, rows)
                res = _run_model_steps(m, spec, steps, rows, gold, floor, f"{name} {twin}", wg, flags, dmax)
                if twin == "default":
                    main = res
                    _model_extras(m, oracle, img_h, spec, rows, name, rng)
                elif twin in ("merge-in-launch", "defer-max-4"):
                    if twin == "merge-in-launch":
                        assert not any(d for _, d in res), f"{name}: the merge-in-launch twin deferred"
                    for (tok, pos), (la, _), (lb, _) in zip(steps, main, res):
                        assert np.array_equal(la, lb), f"{name} pos {pos}: {twin} logits differ from the default's"
            finally:
                m.close()
    finally:
        _clear_hooks()
    _DONE.add(("model", name))
    print(f"{name}: steps at {[p for _, p in steps]} (active splits "
          f"{[_model_plan(spec, p)['active_splits'] for _, p in steps]})")


def _model_extras(m, oracle, img_h, spec, rows, name, rng):
    """Graph replay across position 256, and the multi-token launches."""
    # ---- 24 sampled steps from position 250: graph == fused ---------------------------------------------------------
    prompt = [int(t) for t in rng.integers(0, spec.vocab_size, 251)]
    ga, _ = m.generate(prompt, 274, exec="graph")
    gf, _ = m.generate(prompt, 274, exec="fused")
    assert len(gf) > 251 and ga == gf, f"{name}: graph replay differs from the fused steps"
    # ---- multi-token launches (B-token prefill): a segment across position 256, one across t_long --------------------
    t_long = _model_plan(spec, 0)["t_long"]
    segs = [250] + ([t_long - 6] if t_long < spec.seq_len - 16 else [])
    for pos0 in segs:
        n = 12
        toks = [int(t) for t in rng.integers(0, spec.vocab_size, n)]
        _write_rows(m, spec, rows)
        nanr = np.full((n, spec.kv_dim), np.nan, np.float32)
        for layer in range(spec.n_layers):
            m.write_kv(layer, pos0, nanr, nanr)
        _ffi.debug_set("KH_PREFILL", "gemv")
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        try:
            m.prefill(toks, pos0)
            kernels, variants = _attn_log()
        except _ffi.KhError as e:
            assert e.code == -2, e  # KH_ERR_UNSUPPORTED: outside prefill_supported (the gate wants G = 32 and 64 runs)
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            _write_rows(m, spec, rows)
            return
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        assert variants and all(v[4] == 1 and v[2] == 0 for v in variants), f"{name}: {variants}"
        # host-positioned launches, one per chunk of tokens: a chunk whose last position stays below t_long - 1 runs
        # the per-head-only kernel, one that reaches it the kernel that carries the group path (launch_attn_decode)
        G = _lanes(spec.head_size)
        p = _model_plan(spec, pos0)
        crosses = p["ns_g"] > 0 and pos0 + n >= p["t_long"]
        with_group = f"k_attn_decode<{G},{spec.kv_mul}>"
        allowed = {f"k_attn_decode<{G},0>"} | ({with_group} if crosses else set())
        assert kernels <= allowed and (not crosses or with_group in kernels), \
            f"{name} segment {pos0}: launched {sorted(kernels)}, plan {p}"
        assert {v[5] for v in variants} == {int(k == with_group) for k in kernels}, f"{name}: {variants} {kernels}"
        _LAUNCHED.update(kernels)
        for k in kernels:
            _cell("model", None, f"multi-token:{k}")
        _cell("model", None, f"multi-token:G{G}")
        pf = [m.read_kv(layer, pos0, n) for layer in range(spec.n_layers)]
        # token by token from the same rows
        _write_rows(m, spec, rows)
        for i, t in enumerate(toks):
            m.predict(t, pos0 + i, is_prompt=True, exec="fused")
        for layer in range(spec.n_layers):
            k, v = m.read_kv(layer, pos0, n)
            assert np.array_equal(k, pf[layer][0]) and np.array_equal(v, pf[layer][1]), \
                f"{name} segment {pos0}: multi-token K/V rows differ from token-by-token, layer {layer}"
        # and against the fp64 gold (bit-identity alone compares the kernel with itself)
        g = oracle.OracleModel.from_spec(img_h, spec, cache_len=spec.seq_len)
        ko, vo = g.kv_cache()
        ko[:] = rows[0]
        vo[:] = rows[1]
        for i, t in enumerate(toks):
            g.forward(t, pos0 + i, oracle.ACC_F64)
        for layer in range(spec.n_layers):
            for nm, a, b in (("K", pf[layer][0], ko[layer, pos0:pos0 + n]), ("V", pf[layer][1], vo[layer, pos0:pos0 + n])):
                e = np.abs(a - b)
                assert np.all(e <= KV_ATOL), f"{name} segment {pos0} layer {layer}: {nm} rows off by {np.nanmax(e):.3e}"
        g.close()
    _write_rows(m, spec, rows)


# ---------------------------------------------------------------------------------------------------------- gates
HEAD_CELLS = ("head:single-batch", "head:multi-batch", "head:splits2-16", "head:capped", "head:fenced")
GROUP_CELLS = ("group:1", "group:2-16", "group:17-32", "group:fenced")


def _unreachable(inst, wg, cell):
    """Reason why no geometry can reach a cell of the variant table, or None."""
    if inst.startswith("k_attn_decode<"):
        G, kvm = (int(x) for x in inst[len("k_attn_decode<"):-1].split(","))
        min_hs = {16: 36, 32: 68, 64: 132}[G]  # smallest head size of the lane width
        if kvm > 0 and wg is not None and kvm * min_hs > wg:
            return f"the group's {kvm} x {min_hs}+ outputs do not fit {wg} threads: attn_group_supported refuses it"
    return None


def _required(compiled):
    req = []
    for inst in sorted(compiled):
        kvm = int(inst[:-1].split(",")[1])
        for wg in (256, 512):
            req += [(inst, wg, c) for c in HEAD_CELLS + (GROUP_CELLS if kvm > 0 else ())]
    for G in (16, 32, 64):
        req += [(f"G{G}", None, f"quantum{ts}") for ts in (64, 128, 256)]
    req += [("model", None, c) for c in ("deferred:hs256", "multi-token:G32", "multi-token:G64", "variant2")]
    return req


@pytest.fixture(scope="module")
def compiled():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    return co.kernels(co.code_object_notes(_ffi.LIB_PATH), {"k_attn_decode", "k_attn_generic", "k_mha"})


def _all_ran():
    want = {("operator",) + g for g in ALL_GEOMETRIES} | {("model", n) for n in MODELS} | \
        {("mha", 3, 3, 132), ("mha", 4, 2, 192), ("mha", 4, 4, 256)}
    missing = sorted(map(str, want - _DONE))
    assert not missing, f"tests that did not run to the end (run the whole module): {missing}"


def test_coverage_gate(gpu, compiled):
    """Every compiled k_attn_decode instantiation, k_attn_generic and k_mha were launched and checked, and nothing
    launched is missing from the code objects."""
    _all_ran()
    assert {"k_attn_generic", "k_mha"} <= compiled, sorted(compiled)
    decode = {k for k in compiled if k.startswith("k_attn_decode<")}
    assert decode, "no k_attn_decode instantiation in the library"
    assert _LAUNCHED <= compiled, f"launched but not found in the code objects: {sorted(_LAUNCHED - compiled)}"
    for stem in ("k_attn_decode", "k_attn_generic", "k_mha"):
        comp = {k for k in compiled if k.split("<")[0] == stem}
        seen = {k for k in _LAUNCHED if k.split("<")[0] == stem}
        print(f"{stem}: {len(seen)} of {len(comp)} compiled instantiations launched and checked")
    print("worst |output - gold| of the operator-level checks per lane width: " +
          ", ".join(f"G = {G}: {_WORST.get(G, float('nan')):.3e}" for G in (16, 32, 64)))
    gap = compiled - _LAUNCHED
    assert not gap, f"compiled and never launched: {sorted(gap)}"


def test_variant_gate(gpu, compiled):
    """The variant table (module docstring) has no missing cell; a cell listed unreachable was not reached."""
    _all_ran()
    missing, lines = [], []
    for inst, wg, cell in _required({k for k in compiled if k.startswith("k_attn_decode<")}):
        n = _CELLS.get((inst, wg, cell), 0)
        why = _unreachable(inst, wg, cell)
        lines.append(f"  {inst:22s} {'wg ' + str(wg) if wg else '      ':7s} {cell:20s} "
                     f"{'UNREACHABLE: ' + why if why else str(n) + ' checked launches'}")
        if why:
            assert n == 0, f"{inst} wg {wg} {cell}: documented unreachable ({why}) but reached {n} times"
        elif n == 0:
            missing.append(f"{inst} wg {wg} {cell}")
    print("variant table:\n" + "\n".join(lines))
    assert not missing, f"variant cells never launched: {missing}"
