"""The wide sequence pass on the GPU: kh_model_seq_step_gemm / kh_model_generate_batch_gemm / kh_model_seq_gemm_logits
(csrc/kh_seq_gemm.h: k_sg_embed, k_sg_gemm, k_sg_rope; csrc/kh_model_gemm.hip).

The contract is kh_model_prefill_gemm's, not the bit-exact one of the 8-lane pass: K/V rows and logits are held to the
project's tolerances against the CPU ORACLE fed the same tokens one by one (KV_ATOL_GEMM 5e-6, int8 4x; LOGIT_ATOL
2e-5 / 5e-5), and every pick is an EXACT function of the pass's own logits (kh_model_seq_gemm_logits): compared as
integers and raw bits.  Geometries, layout (2048 cache rows: three slots of 300 rows, 61 of 8) and the loop case are
tests/seq_gemm_cases.py; the histories are written with seq_prefill, which is bit-exact.

Worst errors against the oracle measured on an MI355X, single passes of 1 / 15 / 16 / 17 / 64 lanes and the forced
tiles (test_single_passes prints them as "worst[...]"; DESIGN 3.3h repeats them), all inside the shallow bounds:
    geometry     K/V rows (bound)     logits (bound)
    mha-inter    1.37e-6 (5e-6)       1.88e-6 (2e-5)
    gqa-half     1.73e-6 (5e-6)       2.62e-6 (2e-5)
    half-hs48    1.43e-6 (5e-6)       1.67e-6 (2e-5)
    qwen-bias    1.55e-6 (5e-6)       1.97e-6 (2e-5)
    int8         1.85e-6 (2e-5)       1.92e-6 (5e-5)"""
import ctypes as C

import numpy as np
import pytest
import torch

import code_objects as co
import seq_gemm_cases as G
from kuiperllama_amd import _ffi, build, ops
from kuiperllama_amd.model import KuiperModel

pytestmark = pytest.mark.gpu

STEMS = {"k_sg_gemm", "k_sg_embed", "k_sg_rope"}
NEW_PREFIX = "k_sg_"
_LAUNCHED = set()  # what the passes whose results were compared launched (the gate at the end reads it)
_WORST = {}
SAMP = {"temperature": 0.8, "top_k": 50, "top_p": 0.95}
HOOKS = ("KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU", "KH_PG_SHAPE_STORE")


@pytest.fixture(autouse=True)
def _clean_hooks():
    try:
        yield
    finally:
        for k in HOOKS + ("KH_LAUNCH_LOG",):
            _ffi.debug_set(k, None)


class Ref:
    """the oracle, fed every slot's text token by token: logits and K/V row (per layer) of the slot's lane position"""

    def __init__(self, oracle, name):
        self.spec = spec = G.SPECS[name]
        self.T = G.texts(spec)
        om = oracle.OracleModel.from_spec(G.host_image(spec), spec, cache_len=G.LONG)
        self.logits, self.k, self.v = [], [], []
        for text in self.T:
            self.add(om, text)
        self.om = om

    def add(self, om, text):
        for p, t in enumerate(text):
            lg = om.forward(t, p)
        ko, vo = om.kv_cache()
        self.logits.append(lg.copy())
        self.k.append(ko[:, len(text) - 1].copy())
        self.v.append(vo[:, len(text) - 1].copy())


_REF = {}


def _ref(oracle, name):
    if name not in _REF:
        _REF[name] = Ref(oracle, name)
    return _REF[name]


def _model(spec, lens=G.LENS):
    m = KuiperModel.from_host_image(G.host_image(spec), spec, max_seq_len=spec.seq_len)
    m.seq_slots_var(lens)
    return m


def _fill(m, ref, slots):
    for s in slots:
        if G.lane_pos(s) > 0:
            m.seq_prefill(s, ref.T[s][:G.lane_pos(s)])


def _slots(n, seed):
    """n distinct slots in shuffled order: the long slots first in the draw (n = 1: the one at position 256), then
    short ones from slot 3 (position 0) on"""
    pick = [1] if n == 1 else [0, 1, 2] + list(range(3, n))
    return [int(s) for s in np.random.default_rng(seed).permutation(pick)]


def _rope_kernel(spec, T):
    """does k_sg_rope follow the QKV GEMM of a T-lane pass?  Not where its epilogue rotates: interleaved pairs always,
    half mode when the head size is a multiple of 32 and the planned tile has the partner rows in the wave (R = 2)"""
    if spec.rope_mode == G.INTER:
        return False
    out = (C.c_int32 * 7)()
    r2 = spec.dim % 32 == 0 and spec.kv_dim % 32 == 0
    assert _ffi.lib().kh_plan_prefill_shape(0, T, spec.dim + 2 * spec.kv_dim, spec.dim, int(spec.quant), int(r2), out) == 0
    return spec.head_size % 32 != 0 or out[0] != 2


def _read_all(m, spec):
    return [m.read_kv(layer, 0, spec.seq_len) for layer in range(spec.n_layers)]


def _pass(m, ref, slots, what, pos=None, toks=None, ref_ix=None, **kw):
    """one wide pass against the oracle: the lanes' K/V rows (poisoned first) and logits within the tolerances, every
    other row of the cache byte-identical; returns (picks, launch log, the lanes' logits rows)"""
    spec = ref.spec
    pos = [G.lane_pos(s) for s in slots] if pos is None else pos
    toks = [ref.T[s][-1] for s in slots] if toks is None else toks
    ref_ix = slots if ref_ix is None else ref_ix
    rows = [m.seq_row(s, p) for s, p in zip(slots, pos)]
    poison = np.full((1, spec.kv_dim), np.nan, np.float32)
    for layer in range(spec.n_layers):
        for r in rows:
            m.write_kv(layer, r, poison, poison)
    before = _read_all(m, spec)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    got = m.seq_step(slots, toks, pos, gemm=True, **kw)
    log = set(_ffi.launch_log())
    _ffi.debug_set("KH_LAUNCH_LOG", None)
    after = _read_all(m, spec)
    other = np.ones(spec.seq_len, bool)
    other[rows] = False
    worst_kv = worst_lg = 0.0
    for layer in range(spec.n_layers):
        k, v = after[layer]
        for i, r in enumerate(rows):
            ek = np.abs(k[r] - ref.k[ref_ix[i]][layer]).max()
            ev = np.abs(v[r] - ref.v[ref_ix[i]][layer]).max()
            worst_kv = max(worst_kv, float(ek), float(ev))
            assert ek <= G.kv_atol(spec) and ev <= G.kv_atol(spec), what + (layer, "lane", i, float(ek), float(ev))
        bk, bv = before[layer]
        assert k[other].tobytes() == bk[other].tobytes() and v[other].tobytes() == bv[other].tobytes(), \
            what + (layer, "a row that is no lane's was written")
    rows_lg = []
    for i in range(len(slots)):
        lg = m.seq_gemm_logits(i)
        rows_lg.append(lg)
        if not kw.get("logit_bias") and not kw.get("penalties"):
            e = float(np.abs(lg - ref.logits[ref_ix[i]]).max())
            worst_lg = max(worst_lg, e)
            assert e <= G.logit_atol(spec), what + ("logits of lane", i, e)
    w = _WORST.setdefault(spec.name, [0.0, 0.0])
    w[0], w[1] = max(w[0], worst_kv), max(w[1], worst_lg)
    _LAUNCHED.update(log)
    return got, log, rows_lg


# ---- 1. single passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_single_passes(gpu, oracle, name):
    """n = 1, 15, 16, 17, 64 lanes in shuffled slot order, positions 0 .. 7 and 255 / 256 / 257: K/V rows and logits
    against the oracle, no other row written, h_next[i] = the first maximum of seq_gemm_logits(i).  Then (gqa-half,
    int8) the same 17 lanes under every (R, NT) tile forced on all four GEMMs, the residual GEMMs with K split across
    workgroups in turn: the gate at the end of the file wants every compiled instantiation compared."""
    ref = _ref(oracle, name)
    spec = ref.spec
    m = _model(spec)
    assert m.seq_width(gemm=True) == 64
    _fill(m, ref, range(len(G.LENS)))
    for n in (1, 15, 16, 17, 64):
        slots = _slots(n, seed=n)
        got, log, lg = _pass(m, ref, slots, (name, n))
        assert got == [int(np.argmax(r)) for r in lg], (name, n)
        assert {"k_sg_embed", "k_seq_pick"} <= log and "k_seq_tail" not in log, sorted(log)
        assert ("k_sg_rope" in log) == _rope_kernel(spec, n), sorted(log)
        assert not any(k.startswith(("k_seq_qkv", "k_pf_", "k_seq_embed")) for k in log), sorted(log)
    if name in ("gqa-half", "int8"):
        slots = _slots(17, seed=99)
        for i, (r, nt) in enumerate(((2, 4), (2, 2), (1, 4))):
            for k in HOOKS:
                _ffi.debug_set(k, f"{r},{nt},{1 << i}" + (f",{(2, 4, 1)[i]}" if k.endswith("RESID") else ""))
            got, log, lg = _pass(m, ref, slots, (name, "forced", r, nt))
            assert got == [int(np.argmax(x)) for x in lg]
            q = "true" if spec.quant else "false"
            assert {f"k_sg_gemm<{q},{r},{nt},{e}>" for e in range(4)} <= log, sorted(log)
            # the fused tile RoPE needs the partner tile in the wave: the 16-row tile leaves it to k_sg_rope
            assert ("k_sg_rope" in log) == (name == "gqa-half" and r == 1), sorted(log)
        for k in HOOKS:
            _ffi.debug_set(k, None)
    print(f"worst[{name}]: K/V {_WORST[spec.name][0]:.2e} (bound {G.kv_atol(spec):.0e}), "
          f"logits {_WORST[spec.name][1]:.2e} (bound {G.logit_atol(spec):.0e})")
    m.close()


# ---- 2. samplers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gqa-half", "int8"])
def test_sampled_picks_are_the_sampler_on_the_pass_logits(gpu, oracle, name):
    """a sampler per lane (own seed, temperature, top-k, top-p; every fourth lane greedy): h_next[i] is
    kh_sample_f32_host on seq_gemm_logits(i) with counter pos[i] - exact"""
    ref = _ref(oracle, name)
    m = _model(ref.spec)
    slots = _slots(17, seed=5)
    _fill(m, ref, slots)
    sp = [None if i % 4 == 3 else {"temperature": 0.7 + 0.05 * i, "top_k": (0, 40, 7)[i % 3],
                                   "top_p": (1.0, 0.9, 0.5)[i % 3], "seed": 1000 + i} for i in range(len(slots))]
    got, log, lg = _pass(m, ref, slots, (name, "sampled"), samplings=sp)
    for i, s in enumerate(slots):
        row = torch.from_numpy(lg[i]).to(gpu)
        want = int(np.argmax(lg[i])) if sp[i] is None else ops.sample_host(row, sp[i], counter=G.lane_pos(s))
        assert got[i] == want, (name, i, s, sp[i])
    assert len({g for g, p in zip(got, sp) if p}) > 4  # the draws differ between lanes
    m.close()


# ---- 3. options -------------------------------------------------------------------------------------------------------
def test_options_are_the_operators_on_the_raw_logits(gpu, oracle):
    """penalties on some lanes, a bias with a -inf ban on others, logprobs_top_n = 5: picks, processed rows and records
    equal kh_logit_process_f32 / kh_logprobs_f32 on the pass's RAW logits, which come from a twin call without options
    on a second model - as integers and raw bits"""
    name = "gqa-half"
    ref = _ref(oracle, name)
    spec, V = ref.spec, ref.spec.vocab_size
    slots = [s for s in _slots(17, seed=8)]
    a, b = _model(spec), _model(spec)
    _fill(a, ref, slots)
    _fill(b, ref, slots)
    _, log_a, raw = _pass(a, ref, slots, (name, "raw"))
    assert "k_seq_tail" not in log_a
    pens, bias, samp = [], [], []
    for i, s in enumerate(slots):
        text = ref.T[s]
        pens.append({"repetition": 1.3, "presence": 0.25, "frequency": 0.125, "last_n": (0, 3)[i % 2]}
                    if i % 3 == 0 else None)
        top = int(np.argmax(raw[i]))
        bias.append({top: float("-inf"), text[0]: 1.5, (top + 7) % V: -0.75} if i % 3 == 1 and text[0] != top else None)
        samp.append(dict(SAMP, seed=70 + i) if i % 5 == 4 else None)
    got, log_b, proc = _pass(b, ref, slots, (name, "options"), samplings=samp, penalties=pens, logit_bias=bias,
                             logprobs=5)
    assert "k_seq_tail" in log_b and "k_seq_pick" not in log_b, sorted(log_b)
    ws = ops.logit_process_workspace(V, gpu)
    for i, s in enumerate(slots):
        p = G.lane_pos(s)
        row = torch.from_numpy(raw[i]).to(gpu)
        ids = sorted(bias[i]) if bias[i] else []
        ops.logit_process(row, torch.tensor(ref.T[s], dtype=torch.int32, device=gpu), p, penalties=pens[i] or {},
                          bias_ids=torch.tensor(ids, dtype=torch.int32, device=gpu) if ids else None,
                          bias=torch.tensor([bias[i][k] for k in ids], dtype=torch.float32, device=gpu) if ids else None,
                          workspace=ws)
        want_row = row.cpu().numpy()
        assert proc[i].tobytes() == want_row.tobytes(), (i, s, "processed logits")
        pick = int(np.argmax(want_row)) if samp[i] is None else ops.sample_host(row, samp[i], counter=p)
        assert got[i] == pick, (i, s, pens[i], bias[i], samp[i])
        if bias[i]:
            assert pick != int(np.argmax(raw[i]))  # the ban held
        lp = ops.logprobs(row, torch.tensor([pick], dtype=torch.int32, device=gpu), 5)
        rec = b.seq_logprobs(s, p, 1)
        assert int(rec["token"][0]) == pick
        assert rec["logprob"].tobytes() == lp["logprob"].cpu().numpy().tobytes(), (i, s)
        assert rec["top_ids"].tobytes() == lp["top_ids"].cpu().numpy().tobytes(), (i, s)
        assert rec["top_logprobs"].tobytes() == lp["top_logprobs"].cpu().numpy().tobytes(), (i, s)
    a.close()
    b.close()


# ---- 4. sharing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gqa-half", "int8"])
def test_sharers_ride_beside_their_parents(gpu, oracle, name):
    """slot 3 shares P = 7 rows of slot 0, slot 4 shares P = 256 rows of slot 1; both ride in the first group of 8
    lanes beside their parents and unrelated slots: the tolerances of test 1, k_seq_attn_pfx only for that group"""
    ref = _ref(oracle, name)
    spec = ref.spec
    m = _model(spec)
    slots = [5, 3, 0, 9, 4, 1, 2, 6] + list(range(10, 19))  # 17 lanes: group 0 holds the sharers, groups 1 and 2 none
    _fill(m, ref, [s for s in slots if s not in (3, 4)])
    m.seq_share(0, 3, 7)
    m.seq_share(1, 4, 256)
    rng = np.random.default_rng(3)
    own = {3: [int(t) for t in rng.integers(0, spec.vocab_size, 3)], 4: [int(t) for t in rng.integers(0, spec.vocab_size, 2)]}
    text = {3: ref.T[0][:7] + own[3], 4: ref.T[1][:256] + own[4]}  # positions 0 .. 9 and 0 .. 257
    ix = {}
    for s in (3, 4):
        m.seq_prefill(s, own[s][:-1], pos0=len(text[s]) - len(own[s]))
        key = (name, "sharer", s)
        if key not in _REF:
            ref.add(ref.om, text[s])
            _REF[key] = len(ref.logits) - 1
        ix[s] = _REF[key]
    pos = [len(text[s]) - 1 if s in text else G.lane_pos(s) for s in slots]
    toks = [text[s][-1] if s in text else ref.T[s][-1] for s in slots]
    got, log, lg = _pass(m, ref, slots, (name, "shared"), pos=pos, toks=toks, ref_ix=[ix.get(s, s) for s in slots])
    assert got == [int(np.argmax(r)) for r in lg]
    assert any(k.startswith("k_seq_attn_pfx<") for k in log) and any(k.startswith("k_seq_attn<") for k in log), sorted(log)
    # the same model, a pass without a sharing lane: no k_seq_attn_pfx
    rest = [s for s in slots if s not in (3, 4)]
    got, log, lg = _pass(m, ref, rest, (name, "no sharer"))
    assert not any(k.startswith("k_seq_attn_pfx<") for k in log), sorted(log)
    # the rules of the 8-lane calls: a sharer below its P, a parent below Pmax, penalties on a sharer
    for bad, code in ((dict(slots=[3], tokens=[1], pos=[6]), _ffi.KH_ERR_INVALID_ARG),
                      (dict(slots=[1], tokens=[1], pos=[255]), _ffi.KH_ERR_INVALID_ARG),
                      (dict(slots=[3], tokens=[1], pos=[9], penalties=[{"repetition": 1.2}]), _ffi.KH_ERR_UNSUPPORTED)):
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        with pytest.raises(_ffi.KhError) as e:
            m.seq_step(gemm=True, **bad)
        assert e.value.code == code and not _ffi.launch_log(), (bad, e.value.code, _ffi.launch_log())
    m.close()


# ---- 5. the loop ------------------------------------------------------------------------------------------------------
def test_the_loop_against_a_batch1_twin(gpu, oracle):
    """generate_batch(gemm=True), 20 sequences (16 + 4 lanes per pass), prompts of 1 .. 12 tokens, unequal totals, a
    stop token, against a batch-1 twin's greedy loop per sequence: words agree up to the first pick whose top-1 minus
    top-2 gap (the twin's logits) is below 4 x the logit tolerance, and at least 90 % of the sampled words are
    compared (test_seq_gemm.py checks the oracle's margins of this case on the CPU)."""
    spec = G.SPECS[G.LOOP_SPEC]
    img = G.host_image(spec, wander=True)
    prompts, totals = G.loop_case(spec)
    twin = KuiperModel.from_host_image(img, spec, max_seq_len=64)

    def step(t, p):
        twin.predict(t, p, exec="fused")
        return twin.logits()

    free = [G.greedy_loop(step, pr, tot, (), G.logit_atol(spec))[0] for pr, tot in zip(prompts, totals)]
    stop = (free[5][len(prompts[5]) + 2],)
    want = [G.greedy_loop(step, pr, tot, stop, G.logit_atol(spec)) for pr, tot in zip(prompts, totals)]
    twin.close()
    m = KuiperModel.from_host_image(img, spec, max_seq_len=spec.seq_len)
    m.seq_slots(32)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    got, ms = m.generate_batch(prompts, totals, stop=list(stop), gemm=True)
    log = set(_ffi.launch_log())
    assert any(k.startswith("k_sg_gemm<") for k in log) and "k_seq_pick" in log, sorted(log)
    assert not any(k.startswith("k_pf_cls") for k in log), sorted(log)  # no 8-lane pass behind the prompts
    compared = sampled = 0
    assert any(len(w) < t for (w, _, _), t in zip(want, totals)), "the stop token stopped nobody"
    for s, ((words, near, clean), pr) in enumerate(zip(want, prompts)):
        first = len(pr) - 1
        sampled += len(words) - first
        compared += max(near - first, 0)
        assert got[s][:near] == words[:near], (s, got[s], words, near)
        if clean:
            assert len(got[s]) == len(words), (s, "length", got[s], words)
    assert compared >= 0.9 * sampled, (compared, sampled)
    m.close()


def test_sampled_steps_are_the_sampler_on_each_steps_logits(gpu):
    """one set of 20 sequences stepped 8 times with seq_step(gemm=True) under seeds s, s + 1, ..: every word is the
    sampler applied to that step's own logits row, the word fed back as the next token"""
    spec = G.SPECS[G.LOOP_SPEC]
    m = KuiperModel.from_host_image(G.host_image(spec, wander=True), spec, max_seq_len=spec.seq_len)
    m.seq_slots(32)
    n = 20
    slots = list(range(n))
    sp = [dict(SAMP, seed=500 + s) for s in slots]
    toks = [int(t) for t in np.random.default_rng(2).integers(0, spec.vocab_size, n)]
    for p in range(8):
        got = m.seq_step(slots, toks, [p] * n, samplings=sp, gemm=True)
        for i in range(n):
            row = torch.from_numpy(m.seq_gemm_logits(i)).to(gpu)
            assert got[i] == ops.sample_host(row, sp[i], counter=p), (p, i)
        toks = got
    m.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_an_empty_launch_log(gpu):
    spec = G.SPECS["mha-inter"]
    m = _model(spec)
    V = spec.vocab_size
    cases = [
        (dict(slots=list(range(64)) + [0], tokens=[1] * 65, pos=[0] * 65), _ffi.KH_ERR_RANGE),        # n = 65
        (dict(slots=[4, 7, 4], tokens=[1, 2, 3], pos=[0, 0, 1]), _ffi.KH_ERR_INVALID_ARG),             # a slot twice
        (dict(slots=[4, 7], tokens=[1, 2], pos=[0, G.SHORT]), _ffi.KH_ERR_RANGE),                      # past its slot
        (dict(slots=[4, 7], tokens=[1, 2], pos=[0, -1]), _ffi.KH_ERR_RANGE),
        (dict(slots=[4, 64], tokens=[1, 2], pos=[0, 0]), _ffi.KH_ERR_RANGE),                           # no such slot
        (dict(slots=[4, 7], tokens=[1, V], pos=[0, 0]), _ffi.KH_ERR_RANGE),                            # no such token
        (dict(slots=[4], tokens=[1], pos=[0], logprobs=21), _ffi.KH_ERR_INVALID_ARG),
    ]
    for kw, code in cases:
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        with pytest.raises(_ffi.KhError) as e:
            m.seq_step(gemm=True, **kw)
        assert e.value.code == code and not _ffi.launch_log(), (kw, e.value.code, _ffi.launch_log())
    with pytest.raises(_ffi.KhError) as e:
        m.seq_gemm_logits(0)  # no wide pass yet
    assert e.value.code == _ffi.KH_ERR_UNSUPPORTED
    m.seq_step([4], [1], [0], gemm=True)
    with pytest.raises(_ffi.KhError) as e:
        m.seq_gemm_logits(1)  # that pass had one lane
    assert e.value.code == _ffi.KH_ERR_RANGE
    m.close()
    for bad in (G.ODD_VOCAB, G.SMALL_HEAD):  # a vocabulary that is no multiple of 16; head size 32
        m = KuiperModel.from_host_image(G.host_image(bad), bad)
        m.seq_slots(4)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        for call in (lambda: m.seq_width(gemm=True), lambda: m.seq_step([0, 1], [1, 2], [0, 0], gemm=True),
                     lambda: m.generate_batch([[1, 2], [3]], 4, gemm=True)):
            with pytest.raises(_ffi.KhError) as e:
                call()
            assert e.value.code == _ffi.KH_ERR_UNSUPPORTED, bad.name
        assert not _ffi.launch_log(), (bad.name, _ffi.launch_log())
        if bad is G.ODD_VOCAB:
            assert m.seq_width() == 8 and len(m.seq_step([0, 1], [1, 2], [0, 0])) == 2  # the 8-lane pass runs it
        m.close()


# ---- 7. gates ---------------------------------------------------------------------------------------------------------
def test_a_model_that_never_asks_launches_and_allocates_nothing_new(gpu):
    spec = G.SPECS["gqa-half"]
    m = _model(spec)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    args = ([3, 4, 5], [1, 2, 3], [0, 0, 0])
    m.seq_step(*args)
    m.generate_batch([[1, 2], [3]], 4)
    a0 = _ffi.alloc_stats()
    m.seq_step(*args)
    a1 = _ffi.alloc_stats()
    assert a1["allocs"] == a0["allocs"] and a1["live"] == a0["live"]
    log = _ffi.launch_log()
    assert not any(k.startswith((NEW_PREFIX, "k_pg_")) for k in log), sorted(log)
    m.seq_step(*args, gemm=True)  # the first wide call: the six slabs of the GEMM prefill and the wide logits rows
    a2 = _ffi.alloc_stats()
    assert a2["live"] - a1["live"] == 7, (a1, a2)
    m.seq_step(*args, gemm=True)
    assert _ffi.alloc_stats()["allocs"] == a2["allocs"]
    m.close()


def test_every_compiled_instantiation_of_the_new_stems_was_launched_and_compared(gpu):
    """runs last: what test_single_passes .. test_sharers launched through _pass (every such pass was held against the
    oracle) against the code objects"""
    if not co.tools_present():
        pytest.skip("LLVM tools of the ROCm install not found")
    compiled = co.kernels(co.code_object_notes(build.build_lib()), STEMS)
    assert len(compiled) == 26, sorted(compiled)
    launched = {k for k in _LAUNCHED if k.split("<")[0] in STEMS}
    assert compiled == launched, (sorted(compiled - launched), sorted(launched - compiled))
