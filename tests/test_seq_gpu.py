"""Sequence slots on the GPU: kh_model_seq_prefill / _fork / _step and kh_model_generate_batch (csrc/kh_seq.h:
k_seq_embed, k_seq_qkv, k_seq_pick; csrc/kh_attn.h: k_seq_attn; csrc/kh_model_seq.hip).

Every comparison is EXACT: token ids as integers, K/V rows as raw bytes read through kh_model_read_kv.  The reference
side is always a second, batch-1 model made from the same image: a loop of fused predict calls for a single pass,
its own generate() for the batched loop.  The logits of a pass are the decode classifier's bit for bit
and a pick is a first maximum or the sampler core's draw, so a mismatch is a bug and no tolerance appears here.

The models are the four of tests/score_cases.py: (a) fp32 GQA, 8 lanes per pass, cache 320 = 8 slots of 40; (b) int8,
4 lanes, cache 64 = 4 slots of 16; (c) Qwen2 with bias, 8 lanes, cache 64 = 8 slots of 8; (d) wide fp32 with an odd
vocabulary, 4 lanes, 4 slots of 16.  Tests that need more than `width` slots, or rows past 256, take the same weights
with a longer cache (dataclasses.replace(spec, seq_len=..): the cache is never longer than the image's seq_len).
The last two tests launch the instantiations of k_seq_qkv / k_seq_attn the four models do not reach (KH_SHAPE_QKV,
KH_ATTN_TLONG, six small geometries) and hold the compiled set against everything this file launched."""
import dataclasses

import numpy as np
import pytest
import torch

import code_objects as co
import score_cases as S
from kuiperllama_amd import _ffi, binfmt, build
from kuiperllama_amd.model import KuiperModel, plan_seq_batch

pytestmark = pytest.mark.gpu

NAMES = ["a", "b", "c", "d"]
SLOTS = {"a": 8, "b": 4, "c": 8, "d": 4}  # test 1: the partition of the model's own cache
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
SAMP = {"temperature": 0.8, "top_k": 50, "top_p": 0.95}
STEMS = ("k_seq_qkv", "k_seq_attn", "k_seq_embed", "k_seq_pick")
_LAUNCHED = set()


@pytest.fixture(autouse=True)
def _launch_log():
    """every test of this file runs with the launch log on; what it launched is kept for the gate"""
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        yield
    finally:
        _LAUNCHED.update(_ffi.launch_log())
        _ffi.debug_set("KH_LAUNCH_LOG", None)


def _keep_log():
    _LAUNCHED.update(_ffi.launch_log())


_IMG = {}


def _image(gpu, name, seq_len=None, spec=None):
    """(spec, image) of a score_cases model, optionally with a longer cache; cached"""
    spec = spec or S.SPECS[name]
    if seq_len:
        spec = dataclasses.replace(spec, seq_len=seq_len)
    key = (name, spec.seq_len)
    if key not in _IMG:
        _IMG[key] = (spec, binfmt.synth_image(spec, seed=S.SEEDS.get(name, 13), device=gpu))
        torch.cuda.synchronize()
    return _IMG[key]


def _mk(spec, img, **kw):
    return KuiperModel.from_device_image(img, spec, max_seq_len=spec.seq_len, **kw)


def _sampling(seed):
    return dict(SAMP, seed=seed)


def _same(got, want, what):
    gk, gv = got
    wk, wv = want
    assert gk.shape == wk.shape and gk.tobytes() == wk.tobytes(), what + ("K",)
    assert gv.tobytes() == wv.tobytes(), what + ("V",)


# ---- the token-by-token reference of single passes -------------------------------------------------------------------
class Hist:
    """Per slot s a text H[s] of slot_len tokens, different for every slot; G[s][p] = the greedy pick of a loop of
    fused predict calls on a batch-1 twin fed H[s][:p + 1]; KV[s][layer] = the (K, V) rows that loop left.  sampled():
    the twin's pick at (s, p) under a sampler of its own."""

    def __init__(self, spec, img, n_slots, seed):
        self.spec, self.n_slots, self.L = spec, n_slots, spec.seq_len // n_slots
        rng = np.random.default_rng(seed)
        self.H = [[int(t) for t in rng.integers(0, spec.vocab_size, self.L)] for _ in range(n_slots)]
        self.twin = _mk(spec, img)
        self.G, self.KV = [], []
        for s in range(n_slots):
            self.G.append([self.twin.predict(t, p, exec="fused") for p, t in enumerate(self.H[s])])
            self.KV.append([self.twin.read_kv(layer, 0, self.L) for layer in range(spec.n_layers)])
        self._sampled = {}

    def sampled(self, s, p, sp):
        key = (s, p, tuple(sorted(sp.items())))
        if key not in self._sampled:
            if p:
                self.twin.prefill(self.H[s][:p])
            self.twin.set_sampling(**sp)
            self._sampled[key] = self.twin.predict(self.H[s][p], p, exec="fused")
            self.twin.set_sampling()
        return self._sampled[key]

    def close(self):
        self.twin.close()


def _filled(spec, img, hist, **kw):
    """a model cut into hist's slots, every slot prefilled with all but the last token of its text"""
    m = _mk(spec, img, **kw)
    assert m.seq_slots(hist.n_slots) == hist.L
    for s in range(hist.n_slots):
        m.seq_prefill(s, hist.H[s][:hist.L - 1])
        for layer in range(spec.n_layers):  # kh_model_prefill's contract on the slot's rows
            k, v = hist.KV[s][layer]
            _same(m.read_kv(layer, s * hist.L, hist.L - 1), (k[:hist.L - 1], v[:hist.L - 1]), ("prefill", s, layer))
    return m


def _check_step(m, hist, slots, pos, samplings):
    """one seq_step against the twin: picks, the lanes' rows (poisoned first: the pass must write them), every other
    row of the cache untouched"""
    spec, L = hist.spec, hist.L
    what = (spec.name, tuple(slots), tuple(pos), samplings is not None)
    rows = [s * L + p for s, p in zip(slots, pos)]
    poison = np.full((1, spec.kv_dim), np.nan, np.float32)
    for layer in range(spec.n_layers):
        for r in rows:
            m.write_kv(layer, r, poison, poison)
    before = [m.read_kv(layer, 0, hist.n_slots * L) for layer in range(spec.n_layers)]
    got = m.seq_step(slots, [hist.H[s][p] for s, p in zip(slots, pos)], pos, samplings)
    want = [hist.G[s][p] if samplings is None or samplings[i] is None else hist.sampled(s, p, samplings[i])
            for i, (s, p) in enumerate(zip(slots, pos))]
    assert got == want, what
    other = np.ones(hist.n_slots * L, bool)
    other[rows] = False
    for layer in range(spec.n_layers):
        k, v = m.read_kv(layer, 0, hist.n_slots * L)
        for (s, p), r in zip(zip(slots, pos), rows):
            wk, wv = hist.KV[s][layer]
            assert k[r].tobytes() == wk[p].tobytes() and v[r].tobytes() == wv[p].tobytes(), what + (layer, s, p)
        bk, bv = before[layer]
        assert k[other].tobytes() == bk[other].tobytes() and v[other].tobytes() == bv[other].tobytes(), \
            what + (layer, "a row of another slot or position was written")


# ---- 1. seq_step against a predict loop ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_seq_step_is_a_predict_loop_per_lane(gpu, name):
    spec, img = _image(gpu, name)
    width, ns = S.BATCH[name], SLOTS[name]
    hist = Hist(spec, img, ns, seed=200 + S.SEEDS[name])
    L = hist.L
    assert L == {"a": 40, "b": 16, "c": 8, "d": 16}[name]
    m = _filled(spec, img, hist)
    assert m.seq_width() == width == m.verify_width()
    rng = np.random.default_rng(S.SEEDS[name])
    ladder = [0, L - 1, 3, L // 2, 1, L - 2, 2, 5]  # unequal positions, both ends of a slot among them
    for n in sorted({1, width - 1, width}):
        slots = [int(s) for s in rng.permutation(ns)[:n]]  # shuffled slot order
        pos = [L // 2] if n == 1 else ladder[:n]
        _check_step(m, hist, slots, pos, None)
        _check_step(m, hist, slots, pos, [_sampling(77 + i) for i in range(n)])
    # one greedy lane among sampled ones, every lane at position 0 and every lane at the last row of its slot
    n = min(width, ns)
    mixed = [None if i == 1 else _sampling(500 + i) for i in range(n)]
    _check_step(m, hist, list(range(n)), [0] * n, mixed)
    _check_step(m, hist, list(range(n))[::-1], [L - 1] * n, mixed)
    m.close()
    hist.close()


# ---- 2. generate_batch against generate_until --------------------------------------------------------------------------
class BatchRef:
    """width + 2 slots of 32 rows; sequence s: a prompt of 1, 2, 3 or 2 width + 1 tokens, its own total, greedy for
    s == 1 and sampled with its own seed otherwise.  W[s] / KV[s]: the words of the batch-1 twin's generate() under
    that sampler and the rows it left; Wg / KVg: the same, greedy."""
    L = 32

    def __init__(self, gpu, name):
        self.width = w = S.BATCH[name]
        self.ns = w + 2
        self.spec, self.img = _image(gpu, name, seq_len=self.ns * self.L)
        rng = np.random.default_rng(300 + S.SEEDS[name])
        lens = [1, 2, 3, 2 * w + 1]
        self.prompts = [[int(t) for t in rng.integers(0, self.spec.vocab_size, lens[s % 4])] for s in range(self.ns)]
        self.totals = [min(self.L, len(p) + 6 + (5 * s) % 11) for s, p in enumerate(self.prompts)]
        self.samplings = [None if s == 1 else _sampling(1000 + s) for s in range(self.ns)]
        self.twin = _mk(self.spec, self.img, flags=EXACT)
        self.W, self.KV = self._run(self.samplings)
        self.Wg, self.KVg = self._run([None] * self.ns)

    def _gen(self, s, sp, stop=()):
        self.twin.set_sampling(**(sp or {}))
        words, _ = self.twin.generate(self.prompts[s], self.totals[s], exec="graph", stop=list(stop))
        rows = [self.twin.read_kv(layer, 0, max(len(words), 1)) for layer in range(self.spec.n_layers)]
        self.twin.set_sampling()
        return words, rows

    def _run(self, samplings):
        out = [self._gen(s, samplings[s]) for s in range(self.ns)]
        return [o[0] for o in out], [o[1] for o in out]

    def check(self, m, got, W, KV, what):
        for s, words in enumerate(got):
            assert words == W[s], what + (s,)
            for layer in range(self.spec.n_layers):
                k, v = KV[s][layer]
                _same(m.read_kv(layer, s * self.L, len(words)), (k[:len(words)], v[:len(words)]), what + (s, layer))


@pytest.mark.parametrize("name", NAMES)
def test_generate_batch_is_generate_until_per_sequence(gpu, name):
    r = BatchRef(gpu, name)
    w, ns = r.width, r.ns
    assert all(len(r.W[s]) == r.totals[s] for s in range(ns)) and len(set(r.totals)) > 2
    m = _mk(r.spec, r.img)
    assert m.seq_slots(ns) == r.L
    for n_seq in (1, w, w + 1, ns):  # w + 1 and ns: two passes per step
        got, ms = m.generate_batch(r.prompts[:n_seq], r.totals[:n_seq], r.samplings[:n_seq])
        assert len(got) == n_seq and ms > 0
        r.check(m, got, r.W, r.KV, (name, "sampled", n_seq))
    got, _ = m.generate_batch(r.prompts, r.totals)  # samplings = None: all greedy
    r.check(m, got, r.Wg, r.KVg, (name, "greedy"))
    # the planner is the grouping the call ran: its passes and lanes add up to the words that were sampled
    plan = plan_seq_batch([len(p) - 1 for p in r.prompts], r.totals, w)
    assert sum(map(len, plan)) == sum(t - (len(p) - 1) for p, t in zip(r.prompts, r.totals))
    # a stop token that the reference itself emits a few steps into exactly ONE sequence: that one ends early and
    # leaves the lane table, the others run on to their totals
    sampled = [r.W[s][len(r.prompts[s]) - 1:] for s in range(ns)]
    pick = None
    for t in sorted(range(ns), key=lambda s: len(sampled[s])):  # the shortest first: the others go on for longest
        for i in range(2, len(sampled[t]) - 2):
            tok = sampled[t][i]
            if tok not in sampled[t][:i] and all(tok not in sampled[s] for s in range(ns) if s != t):
                pick = (t, i, tok)
                break
        if pick:
            break
    assert pick, "no sequence emits a token of its own a few steps in: choose other seeds"
    t, i, tok = pick
    want_t, rows_t = r._gen(t, r.samplings[t], stop=[tok])
    assert want_t == r.W[t][:len(r.prompts[t]) - 1 + i]
    got, _ = m.generate_batch(r.prompts, r.totals, r.samplings, stop=[tok])
    W = [want_t if s == t else r.W[s] for s in range(ns)]
    KV = [rows_t if s == t else r.KV[s] for s in range(ns)]
    r.check(m, got, W, KV, (name, "stop", t, i))
    assert len(got[t]) < r.totals[t] and all(len(got[s]) == r.totals[s] for s in range(ns) if s != t)
    m.close()
    r.twin.close()


# ---- 3. fork --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forked_slots_continue_one_prefilled_prompt(gpu, name):
    w = S.BATCH[name]
    spec, img = _image(gpu, name, seq_len=4 * 32)
    rng = np.random.default_rng(400 + S.SEEDS[name])
    P = [int(t) for t in rng.integers(0, spec.vocab_size, 2 * w + 3)]
    T = len(P) + 7
    m = _mk(spec, img)
    assert m.seq_slots(4) == 32
    m.seq_prefill(0, P[:-1])
    for dst in (1, 2, 3):
        m.seq_fork(0, dst, len(P) - 1)
    for layer in range(spec.n_layers):
        src = m.read_kv(layer, 0, len(P) - 1)
        for dst in (1, 2, 3):
            _same(m.read_kv(layer, dst * 32, len(P) - 1), src, (name, "fork", dst, layer))
    samplings = [_sampling(2000 + s) for s in range(4)]
    got, _ = m.generate_batch([P] * 4, T, samplings, cached=[len(P) - 1] * 4)
    twin = _mk(spec, img, flags=EXACT)
    for s in range(4):
        twin.set_sampling(**samplings[s])
        want, _ = twin.generate(P, T, exec="graph")
        assert got[s] == want and len(want) == T, (name, s)
        for layer in range(spec.n_layers):
            _same(m.read_kv(layer, s * 32, T), twin.read_kv(layer, 0, T), (name, "rows", s, layer))
    assert len({tuple(g) for g in got}) > 1  # distinct seeds, distinct continuations
    # a prompt cached in part: the rest of it is fed by the call
    got2, _ = m.generate_batch([P] * 2, T, samplings[:2], cached=[3, 0])
    assert got2 == got[:2]
    twin.close()
    m.close()


# ---- 4. across position 256 --------------------------------------------------------------------------------------------
def test_lanes_on_both_sides_of_the_time_split_threshold(gpu):
    """decode attention starts its time splits at position 256: one lane crosses it while the other sits at 3"""
    spec, img = _image(gpu, "a", seq_len=1280)
    rng = np.random.default_rng(41)
    prompts = [[int(t) for t in rng.integers(0, spec.vocab_size, n)] for n in (251, 4)]
    totals = [len(p) - 1 + 20 for p in prompts]
    samplings = [_sampling(9), None]
    m = _mk(spec, img)
    assert m.seq_slots(4) == 320
    got, _ = m.generate_batch(prompts, totals, samplings)
    twin = _mk(spec, img, flags=EXACT)
    for s in range(2):
        twin.set_sampling(**(samplings[s] or {}))
        want, _ = twin.generate(prompts[s], totals[s], exec="graph")
        assert got[s] == want and len(want) == totals[s], s
        for layer in range(spec.n_layers):
            _same(m.read_kv(layer, s * 320, totals[s]), twin.read_kv(layer, 0, totals[s]), ("rows", s, layer))
    twin.close()
    m.close()


# ---- 5. refusals, and a model that never asks ----------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gpu):
    spec, img = _image(gpu, "a")
    m = _mk(spec, img)
    V = spec.vocab_size
    for bad in (0, 65, 41):  # 41 slots of 7 rows
        with pytest.raises(_ffi.KhError) as ei:
            m.seq_slots(bad)
        assert ei.value.code == _ffi.KH_ERR_INVALID_ARG
    assert m.seq_slots(8) == 40
    m.seq_prefill(0, [1, 2, 3])
    torch.cuda.synchronize()
    _keep_log()
    _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log

    def refused(code, call):
        with pytest.raises(_ffi.KhError) as ei:
            call()
        assert ei.value.code == code, call
        assert not _ffi.launch_log(), _ffi.launch_log()

    step = lambda: m.seq_step([0, 1], [5, 6], [3, 0])  # noqa: E731
    batch = lambda: m.generate_batch([[1, 2], [3]], 12)  # noqa: E731
    settings = [(lambda: m.set_penalties(repetition=1.2), m.set_penalties),
                (lambda: m.set_logit_bias({3: 1.0}), lambda: m.set_logit_bias(None)),
                (lambda: m.set_logprobs(0), lambda: m.set_logprobs(None))]
    for call in (step, batch):
        for on, off in settings:
            on()
            _ffi.debug_set("KH_LAUNCH_LOG", "1")  # whatever switching the setting on launched is not the call's
            refused(_ffi.KH_ERR_UNSUPPORTED, call)
            off()
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_step([0, 8], [5, 6], [3, 0]))      # a slot outside the partition
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_step([0, -1], [5, 6], [3, 0]))
    refused(_ffi.KH_ERR_INVALID_ARG, lambda: m.seq_step([2, 2], [5, 6], [0, 1]))  # two lanes in one slot
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_step([0], [5], [40]))              # a position outside the slot
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_step([0], [V], [0]))
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_step(list(range(8)) + [0], [5] * 9, [0] * 9))  # n > width
    refused(_ffi.KH_ERR_INVALID_ARG, lambda: m.seq_step([0], [5], [0], [{"temperature": 0.8, "top_p": 1.5}]))
    refused(_ffi.KH_ERR_RANGE, lambda: m.generate_batch([[1, 2]], 41))          # total_steps > slot_len
    refused(_ffi.KH_ERR_RANGE, lambda: m.generate_batch([[1]] * 9, 8))          # n_seq > n_slots
    refused(_ffi.KH_ERR_RANGE, lambda: m.generate_batch([[1, V]], 8))
    refused(_ffi.KH_ERR_INVALID_ARG, lambda: m.generate_batch([[1, 2, 3]], 8, cached=[3]))  # more than is fed-only
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_prefill(8, [1, 2]))
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_prefill(0, [1, 2], 39))            # pos0 + n > slot_len
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_fork(0, 8, 4))
    refused(_ffi.KH_ERR_RANGE, lambda: m.seq_fork(0, 1, 41))
    # the model's own sampler is not consulted: a greedy pass stays greedy
    plain = m.seq_step([0, 1], [5, 6], [3, 0])
    m.set_sampling(0.8, 50, 0.95, 7)
    assert m.seq_step([0, 1], [5, 6], [3, 0]) == plain
    m.set_sampling()
    log = _ffi.launch_log()
    assert {"k_seq_embed", "k_seq_pick", "k_seq_qkv<false,1,8>", "k_seq_attn<16,0>", "k_pf_cls<false,8>"} <= log, log
    assert any(k.startswith("seq_attn_launch<") for k in log)
    assert not any(k.startswith(("attn_launch<", "k_attn_decode<", "k_pf_qkv<")) for k in log), log  # a pass's own records
    m.close()
    # a geometry outside the pass (head size 32): unsupported, width included
    from conftest import load_golden
    gspec, gimg, gt, _ = load_golden("hf_llama_half")
    g = KuiperModel.from_host_image(gimg, gspec)
    for call in (g.seq_width, lambda: g.seq_step([0], [int(gt[0])], [0]), lambda: g.generate_batch([[int(gt[0])]], 4),
                 lambda: g.seq_prefill(0, [int(gt[0])])):
        with pytest.raises(_ffi.KhError) as ei:
            call()
        assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
    g.close()


def test_a_model_with_one_slot_launches_no_seq_kernel(gpu):
    spec, img = _image(gpu, "a")
    m = _mk(spec, img, flags=EXACT)
    P = S.tokens("a", 6)
    _keep_log()
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    words, _ = m.generate(P, 20, exec="graph")
    m.set_logprobs(2)
    m.score(P)
    m.set_logprobs(None)
    m.verify(P, 0)
    log = _ffi.launch_log()
    assert log and not any(k.startswith(("k_seq_", "seq_attn_launch")) for k in log), sorted(log)
    # slot 0 of a partition IS the batch-1 sequence's rows: generate after cutting the cache says the same words
    assert m.seq_slots(4) == 80
    assert m.generate(P, 20, exec="graph")[0] == words
    m.close()


# ---- demo CLI ------------------------------------------------------------------------------------------------------------
def test_demo_cli_parallel_prints_one_line_per_sequence(gpu, tmp_path):
    import subprocess
    spec, img = _image(gpu, "a")
    P, T, N, seed = S.tokens("a", 6), 24, 3, 41
    twin = _mk(spec, img, flags=EXACT)
    want = []
    for s in range(N):
        twin.set_sampling(**_sampling(seed + s))
        want.append(twin.generate(P, T, exec="graph")[0])
    twin.close()
    path = tmp_path / "m.bin"
    img.cpu().numpy().tofile(path)
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--max-seq-len", str(spec.seq_len), "--steps", str(T), "--prompt", ",".join(map(str, P)),
            "--temperature", "0.8", "--top-k", "50", "--top-p", "0.95", "--seed", str(seed), "--parallel", str(N)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    at = lines.index("Generating...")
    assert [[int(t) for t in ln.split()] for ln in lines[at + 1:at + 1 + N]] == want
    assert lines[at + 1 + N].startswith("steps/s:")
    bad = subprocess.run(args + ["--repeat-penalty", "1.2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0  # refused, not rerouted


# ---- 6. every instantiation ----------------------------------------------------------------------------------------------
def _geometry(dim, heads, kv_heads, name):
    return binfmt.ModelSpec(dim, 512, 2, heads, kv_heads, 2048, 64, True, binfmt.FAMILY_LLAMA, False, 64,
                            binfmt.ROPE_HALF, 500000.0, 1e-5, name)


# (spec or score_cases name, hooks read at creation, the instantiations the check must launch)
OTHER = [
    ("a", {"KH_SHAPE_QKV": "2,4,64"}, {"k_seq_qkv<false,2,8>"}),
    ("b", {"KH_SHAPE_QKV": "2,2,64"}, {"k_seq_qkv<true,2,4>"}),
    ("d", {"KH_SHAPE_QKV": "1,4,256"}, {"k_seq_qkv<false,1,4>"}),
    ("a", {"KH_ATTN_TLONG": "8"}, {"k_seq_attn<16,2>", "k_seq_attn<16,0>"}),
    (_geometry(256, 4, 1, "seq-16-4"), {"KH_ATTN_TLONG": "8"}, {"k_seq_attn<16,4>"}),
    (_geometry(448, 7, 1, "seq-16-7"), {"KH_ATTN_TLONG": "8"}, {"k_seq_attn<16,7>"}),
    (_geometry(512, 8, 1, "seq-16-8"), {"KH_ATTN_TLONG": "8"}, {"k_seq_attn<16,8>"}),
    (_geometry(512, 4, 2, "seq-32-2"), {"KH_ATTN_TLONG": "8"}, {"k_seq_attn<32,2>"}),
    (_geometry(512, 4, 1, "seq-32-4"), {"KH_ATTN_TLONG": "8"}, {"k_seq_attn<32,4>"}),
    (_geometry(512, 2, 2, "seq-64-0"), {}, {"k_seq_attn<64,0>"}),
]


@pytest.mark.parametrize("case", range(len(OTHER)))
def test_seq_step_on_the_other_instantiations(gpu, case):
    """the pass under the second QKV split and under every head size / KV-group width of decode attention, the group
    path taken by the lanes at or above KH_ATTN_TLONG and the per-head path by those below in ONE launch"""
    which, hooks, must = OTHER[case]
    if isinstance(which, str):
        spec, img = _image(gpu, which, seq_len=64)
    else:
        spec, img = _image(gpu, which.name, spec=which)
    try:
        for k, v in hooks.items():
            _ffi.debug_set(k, v)  # read by kh_model_create_*: the twin is shaped by them too
        hist = Hist(spec, img, 4, seed=600 + case)
        m = _filled(spec, img, hist)
    finally:
        for k in hooks:
            _ffi.debug_set(k, None)
    n = min(m.seq_width(), 4)
    _keep_log()
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    _check_step(m, hist, [2, 0, 3, 1][:n], [15, 3, 9, 0][:n], None)            # above and below TLONG = 8 together
    _check_step(m, hist, [1, 3, 0, 2][:n], [2, 12, 7, 14][:n], [_sampling(case + i) for i in range(n)])
    _check_step(m, hist, [3, 1][:n], [1, 5], None)                              # every lane below: per-head only
    log = _ffi.launch_log()
    assert must <= log, (must, sorted(log))
    m.close()
    hist.close()


def test_instantiation_gate(gpu):
    """every compiled instantiation of the new stems was launched (and checked) by this file, and nothing launched is
    missing from the code objects"""
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    _keep_log()
    compiled = co.kernels(co.code_object_notes(_ffi.LIB_PATH), set(STEMS))
    launched = {k for k in _LAUNCHED if k.split("<")[0] in STEMS}
    for stem in STEMS:
        comp = sorted(k for k in compiled if k.split("<")[0] == stem)
        assert comp, f"no {stem} in the library"
        print(f"{stem}: {len([k for k in comp if k in launched])} of {len(comp)} compiled instantiations launched")
    assert launched <= compiled, f"launched but not found in the code objects: {sorted(launched - compiled)}"
    gap = compiled - launched
    assert not gap, f"compiled and never launched (run the whole module): {sorted(gap)}"
    # the B values and splits the issue names
    assert {"k_seq_qkv<false,1,8>", "k_seq_qkv<false,2,8>", "k_seq_qkv<false,1,4>", "k_seq_qkv<false,2,4>",
            "k_seq_qkv<true,1,4>", "k_seq_qkv<true,2,4>"} == {k for k in compiled if k.startswith("k_seq_qkv<")}
