"""Per-sequence penalties, logit bias and log-probs in batched decode on the GPU: kh_model_seq_step_ex,
kh_model_generate_batch_ex, kh_model_seq_set_history, kh_model_seq_get_logprobs, best_of (csrc/kh_seq.h: k_seq_tail;
csrc/kh_model_seq.hip).

Every comparison is EXACT: token ids as integers, records and K/V rows as raw bytes, no tolerance.  The reference is a
second, batch-1 model of the same image under set_penalties / set_logit_bias / set_logprobs / set_sampling - the
bit-exact path tests/test_logit_proc_gpu.py and tests/test_logprobs_gpu.py gate: a fused predict for a single pass, its
own generate() for the loop.  k_seq_tail chains the same three device cores on the same logits (a pass's logits are the
decode classifier's bit for bit), so a differing byte is a bug.

The models are the four of tests/score_cases.py (8 / 4 / 8 / 4 lanes per pass), with longer caches where a test needs
more slots or rows past 256, as in tests/test_seq_gpu.py.  Their vocabularies (2048, 2051) are below KH_SAMP_CAP, so the
log-prob core's global-memory fallback (more candidates than fit in LDS) is not reached through k_seq_tail here: that
core is unchanged and tests/test_logprobs_gpu.py covers the fallback on it."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import code_objects as co
import score_cases as S
from kuiperllama_amd import _ffi, binfmt, build
from kuiperllama_amd.model import KuiperModel, seq_rank

pytestmark = pytest.mark.gpu

NAMES = ["a", "b", "c", "d"]
SLOTS = {"a": 8, "b": 4, "c": 8, "d": 4}
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
SAMP = {"temperature": 0.8, "top_k": 50, "top_p": 0.95}
REC = ("token", "logprob", "top_ids", "top_logprobs")
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


def _new_log():
    _LAUNCHED.update(_ffi.launch_log())
    _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log


_IMG = {}


def _image(gpu, name, seq_len=None):
    spec = S.SPECS[name]
    if seq_len:
        spec = dataclasses.replace(spec, seq_len=seq_len)
    key = (name, spec.seq_len)
    if key not in _IMG:
        _IMG[key] = (spec, binfmt.synth_image(spec, seed=S.SEEDS[name], device=gpu))
        torch.cuda.synchronize()
    return _IMG[key]


def _mk(spec, img, **kw):
    return KuiperModel.from_device_image(img, spec, max_seq_len=spec.seq_len, **kw)


def _sampling(seed):
    return dict(SAMP, seed=seed)


@dataclasses.dataclass
class Setting:
    """what one sequence asks for; None = the neutral value"""
    pen: dict = None
    bias: dict = None
    samp: dict = None


def _twin_set(twin, st, top_n):
    twin.set_penalties(**(st.pen or {}))
    twin.set_logit_bias(st.bias)
    twin.set_sampling(**(st.samp or {}))
    twin.set_logprobs(top_n)


def _twin_off(twin):
    _twin_set(twin, Setting(), None)


def _rec_same(got, want, what):
    for k in REC:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), what + (k, g, w)


def _text(rng, V, n):
    """n tokens over an alphabet of five: the windows hold repeats, so frequency counts above 1 occur"""
    alphabet = rng.choice(V, 5, replace=False)
    return [int(alphabet[i]) for i in rng.integers(0, 5, n)]


# ---- 1. one pass per lane ---------------------------------------------------------------------------------------------
def _twin_lane(twin, spec, text, p, st, top_n):
    """the twin's pick, record and K/V row at position p of `text` under `st`"""
    _twin_off(twin)
    if p:
        twin.prefill(text[:p])
    _twin_set(twin, st, top_n)
    nxt = twin.predict(text[p], p, exec="fused")
    rec = twin.logprobs(p, 1) if top_n is not None else None
    kv = [twin.read_kv(layer, p, 1) for layer in range(spec.n_layers)]
    _twin_off(twin)
    return nxt, rec, kv


def _all_records(m, ns, L):
    return [m.seq_logprobs(s, 0, L) for s in range(ns)]


def _check_pass(m, twin, spec, H, ns, L, slots, pos, sts, top_n):
    what = (spec.name, tuple(slots), tuple(pos), top_n)
    want = [_twin_lane(twin, spec, H[s], p, st, top_n) for s, p, st in zip(slots, pos, sts)]
    rows = [s * L + p for s, p in zip(slots, pos)]
    kw = dict(samplings=[st.samp for st in sts], penalties=[st.pen for st in sts],
              logit_bias=[st.bias for st in sts], logprobs=top_n)
    toks = [H[s][p] for s, p in zip(slots, pos)]
    if top_n is not None:  # a pass of this width first, so that the records can be read before and after
        m.seq_step(slots[:1], toks[:1], pos[:1], logprobs=top_n)
    for s in range(ns):  # earlier passes recorded their picks behind their positions: the slots' texts again
        m.seq_set_history(s, H[s])
    poison = np.full((1, spec.kv_dim), np.nan, np.float32)
    for layer in range(spec.n_layers):
        for r in rows:
            m.write_kv(layer, r, poison, poison)
    before_kv = [m.read_kv(layer, 0, ns * L) for layer in range(spec.n_layers)]
    before_rec = _all_records(m, ns, L) if top_n is not None else None
    _new_log()
    got = m.seq_step(slots, toks, pos, **kw)
    log = _ffi.launch_log()
    assert "k_seq_tail" in log and "k_seq_pick" not in log, sorted(log)
    assert got == [w[0] for w in want], what
    other = np.ones(ns * L, bool)
    other[rows] = False
    for layer in range(spec.n_layers):
        k, v = m.read_kv(layer, 0, ns * L)
        for i, r in enumerate(rows):
            wk, wv = want[i][2][layer]
            assert k[r].tobytes() == wk[0].tobytes() and v[r].tobytes() == wv[0].tobytes(), what + (layer, i)
        bk, bv = before_kv[layer]
        assert k[other].tobytes() == bk[other].tobytes() and v[other].tobytes() == bv[other].tobytes(), \
            what + (layer, "a row of another slot or position was written")
    if top_n is not None:
        after = _all_records(m, ns, L)
        for i, (s, p) in enumerate(zip(slots, pos)):
            _rec_same({k: after[s][k][p:p + 1] for k in REC}, want[i][1], what + ("lane", i))
        for s in range(ns):
            mask = np.ones(L, bool)
            for s2, p2 in zip(slots, pos):
                if s2 == s:
                    mask[p2] = False
            _rec_same({k: after[s][k][mask] for k in REC}, {k: before_rec[s][k][mask] for k in REC},
                      what + ("a record of another position was written", s))


@pytest.mark.parametrize("name", NAMES)
def test_one_pass_is_the_batch1_tail_per_lane(gpu, name):
    spec, img = _image(gpu, name)
    width, ns = S.BATCH[name], SLOTS[name]
    L = spec.seq_len // ns
    V = spec.vocab_size
    rng = np.random.default_rng(700 + S.SEEDS[name])
    H = [_text(rng, V, L) for _ in range(ns)]
    twin = _mk(spec, img)
    m = _mk(spec, img)
    assert m.seq_slots(ns) == L and m.seq_width() == width
    for s in range(ns):
        m.seq_prefill(s, H[s][:L - 1])
    ladder = [0, L - 1, 3, L // 2, 1, L - 2, 2, 5]  # unequal positions, both ends of a slot among them
    assert L - 1 > 3
    order = [int(s) for s in rng.permutation(ns)]  # shuffled slots
    slots8 = [order[i % ns] for i in range(8)]
    # lane 4 bans the twin's greedy pick at its position, and pushes another token
    ban_slot, ban_pos = slots8[4], ladder[4]
    g = _twin_lane(twin, spec, H[ban_slot], ban_pos, Setting(), None)[0]
    sts = [Setting(),                                                            # 0: neutral beside the others
           Setting(pen={"repetition": 1.3, "last_n": 3}),                         # L - 1: the window's start has moved
           Setting(pen={"presence": 0.4, "frequency": 0.3}),
           Setting(pen={"repetition": 1.1, "presence": 0.25, "last_n": 0}),       # last_n = 0: the whole slot
           Setting(bias={g: -np.inf, (g + 1) % V: 2.0}),
           Setting(pen={"repetition": 1.3}, samp=_sampling(71)),                  # sampled from the processed logits
           Setting(samp=_sampling(72)),                                           # sampled, nothing processed
           Setting(pen={"repetition": 1.3})]
    banned = None
    for top_n in (None, 0, 5, 20):
        for lo in range(0, 8, width):  # 8 lanes: one pass; 4 lanes: two passes, every setting in one of them
            sl, ps, st = slots8[lo:lo + width], ladder[lo:lo + width], sts[lo:lo + width]
            _check_pass(m, twin, spec, H, ns, L, sl, ps, st, top_n)
            if lo <= 4 < lo + width and top_n == 5:
                banned = m.seq_logprobs(ban_slot, ban_pos, 1)
    # the ban held: the twin's greedy pick is not picked and not among the alternatives
    assert banned["token"][0] != g and g not in banned["top_ids"][0]
    m.close()
    twin.close()


# ---- 2. the loop ------------------------------------------------------------------------------------------------------
class LoopRef:
    """width + 2 slots of 32 rows; sequence s: a prompt of 1, 2, 3 or 2 width + 1 tokens, its own total and its own
    setting.  W[s] / R[s]: the words of the batch-1 twin's generate() under that setting with log-probs top_n, and its
    records of [0, len(words))."""
    L = 32
    TOP = 5

    def __init__(self, gpu, name):
        self.width = w = S.BATCH[name]
        self.ns = w + 2
        self.spec, self.img = _image(gpu, name, seq_len=self.ns * self.L)
        V = self.spec.vocab_size
        rng = np.random.default_rng(800 + S.SEEDS[name])
        lens = [1, 2, 3, 2 * w + 1]
        self.prompts = [_text(rng, V, lens[s % 4]) for s in range(self.ns)]
        self.totals = [min(self.L, len(p) + 6 + (5 * s) % 11) for s, p in enumerate(self.prompts)]
        kinds = [Setting(samp=_sampling(1100)),
                 Setting(pen={"repetition": 1.3}),
                 Setting(pen={"presence": 0.4, "frequency": 0.3}, samp=_sampling(1102)),
                 Setting(pen={"repetition": 1.2, "last_n": 4}),
                 Setting(bias={int(rng.integers(0, V)): 3.0, int(rng.integers(0, V)): -np.inf}, samp=_sampling(1104)),
                 Setting()]
        self.sts = [kinds[s % len(kinds)] for s in range(self.ns)]
        self.twin = _mk(self.spec, self.img, flags=EXACT)
        out = [self.gen(s) for s in range(self.ns)]
        self.W, self.R = [o[0] for o in out], [o[1] for o in out]

    def gen(self, s, stop=()):
        _twin_set(self.twin, self.sts[s], self.TOP)
        words, _ = self.twin.generate(self.prompts[s], self.totals[s], exec="graph", stop=list(stop))
        rec = self.twin.logprobs(0, len(words)) if words else None
        _twin_off(self.twin)
        return words, rec

    def kw(self, n):
        return dict(samplings=[st.samp for st in self.sts[:n]], penalties=[st.pen for st in self.sts[:n]],
                    logit_bias=[st.bias for st in self.sts[:n]])

    def check(self, m, got, W, R, what):
        for s, words in enumerate(got):
            assert words == W[s], what + (s,)
            if not words:
                continue
            rec = m.seq_logprobs(s, 0, len(words))
            _rec_same(rec, R[s], what + (s,))
            fed = min(len(self.prompts[s]) - 1, len(words))
            assert (rec["token"][:fed] == -1).all() and np.isnan(rec["logprob"][:fed]).all(), what + (s, "fed-only")
            assert (rec["token"][fed:] >= 0).all(), what + (s, "sampled")


@pytest.mark.parametrize("name", NAMES)
def test_the_loop_is_generate_until_per_sequence(gpu, name):
    r = LoopRef(gpu, name)
    w, ns = r.width, r.ns
    assert all(len(r.W[s]) == r.totals[s] for s in range(ns)) and len(set(r.totals)) > 2
    m = _mk(r.spec, r.img)
    assert m.seq_slots(ns) == r.L
    for n_seq in (1, w, w + 1, ns):  # w + 1 and ns: two passes per step
        _new_log()
        got, ms = m.generate_batch(r.prompts[:n_seq], r.totals[:n_seq], logprobs=r.TOP, **r.kw(n_seq))
        log = _ffi.launch_log()
        assert "k_seq_tail" in log and "k_seq_pick" not in log, sorted(log)
        assert len(got) == n_seq and ms > 0
        r.check(m, got, r.W, r.R, (name, n_seq))
    # everything neutral and log-probs off: the plain call, its words and its kernels
    samplings = r.kw(ns)["samplings"]
    plain, _ = m.generate_batch(r.prompts, r.totals, samplings)
    _new_log()
    same, _ = m.generate_batch(r.prompts, r.totals, samplings, penalties=[None] * ns, logit_bias=[None] * ns,
                               logprobs=None)
    log = _ffi.launch_log()
    assert same == plain
    assert "k_seq_pick" in log and "k_seq_tail" not in log, sorted(log)
    _new_log()
    same, _ = m.generate_batch(r.prompts, r.totals, samplings, penalties=[{"repetition": 1.0, "last_n": 7}] * ns,
                               logit_bias=[{}] * ns)
    log = _ffi.launch_log()
    assert same == plain and "k_seq_pick" in log and "k_seq_tail" not in log, sorted(log)
    # a processor on ONE sequence is enough to change the tail; the others say what the plain call said
    _new_log()
    one, _ = m.generate_batch(r.prompts, r.totals, samplings, penalties=[{"repetition": 1.0}] * (ns - 1) + [{"presence": 0.5}])
    log = _ffi.launch_log()
    assert one[:ns - 1] == plain[:ns - 1] and "k_seq_tail" in log and "k_seq_pick" not in log, sorted(log)
    # a stop token that the reference itself emits a few steps into exactly ONE sequence
    sampled = [r.W[s][len(r.prompts[s]) - 1:] for s in range(ns)]
    pick = None
    for t in sorted(range(ns), key=lambda s: len(sampled[s])):
        for i in range(2, len(sampled[t]) - 2):
            tok = sampled[t][i]
            if tok not in sampled[t][:i] and all(tok not in sampled[s] for s in range(ns) if s != t):
                pick = (t, i, tok)
                break
        if pick:
            break
    assert pick, "no sequence emits a token of its own a few steps in: choose other seeds"
    t, i, tok = pick
    want_t, rec_t = r.gen(t, stop=[tok])
    assert want_t == r.W[t][:len(r.prompts[t]) - 1 + i]
    got, _ = m.generate_batch(r.prompts, r.totals, stop=[tok], logprobs=r.TOP, **r.kw(ns))
    W = [want_t if s == t else r.W[s] for s in range(ns)]
    R = [rec_t if s == t else r.R[s] for s in range(ns)]
    r.check(m, got, W, R, (name, "stop", t, i))
    assert len(got[t]) < r.totals[t] and all(len(got[s]) == r.totals[s] for s in range(ns) if s != t)
    m.close()
    r.twin.close()


# ---- 3. the slot boundary ---------------------------------------------------------------------------------------------
def _predict_loop(twin, prompt, total, swap=None):
    """generate()'s sequence as a loop of fused predict calls; swap = (after position, token): the fed-token record of
    position 0 is replaced behind that position - predict(token, 0) rewrites it, the K/V row it also rewrote is put
    back - which is what a pick stored one entry past the previous slot's end would do to this sequence"""
    nxt = -1
    for p in range(total):
        tok = prompt[p] if p < len(prompt) else nxt
        nxt = twin.predict(tok, p, is_prompt=p < len(prompt) - 1, exec="fused")
        if swap and p == swap[0]:
            rows = [twin.read_kv(layer, 0, 1) for layer in range(twin.spec.n_layers)]
            twin.predict(swap[1], 0, is_prompt=True, exec="fused")
            for layer, (k, v) in enumerate(rows):
                twin.write_kv(layer, 0, k, v)
    return twin.logprobs(0, total)


def test_a_pick_at_a_slots_last_position_stays_out_of_the_next_slot(gpu):
    """Sequence 0 runs to total_steps == slot_len beside sequence 1, which penalises its whole history and goes on for
    three positions after sequence 0 is done.  Entry row + 1 of sequence 0's last position is position 0 of sequence
    1's history: a tail that stored its pick there would change sequence 1's window, hence its record bytes."""
    spec, img = _image(gpu, "c")
    L, V, TOP = 8, spec.vocab_size, 5
    rng = np.random.default_rng(31)
    p0 = [int(t) for t in rng.integers(0, V, 5)]  # sequence 0: passes at positions 4 .. 7
    y = int(rng.integers(0, V))
    pen = {"repetition": 1.5, "last_n": 0}
    twin = _mk(spec, img, flags=EXACT)
    # the position-0 token of sequence 1: one it would otherwise be likely to pick - the head of the twin's
    # unpenalised top list at the first position behind sequence 0's end
    twin.set_logprobs(TOP)
    twin.generate([y, y], L, exec="graph")
    x = int(twin.logprobs(0, L)["top_ids"][5][0])
    p1 = [x, y]                                   # sequence 1: passes at positions 1 .. 7
    twin.set_penalties(**pen)
    want, _ = twin.generate(p1, L, exec="graph")
    rec = twin.logprobs(0, L)
    # the case can fail: with another token in that entry from position 4 on, the twin's records change
    base = _predict_loop(twin, p1, L)
    _rec_same(base, rec, ("the predict loop is generate()",))
    moved = _predict_loop(twin, p1, L, swap=(4, (x + 1) % V))
    assert any(np.ascontiguousarray(moved[k]).tobytes() != np.ascontiguousarray(base[k]).tobytes() for k in REC)
    _twin_off(twin)
    m = _mk(spec, img)
    assert m.seq_slots(8) == L
    got, _ = m.generate_batch([p0, p1], [L, L], penalties=[None, pen], logprobs=TOP)
    assert len(got[0]) == L and got[1] == want
    _rec_same(m.seq_logprobs(1, 0, L), rec, ("sequence 1",))
    # and sequence 0 is the twin's too, to its last position
    twin.set_logprobs(TOP)
    want0, _ = twin.generate(p0, L, exec="graph")
    assert got[0] == want0
    _rec_same(m.seq_logprobs(0, 0, L), twin.logprobs(0, L), ("sequence 0",))
    m.close()
    twin.close()


# ---- 4. forks and best-of ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forks_carry_the_history_and_best_of_ranks_the_twins_samples(gpu, name):
    w = S.BATCH[name]
    L = 32
    spec, img = _image(gpu, name, seq_len=w * L)
    V = spec.vocab_size
    rng = np.random.default_rng(900 + S.SEEDS[name])
    P = _text(rng, V, 2 * w + 3)
    T, fed, seed = len(P) + 7, len(P) - 1, 3000
    pen = {"repetition": 1.3, "last_n": 16}
    samplings = [_sampling(seed + s) for s in range(w)]
    twin = _mk(spec, img, flags=EXACT)
    W, R = [], []
    for s in range(w):
        _twin_set(twin, Setting(pen=pen, samp=samplings[s]), 0)
        W.append(twin.generate(P, T, exec="graph")[0])
        R.append(twin.logprobs(0, T))
    _twin_off(twin)
    assert all(len(x) == T for x in W) and len({tuple(x) for x in W}) > 1
    m = _mk(spec, img)
    assert m.seq_slots(w) == L
    m.seq_prefill(0, P[:fed])
    for dst in range(1, w):
        m.seq_fork(0, dst, fed)
    # one pass on the forked slots: their history is the fork's copy (nothing else wrote it)
    step_pen = {"repetition": 1.4, "frequency": 0.2}
    lanes = list(range(1, w))
    got = m.seq_step(lanes, [P[fed]] * len(lanes), [fed] * len(lanes), penalties=[step_pen] * len(lanes), logprobs=3)
    twin.prefill(P[:fed])
    _twin_set(twin, Setting(pen=step_pen), 3)
    want = twin.predict(P[fed], fed, exec="fused")
    want_rec = twin.logprobs(fed, 1)
    _twin_off(twin)
    assert got == [want] * len(lanes)
    for s in lanes:
        _rec_same(m.seq_logprobs(s, fed, 1), want_rec, (name, "fork", s))
    # seq_set_history + a step on copied K/V rows = the same step behind a seq_prefill
    m2 = _mk(spec, img)
    assert m2.seq_slots(w) == L
    for layer in range(spec.n_layers):
        k, v = m.read_kv(layer, 0, fed)
        m2.write_kv(layer, 2 * L, k, v)
    m2.seq_set_history(2, P[:fed])
    assert m2.seq_step([2], [P[fed]], [fed], penalties=[step_pen], logprobs=3) == [want]
    _rec_same(m2.seq_logprobs(2, fed, 1), want_rec, (name, "set_history"))
    m2.close()
    # the loop on the forks, seeds seed, seed + 1, ..: every sequence is the twin's run with that seed
    got, _ = m.generate_batch([P] * w, T, samplings, cached=[fed] * w, penalties=[pen] * w, logprobs=0)
    for s in range(w):
        assert got[s] == W[s], (name, s)
        _rec_same(m.seq_logprobs(s, 0, T), R[s], (name, "loop", s))
    m.close()
    # best_of on a model of one slot: it cuts the cache itself; the order is kh_seq_rank's on the twin's log-probs
    order, mean = seq_rank([r["logprob"] for r in R], [fed] * w, [T] * w)
    b = _mk(spec, img)
    best = b.best_of(P, w, T, _sampling(seed), penalties=pen, top_n=0)
    assert [x["words"] for x in best] == [W[s] for s in order], name
    assert [x["seed"] for x in best] == [seed + s for s in order]
    assert [np.float64(x["mean_logprob"]).tobytes() for x in best] == [np.float64(mean[s]).tobytes() for s in order]
    assert all(best[i]["mean_logprob"] >= best[i + 1]["mean_logprob"] for i in range(w - 1))
    b.close()
    twin.close()


# ---- 5. across position 256 -------------------------------------------------------------------------------------------
def test_a_lane_across_position_256_beside_one_at_3(gpu):
    """decode attention starts its time splits at position 256: one lane crosses it while the other sits at 3; the
    window of 64 positions slides over the long sequence's history"""
    spec, img = _image(gpu, "a", seq_len=1280)
    rng = np.random.default_rng(43)
    prompts = [_text(rng, spec.vocab_size, n) for n in (251, 4)]
    totals = [len(p) - 1 + 20 for p in prompts]
    sts = [Setting(pen={"repetition": 1.3, "last_n": 64}, samp=_sampling(9)), Setting(pen={"repetition": 1.3, "last_n": 64})]
    m = _mk(spec, img)
    assert m.seq_slots(4) == 320
    got, _ = m.generate_batch(prompts, totals, [st.samp for st in sts], penalties=[st.pen for st in sts], logprobs=5)
    twin = _mk(spec, img, flags=EXACT)
    for s in range(2):
        _twin_set(twin, sts[s], 5)
        want, _ = twin.generate(prompts[s], totals[s], exec="graph")
        assert got[s] == want and len(want) == totals[s], s
        _rec_same(m.seq_logprobs(s, 0, totals[s]), twin.logprobs(0, totals[s]), ("records", s))
        for layer in range(spec.n_layers):
            k, v = m.read_kv(layer, s * 320, totals[s])
            wk, wv = twin.read_kv(layer, 0, totals[s])
            assert k.tobytes() == wk.tobytes() and v.tobytes() == wv.tobytes(), ("rows", s, layer)
    twin.close()
    m.close()


# ---- 6. refusals before any launch ------------------------------------------------------------------------------------
def _raw_step(m, n_bias, ids, vals, top_n=-1):
    """kh_model_seq_step_ex on lane (slot 0, token 5, position 3) with a bias list the wrapper cannot express"""
    o = _ffi.SeqOpts()
    nb = (C.c_int32 * 1)(n_bias)
    o.n_bias = nb
    o.bias_ids = (C.c_int32 * max(len(ids), 1))(*ids)
    o.bias = (C.c_float * max(len(vals), 1))(*vals)
    o.logprobs_top_n = top_n
    nxt = (C.c_int32 * 1)()
    one = lambda v: (C.c_int32 * 1)(v)  # noqa: E731
    return _ffi.lib().kh_model_seq_step_ex(m._h, 1, one(0), one(5), one(3), C.byref(o), nxt)


def test_refusals_come_before_any_launch(gpu):
    spec, img = _image(gpu, "a")
    m = _mk(spec, img)
    V = spec.vocab_size
    assert m.seq_slots(8) == 40
    m.seq_prefill(0, [1, 2, 3])
    torch.cuda.synchronize()
    _new_log()

    def refused(code, call):
        with pytest.raises(_ffi.KhError) as ei:
            call()
        assert ei.value.code == code, call
        assert not _ffi.launch_log(), _ffi.launch_log()

    bad, rng_ = _ffi.KH_ERR_INVALID_ARG, _ffi.KH_ERR_RANGE
    step = lambda **kw: (lambda: m.seq_step([0, 1], [5, 6], [3, 0], **kw))  # noqa: E731
    batch = lambda **kw: (lambda: m.generate_batch([[1, 2], [3]], 12, **kw))  # noqa: E731
    for call in (step, batch):
        refused(bad, call(penalties=[None, {"repetition": 0.0}]))
        refused(bad, call(penalties=[{"repetition": float("nan")}, None]))
        refused(bad, call(penalties=[{"presence": float("inf")}, None]))
        refused(bad, call(penalties=[None, {"last_n": -1}]))
        refused(bad, call(logit_bias=[None, {3: float("nan")}]))
        refused(bad, call(logit_bias=[{3: float("inf")}, None]))
        refused(rng_, call(logit_bias=[None, {i: 1.0 for i in range(65)}]))  # KH_SEQ_BIAS_MAX = 64
        refused(rng_, call(logit_bias=[{V: 1.0}, None]))
        refused(rng_, call(logit_bias=[{-1: 1.0}, None]))
        refused(bad, call(logprobs=21))
        refused(bad, call(logprobs=-2))
        refused(bad, call(samplings=[None, {"temperature": 0.8, "top_p": 1.5}], logprobs=0))
    # what the wrappers' dicts cannot say: a duplicate id, a negative count, a count without arrays
    assert _raw_step(m, 2, [7, 7], [1.0, 2.0]) == bad and not _ffi.launch_log()
    assert _raw_step(m, -1, [7], [1.0]) == bad and not _ffi.launch_log()
    assert _raw_step(m, 65, list(range(65)), [1.0] * 65) == rng_ and not _ffi.launch_log()
    o = _ffi.SeqOpts()
    o.n_bias = (C.c_int32 * 1)(1)
    o.logprobs_top_n = -1
    one = lambda v: (C.c_int32 * 1)(v)  # noqa: E731
    assert _ffi.lib().kh_model_seq_step_ex(m._h, 1, one(0), one(5), one(3), C.byref(o), one(0)) == bad
    assert not _ffi.launch_log()
    # the plain calls' refusals hold for the _ex forms
    refused(rng_, lambda: m.seq_step([0, 8], [5, 6], [3, 0], logprobs=0))
    refused(bad, lambda: m.seq_step([2, 2], [5, 6], [0, 1], logprobs=0))
    refused(rng_, lambda: m.seq_step([0], [5], [40], logprobs=0))
    refused(rng_, lambda: m.seq_step(list(range(8)) + [0], [5] * 9, [0] * 9, logprobs=0))
    refused(rng_, lambda: m.generate_batch([[1, 2]], 41, logprobs=0))
    refused(rng_, lambda: m.generate_batch([[1]] * 9, 8, logprobs=0))
    refused(bad, lambda: m.generate_batch([[1, 2, 3]], 8, cached=[3], logprobs=0))
    refused(rng_, lambda: m.seq_set_history(8, [1, 2]))
    refused(rng_, lambda: m.seq_set_history(0, [1, 2], 39))
    with pytest.raises(_ffi.KhError) as ei:  # no call has left records yet
        _ffi.check(_ffi.lib().kh_model_seq_get_logprobs(m._h, 0, 0, 1, None, None, None, None), "seq_get_logprobs")
    assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
    # the model's own settings are not consulted by the _ex calls; the plain calls keep refusing while they are on
    want = m.seq_step([0, 1], [5, 6], [3, 0], logprobs=0)
    m.set_penalties(repetition=1.7)
    m.set_logit_bias({int(want[0]): -np.inf})
    m.set_logprobs(7)
    m.set_sampling(0.8, 50, 0.95, 7)
    assert m.seq_step([0, 1], [5, 6], [3, 0], logprobs=0) == want
    with pytest.raises(_ffi.KhError) as ei:
        m.seq_step([0, 1], [5, 6], [3, 0])
    assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
    m.set_sampling()
    m.set_logprobs(None)
    m.set_logit_bias(None)
    m.set_penalties()
    refused_after = m.seq_logprobs(0, 3, 1)
    assert refused_after["token"][0] == want[0]
    with pytest.raises(_ffi.KhError) as ei:
        m.seq_logprobs(0, 39, 2)
    assert ei.value.code == rng_
    m.close()
    # an int8 and a wide model past their width of 4
    for name in ("b", "d"):
        spec2, img2 = _image(gpu, name)
        n = _mk(spec2, img2)
        assert n.seq_slots(4) == 16 and n.seq_width() == 4
        _new_log()
        refused(rng_, lambda: n.seq_step([0, 1, 2, 3, 0], [5] * 5, [0] * 5, penalties=[{"repetition": 1.3}] * 5))
        n.close()
    # a geometry kh_model_score refuses (head size 32)
    from conftest import load_golden
    gspec, gimg, gt, _ = load_golden("hf_llama_half")
    g = KuiperModel.from_host_image(gimg, gspec)
    _new_log()
    refused(_ffi.KH_ERR_UNSUPPORTED, lambda: g.seq_step([0], [int(gt[0])], [0], logprobs=0))
    refused(_ffi.KH_ERR_UNSUPPORTED, lambda: g.generate_batch([[int(gt[0])]], 4, penalties=[{"repetition": 1.3}]))
    g.close()


# ---- 7. a model that never asks ---------------------------------------------------------------------------------------
def test_a_model_that_never_asks_launches_no_tail(gpu):
    spec, img = _image(gpu, "a")
    fresh = _mk(spec, img, flags=EXACT)
    figures = lambda x: (x.kv_bytes(), int(x.cfg.weight_bytes), x.cls_screen_info().get("bytes"))  # noqa: E731
    want = figures(fresh)
    fresh.close()
    m = _mk(spec, img, flags=EXACT)
    P = S.tokens("a", 6)
    _new_log()
    m.generate(P, 20, exec="graph")
    m.set_logprobs(2)
    m.score(P)
    m.set_logprobs(None)
    m.verify(P, 0)
    assert m.seq_slots(8) == 40
    m.seq_prefill(1, P)
    m.seq_fork(1, 2, len(P))
    m.seq_step([1, 2], [7, 8], [len(P), len(P)], [None, _sampling(5)])
    m.generate_batch([P, P[:2]], 20, [_sampling(6), None])
    log = _ffi.launch_log()
    assert "k_seq_pick" in log and "k_seq_tail" not in log, sorted(log)
    kv_rows = m.kv_bytes()  # grows with the rows a model reached, not with what its passes end in
    assert (figures(m)[1], figures(m)[2]) == (want[1], want[2])
    # the first call that asks brings the tail, and none of the byte figures moves
    m.seq_step([1], [7], [len(P)], logprobs=0)
    assert "k_seq_tail" in _ffi.launch_log()
    assert m.kv_bytes() == kv_rows and (figures(m)[1], figures(m)[2]) == (want[1], want[2])
    m.close()


# ---- 8. demo CLI ------------------------------------------------------------------------------------------------------
def test_demo_cli_best_of_prints_the_ranked_samples(gpu, tmp_path):
    import subprocess
    spec, img = _image(gpu, "a")
    P, T, N, seed = S.tokens("a", 6), 24, 3, 41
    b = _mk(spec, img)
    best = b.best_of(P, N, T, _sampling(seed), penalties={"repetition": 1.2}, top_n=0)
    b.close()
    assert len(best) == N
    path = tmp_path / "m.bin"
    img.cpu().numpy().tofile(path)
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--max-seq-len", str(spec.seq_len), "--steps", str(T), "--prompt", ",".join(map(str, P)),
            "--temperature", "0.8", "--top-k", "50", "--top-p", "0.95", "--seed", str(seed)]
    out = subprocess.run(args + ["--best-of", str(N), "--repeat-penalty", "1.2", "--logprobs", "0"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    at = lines.index("Generating...")
    for ln, want in zip(lines[at + 1:at + 1 + N], best):
        head, words = ln.split("|")
        mean, sd = head.split()
        assert [int(t) for t in words.split()] == want["words"], ln
        assert int(sd) == want["seed"] and mean == "%.6f" % want["mean_logprob"], ln
    assert lines[at + 1 + N].startswith("steps/s:")
    bad = subprocess.run(args + ["--parallel", str(N), "--repeat-penalty", "1.2"], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode != 0  # --parallel keeps refusing: not rerouted


# ---- 9. the gate ------------------------------------------------------------------------------------------------------
def test_the_tail_kernel_is_compiled_and_was_launched(gpu):
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    _LAUNCHED.update(_ffi.launch_log())
    notes = co.code_object_notes(_ffi.LIB_PATH)
    assert co.kernels(notes, {"k_seq_tail"}) == {"k_seq_tail"}
    assert "k_seq_tail" in _LAUNCHED, "run the whole module"
    scratch = {k: v for k, v in co.kernel_scratch(notes).items() if co.plain_name(k) == "k_seq_tail"}
    assert scratch and all(v == 0 for v in scratch.values()), scratch
