"""Per-sequence constrained decoding in sequence slots and batched decode on the GPU: kh_model_seq_set_constraint,
kh_model_seq_set/get_constraint_state and the launching sequence calls under it (csrc/kh_seq.h: k_seq_tail_fsm;
csrc/kh_model_seq.hip).

Every comparison is EXACT: token ids and states as integers, records and K/V rows as raw bytes.  The reference is always
a twin batch-1 model of the same image under set_constraint(A_s) - the path tests/test_constraint_gpu.py gates - with the
same sampling, penalties, bias and log-probs: its generate() for the loop, a fused predict for a single pass.  For the
wide pass (gemm=True) the contract is the wide pass's own: every pick is exact on the pass's own (masked) logits.

The models are the four of tests/score_cases.py (8, 4, 8 and 4 lanes per pass; (d) has V = 2051, so the mask's last
partial word and its scalar tail are reached), the automata constraint_ref.random_automaton(V, row_sizes(V), seed)."""
import dataclasses

import numpy as np
import pytest
import torch

import code_objects as co
import constraint_ref as CR
import sampling_ref as SR
import score_cases as S
from kuiperllama_amd import _ffi, binfmt, build, ops
from kuiperllama_amd.constraint import TokenAutomaton, from_choices, union
from kuiperllama_amd.model import KuiperModel

pytestmark = pytest.mark.gpu

INF = float("inf")
NAMES = ["a", "b", "c", "d"]
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
SAMP = {"temperature": 0.9, "top_k": 40, "top_p": 0.95}
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)
REC = ("token", "logprob", "top_ids", "top_logprobs")
TOP = 5
STEPS = 24
L = 32  # rows per slot
# Seeds of the automata, one per constrained sequence of test 1 (width of them per model): for sequence s of model k
# (a = 1 .. d = 4) the first seed from 1000 k + 10 s on for which the precondition of that test - the twin's RAW argmax
# lies outside the row of the state at half of the sampled positions at least - holds in all four runs (greedy and
# sampled, with and without penalties, bias and log-probs).  Found by running the twin alone; the test asserts it.
SEEDS = {
    "a": [1000, 1011, 1023, 1030, 1040, 1051, 1062, 1076],
    "b": [2000, 2010, 2020, 2030],
    "c": [3005, 3013, 3020, 3031, 3042, 3054, 3062, 3070],
    "d": [4000, 4010, 4020, 4032],
}
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


def _image(gpu, name, seq_len):
    spec = dataclasses.replace(S.SPECS[name], seq_len=seq_len)
    key = (name, seq_len)
    if key not in _IMG:
        _IMG[key] = (spec, binfmt.synth_image(spec, seed=S.SEEDS[name], device=gpu))
        torch.cuda.synchronize()
    return _IMG[key]


def _mk(spec, img, **kw):
    return KuiperModel.from_device_image(img, spec, max_seq_len=spec.seq_len, **kw)


def _raises(code, call):
    with pytest.raises(_ffi.KhError) as ei:
        call()
    assert ei.value.code == code, ei.value


def _rec_same(got, want, what):
    for k in REC:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), what + (k, g, w)


# ---- the twin ----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Setting:
    """what one sequence asks for; None = the neutral value"""
    auto: TokenAutomaton = None
    pen: dict = None
    bias: dict = None
    samp: dict = None


def _twin_set(twin, st, top_n):
    twin.set_constraint(None)
    twin.set_penalties(**(st.pen or {}))
    twin.set_logit_bias(st.bias)
    twin.set_sampling(**(st.samp or {}))
    twin.set_logprobs(top_n)
    twin.set_constraint(st.auto)


def twin_generate(twin, spec, prompt, steps, st, top_n):
    """-> (words, records of [0, steps) or None, K/V rows [0, steps) of every layer) of generate() under `st`"""
    _twin_set(twin, st, top_n)
    words, _ = twin.generate(prompt, steps, exec="graph")
    rec = twin.logprobs(0, len(words)) if top_n is not None else None
    kv = [twin.read_kv(layer, 0, steps) for layer in range(spec.n_layers)]
    _twin_set(twin, Setting(), None)
    return words, rec, kv


def raw_argmax_outside(raw, auto, prompt, words):
    """On a twin WITHOUT any setting: the sequence fed again, and at every sampled position whether the argmax of the raw
    logits lies outside the row of the state the host walk of `words` is in.  -> one bool per sampled position"""
    n0 = len(prompt) - 1
    fed = list(prompt) + list(words[n0:])
    s, out = auto.start, []
    for p in range(len(words)):
        raw.predict(fed[p], p, is_prompt=p < n0, exec="fused")
        if p >= n0:
            out.append(int(np.argmax(raw.logits())) not in set(auto.allowed(s).tolist()))
            s = auto.step(s, words[p])
            assert s >= 0, (p, words[p])
    return out


# ---- 1. generate_batch -----------------------------------------------------------------------------------------------
RUNS = [(False, False), (True, False), (False, True), (True, True)]  # (sampled, with penalties + bias + log-probs)


class Batch:
    """width constrained sequences - one per lane of a pass, each under its own automaton - plus one unconstrained:
    width + 1 slots of L rows, two passes per step, prompts of 2 and 3 tokens (so the lanes of a pass sit at different
    positions)."""

    def __init__(self, gpu, name, seeds=None):
        self.name = name
        self.width = w = S.BATCH[name]
        self.ns = w + 1
        self.spec, self.img = _image(gpu, name, self.ns * L)
        self.V = V = self.spec.vocab_size
        rng = np.random.default_rng(700 + S.SEEDS[name])
        self.prompts = [[int(t) for t in rng.choice(V, 2 + s % 2, replace=False)] for s in range(self.ns)]
        self.autos = [CR.random_automaton(V, CR.row_sizes(V), seed=sd) for sd in (seeds or SEEDS[name])] + [None]
        assert len(self.autos) == self.ns
        self.bias = []
        for a in self.autos:
            if a is None:
                self.bias.append({int(rng.integers(0, V)): -INF, int(rng.integers(0, V)): 0.75})
                continue
            # an ALLOWED token of the V/8 row that the rows of 1 and 2 ids do not hold: no row is emptied
            small = set(a.allowed(0).tolist()) | set(a.allowed(1).tolist())
            banned = next(int(t) for t in a.allowed(2) if int(t) not in small)
            up = next(int(t) for t in a.allowed(3) if int(t) != banned)
            self.bias.append({banned: -INF, up: 0.75})

    def setting(self, s, sampled, full):
        return Setting(auto=self.autos[s], samp=dict(SAMP, seed=900 + s) if sampled else None,
                       pen=PEN if full else None, bias=self.bias[s] if full else None)

    def kw(self, sampled, full):
        sts = [self.setting(s, sampled, full) for s in range(self.ns)]
        kw = dict(samplings=[st.samp for st in sts])
        if full:
            kw.update(penalties=[st.pen for st in sts], logit_bias=[st.bias for st in sts], logprobs=TOP)
        return kw


@pytest.mark.parametrize("name", NAMES)
def test_generate_batch_is_the_constrained_twin_per_sequence(gpu, name):
    b = Batch(gpu, name)
    spec, ns = b.spec, b.ns
    twin, raw = _mk(spec, b.img, flags=EXACT), _mk(spec, b.img, flags=EXACT)
    m = _mk(spec, b.img)
    assert m.seq_slots(ns) == L and m.seq_width() == b.width
    U, starts = union(b.autos)
    base = [st - a.start if a is not None else None for a, st in zip(b.autos, starts)]
    assert starts[-1] == -1 and len({x for x in base if x is not None}) == b.width
    m.seq_set_constraint(U)
    assert [m.seq_constraint_state(s) for s in range(ns)] == [-1] * ns
    for sampled, full in RUNS:
        what = (name, "sampled" if sampled else "greedy", "full" if full else "plain")
        top_n = TOP if full else None
        want = [twin_generate(twin, spec, b.prompts[s], STEPS, b.setting(s, sampled, full), top_n) for s in range(ns)]
        # the precondition, from the twin alone: else the run shows nothing
        for s in range(b.width):
            out = raw_argmax_outside(raw, b.autos[s], b.prompts[s], want[s][0])
            print(f"{what} sequence {s} (seed {SEEDS[name][s]}): raw argmax outside the row at {sum(out)} of {len(out)}")
            assert 2 * sum(out) >= len(out), what + (s,)
        for s in range(ns):
            m.seq_set_constraint_state(s, starts[s])
        _new_log()
        got, ms = m.generate_batch(b.prompts, STEPS, **b.kw(sampled, full))
        log = _ffi.launch_log()
        assert "k_seq_tail_fsm" in log and "k_seq_tail" not in log and "k_seq_pick" not in log, sorted(log)
        assert ms > 0
        for s in range(ns):
            words, rec, kv = want[s]
            n0 = len(b.prompts[s]) - 1
            assert got[s] == words, what + (s,)
            if full:
                _rec_same(m.seq_logprobs(s, 0, STEPS), rec, what + (s,))
            row0 = m.seq_row(s, 0)
            for layer in range(spec.n_layers):
                k, v = m.read_kv(layer, row0, STEPS)
                assert k.tobytes() == kv[layer][0].tobytes() and v.tobytes() == kv[layer][1].tobytes(), what + (s, layer)
            # the final state is the host walk of the words
            if b.autos[s] is None:
                assert m.seq_constraint_state(s) == -1
            else:
                end, n_ok = b.autos[s].walk(words[n0:])
                assert n_ok == STEPS - n0, what + (s, "a word outside the row of its state")
                assert m.seq_constraint_state(s) == base[s] + end, what + (s,)
    # constraints= builds the union, sets the starts, runs and turns the constraint off again
    m.seq_set_constraint(None)
    got, _ = m.generate_batch(b.prompts, STEPS, constraints=b.autos, **b.kw(True, True))
    assert got == [w[0] for w in want]
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.seq_constraint_state(0))
    for mm in (m, twin, raw):
        mm.close()


# ---- 2. seq_step by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "d"])
def test_seq_step_lanes_at_unrelated_positions(gpu, name):
    b = Batch(gpu, name)
    spec, ns, V, w = b.spec, b.ns, b.V, b.width
    twin = _mk(spec, b.img, flags=EXACT)
    m = _mk(spec, b.img, flags=EXACT)
    m.seq_slots(ns)
    rng = np.random.default_rng(40 + S.SEEDS[name])
    text = [[int(t) for t in rng.choice(V, L, replace=False)] for _ in range(ns)]
    pos = [int(p) for p in rng.permutation(L - 2)[:ns]]
    U, starts = union(b.autos)
    m.seq_set_constraint(U)
    for s in range(ns):
        if pos[s]:
            m.seq_prefill(s, text[s][:pos[s]])
    # lanes: slots w - 1 .. 0 in this order; every second one unconstrained, the others in some state of their automaton
    slots = list(range(w))[::-1]
    state = {}
    for s in slots:
        a = b.autos[s]
        state[s] = -1 if s % 2 else int(rng.integers(0, a.n_states))
        m.seq_set_constraint_state(s, (starts[s] - a.start + state[s]) if state[s] >= 0 else -1)
    for sampled in (False, True):
        sp = [dict(SAMP, seed=70 + s) if sampled else None for s in slots]
        want, after = [], []
        for s, samp in zip(slots, sp):
            a = b.autos[s]
            _twin_set(twin, Setting(), None)
            if pos[s]:
                twin.prefill(text[s][:pos[s]])
            twin.set_sampling(**(samp or {}))
            if state[s] >= 0:
                twin.set_constraint(a)
                twin.constraint_state = state[s]
            want.append(twin.predict(text[s][pos[s]], pos[s], exec="fused"))
            after.append(twin.constraint_state if state[s] >= 0 else -1)
        _new_log()
        got = m.seq_step(slots, [text[s][pos[s]] for s in slots], [pos[s] for s in slots], samplings=sp)
        log = _ffi.launch_log()
        assert "k_seq_tail_fsm" in log and "k_seq_pick" not in log and "k_seq_tail" not in log, sorted(log)
        assert got == want, (name, sampled)
        for s, t, st in zip(slots, got, after):
            off = starts[s] - b.autos[s].start
            assert m.seq_constraint_state(s) == (off + st if st >= 0 else -1), (name, sampled, s)
            if st >= 0:
                assert st == b.autos[s].step(state[s], t)
            # the same pass again from the same state
            m.seq_set_constraint_state(s, (off + state[s]) if state[s] >= 0 else -1)
    # a pass whose lanes are all at -1, the automaton still set: the plain tail, and the unconstrained picks
    free = [s for s in slots if state[s] < 0]
    _twin_set(twin, Setting(), None)
    want = []
    for s in free:
        if pos[s]:
            twin.prefill(text[s][:pos[s]])
        want.append(twin.predict(text[s][pos[s]], pos[s], exec="fused"))
    _new_log()
    got = m.seq_step(free, [text[s][pos[s]] for s in free], [pos[s] for s in free])
    log = _ffi.launch_log()
    assert "k_seq_pick" in log and "k_seq_tail_fsm" not in log and "k_seq_tail" not in log, sorted(log)
    assert got == want
    m.close()
    twin.close()


# ---- 3. fork and share -----------------------------------------------------------------------------------------------
def test_fork_carries_the_state_and_best_of_returns_listed_strings(gpu):
    spec, img = _image(gpu, "a", 8 * L)
    V = spec.vocab_size
    m, twin = _mk(spec, img, flags=EXACT), _mk(spec, img, flags=EXACT)
    m.seq_slots(8)
    A = CR.random_automaton(V, CR.row_sizes(V), seed=51)
    text = S.tokens("a", 6)
    m.seq_set_constraint(A)
    m.seq_prefill(0, text[:5])
    m.seq_set_constraint_state(0, 3)
    m.seq_fork(0, 1, 5)
    assert m.seq_constraint_state(1) == 3 and m.seq_constraint_state(2) == -1
    # in mid-generation: slot 0 moves on the device, the fork continues from where it is
    t = m.seq_step([0], [text[5]], [5])[0]
    s1 = A.step(3, t)
    assert s1 >= 0 and m.seq_constraint_state(0) == s1
    m.seq_fork(0, 2, 6)
    assert m.seq_constraint_state(2) == s1
    _new_log()
    both = m.seq_step([2, 0], [t, t], [6, 6])
    assert "k_seq_tail_fsm" in _ffi.launch_log()
    assert both[0] == both[1] and m.seq_constraint_state(2) == m.seq_constraint_state(0) == A.step(s1, both[0])
    # share leaves states alone, a new layout resets them
    m.seq_share(0, 3, 4)
    assert m.seq_constraint_state(0) == A.step(s1, both[0]) and m.seq_constraint_state(3) == -1
    m.seq_slots(8)
    assert [m.seq_constraint_state(s) for s in range(8)] == [-1] * 8
    m.seq_set_constraint(None)
    # best-of-4 over "one of these strings" on slots that share the prompt's rows
    eos = 2
    choices = [(700, 701, 702), (700, 701), (15, 1999, 3, 3, 8), (15, 4)]
    C_ = from_choices(choices, eos)
    prompt, total, seed = S.tokens("a", 4), 16, 300
    samp = dict(temperature=1.5, top_k=0, top_p=1.0, seed=seed)
    _new_log()
    best = m.best_of(prompt, 4, total, samp, stop=[eos], share=True, constraints=C_)
    assert "k_seq_tail_fsm" in _ffi.launch_log()
    n0 = len(prompt) - 1
    assert sorted(r["seed"] for r in best) == [seed + i for i in range(4)]
    for r in best:
        assert tuple(r["words"][n0:]) in choices, r
        _twin_set(twin, Setting(auto=C_, samp=dict(samp, seed=r["seed"])), 0)
        words, _ = twin.generate(prompt, total, exec="graph", stop=[eos])
        assert r["words"] == words, r
    assert len({tuple(r["words"]) for r in best}) > 1  # the seeds do not all draw one string
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.seq_constraint_state(0))  # turned off behind the call
    m.close()
    twin.close()


# ---- 4. the wide pass ------------------------------------------------------------------------------------------------
def test_wide_pass_picks_are_exact_on_the_masked_logits(gpu):
    n = 12  # two lane groups: 8 + 4
    spec, img = _image(gpu, "a", n * 16)
    V = spec.vocab_size
    assert V == 2048
    m = _mk(spec, img)
    m.seq_slots(n)
    assert m.seq_width(gemm=True) == 64
    autos = [CR.random_automaton(V, CR.row_sizes(V), seed=600 + s) for s in range(n - 1)] + [None]
    U, starts = union(autos)
    m.seq_set_constraint(U)
    for s in range(n):
        m.seq_set_constraint_state(s, starts[s])
    slots = list(range(n))
    sp = [dict(SAMP, seed=500 + s) if s % 2 else None for s in slots]
    toks = [int(t) for t in np.random.default_rng(6).integers(0, V, n)]
    state = list(starts)
    for p in range(8):
        _new_log()
        got = m.seq_step(slots, toks, [p] * n, samplings=sp, gemm=True)
        log = _ffi.launch_log()
        assert "k_seq_tail_fsm" in log and "k_seq_tail" not in log and "k_seq_pick" not in log, sorted(log)
        for i in range(n):
            row = m.seq_gemm_logits(i)
            if state[i] >= 0:
                inside = np.zeros(V, bool)
                inside[U.allowed(state[i])] = True
                assert np.isneginf(row[~inside]).all() and np.isfinite(row[inside]).all(), (p, i)
                assert inside[got[i]], (p, i)
            else:
                assert np.isfinite(row).all()
            if sp[i] is None:
                assert got[i] == int(np.argmax(row)), (p, i)  # the first maximum
            else:
                assert got[i] == ops.sample_host(torch.from_numpy(row).to(gpu), sp[i], counter=p), (p, i)
                ok = SR.Checker(row).accepts(sp[i]["temperature"], sp[i]["top_k"], sp[i]["top_p"], sp[i]["seed"], [p],
                                             [got[i]])
                assert ok.all(), (p, i)
            if state[i] >= 0:
                state[i] = U.step(state[i], got[i])
                assert state[i] >= 0
        assert [m.seq_constraint_state(s) for s in slots] == state, p
        toks = got
    # the loop: every word of a constrained sequence lies in the row of its state
    m.seq_set_constraint(None)
    prompts = [[toks[s], int(got[s])] for s in slots]
    words, _ = m.generate_batch(prompts, 12, samplings=sp, gemm=True, constraints=autos)
    for s in range(n - 1):
        assert autos[s].walk(words[s][1:])[1] == 11, s
    m.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def _calls(m, prompt):
    """what the launching sequence calls launch, on two slots"""
    m.seq_slots(4)
    m.seq_prefill(0, prompt[:2])
    m.seq_fork(0, 1, 2)
    m.seq_step([0, 1], [prompt[2], prompt[2]], [2, 2])
    m.seq_step([1, 0], [prompt[2], prompt[2]], [2, 2], samplings=[dict(SAMP, seed=1), None], logprobs=2)
    m.generate_batch([prompt, prompt[:2]], 8)
    m.generate_batch([prompt, prompt[:2]], 8, penalties=[PEN, None])
    m.seq_step([0, 1], [prompt[2], prompt[2]], [2, 2], gemm=True)


def test_refusals_come_before_any_launch_and_off_is_the_parent(gpu):
    spec, img = _image(gpu, "a", 8 * L)
    V = spec.vocab_size
    prompt = S.tokens("a", 3)
    fresh = _mk(spec, img)
    _new_log()
    _calls(fresh, prompt)
    log_fresh = _ffi.launch_log()
    assert "k_seq_pick" in log_fresh and "k_seq_tail" in log_fresh and "k_seq_tail_fsm" not in log_fresh
    fresh.close()
    m = _mk(spec, img)
    m.seq_slots(4)
    autos = [CR.random_automaton(V, CR.row_sizes(V), seed=80), CR.random_automaton(V, CR.row_sizes(V), seed=81)]
    U, starts = union(autos)
    _new_log()
    # the state calls need the constraint
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.seq_set_constraint_state(0, 0))
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.seq_constraint_state(0))
    # both constraints at once, in either order
    m.set_constraint(autos[0])
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.seq_set_constraint(U))
    m.set_constraint(None)
    m.seq_set_constraint(U)
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.set_constraint(autos[0]))
    # a state, or a slot, out of range
    for slot, st in ((0, -2), (0, U.n_states), (4, 0), (-1, 0)):
        _raises(_ffi.KH_ERR_RANGE, lambda: m.seq_set_constraint_state(slot, st))
    _raises(_ffi.KH_ERR_RANGE, lambda: m.seq_constraint_state(4))
    # an invalid automaton, and one whose mask table would pass KH_FSM_MAX_MASK_BYTES, leave the one in force
    _raises(_ffi.KH_ERR_RANGE, lambda: m.seq_set_constraint(TokenAutomaton(0, [0, 1], [V], [0])))
    _raises(_ffi.KH_ERR_INVALID_ARG, lambda: m.seq_set_constraint(TokenAutomaton(0, [0, 0, 1], [1], [0])))
    n_big = (256 << 20) // (4 * ((V + 31) // 32)) + 1
    big = TokenAutomaton(0, np.arange(n_big + 1), np.zeros(n_big, np.int32), np.zeros(n_big, np.int32))
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.seq_set_constraint(big))
    m.seq_set_constraint_state(0, starts[0])
    m.seq_set_constraint_state(1, starts[1])
    assert [m.seq_constraint_state(s) for s in range(4)] == [starts[0], starts[1], -1, -1]
    # a lane's -inf bias that empties a row of its own component; the same list against the other sequence's is fine
    two = {int(t): -INF for t in autos[0].allowed(1)}
    tk, ps = [prompt[0], prompt[0]], [0, 0]
    _raises(_ffi.KH_ERR_INVALID_ARG, lambda: m.seq_step([0, 1], tk, ps, logit_bias=[two, None]))
    _raises(_ffi.KH_ERR_INVALID_ARG, lambda: m.seq_step([1, 0], tk, ps, logit_bias=[None, two]))
    _raises(_ffi.KH_ERR_INVALID_ARG, lambda: m.seq_step([0, 1], tk, ps, logit_bias=[two, None], gemm=True))
    _raises(_ffi.KH_ERR_INVALID_ARG, lambda: m.generate_batch([prompt, prompt], 8, logit_bias=[two, None]))
    # the plain calls keep refusing the MODEL's own settings
    m.set_penalties(**PEN)
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.seq_step([0, 1], tk, ps))
    _raises(_ffi.KH_ERR_UNSUPPORTED, lambda: m.generate_batch([prompt, prompt], 8))
    m.set_penalties()
    assert _ffi.launch_log() == set(), _ffi.launch_log()  # nothing was launched by any of this
    got = m.seq_step([0, 1], tk, ps, logit_bias=[None, two])
    assert got[0] in autos[0].allowed(autos[0].start) and got[1] in autos[1].allowed(autos[1].start)
    assert got[1] not in two
    assert "k_seq_tail_fsm" in _ffi.launch_log()
    # off: every call launches what a fresh model launches
    m.seq_set_constraint(None)
    _new_log()
    _calls(m, prompt)
    assert _ffi.launch_log() == log_fresh, _ffi.launch_log() ^ log_fresh
    m.close()


# ---- 6. the gate -----------------------------------------------------------------------------------------------------
def test_the_fsm_tail_is_compiled_and_was_launched(gpu):
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    _LAUNCHED.update(_ffi.launch_log())
    notes = co.code_object_notes(_ffi.LIB_PATH)
    assert co.kernels(notes, {"k_seq_tail_fsm", "k_seq_tail"}) == {"k_seq_tail_fsm", "k_seq_tail"}
    assert "k_seq_tail_fsm" in _LAUNCHED, "run the whole module"
    scratch = {k: v for k, v in co.kernel_scratch(notes).items() if co.plain_name(k) == "k_seq_tail_fsm"}
    assert scratch and all(v == 0 for v in scratch.values()), scratch
