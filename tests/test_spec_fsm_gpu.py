"""Constrained lookup decode on the GPU: kh_model_verify_fsm (k_spec_fsm_rows, the pass, k_pf_cls, k_spec_tail_fsm,
k_spec_accept_fsm; csrc/kh_spec.h) and kh_model_generate_lookup_fsm, whose drafter is the automaton itself.

Every comparison is EXACT - token ids, counts, automaton states, log-prob records and K/V rows as raw bytes - and the
reference is always a TWIN model under the same set_constraint and set_* calls: a loop of predict(.., exec="fused")
for the pass, generate(.., exec="graph") for the loop.  The feature states no tolerance and neither does this file.

Models and helpers are tests/test_spec_gpu.py's and tests/test_spec_set_gpu.py's (the four of tests/score_cases.py:
(a) 8 per pass, (b) int8, 4 per pass, (c) Qwen2, (d) wide, 4 per pass, V = 2051 - logit rows off the 16-byte boundary
and a partly filled last mask word: the scalar path of kh_fsm_mask_span); the automata are tests/constraint_ref.py's.
Settings: nothing, S1 (sampler), S2w (penalties over the last 3), S5 (sampler + penalties + a -inf bias + log-probs 5).

S[p] is the automaton state position p is sampled in: S[0] = start, S[p + 1] = next(S[p], R[p + 1])."""
import subprocess

import numpy as np
import pytest
import torch

import constraint_ref as CR
import score_cases as S
import test_spec_gpu as G
import test_spec_set_gpu as SS
from kuiperllama_amd import _ffi, binfmt
from kuiperllama_amd.constraint import TokenAutomaton, from_choices
from kuiperllama_amd.model import lookup_draft_fsm

pytestmark = pytest.mark.gpu

EXACT = SS.EXACT
EOS = 2
KEYS = (None, "S1", "S2w", "S5")
# seeds of random_automaton at which the banned token of S5 leaves every row non-empty (asserted in _automaton)
SEED = {"a": 41, "b": 42, "c": 43, "d": 44}
_BAN, _REF, _TRUTH = {}, {}, {}


def _settings(key):
    return SS.SETTINGS[key] if key else {}


def _ban(gpu, name, key):
    if not _settings(key).get("ban"):
        return []
    if name not in _BAN:
        G._ref(gpu, name)
        _BAN[name] = SS._ban_list(gpu, name)
    return _BAN[name]


def _keeps_rows(A, ban):
    """set_logit_bias / set_constraint refuse a -inf list that empties a row"""
    return all(len(set(A.allowed(s).tolist()) - set(ban)) > 0 for s in range(A.n_states))


def _automaton(gpu, name):
    V = S.SPECS[name].vocab_size
    A = CR.random_automaton(V, CR.row_sizes(V), SEED[name])
    A.check(V)
    assert _keeps_rows(A, _ban(gpu, name, "S5")), (name, SEED[name])
    return A


def _constrained(gpu, name, key, A, **kw):
    m = G._model(gpu, name, **kw)
    SS._apply(m, _settings(key), _ban(gpu, name, key))
    m.set_constraint(A)
    return m


# ---- the token-by-token reference under a constraint and a setting, once per (model, setting, length) ---------------
def _ref(gpu, name, key, T=None):
    width = S.BATCH[name]
    T = T or max(SS.POS0) + width + 2
    if (name, key, T) not in _REF:
        G._ref(gpu, name)  # the image
        A = _automaton(gpu, name)
        twin = _constrained(gpu, name, key, A)
        R, states = [S.tokens(name, 1)[0]], [A.start]
        for p in range(T):
            R.append(twin.predict(R[p], p, exec="fused"))
            states.append(A.step(states[p], R[p + 1]))
            assert states[-1] >= 0, (name, key, p)
        assert twin.constraint_state == states[T]
        _REF[(name, key, T)] = {"A": A, "R": R, "S": states, "T": T,
                                "rec": twin.logprobs(0, T) if "lp" in _settings(key) else None,
                                "kv": [twin.read_kv(layer, 0, T) for layer in range(S.SPECS[name].n_layers)]}
        twin.close()
        if key is None:  # the mask decides words: the run is not the unconstrained one
            assert R[1:8] != G._REF[name]["R"][1:8], name
    return _REF[(name, key, T)]


# ---- 1. the pass ------------------------------------------------------------------------------------------------------
def _one_pass(m, r, name, key, pos0, n, k=None, kind="truth"):
    """kind: "truth" (accept all), "inside" (fed[k] in the row of its state, not the pick), "outside" (not in the row).
    -> False where the row leaves no such token (a row of 1 id has no second one, a row of V ids nothing outside)."""
    A, R, St, V, what = r["A"], r["R"], r["S"], S.SPECS[name].vocab_size, (name, key, pos0, n, k, kind)
    fed = list(R[pos0:pos0 + n])
    if k is not None:
        row = A.allowed(St[pos0 + k - 1]).tolist()  # fed[k] stands for the pick of position pos0 + k - 1
        if kind == "inside":
            cand = [t for t in row if t != R[pos0 + k]]
        else:
            inrow = set(row)
            cand = [t for t in range(V - 1, -1, -1) if t not in inrow][:1] if len(row) < V else []
        if not cand:
            return False
        fed[k] = cand[0]
    a_want = n - 1 if k is None else k - 1

    def run():
        if pos0:
            m.prefill(R[:pos0])
        m.constraint_state = St[pos0]
        return m.verify(fed, pos0, constrained=True)
    nxt, a = run()
    assert nxt.shape == (n,) and a == a_want, (what, a, nxt)
    assert list(nxt[:a + 1]) == R[pos0 + 1:pos0 + a + 2], what
    if kind == "outside":
        assert (nxt[k:] == -1).all() and (nxt[:k] >= 0).all(), (what, nxt)
    else:  # (behind a wrong token INSIDE the row the later fed tokens may or may not be followable)
        assert (nxt[:n if k is None else k + 1] >= 0).all(), (what, nxt)
    assert m.constraint_state == St[pos0 + a + 1], what  # = kh_fsm_walk from the state at entry over the owned picks
    assert A.walk(nxt[:a + 1], St[pos0]) == (St[pos0 + a + 1], a + 1), what
    SS._same_rows(m, r["kv"], pos0, a + 1, what)
    rec = None
    if r["rec"] is not None:
        rec = m.logprobs(pos0, n)
        assert SS._rec_bytes(rec, 0, a + 1) == SS._rec_bytes(r["rec"], pos0, pos0 + a + 1), what
        assert SS._is_none(rec, a + 1, n), what
    # a second identical pass: counters and row states were re-armed, nothing of the first one is in the way
    nxt2, a2 = run()
    assert a2 == a and nxt2.tobytes() == nxt.tobytes(), what
    if rec is not None:
        assert SS._rec_bytes(m.logprobs(pos0, n), 0, n) == SS._rec_bytes(rec, 0, n), what
    # rows, record, counters and the state word are right: the next step continues the twin's sequence
    p = pos0 + a + 1
    assert m.predict(int(nxt[a]), p, exec="fused") == R[p + 1], what
    assert m.constraint_state == St[p + 1], what
    if rec is not None:
        assert SS._rec_bytes(m.logprobs(p, 1), 0, 1) == SS._rec_bytes(r["rec"], p, p + 1), what
    return True


@pytest.mark.parametrize("name", G.NAMES)
@pytest.mark.parametrize("key", KEYS)
def test_pass_picks_what_the_constrained_token_loop_picks(gpu, name, key):
    r = _ref(gpu, name, key)
    width = S.BATCH[name]
    m = _constrained(gpu, name, key, r["A"])
    ran = {"truth": 0, "inside": 0, "outside": 0}
    for pos0 in SS.POS0:
        for n in range(1, width + 1):
            ran["truth"] += _one_pass(m, r, name, key, pos0, n)
            for k in sorted({k for k in (1, n // 2, n - 1) if 1 <= k < n}):
                for kind in ("inside", "outside"):
                    ran[kind] += _one_pass(m, r, name, key, pos0, n, k, kind)
    print(f"model ({name}) {key}: passes {ran}; row sizes met "
          f"{sorted({len(r['A'].allowed(s)) for s in r['S'][:max(SS.POS0) + width]})}")
    assert ran["truth"] == 2 * width and ran["inside"] >= width and ran["outside"] >= width, ran
    m.close()


def test_pass_across_the_time_split_threshold(gpu):
    r = _ref(gpu, "a", "S5", G.CROSS + 8 + 2)
    m = _constrained(gpu, "a", "S5", r["A"])
    assert _one_pass(m, r, "a", "S5", G.CROSS, 8)
    ks = [k for k in range(1, 8) if len(r["A"].allowed(r["S"][G.CROSS + k - 1])) < 2048]
    assert ks and _one_pass(m, r, "a", "S5", G.CROSS, 8, ks[len(ks) // 2], "outside")
    SS._same_rows(m, r["kv"], 0, G.CROSS + 1, "cross")
    m.close()


@pytest.mark.parametrize("key", [None, "S1"])
def test_pass_from_a_row_of_one_id_and_from_a_row_of_every_id(gpu, key):
    G._ref(gpu, "a")
    A, V = _automaton(gpu, "a"), 2048
    sizes = [len(A.allowed(s)) for s in range(A.n_states)]
    twin, m = _constrained(gpu, "a", key, A), _constrained(gpu, "a", key, A)
    for s0 in (sizes.index(1), sizes.index(V)):
        twin.constraint_state = s0
        Q = [S.tokens("a", 1)[0]]
        for p in range(8):
            Q.append(twin.predict(Q[p], p, exec="fused"))
        m.constraint_state = s0
        nxt, a = m.verify(Q[:8], 0, constrained=True)
        assert a == 7 and list(nxt) == Q[1:9], (key, s0)
        if sizes[s0] == 1:
            assert int(nxt[0]) == int(A.allowed(s0)[0])  # whatever the logits say
        assert m.constraint_state == twin.constraint_state == A.walk(Q[1:9], s0)[0]
    twin.close()
    m.close()


# ---- 2. the loop ------------------------------------------------------------------------------------------------------
def _template(V, rng, avoid):
    """a forced run of 6 tokens, then one free position whose row holds V / 8 ids; and round again"""
    ok = np.array([t for t in range(V) if t not in avoid])
    forced = rng.choice(ok, 6, replace=False)
    free = np.sort(rng.choice(ok, V // 8, replace=False)).astype(np.int32)
    rows = [(np.array([t], np.int32), np.array([j + 1], np.int32)) for j, t in enumerate(forced)]
    rows.append((free, np.zeros(len(free), np.int32)))
    row_ptr = np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])])
    return TokenAutomaton(0, row_ptr, np.concatenate([t for t, _ in rows]), np.concatenate([y for _, y in rows]))


def _loop_automaton(name, kind, ban):
    V = S.SPECS[name].vocab_size
    rng = np.random.default_rng(1000 + S.SEEDS[name])
    avoid = set(ban) | {EOS}
    if kind == "choices":  # three 20-token strings with a shared 2-token prefix
        ids = [int(t) for t in rng.choice(V, 80, replace=False) if int(t) not in avoid]
        A = from_choices([tuple(ids[:2] + ids[2 + 18 * i:20 + 18 * i]) for i in range(3)], EOS)
    elif kind == "template":
        A = _template(V, rng, avoid)
    else:  # no row with a single edge
        A = CR.random_automaton(V, [2, V // 8, 1024, 1025, V], SEED[name] + 100)
    A.check(V)
    assert _keeps_rows(A, ban), (name, kind)
    return A


def _truth(gpu, name, key, kind, A, P, T, stop=(), model=None):
    """the twin's generate (graph) under the constraint and the setting: words, records, K/V rows"""
    k = (name, key, kind, tuple(P), T, tuple(stop), model is not None)
    if k not in _TRUTH:
        twin = model(flags=EXACT) if model else G._model(gpu, name, flags=EXACT)
        SS._apply(twin, _settings(key), _ban(gpu, name, key))
        twin.set_constraint(A)
        W = twin.generate(P, T, exec="graph", stop=list(stop) or None)[0]
        _TRUTH[k] = {"W": W, "rec": twin.logprobs(0, T) if "lp" in _settings(key) else None,
                     "kv": [twin.read_kv(layer, 0, T) for layer in range(S.SPECS[name].n_layers)]}
        twin.close()
    return _TRUTH[k]


def _simulate(A, P, W, T, width, hint=None, ngram_max=4, ngram_min=1, miss_steps=8):
    """The loop's own bookkeeping replayed on the known text (no stop token), the host-tracked state included: the
    stats it must report when its words are W, and whether a plain step follows a pass - that step reads the state
    word k_spec_accept_fsm left."""
    text, n_prompt = G._text(P, W), len(P)
    start = n_prompt - 1 if 2 <= n_prompt - 1 < T else 0  # KH_FLAG_PREFILL_EXACT: the B-token prefill
    st = {"passes": 0, "drafted": 0, "accepted": 0, "plain_steps": 0, "forced": 0}
    p, s, behind_pass, step_behind_pass = start, A.start, False, False
    while p < T:
        sampled, first = p >= n_prompt - 1, p == start and start > 0
        d, forced = [], 0
        if sampled and not first:
            d, forced = lookup_draft_fsm(A, s, text[:p + 1], hint, ngram_max, ngram_min, min(width - 1, T - 1 - p))
        if d:
            a = 0
            while a < len(d) and d[a] == text[p + 1 + a]:
                a += 1
            st["passes"] += 1
            st["drafted"] += len(d)
            st["accepted"] += a
            st["forced"] += forced
            s, ok = A.walk(text[p + 1:p + a + 2], s)
            assert ok == a + 1
            p += a + 1
            behind_pass = True
        else:
            k = 1 if first else min(miss_steps or 8, T - p, 8) if sampled else min(n_prompt - 1 - p, T - p, 8)
            for q in range(p, p + k):
                if q >= n_prompt - 1:
                    s = A.step(s, text[q + 1])
                    assert s >= 0
            st["plain_steps"] += k if sampled else 0
            step_behind_pass |= behind_pass and sampled
            behind_pass = False
            p += k
    return st, step_behind_pass, s


def _run(m, t, A, P, T, width, what, hint=None):
    """one constrained lookup run of T steps against the first T positions of the twin's run"""
    W, n0 = t["W"][:T], len(P) - 1
    sim, behind, s_end = _simulate(A, P, W, T, width, hint)
    words, ms, st = m.generate_lookup(P, T, hint=hint, constrained=True)
    assert words == W, what
    assert st == sim, (what, st, sim)
    assert st["accepted"] + st["passes"] + st["plain_steps"] == T - n0 and st["forced"] <= st["drafted"], st
    if t["rec"] is not None:
        assert SS._rec_bytes(m.logprobs(0, T), n0, T) == SS._rec_bytes(t["rec"], n0, T), what
    SS._same_rows(m, t["kv"], 0, T, what)
    assert m.constraint_state == s_end == A.walk(W[n0:])[0], what  # behind the last owned pick
    return st, behind


def _steps_with_a_step_behind_a_pass(A, P, W, Tmax, width, hint=None):
    """the largest T <= Tmax at which the run ends in a plain step behind a pass (the last position drafts nothing)"""
    for T in range(Tmax, Tmax - 2 * width, -1):
        if _simulate(A, P, W[:T], T, width, hint)[1]:
            return T
    raise AssertionError("no run length ends in a step behind a pass")


@pytest.mark.parametrize("name", G.NAMES)
@pytest.mark.parametrize("key", [None, "S5"])
def test_constrained_lookup_generates_the_words_of_generate(gpu, name, key):
    G._ref(gpu, name)
    V, width, Tmax = S.SPECS[name].vocab_size, S.BATCH[name], 62
    P, ban = S.tokens(name, 6), _ban(gpu, name, key)
    m = G._model(gpu, name, flags=EXACT)
    SS._apply(m, _settings(key), ban)
    # (1) one of three 20-token strings: forced behind the branch, into the sink; no hint
    A = _loop_automaton(name, "choices", ban)
    m.set_constraint(A)
    t = _truth(gpu, name, key, "choices", A, P, Tmax)
    T = _steps_with_a_step_behind_a_pass(A, P, t["W"], Tmax, width)
    st, behind = _run(m, t, A, P, T, width, (name, key, "choices", T))
    assert behind and st["forced"] >= 30 and st["accepted"] == st["drafted"], st
    assert m.first_sample()["top1_id"] is not None  # the first sampled step ran alone, with the full classifier
    # ... and a stop token that arrives inside a pass: generate_until's n_words, the state behind the stop
    ts = _truth(gpu, name, key, "choices", A, P, Tmax, stop=(EOS,))
    assert ts["W"] == t["W"][:len(ts["W"])] and t["W"][len(ts["W"])] == EOS and len(ts["W"]) == 5 + 20
    words, _, st = m.generate_lookup(P, Tmax, stop=[EOS], constrained=True)
    assert words == ts["W"] and st["passes"] >= 1 and st["plain_steps"] == 1, (name, key, st)  # (the stop came in a pass)
    assert m.constraint_state == A.walk(ts["W"][5:] + [EOS])[0] == A.n_states - 1
    if ts["rec"] is not None:
        assert SS._rec_bytes(m.logprobs(0, len(words)), 5, len(words)) == SS._rec_bytes(ts["rec"], 5, len(words))
    SS._same_rows(m, ts["kv"], 0, len(words), (name, key, "stop"))
    # (2) the template: six forced tokens, one free position - with a truthful hint, a corrupted one and none
    A = _loop_automaton(name, "template", ban)
    m.set_constraint(A)
    t = _truth(gpu, name, key, "template", A, P, Tmax)
    hint = G._text(P, t["W"])
    bad = [(x + 1) % V if i % 3 == 2 else x for i, x in enumerate(hint)]
    for label, h in (("truth", hint), ("bad hint", bad), ("no hint", None)):
        T = _steps_with_a_step_behind_a_pass(A, P, t["W"], Tmax, width, h)
        st, behind = _run(m, t, A, P, T, width, (name, key, "template", label, T), h)
        assert behind and st["forced"] >= 20 and st["passes"] >= 5, (label, st)
    # (3) no forced row and no hint: whatever the text's own n-grams draft is cut to what the automaton follows
    A = _loop_automaton(name, "free", ban)
    m.set_constraint(A)
    t = _truth(gpu, name, key, "free", A, P, Tmax)
    st, _ = _run(m, t, A, P, Tmax, width, (name, key, "free"))
    assert st["forced"] == 0, st
    # a plain generate on the same model afterwards: the twin's words
    assert m.generate(P, Tmax, exec="graph")[0] == t["W"]
    m.close()


# ---- 3. launches ------------------------------------------------------------------------------------------------------
def _tail(log):
    return {k for k in log if k.startswith("k_spec")}


def test_launch_log_names_the_twins_only_under_a_constraint(gpu):
    r = G._ref(gpu, "a")
    T, P = G._steps("a"), S.tokens("a", 6)
    hint = G._text(P, G._truth(gpu, "a", P, T))
    fed = list(r["R"][:8])
    A = _loop_automaton("a", "template", [])
    m = G._model(gpu, "a", flags=EXACT)

    def logged(passes=False, **kw):
        _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
        st = m.generate_lookup(P, T, hint=hint, **kw)[2]
        assert st["passes"] >= 1 or not passes, st
        m.verify(fed, 0, **kw)
        return _tail(_ffi.launch_log())
    try:
        # the constraint off: exactly the _as_set launches, with nothing set and with settings on
        assert logged(True, constrained=True) == logged(True, as_set=True) == {"k_spec_pick", "k_spec_accept"}
        m.set_sampling(*SS.SAMP)
        assert logged(constrained=True) == logged(as_set=True) == {"k_spec_tail", "k_spec_accept_set"}
        m.set_penalties(**SS.PEN)
        assert logged(constrained=True) == logged(as_set=True) == {"k_spec_hist", "k_spec_tail", "k_spec_accept_set"}
        # on: the three twins and none of the others - with the settings, and with nothing else set
        twins = {"k_spec_fsm_rows", "k_spec_tail_fsm", "k_spec_accept_fsm"}
        m.set_constraint(A)
        assert logged(True, constrained=True) == twins
        m.set_sampling()
        m.set_penalties()
        assert logged(True, constrained=True) == twins
        # the four calls without _fsm refuse as before, ahead of any launch
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        for call in (lambda: m.verify(fed, 0), lambda: m.verify(fed, 0, as_set=True),
                     lambda: m.generate_lookup(P, T, hint=hint), lambda: m.generate_lookup(P, T, hint=hint, as_set=True)):
            with pytest.raises(_ffi.KhError) as ei:
                call()
            assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
        assert _ffi.launch_log() == set()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


def test_errors_come_before_any_launch_and_the_slot_constraint_is_not_read(gpu):
    r = G._ref(gpu, "a")
    R, V = r["R"], 2048
    A = _automaton(gpu, "a")
    m = G._model(gpu, "a", flags=EXACT)
    m.set_constraint(A)
    cap = m.cfg.cache_len
    try:
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        for call, want in ((lambda: m.verify(R[:9], 0, constrained=True), _ffi.KH_ERR_RANGE),          # n above the width
                           (lambda: m.verify([R[0], V, R[1]], 0, constrained=True), _ffi.KH_ERR_RANGE),  # outside the vocabulary
                           (lambda: m.verify([R[0], -1], 0, constrained=True), _ffi.KH_ERR_RANGE),
                           (lambda: m.verify(R[:4], cap - 3, constrained=True), _ffi.KH_ERR_RANGE),      # past the cache
                           (lambda: m.verify([], 0, constrained=True), _ffi.KH_ERR_INVALID_ARG),
                           (lambda: m.verify(R[:4], -1, constrained=True), _ffi.KH_ERR_INVALID_ARG),
                           (lambda: m.generate_lookup(R[:4], cap + 1, constrained=True), _ffi.KH_ERR_RANGE),
                           (lambda: m.generate_lookup(R[:4], 16, hint=[0, V], constrained=True), _ffi.KH_ERR_RANGE),
                           (lambda: m.generate_lookup(R[:4], 16, miss_steps=9, constrained=True), _ffi.KH_ERR_INVALID_ARG),
                           (lambda: m.generate_lookup([], 16, constrained=True), _ffi.KH_ERR_INVALID_ARG)):
            with pytest.raises(_ffi.KhError) as ei:
                call()
            assert ei.value.code == want
        assert _ffi.launch_log() == set()
        assert m.constraint_state == A.start
        # the per-sequence constraint alone: the _as_set pass, no mask
        m.set_constraint(None)
        m.seq_set_constraint(A)
        fed = list(R[:8])
        fed[5] = (fed[5] + 1) % V
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        got, want = m.verify(fed, 0, constrained=True), m.verify(fed, 0, as_set=True)
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] == 4 and list(got[0][:5]) == R[1:6]
        assert _tail(_ffi.launch_log()) == {"k_spec_pick", "k_spec_accept"}
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


# ---- 4. W16: the pass reads the 16-bit copy, the tail does not care ---------------------------------------------------
def test_constrained_lookup_on_a_w16_model(gpu):
    spec, Tmax = S.SPECS["a"], 62
    img = binfmt.synth_image(spec, seed=S.SEEDS["a"], device=gpu, final_norm_std=1.0)
    binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()

    def make(flags):
        return G.KuiperModel.from_device_image(img, spec, max_seq_len=spec.seq_len, flags=flags)
    P = S.tokens("a", 6)
    A = _loop_automaton("a", "template", [])
    t = _truth(gpu, "a", "S2w", "template-w16", A, P, Tmax, model=make)  # the fp32 twin on the same image
    m = make(EXACT | _ffi.KH_FLAG_W16)
    assert m.w16_info()["state"] == 1 and m.w16_pass_info()["classes"], (m.w16_info(), m.w16_pass_info())
    SS._apply(m, SS.SETTINGS["S2w"])
    m.set_constraint(A)
    T = _steps_with_a_step_behind_a_pass(A, P, t["W"], Tmax, 8)
    st, behind = _run(m, t, A, P, T, 8, "w16")
    # (the text repeats its forced runs, so the n-gram rule drafts the free positions from them, and may be wrong there)
    assert behind and st["forced"] >= 20 and st["accepted"] >= st["forced"], st
    m.close()


# ---- 5. demo CLI ------------------------------------------------------------------------------------------------------
def test_demo_cli_lookup_constrained_prints_the_words_of_the_run_without_lookup(gpu, tmp_path):
    from kuiperllama_amd import build
    G._ref(gpu, "a")
    spec, P = S.SPECS["a"], S.tokens("a", 6)
    choices = [(700, 701, 702, 703, 704, 705, 706, 707), (700, 701, 15, 1999, 3, 3, 8), (700, 701, 9)]
    path = tmp_path / "m.bin"
    G._REF["a"]["img"].cpu().numpy().tofile(path)
    exe = build.build_demo()
    base = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--exact-prefill", "--max-seq-len", str(spec.seq_len), "--steps", "32", "--prompt", ",".join(map(str, P)),
            "--stop", str(EOS), "--choices", ";".join(",".join(map(str, c)) for c in choices),
            "--temperature", str(SS.SAMP[0]), "--seed", str(SS.SAMP[3])]

    def words(args, mark):
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.strip().splitlines()
        at = next(i for i, ln in enumerate(lines) if ln.startswith(mark))
        return [int(x) for x in lines[at - 1].split()], lines[at]
    plain, _ = words(base, "steps/s:")
    spec_, stats = words(base + ["--lookup-constrained", "3"], "lookup:")
    assert spec_ == plain and tuple(plain[5:]) in choices, (plain, spec_)
    f = stats.split()
    st = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
    assert st["forced"] >= 1 and st["accepted"] == st["drafted"] >= st["forced"], stats
    bad = subprocess.run(base + ["--lookup-as-set"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0  # the calls without _fsm know no automaton: refused, not rerouted
