"""Speculative decode under the model's settings on the GPU: kh_model_verify_as_set (the pass, k_pf_cls, k_spec_hist,
k_spec_tail, k_spec_accept_set; csrc/kh_spec.h) and kh_model_generate_lookup_as_set.

Every comparison is EXACT - token ids, counts, log-prob records and K/V rows as raw bytes - and the reference is always
a TWIN model under the same set_* calls: a loop of predict(.., exec="fused") for the pass, generate(.., exec="graph")
for the loop.  A draft is accepted where it equals the pick the settings make, the seeded draw included, so the words
are the twin's: the feature states no tolerance and neither does this file.

Models, case generator and helpers are tests/test_spec_gpu.py's (the four of tests/score_cases.py).  Settings:
  S1   sampler only: T 0.8, top-k 50, top-p 0.95, a seed
  S2   greedy with penalties 1.3 / 0.2 / 0.1 over every fed token (S2) and over the last 3 (S2w: the window starts
       inside a pass, so the pass's own tokens alone decide the counts)
  S3   greedy with a bias list that bans, with -inf, the token the raw logits pick at the first verified position
       (position 0 of the first case: the pick there is the runner-up, and the ban holds at every later position)
  S4   greedy with log-probs, top_n 0 (S4) and 5 (S4t)
  S5   S1 + S2w + S3 + log-probs 5

What the pass test cannot see: predict() feeds its own token (set_state), so the entry hist[pos0 + a + 1] that the
accept launch leaves for the next step's penalty window is checked by the loop tests, where graph steps follow a pass
without any host-side reset (_simulate asserts that such a step exists in the runs that matter)."""
import subprocess

import numpy as np
import pytest
import torch

import score_cases as S
import test_spec_gpu as G
from kuiperllama_amd import _ffi, binfmt
from kuiperllama_amd.model import lookup_draft

pytestmark = pytest.mark.gpu

INF = float("inf")
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
SAMP = (0.8, 50, 0.95, 0xC0FFEE)
PEN = dict(repetition=1.3, presence=0.2, frequency=0.1)
SETTINGS = {
    "S1": dict(samp=SAMP),
    "S2": dict(pen=dict(PEN, last_n=0)),
    "S2w": dict(pen=dict(PEN, last_n=3)),
    "S3": dict(ban=True),
    "S4": dict(lp=0),
    "S4t": dict(lp=5),
    "S5": dict(samp=SAMP, pen=dict(PEN, last_n=3), ban=True, lp=5),
}
POS0 = (0, 5)  # G._cases


def _apply(m, st, ban=()):
    if "samp" in st:
        m.set_sampling(*st["samp"])
    if "pen" in st:
        m.set_penalties(**st["pen"])
    if ban:
        m.set_logit_bias({int(t): -INF for t in ban})
    if "lp" in st:
        m.set_logprobs(st["lp"])


def _predict_loop(m, t0, T):
    R = [t0]
    for p in range(T):
        R.append(m.predict(R[p], p, exec="fused"))
    return R


def _rec_bytes(rec, lo, hi):
    return tuple(rec[f][lo:hi].tobytes() for f in ("token", "logprob", "top_ids", "top_logprobs"))


def _is_none(rec, lo, hi):
    return ((rec["token"][lo:hi] == -1).all() and (rec["top_ids"][lo:hi] == -1).all()
            and (rec["logprob"][lo:hi].view(np.uint32) == 0xFFFFFFFF).all()
            and (rec["top_logprobs"][lo:hi].view(np.uint32) == 0xFFFFFFFF).all())


# ---- the token-by-token reference under a setting, once per (model, setting) ----------------------------------------
_REF = {}


def _ban_list(gpu, name):
    """S3: the token the RAW logits pick at the first verified position - position 0, behind the model's first token,
    whatever the settings are"""
    raw = G._model(gpu, name)
    pick = raw.predict(S.tokens(name, 1)[0], 0, exec="fused")
    raw.close()
    return [pick]


def _ref(gpu, name, key):
    if (name, key) not in _REF:
        G._ref(gpu, name)  # the image
        st, width = SETTINGS[key], S.BATCH[name]
        T = G.CROSS + width + 2 if (name, key) == ("a", "S5") else max(POS0) + width + 2
        ban = _ban_list(gpu, name) if st.get("ban") else []
        twin = G._model(gpu, name)
        _apply(twin, st, ban)
        R = _predict_loop(twin, S.tokens(name, 1)[0], T)
        r = {"st": st, "ban": ban, "R": R, "T": T,
             "rec": twin.logprobs(0, T) if "lp" in st else None,
             "kv": [twin.read_kv(layer, 0, T) for layer in range(S.SPECS[name].n_layers)]}
        twin.close()
        assert not set(ban) & set(R[1:]), (name, key, ban)  # without processing R[1] would be visibly different
        _REF[(name, key)] = r
    return _REF[(name, key)]


def _same_rows(m, kv, row0, nrows, what):
    for layer, (k, v) in enumerate(kv):
        gk, gv = m.read_kv(layer, row0, nrows)
        assert gk.tobytes() == k[row0:row0 + nrows].tobytes(), (what, layer, row0, nrows, "K")
        assert gv.tobytes() == v[row0:row0 + nrows].tobytes(), (what, layer, row0, nrows, "V")


# ---- 1. the pass ------------------------------------------------------------------------------------------------------
def _one_pass(m, r, name, key, pos0, n, k):
    R, V, what = r["R"], S.SPECS[name].vocab_size, (name, key, pos0, n, k)
    if pos0:
        m.prefill(R[:pos0])
    fed = list(R[pos0:pos0 + n])
    if k is not None:
        fed[k] = (R[pos0 + k] + 1) % V
    nxt, a = m.verify(fed, pos0, as_set=True)
    assert nxt.shape == (n,)
    assert a == (n - 1 if k is None else k - 1), what
    assert list(nxt[:a + 1]) == R[pos0 + 1:pos0 + a + 2], what
    _same_rows(m, r["kv"], pos0, a + 1, what)
    rec = None
    if r["rec"] is not None:
        rec = m.logprobs(pos0, n)
        assert _rec_bytes(rec, 0, a + 1) == _rec_bytes(r["rec"], pos0, pos0 + a + 1), what
        assert _is_none(rec, a + 1, n), what
    # a second identical pass: the counters were re-armed, nothing of the first one is in the way
    nxt2, a2 = m.verify(fed, pos0, as_set=True)
    assert a2 == a and nxt2.tobytes() == nxt.tobytes(), what
    if rec is not None:
        assert _rec_bytes(m.logprobs(pos0, n), 0, n) == _rec_bytes(rec, 0, n), what
    # accepted rows, fed-token record and counters are right: the next step continues the twin's sequence
    p = pos0 + a + 1
    assert m.predict(int(nxt[a]), p, exec="fused") == R[p + 1], what
    if rec is not None:
        assert _rec_bytes(m.logprobs(p, 1), 0, 1) == _rec_bytes(r["rec"], p, p + 1), what


PASS_CASES = [(n, "S5") for n in G.NAMES] + [("a", k) for k in ("S1", "S2", "S2w", "S3", "S4", "S4t")]


@pytest.mark.parametrize("name,key", PASS_CASES)
def test_pass_picks_what_the_token_loop_picks(gpu, name, key):
    r = _ref(gpu, name, key)
    m = G._model(gpu, name)
    _apply(m, r["st"], r["ban"])
    for pos0, n, k in G._cases(S.BATCH[name]):
        _one_pass(m, r, name, key, pos0, n, k)
    m.close()


def test_pass_across_the_time_split_threshold(gpu):
    r = _ref(gpu, "a", "S5")
    m = G._model(gpu, "a")
    _apply(m, r["st"], r["ban"])
    _one_pass(m, r, "a", "S5", G.CROSS, 8, None)
    _one_pass(m, r, "a", "S5", G.CROSS, 8, 5)
    _same_rows(m, r["kv"], 0, G.CROSS + 5, "cross")
    m.close()


# ---- 2. the loop ------------------------------------------------------------------------------------------------------
_TRUTH = {}


def _loop_ban(gpu, name, st):
    return _ref(gpu, name, "S5" if "samp" in st else "S3")["ban"] if st.get("ban") else []


def _truth(gpu, name, key, prompt, T, stop=(), model=None):
    """the twin's generate (graph) under the setting: words, records of every position, K/V rows"""
    k = (name, key, tuple(prompt), T, tuple(stop), model is not None)
    if k not in _TRUTH:
        G._ref(gpu, name)
        st = SETTINGS[key]
        twin = model(flags=EXACT) if model else G._model(gpu, name, flags=EXACT)
        _apply(twin, st, _loop_ban(gpu, name, st))
        W = twin.generate(prompt, T, exec="graph", stop=list(stop) or None)[0]
        _TRUTH[k] = {"W": W, "rec": twin.logprobs(0, T) if "lp" in st else None,
                     "kv": [twin.read_kv(layer, 0, T) for layer in range(S.SPECS[name].n_layers)]}
        twin.close()
    return _TRUTH[k]


def _simulate(P, W, T, width, hint=None, ngram_max=4, ngram_min=1, miss_steps=8):
    """The loop's own bookkeeping replayed on the known text (no stop token): the stats it must report when its words
    are W, and whether a plain step follows a pass (it reads the state and the fed-token record the pass left)."""
    text, n_prompt = G._text(P, W), len(P)
    start = n_prompt - 1 if 2 <= n_prompt - 1 < T else 0  # KH_FLAG_PREFILL_EXACT: the B-token prefill
    st = {"passes": 0, "drafted": 0, "accepted": 0, "plain_steps": 0}
    p, behind_pass, step_behind_pass = start, False, False
    while p < T:
        sampled, first = p >= n_prompt - 1, p == start and start > 0
        d = []
        if sampled and not first:
            d = lookup_draft(text[:p + 1], hint, ngram_max, ngram_min, min(width - 1, T - 1 - p))
        if d:
            a = 0
            while a < len(d) and d[a] == text[p + 1 + a]:
                a += 1
            st["passes"] += 1
            st["drafted"] += len(d)
            st["accepted"] += a
            p += a + 1
            behind_pass = True
        else:
            k = 1 if first else min(miss_steps or 8, T - p, 8) if sampled else min(n_prompt - 1 - p, T - p, 8)
            st["plain_steps"] += k if sampled else 0
            step_behind_pass |= behind_pass
            behind_pass = False
            p += k
    return st, step_behind_pass


def _check_run(m, t, out, n_prompt, what, sim=None):
    words, ms, st = out
    W = t["W"]
    assert words == W, what
    if sim is not None:
        assert st == sim, (what, st, sim)
        G._check(words, st, W, n_prompt)
    if t["rec"] is not None:
        lo, hi = n_prompt - 1, len(W)
        assert _rec_bytes(m.logprobs(0, hi), lo, hi) == _rec_bytes(t["rec"], lo, hi), what
    _same_rows(m, t["kv"], 0, len(W), what)


LOOP_CASES = [(n, k) for n in G.NAMES for k in ("S1", "S2w", "S5")]


@pytest.mark.parametrize("name,key", LOOP_CASES)
def test_lookup_as_set_generates_the_words_of_generate(gpu, name, key):
    st_, V, width, T = SETTINGS[key], S.SPECS[name].vocab_size, S.BATCH[name], G._steps(name)
    P = S.tokens(name, 6)
    t = _truth(gpu, name, key, P, T)
    W = t["W"]
    assert len(W) == T
    m = G._model(gpu, name, flags=EXACT)
    _apply(m, st_, _loop_ban(gpu, name, st_))
    # the truth as the hint: behind the plain first step the first pass is deterministic, and under exactness the
    # seeded draws reproduce the truth - every draft of it is accepted
    hint = G._text(P, W)
    sim, _ = _simulate(P, W, T, width, hint)
    out = m.generate_lookup(P, T, hint=hint, as_set=True)
    _check_run(m, t, out, 6, (name, key, "truth"), sim)
    assert out[2]["accepted"] >= width - 1 and out[2]["passes"] >= 1 and out[1] > 0, out[2]
    assert m.first_sample()["top1_id"] is not None  # the first sampled step ran alone, with the full classifier
    # every third token of the hint wrong
    bad = [(x + 1) % V if i % 3 == 2 else x for i, x in enumerate(hint)]
    sim, _ = _simulate(P, W, T, width, bad)
    _check_run(m, t, m.generate_lookup(P, T, hint=bad, as_set=True), 6, (name, key, "bad hint"), sim)
    # the hint ends inside the text and only 6-grams are searched: passes, then steps on the step graphs behind them
    cut = hint[:6 + width + 2]
    for miss in (1, 8):
        sim, behind = _simulate(P, W, T, width, cut, 6, 6, miss)
        out = m.generate_lookup(P, T, hint=cut, ngram_max=6, ngram_min=6, miss_steps=miss, as_set=True)
        _check_run(m, t, out, 6, (name, key, "cut hint", miss), sim)
        assert behind and out[2]["passes"] >= 1 and out[2]["plain_steps"] >= 2, (name, key, out[2])
    # no hint at all, nothing to find but exact 6-grams
    for miss in (1, 8):
        sim, _ = _simulate(P, W, T, width, None, 6, 6, miss)
        out = m.generate_lookup(P, T, ngram_max=6, ngram_min=6, miss_steps=miss, as_set=True)
        _check_run(m, t, out, 6, (name, key, "no hint", miss), sim)
    # the last pass is clipped by total_steps
    Tc = 6 + width + 3
    tc = _truth(gpu, name, key, P, Tc)
    assert tc["W"] == W[:Tc]
    sim, _ = _simulate(P, tc["W"], Tc, width, hint)
    _check_run(m, tc, m.generate_lookup(P, Tc, hint=hint, as_set=True), 6, (name, key, "clipped"), sim)
    # a stop token inside an accepted run (the first sampled word from index 3 on that has not occurred earlier)
    sampled = W[5:]
    new = [i for i in range(len(sampled)) if sampled[i] not in sampled[:i]]
    i = next((i for i in new if i >= 3), new[-1])
    ts = _truth(gpu, name, key, P, T, stop=(sampled[i],))
    assert ts["W"] == W[:5 + i]
    out = m.generate_lookup(P, T, stop=[sampled[i]], hint=hint, as_set=True)
    _check_run(m, ts, out, 6, (name, key, "stop", i))
    assert out[2]["passes"] >= 1, out[2]
    # a plain generate on the same model afterwards: the twin's words
    assert m.generate(P, T, exec="graph")[0] == W
    m.close()


@pytest.mark.parametrize("name,key", LOOP_CASES)
def test_lookup_as_set_drafts_from_a_periodic_prompt(gpu, name, key):
    st_, width, T = SETTINGS[key], S.BATCH[name], G._steps(name) + 2
    P = [5, 9] * 4
    t = _truth(gpu, name, key, P, T)
    m = G._model(gpu, name, flags=EXACT)
    _apply(m, st_, _loop_ban(gpu, name, st_))
    for miss in (8, 1):
        sim, _ = _simulate(P, t["W"], T, width, miss_steps=miss)
        out = m.generate_lookup(P, T, miss_steps=miss, as_set=True)
        _check_run(m, t, out, 8, (name, key, "periodic", miss), sim)
    # by the drafter's definition: with one step per miss the loop visits every position behind the plain first step
    # until one drafts (with 8 it asks at every eighth only, and what it finds there is the text's business)
    text = G._text(P, t["W"])
    expect = any(lookup_draft(text[:p + 1], None, 4, 1, 1) for p in range(8, T - 1))
    print(f"model ({name}) {key}: a draft is due: {expect}; stats {out[2]}")
    # Whether one does is the text's business: 11 of these 12 twins repeat a token among their sampled words; model (d)
    # under S5 does not in its 17, no draft is due there, and a correct loop drafts nothing (stats == sim above holds
    # either way).  So the requirement is the equivalence, and that the text did not change under the other eleven.
    assert (out[2]["drafted"] > 0) == expect, out[2]
    assert expect or (name, key) == ("d", "S5"), "the twin's text changed: see the comment above"
    m.close()


def test_lookup_as_set_long_run_crosses_the_time_split_threshold(gpu):
    P, T = S.tokens("a", 6), S.LONG_N
    t = _truth(gpu, "a", "S5", P, T)
    m = G._model(gpu, "a", flags=EXACT)
    _apply(m, SETTINGS["S5"], _loop_ban(gpu, "a", SETTINGS["S5"]))
    hint = G._text(P, t["W"])
    sim, _ = _simulate(P, t["W"], T, 8, hint)
    out = m.generate_lookup(P, T, hint=hint, as_set=True)
    _check_run(m, t, out, 6, "long", sim)
    assert out[2]["accepted"] >= 7 and out[2]["passes"] < T - 5, out[2]
    m.close()


# ---- 3. neutral and unchanged -----------------------------------------------------------------------------------------
def _tail(log):
    return {k for k in log if k.startswith("k_spec")}


def test_nothing_set_is_the_plain_path(gpu):
    r = G._ref(gpu, "a")
    R, V, T = r["R"], S.SPECS["a"].vocab_size, G._steps("a")
    P = S.tokens("a", 6)
    W = G._truth(gpu, "a", P, T)
    hint = G._text(P, W)
    m = G._model(gpu, "a", flags=EXACT)
    fed = list(R[:8])
    fed[5] = (fed[5] + 1) % V
    plain, neutral = m.verify(fed, 0), m.verify(fed, 0, as_set=True)
    assert neutral[0].tobytes() == plain[0].tobytes() and neutral[1] == plain[1] == 4
    try:
        _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
        w0, _, s0 = m.generate_lookup(P, T, hint=hint)
        log_plain = set(_ffi.launch_log())
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        w1, _, s1 = m.generate_lookup(P, T, hint=hint, as_set=True)
        m.verify(fed, 0, as_set=True)
        log = set(_ffi.launch_log())
        assert (w1, s1) == (w0, s0) and w0 == W
        # (the first run also captured the step graphs: compare the launches of the pass's tail only)
        assert _tail(log) == _tail(log_plain) == {"k_spec_pick", "k_spec_accept"}, sorted(log ^ log_plain)
        # a setting made and taken back is neutral again; one that is on selects the tail
        m.set_sampling(*SAMP)
        m.set_sampling()
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        assert m.generate_lookup(P, T, hint=hint, as_set=True)[0] == W
        assert "k_spec_tail" not in _ffi.launch_log()
        m.set_sampling(*SAMP)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        m.generate_lookup(P, T, hint=hint, as_set=True)
        log = set(_ffi.launch_log())
        assert {"k_spec_tail", "k_spec_accept_set"} <= log and not {"k_spec_pick", "k_spec_accept", "k_spec_hist"} & log
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


def test_plain_calls_still_refuse_and_new_calls_check_their_arguments(gpu):
    r = G._ref(gpu, "a")
    R, V, T = r["R"], S.SPECS["a"].vocab_size, G._steps("a")
    P = S.tokens("a", 6)
    m = G._model(gpu, "a", flags=EXACT)
    cap = m.cfg.cache_len
    m.set_sampling(*SAMP)
    m.prefill(R[:4])
    sentinel = [m.read_kv(layer, 0, 12) for layer in range(S.SPECS["a"].n_layers)]

    def code(call):
        with pytest.raises(_ffi.KhError) as ei:
            call()
        for layer, (k, v) in enumerate(sentinel):  # before any launch
            gk, gv = m.read_kv(layer, 0, 12)
            assert gk.tobytes() == k.tobytes() and gv.tobytes() == v.tobytes()
        return ei.value.code
    assert code(lambda: m.generate_lookup(P, T, hint=R[:8])) == _ffi.KH_ERR_UNSUPPORTED
    assert code(lambda: m.verify([], 0, as_set=True)) == _ffi.KH_ERR_INVALID_ARG
    assert code(lambda: m.verify(R[:4], -1, as_set=True)) == _ffi.KH_ERR_INVALID_ARG
    assert code(lambda: m.verify(R[:9], 0, as_set=True)) == _ffi.KH_ERR_RANGE
    assert code(lambda: m.verify(R[:4], cap - 3, as_set=True)) == _ffi.KH_ERR_RANGE
    assert code(lambda: m.verify([R[0], V, R[1]], 0, as_set=True)) == _ffi.KH_ERR_RANGE
    assert code(lambda: m.verify([R[0], -1], 0, as_set=True)) == _ffi.KH_ERR_RANGE
    assert code(lambda: m.generate_lookup([], T, as_set=True)) == _ffi.KH_ERR_INVALID_ARG
    assert code(lambda: m.generate_lookup(P, T, miss_steps=9, as_set=True)) == _ffi.KH_ERR_INVALID_ARG
    assert code(lambda: m.generate_lookup(P, T, ngram_max=1, ngram_min=2, as_set=True)) == _ffi.KH_ERR_INVALID_ARG
    assert code(lambda: m.generate_lookup(P, T, hint=[0, V], as_set=True)) == _ffi.KH_ERR_RANGE
    assert code(lambda: m.generate_lookup(P, cap + 1, as_set=True)) == _ffi.KH_ERR_RANGE
    assert code(lambda: m.generate_lookup([P[0], V], T, as_set=True)) == _ffi.KH_ERR_RANGE
    m.close()
    # a geometry outside the pass (head size 32): only the geometry predicate is left
    spec, img, gt, _ = G.load_golden("hf_llama_half")
    g = G.KuiperModel.from_host_image(img, spec)
    g.set_sampling(*SAMP)
    for call in (lambda: g.verify([int(x) for x in gt[:4]], 0, as_set=True),
                 lambda: g.generate_lookup([int(x) for x in gt[:4]], 12, as_set=True)):
        with pytest.raises(_ffi.KhError) as ei:
            call()
        assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
    g.close()


# ---- 4. W16: the pass reads the 16-bit copy, the tail does not care ---------------------------------------------------
def test_lookup_as_set_on_a_w16_model(gpu):
    spec, T = S.SPECS["a"], G._steps("a")
    img = binfmt.synth_image(spec, seed=S.SEEDS["a"], device=gpu, final_norm_std=1.0)
    binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()

    def make(flags):
        return G.KuiperModel.from_device_image(img, spec, max_seq_len=spec.seq_len, flags=flags)
    P = S.tokens("a", 6)
    t = _truth(gpu, "a", "S2w", P, T, model=make)  # the fp32 twin on the same image
    m = make(EXACT | _ffi.KH_FLAG_W16)
    assert m.w16_info()["state"] == 1 and m.w16_pass_info()["classes"], (m.w16_info(), m.w16_pass_info())
    _apply(m, SETTINGS["S2w"])
    hint = G._text(P, t["W"])
    sim, _ = _simulate(P, t["W"], T, 8, hint)
    out = m.generate_lookup(P, T, hint=hint, as_set=True)
    _check_run(m, t, out, 6, "w16", sim)
    assert out[2]["accepted"] >= 7 and out[2]["passes"] >= 1, out[2]
    m.close()


# ---- 5. demo CLI ------------------------------------------------------------------------------------------------------
def test_demo_cli_lookup_as_set_prints_the_words_of_the_run_without_lookup(gpu, tmp_path):
    from kuiperllama_amd import build
    spec, T = S.SPECS["a"], G._steps("a")
    P = S.tokens("a", 6)
    t = _truth(gpu, "a", "S1", P, T)
    path = tmp_path / "m.bin"
    G._REF["a"]["img"].cpu().numpy().tofile(path)
    exe = build.build_demo()
    base = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--exact-prefill", "--max-seq-len", str(spec.seq_len), "--steps", str(T), "--prompt", ",".join(map(str, P)),
            "--temperature", str(SAMP[0]), "--top-k", str(SAMP[1]), "--top-p", str(SAMP[2]), "--seed", str(SAMP[3])]

    def words(args, mark):
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.strip().splitlines()
        at = next(i for i, ln in enumerate(lines) if ln.startswith(mark))
        return [int(x) for x in lines[at - 1].split()], lines[at]
    plain, _ = words(base, "steps/s:")
    spec_, stats = words(base + ["--lookup-as-set", "3", "--hint", ",".join(map(str, G._text(P, t["W"])))], "lookup:")
    assert spec_ == plain == t["W"]
    f = stats.split()
    assert {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}["accepted"] >= 7, stats
