"""Constrained decoding on the GPU (csrc/kh_fsm.h): the mask operator bit for bit against numpy, and the model paths
against the reference the header names - a host-driven loop of predict on a twin model WITHOUT a constraint whose logit
bias is re-set at every step to -inf on the ids outside the row of the host-walked state (tests/constraint_ref.py)."""
import re

import numpy as np
import pytest
import torch

import constraint_ref as CR
from conftest import load_golden
from kuiperllama_amd import _ffi, binfmt, ops
from kuiperllama_amd.constraint import TokenAutomaton, from_choices, from_regex

pytestmark = pytest.mark.gpu

INF = float("inf")
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)  # (the logit-proc test's)
FLAT_SPEC = binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 128, True, binfmt.FAMILY_LLAMA, False, 64,
                             binfmt.ROPE_HALF, 500000.0, 1e-5, "flat-synth")
SAMP = (0.9, 40, 0.95, 0xC0FFEE)


def _model(case, gpu, flags=0, max_seq_len=128):
    """-> (model, vocabulary, prompt of two tokens, steps)"""
    from kuiperllama_amd.model import KuiperModel
    if case == "flat-synth":
        img_d = binfmt.synth_image(FLAT_SPEC, seed=3, device=gpu)
        torch.cuda.synchronize()
        return KuiperModel.from_device_image(img_d, FLAT_SPEC, max_seq_len=max_seq_len, flags=flags), 2048, [1, 263], 64
    spec, img, toks, _ = load_golden(case)
    return (KuiperModel.from_host_image(img, spec, flags=flags), spec.vocab_size, [int(t) for t in toks[:2]],
            min(64, spec.seq_len))


def _predict_loop(m, prompt, steps, exec="fused"):
    words, fed = [], list(prompt)
    for p in range(steps):
        is_prompt = p < len(prompt) - 1
        nxt = m.predict(fed[p], p, is_prompt=is_prompt, exec=exec)
        words.append(prompt[p + 1] if is_prompt else nxt)
        if p + 1 >= len(fed):
            fed.append(words[-1])
    return words


# ---- 1. operator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [501, 2048, 128256])
def test_operator_bit_for_bit(gpu, V):
    rng = np.random.default_rng(V)
    lg = rng.normal(0.0, 3.0, V).astype(np.float32)
    kind = rng.integers(0, 8, V)
    lg[kind == 0] = 0.0
    lg[kind == 1] = -INF
    last0 = 32 * ((V - 1) // 32)
    masks = {"all ones": np.arange(V), "only bit 0": [0], "only bit V - 1": [V - 1],
             "only the last word": np.arange(last0, V), "alternating": np.arange(0, V, 2),
             "density 1/8": np.flatnonzero(rng.random(V) < 0.125)}
    buf = torch.empty(V + 1, dtype=torch.float32, device=gpu)
    for name, allowed in masks.items():
        words = CR.mask_words(allowed, V, garbage_seed=V + len(name))  # garbage above bit V of the last word
        want = CR.apply_words(lg, words)
        assert want.tobytes() == CR.mask(lg, allowed).tobytes()
        mw = torch.from_numpy(words.view(np.int32).copy()).to(gpu)
        for off in (0, 1):  # a 16-byte aligned vector, and one that is not (the scalar path)
            d = buf[off:off + V]
            d.copy_(torch.from_numpy(lg))
            ops.token_mask(d, mw)
            got = d.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (name, off)  # raw bits: the untouched entries too
        if name != "all ones":
            assert np.isneginf(want).sum() > np.isneginf(lg).sum()


# ---- 2. every picked token ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["flat-synth", "hf_llama_half", "ref_llama_int8_untied"])
def test_every_picked_token_equals_the_bias_loop(gpu, case):
    m, V, prompt, steps = _model(case, gpu)
    twin = _model(case, gpu)[0]
    # seeds at which the precondition below holds, greedy and sampled, and the runs meet rows of all six sizes
    A = CR.random_automaton(V, CR.row_sizes(V), seed={"flat-synth": 13, "hf_llama_half": 12}.get(case, 13))
    A.check(V)
    n0 = len(prompt) - 1
    for samp in (None, SAMP):
        for mm in (m, twin):
            mm.set_sampling(*samp) if samp else mm.set_sampling()
        m.set_constraint(A)
        words, _ = m.generate(prompt, steps, exec="graph")
        got_logits = m.logits()
        want, states, raws = CR.twin_loop(twin, A, prompt, steps, raw_argmax=True)
        # the precondition: at half of the sampled positions at least, the raw argmax lies outside the row - else the
        # run shows nothing
        outside = [r not in set(A.allowed(s).tolist()) for r, s in zip(raws, states)]
        print(f"{case} samp={samp is not None}: raw argmax outside the row at {sum(outside)} of {len(outside)} positions; "
              f"row sizes met {sorted({len(A.allowed(s)) for s in states})}")
        assert 2 * sum(outside) >= len(outside)
        assert words == want
        assert got_logits.tobytes() == twin.logits().tobytes()
        assert A.walk(words[n0:])[1] == steps - n0  # every word lies in the row of its state
        # the state behind a predict loop is the host walk's
        m.set_constraint(A)  # (state = start)
        loop = _predict_loop(m, prompt, 12)
        assert loop == want[:12]
        assert m.constraint_state == A.walk(loop[n0:])[0]
        m.set_constraint(None)
    m.close()
    twin.close()


# ---- 3. with everything on ------------------------------------------------------------------------------------------
def test_with_penalties_bias_sampler_and_logprobs(gpu):
    m, V, prompt, steps = _model("flat-synth", gpu)
    twin = _model("flat-synth", gpu)[0]
    A = CR.random_automaton(V, CR.row_sizes(V), seed=12)
    n0 = len(prompt) - 1
    small = set(A.allowed(0).tolist()) | set(A.allowed(1).tolist())
    banned = next(int(t) for t in A.allowed(2) if int(t) not in small)  # an ALLOWED token of the V/8 row; no row is emptied
    up = next(int(t) for t in A.allowed(3) if int(t) != banned)
    user = {banned: -INF, up: 0.75}
    for mm in (m, twin):
        mm.set_penalties(**PEN)
        mm.set_sampling(*SAMP)
        mm.set_logprobs(5)
    m.set_logit_bias(user)
    m.set_constraint(A)
    words, _ = m.generate(prompt, steps, exec="graph")
    rec = m.logprobs(n0, steps - n0)
    want, states, _ = CR.twin_loop(twin, A, prompt, steps, user_bias=user)
    assert words == want and banned not in words[n0:]
    ref = twin.logprobs(n0, steps - n0)
    for k in ("token", "logprob", "top_ids", "top_logprobs"):
        assert rec[k].tobytes() == ref[k].tobytes(), k
    assert list(rec["token"]) == words[n0:]
    # a banned id in a top list has log-prob -inf: rows of 1 and 2 ids leave at least 3 such entries among 5
    narrow = [i for i, s in enumerate(states) if len(A.allowed(s)) <= 2]
    assert narrow
    for i in narrow:
        row = set(A.allowed(states[i]).tolist()) - {banned}
        for t, lp in zip(rec["top_ids"][i], rec["top_logprobs"][i]):
            assert (int(t) in row) == bool(np.isfinite(lp)) and (np.isfinite(lp) or lp == -INF)
    m.close()
    twin.close()


# ---- 4. entry points agree ------------------------------------------------------------------------------------------
def test_entry_points_agree(gpu):
    m, V, _, _ = _model("hf_llama_half", gpu)
    twin = _model("hf_llama_half", gpu)[0]
    _, _, toks, _ = load_golden("hf_llama_half")
    prompt = [int(t) for t in toks[:3]]
    n0 = len(prompt) - 1
    A = CR.random_automaton(V, CR.row_sizes(V), seed=13)
    m.set_constraint(A)
    for samp in (None, (1.0, 0, 0.9, 77)):
        m.set_sampling(*samp) if samp else m.set_sampling()
        g, _ = m.generate(prompt, 64, exec="graph")
        assert A.walk(g[n0:])[1] == 64 - n0
        assert m.generate(prompt, 64, exec="graph")[0] == g  # the state is re-armed (and the graph warm-up undone)
        assert m.generate(prompt, 64, exec="fused")[0] == g
        assert m.generate(prompt, 13, exec="graph")[0] == g[:13]
        absent = next(t for t in range(V) if t not in g)
        assert m.generate(prompt, 64, exec="graph", stop=[absent])[0] == g
        m.set_constraint(A)
        assert _predict_loop(m, prompt, 64) == g
        assert m.constraint_state == A.walk(g[n0:])[0]
        # unfused: the reference's launch sequence with k_token_mask ahead of the processors and k_fsm_advance behind
        # the pick - against the bias loop on the twin, unfused too.  Its logits carry another summation order than the
        # fused step's, so a seeded draw may differ from g where the greedy words do not
        un, _ = m.generate(prompt, 40, exec="unfused")
        twin.set_sampling(*samp) if samp else twin.set_sampling()
        assert un == CR.twin_loop(twin, A, prompt, 40, exec="unfused")[0]
        assert m.logits().tobytes() == twin.logits().tobytes()
        if samp is None:
            assert un == g[:40]
        m.constraint_state = A.start
        assert _predict_loop(m, prompt, 40, exec="unfused") == un
    m.close()
    twin.close()


@pytest.mark.parametrize("exact", [False, True])
def test_a_prefilled_prompt_does_not_advance_the_state(gpu, exact):
    """A prompt of 20 tokens through the GEMM prefill and, with KH_FLAG_PREFILL_EXACT, through the bit-identical one."""
    flags = _ffi.KH_FLAG_PREFILL_EXACT if exact else 0
    m, V, _, _ = _model("flat-synth", gpu, flags=flags)
    prompt = [int(t) for t in np.random.default_rng(8).choice(V, 20, replace=False)]
    n0 = len(prompt) - 1
    A = CR.random_automaton(V, CR.row_sizes(V), seed=14)
    m.set_constraint(A)
    words, _ = m.generate(prompt, 48, exec="graph")
    assert m.first_sample()["prefill_mode"] == ("gemv" if exact else "gemm")
    assert words[:n0] == prompt[1:]
    assert words[n0] in A.allowed(A.start) and m.first_sample()["top1_id"] == words[n0]
    assert A.walk(words[n0:])[1] == 48 - n0
    assert m.generate(prompt, 48, exec="graph")[0] == words
    if exact:  # the rows are the token-by-token ones: the twin loop gives the same words
        twin = _model("flat-synth", gpu)[0]
        assert CR.twin_loop(twin, A, prompt, 48)[0] == words
        twin.close()
    m.close()


# ---- 5. row edges of the lookup -------------------------------------------------------------------------------------
def test_first_and_last_entry_of_a_row(gpu):
    m, V, prompt, _ = _model("flat-synth", gpu)
    rng = np.random.default_rng(15)
    wide = np.sort(rng.choice(V, 1025, replace=False)).astype(np.int32)
    nxt_wide = np.full(1025, 3, np.int32)
    nxt_wide[0], nxt_wide[-1] = 1, 2
    one = np.array([int(wide[512])], np.int32)
    rows = [(wide, nxt_wide), (one, np.array([2], np.int32)), (np.arange(V, dtype=np.int32), np.zeros(V, np.int32)),
            (np.array([3, 9], np.int32), np.array([0, 3], np.int32))]
    row_ptr = np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])])
    A = TokenAutomaton(0, row_ptr, np.concatenate([t for t, _ in rows]), np.concatenate([y for _, y in rows]))
    A.check(V)
    m.set_constraint(A)
    for exec_mode in ("fused", "unfused"):
        for tok, want in ((int(wide[0]), 1), (int(wide[-1]), 2), (int(wide[7]), 3)):
            m.constraint_state = 0
            m.set_logit_bias({tok: 1e6})
            assert m.predict(prompt[0], 0, exec=exec_mode) == tok
            assert m.constraint_state == want, (exec_mode, tok)
        m.set_logit_bias(None)
        m.constraint_state = 1  # the 1-edge row: whatever the logits say
        assert m.predict(prompt[0], 0, exec=exec_mode) == int(one[0])
        assert m.constraint_state == 2
        assert m.predict(prompt[0], 0, is_prompt=True, exec=exec_mode) == -1  # fed, not sampled: no mask, no move
        assert m.constraint_state == 2
    m.close()


# ---- 6. no recapture, no stale pointers -----------------------------------------------------------------------------
def test_new_automata_need_no_recapture_and_off_is_untouched(gpu):
    from kuiperllama_amd.model import KuiperModel
    spec, img, toks, _ = load_golden("hf_llama_half")
    V = spec.vocab_size
    prompt = [int(t) for t in toks[:2]]
    lpt = 5 * spec.n_layers + 2
    fresh = KuiperModel.from_host_image(img, spec)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        want_off, _ = fresh.generate(prompt, 32, exec="graph")
        want_logits = fresh.logits()
        log_fresh = _ffi.launch_log()
        A = CR.random_automaton(V, [3, V // 4], seed=16)
        B = CR.random_automaton(V, [1 + (7 * i) % (V // 2) for i in range(40)], seed=17)
        ref = {id(X): CR.twin_loop(fresh, X, prompt, 32)[0] for X in (A, B)}
        fresh.close()
        m = KuiperModel.from_host_image(img, spec)
        assert m.cfg.launches_per_token == lpt
        for i, X in enumerate((A, B, A)):
            m.set_constraint(X)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
            assert m.generate(prompt, 32, exec="graph")[0] == ref[id(X)]
            log_on = _ffi.launch_log()
            if i == 0:  # the step graphs are captured by the first run: what they launch
                assert "k_sample_proc_fsm" in log_on
                assert not any(k.startswith(("k_sample_screen", "k_cls_screen")) for k in log_on)
                assert "k_sample_proc" not in log_on and "k_sample_lp" not in log_on
            else:  # another automaton, of another size: the same graphs replayed - nothing is captured or launched eagerly
                assert log_on == set(), log_on
        counts = m.profile_step(1, 2)
        assert sum(v["launches_per_step"] for v in counts.values()) == lpt and m.cfg.launches_per_token == lpt
        m.set_constraint(None)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        assert m.generate(prompt, 32, exec="graph")[0] == want_off
        assert m.logits().tobytes() == want_logits.tobytes()
        log_off = _ffi.launch_log()
        assert log_off <= log_fresh, log_off - log_fresh  # off launches no kernel that a fresh model does not launch
        counts = m.profile_step(1, 2)
        assert sum(v["launches_per_step"] for v in counts.values()) == lpt and m.cfg.launches_per_token == lpt
        with pytest.raises(_ffi.KhError) as ei:
            m.constraint_state
        assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(gpu):
    m, V, prompt, _ = _model("flat-synth", gpu)
    A = CR.random_automaton(V, CR.row_sizes(V), seed=18)
    two = [int(t) for t in A.allowed(1)]
    empties = {t: -INF for t in two}  # every token of the 2-edge row
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        # a row emptied by a -inf bias, in both setting orders
        m.set_logit_bias(empties)
        with pytest.raises(_ffi.KhError) as ei:
            m.set_constraint(A)
        assert ei.value.code == _ffi.KH_ERR_INVALID_ARG
        m.set_logit_bias(None)
        m.set_constraint(A)
        with pytest.raises(_ffi.KhError) as ei:
            m.set_logit_bias(empties)
        assert ei.value.code == _ffi.KH_ERR_INVALID_ARG
        m.set_logit_bias({two[0]: -INF, two[1]: -1.0})  # one token of the row left: fine
        m.set_logit_bias(None)
        # an invalid automaton leaves the one in force
        with pytest.raises(_ffi.KhError) as ei:
            m.set_constraint(TokenAutomaton(0, [0, 1], [V], [0]))
        assert ei.value.code == _ffi.KH_ERR_RANGE
        with pytest.raises(_ffi.KhError) as ei:
            m.set_constraint(TokenAutomaton(0, [0, 0, 1], [1], [0]))
        assert ei.value.code == _ffi.KH_ERR_INVALID_ARG
        # ... and so does one whose mask table (a row of V / 32 words per state) would pass KH_FSM_MAX_MASK_BYTES
        n_big = (256 << 20) // (4 * ((V + 31) // 32)) + 1
        big = TokenAutomaton(0, np.arange(n_big + 1), np.zeros(n_big, np.int32), np.zeros(n_big, np.int32))
        with pytest.raises(_ffi.KhError) as ei:
            m.set_constraint(big)
        assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
        assert m.constraint_state == A.start
        for bad in (-1, A.n_states):
            with pytest.raises(_ffi.KhError) as ei:
                m.constraint_state = bad
            assert ei.value.code == _ffi.KH_ERR_RANGE
        # what runs B-token passes refuses while a constraint is set
        calls = {"verify": lambda: m.verify(prompt, 0),
                 "verify_as_set": lambda: m.verify(prompt, 0, as_set=True),
                 "generate_lookup": lambda: m.generate_lookup(prompt, 16),
                 "seq_step": lambda: m.seq_step([0], [prompt[0]], [0]),
                 "seq_prefill": lambda: m.seq_prefill(0, prompt),
                 "generate_batch": lambda: m.generate_batch([prompt], 8)}
        for name, call in calls.items():
            with pytest.raises(_ffi.KhError) as ei:
                call()
            assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED, name
        assert _ffi.launch_log() == set()  # nothing was launched by any of this
        m.set_constraint(None)
        assert len(m.verify(prompt, 0)[0]) == len(prompt)  # ... and runs again without one
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


# ---- 8. end to end with the helpers ---------------------------------------------------------------------------------
def test_choices_and_regex_end_to_end(gpu):
    m, V, prompt, _ = _model("flat-synth", gpu)
    eos = 2
    choices = [(700, 701, 702), (700, 701), (15, 1999, 3, 3, 8)]
    m.set_constraint(from_choices(choices, eos))
    for samp in (None, (1.0, 0, 1.0, 5), (1.0, 0, 1.0, 6)):
        m.set_sampling(*samp) if samp else m.set_sampling()
        words, _ = m.generate(prompt, 32, exec="graph", stop=[eos])
        assert tuple(words[len(prompt) - 1:]) in choices, words
    # a toy vocabulary mapped onto ids of the model: id 100 + i spells TOY[i], every other id spells nothing
    toy = [b"a", b"b", b"c", b"d", b"ab", b"cd", b"abc", b"bd", b"cc", b"dd"]
    vocab = [b""] * V
    for i, b in enumerate(toy):
        vocab[100 + i] = b
    A = from_regex(r"(ab|c)+d", vocab, eos)
    A.check(V)
    m.set_constraint(A)
    done = 0
    for seed in range(6):
        m.set_sampling(3.0, 0, 1.0, seed)  # a flat distribution: some run ends well inside 48 steps
        words, _ = m.generate(prompt, 48, exec="graph", stop=[eos])
        out = words[len(prompt) - 1:]
        assert all(100 <= t < 100 + len(toy) for t in out)
        text = b"".join(vocab[t] for t in out)
        if len(words) < 48:  # the run reached eos: the text is a full match
            assert re.fullmatch(rb"(ab|c)+d", text), text
            done += 1
        else:  # cut by the step limit: still a prefix the pattern can complete
            assert A.walk(out)[1] == len(out)
    assert done > 0
    m.close()
