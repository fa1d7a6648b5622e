"""Numpy statement of constrained decoding (include/kuiper_hip.h, "Constrained decoding"; csrc/kh_fsm.h): at a sampled
position the logits outside the row of the automaton state become -inf, then logit_proc_ref.process, then the pick, then
the transition.  Also what the constraint tests share: random automata, the bit table of a row, the bias list that bans
what a row does not hold, and the host-driven twin loop that is the reference of the model tests."""
import numpy as np

import logit_proc_ref as R
from kuiperllama_amd.constraint import TokenAutomaton

INF = float("inf")


def mask(logits, allowed):
    """float32 logits with -inf wherever the id is not in `allowed`; the other entries keep their bits."""
    out = np.array(logits, dtype=np.float32, copy=True)
    ban = np.ones(out.shape[0], bool)
    ban[np.asarray(allowed, dtype=np.int64)] = False
    out[ban] = -INF
    return out


def mask_words(allowed, V, garbage_seed=None):
    """The operator's bit table of a row: ceil(V / 32) uint32 words, bit v & 31 of word v >> 5 set = v allowed.  With a
    seed the bits above V in the last word are random (the operator must ignore them)."""
    words = np.zeros((V + 31) // 32, np.uint32)
    a = np.asarray(allowed, dtype=np.int64)
    np.bitwise_or.at(words, a >> 5, (np.uint32(1) << (a & 31).astype(np.uint32)))
    if garbage_seed is not None and V % 32:
        g = np.random.default_rng(garbage_seed).integers(0, 1 << 32, dtype=np.uint64)
        words[-1] |= np.uint32(g & 0xFFFFFFFF) & ~np.uint32((1 << (V % 32)) - 1)
    return words


def apply_words(logits, words):
    """The operator in numpy: bit clear -> -inf."""
    V = logits.shape[0]
    v = np.arange(V)
    bit = (words[v >> 5] >> (v & 31).astype(np.uint32)) & np.uint32(1)
    out = logits.copy()
    out[bit == 0] = -INF
    return out


def step(logits, automaton, state, fed, pos, pick, penalties=None, bias=None):
    """One sampled position: (processed logits, token, state behind it).  pick: processed logits -> token id."""
    proc = R.process(mask(logits, automaton.allowed(state)), fed, pos, bias=bias, **(penalties or {}))
    t = int(pick(proc))
    return proc, t, automaton.step(state, t)


def random_automaton(V, sizes, seed):
    """One state per entry of `sizes`, whose row holds that many random ids with random targets; every state is reachable
    from state 0 (state i's first edge leads to state i + 1, the last state's to 0)."""
    rng = np.random.default_rng(seed)
    n = len(sizes)
    row_ptr, tokens, nxt = [0], [], []
    for s, k in enumerate(sizes):
        t = np.sort(rng.choice(V, int(k), replace=False)).astype(np.int32)
        y = rng.integers(0, n, int(k)).astype(np.int32)
        y[0] = (s + 1) % n
        if k > 1:
            y[-1] = (s + 2) % n
        tokens.append(t)
        nxt.append(y)
        row_ptr.append(row_ptr[-1] + int(k))
    return TokenAutomaton(0, row_ptr, np.concatenate(tokens), np.concatenate(nxt))


def row_sizes(V):
    """1, 2, V/8, 1024, 1025 and V edges (the middle pair around half the vocabulary where it is smaller than 2048)"""
    return [1, 2, V // 8, min(1024, V // 2), min(1025, V // 2 + 1), V]


def ban_bias(automaton, state, V, user=None):
    """The logit bias that equals the mask of `state` - -inf on every id outside the row, nothing for a row of V ids -
    in union with a user's list (a banned id stays banned)."""
    row = automaton.allowed(state)
    out = dict(user or {})
    if len(row) < V:
        ban = np.ones(V, bool)
        ban[row] = False
        out.update({int(v): -INF for v in np.flatnonzero(ban)})
    return out


def twin_loop(twin, automaton, prompt, steps, user_bias=None, exec="fused", raw_argmax=False, fed_prefix=0):
    """The reference: a host-driven loop of predict on a model WITHOUT a constraint whose logit bias is re-set at every
    sampled step to the mask of the state, the state walked on the host.  Positions below fed_prefix are taken from the
    cache as an earlier call left it.  -> (words, states ahead of every sampled position, raw argmax of every sampled
    position or None)."""
    V = twin.cfg.vocab_size
    s = automaton.start
    words, states, raws = [], [], []
    fed = [int(t) for t in prompt]
    for p in range(steps):
        is_prompt = p < len(prompt) - 1
        if is_prompt:
            if p >= fed_prefix:
                twin.predict(fed[p], p, is_prompt=True, exec=exec)
            words.append(fed[p + 1])
            continue
        if raw_argmax:  # the raw logits of the position: the same step with no bias at all
            twin.set_logit_bias(None)
            twin.predict(fed[p], p, exec=exec)
            raws.append(int(np.argmax(twin.logits())))
        twin.set_logit_bias(ban_bias(automaton, s, V, user_bias))
        states.append(s)
        t = twin.predict(fed[p], p, exec=exec)
        words.append(t)
        fed.append(t)
        s = automaton.step(s, t)
        assert s >= 0, (p, t)
    return words, states, (raws if raw_argmax else None)
