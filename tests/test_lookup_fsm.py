"""The drafter of constrained lookup decode, CPU side (kh_lookup_draft_fsm, csrc/kh_lookup.h) against a plain-Python
statement of its two rules, written here from TokenAutomaton.allowed / step, TokenAutomaton.forced_run (rule (a) in
numpy) and model.lookup_draft (the n-gram drafter, which tests/test_lookup.py holds to its own reference):

  from `state`, until cap tokens are out or neither rule adds one
    (a) while the row of the current state has exactly ONE edge: that token, and on along the edge (n_forced counts);
    (b) otherwise lookup_draft(seq + out so far, same hint and bounds, the remaining room), of which the longest prefix
        the automaton can follow from the current state is kept and followed; nothing kept: stop.

All at V = 2048.  Every test needs the new symbols: none passes without the feature."""
import ctypes as C

import numpy as np
import pytest

import constraint_ref as CR
from kuiperllama_amd import _ffi, build
from kuiperllama_amd.constraint import TokenAutomaton, from_choices
from kuiperllama_amd.model import lookup_draft, lookup_draft_fsm

V = 2048
EOS = 2


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def ref(A, state, seq, hint=None, hi=4, lo=1, cap=7):
    """-> (tokens, n_forced, n-gram proposals that were cut: [(proposed, kept)])"""
    out, forced, s, cuts = [], 0, int(state), []
    while len(out) < cap:
        before = len(out)
        run = A.forced_run(s, cap - len(out))  # (a)
        out += run
        forced += len(run)
        s = A.walk(run, s)[0]
        if len(out) < cap:  # (b)
            assert len(A.allowed(s)) != 1
            d = lookup_draft(list(seq) + out, hint, hi, lo, cap - len(out))
            kept = 0
            for t in d:
                nx = A.step(s, t)
                if nx < 0:
                    break
                s = nx
                out.append(t)
                kept += 1
            if d:
                cuts.append((len(d), kept))
        if len(out) == before:
            break
    return out, forced, cuts


def check(A, state, seq, hint=None, hi=4, lo=1, cap=7):
    want, forced, cuts = ref(A, state, seq, hint, hi, lo, cap)
    got = lookup_draft_fsm(A, state, seq, hint, hi, lo, cap)
    assert got == (want, forced), (state, seq, hint, hi, lo, cap, got, want, forced)
    assert len(want) <= cap and A.walk(want, state)[1] == len(want)  # every drafted token is followable
    return want, forced, cuts


def test_symbols_are_exported(lib):
    for name in ("kh_lookup_draft_fsm", "kh_model_verify_fsm", "kh_model_generate_lookup_fsm"):
        assert name in _ffi.EXPORTS and hasattr(lib, name), name


def test_forced_run_is_rule_a():
    A = from_choices([(10, 11, 20), (10, 11, 30, 31)], EOS)
    assert A.forced_run(0, 7) == [10, 11] and A.forced_run(0, 1) == [10] and A.forced_run(0, 0) == []
    s = A.walk([10, 11])[0]
    assert len(A.allowed(s)) == 2 and A.forced_run(s, 7) == []
    assert A.forced_run(A.walk([10, 11, 30])[0], 7) == [31] + [EOS] * 6  # into the sink, whose self-edge goes on


def test_choices_forced_runs_end_at_before_and_past_cap(lib):
    tails = {n: tuple(100 * n + i for i in range(n)) for n in (1, 6, 7, 8)}
    A = from_choices([(10, 11) + t for t in tails.values()], EOS)
    A.check(V)
    # from the start: the shared prefix is forced, the branching row ends the run BEFORE cap (nothing to look up)
    for cap in (2, 3, 7):
        assert check(A, 0, [5], cap=cap)[:2] == ([10, 11], 2)
    assert check(A, 0, [5], cap=1)[:2] == ([10], 1)
    branch = A.walk([10, 11])[0]
    assert len(A.allowed(branch)) == 4 and check(A, branch, [5, 10, 11])[:2] == ([], 0)
    # behind the first token of a tail: the rest of the tail, eos, and the sink's self-edge up to cap
    for n, t in tails.items():
        s = A.walk([10, 11, t[0]])[0]
        seq = [5, 10, 11, t[0]]
        for cap in (0, 1, 6, 7, 8):
            want = (list(t[1:]) + [EOS] * 9)[:cap]
            assert check(A, s, seq, cap=cap)[:2] == (want, cap), (n, cap)
    # cap 7: the 8-token tail's own run ends exactly AT cap, the 7-token tail's one short of it, the 6-token tail's two
    assert check(A, A.walk([10, 11, 800])[0], [800])[0] == [801, 802, 803, 804, 805, 806, 807]
    assert check(A, A.walk([10, 11, 700])[0], [700])[0] == [701, 702, 703, 704, 705, 706, EOS]
    assert check(A, A.walk([10, 11, 600])[0], [600])[0] == [601, 602, 603, 604, 605, EOS, EOS]
    # a hint that names a choice: the branching row follows it (rule (b) runs to its proposal's end, through rows that
    # rule (a) would have forced), and one that names no choice is cut at the branch
    hint = [10, 11] + list(tails[6])
    out, forced, cuts = check(A, 0, [5], hint=hint, cap=7)
    assert out == [10, 11] + list(tails[6])[:5] and forced == 2 and cuts == [(5, 5)]
    out, forced, cuts = check(A, 0, [5], hint=[10, 11, 600, 77, 602], cap=7)
    assert out == [10, 11, 600, 601, 602, 603, 604] and forced == 6 and cuts == [(3, 1)]


def test_single_choice_is_forced_into_the_sink(lib):
    A = from_choices([(4, 5, 6)], EOS)
    for cap in (0, 1, 3, 4, 7):
        assert check(A, 0, [9], cap=cap)[:2] == (([4, 5, 6] + [EOS] * 4)[:cap], cap)
    sink = A.n_states - 1
    assert check(A, sink, [9], cap=7)[:2] == ([EOS] * 7, 7)


def test_rows_without_a_forced_token_keep_what_the_automaton_follows(lib):
    A = CR.random_automaton(V, [2, V // 8, 1024, 1025, V], seed=31)
    A.check(V)
    rng = np.random.default_rng(32)
    zero = partial = full = 0
    for trial in range(400):
        s = int(rng.integers(0, A.n_states))
        row = A.allowed(s)
        inside = [int(t) for t in rng.choice(row, min(3, len(row)), replace=False)]
        alphabet = inside + [int(t) for t in rng.integers(0, V, 2)]
        seq = [alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(2, 24)))]
        hint = [alphabet[int(i)] for i in rng.integers(0, len(alphabet), 12)] if trial % 3 == 0 else None
        lo = int(rng.integers(1, 3))
        out, forced, cuts = check(A, s, seq, hint, lo + int(rng.integers(0, 4)), lo, int(rng.integers(0, 9)))
        assert forced == 0
        if cuts:  # the output starts with the first proposal, cut at its first token outside the row
            zero += cuts[0][1] == 0
            partial += 0 < cuts[0][1] < cuts[0][0]
            full += cuts[0][1] == cuts[0][0]
            if cuts[0][1] == 0:
                assert out == []
    assert zero > 10 and partial > 10 and full > 10, (zero, partial, full)  # the cases bite
    # by hand: the proposal's first token lies outside the row - cut at token 0
    s = 0
    a, b = int(A.allowed(s)[0]), next(t for t in range(V) if t not in set(A.allowed(s).tolist()))
    assert lookup_draft([a, b, a], None, 4, 1, 7) == [b, a]
    assert check(A, s, [a, b, a])[:2] == ([], 0)
    # ... and inside it: kept up to the first token its state's row does not hold
    b2 = int(A.allowed(s)[1])
    out, forced, cuts = check(A, s, [a, b2, a])
    assert out[:1] == [b2] and forced == 0 and cuts[0][0] == 2


def test_forced_then_ngram_then_forced_in_one_call(lib):
    every = np.arange(V, dtype=np.int32)
    to2 = np.full(V, 2, np.int32)
    to2[9] = 3  # token 9 leaves the free state
    rows = [(np.array([5], np.int32), np.array([1], np.int32)), (np.array([6], np.int32), np.array([2], np.int32)),
            (every, to2), (np.array([12], np.int32), np.array([4], np.int32)),
            (np.array([13], np.int32), np.array([5], np.int32)), (every, np.full(V, 5, np.int32))]
    row_ptr = np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])])
    A = TokenAutomaton(0, row_ptr, np.concatenate([t for t, _ in rows]), np.concatenate([y for _, y in rows]))
    A.check(V)
    seq = [3, 1, 5, 6, 7, 8, 9, 40, 3, 1]
    # 5 6 forced; [3 1 5 6] is found at the front and proposes 7 8 9 40 3, of which 40 has no edge behind 9; 12 13 forced
    out, forced, cuts = check(A, 0, seq, cap=7)
    assert out == [5, 6, 7, 8, 9, 12, 13] and forced == 4 and cuts == [(5, 3)]
    assert check(A, 0, seq, cap=6)[:2] == ([5, 6, 7, 8, 9, 12], 3)
    assert check(A, 0, seq, cap=8)[:2] == ([5, 6, 7, 8, 9, 12, 13], 4)  # the last state is free and nothing matches
    for cap in (0, 1, 2, 3, 5):
        check(A, 0, seq, cap=cap)
    assert check(A, 0, seq, cap=0)[:2] == ([], 0) and check(A, 0, seq, cap=1)[:2] == ([5], 1)


def test_error_codes_before_anything_is_touched(lib):
    A = from_choices([(4, 5, 6)], EOS)
    f = lib.kh_lookup_draft_fsm
    a, keep = _ffi.fsm(A.start, A.row_ptr, A.tokens, A.next)
    seq = (C.c_int32 * 3)(1, 2, 1)
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    nf = C.c_int32(-7)
    none = C.POINTER(C.c_int32)()

    def call(fsm, state, hi=4, lo=1, n_seq=3, cap=4, o=out):
        return f(C.byref(fsm) if fsm is not None else None, state, seq, n_seq, none, 0, hi, lo, o, cap, C.byref(nf))
    assert call(a, 0) == 4 and list(out) == [4, 5, 6, EOS] and nf.value == 4
    out[:] = [-7] * 4
    nf.value = -7
    # a malformed automaton: kh_fsm_check's codes
    assert call(None, 0) == _ffi.KH_ERR_INVALID_ARG
    empty_row, k1 = _ffi.fsm(0, [0, 0, 1], [1], [0])
    assert call(empty_row, 0) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_fsm_check(C.byref(empty_row), V) == _ffi.KH_ERR_INVALID_ARG
    bad_next, k2 = _ffi.fsm(0, [0, 1], [1], [3])
    assert call(bad_next, 0) == _ffi.KH_ERR_INVALID_ARG
    descending, k3 = _ffi.fsm(0, [0, 2], [5, 4], [0, 0])
    assert call(descending, 0) == _ffi.KH_ERR_INVALID_ARG
    bad_start, k4 = _ffi.fsm(2, [0, 1], [1], [0])
    assert call(bad_start, 0) == _ffi.KH_ERR_INVALID_ARG
    # a state out of range
    for s in (-1, A.n_states):
        assert call(a, s) == _ffi.KH_ERR_RANGE
    # the n-gram bounds and sizes: kh_lookup_draft's
    assert call(a, 0, hi=2, lo=3) == _ffi.KH_ERR_INVALID_ARG
    assert call(a, 0, hi=0, lo=5) == _ffi.KH_ERR_INVALID_ARG
    assert call(a, 0, hi=-1) == _ffi.KH_ERR_INVALID_ARG
    assert call(a, 0, n_seq=-1) == _ffi.KH_ERR_INVALID_ARG
    assert call(a, 0, cap=-1) == _ffi.KH_ERR_INVALID_ARG
    assert call(a, 0, o=none) == _ffi.KH_ERR_INVALID_ARG
    assert list(out) == [-7] * 4 and nf.value == -7  # nothing was written by any of them
    assert call(a, 0, cap=0, o=none) == 0 and nf.value == 0
    with pytest.raises(_ffi.KhError) as ei:
        lookup_draft_fsm(A, A.n_states, [1])
    assert ei.value.code == _ffi.KH_ERR_RANGE
    del keep, k1, k2, k3, k4
