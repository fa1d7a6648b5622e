"""Per-sequence constrained decoding, the host side (no GPU): constraint.union, the component labels and the
emptied-row rule of kh_model_seq_set_constraint (csrc/kh_fsm.h: KhFsmReach, through the stateless entry points
kh_fsm_components / kh_fsm_bias_empties) against their numpy statement, and the ctypes signatures of the new calls."""
import ctypes as C

import numpy as np
import pytest

import constraint_ref as CR
from kuiperllama_amd import _ffi
from kuiperllama_amd.constraint import TokenAutomaton, from_choices, union

INF = float("inf")
V = 2051
BIAS_MAX = 64  # KH_SEQ_BIAS_MAX


@pytest.fixture(scope="module")
def lib():
    return _ffi.lib()


def _fsm(a):
    return _ffi.fsm(a.start, a.row_ptr, a.tokens, a.next)


def _automata():
    return [CR.random_automaton(V, CR.row_sizes(V), seed=31), from_choices([(5, 6, 7), (5, 9)], eos=2),
            CR.random_automaton(V, [3, 1, 70, V], seed=32)]


# ---- constraint.union ------------------------------------------------------------------------------------------------
def test_union_passes_the_check_and_walks_as_its_parts(lib):
    parts = _automata()
    given = [parts[0], None, parts[1], parts[2], None]
    U, starts = union(given)
    U.check(V)
    f, keep = _fsm(U)
    assert lib.kh_fsm_check(C.byref(f), V) == 0
    assert U.n_states == sum(a.n_states for a in parts) and U.n_edges == sum(a.n_edges for a in parts)
    assert [s < 0 for s in starts] == [a is None for a in given]
    rng = np.random.default_rng(33)
    base = 0
    for a, st in zip(given, starts):
        if a is None:
            continue
        assert st == base + a.start
        for trial in range(40):
            # a string that follows the automaton for a while and then (usually) leaves it
            s, text = a.start, []
            for _ in range(int(rng.integers(0, 12))):
                row = a.allowed(s)
                t = int(row[rng.integers(len(row))])
                text.append(t)
                s = a.step(s, t)
            text += [int(t) for t in rng.integers(0, V, int(rng.integers(0, 3)))]
            end_a, n_a = a.walk(text)
            end_u, n_u = U.walk(text, state=st)
            assert (end_u, n_u) == (base + end_a, n_a), (trial, text)
            out, n_ok = C.c_int32(-7), C.c_int64(-7)
            arr = (C.c_int32 * max(len(text), 1))(*text)
            assert lib.kh_fsm_walk(C.byref(f), st, arr, len(text), C.byref(out), C.byref(n_ok)) == 0
            assert (out.value, n_ok.value) == (end_u, n_u)
        base += a.n_states
    del keep


def test_union_of_one_automaton_is_that_automaton_and_none_entries():
    a = _automata()[0]
    U, starts = union([a])
    assert starts == [a.start] and U.start == a.start
    for k in ("row_ptr", "tokens", "next"):
        assert getattr(U, k).dtype == getattr(a, k).dtype and getattr(U, k).tobytes() == getattr(a, k).tobytes()
    U, starts = union([None, a, None])
    assert starts == [-1, a.start, -1] and U.tokens.tobytes() == a.tokens.tobytes()
    # one object given n times (n samples under one constraint) is laid down once
    U, starts = union([a, a, None, a])
    assert starts == [a.start, a.start, -1, a.start] and U.n_states == a.n_states
    # ... two equal automata that are different objects are not merged
    b = TokenAutomaton(a.start, a.row_ptr, a.tokens, a.next)
    U, starts = union([a, b])
    assert starts == [a.start, a.n_states + a.start] and U.n_states == 2 * a.n_states
    with pytest.raises(ValueError):
        union([None, None])
    with pytest.raises(ValueError):
        union([])


# ---- component labels and the emptied-row rule -------------------------------------------------------------------------
def _labels_numpy(a):
    """label[s] = the smallest state of the weakly connected component of s: min-label propagation to a fixed point"""
    src = np.repeat(np.arange(a.n_states), np.diff(a.row_ptr))
    dst = a.next.astype(np.int64)
    lab = np.arange(a.n_states)
    while True:
        new = lab.copy()
        np.minimum.at(new, src, lab[dst])
        np.minimum.at(new, dst, lab[src])
        if (new == lab).all():
            return lab
        lab = new


def _empties_numpy(a, lab, state, bias):
    """does the list's -inf part hold every token of a row of at most BIAS_MAX edges in the component of `state`?"""
    if state < 0:
        return False
    banned = {t for t, v in bias.items() if v == -INF}
    return any(lab[s] == lab[state] and len(a.allowed(s)) <= BIAS_MAX and set(a.allowed(s).tolist()) <= banned
               for s in range(a.n_states))


def _lib_labels(lib, a):
    f, keep = _fsm(a)
    out = (C.c_int32 * a.n_states)()
    assert lib.kh_fsm_components(C.byref(f), out) == 0
    return np.array(out[:], np.int64)


def _lib_empties(lib, a, state, bias):
    f, keep = _fsm(a)
    ids = (C.c_int32 * max(len(bias), 1))(*bias.keys())
    val = (C.c_float * max(len(bias), 1))(*bias.values())
    out = C.c_int32(-7)
    rc = lib.kh_fsm_bias_empties(C.byref(f), state, ids, val, len(bias), C.byref(out))
    return rc, out.value


def test_component_labels_against_numpy(lib):
    parts = _automata()
    U, starts = union(parts)
    lab = _lib_labels(lib, U)
    assert (lab == _labels_numpy(U)).all()
    # the parts are connected (random_automaton chains its states, a trie hangs on its root): one label each, the
    # part's first state
    base = 0
    for a in parts:
        assert (lab[base:base + a.n_states] == base).all()
        base += a.n_states
    # several components inside one automaton, labels in both directions of an edge, a self-loop
    # 0 -> 2, 1 -> 1, 2 -> 2, 3 -> 1, 4 -> 0: components {0, 2, 4}, {1, 3}
    a = TokenAutomaton(0, [0, 1, 2, 3, 4, 5], [7, 7, 7, 7, 7], [2, 1, 2, 1, 0])
    want = np.array([0, 1, 0, 1, 0])
    assert (_labels_numpy(a) == want).all() and (_lib_labels(lib, a) == want).all()
    rng = np.random.default_rng(34)
    for trial in range(30):  # sparse random graphs: many components
        n = int(rng.integers(1, 40))
        a = TokenAutomaton(0, np.arange(n + 1), rng.integers(0, V, n), rng.integers(0, n, n))
        assert (_lib_labels(lib, a) == _labels_numpy(a)).all(), trial


def test_emptied_row_rule_against_numpy(lib):
    parts = _automata()  # rows of 1, 2 (part 0), the trie's rows (part 1), 3, 1, 70 (part 2): only rows <= 64 count
    U, starts = union(parts)
    lab = _labels_numpy(U)
    two = [int(t) for t in parts[0].allowed(1)]
    seventy = [int(t) for t in parts[2].allowed(2)]
    cases = [({t: -INF for t in two}, "the 2-edge row of part 0"),
             ({two[0]: -INF, two[1]: -1e9}, "one of its tokens left"),
             ({two[0]: -INF}, "half of it"),
             ({t: -INF for t in two + [1, 3, 4]}, "a superset of it"),
             ({t: -INF for t in seventy[:BIAS_MAX]}, "64 of a row of 70"),
             ({int(parts[2].allowed(1)[0]): -INF}, "the 1-edge row of part 2"),
             ({2: -INF}, "the sink of the trie"),
             ({5: -INF}, "the root of the trie"),
             ({}, "nothing")]
    hits = 0
    for bias, what in cases:
        for st in [-1] + starts + [starts[0] + 3, starts[2] + 1]:
            rc, got = _lib_empties(lib, U, st, bias)
            want = _empties_numpy(U, lab, st, bias)
            assert rc == 0 and got == int(want), (what, st)
            hits += want
    assert hits >= 6  # the list is not all "no"
    # the same list empties a row of ITS component only
    bias = {t: -INF for t in two}
    assert _lib_empties(lib, U, starts[0], bias) == (0, 1)
    assert _lib_empties(lib, U, starts[1], bias) == (0, 0) and _lib_empties(lib, U, starts[2], bias) == (0, 0)
    # refusals
    assert _lib_empties(lib, U, U.n_states, bias)[0] == _ffi.KH_ERR_RANGE
    assert _lib_empties(lib, U, -2, bias)[0] == _ffi.KH_ERR_RANGE
    assert _lib_empties(lib, U, 0, {t: -INF for t in range(BIAS_MAX + 1)})[0] == _ffi.KH_ERR_RANGE
    bad = TokenAutomaton(0, [0, 0, 1], [1], [0])  # a row without an edge
    assert _lib_empties(lib, bad, 0, bias)[0] == _ffi.KH_ERR_INVALID_ARG
    f, keep = _fsm(bad)
    assert lib.kh_fsm_components(C.byref(f), (C.c_int32 * 2)()) == _ffi.KH_ERR_INVALID_ARG


# ---- the entry points ------------------------------------------------------------------------------------------------
def test_new_entry_points_resolve_and_refuse_null(lib):
    sig = {"kh_model_seq_set_constraint": 2, "kh_model_seq_set_constraint_state": 3,
           "kh_model_seq_get_constraint_state": 3, "kh_fsm_components": 2, "kh_fsm_bias_empties": 6}
    for name, n in sig.items():
        assert name in _ffi.EXPORTS
        assert len(getattr(lib, name).argtypes) == n, name
    # no model: refused before anything is touched
    assert lib.kh_model_seq_set_constraint(None, None) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_model_seq_set_constraint_state(None, 0, 0) == _ffi.KH_ERR_INVALID_ARG
    assert lib.kh_model_seq_get_constraint_state(None, 0, None) == _ffi.KH_ERR_INVALID_ARG
