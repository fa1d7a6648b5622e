"""Constrained decoding on the host (csrc/kh_fsm.h, kuiperllama_amd/constraint.py): the library's checks and walk of a
token automaton, the trie of from_choices, from_regex against Python's re.fullmatch on toy vocabularies (soundness,
completeness over every tokenisation, no empty row), one construction at a 128k vocabulary, and vocab_bytes on the
golden tokenizers.  CPU only."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

from kuiperllama_amd import _ffi, build
from kuiperllama_amd.constraint import TokenAutomaton, from_choices, from_regex


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def _check(lib, start, row_ptr, tokens, nxt, vocab, n_states=None):
    a, keep = _ffi.fsm(start, row_ptr, tokens, nxt, n_states)
    return lib.kh_fsm_check(C.byref(a), vocab)


# ---- kh_fsm_check ---------------------------------------------------------------------------------------------------
VALID = dict(start=0, row_ptr=[0, 2, 3, 4], tokens=[1, 5, 2, 9], nxt=[1, 2, 0, 2])
REFUSALS = {
    "n_states <= 0": (dict(VALID, n_states=0), -1),
    "start below 0": (dict(VALID, start=-1), -1),
    "start past the last state": (dict(VALID, start=3), -1),
    "next outside the states": (dict(VALID, nxt=[1, 3, 0, 2]), -1),
    "negative next": (dict(VALID, nxt=[1, 2, -1, 2]), -1),
    "row_ptr does not start at 0": (dict(VALID, row_ptr=[1, 2, 3, 4]), -1),
    "row_ptr decreases": (dict(VALID, row_ptr=[0, 3, 2, 4]), -1),
    "a row is not ascending": (dict(VALID, tokens=[5, 1, 2, 9]), -1),
    "a row repeats an id": (dict(VALID, tokens=[5, 5, 2, 9]), -1),
    "a row with no edge": (dict(VALID, row_ptr=[0, 2, 2, 4]), -1),
    "a token past the vocabulary": (dict(VALID, tokens=[1, 5, 2, 10]), _ffi.KH_ERR_RANGE),
    "a negative token": (dict(VALID, tokens=[-1, 5, 2, 9]), _ffi.KH_ERR_RANGE),
}


def test_check_accepts_a_valid_automaton(lib):
    assert _check(lib, vocab=10, **VALID) == 0
    TokenAutomaton(VALID["start"], VALID["row_ptr"], VALID["tokens"], VALID["nxt"]).check(10)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_check_refuses(lib, name):
    kw, code = REFUSALS[name]
    assert _check(lib, vocab=10, **kw) == code
    if "n_states" not in kw:  # the Python class states the same checks
        with pytest.raises((ValueError, IndexError)):
            TokenAutomaton(kw["start"], kw["row_ptr"], kw["tokens"], kw["nxt"]).check(10)


def test_check_refuses_null_arrays(lib):
    rp = (C.c_int64 * 2)(0, 1)
    tk = (C.c_int32 * 1)(0)
    null64, null32 = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
    assert lib.kh_fsm_check(None, 10) == -1
    assert lib.kh_fsm_check(C.byref(_ffi.Fsm(1, 0, null64, tk, tk)), 10) == -1
    assert lib.kh_fsm_check(C.byref(_ffi.Fsm(1, 0, rp, null32, tk)), 10) == -1
    assert lib.kh_fsm_check(C.byref(_ffi.Fsm(1, 0, rp, tk, null32)), 10) == -1
    assert lib.kh_fsm_check(C.byref(_ffi.Fsm(1, 0, rp, tk, tk)), 10) == 0
    # the model calls make the same checks ahead of anything else
    assert lib.kh_model_set_constraint(None, None) == -1
    assert lib.kh_model_get_constraint_state(None, None) == -1
    assert lib.kh_token_mask_f32(None, 4, None, None) == -1


# ---- kh_fsm_walk ----------------------------------------------------------------------------------------------------
def test_walk_matches_the_python_walk(lib):
    rng = np.random.default_rng(5)
    V, n = 50, 7
    row_ptr, tokens, nxt = [0], [], []
    for s in range(n):
        t = np.sort(rng.choice(V, int(rng.integers(1, 30)), replace=False))
        tokens += list(t)
        nxt += list(rng.integers(0, n, len(t)))
        row_ptr.append(len(tokens))
    A = TokenAutomaton(2, row_ptr, tokens, nxt)
    A.check(V)
    a, keep = _ffi.fsm(A.start, A.row_ptr, A.tokens, A.next)
    stopped = 0
    for trial in range(200):
        s0 = int(rng.integers(0, n))
        seq = []
        s = s0
        for _ in range(int(rng.integers(0, 12))):  # a legal path, then (half of the trials) one token off it
            row = A.allowed(s)
            t = int(rng.choice(row))
            seq.append(t)
            s = A.step(s, t)
        if trial % 2:
            seq += [int(rng.integers(0, V)) for _ in range(3)]
        arr = (C.c_int32 * max(len(seq), 1))(*seq)
        out, ok = C.c_int32(-7), C.c_int64(-7)
        assert lib.kh_fsm_walk(C.byref(a), s0, arr, len(seq), C.byref(out), C.byref(ok)) == 0
        assert (out.value, ok.value) == A.walk(seq, s0)
        stopped += ok.value < len(seq)
    assert stopped > 20
    out, ok = C.c_int32(), C.c_int64()
    assert lib.kh_fsm_walk(C.byref(a), n, None, 0, C.byref(out), C.byref(ok)) == _ffi.KH_ERR_RANGE
    assert lib.kh_fsm_walk(C.byref(a), 0, None, 0, C.byref(out), C.byref(ok)) == 0 and (out.value, ok.value) == (0, 0)
    assert A.walk([], None) == (2, 0)


# ---- from_choices ---------------------------------------------------------------------------------------------------
def _paths(A, eos, depth):
    """every token path from the start of at most `depth` tokens that ends with its first eos"""
    rows = [[(int(t), int(y)) for t, y in zip(A.allowed(s), A.next[A.row_ptr[s]:A.row_ptr[s + 1]])]
            for s in range(A.n_states)]
    out, todo = [], [((), A.start)]
    while todo:
        path, s = todo.pop()
        for t, y in rows[s]:
            if t == eos:
                out.append(path)
            elif len(path) < depth:
                todo.append((path + (t,), y))
    return out


def test_from_choices_accepts_exactly_the_given_sequences():
    eos = 99
    seqs = [(5, 6, 7), (5, 6), (5, 8), (1,), (5, 6, 7, 2, 3)]  # (5, 6) is a prefix of two others
    A = from_choices(seqs, eos)
    A.check(100)
    assert sorted(_paths(A, eos, 8)) == sorted(seqs)
    s, ok = A.walk([5, 6])
    assert ok == 2 and sorted(A.allowed(s)) == [7, eos]  # accepting mid-trie
    sink, ok = A.walk([1, eos, eos, eos])
    assert ok == 4 and list(A.allowed(sink)) == [eos] and A.step(sink, eos) == sink
    assert A.walk([5, 7])[1] == 1
    assert sorted(A.allowed(A.start)) == [1, 5]
    with pytest.raises(ValueError):
        from_choices([(1, eos, 2)], eos)
    with pytest.raises(ValueError):
        from_choices([], eos)
    E = from_choices([(), (3,)], eos)  # the empty answer
    assert sorted(_paths(E, eos, 3)) == [(), (3,)]


# ---- from_regex -----------------------------------------------------------------------------------------------------
ALPHABET = b"abcd1 "
MULTI = [b"ab", b"abc", b"cd", b"dd", b"aa", b"ba", b"bc", b"ca", b"da", b"d1", b"11", b"1 ", b" a", b"  ", b"abab",
         b"cdc", b"a1", b"bcd", b"cab", b"dab", b"cc"]
# one token that straddles two pattern elements ("cd" over the group and the literal of (ab|c)+d is among MULTI; this one
# straddles a repetition and what follows it), one empty special token, and eos
TOY = [bytes([c]) for c in ALPHABET] + MULTI + [b"bd", b"", b"</s>"]
EOS = len(TOY) - 1
PATTERNS = [
    r"(ab|c)+d",
    r"a*b",
    r"a?b+c*",
    r"[abc]{2}d",
    r"[^a]{1,3}",
    r"a.c",
    r"\d+( \d+)?",
    r"\w\s\w",
    r"(a|b|cd){2,4}",
    r"[a-b1]*d",
    r"ab|cd|",
    r"(a(b|c)){1,2}d?",
    r"a\.?b|[\d\s]+",
    r"[^\w]a|\\?d",
]
DEPTH = 6


def _tokenisations(s, vocab):
    """every way to write the bytes s as tokens of `vocab` (empty tokens never)"""
    if not s:
        return [()]
    out = []
    for i, b in enumerate(vocab):
        if b and i != EOS and s.startswith(b):
            out += [(i,) + rest for rest in _tokenisations(s[len(b):], vocab)]
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
def test_from_regex_matches_re_fullmatch(pattern):
    A = from_regex(pattern, TOY, EOS)
    A.check(len(TOY))
    rx = re.compile(pattern.encode())
    # no reachable state has an empty row (check() refuses one), and every state is reachable
    seen, todo = {A.start}, [A.start]
    while todo:
        s = todo.pop()
        for y in A.next[A.row_ptr[s]:A.row_ptr[s + 1]]:
            if int(y) not in seen:
                seen.add(int(y))
                todo.append(int(y))
    assert seen == set(range(A.n_states))
    empty = TOY.index(b"")
    assert empty not in A.tokens
    # soundness: every path of up to 6 tokens that ends in eos decodes to a full match
    paths = _paths(A, EOS, DEPTH)
    assert paths
    for p in paths:
        text = b"".join(TOY[t] for t in p)
        assert rx.fullmatch(text), (pattern, p, text)
    # completeness: every tokenisation of every matching string of up to 6 bytes is a path
    have = set(paths)
    n_match = 0
    for n in range(DEPTH + 1):
        for s in itertools.product(ALPHABET, repeat=n):
            s = bytes(s)
            if not rx.fullmatch(s):
                continue
            n_match += 1
            for tk in _tokenisations(s, TOY):
                assert tk in have, (pattern, s, tk)
                st, ok = A.walk(list(tk) + [EOS])
                assert ok == len(tk) + 1
    assert n_match > 0
    # behind eos: the sink
    sink, _ = A.walk(list(paths[0]) + [EOS])
    assert list(A.allowed(sink)) == [EOS] and A.step(sink, EOS) == sink


def test_from_regex_on_a_vocabulary_without_single_bytes():
    """Token-level pruning: byte-level states that no token reaches or leaves are dropped, so no row is empty."""
    vocab = [b"ab", b"abab", b"c", b"", b"<eos>"]
    A = from_regex(r"(ab)+c?|abx", vocab, 4)
    A.check(len(vocab))
    rx = re.compile(rb"(ab)+c?|abx")
    want = [p for n in range(1, 4) for p in itertools.product(range(3), repeat=n)
            if rx.fullmatch(b"".join(vocab[t] for t in p))]
    assert sorted(_paths(A, 4, 3)) == sorted(want) and (0, 1, 2) in want
    with pytest.raises(ValueError):
        from_regex(r"x+", vocab, 4)  # nothing this vocabulary can spell


@pytest.mark.parametrize("pattern", [r"a*?", r"a{2,}", r"(?:a)", r"(?P<n>a)", r"^a", r"a$", r"\bword", r"\1", r"a{,2}",
                                     r"(a", r"a)", r"[a", r"*a", r"\D", r"[[:alpha:]]", r"a++", r"[z-a]", r"a{3,2}"])
def test_from_regex_refuses_unsupported_syntax(pattern):
    with pytest.raises(ValueError):
        from_regex(pattern, TOY, EOS)


def test_from_regex_at_128k_tokens():
    V = 128256
    rng = np.random.default_rng(0)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789 .,{}\":-_\n", np.uint8)
    vocab = [bytes([b]) for b in range(256)]
    lens = rng.integers(1, 13, V - 256 - 2)
    flat = letters[rng.integers(0, len(letters), int(lens.sum()))].tobytes()
    at = np.concatenate([[0], np.cumsum(lens)])
    vocab += [flat[at[i]:at[i + 1]] for i in range(len(lens))] + [b"", b"<|eot|>"]
    assert len(vocab) == V
    A = from_regex(r'\{"name": "[a-z]{1,12}", "n": \d{1,3}(\.\d+)?\}', vocab, V - 1)
    A.check(V)
    assert A.n_states > 10 and A.n_edges > A.n_states
    st, ok = A.walk([ord(c) for c in '{"name": "bob", "n": 42}'] + [V - 1])
    assert ok == 25 and list(A.allowed(st)) == [V - 1]


# ---- vocab_bytes ----------------------------------------------------------------------------------------------------
TEXTS = ["Hello world, this is a test.", " leading space", "the quick  brown fox 123", "naïve café ☃", "a\tb\nc"]


@pytest.mark.parametrize("name,flavor", [("llama3_like", 0), ("qwen2_like", 1)])
@pytest.mark.parametrize("ref_spaces", [True, False])
def test_vocab_bytes_of_a_bpe_tokenizer(lib, name, flavor, ref_spaces):
    import os
    from conftest import GOLDEN
    from kuiperllama_amd.constraint import vocab_bytes
    from kuiperllama_amd.tokenizer import BpeTokenizer
    t = BpeTokenizer.from_file(os.path.join(GOLDEN, f"bpe_{name}.json"), flavor, ref_spaces)
    vb = vocab_bytes(t)
    assert len(vb) == t.vocab_size
    special = {t.bos_id, t.eos_id, *t.stop_ids}
    assert all((vb[i] == b"") == (i in special) for i in range(len(vb)))
    for s in TEXTS:
        ids = t.encode(s, bos=False)
        assert b"".join(vb[i] for i in ids) == t.decode_bytes(ids) == s.encode()
    # ... and it feeds from_regex: the tokenizer's own encoding of a matching text is a path
    A = from_regex(r"[a-z]+( [a-z]+)*\.?", vb, t.eos_id)
    ids = t.encode("the quick brown fox.", bos=False)
    assert A.walk(ids + [t.eos_id])[1] == len(ids) + 1
    assert A.walk(t.encode("the Quick", bos=False))[1] < len(t.encode("the Quick", bos=False))


@pytest.mark.parametrize("name", ["llama_like", "plain"])
def test_vocab_bytes_of_a_sentencepiece_tokenizer(lib, name):
    import os
    from conftest import GOLDEN
    from kuiperllama_amd.constraint import vocab_bytes
    from kuiperllama_amd.tokenizer import SpmTokenizer
    t = SpmTokenizer.from_file(os.path.join(GOLDEN, f"spm_{name}.model"))
    vb = vocab_bytes(t)
    assert len(vb) == t.vocab_size
    assert all(vb[i] == b"" for i in (t.bos_id, t.eos_id, t.unk_id))
    if name == "llama_like":  # byte fallback: every byte value is some token's whole byte string
        assert {bytes([b]) for b in range(256)} <= set(vb)
    n_checked = 0
    for s in TEXTS:
        ids = t.encode(s, bos=False)
        if t.unk_id in ids:  # no byte fallback in this model: the text is not representable
            assert name == "plain"
            continue
        cat = b"".join(vb[i] for i in ids)
        dec = t.decode(ids).encode()
        assert cat in (dec, b" " + dec), (s, cat, dec)  # the decoder drops the dummy prefix's space, the tokens hold it
        n_checked += 1
    assert n_checked >= 2
