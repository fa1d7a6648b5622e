"""The drafter of speculative greedy decode, CPU side (kh_lookup_draft, csrc/kh_lookup.h) against the Python statement
of its three rules (tests/lookup_ref.py), and the argument checks of the new entry points that come before any device
call.  Small alphabets make matches and ambiguous matches the common case.  Every test needs the new symbols: none
passes without the feature."""
import ctypes as C

import numpy as np
import pytest

import lookup_ref as R
from kuiperllama_amd import _ffi, build
from kuiperllama_amd.model import lookup_draft


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def test_symbols_are_exported(lib):
    for name in ("kh_lookup_draft", "kh_model_verify_width", "kh_model_verify", "kh_model_generate_lookup",
                 "kh_argmax_rows_f32"):
        assert name in _ffi.EXPORTS and hasattr(lib, name), name


def _cases():
    rng = np.random.default_rng(20)
    out = []
    for i in range(400):
        k = int(rng.integers(3, 6))  # alphabet of 3 .. 5 symbols
        seq = [int(t) for t in rng.integers(0, k, int(rng.integers(1, 40)))]
        hint = [int(t) for t in rng.integers(0, k, int(rng.integers(1, 30)))] if i % 2 else None
        lo = int(rng.integers(1, 4))
        hi = lo + int(rng.integers(0, 5))  # sometimes longer than the sequence
        out.append((seq, hint, hi, lo, int(rng.integers(0, 9))))
    return out


def test_random_sequences_follow_the_three_rules(lib):
    hits = ambiguous = from_hint = 0
    for seq, hint, hi, lo, cap in _cases():
        want = R.draft(seq, hint, hi, lo, cap)
        assert lookup_draft(seq, hint, hi, lo, cap) == want, (seq, hint, hi, lo, cap)
        hits += bool(want)
        from_hint += bool(want) and hint is not None and R.draft(seq, None, hi, lo, cap) != want
        g = min(lo, len(seq))
        ambiguous += sum(seq[j:j + g] == seq[len(seq) - g:] for j in range(len(seq) - g)) > 1
    assert hits > 200 and ambiguous > 100 and from_hint > 20, (hits, ambiguous, from_hint)  # the cases bite


def test_named_cases(lib):
    d = lookup_draft
    # g larger than the sequence: the search starts at the sequence's own length
    assert d([7, 8], [1, 7, 8, 9, 4], ngram_max=6) == [9, 4]
    assert d([7], None, ngram_max=6) == []            # no earlier occurrence of a one-token sequence
    assert d([7, 7], None, ngram_max=6) == [7]        # ... of its last token there is
    assert d([3, 4, 5], None, ngram_max=4, ngram_min=4) == []  # ngram_min above the sequence's length
    # cap 0
    assert d([1, 2, 1, 2], [1, 2, 3], cap=0) == []
    # a match whose only follower would be past the end: hint ends with the key; the sequence's only match is its suffix
    assert d([1, 2], [0, 1, 2], ngram_min=2) == []
    assert d([0, 1, 2], None, ngram_min=2) == []
    assert d([1, 2], [0, 1, 2], ngram_min=1) == []    # 2 occurs in the hint only at its end, in the sequence only last
    # hint priority: the hint wins at the same g even where the sequence matches too
    assert d([1, 2, 5, 1, 2], [9, 1, 2, 6]) == [6]
    # ... but a LONGER match in the sequence beats a shorter one in the hint: the first g that matches wins
    assert d([4, 1, 2, 5, 4, 1, 2], [9, 1, 2, 6], ngram_max=3) == [5, 4, 1, 2]
    # earliest in the hint
    assert d([1, 2], [1, 2, 3, 1, 2, 4]) == [3, 1, 2, 4]
    # most recent in the sequence
    assert d([1, 2, 3, 1, 2, 4, 1, 2], None) == [4, 1, 2]
    # the draft is cut to cap, and ends where the source ends
    assert d([1, 2], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10], cap=7) == [3, 4, 5, 6, 7, 8, 9]
    assert d([1, 2], [1, 2, 3], cap=7) == [3]


def test_defaults_and_argument_checks(lib):
    seq, hint = [1, 2, 3, 4, 9, 1, 2, 3, 4], [0, 4, 7]
    # 0 -> ngram_max 4 / ngram_min 1
    assert lookup_draft(seq, None, 0, 0) == lookup_draft(seq, None, 4, 1) == R.draft(seq, None, 4, 1, 7) == [9, 1, 2, 3, 4]
    assert lookup_draft(seq, None, 3, 0) == R.draft(seq, None, 3, 1, 7)
    assert lookup_draft([5, 6, 4], hint, 0, 0) == [7] == R.draft([5, 6, 4], hint, 4, 1, 7)  # reached ngram_min = 1
    assert lookup_draft([5, 6, 4], hint, 0, 2) == []
    arr = (C.c_int32 * 4)(1, 2, 1, 2)
    out = (C.c_int32 * 4)()
    none = C.POINTER(C.c_int32)()
    f = lib.kh_lookup_draft
    assert f(arr, 4, none, 0, 4, 1, out, 4) == 2 and list(out[:2]) == [1, 2]
    assert f(arr, 0, none, 0, 4, 1, out, 4) == 0          # an empty sequence drafts nothing
    assert f(none, 0, none, 0, 4, 1, none, 0) == 0
    assert f(arr, 4, none, 0, 2, 3, out, 4) == _ffi.KH_ERR_INVALID_ARG   # ngram_max < ngram_min
    assert f(arr, 4, none, 0, 0, 5, out, 4) == _ffi.KH_ERR_INVALID_ARG   # ... after the default: 4 < 5
    assert f(arr, 4, none, 0, -1, 1, out, 4) == _ffi.KH_ERR_INVALID_ARG
    assert f(arr, -1, none, 0, 4, 1, out, 4) == _ffi.KH_ERR_INVALID_ARG
    assert f(none, 4, none, 0, 4, 1, out, 4) == _ffi.KH_ERR_INVALID_ARG  # a size without a pointer
    assert f(arr, 4, none, 3, 4, 1, out, 4) == _ffi.KH_ERR_INVALID_ARG
    assert f(arr, 4, none, 0, 4, 1, none, 4) == _ffi.KH_ERR_INVALID_ARG
    assert f(arr, 4, none, 0, 4, 1, out, -1) == _ffi.KH_ERR_INVALID_ARG


def test_entry_points_reject_bad_arguments_without_touching_the_device(lib):
    fake = C.c_void_p(0x1000)  # never dereferenced: these checks come first
    toks = (C.c_int32 * 4)(1, 2, 3, 4)
    out = (C.c_int32 * 8)()
    n = C.c_int32(0)
    none = C.POINTER(C.c_int32)()
    bad = _ffi.KH_ERR_INVALID_ARG
    v = lib.kh_model_verify
    assert v(None, toks, 4, 0, out, C.byref(n)) == bad
    assert v(fake, none, 4, 0, out, C.byref(n)) == bad
    assert v(fake, toks, 0, 0, out, C.byref(n)) == bad
    assert v(fake, toks, 4, -1, out, C.byref(n)) == bad
    assert v(fake, toks, 4, 0, none, C.byref(n)) == bad
    assert v(fake, toks, 4, 0, out, None) == bad
    assert lib.kh_model_verify_width(None, C.byref(n)) == bad
    assert lib.kh_model_verify_width(fake, None) == bad
    g = lib.kh_model_generate_lookup

    def opts(*a):
        return C.byref(_ffi.LookupOpts(*a))
    ok = opts(0, 0, 0, None, 0)
    assert g(None, toks, 4, 8, none, 0, ok, out, C.byref(n), None, None) == bad
    assert g(fake, none, 4, 8, none, 0, ok, out, C.byref(n), None, None) == bad
    assert g(fake, toks, 0, 8, none, 0, ok, out, C.byref(n), None, None) == bad
    assert g(fake, toks, 4, 0, none, 0, ok, out, C.byref(n), None, None) == bad
    assert g(fake, toks, 4, 8, none, 1, ok, out, C.byref(n), None, None) == bad   # stop count without a pointer
    assert g(fake, toks, 4, 8, none, 0, ok, none, C.byref(n), None, None) == bad
    assert g(fake, toks, 4, 8, none, 0, ok, out, None, None, None) == bad
    for o in (opts(2, 3, 1, None, 0), opts(0, 5, 1, None, 0), opts(-1, 1, 1, None, 0), opts(4, 1, 9, None, 0),
              opts(4, 1, -1, None, 0), opts(4, 1, 1, None, 3), opts(4, 1, 1, None, -1)):
        assert g(fake, toks, 4, 8, none, 0, o, out, C.byref(n), None, None) == bad
    r = lib.kh_argmax_rows_f32
    assert r(None, 8, 8, 1, fake, None) == bad
    assert r(fake, 8, 8, 1, None, None) == bad
    assert r(fake, 0, 8, 1, fake, None) == bad
    assert r(fake, 8, 8, 0, fake, None) == bad
    assert r(fake, 9, 8, 1, fake, None) == bad    # row_stride < n
    assert r(fake, 5, 6, 1, fake, None) == bad    # row_stride not a multiple of 4
