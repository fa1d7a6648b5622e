"""Token automata for constrained decoding (include/kuiper_hip.h, "Constrained decoding"; KuiperModel.set_constraint).

A TokenAutomaton is a deterministic automaton over token ids in CSR form: row s = tokens[row_ptr[s]:row_ptr[s + 1]] holds
the ids allowed in state s, ascending, and next[] the state behind each.  The end of the output is part of the
automaton: accepting states carry an edge on `eos` into a sink whose only edge is `eos` onto itself.

  from_choices(token_seqs, eos)          "answer with one of these": the trie of the sequences
  from_regex(pattern, vocab_bytes, eos)  "emit text that matches this pattern": full-match semantics over bytes
  vocab_bytes(tokenizer)                 the byte string of every token of a SpmTokenizer / BpeTokenizer
  union(automata)                        one automaton for sequences with different constraints, and their start states

Pure numpy; nothing here touches the GPU or the library.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np


class TokenAutomaton:
    def __init__(self, start: int, row_ptr, tokens, next):  # noqa: A002 (the header's name)
        self.start = int(start)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        self.tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        self.next = np.ascontiguousarray(next, dtype=np.int32)

    @property
    def n_states(self) -> int:
        return len(self.row_ptr) - 1

    @property
    def n_edges(self) -> int:
        return len(self.tokens)

    def check(self, vocab: int) -> None:
        """kh_fsm_check's checks; raises ValueError (IndexError for a token outside [0, vocab))."""
        n = self.n_states
        if n <= 0 or not 0 <= self.start < n:
            raise ValueError("n_states <= 0 or start outside [0, n_states)")
        rp = self.row_ptr
        if rp[0] != 0 or rp[-1] != len(self.tokens) or len(self.next) != len(self.tokens):
            raise ValueError("row_ptr does not run from 0 to n_edges")
        if np.any(np.diff(rp) <= 0):
            raise ValueError("row_ptr decreases, or a row has no edge")
        inner = np.ones(len(self.tokens), bool)
        inner[rp[:-1]] = False  # the first edge of every row has no left neighbour in its row
        if np.any(self.tokens[1:][inner[1:]] <= self.tokens[:-1][inner[1:]]):
            raise ValueError("a row is not strictly ascending")
        if np.any((self.next < 0) | (self.next >= n)):
            raise ValueError("next outside [0, n_states)")
        if np.any((self.tokens < 0) | (self.tokens >= vocab)):
            raise IndexError("token outside [0, vocab)")

    def allowed(self, state: int) -> np.ndarray:
        return self.tokens[self.row_ptr[state]:self.row_ptr[state + 1]]

    def step(self, state: int, token: int) -> int:
        """next(state, token), or -1 where the row does not hold the token."""
        lo, hi = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        i = lo + int(np.searchsorted(self.tokens[lo:hi], token))
        return int(self.next[i]) if i < hi and self.tokens[i] == token else -1

    def walk(self, tokens: Sequence[int], state: Optional[int] = None) -> Tuple[int, int]:
        """(state behind the tokens it could follow, how many those were): kh_fsm_walk."""
        s = self.start if state is None else int(state)
        for i, t in enumerate(tokens):
            nx = self.step(s, int(t))
            if nx < 0:
                return s, i
            s = nx
        return s, len(tokens)

    def forced_run(self, state: int, cap: int) -> List[int]:
        """The tokens that MUST follow from `state`, at most `cap`: while the row of the state holds exactly one id,
        that id, and on along its edge (rule (a) of kh_lookup_draft_fsm; the sink's self-edge keeps a run going)."""
        out, s = [], int(state)
        while len(out) < cap and self.row_ptr[s + 1] - self.row_ptr[s] == 1:
            e = int(self.row_ptr[s])
            out.append(int(self.tokens[e]))
            s = int(self.next[e])
        return out


def _from_rows(start: int, rows: List[dict]) -> TokenAutomaton:
    row_ptr, tokens, nxt = [0], [], []
    for r in rows:
        for t in sorted(r):
            tokens.append(t)
            nxt.append(r[t])
        row_ptr.append(len(tokens))
    return TokenAutomaton(start, row_ptr, tokens, nxt)


def from_choices(token_seqs: Sequence[Sequence[int]], eos: int) -> TokenAutomaton:
    """The trie of the given token sequences: exactly those, each followed by `eos`, are the accepted paths (a sequence
    that is a prefix of another is accepting mid-trie).  State 0 is the root, the last state the sink."""
    if len(token_seqs) == 0:
        raise ValueError("from_choices: no sequence")
    rows: List[dict] = [{}]
    accepting = []
    for seq in token_seqs:
        s = 0
        for t in seq:
            t = int(t)
            if t == eos:
                raise ValueError("from_choices: eos inside a sequence")
            if t not in rows[s]:
                rows.append({})
                rows[s][t] = len(rows) - 1
            s = rows[s][t]
        accepting.append(s)
    sink = len(rows)
    rows.append({int(eos): sink})
    for s in accepting:
        rows[s][int(eos)] = sink
    return _from_rows(0, rows)


def union(automata: Sequence[Optional[TokenAutomaton]]) -> Tuple[TokenAutomaton, List[int]]:
    """One automaton for sequences with different constraints (KuiperModel.seq_set_constraint): the given automata side
    by side, the states of automata[i] renumbered by the number of states ahead of it.  Returns (the union, starts):
    starts[i] is automata[i]'s start state in the union - the state to give sequence i's slot - and -1 where automata[i]
    is None (an unconstrained sequence).  An object given more than once is laid down once and its entries share the
    start (n samples under one constraint cost one copy).  The union's own `start` is that of the first automaton; the
    union of one automaton is that automaton.  ValueError where there is no automaton at all."""
    given = [a for a in automata if a is not None]
    if not given:
        raise ValueError("union: no automaton")
    starts, state0, edge0, seen = [], 0, 0, {}
    row_ptr, tokens, nxt = [np.zeros(1, np.int64)], [], []
    for a in automata:
        if a is None or id(a) in seen:
            starts.append(-1 if a is None else seen[id(a)])
            continue
        starts.append(state0 + a.start)
        seen[id(a)] = starts[-1]
        row_ptr.append(a.row_ptr[1:] + edge0)
        tokens.append(a.tokens)
        nxt.append(a.next + np.int32(state0))
        state0 += a.n_states
        edge0 += a.n_edges
    start = next(s for s in starts if s >= 0)
    return TokenAutomaton(start, np.concatenate(row_ptr), np.concatenate(tokens), np.concatenate(nxt)), starts


# ---- regular expressions over bytes --------------------------------------------------------------------------------
_META = set("\\.[]()|*+?{}^$")


def _set(*bs) -> np.ndarray:
    m = np.zeros(256, bool)
    for b in bs:
        if isinstance(b, tuple):
            m[b[0]:b[1] + 1] = True
        else:
            m[b] = True
    return m


_DIGIT = _set((48, 57))
_WORD = _set((48, 57), (65, 90), (97, 122), 95)
_SPACE = _set(9, 10, 11, 12, 13, 32)
_ANY = ~_set(10)


class _Parser:
    """pattern -> tree of ("set", mask) | ("cat", [..]) | ("alt", [..]) | ("rep", node, lo, hi) (hi None: unbounded)."""

    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0

    def fail(self, what: str):
        raise ValueError(f"from_regex: {what} at offset {self.i} of {self.p!r}")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() not in ("", "|", ")"):
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                lo, hi = 0, None
                self.i += 1
            elif c == "+":
                lo, hi = 1, None
                self.i += 1
            elif c == "?":
                lo, hi = 0, 1
                self.i += 1
            elif c == "{":
                j = self.p.find("}", self.i)
                body = self.p[self.i + 1:j] if j > 0 else ""
                parts = body.split(",")
                if j < 0 or len(parts) > 2 or not all(x.isascii() and x.isdigit() for x in parts):
                    self.fail("only {m} and {m,n} are supported")
                lo = int(parts[0])
                hi = int(parts[-1])
                if hi < lo:
                    self.fail("{m,n} with n < m")
                self.i = j + 1
            else:
                return node
            if self.peek() in ("?", "+"):
                self.fail("lazy and possessive quantifiers are not supported")
            node = ("rep", node, lo, hi)

    def escape(self, in_class: bool) -> np.ndarray:
        self.i += 1
        c = self.peek()
        if c == "":
            self.fail("dangling backslash")
        self.i += 1
        if c == "d":
            return _DIGIT
        if c == "w":
            return _WORD
        if c == "s":
            return _SPACE
        if c == "n":
            return _set(10)
        if c == "t":
            return _set(9)
        if c in _META or (in_class and c in "-"):
            return _set(ord(c))
        self.i -= 1
        self.fail(f"escape \\{c} is not supported")

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                self.fail("(?...) groups are not supported")
            node = self.alt()
            if self.peek() != ")":
                self.fail("missing ')'")
            self.i += 1
            return node
        if c == "[":
            return ("set", self.char_class())
        if c == ".":
            self.i += 1
            return ("set", _ANY)
        if c == "\\":
            return ("set", self.escape(False))
        if c in "*+?{":
            self.fail("nothing to repeat")
        if c in "^$}]":
            self.fail(f"{c!r} is not supported (the match is a full match; escape a literal)")
        self.i += 1
        raw = c.encode("utf-8")
        return ("set", _set(raw[0])) if len(raw) == 1 else ("cat", [("set", _set(b)) for b in raw])

    def char_class(self) -> np.ndarray:
        self.i += 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        m = np.zeros(256, bool)
        first = True
        while True:
            c = self.peek()
            if c == "":
                self.fail("missing ']'")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[":
                self.fail("'[' inside a class: escape it")
            if c == "\\":
                lo_set = self.escape(True)
            else:
                if ord(c) > 127:
                    self.fail("non-ASCII character in a class")
                self.i += 1
                lo_set = _set(ord(c))
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                if lo_set.sum() != 1:
                    self.fail("a range cannot start at a class escape")
                self.i += 1
                d = self.peek()
                if d == "\\":
                    hi_set = self.escape(True)
                else:
                    if ord(d) > 127:
                        self.fail("non-ASCII character in a class")
                    self.i += 1
                    hi_set = _set(ord(d))
                if hi_set.sum() != 1:
                    self.fail("a range cannot end at a class escape")
                lo, hi = int(np.argmax(lo_set)), int(np.argmax(hi_set))
                if hi < lo:
                    self.fail("reversed range")
                m[lo:hi + 1] = True
            else:
                m |= lo_set
        return ~m if neg else m


class _Nfa:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.on: List[Optional[Tuple[np.ndarray, int]]] = []

    def new(self) -> int:
        self.eps.append([])
        self.on.append(None)
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        """Thompson's construction: (entry, exit) of the fragment."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.on[a] = (node[1], b)
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                x, y = self.build(item)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for item in node[1]:
                x, y = self.build(item)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if hi is None:  # a loop behind the mandatory copies
            x, y = self.build(sub)
            end = self.new()
            self.eps[b] += [x, end]
            self.eps[y] += [x, end]
            return a, end
        end = self.new()
        for _ in range(hi - lo):  # each optional copy may be skipped, with everything behind it
            x, y = self.build(sub)
            self.eps[b] += [x, end]
            b = y
        self.eps[b].append(end)
        return a, end


def _byte_dfa(pattern: str) -> Tuple[np.ndarray, np.ndarray, int]:
    """(table [n, 256] int32 with -1 = dead, accepting [n] bool, start): the pruned byte-level DFA of the pattern -
    every state reaches an accepting one."""
    nfa = _Nfa()
    entry, final = nfa.build(_Parser(pattern).parse())
    sets = [t[0] for t in nfa.on if t is not None]
    # bytes that no set tells apart fall into one class
    sig = np.stack(sets, 0) if sets else np.zeros((1, 256), bool)
    _, cls_of = np.unique(sig.T, axis=0, return_inverse=True)
    cls_of = np.asarray(cls_of).reshape(-1)
    n_cls = int(cls_of.max()) + 1
    rep = [int(np.argmax(cls_of == k)) for k in range(n_cls)]

    def closure(states) -> frozenset:
        seen, todo = set(states), list(states)
        while todo:
            for y in nfa.eps[todo.pop()]:
                if y not in seen:
                    seen.add(y)
                    todo.append(y)
        return frozenset(seen)

    d0 = closure([entry])
    ids = {d0: 0}
    order = [d0]
    rows = []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        row = np.full(n_cls, -1, np.int64)
        for ci in range(n_cls):
            b = rep[ci]
            tgt = [nfa.on[x][1] for x in cur if nfa.on[x] is not None and nfa.on[x][0][b]]
            if not tgt:
                continue
            nxt = closure(tgt)
            if nxt not in ids:
                ids[nxt] = len(order)
                order.append(nxt)
                if len(order) > 20000:
                    raise ValueError("from_regex: the pattern needs more than 20000 DFA states")
            row[ci] = ids[nxt]
        rows.append(row)
    tab = np.stack(rows, 0)[:, cls_of]  # [n, 256]
    acc = np.array([final in st for st in order], bool)
    # states from which no accepting state is reachable go (their edges become dead)
    n = len(order)
    live = acc.copy()
    while True:
        reach = live[np.where(tab >= 0, tab, 0)] & (tab >= 0)
        new = live | reach.any(1)
        if np.array_equal(new, live):
            break
        live = new
    if not live[0]:
        raise ValueError("from_regex: the pattern matches nothing")
    renum = np.full(n + 1, -1, np.int64)
    renum[np.nonzero(live)[0]] = np.arange(int(live.sum()))
    tab = renum[np.where(tab >= 0, tab, n)][live]
    return tab.astype(np.int32), acc[live], int(renum[0])


def from_regex(pattern: str, vocab_bytes: Sequence[bytes], eos: int) -> TokenAutomaton:
    """Token sequences whose concatenated bytes FULLY match `pattern`, each followed by `eos`.

    The supported subset: literals; the escapes \\d \\w \\s \\. \\\\ \\n \\t and escaped metacharacters; `.` (any byte but
    \\n); classes and negated classes with ranges; groups; `|`; `* + ?`, `{m}`, `{m,n}`.  Anything else raises
    ValueError.  The classes are the ASCII ones of Python's `re` on bytes patterns.  vocab_bytes[i] is the byte string of
    token i; tokens with an empty byte string (specials) are never allowed, and `eos` is allowed exactly in accepting
    states, where it leads into the sink.  Pipeline: Thompson NFA, subset construction, removal of the states from which
    no accepting state is reachable, then the token-level index - every token's bytes walked from every state, vectorised
    over the tokens per byte position; states that no token path connects to the start or to the end are dropped.
    A model keeps ceil(V / 32) mask words per state of the automaton it is given (16 KiB at V = 128256) and refuses
    past 256 MiB of them (KH_FSM_MAX_MASK_BYTES): a pattern of thousands of states is a large object on the device."""
    tab, acc, d_start = _byte_dfa(pattern)
    V = len(vocab_bytes)
    eos = int(eos)
    if not 0 <= eos < V:
        raise ValueError("from_regex: eos outside the vocabulary")
    lens = np.fromiter((len(b) for b in vocab_bytes), np.int64, V)
    lens[eos] = 0  # the stop token is never spelled out
    L = int(lens.max()) if V else 0
    B = np.zeros((V, max(L, 1)), np.uint8)
    for j in range(L):  # byte j of every token that has one
        idx = np.nonzero(lens > j)[0]
        B[idx, j] = np.fromiter((vocab_bytes[i][j] for i in idx), np.uint8, len(idx))
    by_len = [np.nonzero(lens > j)[0] for j in range(L)]
    n = len(tab)
    sink = n
    edges_t, edges_n = [], []
    for s in range(n):
        cur = np.full(V, s, np.int32)
        cur[lens == 0] = -1
        for j in range(L):
            idx = by_len[j]
            idx = idx[cur[idx] >= 0]
            if len(idx) == 0:
                break
            cur[idx] = tab[cur[idx], B[idx, j]]
        t = np.nonzero(cur >= 0)[0]
        edges_t.append(t.astype(np.int32))
        edges_n.append(cur[t])
    # token-level pruning: states that reach the sink, among those the start reaches
    good = acc.copy()
    while True:
        new = good | np.array([bool(good[e].any()) for e in edges_n])
        if np.array_equal(new, good):
            break
        good = new
    if not good[d_start]:
        raise ValueError("from_regex: no token sequence of this vocabulary matches the pattern")
    keep, todo = {d_start}, [d_start]
    while todo:
        s = todo.pop()
        for y in np.unique(edges_n[s][good[edges_n[s]]]):
            if int(y) not in keep:
                keep.add(int(y))
                todo.append(int(y))
    order = sorted(keep)
    renum = np.full(n, -1, np.int64)
    renum[order] = np.arange(len(order))
    sink = len(order)
    row_ptr, tokens, nxt = [0], [], []
    for s in order:
        ok = good[edges_n[s]]
        t, y = edges_t[s][ok], renum[edges_n[s][ok]]
        if acc[s]:
            at = int(np.searchsorted(t, eos))
            t, y = np.insert(t, at, eos), np.insert(y, at, sink)
        tokens.append(t)
        nxt.append(y)
        row_ptr.append(row_ptr[-1] + len(t))
    tokens.append(np.array([eos], np.int32))
    nxt.append(np.array([sink], np.int64))
    row_ptr.append(row_ptr[-1] + 1)
    return TokenAutomaton(int(renum[d_start]), row_ptr, np.concatenate(tokens), np.concatenate(nxt))


def vocab_bytes(tokenizer) -> List[bytes]:
    """The byte string of every token id of a BpeTokenizer or SpmTokenizer, for from_regex.  Special tokens (BOS, EOS,
    the stop ids, SentencePiece's unknown) get b"", so a constraint never allows them.  BPE: the token's own bytes
    (decode_bytes of the single id, spaces as the tokenizer's ref_spaces setting decodes them).  SentencePiece: the
    decoder drops the space of a leading word-start marker, so each token is decoded behind a reference token and the
    reference's bytes are cut off; byte-fallback tokens give their single byte.  For every encoding without an
    unknown token the concatenated byte strings are the decoder's output (but for the text's first space, which the
    SentencePiece decoder drops)."""
    import ctypes as C

    from . import _ffi
    from .tokenizer import BpeTokenizer, SpmTokenizer
    n = tokenizer.vocab_size
    if isinstance(tokenizer, BpeTokenizer):
        special = {tokenizer.bos_id, tokenizer.eos_id, *tokenizer.stop_ids}
        return [b"" if i in special else tokenizer.decode_bytes([i]) for i in range(n)]
    if not isinstance(tokenizer, SpmTokenizer):
        raise TypeError("vocab_bytes: a BpeTokenizer or a SpmTokenizer")
    special = {tokenizer.bos_id, tokenizer.eos_id, tokenizer.unk_id}

    def raw(ids) -> bytes:
        arr = (C.c_int32 * len(ids))(*ids)
        cap = 64 * len(ids) + 64
        ln = C.c_int64(0)
        while True:
            out = C.create_string_buffer(cap)
            rc = _ffi.lib().kh_spm_decode(tokenizer._h, arr, len(ids), out, cap, C.byref(ln))
            if rc == _ffi.KH_ERR_RANGE and ln.value > cap:
                cap = ln.value
                continue
            _ffi.check(rc, "kh_spm_decode")
            return out.raw[:ln.value]
    # the reference: an ordinary piece of two letters at least (a byte-fallback token decodes to one byte, and the
    # decoder still drops the leading space of what follows it)
    ref = next(i for i in range(n) if i not in special and len(raw([i])) >= 2 and raw([i]).isalnum())
    head = raw([ref])
    out = []
    for i in range(n):
        if i in special:
            out.append(b"")
            continue
        both = raw([ref, i])
        out.append(both[len(head):] if both.startswith(head) else raw([i]))
    # byte-fallback tokens <0x80> .. <0xFF> are no text on their own: the decoder answers U+FFFD.  SentencePiece lays
    # the 256 byte tokens out in one run of ids, so the 128 of them are consecutive and the first is <0x80>
    bad = [i for i, b in enumerate(out) if b == b"\xef\xbf\xbd"]
    if bad:
        if len(bad) != 128 or bad[-1] - bad[0] != 127:
            raise ValueError("vocab_bytes: the byte-fallback tokens of this model are not one run of ids")
        for i in bad:
            out[i] = bytes([0x80 + i - bad[0]])
    return out
