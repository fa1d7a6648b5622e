"""fp64 statement of the sampler's semantics (include/kuiper_hip.h, kh_sampling) and the checker the GPU tests use.

    S, w = kept_set(logits, T, K, P)       the set S in (logit desc, index asc) order and the weights of S
    pick(logits, T, K, P, seed, counter)   the token the semantics select
    Checker(logits).accepts(...)           whether GPU picks are the semantics' picks up to fp32 round-off

Exact statements for TWO-LEVEL rows (tests/test_sampler_edges_gpu.py).  The device weighs a token with
round(expf(e) * 2^sb), e = (l - l_max) / T in fp32: exactly 2^sb at e == 0 and exactly 0 at e <= -104 or l = -inf.
On a row whose tokens sit either at the maximum (the set A) or at such a zero-weight level every sum the sampler forms
is an integer multiple of 2^sb, so its kept set and its pick are integers with no rounding anywhere:

    two_level_kept(nA, V, K, P)                        (n, m): top-k keeps n tokens of A, top-p the first m of them
    two_level_pick(A_sorted, V, K, P, seed, counter)   the pick: A_sorted[floor(u * m)] with u an exact rational
    philox_u24(seed, counters)                         x >> 8 of a whole array of counters (numpy uint64)
    extreme_counters(seed)                             the counters of the smallest and the largest u among the first 2^20
    predict_path(logits, T, K, P)                      which branches of kh_sample_core such a row takes
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TOL = 1e-5


def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = (int(x) & MASK for x in ctr)
    k0, k1 = (int(x) & MASK for x in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
    return c0, c1, c2, c3


def uniform(seed: int, counter: int) -> float:
    x = philox4x32_10((counter & MASK, 0, 0, 0), (seed & MASK, (seed >> 32) & MASK))[0]
    return ((x >> 8) + 0.5) * 2.0 ** -24


def order(logits) -> np.ndarray:
    """token indices sorted by (logit descending, index ascending)"""
    lg = np.asarray(logits, np.float64)
    return np.lexsort((np.arange(lg.size), -lg))


def kept_set(logits, T, K, P, ordr=None, slack=0):
    """(S in order, fp64 weights of S in order, Z of the top-k set).  slack = -1 / +1: the top-p prefix one token
    shorter / longer than the semantics' (the checker's tolerance at the top-p edge)."""
    lg = np.asarray(logits, np.float64)
    o = order(lg) if ordr is None else ordr
    V = lg.size
    keep = o[:K] if 0 < K < V else o
    w = np.exp((lg[keep] - lg.max()) / T)
    zk = w.sum()
    n = len(keep)
    if P < 1:
        cum = np.cumsum(w)
        n = int(np.searchsorted(cum, P * zk, side="left")) + 1  # shortest prefix with sum >= P * Z
        n = min(max(n + slack, 1), len(keep))
    return keep[:n], w[:n], zk


def _pick_in(S, w, u):
    idx = np.argsort(S, kind="stable")
    s_idx, s_w = S[idx], w[idx]
    cum = np.cumsum(s_w)
    j = int(np.searchsorted(cum, u * cum[-1], side="right"))
    return int(s_idx[min(j, len(s_idx) - 1)])


def pick(logits, T, K, P, seed, counter) -> int:
    lg = np.asarray(logits, np.float64)
    if T <= 0:
        return int(np.argmax(lg))
    S, w, _ = kept_set(lg, T, K, P)
    return _pick_in(S, w, uniform(seed, counter))


class Checker:
    """Accepts a pick j when it is the semantics' pick, or when u * Z_S lies within TOL * Z_S of the boundary between
    j and its neighbour in index order; at the top-p edge, the sets one token shorter / longer are admitted when the
    edge token's cumulative weight is within TOL relative of P."""

    def __init__(self, logits):
        self.lg = np.asarray(logits, np.float64)
        self.o = order(self.lg)

    def sets(self, T, K, P):
        base = kept_set(self.lg, T, K, P, self.o)
        out = [base]
        if P < 1:
            S, w, zk = base
            cum = np.cumsum(w)
            if len(S) > 1 and cum[-2] >= P * zk * (1 - TOL):
                out.append(kept_set(self.lg, T, K, P, self.o, slack=-1))
            if cum[-1] <= P * zk * (1 + TOL):
                longer = kept_set(self.lg, T, K, P, self.o, slack=+1)
                if len(longer[0]) > len(S):
                    out.append(longer)
        return out

    def accepts(self, T, K, P, seed, counters, picks):
        """-> bool array, one per (counter, pick)"""
        picks = np.asarray(picks, np.int64)
        counters = np.asarray(counters, np.int64)
        if T <= 0:
            return picks == int(np.argmax(self.lg))
        ok = np.zeros(picks.size, bool)
        us = np.array([uniform(seed, int(c)) for c in counters])
        for S, w, _ in self.sets(T, K, P):
            idx = np.argsort(S, kind="stable")
            s_idx, s_w = S[idx], w[idx]
            cum = np.cumsum(s_w)
            z = cum[-1]
            thr = us * z
            pos = np.searchsorted(s_idx, picks)
            inside = (pos < s_idx.size) & (s_idx[np.minimum(pos, s_idx.size - 1)] == picks)
            p = np.minimum(pos, s_idx.size - 1)
            before = np.where(p > 0, cum[np.maximum(p - 1, 0)], 0.0)
            after = cum[p]
            tol = TOL * z
            ok |= inside & (before - tol <= thr) & (thr < after + tol)
        return ok


# ---- exact statements for two-level rows -----------------------------------------------------------------------------
SAMP_NB, SAMP_BPU, SAMP_CAP = 2048, 32, 4096  # kh_sample.h: KH_SAMP_NB, KH_SAMP_BPU, KH_SAMP_CAP


def philox_u24(seed: int, counters) -> np.ndarray:
    """x >> 8 for x = Philox4x32-10(counter (c, 0, 0, 0), key (seed lo, seed hi))[0], for an array of counters at once
    (uint64 arithmetic: a 32 x 32-bit product fits)"""
    u = np.uint64
    mask, sh = u(MASK), u(32)
    c0 = np.asarray(counters).astype(np.uint64) & mask
    c1, c2, c3 = np.zeros_like(c0), np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = u(M0) * c0, u(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ u(k0), p1 & mask, (p0 >> sh) ^ c3 ^ u(k1), p0 & mask
    return c0 >> u(8)


def extreme_counters(seed: int, n: int = 1 << 20):
    """(counter of the smallest u, counter of the largest u) among the counters 0 .. n - 1 of a seed"""
    x = philox_u24(seed, np.arange(n, dtype=np.uint64))
    return int(np.argmin(x)), int(np.argmax(x))


def two_level_kept(nA: int, V: int, K: int, P: float):
    """(n, m) on a two-level row with nA tokens at the maximum: top-k keeps the first n of them (tokens of weight zero
    beyond them never matter), top-p the first m = ceil(P32 * n) of those, P32 the fp32 value of P as a rational."""
    n = K if 0 < K < V and K < nA else nA
    p32 = Fraction(float(np.float32(P)))
    m = n if p32 >= 1 else min(n, max(1, math.ceil(p32 * n)))
    return n, m


def two_level_pick(A_sorted, V: int, K: int, P: float, seed: int, counter: int) -> int:
    """The pick on a two-level row whose maximum sits at the ascending indices A_sorted: S = the first m of them, each
    of weight one, and the pick is the first whose prefix count exceeds u * m: S[floor(u * m)], with
    u = ((x >> 8) + 1/2) / 2^24 = (2 (x >> 8) + 1) / 2^25 exactly.  Integer arithmetic only."""
    if V <= 1:
        return 0
    _, m = two_level_kept(len(A_sorted), V, K, P)
    x = philox4x32_10((counter & MASK, 0, 0, 0), (seed & MASK, (seed >> 32) & MASK))[0] >> 8
    return int(A_sorted[((2 * x + 1) * m) >> 25])


def bins_f32(logits, T):
    """(e, first-pass bin) of every token in the header's fp32 arithmetic (KhSampCtx::expo / bin_of):
    e = (l - l_max) / T; bin = min(int(-e * 32), 2047) while e > -64, else 2047."""
    lg = np.asarray(logits, np.float32)
    with np.errstate(invalid="ignore"):
        e = (lg - lg.max()) / np.float32(T)
    assert e.dtype == np.float32
    scaled = -np.maximum(e, np.float32(-SAMP_NB // SAMP_BPU)) * np.float32(SAMP_BPU)
    return e, np.minimum(scaled.astype(np.int64), SAMP_NB - 1)


def predict_path(logits, T, K, P) -> dict:
    """The control flow of kh_sample_core on a two-level row, from the header's rules alone: the candidate count, whether
    the candidates are compacted into LDS, which radix descents run and whether the boundary key is cut by index.
    Tokens sit at the maximum (e == 0: bin 0, weight one), at a zero-weight level (e <= -104 or -inf: the last bin),
    or - only where 0 < K <= |A| cuts it off - at a weighted third level in a bin of its own."""
    lg = np.asarray(logits, np.float32)
    V = lg.size
    if V <= 1:
        return {"trivial": True}
    e, b = bins_f32(lg, T)
    top = e == 0
    zero = ~top & ((e <= -104) | np.isneginf(lg))
    third = ~top & ~zero
    nA = int(top.sum())
    use_k = 0 < K < V
    use_p = bool(np.float32(P) < 1)
    assert (b[top] == 0).all() and (b[zero] == SAMP_NB - 1).all()
    if third.any():
        assert use_k and K <= nA and (b[third] > 0).all(), "a weighted third level only where top-k cuts it off"
    # candidates: the bins up to the one where the top-k count (without top-k: the top-p weight) is reached
    cum = np.cumsum(np.bincount(b, minlength=SAMP_NB))
    if use_k:
        ncand = int(cum[np.searchsorted(cum, K, side="left")])
    elif use_p:
        ncand = int(cum[0])  # all the weight is in bin 0, and 0 < P32 * Z <= Z
    else:
        ncand = V
    descents, bounded, m_key, ties = [], False, 0, 0
    if use_k:  # the order key of the K-th token, the count above it and the run of its equals
        t = np.sort(lg)[::-1][K - 1]
        m_key, ties, bounded = K - int((lg > t).sum()), int((lg == t).sum()), True
        descents.append("top-k key")
    if use_p:  # the weight P32 * Z_S is always reached inside A: the boundary key is the maximum
        m_key, ties, bounded = two_level_kept(nA, V, K, P)[1], nA, True
        descents.append("top-p key")
    cut = bounded and m_key < ties
    if cut:
        descents.append("index cut")
    descents.append("pick")
    vbits = V.bit_length()
    return {"trivial": False, "ncand": ncand, "in_lds": ncand <= SAMP_CAP, "descents": tuple(descents),
            "mode": ("neither", "top-k only", "top-p only", "both")[use_k + 2 * use_p], "index_cut": cut,
            "m_key": m_key, "ties": ties, "m_key_lt_ties": bounded and m_key < ties,
            "levels": 1 if vbits <= 8 else 2 if vbits <= 19 else 3}
