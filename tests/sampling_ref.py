"""fp64 statement of the sampler's semantics (include/kuiper_hip.h, kh_sampling) and the checker the GPU tests use.

    S, w = kept_set(logits, T, K, P)       the set S in (logit desc, index asc) order and the weights of S
    pick(logits, T, K, P, seed, counter)   the token the semantics select
    Checker(logits).accepts(...)           whether GPU picks are the semantics' picks up to fp32 round-off
"""
from __future__ import annotations

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
