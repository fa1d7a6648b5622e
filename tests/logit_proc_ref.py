"""numpy float32 twin of the logit processors (include/kuiper_hip.h, kh_penalties; csrc/kh_logit_proc.h).

Every operation is one numpy float32 operation, so it is rounded once and never contracted: the device result must
carry the same bits.  `history[j]` is the token fed at position j; the window ends at position `pos`."""
import numpy as np

F = np.float32


def window(history, pos, last_n):
    lo = max(0, pos + 1 - last_n) if last_n > 0 else 0
    return np.asarray(history[lo:pos + 1], dtype=np.int64)


def counts(history, pos, last_n, V):
    w = window(history, pos, last_n)
    w = w[(w >= 0) & (w < V)]
    return np.bincount(w, minlength=V)[:V]


def process(logits, history, pos, repetition=1.0, presence=0.0, frequency=0.0, last_n=0, bias=None):
    """-> processed copy of `logits` (float32).  bias: {id: value} or a list of (id, value)."""
    out = np.array(logits, dtype=F, copy=True)
    V = out.size
    r, pres, freq = F(repetition), F(presence), F(frequency)
    c = counts(history, pos, last_n, V)
    ids = np.nonzero(c)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        if ids.size and r != F(1):
            l = out[ids]
            out[ids] = np.where(l > 0, l / r, l * r).astype(F)
        if ids.size and (pres != F(0) or freq != F(0)):
            out[ids] = out[ids] - (c[ids].astype(F) * freq + pres)
        for i, b in (bias.items() if isinstance(bias, dict) else (bias or [])):
            out[int(i)] = out[int(i)] + F(b)
    assert out.dtype == F
    return out


def greedy(processed):
    """first maximum, lowest index"""
    return int(np.argmax(processed))
