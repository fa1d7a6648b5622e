"""fp64 twin of the log-probabilities (include/kuiper_hip.h, "Log-probabilities"; csrc/kh_logprobs.h).

The logits are the device's float32 values; everything after that is float64.  The order is the sampler's: logit
descending, index ascending (-0 and +0 are one value), so ties at the cut go to the lower index and -inf entries come
last in index order."""
import numpy as np

MAX_TOP = 20


def order(logits):
    """token ids in the order (logit descending, index ascending)"""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    return np.lexsort((np.arange(l.size), -l))  # (the last key is the primary one; lexsort is stable)


def logprobs(logits, top_n=0):
    """-> (lse, lp[V], top_ids[top_n], top_lp[top_n]) in float64 / int64; lp is -inf where the logit is"""
    l32 = np.asarray(logits, dtype=np.float32)
    assert l32.ndim == 1 and 0 <= top_n <= min(MAX_TOP, l32.size)
    l = l32.astype(np.float64)
    assert not np.isnan(l).any() and not np.isposinf(l).any() and np.isfinite(l).any()
    m = l.max()
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(l - m).sum())
        lp = l - lse
    top_ids = order(l32)[:top_n].astype(np.int64)
    return float(lse), lp, top_ids, lp[top_ids]


def tol(V, lse, lp=0.0):
    """The bound the device's fp32 values are held to: 2^-24 (ceil(V / 1024) + 16) covers the sum of exp - a
    thread's chain of adds, the tree over the workgroup, expf and its argument - and 2^-23 (|lse| + |lp|) the
    roundings of m + log Z and l - lse."""
    return 2.0 ** -24 * (-(-V // 1024) + 16) + 2.0 ** -23 * (abs(lse) + abs(lp))
