"""numpy twin of the int8 tier of the screened classifier (kuiperllama_amd/csrc/kh_cls_screen.h): the group-scaled
int8 copy as k_cls_q8_build makes it, the fp64 bound its per-row table must reach, the fp32-ordered sum of
k_cls_screen_q8 and the interval [a8 - b8, a8 + b8].  fp32 operations are emulated as in cls_screen_ref.py, whose
stage() and interval() serve both tiers (same rs, same cb, same track())."""
import numpy as np

import cls_screen_ref as R

F32 = np.float32
G = 64      # weights per scale
LOAD = 16   # weights a lane takes per load: one FMA chain from 0, then one fma(scale, t, a)


def gamma2(K):
    """2 gamma_n with the tier's n = ceil(K / 64) + 24 (head of kh_cls_screen.h)."""
    n = (K + R.WAVE - 1) // R.WAVE + 24
    u = 2.0 ** -24
    return 2.0 * n * u / (1.0 - n * u)


def quantise(W):
    """(q int8 [R, K], sc fp32 [R, K / 64]): sc = max|w| / 127 per group in fp32, q = rint(w / sc) clamped to +-127;
    a group that is all zero or holds a NaN / Inf: sc = 0, q = 0."""
    W = np.asarray(W, dtype=F32)
    Rn, K = W.shape
    assert K % G == 0
    Wg = W.reshape(Rn, K // G, G)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(Wg).all(2)
        am = np.where(bad, F32(0), np.abs(np.where(np.isfinite(Wg), Wg, F32(0))).max(2)).astype(F32)
        sc = (am / F32(127.0)).astype(F32)
        t = np.where(sc[..., None] > 0, np.rint((Wg / np.where(sc > 0, sc, F32(1))[..., None]).astype(F32)), F32(0))
        t = np.where(np.isnan(t), F32(0), np.clip(t, -127, 127))
    return t.astype(np.int8).reshape(Rn, K), sc


def dequant64(q, sc):
    """sc o q in fp64 (exact: fp32 x 8-bit integer)."""
    Rn, K = q.shape
    return (q.reshape(Rn, K // G, G).astype(np.float64) * sc.astype(np.float64)[..., None]).reshape(Rn, K)


def quant_err64(W, q, sc):
    """|w_r - sc o q_r|_2 per row in fp64: what every stored e8[r] must reach; inf for rows with a NaN / Inf weight."""
    W64 = np.asarray(W, dtype=F32).astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.sqrt(((W64 - dequant64(q, sc)) ** 2).sum(1))
    return np.where(np.isfinite(W64).all(1) & (e < np.inf), e, np.inf)


def e8_twin(W, q, sc):
    """The table as k_cls_q8_build forms it: (|w - sc o q| + 2 gamma_n (|w| + |sc o q|)) (1 + 1e-9), rounded up."""
    W64 = np.asarray(W, dtype=F32).astype(np.float64)
    D = dequant64(q, sc)
    with np.errstate(all="ignore"):
        e = (np.sqrt(((W64 - D) ** 2).sum(1)) + gamma2(W64.shape[1]) * (np.sqrt((W64 ** 2).sum(1)) + np.sqrt((D ** 2).sum(1))))
        e = e * (1.0 + 1e-9)
        f = e.astype(F32)
        f = np.where(f.astype(np.float64) < e, np.nextafter(f, F32(np.inf)), f)
        f = np.where(e < np.inf, f, F32(np.inf))
    return f.astype(F32)


def lane_dot_q8(q, sc, g):
    """The sum a wave of k_cls_screen_q8 forms for every row: lane l takes the loads l, l + 64, ... of 16 weights (all of
    one group); per load t = 16 FMAs q_i g_i from 0, then a = fma(sc, t, a); then the butterfly."""
    Rn, K = q.shape
    nload = K // LOAD
    rounds = (nload + R.WAVE - 1) // R.WAVE
    g64 = np.asarray(g, dtype=F32).astype(np.float64)
    acc = np.zeros((Rn, R.WAVE), np.float64)  # fp32 values
    for j in range(rounds):
        lo, hi = j * R.WAVE, min(nload, (j + 1) * R.WAVE)
        n = hi - lo
        qq = q[:, lo * LOAD: hi * LOAD].reshape(Rn, n, LOAD).astype(np.float64)
        gg = g64[lo * LOAD: hi * LOAD].reshape(n, LOAD)
        t = np.zeros((Rn, n), np.float64)
        with np.errstate(all="ignore"):
            for e in range(LOAD):
                t = (qq[:, :, e] * gg[None, :, e] + t).astype(F32).astype(np.float64)
            s = sc[:, (np.arange(lo, hi) * LOAD) // G].astype(np.float64)
            acc[:, :n] = (s * t + acc[:, :n]).astype(F32).astype(np.float64)
    return R._butterfly(acc.astype(F32))


def intervals(q, sc, e8, x, wnorm, eps, wg):
    """-> (a8, b8, lb8, ub8) of every row at workgroup width wg."""
    g, rs, cb = R.stage(x, wnorm, eps, wg)
    return R.interval(lane_dot_q8(q, sc, g), e8, rs, cb)
