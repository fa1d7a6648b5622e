"""numpy reference of the screened classifier's interval (kuiperllama_amd/csrc/kh_cls_screen.h): the bf16 copy, the
per-row error norm, the fp32-ordered sums of k_cls and k_cls_screen, and [a - b, a + b].

fp32 arithmetic is emulated operation by operation: a product of two fp32 values is exact in fp64, so
fma(a, b, c) = fp32(fp64(a) * fp64(b) + fp64(c)) up to a double rounding that can move the fp32 result by one
unit in the last place in rare cases - still a correctly ordered fp32 sum in the sense of the error analysis (one
rounding of relative size <= 2^-24 (1 + 2^-29) per operation), which is all the interval claims to cover.
"""
import numpy as np

F32 = np.float32
WAVE = 64


def bf16_rne(w):
    """fp32 -> bf16 (round to nearest even) -> fp32, NaN kept quiet: kh_cls_screen.h::bf16_rne."""
    u = np.ascontiguousarray(w, dtype=F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    r = np.where(nan, (u >> 16) | 0x40, r)
    return ((r & 0xffff) << 16).astype(np.uint32).view(F32)


def gamma2(K):
    n = (K + WAVE - 1) // WAVE + 8
    u = 2.0 ** -24
    return 2.0 * n * u / (1.0 - n * u)


def cls_err(W):
    """Per-row e[r] >= |w - bf16(w)|_2 + 2 gamma_n (|w|_2 + |bf16(w)|_2), fp64, rounded up to fp32."""
    W = np.asarray(W, dtype=F32)
    Wb = bf16_rne(W)
    W64, B64 = W.astype(np.float64), Wb.astype(np.float64)
    with np.errstate(all="ignore"):
        e = (np.sqrt(((W64 - B64) ** 2).sum(1)) + gamma2(W.shape[1]) * (np.sqrt((W64 ** 2).sum(1)) + np.sqrt((B64 ** 2).sum(1))))
        e = e * (1.0 + 1e-9)
        f = e.astype(F32)
        f = np.where(f.astype(np.float64) < e, np.nextafter(f, F32(np.inf)), f)
        f = np.where(e < np.inf, f, F32(np.inf))
    return Wb, f.astype(F32)


def _fma(a, b, c):
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _butterfly(v):
    """wave_sum: xor 1, 2, 4, 8, 16, 32 over the last axis of 64 lanes; every lane ends with the same sum."""
    idx = np.arange(WAVE)
    for k in (1, 2, 4, 8, 16, 32):
        with np.errstate(all="ignore"):
            v = (v + v[..., idx ^ k]).astype(F32)
    return v[..., 0]


class LaneDot:
    """lane_dot for many vectors against one matrix: the matrix is padded, widened and laid out once."""

    def __init__(self, W, per_load):
        W = np.asarray(W, dtype=F32)
        R, K = W.shape
        assert K % per_load == 0
        self.R, self.K, self.per_load = R, K, per_load
        nload = K // per_load
        self.rounds = (nload + WAVE - 1) // WAVE
        self.pad = self.rounds * WAVE * per_load
        Wp = np.zeros((R, self.pad), F32)
        Wp[:, :K] = W
        # [round, element of the load, row, lane], fp64: a product of two fp32 values is exact there
        self.Wp = np.ascontiguousarray(Wp.reshape(R, self.rounds, WAVE, per_load).transpose(1, 3, 0, 2), dtype=np.float64)
        self.valid = (np.arange(self.pad) < K).reshape(self.rounds, WAVE, per_load)

    def dot(self, g):
        gp = np.zeros(self.pad, np.float64)
        gp[:self.K] = np.asarray(g, dtype=F32)
        gp = gp.reshape(self.rounds, WAVE, self.per_load)
        acc = np.zeros((self.R, WAVE), np.float64)  # fp32 values
        for j in range(self.rounds):
            for e in range(self.per_load):
                with np.errstate(all="ignore"):
                    nxt = (self.Wp[j, e] * gp[j, :, e][None, :] + acc).astype(F32)
                v = self.valid[j, :, e]
                if v.all():
                    acc = nxt.astype(np.float64)
                else:
                    acc[:, v] = nxt[:, v]
        return _butterfly(acc.astype(F32))


def lane_dot(W, g, per_load):
    """The sum a wave forms for every row of W (fp32 values; bf16 rows are passed widened): lane l takes the loads
    l, l + 64, ... of `per_load` consecutive weights each (4: k_cls's float4, 8: k_cls_screen's eight bf16) and runs one
    FMA chain over them, then the butterfly.  Lanes past the end add exact zeros (skipped here)."""
    return LaneDot(W, per_load).dot(g)


def stage(x, wnorm, eps, wg):
    """Stager<true, ...>::finish + stage_rs at workgroup width wg: g = w_norm * x, rs; and the screen's |g|_2 factor
    cb = rs * sqrt(sum g^2) * (1 + 2^-17), all in fp32 in the kernels' order."""
    x = np.asarray(x, dtype=F32)
    wn = np.asarray(wnorm, dtype=F32)
    M = x.size
    M4 = M // 4
    g = (wn * x).astype(F32)
    maxv = (M4 + wg - 1) // wg

    def block_sum_sq(v):
        v4 = v.reshape(M4, 4)
        ss = np.zeros(wg, F32)
        for k in range(maxv):
            i = np.arange(wg) + k * wg
            ok = i < M4
            q = v4[np.where(ok, i, 0)]
            t = np.zeros(wg, F32)
            for e in range(4):
                t = _fma(q[:, e], q[:, e], t)
            ss = (ss + np.where(ok, t, F32(0))).astype(F32)
        waves = _butterfly(ss.reshape(wg // WAVE, WAVE))
        r = F32(0)
        for w in waves:
            r = F32(r + w)
        return r

    r = block_sum_sq(x)
    rs = F32(1.0) / np.sqrt(F32(F32(r / F32(M)) + F32(eps)), dtype=F32)
    gg = block_sum_sq(g)
    cb = F32(F32(rs * np.sqrt(gg, dtype=F32)) * F32(1.0 + 2.0 ** -17))
    return g, F32(rs), cb


def interval(s_bf, e, rs, cb):
    """k_cls_screen::track: a = rs * sum, b = fma(cb, e, |a| 2^-18) + 1e-30; non-finite -> (-inf, +inf)."""
    with np.errstate(all="ignore"):
        a = (s_bf * rs).astype(F32)
        b = (_fma(np.broadcast_to(cb, a.shape), e, (np.abs(a) * F32(2.0 ** -18)).astype(F32)) + F32(1e-30)).astype(F32)
        ok = (np.abs(a) < np.inf) & (b < np.inf)
        lb = np.where(ok, (a - b).astype(F32), F32(-np.inf))
        ub = np.where(ok, (a + b).astype(F32), F32(np.inf))
    return a, b, lb, ub


def screen_and_logits(W, x, wnorm, eps=1e-5, wg=512):
    """-> (logits as k_cls forms them, lb, ub, b) for every row of W."""
    g, rs, cb = stage(x, wnorm, eps, wg)
    Wb, e = cls_err(W)
    with np.errstate(all="ignore"):
        logits = (lane_dot(W, g, 4) * rs).astype(F32)
    _, b, lb, ub = interval(lane_dot(Wb, g, 8), e, rs, cb)
    return logits, lb, ub, b


def screened_argmax(logits, lb, ub, cap):
    """The sampler's decision from the intervals: (token, candidates, overflow).  Candidates are the rows whose upper
    bound reaches the best lower bound; more than `cap` of them is an overflow (the exact classifier decides)."""
    L = lb.max()
    cand = np.flatnonzero(ub >= L)
    if cand.size == 0 or cand.size > cap:
        return int(np.argmax(np.where(np.isnan(logits), -np.inf, logits))), cand.size, True
    v = np.where(np.isnan(logits[cand]), -np.inf, logits[cand])
    return int(cand[np.argmax(v)]), cand.size, False


def bf16_bits(w):
    """The 16 stored bits of bf16_rne(w), as k_cls_bf16_build writes them."""
    return (bf16_rne(w).view(np.uint32) >> 16).astype(np.uint16)


def err_exact64(W):
    """|w - bf16(w)|_2 + 2 gamma_n (|w|_2 + |bf16(w)|_2) per row in fp64, without the (1 + 1e-9) factor and without the
    rounding up to fp32: what every stored e[r] must reach.  inf for rows with a non-finite weight or bf16 weight."""
    W = np.asarray(W, dtype=F32)
    W64, B64 = W.astype(np.float64), bf16_rne(W).astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.sqrt(((W64 - B64) ** 2).sum(1)) + gamma2(W.shape[1]) * (np.sqrt((W64 ** 2).sum(1)) + np.sqrt((B64 ** 2).sum(1)))
    return np.where(e < np.inf, e, np.inf)


def gold_logits64(W, x, wnorm, eps):
    """The classifier in fp64 on the fp32 inputs: (W (wnorm o x)) / sqrt(mean(x^2) + eps)."""
    x64 = np.asarray(x, dtype=F32).astype(np.float64)
    g64 = np.asarray(wnorm, dtype=F32).astype(np.float64) * x64
    with np.errstate(all="ignore"):
        return (np.asarray(W, dtype=F32).astype(np.float64) @ g64) / np.sqrt((x64 * x64).mean() + float(eps))


def bf16_row_norms(W):
    """|bf16(w_r)|_2 per row, fp64."""
    with np.errstate(all="ignore"):
        return np.sqrt((bf16_rne(W).astype(np.float64) ** 2).sum(1))


def twin_tolerance(nb, K, g, rs, b):
    """tau_r = 2 gamma_n rs |bf16(w_r)|_2 |g|_2 + 2^-5 b_r (nb = bf16_row_norms, K the row length): how far the GPU's
    lb / ub may lie from the twin's.  Both are fp32 sums of the same products in a valid order (first term: each within
    gamma_n of the exact sum); lb / ub are fp32 roundings of a -+ b, and for a row that is exact in bf16 b can be as
    small as 2^-18 |a| (second term)."""
    with np.errstate(all="ignore"):
        ng = np.sqrt((np.asarray(g, dtype=F32).astype(np.float64) ** 2).sum())
        return gamma2(K) * float(rs) * nb * ng + 2.0 ** -5 * b.astype(np.float64)
