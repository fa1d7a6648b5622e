"""CPU checks of the screened classifier's interval (csrc/kh_cls_screen.h) on the numpy reference of
tests/cls_screen_ref.py: for every row the logit k_cls would store - the fp32 sum in k_cls's own order - lies inside
[a - b, a + b], the interval k_cls_screen forms from the bf16 copy; and the argmax decided from the intervals is the
argmax of the logits, ties to the lowest index."""
import numpy as np
import pytest

import cls_screen_ref as R

F32 = np.float32


def _rows(K, rng, n_random=384):
    """Seeded N(0, 0.02) rows as binfmt.synth_image draws them, and the rows an exporter can also produce: zeros,
    denormals, large outliers of either sign, rows of one magnitude that all round the same way, huge rows."""
    W = rng.normal(0.0, 0.02, (n_random, K)).astype(F32)
    special = []
    special.append(np.zeros(K, F32))
    special.append(np.full(K, 1e-40, F32))                                  # denormals
    special.append((rng.normal(0, 1, K) * 1e-39).astype(F32))               # signed denormals
    z = rng.normal(0.0, 0.02, K).astype(F32)
    z[::97] = 1e3
    special.append(z.copy())                                               # + outliers
    z[::89] = -1e3
    special.append(z.copy())                                               # +- outliers
    special.append(np.full(K, F32(1.00390625) * F32(0.02), F32))           # every weight rounds the same way
    special.append(-np.full(K, F32(1.0 + 2.0 ** -9 + 2.0 ** -20), F32))    # just above a bf16 tie
    special.append((rng.normal(0.0, 0.02, K) * 1e4).astype(F32))           # a row 10^4 times the others
    special.append((rng.normal(0.0, 1.0, K) * 1e-20).astype(F32))          # tiny but normal
    z = np.zeros(K, F32)
    z[K // 2] = 3e38                                                       # bf16 rounds it to +inf
    special.append(z)
    return np.concatenate([W, np.stack(special)], 0)


@pytest.mark.parametrize("K", [896, 2048, 4096])
@pytest.mark.parametrize("xkind", ["unit", "outliers", "tiny", "zero"])
def test_fp32_ordered_logit_lies_inside_the_interval(K, xkind):
    rng = np.random.default_rng(1000 + K)
    W = _rows(K, rng)
    x = rng.normal(0.0, 1.0, K).astype(F32)
    if xkind == "outliers":
        x[::61] *= 50.0
    elif xkind == "tiny":
        x *= F32(1e-18)
    elif xkind == "zero":
        x[:] = 0
    wnorm = (1.0 + rng.normal(0.0, 0.05, K)).astype(F32)
    for wg in (256, 512):
        logits, lb, ub, b = R.screen_and_logits(W, x, wnorm, eps=1e-5, wg=wg)
        fin = np.isfinite(logits)
        assert fin[:384].all()
        ok = (lb <= logits) & (logits <= ub)
        bad = np.flatnonzero(fin & ~ok)
        assert bad.size == 0, (K, xkind, wg, bad[:5], logits[bad[:5]], lb[bad[:5]], ub[bad[:5]])
        # a non-finite logit (the 3e38 row: its bf16 is +inf) must carry the interval of everything
        nf = np.flatnonzero(~fin)
        assert np.all(lb[nf] == -np.inf) and np.all(ub[nf] == np.inf)
        if xkind == "unit":
            # the bound is the bf16 rounding, not slack: per row |w - bf16 w|_2 |g|_2 is about 0.02 sqrt(K) 2^-9 /
            # sqrt(3) x sqrt(K) = 0.068 at K = 2048 (unit-rms input, relative rounding error uniform in +-2^-9)
            want = 0.02 * K * 2.0 ** -9 / np.sqrt(3.0)
            assert 0.5 * want < np.median(b[:384]) < 1.5 * want, (np.median(b[:384]), want)


def test_bf16_copy_rounds_to_nearest_even_and_err_is_an_upper_bound():
    w = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8,
                  0.0, -0.0, 1e-40, np.inf, -np.inf, 3.4e38], F32)
    b = R.bf16_rne(w)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, -0.0, 0.0, np.inf, -np.inf, np.inf], F32)
    # 1e-40 sits below half of the smallest bf16 denormal (2^-133 = 9.2e-41 ... its half is 4.6e-41): rounds to 2^-133
    want[7] = F32(2.0 ** -133)
    np.testing.assert_array_equal(b.view(np.uint32), want.view(np.uint32))
    assert np.isnan(R.bf16_rne(np.array([np.nan], F32))[0])
    rng = np.random.default_rng(7)
    W = rng.normal(0.0, 0.02, (64, 2048)).astype(F32)
    Wb, e = R.cls_err(W)
    exact = np.sqrt(((W.astype(np.float64) - Wb.astype(np.float64)) ** 2).sum(1))
    assert np.all(e.astype(np.float64) >= exact)
    assert np.all(e.astype(np.float64) <= exact * 1.02)  # the rounding term is a small part of it at this length


@pytest.mark.parametrize("K", [896, 2048])
def test_argmax_from_the_intervals_is_the_argmax_of_the_logits(K):
    rng = np.random.default_rng(K)
    W = rng.normal(0.0, 0.02, (4096, K)).astype(F32)
    wnorm = np.ones(K, F32)
    x = rng.normal(0.0, 1.0, K).astype(F32)
    logits, lb, ub, _ = R.screen_and_logits(W, x, wnorm)
    tok, n, over = R.screened_argmax(logits, lb, ub, cap=32)
    assert tok == int(np.argmax(logits)) and not over and 1 <= n <= 4, (tok, n, over)
    # two identical best rows: both are candidates, the lower index wins
    best = int(np.argmax(logits))
    W2 = W.copy()
    other = (best + 1234) % W.shape[0]
    W2[other] = W2[best]
    logits, lb, ub, _ = R.screen_and_logits(W2, x, wnorm)
    tok, n, over = R.screened_argmax(logits, lb, ub, cap=32)
    assert tok == min(best, other) and n >= 2 and not over
    # hundreds of rows inside the bound of the best: overflow, and the exact classifier decides
    W3 = W.copy()
    for i in range(300):
        r = W[best].copy()
        r[i] = np.nextafter(r[i], F32(np.inf) if i % 2 else F32(-np.inf))
        W3[(best + 1 + i) % W.shape[0]] = r
    logits, lb, ub, _ = R.screen_and_logits(W3, x, wnorm)
    tok, n, over = R.screened_argmax(logits, lb, ub, cap=32)
    assert over and n > 300 and tok == int(np.argmax(logits))
    # every logit equal (final norm all zeros): every row is a candidate, token 0
    logits, lb, ub, _ = R.screen_and_logits(W, x, np.zeros(K, F32))
    tok, n, over = R.screened_argmax(logits, lb, ub, cap=32)
    assert over and n == W.shape[0] and tok == 0 and np.all(logits == 0)


def test_lane_dot_layout_cache_is_the_plain_formula():
    """cls_screen_R.LaneDot lays the matrix out once for many vectors; its sums are those of the plain formula
    (pad, one fp32 FMA per weight and lane with the lanes past the end skipped, the butterfly), bit for bit, on rows
    with NaN, Inf and huge weights, at a row length that ends inside a round of loads, for both load widths."""
    rng = np.random.default_rng(5)
    K = 1152 + 64
    W = rng.normal(0.0, 0.05, (9, K)).astype(F32)
    W[1, 7] = np.nan
    W[2, K - 1] = np.inf
    W[3, 100] = -np.inf
    W[4, 5] = F32(3.4e38)
    W[5] = 0
    g = rng.normal(0.0, 1.0, K).astype(F32)
    g[::61] *= 50

    def plain(W, g, per_load):
        n, K = W.shape
        rounds = (K // per_load + R.WAVE - 1) // R.WAVE
        pad = rounds * R.WAVE * per_load
        Wp = np.zeros((n, pad), F32)
        Wp[:, :K] = W
        gp = np.zeros(pad, F32)
        gp[:K] = g
        Wp = Wp.reshape(n, rounds, R.WAVE, per_load)
        gp = gp.reshape(rounds, R.WAVE, per_load)
        valid = (np.arange(pad) < K).reshape(rounds, R.WAVE, per_load)
        acc = np.zeros((n, R.WAVE), F32)
        for j in range(rounds):
            for e in range(per_load):
                nxt = R._fma(Wp[:, j, :, e], np.broadcast_to(gp[j, :, e], (n, R.WAVE)), acc)
                acc = np.where(valid[j, :, e][None, :], nxt, acc)
        return R._butterfly(acc)

    for per_load in (4, 8):
        for vec in (g, np.zeros(K, F32)):
            got = R.LaneDot(W, per_load).dot(vec)
            want = plain(W, vec, per_load)
            assert got.dtype == F32
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (per_load, got, want)
        assert np.array_equal(R.lane_dot(W, g, per_load).view(np.uint32), plain(W, g, per_load).view(np.uint32))

