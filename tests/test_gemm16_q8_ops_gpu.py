"""ops.gemm_q8_bf16 (kh_gemm_q8_bf16_f32): the K loop of KH_FLAG_GEMM16_Q8 (csrc/kh_gemm_q16.h) under its STORE epilogue
with a row-major B, against an fp64 statement of  y[t][m] = sum_g s[m][g] * sum_{k in g} q[m][k] * x[t][k]
(tests/gemm_q16_ref.py::gold).

Shapes (M, K, T), the smallest that reach each path (the entry picks tile and K split from its sizes):

  16, 64, 1       one block, R = 1, a range shorter than the ring
  32, 128, 17     R = 2, two token tiles, padding rows
  48, 576, 33     R = 1 because 32 does not divide M; nine blocks over two waves (4 + 5): a count that is neither below
                  nor a multiple of any ring depth
  64, 512, 40     NT = 4, two waves
  32, 2048, 512   four waves, every token slice

Bit for bit: integer x in [-64, 64] (every block of every token holds +64, -64 and zeros), weights over the whole int8
range with -128 and 127 in every row, power-of-two scales from 2^-6 .. 2^2.  Every product, every scaled partial and -
asserted by the test itself, from sum |s q x| against the row's smallest scale - every partial sum in any order is
exact in fp32, so the result must equal the fp64 gold cast to fp32, compared as raw bits.  (x is sparse - eight
non-zero columns per block - and a row's scales span three neighbouring powers of two, the rows together all nine: that
is what keeps 2048-column sums within 24 bits.)  One-hot x rows recover s * q for every column of every group: the
column permutation of the two MFMA steps and the scale's row ownership.

Tolerance: random unit-variance x, random scales:  |y - gold| <= 4 * 2^-24 * sum |s q x|  per element - at most three
fp32 accumulation steps per 32 columns beyond the exact products, far below it - and the present ops.matmul_q8 on the
same inputs must hold the same bound, which shows the input choice is fair.
"""
import numpy as np
import pytest
import torch

import gemm_q16_ref as ref
from kuiperllama_amd import _ffi, ops

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64, 1), (32, 128, 17), (48, 576, 33), (64, 512, 40), (32, 2048, 512)]
EPS = 2.0 ** -24


def _run(gpu, x, q, s, out=None):
    y = ops.gemm_q8_bf16(torch.from_numpy(x).to(gpu), torch.from_numpy(q).to(gpu), torch.from_numpy(s).to(gpu), out)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _weights(rng, M, K):
    q = rng.integers(-128, 128, (M, K)).astype(np.int8)
    cols = np.stack([rng.permutation(K)[:2] for _ in range(M)])
    q[np.arange(M), cols[:, 0]] = -128
    q[np.arange(M), cols[:, 1]] = 127
    return q


def _pow2_scales(rng, M, G):
    """scales[M][G]: row r draws from 2^(e_r) .. 2^(e_r + 2), e_r in -6 .. 0 - all nine exponents -6 .. 2 over the rows"""
    e_r = np.arange(M) % 7 - 6
    e = e_r[:, None] + rng.integers(0, 3, (M, G))
    e[:, 0] = e_r  # (a row's smallest scale is e_r whenever G > 0)
    return np.exp2(e).astype(np.float32)


def _exact_case(rng, M, K, T):
    G = K // 64
    q, s = _weights(rng, M, K), _pow2_scales(rng, M, G)
    x = np.zeros((T, K), np.float32)
    for t in range(T):
        for g in range(G):
            c = 64 * g + rng.permutation(64)[:8]
            x[t, c] = np.concatenate([[64, -64], rng.integers(-64, 65, 6)]).astype(np.float32)
    return x, q, s


@pytest.mark.parametrize("M,K,T", SHAPES)
def test_integers_and_power_of_two_scales_are_bit_exact(gpu, M, K, T):
    rng = np.random.default_rng(100000 * M + 10 * K + T)
    x, q, s = _exact_case(rng, M, K, T)
    assert q.min() == -128 and q.max() == 127 and set(np.log2(s).ravel().tolist()) <= set(range(-6, 3))
    for g in range(K // 64):
        blk = x[:, 64 * g:64 * g + 64]
        assert np.all(blk.max(axis=1) == 64) and np.all(blk.min(axis=1) == -64) and np.all((blk == 0).sum(axis=1) >= 56)
    g64, mag = ref.gold(x, q, s)
    # every partial sum, in any order, is a multiple of the row's smallest scale and below 2^24 of them: exact in fp32
    assert float((mag / s.min(axis=1)[None, :].astype(np.float64)).max()) < 2.0 ** 24
    got = _run(gpu, x, q, s)
    want = g64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), g64)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), f"M {M} K {K} T {T}: {len(bad)} of {got.size} differ, first (token, row) {bad[0]}: " \
                         f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("M,K,T", SHAPES)
def test_one_hot_rows_recover_scale_times_weight(gpu, M, K, T):
    """x[t] = e_c: y[t][m] must be s[m][c / 64] * q[m][c], bit for bit, for every column c of every group (the columns
    in chunks of the shape's own T, so its tile and K split run)."""
    rng = np.random.default_rng(200000 * M + 10 * K + T)
    q, s = _weights(rng, M, K), _pow2_scales(rng, M, K // 64)
    want_all = (q.astype(np.float32) * np.repeat(s, 64, axis=1)).T  # [K][M], exact products
    for c0 in range(0, K, T):
        n = min(T, K - c0)
        x = np.zeros((T, K), np.float32)
        x[np.arange(n), c0 + np.arange(n)] = 1.0
        got = _run(gpu, x, q, s)
        want = np.zeros((T, M), np.float32)
        want[:n] = want_all[c0:c0 + n]
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert not len(bad), f"M {M} K {K} T {T}: column {c0 + int(bad[0][0])}, row {int(bad[0][1])}: " \
                             f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r} ({len(bad)} differ)"


@pytest.mark.parametrize("M,K,T", SHAPES)
def test_random_inputs_within_the_derived_bound(gpu, M, K, T):
    rng = np.random.default_rng(300000 * M + 10 * K + T)
    q = _weights(rng, M, K)
    s = (np.abs(rng.standard_normal((M, K // 64))) * 0.01 + 1e-4).astype(np.float32)
    x = rng.standard_normal((T, K), dtype=np.float32)
    g64, mag = ref.gold(x, q, s)
    lim = 4.0 * EPS * mag
    got = _run(gpu, x, q, s)
    e16 = np.abs(got.astype(np.float64) - g64)
    # the present int8 GEMV on the same inputs, one token at a time
    xd, qd, sd = torch.from_numpy(x).to(gpu), torch.from_numpy(q).to(gpu), torch.from_numpy(s).to(gpu)
    y8 = torch.empty((T, M), dtype=torch.float32, device=gpu)
    for t in range(T):
        ops.matmul_q8(xd[t], qd, sd, 64, y8[t])
    torch.cuda.synchronize()
    e8 = np.abs(y8.cpu().numpy().astype(np.float64) - g64)
    print(f"M {M} K {K} T {T}: worst |y - gold| / (2^-24 sum|sqx|): gemm_q8_bf16 {float((e16 / (EPS * mag)).max()):.3f}, "
          f"matmul_q8 {float((e8 / (EPS * mag)).max()):.3f} (bound 4)")
    assert np.all(e8 <= lim), "ops.matmul_q8 misses the bound: the inputs are not a fair yardstick"
    bad = np.argwhere(~(e16 <= lim))
    assert not len(bad), f"M {M} K {K} T {T}: {len(bad)} elements beyond the bound, first {bad[0]}: " \
                         f"{e16[tuple(bad[0])]:.3e} > {lim[tuple(bad[0])]:.3e}"


def test_ldy_beyond_m_keeps_the_columns_past_m(gpu):
    M, K, T, ldy = 32, 128, 17, 44
    rng = np.random.default_rng(5)
    x, q, s = _exact_case(rng, M, K, T)
    sent = (np.arange(T * ldy, dtype=np.float32).reshape(T, ldy) * 0.25 - 7.0)
    buf = torch.from_numpy(sent.copy()).to(gpu)
    assert buf.stride(0) == ldy
    got = _run(gpu, x, q, s, out=buf)
    want = ref.gold(x, q, s)[0].astype(np.float32)
    assert np.array_equal(got[:, :M].view(np.uint32), want.view(np.uint32))
    assert got[:, M:].tobytes() == sent[:, M:].tobytes()


def test_preconditions(gpu):
    def rc(T, M, K, ldy=None, x_off=0):
        x = torch.zeros((T * K + 4,), dtype=torch.float32, device=gpu)
        w = torch.zeros((M, K), dtype=torch.int8, device=gpu)
        s = torch.ones((M, max(K // 64, 1)), dtype=torch.float32, device=gpu)
        ldy = (M + 3) // 4 * 4 if ldy is None else ldy
        y = torch.zeros((T, max(ldy, 4)), dtype=torch.float32, device=gpu)
        return _ffi.lib().kh_gemm_q8_bf16_f32(x.data_ptr() + 4 * x_off, w.data_ptr(), s.data_ptr(), y.data_ptr(), T, M, K,
                                              ldy, None)
    assert rc(4, 24, 64) == _ffi.KH_ERR_UNSUPPORTED    # M % 16
    assert rc(4, 16, 96) == _ffi.KH_ERR_UNSUPPORTED    # K % 64
    assert rc(4, 16, 32) == _ffi.KH_ERR_UNSUPPORTED
    assert rc(513, 16, 64) == _ffi.KH_ERR_UNSUPPORTED  # T > 512
    assert rc(0, 16, 64) == _ffi.KH_ERR_INVALID_ARG
    assert rc(4, 16, 64, ldy=12) == _ffi.KH_ERR_INVALID_ARG   # ldy < M
    assert rc(4, 16, 64, ldy=18) == _ffi.KH_ERR_INVALID_ARG   # ldy % 4
    assert rc(4, 16, 64, x_off=1) == _ffi.KH_ERR_INVALID_ARG  # x not 16-byte aligned
    assert rc(512, 16, 64) == 0
