"""ops.gemm_w16 (kh_gemm_w16_f32): the K loop of KH_FLAG_GEMM16 (csrc/kh_gemm_w16.h) under its STORE epilogue, on inputs
a model never produces - so the lane maps of v_mfma_f32_16x16x32_bf16, the packing of the three bf16 terms and the
K partition are checked exactly, without a tolerance:

  one-hot rows   row r of W holds a single +-2^e at column r mod K: y[t][r] is ONE product w * x[t][r mod K], and its
                 three terms w * hi, w * mid, w * lo add up exactly in any order - so y must be that product bit for
                 bit.  A k position paired with the wrong partner, a dropped or doubled term, or a row / token in the
                 wrong accumulator register all change bits.  "The product" is the dot product's value: accumulators
                 start at +0, so x = -0 gives +0 + (-0 * w) = +0.
  integers       |x| < 2^11, |w| <= 16, K = 256: every partial sum is an integer below 2^24 - y equals the int64
                 product whatever the summation order.
  general        random bf16-rounded W, random x against an fp64 matmul: within twice the error of the fp32 GEMV
                 (kh_matmul_f32, row by row) on the same operands, plus one ulp of the largest |y|.

Sizes: M with and without a 32-row tile (R = 2 / R = 1), T = 1, 17, 100 leave padding tokens and T = 100 takes several
token slices; K = 32 and 96 give a wave 1 and 3 blocks (below the ring depth), K = 256 two waves, K = 1024 four.
"""
import numpy as np
import pytest
import torch

import split3_ref as s3
from kuiperllama_amd import _ffi, ops

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
SPECIAL = {0: 0.0, 1: -0.0, 2: FMAX, 3: -FMAX}  # column -> value, on every other token


def _x_values(rng, T, K):
    m = rng.integers(1 << 23, 1 << 24, (T, K)).astype(np.float64)  # full 24-bit significands
    e = rng.integers(-30, 31, (T, K)).astype(np.float64)
    x = (rng.choice([-1.0, 1.0], (T, K)) * m * np.exp2(e - 23)).astype(np.float32)
    for c, v in SPECIAL.items():
        x[(c & 1)::2, c] = np.float32(v)
    return x


def _run(gpu, x, w):
    y = ops.gemm_w16(torch.from_numpy(x).to(gpu),
                     torch.from_numpy(s3.bf16_bits(w).view(np.int16)).to(gpu))
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("K,M", [(32, 48), (32, 64), (96, 96), (96, 112), (1024, 1024), (1024, 1040)])
@pytest.mark.parametrize("T", [1, 16, 17, 100])
def test_one_hot_rows_are_bit_exact(gpu, K, M, T):
    rng = np.random.default_rng(1000 * K + 10 * M + T)
    x = _x_values(rng, T, K)
    col = np.arange(M) % K
    e = rng.integers(-8, 9, M)
    e[np.isin(col, (2, 3))] = -np.abs(e[np.isin(col, (2, 3))])  # the largest finite value stays finite
    wv = (rng.choice([-1.0, 1.0], M) * np.exp2(e)).astype(np.float32)
    w = np.zeros((M, K), np.float32)
    w[np.arange(M), col] = wv
    got = _run(gpu, x, w)
    want = np.float32(0) + x[:, col] * wv[None, :]  # one exact product per element, added to +0
    assert np.isfinite(want).all()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), f"K {K} M {M} T {T}: {len(bad)} of {got.size} differ, first (token, row) {bad[0]}: " \
                         f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("M", [64, 80])
def test_integers_equal_the_int64_product(gpu, M):
    rng = np.random.default_rng(77 + M)
    T, K = 100, 256
    xi = rng.integers(-(1 << 11) + 1, 1 << 11, (T, K))
    wi = rng.integers(-16, 17, (M, K))
    got = _run(gpu, xi.astype(np.float32), wi.astype(np.float32))
    want = (xi.astype(np.int64) @ wi.astype(np.int64).T)
    assert np.abs(want).max() < 1 << 24
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


def test_general_within_twice_the_fp32_gemv_error(gpu):
    rng = np.random.default_rng(99)
    T, K, M = 64, 1024, 128
    w = s3.trunc16(rng.standard_normal((M, K), dtype=np.float32) * np.float32(0.05))
    x = rng.standard_normal((T, K), dtype=np.float32)
    y64 = x.astype(np.float64) @ w.astype(np.float64).T
    got = _run(gpu, x, w)
    xd, wd = torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu)
    y32 = torch.empty((T, M), dtype=torch.float32, device=gpu)
    for t in range(T):  # the fp32 yardstick: the GEMV kernel of kh_matmul_f32, one row of x at a time
        ops.matmul(xd[t], wd, y32[t])
    torch.cuda.synchronize()
    e16 = float(np.abs(got - y64).max())
    e32 = float(np.abs(y32.cpu().numpy() - y64).max())
    ulp = float(np.spacing(np.float32(np.abs(y64).max())))
    print(f"gemm_w16 vs fp64: {e16:.3e}; kh_matmul_f32 vs fp64: {e32:.3e}; 1 ulp of max |y|: {ulp:.3e}")
    assert e16 <= 2.0 * e32 + ulp


def test_preconditions(gpu):
    def rc(T, M, K):
        x = torch.zeros((T, K), dtype=torch.float32, device=gpu)
        w = torch.zeros((M, K), dtype=torch.int16, device=gpu)
        y = torch.zeros((T, (M + 3) // 4 * 4), dtype=torch.float32, device=gpu)
        return _ffi.lib().kh_gemm_w16_f32(x.data_ptr(), w.data_ptr(), y.data_ptr(), T, M, K, y.stride(0), None)
    assert rc(4, 24, 32) == _ffi.KH_ERR_UNSUPPORTED   # M % 16
    assert rc(4, 16, 48) == _ffi.KH_ERR_UNSUPPORTED   # K % 32
    assert rc(513, 16, 32) == _ffi.KH_ERR_UNSUPPORTED  # T > 512
    assert rc(512, 16, 32) == 0
