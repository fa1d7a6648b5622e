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

import gemm16_cases as g16
import split3_ref as s3
from kuiperllama_amd import ops

pytestmark = pytest.mark.gpu


def _run(gpu, x, w):
    y = ops.gemm_w16(torch.from_numpy(x).to(gpu),
                     torch.from_numpy(s3.bf16_bits(w).view(np.int16)).to(gpu))
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("K,M", [(32, 48), (32, 64), (96, 96), (96, 112), (1024, 1024), (1024, 1040)])
@pytest.mark.parametrize("T", [1, 16, 17, 100])
def test_one_hot_rows_are_bit_exact(gpu, K, M, T):
    rng = np.random.default_rng(1000 * K + 10 * M + T)
    x = g16.x_values(rng, T, K)
    col = np.arange(M) % K
    e = rng.integers(-8, 9, M)
    e[np.isin(col, (2, 3))] = -np.abs(e[np.isin(col, (2, 3))])  # the largest finite value stays finite
    g16.one_hot(_run, gpu, x, (rng.choice([-1.0, 1.0], M) * np.exp2(e)).astype(np.float32), K, f"K {K} M {M} T {T}")


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
    g16.general_case(g16.W16, _run, gpu, s3.trunc16)


def test_preconditions(gpu):
    g16.preconditions(g16.W16, gpu)
