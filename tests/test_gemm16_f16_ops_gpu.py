"""ops.gemm_h16 (kh_gemm_h16_f32): the K loop of KH_FLAG_GEMM16_F16 (csrc/kh_gemm_h16.h) under its STORE epilogue, on
inputs a model never produces.  One-hot rows (one product per output, exact in any order of its six terms), integers
(every partial sum below 2^23) and a general case against the fp32 GEMV's error.  M with and without a 32-row tile;
T = 1, 17, 100 leave padding tokens; K = 32 and 96 lie below the ring depth, K = 160 gives 5 blocks (past the deepest
ring, with a remainder), K = 1024 four K waves."""
import numpy as np
import pytest
import torch

import gemm16_cases as g16
from kuiperllama_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(32, 48), (32, 64), (96, 96), (160, 112), (1024, 1024), (1024, 1040)]
TOKENS = [1, 16, 17, 100]


def _run(gpu, x, w):
    h = w.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), w)  # w is fp16-exact
    y = ops.gemm_h16(torch.from_numpy(x).to(gpu), torch.from_numpy(h.view(np.int16)).to(gpu))
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("K,M", SHAPES)
@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("kind", ["powers of two", "full significands"])
def test_one_hot_rows_are_bit_exact(gpu, kind, K, M, T):
    rng = np.random.default_rng(1000 * K + 10 * M + T)
    if kind == "powers of two":  # +-2^e over fp16's whole range (w_lo = 0) against full 24-bit x
        x = g16.x_values(rng, T, K)  # +-0 and +-FLT_MAX in columns 0 .. 3
        m = np.ones(M)
        e = (np.arange(M) * 7 + T) % 40 - 24  # -24 .. 15, subnormals included; every value where M >= 40
        big = np.isin(np.arange(M) % K, (2, 3))
        e[big] = -np.abs(e[big])  # the largest finite value stays finite
    else:  # odd 11-bit significands (w_lo != 0) against x of at most 12 significant bits: the product fits 24 bits
        k = rng.integers(1, 1 << 12, (T, K)).astype(np.float64)
        x = (rng.choice([-1.0, 1.0], (T, K)) * k * np.exp2(rng.integers(-30, 31, (T, K)))).astype(np.float32)
        x[0::2, 0], x[1::2, 1] = np.float32(0.0), np.float32(-0.0)
        m = (rng.integers(512, 1024, M) * 2 + 1).astype(np.float64)
        e = (np.arange(M) * 7 + T) % 30 - 24  # -24 .. 5: fp16's normal range for an 11-bit significand
    g16.one_hot(_run, gpu, x, (rng.choice([-1.0, 1.0], M) * m * np.exp2(e)).astype(np.float32), K, f"{kind} K {K} M {M} T {T}")


@pytest.mark.parametrize("M", [64, 80])
def test_integers_equal_the_int64_product(gpu, M):
    rng = np.random.default_rng(77 + M)
    T, K = 100, 256
    xi = rng.integers(-31, 32, (T, K))
    wi = rng.integers(-1023, 1024, (M, K))
    assert (np.abs(xi).astype(np.int64) @ np.abs(wi).astype(np.int64).T).max() < 1 << 23  # every partial sum
    got = _run(gpu, xi.astype(np.float32), wi.astype(np.float32))
    want = xi.astype(np.int64) @ wi.astype(np.int64).T
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


def test_general_within_twice_the_fp32_gemv_error(gpu):
    g16.general_case(g16.H16, _run, gpu, lambda w: w.astype(np.float16).astype(np.float32))


def test_preconditions(gpu):
    g16.preconditions(g16.H16, gpu)
