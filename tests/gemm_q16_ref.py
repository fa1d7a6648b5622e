"""The arithmetic of csrc/kh_gemm_q16.h (pg_kloop_q16), stated in numpy.

One group of 64 columns of an int8 group-64 matrix row, scale s, against one token's activations x:

    t_step = sum over the step's 32 columns of q * (hi + mid + lo)      exact bf16 x bf16 products, fp32 accumulation
    acc    = fma(s, t_step, acc)                                         step 0, then step 1

  * an int8 value q becomes the bf16 operand by int8 -> fp32 -> upper 16 bits: exact for all 256 values;
  * lane (i = l & 15, h = l >> 4) holds bytes 16h .. 16h + 15 of the group; MFMA step s contracts, at k index 8h + e,
    the lane's byte 8s + e - column 16h + 8s + e of the group - with the activation the B operand holds at the same k
    index: element e of quarters 2s and 2s + 1 of the int8 tiled slab (pg_tiled_index(true, ...)) at lane quarter h;
  * (hi, mid, lo) is split3_ref.split3(x).
"""
import numpy as np


def int8_to_bf16_bits(q):
    """uint16 bf16 fields the kernel makes of int8 values: the upper halves of float32(q)."""
    f = np.ascontiguousarray(q, dtype=np.int8).astype(np.float32)
    return (f.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_bits_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def a_columns(step):
    """[64 lanes][8]: the group column whose weight lane l feeds at element e of MFMA step `step` (its k index is
    8 * (l >> 4) + e)."""
    lane = np.arange(64)
    h = lane >> 4
    return (16 * h + 8 * step)[:, None] + np.arange(8)[None, :]


def tiled_index_q8(k, t, tcap):
    """csrc/kh_gemm.h::pg_tiled_index(true, k, t, tcap): position (in floats) of activation (token t, column k)."""
    b, r = k >> 6, k & 63
    h, q, e = r >> 4, (r >> 2) & 3, r & 3
    return (((b * 4 + q) * tcap + t) * 4 + h) * 4 + e


def b_columns(step, tcap=128, token=5, block=3):
    """[64 lanes][8]: the group column of the activation lane l feeds at element e of step `step`, read back from the
    tiled slab: the lane loads float4s at quarters 2 * step and 2 * step + 1, lane quarter h (the kernel's addressing:
    base + (token * 16 + 4 h) + block * 4 * tcap * 16 + quarter * tcap * 16)."""
    where = {int(tiled_index_q8(64 * block + c, token, tcap)): c for c in range(64)}
    out = np.zeros((64, 8), np.int64)
    for lane in range(64):
        h = lane >> 4
        for half in range(2):
            quarter = 2 * step + half
            at = token * 16 + 4 * h + block * 4 * tcap * 16 + quarter * tcap * 16
            for e in range(4):
                out[lane, 4 * half + e] = where[at + e]
    return out


def gold(x, q, scales):
    """fp64 statement of y[t][m] = sum_g s[m][g] * sum_{k in g} q[m][k] * x[t][k]  and  sum |s q x| (the error scale)."""
    x64 = np.asarray(x, np.float64)
    w64 = np.asarray(q, np.float64) * np.repeat(np.asarray(scales, np.float64), 64, axis=1)
    return x64 @ w64.T, np.abs(x64) @ np.abs(w64).T

