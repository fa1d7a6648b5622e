"""The three-term bf16 split of csrc/kh_gemm_w16.h (pg_split3), stated in numpy.

    hi  = x & 0xffff0000
    mid = (x - hi) & 0xffff0000
    lo  = x - hi - mid

All arithmetic is fp32; both subtractions are exact (x - hi holds the lower 16 significand bits of x, x - hi - mid the
lowest 8), so hi + mid + lo == x for every finite x, and each part is a bf16 value - its low 16 bits are zero - unless
lo falls into the fp32 subnormals.  The kernel packs the UPPER halves of the three parts into its MFMA operands.
"""
import numpy as np

_MASK = np.uint32(0xFFFF0000)


def trunc16(x):
    """x with the low 16 bits of every fp32 word cleared."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & _MASK).view(np.float32)


def split3(x):
    """(hi, mid, lo) as fp32 arrays, computed as the kernel does."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = trunc16(x)
    r = x - hi
    mid = trunc16(r)
    lo = r - mid
    return hi, mid, lo


def packed_upper_halves(x):
    """The three bf16 operands the kernel feeds: uint16 upper halves of hi, mid, lo."""
    return tuple((p.view(np.uint32) >> np.uint32(16)).astype(np.uint16) for p in split3(x))


def is_bf16(x):
    """Elementwise: is the fp32 value a bf16 value (low 16 bits zero)?"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF)) == 0


def bf16_bits(w):
    """uint16 bf16 fields of bf16-exact fp32 values."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert is_bf16(w).all()
    return (w.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
