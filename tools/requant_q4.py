#!/usr/bin/env python3
"""Requantise the matrices of an int8 KuiperLLama .bin to 4 bits per value, keeping the int8 format:

    python tools/requant_q4.py in.bin out.bin

The output is an ordinary int8 checkpoint (same header, tensor table, layout and group size) whose quantised values all
lie in [-7, 7], so KH_FLAG_Q4 / `kuiper_demo --q4` decodes it from a packed 4-bit copy (binfmt.requantize_matrices_q4:
per group s' = max|q * s| / 7, q' = round(q * s / s')).  This changes the model: its quality at 4 bits is the user's to
judge.  The library itself never rounds a weight.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from kuiperllama_amd import binfmt  # noqa: E402


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    img = np.fromfile(argv[1], dtype=np.uint8)
    spec = binfmt.spec_from_image(img, quant=True)
    need = binfmt.image_nbytes(spec)
    if img.size < need:
        print(f"{argv[1]}: {img.size} bytes, an int8 image of this header has {need}", file=sys.stderr)
        return 1
    binfmt.requantize_matrices_q4(img, spec)
    assert binfmt.matrices_q4_exact(img, spec)
    img.tofile(argv[2])
    print(f"{argv[2]}: {len(binfmt.q4_tensors(spec))} matrices requantised, group size {spec.group_size}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
