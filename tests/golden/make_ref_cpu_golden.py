"""Writes tests/golden/ref_cpu_backend.npz: what the reference's OWN CPU backend (oracle/_ref/ref_cpu_model*, built by
build() where the reference checkout exists) computes on the committed goldens, so that
tests/test_ref_cpu_backend.py can hold the oracle against it on a box without that build.

Per golden <name>:  <name>__logits  float32 [T, V]  teacher-forced over the golden's T tokens
                    <name>__words   int32   [S]     greedy run of S = min(24, seq_len) steps from prompt PROMPT

    python tests/golden/make_ref_cpu_golden.py      (after build(), in the build container)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/: conftest + the test module's runner

from conftest import load_golden  # noqa: E402
from test_ref_cpu_backend import GOLDEN_NAMES, GREEDY_PROMPT, REF_CPU_GOLDEN, greedy_steps, run_ref_cpu  # noqa: E402


def main():
    out = {}
    for name in GOLDEN_NAMES:
        spec, img, toks, _ = load_golden(name)
        toks = [int(t) for t in toks]
        _, lg, _ = run_ref_cpu(spec, img, len(toks), toks, want_logits=True, threads=2)
        words, _, _ = run_ref_cpu(spec, img, greedy_steps(spec), GREEDY_PROMPT, threads=2)
        out[name + "__logits"] = lg.astype(np.float32)
        out[name + "__words"] = np.asarray(words, dtype=np.int32)
    np.savez_compressed(REF_CPU_GOLDEN, **out)
    print(REF_CPU_GOLDEN, sorted(out))


if __name__ == "__main__":
    main()
