"""Cost of constrained decoding (csrc/kh_fsm.h, k_sample_proc_fsm) on the GPU: same-box A/B against the parent commit.

Medians of alternated runs of a 128-step generate(exec="graph") on synthetic images of two geometries.  The baseline is
the PARENT commit's tree with a one-entry logit bias, which puts it on the tail the constraint extends, k_sample_proc.
Against it, this tree with the same bias and
  (a) no constraint            - must lie inside the parent's run-to-run range: the off path is untouched
  (b) a 6-state automaton whose rows hold V/8 ids
  (c) the same with rows of V ids: nothing is masked, the lookup walks the longest row there is

    python tools/constraint_ab.py --parent-tree DIR [--rounds 5] [--out profiles/constraint_ab.txt]

DIR is a checkout of the parent commit with its library built (python -m kuiperllama_amd.build inside it).  Every round
starts one process per tree, parent first, so the two alternate on one box; a process reports the median of three runs
per mode, modes interleaved.  Times are the library's own (HIP events around the step loop).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESETS = ("llama3.2-1b", "llama2-7b-int8")

# runs in either tree: only what both have, plus set_constraint where the tree has it
_WORKER = r"""
import json, sys
import numpy as np, torch
from kuiperllama_amd import binfmt
from kuiperllama_amd.model import KuiperModel
name, modes = sys.argv[1], sys.argv[2].split(",")
spec = binfmt.PRESETS[name]
V = spec.vocab_size
img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
torch.cuda.synchronize()
m = KuiperModel.from_device_image(img, spec, max_seq_len=256)
m.set_logit_bias({5: -1.0})
auto = {}
if "b" in modes or "c" in modes:
    from kuiperllama_amd.constraint import TokenAutomaton
    rng = np.random.default_rng(7)
    for mode, k in (("b", V // 8), ("c", V)):
        rows = [np.sort(rng.choice(V, k, replace=False)).astype(np.int32) for _ in range(6)]
        auto[mode] = TokenAutomaton(0, np.arange(7) * k, np.concatenate(rows), rng.integers(0, 6, 6 * k))
def arm(mode):
    if mode in auto:
        m.set_constraint(auto[mode])
    elif auto:
        m.set_constraint(None)
out = {mode: [] for mode in modes}
for mode in modes:
    arm(mode)
    for _ in range(2):
        m.generate([1, 263], 128, exec="graph")
for _ in range(3):
    for mode in modes:
        arm(mode)
        out[mode].append(m.generate([1, 263], 128, exec="graph")[1])
print("AB " + json.dumps({k: float(np.median(v)) for k, v in out.items()}))
"""


def run(tree, name, modes):
    r = subprocess.run([sys.executable, "-c", _WORKER, name, ",".join(modes)], cwd=tree, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=tree), timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("AB "))
    return json.loads(line[3:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--presets", default=",".join(PRESETS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("constraint_ab: no GPU (timings are taken on the GPU or not at all)")
    lines = ["# constrained decoding: 128-step generate(exec=graph), ms per run (HIP events around the step loop)",
             f"# median [min .. max] over {a.rounds} alternated rounds; each round: median of 3 runs per mode",
             f"# device: {torch.cuda.get_device_name(0)}"]
    for name in a.presets.split(","):
        got = {"parent": [], "a": [], "b": [], "c": []}
        for _ in range(a.rounds):
            got["parent"].append(run(os.path.abspath(a.parent_tree), name, ["parent"])["parent"])
            r = run(ROOT, name, ["a", "b", "c"])
            for k in "abc":
                got[k].append(r[k])
            print(f"# {name} round {len(got['a'])}: " + " ".join(f"{k}={got[k][-1]:.3f}" for k in got), flush=True)
        base = float(np.median(got["parent"]))
        lines.append(f"## {name}")
        labels = {"parent": "parent commit, one-entry bias", "a": "(a) this commit, no constraint, same bias",
                  "b": "(b) 6 states, rows of V/8 ids", "c": "(c) 6 states, rows of V ids"}
        for k in ("parent", "a", "b", "c"):
            v = got[k]
            med = float(np.median(v))
            lines.append(f"{labels[k]:44s} {med:8.3f} [{min(v):8.3f} .. {max(v):8.3f}]  {100 * (med / base - 1):+6.2f} %"
                         f"  {1e3 * (med - base) / 128:+7.2f} us/token")
        inside = min(got["parent"]) <= float(np.median(got["a"])) <= max(got["parent"])
        lines.append(f"(a) inside the parent's range: {'yes' if inside else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
