"""Cost of per-sequence constrained decoding (csrc/kh_seq.h: k_seq_tail_fsm) on the GPU: same-box A/B against the parent
commit.

Medians of alternated runs of generate_batch at Llama-3.2-1B geometry (synthetic image), 128 steps: 8 sequences on the
8-lane pass and 64 sequences on the wide pass (gemm=True).  The baseline is the PARENT commit's tree, greedy, nothing
set: its passes end in k_seq_pick.  Against it, this tree with
  (a) no sequence constraint   - must lie inside the parent's run-to-run range: the off path is untouched
  (t) a one-entry logit bias per sequence, no constraint: the passes end in k_seq_tail, the tail the twin extends
  (b) a 6-state automaton whose rows hold V/8 ids, every slot at state 0: k_seq_tail_fsm
  (c) the same with rows of V ids: nothing is masked, the transition walks the longest row there is

    python tools/seq_constraint_ab.py --parent-tree DIR [--rounds 5] [--out profiles/seq_constraint_ab.txt]

DIR is a checkout of the parent commit with its library built (python -m kuiperllama_amd.build inside it).  Every round
starts one process per tree, parent first, so the two alternate on one box; a process reports the median of three runs
per mode, modes interleaved.  Times are the library's own (HIP events around the passes).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (("8 sequences, 8-lane pass", 8, False), ("64 sequences, wide pass", 64, True))
STEPS = 128

# runs in either tree: only what both have, plus seq_set_constraint where the tree has it
_WORKER = r"""
import json, sys
import numpy as np, torch
from kuiperllama_amd import binfmt
from kuiperllama_amd.model import KuiperModel
modes, steps = sys.argv[1].split(","), int(sys.argv[2])
spec = binfmt.PRESETS["llama3.2-1b"]
V = spec.vocab_size
img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
torch.cuda.synchronize()
m = KuiperModel.from_device_image(img, spec, max_seq_len=64 * (steps + 32))
auto = {}
if "b" in modes or "c" in modes:
    from kuiperllama_amd.constraint import TokenAutomaton
    rng = np.random.default_rng(7)
    for mode, k in (("b", V // 8), ("c", V)):
        rows = [np.sort(rng.choice(V, k, replace=False)).astype(np.int32) for _ in range(6)]
        auto[mode] = TokenAutomaton(0, np.arange(7) * k, np.concatenate(rows), rng.integers(0, 6, 6 * k))
def run(mode, n, gemm):
    kw = {}
    if auto:
        m.seq_set_constraint(auto.get(mode))
        if mode in auto:
            for s in range(n):
                m.seq_set_constraint_state(s, 0)
    if mode == "t":
        kw["logit_bias"] = [{5: -1.0}] * n
    return m.generate_batch([[1, 263]] * n, steps, gemm=gemm, **kw)[1]
res = {}
for label, n, gemm in json.loads(sys.argv[3]):
    m.seq_slots(n)
    out = {mode: [] for mode in modes}
    for mode in modes:
        for _ in range(2):
            run(mode, n, gemm)
    for _ in range(3):
        for mode in modes:
            out[mode].append(run(mode, n, gemm))
    res[label] = {k: float(np.median(v)) for k, v in out.items()}
print("AB " + json.dumps(res))
"""


def run(tree, modes):
    r = subprocess.run([sys.executable, "-c", _WORKER, ",".join(modes), str(STEPS), json.dumps(CONFIGS)], cwd=tree,
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=tree), timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("AB "))
    return json.loads(line[3:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("seq_constraint_ab: no GPU (timings are taken on the GPU or not at all)")
    lines = [f"# per-sequence constrained decoding: {STEPS}-step generate_batch at Llama-3.2-1B geometry, ms per run",
             "# (HIP events around the passes); greedy, prompts of 2 tokens",
             f"# median [min .. max] over {a.rounds} alternated rounds; each round: median of 3 runs per mode",
             f"# device: {torch.cuda.get_device_name(0)}"]
    keys = ("parent", "a", "t", "b", "c")
    got = {label: {k: [] for k in keys} for label, _, _ in CONFIGS}
    for rnd in range(a.rounds):
        p = run(os.path.abspath(a.parent_tree), ["parent"])
        r = run(ROOT, ["a", "t", "b", "c"])
        for label, _, _ in CONFIGS:
            got[label]["parent"].append(p[label]["parent"])
            for k in keys[1:]:
                got[label][k].append(r[label][k])
            print(f"# {label} round {rnd + 1}: " + " ".join(f"{k}={got[label][k][-1]:.3f}" for k in keys), flush=True)
    labels = {"parent": "parent commit, nothing set (k_seq_pick)", "a": "(a) this commit, no constraint (k_seq_pick)",
              "t": "(t) one-entry bias, no constraint (k_seq_tail)", "b": "(b) 6 states, rows of V/8 ids (k_seq_tail_fsm)",
              "c": "(c) 6 states, rows of V ids (k_seq_tail_fsm)"}
    for label, n, _ in CONFIGS:
        g = got[label]
        base = float(np.median(g["parent"]))
        lines.append(f"## {label}")
        for k in keys:
            v = g[k]
            med = float(np.median(v))
            lines.append(f"{labels[k]:50s} {med:9.3f} [{min(v):9.3f} .. {max(v):9.3f}]  {100 * (med / base - 1):+6.2f} %"
                         f"  {1e3 * (med - base) / STEPS:+8.2f} us/pass-step  {1e3 * n * STEPS / med:9.0f} tok/s")
        inside = min(g["parent"]) <= float(np.median(g["a"])) <= max(g["parent"])
        lines.append(f"(a) inside the parent's range: {'yes' if inside else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
