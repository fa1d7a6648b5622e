"""Cost of per-token log-probabilities (csrc/kh_logprobs.h, k_sample_lp) on the GPU.

    python tools/logprobs_time.py [--out profiles/logprobs_cost.txt] [--preset llama3.2-1b] [--parent-tree DIR]

1. Operator: kh_logprobs_f32 alone (one row: one 1024-thread workgroup, its own maximum pass included) at V = 32000,
   128256 and 151936 with N = 0, 5 and 20, on normal(0, 2) logits.  Average of back-to-back launches captured in a torch
   CUDA graph, between two events.
2. Model, seeded synthetic image of the preset: the decode step at position 64 replayed as a 1-step hipGraph
   (kh_model_time_step, median of 31: always the full classifier), the us per token of a 128-step graph-mode generate
   (best of 4: greedy runs without processors or log-probs screen the classifier) and the step's last launch alone, for
   greedy, sampled (T 0.8, K 50) and processors on (repetition 1.3, presence 0.5, frequency 0.2, last_n 64, two bias
   entries), each with log-probs off and on (N = 5; N = 20 for the greedy pick as well).
   --parent-tree DIR: a built checkout of the parent commit; its figures for the three picks are taken twice, before
   and after this tree's, each in a process of its own that imports the package from DIR, on the same box: the two runs
   give the spread that "log-probs off" is held against.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMP = dict(temperature=0.8, top_k=50, top_p=1.0, seed=1)
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2, last_n=64)
BIAS = {5: -1.0, 77: 0.5}
PICKS = (("greedy", None, False), ("sampled", SAMP, False), ("processors", None, True))

# the three picks through the entry points the parent commit has; prints one JSON line
_BASELINE = r"""
import json, sys
import numpy as np, torch
from kuiperllama_amd import binfmt
from kuiperllama_amd.model import KuiperModel
spec = binfmt.PRESETS[sys.argv[1]]
img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
torch.cuda.synchronize()
m = KuiperModel.from_device_image(img, spec, max_seq_len=256)
out = {}
for label, samp, proc in (("greedy", None, False), ("sampled", dict(temperature=0.8, top_k=50, top_p=1.0, seed=1), False),
                          ("processors", None, True)):
    m.set_sampling(**samp) if samp else m.set_sampling()
    m.set_penalties(repetition=1.3, presence=0.5, frequency=0.2, last_n=64) if proc else m.set_penalties()
    m.set_logit_bias({5: -1.0, 77: 0.5} if proc else None)
    m.generate([1, 263], 72, exec="graph")
    step = float(np.median(m.time_step(64, 31)))
    gen = min(m.generate([1, 263], 128, exec="graph")[1] for _ in range(4)) * 1e3 / 128
    out[label] = [step, gen]
m.close()
print("BASELINE " + json.dumps(out))
"""


def baseline(tree, preset):
    r = subprocess.run([sys.executable, "-c", _BASELINE, preset], cwd=tree, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=tree), timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("BASELINE "))
    return json.loads(line[len("BASELINE "):])


def _graph_us(fn, reps=100):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()  # warm
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(5):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(best))


def operator_rows():
    from kuiperllama_amd import _ffi
    dev = torch.device("cuda:0")
    rows = []
    for V in (32000, 128256, 151936):
        rng = np.random.default_rng(V)
        lg = torch.from_numpy(rng.normal(0.0, 2.0, V).astype(np.float32)).to(dev)
        ids = torch.tensor([V // 2], dtype=torch.int32, device=dev)
        lse = torch.empty(1, dtype=torch.float32, device=dev)
        lp = torch.empty(1, dtype=torch.float32, device=dev)
        tid = torch.empty(20, dtype=torch.int32, device=dev)
        tlp = torch.empty(20, dtype=torch.float32, device=dev)
        for N in (0, 5, 20):
            def call():  # preallocated outputs: the graph holds nothing but the kernel
                _ffi.check(_ffi.lib().kh_logprobs_f32(lg.data_ptr(), V, 1, ids.data_ptr(), N, lse.data_ptr(),
                                                      lp.data_ptr(), tid.data_ptr(), tlp.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "kh_logprobs_f32")
            rows.append((V, N, _graph_us(call)))
    return rows


def model_rows(preset, pos=64):
    from kuiperllama_amd import binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS[preset]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec, max_seq_len=256)
    rows = []
    for pick, samp, proc in PICKS:
        for top_n in (None, 5, 20) if pick == "greedy" else (None, 5):
            m.set_sampling(**samp) if samp else m.set_sampling()
            m.set_penalties(**PEN) if proc else m.set_penalties()
            m.set_logit_bias(BIAS if proc else None)
            m.set_logprobs(top_n)
            m.generate([1, 263], pos + 8, exec="graph")  # captures this tail's graphs, fills rows and records
            step = float(np.median(m.time_step(pos, 31)))
            tail = m.profile_kernel("sample", pos, reps=50)
            gen = min(m.generate([1, 263], 128, exec="graph")[1] for _ in range(4)) * 1e3 / 128
            rows.append((pick, "off" if top_n is None else f"on, N {top_n}", step, gen, tail))
    m.close()
    return spec.vocab_size, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprobs_cost.txt"))
    ap.add_argument("--preset", default="llama3.2-1b")
    ap.add_argument("--parent-tree", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    lines = ["# tools/logprobs_time.py: cost of per-token log-probabilities on one MI355X (gfx950)", "",
             "## operator alone: kh_logprobs_f32, one row, back-to-back launches in a graph (us per launch)",
             f"{'V':>7} {'N':>3} {'us':>8}"]
    for V, N, us in operator_rows():
        lines.append(f"{V:>7} {N:>3} {us:8.2f}")
        print(lines[-1], flush=True)
    base = [baseline(a.parent_tree, a.preset)] if a.parent_tree else []
    V, rows = model_rows(a.preset)
    if a.parent_tree:
        base.append(baseline(a.parent_tree, a.preset))
    lines += ["", f"## model {a.preset} (V = {V}, synthetic weights): 1-step hipGraph at position 64 (median of 31, full",
              "## classifier), us per token of a 128-step graph-mode generate (best of 4; a greedy run without processors or",
              "## log-probs screens the classifier), last launch alone",
              f"{'pick':<11} {'log-probs':<14} {'step us':>8} {'generate us/tok':>15} {'last launch us':>14}"]
    for i, b in enumerate(base):
        for pick, (step, gen) in b.items():
            lines.append(f"{pick:<11} {'parent run ' + str(i + 1):<14} {step:8.1f} {gen:15.1f}")
            print(lines[-1], flush=True)
    for pick, lp, step, gen, tail in rows:
        lines.append(f"{pick:<11} {lp:<14} {step:8.1f} {gen:15.1f} {tail:14.2f}")
        print(lines[-1], flush=True)
    if len(base) == 2:
        lines += ["", "## log-probs off against the parent commit (us; spread = |parent run 1 - parent run 2|)",
                  f"{'pick':<11} {'step: parent':>13} {'spread':>7} {'off':>8} {'generate: parent':>17} {'spread':>7} {'off':>8}"]
        off = {pick: (step, gen) for pick, lp, step, gen, _ in rows if lp == "off"}
        for pick in off:
            (s1, g1), (s2, g2) = base[0][pick], base[1][pick]
            lines.append(f"{pick:<11} {(s1 + s2) / 2:13.1f} {abs(s1 - s2):7.1f} {off[pick][0]:8.1f} "
                         f"{(g1 + g2) / 2:17.1f} {abs(g1 - g2):7.1f} {off[pick][1]:8.1f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
