"""Cost of the logit processors (csrc/kh_logit_proc.h, k_sample_proc) on the GPU.

    python tools/logit_proc_time.py [--out profiles/logit_proc_cost.txt] [--presets llama3.2-1b,qwen2.5-0.5b]
                                    [--parent-tree DIR]

1. Operator: kh_logit_process_f32 alone at V = 128256 on windows of 64, 4096 and 131072 positions (random tokens, all
   three penalties and two bias entries).  Average of back-to-back launches captured in a torch CUDA graph, between
   two events.
2. Model, seeded synthetic images of the presets: the decode step at position 64 replayed as a 1-step hipGraph
   (kh_model_time_step, median of 31: always the full classifier) and the us per token of a 128-step graph-mode
   generate (best of 3: greedy runs without processors screen the classifier), greedy and sampled (T 0.8, K 50), with
   processors off and on (repetition 1.3, presence 0.5, frequency 0.2; last_n 64 and 0).
   --parent-tree DIR: a built checkout of the parent commit; its greedy and sampled figures are taken in a process
   of their own that imports the package from DIR, on the same box, and the differences are stated against them.
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
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2)

# greedy and sampled steps through the entry points every version of the package has; prints one JSON line
_BASELINE = r"""
import json, sys
import numpy as np, torch
from kuiperllama_amd import binfmt
from kuiperllama_amd.model import KuiperModel
out = {}
for name in sys.argv[1].split(","):
    spec = binfmt.PRESETS[name]
    img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec, max_seq_len=256)
    for label, p in (("greedy", None), ("sampled", dict(temperature=0.8, top_k=50, top_p=1.0, seed=1))):
        m.set_sampling(**p) if p else m.set_sampling()
        m.generate([1, 263], 72, exec="graph")
        step = float(np.median(m.time_step(64, 31)))
        gen = min(m.generate([1, 263], 128, exec="graph")[1] for _ in range(4)) * 1e3 / 128
        out[name + " " + label] = [step, gen]
    m.close()
    del img
    torch.cuda.empty_cache()
print("BASELINE " + json.dumps(out))
"""


def baseline(tree, presets):
    r = subprocess.run([sys.executable, "-c", _BASELINE, ",".join(presets)], cwd=tree, capture_output=True, text=True,
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


def operator_rows(V=128256):
    from kuiperllama_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(V)
    lg = torch.from_numpy(rng.normal(0.0, 2.0, V).astype(np.float32)).to(dev)
    ws = ops.logit_process_workspace(V, dev)
    ids = torch.tensor([5, 77], dtype=torch.int32, device=dev)
    val = torch.tensor([-1.0, 0.5], dtype=torch.float32, device=dev)
    rows = []
    for W in (64, 4096, 131072):
        hist = torch.from_numpy(rng.integers(0, V, W).astype(np.int32)).to(dev)
        pen = dict(PEN, last_n=0)
        rows.append((V, W, _graph_us(lambda: ops.logit_process(lg, hist, W - 1, pen, ids, val, ws))))
    return rows


def model_rows(presets, pos=64):
    from kuiperllama_amd import binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    rows = []
    for name in presets:
        spec = binfmt.PRESETS[name]
        img = binfmt.synth_image(spec, seed=1234, device=dev)
        torch.cuda.synchronize()
        m = KuiperModel.from_device_image(img, spec, max_seq_len=256)
        for samp_label, samp in (("greedy", None), ("sampled", SAMP)):
            for proc_label, last_n in (("off", None), ("on, last_n 64", 64), ("on, last_n 0", 0)):
                m.set_sampling(**samp) if samp else m.set_sampling()
                if last_n is None:
                    m.set_penalties()
                    m.set_logit_bias(None)
                else:
                    m.set_penalties(last_n=last_n, **PEN)
                    m.set_logit_bias({5: -1.0, 77: 0.5})
                m.generate([1, 263], pos + 8, exec="graph")  # captures this tail's graphs, fills rows and record
                step = float(np.median(m.time_step(pos, 31)))
                tail = m.profile_kernel("sample", pos, reps=50)
                gen = min(m.generate([1, 263], 128, exec="graph")[1] for _ in range(4)) * 1e3 / 128
                rows.append((name, spec.vocab_size, samp_label, proc_label, step, gen, tail))
        m.close()
        del img
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_proc_cost.txt"))
    ap.add_argument("--presets", default="llama3.2-1b,qwen2.5-0.5b")
    ap.add_argument("--parent-tree", default=None)
    a = ap.parse_args()
    presets = [p for p in a.presets.split(",") if p]
    sys.path.insert(0, ROOT)
    lines = ["# tools/logit_proc_time.py: cost of penalties + logit bias on one MI355X (gfx950)", "",
             "## operator alone: kh_logit_process_f32, back-to-back launches in a graph (us per launch)",
             f"{'V':>7} {'window':>7} {'us':>8}"]
    for V, W, us in operator_rows():
        lines.append(f"{V:>7} {W:>7} {us:8.2f}")
        print(lines[-1], flush=True)
    base = baseline(a.parent_tree, presets) if a.parent_tree else {}
    lines += ["", "## model: 1-step hipGraph at position 64 (median of 31, full classifier), us per token of a 128-step",
              "## graph-mode generate (best of 4; greedy without processors screens the classifier), last launch alone",
              f"{'preset':<13} {'V':>7} {'pick':<8} {'processors':<14} {'step us':>8} {'vs parent':>9} "
              f"{'generate us/tok':>15} {'vs parent':>9} {'last launch us':>14}"]
    for name, (step, gen) in base.items():
        preset, pick = name.rsplit(" ", 1)
        lines.append(f"{preset:<13} {'':>7} {pick:<8} {'parent commit':<14} {step:8.1f} {'':>9} {gen:15.1f}")
        print(lines[-1], flush=True)
    for name, V, pick, proc, step, gen, tail in model_rows(presets):
        b = base.get(f"{name} {pick}")
        d_step = f"{step - b[0]:+9.1f}" if b else f"{'':>9}"
        d_gen = f"{gen - b[1]:+9.1f}" if b else f"{'':>9}"
        lines.append(f"{name:<13} {V:>7} {pick:<8} {proc:<14} {step:8.1f} {d_step} {gen:15.1f} {d_gen} {tail:14.2f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
