"""Cost of seeded sampling (csrc/kh_sample.h) on the GPU.

    python tools/sample_time.py [--out profiles/sample_cost.txt] [--presets llama3.2-1b,qwen2.5-0.5b]

1. Operator: kh_sample_f32 (one draw, one 1024-thread workgroup) on peaked (Zipf-like l_i = -1.1 ln(rank)) and flat
   (normal, sigma 0.5) logits of the BASELINE vocabularies, against kh_argmax_f32.  Average of back-to-back launches
   captured in a torch CUDA graph, between two events (no host enqueue gaps in the figure).
2. Model: the decode step at position 64 replayed as a 1-step hipGraph (kh_model_time_step, median of 31) greedy and
   sampled, on seeded synthetic images of the BASELINE presets; plus the sampler launch alone inside the model
   (kh_model_profile_kernel "sample": on the synthetic model's own logits, after k_cls).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kuiperllama_amd import binfmt, ops  # noqa: E402
from kuiperllama_amd.model import KuiperModel  # noqa: E402

SAMPLED = [("T=0.8 P=0.95 K=0", dict(temperature=0.8, top_k=0, top_p=0.95, seed=1)),
           ("T=0.8 P=0.95 K=50", dict(temperature=0.8, top_k=50, top_p=0.95, seed=1)),
           ("T=1 (no top-k / top-p)", dict(temperature=1.0, top_k=0, top_p=1.0, seed=1))]


def _logits(kind, V):
    rng = np.random.default_rng(V)
    if kind == "peaked":
        return (-1.1 * np.log(rng.permutation(V) + 1.0)).astype(np.float32)
    return rng.normal(0.0, 0.5, V).astype(np.float32)


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


def operator_rows(vocabs):
    rows = []
    dev = torch.device("cuda:0")
    for V in vocabs:
        for kind in ("peaked", "flat"):
            lg = torch.from_numpy(_logits(kind, V)).to(dev)
            out = torch.empty(1, dtype=torch.int32, device=dev)
            rows.append((V, kind, "argmax (greedy)", _graph_us(lambda: ops.argmax(lg, out))))
            for name, p in SAMPLED:
                rows.append((V, kind, name, _graph_us(lambda: ops.sample(lg, out, p, 0))))
    return rows


def model_rows(presets, pos=64):
    rows = []
    dev = torch.device("cuda:0")
    for name in presets:
        spec = binfmt.PRESETS[name]
        img = binfmt.synth_image(spec, seed=1234, device=dev)
        torch.cuda.synchronize()
        m = KuiperModel.from_device_image(img, spec, max_seq_len=256)
        res = {}
        for label, p in [("greedy", None)] + SAMPLED[:2]:
            if p is None:
                m.set_sampling()
            else:
                m.set_sampling(**p)
            m.generate([1, 263], pos + 8, exec="graph")  # captures this sampler's graphs, fills rows 0 .. pos
            step = float(np.median(m.time_step(pos, 31)))
            samp_us = m.profile_kernel("sample", pos, reps=50)
            res[label] = (step, samp_us)
        m.close()
        del img
        torch.cuda.empty_cache()
        g = res["greedy"][0]
        for label, (step, samp_us) in res.items():
            rows.append((name, spec.vocab_size, label, step, step - g, samp_us))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_cost.txt"))
    ap.add_argument("--presets", default="llama3.2-1b,qwen2.5-0.5b,stories15M,tinyllama-1.1b")
    a = ap.parse_args()
    lines = ["# tools/sample_time.py: seeded sampling cost on one MI355X (gfx950)", "",
             "## operator: one draw, back-to-back launches in a graph (us per launch)",
             f"{'V':>7} {'logits':>7}  {'sampler':<24} {'us':>7}"]
    for V, kind, name, us in operator_rows([32000, 128256, 151936]):
        lines.append(f"{V:>7} {kind:>7}  {name:<24} {us:7.2f}")
        print(lines[-1], flush=True)
    lines += ["", "## model: decode step at position 64 (1-step hipGraph, median of 31) and the sampler launch alone",
              f"{'preset':<15} {'V':>7}  {'sampler':<24} {'step us':>8} {'vs greedy':>9} {'sample-launch us':>16}"]
    for name, V, label, step, d, s in model_rows([p for p in a.presets.split(",") if p]):
        lines.append(f"{name:<15} {V:>7}  {label:<24} {step:8.1f} {d:+9.1f} {s:16.2f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
