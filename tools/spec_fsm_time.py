"""Constrained lookup decode (kh_model_generate_lookup_fsm, csrc/kh_spec.h: k_spec_fsm_rows / k_spec_tail_fsm /
k_spec_accept_fsm) on the GPU: same-box A/B against the parent commit, after tools/constraint_ab.py's method.

The baseline is the PARENT commit's library running generate(exec="graph") under the same automaton - the only
constrained path the parent has.  Against it, this tree's generate_lookup(constrained=True): 128 sampled steps on
synthetic images of two geometries, greedy and with a sampler plus log-probs 5, under three automata:
  (i)   from_choices of four 120-token strings that branch at the first token: everything behind it is forced
  (ii)  a template: a forced run of 6 tokens, then one free position whose row holds V/8 ids, and round again
  (iii) constraint_ab's 6-state automaton with rows of V/8 ids: no forced token, no hint - the new call can only lose,
        by one stream sync per miss_steps steps
Every figure is the call's own elapsed_ms (HIP events around the loop); the words of the two trees are compared on
every row of every round.  This tree also times the constrained PASS against the _as_set pass of the same tokens (the
price of k_spec_fsm_rows, the mask and the advance): wall clock around the synchronous call, median of 30.

    python tools/spec_fsm_time.py --parent-tree DIR [--rounds 5] [--out profiles/spec_fsm_ab.txt]

DIR is a checkout of the parent commit with its library built (python -m kuiperllama_amd.build inside it).  Every round
starts one process per tree, parent first, so the two alternate on one box; a process reports the median of three runs
per mode, modes interleaved.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESETS = ("llama3.2-1b", "llama2-7b-int8")
AUTOMATA = ("i", "ii", "iii")
CONFIGS = ("greedy", "sampled")
STEPS = 128

# runs in either tree: the automata are built from what both trees have; role "new" calls the new entry points
_WORKER = r"""
import json, sys, time
import numpy as np, torch
from kuiperllama_amd import binfmt
from kuiperllama_amd.constraint import TokenAutomaton, from_choices
from kuiperllama_amd.model import KuiperModel
name, role, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
spec = binfmt.PRESETS[name]
V = spec.vocab_size
img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
torch.cuda.synchronize()
m = KuiperModel.from_device_image(img, spec, max_seq_len=256)
P = [1, 263]
T = steps + len(P) - 1
rng = np.random.default_rng(7)
auto = {}
ids = [int(t) for t in rng.choice(V, 500, replace=False) if int(t) != 2]
auto["i"] = from_choices([tuple(ids[120 * i:120 * (i + 1)]) for i in range(4)], 2)
forced = ids[480:486]
free = np.sort(rng.choice(V, V // 8, replace=False)).astype(np.int32)
rows = [(np.array([t], np.int32), np.array([j + 1], np.int32)) for j, t in enumerate(forced)] + [(free, np.zeros(len(free), np.int32))]
auto["ii"] = TokenAutomaton(0, np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])]),
                            np.concatenate([t for t, _ in rows]), np.concatenate([y for _, y in rows]))
k = V // 8
rows6 = [np.sort(rng.choice(V, k, replace=False)).astype(np.int32) for _ in range(6)]
auto["iii"] = TokenAutomaton(0, np.arange(7) * k, np.concatenate(rows6), rng.integers(0, 6, 6 * k))
def arm(config, a):
    if config == "greedy":
        m.set_sampling()
        m.set_logprobs(None)
    else:
        m.set_sampling(0.8, 50, 0.95, 0xC0FFEE)
        m.set_logprobs(5)
    m.set_constraint(a)
def run(a):
    if role == "parent":
        w, ms = m.generate(P, T, exec="graph")
        return w, ms, None
    return m.generate_lookup(P, T, constrained=True)
modes = [(c, a) for c in ("greedy", "sampled") for a in ("i", "ii", "iii")]
out = {f"{c}/{a}": {"ms": []} for c, a in modes}
for c, a in modes:
    arm(c, auto[a])
    for _ in range(2):
        run(a)
for _ in range(3):
    for c, a in modes:
        arm(c, auto[a])
        w, ms, st = run(a)
        o = out[f"{c}/{a}"]
        o["ms"].append(ms)
        o["words"], o["stats"] = w, st
for o in out.values():
    o["ms"] = float(np.median(o["ms"]))
if role == "new":  # the constrained pass against the _as_set pass of the same tokens, on this library
    width = m.verify_width()
    A = auto["ii"]
    for c in ("greedy", "sampled"):
        arm(c, A)
        text = P + m.generate(P, T, exec="graph")[0][len(P) - 1:]
        p0 = 16
        fed, s0 = text[p0:p0 + width], A.walk(text[len(P):p0 + 1])[0]
        def timed(constrained):
            ts = []
            for _ in range(32):
                if constrained:
                    m.constraint_state = s0
                t0 = time.perf_counter()
                nxt, a = m.verify(fed, p0, constrained=True) if constrained else m.verify(fed, p0, as_set=True)
                ts.append(1e3 * (time.perf_counter() - t0))
            return float(np.median(ts[2:])), int(a)
        on, a_on = timed(True)
        m.set_constraint(None)
        off, a_off = timed(False)
        out[f"pass/{c}"] = {"constrained_ms": on, "as_set_ms": off, "width": width, "accepted": [a_on, a_off]}
print("AB " + json.dumps(out))
"""


def run(tree, name, role):
    r = subprocess.run([sys.executable, "-c", _WORKER, name, role, str(STEPS)], cwd=tree, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=tree), timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("AB "))
    return json.loads(line[3:])


def _row(label, v, base=None):
    med = float(np.median(v))
    tail = f"  {base / med:5.2f}x" if base else ""
    return f"{label:52s} {med:8.3f} [{min(v):8.3f} .. {max(v):8.3f}]{tail}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--presets", default=",".join(PRESETS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("spec_fsm_time: no GPU (timings are taken on the GPU or not at all)")
    lines = [f"# constrained lookup decode: {STEPS} sampled steps, ms per run (HIP events around the loop)",
             f"# median [min .. max] over {a.rounds} alternated rounds; each round: median of 3 runs per mode",
             "# parent = the parent commit's generate(exec=graph) under the automaton; new = generate_lookup(constrained)",
             "# x = parent median / new median; pass rows: wall clock around one synchronous verify call, median of 30",
             f"# device: {torch.cuda.get_device_name(0)}"]

    def flush():
        text = "\n".join(lines) + "\n"
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return text
    labels = {"i": "(i) four 120-token choices, all forced", "ii": "(ii) template: 6 forced, 1 free of V/8",
              "iii": "(iii) 6 states, rows of V/8, nothing forced"}
    for name in a.presets.split(","):
        modes = [f"{c}/{k}" for c in CONFIGS for k in AUTOMATA]
        got = {mode: {"parent": [], "new": []} for mode in modes}
        passes = {c: {"constrained_ms": [], "as_set_ms": []} for c in CONFIGS}
        same, stats, width = True, {}, 0
        for rnd in range(a.rounds):
            par = run(os.path.abspath(a.parent_tree), name, "parent")
            new = run(ROOT, name, "new")
            for mode in modes:
                got[mode]["parent"].append(par[mode]["ms"])
                got[mode]["new"].append(new[mode]["ms"])
                same = same and par[mode]["words"] == new[mode]["words"]
                stats[mode] = new[mode]["stats"]
            for c in CONFIGS:
                for k in passes[c]:
                    passes[c][k].append(new[f"pass/{c}"][k])
                width = new[f"pass/{c}"]["width"]
            print(f"# {name} round {rnd + 1}: " + " ".join(
                f"{mode}={got[mode]['parent'][-1]:.2f}/{got[mode]['new'][-1]:.2f}" for mode in modes), flush=True)
        lines.append(f"## {name}")
        for c in CONFIGS:
            lines.append(f"### {'greedy' if c == 'greedy' else 'sampler (T 0.8, top-k 50, top-p 0.95) + log-probs 5'}")
            for k in AUTOMATA:
                g = got[f"{c}/{k}"]
                lines.append(_row(f"{labels[k]}: parent", g["parent"]))
                lines.append(_row(f"{labels[k]}: new", g["new"], float(np.median(g["parent"]))))
                lines.append(f"    stats {json.dumps(stats[f'{c}/{k}'], sort_keys=True)}")
            p = passes[c]
            lines.append(_row(f"one pass of {width}: _as_set, constraint off", p["as_set_ms"]))
            lines.append(_row(f"one pass of {width}: constrained", p["constrained_ms"]))
        lines.append(f"words equal on every row of every round: {'yes' if same else 'NO'}")
        flush()
    print(flush(), end="")


if __name__ == "__main__":
    main()
