"""Same-box A/B of the int8 tier ahead of the bf16 classifier screen: the parent commit's tree against this one.

    python tools/cls_screen_q8_ab.py --parent <tree of the parent commit, built> [--rounds 3] [--out profiles/cls_screen_q8_ab.txt]

Each round runs `python bench.py --gpus 1 --steps 128 --warmup 16` in the parent tree, then in this tree, each as a
fresh process (plain line: tok/s of the flagship workload).  Then once per tree `--dump-outputs` (words.npy and
logits.npy must be byte-identical); Llama-2-7B int8 greedy and Llama-3.2-1B sampled decode, alternating between the
trees as fresh processes (neither runs the tier: they must be unchanged); and in this tree: creation cost and HBM of the
int8 copy, survivors and bf16 candidates per step over the benchmark's steps, tier-1 spills and overflow steps (both
must be 0), and the cost of a forced-overflow step (a zero final norm) against the two-launch tail and no screen.
With --rocprof: `rocprofv3 --kernel-trace --stats` of the bench command in both trees, the step tail's kernels.
With --sweep: the step loop under a few KH_SHAPE_SCREEN_Q8 launch shapes of tier 1, in this tree.

The acceptance rule printed at the end: the tier stays on by default only if every new run beats every parent run and
the median gain exceeds three times the larger max - min spread either build shows across its own rounds.
"""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tree, extra=(), timeout=420):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "16", *extra]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree} ({p.returncode}):\n{p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def side(tree, what, timeout=420):
    """tok/s of a workload the tier does not touch, measured by a fresh process on the package of `tree`."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", what, "--tree", tree], cwd=tree,
                       capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"--side {what} failed in {tree} ({p.returncode}):\n{p.stderr[-2000:]}")
    return float(p.stdout.strip().splitlines()[-1])


def run_side(tree, what):
    sys.path.insert(0, tree)
    import torch
    from kuiperllama_amd import binfmt
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS["llama2-7b-int8" if what == "int8" else "llama3.2-1b"]
    img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec)
    if what == "sampled":
        m.set_sampling(temperature=0.8, top_k=50, seed=7)
    m.generate([1, 263], 16)
    ms = [m.generate([1, 263], 128)[1] for _ in range(5)]
    m.close()
    print(128 / statistics.median(ms) * 1e3)


def details(lines):
    import torch
    sys.path.insert(0, ROOT)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS["llama3.2-1b"]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    KuiperModel.from_device_image(img, spec).close()  # the process's first-use costs are not the copy's
    t = {"0": [], None: []}
    for hook in ("0", None, "0", None, "0", None):
        _ffi.debug_set("KH_CLS_SCREEN_Q8", hook)
        t0 = time.perf_counter()
        m = KuiperModel.from_device_image(img, spec)
        t[hook].append((time.perf_counter() - t0) * 1e3)
        j = m.cls_screen_q8_info()
        m.close()
    a, b = statistics.median(t["0"]), statistics.median(t[None])
    m = KuiperModel.from_device_image(img, spec)
    lines.append(f"model creation (weights resident, alternating, median of 3): {a:.1f} ms without, {b:.1f} ms with the int8 "
                 f"copy: {b - a:+.1f} ms (conversion kernel {j['build_us'] / 1e3:.2f} ms, the rest is the allocation and the "
                 f"tier's self-test); HBM added {j['bytes'] / 1e6:.1f} MB beside the bf16 copy's "
                 f"{m.cls_screen_info()['bytes'] / 1e6:.1f} MB; self-test {j['selftest']}")

    def timed(label):
        m.generate([1, 263], 16)
        i0, j0 = m.cls_screen_info(), m.cls_screen_q8_info()
        ms = [m.generate([1, 263], 128)[1] for _ in range(5)]
        i1, j1 = m.cls_screen_info(), m.cls_screen_q8_info()
        n, n8 = i1["steps"] - i0["steps"], j1["steps"] - j0["steps"]
        lines.append(f"{label}: {n} screened steps, {n8} of them behind tier 1, "
                     f"{(j1['survivors'] - j0['survivors']) / max(1, n8):.2f} survivors per step, "
                     f"{(i1['candidates'] - i0['candidates']) / max(1, n):.3f} bf16 candidates per step, "
                     f"{j1['spill_steps'] - j0['spill_steps']} tier-1 spills, {i1['overflow_steps'] - i0['overflow_steps']} overflow "
                     f"steps; step loop {statistics.median(ms) / 128 * 1e3:.1f} us per token (HIP events, median of 5)")
        return statistics.median(ms) / 128 * 1e3
    timed("three-launch tail")
    _ffi.debug_set("KH_CLS_SCREEN_Q8", "0")
    timed("two-launch tail (KH_CLS_SCREEN_Q8=0, same process)")
    _ffi.debug_set("KH_CLS_SCREEN_Q8", None)
    m.close()
    # forced overflow: every logit equal, tier 1 spills, the bf16 launch scans every row, the sampler overflows
    ents = {e.name: e for e in binfmt.layout(spec)[0]}
    binfmt.tensor_from_image(img, ents["final_norm"]).zero_()
    m = KuiperModel.from_device_image(img, spec)
    a = timed("forced overflow (final norm zero), three-launch tail")
    _ffi.debug_set("KH_CLS_SCREEN_Q8", "0")
    b = timed("forced overflow, two-launch tail")
    _ffi.debug_set("KH_CLS_SCREEN", "0")
    c = statistics.median(m.generate([1, 263], 128)[1] for _ in range(5)) / 128 * 1e3
    _ffi.debug_set("KH_CLS_SCREEN", None)
    _ffi.debug_set("KH_CLS_SCREEN_Q8", None)
    lines.append(f"forced overflow costs {a - b:+.1f} us per token over the two-launch tail (the tier-1 launch); unscreened {c:.1f}")
    m.close()


def rocprof(tree):
    """Lines of the kernel statistics of one bench run under rocprofv3 that name the step tail's kernels."""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "p", "--",
               sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "16"]
        p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=420)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed in {tree} ({p.returncode}):\n{p.stderr[-2000:]}")
        for d, _, files in os.walk(td):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    rows = open(os.path.join(d, f)).read().splitlines()
                    return [rows[0]] + [r for r in rows[1:] if "k_cls_screen" in r or "k_sample_screen" in r]
    raise RuntimeError("rocprofv3 wrote no kernel statistics")


SWEEP = (None, "2,512,256", "2,1024,256", "2,1536,256", "2,384,512", "2,512,512", "2,1024,512", "4,768,256")


def sweep(lines):
    """Step loop per token under tier-1 launch shapes (u, grid, wg); None is the planned shape."""
    import torch
    sys.path.insert(0, ROOT)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS["llama3.2-1b"]
    img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    for shape in SWEEP:
        _ffi.debug_set("KH_SHAPE_SCREEN_Q8", shape)
        m = KuiperModel.from_device_image(img, spec)
        _ffi.debug_set("KH_SHAPE_SCREEN_Q8", None)
        us = {}
        for hook in (None, "0"):
            _ffi.debug_set("KH_CLS_SCREEN_Q8", hook)
            m.generate([1, 263], 16)
            us[hook] = statistics.median(m.generate([1, 263], 128)[1] for _ in range(5)) / 128 * 1e3
        _ffi.debug_set("KH_CLS_SCREEN_Q8", None)
        m.close()
        lines.append(f"KH_SHAPE_SCREEN_Q8={shape or '(unset: 2, 3 per CU, 256)'}: three-launch tail {us[None]:.1f} us per token, "
                     f"two-launch tail {us['0']:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_screen_q8_ab.txt"))
    ap.add_argument("--no-sides", action="store_true", help="skip the Llama-2-7B int8 and sampled alternations")
    ap.add_argument("--rocprof", action="store_true", help="also rocprofv3 kernel statistics of the bench command, both trees")
    ap.add_argument("--sweep", action="store_true", help="also the step loop under a few tier-1 launch shapes")
    ap.add_argument("--side", choices=("int8", "sampled"))
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.side:
        return run_side(a.tree, a.side)
    if not a.parent:
        ap.error("--parent is required")
    a.parent = os.path.abspath(a.parent)
    lines = ["# tools/cls_screen_q8_ab.py: parent commit vs int8 tier ahead of the bf16 screen, one MI355X, alternating fresh processes",
             "# python bench.py --gpus 1 --steps 128 --warmup 16 (plain line), tok/s of Llama-3.2-1B fp32", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    old, new = [], []
    for r in range(a.rounds):
        old.append(bench(a.parent)["value"])
        new.append(bench(ROOT)["value"])
        emit(f"round {r + 1}: parent {old[-1]:.1f}  int8 tier {new[-1]:.1f}  ({(new[-1] / old[-1] - 1) * 100:+.2f} %)")
    gain = (statistics.median(new) / statistics.median(old) - 1) * 100
    spread = max((max(v) - min(v)) / statistics.median(v) * 100 for v in (old, new))
    every = min(new) > max(old)
    emit(f"median: parent {statistics.median(old):.1f}  int8 tier {statistics.median(new):.1f}  gain {gain:+.2f} % (byte model: "
         f"+3.5 to +4 %); larger max - min spread of a build {spread:.2f} %")
    emit(f"acceptance: every new run above every parent run: {every}; gain above three times the spread: {gain > 3 * spread}"
         f" -> the tier {'stays on' if every and gain > 3 * spread else 'does NOT qualify to be on'} by default")
    with tempfile.TemporaryDirectory() as td:
        for name, tree in (("parent", a.parent), ("new", ROOT)):
            bench(tree, ("--dump-outputs", os.path.join(td, name)))
        for f in ("words.npy", "logits.npy"):
            same = filecmp.cmp(os.path.join(td, "parent", f), os.path.join(td, "new", f), shallow=False)
            emit(f"--dump-outputs {f}: {'byte-identical' if same else 'DIFFERENT'}")
    if not a.no_sides:
        for what, label in (("int8", "Llama-2-7B int8 greedy"), ("sampled", "Llama-3.2-1B sampled (t 0.8, top-k 50)")):
            o, n = [], []
            for _ in range(2):
                o.append(side(a.parent, what))
                n.append(side(ROOT, what))
            emit(f"{label}, tok/s of the step loop, alternating: parent {o[0]:.1f} {o[1]:.1f}  new {n[0]:.1f} {n[1]:.1f}  "
                 f"({(statistics.mean(n) / statistics.mean(o) - 1) * 100:+.2f} %: the tier does not run here)")
    d = []
    details(d)
    for s in d:
        emit(s)
    if a.rocprof:
        for name, tree in (("parent", a.parent), ("this", ROOT)):
            emit("")
            emit(f"# rocprofv3 --kernel-trace --stats -- python bench.py --gpus 1 --steps 128 --warmup 16, {name} tree: the step "
                 "tail's kernels (ns; the one long k_cls_screen call of this tree is the bf16 self-test's full scan)")
            for row in rocprof(tree):
                emit(row[:200])
    if a.sweep:
        emit("")
        emit("# tier-1 launch shapes (u, grid, wg), this tree: step loop of 5 x 128 steps (HIP events, median), one model each")
        d = []
        sweep(d)
        for s in d:
            emit(s)


if __name__ == "__main__":
    main()
