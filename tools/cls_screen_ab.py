"""Same-box A/B of the screened classifier: the parent commit's tree against this one, alternating.

    python tools/cls_screen_ab.py --parent <tree of the parent commit, built> [--rounds 3] [--out profiles/cls_screen_ab.txt]

Each round runs `python bench.py --gpus 1 --steps 128 --warmup 16` in the parent tree, then in this tree, each as a
fresh process (plain line: tok/s of the flagship workload).  Then once per tree `--dump-outputs` (words.npy and
logits.npy must be byte-identical), and in this tree: model-creation cost and HBM bytes of the bf16 copy, candidate
rows per step over the 128 benchmark steps, the cost of logits() behind a screened run, and forced overflow steps
(a zero final norm: every logit equal, every step overflows).
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


def details(lines):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS["llama3.2-1b"]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    t = {}
    for flag in (_ffi.KH_FLAG_NO_CLS_SCREEN, 0):
        t0 = time.perf_counter()
        m = KuiperModel.from_device_image(img, spec, flags=flag)
        t[flag] = (time.perf_counter() - t0) * 1e3
        if flag:
            m.close()
    info = m.cls_screen_info()
    lines.append(f"model creation (weights resident): {t[_ffi.KH_FLAG_NO_CLS_SCREEN]:.1f} ms without, {t[0]:.1f} ms with "
                 f"the bf16 copy (conversion kernel {info['build_us'] / 1e3:.2f} ms); HBM added {info['bytes'] / 1e6:.1f} MB; "
                 f"self-test {info['selftest']}")
    m.generate([1, 263], 16)
    i0 = m.cls_screen_info()
    ms = [m.generate([1, 263], 128)[1] for _ in range(5)]
    i1 = m.cls_screen_info()
    n = i1["steps"] - i0["steps"]
    lines.append(f"screened: {n} steps, {(i1['candidates'] - i0['candidates']) / n:.3f} candidate rows per step, "
                 f"{i1['overflow_steps'] - i0['overflow_steps']} overflow steps; step loop "
                 f"{statistics.median(ms) / 128 * 1e3:.1f} us per token (HIP events, median of 5)")
    m.generate([1, 263], 128)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.logits()
    t_stale = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    m.logits()
    t_fresh = (time.perf_counter() - t0) * 1e6
    lines.append(f"logits() behind a screened run: {t_stale:.0f} us (k_cls on the saved input + copy), again: {t_fresh:.0f} us")
    _ffi.debug_set("KH_CLS_SCREEN", "0")
    ms0 = [m.generate([1, 263], 128)[1] for _ in range(5)]
    _ffi.debug_set("KH_CLS_SCREEN", None)
    m.close()
    # forced overflow: every logit equal
    ents = {e.name: e for e in binfmt.layout(spec)[0]}
    binfmt.tensor_from_image(img, ents["final_norm"]).zero_()
    m = KuiperModel.from_device_image(img, spec)
    m.generate([1, 263], 16)
    i0 = m.cls_screen_info()
    msv = [m.generate([1, 263], 128)[1] for _ in range(5)]
    i1 = m.cls_screen_info()
    lines.append(f"forced overflow (final norm zero, {i1['overflow_steps'] - i0['overflow_steps']} of "
                 f"{i1['steps'] - i0['steps']} steps overflow): {statistics.median(msv) / 128 * 1e3:.1f} us per token against "
                 f"{statistics.median(ms0) / 128 * 1e3:.1f} unscreened (KH_CLS_SCREEN=0, same process) and "
                 f"{statistics.median(ms) / 128 * 1e3:.1f} screened")
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_screen_ab.txt"))
    ap.add_argument("--full", action="store_true", help="also one alternation of --full (secondary_value: Llama-2-7B int8)")
    a = ap.parse_args()
    lines = ["# tools/cls_screen_ab.py: parent commit vs screened classifier, one MI355X, alternating fresh processes",
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
        emit(f"round {r + 1}: parent {old[-1]:.1f}  screened {new[-1]:.1f}  ({(new[-1] / old[-1] - 1) * 100:+.2f} %)")
    gain = (statistics.median(new) / statistics.median(old) - 1) * 100
    emit(f"median: parent {statistics.median(old):.1f}  screened {statistics.median(new):.1f}  gain {gain:+.2f} % "
         f"(byte model: about +8 %); every screened run above every parent run: {min(new) > max(old)}")
    with tempfile.TemporaryDirectory() as td:
        for name, tree in (("parent", a.parent), ("new", ROOT)):
            bench(tree, ("--dump-outputs", os.path.join(td, name)))
        for f in ("words.npy", "logits.npy"):
            same = filecmp.cmp(os.path.join(td, "parent", f), os.path.join(td, "new", f), shallow=False)
            emit(f"--dump-outputs {f}: {'byte-identical' if same else 'DIFFERENT'}")
    if a.full:
        o = bench(a.parent, ("--full", "--no-cpu-baseline"), timeout=900)
        n = bench(ROOT, ("--full", "--no-cpu-baseline"), timeout=900)
        emit(f"--full secondary_value (Llama-2-7B int8, not screened): parent {o.get('secondary_value')}  new {n.get('secondary_value')}")
        k = n.get("roofline", {}).get("kernels_avg_us")
        emit(f"--full per-kernel figures of the new build (single-step entry points: `cls` is the full k_cls): {k}")
    d = []
    details(d)
    for s in d:
        emit(s)


if __name__ == "__main__":
    main()
