"""Same-box A/B of Q4 (KH_FLAG_Q4): decode from the packed 4-bit copy of a 4-bit-exact int8 image against the same image
streamed as int8.

    python tools/q4_ab.py [--models llama2-7b-int8,tinyllama-1.1b-int8] [--out profiles/q4_ab.txt]
                          [--parent <tree of the parent commit, built>] [--rounds 3]

One process per model (this script re-invoked with --model) on a synthetic image of the geometry, requantised to 4 bits
(binfmt.requantize_matrices_q4); the models of a comparison share the device image.  After warm-up:
  * per launch class (qkv, wo, ffn13, w2, cls): kh_model_profile_kernel at position 64, flag off and flag on (every
    class on the copy, hook KH_Q4_CLASSES=0x1f) alternated five times: median and range.  Flag off launches what an int8
    model launches - for ffn13 and cls the LDS-DMA ring kernel.  Adoption rule (DESIGN 3.1c's): a class stays in plan_q4
    (kh_model_q4.hip) only if its Q4 median is below the flag-off median by more than the range of the flag-off runs.
  * 128-step generate, greedy and sampled (T 0.8, K 50, P 0.95), same alternation, of the flag-off model, the model with
    every class on the copy, - where the rule keeps some classes and not all - the model with the kept classes, and the
    model under the default plan (no hook) where that is yet another set.
  * the copy's bytes and build time.
  * --parent: `python bench.py --gpus 1 --steps 128 --warmup 16 --no-cpu-baseline` in the parent tree and in this one,
    alternating fresh processes: the flag-off path against the commit before Q4.
Not measurable here: model quality at 4 bits with symmetric groups, and anything on real checkpoints.
"""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("qkv", "wo", "ffn13", "w2", "cls")
ROUNDS = 5


def _med_range(v):
    return statistics.median(v), max(v) - min(v)


def _spec(name):
    sys.path.insert(0, ROOT)
    from kuiperllama_amd import binfmt
    if name in binfmt.PRESETS:
        return binfmt.PRESETS[name]
    base = name[:-len("-int8")]  # a BASELINE fp32 geometry as an int8 model, group 64
    return dataclasses.replace(binfmt.PRESETS[base], quant=True, shared_classifier=False, group_size=64, name=name)


def one_model(name):
    import torch
    spec = _spec(name)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    binfmt.requantize_matrices_q4(img, spec)
    torch.cuda.synchronize()
    cap = 2048

    def create(mask):
        _ffi.debug_set("KH_Q4_CLASSES", hex(mask))
        try:
            return KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_Q4)
        finally:
            _ffi.debug_set("KH_Q4_CLASSES", None)
    m = {"int8": KuiperModel.from_device_image(img, spec, max_seq_len=cap), "q4-all": create(0x1f)}
    info = m["q4-all"].q4_info()
    print(f"## {name}: dim {spec.dim} hidden {spec.hidden_dim} layers {spec.n_layers} vocab {spec.vocab_size} group "
          f"{spec.group_size}; Q4 state {info['state']}, copy {info['bytes'] / 1e6:.1f} MB built in "
          f"{info['build_us'] / 1e3:.2f} ms")
    assert info["state"] == 1 and len(info["classes"]) == 5, info
    for k in m:  # warm-up: every kernel once
        for c in CLASSES:
            m[k].profile_kernel(c, 64, reps=8)
    keep_mask = 0
    for i, c in enumerate(CLASSES):
        t = {k: [] for k in m}
        for _ in range(ROUNDS):
            for k in m:
                t[k].append(m[k].profile_kernel(c, 64, reps=32))
        (m0, r0), (m1, r1) = _med_range(t["int8"]), _med_range(t["q4-all"])
        keep = m1 < m0 - r0
        keep_mask |= int(keep) << i
        print(f"{c:6s} int8 {m0:7.2f} us (range {r0:.2f})   Q4 {m1:7.2f} us (range {r1:.2f})   {(m1 / m0 - 1) * 100:+6.1f} %   "
              f"{'adopt' if keep else 'DROP (not below int8 by more than its range)'}")
    kept = [c for i, c in enumerate(CLASSES) if keep_mask >> i & 1]
    print(f"classes the adoption rule keeps: {','.join(kept) if kept else 'none'} (mask {hex(keep_mask)})")
    if keep_mask not in (0, 0x1f):
        m["q4-kept"] = create(keep_mask)
    m["q4-plan"] = KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_Q4)  # no hook: plan_q4
    plan = m["q4-plan"].q4_info()["classes"]
    print(f"classes of the default plan (plan_q4): {','.join(plan) if plan else 'none'}")
    if plan == kept and "q4-kept" in m or len(plan) == 5:
        m.pop("q4-plan").close()  # measured under another name
    for label in ("greedy", "sampled"):
        for k in m:
            if label == "sampled":
                m[k].set_sampling(temperature=0.8, top_k=50, top_p=0.95, seed=7)
            m[k].generate([1, 263], 128)  # graph capture, warm-up
        t = {k: [] for k in m}
        for _ in range(ROUNDS):
            for k in m:
                t[k].append(128.0 / (m[k].generate([1, 263], 128)[1] * 1e-3))
        base = statistics.median(t["int8"])
        for k in m:
            md, rg = _med_range(t[k])
            print(f"generate 128 {label:7s} {k:8s}: {md:8.1f} tok/s (range {rg:.1f})"
                  + ("" if k == "int8" else f"   {(md / base - 1) * 100:+.1f} % vs int8"))
    for k in m:
        m[k].close()


def bench(tree, timeout=900):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "16", "--no-cpu-baseline"]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree} ({p.returncode}):\n{p.stderr[-2000:]}")
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return line["value"], line.get("secondary_value")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="(internal) measure one model in this process and print its lines")
    ap.add_argument("--models", default="llama2-7b-int8,tinyllama-1.1b-int8")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q4_ab.txt"))
    a = ap.parse_args()
    if a.model:
        return one_model(a.model)
    lines = ["# tools/q4_ab.py: Q4 (KH_FLAG_Q4) against int8 on requantised synthetic images, one MI355X, one process per "
             "model", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for name in [n for n in a.models.split(",") if n]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", name], capture_output=True, text=True,
                           timeout=900)
        for s in p.stdout.splitlines():
            emit(s)
        if p.returncode != 0:
            emit(f"## {name}: not measured (exit {p.returncode}): {p.stderr.strip().splitlines()[-1:] or ''}")
        emit("")
    if a.parent:
        emit("# flag off against the parent commit: python bench.py --gpus 1 --steps 128 --warmup 16 --no-cpu-baseline, "
             "alternating fresh processes, tok/s of the flagship (Llama-3.2-1B fp32) and of the int8 secondary "
             "(Llama-2-7B int8)")
        old, new = [], []
        for r in range(a.rounds):
            old.append(bench(a.parent))
            new.append(bench(ROOT))
            emit(f"round {r + 1}: parent {old[-1][0]:.1f} / {old[-1][1]}  this tree {new[-1][0]:.1f} / {new[-1][1]}")
        for i, what in ((0, "flagship"), (1, "int8 secondary")):
            o, n = [v[i] for v in old], [v[i] for v in new]
            if any(v is None for v in o + n):
                continue
            spread = max(o + n) - min(o + n)
            d = statistics.median(n) - statistics.median(o)
            emit(f"{what}: median parent {statistics.median(o):.1f}  this tree {statistics.median(n):.1f}  difference "
                 f"{d:+.1f} tok/s; spread of the {2 * a.rounds} runs {spread:.1f}: "
                 f"{'inside' if abs(d) <= spread else 'OUTSIDE'} the spread")


if __name__ == "__main__":
    main()
