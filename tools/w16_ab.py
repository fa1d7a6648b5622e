"""Same-box A/B of W16 (KH_FLAG_W16): decode from the 16-bit copy of a bf16-exact image against the same image
streamed as fp32.

    python tools/w16_ab.py [--models llama3.2-1b,tinyllama-1.1b,qwen2.5-0.5b,llama2-7b] [--out profiles/w16_ab.txt]
                           [--parent <tree of the parent commit, built>] [--rounds 3]

One process per model (this script re-invoked with --model) on a synthetic image of the BASELINE geometry whose
matrices were rounded to bf16 (binfmt.round_matrices_bf16); the flag-off and the flag-on model share the device image.
  * per launch class (qkv, wo, ffn13, w2, cls): kh_model_profile_kernel at position 64, flag off and on alternated
    five times: median and range.  Adoption rule: a class whose W16 median is not below the fp32 median by more than
    the range of the fp32 runs should be taken out of plan_w16 (kh_model_w16.hip); the file names such classes.
  * 128-step generate, greedy and sampled (T 0.8, K 50, P 0.95), same alternation: tok/s and the HBM rate reached with
    the bytes the byte model (binfmt.ModelSpec.algorithmic_bytes_per_token at position 64) says are streamed - the
    matrices of the adopted classes at 2 bytes per weight with the flag on; a greedy step screens the classifier from
    its bf16 copy with and without the flag (kh_cls_screen.h), so its classifier counts 2 bytes per weight in both.
  * --parent: `python bench.py --gpus 1 --steps 128 --warmup 16 --no-cpu-baseline` in the parent tree and in this one,
    alternating fresh processes: the flag-off path against the commit before W16.
"""
import argparse
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


def one_model(name):
    import torch
    sys.path.insert(0, ROOT)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS[name]
    dev = torch.device("cuda:0")
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()
    cap = 2048
    m = {0: KuiperModel.from_device_image(img, spec, max_seq_len=cap),
         1: KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_W16)}
    info = m[1].w16_info()
    print(f"## {name}: dim {spec.dim} hidden {spec.hidden_dim} layers {spec.n_layers} vocab {spec.vocab_size}; W16 state "
          f"{info['state']}, copy {info['bytes'] / 1e6:.1f} MB built in {info['build_us'] / 1e3:.2f} ms, classes "
          f"{','.join(info['classes'])}")
    assert info["state"] == 1, info
    out = []
    for c in CLASSES:
        t = {0: [], 1: []}
        for _ in range(ROUNDS):
            for f in (0, 1):
                t[f].append(m[f].profile_kernel(c, 64, reps=32))
        (m0, r0), (m1, r1) = _med_range(t[0]), _med_range(t[1])
        keep = m1 < m0 - r0
        kb = spec.kernel_bytes()[c]
        if not keep:
            out.append(c)
        print(f"{c:6s} fp32 {m0:7.2f} us (range {r0:.2f})   W16 {m1:7.2f} us (range {r1:.2f})   {(m1 / m0 - 1) * 100:+6.1f} %   "
              f"fp32 {kb / m0 / 1e6:.2f} TB/s   {'adopt' if keep else 'TAKE OUT (not below fp32 by more than its range)'}")
    print(f"classes the adoption rule takes out: {','.join(out) if out else 'none'}")
    mat = spec.weight_elems()  # matrix weights streamed per token
    cls = spec.vocab_size * spec.dim
    base = spec.algorithmic_bytes_per_token(64)
    for label in ("greedy", "sampled"):
        for f in (0, 1):
            if label == "sampled":
                m[f].set_sampling(temperature=0.8, top_k=50, top_p=0.95, seed=7)
            m[f].generate([1, 263], 128)  # graph capture, warm-up
        t = {0: [], 1: []}
        for _ in range(ROUNDS):
            for f in (0, 1):
                t[f].append(128.0 / (m[f].generate([1, 263], 128)[1] * 1e-3))
        screened = label == "greedy"  # the greedy tail reads the classifier's bf16 copy with and without W16
        by = {0: base - (2 * cls if screened else 0),
              1: base - 2 * (mat - cls) - 2 * cls}
        for f in (0, 1):
            md, rg = _med_range(t[f])
            print(f"generate 128 {label:7s} {'W16 ' if f else 'fp32'}: {md:8.1f} tok/s (range {rg:.1f}), "
                  f"{by[f] / 1e6:.1f} MB per token -> {by[f] * md / 1e12:.2f} TB/s")
        print(f"generate 128 {label:7s} W16 vs fp32: {(statistics.median(t[1]) / statistics.median(t[0]) - 1) * 100:+.1f} %")
    for f in (0, 1):
        m[f].close()


def bench(tree, timeout=600):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "16", "--no-cpu-baseline"]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree} ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="(internal) measure one model in this process and print its lines")
    ap.add_argument("--models", default="llama3.2-1b,tinyllama-1.1b,qwen2.5-0.5b,llama2-7b")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w16_ab.txt"))
    a = ap.parse_args()
    if a.model:
        return one_model(a.model)
    lines = ["# tools/w16_ab.py: W16 (KH_FLAG_W16) against fp32 on bf16-rounded synthetic images, one MI355X, one process "
             "per model", ""]

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
             "alternating fresh processes, tok/s of Llama-3.2-1B fp32")
        old, new = [], []
        for r in range(a.rounds):
            old.append(bench(a.parent))
            new.append(bench(ROOT))
            emit(f"round {r + 1}: parent {old[-1]:.1f}  this tree {new[-1]:.1f}")
        spread = max(old + new) - min(old + new)
        d = statistics.median(new) - statistics.median(old)
        emit(f"median: parent {statistics.median(old):.1f}  this tree {statistics.median(new):.1f}  difference {d:+.1f} tok/s; "
             f"spread of the {2 * a.rounds} runs {spread:.1f}: {'inside' if abs(d) <= spread else 'OUTSIDE'} the spread")


if __name__ == "__main__":
    main()
