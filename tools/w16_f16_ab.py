"""Same-box A/B of the fp16 format of W16 (KH_FLAG_W16_F16): decode and the B-token passes from the fp16-format 16-bit
copy of an fp16-exact image against the same image streamed as fp32, and against the bf16 format at the same geometry.

    python tools/w16_f16_ab.py [--models llama3.2-1b,tinyllama-1.1b,qwen2.5-0.5b,llama2-7b] [--out profiles/w16_f16_ab.txt]
                               [--parent-lib <libkuiper_hip.so of the parent commit>] [--rounds 3]

One process per model (this script re-invoked with --model) on a synthetic image of the BASELINE geometry whose
matrices were rounded to fp16 (binfmt.round_matrices_fp16); every model of the process shares that device image, except
the bf16 comparison model, which needs a bf16-rounded image of the same geometry (same bytes, other values).
  * per launch class (qkv, wo, ffn13, w2, cls): kh_model_profile_kernel at position 64; flag off, fp16 copy and bf16
    copy alternated five times: median and range.  The baseline is the fp32 run.  Adoption rule: a class
    whose fp16 median is not below the fp32 median by more than the range of the fp32 runs should be masked out for the
    fp16 format; the file names such classes.  fp16 against bf16: same bytes, same instruction count expected.
  * 128-step generate, greedy and sampled (T 0.8, K 50, P 0.95), flag off and on alternated five times: tok/s.
  * the passes, one flag-on model per setting of KH_W16_PASS (0 fp32, 1 default, 0x1f all, each single class), and the
    bf16 model with 0x1f: kh_model_time_prefill of 64 tokens per pass and a score of 64 tokens (wall clock), alternated
    five times.  The adoption rule per class, on the prefill pass for qkv, wo, ffn13 and w2, on score for cls.
  * --parent-lib: `python bench.py --gpus 1 --steps 128 --warmup 16 --no-cpu-baseline` with the parent's library
    (KH_LIB) and with this tree's, alternating fresh processes: the flag-off path must not move.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("qkv", "wo", "ffn13", "w2", "cls")
SETTINGS = (("0", "fp32"), ("1", "default"), ("0x1f", "all"), ("0x1", "qkv"), ("0x2", "wo"), ("0x4", "ffn13"), ("0x8", "w2"),
            ("0x10", "cls"))
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
    binfmt.round_matrices_fp16(img, spec)
    img_b = binfmt.synth_image(spec, seed=1234, device=dev)
    binfmt.round_matrices_bf16(img_b, spec)
    torch.cuda.synchronize()
    cap = 2048
    F16 = _ffi.KH_FLAG_W16_F16
    off = KuiperModel.from_device_image(img, spec, max_seq_len=cap)
    m = {}
    for hook, label in SETTINGS:
        _ffi.debug_set("KH_W16_PASS", hook)
        m[label] = KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=F16)
    _ffi.debug_set("KH_W16_PASS", "0x1f")
    bf = KuiperModel.from_device_image(img_b, spec, max_seq_len=cap, flags=F16)
    _ffi.debug_set("KH_W16_PASS", None)
    on = m["default"]
    info = on.w16_info()
    print(f"## {name}: dim {spec.dim} hidden {spec.hidden_dim} layers {spec.n_layers} vocab {spec.vocab_size}; state "
          f"{info['state']}, format {on.w16_format()['format']}, copy {info['bytes'] / 1e6:.1f} MB built in "
          f"{info['build_us'] / 1e3:.2f} ms (the bf16 attempt and the fp16 build), classes {','.join(info['classes'])}; "
          f"default pass mask {','.join(on.w16_pass_info()['classes']) or 'none'}; bf16 model: format {bf.w16_format()['format']}")
    assert info["state"] == 1 and on.w16_format()["format"] == "fp16" and bf.w16_format()["format"] == "bf16"
    out = []
    for c in CLASSES:
        t = {"fp32": [], "fp16": [], "bf16": []}
        for _ in range(ROUNDS):
            for label, mm in (("fp32", off), ("fp16", on), ("bf16", bf)):
                t[label].append(mm.profile_kernel(c, 64, reps=32))
        (m0, r0), (m1, r1), (m2, r2) = _med_range(t["fp32"]), _med_range(t["fp16"]), _med_range(t["bf16"])
        keep = m1 < m0 - r0
        if not keep:
            out.append(c)
        print(f"{c:6s} fp32 {m0:7.2f} us (range {r0:.2f})   fp16 copy {m1:7.2f} us (range {r1:.2f})   {(m1 / m0 - 1) * 100:+6.1f} %   "
              f"{'adopt' if keep else 'MASK OUT (not below fp32 by more than its range)'}   |   bf16 copy {m2:7.2f} us (range "
              f"{r2:.2f}), fp16 - bf16 {m1 - m2:+.2f} us: {'inside' if abs(m1 - m2) <= max(r1, r2) else 'OUTSIDE'} the ranges")
    print(f"decode classes the adoption rule masks out for fp16: {','.join(out) if out else 'none'}")
    for label in ("greedy", "sampled"):
        for mm in (off, on):
            if label == "sampled":
                mm.set_sampling(temperature=0.8, top_k=50, top_p=0.95, seed=7)
            mm.generate([1, 263], 128)  # graph capture, warm-up
        t = {0: [], 1: []}
        words = {}
        for _ in range(ROUNDS):
            for f, mm in ((0, off), (1, on)):
                w, ms = mm.generate([1, 263], 128)
                t[f].append(128.0 / (ms * 1e-3))
                if words.setdefault(label, w) != w:
                    raise SystemExit(f"{name}: {label} words differ between flag off and on")
        for f in (0, 1):
            md, rg = _med_range(t[f])
            print(f"generate 128 {label:7s} {'fp16 copy' if f else 'fp32     '}: {md:8.1f} tok/s (range {rg:.1f})")
        print(f"generate 128 {label:7s} fp16 copy vs fp32: {(statistics.median(t[1]) / statistics.median(t[0]) - 1) * 100:+.1f} %")
    for mm in (off, on):
        mm.set_sampling()
    # ---- the passes
    width = m["fp32"].seq_width()
    toks = [1] + [263 + 7 * i for i in range(63)]
    figures = ("prefill/pass ms", "score64 ms")
    runs = dict(m)
    runs["bf16 all"] = bf
    t = {label: {f: [] for f in figures} for label in runs}
    ref = None
    for rnd in range(ROUNDS + 1):  # round 0: warm-up, not recorded
        for label, mm in runs.items():
            ms = mm.time_prefill(toks, 0, mode="gemv") / (len(toks) / width)
            mm.set_logprobs(0)
            t0 = time.perf_counter()
            rec = mm.score(toks, 0)
            sc = (time.perf_counter() - t0) * 1e3
            mm.set_logprobs(None)
            if label != "bf16 all":
                ref = ref or rec["logprob"].tobytes()
                if rec["logprob"].tobytes() != ref:
                    raise SystemExit(f"{name}: score records of setting {label} differ from the first setting's")
            if rnd:
                t[label]["prefill/pass ms"].append(ms)
                t[label]["score64 ms"].append(sc)
    print(f"passes, {width} tokens per pass; score records equal over the {len(m)} fp16 settings: yes")
    print(f"{'passes on':10s}" + "".join(f"{f:>28s}" for f in figures))
    for label in runs:
        print(f"{label:10s}" + "".join("{:>17.3f} (range {:.3f})".format(*_med_range(t[label][f])) for f in figures))
    out = []
    for c in CLASSES:
        f = "score64 ms" if c == "cls" else "prefill/pass ms"
        (m0, r0), (m1, _) = _med_range(t["fp32"][f]), _med_range(t[c][f])
        keep = m1 < m0 - r0
        if not keep:
            out.append(c)
        print(f"{c:6s} {f}: fp32 {m0:.3f} (range {r0:.3f})  fp16 copy {m1:.3f}  {(m1 / m0 - 1) * 100:+6.1f} %   "
              f"{'adopt' if keep else 'LEAVE OUT (not below fp32 by more than its range)'}")
    print(f"pass classes the adoption rule leaves out for fp16: {','.join(out) if out else 'none'}")
    for f in figures:
        (a, ra), (b, rb) = _med_range(t["all"][f]), _med_range(t["bf16 all"][f])
        print(f"all five classes, {f}: fp16 copy {a:.3f}, bf16 copy {b:.3f}, difference {a - b:+.3f}: "
              f"{'inside' if abs(a - b) <= max(ra, rb) else 'OUTSIDE'} the ranges")
    for mm in [off, bf] + list(m.values()):
        mm.close()


def bench(lib, timeout=600):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "16", "--no-cpu-baseline"]
    env = dict(os.environ)
    if lib:
        env["KH_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py failed with library {lib or 'of this tree'} ({p.returncode}):\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="(internal) measure one model in this process and print its lines")
    ap.add_argument("--models", default="llama3.2-1b,tinyllama-1.1b,qwen2.5-0.5b,llama2-7b")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w16_f16_ab.txt"))
    a = ap.parse_args()
    if a.model:
        return one_model(a.model)
    lines = ["# tools/w16_f16_ab.py: the fp16 format of W16 (KH_FLAG_W16_F16) against fp32 and against the bf16 format, "
             "fp16-rounded synthetic images, one MI355X, one process per model", ""]

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
    if a.parent_lib:
        emit("# flag off against the parent commit: python bench.py --gpus 1 --steps 128 --warmup 16 --no-cpu-baseline, "
             "alternating fresh processes (the parent's library through KH_LIB), tok/s of Llama-3.2-1B fp32")
        old, new = [], []
        for r in range(a.rounds):
            old.append(bench(a.parent_lib))
            new.append(bench(None))
            emit(f"round {r + 1}: parent {old[-1]:.1f}  this tree {new[-1]:.1f}")
        spread = max(old + new) - min(old + new)
        d = statistics.median(new) - statistics.median(old)
        emit(f"median: parent {statistics.median(old):.1f}  this tree {statistics.median(new):.1f}  difference {d:+.1f} tok/s; "
             f"spread of the {2 * a.rounds} runs {spread:.1f}: {'inside' if abs(d) <= spread else 'OUTSIDE'} the spread")


if __name__ == "__main__":
    main()
