"""Same-box A/B of the B-token passes of Q4 models (kh_q4_pass.h): prefill, score, generate_batch and generate_lookup of
a KH_FLAG_Q4 model with its passes on the packed 4-bit copy against the same model with its passes on the int8 matrices.

    python tools/q4_pass_ab.py [--models llama2-7b-int8,tinyllama-1.1b-int8] [--lib LABEL=PATH ...]
                               [--out profiles/q4_pass_ab.txt] [--parent-lib PATH [--rounds 3]]

One process per model (this script re-invoked with --model) on a synthetic image of the geometry, requantised to 4 bits
(binfmt.requantize_matrices_q4; the geometries of tools/q4_ab.py); every model of the process has the flag on and shares
the device image.  One model per setting of the hook KH_Q4_PASS (read at creation): 0 (passes on int8), 0x1f (all five
classes) and each single class (0x1 qkv, 0x2 wo, 0x4 ffn13, 0x8 w2, 0x10 cls), alternated five times.  Figures, median
and range of the five:
  * kh_model_time_prefill (the B-token kernels) of 64 tokens, per pass;
  * score of 64 tokens with log-probs of the fed tokens only (wall clock around the call);
  * generate_batch at full width, 128 steps: the call's own elapsed_ms;
  * generate_lookup of 128 words with the truth as hint: the call's own elapsed_ms.
The words of every row of a case must be equal, or the script stops.
Adoption rule, per class: its pass stays on the copy only if its median lies below the KH_Q4_PASS=0
median by more than the range of those runs - on the prefill pass for qkv, wo, ffn13 and w2, on score for cls (a
prefill runs no classifier) - on every measured geometry.  KH_Q4_PASS_DEFAULT (kh_model_internal.h) is that set.
--lib (repeatable): the builds of the library to measure, this tree's when none is given (kuiperllama_amd/build.py
--variant NAME KH_PF_U_Q4=4 -> kuiperllama_amd/lib/NAME.so): how KH_PF_U_Q4 was chosen.
--parent-lib: a build of the parent commit's sources (build.py --variant-at <commit> NAME); `python bench.py --gpus 1
--steps 128 --warmup 16 --no-cpu-baseline` with KH_LIB on it and on this tree's library, alternating fresh processes:
decode, which this change does not touch, against the commit before it.
Not measurable here: anything on real checkpoints, and model quality at 4 bits with symmetric groups."""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("qkv", "wo", "ffn13", "w2", "cls")
SETTINGS = (("0", "int8"), ("0x1f", "all"), ("0x1", "qkv"), ("0x2", "wo"), ("0x4", "ffn13"), ("0x8", "w2"), ("0x10", "cls"))
ROUNDS = 5
FIGURES = ("prefill/pass ms", "score64 ms", "batch128 ms", "lookup128 ms")


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
    m = {}
    for hook, label in SETTINGS:
        _ffi.debug_set("KH_Q4_PASS", hook)
        m[label] = KuiperModel.from_device_image(img, spec, max_seq_len=2048, flags=_ffi.KH_FLAG_Q4)
    _ffi.debug_set("KH_Q4_PASS", None)
    info = m["all"].q4_info()
    assert info["state"] == 1, info
    md = KuiperModel.from_device_image(img, spec, max_seq_len=2048, flags=_ffi.KH_FLAG_Q4)  # no hook: the default mask
    default = md.q4_pass_info()["classes"]
    md.close()
    width = m["int8"].seq_width()
    print(f"## {name}: dim {spec.dim} hidden {spec.hidden_dim} layers {spec.n_layers} vocab {spec.vocab_size} group "
          f"{spec.group_size}; {width} tokens per pass; decode classes {','.join(info['classes']) or 'none'}; default pass "
          f"mask {','.join(default) or 'none'}")
    for label in m:
        want = {"int8": [], "all": list(CLASSES)}.get(label, [label])
        assert m[label].q4_pass_info()["classes"] == want, (label, m[label].q4_pass_info())
    toks = [1] + [263 + 7 * i for i in range(63)]
    prompts = [[1, 263 + s] for s in range(width)]
    truth, _ = m["int8"].generate([1, 263], 129)
    t = {label: {f: [] for f in FIGURES} for label in m}
    words = {}

    def same(case, label, w):
        if words.setdefault(case, w) != w:
            raise SystemExit(f"{name}: {case} words of setting {label} differ from the first setting's")

    for mm in m.values():
        mm.seq_slots(width)
    for rnd in range(ROUNDS + 1):  # round 0: warm-up, not recorded
        for label, mm in m.items():
            ms = mm.time_prefill(toks, 0, mode="gemv") / (len(toks) / width)
            mm.set_logprobs(0)
            t0 = time.perf_counter()
            rec = mm.score(toks, 0)
            sc = (time.perf_counter() - t0) * 1e3
            mm.set_logprobs(None)
            same("score", label, rec["logprob"].tobytes())
            bw, bms = mm.generate_batch(prompts, 129)
            same("generate_batch", label, bw)
            lw, lms, stats = mm.generate_lookup([1, 263], 129, hint=truth)
            same("generate_lookup", label, (lw, stats["accepted"]))
            assert lw == truth
            if rnd:
                for f, v in zip(FIGURES, (ms, sc, bms, lms)):
                    t[label][f].append(v)
    print(f"words of score, generate_batch and generate_lookup equal over the {len(m)} settings: yes")
    print(f"{'passes on':10s}" + "".join(f"{f:>28s}" for f in FIGURES))
    for label in m:
        print(f"{label:10s}" + "".join("{:>17.3f} (range {:.3f})".format(*_med_range(t[label][f])) for f in FIGURES))
    keep = []
    for c in CLASSES:
        f = "score64 ms" if c == "cls" else "prefill/pass ms"
        (m0, r0), (m1, _) = _med_range(t["int8"][f]), _med_range(t[c][f])
        if m1 < m0 - r0:
            keep.append(c)
        print(f"{c:6s} {f}: int8 {m0:.3f} (range {r0:.3f})  copy {m1:.3f}  {(m1 / m0 - 1) * 100:+6.1f} %   "
              f"{'adopt' if c in keep else 'LEAVE OUT (not below int8 by more than its range)'}")
    print(f"classes the adoption rule keeps on this geometry: {','.join(keep) if keep else 'none'}")
    for f in FIGURES:
        print(f"all vs int8, {f}: {(statistics.median(t['all'][f]) / statistics.median(t['int8'][f]) - 1) * 100:+.1f} %")
    for mm in m.values():
        mm.close()


def bench(lib, timeout=900):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "16", "--no-cpu-baseline"]
    env = dict(os.environ)
    if lib:
        env["KH_LIB"] = os.path.abspath(lib)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    if p.returncode != 0:
        raise RuntimeError(f"bench.py failed with KH_LIB={lib!r} ({p.returncode}):\n{p.stderr[-2000:]}")
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return line["value"], line.get("secondary_value")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="(internal) measure one model in this process and print its lines")
    ap.add_argument("--models", default="llama2-7b-int8,tinyllama-1.1b-int8")
    ap.add_argument("--lib", action="append", default=[], help="LABEL=PATH of a build of the library (PATH empty: this tree's)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q4_pass_ab.txt"))
    a = ap.parse_args()
    if a.model:
        return one_model(a.model)
    lines = ["# tools/q4_pass_ab.py: the B-token passes of Q4 models on the 4-bit copy against int8, requantised synthetic "
             "images, one MI355X, one process per model, flag on throughout", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    libs = [tuple(x.rsplit("=", 1)) for x in a.lib] or [("this build", "")]  # an empty PATH: the tree's own library
    for label, path in libs:
        emit(f"# ---- library: {label}")
        env = dict(os.environ)
        if path:
            env["KH_LIB"] = os.path.abspath(path)
        for name in [n for n in a.models.split(",") if n]:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", name], capture_output=True,
                               text=True, timeout=900, env=env)
            for s in p.stdout.splitlines():
                emit(s)
            if p.returncode != 0:
                emit(f"## {name}: not measured (exit {p.returncode}): {p.stderr.strip().splitlines()[-1:] or ''}")
            emit("")
    if a.parent_lib:
        emit("# decode against the parent commit's library: python bench.py --gpus 1 --steps 128 --warmup 16 "
             "--no-cpu-baseline, alternating fresh processes, tok/s of the flagship (Llama-3.2-1B fp32) and of the int8 "
             "secondary (Llama-2-7B int8)")
        old, new = [], []
        for r in range(a.rounds):
            old.append(bench(a.parent_lib))
            new.append(bench(None))
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
