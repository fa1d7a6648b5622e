#!/usr/bin/env python3
"""Same-box A/B of KH_FLAG_WIDE_ATTN (csrc/kh_seq_attn_wide.h): the wide pass's attention as k_sg_attn + k_sg_attn_merge
per layer against the grouped k_seq_attn launches.  Output: profiles/wide_attn_ab.txt.

    python tools/wide_attn_ab.py ab [--model llama3.2-1b] [--cases a,b] [--reps 5] [--out FILE]
    KH_LIB=<another build> python tools/wide_attn_ab.py ab --cases a      # a library without the flag: "off" rows only
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/wide_attn_ab.py pass
    python tools/wide_attn_ab.py table DIR/.../*_kernel_trace.csv

ab:    two models on one synthetic device image, flag off and flag on, in ONE process; the rows alternate within a
       repetition, the first repetition warms up; median and range of `--reps` runs of the call's own elapsed_ms.
       a: generate_batch(gemm=True), 64 and 16 sequences, 32-token prompts cached, 128 sampled steps, no sharing (the case
          of tools/seq_gemm_ab.py);
       b: best_of(n=64, share=True, gemm=True)'s batched loop over prompts of 512 / 2048 / 8192 tokens, 32 sampled steps:
          slot 0 is prefilled (not timed), 63 slots share its rows.
pass:  32 wide passes of 64 lanes at positions 32 .. 63 under the flag (for a kernel trace); table: the trace by class."""
import argparse
import csv
import dataclasses
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMP = dict(temperature=0.8, top_k=50, top_p=0.95)
PROMPT, STEPS, SHARE_STEPS, CACHE = 32, 128, 32, 64 * 192


def _models(name, cache):
    import torch
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    spec = dataclasses.replace(binfmt.PRESETS[name], seq_len=cache)
    img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    flags = {"off": 0}
    if hasattr(_ffi, "KH_FLAG_WIDE_ATTN"):
        flags["on"] = _ffi.KH_FLAG_WIDE_ATTN
    return spec, {k: KuiperModel.from_device_image(img, spec, max_seq_len=cache, flags=f) for k, f in flags.items()}


def _measure(models, run, reps):
    """run(model) -> elapsed ms; alternated, the first repetition warms up: {key: (median, min, max)}"""
    t = {k: [] for k in models}
    for rep in range(reps + 1):
        for k, m in models.items():
            ms = run(m)
            if rep:
                t[k].append(ms)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def _row(label, steps, n, res):
    cols = "   ".join(f"{k} {v[0] / steps:7.3f} ms/step ({v[1] / steps:.3f} .. {v[2] / steps:.3f}), "
                      f"{n * steps / v[0] * 1e3:7.0f} tok/s" for k, v in res.items())
    gain = f"   on/off {res['on'][0] / res['off'][0]:.3f}" if "on" in res else ""
    return f"{label:28s} {cols}{gain}"


def ab(args):
    from kuiperllama_amd.model import plan_shared_layout
    out = [f"# tools/wide_attn_ab.py ab: {args.model}, library {os.environ.get('KH_LIB', 'this tree')}, median (min .. max) "
           f"of {args.reps} alternated runs, one MI355X"]
    print(out[0], flush=True)
    rng = np.random.default_rng(0)

    def emit(line):
        out.append(line)
        print(line, flush=True)

    if "a" in args.cases:
        spec, models = _models(args.model, CACHE)
        prompts = [[int(t) for t in rng.integers(0, spec.vocab_size, PROMPT)] for _ in range(64)]
        for m in models.values():
            m.seq_slots(64)
            for s in range(64):
                m.seq_prefill(s, prompts[s][:-1])
        sp = [dict(SAMP, seed=100 + s) for s in range(64)]
        total = PROMPT - 1 + STEPS
        for n in (64, 16):
            res = _measure(models, lambda m: m.generate_batch(prompts[:n], total, sp[:n], cached=[PROMPT - 1] * n,
                                                              gemm=True)[1], args.reps)
            emit(_row(f"a: {n} sequences, no sharing", STEPS, n, res))
        for m in models.values():
            m.close()
    if "b" in args.cases:
        for P in (512, 2048, 8192):
            total = P - 1 + SHARE_STEPS
            spec, models = _models(args.model, P + 64 * (SHARE_STEPS + 8))
            prompt = [int(t) for t in rng.integers(0, spec.vocab_size, P)]
            for m in models.values():
                m.seq_slots_var(plan_shared_layout(int(m.cfg.cache_len), 64, P - 1, total))
                m.seq_prefill(0, prompt[:-1], gemm=True)
                for s in range(1, 64):
                    m.seq_share(0, s, P - 1)
            sp = [dict(SAMP, seed=7 + s) for s in range(64)]
            res = _measure(models, lambda m: m.generate_batch([prompt] * 64, total, sp, cached=[P - 1] * 64, gemm=True)[1],
                           args.reps)
            emit(_row(f"b: best_of 64, shared prompt {P}", SHARE_STEPS, 64, res))
            for m in models.values():
                m.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(out) + "\n\n")


def one_pass(args):
    spec, models = _models(args.model, CACHE)
    m = models["on"]
    m.seq_slots(64)
    rng = np.random.default_rng(0)
    for s in range(64):
        m.seq_prefill(s, [int(t) for t in rng.integers(0, spec.vocab_size, PROMPT)])
    toks, sp = [1] * 64, [dict(SAMP, seed=s) for s in range(64)]
    for p in range(PROMPT, PROMPT + 32):
        toks = m.seq_step(list(range(64)), toks, [p] * 64, samplings=sp, gemm=True)


CLASSES = (("k_sg_gemm", "GEMMs (QKV, wo, SwiGLU, w2)"), ("k_sg_attn_merge", "attention merge"),
           ("k_sg_attn", "attention (one launch)"), ("k_seq_attn", "grouped attention"), ("k_seq_pick", "grouped tail"),
           ("k_seq_tail", "grouped tail"), ("k_pg_rmsnorm", "RMSNorm"), ("k_sg_", "embed / RoPE"))


def table(path, out):
    tot, cnt, passes = {}, {}, 0
    with open(path) as f:
        for r in csv.DictReader(f):
            nm = re.sub(r"\(.*$", "", re.sub(r"^void ", "", r["Kernel_Name"]))
            cls = next((c for k, c in CLASSES if nm.startswith(k)), None)
            if nm.startswith("k_sg_gemm") and re.search(r",\s*3>", nm):
                cls = "classifier GEMM"
            passes += nm.startswith("k_sg_embed")
            if cls is None:
                continue
            tot[cls] = tot.get(cls, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            cnt[cls] = cnt.get(cls, 0) + 1
    lines = [f"# tools/wide_attn_ab.py table: kernel time of {passes} wide passes of 64 lanes under KH_FLAG_WIDE_ATTN by "
             "launch class (rocprofv3 --kernel-trace)", f"{'class':32s} {'launches/pass':>13s} {'us/pass':>9s} {'share':>6s}"]
    allus = sum(tot.values())
    for c in sorted(tot, key=tot.get, reverse=True):
        lines.append(f"{c:32s} {cnt[c] / passes:13.1f} {tot[c] / passes:9.1f} {100 * tot[c] / allus:5.1f}%")
    lines.append(f"{'sum of kernel time':32s} {sum(cnt.values()) / passes:13.1f} {allus / passes:9.1f}")
    print("\n".join(lines))
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab", "pass", "table"])
    ap.add_argument("arg", nargs="?")
    ap.add_argument("--model", default="llama3.2-1b")
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"ab": ab, "pass": one_pass, "table": lambda x: table(x.arg, x.out)}[a.mode](a)
