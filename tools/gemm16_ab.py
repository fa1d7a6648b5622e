"""Same-box A/B of the GEMM pass on the bf16 matrix cores against the same model on the fp32 matrix cores, one core per
run: w16 - KH_FLAG_GEMM16 (csrc/kh_gemm_w16.h), a W16 model from its bf16-format copy; h16 - KH_FLAG_GEMM16_F16
(csrc/kh_gemm_h16.h), an fp16-origin fp32 model from its fp16-format copy; q16 - KH_FLAG_GEMM16_Q8 (csrc/kh_gemm_q16.h),
an int8 group-64 model from its int8 image.

    python tools/gemm16_ab.py [--core w16|h16|q16] [--models NAME,...] [--tree LABEL=PATH ...] [--out FILE]

--models and --out default per core (CORES below): the BASELINE geometries the core was measured on, and
profiles/gemm16_ab.txt, profiles/gemm16_f16_ab.txt, profiles/gemm16_q8_ab.txt.  A q16 model name ending in -int8 that is
no preset is that preset's geometry, quantised.

One process per model (this script re-invoked with --model) on a synthetic image of the geometry made exact for the core
(matrices rounded to bf16 / to fp16 / int8 as synthesised); every model of the process has the copy's flag on (w16:
KH_FLAG_W16, h16: KH_FLAG_W16_F16) and shares the device image.  Settings: flag off; flag on with every class (the core's
class-mask hook = 0x1f); flag on with the default mask; and each single class (0x1 qkv, 0x2 wo, 0x4 ffn13, 0x8 w2,
0x10 cls), alternated ROUNDS times behind one warm-up round.  Figures, median and range over the rounds:
  * kh_model_time_prefill (mode gemm) of 128 and of 512 prompt tokens, as prompt tok/s and ms;
  * seq_prefill_many of 64 x 32 tokens (wall clock around the call and a device synchronise);
  * generate_batch(gemm=True) of 16 and of 64 sequences, 24 sampled steps: the call's own elapsed_ms.
Per-class times: a single-class model differs from the flag-off model in that class's GEMMs alone, so the difference
of their 512-token prefill times (cls: of their 64-sequence batches; a prefill runs no classifier) is the class's.
Adoption rule (3.1g for h16, 3.1f for q16): a class joins the default mask if its single-class median lies
below the flag-off median by more than the range of the flag-off runs, on every geometry measured (w16: on llama3.2-1b
and on llama2-7b).
--tree (repeatable): another checkout of the project to measure beside this one, e.g. the parent commit with its own
library built; a tree without the flag measures the flag-off row only.  That row of this tree must match it."""
import argparse
import dataclasses
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = ((None, "off"), ("0x1f", "all"), ("default", "default"), ("0x1", "qkv"), ("0x2", "wo"), ("0x4", "ffn13"),
            ("0x8", "w2"), ("0x10", "cls"))
ROUNDS = 5
FIGURES = ("prefill128 ms", "prefill512 ms", "slots 64x32 ms", "batch16 ms", "batch64 ms")
STEPS = 24
# core -> what differs: the flag and the copy's flag beside it (names in _ffi), how the image is made exact (binfmt), the
# class-mask hook, the info method, the default --models and --out, the header's two phrases, and three phrases of the lines
CORES = {
    "w16": dict(flag="KH_FLAG_GEMM16", copy_flag="KH_FLAG_W16", make_exact="round_matrices_bf16", hook="KH_GEMM16_CLASSES",
                info="gemm16_info", models="llama3.2-1b,tinyllama-1.1b,qwen2.5-0.5b,llama2-7b", out="gemm16_ab.txt",
                header=("W16 models", "bf16-rounded synthetic images"), ran="classes with K % 32 == 0",
                keeps="keeps its fp32 kernel on this geometry (K % 32)"),
    "h16": dict(flag="KH_FLAG_GEMM16_F16", copy_flag="KH_FLAG_W16_F16", make_exact="round_matrices_fp16",
                hook="KH_GEMM16_F16_CLASSES", info="gemm16_f16_info", models="llama3.2-1b,tinyllama-1.1b,llama2-7b",
                out="gemm16_f16_ab.txt", header=("fp16-origin models", "fp16-rounded synthetic images"),
                ran="classes with K % 32 == 0", keeps="keeps its fp32 kernel on this geometry (K % 32)"),
    "q16": dict(flag="KH_FLAG_GEMM16_Q8", copy_flag=None, make_exact=None, hook="KH_GEMM16_Q8_CLASSES",
                info="gemm16_q8_info", models="llama2-7b-int8,tinyllama-1.1b-int8", out="gemm16_q8_ab.txt",
                header=("int8 group-64 models", "synthetic int8 images"), ran="under 0x1f",
                keeps="keeps its int8 kernel on this geometry"),
}


def _med_range(v):
    return statistics.median(v), max(v) - min(v)


def one_model(core, name, tree):
    import torch
    sys.path.insert(0, tree)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    c = CORES[core]
    has_flag = hasattr(_ffi, c["flag"])
    spec = binfmt.PRESETS.get(name)
    if core == "q16":
        spec = spec or dataclasses.replace(binfmt.PRESETS[name[:-len("-int8")]], quant=True, group_size=64, name=name)
        assert spec.quant and spec.group_size == 64, spec
    dev = torch.device("cuda:0")
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    if c["make_exact"]:
        img = getattr(binfmt, c["make_exact"])(img, spec)
    torch.cuda.synchronize()
    m = {}
    for hook, label in SETTINGS if has_flag else SETTINGS[:1]:
        flags = getattr(_ffi, c["copy_flag"]) if c["copy_flag"] else 0
        if hook is not None:
            flags |= getattr(_ffi, c["flag"])
            _ffi.debug_set(c["hook"], None if hook == "default" else hook)
        m[label] = KuiperModel.from_device_image(img, spec, max_seq_len=2048, flags=flags)
    if has_flag:
        _ffi.debug_set(c["hook"], None)
    if core == "w16":
        assert m["off"].w16_info()["state"] == 1, m["off"].w16_info()
    if core == "h16":
        assert m["off"].w16_format()["format"] == "fp16", m["off"].w16_format()
    info = {label: getattr(mm, c["info"]) for label, mm in m.items()} if has_flag else {}
    print(f"## {name}: dim {spec.dim} hidden {spec.hidden_dim} layers {spec.n_layers} vocab {spec.vocab_size}"
          + (f"; default mask {','.join(info['default']()['classes']) or 'none'}; {c['ran']}: "
             f"{','.join(info['all']()['classes'])}" if has_flag else f"; this tree has no {c['flag']}"))
    toks = [1] + [(263 + 7 * i) % spec.vocab_size for i in range(511)]
    segs = [[(11 + 5 * s + 3 * i) % spec.vocab_size for i in range(32)] for s in range(64)]
    prompts = [[1, 263 + s] for s in range(64)]
    t = {label: {f: [] for f in FIGURES} for label in m}
    for mm in m.values():
        mm.seq_slots(64)
    for rnd in range(ROUNDS + 1):  # round 0: warm-up, not recorded
        for label, mm in m.items():
            p128 = mm.time_prefill(toks[:128], 0, mode="gemm")
            p512 = mm.time_prefill(toks, 0, mode="gemm")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mm.seq_prefill_many(list(range(64)), segs)
            torch.cuda.synchronize()
            sl = (time.perf_counter() - t0) * 1e3
            _, b16 = mm.generate_batch(prompts[:16], STEPS + 1, gemm=True)
            _, b64 = mm.generate_batch(prompts, STEPS + 1, gemm=True)
            if rnd:
                for f, v in zip(FIGURES, (p128, p512, sl, b16, b64)):
                    t[label][f].append(v)
    print(f"{'setting':8s}" + "".join(f"{f:>27s}" for f in FIGURES) + f"{'prompt tok/s 128 / 512':>26s}")
    for label in m:
        a, b = statistics.median(t[label][FIGURES[0]]), statistics.median(t[label][FIGURES[1]])
        print(f"{label:8s}" + "".join("{:>16.3f} (range {:.3f})".format(*_med_range(t[label][f])) for f in FIGURES)
              + f"{128e3 / a:>14.0f} /{512e3 / b:>9.0f}")
    if not has_flag:
        return
    for f in FIGURES:
        off = statistics.median(t["off"][f])
        print(f"{f}: off / all {off / statistics.median(t['all'][f]):.2f} x, off / default "
              f"{off / statistics.median(t['default'][f]):.2f} x")
    print("per-class time with the flag off -> on (difference to the flag-off model), and the adoption rule:")
    ran = info["all"]()["classes"]
    for cl in ("qkv", "wo", "ffn13", "w2", "cls"):
        f = "batch64 ms" if cl == "cls" else "prefill512 ms"
        (m0, r0), (m1, r1) = _med_range(t["off"][f]), _med_range(t[cl][f])
        if cl not in ran:
            print(f"{cl:6s} {c['keeps']}")
            continue
        print(f"{cl:6s} {f}: off {m0:.3f} (range {r0:.3f})  class on {m1:.3f} (range {r1:.3f})  {m1 - m0:+.3f} ms "
              f"({(m1 / m0 - 1) * 100:+.1f} %)  {'passes' if m1 < m0 - r0 else 'FAILS (not below flag-off by more than its range)'}")
    for mm in m.values():
        mm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="(internal) measure one model in this process and print its lines")
    ap.add_argument("--core", choices=sorted(CORES), default="w16")
    ap.add_argument("--models", help="default: the core's (CORES)")
    ap.add_argument("--tree", action="append", default=[], help="LABEL=PATH of another checkout to measure too")
    ap.add_argument("--this-tree", default=ROOT, help="(internal) the checkout --model measures")
    ap.add_argument("--out", help="default: the core's file under profiles/ (CORES)")
    a = ap.parse_args()
    if a.model:
        return one_model(a.core, a.model, a.this_tree)
    c = CORES[a.core]
    a.models = a.models if a.models is not None else c["models"]
    a.out = a.out or os.path.join(ROOT, "profiles", c["out"])
    lines = [f"# tools/gemm16_ab.py --core {a.core}: the GEMM pass of {c['header'][0]} on the bf16 matrix cores ({c['flag']}) "
             f"against the fp32 matrix cores, {c['header'][1]}, one MI355X, one process per model and tree", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    trees = [tuple(x.split("=", 1)) for x in a.tree] + [("this tree", ROOT)]
    for name in [n for n in a.models.split(",") if n]:
        for label, path in trees:
            emit(f"# ---- {label}")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--core", a.core, "--model", name, "--this-tree",
                                os.path.abspath(path)], capture_output=True, text=True, timeout=900,
                               cwd=os.path.abspath(path))
            for s in p.stdout.splitlines():
                emit(s)
            if p.returncode != 0:  # nothing more is started on the device behind a process that failed
                emit(f"## {name}: not measured (exit {p.returncode}): {p.stderr.strip().splitlines()[-1:] or ''}")
                return p.returncode
            emit("")


if __name__ == "__main__":
    sys.exit(main())
