"""Same-box A/B of KH_FLAG_GEMM16_Q8 (csrc/kh_gemm_q16.h): the GEMM pass of an int8 group-64 model on the bf16 matrix cores
from its int8 image, against the same model on the fp32 matrix cores (the twin of tools/gemm16_ab.py).

    python tools/gemm16_q8_ab.py [--models llama2-7b-int8,tinyllama-1.1b-int8]
                                 [--tree LABEL=PATH ...] [--out profiles/gemm16_q8_ab.txt]

One process per model (this script re-invoked with --model) on a synthetic int8 group-64 image of the BASELINE geometry
(tinyllama-1.1b-int8: TinyLlama's geometry, quantised); every model of the process shares the device image.  Settings:
flag off; flag on with every class (hook KH_GEMM16_Q8_CLASSES=0x1f); flag on with the default mask; and each single
class (0x1 qkv, 0x2 wo, 0x4 ffn13, 0x8 w2, 0x10 cls), alternated ROUNDS times behind one warm-up round.  Figures, median
and range over the rounds:
  * kh_model_time_prefill (mode gemm) of 128 and of 512 prompt tokens, as prompt tok/s and ms;
  * seq_prefill_many of 64 x 32 tokens (wall clock around the call and a device synchronise);
  * generate_batch(gemm=True) of 16 and of 64 sequences, 24 sampled steps: the call's own elapsed_ms.
Per-class times: a single-class model differs from the flag-off model in that class's GEMMs alone, so the difference
of their 512-token prefill times (cls: of their 64-sequence batches; a prefill runs no classifier) is the class's.
Adoption rule: a class joins the default mask if its single-class median lies below the flag-off median
by more than the range of the flag-off runs, on both geometries.
--tree (repeatable): another checkout of the project to measure beside this one, e.g. the parent commit with its own
library built; a tree without the flag measures the flag-off row only.  That row of this tree must match it."""
import argparse
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


def _med_range(v):
    return statistics.median(v), max(v) - min(v)


def one_model(name, tree):
    import torch
    sys.path.insert(0, tree)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    import dataclasses
    has_flag = hasattr(_ffi, "KH_FLAG_GEMM16_Q8")
    spec = binfmt.PRESETS.get(name) or dataclasses.replace(binfmt.PRESETS[name[:-len("-int8")]], quant=True,
                                                           group_size=64, name=name)
    assert spec.quant and spec.group_size == 64, spec
    dev = torch.device("cuda:0")
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    m = {}
    for hook, label in SETTINGS if has_flag else SETTINGS[:1]:
        flags = 0
        if hook is not None:
            flags |= _ffi.KH_FLAG_GEMM16_Q8
            _ffi.debug_set("KH_GEMM16_Q8_CLASSES", None if hook == "default" else hook)
        m[label] = KuiperModel.from_device_image(img, spec, max_seq_len=2048, flags=flags)
    if has_flag:
        _ffi.debug_set("KH_GEMM16_Q8_CLASSES", None)
    print(f"## {name}: dim {spec.dim} hidden {spec.hidden_dim} layers {spec.n_layers} vocab {spec.vocab_size}"
          + (f"; default mask {','.join(m['default'].gemm16_q8_info()['classes']) or 'none'}; under 0x1f: "
             f"{','.join(m['all'].gemm16_q8_info()['classes'])}" if has_flag else "; this tree has no KH_FLAG_GEMM16_Q8"))
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
    ran = m["all"].gemm16_q8_info()["classes"]
    for c in ("qkv", "wo", "ffn13", "w2", "cls"):
        f = "batch64 ms" if c == "cls" else "prefill512 ms"
        (m0, r0), (m1, r1) = _med_range(t["off"][f]), _med_range(t[c][f])
        if c not in ran:
            print(f"{c:6s} keeps its int8 kernel on this geometry")
            continue
        print(f"{c:6s} {f}: off {m0:.3f} (range {r0:.3f})  class on {m1:.3f} (range {r1:.3f})  {m1 - m0:+.3f} ms "
              f"({(m1 / m0 - 1) * 100:+.1f} %)  {'passes' if m1 < m0 - r0 else 'FAILS (not below flag-off by more than its range)'}")
    for mm in m.values():
        mm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="(internal) measure one model in this process and print its lines")
    ap.add_argument("--models", default="llama2-7b-int8,tinyllama-1.1b-int8")
    ap.add_argument("--tree", action="append", default=[], help="LABEL=PATH of another checkout to measure too")
    ap.add_argument("--this-tree", default=ROOT, help="(internal) the checkout --model measures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm16_q8_ab.txt"))
    a = ap.parse_args()
    if a.model:
        return one_model(a.model, a.this_tree)
    lines = ["# tools/gemm16_q8_ab.py: the GEMM pass of int8 group-64 models on the bf16 matrix cores (KH_FLAG_GEMM16_Q8) "
             "against the fp32 matrix cores, synthetic int8 images, one MI355X, one process per model and tree", ""]

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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", name, "--this-tree",
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
