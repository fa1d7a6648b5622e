"""Timing of sequence scoring on the GEMM pass (kh_model_score_gemm, csrc/kh_score_gemm.h) for
profiles/score_gemm_ab.txt: a checkout of the parent commit (with its library built) against this tree, fresh processes
alternating on one GPU, median and range over the rounds.

    python tools/score_gemm_time.py --parent-tree DIR [--rounds 5] [--bench] > profiles/score_gemm_ab.txt

Per process and geometry (binfmt.PRESETS, synthetic weights): top_n 0 and 5, 128 / 512 / 2048 tokens at position 0 -
kh_model_score, kh_model_score_gemm (this tree only) and kh_model_prefill_gemm of the same tokens (the floor: what the
classifier tail costs is the difference), each a host clock around the call and a device synchronise, the median of 3
after a warm-up call; and kh_model_time_prefill of a 128-token GEMM prefill.  The operator alone (this tree): 512 tokens
on a 128 256 x 2048 classifier, top_n 5, with and without the one-workgroup-per-CU request (hook KH_PG_SOLO).
--bench: `python bench.py --gpus 1 --steps 128 --warmup 16 --no-cpu-baseline` in both trees as well.

    python tools/score_gemm_time.py --w16 --parent-tree DIR [--geoms llama3.2-1b,llama2-7b] > profiles/score_gemm_w16_ab.txt

--w16: the classifier on the bf16 matrix cores (csrc/kh_score_gemm_w16.h) instead of all the above.  Per process a
bf16-rounded synthetic image under KH_FLAG_W16 | KH_FLAG_GEMM16, created under KH_GEMM16_CLASSES=0xf (the classifier on
the fp32 image: the parent tree and this one) or 0x1f (k_pg_cls_lse_w16: this tree); kh_model_score_gemm of 128 / 512 /
2048 tokens, top_n 5, clocked as above.  One warm-up round, then --rounds rounds, the three variants alternating.
--w16-child GEOM MASK is one such process (what a kernel trace wraps)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = ("llama3.2-1b", "llama2-7b-int8")
LENS = (128, 512, 2048)
TOPS = (0, 5)

_CHILD = r"""
import ctypes as C, json, sys, time
import numpy as np, torch
from kuiperllama_amd import _ffi, binfmt
from kuiperllama_amd.model import KuiperModel
spec = binfmt.PRESETS[sys.argv[1]]
img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
torch.cuda.synchronize()
m = KuiperModel.from_device_image(img, spec, max_seq_len=2048)
L = _ffi.lib()
toks = [int(t) for t in np.random.default_rng(5).integers(0, spec.vocab_size, 2048)]
calls = [n for n in ("kh_model_score", "kh_model_score_gemm", "kh_model_prefill_gemm") if hasattr(L, n)]
out = {}
def clock(fn, n):
    t = (C.c_int32 * n)(*toks[:n])
    ms = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _ffi.check(fn(m._h, t, n, 0), "call")
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms[1:]))
for top in (0, 5):
    m.set_logprobs(top)
    for n in (128, 512, 2048):
        for name in calls:
            if name == "kh_model_prefill_gemm" and top:
                continue
            out[f"{name[9:]} n={n} top={top}"] = clock(getattr(L, name), n)
m.set_logprobs(None)
m.time_prefill(toks[:128], 0, "gemm")
out["time_prefill gemm n=128"] = float(np.median([m.time_prefill(toks[:128], 0, "gemm") for _ in range(5)]))
m.close()
print("RESULT " + json.dumps(out))
"""

_CHILD_W16 = r"""
import ctypes as C, json, sys, time
import numpy as np, torch
from kuiperllama_amd import _ffi, binfmt
from kuiperllama_amd.model import KuiperModel
spec = binfmt.PRESETS[sys.argv[1]]
img = binfmt.round_matrices_bf16(binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0")), spec)
torch.cuda.synchronize()
_ffi.debug_set("KH_GEMM16_CLASSES", sys.argv[2])
m = KuiperModel.from_device_image(img, spec, max_seq_len=2048, flags=_ffi.KH_FLAG_W16 | _ffi.KH_FLAG_GEMM16)
_ffi.debug_set("KH_GEMM16_CLASSES", None)
want = ["qkv", "wo", "ffn13", "w2"] + (["cls"] if int(sys.argv[2], 0) & 16 else [])
assert m.gemm16_info()["classes"] == want, m.gemm16_info()
toks = [int(t) for t in np.random.default_rng(5).integers(0, spec.vocab_size, 2048)]
m.set_logprobs(5)
out = {}
for n in (128, 512, 2048):
    t = (C.c_int32 * n)(*toks[:n])
    ms = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _ffi.check(_ffi.lib().kh_model_score_gemm(m._h, t, n, 0), "call")
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out[f"score_gemm n={n} top=5"] = float(np.median(ms[1:]))
    out[f"sum_logprob n={n}"] = float(np.nansum(m.logprobs(0, n)["logprob"]))
m.close()
print("RESULT " + json.dumps(out))
"""

_OP = r"""
import json, numpy as np, torch
from kuiperllama_amd import _ffi, ops
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(3)
w = torch.randn((128256, 2048), device=dev, generator=g) * 0.02
x = torch.randn((512, 2048), device=dev, generator=g)
tg = torch.randint(0, 128256, (512,), device=dev, dtype=torch.int32)
out = {}
for solo in ("1", "0", "1", "0"):
    _ffi.debug_set("KH_PG_SOLO", None if solo == "1" else "0")
    ops.cls_logprobs(w, x, tg, 5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(5):
        e0.record(); ops.cls_logprobs(w, x, tg, 5); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    out.setdefault("solo " + solo, []).append(float(np.median(ms)))
print("RESULT " + json.dumps(out))
"""


def run(tree, code, *args, timeout=900):
    r = subprocess.run([sys.executable, "-c", code, *args], cwd=tree, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=tree), timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])


def bench(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "128", "--warmup", "16", "--no-cpu-baseline"],
                       cwd=tree, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=tree), timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("{")))["value"]


def stat(v):
    return f"{np.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]"


def w16_ab(parent_tree, geoms, rounds):
    variants = (("0xf parent", parent_tree, "0xf"), ("0xf tree", ROOT, "0xf"), ("0x1f tree", ROOT, "0x1f"))
    print(f"score_gemm_w16_ab: kh_model_score_gemm, top_n 5, bf16-rounded synthetic images under KH_FLAG_W16 | KH_FLAG_GEMM16;\n"
          f"fresh processes, the variants alternating, one warm-up round and {rounds} rounds; ms per call, median [min .. max]\n"
          "0xf: the classifier on the fp32 image (k_pg_cls_lse); 0x1f: on the bf16 copy (k_pg_cls_lse_w16)\n"
          "NOT measured: real checkpoints, real text, fp16-format and int8 twins of the kernel", flush=True)
    for geom in geoms:
        res = {}
        for rnd in range(rounds + 1):
            for label, tree, mask in variants[::1 if rnd % 2 else -1]:  # no variant always runs behind the same one
                for k, v in run(tree, _CHILD_W16, geom, mask).items():
                    if rnd:
                        res.setdefault((k, label), []).append(v)
        print(f"\n## {geom}")
        for n in LENS:
            for label, _, _ in variants:
                print(f"score_gemm n={n:<5d} {label:11s} {stat(res[(f'score_gemm n={n} top=5', label)])}"
                      f"   sum of log-probs {res[(f'sum_logprob n={n}', label)][0]:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    if len(sys.argv) == 4 and sys.argv[1] == "--w16-child":
        sys.argv = [sys.argv[0]] + sys.argv[2:]
        sys.path.insert(0, ROOT)
        exec(_CHILD_W16, {"__name__": "__main__"})
        return
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-only", action="store_true")
    ap.add_argument("--w16", action="store_true")
    ap.add_argument("--geoms", default="llama3.2-1b,llama2-7b")
    a = ap.parse_args()
    if a.w16:
        return w16_ab(os.path.abspath(a.parent_tree), a.geoms.split(","), a.rounds)
    trees = (("parent", os.path.abspath(a.parent_tree)), ("tree", ROOT))
    print(f"score_gemm_ab: fresh processes, parent and tree alternating, {a.rounds} rounds; median [min .. max]\n"
          "synthetic weights (binfmt.synth_image), random token ids; NOT measured: real checkpoints, real text", flush=True)
    for geom in () if a.bench_only else GEOMS:
        res = {}
        for _ in range(a.rounds):
            for label, tree in trees:
                for k, v in run(tree, _CHILD, geom).items():
                    res.setdefault((k, label), []).append(v)
        print(f"\n## {geom}: ms per call")
        for k in sorted({k for k, _ in res}, key=lambda s: (s.split()[0], int(s.split("n=")[1].split()[0]), s)):
            for label, _ in trees:
                if (k, label) in res:
                    print(f"{k:32s} {label:6s} {stat(res[(k, label)])}", flush=True)
    op = {} if a.bench_only else run(ROOT, _OP)
    print("\n## operator alone, 512 tokens x 128256 x 2048 fp32, top_n 5: ms (k_cls_pack + k_pg_cls_lse + k_pg_lse_merge), "
          "two alternating blocks of 5 each")
    for k, v in op.items():
        print(f"{k}: {v}")
    if a.bench or a.bench_only:
        vals = {}
        for _ in range(a.rounds):
            for label, tree in trees:
                vals.setdefault(label, []).append(bench(tree))
        print("\n## python bench.py --gpus 1 --steps 128 --warmup 16 --no-cpu-baseline: decode tok/s")
        for label, _ in trees:
            print(f"{label:6s} {stat(vals[label])}", flush=True)


if __name__ == "__main__":
    main()
