#!/usr/bin/env python3
"""The wide sequence pass (csrc/kh_seq_gemm.h: up to 64 sequences per sweep of the weights, GEMMs on the matrix cores)
against the 8-lane pass, and where a wide pass spends its time.  Output: profiles/seq_gemm_ab.txt.

    python -m kuiperllama_amd.build --variant-at <parent commit> parent      # the baseline library, where git is
    python tools/seq_gemm_ab.py ab --baseline-lib kuiperllama_amd/lib/parent.so [--out FILE] [--cases a,b] [--reps 5]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/seq_gemm_ab.py pass <preset>
    python tools/seq_gemm_ab.py table DIR/.../*_kernel_trace.csv
    python tools/seq_gemm_ab.py prefill --baseline-lib kuiperllama_amd/lib/parent.so

ab:      per geometry (synthetic image) and n_seq in 8 / 16 / 32 / 64: prompts of 32 tokens, cached (seq_prefill, not
         timed), 128 sampled steps (temperature 0.8, top-k 50, top-p 0.95, seeds s, s + 1, ..); generate_batch(gemm=True)
         of this tree against kh_model_generate_batch_from of the baseline library on the same device image, both in ONE
         process, the rows alternating within a repetition; median of `--reps` runs of the call's own elapsed_ms (HIP
         events on the model stream).  ms per step = elapsed / 128 (a step = every sequence advanced once: one wide
         pass, n_seq / width 8-lane passes); tok/s = n_seq x 128 / elapsed.
pass:    32 wide passes of 64 lanes at positions 32 .. 63 (for a kernel trace); table: the trace by launch class.
prefill: kh_model_time_prefill of a 128-token prefill_gemm, baseline library against this tree, alternating (the
         statements of k_pg_gemm moved into csrc/kh_gemm_body.h)."""
import argparse
import csv
import ctypes as C
import dataclasses
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMP = dict(temperature=0.8, top_k=50, top_p=0.95)
PRESETS = ["llama3.2-1b", "tinyllama-1.1b", "qwen2.5-0.5b", "llama2-7b-int8"]
PROMPT, STEPS, CACHE = 32, 128, 64 * 192


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


class Baseline:
    """another build of the library on the same device image (ctypes): the 8-lane batched loop and the GEMM prefill"""

    def __init__(self, lib_path, image, spec, max_seq_len):
        from kuiperllama_amd import _ffi
        self.ffi, self.L = _ffi, C.CDLL(lib_path)
        L, i32, p32 = self.L, C.c_int32, C.POINTER(C.c_int32)
        L.kh_model_create_from_device_weights.argtypes = [p32, C.c_void_p, C.c_size_t, C.POINTER(_ffi.ModelOpts),
                                                          C.POINTER(C.c_void_p)]
        L.kh_model_seq_slots.argtypes = [C.c_void_p, i32, p32]
        L.kh_model_seq_prefill.argtypes = [C.c_void_p, i32, p32, i32, i32]
        L.kh_model_generate_batch_from.argtypes = [C.c_void_p, i32, p32, p32, p32, p32, C.POINTER(_ffi.Sampling), p32,
                                                   i32, p32, i32, p32, C.POINTER(C.c_float)]
        L.kh_model_time_prefill.argtypes = [C.c_void_p, p32, i32, i32, i32, C.POINTER(C.c_float)]
        L.kh_model_destroy.argtypes = [C.c_void_p]
        L.kh_model_destroy.restype = None
        hb = spec.header_bytes()
        weights = image[hb:]
        assert weights.data_ptr() % 16 == 0
        header = np.frombuffer(image[:32].cpu().numpy().tobytes(), dtype=np.int32)
        o = _ffi.ModelOpts(spec.family, int(spec.quant), spec.rope_mode, spec.rope_theta, spec.rms_eps, max_seq_len, 0, 0)
        self.h = C.c_void_p()
        rc = L.kh_model_create_from_device_weights(_i32(header.tolist()[:8]), weights.data_ptr(), weights.numel(),
                                                   C.byref(o), C.byref(self.h))
        assert rc == 0, rc
        self._keep = image

    def seq_slots(self, n):
        out = C.c_int32(0)
        assert self.L.kh_model_seq_slots(self.h, n, C.byref(out)) == 0
        return out.value

    def seq_prefill(self, slot, toks):
        assert self.L.kh_model_seq_prefill(self.h, slot, _i32(toks), len(toks), 0) == 0

    def generate_batch(self, prompts, total, samplings, cached):
        n = len(prompts)
        sp = (self.ffi.Sampling * n)(*[self.ffi.sampling(**s) for s in samplings])
        words, nw, ms = (C.c_int32 * (n * total))(), (C.c_int32 * n)(), C.c_float(0)
        rc = self.L.kh_model_generate_batch_from(self.h, n, _i32([t for p in prompts for t in p]),
                                                 _i32([len(p) for p in prompts]), _i32(cached), _i32([total] * n), sp,
                                                 None, 0, words, total, nw, C.byref(ms))
        assert rc == 0, rc
        return ms.value

    def time_prefill(self, toks):
        ms = C.c_float(0)
        assert self.L.kh_model_time_prefill(self.h, _i32(toks), len(toks), 0, 2, C.byref(ms)) == 0
        return ms.value

    def close(self):
        self.L.kh_model_destroy(self.h)


def _image(name):
    import torch
    from kuiperllama_amd import binfmt
    spec = binfmt.PRESETS[name]
    spec = dataclasses.replace(spec, seq_len=max(spec.seq_len, CACHE))  # 64 slots of 192 rows (TinyLlama: 2048)
    img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    return spec, img


def ab(args):
    from kuiperllama_amd.model import KuiperModel
    lines = ["# tools/seq_gemm_ab.py ab: generate_batch(gemm=True) of this tree vs generate_batch of the baseline library",
             f"# prompts of {PROMPT} tokens (cached), {STEPS} sampled steps, median of {args.reps} runs, one MI355X",
             f"{'geometry':16s} {'n_seq':>5s} {'8-lane ms/step':>15s} {'wide ms/step':>13s} {'8-lane tok/s':>13s} "
             f"{'wide tok/s':>11s} {'wide/8-lane':>11s}"]
    _write(args.out, lines, end="")  # every row is written as it is measured
    rng = np.random.default_rng(0)
    for name in args.cases.split(","):
        spec, img = _image(name)
        cache = min(spec.seq_len, CACHE)
        new = KuiperModel.from_device_image(img, spec, max_seq_len=cache)
        old = Baseline(args.baseline_lib, img, spec, cache)
        total = PROMPT - 1 + STEPS
        new.seq_slots(64)
        assert old.seq_slots(64) * 64 <= cache
        prompts = [[int(t) for t in rng.integers(0, spec.vocab_size, PROMPT)] for _ in range(64)]
        for s in range(64):
            new.seq_prefill(s, prompts[s][:-1])
            old.seq_prefill(s, prompts[s][:-1])
        sp = [dict(SAMP, seed=100 + s) for s in range(64)]
        breakeven = None
        for n in (8, 16, 32, 64):
            t_old, t_new = [], []
            for rep in range(args.reps + 1):  # the first repetition warms up
                a = old.generate_batch(prompts[:n], total, sp[:n], [PROMPT - 1] * n)
                b = new.generate_batch(prompts[:n], total, sp[:n], cached=[PROMPT - 1] * n, gemm=True)[1]
                if rep:
                    t_old.append(a)
                    t_new.append(b)
            a, b = float(np.median(t_old)), float(np.median(t_new))
            if breakeven is None and b < a:
                breakeven = n
            row = (f"{name:16s} {n:5d} {a / STEPS:15.3f} {b / STEPS:13.3f} {n * STEPS / a * 1e3:13.0f} "
                   f"{n * STEPS / b * 1e3:11.0f} {a / b:11.2f}")
            print(row, flush=True)
            _write(args.out, [row], end="")
        row = (f"# {name}: the wide call is faster from n_seq = {breakeven} on" if breakeven else
               f"# {name}: the wide call is not faster at any measured n_seq")
        print(row, flush=True)
        _write(args.out, [row], end="")
        new.close()
        old.close()
        del img
    _write(args.out, [""], end="")


def prefill(args):
    from kuiperllama_amd.model import KuiperModel
    lines = ["# tools/seq_gemm_ab.py prefill: kh_model_time_prefill, 128-token prefill_gemm, baseline library vs this "
             "tree, alternating, ms (min / median / max of 9)"]
    for name in args.cases.split(","):
        spec, img = _image(name)
        new = KuiperModel.from_device_image(img, spec, max_seq_len=512)
        old = Baseline(args.baseline_lib, img, spec, 512)
        toks = [int(t) for t in np.random.default_rng(1).integers(0, spec.vocab_size, 128)]
        a, b = [], []
        for rep in range(10):
            x, y = old.time_prefill(toks), new.time_prefill(toks, 0, "gemm")
            if rep:
                a.append(x)
                b.append(y)
        lines.append(f"{name:16s} baseline {min(a):.3f} / {np.median(a):.3f} / {max(a):.3f}   this tree {min(b):.3f} / "
                     f"{np.median(b):.3f} / {max(b):.3f}")
        print(lines[-1], flush=True)
        new.close()
        old.close()
    _write(args.out, lines)


def one_pass(name):
    from kuiperllama_amd.model import KuiperModel
    spec, img = _image(name)
    m = KuiperModel.from_device_image(img, spec, max_seq_len=min(spec.seq_len, CACHE))
    m.seq_slots(64)
    rng = np.random.default_rng(0)
    for s in range(64):
        m.seq_prefill(s, [int(t) for t in rng.integers(0, spec.vocab_size, PROMPT)])
    toks = [1] * 64
    sp = [dict(SAMP, seed=s) for s in range(64)]
    for p in range(PROMPT, PROMPT + 32):
        toks = m.seq_step(list(range(64)), toks, [p] * 64, samplings=sp, gemm=True)
    m.close()


CLASSES = (("k_sg_gemm", "GEMMs (QKV, wo, SwiGLU, w2)"), ("k_seq_attn", "grouped attention"),
           ("k_seq_pick", "grouped tail"), ("k_seq_tail", "grouped tail"), ("k_pg_rmsnorm", "RMSNorm"),
           ("k_sg_", "embed / RoPE"))


def table(path, out):
    tot, cnt, passes = {}, {}, 0
    with open(path) as f:
        for r in csv.DictReader(f):
            nm = re.sub(r"\(.*$", "", re.sub(r"^void ", "", r["Kernel_Name"]))
            cls = next((c for k, c in CLASSES if nm.startswith(k)), None)
            if nm.startswith("k_sg_gemm") and re.search(r",\s*3>", nm):
                cls = "classifier GEMM"
            if nm.startswith("k_sg_embed"):
                passes += 1
            if cls is None:
                continue
            tot[cls] = tot.get(cls, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            cnt[cls] = cnt.get(cls, 0) + 1
    lines = [f"# tools/seq_gemm_ab.py table: kernel time of {passes} wide passes of 64 lanes by launch class (rocprofv3 "
             "--kernel-trace)", f"{'class':32s} {'launches/pass':>13s} {'us/pass':>9s} {'share':>6s}"]
    allus = sum(tot.values())
    for c in sorted(tot, key=tot.get, reverse=True):
        lines.append(f"{c:32s} {cnt[c] / passes:13.1f} {tot[c] / passes:9.1f} {100 * tot[c] / allus:5.1f}%")
    lines.append(f"{'sum of kernel time':32s} {sum(cnt.values()) / passes:13.1f} {allus / passes:9.1f}")
    print("\n".join(lines))
    _write(out, lines)


def _write(out, lines, end="\n"):
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n" + end)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab", "pass", "table", "prefill"])
    ap.add_argument("arg", nargs="?")
    ap.add_argument("--baseline-lib", default=os.path.join(ROOT, "kuiperllama_amd", "lib", "parent.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=",".join(PRESETS))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.mode == "ab":
        ab(a)
    elif a.mode == "prefill":
        prefill(a)
    elif a.mode == "pass":
        one_pass(a.arg or PRESETS[0])
    else:
        table(a.arg, a.out)
