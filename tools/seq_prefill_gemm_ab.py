#!/usr/bin/env python3
"""The GEMM prefill into sequence slots (csrc/kh_seq_prefill.h: prompt segments of several slots per sweep of the
weights, on the matrix cores) against the parent commit's seq_prefill loop.  Output: profiles/seq_prefill_gemm_ab.txt.

    python -m kuiperllama_amd.build --variant-at <parent commit> parent      # the baseline library, where git is
    python tools/seq_prefill_gemm_ab.py ab --baseline-lib kuiperllama_amd/lib/parent.so [--out FILE] [--cases a,b]
    python tools/seq_prefill_gemm_ab.py prefill --baseline-lib kuiperllama_amd/lib/parent.so
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/seq_prefill_gemm_ab.py pass
    python tools/seq_prefill_gemm_ab.py table DIR/.../*_kernel_stats.csv
    python tools/seq_prefill_gemm_ab.py symbols --baseline-lib kuiperllama_amd/lib/parent.so     # no GPU

ab:      per geometry (synthetic image), both libraries on ONE device image in one process, the calls alternating
         within a repetition, median of `--reps` runs of a host clock around calls that end in a stream synchronise:
         (i)   one prompt of 128 / 512 / 3000 tokens into slot 1 of 2: kh_model_seq_prefill of the baseline library,
               seq_prefill(gemm=True) of this tree, and this tree's batch-1 prefill_gemm of the same tokens (the
               lone-segment pass is that call but for its attention's query-tile sharing from position 2048 on);
         (ii)  64 prompts of 32 tokens into 64 slots: 64 kh_model_seq_prefill calls against one seq_prefill_many;
         (iii) 8 prompts of 300 tokens into 8 slots, likewise.
         Prompt tok/s = fed tokens / time; "pad" = the share of a call's slab tokens that are padding.
prefill: kh_model_time_prefill of a 128-token prefill_gemm, baseline library against this tree, alternating (the
         statements of k_pg_attn moved into csrc/kh_pattn_body.h; no other existing kernel changed).
pass:    one 512-token prompt on Llama-3.2-1B geometry fed nine times each way, alternating - seq_prefill(1, tokens,
         gemm=True) and the batch-1 prefill_gemm(tokens) - for a kernel trace; table: the k_rg_* / k_pg_* rows of its
         kernel statistics.
symbols: the disassembly of every kernel of the baseline library against the same symbol of this tree's (LLVM tools
         of the ROCm install, no GPU): how many are identical, which differ, which are new.
`ab` starts the output file; the other modes append their section to it."""
import argparse
import ctypes as C
import dataclasses
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PRESETS = ["llama3.2-1b", "tinyllama-1.1b", "qwen2.5-0.5b", "llama2-7b-int8"]
CACHE = 8192


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


class Baseline:
    """another build of the library on the same device image (ctypes): its seq_prefill and the GEMM prefill's timer"""

    def __init__(self, lib_path, image, spec, max_seq_len):
        from kuiperllama_amd import _ffi
        self.L = L = C.CDLL(lib_path)
        i32, p32 = C.c_int32, C.POINTER(C.c_int32)
        L.kh_model_create_from_device_weights.argtypes = [p32, C.c_void_p, C.c_size_t, C.POINTER(_ffi.ModelOpts),
                                                          C.POINTER(C.c_void_p)]
        L.kh_model_seq_slots.argtypes = [C.c_void_p, i32, p32]
        L.kh_model_seq_prefill.argtypes = [C.c_void_p, i32, p32, i32, i32]
        L.kh_model_time_prefill.argtypes = [C.c_void_p, p32, i32, i32, i32, C.POINTER(C.c_float)]
        L.kh_model_destroy.argtypes = [C.c_void_p]
        L.kh_model_destroy.restype = None
        weights = image[spec.header_bytes():]
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
    spec = dataclasses.replace(spec, seq_len=max(spec.seq_len, CACHE))
    img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    return spec, img


def _clock(call):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _write(path, lines, end="\n"):
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n" + end)


def ab(args):
    from kuiperllama_amd.model import KuiperModel
    head = ["# tools/seq_prefill_gemm_ab.py ab: the GEMM prefill into slots of this tree vs kh_model_seq_prefill of the "
            "baseline library",
            f"# host clock around synchronising calls, median of {args.reps} alternating runs, one MI355X, synthetic images",
            f"{'geometry':16s} {'case':>12s} {'tokens':>6s} {'pad':>5s} {'VALU loop ms':>13s} {'new call ms':>12s} "
            f"{'prefill_gemm ms':>16s} {'VALU tok/s':>11s} {'new tok/s':>10s} {'new/VALU':>9s} {'new/prefill_gemm':>17s}"]
    open(args.out, "w").close()  # a new file: a second run does not repeat the tables
    _write(args.out, head, end="")
    rng = np.random.default_rng(0)
    for name in args.cases.split(","):
        spec, img = _image(name)
        new = KuiperModel.from_device_image(img, spec, max_seq_len=CACHE)
        old = Baseline(args.baseline_lib, img, spec, CACHE)
        cases = [("1 x 128", 2, [128]), ("1 x 512", 2, [512]), ("1 x 3000", 2, [3000]),
                 ("64 x 32", 64, [32] * 64), ("8 x 300", 8, [300] * 8)]
        for label, n_slots, lens in cases:
            new.seq_slots(n_slots)
            old.seq_slots(n_slots)
            slots = [1] if len(lens) == 1 else list(range(len(lens)))
            prompts = [[int(t) for t in rng.integers(0, spec.vocab_size, n)] for n in lens]
            total = sum(lens)
            pad = 1.0 - total / sum(16 * ((n + 15) // 16) for n in lens)

            def valu():
                for s, p in zip(slots, prompts):
                    old.seq_prefill(s, p)

            t_old, t_new, t_pg = [], [], []
            for rep in range(args.reps + 1):  # the first repetition warms up
                a = _clock(valu)
                b = _clock(lambda: new.seq_prefill_many(slots, prompts))
                c = _clock(lambda: new.prefill_gemm(prompts[0])) if len(lens) == 1 else None
                if rep:
                    t_old.append(a)
                    t_new.append(b)
                    t_pg.append(c)
            a, b = float(np.median(t_old)), float(np.median(t_new))
            c = float(np.median(t_pg)) if len(lens) == 1 else None
            row = (f"{name:16s} {label:>12s} {total:6d} {pad:5.2f} {a:13.3f} {b:12.3f} "
                   f"{(f'{c:.3f}' if c else '-'):>16s} {total / a * 1e3:11.0f} {total / b * 1e3:10.0f} {a / b:9.2f} "
                   f"{(f'{b / c:.3f}' if c else '-'):>17s}")
            print(row, flush=True)
            _write(args.out, [row], end="")
        new.close()
        old.close()
        del img
    _write(args.out, [""], end="")


def prefill(args):
    from kuiperllama_amd.model import KuiperModel
    lines = ["# tools/seq_prefill_gemm_ab.py prefill: kh_model_time_prefill, 128-token prefill_gemm, baseline library vs "
             "this tree, alternating, ms (min / median / max of 9)"]
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


def one_pass():
    from kuiperllama_amd.model import KuiperModel
    spec, img = _image("llama3.2-1b")
    m = KuiperModel.from_device_image(img, spec, max_seq_len=CACHE)
    m.seq_slots(2)
    toks = [int(t) for t in np.random.default_rng(0).integers(0, spec.vocab_size, 512)]
    for _ in range(9):
        m.seq_prefill(1, toks, gemm=True)
        m.prefill_gemm(toks)
    m.close()


def table(path, out):
    import csv
    import re
    lines = ["# tools/seq_prefill_gemm_ab.py table: kernel time of one 512-token prompt on Llama-3.2-1B fed as one segment "
             "into slot 1 and by the batch-1 prefill_gemm, 9 calls each, alternating (rocprofv3 --kernel-trace --stats)"]
    with open(path) as f:
        for r in csv.DictReader(f):
            if re.search(r"k_rg_|k_pg_", r["Name"]):
                lines.append(f'{r["Name"][:90]:90s} calls {r["Calls"]:>6s} avg_ns {float(r["AverageNs"]):12.0f} '
                             f'total_ns {float(r["TotalDurationNs"]):14.0f}')
    print("\n".join(lines))
    _write(out, lines)


def _kernel_text(lib):
    """{symbol: its disassembled instructions} of every gfx950 code object bundled into the shared library"""
    import re
    import shutil
    import subprocess
    import tempfile
    llvm, magic = "/opt/rocm/lib/llvm/bin", b"__CLANG_OFFLOAD_BUNDLE__"
    td, out = tempfile.mkdtemp(prefix="kh_sym_"), {}
    try:
        fat = os.path.join(td, "fat.bin")
        subprocess.check_call([f"{llvm}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for i, s in enumerate(starts):
            chunk, co = os.path.join(td, f"b{i}.bin"), os.path.join(td, f"co{i}.elf")
            with open(chunk, "wb") as f:
                f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={chunk}", f"--output={co}"],
                                  stderr=subprocess.DEVNULL)
            if os.path.getsize(co) == 0:
                continue  # a translation unit without device code
            dis = subprocess.check_output([f"{llvm}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                          text=True)
            name = None
            for line in dis.splitlines():
                m = re.match(r"^<(\S+)>:", line)
                if m:
                    name = m.group(1)
                    out.setdefault(name, [])
                elif name and line.strip():
                    out[name].append(re.sub(r"//.*", "", line).strip())
    finally:
        shutil.rmtree(td, ignore_errors=True)
    return out


def symbols(args):
    from kuiperllama_amd import build
    a, b = _kernel_text(args.baseline_lib), _kernel_text(build.LIB_PATH)
    same = [k for k in a if a[k] == b.get(k)]
    lines = [f"# tools/seq_prefill_gemm_ab.py symbols: disassembly per kernel, baseline library vs this tree: {len(same)} of "
             f"the baseline's {len(a)} identical, {len(set(b) - set(a))} new"]
    lines += [f"differs: {k} ({len(a[k])} against {len(b[k])} instructions)" for k in a if k in b and a[k] != b[k]]
    lines += [f"gone: {k}" for k in sorted(set(a) - set(b))] + [f"new: {k}" for k in sorted(set(b) - set(a))]
    print("\n".join(lines))
    _write(args.out, lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["ab", "prefill", "pass", "table", "symbols"])
    ap.add_argument("path", nargs="?", help="table: the kernel statistics CSV of the traced `pass` run")
    ap.add_argument("--baseline-lib", help="ab, prefill, symbols: the parent commit's build of the library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_prefill_gemm_ab.txt"))
    ap.add_argument("--cases", default=",".join(PRESETS))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.mode in ("ab", "prefill", "symbols") and not args.baseline_lib:
        ap.error(f"{args.mode} needs --baseline-lib")
    if args.mode == "pass":
        one_pass()
    elif args.mode == "table":
        if not args.path:
            ap.error("table needs the CSV")
        table(args.path, args.out)
    else:
        {"ab": ab, "prefill": prefill, "symbols": symbols}[args.mode](args)


if __name__ == "__main__":
    main()
