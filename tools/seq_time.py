"""Throughput of kh_model_generate_batch (sequence slots: csrc/kh_seq.h, csrc/kh_model_seq.hip) against the token loop
run once per sequence.

    python -m kuiperllama_amd.build --variant-at <parent commit> parent     # the baseline library, where git is
    python tools/seq_time.py --baseline-lib kuiperllama_amd/lib/parent.so [--out profiles/seq_cost.txt]
                             [--cases llama3.2-1b:1,2,4,8;llama2-7b-int8:1,2,4] [--steps 128] [--reps 5]

Seeded synthetic image of each preset, shared by two models in ONE process: a batch-1 model on the baseline library
(loaded beside this one; it runs kh_model_set_sampling + kh_model_generate, n_seq times back to back), and a model on
the library built from these sources whose cache is cut into as many slots as the widest row needs.  Workload: one
prompt of 6 distinct tokens, `--steps` sampled steps per sequence, temperature 0.8 / top-k 50 / top-p 0.95, seeds
seed, seed + 1, ... - n samples of a prompt; every sequence prefills its own copy of the prompt, nothing is forked.
Both models are created with KH_FLAG_PREFILL_EXACT.  Every sequence's words are compared with the baseline's: a row
that differs aborts the run.  Median of `--reps` runs, the rows alternating within a repetition; a batch row's figure
is the call's own elapsed_ms (HIP events on the model stream around the prompt passes and the loop), a baseline
row's the sum of its n_seq calls' elapsed_ms.  tok/s = n_seq x sampled steps / median: the aggregate over sequences.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMP = dict(temperature=0.8, top_k=50, top_p=0.95)
SEED = 1234


class BaselineModel:
    """kh_model_set_sampling + kh_model_generate of another build of the library on the same device image (ctypes)."""

    def __init__(self, lib_path, image, weights, spec, max_seq_len, flags):
        from kuiperllama_amd import _ffi
        self.L = L = C.CDLL(lib_path)
        i32 = C.c_int32
        L.kh_model_create_from_device_weights.argtypes = [C.POINTER(i32), C.c_void_p, C.c_size_t,
                                                          C.POINTER(_ffi.ModelOpts), C.POINTER(C.c_void_p)]
        L.kh_model_generate.argtypes = [C.c_void_p, C.POINTER(i32), i32, i32, i32, C.POINTER(i32), C.POINTER(i32),
                                        C.POINTER(C.c_float)]
        L.kh_model_set_sampling.argtypes = [C.c_void_p, C.POINTER(_ffi.Sampling)]
        L.kh_model_destroy.argtypes = [C.c_void_p]
        L.kh_model_destroy.restype = None
        assert weights.data_ptr() % 16 == 0
        header = np.frombuffer(image[:32].cpu().numpy().tobytes(), dtype=np.int32)
        hdr = (i32 * 8)(*header.tolist()[:8])
        o = _ffi.ModelOpts(spec.family, int(spec.quant), spec.rope_mode, spec.rope_theta, spec.rms_eps, max_seq_len, 0,
                           flags)
        self.h = C.c_void_p()
        rc = L.kh_model_create_from_device_weights(hdr, weights.data_ptr(), weights.numel(), C.byref(o), C.byref(self.h))
        assert rc == 0, rc
        self._keep = weights

    def generate(self, prompt, total_steps, sampling):
        from kuiperllama_amd import _ffi
        sp = _ffi.sampling(**sampling)
        rc = self.L.kh_model_set_sampling(self.h, C.byref(sp))
        assert rc == 0, rc
        pr = (C.c_int32 * len(prompt))(*prompt)
        words = (C.c_int32 * total_steps)()
        n, ms = C.c_int32(0), C.c_float(0.0)
        rc = self.L.kh_model_generate(self.h, pr, len(prompt), total_steps, 0, words, C.byref(n), C.byref(ms))
        assert rc == 0, rc
        return list(words[:n.value]), float(ms.value)

    def close(self):
        self.L.kh_model_destroy(self.h)


def run_preset(preset, n_seqs, steps, reps, baseline_lib):
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS[preset]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    P = [int(t) for t in rng.choice(spec.vocab_size, 6, replace=False)]
    T = len(P) - 1 + steps
    slots = max(n_seqs)
    slot_len = (T + 7) & ~7
    cap = slots * slot_len
    m = KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    assert m.seq_slots(slots) == slot_len
    hb = spec.header_bytes()
    weights = img[hb:] if (img.data_ptr() + hb) % 16 == 0 else m._keep
    base = BaselineModel(baseline_lib, img, weights, spec, cap, _ffi.KH_FLAG_PREFILL_EXACT)
    width = m.seq_width()
    samplings = [dict(SAMP, seed=SEED + s) for s in range(slots)]
    truth = [base.generate(P, T, sp)[0] for sp in samplings]

    def loop(n):
        total = 0.0
        for s in range(n):
            w, ms = base.generate(P, T, samplings[s])
            if w != truth[s]:
                raise SystemExit(f"{preset}: the baseline's own words changed between runs (sequence {s})")
            total += ms
        return total

    def batch(n):
        words, ms = m.generate_batch([P] * n, T, samplings[:n])
        if words != truth[:n]:
            bad = [s for s in range(n) if words[s] != truth[s]]
            raise SystemExit(f"{preset} n_seq {n}: words of sequences {bad} differ from the baseline's")
        return ms
    variants = {}
    for n in n_seqs:
        variants[(n, "token loop x n_seq, baseline lib")] = lambda n=n: loop(n)
        variants[(n, "generate_batch")] = lambda n=n: batch(n)
    for f in variants.values():  # warm: graphs, buffers, LDS opt-ins
        f()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            ms[k].append(f())
    rows = []
    for (n, what), v in ms.items():
        med = float(np.median(v))
        rows.append((preset, width, n, what, med, n * steps / med * 1e3, min(v), max(v)))
        print(rows[-1], flush=True)
    m.close()
    base.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_cost.txt"))
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--cases", default="llama3.2-1b:1,2,4,8;llama2-7b-int8:1,2,4")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    lines = ["# tools/seq_time.py: kh_model_generate_batch against the token loop run once per sequence, one MI355X (gfx950), synthetic weights",
             f"# 6-token prompt, {a.steps} sampled steps per sequence (T 0.8, top-k 50, top-p 0.95, seeds {SEED}, {SEED + 1}, ...); median of {a.reps} alternated runs",
             "# batch: the call's elapsed_ms; token loop: sum of the n_seq calls' elapsed_ms on the parent commit's library, same process, same image",
             "# tok/s = n_seq x sampled steps / median (aggregate); x = batch tok/s / token-loop tok/s; every sequence's words equal the baseline's",
             f"{'preset':<15} {'w':>1} {'n_seq':>5} {'row':<33} {'median ms':>10} {'tok/s':>8} {'min ms':>9} {'max ms':>9} {'x':>5}"]
    for case in a.cases.split(";"):
        preset, ns = case.split(":")
        rows = run_preset(preset, [int(x) for x in ns.split(",")], a.steps, a.reps, a.baseline_lib)
        loop_tps = {n: tps for _, _, n, what, _, tps, _, _ in rows if what != "generate_batch"}
        for p, w, n, what, med, tps, lo, hi in rows:
            x = f"{tps / loop_tps[n]:5.2f}" if what == "generate_batch" else ""
            lines.append(f"{p:<15} {w:>1} {n:>5} {what:<33} {med:10.3f} {tps:8.0f} {lo:9.3f} {hi:9.3f} {x:>5}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
