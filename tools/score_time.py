"""Cost of sequence scoring (kh_model_score: csrc/kh_prefill.h::k_pf_cls, csrc/kh_logprobs.h::k_score_lp) on the GPU.

    python tools/score_time.py [--out profiles/score_cost.txt] [--presets llama3.2-1b,llama2-7b-int8] [--n 128,512]

Seeded synthetic image of each preset; for every n, scored tokens per second of
  * kh_model_score with top_n = 0 and with top_n = 20,
  * kh_model_time_prefill(.., KH_PREFILL_GEMV) on the same tokens: the same B-token pass without the last layer's
    attention / wo / FFN, the classifier and the records - the difference is what scoring adds,
  * a loop of kh_model_predict with log-probs on (top_n = 0): what a caller had before kh_model_score, one host round
    trip and one full pass over the weights per token.
Median of `--reps` (5) runs, the four variants alternating within a repetition; every figure between two HIP events on
the model stream (the prefill figure is kh_model_time_prefill's own, taken the same way).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_preset(preset, ns, reps):
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS[preset]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec, max_seq_len=max(ns) + 8)
    stream = torch.cuda.ExternalStream(m.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lib = _ffi.lib()
    rng = np.random.default_rng(7)

    def timed(fn):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    rows = []
    for n in ns:
        toks = [int(t) for t in rng.integers(0, spec.vocab_size, n)]
        arr = (C.c_int32 * n)(*toks)

        def score(top_n):
            m.set_logprobs(top_n)
            return timed(lambda: _ffi.check(lib.kh_model_score(m._h, arr, n, 0), "kh_model_score"))

        def predict_loop():
            m.set_logprobs(0)

            def loop():
                for p, t in enumerate(toks):
                    m.predict(t, p, is_prompt=False, exec="fused")
            return timed(loop)
        variants = {"score, top_n 0": lambda: score(0), "score, top_n 20": lambda: score(20),
                    "prefill (gemv)": lambda: m.time_prefill(toks, 0, mode="gemv"), "predict loop": predict_loop}
        for f in variants.values():  # warm: buffers, LDS opt-ins, resident-grid queries
            f()
        ms = {k: [] for k in variants}
        for _ in range(reps):
            for k, f in variants.items():
                ms[k].append(f())
        for k in variants:
            med = float(np.median(ms[k]))
            rows.append((preset, n, k, med, n / med * 1e3, min(ms[k]), max(ms[k])))
            print(rows[-1], flush=True)
    m.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_cost.txt"))
    ap.add_argument("--presets", default="llama3.2-1b,llama2-7b-int8")
    ap.add_argument("--n", default="128,512")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    ns = [int(x) for x in a.n.split(",")]
    lines = ["# tools/score_time.py: cost of sequence scoring on one MI355X (gfx950), synthetic weights",
             f"# median of {a.reps} alternated runs, HIP events on the model stream; tok/s = n / median",
             f"{'preset':<15} {'n':>4} {'variant':<16} {'median ms':>10} {'tok/s':>9} {'min ms':>9} {'max ms':>9}"]
    for preset in a.presets.split(","):
        for p, n, k, med, tps, lo, hi in run_preset(preset, ns, a.reps):
            lines.append(f"{p:<15} {n:>4} {k:<16} {med:10.3f} {tps:9.0f} {lo:9.3f} {hi:9.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
