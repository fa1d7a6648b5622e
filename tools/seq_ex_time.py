"""Cost of per-sequence penalties, logit bias and log-probs in batched decode (k_seq_tail in place of k_seq_pick:
csrc/kh_seq.h, csrc/kh_model_seq.hip).

    python -m kuiperllama_amd.build --variant-at <parent commit> parent     # the baseline library, where git is
    python tools/seq_ex_time.py --baseline-lib kuiperllama_amd/lib/parent.so [--out profiles/seq_ex_cost.txt]
                                [--cases llama3.2-1b;llama2-7b-int8] [--steps 128] [--reps 5] [--baseline-first]

Seeded synthetic image of each preset, shared by two models in ONE process, each cut into `width` slots: one on the
parent commit's library (ctypes; kh_model_generate_batch with everything off) and one on the library built from these
sources.  Workload: `width` samples of one 6-token prompt (full width: 8 lanes fp32, 4 int8), `--steps` sampled steps
per sequence at temperature 0.8 / top-k 50 / top-p 0.95, seeds seed, seed + 1, ...; every sequence prefills its own copy.
A row's figure is the call's own elapsed_ms (HIP events on the model stream around the prompt passes and the loop);
median of `--reps` runs, the rows alternating within a repetition.  tok/s = width x sampled steps / median.

The tail is not timed as a kernel: no entry point launches it alone.  "tail: ..." rows are what ONE PASS costs more
than a pass that ends in k_seq_pick - (median of the row - median of the off row) / passes, in microseconds - with
log-probs N = 0 / 5 / 20 and with a repetition penalty over a window of 64 positions and over the whole slot (last_n
0).  The words of the off rows are compared with the baseline's; rows with a processor on say other words by design.
--baseline-first creates the baseline's model ahead of this library's and runs its row last in every repetition instead
of first: the two "off" rows differ by where their buffers landed and by their place in the rotation, and this swaps both.
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


class BaselineBatch:
    """kh_model_seq_slots + kh_model_generate_batch of another build of the library on the same device image"""

    def __init__(self, lib_path, image, weights, spec, max_seq_len, flags, slots):
        from kuiperllama_amd import _ffi
        self.L = L = C.CDLL(lib_path)
        i32 = C.c_int32
        P = C.POINTER
        L.kh_model_create_from_device_weights.argtypes = [P(i32), C.c_void_p, C.c_size_t, P(_ffi.ModelOpts),
                                                          P(C.c_void_p)]
        L.kh_model_seq_slots.argtypes = [C.c_void_p, i32, P(i32)]
        L.kh_model_generate_batch.argtypes = [C.c_void_p, i32, P(i32), P(i32), P(i32), P(_ffi.Sampling), P(i32), i32,
                                              P(i32), i32, P(i32), P(C.c_float)]
        L.kh_model_destroy.argtypes = [C.c_void_p]
        L.kh_model_destroy.restype = None
        header = np.frombuffer(image[:32].cpu().numpy().tobytes(), dtype=np.int32)
        hdr = (i32 * 8)(*header.tolist()[:8])
        o = _ffi.ModelOpts(spec.family, int(spec.quant), spec.rope_mode, spec.rope_theta, spec.rms_eps, max_seq_len, 0,
                           flags)
        self.h = C.c_void_p()
        rc = L.kh_model_create_from_device_weights(hdr, weights.data_ptr(), weights.numel(), C.byref(o), C.byref(self.h))
        assert rc == 0, rc
        assert L.kh_model_seq_slots(self.h, slots, None) == 0
        self._keep = weights

    def generate_batch(self, prompts, total, samplings):
        from kuiperllama_amd import _ffi
        n = len(prompts)
        flat = [t for p in prompts for t in p]
        sp = (_ffi.Sampling * n)(*[_ffi.sampling(**s) for s in samplings])
        words, nw, ms = (C.c_int32 * (n * total))(), (C.c_int32 * n)(), C.c_float(0.0)
        rc = self.L.kh_model_generate_batch(self.h, n, (C.c_int32 * len(flat))(*flat),
                                            (C.c_int32 * n)(*[len(p) for p in prompts]), (C.c_int32 * n)(*([total] * n)),
                                            sp, None, 0, words, total, nw, C.byref(ms))
        assert rc == 0, rc
        return [list(words[s * total:s * total + nw[s]]) for s in range(n)], float(ms.value)

    def close(self):
        self.L.kh_model_destroy(self.h)


def run_preset(preset, steps, reps, baseline_lib, baseline_first=False):
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS[preset]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    P = [int(t) for t in rng.choice(spec.vocab_size, 6, replace=False)]
    T = len(P) - 1 + steps
    slot_len = (T + 7) & ~7
    probe = KuiperModel.from_device_image(img, spec, max_seq_len=8 * slot_len, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    width = probe.seq_width()
    hb = spec.header_bytes()
    weights = img[hb:] if (img.data_ptr() + hb) % 16 == 0 else probe._keep  # the wrapper's 16-byte aligned copy
    probe.close()
    cap = width * slot_len
    mk_base = lambda: BaselineBatch(baseline_lib, img, weights, spec, cap, _ffi.KH_FLAG_PREFILL_EXACT, width)  # noqa: E731
    base = mk_base() if baseline_first else None
    m = KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    assert m.seq_slots(width) == slot_len
    base = base or mk_base()
    samplings = [dict(SAMP, seed=SEED + s) for s in range(width)]
    truth = base.generate_batch([P] * width, T, samplings)[0]

    def parent():
        w, ms = base.generate_batch([P] * width, T, samplings)
        if w != truth:
            raise SystemExit(f"{preset}: the baseline's own words changed between runs")
        return ms

    def ours(check, **kw):
        def f():
            w, ms = m.generate_batch([P] * width, T, samplings, **kw)
            if check and w != truth:
                raise SystemExit(f"{preset}: words with everything off differ from the baseline's")
            return ms
        return f
    rep64, rep_all = [{"repetition": 1.3, "last_n": 64}] * width, [{"repetition": 1.3, "last_n": 0}] * width
    variants = {
        "generate_batch off, parent lib": parent,
        "generate_batch off": ours(True),
        "generate_batch off (_ex, neutral)": ours(True, penalties=[None] * width),
        "tail: logprobs 0": ours(False, logprobs=0),
        "tail: logprobs 5": ours(False, logprobs=5),
        "tail: logprobs 20": ours(False, logprobs=20),
        "tail: penalty, window 64": ours(False, penalties=rep64),
        "tail: penalty, whole slot": ours(False, penalties=rep_all),
        "tail: penalty 64 + logprobs 5": ours(False, penalties=rep64, logprobs=5),
    }
    if baseline_first:
        variants["generate_batch off, parent lib"] = variants.pop("generate_batch off, parent lib")  # now the last row
    for f in variants.values():  # warm: buffers, LDS opt-ins
        f()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            ms[k].append(f())
    off = float(np.median(ms["generate_batch off"]))
    rows = []
    for what, v in ms.items():
        med = float(np.median(v))
        extra = (med - off) / steps * 1e3 if what.startswith("tail") else None  # one pass per step at full width
        rows.append((preset, width, what, med, width * steps / med * 1e3, min(v), max(v), extra))
        print(rows[-1], flush=True)
    m.close()
    base.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_ex_cost.txt"))
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--cases", default="llama3.2-1b;llama2-7b-int8")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-first", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    lines = ["# tools/seq_ex_time.py: kh_model_generate_batch with per-sequence log-probs / penalties (k_seq_tail) against everything off (k_seq_pick), one MI355X (gfx950), synthetic weights",
             f"# full width (8 lanes fp32, 4 int8), 6-token prompt, {a.steps} sampled steps per sequence (T 0.8, top-k 50, top-p 0.95, seeds {SEED}, {SEED + 1}, ...); median of {a.reps} alternated runs of the call's elapsed_ms",
             "# parent lib: the parent commit's library, same process, same image; the off rows' words equal its words",
             "# tok/s = width x sampled steps / median (aggregate); +us/pass = (median - median of 'generate_batch off') / passes: what the tail adds to ONE pass (not a kernel timing)",
             f"{'preset':<15} {'w':>1} {'row':<34} {'median ms':>10} {'tok/s':>8} {'min ms':>9} {'max ms':>9} {'+us/pass':>9}"]
    for preset in a.cases.split(";"):
        for p, w, what, med, tps, lo, hi, extra in run_preset(preset, a.steps, a.reps, a.baseline_lib, a.baseline_first):
            x = "" if extra is None else f"{extra:9.1f}"
            lines.append(f"{p:<15} {w:>1} {what:<34} {med:10.3f} {tps:8.0f} {lo:9.3f} {hi:9.3f} {x:>9}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
