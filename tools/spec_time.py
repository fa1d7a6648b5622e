"""Cost of speculative greedy decode (kh_model_generate_lookup: csrc/kh_spec.h, csrc/kh_lookup.h) against the token
loop, as a curve over the acceptance rate.

    python -m kuiperllama_amd.build --variant-at <parent commit> parent     # the baseline library, where git is
    python tools/spec_time.py --baseline-lib kuiperllama_amd/lib/parent.so [--out profiles/spec_cost.txt]
                              [--presets llama3.2-1b,llama2-7b-int8] [--n 128,512] [--reps 5]

Seeded synthetic image of each preset, shared by two models in ONE process: one on the baseline library (loaded beside
this one; it only runs kh_model_generate), one on the library built from these sources.  Prompt of 6 distinct tokens, n
sampled steps, both models created with KH_FLAG_PREFILL_EXACT.  Rows:
  (i)   kh_model_generate of the baseline library, and of this one (must agree: the feature changes no existing path)
  (ii)  generate_lookup with nothing ever drafted (an n-gram length no sequence has), miss_steps 1, 2, 4 and 8: the
        price of one host round trip per miss_steps steps
  (iii) the truth as the hint: the upper bound
  (iv)  the truth hint with one token in every k wrong, k = 8, 4, 3, 2: the curve against acceptance
Hinted rows run one step on the step graphs where nothing is drafted (miss_steps 1) and search n-grams of up to 32 tokens, so that a repeat in the synthetic model's text does not send the drafter
to an earlier place with another continuation.  Every row's words are compared with the baseline's: a row that differs
aborts the run.  Median of `--reps` runs, the rows alternating within a repetition; each figure is the call's own
elapsed_ms (HIP events on the model stream around the prompt phase and the loop); steps/s = total steps / median.
Acceptance on real text is NOT measured here: there are no real checkpoints, and a synthetic model's text says nothing
about it.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 1 << 20  # an n-gram length no sequence reaches: nothing is ever drafted


class BaselineModel:
    """kh_model_generate of another build of the library on the same device image (ctypes, RTLD_LOCAL)."""

    def __init__(self, lib_path, image, weights, spec, max_seq_len, flags):
        from kuiperllama_amd import _ffi
        self.L = L = C.CDLL(lib_path)
        i32 = C.c_int32
        L.kh_model_create_from_device_weights.argtypes = [C.POINTER(i32), C.c_void_p, C.c_size_t,
                                                          C.POINTER(_ffi.ModelOpts), C.POINTER(C.c_void_p)]
        L.kh_model_generate.argtypes = [C.c_void_p, C.POINTER(i32), i32, i32, i32, C.POINTER(i32), C.POINTER(i32),
                                        C.POINTER(C.c_float)]
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

    def generate(self, prompt, total_steps):
        pr = (C.c_int32 * len(prompt))(*prompt)
        words = (C.c_int32 * total_steps)()
        n, ms = C.c_int32(0), C.c_float(0.0)
        rc = self.L.kh_model_generate(self.h, pr, len(prompt), total_steps, 0, words, C.byref(n), C.byref(ms))
        assert rc == 0, rc
        return list(words[:n.value]), float(ms.value)

    def close(self):
        self.L.kh_model_destroy(self.h)


def run_preset(preset, ns, reps, baseline_lib):
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS[preset]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    cap = max(ns) + 16
    m = KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    # the bytes behind the header, 16-byte aligned: the image itself or the aligned copy the model above made of them
    hb = spec.header_bytes()
    weights = img[hb:] if (img.data_ptr() + hb) % 16 == 0 else m._keep
    base = BaselineModel(baseline_lib, img, weights, spec, cap, _ffi.KH_FLAG_PREFILL_EXACT) if baseline_lib else None
    width = m.verify_width()
    rng = np.random.default_rng(7)
    P = [int(t) for t in rng.choice(spec.vocab_size, 6, replace=False)]
    rows = []
    for n in ns:
        T = len(P) - 1 + n
        W = (base or m).generate(P, T)[0]
        text = P + W[len(P) - 1:]

        def lookup(**kw):
            words, ms, st = m.generate_lookup(P, T, **kw)
            if words != W:
                raise SystemExit(f"{preset} n {n} {kw.keys()}: words differ from the baseline's")
            return ms, st

        def wrong(k):
            return [(t + 1) % spec.vocab_size if i % k == k - 1 else t for i, t in enumerate(text)]
        variants = {}
        if base:
            variants["(i) generate, baseline lib"] = lambda: (base.generate(P, T)[1], None)
        variants["(i) generate, this lib"] = lambda: (m.generate(P, T)[1], None)
        for miss in (1, 2, 4, 8):
            variants[f"(ii) no draft, miss {miss}"] = (
                lambda miss=miss: lookup(ngram_max=NEVER, ngram_min=NEVER, miss_steps=miss))
        variants["(iii) truth hint"] = lambda: lookup(hint=text, ngram_max=32, miss_steps=1)
        for k in (8, 4, 3, 2):
            variants[f"(iv) 1 in {k} wrong"] = (lambda k=k: lookup(hint=wrong(k), ngram_max=32, miss_steps=1))
        if m.generate(P, T)[0] != W:
            raise SystemExit(f"{preset} n {n}: this library's generate differs from the baseline's")
        for f in variants.values():  # warm: graphs, buffers, LDS opt-ins
            f()
        ms = {k: [] for k in variants}
        stats = {}
        for _ in range(reps):
            for k, f in variants.items():
                t, st = f()
                ms[k].append(t)
                stats[k] = st
        for k in variants:
            med, st = float(np.median(ms[k])), stats[k]
            per_pass = (st["accepted"] + st["passes"]) / st["passes"] if st and st["passes"] else float("nan")
            rows.append((preset, width, n, k, med, T / med * 1e3, min(ms[k]), max(ms[k]), st["passes"] if st else 0,
                         per_pass, st["plain_steps"] if st else T))
            print(rows[-1], flush=True)
    m.close()
    if base:
        base.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_cost.txt"))
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--presets", default="llama3.2-1b,llama2-7b-int8")
    ap.add_argument("--n", default="128,512")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    ns = [int(x) for x in a.n.split(",")]
    lines = ["# tools/spec_time.py: speculative greedy decode against the token loop on one MI355X (gfx950), synthetic weights",
             f"# median of {a.reps} alternated runs, elapsed_ms of each call (HIP events on the model stream); steps/s = total steps / median",
             "# tok/pass = words per verify pass (accepted + 1); plain = steps run on the step graphs; baseline lib: "
             + ("the parent commit's sources, same process, same image" if a.baseline_lib else "NOT GIVEN"),
             "# acceptance on real text is not measured: synthetic weights, hints made from the truth",
             f"{'preset':<15} {'w':>1} {'n':>4} {'row':<27} {'median ms':>10} {'steps/s':>8} {'min ms':>9} {'max ms':>9} {'passes':>6} {'tok/pass':>8} {'plain':>5}"]
    for preset in a.presets.split(","):
        for p, w, n, k, med, tps, lo, hi, passes, per, plain in run_preset(preset, ns, a.reps, a.baseline_lib):
            lines.append(f"{p:<15} {w:>1} {n:>4} {k:<27} {med:10.3f} {tps:8.0f} {lo:9.3f} {hi:9.3f} {passes:>6} {per:8.2f} {plain:>5}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
