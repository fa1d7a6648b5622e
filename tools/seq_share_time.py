"""Cost of a shared prompt prefix in batched decode (kh_model_seq_share, csrc/kh_attn.h::k_seq_attn_pfx) against the
parent commit's library running the FORKED layout (copies of the prompt's rows, k_seq_attn).

    python -m kuiperllama_amd.build --variant-at <parent commit> parent     # the baseline library, where git is
    python tools/seq_share_time.py --baseline-lib kuiperllama_amd/lib/parent.so [--out profiles/seq_share_cost.txt]
                                   [--cases llama3.2-1b;llama2-7b-int8] [--prompts 512,2048,8192] [--steps 128] [--reps 5]

Seeded synthetic image of each preset, shared by the models of ONE process.  Workload: full width (8 lanes fp32, 4 int8)
samples of one prompt of 512 / 2048 / 8192 tokens, prefilled once, `--steps` sampled steps per sequence (T 0.8, top-k 50,
top-p 0.95, seeds seed, seed + 1, ...).  Rows: the parent library on `width` equal slots with kh_model_seq_fork; this
library on the shared layout (plan_shared_layout) with the attention grid as planned, and with grid.x padded to a
multiple of 8 (hook KH_SEQ_PFX_PAD=1, read at model creation).  A row's figure is the call's own elapsed_ms (HIP events
around the loop; the prompt is cached in every row), median of `--reps` runs, the rows alternating within a repetition.
The words of the shared rows are compared with the forked row's.  Where the forked layout does not fit the preset's cache
the row says so and the shared rows stand alone.  rows = cache rows the layout commits (kh_model_kv_bytes / bytes per row).
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


class BaselineForked:
    """the forked layout on another build of the library, same device image"""

    def __init__(self, lib_path, image, weights, spec, max_seq_len, flags, slots):
        from kuiperllama_amd import _ffi
        self.L = L = C.CDLL(lib_path)
        i32, P = C.c_int32, C.POINTER
        L.kh_model_create_from_device_weights.argtypes = [P(i32), C.c_void_p, C.c_size_t, P(_ffi.ModelOpts),
                                                          P(C.c_void_p)]
        L.kh_model_seq_slots.argtypes = [C.c_void_p, i32, P(i32)]
        L.kh_model_seq_prefill.argtypes = [C.c_void_p, i32, P(i32), i32, i32]
        L.kh_model_seq_fork.argtypes = [C.c_void_p, i32, i32, i32]
        L.kh_model_generate_batch_from.argtypes = [C.c_void_p, i32, P(i32), P(i32), P(i32), P(i32), P(_ffi.Sampling),
                                                   P(i32), i32, P(i32), i32, P(i32), P(C.c_float)]
        L.kh_model_kv_bytes.argtypes = [C.c_void_p, P(C.c_int64), P(C.c_int64)]
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
        self.slots, self._keep = slots, weights

    def fill(self, prompt, fed):
        arr = (C.c_int32 * fed)(*prompt[:fed])
        assert self.L.kh_model_seq_prefill(self.h, 0, arr, fed, 0) == 0
        for s in range(1, self.slots):
            assert self.L.kh_model_seq_fork(self.h, 0, s, fed) == 0

    def generate(self, prompt, fed, total, samplings):
        from kuiperllama_amd import _ffi
        n = self.slots
        flat = prompt * n
        sp = (_ffi.Sampling * n)(*[_ffi.sampling(**s) for s in samplings])
        words, nw, ms = (C.c_int32 * (n * total))(), (C.c_int32 * n)(), C.c_float(0.0)
        rc = self.L.kh_model_generate_batch_from(self.h, n, (C.c_int32 * len(flat))(*flat),
                                                 (C.c_int32 * n)(*([len(prompt)] * n)), (C.c_int32 * n)(*([fed] * n)),
                                                 (C.c_int32 * n)(*([total] * n)), sp, None, 0, words, total, nw,
                                                 C.byref(ms))
        assert rc == 0, rc
        return [list(words[s * total:s * total + nw[s]]) for s in range(n)], float(ms.value)

    def committed(self):
        r, c = C.c_int64(0), C.c_int64(0)
        assert self.L.kh_model_kv_bytes(self.h, C.byref(r), C.byref(c)) == 0
        return int(c.value)

    def close(self):
        self.L.kh_model_destroy(self.h)


def run_case(preset, n_prompt, steps, reps, baseline_lib):
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel, plan_shared_layout
    dev = torch.device("cuda:0")
    spec = binfmt.PRESETS[preset]
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    prompt = [int(t) for t in rng.integers(0, spec.vocab_size, n_prompt + 1)]  # n_prompt fed-only positions
    fed, T = n_prompt, n_prompt + steps
    probe = KuiperModel.from_device_image(img, spec, max_seq_len=64, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    width = probe.seq_width()
    hb = spec.header_bytes()
    weights = img[hb:] if (img.data_ptr() + hb) % 16 == 0 else probe._keep
    probe.close()
    row_bytes = 2 * spec.n_layers * (spec.dim // spec.n_heads * spec.n_kv_heads) * 4
    need_forked = width * ((T + 7) & ~7)
    try:
        lens = plan_shared_layout(spec.seq_len, width, fed, T)
    except ValueError:
        return [(preset, width, n_prompt, "shared layout", None, f"does not fit the preset's cache of {spec.seq_len} rows")]
    forked_fits = need_forked <= spec.seq_len
    cap = need_forked if forked_fits else sum(lens)  # the same cache length on both sides where both fit
    samplings = [dict(SAMP, seed=SEED + s) for s in range(width)]
    rows, variants, truth, closers = [], {}, None, []
    if forked_fits:
        base = BaselineForked(baseline_lib, img, weights, spec, cap, _ffi.KH_FLAG_PREFILL_EXACT, width)
        base.fill(prompt, fed)
        truth = base.generate(prompt, fed, T, samplings)[0]
        variants["forked, parent lib"] = lambda: base.generate(prompt, fed, T, samplings)
        closers.append(base.close)
    else:
        rows.append((preset, width, n_prompt, "forked, parent lib", None,
                     f"does not fit: {need_forked} rows, the cache holds {spec.seq_len}"))

    def shared_model(pad):
        _ffi.debug_set("KH_SEQ_PFX_PAD", "1" if pad else None)
        try:
            m = KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_PREFILL_EXACT)
        finally:
            _ffi.debug_set("KH_SEQ_PFX_PAD", None)
        m.seq_slots_var(lens)
        m.seq_prefill(0, prompt[:fed])
        for s in range(1, width):
            m.seq_share(0, s, fed)
        closers.append(m.close)
        return m
    models = {"shared": shared_model(False), "shared, grid padded to 8": shared_model(True)}
    for k, m in models.items():
        variants[k] = (lambda m: lambda: m.generate_batch([prompt] * width, T, samplings, cached=[fed] * width))(m)
    words = {k: f()[0] for k, f in variants.items()}  # warm, and the words
    truth = truth or words["shared"]
    for k, w in words.items():
        if w != truth:
            raise SystemExit(f"{preset} prompt {n_prompt}: the words of '{k}' differ from the first row's")
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            ms[k].append(f()[1])
    for k, v in ms.items():
        med = float(np.median(v))
        committed = base.committed() if k.startswith("forked") else models[k].kv_bytes()[1]
        rows.append((preset, width, n_prompt, k, (med, width * steps / med * 1e3, med / steps, min(v), max(v),
                                                  committed // row_bytes), ""))
        print(rows[-1], flush=True)
    for c in closers:
        c()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_share_cost.txt"))
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--cases", default="llama3.2-1b;llama2-7b-int8")
    ap.add_argument("--prompts", default="512,2048,8192")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    lines = ["# tools/seq_share_time.py: kh_model_generate_batch on a shared prompt prefix (k_seq_attn_pfx) against the parent commit's library on forked copies (k_seq_attn), one MI355X (gfx950), synthetic weights",
             f"# full width (8 lanes fp32, 4 int8), the prompt cached, {a.steps} sampled steps per sequence (T 0.8, top-k 50, top-p 0.95, seeds {SEED}, {SEED + 1}, ...); median of {a.reps} alternated runs of the call's elapsed_ms; same words in every row of a case",
             "# tok/s = width x steps / median (aggregate); ms/pass = median / steps (one pass per step at full width); rows = cache rows committed (kh_model_kv_bytes)",
             f"{'preset':<15} {'w':>1} {'prompt':>6} {'row':<26} {'median ms':>10} {'tok/s':>8} {'ms/pass':>8} {'min ms':>9} {'max ms':>9} {'rows':>7}"]
    for preset in a.cases.split(";"):
        for n_prompt in [int(x) for x in a.prompts.split(",")]:
            for p, w, n, what, fig, note in run_case(preset, n_prompt, a.steps, a.reps, a.baseline_lib):
                head = f"{p:<15} {w:>1} {n:>6} {what:<26}"
                if fig is None:
                    lines.append(f"{head} {note}")
                else:
                    med, tps, per, lo, hi, rows = fig
                    lines.append(f"{head} {med:10.3f} {tps:8.0f} {per:8.4f} {lo:9.3f} {hi:9.3f} {rows:>7}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
