"""Cost of speculative decode under the model's settings (kh_model_generate_lookup_as_set, kh_model_verify_as_set:
csrc/kh_spec.h) against the token loop under the same settings, and of the pass's tail against the greedy pair.

    python tools/spec_set_time.py [--out profiles/spec_set_ab.txt] [--presets llama3.2-1b,llama2-7b-int8]
                                  [--n 128] [--reps 5] [--no-rocprof]

Seeded synthetic image of each preset, one model created with KH_FLAG_PREFILL_EXACT, prompt of 6 distinct tokens, n
sampled steps.  Settings: S1 = temperature 0.8, top-k 50, top-p 0.95, a seed; S2 = greedy with penalties repetition
1.3, presence 0.2, frequency 0.1 over every fed token.  Per preset and setting, rows alternating within a repetition:
  (i)   generate under the setting: the token loop
  (ii)  generate_lookup(as_set=True) with the truth as the hint (n-grams up to 32, one plain step per miss): FULL
        acceptance, the upper bound and nothing else
  (iii) generate_lookup(as_set=True) with nothing ever drafted (an n-gram length no sequence has), miss_steps 8 and 1:
        the price of asking
Every row's words are compared with (i)'s: a row that differs aborts the run.  Each figure is the call's own elapsed_ms
(HIP events on the model stream around the prompt phase and the loop), median of --reps; steps/s = total steps / median.
  (iv)  one verify pass of full width at position 64, host clock around the synchronising call, median of 200 calls
        alternating between nothing set (k_spec_pick + k_spec_accept), S1, S2, log-probs 5 and all of them together.
Then, in a run of its own (`rocprofv3 --kernel-trace --stats`, child process `--passes`): kernel times of the same
passes - the tail's launches by name and the sum over every kernel of a pass.
Acceptance on real text is NOT measured here: there are no real checkpoints, and a synthetic model's text says nothing
about it.
"""
import argparse
import csv
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 1 << 20  # an n-gram length no sequence reaches: nothing is ever drafted
SAMP = (0.8, 50, 0.95, 0xC0FFEE)
PEN = dict(repetition=1.3, presence=0.2, frequency=0.1, last_n=0)
POS0 = 64
PASS_SETTINGS = ("none", "S1", "S2", "lp5", "all")


def apply(m, key):
    m.set_sampling(*SAMP) if key in ("S1", "all") else m.set_sampling()
    m.set_penalties(**PEN) if key in ("S2", "all") else m.set_penalties()
    m.set_logprobs(5 if key in ("lp5", "all") else None)


def make(preset, cap):
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS[preset]
    img = binfmt.synth_image(spec, seed=1234, device=torch.device("cuda:0"))
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img, spec, max_seq_len=cap, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    rng = np.random.default_rng(7)
    return m, spec, [int(t) for t in rng.choice(spec.vocab_size, 6, replace=False)]


def pass_tokens(m, spec):
    """POS0 fed tokens and a full-width pass behind them (any tokens do: the launches do not depend on acceptance)"""
    rng = np.random.default_rng(11)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, POS0 + m.verify_width())]
    m.prefill(toks[:POS0])
    return toks[POS0:]


def run_passes(preset, calls):
    """child of the profiled run: `calls` passes per setting, alternating"""
    m, spec, _ = make(preset, POS0 + 16)
    fed = pass_tokens(m, spec)
    for _ in range(calls):
        for key in PASS_SETTINGS:
            apply(m, key)
            m.verify(fed, POS0, as_set=True)
    m.close()


def run_preset(preset, n, reps):
    m, spec, P = make(preset, max(n + 16, POS0 + 16))
    T, width, rows = len(P) - 1 + n, m.verify_width(), []
    for key in ("S1", "S2"):
        apply(m, key)
        W = m.generate(P, T)[0]
        text = P + W[len(P) - 1:]

        def lookup(**kw):
            words, ms, st = m.generate_lookup(P, T, as_set=True, **kw)
            if words != W:
                raise SystemExit(f"{preset} {key} {sorted(kw)}: words differ from generate's")
            return ms, st
        variants = {"(i) generate": lambda: (m.generate(P, T)[1], None),
                    "(ii) truth hint": lambda: lookup(hint=text, ngram_max=32, miss_steps=1),
                    "(iii) no draft, miss 8": lambda: lookup(ngram_max=NEVER, ngram_min=NEVER, miss_steps=8),
                    "(iii) no draft, miss 1": lambda: lookup(ngram_max=NEVER, ngram_min=NEVER, miss_steps=1)}
        for f in variants.values():  # warm: graphs, buffers
            f()
        ms, stats = {k: [] for k in variants}, {}
        for _ in range(reps):
            for k, f in variants.items():
                t, stats[k] = f()
                ms[k].append(t)
        for k in variants:
            med, st = float(np.median(ms[k])), stats[k]
            per = (st["accepted"] + st["passes"]) / st["passes"] if st and st["passes"] else float("nan")
            rows.append(f"{preset:<15} {width:>1} {key:<3} {k:<23} {med:10.3f} {T / med * 1e3:8.0f} {min(ms[k]):9.3f} "
                        f"{max(ms[k]):9.3f} {st['passes'] if st else 0:>6} {per:8.2f} {st['plain_steps'] if st else T:>5}")
            print(rows[-1], flush=True)
    # (iv) one pass, host clock around the synchronising call
    fed = pass_tokens(m, spec)
    us = {key: [] for key in PASS_SETTINGS}
    for it in range(210):
        for key in PASS_SETTINGS:
            apply(m, key)
            t0 = time.perf_counter()
            m.verify(fed, POS0, as_set=True)
            if it >= 10:
                us[key].append((time.perf_counter() - t0) * 1e6)
    passes = []
    for key in PASS_SETTINGS:
        q = np.percentile(us[key], [50, 10, 90])
        passes.append(f"{preset:<15} {width:>1} pass under {key:<5} median {q[0]:8.1f} us  p10 {q[1]:8.1f}  p90 {q[2]:8.1f}")
        print(passes[-1], flush=True)
    m.close()
    return rows, passes


def rocprof(preset, calls):
    """kernel statistics of run_passes under rocprofv3: the tail's kernels, and the sum over all kernels per pass"""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "p", "--",
               sys.executable, os.path.abspath(__file__), "--passes", preset, "--calls", str(calls)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 failed ({p.returncode}):\n{p.stderr[-2000:]}")
        for d, _, files in os.walk(td):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    rows = open(os.path.join(d, f)).read().splitlines()
                    out = [rows[0]] + [r for r in rows[1:] if "k_spec" in r or "k_pf_cls" in r]
                    recs = list(csv.DictReader(rows))
                    if recs and "TotalDurationNs" in recs[0] and "Name" in recs[0]:
                        total = sum(float(r["TotalDurationNs"]) for r in recs if "k_pf_" in r["Name"] or "attn" in r["Name"])
                        n_pass = calls * len(PASS_SETTINGS)
                        out.append(f"# k_pf_* and attention kernels of the run: {total / n_pass / 1e3:.1f} us per pass (an upper "
                                   f"bound of a pass's own kernels: the {POS0}-token prefill ahead of the {n_pass} passes and the "
                                   "attention launches of the creation-time self-tests are in it)")
                    return out
    raise RuntimeError("rocprofv3 wrote no kernel statistics")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_set_ab.txt"))
    ap.add_argument("--presets", default="llama3.2-1b,llama2-7b-int8")
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--passes", default=None, help="(child of the profiled run) preset")
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.passes:
        return run_passes(a.passes, a.calls)
    lines = ["# tools/spec_set_time.py: speculative decode under the model's settings against the token loop under the same settings,",
             "# one MI355X (gfx950), synthetic weights.  S1: T 0.8, top-k 50, top-p 0.95, seeded; S2: greedy, penalties 1.3 / 0.2 / 0.1.",
             f"# median of {a.reps} alternated runs, elapsed_ms of each call (HIP events on the model stream); steps/s = total steps / median",
             "# tok/pass = words per verify pass (accepted + 1); plain = steps run on the step graphs",
             "# hints are made from the truth: FULL acceptance, an upper bound; acceptance on real text is not measured",
             f"{'preset':<15} {'w':>1} {'set':<3} {'row':<23} {'median ms':>10} {'steps/s':>8} {'min ms':>9} {'max ms':>9} {'passes':>6} {'tok/pass':>8} {'plain':>5}"]
    passes = ["", f"# (iv) one verify_as_set pass of full width at position {POS0}: host clock around the synchronising call, 200 calls per",
              "# setting, alternating (none = k_spec_pick + k_spec_accept; the others k_spec_tail + k_spec_accept_set, S2 / all behind k_spec_hist)"]
    for preset in a.presets.split(","):
        r, p = run_preset(preset, a.n, a.reps)
        lines += r
        passes += p
    lines += passes
    if not a.no_rocprof:
        for preset in a.presets.split(","):
            lines += ["", f"# rocprofv3 --kernel-trace --stats of {a.calls} such passes per setting ({', '.join(PASS_SETTINGS)}), {preset}: "
                      "the tail's kernels and k_pf_cls (ns)"]
            lines += rocprof(preset, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
