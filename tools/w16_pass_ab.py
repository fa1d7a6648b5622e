"""Same-box A/B of the B-token passes of W16 models (kh_w16_pass.h): prefill, score, generate_batch and generate_lookup
of a KH_FLAG_W16 model with its passes on the 16-bit copy against the same model with its passes on the fp32 matrices.

    python tools/w16_pass_ab.py [--models llama3.2-1b,tinyllama-1.1b,qwen2.5-0.5b,llama2-7b]
                                [--lib LABEL=PATH ...] [--out profiles/w16_pass_ab.txt]

One process per model (this script re-invoked with --model) on a synthetic image of the BASELINE geometry whose
matrices were rounded to bf16; every model of the process has the flag on and shares the device image.  One model per
setting of the hook KH_W16_PASS (read at creation): 0 (passes on fp32), 1 (the default mask), 0x1f (all five classes)
and each single class (0x1 qkv, 0x2 wo, 0x4 ffn13, 0x8 w2, 0x10 cls), alternated five times.  Figures, median and range of the five:
  * kh_model_time_prefill (the B-token kernels) of 64 tokens, per pass;
  * score of 64 tokens with log-probs of the fed tokens only (wall clock around the call);
  * generate_batch at full width, 128 steps: the call's own elapsed_ms;
  * generate_lookup of 128 words with the truth as hint: the call's own elapsed_ms.
The words of every row of a case must be equal, or the script stops.
Adoption rule, per class: its pass stays on the copy only if its median lies below the KH_W16_PASS=0
median by more than the range of those runs - on the prefill pass for qkv, wo, ffn13 and w2, on score for cls (a
prefill runs no classifier).
--lib (repeatable): the builds of the library to measure, this tree's when none is given (kuiperllama_amd/build.py
--variant NAME KH_PF_U_W16=8 -> kuiperllama_amd/lib/NAME.so): how KH_PF_U_W16 was chosen."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (("0", "fp32"), ("1", "default"), ("0x1f", "all"), ("0x1", "qkv"), ("0x2", "wo"), ("0x4", "ffn13"), ("0x8", "w2"),
            ("0x10", "cls"))
ROUNDS = 5
FIGURES = ("prefill/pass ms", "score64 ms", "batch128 ms", "lookup128 ms")


def _med_range(v):
    return statistics.median(v), max(v) - min(v)


def one_model(name):
    import torch
    sys.path.insert(0, ROOT)
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS[name]
    dev = torch.device("cuda:0")
    img = binfmt.synth_image(spec, seed=1234, device=dev)
    binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()
    m = {}
    for hook, label in SETTINGS:
        _ffi.debug_set("KH_W16_PASS", hook)
        m[label] = KuiperModel.from_device_image(img, spec, max_seq_len=2048, flags=_ffi.KH_FLAG_W16)
    _ffi.debug_set("KH_W16_PASS", None)
    assert m["default"].w16_info()["state"] == 1, m["default"].w16_info()
    width = m["fp32"].seq_width()
    print(f"## {name}: dim {spec.dim} hidden {spec.hidden_dim} layers {spec.n_layers} vocab {spec.vocab_size}; {width} "
          f"tokens per pass; default mask {','.join(m['default'].w16_pass_info()['classes']) or 'none'}")
    for label in m:
        want = {"fp32": [], "default": m["default"].w16_pass_info()["classes"],
                "all": list(_ffi.KH_W16_CLASSES)}.get(label, [label])
        assert m[label].w16_pass_info()["classes"] == want, (label, m[label].w16_pass_info())
    toks = [1] + [263 + 7 * i for i in range(63)]
    prompts = [[1, 263 + s] for s in range(width)]
    truth, _ = m["fp32"].generate([1, 263], 129)
    t = {label: {f: [] for f in FIGURES} for label in m}
    words = {}

    def same(case, label, w):
        if words.setdefault(case, w) != w:
            raise SystemExit(f"{name}: {case} words of setting {label} differ from the first setting's")

    for mm in m.values():
        mm.seq_slots(width)
    for rnd in range(ROUNDS + 1):  # round 0: warm-up, not recorded
        for label, mm in m.items():
            ms = mm.time_prefill(toks, 0, mode="gemv") / (len(toks) / width)
            mm.set_logprobs(0)
            t0 = time.perf_counter()
            rec = mm.score(toks, 0)
            sc = (time.perf_counter() - t0) * 1e3
            mm.set_logprobs(None)
            same("score", label, rec["logprob"].tobytes())
            bw, bms = mm.generate_batch(prompts, 129)
            same("generate_batch", label, bw)
            lw, lms, stats = mm.generate_lookup([1, 263], 129, hint=truth)
            same("generate_lookup", label, (lw, stats["accepted"]))
            assert lw == truth
            if rnd:
                for f, v in zip(FIGURES, (ms, sc, bms, lms)):
                    t[label][f].append(v)
    print(f"words of score, generate_batch and generate_lookup equal over the {len(m)} settings: yes")
    print(f"{'passes on':10s}" + "".join(f"{f:>28s}" for f in FIGURES))
    for label in m:
        print(f"{label:10s}" + "".join("{:>17.3f} (range {:.3f})".format(*_med_range(t[label][f])) for f in FIGURES))
    out = []
    for c in ("qkv", "wo", "ffn13", "w2", "cls"):
        f = "score64 ms" if c == "cls" else "prefill/pass ms"
        (m0, r0), (m1, _) = _med_range(t["fp32"][f]), _med_range(t[c][f])
        keep = m1 < m0 - r0
        if not keep:
            out.append(c)
        print(f"{c:6s} {f}: fp32 {m0:.3f} (range {r0:.3f})  copy {m1:.3f}  {(m1 / m0 - 1) * 100:+6.1f} %   "
              f"{'adopt' if keep else 'LEAVE OUT (not below fp32 by more than its range)'}")
    print(f"classes the adoption rule leaves out: {','.join(out) if out else 'none'}")
    for label in ("default", "all"):
        for f in FIGURES:
            print(f"{label} vs fp32, {f}: {(statistics.median(t[label][f]) / statistics.median(t['fp32'][f]) - 1) * 100:+.1f} %")
    for mm in m.values():
        mm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", help="(internal) measure one model in this process and print its lines")
    ap.add_argument("--models", default="llama3.2-1b,tinyllama-1.1b,qwen2.5-0.5b,llama2-7b")
    ap.add_argument("--lib", action="append", default=[], help="LABEL=PATH of a build of the library (PATH empty: this tree's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w16_pass_ab.txt"))
    a = ap.parse_args()
    if a.model:
        return one_model(a.model)
    lines = ["# tools/w16_pass_ab.py: the B-token passes of W16 models on the 16-bit copy against fp32, bf16-rounded "
             "synthetic images, one MI355X, one process per model, flag on throughout", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    libs = [tuple(x.rsplit("=", 1)) for x in a.lib] or [("this build", "")]  # an empty PATH: the tree's own library
    for label, path in libs:
        emit(f"# ---- library: {label}")
        env = dict(os.environ)
        if path:
            env["KH_LIB"] = os.path.abspath(path)
        for name in [n for n in a.models.split(",") if n]:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", name], capture_output=True,
                               text=True, timeout=900, env=env)
            for s in p.stdout.splitlines():
                emit(s)
            if p.returncode != 0:
                emit(f"## {name}: not measured (exit {p.returncode}): {p.stderr.strip().splitlines()[-1:] or ''}")
            emit("")


if __name__ == "__main__":
    main()
