#!/usr/bin/env python3
"""SHA-256 digests of what the three callers of the GEMM pass (csrc/kh_model_gemm.hip) leave behind, for a byte-for-byte
comparison of two builds of the library: the kernels, their arguments and the summation orders are fixed, so a build
that only moved host code must reproduce every digest.  Output: profiles/gemm_pass_digest.txt.

    git worktree add DIR <parent commit> && (cd DIR && python -m kuiperllama_amd.build)   # the baseline library, from
    cp DIR/kuiperllama_amd/lib/libkuiper_hip.so kuiperllama_amd/lib/parent.so             # its own list of sources
    python tools/gemm_pass_digest.py --lib kuiperllama_amd/lib/parent.so --label parent [--out FILE]
    python tools/gemm_pass_digest.py --lib kuiperllama_amd/lib/libkuiper_hip.so --label tree [--out FILE]
    python tools/gemm_pass_digest.py compare [--out FILE]       # no GPU: the two sections line by line

One process per library (the Python binding runs on --lib).  Per geometry of tests/seq_gemm_cases.py, a fresh model per
line:
prefill: prefill_gemm of 290 tokens at position 0 and 28 more at position 290 - all K/V rows; under the heuristic
         shapes, under each (R, NT) tile tests/test_seq_prefill_gemm_gpu.py forces on the three GEMMs, and once with
         KH_PG_ATTN=0 (the decode-attention fallback).
ragged:  one seq_prefill_many of 22 segments in shuffled slot order - 290 tokens, a sharer's 40 tokens behind 37 shared
         rows, 1 .. 8 tokens in 20 short slots; two passes, one segment in both - all K/V rows; heuristic shapes and each
         forced tile.
wide:    one 17-lane seq_step(gemm=True) at positions 0 .. 7 and 255 / 256 / 257 behind exactly fed rows - all K/V rows,
         the lanes' seq_gemm_logits rows and the picks; heuristic shapes and each (R, NT) tile
         tests/test_seq_gemm_gpu.py forces on the four GEMMs.
Each run appends its section to the output file; `compare` appends the verdict and exits 1 on any difference."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PG_HOOKS = ("KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU")
SG_HOOKS = PG_HOOKS + ("KH_PG_SHAPE_STORE",)
# (R, NT, ks, kz of the residual GEMMs): test_seq_prefill_gemm_gpu.py::test_ragged_calls, test_seq_gemm_gpu.py::test_single_passes
PG_FORCED = [None, (2, 8, 1, 2), (2, 4, 2, 4), (2, 2, 1, 1), (1, 4, 2, 2)]
SG_FORCED = [None, (2, 4, 1, 2), (2, 2, 2, 4), (1, 4, 4, 1)]


def _write(path, lines):
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")


def _force(ffi, hooks, cfg):
    for k in hooks:
        ffi.debug_set(k, None if cfg is None else
                      f"{cfg[0]},{cfg[1]},{cfg[2]}" + (f",{cfg[3]}" if k.endswith("RESID") else ""))


def _kv(m, spec):
    h = hashlib.sha256()
    for layer in range(spec.n_layers):
        k, v = m.read_kv(layer, 0, spec.seq_len)
        h.update(k.tobytes())
        h.update(v.tobytes())
    return h.hexdigest()


def _cfg(cfg):
    return "heuristic" if cfg is None else "forced %d,%d,%d,kz%d" % cfg


def digests(G, ffi, KuiperModel):
    """(line label, {what: sha256}) per geometry, case and shape"""
    for name in sorted(G.SPECS):
        spec = G.SPECS[name]

        def model(slots):
            m = KuiperModel.from_host_image(G.host_image(spec), spec, max_seq_len=spec.seq_len)
            if slots:
                m.seq_slots_var(G.LENS)
            return m

        text = [int(t) for t in np.random.default_rng(17).integers(0, spec.vocab_size, 318)]
        for cfg in PG_FORCED + ["attn0"]:
            m = model(False)
            _force(ffi, PG_HOOKS, None if cfg == "attn0" else cfg)
            ffi.debug_set("KH_PG_ATTN", "0" if cfg == "attn0" else None)
            m.prefill_gemm(text[:290])
            m.prefill_gemm(text[290:], 290)
            yield f"{name} prefill {'KH_PG_ATTN=0' if cfg == 'attn0' else _cfg(cfg)}", {"kv": _kv(m, spec)}
            ffi.debug_set("KH_PG_ATTN", None)
            m.close()

        rng = np.random.default_rng(20)
        lens = {1: 40, 2: 290}
        lens.update({s: 1 + (3 * s) % 8 for s in range(3, 23)})
        order = [int(s) for s in rng.permutation(sorted(lens))]
        segs = {s: [int(t) for t in rng.integers(0, spec.vocab_size, lens[s])] for s in sorted(lens)}
        parent = [int(t) for t in rng.integers(0, spec.vocab_size, 48)]
        for cfg in PG_FORCED:
            m = model(True)
            _force(ffi, PG_HOOKS, cfg)
            m.seq_prefill(0, parent, gemm=True)
            m.seq_share(0, 1, 37)
            m.seq_prefill_many(order, [segs[s] for s in order], [37 if s == 1 else 0 for s in order])
            yield f"{name} ragged {_cfg(cfg)}", {"kv": _kv(m, spec)}
            m.close()

        texts = G.texts(spec)
        pick = [0, 1, 2] + list(range(3, 17))
        slots = [int(s) for s in np.random.default_rng(99).permutation(pick)]
        for cfg in SG_FORCED:
            m = model(True)
            for s in slots:
                if G.lane_pos(s) > 0:
                    m.seq_prefill(s, texts[s][:G.lane_pos(s)])
            _force(ffi, SG_HOOKS, cfg)
            picks = m.seq_step(slots, [texts[s][-1] for s in slots], [G.lane_pos(s) for s in slots], gemm=True)
            lg = hashlib.sha256()
            for i in range(len(slots)):
                lg.update(m.seq_gemm_logits(i).tobytes())
            yield f"{name} wide {_cfg(cfg)}", {"kv": _kv(m, spec), "logits": lg.hexdigest(),
                                               "picks": hashlib.sha256(np.asarray(picks, np.int32).tobytes()).hexdigest()}
            _force(ffi, SG_HOOKS, None)
            m.close()


def run(args):
    os.environ["KH_LIB"] = os.path.abspath(args.lib)  # before the binding is imported: it loads this library
    import seq_gemm_cases as G
    from kuiperllama_amd import _ffi
    from kuiperllama_amd.model import KuiperModel
    lines = [f"# tools/gemm_pass_digest.py [{args.label}]: sha256 per geometry, case and GEMM shape, one MI355X"]
    for label, d in digests(G, _ffi, KuiperModel):
        lines.append(f"{label:44s} " + " ".join(f"{k} {v}" for k, v in d.items()))
        print(lines[-1], flush=True)
    _write(args.out, lines + [""])


def compare(args):
    sect, cur = {}, None
    for line in open(args.out):
        if line.startswith("# tools/gemm_pass_digest.py ["):
            cur = sect.setdefault(line[line.index("[") + 1:line.index("]")], [])
        elif cur is not None and " kv " in line:
            cur.append(line.rstrip())
    assert len(sect) == 2, f"{args.out}: want the sections of two libraries, have {sorted(sect)}"
    (la, a), (lb, b) = sect.items()
    bad = [x for x in a if x not in b] + [x for x in b if x not in a]
    lines = [f"# tools/gemm_pass_digest.py compare: [{la}] {len(a)} lines, [{lb}] {len(b)} lines: " +
             ("every digest equal" if not bad and a else f"{len(bad)} lines DIFFER")] + bad
    print("\n".join(lines))
    _write(args.out, lines + [""])
    return 1 if bad or not a else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "compare"])
    ap.add_argument("--lib", help="run: the build of the library to digest")
    ap.add_argument("--label", default=None, help="run: the section's name (default: the library's file name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_pass_digest.txt"))
    args = ap.parse_args()
    if args.mode == "compare":
        sys.exit(compare(args))
    if not args.lib:
        ap.error("run needs --lib")
    args.label = args.label or os.path.basename(args.lib)
    run(args)


if __name__ == "__main__":
    main()
