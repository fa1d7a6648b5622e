#!/usr/bin/env python3
"""SHA-256 digests of everything the public API returns behind the last launch of a decode step - k_sample,
k_sample_screen, k_sample_topp, k_sample_proc, k_sample_lp (csrc/kh_step_tail.h) - and behind the row tails that share
their helpers (k_seq_tail, k_spec_tail, k_spec_accept[_set], k_score_lp), for a byte-for-byte comparison of two builds of
the library.  Output: profiles/step_tail_digest.txt.

    git worktree add DIR <parent commit> && (cd DIR && python -m kuiperllama_amd.build)   # the baseline library
    cp DIR/kuiperllama_amd/lib/libkuiper_hip.so kuiperllama_amd/lib/parent.so
    python tools/step_tail_digest.py --lib kuiperllama_amd/lib/parent.so --label parent [--out FILE]
    python tools/step_tail_digest.py --lib kuiperllama_amd/lib/libkuiper_hip.so --label tree [--out FILE]
    python tools/step_tail_digest.py compare [--out FILE]       # no GPU: the two sections line by line
    python tools/step_tail_digest.py objects --lib TREE.so --parent-lib PARENT.so [--out FILE]   # no GPU

One process per library (the Python binding runs on --lib).  One geometry, tests/test_logprobs_gpu.py::FLAT_SPEC (dim
256, hidden 512, 2 layers, 4 heads, 2 KV heads, vocabulary 2048) with 32 cache rows: fp32 for the screened tails, int8
for the rest.  A line is one sha256 over what the case returns - words and their count, predict's token, logits(), the
log-prob records of every position, first_sample, the verify block, the lookup stats, seq_logprobs - and names the tail
kernels its launch log saw (eager launches and graph captures; k_sample itself is not logged) and the error codes it
holds, if any.  Cases:
generate      graph and fused exec under each tail - greedy, both screen levels, sampled, processors, processors +
              sampled, log-probs N = 0 / 5 / 20 over the greedy, sampled and processor picks - with prompts of 1 and 3
              tokens fed token by token (KH_PREFILL=token: the forced branch runs inside the tail), 20 steps and
              total_steps = cache_len (the last step sits on the words / hist / record guards); once more per setting
              with the default prompt phase (first_sample); with a stop token
predict       at a prompt position and at a sampled one, under each setting
verify        verify, verify_as_set, generate_lookup and generate_lookup_as_set under each setting, a rejected draft in
              the pass
seq           seq_step_ex and generate_batch_ex with per-slot processors, samplers and records, one lane at its slot's
              last position
score         N = 0 and 5
`compare` appends the verdict and exits 1 on any difference.  `objects` reads the two libraries' gfx950 code objects
(tests/code_objects.py) and appends, per tail kernel, VGPRs, SGPRs, LDS, scratch and instruction count of both, and
whether the instruction streams are equal up to register numbers."""
import argparse
import dataclasses
import hashlib
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TAG = "# tools/step_tail_digest.py ["
CACHE = 32
INF = float("inf")
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)
BIAS = {5: -INF, 11: 1.0}
SAMP = dict(temperature=0.8, top_k=50, top_p=0.95, seed=0xC0FFEE)
# (label, sampler, processors, log-probs)
PICKS = [("greedy", False, False), ("sampled", True, False), ("processors", False, True)]
SETTINGS = ([(p, s, pr, None) for p, s, pr in PICKS] + [("processors+sampled", True, True, None)] +
            [(f"{p} lp{n}", s, pr, n) for p, s, pr in PICKS for n in (0, 5, 20)])
TAILS = ("k_sample", "k_sample_screen", "k_sample_topp", "k_sample_proc", "k_sample_lp", "k_seq_tail", "k_seq_pick",
         "k_spec_tail", "k_spec_pick", "k_spec_accept", "k_spec_accept_set", "k_score_lp", "k_set_state")
LOGGED = TAILS + ("k_cls_screen", "k_cls_screen_q8")  # the screen level shows in the launches ahead of the tail


def _write(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")


def _feed(h, x):
    if isinstance(x, dict):
        for k in sorted(x):
            h.update(str(k).encode())
            _feed(h, x[k])
    elif isinstance(x, (list, tuple)):
        h.update(b"[%d" % len(x))
        for v in x:
            _feed(h, v)
    elif isinstance(x, np.ndarray):
        h.update(str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes())
    elif isinstance(x, float):
        h.update(np.float64(x).tobytes())
    else:
        h.update(repr(x).encode())


def _sha(*parts):
    h = hashlib.sha256()
    _feed(h, parts)
    return h.hexdigest()


def digests(ffi, binfmt, KuiperModel, torch):
    """(line label, sha256, tail kernels launched) per case"""
    from test_logprobs_gpu import FLAT_SPEC
    dev = torch.device("cuda:0")
    V = FLAT_SPEC.vocab_size

    def model(quant):
        # (the int8 export has its own classifier: binfmt.layout)
        spec = dataclasses.replace(FLAT_SPEC, quant=quant, shared_classifier=not quant)
        img = binfmt.synth_image(spec, seed=3, device=dev)
        torch.cuda.synchronize()
        return KuiperModel.from_device_image(img, spec, max_seq_len=CACHE)

    def settle(m, samp, proc, lp):
        m.set_sampling(**SAMP) if samp else m.set_sampling()
        m.set_penalties(**PEN) if proc else m.set_penalties()
        m.set_logit_bias(BIAS if proc else None)
        m.set_logprobs(lp)

    errors = []

    def safe(fn):  # an error code is a result like any other; the line says how many it holds
        try:
            return fn()
        except ffi.KhError as e:
            errors.append(str(e))
            return f"KhError {e}"

    def records(m, lp):
        return None if lp is None else safe(lambda: m.logprobs(0, m.cfg.cache_len))

    def logged(fn):
        ffi.debug_set("KH_LAUNCH_LOG", "1")
        try:
            out = fn()
            log = ffi.launch_log()
        finally:
            ffi.debug_set("KH_LAUNCH_LOG", None)
        names = sorted({k.split("<")[0] for k in log} & set(LOGGED)) + ([f"{len(errors)} KhError"] if errors else [])
        del errors[:]
        return out, ",".join(names)

    def gen(m, prompt, steps, lp, **kw):
        words = safe(lambda: m.generate(prompt, steps, **kw)[0])
        return [words, len(words), safe(m.logits), records(m, lp), safe(m.first_sample)]

    P3 = [1, 263, 7]
    # ---- generate under each tail
    q8 = model(True)
    f32 = model(False)
    cases = [(q8, label, None, (s, pr, lp)) for label, s, pr, lp in SETTINGS]
    cases += [(f32, "greedy screen level 2", None, (False, False, None)),
              (f32, "greedy screen level 1", "0", (False, False, None))]
    for m, label, q8_hook, (s, pr, lp) in cases:
        settle(m, s, pr, lp)
        ffi.debug_set("KH_CLS_SCREEN_Q8", q8_hook)
        for exec_ in ("graph", "fused"):
            for prompt in (P3[:1], P3):
                for steps in (20, m.cfg.cache_len):
                    os.environ["KH_PREFILL"] = "token"
                    try:
                        info0 = m.cls_screen_info()
                        out, tails = logged(lambda: gen(m, prompt, steps, lp, exec=exec_))
                        info1 = m.cls_screen_info()
                    finally:
                        del os.environ["KH_PREFILL"]
                    scr = {k: info1[k] - info0[k] for k in ("steps", "candidates", "overflow_steps")}
                    yield f"generate {label}, {exec_}, prompt {len(prompt)}, {steps} steps", _sha(out, scr), tails
        out, tails = logged(lambda: gen(m, P3, 20, lp))
        yield f"generate {label}, graph, prompt 3, 20 steps, default prompt phase", _sha(out), tails
        stop = [out[0][11]] if isinstance(out[0], list) and len(out[0]) > 11 else [0]
        out, tails = logged(lambda: gen(m, P3, 20, lp, stop=stop))
        yield f"generate_until {label}, stop token", _sha(out), tails
        ffi.debug_set("KH_CLS_SCREEN_Q8", None)
    # ---- predict
    for label, s, pr, lp in SETTINGS:
        settle(q8, s, pr, lp)
        out, tails = logged(lambda: [safe(lambda: q8.predict(1, 0, True)), safe(q8.logits), records(q8, lp),
                                     safe(lambda: q8.predict(263, 1, False)), safe(q8.logits), records(q8, lp)])
        yield f"predict {label}", _sha(out), tails
    # ---- the verify pass and draft + verify
    W = q8.verify_width()
    for label, s, pr, lp in SETTINGS:
        settle(q8, s, pr, lp)
        truth = q8.generate(P3 + [9], 16)[0]
        fed = [9] + [int(t) for t in truth[3:3 + W - 1]]
        fed[2] = (fed[2] + 1) % V  # the pass accepts one draft and rejects the rest
        for as_set in (False, True):
            if not as_set and label != "greedy":
                continue  # the plain entry points are greedy whatever the model's settings say
            def ver():
                q8.prefill(P3)
                nxt, a = q8.verify(fed, 3, as_set=as_set)
                return [nxt, a, safe(q8.logits), records(q8, lp), safe(lambda: q8.predict(int(nxt[a]), 3 + a + 1))]
            out, tails = logged(lambda: safe(ver))
            yield f"verify{'_as_set' if as_set else ''} {label}", _sha(out), tails
            def look():
                words, _, st = q8.generate_lookup([5, 9] * 3, 28, hint=[5, 9] * 3 + [int(t) for t in truth],
                                                  as_set=as_set)
                return [words, len(words), st, safe(q8.logits), records(q8, lp), safe(q8.first_sample)]
            out, tails = logged(lambda: safe(look))
            yield f"generate_lookup{'_as_set' if as_set else ''} {label}", _sha(out), tails
    # ---- score
    for n in (0, 5):
        settle(q8, False, False, n)
        out, tails = logged(lambda: safe(lambda: q8.score([1, 263, 7, 9, 5, 11, 300, 2047, 0, 12], 0)))
        yield f"score N {n}", _sha(out), tails
    q8.close()
    f32.close()
    # ---- sequence slots: per-slot processors, samplers and records
    m = model(True)
    slot_len = m.seq_slots(4)
    rng = np.random.default_rng(5)
    text = [[int(t) for t in rng.integers(0, V, slot_len)] for _ in range(4)]
    at = [0, 3, slot_len - 1, 5]  # slot 2 steps at its last position
    samp = [None, SAMP, None, dict(SAMP, seed=7)]
    pen = [PEN, None, dict(PEN, last_n=0), None]
    bias = [BIAS, None, None, {3: 2.0}]
    for n in (None, 0, 5):
        def step():
            for s in range(4):
                if at[s]:
                    m.seq_prefill(s, text[s][:at[s]])
            picks = m.seq_step([0, 1, 2, 3], [text[s][at[s]] for s in range(4)], at, samplings=samp, penalties=pen,
                               logit_bias=bias, logprobs=n)
            return [picks, None if n is None else [m.seq_logprobs(s, 0, slot_len) for s in range(4)]]
        out, tails = logged(lambda: safe(step))
        yield f"seq_step_ex logprobs {n}", _sha(out), tails
        def batch():
            words, _ = m.generate_batch([text[s][:1 + s % 3] for s in range(4)], [slot_len, 5, slot_len, 3],
                                        samplings=samp, penalties=pen, logit_bias=bias, logprobs=n)
            return [words, None if n is None else [m.seq_logprobs(s, 0, slot_len) for s in range(4)]]
        out, tails = logged(lambda: safe(batch))
        yield f"generate_batch_ex logprobs {n}", _sha(out), tails
    m.close()


def run(args):
    os.environ["KH_LIB"] = os.path.abspath(args.lib)  # before the binding is imported: it loads this library
    import torch
    from kuiperllama_amd import _ffi, binfmt
    from kuiperllama_amd.model import KuiperModel
    lines = [f"{TAG}{args.label}]: sha256 per case of what the API returns, one MI355X"]
    for label, sha, tails in digests(_ffi, binfmt, KuiperModel, torch):
        lines.append(f"{label:74s} sha {sha}  {tails}")
        print(lines[-1], flush=True)
    _write(args.out, lines + [""])


def compare(args):
    sect, cur = {}, None
    for line in open(args.out):
        if line.startswith(TAG):
            cur = sect.setdefault(line[len(TAG):line.index("]")], [])
        elif line.startswith("#") or not line.strip():
            cur = None if line.startswith("#") else cur
        elif cur is not None and " sha " in line:
            cur.append(line.rstrip())
    assert len(sect) == 2, f"{args.out}: want the sections of two libraries, have {sorted(sect)}"
    (la, a), (lb, b) = sect.items()
    bad = [x for x in a if x not in b] + [x for x in b if x not in a]
    lines = [f"# tools/step_tail_digest.py compare: [{la}] {len(a)} lines, [{lb}] {len(b)} lines: " +
             ("every digest equal" if not bad and a else f"{len(bad)} lines DIFFER")] + bad
    print("\n".join(lines))
    _write(args.out, lines + [""])
    return 1 if bad or not a else 0


# ---- code objects ---------------------------------------------------------------------------------------------------
_REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")


def _kernels(lib):
    """{demangled kernel name: (vgprs, sgprs, lds bytes, scratch bytes, [instruction, register numbers masked])} of the
    tail kernels in the gfx950 code objects of `lib`"""
    import code_objects as co
    out = {}
    td = tempfile.mkdtemp(prefix="kh_tail_")
    fat = os.path.join(td, "fat.bin")
    subprocess.check_call([co.TOOLS[0], "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(co.MAGIC), blob)]
    for i, s in enumerate(starts):
        chunk, elf = os.path.join(td, f"b{i}.bin"), os.path.join(td, f"co{i}.elf")
        with open(chunk, "wb") as f:
            f.write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.check_call([co.TOOLS[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={chunk}", f"--output={elf}"], stderr=subprocess.DEVNULL)
        if os.path.getsize(elf) == 0:
            continue
        meta = {}
        for blk in re.split(r"\n\s+- \.agpr_count:", subprocess.check_output([co.TOOLS[2], "--notes", elf], text=True)):
            nm = re.search(r"\.name:\s+(_Z\S+)", blk)
            if nm:
                g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                meta[nm.group(1)] = (g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"),
                                     g("private_segment_fixed_size"))
        dis = subprocess.check_output([os.path.join(co.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", elf], text=True)
        for sym, body in re.findall(r"^[0-9a-f]+ <(_Z\w+)>:\n(.*?)(?=^\s*$|\Z)", dis, flags=re.M | re.S):
            name = co.template_name(sym) or co.plain_name(sym)
            if sym not in meta or not name or name.split("<")[0] not in TAILS:
                continue
            ins = []
            for ln in body.splitlines():
                t = ln.split("//")[0].strip()
                if t and not t.startswith("s_nop") and not t.startswith("s_code_end"):
                    ins.append(_REG.sub(r"\1#", re.sub(r"\b(s_c?branch\w*)\s+\S+", r"\1 L", t)))
            out.setdefault(name, meta[sym] + (ins,))
    return out


def objects(args):
    a, b = _kernels(args.parent_lib), _kernels(args.lib)
    lines = ["# tools/step_tail_digest.py objects: gfx950 code objects of the tail kernels, parent | tree",
             f"{'kernel':<24} {'VGPR':>9} {'SGPR':>9} {'LDS bytes':>13} {'scratch':>7} {'instructions':>13}  stream"]
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            lines.append(f"{k:<24} only in {'parent' if k in a else 'tree'}")
            continue
        p, t = a[k], b[k]
        same = "equal up to register numbers" if p[4] == t[4] else "differs"
        lines.append(f"{k:<24} {p[0]:>4}|{t[0]:<4} {p[1]:>4}|{t[1]:<4} {p[2]:>6}|{t[2]:<6} {p[3]:>3}|{t[3]:<3} "
                     f"{len(p[4]):>6}|{len(t[4]):<6}  {same}")
    print("\n".join(lines))
    _write(args.out, lines + [""])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", nargs="?", default="run", choices=["run", "compare", "objects"])
    ap.add_argument("--lib", help="run / objects: the build of the library to digest")
    ap.add_argument("--parent-lib", help="objects: the parent commit's build")
    ap.add_argument("--label", default=None, help="run: the section's name (default: the library's file name)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_tail_digest.txt"))
    args = ap.parse_args()
    if args.mode == "compare":
        sys.exit(compare(args))
    if not args.lib or (args.mode == "objects" and not args.parent_lib):
        ap.error("run needs --lib, objects --lib and --parent-lib")
    if args.mode == "objects":
        return objects(args)
    args.label = args.label or os.path.basename(args.lib)
    run(args)


if __name__ == "__main__":
    main()
