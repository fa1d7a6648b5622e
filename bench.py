#!/usr/bin/env python3
"""bench.py — decode tokens/sec of the MI355X-native KuiperLLama decode path.

Contract (driver):  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  N>1 is launched by the driver as  python -m torch.distributed.run --nproc-per-node N ...
  One JSON line on stdout (rank 0).

* plain run: set up the workload, W warm-up steps, the K timed steps, the line (`metric`, `value`,
             `unit`, `higher_is_better`, `dtype`, `ms_per_step` = ms of one timed step) - nothing
             else.  Everything below that takes runs of its own (second workload, roofline kernel
             timings, CPU baselines, other configs, latency / prefill / long-context / load probes)
             runs only with --full.
* --dump-outputs DIR : after the timed steps, what their last step handed the caller of generate():
             DIR/words.npy (the K generated token ids, float64) and DIR/logits.npy (the logits of
             the last step, float32).  Same arguments -> same seeded weights and prompt -> same
             inputs in every run, so two builds can be compared output for output.
* metric   : BASELINE.json "decode tokens/sec" (batch-1 greedy, the reference's generate()
             loop, demo/main.cpp:5-47), workload = configs[1] Llama-3.2-1B fp32; with --full the
             second half of the metric (Llama-2-7B int8) is measured in the same run and reported
             under "secondary".
* a "step" : one decode step = one forward pass of the whole model + greedy argmax for one
             token, all inside one hipGraph replay.  Weights, KV cache and activations are
             resident in HBM before the timed region starts.
* data     : synthetic — seeded random weights of the exact architecture written in the
             reference's .bin layout (kuiperllama_amd/binfmt.py); no checkpoints exist offline.
* N>1      : the path is single-stream autoregressive and does not shard:
             N independent replicas, one process per GPU, no data-path collective; the only
             communication is the barrier + max-over-ranks of the timing.  value = N*K / max t.
* roofline : dominant kernel = the fused w1/w3+SwiGLU GEMV ("ffn13"); achieved = its
             algorithmic bytes per launch / its average launch duration measured with HIP
             events on the model's own stream (kh_model_profile_step) right after the timed
             region.  "step" adds the whole-token figure (bytes/token x tok/s).
* cpu_baseline : kind "reference" = the reference's OWN CPU backend (oracle/_ref/ref_cpu_model*:
             its cpu/*.cpp kernels + model classes compiled where they lie over an Armadillo
             stand-in on numpy's OpenBLAS) timed on this host's cores on a bounded number of
             tokens of the same workload, its tokens compared with the GPU's; the oracle
             (oracle/, the restatement the parity tests use) beside it as cpu_baseline.port,
             and alone (kind "port") where the reference has no CPU path (int8).
* layout   : both halves of the metric and their roofline fractions as scalars inside
             `roofline` / `config` and again in `summary` at the end of the line (assemble_line).
* other_configs : the remaining BASELINE.json configs (Qwen2.5-0.5B, TinyLlama-1.1B = the
             north-star floor of 60 tok/s, Llama-2-7B fp32 = one replica of config 5) measured
             briefly into the same line, each with a token check against a short oracle pass.
             --no-others for rocprofv3 runs (they launch the same kernel instantiations at other
             sizes and would blur the --stats average of the headline workload).
* long_context : single-step latency of the headline workload deep in its 131072-row cache.
* --full --no-extras : only the contract's timed region + the roofline kernel.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from kuiperllama_amd import binfmt  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
# logits vs the oracle at one greedy step (tests/test_model_gpu.py holds the same bounds at full size)
LOGIT_TOL_F32, LOGIT_TOL_Q8, LOGIT_CHECK_POS = 4e-5, 1e-4, 8
PROMPT = [1, 263]  # BOS + "a": the demo prompt (demo/main.cpp:64) under the Llama-2 vocab


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def ffn13_bytes(spec: binfmt.ModelSpec) -> float:
    """Algorithmic bytes of one ffn13 launch: w1 and w3 rows once (+ scales), x and the norm
    weight once, h written once."""
    n = 2 * spec.hidden_dim * spec.dim
    w = n + (n // spec.group_size) * 4 if spec.quant else n * 4
    return float(w + 2 * spec.dim * 4 + spec.hidden_dim * 4)


def build_model(spec, device_index, seed=1234, max_seq_len=0):
    from kuiperllama_amd.model import KuiperModel
    dev = torch.device(f"cuda:{device_index}")
    t0 = time.time()
    img = binfmt.synth_image(spec, seed=seed, device=dev)
    torch.cuda.synchronize(dev)
    log(f"[bench] synthesised {spec.name}: {img.numel() / 1e9:.2f} GB in {time.time() - t0:.1f}s")
    m = KuiperModel.from_device_image(img, spec, max_seq_len=max_seq_len, device=device_index)
    return m, img


def timed_generate(m, steps, warmup, world, dev):
    from kuiperllama_amd import replicas
    # untimed: builds + warms the graph; a run longer than the default 256-step token buffers
    # is rehearsed at full length so no (re)allocation or re-capture lands in the timed region
    m.generate(PROMPT, steps if steps > 256 else max(warmup, 2), exec="graph")
    res = {}

    def run():
        res["words"], res["ev_ms"] = m.generate(PROMPT, steps, exec="graph")  # syncs its stream

    wall, _ = replicas.timed_replica_run(run, steps, world, dev,
                                         lambda: torch.cuda.synchronize(dev))
    return res["words"], wall, res["ev_ms"]


def cpu_baseline(spec, img_host, gpu_words, max_tokens, budget_s, min_sample_s=10.0, gpu_logits=None):
    """Oracle (port of the reference CPU backend) on this host's cores, bounded sample.  Two
    matmul variants: (i) the oracle's own OpenMP row-parallel GEMV, (ii) the oracle
    with its fp32 matmuls routed through numpy's bundled OpenBLAS sgemv (the reference's
    Armadillo -> BLAS path).  The team size of each is calibrated on one token; the faster
    variant is the one sampled and reported."""
    from oracle import oracle as O
    om = O.OracleModel.from_spec(img_host, spec, cache_len=max(256, max_tokens + 1))
    # a DRAM-bound GEMV stops scaling long before 256 SMT threads; cgroup quotas can make
    # nproc a lie (O.effective_cpus reads the quota)
    eff = O.effective_cpus()
    cands = sorted({c for c in (eff, eff // 2, 64, 32, 16, 8) if 1 <= c <= eff}, reverse=True)
    best = None  # (ms/token, variant, threads)
    calib = {}
    for variant in ("openmp", "openblas"):
        if variant == "openblas" and spec.quant:
            continue  # the int8 matmul has no BLAS form
        for c in cands:
            if variant == "openblas":
                if not O.use_openblas(c):
                    break
                O.set_threads(min(c, 8))  # the small non-matmul loops
            else:
                O.use_openblas(0)
                O.set_threads(c)
            om.forward(PROMPT[0], 0)  # warm (page-in) then time one token
            t = time.perf_counter()
            om.forward(PROMPT[0], 0)
            dt1 = time.perf_counter() - t
            log(f"[bench] cpu calibration: {variant} {c} threads -> {dt1 * 1e3:.1f} ms/token")
            calib[f"{variant}:{c}"] = round(dt1 * 1e3, 2)
            if best is None or dt1 < best[0]:
                best = (dt1, variant, c)
            if dt1 > 4.0:
                break
    _, variant, threads = best
    if variant == "openblas":
        O.use_openblas(threads)
        O.set_threads(min(threads, 8))
    else:
        O.use_openblas(0)
        O.set_threads(threads)
    # whole passes of the same decode (up to max_tokens steps each) until >= ~10 s of CPU work,
    # token by token so the sample can stop at the budget
    seq = list(PROMPT)
    t0 = time.perf_counter()
    n = 0
    first_words = None
    passes = 0
    logit_check = None
    while True:
        words = []
        for pos in range(max_tokens):
            tok = seq[pos] if pos < len(PROMPT) else words[pos - 1]
            lg = om.forward(int(tok), pos)
            if gpu_logits is not None and logit_check is None and pos == gpu_logits[0]:
                # SURVEY 8(c) stated tolerance, checked in the record itself: the GPU's logits of the same
                # greedy step (same prompt, same fed tokens while the words agree) against the oracle's
                tol = LOGIT_TOL_Q8 if spec.quant else LOGIT_TOL_F32
                err = float(np.abs(lg - gpu_logits[1]).max())
                logit_check = {"pos": pos, "max_abs_err": err, "tolerance": tol, "ok": bool(err <= tol)}
            nxt = PROMPT[pos + 1] if pos < len(PROMPT) - 1 else int(np.argmax(lg))
            words.append(nxt)
            n += 1
            if time.perf_counter() - t0 > budget_s:
                break
        passes += 1
        if first_words is None:
            first_words = words
        if time.perf_counter() - t0 > min(min_sample_s, budget_s):
            break
    dt = time.perf_counter() - t0
    words = first_words
    O.use_openblas(0)
    # token-for-token check on the common prefix of the CPU pass and the GPU's own greedy run from
    # the same prompt (the GPU list is at least as long as the CPU pass, see measure())
    n_cmp = min(len(words), len(gpu_words))
    div = next((i for i in range(n_cmp) if words[i] != gpu_words[i]), None)
    match = n_cmp > 0 and div is None
    how = ("fp32 matmuls via numpy's bundled OpenBLAS sgemv (the reference's Armadillo->BLAS path)"
           if variant == "openblas" else
           ("OpenMP row-parallel int8 group-dequant GEMV" if spec.quant else "OpenMP row-parallel fp32 GEMV"))
    return {"value": n / dt, "unit": "tokens/s", "cores": threads, "kind": "port",
            "host": host_cpu_facts(),
            "sample": f"{n} decode steps = {passes} pass(es) over the first {len(words)} steps of the "
                      f"same greedy decode ({spec.name}, prompt {PROMPT}), {how}, {dt:.1f}s",
            "variant": variant, "calibration_ms_per_token": calib,
            "tokens_match_gpu": bool(match), "tokens_compared": n_cmp, "first_divergence": div,
            "max_logit_err_vs_oracle": logit_check}


def cpu_baseline_reference(spec, img_host, gpu_words, max_tokens, budget_s, min_sample_s=10.0, gpu_logits=None):
    """The reference's OWN CPU backend, timed on this host (cpu_baseline.kind = "reference"): oracle/_ref/ref_cpu_model*
    = the reference's model / operator classes, CPU getters and its ten CPU kernels (kuiper/source/op/kernels/cpu/*.cpp)
    compiled where they lie in the build container, Armadillo answered by tests/cpp/ref_stubs/armadillo over numpy's
    bundled OpenBLAS (the reference's Armadillo -> BLAS sgemv path), run on the image the GPU just decoded (written to
    /dev/shm), same prompt, whole greedy passes of up to max_tokens steps until ~min_sample_s of decode time.  Returns
    None when no build of the backend fits the workload (int8: the reference has no CPU int8; a flavour without a
    build) or the binaries are absent - the caller falls back to the oracle ("port")."""
    from kuiperllama_amd import build as kbuild
    from oracle import oracle as O
    flavor = kbuild.ref_cpu_flavor(spec)
    exe = kbuild.REF_CPU_BINS.get(flavor) if flavor else None
    if not exe or not os.path.exists(exe):
        return None
    nbytes = int(np.asarray(img_host).nbytes)
    try:
        st = os.statvfs("/dev/shm")
        if st.f_bavail * st.f_frsize < nbytes + (1 << 30) or host_mem_available_gb() < 1.3 * nbytes / 1e9 + 8:
            log(f"[bench] reference CPU backend skipped for {spec.name}: not enough /dev/shm or host memory")
            return None
    except OSError:
        return None
    tok_model = os.path.join(ROOT, "tests", "golden", "spm_llama_like.model")
    path = f"/dev/shm/kh_bench_refcpu_{os.getpid()}.bin"
    lpath = path + ".logits"
    eff = O.effective_cpus()
    prompt = ",".join(map(str, PROMPT))

    def run(steps, threads, budget, logits=False):
        cmd = [exe, path, tok_model, str(steps), prompt, str(budget)] + ([lpath] if logits else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=max(120.0, 6 * budget_s),
                           env=dict(os.environ, KH_REF_BLAS_THREADS=str(threads)))
        if r.returncode != 0:
            raise RuntimeError(f"{os.path.basename(exe)} failed: {r.stdout[-300:]} {r.stderr[-300:]}")
        lines = r.stdout.strip().split("\n")
        words = [int(x) for x in lines[0].split()[1:]]
        ms = float(lines[2].split(" steps in ")[1].split(" ms")[0])
        return words, ms * 1e-3, lines[1].replace("blas: ", "")
    try:
        np.asarray(img_host).tofile(path)
        calib = {}
        best = None
        for c in sorted({c for c in (eff, eff // 2, 8) if 1 <= c <= eff}, reverse=True):
            w, sec, _ = run(4, c, 30.0)
            calib[str(c)] = round(sec / len(w) * 1e3, 2)
            log(f"[bench] reference CPU backend calibration: {c} BLAS threads -> {sec / len(w) * 1e3:.1f} ms/token")
            if best is None or sec / len(w) < best[0]:
                best = (sec / len(w), c)
        threads = best[1]
        t0 = time.perf_counter()
        n, dt, passes, first_words, blas, logit_check = 0, 0.0, 0, None, None, None
        while True:
            want_lg = gpu_logits is not None and first_words is None
            words, sec, blas = run(max_tokens, threads, max(1.0, budget_s - (time.perf_counter() - t0)), logits=want_lg)
            n += len(words)
            dt += sec
            passes += 1
            if first_words is None:
                first_words = words
                if want_lg and len(words) > gpu_logits[0]:
                    lg = np.fromfile(lpath, dtype=np.float32).reshape(len(words), -1)[gpu_logits[0]]
                    err = float(np.abs(lg - gpu_logits[1]).max())
                    logit_check = {"pos": gpu_logits[0], "max_abs_err": err, "tolerance": LOGIT_TOL_F32,
                                   "ok": bool(err <= LOGIT_TOL_F32)}
            if dt > min(min_sample_s, budget_s) or time.perf_counter() - t0 > budget_s:
                break
    finally:
        for f in (path, lpath):
            if os.path.exists(f):
                os.unlink(f)
    words = first_words
    n_cmp = min(len(words), len(gpu_words))
    div = next((i for i in range(n_cmp) if words[i] != gpu_words[i]), None)
    return {"value": n / dt, "unit": "tokens/s", "cores": threads, "kind": "reference", "host": host_cpu_facts(),
            "sample": f"{n} decode steps = {passes} pass(es) over the first {len(words)} steps of the same greedy decode "
                      f"({spec.name}, prompt {PROMPT}) by {os.path.basename(exe)}: the reference's LLama2Model / Qwen2Model "
                      f"on kDeviceCPU over its own cpu/*.cpp kernels, {dt:.1f}s of decode time",
            "variant": f"reference translation units ({flavor} flavour build) over tests/cpp/ref_stubs/armadillo; sgemv from {blas}",
            "calibration_ms_per_token": calib,
            "tokens_match_gpu": bool(n_cmp > 0 and div is None), "tokens_compared": n_cmp, "first_divergence": div,
            "max_logit_err_vs_reference_cpu": logit_check}


def host_cpu_facts() -> dict:
    """What the CPU baseline ran on: logical CPUs the OS shows, the cgroup quota, and what the
    process may really use (the baseline moves +-30 % between boxes with these)."""
    from oracle import oracle as O
    quota = None
    try:
        txt = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if txt[0] == "max" else round(float(txt[0]) / float(txt[1]), 2)
    except (OSError, ValueError, IndexError):
        pass
    model = None
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"nproc": os.cpu_count(), "cgroup_cpu_quota": quota, "effective_cpus": O.effective_cpus(),
            "cpu_model": model}


TRAFFIC_FILE = os.path.join("profiles", "pmc_traffic.json")


def load_traffic(kernel_key):
    """-> (HBM bytes per launch or None, provenance).  NOT measured in this run: PMC counters need
    their own rocprofv3 passes (the guide's HBM section), so the figure is read from the committed
    summary of those passes (tools/profile_pmc.sh -> tools/rocpd_summary.py); the provenance names
    the file, the commit the counters were collected on and the correction applied."""
    p = os.path.join(ROOT, TRAFFIC_FILE)
    try:
        with open(p) as f:
            doc = json.load(f)
        ent = doc.get(kernel_key)
        meta = doc.get("_meta", {})
        from kuiperllama_amd.build import kernel_sources_sha1
        src = {"file": TRAFFIC_FILE, "measured_in_this_run": False,
               "collected_on_commit": meta.get("commit"), "collected_by": meta.get("command"),
               # the device-code headers hashed at collection time against the ones this run was built from: a kernel
               # change after the PMC passes shows here instead of silently keeping a stale ratio
               "kernel_sources_unchanged": (meta.get("kernel_sources_sha1") == kernel_sources_sha1()
                                            if meta.get("kernel_sources_sha1") else None),
               "correction": "FETCH_SIZE KiB x1024 x2 (gfx950 half-count) + WRITE_SIZE KiB x1024"}
        return (float(ent["hbm_bytes"]) if ent else None), src
    except Exception:
        return None, {"file": TRAFFIC_FILE, "measured_in_this_run": False, "error": "unreadable"}


def host_mem_available_gb() -> float:
    """Host memory this process may still take: min(MemAvailable, cgroup limit - usage)."""
    avail = float("inf")
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable:"):
                avail = int(ln.split()[1]) / 1e6
    except OSError:
        pass
    try:
        mx = open("/sys/fs/cgroup/memory.max").read().strip()
        if mx != "max":
            cur = int(open("/sys/fs/cgroup/memory.current").read())
            avail = min(avail, (int(mx) - cur) / 1e9)
    except (OSError, ValueError):
        pass
    return avail


def cpu_int8_restated(spec_q8, img_q8_dev, args, gpu_words, gpu_logits):
    """the reference has NO CPU int8 path (kernels_interfaces.cpp:54-61), so
    the CPU comparison points for Llama-2-7B int8 are (i) CPU fp32 Llama-2-7B - measured with the
    fp32 image under other_configs.llama2-7b.cpu_baseline - and (ii) the oracle's own restated CPU
    int8 (cuda/matmul_kernel.cu:56-87 on the host), measured here on the very image the GPU ran;
    both clearly labelled."""
    from oracle import oracle as O
    # Token parity of the int8 half of the metric INSIDE the record: one pass of >= 64 greedy steps of the oracle on
    # the 7 GB image (0.5-0.7 s per token on 16 host cores: ~45 s, once) when the host has the cores for it; a short
    # pass (16 steps, a third of the CPU budget) otherwise, with the reason stated.
    eff = O.effective_cpus()
    third = max(4.0, args.cpu_budget_s / 3)
    deep = eff >= 16 and time_left(args) > 150
    n_tok, budget = (72, 60.0) if deep else (16, third)
    img_h = img_q8_dev.cpu().numpy()
    try:
        r = cpu_baseline(spec_q8, img_h, gpu_words, n_tok, budget, min_sample_s=third, gpu_logits=gpu_logits)
    finally:
        del img_h
    out = {k: r[k] for k in ("value", "unit", "cores", "kind", "sample", "variant", "host", "tokens_match_gpu",
                             "tokens_compared", "first_divergence", "max_logit_err_vs_oracle")}
    out["tokens_target"] = n_tok
    if not deep:
        out["short_pass_reason"] = (f"{eff} effective host CPUs (< 16)" if eff < 16
                                    else "wall-clock budget of the run (--budget-s) nearly spent")
    out["label"] = ("oracle restatement of cuda/matmul_kernel.cu:56-87 on the host; the reference itself "
                    "has no CPU int8")
    return {"cpu_int8_restated": out,
            "cpu_fp32": {"see": "other_configs.llama2-7b.cpu_baseline (reference-equivalent CPU fp32 path on "
                                "Llama-2-7B: same shapes, fp32 weights)"}}


def other_config(spec, local_rank, args, steps=128):
    """One of the remaining BASELINE configs in the same record (not the contract's timed region):
    128 greedy steps from pos 0, hipGraph replay, best of 3 -> tok/s, ms per step, whole-step
    fraction of 8 TB/s; then a bounded CPU-oracle pass over the same image for the token check
    (common prefix with the GPU's words) and that config's CPU tok/s."""
    m, img = build_model(spec, local_rank)
    try:
        m.generate(PROMPT, 16, exec="graph")
        runs = [m.generate(PROMPT, steps, exec="graph") for _ in range(3)]
        words, ms = min(runs, key=lambda r: r[1])
        lat = {str(p): round(sorted(m.time_step(p, 5))[2], 2) for p in (0, 64, 127)}
    finally:
        m.close()
    tok_s = steps / (ms * 1e-3)
    bytes_tok = spec.algorithmic_bytes_per_token((steps - 1) / 2.0)
    out = {"value": tok_s, "unit": "tokens/s", "ms_per_step": ms / steps, "steps": steps,
           "dtype": "int8 weights x f32 activations" if spec.quant else "f32",
           "bytes_per_token": bytes_tok, "step_frac_of_8TBs": bytes_tok * tok_s / 8e12,
           "latency_us_at_pos": lat, "words_head": words[:8],
           "tokens_match": None, "tokens_compared": 0}
    if not args.no_cpu_baseline:
        need_gb = binfmt.image_nbytes(spec) / 1e9
        have = host_mem_available_gb()
        if have < need_gb + 8:
            out["cpu_baseline"] = {"skipped": f"host memory {have:.0f} GB < {need_gb + 8:.0f} GB needed"}
        else:
            big = need_gb > 8
            budget = max(4.0, args.cpu_budget_s / 3) if big else 3.0
            img_h = img.cpu().numpy()
            try:
                r = None
                try:
                    r = cpu_baseline_reference(spec, img_h, words, 16 if big else 32, budget,
                                               min_sample_s=budget if big else 1.5)
                except Exception as e:  # noqa: BLE001
                    log(f"[bench] reference CPU backend unavailable for {spec.name}: {e!r}")
                if r is None:
                    r = cpu_baseline(spec, img_h, words, 16 if big else 32, budget, min_sample_s=budget if big else 1.5)
            finally:
                del img_h
            out["cpu_baseline"] = {k: r[k] for k in ("value", "unit", "cores", "kind", "sample", "variant", "host")}
            out["tokens_match"] = r["tokens_match_gpu"]
            out["tokens_compared"] = r["tokens_compared"]
            out["first_divergence"] = r["first_divergence"]
    del img
    torch.cuda.empty_cache()
    return out


LONG_POSITIONS = (1023, 2047, 4095, 4096, 32768, 131071)  # 1023 / 2047: time splits merged by k_wo_comb; from 4095: GQA group path


def long_context(m, spec, dev):
    """Single-step latency of the graph-replayed decode step deep in the cache:
    the K/V rows below the probed position are filled with random values on the GPU
    (kh_model_write_kv takes device pointers too), then for each position the whole step
    (kh_model_time_step, median of 9) and the attention kernel alone (back-to-back launches over
    all layers).  attn_kv_frac = K/V bytes the position's attention must read
    (L * 2 * (pos+1) * kv_dim * 4) / attention time of the L launches / 8 TB/s."""
    cache_len = int(m.cfg.cache_len)
    poss = [p for p in LONG_POSITIONS if p < cache_len]
    if not poss:
        return None
    top = max(poss) + 1
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    rows = 16384
    for l in range(spec.n_layers):
        for r0 in range(0, top, rows):
            n = min(rows, top - r0)
            kv = torch.empty((2, n, spec.kv_dim), dtype=torch.float32, device=dev).normal_(0.0, 1.0, generator=gen)
            m.write_kv_device(l, r0, kv[0], kv[1])
    torch.cuda.synchronize(dev)
    out = {}
    wo_short = m.profile_kernel("wo", 64, reps=4)  # wo with a plain input vector (nothing to merge)
    for p in poss:
        us = sorted(m.time_step(p, 9))
        attn_us = m.profile_kernel("attn", p, reps=4)
        wo_us = m.profile_kernel("wo", p, reps=4)
        # between position 256 and the GQA group path the split partials are merged by the wo kernel
        # (k_wo_comb): what that adds to wo is attention time and is charged to it here
        merge_us = max(0.0, wo_us - wo_short)
        kv_bytes = 2.0 * (p + 1) * spec.kv_dim * 4
        out[str(p)] = {"step_us": round(us[len(us) // 2], 2), "attn_us_per_layer": round(attn_us + merge_us, 2),
                       "attn_kernel_us": round(attn_us, 2), "wo_us": round(wo_us, 2),
                       "wo_us_plain_input": round(wo_short, 2),
                       "attn_kv_bytes_per_layer": kv_bytes,
                       "attn_kv_frac": kv_bytes / ((attn_us + merge_us) * 1e-6) / (HBM_PEAK_GBS * 1e9)}
    return out


def load_probe(spec, img_dev, device_index, gpu_words):
    """Model::read_model_file + to_cuda (model.cpp:41-123) timed on a real file - the .bin
    image the GPU just decoded from, written to /dev/shm (page-cache resident, as a second load of a
    checkpoint is), loaded with kh_model_create_from_file (mmap -> double-buffered pinned chunks -> one
    HBM arena), then 8 greedy steps as a sanity check against the words of the timed run."""
    from kuiperllama_amd.model import KuiperModel
    nbytes = int(img_dev.numel())
    st = os.statvfs("/dev/shm")
    if st.f_bavail * st.f_frsize < nbytes + (1 << 30) or host_mem_available_gb() < 2 * nbytes / 1e9 + 4:
        return {"skipped": "not enough /dev/shm or host memory for the image"}
    path = f"/dev/shm/kh_bench_{os.getpid()}.bin"
    try:
        img_dev.cpu().numpy().tofile(path)
        t0 = time.perf_counter()
        m = KuiperModel.from_file(path, spec, device=device_index)
        wall = time.perf_counter() - t0
        up_ms = m.load_ms
        words, _ = m.generate(PROMPT, 8, exec="graph")
        m.close()
    finally:
        if os.path.exists(path):
            os.unlink(path)
    return {"bytes": nbytes, "ms": round(wall * 1e3, 1), "GB/s": round(nbytes / wall / 1e9, 2),
            "upload_ms": round(up_ms, 1), "upload_GB/s": round(nbytes / (up_ms * 1e-3) / 1e9, 2) if up_ms else None,
            "what": "kh_model_create_from_file on the .bin image in /dev/shm: `ms` = the whole call (open, mmap, "
                    "header, chunked pinned upload, buffers, sin/cos table, launch plans), `upload_ms` = the weight "
                    "upload alone (kh_model_get_load_ms)",
            "decode_matches_timed_run": words == list(gpu_words[:8])}


_T0 = time.time()


def time_left(args) -> float:
    """Seconds left of the wall-clock budget of the optional sections (the contract line must be printed)."""
    return args.budget_s - (time.time() - _T0)


def measure(spec, args, rank, world, local_rank, primary):
    from kuiperllama_amd import replicas
    dev = torch.device(f"cuda:{local_rank}")
    m, img = build_model(spec, local_rank)
    words, wall, ev_ms = timed_generate(m, args.steps, args.warmup, world, dev)
    # what the last timed step handed its caller, read back before anything else runs on the model
    outputs = ({"words": np.asarray(words, dtype=np.float64), "logits": m.logits()}
               if primary and args.dump_outputs else None)
    tok_s = world * args.steps / wall
    mean_pos = (args.steps - 1) / 2.0
    bytes_tok = spec.algorithmic_bytes_per_token(mean_pos)
    # every replica's own rate (HIP events around its step loop), gathered for the spread
    per = replicas.gather_per_replica(args.steps / (ev_ms * 1e-3), world, dev)
    out = {
        "value": tok_s, "ms_per_step": 1e3 * wall / args.steps, "hip_event_ms": ev_ms,
        "bytes_per_token": bytes_tok,
        "step_gbs": bytes_tok * (args.steps / wall) / 1e9,
        "words_head": words[:8],
        "replicas": replicas.spread(per),
    }
    cfg = getattr(m, "cfg", None)  # kh_config: what the self-checks of kh_model_create_* decided for this model
    out["selftests"] = {"ring": getattr(cfg, "ring_selftest", None), "attn_merge": getattr(cfg, "attn_merge_selftest", None),
                        "legend": "0 n/a, 1 passed, -1 failed: fallback in use, 2 (attn_merge) fenced form requested"}
    if hasattr(m, "kv_bytes"):
        kv_res, kv_com = m.kv_bytes()
        out["kv_cache"] = {"reserved_bytes": kv_res, "committed_bytes_after_timed_run": kv_com,
                           "what": "address range of the reference's [layer, seq_len, kv_dim] x 2 allocation vs the HBM "
                                   "mapped behind it after the timed run (8-MiB chunks, on demand)"}
    if outputs is not None:
        out["outputs"] = outputs
    if not args.full:  # a plain run: the timed region is all it measures
        m.close()
        return out
    ref_words = words
    if args.extras:
        # SURVEY 8d extras, all outside the contract's timed region: repeated runs (median) and the
        # single-step latency at pos 0 / 64 / 127
        reps = []
        for _ in range(max(0, args.repeats - 1)):
            _, ms = m.generate(PROMPT, args.steps, exec="graph")
            reps.append(args.steps / (ms * 1e-3))
        if reps:
            allr = sorted(reps + [args.steps / (ev_ms * 1e-3)])
            out["runs"] = {"n": len(allr), "median_tok_s": allr[len(allr) // 2], "min_tok_s": allr[0],
                           "max_tok_s": allr[-1], "clock": "HIP events around the step loop, per replica"}
        # the 128-step greedy run of the metric's definition (SURVEY 8d / demo/main.cpp:69), untimed by
        # the contract when --steps is smaller: source of the CPU token comparison
        ref_steps = max(args.steps, args.cpu_tokens, 128)
        ref_words, ref_ms = (words, ev_ms) if ref_steps == args.steps else m.generate(PROMPT, ref_steps, exec="graph")
        out["tok_s_128_steps"] = ref_steps / (ref_ms * 1e-3)
        out["tok_s_128_steps_is"] = (f"the SURVEY 8(d) metric: {ref_steps} greedy steps from pos 0 (demo/main.cpp:69, "
                                     "mean pos 63.5), HIP events around the step loop; `value` is the same loop over "
                                     "--steps steps on the driver's clock")
        lat = {}
        for p in (0, 64, 127):
            us = sorted(m.time_step(p, 9))
            lat[str(p)] = round(us[len(us) // 2], 2)
        out["latency_us_at_pos"] = lat
    # prompt phase (extends the reference): 128 fed-only prompt tokens, timed alone
    # with HIP events on the model stream (kh_model_time_prefill)
    if args.extras and (primary or args.prefill_secondary):
        rng = np.random.default_rng(0)
        pp = [int(t) for t in rng.integers(0, spec.vocab_size, 128)]
        pf = {}
        for mode in ("gemm", "gemv", "token"):
            try:
                pf[mode] = min(m.time_prefill(pp, 0, mode) for _ in range(3))
            except Exception as e:  # noqa: BLE001
                pf[mode] = None
                log(f"[bench] prefill mode {mode}: {e!r}")
        out["prefill"] = {"prompt_tokens": len(pp)}
        names = {"gemm": "mfma_gemm", "gemv": "b_token_gemv", "token": "token_by_token"}
        for mode, ms in pf.items():
            if ms:
                out["prefill"][names[mode] + "_tok_s"] = len(pp) / (ms * 1e-3)
        if pf.get("gemm") and pf.get("token"):
            out["prefill"]["speedup_gemm_vs_token"] = pf["token"] / pf["gemm"]
        # longer prompts: one weight pass takes up to 512 tokens (the small-M GEMMs then get the big
        # register tile), 1024 = two such passes with causal attention over up to 1024 timesteps
        if pf.get("gemm"):
            for n in (512, 1024):
                if spec.seq_len < n:
                    continue
                try:
                    lp = [int(t) for t in rng.integers(0, spec.vocab_size, n)]
                    m.time_prefill(lp, 0, "gemm")
                    ms = min(m.time_prefill(lp, 0, "gemm") for _ in range(2))
                    out["prefill"][f"mfma_gemm_{n}_prompt_tok_s"] = len(lp) / (ms * 1e-3)
                except Exception as e:  # noqa: BLE001
                    log(f"[bench] {n}-token prefill: {e!r}")
        out["prefill"]["note"] = ("mfma_gemm: fp32-MFMA GEMMs + MFMA causal attention, weights streamed once per "
                                  "pass of up to 512 prompt tokens (prompt_tokens = 128: one 128-token pass), fp32 "
                                  "tolerance vs the oracle; b_token_gemv: 8/4 tokens per weight pass on the VALU, "
                                  "bit-identical to token_by_token (the reference's prompt phase)")
    # per-kernel durations measured live with HIP events on the model's stream.  The roofline
    # figure uses back-to-back launches of the kernel over all layers between two events (no
    # event between launches); "kernels_avg_us_evented" is the whole step with an event after
    # every kernel (adds ~3 us per kernel, kept as a cross-check of the launch sequence).
    ppos = min(args.steps - 1, 64)
    b2b = m.profile_kernels(ppos, reps=8)
    k_us = b2b["ffn13"]
    kb = ffn13_bytes(spec)
    achieved = kb / (k_us * 1e-6) / 1e9
    tr, tr_src = load_traffic(f"{spec.name}:ffn13")
    L = spec.n_layers
    out["roofline"] = {
        "bound": "hbm", "kernel": "k_ffn13 (w1,w3 GEMV + SwiGLU)", "achieved": achieved,
        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": tr, "traffic_source": tr_src, "bytes_per_launch": kb, "avg_launch_us": k_us,
        "step": {"achieved": out["step_gbs"], "frac": out["step_gbs"] / HBM_PEAK_GBS,
                 "bytes_per_token": bytes_tok},
        "kernels_avg_us": {n: round(v, 3) for n, v in b2b.items()},
        "kernels_sum_us_per_token": round(sum(v * (L if n not in ("cls", "sample") else 1)
                                              for n, v in b2b.items()), 1),
    }
    if args.extras:
        prof = m.profile_step(start_pos=ppos, n_steps=8)
        out["roofline"]["kernels_avg_us_evented"] = {n: round(v["avg_us"], 3) for n, v in prof.items()}
        if primary and world == 1 and time_left(args) > 60:
            try:
                lc = long_context(m, spec, dev)
                if lc:
                    out["long_context"] = lc
            except Exception as e:  # noqa: BLE001  (the contract's numbers must still be reported)
                out["long_context"] = {"error": repr(e)}
    gpu_logits = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.extras:
        # logits of greedy step LOGIT_CHECK_POS of the same prompt, for the record's own tolerance check
        m.generate(PROMPT, LOGIT_CHECK_POS + 1, exec="graph")
        gpu_logits = (LOGIT_CHECK_POS, m.logits())
    m.close()
    del m
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.extras:
        if primary:
            img_h = img.cpu().numpy()
            ref = None
            try:
                ref = cpu_baseline_reference(spec, img_h, ref_words, args.cpu_tokens, args.cpu_budget_s,
                                             gpu_logits=gpu_logits)
            except Exception as e:  # noqa: BLE001  (fall back to the port, say why)
                log(f"[bench] reference CPU backend unavailable: {e!r}")
                out["cpu_baseline_reference_error"] = repr(e)
            if ref is not None:
                # the reference's own CPU backend is the reported baseline; the oracle ("port": the restatement the
                # parity tests use) is timed beside it on a shorter sample, and carries the logit check vs the oracle
                port = cpu_baseline(spec, img_h, ref_words, min(args.cpu_tokens, 48), max(4.0, args.cpu_budget_s / 3),
                                    min_sample_s=4.0, gpu_logits=gpu_logits)
                ref["port"] = {k: port[k] for k in ("value", "unit", "cores", "kind", "sample", "variant",
                                                    "tokens_match_gpu", "tokens_compared", "max_logit_err_vs_oracle")}
                ref["max_logit_err_vs_oracle"] = port["max_logit_err_vs_oracle"]
                out["cpu_baseline"] = ref
            else:
                out["cpu_baseline"] = cpu_baseline(spec, img_h, ref_words, args.cpu_tokens, args.cpu_budget_s,
                                                   gpu_logits=gpu_logits)
            del img_h
        elif spec.name == "llama2-7b-int8":
            try:
                out["cpu_baseline"] = cpu_int8_restated(spec, img, args, ref_words, gpu_logits)
                out["max_logit_err_vs_oracle"] = out["cpu_baseline"]["cpu_int8_restated"]["max_logit_err_vs_oracle"]
            except Exception as e:  # noqa: BLE001  (the GPU numbers must still be reported)
                out["cpu_baseline"] = {"error": repr(e)}
    if primary and rank == 0 and world == 1 and args.extras and time_left(args) > 30:
        try:
            out["load"] = load_probe(spec, img, local_rank, words)
        except Exception as e:  # noqa: BLE001
            out["load"] = {"error": repr(e)}
    del img
    torch.cuda.empty_cache()
    return out


DEFAULT_OTHERS = "stories15M,qwen2.5-0.5b,tinyllama-1.1b,llama2-7b"
NORTH_STAR_FLOOR = {"config": "tinyllama-1.1b", "target_tok_s": 60.0,
                    "source": "north_star: >= the reference's 60 tok/s on TinyLlama-1.1B fp32 "
                              "(/root/reference/readme.md:25: 60.34 tok/s, RTX 3060 Laptop)"}


def _flat_first(d: dict) -> dict:
    """Scalars before nested objects (key order is the print order): a reader that keeps only scalar members
    of `roofline` / `config`, or only the head of a long object, still gets the numbers."""
    return {**{k: v for k, v in d.items() if not isinstance(v, (dict, list))},
            **{k: v for k, v in d.items() if isinstance(v, (dict, list))}}


DATA = ("synthetic via kuiperllama_amd.binfmt.synth_image (seeded torch RNG on the GPU, the "
        "reference exporter's .bin byte layout and init std; not the reference exporter itself)")
DUMP_LIMIT_BYTES = 64 << 20


def _contract_head(spec, args, world, res) -> dict:
    """The contract's scalar keys, in the contract's order: the head of every line."""
    return {"metric": "decode tokens/sec",
            "value": res["value"], "unit": "tokens/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": res["ms_per_step"], "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "int8 weights x f32 activations" if spec.quant else "f32"}


def _config_head(spec, args, world, timing_backend) -> dict:
    return {"workload": f"{spec.name} greedy decode, batch 1, prompt {PROMPT}, "
                        f"{args.steps} steps from pos 0 (demo/main.cpp generate)",
            "parallelism": f"replicas{world} (no shard, no data-path collective; one process "
                           f"per GPU, HIP_VISIBLE_DEVICES/LOCAL_RANK pinning)",
            "timing_backend": timing_backend,
            "exec": "hipGraph replay, 5L+2 fused HIP kernels per token",
            "kv_cache_rows": spec.seq_len}


def plain_line(spec, args, world, res, timing_backend) -> dict:
    """The line of a plain run (no --full): the contract's keys and what the timed run itself reported."""
    return {**_contract_head(spec, args, world, res),
            "hip_event_ms": res["hip_event_ms"], "step_gbs": res["step_gbs"], "data": DATA,
            "config": _config_head(spec, args, world, timing_backend),
            "replicas": res["replicas"], "kv_cache": res.get("kv_cache"), "selftests": res.get("selftests"),
            "words_head": res["words_head"]}


def dump_outputs(out_dir: str, outputs: dict) -> None:
    """outputs {name: float32 / float64 array} -> out_dir/<name>.npy, at most DUMP_LIMIT_BYTES in all."""
    total = sum(a.nbytes for a in outputs.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes > {DUMP_LIMIT_BYTES}")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in outputs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, name + ".npy"), a)


def assemble_line(spec, args, world, res, secondary, others, skipped, timing_backend) -> dict:
    """The ONE JSON line.  Both halves of BASELINE.json's metric (Llama-3.2-1B fp32 and Llama-2-7B int8 decode
    tok/s) and their roofline fractions are carried as SCALARS inside `roofline` and `config` (a record parser that
    keeps the contract's objects but only the names of extra top-level keys loses `secondary` otherwise), the
    contract's scalar keys come first, the bulky sections last, and `summary` repeats the scalars at the very end
    (a tail of the line that lost its head still has them).  tests/test_bench_logic.py pins this layout."""
    sec_ok = isinstance(secondary, dict) and "value" in secondary
    sr = secondary["roofline"] if sec_ok else {}
    summary = {
        "value": res["value"], "ms_per_step": res["ms_per_step"],
        "tok_s_128_steps": res.get("tok_s_128_steps"),
        "kernel_frac": res["roofline"]["frac"], "step_frac": res["roofline"]["step"]["frac"],
        "secondary_workload": secondary["config"]["workload"] if sec_ok else None,
        "secondary_value": secondary["value"] if sec_ok else None,
        "secondary_ms_per_step": secondary["ms_per_step"] if sec_ok else None,
        "secondary_tok_s_128_steps": secondary.get("tok_s_128_steps") if sec_ok else None,
        "secondary_kernel_frac": sr.get("frac"),
        "secondary_step_frac": sr.get("step", {}).get("frac"),
    }
    roofline = dict(res["roofline"])
    roofline["step_frac"] = summary["step_frac"]
    roofline["step_achieved"] = res["roofline"]["step"]["achieved"]
    roofline["secondary_frac"] = summary["secondary_kernel_frac"]
    roofline["secondary_achieved"] = sr.get("achieved")
    roofline["secondary_step_frac"] = summary["secondary_step_frac"]
    roofline["secondary_step_achieved"] = sr.get("step", {}).get("achieved")
    config = {**_config_head(spec, args, world, timing_backend),
              "tok_s_128_steps": summary["tok_s_128_steps"],
              "secondary_workload": summary["secondary_workload"],
              "secondary_value": summary["secondary_value"],
              "secondary_ms_per_step": summary["secondary_ms_per_step"],
              "secondary_tok_s_128_steps": summary["secondary_tok_s_128_steps"],
              "kv_cache_committed_bytes": (res.get("kv_cache") or {}).get("committed_bytes_after_timed_run"),
              "kv_cache_reserved_bytes": (res.get("kv_cache") or {}).get("reserved_bytes"),
              "selftest_ring": res.get("selftests", {}).get("ring"),
              "selftest_attn_merge": res.get("selftests", {}).get("attn_merge"),
              "secondary_selftest_ring": (secondary.get("selftests") or {}).get("ring") if sec_ok else None,
              "secondary_selftest_attn_merge": (secondary.get("selftests") or {}).get("attn_merge") if sec_ok else None}
    line = {
        **_contract_head(spec, args, world, res),
        "tok_s_128_steps": summary["tok_s_128_steps"],
        "secondary_value": summary["secondary_value"],
        "secondary_ms_per_step": summary["secondary_ms_per_step"],
        "secondary_step_frac": summary["secondary_step_frac"],
        "data": DATA,
        "config": config,
        "roofline": _flat_first(roofline),
    }
    if "cpu_baseline" in res:
        line["cpu_baseline"] = _flat_first(res["cpu_baseline"])
    line["replicas"] = res["replicas"]
    if "kv_cache" in res:
        line["kv_cache"] = res["kv_cache"]
    line["selftests"] = res.get("selftests")
    line["runs"] = res.get("runs")
    line["tok_s_128_steps_is"] = res.get("tok_s_128_steps_is")
    line["latency_us_at_pos"] = res.get("latency_us_at_pos")
    line["prefill"] = res.get("prefill")
    if "long_context" in res:
        line["long_context"] = res["long_context"]
    if "load" in res:
        line["load"] = res["load"]
    if skipped:
        line["skipped_sections"] = skipped
    if secondary is not None:
        line["secondary"] = secondary
    if others:
        line["other_configs"] = others
        fl = others.get(NORTH_STAR_FLOOR["config"])
        if fl and "value" in fl:
            line["north_star_floor"] = dict(NORTH_STAR_FLOOR, tok_s=fl["value"],
                                            met=bool(fl["value"] >= NORTH_STAR_FLOOR["target_tok_s"]),
                                            tokens_match=fl.get("tokens_match"))
    line["summary"] = summary
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)  # generate(model, "a", 128), main.cpp:69
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--workload", default=None, choices=sorted(binfmt.PRESETS),
                    help="default: llama3.2-1b on one GPU (BASELINE configs[1]); llama2-7b fp32 for "
                         "N > 1 (configs[4]: independent replicas)")
    ap.add_argument("--secondary", default=None,
                    help="second workload of the metric, measured in the same run ('' = none; "
                         "default llama2-7b-int8 on one GPU, none for N > 1)")
    ap.add_argument("--repeats", type=int, default=5,
                    help="extra untimed-by-the-contract runs for the median (SURVEY 8d)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-tokens", type=int, default=128)
    ap.add_argument("--cpu-budget-s", type=float, default=25.0)
    ap.add_argument("--prefill-secondary", action=argparse.BooleanOptionalAction, default=True,
                    help="also time the prompt phase of the secondary workload")
    ap.add_argument("--extras", action=argparse.BooleanOptionalAction, default=True,
                    help="--full --no-extras: only the contract's timed region and the roofline kernel (no "
                         "repeated runs, 128-step reference run, latency probes, prefill, long context, CPU "
                         "baseline, other configs)")
    ap.add_argument("--others", default=None,
                    help=f"comma-separated further BASELINE configs measured briefly into the same line "
                         f"(default on one GPU: {DEFAULT_OTHERS}; '' or --no-others: none)")
    ap.add_argument("--budget-s", type=float, default=420.0,
                    help="wall-clock budget of the whole command: optional sections (long context, load probe, "
                         "other configs) that would start after it are skipped and named in `skipped_sections`, "
                         "so the contract line is always printed")
    ap.add_argument("--no-others", action="store_true",
                    help="skip the other BASELINE configs (rocprofv3 runs: they launch the same kernel "
                         "instantiations at other sizes and would blur the --stats average)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the timed region: secondary workload, roofline kernel timings, CPU "
                         "baselines, other configs, latency / prefill / long-context / load probes (the options "
                         "above shape these sections; a plain run is set-up, warm-up, timed steps and the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the words and last-step logits of the timed run as DIR/<name>.npy")
    args = ap.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the decode path has no CPU fallback")
    from kuiperllama_amd import replicas
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    # RCCL carries the timing protocol; KH_BENCH_DIST_BACKEND=gloo is the CPU test hook
    # (tests/test_bench_main_gloo.py runs this function with world_size 2 and no GPU)
    rank, world, local_rank = replicas.init_from_env(os.environ.get("KH_BENCH_DIST_BACKEND", "nccl"),
                                                     torch.device(f"cuda:{local_rank}"))
    if world != args.gpus:
        log(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    if args.workload is None:
        args.workload = replicas.default_workload(world)
    spec = binfmt.PRESETS[args.workload]
    if not args.full:
        res = measure(spec, args, rank, world, local_rank, primary=True)
        if rank == 0:
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, res["outputs"])
            print(json.dumps(plain_line(spec, args, world, res, replicas.backend_in_use(world))), flush=True)
        replicas.shutdown(world)
        return
    if args.secondary is None:
        args.secondary = "llama2-7b-int8" if world == 1 else ""
    if args.others is None:
        args.others = DEFAULT_OTHERS if world == 1 else ""
    if args.no_others or not args.extras:
        args.others = ""

    skipped = []
    res = measure(spec, args, rank, world, local_rank, primary=True)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, res["outputs"])
    secondary = None
    if args.secondary and args.secondary != args.workload:
        try:
            s2 = binfmt.PRESETS[args.secondary]
            r2 = measure(s2, args, rank, world, local_rank, primary=False)
            secondary = {"config": {"workload": f"{s2.name} greedy decode, batch 1, "
                                                f"{args.steps} steps, replicas{world}"},
                         "value": r2["value"], "unit": "tokens/s", "ms_per_step": r2["ms_per_step"],
                         "dtype": "int8 weights x f32 activations" if s2.quant else "f32",
                         "roofline": r2["roofline"], "runs": r2.get("runs"),
                         "tok_s_128_steps": r2.get("tok_s_128_steps"),
                         "latency_us_at_pos": r2.get("latency_us_at_pos"),
                         "prefill": r2.get("prefill"), "selftests": r2.get("selftests")}
            if "cpu_baseline" in r2:
                secondary["cpu_baseline"] = r2["cpu_baseline"]
            if "max_logit_err_vs_oracle" in r2:
                secondary["max_logit_err_vs_oracle"] = r2["max_logit_err_vs_oracle"]
        except Exception as e:  # the primary number must still be reported
            secondary = {"error": repr(e)}

    others = None
    if args.others:
        others = {}
        torch.cuda.empty_cache()
        for w in [x for x in args.others.split(",") if x and x not in (args.workload, args.secondary)]:
            # the 26 GB fp32 image needs ~90 s (synthesis, 3 x 128 steps, host copy, CPU pass); the rest ~10 s
            if time_left(args) < (100 if binfmt.image_nbytes(binfmt.PRESETS[w]) > 8e9 else 15):
                skipped.append(f"other_configs.{w}")
                continue
            try:
                others[w] = other_config(binfmt.PRESETS[w], local_rank, args)
            except Exception as e:  # noqa: BLE001 - the contract's numbers must still be reported
                others[w] = {"error": repr(e)}

    if rank == 0:
        line = assemble_line(spec, args, world, res, secondary, others, skipped, replicas.backend_in_use(world))
        print(json.dumps(line), flush=True)
    replicas.shutdown(world)


if __name__ == "__main__":
    main()
