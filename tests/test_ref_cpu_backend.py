"""The reference's OWN CPU backend as the checker (north_star: "outputs match the reference CPU (armadillo/OpenBLAS)
backend token-for-token").  oracle/_ref/ref_cpu_model{,_llama3,_qwen2} = the reference's model / operator classes, CPU
getters and its ten CPU kernels (kuiper/source/op/kernels/cpu/*.cpp) compiled where they lie; only Armadillo itself is a
stand-in (tests/cpp/ref_stubs/armadillo over numpy's OpenBLAS).  Built in the build container (oracle/Makefile
`ref_cpu`), the binaries travel to the GPU box.

CPU tests: the oracle (oracle/kuiper_oracle.c, the restatement every other parity test leans on) against that backend
on the committed goldens - words and LOGITS; what the backend computed there is stored in tests/golden/ref_cpu_backend.npz
(tests/golden/make_ref_cpu_golden.py), so these need no build of it, and run it live as well where it is built.  GPU
tests: the HIP path against it, mid-size and at full size."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from kuiperllama_amd import binfmt, build

TOK = os.path.join(GOLDEN, "spm_llama_like.model")
REF_CPU_GOLDEN = os.path.join(GOLDEN, "ref_cpu_backend.npz")
GOLDEN_NAMES = ["ref_llama_gqa_tied", "ref_llama_mha_untied", "hf_llama_half", "hf_qwen2_half"]
GREEDY_PROMPT = [1, 7, 3]


def greedy_steps(spec):
    return min(24, spec.seq_len)


def _built(spec):
    flavor = build.ref_cpu_flavor(spec)
    return bool(flavor) and os.path.exists(build.REF_CPU_BINS[flavor])


def _exe(spec):
    flavor = build.ref_cpu_flavor(spec)
    exe = build.REF_CPU_BINS.get(flavor) if flavor else None
    if not exe or not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_cpu_model* not built (no reference checkout at build time)")
    return exe


def run_ref_cpu(spec, img, steps, prompt, want_logits=False, threads=8, budget_s=1e9):
    """-> (words, logits [steps, vocab] or None, tokens/s) of the reference CPU backend on this image."""
    exe = _exe(spec)
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        p = os.path.join(td, "m.bin")
        np.asarray(img).tofile(p)
        lp = os.path.join(td, "logits.f32")
        cmd = [exe, p, TOK, str(steps), ",".join(map(str, prompt)), str(budget_s)] + ([lp] if want_logits else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1800,
                           env=dict(os.environ, KH_REF_BLAS_THREADS=str(threads)))
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().split("\n")
        words = [int(x) for x in lines[0].split()[1:]]
        assert "openblas" in lines[1], lines[1]  # the BLAS path, not the stand-in's plain loops
        lg = np.fromfile(lp, dtype=np.float32).reshape(len(words), -1) if want_logits else None
    return words, lg, float(lines[2].split(" = ")[1].split(" tokens/s")[0])


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_oracle_equals_reference_cpu_backend_on_goldens(oracle, name):
    """Pins the oracle against the reference's own C++ CPU code (not only its Python model): teacher-forced over the
    golden's tokens, the logits of LLama2Model / Qwen2Model::forward on kDeviceCPU agree with the oracle's to 1e-6
    and with the reference-Python golden logits to 2e-6; a greedy run gives the same words.  Held against the stored
    outputs of that backend always, and against a live run of it where it is built."""
    spec, img, toks, golden = load_golden(name)
    toks = [int(t) for t in toks]
    steps = greedy_steps(spec)
    z = np.load(REF_CPU_GOLDEN)
    runs = [("stored", z[name + "__logits"], [int(w) for w in z[name + "__words"]])]
    if _built(spec):
        _, lg, _ = run_ref_cpu(spec, img, len(toks), toks, want_logits=True, threads=2)
        w2, _, _ = run_ref_cpu(spec, img, steps, GREEDY_PROMPT, threads=2)
        runs.append(("live", lg, w2))
    want = oracle.OracleModel.from_spec(img, spec).generate(GREEDY_PROMPT, steps)
    for how, lg, w2 in runs:
        assert lg.shape == (len(toks), spec.vocab_size), (how, lg.shape)
        om = oracle.OracleModel.from_spec(img, spec)
        for t, tok in enumerate(toks):
            lo = om.forward(tok, t)
            assert np.abs(lo - lg[t]).max() <= 1e-6, (name, how, t, float(np.abs(lo - lg[t]).max()))
            assert np.abs(golden[t] - lg[t]).max() <= 2e-6, (name, how, t)
        assert w2 == want, (name, how)


_MID = {
    "default-mha": binfmt.ModelSpec(512, 1408, 3, 4, 4, 2048, 160, False, binfmt.FAMILY_LLAMA, False, 64,
                                    binfmt.ROPE_INTERLEAVED, 10000.0, 1e-5, "cpu-mid-llama2"),
    "llama3-gqa": binfmt.ModelSpec(512, 1408, 4, 8, 2, 4096, 160, True, binfmt.FAMILY_LLAMA, False, 64,
                                   binfmt.ROPE_HALF, 500000.0, 1e-5, "cpu-mid-llama3"),
    "qwen2-bias": binfmt.ModelSpec(448, 1216, 3, 7, 1, 3000, 160, True, binfmt.FAMILY_QWEN2, False, 64,
                                   binfmt.ROPE_HALF, 1000000.0, 1e-6, "cpu-mid-qwen2"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_MID))
def test_hip_decode_equals_reference_cpu_backend_mid_size(gpu, name):
    """Token for token and logit by logit against the reference's own CPU backend: 96 greedy steps of the fused
    hipGraph path give the words LLama2Model / Qwen2Model produce on kDeviceCPU, and a teacher-forced pass over 24
    random tokens agrees in every logit to 2e-5 (fp32 round-off of two summation orders)."""
    import torch
    from kuiperllama_amd.model import KuiperModel
    spec = _MID[name]
    fstd = 1.0 if spec.shared_classifier else None
    img = binfmt.synth_image(spec, seed=31, device=gpu, final_norm_std=fstd).cpu().numpy()
    torch.cuda.synchronize()
    steps, prompt = 96, [1, 263]
    want, _, _ = run_ref_cpu(spec, img, steps, prompt)
    m = KuiperModel.from_host_image(img, spec)
    words, _ = m.generate(prompt, steps, exec="graph")
    assert words == want
    assert len(set(want)) >= 5
    rng = np.random.default_rng(3)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, 24)]
    _, lg, _ = run_ref_cpu(spec, img, len(toks), toks, want_logits=True)
    worst = 0.0
    for t, tok in enumerate(toks):
        m.predict(tok, t, exec="fused")
        worst = max(worst, float(np.abs(m.logits() - lg[t]).max()))
    m.close()
    assert worst <= 2e-5, worst
    print(f"{spec.name}: 96 words equal the reference CPU backend's; max |logit - reference CPU| {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("preset,steps", [("llama3.2-1b", 128), ("tinyllama-1.1b", 128), ("qwen2.5-0.5b", 128),
                                          ("stories15M", 128), ("llama2-7b", 24)])
def test_hip_decode_equals_reference_cpu_backend_full_size(gpu, preset, steps):
    """Every fp32 BASELINE config at FULL size against the reference's own CPU backend (the LLAMA3_SUPPORT build for
    Llama-3.2-1B, the QWEN2_SUPPORT build with Qwen2Model for Qwen2.5-0.5B, the plain build for TinyLlama, stories15M
    and Llama-2-7B), at the north-star length of 128 greedy steps (24 for the 26 GB image: 9 tok/s on the host):
    words identical, logits of the last step within 4e-5."""
    import torch
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS[preset]
    need_gb = binfmt.image_nbytes(spec) / 1e9
    try:
        avail = next(int(ln.split()[1]) for ln in open("/proc/meminfo") if ln.startswith("MemAvailable:")) / 1e6
    except (OSError, StopIteration):
        avail = 1e9
    if avail < 2.5 * need_gb + 8:
        pytest.skip(f"host memory {avail:.0f} GB: the image, its /dev/shm copy and the backend's mapping need {2.5 * need_gb + 8:.0f}")
    fstd = 1.0 if spec.shared_classifier else None
    img_d = binfmt.synth_image(spec, seed=1234, device=gpu, final_norm_std=fstd)
    torch.cuda.synchronize()
    img = img_d.cpu().numpy()
    prompt = [1, 263]
    cpus = os.cpu_count() or 8
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            cpus = max(1, int(q) // int(per))
    except (OSError, ValueError):
        pass
    want, lg, tok_s = run_ref_cpu(spec, img, steps, prompt, want_logits=True, threads=min(cpus, 16))
    m = KuiperModel.from_device_image(img_d, spec, max_seq_len=min(spec.seq_len, 1024))
    words, _ = m.generate(prompt, steps, exec="graph")
    assert words == want, next((i, a, b) for i, (a, b) in enumerate(zip(words, want)) if a != b)
    err = float(np.abs(m.logits() - lg[-1]).max())
    m.close()
    # two fp32 summation orders (OpenBLAS's sgemv blocking vs wave-strided + butterfly): each sits a few 1e-5 from the
    # exact value on the 32-layer, 4096-wide model (tests/test_model_gpu.py bounds that one against the fp64 gold run:
    # |HIP - oracle32| <= 3 |oracle32 - gold64|); 4e-5 as everywhere else for the other geometries
    tol = 1e-4 if spec.dim >= 4096 else 4e-5
    assert err <= tol, err
    assert len(set(want)) >= (5 if spec.dim < 1024 else min(20, steps // 2))  # not a fixed point (short cycles on the 15M model)
    print(f"{preset}: {steps} words equal the reference CPU backend's ({tok_s:.1f} tok/s on the host); "
          f"|logit - reference CPU| at the last step {err:.2e}")
