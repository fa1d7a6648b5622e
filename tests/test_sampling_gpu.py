"""Seeded temperature / top-k / top-p sampling on the GPU (csrc/kh_sample.h): the operator against the fp64
semantics of tests/sampling_ref.py, and the model paths (graph, fused, unfused; generate, generate_until, predict)
token by token against the same checker on the model's own logits."""
import subprocess

import numpy as np
import pytest
import torch

import sampling_ref as R
from conftest import load_golden
from kuiperllama_amd import _ffi, binfmt, build, ops

pytestmark = pytest.mark.gpu


def _logits(kind, V, seed=0):
    rng = np.random.default_rng(seed + V)
    if kind == "peaked":  # Zipf-like: l = -1.1 ln(rank), ranks shuffled over the vocabulary
        lg = -1.1 * np.log(rng.permutation(V) + 1.0)
    elif kind == "flat":
        lg = rng.normal(0.0, 0.5, V)
    else:  # "tied": few distinct values, ties everywhere (top-k / top-p edges fall inside runs of equal logits)
        lg = np.round(rng.normal(0.0, 1.0, V) * 4) / 4
    return lg.astype(np.float32)


def _draw(lg_d, T, K, P, seed, n, counter0=0):
    out = torch.empty(n, dtype=torch.int32, device=lg_d.device)
    ops.sample(lg_d, out, dict(temperature=T, top_k=K, top_p=P, seed=seed), counter0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("V", [501, 32000, 128256, 151936])
@pytest.mark.parametrize("kind", ["peaked", "flat", "tied"])
def test_operator_draws_are_the_semantics_picks(gpu, V, kind):
    lg = _logits(kind, V)
    lg_d = torch.from_numpy(lg).to(gpu)
    ch = R.Checker(lg)
    am = torch.empty(1, dtype=torch.int32, device=gpu)
    ops.argmax(lg_d, am)
    torch.cuda.synchronize()
    seed = 0x1234_5678_9ABC + V
    n = 256
    for T in (0.3, 1.0, 2.0):
        for K in (0, 1, 50, 1000, V):
            for P in (1.0, 0.95, 0.5, 1e-6):
                got = _draw(lg_d, T, K, P, seed, n, counter0=17)
                ok = ch.accepts(T, K, P, seed, np.arange(17, 17 + n), got)
                assert ok.all(), (f"V={V} {kind} T={T} K={K} P={P}: {int((~ok).sum())} draws rejected, first "
                                  f"counter {17 + int(np.argmin(ok))} pick {got[np.argmin(ok)]}")
                if K == 1:
                    assert (got == int(am.item())).all()
                if T == 1.0 and P in (1.0, 0.95):  # bit-reproducible from call to call
                    assert (_draw(lg_d, T, K, P, seed, n, counter0=17) == got).all()


def test_operator_greedy_and_host_form(gpu):
    lg = _logits("flat", 32000, 5)
    lg_d = torch.from_numpy(lg).to(gpu)
    assert (_draw(lg_d, 0.0, 50, 0.9, 1, 300) == int(np.argmax(lg))).all()
    assert (_draw(lg_d, -2.0, 0, 1.0, 1, 1) == int(np.argmax(lg))).all()
    many = _draw(lg_d, 0.8, 40, 0.9, 99, 8, counter0=1000)
    for i in range(8):
        assert ops.sample_host(lg_d, _ffi.sampling(0.8, 40, 0.9, 99), 1000 + i) == many[i]
    # unaligned logits (operator entry with an odd offset): same semantics
    sub = lg_d[1:]
    got = _draw(sub, 1.0, 0, 0.95, 3, 64)
    assert R.Checker(lg[1:]).accepts(1.0, 0, 0.95, 3, np.arange(64), got).all()


def test_operator_distribution_chi_square(gpu):
    from scipy import stats
    V, n = 1000, 100_000
    rng = np.random.default_rng(42)
    lg = rng.normal(0.0, 1.5, V).astype(np.float32)
    lg_d = torch.from_numpy(lg).to(gpu)
    for T, K, P in ((1.0, 0, 1.0), (0.7, 200, 0.9)):
        got = _draw(lg_d, T, K, P, 20240917, n)
        S, w, _ = R.kept_set(lg, T, K, P)
        p = np.zeros(V)
        p[S] = w / w.sum()
        assert p[got].min() > 0, "a token outside S was drawn"
        cnt = np.bincount(got, minlength=V)[S]
        exp = p[S] * n
        chi2 = ((cnt - exp) ** 2 / exp).sum()
        pval = stats.chi2.sf(chi2, len(S) - 1)
        assert pval > 1e-4, (T, K, P, chi2, pval)


# ---- model paths -------------------------------------------------------------------------------------------------
def _golden_model(name, flags=0):
    from kuiperllama_amd.model import KuiperModel
    spec, img, toks, _ = load_golden(name)
    return KuiperModel.from_host_image(img, spec, flags=flags), spec, img, toks


def _synth_model(preset, gpu, seed=1234, max_seq_len=256, flags=0):
    from kuiperllama_amd.model import KuiperModel
    spec = binfmt.PRESETS[preset] if isinstance(preset, str) else preset
    img_d = binfmt.synth_image(spec, seed=seed, device=gpu)
    torch.cuda.synchronize()
    return KuiperModel.from_device_image(img_d, spec, max_seq_len=max_seq_len, flags=flags), spec


def _fed(prompt, words, p):
    return int(prompt[p]) if p < len(prompt) else int(words[p - 1])


def _replay_check(m, prompt, words, samp, exec="fused", check_equal=True):
    """predict() one position at a time over the fed tokens; every sampled word must be the checker's pick for
    Philox(seed, pos) on that position's logits (and, on the same kernels, the predict draw itself)."""
    T, K, P, seed = samp
    for p in range(len(words)):
        nxt = m.predict(_fed(prompt, words, p), p, is_prompt=p < len(prompt) - 1, exec=exec)
        if p < len(prompt) - 1:
            assert words[p] == prompt[p + 1]
            continue
        lg = m.logits()
        assert R.Checker(lg).accepts(T, K, P, seed, [p], [words[p]]).all(), (exec, p, words[p])
        if check_equal:
            assert nxt == words[p], (exec, p, nxt, words[p])


CASES = [("golden-f32", 0.9, 0, 0.95), ("golden-int8", 1.2, 20, 1.0), ("llama3.2-1b", 0.8, 50, 0.95)]


@pytest.mark.parametrize("case,T,K,P", CASES)
def test_model_every_sampled_token_is_checked(gpu, case, T, K, P):
    if case == "golden-f32":
        m, spec, _, toks = _golden_model("hf_llama_half")
        prompt = [int(t) for t in toks[:3]]
    elif case == "golden-int8":
        m, spec, _, toks = _golden_model("ref_llama_int8_untied")
        prompt = [int(t) for t in toks[:2]]
    else:
        m, spec = _synth_model(case, gpu, max_seq_len=128)
        prompt = [1, 263]
    seed = 0xC0FFEE
    m.set_sampling(T, K, P, seed)
    assert m.sampling == {"temperature": pytest.approx(T), "top_k": K, "top_p": pytest.approx(P), "seed": seed}
    steps = min(64, spec.seq_len)
    words, _ = m.generate(prompt, steps, exec="graph")
    assert len(words) == steps
    assert len(set(words[len(prompt) - 1:])) > 3  # sampled, not one id repeated
    _replay_check(m, prompt, words, (T, K, P, seed))
    m.close()


def test_model_modes_chunkings_and_entry_points_agree(gpu):
    m, spec, _, toks = _golden_model("hf_llama_half")
    prompt = [int(t) for t in toks[:3]]
    m.set_sampling(1.0, 0, 0.9, 77)
    g, _ = m.generate(prompt, 64, exec="graph")
    f, _ = m.generate(prompt, 64, exec="fused")
    assert g == f
    short, _ = m.generate(prompt, 13, exec="graph")
    assert short == g[:13]
    absent = next(t for t in range(spec.vocab_size) if t not in g)
    u, _ = m.generate(prompt, 64, exec="graph", stop=[absent])
    assert u == g
    # unfused: the reference's launch sequence with kh_sample_f32 in place of the argmax
    un, _ = m.generate(prompt, 40, exec="unfused")
    _replay_check(m, prompt, un, (1.0, 0, 0.9, 77), exec="unfused")
    m.close()


PREFILL_SPEC = binfmt.ModelSpec(512, 1408, 2, 8, 2, 4096, 160, True, binfmt.FAMILY_LLAMA, False, 64,
                                binfmt.ROPE_HALF, 500000.0, 1e-5, "prefill-synth")


def test_model_prompt_prefill_paths(gpu):
    from kuiperllama_amd.model import KuiperModel
    spec = PREFILL_SPEC
    img_d = binfmt.synth_image(spec, seed=21, device=gpu)
    torch.cuda.synchronize()
    rng = np.random.default_rng(8)
    prompt = [int(t) for t in rng.integers(0, spec.vocab_size, 20)]
    samp = (0.9, 40, 0.95, 5)
    m = KuiperModel.from_device_image(img_d, spec, max_seq_len=128, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    m.set_sampling(*samp)
    words, _ = m.generate(prompt, 68, exec="graph")
    assert m.first_sample()["prefill_mode"] == "gemv"
    _replay_check(m, prompt, words, samp)
    m.close()
    # default GEMM prefill: the requested words, the first sampled word keyed at position n_prompt - 1
    m = KuiperModel.from_device_image(img_d, spec, max_seq_len=128)
    m.set_sampling(*samp)
    words, _ = m.generate(prompt, 48, exec="graph")
    assert len(words) == 48 and words[:len(prompt) - 1] == prompt[1:]
    assert m.first_sample()["prefill_mode"] == "gemm"
    one, _ = m.generate(prompt, len(prompt), exec="graph")  # the first sampled step is the last one: its logits
    lg = m.logits()
    assert one[-1] == words[len(prompt) - 1]
    lg_d = torch.from_numpy(lg).to(gpu)
    assert _draw(lg_d, *samp, 1, counter0=len(prompt) - 1)[0] == one[-1]
    assert R.Checker(lg).accepts(*samp, [len(prompt) - 1], [one[-1]]).all()
    m.close()


def test_seeds_and_stop_tokens(gpu):
    spec = binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 128, True, binfmt.FAMILY_LLAMA, False, 64,
                            binfmt.ROPE_HALF, 500000.0, 1e-5, "flat-synth")
    m, _ = _synth_model(spec, gpu, seed=3, max_seq_len=128)
    prompt = [1, 263]
    runs = []
    for seed in (1, 2, 3):
        m.set_sampling(1.0, 0, 1.0, seed)
        runs.append(m.generate(prompt, 80, exec="graph")[0])
    assert runs[0] != runs[1] and runs[1] != runs[2] and runs[0] != runs[2]
    m.set_sampling(1.0, 0, 1.0, 1)
    again, _ = m.generate(prompt, 80, exec="graph")
    assert again == runs[0]
    full = runs[0]
    k = next(i for i in range(len(prompt) + 8, len(full)) if full[i] not in full[len(prompt) - 1:i])
    for ex in ("graph", "fused"):
        until, _ = m.generate(prompt, 80, exec=ex, stop=[full[k]])
        assert until == full[:k], ex
    m.close()


def test_greedy_is_untouched(gpu, oracle):
    m, spec, img, toks = _golden_model("hf_llama_half")
    prompt = [int(t) for t in toks[:2]]
    want = oracle.OracleModel.from_spec(img, spec).generate(prompt, 32)
    lpt = m.cfg.launches_per_token
    assert lpt == 5 * spec.n_layers + 2
    m.set_sampling(0.7, 0, 0.9, 11)
    sampled, _ = m.generate(prompt, 32, exec="graph")
    assert sampled != want
    counts = m.profile_step(1, 2)
    assert sum(v["launches_per_step"] for v in counts.values()) == lpt
    m.set_sampling()
    assert m.sampling["temperature"] == 0.0
    for ex in ("graph", "fused"):
        assert m.generate(prompt, 32, exec=ex)[0] == want, ex
    m.close()


def test_demo_cli_sampling(gpu, tmp_path):
    spec, img, toks, _ = load_golden("hf_llama_half")
    path = tmp_path / "m.bin"
    img.tofile(path)
    prompt = [int(t) for t in toks[:3]]
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--steps", "40", "--prompt", ",".join(map(str, prompt)), "--temperature", "0.9", "--top-k", "30",
            "--top-p", "0.9", "--seed", "123456789"]
    outs = []
    for _ in range(2):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([int(t) for t in r.stdout.strip().splitlines()[1].split()])
    assert outs[0] == outs[1]
    from kuiperllama_amd.model import KuiperModel
    m = KuiperModel.from_host_image(img, spec)
    m.set_sampling(0.9, 30, 0.9, 123456789)
    assert m.generate(prompt, 40, exec="graph")[0] == outs[0]
    m.close()
    bad = subprocess.run(args[:-2] + ["--top-p", "1.5"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
