"""Repetition / presence / frequency penalties and logit bias on the GPU (csrc/kh_logit_proc.h): the operator bit for
bit against the numpy float32 twin tests/logit_proc_ref.py, and the model paths (graph, fused, unfused; generate,
generate_until, predict; both prefills) token by token against the twin applied to the model's own raw logits."""
import subprocess

import numpy as np
import pytest
import torch

import logit_proc_ref as R
import sampling_ref as S
from conftest import load_golden
from kuiperllama_amd import _ffi, binfmt, build, ops

pytestmark = pytest.mark.gpu

INF = float("inf")
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)
FLAT_SPEC = binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 128, True, binfmt.FAMILY_LLAMA, False, 64,
                             binfmt.ROPE_HALF, 500000.0, 1e-5, "flat-synth")
PREFILL_SPEC = binfmt.ModelSpec(512, 1408, 2, 8, 2, 4096, 160, True, binfmt.FAMILY_LLAMA, False, 64,
                                binfmt.ROPE_HALF, 500000.0, 1e-5, "prefill-synth")


# ---- 1. operator ----------------------------------------------------------------------------------------------------
def _raw_logits(V):
    rng = np.random.default_rng(V)
    lg = rng.normal(0.0, 2.0, V).astype(np.float32)
    kind = rng.integers(0, 8, V)
    lg[kind == 0] = 0.0
    lg[kind == 1] = -INF
    lg[int(rng.integers(0, V))] = 9.5  # one clear raw argmax
    return lg


def _histories(V, lg):
    """(name, history, pos, last_n): the window ends at pos; entries behind pos must not be read."""
    rng = np.random.default_rng(V + 1)
    pos_id, zero_id, neg_id, ninf_id = (int(np.flatnonzero(c)[3]) for c in ((lg > 0) & (lg < 9), lg == 0, (lg < 0) & np.isfinite(lg),
                                                                              np.isneginf(lg)))
    out = []
    h = rng.integers(0, V, 40)
    h[10] = neg_id
    out.append(("window of one position", h, 10, 1))
    out.append(("one token 1500 times", np.full(1500, pos_id), 1499, 0))
    h = rng.integers(0, V, 3000)
    h[::7] = zero_id
    h[5::11] = -1
    h[3::13] = V + 7
    h[1::17] = ninf_id
    out.append(("3000 entries, foreign ids", h, 2999, 0))
    out.append(("3000 entries, window 1100", h, 2999, 1100))
    h = np.array([pos_id] * 10 + [zero_id] * 20 + [ninf_id] * 3 + [neg_id] * 5)
    out.append(("last_n cuts a run", h, len(h) - 1, 15))
    out.append(("stale entries behind pos", np.concatenate([h, np.full(50, pos_id)]), len(h) - 1, 0))
    if V == 501:
        out.append(("every id in the window", np.concatenate([rng.permutation(V), rng.integers(0, V, 700)]), V + 699, 0))
    return out


@pytest.mark.parametrize("V", [501, 32000, 128256])
def test_operator_is_the_twin_bit_for_bit(gpu, V):
    lg = _raw_logits(V)
    ws = ops.logit_process_workspace(V, gpu)
    assert ws.numel() == V and ws.dtype == torch.int32
    am = int(np.argmax(lg))
    for name, hist, pos, last_n in _histories(V, lg):
        in_win = [int(t) for t in R.window(hist, pos, last_n) if 0 <= t < V and t != am]
        bias = {am: -INF, in_win[0]: 1.75, (am + 1) % V: -0.5}  # bans the raw argmax; raises a penalised token
        hist_d = torch.from_numpy(np.ascontiguousarray(hist, np.int32)).to(gpu)
        ids_d = torch.tensor(list(bias), dtype=torch.int32, device=gpu)
        val_d = torch.tensor(list(bias.values()), dtype=torch.float32, device=gpu)
        for pen, with_bias in ((dict(PEN, last_n=last_n), True), (dict(repetition=1.0, presence=0.0, frequency=0.7, last_n=last_n), False),
                               (dict(repetition=0.8, presence=0.0, frequency=0.0, last_n=last_n), True),
                               (dict(repetition=1.0, presence=0.0, frequency=0.0, last_n=last_n), True)):
            want = R.process(lg, hist, pos, bias=bias if with_bias else None, **pen)
            assert not np.isnan(want).any()
            outs = []
            for rep in range(2):  # the second call: a fresh copy of the logits, the table the first call left
                lg_d = torch.from_numpy(lg).to(gpu)
                p = torch.tensor([pos], dtype=torch.int32, device=gpu) if rep else pos  # both forms of the position
                ops.logit_process(lg_d, hist_d, p, pen, ids_d if with_bias else None, val_d if with_bias else None, ws)
                torch.cuda.synchronize()
                outs.append(lg_d.cpu().numpy())
                assert int(ws.abs().max().item()) == 0, (V, name, pen, "workspace not re-armed")
            bad = np.flatnonzero(outs[0].view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (V, name, pen, bad[:5], outs[0][bad[:5]], want[bad[:5]], lg[bad[:5]])
            assert outs[1].tobytes() == outs[0].tobytes(), (V, name, pen)
            if with_bias:
                assert outs[0][am] == -INF
    # off: nothing launched, the logits keep their bits
    lg_d = torch.from_numpy(lg).to(gpu)
    ops.logit_process(lg_d, hist_d, 3, None, None, None, None)
    torch.cuda.synchronize()
    assert lg_d.cpu().numpy().tobytes() == lg.tobytes()


# ---- model helpers --------------------------------------------------------------------------------------------------
def _golden_model(name, flags=0):
    from kuiperllama_amd.model import KuiperModel
    spec, img, toks, _ = load_golden(name)
    return KuiperModel.from_host_image(img, spec, flags=flags), spec, img, toks


def _synth_model(spec, gpu, seed=1234, max_seq_len=256, flags=0):
    from kuiperllama_amd.model import KuiperModel
    img_d = binfmt.synth_image(spec, seed=seed, device=gpu)
    torch.cuda.synchronize()
    return KuiperModel.from_device_image(img_d, spec, max_seq_len=max_seq_len, flags=flags)


def _fed(prompt, words):
    """token fed at every position 0 .. len(words)"""
    return [int(t) for t in prompt] + [int(w) for w in words[len(prompt) - 1:]]


def _exact_check(m, prompt, words, pen, bias, samp=None, exec="fused", first=0):
    """Processors off, predict() one position at a time over the fed tokens: the twin applied to each position's raw
    logits with the fed history decides the word - its first maximum, or with a sampler the checker's pick for
    Philox(seed, pos) on the processed logits.  Positions below `first` are taken from the cache as the run left it."""
    m.set_penalties()
    m.set_logit_bias(None)
    fed = _fed(prompt, words)
    for p in range(first, len(words)):
        is_prompt = p < len(prompt) - 1
        m.predict(fed[p], p, is_prompt=is_prompt, exec=exec)
        if is_prompt:
            assert words[p] == prompt[p + 1]
            continue
        proc = R.process(m.logits(), fed, p, bias=bias, **pen)
        if samp is None:
            assert words[p] == R.greedy(proc), (exec, p, words[p], R.greedy(proc))
        else:
            T, K, P, seed = samp
            assert S.Checker(proc).accepts(T, K, P, seed, [p], [words[p]]).all(), (exec, p, words[p])


def _two_bias_entries(m, prompt, steps):
    """-inf on the word an unprocessed greedy run repeats most, a positive value on its last word"""
    m.set_penalties()
    m.set_logit_bias(None)
    m.set_sampling()
    w, _ = m.generate(prompt, steps, exec="graph")
    tail = w[len(prompt) - 1:]
    top = max(set(tail), key=tail.count)
    other = next(t for t in reversed(tail + [(top + 1) % m.cfg.vocab_size]) if t != top)
    return {int(top): -INF, int(other): 1.0}


# ---- 2. every picked token ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hf_llama_half", "ref_llama_int8_untied", "flat-synth"])
def test_model_every_picked_token_is_checked(gpu, case):
    if case == "flat-synth":
        m, spec, prompt = _synth_model(FLAT_SPEC, gpu, seed=3, max_seq_len=128), FLAT_SPEC, [1, 263]
    else:
        m, spec, _, toks = _golden_model(case)
        prompt = [int(t) for t in toks[:3 if case == "hf_llama_half" else 2]]
    steps = min(64, spec.seq_len)
    bias = _two_bias_entries(m, prompt, steps)
    m.set_penalties(**PEN)
    m.set_logit_bias(bias)
    assert m.penalties == {"repetition": pytest.approx(1.3), "presence": 0.5, "frequency": pytest.approx(0.2), "last_n": 16}
    words, _ = m.generate(prompt, steps, exec="graph")
    assert len(words) == steps
    banned = next(t for t, b in bias.items() if b == -INF)
    assert banned not in words[len(prompt) - 1:]
    _exact_check(m, prompt, words, PEN, bias)
    # sampled picks on the processed logits, counter = position
    samp = (0.9, 40, 0.95, 0xC0FFEE)
    m.set_penalties(**PEN)
    m.set_logit_bias(bias)
    m.set_sampling(*samp)
    sw, _ = m.generate(prompt, steps, exec="graph")
    assert banned not in sw[len(prompt) - 1:]
    _exact_check(m, prompt, sw, PEN, bias, samp=samp)
    m.close()


# ---- 3. effect, whatever the model ----------------------------------------------------------------------------------
def test_effect_without_knowing_the_model(gpu):
    m = _synth_model(FLAT_SPEC, gpu, seed=3, max_seq_len=128)
    prompt, steps = [1, 263, 7], 64
    n0 = len(prompt) - 1  # words[n0:] are sampled
    for samp in (None, (1.0, 0, 1.0, 5)):
        m.set_sampling(*samp) if samp else m.set_sampling()
        m.set_logit_bias(None)
        m.set_penalties(presence=1e6, last_n=0)
        w, _ = m.generate(prompt, steps, exec="graph")
        fed = _fed(prompt, w)
        for p in range(n0, steps):
            assert w[p] not in fed[:p + 1], (samp, p, w[p])
        m.set_penalties(presence=1e6, last_n=4)
        w, _ = m.generate(prompt, steps, exec="graph")
        fed = _fed(prompt, w)
        for p in range(n0, steps):
            assert w[p] not in fed[max(0, p - 3):p + 1], (samp, p, w[p])
        m.set_penalties()
        free, _ = m.generate(prompt, steps, exec="graph")
        ban = free[n0]
        m.set_logit_bias({ban: -INF})
        w, _ = m.generate(prompt, steps, exec="graph")
        assert ban not in w[n0:] and w[:n0] == prompt[1:]
        m.set_logit_bias({ban: -INF, 1999: 1e6})
        w, _ = m.generate(prompt, steps, exec="graph")
        assert w[n0:] == [1999] * (steps - n0)
    # what needs the model's vocabulary to be refused
    V = m.cfg.vocab_size
    with pytest.raises(_ffi.KhError) as ei:
        m.set_logit_bias({V: 1.0})
    assert ei.value.code == _ffi.KH_ERR_RANGE
    with pytest.raises(_ffi.KhError) as ei:
        m.set_logit_bias({t: -INF for t in range(V)})
    assert ei.value.code == -1
    m.set_logit_bias({t: -INF for t in range(V - 1)})  # one token left (a list that outgrows its buffer: new graphs)
    m.set_sampling()
    w, _ = m.generate(prompt, 12, exec="graph")
    assert w[n0:] == [V - 1] * (12 - n0)
    m.close()


# ---- 4. modes and entry points --------------------------------------------------------------------------------------
def test_modes_chunkings_and_entry_points_agree(gpu):
    m, spec, _, toks = _golden_model("hf_llama_half")
    prompt = [int(t) for t in toks[:3]]
    bias = _two_bias_entries(m, prompt, 64)
    for samp in (None, (1.0, 0, 0.9, 77)):
        def on():
            m.set_penalties(**PEN)
            m.set_logit_bias(bias)
            m.set_sampling(*samp) if samp else m.set_sampling()
        on()
        g, _ = m.generate(prompt, 64, exec="graph")
        f, _ = m.generate(prompt, 64, exec="fused")
        assert g == f
        short, _ = m.generate(prompt, 13, exec="graph")
        assert short == g[:13]
        absent = next(t for t in range(spec.vocab_size) if t not in g)
        u, _ = m.generate(prompt, 64, exec="graph", stop=[absent])
        assert u == g
        loop, fed = [], list(prompt)
        for p in range(64):
            is_prompt = p < len(prompt) - 1
            nxt = m.predict(fed[p], p, is_prompt=is_prompt, exec="fused")
            loop.append(prompt[p + 1] if is_prompt else nxt)
            if p + 1 >= len(fed):
                fed.append(loop[-1])
        assert loop == g
        # unfused: the reference's launch sequence with kh_logit_process_f32 ahead of the argmax / the draw
        un, _ = m.generate(prompt, 40, exec="unfused")
        _exact_check(m, prompt, un, PEN, bias, samp=samp, exec="unfused")
        on()
        fed = _fed(prompt, un)
        for p in range(len(prompt) - 1, 40):  # ... and predict, unfused, draws the same
            assert m.predict(fed[p], p, exec="unfused") == un[p]
    m.close()


# ---- 5. prompt paths ------------------------------------------------------------------------------------------------
def test_prompt_prefill_paths(gpu):
    from kuiperllama_amd.model import KuiperModel
    spec = PREFILL_SPEC
    img_d = binfmt.synth_image(spec, seed=21, device=gpu)
    torch.cuda.synchronize()
    rng = np.random.default_rng(8)
    prompt = [int(t) for t in rng.choice(spec.vocab_size, 20, replace=False)]
    pen = dict(repetition=1.0, presence=1e6, frequency=0.0, last_n=0)
    m = KuiperModel.from_device_image(img_d, spec, max_seq_len=128, flags=_ffi.KH_FLAG_PREFILL_EXACT)
    m.set_penalties(**pen)
    words, _ = m.generate(prompt, 68, exec="graph")
    assert m.first_sample()["prefill_mode"] == "gemv"
    assert m.first_sample()["top1_id"] == words[len(prompt) - 1]
    _exact_check(m, prompt, words, pen, None)
    m.close()
    m = KuiperModel.from_device_image(img_d, spec, max_seq_len=128)
    m.set_penalties(**pen)
    words, _ = m.generate(prompt, 48, exec="graph")
    fs = m.first_sample()
    assert fs["prefill_mode"] == "gemm" and words[:len(prompt) - 1] == prompt[1:]
    assert fs["top1_id"] == words[len(prompt) - 1]
    fed = _fed(prompt, words)
    for p in range(len(prompt) - 1, 48):
        assert words[p] not in fed[:p + 1], (p, words[p])
    # the public prefill entry points keep the record too: prefill, then predict the rest
    m.prefill_gemm(prompt[:-1], 0)
    nxt = m.predict(prompt[-1], len(prompt) - 1)
    assert nxt not in prompt and nxt == words[len(prompt) - 1]
    m.close()


# ---- 6. a window deeper than the workgroup --------------------------------------------------------------------------
def test_window_deeper_than_the_workgroup(gpu):
    spec = binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 2048, True, binfmt.FAMILY_LLAMA, False, 64,
                            binfmt.ROPE_HALF, 500000.0, 1e-5, "deep-synth")
    m = _synth_model(spec, gpu, seed=3, max_seq_len=2048)
    prompt, steps = [1, 263], 1100
    pen = dict(repetition=1.0, presence=0.0, frequency=0.3, last_n=0)
    m.set_penalties(**pen)
    words, _ = m.generate(prompt, steps, exec="graph")
    assert len(words) == steps
    assert max(np.bincount(words)) > 1  # counts above one enter the frequency term
    _exact_check(m, prompt, words, pen, None, first=1030)
    m.close()


# ---- 7. off is untouched --------------------------------------------------------------------------------------------
def test_off_is_untouched(gpu):
    m, spec, img, toks = _golden_model("hf_llama_half")
    prompt = [int(t) for t in toks[:2]]
    lpt = m.cfg.launches_per_token
    assert lpt == 5 * spec.n_layers + 2
    from kuiperllama_amd.model import KuiperModel
    fresh = KuiperModel.from_host_image(img, spec)
    want, _ = fresh.generate(prompt, 32, exec="graph")
    want_logits = fresh.logits()
    fresh.set_sampling(0.7, 0, 0.9, 11)
    want_sampled, _ = fresh.generate(prompt, 32, exec="graph")
    fresh.close()
    screens = bool(m.cls_screen_info()["on"])
    m.set_penalties(**PEN)
    m.set_logit_bias({int(want[-1]): -INF})
    steps0 = m.cls_screen_info()["steps"]
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        changed, _ = m.generate(prompt, 32, exec="graph")
        log_on = _ffi.launch_log()
        assert "k_sample_proc" in log_on and not any(k.startswith(("k_sample_screen", "k_cls_screen")) for k in log_on)
        assert changed != want and m.cls_screen_info()["steps"] == steps0  # no screened step while processors are on
        counts = m.profile_step(1, 2)
        assert sum(v["launches_per_step"] for v in counts.values()) == lpt
        assert m.cfg.launches_per_token == lpt
        m.set_penalties()
        m.set_logit_bias(None)
        assert m.penalties == {"repetition": 1.0, "presence": 0.0, "frequency": 0.0, "last_n": 0}
        _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
        for ex in ("graph", "fused"):
            assert m.generate(prompt, 32, exec=ex)[0] == want, ex
        assert m.logits().tobytes() == want_logits.tobytes()
        log_off = _ffi.launch_log()
        assert "k_sample_proc" not in log_off
        if screens:
            assert any(k.startswith("k_sample_screen") for k in log_off) and any(k.startswith("k_cls_screen") for k in log_off)
            assert m.cls_screen_info()["steps"] > steps0
        m.set_penalties(1.0, 0.0, 0.0, 64)  # all neutral whatever the window: still off
        m.set_sampling(0.7, 0, 0.9, 11)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        assert m.generate(prompt, 32, exec="graph")[0] == want_sampled
        log_s = _ffi.launch_log()
        assert "k_sample_topp" in log_s and "k_sample_proc" not in log_s
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


# ---- 8. demo CLI ----------------------------------------------------------------------------------------------------
def test_demo_cli_flags(gpu, tmp_path):
    spec, img, toks, _ = load_golden("hf_llama_half")
    path = tmp_path / "m.bin"
    img.tofile(path)
    prompt = [int(t) for t in toks[:3]]
    from kuiperllama_amd.model import KuiperModel
    m = KuiperModel.from_host_image(img, spec)
    free, _ = m.generate(prompt, 40, exec="graph")
    ban = int(free[-1])
    up = next((int(t) for t in free[len(prompt) - 1:] if t != ban), (ban + 1) % spec.vocab_size)  # distinct ids
    m.set_penalties(1.3, 0.5, 0.2, 16)
    m.set_logit_bias({ban: -INF, up: 0.75})
    want, _ = m.generate(prompt, 40, exec="graph")
    m.close()
    assert want != free
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--steps", "40", "--prompt", ",".join(map(str, prompt)), "--repeat-penalty", "1.3", "--presence-penalty",
            "0.5", "--frequency-penalty", "0.2", "--repeat-last-n", "16", "--logit-bias", f"{ban}=-inf",
            "--logit-bias", f"{up}=0.75"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [int(t) for t in r.stdout.strip().splitlines()[1].split()] == want
    bad = subprocess.run(args + ["--repeat-penalty", "0"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
