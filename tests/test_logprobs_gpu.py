"""Per-token log-probabilities on the GPU (csrc/kh_logprobs.h): the operator against the fp64 twin
tests/logprobs_ref.py, and the model paths (graph, fused, unfused; generate, generate_until, predict; both prefills):
no token changes, and every record is the twin of the logits the pick was made from.

Tolerance of every float (logprobs_ref.tol): 2^-24 (ceil(V / 1024) + 16) + 2^-23 (|lse| + |lp|).  The kernel sums exp
in fp32 as the bound assumes, with shorter chains: thread t of 1024 owns float4 t, t + 1024, ... and keeps one partial
per component, so a partial is a chain of at most ceil(V / 4096) adds (+ 1 for an element of the tail that is no whole
float4; a row that is not 16-byte aligned - odd V, rows > 0 - falls back to one partial per thread over elements t,
t + 1024, ...: at most ceil(V / 1024) adds); two adds join the four partials, six shuffle levels the wave and four the
sixteen waves.  That is at most ceil(V / 1024) + 13 roundings of relative size 2^-24 on the way to Z; expf and its
argument l - m take the rest of the first term, and log Z carries that relative error as an absolute one.  The second term covers the
roundings of logf, m + log Z and l - lse.  Ids are compared exactly: ordering fp32 values involves no arithmetic."""
import numpy as np
import pytest
import torch

import logit_proc_ref as R
import logprobs_ref as L
from conftest import load_golden
from kuiperllama_amd import _ffi, binfmt, ops

pytestmark = pytest.mark.gpu

INF = float("inf")
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)
SAMP = (0.8, 50, 0.95, 0xC0FFEE)
FLAT_SPEC = binfmt.ModelSpec(256, 512, 2, 4, 2, 2048, 128, True, binfmt.FAMILY_LLAMA, False, 64,
                             binfmt.ROPE_HALF, 500000.0, 1e-5, "flat-synth")
PREFILL_SPEC = binfmt.ModelSpec(512, 1408, 2, 8, 2, 4096, 160, True, binfmt.FAMILY_LLAMA, False, 64,
                                binfmt.ROPE_HALF, 500000.0, 1e-5, "prefill-synth")
STEPS = 27  # three 8-step graph chunks and a remainder


# ---- 1. operator ----------------------------------------------------------------------------------------------------
def _rows(V):
    """[5, V]: normal(0, 2) with one eighth exact zeros, one eighth -inf, one clear maximum and equal values across
    the cuts at 5 and 20; all equal; one finite logit among -inf; mean +40 sigma 8; mean -60."""
    rng = np.random.default_rng(V)
    lg = rng.normal(0.0, 2.0, V).astype(np.float32)
    kind = rng.integers(0, 8, V)
    lg[kind == 0] = 0.0
    lg[kind == 1] = -INF
    lg[int(rng.integers(0, V))] = 9.5
    o = L.order(lg)
    lg[o[3:7]] = lg[o[3]]      # ranks 3 .. 6 equal: the cut at 5 falls among them
    lg[o[17:24]] = lg[o[17]]   # ranks 17 .. 23 equal: the cut at 20
    rows = np.empty((5, V), np.float32)
    rows[0] = lg
    rows[1] = 1.25
    rows[2] = -INF
    rows[2, (2 * V) // 3] = -3.0
    rows[3] = rng.normal(40.0, 8.0, V).astype(np.float32)
    rows[3, kind == 1] = -INF
    rows[3, kind == 0] = 40.0
    rows[4] = rng.normal(-60.0, 2.0, V).astype(np.float32)
    rows[4, kind == 2] = -INF
    return rows


_TWIN = {}


def _twin(V):
    """the rows and their fp64 records at the widest list, computed once"""
    if V not in _TWIN:
        rows = _rows(V)
        _TWIN[V] = (rows, [L.logprobs(r, 20) for r in rows])
    return _TWIN[V]


def _check_floats(got, want, V, lse, what, is_lse=False):
    """-> largest err / tol (an lse has no |lp| term); -inf must be -inf, nothing may be NaN"""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    assert not np.isnan(got).any(), what
    ninf = np.isneginf(want)
    assert (np.isneginf(got) == ninf).all(), what
    worst = 0.0
    for g, w in zip(got[~ninf], want[~ninf]):
        t = L.tol(V, lse, 0.0 if is_lse else w)
        worst = max(worst, abs(g - w) / t)
        assert abs(g - w) <= t, (what, g, w, abs(g - w) / t)
    return worst


@pytest.mark.parametrize("V", [501, 32000, 128256])
def test_operator_against_the_fp64_twin(gpu, V):
    rows, twin = _twin(V)
    rng = np.random.default_rng(V + 1)
    # per row: the maximum, any token, the only finite one, a -inf one (exactly -inf), a finite one
    ids = np.array([int(np.argmax(rows[0])), int(rng.integers(0, V)), (2 * V) // 3,
                    int(np.flatnonzero(np.isneginf(rows[3]))[2]), int(np.flatnonzero(np.isfinite(rows[4]))[5])], np.int32)
    lg_d = torch.from_numpy(rows).to(gpu)
    worst = 0.0
    for bad_row, bad_id in ((None, 0), (1, V), (4, -1)):
        use = ids.copy()
        if bad_row is not None:
            use[bad_row] = bad_id
        ids_d = torch.from_numpy(use).to(gpu)
        for N in (0, 1, 5, 20):
            out = ops.logprobs(lg_d, ids_d, N)
            torch.cuda.synchronize()
            lse, lp = out["lse"].cpu().numpy(), out["logprob"].cpu().numpy()
            tid, tlp = out["top_ids"].cpu().numpy(), out["top_logprobs"].cpu().numpy()
            assert tid.shape == tlp.shape == (5, N)
            for r in range(5):
                w_lse, w_lp, w_ids, w_tlp = twin[r]
                what = (V, N, r, bad_row)
                worst = max(worst, _check_floats(lse[r], w_lse, V, w_lse, what, is_lse=True))
                if r == bad_row:
                    assert np.isnan(lp[r]), what
                else:
                    worst = max(worst, _check_floats(lp[r], w_lp[use[r]], V, w_lse, what))
                assert list(tid[r]) == list(w_ids[:N]), (what, tid[r], w_ids[:N])
                worst = max(worst, _check_floats(tlp[r], w_tlp[:N], V, w_lse, what))
    print(f"V={V}: largest err / tol = {worst:.3f}")
    # every output is optional, a single vector is one row
    one = ops.logprobs(lg_d[0], torch.from_numpy(ids[:1]).to(gpu), 5)
    torch.cuda.synchronize()
    assert list(one["top_ids"].cpu().numpy()[0]) == list(twin[0][2][:5])
    rc = _ffi.lib().kh_logprobs_f32(lg_d.data_ptr(), V, 5, None, 5, None, None, None, None,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0


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


def _models(gpu, case):
    if case == "flat-synth":
        return _synth_model(FLAT_SPEC, gpu, seed=3, max_seq_len=128), [1, 263, 7]
    m, _, _, toks = _golden_model(case)
    return m, [int(t) for t in toks[:3]]


BIAS = {5: -INF, 11: 1.0}
CONFIGS = {"greedy": (None, None, None), "sampled": (None, None, SAMP), "penalties+bias": (PEN, BIAS, None),
           "penalties+sampled": (PEN, BIAS, SAMP)}


def _configure(m, pen, bias, samp):
    m.set_penalties(**pen) if pen else m.set_penalties()
    m.set_logit_bias(bias)
    m.set_sampling(*samp) if samp else m.set_sampling()


def _fed(prompt, words):
    """token fed at every position 0 .. len(words)"""
    return [int(t) for t in prompt] + [int(w) for w in words[len(prompt) - 1:]]


def _is_none(rec, p):
    return (rec["token"][p] == -1 and np.isnan(rec["logprob"][p]) and (rec["top_ids"][p] == -1).all() and
            np.isnan(rec["top_logprobs"][p]).all())


def _check_record(rec, p, token, logits, V, top_n):
    """record p against the twin of the fp32 logits the pick was made from"""
    lse, lp, ids, tlp = L.logprobs(logits, top_n)
    what = (p, token)
    assert rec["token"][p] == token, what
    assert list(rec["top_ids"][p]) == list(ids), (what, rec["top_ids"][p], ids)
    _check_floats(rec["logprob"][p], lp[token], V, lse, what)
    _check_floats(rec["top_logprobs"][p], tlp, V, lse, what)


def _records_check(m, prompt, words, rec, pen, bias, exec, top_n):
    """Log-probs and processors off, predict() one position at a time over the fed tokens in the same exec family
    (graph and fused share their kernels): the twin of each position's logits - processed by the processors' own twin
    where they were on - is the record."""
    m.set_logprobs(None)
    m.set_penalties()
    m.set_logit_bias(None)
    m.set_sampling()
    fed, V = _fed(prompt, words), m.cfg.vocab_size
    for p in range(len(words)):
        is_prompt = p < len(prompt) - 1
        m.predict(fed[p], p, is_prompt=is_prompt, exec="unfused" if exec == "unfused" else "fused")
        if is_prompt:
            assert _is_none(rec, p), p
            continue
        lg = m.logits()
        if pen or bias:
            lg = R.process(lg, fed, p, bias=bias, **(pen or {}))
        _check_record(rec, p, words[p], lg, V, top_n)


# ---- 2. no token changes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["flat-synth", "hf_llama_half"])
def test_model_tokens_are_unchanged(gpu, case):
    m, prompt = _models(gpu, case)
    for ex in ("graph", "fused", "unfused"):
        for name, cfg in CONFIGS.items():
            _configure(m, *cfg)
            m.set_logprobs(None)
            want, _ = m.generate(prompt, STEPS, exec=ex)
            m.set_logprobs(5)
            assert m.logprobs_setting == 5
            got, _ = m.generate(prompt, STEPS, exec=ex)
            assert got == want, (case, ex, name)
            assert len(got) == STEPS
    m.close()


# ---- 3. every record ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,execs", [("flat-synth", ("graph", "fused", "unfused")), ("hf_llama_half", ("graph",))])
def test_model_records_are_the_twin_of_the_logits(gpu, case, execs):
    m, prompt = _models(gpu, case)
    for ex in execs:
        for name, (pen, bias, samp) in CONFIGS.items():
            _configure(m, pen, bias, samp)
            m.set_logprobs(5)
            words, _ = m.generate(prompt, STEPS, exec=ex)
            rec = m.logprobs(0, STEPS)
            assert rec["top_ids"].shape == rec["top_logprobs"].shape == (STEPS, 5)
            if bias:
                assert not np.isin(5, rec["top_ids"][len(prompt) - 1:])  # a banned token is no alternative
            _records_check(m, prompt, words, rec, pen, bias, ex, 5)
    m.close()


def test_gemm_prefill_prompt(gpu):
    m = _synth_model(PREFILL_SPEC, gpu, seed=21, max_seq_len=128)
    rng = np.random.default_rng(8)
    prompt = [int(t) for t in rng.choice(PREFILL_SPEC.vocab_size, 20, replace=False)]
    m.set_logprobs(20)
    m.generate([1, 2], 16, exec="graph")  # records of sampled steps at the later prompt positions
    assert not _is_none(m.logprobs(0, 16), 9)
    words, _ = m.generate(prompt, len(prompt), exec="graph")  # the last step is the first sampled one
    assert m.first_sample()["prefill_mode"] == "gemm"
    rec = m.logprobs(0, len(prompt))
    for p in range(len(prompt) - 1):
        assert _is_none(rec, p), p
    _check_record(rec, len(prompt) - 1, words[-1], m.logits(), PREFILL_SPEC.vocab_size, 20)
    # the public prefill entry points leave "none" records too
    m.generate([1, 2], 16, exec="graph")
    m.prefill_gemm(prompt[:-1], 0)
    nxt = m.predict(prompt[-1], len(prompt) - 1)
    rec = m.logprobs(0, len(prompt))
    assert all(_is_none(rec, p) for p in range(len(prompt) - 1)) and nxt == words[-1]
    _check_record(rec, len(prompt) - 1, nxt, m.logits(), PREFILL_SPEC.vocab_size, 20)
    m.close()


def test_stop_token_and_predict_loop(gpu):
    m, prompt = _models(gpu, "hf_llama_half")
    n0 = len(prompt) - 1
    stopped = 0
    for name in ("greedy", "penalties+sampled"):
        def on():
            _configure(m, *CONFIGS[name])
            m.set_logprobs(5)
        on()
        words, _ = m.generate(prompt, STEPS, exec="graph")
        rec = m.logprobs(0, STEPS)
        # a stop token in the middle of the run: the records of the returned words are theirs
        firsts = [j for j in range(n0 + 1, STEPS) if words[j] not in words[n0:j]]  # (a greedy run may just repeat)
        if firsts:
            j = firsts[len(firsts) // 2]
            cut, _ = m.generate(prompt, STEPS, exec="graph", stop=[words[j]])
            assert cut == words[:j]
            part = m.logprobs(n0, len(cut) - n0)
            assert list(part["token"]) == cut[n0:]
            for k in ("logprob", "top_ids", "top_logprobs"):
                assert part[k].tobytes() == rec[k][n0:j].tobytes(), (name, k)
            stopped += 1
        # a loop of predict calls writes the records generate writes (graph and fused share their kernels)
        for ex in ("fused", "unfused"):
            if ex == "unfused":
                words, _ = m.generate(prompt, STEPS, exec="unfused")
                rec = m.logprobs(0, STEPS)
            m.generate([prompt[0], prompt[0]], STEPS, exec="graph")  # other records everywhere
            fed = list(prompt)
            for p in range(STEPS):
                nxt = m.predict(fed[p], p, is_prompt=p < n0, exec=ex)
                if p + 1 >= len(fed):
                    fed.append(nxt)
            assert fed[1:] == words, (name, ex)
            loop = m.logprobs(0, STEPS)
            assert all(_is_none(loop, p) for p in range(n0))
            for k in rec:
                assert loop[k].tobytes() == rec[k].tobytes(), (name, ex, k)
    assert stopped >= 1
    m.close()


# ---- 4. launches ----------------------------------------------------------------------------------------------------
def test_launches(gpu):
    from kuiperllama_amd.model import KuiperModel
    m, spec, img, toks = _golden_model("hf_llama_half")
    prompt = [int(t) for t in toks[:2]]
    lpt = m.cfg.launches_per_token
    assert lpt == 5 * spec.n_layers + 2

    def run(model):
        _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
        out = [model.generate(prompt, 32, exec=ex)[0] for ex in ("graph", "fused")]
        assert out[0] == out[1]
        return out[0], _ffi.launch_log()
    try:
        fresh = KuiperModel.from_host_image(img, spec)
        want, log_fresh = run(fresh)
        fresh.close()
        screens = bool(m.cls_screen_info()["on"])
        assert "k_sample_lp" not in log_fresh
        m.set_logprobs(5)
        steps0 = m.cls_screen_info()["steps"]
        got, log_on = run(m)
        assert got == want
        assert "k_sample_lp" in log_on and not any(k.startswith(("k_sample_screen", "k_cls_screen")) for k in log_on)
        assert m.cls_screen_info()["steps"] == steps0  # no screened step while log-probs are on
        five = m.logprobs(0, 32)
        counts = m.profile_step(1, 2)
        assert sum(v["launches_per_step"] for v in counts.values()) == lpt
        assert m.cfg.launches_per_token == lpt
        # a wider list between two generates: no recapture, records of the new width
        m.set_logprobs(20)
        assert m.generate(prompt, 32, exec="graph")[0] == want
        wide = m.logprobs(0, 32)
        assert wide["top_ids"].shape == wide["top_logprobs"].shape == (32, 20)
        assert (wide["top_ids"][:, :5] == five["top_ids"]).all() and (wide["top_ids"][1:] >= 0).all()
        assert wide["logprob"].tobytes() == five["logprob"].tobytes()
        m.set_logprobs(0)
        assert m.generate(prompt, 32, exec="graph")[0] == want
        zero = m.logprobs(0, 32)
        assert zero["top_ids"].shape == (32, 0) and zero["logprob"].tobytes() == five["logprob"].tobytes()
        # off again: the launches of a fresh model
        m.set_logprobs(None)
        assert m.logprobs_setting is None
        got, log_off = run(m)
        assert got == want and log_off == log_fresh
        if screens:
            assert any(k.startswith("k_sample_screen") for k in log_off) and m.cls_screen_info()["steps"] > steps0
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    m.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    m = _synth_model(FLAT_SPEC, gpu, seed=3, max_seq_len=128)

    def code(f, *a):
        with pytest.raises(_ffi.KhError) as ei:
            f(*a)
        return ei.value.code
    assert code(m.logprobs, 0, 1) == _ffi.KH_ERR_UNSUPPORTED  # never turned on
    assert code(m.set_logprobs, 21) == _ffi.KH_ERR_INVALID_ARG
    assert code(m.set_logprobs, -2) == _ffi.KH_ERR_INVALID_ARG
    assert code(m.logprobs, 0, 1) == _ffi.KH_ERR_UNSUPPORTED and m.logprobs_setting is None
    m.set_logprobs(3)
    cap = m.cfg.cache_len
    assert code(m.logprobs, cap, 1) == _ffi.KH_ERR_RANGE
    assert code(m.logprobs, cap - 1, 2) == _ffi.KH_ERR_RANGE
    assert code(m.logprobs, -1, 1) == _ffi.KH_ERR_RANGE
    rec = m.logprobs(0, cap)  # nothing sampled yet: every record is "none"
    assert all(_is_none(rec, p) for p in range(cap)) and rec["top_ids"].shape == (cap, 3)
    m.set_logprobs(None)
    assert m.logprobs(cap - 1, 1)["top_ids"].shape == (1, 0)  # off, but the records stay readable
    m.close()


# ---- 6. demo CLI ----------------------------------------------------------------------------------------------------
def test_demo_cli_prints_the_records(gpu, tmp_path):
    import subprocess
    from kuiperllama_amd import build
    from kuiperllama_amd.model import KuiperModel
    spec, img, toks, _ = load_golden("hf_llama_half")
    path = tmp_path / "m.bin"
    img.tofile(path)
    prompt = [int(t) for t in toks[:3]]
    m = KuiperModel.from_host_image(img, spec)
    m.set_logprobs(3)
    want, _ = m.generate(prompt, 20, exec="graph")
    rec = m.logprobs(0, 20)
    m.close()
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--steps", "20", "--prompt", ",".join(map(str, prompt)), "--logprobs", "3"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.strip().splitlines()
    assert [int(t) for t in out[1].split()] == want
    lines = [ln for ln in out[2:] if "|" in ln]
    assert len(lines) == 20 - (len(prompt) - 1)
    for ln, p in zip(lines, range(len(prompt) - 1, 20)):
        head, tops = ln.split("|")
        pos, tok, lp = head.split()
        assert (int(pos), int(tok)) == (p, want[p]) and float(lp) == pytest.approx(float(rec["logprob"][p]), abs=2e-6)
        pairs = [t.split(":") for t in tops.split()]
        assert [int(i) for i, _ in pairs] == list(rec["top_ids"][p])
        assert [float(v) for _, v in pairs] == pytest.approx([float(v) for v in rec["top_logprobs"][p]], abs=2e-6)
    bad = subprocess.run(args[:-1] + ["21"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
