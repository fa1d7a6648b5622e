"""Speculative greedy decode on the GPU: the row argmax (kh_argmax_rows_f32, csrc/kh_spec.h::k_spec_pick), the verify
pass (kh_model_verify: a full-depth B-token pass, k_pf_cls, k_spec_pick, k_spec_accept) and the prompt-lookup loop
(kh_model_generate_lookup).

Every comparison is EXACT: token ids, counts, and K/V rows as raw bits.  The reference of a verify pass is a loop of
fused predict calls on a twin model, R[p + 1] = predict(R[p], p); the reference of the lookup loop is the twin's own
generate().  The feature states no tolerance and neither does this file.

The models are the four of tests/score_cases.py - the smallest shapes that reach every instantiation of the pass:
(a) fp32, 8 tokens per pass, a cache of 320 rows; (b) int8, 4 per pass; (c) Qwen2 with bias; (d) wide fp32, 4 per
pass, an odd vocabulary of 2051 (clamped last pair, padded row stride of the logits scratch)."""
import numpy as np
import pytest
import torch

import score_cases as S
from conftest import load_golden
from kuiperllama_amd import _ffi, binfmt, ops
from kuiperllama_amd.model import KuiperModel, lookup_draft

pytestmark = pytest.mark.gpu

NAMES = ["a", "b", "c", "d"]
INF = float("inf")
CROSS = 252  # model (a): a pass of 8 from here covers positions 252 .. 259, across 256 where the time splits start


# ---- the token-by-token reference, once per model ---------------------------------------------------------------------
_REF = {}


def _model(gpu, name, **kw):  # (after _ref(gpu, name))
    return KuiperModel.from_device_image(_REF[name]["img"], S.SPECS[name], max_seq_len=S.SPECS[name].seq_len, **kw)


def _ref(gpu, name):
    """R: the greedy sequence of a loop of fused predict calls; kv[layer] = the (K, V) rows that loop left; one logits
    vector of it"""
    if name not in _REF:
        spec, width = S.SPECS[name], S.BATCH[name]
        T = CROSS + width + 2 if name == "a" else 5 + width + 2
        img = binfmt.synth_image(spec, seed=S.SEEDS[name], device=gpu)
        torch.cuda.synchronize()
        _REF[name] = r = {"img": img}
        twin = _model(gpu, name)
        R = [S.tokens(name, 1)[0]]
        for p in range(T):
            R.append(twin.predict(R[p], p, exec="fused"))
        r["R"] = R  # T + 1 tokens: positions 0 .. T - 1 were fed
        r["logits"] = twin.logits()
        r["kv"] = [twin.read_kv(layer, 0, T) for layer in range(spec.n_layers)]
        twin.close()
    return _REF[name]


def _same_rows(m, name, row0, nrows):
    for layer, (k, v) in enumerate(_REF[name]["kv"]):
        gk, gv = m.read_kv(layer, row0, nrows)
        assert gk.tobytes() == k[row0:row0 + nrows].tobytes(), (name, layer, row0, nrows, "K")
        assert gv.tobytes() == v[row0:row0 + nrows].tobytes(), (name, layer, row0, nrows, "V")


# ---- 1. the operator: first maximum of every row ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [2051, 2048])
def test_argmax_rows_on_crafted_rows(gpu, n):
    real = _ref(gpu, "d" if n == 2051 else "a")["logits"]
    assert real.shape == (n,)
    rng = np.random.default_rng(n)

    def crafted(rows):
        x = rng.standard_normal((rows, n)).astype(np.float32)
        for r in range(rows):
            kind = r % 8
            if kind == 0:
                x[r, 0] = 9.0                      # maximum at index 0
            elif kind == 1:
                x[r, n - 1] = 9.0                  # at n - 1
            elif kind == 2:
                x[r, [n - 1, 1037, 17]] = 9.0      # duplicated: ties -> lowest index
            elif kind == 3:
                x[r, :] = -1.25                    # all equal
            elif kind == 4:
                x[r, rng.random(n) < 0.5] = -INF   # -inf entries
            elif kind == 5:
                x[r, :] = -INF                     # nothing but -inf: index 0
            elif kind == 6:
                x[r, :] = real                     # a real logits vector of kh_model_predict
            else:
                x[r, 16 * 64 + 3] = x[r, 16 * 64 + 4] = 9.0  # a tie inside one thread's run of 16
        return x
    for stride in ((n + 3) & ~3, ((n + 3) & ~3) + 8, 4096):
        for rows in (1, 4, 8, 11):  # 11: two grids
            for misaligned in (False, True):  # rows off the 16-byte boundary take the walker's scalar path
                x = crafted(rows)
                buf = torch.full((rows * stride + 4,), INF, dtype=torch.float32, device=gpu)  # padding would win if read
                t = buf[1:1 + rows * stride] if misaligned else buf[:rows * stride]
                t = t.view(rows, stride)
                t[:, :n] = torch.from_numpy(x).to(gpu)
                assert t.is_contiguous() and (t.data_ptr() % 16 != 0) == misaligned
                out = torch.full((rows,), -7, dtype=torch.int32, device=gpu)
                ops.argmax_rows(t, n, out)
                torch.cuda.synchronize()
                assert out.cpu().tolist() == [int(np.argmax(r)) for r in x], (n, stride, rows, misaligned)
    # the row form agrees with the single-row operator on the real vector
    one = torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.argmax(torch.from_numpy(real).to(gpu), one)
    torch.cuda.synchronize()
    assert int(one.item()) == int(np.argmax(real))


# ---- 2. the verify pass -----------------------------------------------------------------------------------------------
def _cases(width):
    for pos0 in (0, 5):
        for n in sorted({1, 2, width - 1, width}):
            for k in [None] + sorted({k for k in (1, n // 2, n - 1) if 1 <= k < n}):
                yield pos0, n, k


@pytest.mark.parametrize("name", NAMES)
def test_verify_accepts_exactly_the_right_drafts(gpu, name):
    r = _ref(gpu, name)
    R, V, width = r["R"], S.SPECS[name].vocab_size, S.BATCH[name]
    m = _model(gpu, name)
    assert m.verify_width() == width
    behind_checked = False
    for pos0, n, k in _cases(width):
        what = (name, pos0, n, k)
        if pos0:
            m.prefill(R[:pos0])
        fed = list(R[pos0:pos0 + n])
        if k is not None:
            fed[k] = (R[pos0 + k] + 1) % V
        nxt, a = m.verify(fed, pos0)
        assert nxt.shape == (n,)
        assert a == (n - 1 if k is None else k - 1), what
        assert list(nxt[:a + 1]) == R[pos0 + 1:pos0 + a + 2], what
        _same_rows(m, name, pos0, a + 1)  # the accepted rows, bit for bit
        if k is not None and n == width and k == n // 2 and pos0 == 5:
            # the picks BEHIND the rejection: what a predict loop says when fed the same wrong tokens
            twin = _model(gpu, name)
            twin.prefill(R[:pos0])
            assert list(nxt) == [twin.predict(t, pos0 + i, exec="fused") for i, t in enumerate(fed)], what
            twin.close()
            behind_checked = True
        # accepted rows are right, stale rows are harmless: the next step continues the sequence
        assert m.predict(int(nxt[a]), pos0 + a + 1, exec="fused") == R[pos0 + a + 2], what
    assert behind_checked
    m.close()


def test_verify_across_the_time_split_threshold(gpu):
    r = _ref(gpu, "a")
    R = r["R"]
    m = _model(gpu, "a")
    m.prefill(R[:CROSS])
    nxt, a = m.verify(R[CROSS:CROSS + 8], CROSS)
    assert a == 7 and list(nxt) == R[CROSS + 1:CROSS + 9]
    _same_rows(m, "a", 0, CROSS + 8)
    assert m.predict(int(nxt[7]), CROSS + 8, exec="fused") == R[CROSS + 9]
    m.close()


def test_verify_ignores_the_settings(gpu):
    """sampler, processors and log-probs are neither consulted nor touched"""
    r = _ref(gpu, "a")
    R, V = r["R"], S.SPECS["a"].vocab_size
    m = _model(gpu, "a")
    fed = list(R[:8])
    fed[5] = (fed[5] + 1) % V
    plain = m.verify(fed, 0)
    m.set_sampling(0.8, 50, 0.95, 0xC0FFEE)
    m.set_penalties(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)
    m.set_logit_bias({int(R[3]): -INF, 11: 2.0})
    m.set_logprobs(3)
    before = (m.sampling, m.penalties, m.logprobs_setting)
    loaded = m.verify(fed, 0)
    assert list(loaded[0]) == list(plain[0]) and loaded[1] == plain[1] == 4
    assert (m.sampling, m.penalties, m.logprobs_setting) == before
    rec = m.logprobs(0, 8)
    assert (rec["token"] == -1).all()  # no record was written
    m.close()


def test_verify_errors(gpu):
    r = _ref(gpu, "a")
    R, V = r["R"], S.SPECS["a"].vocab_size
    m = _model(gpu, "a")
    cap = m.cfg.cache_len
    m.prefill(R[:4])
    sentinel = [m.read_kv(layer, 0, 12) for layer in range(S.SPECS["a"].n_layers)]

    def code(*a):
        with pytest.raises(_ffi.KhError) as ei:
            m.verify(*a)
        return ei.value.code
    assert code([], 0) == _ffi.KH_ERR_INVALID_ARG
    assert code(R[:4], -1) == _ffi.KH_ERR_INVALID_ARG
    assert code(R[:9], 0) == _ffi.KH_ERR_RANGE            # n > width
    assert code(R[:4], cap - 3) == _ffi.KH_ERR_RANGE       # pos0 + n > cache_len
    assert code(R[:4], cap) == _ffi.KH_ERR_RANGE
    assert code([R[0], V, R[1]], 0) == _ffi.KH_ERR_RANGE
    assert code([R[0], -1], 0) == _ffi.KH_ERR_RANGE
    for layer, (k, v) in enumerate(sentinel):  # every error came before any launch
        gk, gv = m.read_kv(layer, 0, 12)
        assert gk.tobytes() == k.tobytes() and gv.tobytes() == v.tobytes()
    nxt, a = m.verify(R[4:8], 4)  # the rows are still the prefill's
    assert a == 3 and list(nxt) == R[5:9]
    m.close()
    # a geometry outside the pass (head size 32): unsupported, width included
    spec, img, gt, _ = load_golden("hf_llama_half")
    g = KuiperModel.from_host_image(img, spec)
    for call in (lambda: g.verify([int(t) for t in gt[:4]], 0), g.verify_width,
                 lambda: g.generate_lookup([int(t) for t in gt[:4]], 12)):
        with pytest.raises(_ffi.KhError) as ei:
            call()
        assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
    g.close()


# ---- 3. the lookup loop -----------------------------------------------------------------------------------------------
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
_TRUTH = {}


def _steps(name):
    return 6 + 3 * S.BATCH[name] + 4


def _truth(gpu, name, prompt, T, **kw):
    """words of the twin's generate (graph), cached"""
    _ref(gpu, name)
    key = (name, tuple(prompt), T, tuple(sorted(kw.items())))
    if key not in _TRUTH:
        twin = _model(gpu, name, flags=EXACT)
        _TRUTH[key] = twin.generate(prompt, T, exec="graph", **kw)[0]
        twin.close()
    return _TRUTH[key]


def _text(prompt, words):
    """the token of every position: the prompt, then the sampled words (words[:n_prompt - 1] are the forced prompt)"""
    return list(prompt) + list(words[len(prompt) - 1:])


def _check(words, stats, W, n_prompt):
    assert words == W
    assert stats["accepted"] + stats["passes"] + stats["plain_steps"] == len(W) - (n_prompt - 1), stats
    assert 0 <= stats["accepted"] <= stats["drafted"] and stats["passes"] <= stats["drafted"], stats


@pytest.mark.parametrize("name", NAMES)
def test_lookup_generates_the_words_of_generate(gpu, name):
    V, width, T = S.SPECS[name].vocab_size, S.BATCH[name], _steps(name)
    P = S.tokens(name, 6)
    W = _truth(gpu, name, P, T)
    assert len(W) == T
    m = _model(gpu, name, flags=EXACT)
    assert m.verify_width() == width
    # the truth as the hint: the first pass is deterministic - behind the plain first step, the suffix of the sequence
    # is found at the hint's own copy of it and its followers are the truth
    hint = _text(P, W)
    words, ms, st = m.generate_lookup(P, T, hint=hint)
    _check(words, st, W, 6)
    assert st["accepted"] >= width - 1 and st["passes"] >= 1 and ms > 0, st
    assert m.first_sample()["top1_id"] == W[5]  # the first sampled step ran alone, with the full classifier
    # ... the literal prompt + words (the forced words repeat the prompt)
    words, _, st = m.generate_lookup(P, T, hint=list(P) + list(W))
    _check(words, st, W, 6)
    # every third token of the hint wrong
    bad = [(t + 1) % V if i % 3 == 2 else t for i, t in enumerate(hint)]
    words, _, st = m.generate_lookup(P, T, hint=bad)
    _check(words, st, W, 6)
    # no hint, nothing to find but exact 6-grams: the step graphs, 1, 4 and 8 steps per round trip; 0 is the default, 8
    seen = []
    for miss in (1, 4, 8, 0):
        words, _, st = m.generate_lookup(P, T, ngram_max=6, ngram_min=6, miss_steps=miss)
        _check(words, st, W, 6)
        seen.append(st)
    assert seen[3] == seen[2]
    # the last pass is clipped by total_steps
    Tc = 6 + width + 3
    Wc = _truth(gpu, name, P, Tc)
    words, _, st = m.generate_lookup(P, Tc, hint=hint)
    _check(words, st, Wc, 6)
    assert Wc == W[:Tc]
    # a generate on the same model after lookup runs: the same words
    assert m.generate(P, T, exec="graph")[0] == W
    m.close()


@pytest.mark.parametrize("name", ["a", "b"])
def test_lookup_drafts_from_a_periodic_prompt(gpu, name):
    T = _steps(name) + 2
    P = [5, 9] * 4
    W = _truth(gpu, name, P, T)
    m = _model(gpu, name, flags=EXACT)
    words, _, st = m.generate_lookup(P, T)
    _check(words, st, W, 8)
    # by the drafter's definition: the loop visits every position behind the plain first step until one drafts
    text = _text(P, W)
    expect = any(lookup_draft(text[:p + 1], None, 4, 1, 1) for p in range(8, T - 1))
    print(f"model ({name}): a draft is due: {expect}; stats {st}")
    assert st["drafted"] > 0 and expect, st
    # a prompt too short for a prefill: the prompt phase runs on the step graphs, and [5, 5] drafts at once
    W2 = _truth(gpu, name, [5, 5], T)
    words, _, st = m.generate_lookup([5, 5], T)
    _check(words, st, W2, 2)
    assert st["drafted"] > 0 and m.first_sample() is None, st
    m.close()


def test_lookup_long_run_crosses_the_time_split_threshold(gpu):
    P = S.tokens("a", 6)
    T = S.LONG_N
    W = _truth(gpu, "a", P, T)
    m = _model(gpu, "a", flags=EXACT)
    words, _, st = m.generate_lookup(P, T, hint=_text(P, W))
    _check(words, st, W, 6)
    assert st["accepted"] >= 7 and st["passes"] < T - 5, st
    words, _, st = m.generate_lookup(P, T, ngram_max=6, ngram_min=6, miss_steps=8)
    _check(words, st, W, 6)
    m.close()


@pytest.mark.parametrize("name", ["a", "b"])
def test_lookup_stops_like_generate_until(gpu, name):
    T = _steps(name)
    P = S.tokens(name, 6)
    W = _truth(gpu, name, P, T)
    sampled = W[5:]
    # the first sampled word at index >= 3 that has not occurred earlier: inside the first pass's accepted run when a
    # pass takes 8 tokens (positions 6 .. 13).  A synthetic model's text can settle into a cycle before that: then the
    # latest first occurrence it has
    new = [i for i in range(len(sampled)) if sampled[i] not in sampled[:i]]
    i = next((i for i in new if i >= 3), new[-1])
    print(f"model ({name}): stop at sampled index {i} of {sampled[:12]}")
    m = _model(gpu, name, flags=EXACT)
    for stop in ([sampled[i]], [W[3]], [sampled[i], 1, 2]):
        want = _truth(gpu, name, P, T, stop=tuple(stop))
        words, _, st = m.generate_lookup(P, T, stop=stop, hint=_text(P, W))
        assert words == want, (stop, st)
    assert _truth(gpu, name, P, T, stop=(sampled[i],)) == W[:5 + i]
    m.close()


def test_fused_truth_is_the_graph_truth(gpu):
    P = S.tokens("a", 6)
    W = _truth(gpu, "a", P, _steps("a"))
    twin = _model(gpu, "a", flags=EXACT)
    assert twin.generate(P, _steps("a"), exec="fused")[0] == W
    twin.close()


def test_lookup_refuses_what_it_does_not_cover(gpu):
    T = _steps("a")
    P = S.tokens("a", 6)
    W = _truth(gpu, "a", P, T)
    m = _model(gpu, "a", flags=EXACT)
    assert m.generate(P[:3], 12, exec="graph")[0]  # some state to keep
    kv = [m.read_kv(layer, 0, 16) for layer in range(S.SPECS["a"].n_layers)]

    def refused():
        with pytest.raises(_ffi.KhError) as ei:
            m.generate_lookup(P, T, hint=_text(P, W))
        assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
        for layer, (k, v) in enumerate(kv):  # before any launch
            gk, gv = m.read_kv(layer, 0, 16)
            assert gk.tobytes() == k.tobytes() and gv.tobytes() == v.tobytes()
    m.set_sampling(0.8, 50, 0.95, 7)
    refused()
    m.set_sampling()
    m.set_penalties(repetition=1.2)
    refused()
    m.set_penalties()
    m.set_logit_bias({3: 1.0})
    refused()
    m.set_logit_bias(None)
    m.set_logprobs(0)
    refused()
    m.set_logprobs(None)
    assert m.generate(P, T, exec="graph")[0] == W
    with pytest.raises(_ffi.KhError) as ei:
        m.generate_lookup(P, T, hint=[0, S.SPECS["a"].vocab_size])
    assert ei.value.code == _ffi.KH_ERR_RANGE
    with pytest.raises(_ffi.KhError) as ei:
        m.generate_lookup(P, m.cfg.cache_len + 1)
    assert ei.value.code == _ffi.KH_ERR_RANGE
    words, _, st = m.generate_lookup(P, T, hint=_text(P, W))
    _check(words, st, W, 6)
    m.close()


def test_launch_log_names_the_new_kernels_only_where_they_run(gpu):
    want = {"a": "k_pf_cls<false,8>", "b": "k_pf_cls<true,4>"}
    try:
        for name, kern in want.items():
            T = _steps(name)
            P = S.tokens(name, 6)
            W = _truth(gpu, name, P, T)
            m = _model(gpu, name, flags=EXACT)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
            m.generate(P, T, exec="graph")
            log = _ffi.launch_log()
            assert log and not any(k.startswith(("k_spec", "k_pf_cls")) for k in log), log  # a plain generate: none
            m.generate_lookup(P, T, hint=_text(P, W))
            log = _ffi.launch_log()
            assert {"k_spec_pick", "k_spec_accept", kern} <= log, (name, sorted(log))
            m.close()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)


# ---- 4. demo CLI ------------------------------------------------------------------------------------------------------
def test_demo_cli_lookup_prints_the_words_and_the_stats(gpu, tmp_path):
    import subprocess
    from kuiperllama_amd import build
    spec, T = S.SPECS["a"], _steps("a")
    P = S.tokens("a", 6)
    W = _truth(gpu, "a", P, T)
    path = tmp_path / "m.bin"
    _REF["a"]["img"].cpu().numpy().tofile(path)
    hint = _text(P, W)
    m = _model(gpu, "a", flags=EXACT)
    _, _, st = m.generate_lookup(P, T, hint=hint, ngram_max=3)
    m.close()
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--exact-prefill", "--max-seq-len", str(spec.seq_len), "--steps", str(T),
            "--prompt", ",".join(map(str, P)), "--lookup", "3", "--hint", ",".join(map(str, hint))]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.startswith("lookup:"))
    assert [int(t) for t in lines[at - 1].split()] == W
    f = lines[at].split()
    assert {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)} == st
    bad = subprocess.run(args + ["--temperature", "0.8"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0  # greedy only: refused, not rerouted
