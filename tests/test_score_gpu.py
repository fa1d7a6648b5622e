"""Sequence scoring on the GPU (kh_model_score: csrc/kh_prefill.h::k_pf_cls, csrc/kh_logprobs.h::k_score_lp).

The gate is BIT EQUALITY with what the tested pieces produce token by token: the logits of a loop of fused predict
calls on a twin model, handed row by row (each on a 16-byte aligned address, as the model's own logits buffer is) to
the operator kh_logprobs_f32.  Floats are compared as uint32, ids exactly; no tolerance is stated here.  The same
floats are also held to tests/logprobs_ref.tol against the fp64 twin, the existing bound of this core, and - model (a),
independently of every kernel of the project - to the oracle's fp64 log-softmax within 2 x 4e-5 + tol: the fp32 logit
parity bound enters once through l_i and once through lse.

No committed golden model fits the oracle check: every one has head_size <= 32, outside the mirrored prefill kernels,
so it runs on model (a) alone (one of them serves as the unsupported geometry of the error test).

Error table: with the widths the planner itself picks, the staging condition kh_stage_fits4(dim, classifier width)
never fails where prefill_supported holds - qkv and ffn13 run 256 threads, the classifier 256 (int8) or 512 (fp32) -
and only KH_SHAPE_QKV / KH_SHAPE_FFN overrides to 512 threads on an int8 model wider than 4096 reach it; that branch is
not exercised here.  KH_ERR_UNSUPPORTED is covered by "log-probs off" and by an unsupported geometry."""
import numpy as np
import pytest
import torch

import logprobs_ref as L
import score_cases as S
from conftest import load_golden
from kuiperllama_amd import _ffi, binfmt, ops
from kuiperllama_amd.model import KuiperModel

pytestmark = pytest.mark.gpu

INF = float("inf")
TOPS = (0, 3, 20)
KEYS = ("token", "logprob", "top_ids", "top_logprobs")


# ---- the token-by-token reference, once per model ---------------------------------------------------------------------
_REF = {}


def _model(gpu, name, **kw):  # (after _ref(gpu, name))
    r = _REF[name]
    return KuiperModel.from_device_image(r["img"], S.SPECS[name], max_seq_len=S.SPECS[name].seq_len, **kw)


def _ref(gpu, name):
    """image, tokens, and the logits a loop of fused predict calls leaves at every position: [T, vstride] on the
    device, vstride = V rounded up to 4 floats so that every row starts on a 16-byte boundary"""
    if name not in _REF:
        spec = S.SPECS[name]
        T = S.LONG_N + 1 if name == "a" else 5 + max(S.lengths(name)) + 1
        img = binfmt.synth_image(spec, seed=S.SEEDS[name], device=gpu)
        torch.cuda.synchronize()
        _REF[name] = r = {"img": img, "tokens": S.tokens(name, T)}
        twin = _model(gpu, name)
        V = spec.vocab_size
        rows = torch.zeros((T, (V + 3) & ~3), dtype=torch.float32, device=gpu)
        for p, t in enumerate(r["tokens"]):
            twin.predict(t, p, is_prompt=False, exec="fused")
            rows[p, :V] = torch.from_numpy(twin.logits()).to(gpu)
        twin.close()
        r["rows"] = rows
        r["want"] = {}
    return _REF[name]


def _want(gpu, name, p, target, top_n):
    """the operator on row p with id = target: (lp, top_ids, top_lp) as numpy, cached"""
    r = _ref(gpu, name)
    key = (p, target, top_n)
    if key not in r["want"]:
        V = S.SPECS[name].vocab_size
        out = ops.logprobs(r["rows"][p, :V], torch.tensor([target], dtype=torch.int32, device=gpu), top_n)
        torch.cuda.synchronize()
        r["want"][key] = (out["logprob"].cpu().numpy()[0], out["top_ids"].cpu().numpy()[0],
                          out["top_logprobs"].cpu().numpy()[0])
    return r["want"][key]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _check_bits(gpu, name, rec, pos0, n, top_n, twin64=True):
    """records of a score call of tokens[pos0 : pos0 + n] against the operator on the token-by-token logits, as raw
    bits; and against the fp64 twin of those logits within logprobs_ref.tol"""
    r = _ref(gpu, name)
    toks, V = r["tokens"], S.SPECS[name].vocab_size
    assert rec["top_ids"].shape == rec["top_logprobs"].shape == (n, top_n)
    for i in range(n):
        p = pos0 + i
        target = toks[p + 1] if i + 1 < n else -1
        lp, ids, tlp = _want(gpu, name, p, target, top_n)
        what = (name, pos0, n, top_n, p)
        assert rec["token"][i] == target, what
        assert list(rec["top_ids"][i]) == list(ids), what
        if target < 0:
            assert np.isnan(rec["logprob"][i]) and np.isnan(lp), what  # NaN equals NaN
        else:
            assert _bits(rec["logprob"][i]) == _bits(lp), (what, rec["logprob"][i], lp)
        assert (_bits(rec["top_logprobs"][i]) == _bits(tlp)).all(), (what, rec["top_logprobs"][i], tlp)
        if twin64:
            row = r["rows"][p, :V].cpu().numpy()
            lse, lp64, ids64, tlp64 = L.logprobs(row, top_n)
            assert list(rec["top_ids"][i]) == list(ids64), what
            if target >= 0:
                assert abs(float(rec["logprob"][i]) - lp64[target]) <= L.tol(V, lse, lp64[target]), what
            for g, w in zip(rec["top_logprobs"][i], tlp64):
                assert abs(float(g) - w) <= L.tol(V, lse, w), what


# ---- 1. bit equality with the token-by-token path ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_records_equal_the_token_by_token_path_bit_for_bit(gpu, name):
    r = _ref(gpu, name)
    toks = r["tokens"]
    m = _model(gpu, name)
    for top_n in TOPS:
        m.set_logprobs(top_n)
        for pos0 in (0, 5):
            for n in S.lengths(name):
                if pos0:  # the rows below pos0: scored on even lengths, prefilled on odd ones
                    m.score(toks[:pos0]) if n % 2 == 0 else m.prefill(toks[:pos0])
                rec = m.score(toks[pos0:pos0 + n], pos0)
                _check_bits(gpu, name, rec, pos0, n, top_n, twin64=top_n == 20)
                lp = rec["logprob"][:n - 1].astype(np.float64)
                assert rec["sum_logprob"] == float(lp.sum())
                if n > 1:
                    assert rec["perplexity"] == pytest.approx(np.exp(-lp.sum() / (n - 1)), rel=1e-12)
    m.close()


def test_long_run_crosses_the_time_split_threshold(gpu):
    r = _ref(gpu, "a")
    m = _model(gpu, "a")
    m.set_logprobs(20)
    rec = m.score(r["tokens"][:S.LONG_N])
    _check_bits(gpu, "a", rec, 0, S.LONG_N, 20)
    assert np.isfinite(rec["sum_logprob"]) and rec["perplexity"] > 1.0
    m.close()


# ---- 2. independent check against the oracle --------------------------------------------------------------------------
def test_scores_agree_with_the_oracle(gpu, oracle):
    img = S.oracle_image()
    toks, rows = S.oracle_rows(oracle, img)
    lp64, order, checkable = S.oracle_expectation(rows)
    V = S.SPECS["a"].vocab_size
    m = KuiperModel.from_host_image(img, S.SPECS["a"])
    m.set_logprobs(S.ORACLE_TOP)
    rec = m.score(toks)
    m.close()
    lse = -lp64 + rows.astype(np.float64)  # (every column: the row's lse)
    worst = 0.0
    for p in range(S.ORACLE_T):
        ids = [toks[p + 1]] if p + 1 < S.ORACLE_T else []
        got = [float(rec["logprob"][p])] if ids else []
        if checkable[p]:
            assert list(rec["top_ids"][p]) == list(order[p]), p
            ids += list(order[p])
            got += [float(v) for v in rec["top_logprobs"][p]]
        for g, i in zip(got, ids):
            bound = 2 * S.LOGIT_PARITY + L.tol(V, lse[p, 0], lp64[p, i])
            worst = max(worst, abs(g - lp64[p, i]) / bound)
            assert abs(g - lp64[p, i]) <= bound, (p, i, g, lp64[p, i], bound)
    print(f"largest err / bound = {worst:.3f}; top lists checked at {int(checkable.sum())} of {S.ORACLE_T} positions")
    assert checkable.mean() >= 0.9


# ---- 3. state left behind ---------------------------------------------------------------------------------------------
def _tail_none(rec, p, lo):
    """the record's top list holds no entry from index lo on"""
    return (rec["top_ids"][p, lo:] == -1).all() and np.isnan(rec["top_logprobs"][p, lo:]).all()


def _is_none(rec, p):
    return rec["token"][p] == -1 and np.isnan(rec["logprob"][p]) and _tail_none(rec, p, 0)


@pytest.mark.parametrize("name,pos0", [("a", 0), ("a", 5), ("b", 5)])
def test_state_left_behind(gpu, name, pos0):
    r = _ref(gpu, name)
    spec, toks, n = S.SPECS[name], r["tokens"], 2 * S.BATCH[name] + 3
    m, twin, fresh = _model(gpu, name), _model(gpu, name), _model(gpu, name)
    m.set_logprobs(20)
    words0, _ = m.generate(toks[:2], 40, exec="graph")  # sentinel records at positions 1 .. 39
    before = m.logprobs(0, 40)
    assert not _is_none(before, pos0 + n) and not _is_none(before, 39)
    m.set_logprobs(3)
    if pos0:
        m.prefill(toks[:pos0])
        twin.prefill(toks[:pos0])
    m.score(toks[pos0:pos0 + n], pos0)
    twin.prefill(toks[pos0:pos0 + n], pos0)
    for layer in range(spec.n_layers):  # the last layer included
        ka, va = m.read_kv(layer, 0, pos0 + n)
        kb, vb = twin.read_kv(layer, 0, pos0 + n)
        assert ka.tobytes() == kb.tobytes() and va.tobytes() == vb.tobytes(), layer
    # entries >= top_n are "none", records outside the range are the generate's
    m.set_logprobs(20)
    after = m.logprobs(0, 40)
    for p in range(pos0, pos0 + n):
        assert _tail_none(after, p, 3) and (after["top_ids"][p, :3] >= 0).all(), p
    for p in range(pos0):
        assert _is_none(after, p), p  # the prefill's "none"
    for p in range(pos0 + n, 40):
        for k in KEYS:
            assert after[k][p].tobytes() == before[k][p].tobytes(), (p, k)
    # the next step sees the same cache
    m.set_logprobs(None)
    a = m.predict(toks[pos0 + n], pos0 + n)
    b = twin.predict(toks[pos0 + n], pos0 + n)
    assert a == b and m.logits().tobytes() == twin.logits().tobytes()
    # decode state, sampler and processors were not touched: a generate produces a fresh model's words
    assert m.generate(toks[:3], 24, exec="graph")[0] == fresh.generate(toks[:3], 24, exec="graph")[0]
    for x in (m, twin, fresh):
        x.close()


# ---- 4. raw logits only -----------------------------------------------------------------------------------------------
def test_processors_and_sampler_never_enter(gpu):
    r = _ref(gpu, "a")
    toks = r["tokens"][:19]
    m = _model(gpu, "a")
    m.set_logprobs(5)
    plain = m.score(toks)
    m.set_penalties(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)
    m.set_logit_bias({toks[4]: -INF, toks[9]: 2.0, 11: 1.0})  # a token of the sequence is banned
    m.set_sampling(0.8, 50, 0.95, 0xC0FFEE)
    loaded = m.score(toks)
    for k in KEYS:
        assert loaded[k].tobytes() == plain[k].tobytes(), k
    assert np.isfinite(loaded["logprob"][3])  # the banned token's own log-prob: finite, the raw one
    assert loaded["sum_logprob"] == plain["sum_logprob"]
    m.close()


# ---- 5. launch log ----------------------------------------------------------------------------------------------------
def test_launch_log_names_the_new_kernels(gpu):
    want = {"a": "k_pf_cls<false,8>", "b": "k_pf_cls<true,4>", "d": "k_pf_cls<false,4>"}
    try:
        for name, kern in want.items():
            r = _ref(gpu, name)
            m = _model(gpu, name)
            m.set_logprobs(0)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
            m.prefill(r["tokens"][:5])
            m.generate(r["tokens"][:3], 12, exec="graph")
            log = _ffi.launch_log()
            assert not any(k.startswith(("k_pf_cls", "k_score_lp")) for k in log), log  # never scored: never launched
            m.score(r["tokens"][:S.BATCH[name] + 1])
            log = _ffi.launch_log()
            assert kern in log and "k_score_lp" in log, (name, sorted(log))
            assert [k for k in log if k.startswith("k_pf_cls")] == [kern]
            m.close()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)


# ---- 6. errors --------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    r = _ref(gpu, "a")
    toks, V = r["tokens"], S.SPECS["a"].vocab_size
    m = _model(gpu, "a")
    cap = m.cfg.cache_len

    def code(*a):
        with pytest.raises(_ffi.KhError) as ei:
            m.score(*a)
        return ei.value.code
    assert code(toks[:4]) == _ffi.KH_ERR_UNSUPPORTED  # log-probs never turned on
    m.set_logprobs(2)
    m.set_logprobs(None)
    assert code(toks[:4]) == _ffi.KH_ERR_UNSUPPORTED  # turned off again
    m.set_logprobs(2)
    m.generate(toks[:2], 16, exec="graph")
    before = m.logprobs(0, cap)
    assert code([]) == _ffi.KH_ERR_INVALID_ARG
    assert code(toks[:4], -1) == _ffi.KH_ERR_INVALID_ARG
    assert code(toks[:4], cap - 3) == _ffi.KH_ERR_RANGE
    assert code(toks[:4], cap) == _ffi.KH_ERR_RANGE
    assert code([toks[0], V, toks[1]]) == _ffi.KH_ERR_RANGE
    assert code([toks[0], -1]) == _ffi.KH_ERR_RANGE
    lib = _ffi.lib()
    assert lib.kh_model_score(m._h, None, 4, 0) == _ffi.KH_ERR_INVALID_ARG
    after = m.logprobs(0, cap)
    for k in KEYS:  # every error came before any launch
        assert after[k].tobytes() == before[k].tobytes(), k
    assert m.score(toks[:4], cap - 4)["token"][-1] == -1  # the last rows of the cache are in range
    m.close()
    # a geometry outside the mirrored kernels (head size 32): unsupported, and no fallback fills the records
    spec, img, gt, _ = load_golden("hf_llama_half")
    g = KuiperModel.from_host_image(img, spec)
    g.set_logprobs(2)
    with pytest.raises(_ffi.KhError) as ei:
        g.score([int(t) for t in gt[:4]])
    assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED
    rec = g.logprobs(0, 4)
    assert (rec["token"] == -1).all() and np.isnan(rec["logprob"]).all()
    g.close()


# ---- 7. demo CLI ------------------------------------------------------------------------------------------------------
def test_demo_cli_scores_the_prompt(gpu, tmp_path):
    import subprocess
    from kuiperllama_amd import build
    spec = S.SPECS["a"]
    r = _ref(gpu, "a")
    toks = r["tokens"][:11]
    path = tmp_path / "m.bin"
    r["img"].cpu().numpy().tofile(path)
    m = _model(gpu, "a")
    m.set_logprobs(2)
    rec = m.score(toks)
    m.close()
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--prompt", ",".join(map(str, toks)), "--logprobs", "2", "--score"]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    recs = [ln for ln in lines if "|" in ln]
    assert len(recs) == len(toks)
    for p, ln in enumerate(recs):
        head, tops = ln.split("|")
        pos, tok, lp = head.split()
        assert (int(pos), int(tok)) == (p, int(rec["token"][p]))
        if p + 1 < len(toks):
            assert float(lp) == pytest.approx(float(rec["logprob"][p]), abs=2e-6)
        else:
            assert np.isnan(float(lp))
        pairs = [t.split(":") for t in tops.split()]
        assert [int(i) for i, _ in pairs] == list(rec["top_ids"][p])
        assert [float(v) for _, v in pairs] == pytest.approx([float(v) for v in rec["top_logprobs"][p]], abs=2e-6)
    tail = dict(ln.split(":") for ln in lines if ln.startswith(("sum_logprob:", "perplexity:")))
    assert float(tail["sum_logprob"]) == pytest.approx(rec["sum_logprob"], abs=2e-5)
    assert float(tail["perplexity"]) == pytest.approx(rec["perplexity"], rel=1e-5)
    bad = subprocess.run([a for a in args if a not in ("--logprobs", "2")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0  # --score needs --logprobs
