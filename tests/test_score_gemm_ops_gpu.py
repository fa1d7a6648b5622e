"""ops.cls_logprobs (kh_cls_logprobs_f32: csrc/kh_score_gemm.h, k_pg_cls_lse + k_pg_lse_merge) against numpy fp64:
W.astype(f64) @ X.T, log-sum-exp, target log-prob, top-N by (value descending, id ascending).

Shapes at the kernel's seams: dim 64 / 192 (the phase loop and the ring); vocab 16, one 128-row block, one block + 16,
three blocks + 16, and 16400 rows x 129 tokens (more workgroups than the chip holds at once); T 1, 15,
16, 17, and one slice + 1 of both token tiles (65, 129).  Targets sit on the first and last row of a block; the last
token's id is -1 (NaN).  Rows 127 and 128 are equal - a tie across the block boundary, on top of token 0's list; in
"few" only rows 0 .. 9 have finite logits.

Two kinds of data.  "grid": W, X multiples of 2^-5 with |sum| < 2^9 - every product and partial sum is exact in fp32 in
any order, so the kernel's logits ARE the fp64 ones: ids (natural ties included) must be equal exactly, target logit -
max exactly, and lse / lp within logprobs_ref.tol alone.  "normal": Gaussian data; a logit is a chain of dim fmaf, so
|l32 - l64| <= g = dim 2^-24 sum_k |w_k x_k|; lse moves by at most max g and lp by g_target + max g, added to tol; ids
must be equal exactly wherever no gap among the first top_n + 1 fp64 logits is within 2 max g (nothing else can
reorder them)."""
import numpy as np
import pytest
import torch

import logprobs_ref as L
from kuiperllama_amd import ops

pytestmark = pytest.mark.gpu

VOCABS = (16, 128, 144, 400)
TS = (1, 15, 16, 17, 65, 129)
CASES = [((64, 192)[(vi + ti) % 2], v, t, False) for vi, v in enumerate(VOCABS) for ti, t in enumerate(TS)]
CASES += [(64, 144, 17, True), (192, 400, 65, True)]  # fewer finite logits than top_n
CASES += [(64, 16400, 129, False)]


def _data(kind, dim, vocab, T, few):
    rng = np.random.default_rng(dim * 1000003 + vocab * 1009 + T)
    if kind == "grid":
        w = rng.integers(-32, 33, (vocab, dim)).astype(np.float32) / 32
        x = rng.integers(-64, 65, (T, dim)).astype(np.float32) / 32
    else:
        w = (0.5 * rng.standard_normal((vocab, dim))).astype(np.float32)
        x = rng.standard_normal((T, dim)).astype(np.float32)
    if vocab > 128:
        w[127] = w[128] = np.sign(x[0]) * (1.0 if kind == "grid" else 0.5)  # equal rows, token 0's largest logits
    if few:
        w[10:, 0] = -np.inf
        x[:, 0] = 1.0
    edges = [r for r in (0, 127, 128, 255, 256, vocab - 1) if r < vocab]
    tgt = np.array([edges[t % len(edges)] for t in range(T)], np.int32)
    tgt[-1] = -1
    return w, x, tgt


@pytest.mark.parametrize("kind", ["grid", "normal"])
@pytest.mark.parametrize("dim,vocab,T,few", CASES)
def test_cls_logprobs_against_fp64(gpu, kind, dim, vocab, T, few):
    w, x, tgt = _data(kind, dim, vocab, T, few)
    w64, x64 = w.astype(np.float64), x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        lg = x64 @ w64.T  # [T, vocab]
    g = np.zeros_like(lg)
    if kind == "normal":
        g = dim * 2.0 ** -24 * (np.abs(x64) @ np.abs(np.where(np.isfinite(w64), w64, 0.0)).T)
    gmax = g.max(axis=1)
    dw, dx, dt = (torch.from_numpy(a).to(gpu) for a in (w, x, tgt))
    worst = 0.0
    for top_n in (0, 1, min(20, vocab)):
        out = {k: v.cpu().numpy() for k, v in ops.cls_logprobs(dw, dx, dt, top_n).items()}
        assert out["top_ids"].shape == out["top_logprobs"].shape == (T, top_n)
        for t in range(T):
            what = (kind, dim, vocab, T, top_n, t)
            lse, lp = _lse64(lg[t])
            order = np.lexsort((np.arange(vocab), -lg[t]))
            close = lambda got, i: (got == lp[i]) if np.isneginf(lp[i]) else \
                abs(float(got) - lp[i]) <= L.tol(vocab, lse, lp[i]) + g[t, i] + gmax[t]
            err = abs(float(out["lse"][t]) - lse)
            worst = max(worst, err / (L.tol(vocab, lse) + gmax[t]))
            assert err <= L.tol(vocab, lse) + gmax[t], what
            if tgt[t] < 0:
                assert np.isnan(out["logprob"][t]) and np.isnan(out["target_logit"][t]), what
            else:
                assert close(out["logprob"][t], tgt[t]), what
                if kind == "grid":
                    assert float(out["target_logit"][t]) - float(out["max"][t]) == lg[t, tgt[t]] - lg[t].max(), what
            head = lg[t, order[:top_n + 1]]
            with np.errstate(invalid="ignore"):
                gaps = head[:-1] - head[1:]
            if kind == "grid" or (np.isfinite(head).all() and (gaps > 2 * gmax[t]).all()):
                assert list(out["top_ids"][t]) == list(order[:top_n]), what
                for got, i in zip(out["top_logprobs"][t], order[:top_n]):
                    assert close(got, i), what
    none = ops.cls_logprobs(dw, dx, None, 0)  # no targets: NaN, the same lse
    assert torch.isnan(none["logprob"]).all() and torch.equal(none["lse"].cpu(), torch.from_numpy(out["lse"]))
    print(f"{kind} dim {dim} vocab {vocab} T {T}: largest lse error / bound = {worst:.3f}")


def _lse64(l):
    m = l.max()
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(l - m).sum())
    return float(lse), l - lse
