"""ops.cls_logprobs with a bfloat16 w (kh_cls_logprobs_w16_f32: csrc/kh_score_gemm_w16.h) against numpy fp64, by the method
of test_score_gemm_ops_gpu.py: its "grid" and "normal" data (W bf16-exact; no -inf weights: the entry wants finite ones),
its per-token checks and its tie rule.  Shapes at this kernel's seams: dim 32 (one block: the prologue alone), 64 (both
LDS buffers), 96 (an odd block count) and 160 (longer than the weight ring, no multiple of its depth); vocab 16 (three
waves without a valid tile) .. 400; T 1 .. 17 (NT = 4, padded tiles), 65 (NT = 8), 129 (two slices); 16400 x 129: more
workgroups than CUs.  "grid": every product and partial sum is exact in fp32 (|sum| <= 320 < 2^9 at dim 160).  "normal":
the logit perturbation g is the bound gemm16_cases.general_case holds ops.gemm_w16 to on random operands."""
import numpy as np
import pytest
import torch

import logprobs_ref as L
import split3_ref as s3
from kuiperllama_amd import ops
from test_score_gemm_ops_gpu import _lse64

pytestmark = pytest.mark.gpu

DIMS = (32, 64, 96, 160)
VOCABS = (16, 128, 144, 400)
TS = (1, 15, 16, 17, 65, 129)
CASES = [(DIMS[(vi + ti) % 4], v, t) for vi, v in enumerate(VOCABS) for ti, t in enumerate(TS)]
CASES += [(64, 16400, 129)]


def _data(kind, dim, vocab, T):
    rng = np.random.default_rng(dim * 1000003 + vocab * 1009 + T)
    if kind == "grid":
        w = rng.integers(-32, 33, (vocab, dim)).astype(np.float32) / 32
        x = rng.integers(-64, 65, (T, dim)).astype(np.float32) / 32
    else:
        w = s3.trunc16((0.5 * rng.standard_normal((vocab, dim))).astype(np.float32))
        x = rng.standard_normal((T, dim)).astype(np.float32)
    if vocab > 128:
        w[127] = w[128] = np.sign(x[0]) * (1.0 if kind == "grid" else 0.5)  # equal rows, token 0's largest logits
    edges = [r for r in (0, 127, 128, 255, 256, vocab - 1) if r < vocab]
    tgt = np.array([edges[t % len(edges)] for t in range(T)], np.int32)
    tgt[-1] = -1
    return w, x, tgt


def _gemv_bound(gpu, w, x, lg):
    """2 x |kh_matmul_f32 - fp64| + one ulp of the largest |logit| (gemm16_cases.general_case)"""
    xd, wd = torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu)
    y32 = torch.empty(lg.shape, dtype=torch.float32, device=gpu)
    for t in range(x.shape[0]):
        ops.matmul(xd[t], wd, y32[t])
    e32 = float(np.abs(y32.cpu().numpy() - lg).max())
    return 2.0 * e32 + float(np.spacing(np.float32(np.abs(lg).max())))


@pytest.mark.parametrize("kind", ["grid", "normal"])
@pytest.mark.parametrize("dim,vocab,T", CASES)
def test_cls_logprobs_bf16_against_fp64(gpu, kind, dim, vocab, T):
    w, x, tgt = _data(kind, dim, vocab, T)
    assert s3.is_bf16(w).all()
    lg = x.astype(np.float64) @ w.astype(np.float64).T  # [T, vocab]
    g = _gemv_bound(gpu, w, x, lg) if kind == "normal" else 0.0
    dw = torch.from_numpy(s3.bf16_bits(w).view(np.int16)).to(gpu).view(torch.bfloat16)
    dx, dt = torch.from_numpy(x).to(gpu), torch.from_numpy(tgt).to(gpu)
    worst = 0.0
    for top_n in (0, 1, min(20, vocab)):
        out = {k: v.cpu().numpy() for k, v in ops.cls_logprobs(dw, dx, dt, top_n).items()}
        assert out["top_ids"].shape == out["top_logprobs"].shape == (T, top_n)
        for t in range(T):
            what = (kind, dim, vocab, T, top_n, t)
            lse, lp = _lse64(lg[t])
            order = np.lexsort((np.arange(vocab), -lg[t]))
            close = lambda got, i: abs(float(got) - lp[i]) <= L.tol(vocab, lse, lp[i]) + 2 * g
            err = abs(float(out["lse"][t]) - lse)
            worst = max(worst, err / (L.tol(vocab, lse) + g))
            assert err <= L.tol(vocab, lse) + g, what
            if tgt[t] < 0:
                assert np.isnan(out["logprob"][t]) and np.isnan(out["target_logit"][t]), what
            else:
                assert close(out["logprob"][t], tgt[t]), what
                if kind == "grid":
                    assert float(out["target_logit"][t]) - float(out["max"][t]) == lg[t, tgt[t]] - lg[t].max(), what
            head = lg[t, order[:top_n + 1]]
            if kind == "grid" or (head[:-1] - head[1:] > 2 * g).all():
                assert list(out["top_ids"][t]) == list(order[:top_n]), what
                for got, i in zip(out["top_logprobs"][t], order[:top_n]):
                    assert close(got, i), what
    none = ops.cls_logprobs(dw, dx, None, 0)  # no targets: NaN, the same lse
    assert torch.isnan(none["logprob"]).all() and torch.equal(none["lse"].cpu(), torch.from_numpy(out["lse"]))
    print(f"{kind} dim {dim} vocab {vocab} T {T}: largest lse error / bound = {worst:.3f}")
