"""KuiperModel.score(tokens, gemm=True) with the classifier on the bf16 matrix cores (csrc/kh_score_gemm_w16.h) against
the same call with the classifier on the fp32 image: models of ONE bf16-rounded image under KH_FLAG_W16 | KH_FLAG_GEMM16,
created under KH_GEMM16_CLASSES=0x1f, 0xf and the default mask.  They run the same layer kernels (byte-equal K/V rows)
and differ in the classifier alone.  Geometries: those of score_gemm_cases.CASES with dim % 32 == 0 and vocab_size % 16
== 0 that are not int8 (an int8 image has no 16-bit copy); strings and the pass boundary: score_gemm_cases.runs (on the
CPU oracle the rounded images leave 0 of 83 positions of either geometry with a near tie)."""
import numpy as np
import pytest

import score_gemm_cases as K
from kuiperllama_amd import _ffi, binfmt
from kuiperllama_amd.model import KuiperModel

pytestmark = pytest.mark.gpu
TOP = K.TOP
NAMES = [n for n, (spec, _) in K.CASES.items() if spec.dim % 32 == 0 and spec.vocab_size % 16 == 0 and not spec.quant]
FLAGS = _ffi.KH_FLAG_W16 | _ffi.KH_FLAG_GEMM16


def _model(img, spec, mask):
    _ffi.debug_set("KH_GEMM16_CLASSES", mask)
    try:
        m = KuiperModel.from_host_image(img, spec, max_seq_len=spec.seq_len, flags=FLAGS)
    finally:
        _ffi.debug_set("KH_GEMM16_CLASSES", None)
    m.set_logprobs(TOP + 1)
    return m


def _scores(m, spec, name):
    """-> ([records of a run], [K/V rows of a run], the launches)"""
    recs, rows = [], []
    try:
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        for chunk, text in K.runs(name):
            _ffi.debug_set("KH_PG_CHUNK", chunk)
            recs.append(m.score(text, gemm=True))
            rows.append([m.read_kv(layer, 0, len(text)) for layer in range(spec.n_layers)])
        return recs, rows, set(_ffi.launch_log())
    finally:
        _ffi.debug_set("KH_PG_CHUNK", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)


def _cls_stems(log):
    return {k.split("<")[0] for k in log if k.startswith("k_pg_cls_lse")}


@pytest.mark.parametrize("name", NAMES)
def test_bf16_classifier_against_the_fp32_one(gpu, name):
    spec = K.CASES[name][0]
    img = binfmt.round_matrices_bf16(K.image(name), spec)
    m16, m32, mdef = _model(img, spec, "0x1f"), _model(img, spec, "0xf"), _model(img, spec, None)
    try:
        assert m16.gemm16_info()["classes"] == ["qkv", "wo", "ffn13", "w2", "cls"]
        assert m32.gemm16_info()["classes"] == mdef.gemm16_info()["classes"] == ["qkv", "wo", "ffn13", "w2"]
        (got, kv16, log16), (want, kv32, log32) = _scores(m16, spec, name), _scores(m32, spec, name)
        assert _cls_stems(log16) == {"k_pg_cls_lse_w16"} and _cls_stems(log32) == {"k_pg_cls_lse"}, (log16, log32)
        assert log16 & {"k_pg_cls_lse_w16<4>", "k_pg_cls_lse_w16<8>"}
        assert {k for k in log16 if not k.startswith("k_pg_cls_lse")} == {k for k in log32 if not k.startswith("k_pg_cls_lse")}
        assert _scores(mdef, spec, name)[2] == log32  # inert: the default mask leaves the classifier where it was
        left_out = total = 0
        for g, w, rows16, rows32 in zip(got, want, kv16, kv32):
            n = len(w["token"])
            assert list(g["token"]) == list(w["token"]) and g["token"][-1] == -1
            assert np.isnan(g["logprob"][-1]) and (g["top_ids"][-1] >= 0).all()
            err = max(np.abs(g["logprob"][:-1] - w["logprob"][:-1]).max(),
                      np.abs(g["top_logprobs"][:, :TOP] - w["top_logprobs"][:, :TOP]).max())
            print(f"model {name}, {n} tokens: largest log-prob difference {err:.3e}, bound {K.tol(name):.3e}")
            assert err <= K.tol(name)
            ok = K.clear(w["top_logprobs"], name)
            assert (g["top_ids"][ok, :TOP] == w["top_ids"][ok, :TOP]).all()
            left_out, total = left_out + n - int(ok.sum()), total + n
            for (k16, v16), (k32, v32) in zip(rows16, rows32):
                assert k16.tobytes() == k32.tobytes() and v16.tobytes() == v32.tobytes()
        print(f"model {name}: top ids left unchecked at {left_out} of {total} positions")
        assert left_out < 0.05 * total
    finally:
        for m in (m16, m32, mdef):
            m.close()
