"""KuiperModel.score(tokens, gemm=True) (kh_model_score_gemm, csrc/kh_score_gemm.h) against score(tokens) of a twin
model, on the models and token strings of tests/score_gemm_cases.py.  The contract is kh_model_prefill_gemm's: logprob
and top_logprobs within twice the GEMM logit tolerance at EVERY position (the k-th largest of perturbed values stays
within the perturbation), top_ids equal wherever the VALU run's first TOP + 1 log-probs have no near tie; the share left
out is printed and must stay under 5 % (tests/test_score_gemm.py: the same strings on the CPU oracle)."""
import numpy as np
import pytest

import score_cases as S
import score_gemm_cases as K
from kuiperllama_amd import _ffi, binfmt, constraint
from kuiperllama_amd.model import KuiperModel

pytestmark = pytest.mark.gpu
TOP = K.TOP


def _model(name):
    spec = K.CASES[name][0]
    return KuiperModel.from_host_image(K.image(name), spec, max_seq_len=spec.seq_len)


@pytest.mark.parametrize("name", list(K.CASES))
def test_records_match_the_valu_pass_and_the_state_is_prefill_gemm_s(gpu, name):
    spec, m, twin = K.CASES[name][0], _model(name), _model(name)
    m.set_logprobs(TOP + 1)
    twin.set_logprobs(TOP + 1)
    left_out = total = 0
    try:
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        for chunk, text in K.runs(name):
            n = len(text)
            _ffi.debug_set("KH_PG_CHUNK", chunk)
            got, want = m.score(text, gemm=True), twin.score(text)
            assert list(got["token"]) == list(want["token"]) and got["token"][-1] == -1
            assert np.isnan(got["logprob"][-1]) and (got["top_ids"][-1] >= 0).all()  # the last position: a filled list
            assert np.abs(got["logprob"][:-1] - want["logprob"][:-1]).max() <= K.tol(name)
            assert np.abs(got["top_logprobs"][:, :TOP] - want["top_logprobs"][:, :TOP]).max() <= K.tol(name)
            ok = K.clear(want["top_logprobs"], name)
            assert (got["top_ids"][ok, :TOP] == want["top_ids"][ok, :TOP]).all()
            left_out, total = left_out + n - int(ok.sum()), total + n
            twin.prefill_gemm(text)  # (the same passes under the same hook)
            for layer in range(spec.n_layers):
                for a, b in zip(m.read_kv(layer, 0, n), twin.read_kv(layer, 0, n)):
                    assert a.tobytes() == b.tobytes(), (layer, n)
        want_kernel = f"k_pg_cls_lse<{'true' if spec.quant else 'false'},{8 if name == 'q8' else 4}>"
        assert want_kernel in _ffi.launch_log(), sorted(_ffi.launch_log())
    finally:
        _ffi.debug_set("KH_PG_CHUNK", None)
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    print(f"model {name}: top ids left unchecked at {left_out} of {total} positions")
    assert left_out < 0.05 * total
    m.close()
    twin.close()


def test_refusals_launch_nothing_and_the_default_is_the_valu_pass(gpu):
    toks = S.tokens("a", 9)
    m, twin = _model("a"), _model("a")
    img_d = binfmt.synth_image(S.SPECS["d"], seed=11, device=gpu)
    d = KuiperModel.from_device_image(img_d, S.SPECS["d"])

    def refused(model, t):
        _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
        with pytest.raises(_ffi.KhError) as ei:
            model.score(t, gemm=True)
        assert ei.value.code == _ffi.KH_ERR_UNSUPPORTED and not _ffi.launch_log(), _ffi.launch_log()

    def log_of(model, *args, **kw):
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        model.score(*args, **kw)
        return sorted(_ffi.launch_log())
    try:
        refused(m, toks)  # log-probs never turned on
        m.set_logprobs(2)
        twin.set_logprobs(2)
        m.set_constraint(constraint.from_choices([toks[:3]], toks[3]))
        refused(m, toks)  # a constraint is set
        m.set_constraint(None)
        d.set_logprobs(2)
        refused(d, S.tokens("d", 5))  # vocab_size % 16 != 0
        plain = log_of(twin, toks)
        assert log_of(m, toks, 0, gemm=False) == plain and "k_score_lp" in plain  # what it always launched
        assert not any(k.startswith(("k_pg_cls_lse", "k_pg_lse_merge")) for k in plain)
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        for x in (m, twin, d):
            x.close()
