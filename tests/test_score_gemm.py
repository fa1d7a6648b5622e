"""CPU side of sequence scoring on the GEMM pass (kh_model_score_gemm, csrc/kh_score_gemm.h): the symbols and the Python
keyword exist, and - on the oracle, which loads fp32, int8 and Qwen2 images alike - the very token strings the GPU test
scores leave under 5 % of the positions with a near tie among the first TOP + 1 logits."""
import inspect

import numpy as np
import pytest

import score_gemm_cases as K
from kuiperllama_amd import _ffi
from kuiperllama_amd.model import KuiperModel


def test_symbols_and_keyword_exist():
    lib = _ffi.lib()
    for n in ("kh_model_score_gemm", "kh_cls_logprobs_f32", "kh_cls_logprobs_workspace_bytes"):
        assert n in _ffi.EXPORTS and hasattr(lib, n), n
    assert inspect.signature(KuiperModel.score).parameters["gemm"].default is False
    assert lib.kh_model_score_gemm(None, None, 4, 0) == _ffi.KH_ERR_INVALID_ARG


@pytest.mark.parametrize("name", list(K.CASES))
def test_oracle_top_lists_are_clear_of_the_tolerance(oracle, name):
    near = total = 0
    for _, text in K.runs(name):
        om = oracle.OracleModel.from_spec(K.image(name), K.CASES[name][0])
        rows = np.stack([np.array(om.forward(t, p), np.float64) for p, t in enumerate(text)])
        om.close()
        near += int((~K.clear(-np.sort(-rows, axis=1)[:, :K.TOP + 1], name)).sum())
        total += len(text)
    print(f"{name}: {near} of {total} positions with a near tie")
    assert near < 0.05 * total
