"""CPU side of the scoring classifier on the bf16 matrix cores (csrc/kh_score_gemm_w16.h): the library holds exactly the
two k_pg_cls_lse_w16 instantiations, and kh_cls_logprobs_w16_f32 answers its argument codes before any device call."""
import ctypes as C

import pytest

import code_objects as co
from kuiperllama_amd import _ffi, build


def test_compiled_instantiations():
    if not co.tools_present():
        pytest.skip("LLVM tools of the ROCm install not found")
    got = co.instantiations(co.code_object_notes(build.build_lib()), {"k_pg_cls_lse_w16"})
    assert got == {"k_pg_cls_lse_w16<4>", "k_pg_cls_lse_w16<8>"}, sorted(got)


# (W16, X, workspace, T, vocab, dim) -> code; 16 stands for any non-NULL, 16-byte aligned address: none is followed
@pytest.mark.parametrize("w,x,ws,T,vocab,dim,code", [
    (None, 16, 16, 4, 16, 32, "KH_ERR_INVALID_ARG"),
    (16, None, 16, 4, 16, 32, "KH_ERR_INVALID_ARG"),
    (16, 16, None, 4, 16, 32, "KH_ERR_INVALID_ARG"),
    (16, 16, 16, 513, 16, 32, "KH_ERR_RANGE"),
    (16, 16, 16, 4, 16, 48, "KH_ERR_UNSUPPORTED"),   # dim % 32 (the fp32 entry takes 48)
    (16, 16, 16, 4, 16, 16, "KH_ERR_UNSUPPORTED"),
    (16, 16, 16, 4, 24, 32, "KH_ERR_UNSUPPORTED"),   # vocab % 16
])
def test_argument_codes_come_before_any_device_call(w, x, ws, T, vocab, dim, code):
    assert "kh_cls_logprobs_w16_f32" in _ffi.EXPORTS
    p = lambda v: None if v is None else C.c_void_p(v)
    rc = _ffi.lib().kh_cls_logprobs_w16_f32(p(w), p(x), T, vocab, dim, None, 0, None, None, None, None, None, None, p(ws),
                                            0, None)
    assert rc == getattr(_ffi, code)
