"""The B-token passes of W16 models (kh_w16_pass.h), host side: the hook KH_W16_PASS, the ABI of kh_model_w16_info and
the kernels in the library's gfx950 code objects - the five _w16 pass stems with exactly the fp32 lists' products
(B in {8, 4}, gemv_res {8, 4, 2}; SPLIT {2, 1} for qkv, {4, 2, 1} for gemv_res), none with scratch, and the fp32 /
int8 pass kernels with the sets they had before the twins existed.  CPU only."""
import code_objects as co
import wcopy_cases as wc
from kuiperllama_amd import _ffi, build

W16_PASS, EXISTING = wc.PASS_W16_COMPILED, wc.PASS_COMPILED_BEFORE


def test_hook_is_in_the_table():
    build.build_lib()
    assert "KH_W16_PASS".startswith(_ffi._HOOK_PREFIXES)  # sync_env mirrors it from the environment
    assert _ffi.debug_get("KH_W16_PASS") is None
    with wc.hook("KH_W16_PASS", "0x5"):
        assert _ffi.debug_get("KH_W16_PASS") == "0x5"
    assert _ffi.debug_get("KH_W16_PASS") is None


def test_w16_info_abi():
    build.build_lib()
    L = _ffi.lib()
    out = (_ffi._i64 * 8)()
    assert L.kh_model_w16_info(None, out) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_model_w16_info(None, None) == _ffi.KH_ERR_INVALID_ARG
    from kuiperllama_amd.model import KuiperModel
    assert callable(KuiperModel.w16_pass_info)  # fails on a library without the feature


def test_pass_kernels_in_the_code_objects():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    notes = co.code_object_notes(build.build_lib())
    assert set(W16_PASS) == wc.PASS["w16"] and set(EXISTING) == wc.PASS_F32
    assert sum(len(v) for v in W16_PASS.values()) == 21
    for stem, want in W16_PASS.items():
        got = co.instantiations(notes, {stem})
        assert got == want, (stem, sorted(got - want), sorted(want - got))
    for stem, want in EXISTING.items():
        got = co.instantiations(notes, {stem})
        assert got == want, (stem, sorted(got - want), sorted(want - got))
    scratch = {co.template_name(k): v for k, v in co.kernel_scratch(notes).items()
               if (co.template_name(k) or "").split("<")[0] in W16_PASS}
    assert len(scratch) == 21, sorted(scratch)
    assert not any(scratch.values()), {k: v for k, v in scratch.items() if v}
