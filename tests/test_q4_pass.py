"""The B-token passes of Q4 models (kh_q4_pass.h), host side: the hook KH_Q4_PASS, the ABI of kh_model_q4_info, the
build lists and the kernels in the library's gfx950 code objects - the five _q4 pass stems with exactly the int8 level
of the fp32 lists (B 4, gemv_res {4, 2}; SPLIT {2, 1} for qkv, {4, 2, 1} for gemv_res: 12 instantiations), none with
scratch, and every other pass / decode set as it was before the twins existed.  CPU only."""
import code_objects as co
import wcopy_cases as wc
from kuiperllama_amd import _ffi, build

PASS_Q4 = {s + "_q4" for s in wc.PASS_F32}
# the int8 level of wc.PASS_COMPILED_BEFORE with the stem renamed
Q4_PASS_COMPILED = {stem + "_q4": {k.replace(f"{stem}<true,", f"{stem}_q4<") for k in names if k.startswith(f"{stem}<true,")}
                    for stem, names in wc.PASS_COMPILED_BEFORE.items()}
COUNTS = {"k_pf_qkv_q4": 2, "k_seq_qkv_q4": 2, "k_pf_ffn13_q4": 1, "k_pf_gemv_res_q4": 6, "k_pf_cls_q4": 1}


def test_hook_is_in_the_table():
    build.build_lib()
    assert "KH_Q4_PASS".startswith(_ffi._HOOK_PREFIXES)  # sync_env mirrors it from the environment
    assert _ffi.debug_get("KH_Q4_PASS") is None
    with wc.hook("KH_Q4_PASS", "0x5"):
        assert _ffi.debug_get("KH_Q4_PASS") == "0x5"
    assert _ffi.debug_get("KH_Q4_PASS") is None


def test_q4_info_abi_and_build_lists():
    build.build_lib()
    L = _ffi.lib()
    out = (_ffi._i64 * 8)()
    assert L.kh_model_q4_info(None, out) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_model_q4_info(None, None) == _ffi.KH_ERR_INVALID_ARG
    from kuiperllama_amd.model import KuiperModel
    assert callable(KuiperModel.q4_pass_info)  # fails on a library without the feature
    assert "kh_model_q4_pass.hip" in build.SOURCES and "kh_q4_pass.h" in build.HEADERS


def test_pass_kernels_in_the_code_objects():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    notes = co.code_object_notes(build.build_lib())
    assert set(Q4_PASS_COMPILED) == PASS_Q4
    assert {k: len(v) for k, v in Q4_PASS_COMPILED.items()} == COUNTS and sum(COUNTS.values()) == 12
    assert Q4_PASS_COMPILED["k_pf_gemv_res_q4"] == {f"k_pf_gemv_res_q4<{sp},{b}>" for sp in (4, 2, 1) for b in (4, 2)}
    for stem, want in Q4_PASS_COMPILED.items():  # fails on a library without the feature: no such kernels
        got = co.instantiations(notes, {stem})
        assert got == want, (stem, sorted(got - want), sorted(want - got))
    scratch = {co.template_name(k): v for k, v in co.kernel_scratch(notes).items()
               if (co.template_name(k) or "").split("<")[0] in PASS_Q4}
    assert len(scratch) == 12, sorted(scratch)
    assert not any(scratch.values()), {k: v for k, v in scratch.items() if v}


def test_the_other_sets_are_what_they_were():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    notes = co.code_object_notes(build.build_lib())
    # the fp32 / int8 pass kernels, their _w16 twins and the _h16 mirror of those
    for stem, want in wc.PASS_COMPILED_BEFORE.items():
        got = co.instantiations(notes, {stem})
        assert got == want, (stem, sorted(got - want), sorted(want - got))
    for stem, want in wc.PASS_W16_COMPILED.items():
        got = co.instantiations(notes, {stem})
        assert got == want, (stem, sorted(got - want), sorted(want - got))
        h16 = stem[:-4] + "_h16"
        assert h16 in wc.PASS["h16"]
        got = co.instantiations(notes, {h16})
        assert got == {k.replace(stem, h16) for k in want}, (h16, sorted(got))
    # the 89 decode _q4 instantiations: the int8 lists of their twins (tests/test_q4.py)
    decode = {
        "k_qkv_q4": {f"k_qkv_q4<{u},{mv},{sp}>" for u in (4, 2) for mv in (4, 2, 1, 0) for sp in (1, 2)},
        "k_gemv_res_q4": {f"k_gemv_res_q4<{u},{mv},{sp}>" for u in (4, 3, 2) for mv in (6, 4, 2, 1, 0) for sp in (1, 2, 4)},
        "k_wo_comb_q4": {f"k_wo_comb_q4<{u},{mv},{sp}>" for u in (4, 2) for mv in (2, 4) for sp in (1, 2, 4)},
        "k_ffn13_q4": {f"k_ffn13_q4<{u},{mv}>" for u in (4, 2) for mv in (4, 2, 1, 0)},
        "k_cls_q4": {f"k_cls_q4<{u},{mv}>" for u in (4, 2) for mv in (4, 2, 1, 0)},
    }
    assert set(decode) == wc.DECODE["q4"] and sum(len(v) for v in decode.values()) == 89
    for stem, want in decode.items():
        got = co.instantiations(notes, {stem})
        assert got == want, (stem, sorted(got - want), sorted(want - got))
