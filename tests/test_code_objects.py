"""The gfx950 code objects inside the built library: no kernel may use scratch memory (a register spill in a
latency-bound decode kernel is a memory round trip per use), and the kernels the decode step launches exist.
Reads the .hip_fatbin section of kuiperllama_amd/lib/libkuiper_hip.so with the LLVM tools of the ROCm install (no GPU).
Round 6 found 20-24 bytes of scratch in six k_wo_comb instantiations after a branch had been removed from their
merge loop (the compiler hoisted every factor read and crossed the 128-register cap): this test is the tripwire."""
import pytest

import code_objects as co
from kuiperllama_amd import build


def _code_object_notes():
    if not co.tools_present():
        pytest.skip("LLVM tools of the ROCm install not found")
    return co.code_object_notes(build.build_lib())


def test_no_kernel_uses_scratch_and_step_kernels_exist():
    kernels = co.kernel_scratch(_code_object_notes())
    assert len(kernels) > 100, f"only {len(kernels)} kernel descriptors parsed"
    spilled = {k: v for k, v in kernels.items() if v}
    assert not spilled, f"kernels with scratch (bytes): {spilled}"
    for stem in ("k_qkv", "k_attn_decode", "k_gemv_res", "k_wo_comb", "k_ffn13", "k_ffn13_ring", "k_cls", "k_cls_ring",
                 "k_sample", "k_pg_gemm", "k_pg_attn"):
        assert any(stem in k for k in kernels), f"no {stem} instantiation in the library"


def test_qkv_is_compiled_for_its_reachable_splits_only():
    """k_qkv's shape is never split more than twice (plan_decode_shapes: max_split 2; the KH_SHAPE_QKV hook rejects 4),
    so the library compiles SPLIT 1 and 2 only: 40 instantiations = fp32 U 8/4/2 and int8 U 4/2, times MAXV 4/2/1/0,
    times SPLIT 1/2.  The mangled-name reader of code_objects.py must also read the arguments back.
    Every other kernel picked from per-parameter value lists (kh_dispatch.h) is pinned the same way: the lists of its
    launch site compile exactly these products, 265 instantiations in all."""
    assert co.template_name("_Z5k_qkvILb0ELi2ELi0ELi1EEv9KhQkvArgs") == "k_qkv<false,2,0,1>"
    assert co.template_name("_Z12k_ffn13_ringILi2ELi4ELb0E9StagerAsmILb1ELi4ELi0EEEv11KhFfn13Args") == \
        "k_ffn13_ring<2,4,false>"
    qkv = co.instantiations(_code_object_notes(), {"k_qkv"})
    want = {f"k_qkv<{q},{u},{mv},{sp}>" for q, us in (("false", (8, 4, 2)), ("true", (4, 2))) for u in us
            for mv in (4, 2, 1, 0) for sp in (1, 2)}
    assert qkv == want, (sorted(qkv - want), sorted(want - qkv))
    notes = _code_object_notes()
    Q = (("false", (8, 4, 2)), ("true", (4, 2)))  # <QUANT, U ...>: U as k_qkv's
    want = {
        "k_gemv_res": {f"k_gemv_res<{q},{u},{mv},{sp}>" for q, us in (("false", (8, 4, 2)), ("true", (4, 3, 2)))
                       for u in us for mv in (6, 4, 2, 1, 0) for sp in (1, 2, 4)},
        "k_wo_comb": {f"k_wo_comb<{q},{u},{mv},{sp}>" for q, us in Q for u in us for mv in (2, 4) for sp in (1, 2, 4)},
        "k_ffn13": {f"k_ffn13<{q},{u},{mv}>" for q, us in Q for u in us for mv in (4, 2, 1, 0)},
        "k_cls": {f"k_cls<{q},{u},{mv}>" for q, us in Q for u in us for mv in (4, 2, 1, 0)},
        "k_ffn13_ring": {"k_ffn13_ring<2,4,false>"},
        "k_cls_ring": {"k_cls_ring<2,4,false>"},
        "k_cls_screen": {f"k_cls_screen<{u},{mv}>" for u in (4, 2) for mv in (4, 2, 1)},
        "k_sample_screen": {f"k_sample_screen<{u},{mv}>" for u in (8, 4, 2) for mv in (4, 2, 1)},
        "k_pf_gemv_res": {f"k_pf_gemv_res<{q},{sp},{b}>" for q, bs in (("false", (8, 4, 2)), ("true", (4, 2)))
                          for sp in (1, 2, 4) for b in bs},
        "k_pf_qkv": {f"k_pf_qkv<{q},{sp},{b}>" for q, bs in (("false", (8, 4)), ("true", (4,))) for sp in (1, 2) for b in bs},
        "k_pf_ffn13": {f"k_pf_ffn13<{q},{b}>" for q, bs in (("false", (8, 4)), ("true", (4,))) for b in bs},
        "k_pg_gemm": {f"k_pg_gemm<{q},{r},{nt},{epi}>" for q in ("false", "true")
                      for r, nt in ((2, 8), (2, 4), (2, 2), (1, 4)) for epi in (0, 1, 2)},
    }
    assert len(qkv) + sum(len(w) for w in want.values()) == 265
    for stem, w in want.items():
        got = co.instantiations(notes, {stem})
        assert got == w, (stem, sorted(got - w), sorted(w - got))


def test_plain_kernel_names_are_read_back():
    """k_pg_rope is a static, non-template kernel: template_name() has no name for it, plain_name() and kernels() do."""
    assert co.plain_name("_ZL9k_pg_ropePfS_PKfS1_iiiii") == "k_pg_rope"
    assert co.plain_name("_Z8k_samplePKfiPi") == "k_sample"
    assert co.plain_name("_Z5k_qkvILb0ELi2ELi0ELi1EEv9KhQkvArgs") is None
    assert co.plain_name("main") is None
    assert co.template_name("_ZL9k_pg_ropePfS_PKfS1_iiiii") is None
    got = co.kernels(_code_object_notes(), {"k_pg_rope", "k_pg_rmsnorm"})
    assert got == {"k_pg_rope", "k_pg_rmsnorm<false>", "k_pg_rmsnorm<true>"}, sorted(got)
