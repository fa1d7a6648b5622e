"""The wide sequence pass without a GPU (csrc/kh_seq_gemm.h, kh_model_gemm.hip): the C-ABI symbols and their
ctypes signatures, kh_plan_seq_batch_wide against the Python twin of the grouping rule, the refusals that need no
device, the new kernel stems in the gfx950 code objects (zero scratch, exactly the instantiations the launch site
reaches), and the CPU oracle's margins on the batched-loop case of test_seq_gemm_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import code_objects as co
import seq_gemm_cases as G
from kuiperllama_amd import _ffi, build
from kuiperllama_amd.model import plan_seq_batch

NEW = ("kh_model_seq_width_gemm", "kh_model_seq_step_gemm", "kh_model_generate_batch_gemm", "kh_model_seq_gemm_logits",
       "kh_plan_seq_batch_wide")


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def test_symbols_and_signatures():
    L = _ffi.lib()
    for name in NEW:
        assert name in _ffi.EXPORTS and hasattr(L, name), name
    assert L.kh_model_seq_step_gemm.argtypes == L.kh_model_seq_step_ex.argtypes
    assert L.kh_model_generate_batch_gemm.argtypes == L.kh_model_generate_batch_ex.argtypes
    assert L.kh_plan_seq_batch_wide.argtypes == L.kh_plan_seq_batch.argtypes
    assert len(L.kh_model_seq_width_gemm.argtypes) == 2 and len(L.kh_model_seq_gemm_logits.argtypes) == 3


@pytest.mark.parametrize("width", [9, 16, 64])
def test_plan_wide_is_the_grouping_rule(width):
    rng = np.random.default_rng(width)
    for n_seq in sorted({1, width - 1, width, min(width + 1, 64), 64}):
        first = [int(x) for x in rng.integers(0, 5, n_seq)]
        totals = [f + int(x) for f, x in zip(first, rng.integers(1, 9, n_seq))]
        assert plan_seq_batch(first, totals, width, wide=True) == G.plan_twin(first, totals, width), (width, n_seq)


def test_plan_wide_refuses_65_and_the_narrow_plan_keeps_refusing_9():
    L, n = _ffi.lib(), C.c_int32(0)
    one = _i32([0])
    assert L.kh_plan_seq_batch_wide(1, 65, one, _i32([1]), None, 0, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_plan_seq_batch_wide(1, 0, one, _i32([1]), None, 0, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_plan_seq_batch_wide(65, 64, _i32([0] * 65), _i32([1] * 65), None, 0, C.byref(n)) == \
        _ffi.KH_ERR_INVALID_ARG
    # accepted: the pass count comes back with KH_ERR_RANGE while cap_passes is too small, as kh_plan_seq_batch's
    assert L.kh_plan_seq_batch_wide(1, 64, one, _i32([1]), None, 0, C.byref(n)) == _ffi.KH_ERR_RANGE and n.value == 1
    assert L.kh_plan_seq_batch(1, 9, one, _i32([1]), None, 0, C.byref(n)) == _ffi.KH_ERR_INVALID_ARG


def test_null_refusals_touch_no_device():
    """no model: every entry point answers KH_ERR_INVALID_ARG before it looks at anything else"""
    L = _ffi.lib()
    w, nxt, lg, ms = C.c_int32(0), _i32([0, 0]), (C.c_float * 4)(), C.c_float(0)
    two = _i32([0, 0])
    assert L.kh_model_seq_width_gemm(None, C.byref(w)) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_model_seq_step_gemm(None, 2, two, two, two, None, nxt) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_model_seq_step_gemm(None, 65, two, two, two, None, nxt) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_model_seq_gemm_logits(None, 0, lg) == _ffi.KH_ERR_INVALID_ARG
    assert L.kh_model_generate_batch_gemm(None, 2, two, two, None, two, None, None, 0, nxt, 1, two,
                                          C.byref(ms)) == _ffi.KH_ERR_INVALID_ARG


def _notes():
    if not co.tools_present():
        pytest.skip("LLVM tools of the ROCm install not found")
    return co.code_object_notes(build.build_lib())


def sg_gemm_set():
    """what kh_model_gemm.hip: pg_gemm can reach on a lane table: fp32 and int8, the tiles pg_shape picks or a KH_PG_SHAPE_* hook
    forces at <= 64 tokens (no 128-token tile), the three epilogues of the layer and KH_PG_STORE = 3"""
    return {f"k_sg_gemm<{q},{r},{nt},{epi}>" for q in ("false", "true") for r, nt in ((2, 4), (2, 2), (1, 4))
            for epi in (0, 1, 2, 3)}


def test_new_stems_are_compiled_without_scratch_for_the_reachable_set():
    notes = _notes()
    scratch = co.kernel_scratch(notes)
    mine = {k: v for k, v in scratch.items() if "k_sg_" in k}
    assert mine and not any(mine.values()), mine
    got = co.kernels(notes, {"k_sg_gemm", "k_sg_embed", "k_sg_rope"})
    assert got == sg_gemm_set() | {"k_sg_embed", "k_sg_rope"}, sorted(got ^ (sg_gemm_set() | {"k_sg_embed", "k_sg_rope"}))
    # the classifier epilogue exists under the new stem only
    assert not any(k.endswith(",3>") for k in co.instantiations(notes, {"k_pg_gemm"}))


def test_the_loop_case_has_margins(oracle):
    """test_seq_gemm_gpu.py compares the words of generate_batch(gemm=True) with a batch-1 twin up to the first pick
    whose top-1 minus top-2 gap is below 4 x the logit tolerance, and wants 90 % of the sampled words compared: the
    oracle's own margins on that case (same weights, same prompts) must leave that much."""
    spec = G.SPECS[G.LOOP_SPEC]
    om = oracle.OracleModel.from_spec(G.host_image(spec, wander=True), spec, cache_len=64)
    prompts, totals = G.loop_case(spec)
    free = [G.greedy_loop(lambda t, p: om.forward(t, p), pr, tot, (), G.logit_atol(spec))[0]
            for pr, tot in zip(prompts, totals)]
    stop = (free[5][len(prompts[5]) + 2],)
    compared = sampled = 0
    distinct = set()
    for pr, tot in zip(prompts, totals):
        words, near, _ = G.greedy_loop(lambda t, p: om.forward(t, p), pr, tot, stop, G.logit_atol(spec))
        first = len(pr) - 1
        sampled += len(words) - first
        compared += max(near - first, 0)
        distinct.update(words[first:])
    assert sampled >= 150 and len(distinct) >= 20, (sampled, len(distinct))
    assert compared >= 0.9 * sampled, (compared, sampled)
    om.close()
