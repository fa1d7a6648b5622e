"""The C-ABI library loads without a GPU and exports every symbol include/kuiper_hip.h declares;
argument validation happens before any device call.  CPU only (no compute)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, load_golden
from kuiperllama_amd import _ffi, build


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _ffi.lib()


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "kuiper_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kh_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    names = _declared_functions()
    assert len(names) >= 28
    for n in names:
        assert hasattr(lib, n), f"{n} declared in kuiper_hip.h but not exported"
    assert sorted(_ffi.EXPORTS) == names


def test_version_and_error_strings(lib):
    assert lib.kh_version() == 100
    assert _ffi.error_string(0) == "success"
    assert "invalid" in _ffi.error_string(-1)
    assert "exception" in _ffi.error_string(_ffi.KH_ERR_INTERNAL)  # no C++ exception crosses the C ABI (kh_api_guard)
    assert lib.kh_kclass_name(3).decode() == "ffn13"


def test_invalid_arguments_are_rejected_without_touching_the_device(lib):
    assert lib.kh_add_f32(None, None, None, 4, None) == -1
    assert lib.kh_matmul_f32(None, None, None, 4, 4, 1.0, None) == -1
    assert lib.kh_matmul_q8(None, None, None, 64, None, 64, 4, None) == -1
    assert lib.kh_rmsnorm_f32(None, None, None, 0, 1e-5, None) == -1
    assert lib.kh_argmax_f32(None, 0, None, None) == -1
    assert lib.kh_model_get_config(None, None) == -1
    h = C.c_void_p()
    assert lib.kh_model_create_from_file(b"/nonexistent/model.bin",
                                         C.byref(_ffi.ModelOpts(0, 0, 0, 1e4, 1e-5, 0, 0, 0)),
                                         C.byref(h)) == -3  # KH_ERR_IO (reference: PathNotValid)


def test_model_creation_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from kuiperllama_amd.model import KuiperModel
    spec, img, _, _ = load_golden("ref_llama_gqa_tied")
    with pytest.raises(_ffi.KhError) as ei:
        KuiperModel.from_host_image(img, spec)
    assert ei.value.code == -5  # KH_ERR_NO_DEVICE: no silent CPU fallback


def test_ops_refuse_cpu_tensors():
    import torch
    from kuiperllama_amd import ops
    a = torch.zeros(4)
    with pytest.raises(ValueError):
        ops.add(a, a, a)


def test_debug_hooks_live_in_one_table_not_in_getenv(lib, monkeypatch):
    """Tuning / test hooks: set, read back, listed, cleared through kh_debug_*; the launch-plan entry
    points honour a hook set through the API; no translation unit of the library calls getenv."""
    assert lib.kh_debug_set(b"NOT_A_HOOK", b"1") == -1
    assert _ffi.debug_get("KH_TEST_HOOK") is None
    _ffi.debug_set("KH_TEST_HOOK", "abc")
    assert _ffi.debug_get("KH_TEST_HOOK") == "abc"
    n = lib.kh_debug_list(None, 0)
    buf = C.create_string_buffer(int(n))
    lib.kh_debug_list(buf, n)
    assert "KH_TEST_HOOK" in buf.value.decode().split("\n")
    _ffi.debug_set("KH_TEST_HOOK", None)
    assert _ffi.debug_get("KH_TEST_HOOK") is None
    # a shape hook set through the API changes the plan and SURVIVES the binding's environment mirror
    # (sync_env only manages the keys it took from os.environ); an environment variable of the same name
    # overrides it while it exists; clearing goes through the API again
    base = _ffi.plan_decode_shapes(2048, 8192, 512, 128256, False)["ffn13"]
    _ffi.debug_set("KH_SHAPE_FFN", "1,4,256,256")
    out = (C.c_int32 * 20)()
    assert lib.kh_plan_decode_shapes(2048, 8192, 512, 128256, 0, out) == 0
    assert list(out[8:12]) == [1, 4, 256, 256]
    assert _ffi.plan_decode_shapes(2048, 8192, 512, 128256, False)["ffn13"]["grid"] == 256  # sync_env left it alone
    monkeypatch.setenv("KH_SHAPE_FFN", "1,4,512,256")
    assert _ffi.plan_decode_shapes(2048, 8192, 512, 128256, False)["ffn13"]["grid"] == 512
    monkeypatch.delenv("KH_SHAPE_FFN")
    assert _ffi.plan_decode_shapes(2048, 8192, 512, 128256, False)["ffn13"] == base  # the mirrored key is cleared
    _ffi.debug_set("KH_SHAPE_FFN", None)
    # the LDS-DMA ring plan: int8 geometries whose input vector the 256-thread staging holds take it, KH_RING=0 turns it off
    assert _ffi.plan_decode_ring(4096, 11008, 32000, True) == {"ffn13": {"slots": 2, "grid": 512}, "cls": {"slots": 2, "grid": 512}}
    assert _ffi.plan_decode_ring(512, 1408, 501, True) == {"ffn13": {"slots": 2, "grid": 352}, "cls": {"slots": 2, "grid": 63}}
    assert _ffi.plan_decode_ring(2048, 8192, 128256, False)["ffn13"]["slots"] == 0   # fp32
    assert _ffi.plan_decode_ring(448, 1216, 3000, True)["cls"] == {"slots": 2, "grid": 375}  # partial pieces are fine
    assert _ffi.plan_decode_ring(8192, 28672, 128256, True)["ffn13"]["slots"] == 0  # 32 floats per staging thread
    monkeypatch.setenv("KH_RING", "0")
    assert _ffi.plan_decode_ring(4096, 11008, 32000, True)["ffn13"]["slots"] == 0
    monkeypatch.delenv("KH_RING")
    # a KH_SHAPE_FFN / KH_SHAPE_CLS hook names a register-tile launch: the ring must not take that launch over
    # (the B-token prefill follows the hook, decode silently ignored it)
    monkeypatch.setenv("KH_SHAPE_FFN", "1,4,512,256")
    r = _ffi.plan_decode_ring(4096, 11008, 32000, True)
    assert r["ffn13"]["slots"] == 0 and r["cls"]["slots"] == 2
    monkeypatch.delenv("KH_SHAPE_FFN")
    monkeypatch.setenv("KH_SHAPE_CLS", "1,4,512,256")
    r = _ffi.plan_decode_ring(4096, 11008, 32000, True)
    assert r["ffn13"]["slots"] == 2 and r["cls"]["slots"] == 0
    monkeypatch.delenv("KH_SHAPE_CLS")
    assert _ffi.plan_decode_ring(4096, 11008, 32000, True)["cls"]["slots"] == 2
    _ffi.sync_env()
    csrc = os.path.join(ROOT, "kuiperllama_amd", "csrc")
    for f in os.listdir(csrc):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_launch_helpers_take_their_target_as_arguments_not_toggled_model_state():
    """What a launch helper does beyond the model's plan travels as an argument: no source of the library
    redirects a helper by editing kh_model around the call.  The step tail, the classifier's buffers, ring or register
    tiles, the fenced merge and the screen's debug arrays have no field to toggle or none is assigned; scr.stale has
    three writers at the most; KH_ATTN_FENCED is read in one helper."""
    csrc = os.path.join(ROOT, "kuiperllama_amd", "csrc")
    lines = [(f, n + 1, re.sub(r"//.*", "", ln)) for f in sorted(os.listdir(csrc))
             for n, ln in enumerate(open(os.path.join(csrc, f)).read().split("\n"))]

    def sites(pattern):
        return [f"{f}:{n}" for f, n, ln in lines if re.search(pattern, ln)]
    assert sites(r"\b(scr|s)\.now\b|\bbool\s+now\b") == []           # ClsScreen::now
    assert sites(r"\b(scr|s)\.dbg_[lu]b\b") == []                    # ClsScreen::dbg_lb / dbg_ub
    assert sites(r"\bScreenOff\b|\bsg_sampler\b|\bstep_graph_n\b") == []
    assert sites(r"\bm->(x|logits|ring\.ffn_r|ring\.cls_r)\s*=[^=]") == []
    fenced = sites(r"(->|\.)attn_fenced\s*=[^=]")
    assert sorted(s.split(":")[0] for s in fenced) == ["kh_model_load.hip", "kh_model_selftest.hip"], fenced
    assert sites(r"(->|\.)attn_fenced\s*=\s*true;") == [s for s in fenced if s.startswith("kh_model_selftest.hip")]
    stale = sites(r"\.stale\s*=[^=]")  # the step enqueuer, the classifier launch into the model's buffer
    assert 1 <= len(stale) <= 3, stale
    assert {s.split(":")[0] for s in stale} <= {"kh_model_step.hip", "kh_model_internal.h"}, stale
    hook = sites(r'"KH_ATTN_FENCED"')
    assert len(hook) == 1 and hook[0].startswith("kh_attn.h:"), hook


def test_launch_log_hook_and_qkv_split_limit(lib):
    """KH_LAUNCH_LOG: kh_debug_launch_log reads the set of launched kernel instantiations like kh_debug_list (bytes
    needed, NUL-terminated, truncated to the buffer); setting, resetting and unsetting the hook leave it empty (no
    launch here: no device).  Every decode-GEMV, screened-classifier, B-token and GEMM prefill launch in the step /
    prefill / screen sources goes through the helper that logs it (kh_dispatch.h: kh_launch(KH_KERNEL(...))): those
    sources launch nothing but plain, non-template kernels themselves, and spell an instantiation of the logged
    families nowhere else (but for an LDS opt-in).  The qkv shape hook refuses split 4 (qkv's SPLIT = 4 kernels are not compiled)."""
    import re
    assert lib.kh_debug_launch_log(None, 0) == 1
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    assert _ffi.launch_log() == set()
    buf = C.create_string_buffer(4)
    buf.value = b"abc"
    assert lib.kh_debug_launch_log(buf, 4) == 1 and buf.value == b""
    _ffi.debug_set("KH_LAUNCH_LOG", "1")  # reset: a new, empty log
    assert _ffi.launch_log() == set()
    _ffi.debug_set("KH_LAUNCH_LOG", None)
    assert _ffi.launch_log() == set() and _ffi.debug_get("KH_LAUNCH_LOG") is None
    csrc = os.path.join(ROOT, "kuiperllama_amd", "csrc")
    family = r"k_qkv|k_gemv_res|k_wo_comb|k_ffn13|k_cls|k_ffn13_ring|k_cls_ring|k_cls_screen|k_sample_screen|k_pf_gemv_res|k_pf_qkv|k_pf_ffn13|k_pg_gemm|k_sg_gemm|k_rg_gemm"
    for f in ("kh_model_step.hip", "kh_model_prefill.hip", "kh_model_gemm.hip", "kh_model_screen.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert "<<<" not in src, f
        # a direct launch names a plain kernel: not an instantiation (k<...>), not a kernel passed in as a value
        for m in re.finditer(r"hipLaunchKernelGGL\(\s*([^,]*),", src):
            where = f"{f}:{src.count(chr(10), 0, m.start()) + 1}"
            assert re.fullmatch(r"k_[a-z0-9_]+", m.group(1)), f"{where}: launch outside kh_launch"
        # an instantiation of the families is spelled by KH_KERNEL alone (which hands it to the logging helper)
        for m in re.finditer(r"\b(%s)\s*<" % family, src):
            where = f"{f}:{src.count(chr(10), 0, m.start()) + 1}"
            assert "hipFuncSetAttribute(" in src[max(0, m.start() - 120):m.start()], f"{where}: instantiation outside KH_KERNEL"
        sites = re.findall(r"(?:\b(?:kh_launch|pf_launch)\(|\bkh_launch_prep\(\w+, )KH_KERNEL\(", src)
        assert len(sites) == src.count("KH_KERNEL(") > 0, f"{f}: KH_KERNEL outside a logging launch"
    base = _ffi.plan_decode_shapes(2048, 8192, 512, 128256, False)["qkv"]
    _ffi.debug_set("KH_SHAPE_QKV", "2,4,64,512")
    assert _ffi.plan_decode_shapes(2048, 8192, 512, 128256, False)["qkv"] == {"split": 2, "u": 4, "grid": 64, "wg": 512}
    _ffi.debug_set("KH_SHAPE_QKV", "4,4,64,512")
    assert _ffi.plan_decode_shapes(2048, 8192, 512, 128256, False)["qkv"] == base
    _ffi.debug_set("KH_SHAPE_QKV", None)
