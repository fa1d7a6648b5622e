"""ctypes binding of libkuiper_hip.so (include/kuiper_hip.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises, and
any op called without a GPU returns the library's error code as an exception.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KH_LIB") or os.path.join(_PKG, "lib", "libkuiper_hip.so")  # KH_LIB: experiment builds

# every symbol include/kuiper_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "kh_error_string", "kh_version", "kh_device_count",
    "kh_add_f32", "kh_matmul_f32", "kh_gemm_w16_f32", "kh_gemm_q8_bf16_f32", "kh_matmul_q8", "kh_embedding_f32", "kh_embedding_f32_host", "kh_swiglu_f32",
    "kh_rmsnorm_f32", "kh_rope_f32", "kh_sincos_cache_f32", "kh_mha_f32", "kh_mha_decode_f32", "kh_mha_prefill_f32",
    "kh_mha_prefill_layout_f32", "kh_mha_prefill_tiles_f32",
    "kh_mha_decode_workspace_bytes", "kh_argmax_f32", "kh_argmax_rows_f32",
    "kh_argmax_f32_host", "kh_sample_f32", "kh_sample_f32_host", "kh_logit_process_workspace_bytes", "kh_logit_process_f32", "kh_logprobs_f32", "kh_softmax_f32", "kh_scale_f32", "kh_scale_sum_f32",
    "kh_model_create_from_file", "kh_model_create_from_host_image",
    "kh_model_create_from_device_weights", "kh_model_destroy", "kh_model_get_config",
    "kh_model_stream", "kh_model_get_load_ms", "kh_model_predict", "kh_model_get_logits", "kh_model_cls_screen_info", "kh_model_cls_screen_probe", "kh_model_cls_screen_read", "kh_model_cls_screen_q8_info", "kh_model_cls_screen_q8_probe", "kh_model_cls_screen_q8_read", "kh_model_w16_info", "kh_model_q4_info", "kh_model_gemm16_info", "kh_model_gemm16_q8_info", "kh_model_get_kv", "kh_model_kv_bytes", "kh_model_read_kv", "kh_model_write_kv",
    "kh_spm_create_from_file", "kh_spm_create_from_memory", "kh_spm_destroy", "kh_spm_vocab_size",
    "kh_spm_bos_id", "kh_spm_eos_id", "kh_spm_unk_id", "kh_spm_encode", "kh_spm_decode",
    "kh_bpe_create_from_file", "kh_bpe_create_from_memory", "kh_bpe_destroy", "kh_bpe_vocab_size",
    "kh_bpe_bos_id", "kh_bpe_eos_id", "kh_bpe_stop_id", "kh_bpe_encode", "kh_bpe_decode",
    "kh_model_generate", "kh_model_generate_until", "kh_model_first_sample", "kh_model_set_sampling", "kh_model_get_sampling", "kh_model_set_penalties", "kh_model_get_penalties", "kh_model_set_logit_bias", "kh_model_set_logprobs", "kh_model_get_logprobs_setting", "kh_model_get_logprobs", "kh_model_time_step", "kh_model_prefill", "kh_model_prefill_gemm", "kh_model_score", "kh_model_verify_width", "kh_model_verify", "kh_model_generate_lookup", "kh_model_verify_as_set", "kh_model_generate_lookup_as_set", "kh_lookup_draft", "kh_lookup_draft_fsm", "kh_model_verify_fsm", "kh_model_generate_lookup_fsm", "kh_model_seq_slots", "kh_model_seq_width", "kh_model_seq_prefill", "kh_model_seq_fork", "kh_model_seq_step", "kh_model_generate_batch", "kh_model_generate_batch_from", "kh_model_seq_step_ex", "kh_model_generate_batch_ex", "kh_model_seq_set_history", "kh_model_seq_get_logprobs", "kh_seq_rank", "kh_model_time_prefill", "kh_model_profile_kernel", "kh_model_profile_step", "kh_kclass_name",
    "kh_plan_decode_shapes", "kh_plan_decode_ring", "kh_plan_w16", "kh_plan_q4", "kh_plan_gemm16", "kh_plan_gemm16_q8", "kh_plan_prefill_shape", "kh_plan_attention", "kh_plan_attention_launch", "kh_plan_seq_slots", "kh_plan_seq_batch",
    "kh_model_seq_slots_var", "kh_plan_seq_slots_var", "kh_model_seq_share", "kh_model_seq_row",
    "kh_model_seq_width_gemm", "kh_model_seq_step_gemm", "kh_model_generate_batch_gemm", "kh_model_seq_gemm_logits", "kh_plan_seq_batch_wide",
    "kh_plan_seq_prefill_gemm", "kh_model_seq_prefill_gemm",
    "kh_fsm_check", "kh_fsm_walk", "kh_token_mask_f32", "kh_model_set_constraint", "kh_model_get_constraint_state", "kh_model_set_constraint_state",
    "kh_model_seq_set_constraint", "kh_model_seq_set_constraint_state", "kh_model_seq_get_constraint_state", "kh_fsm_components", "kh_fsm_bias_empties",
    "kh_debug_set", "kh_debug_get", "kh_debug_list", "kh_debug_launch_log", "kh_debug_alloc_stats",
]

KH_EXEC_GRAPH, KH_EXEC_FUSED, KH_EXEC_UNFUSED = 0, 1, 2
KH_NUM_KCLASS = 7
KH_ERR_INVALID_ARG = -1
KH_ERR_UNSUPPORTED = -2
KH_ERR_RANGE = -6
KH_ERR_INTERNAL = -7
KH_FLAG_ATTN_MERGE_IN_LAUNCH = 1
KH_FLAG_ATTN_MERGE_FENCED = 2
KH_FLAG_PREFILL_EXACT = 4
KH_FLAG_NO_CLS_SCREEN = 8
KH_FLAG_W16 = 16
KH_FLAG_W16_F16 = 32  # the copy in whichever of bf16 / fp16 the image is exact in (KuiperModel.w16_format)
KH_W16_CLASSES = ("qkv", "wo", "ffn13", "w2", "cls")  # bit i of a class mask (kh_model_w16_info, kh_plan_w16)
KH_FLAG_Q4 = 64  # a 4-bit-exact int8 model decodes from a packed 4-bit copy of its matrices (KuiperModel.q4_info)
KH_FLAG_GEMM16 = 128  # the GEMM pass of a W16 model on the bf16 matrix cores, fp32-accurate (KuiperModel.gemm16_info)
# kh_model_gemm16_info, slot 2: why the flag does nothing on a model
KH_GEMM16_REASONS = ("on", "flag not set", "no W16 flag", "int8 model", "image not bf16-exact", "fp16-format copy",
                     "geometry", "no class", "self-check failed")
KH_FLAG_GEMM16_Q8 = 256  # the GEMM pass of an int8 group-64 model on the bf16 matrix cores (KuiperModel.gemm16_q8_info)
# kh_model_gemm16_q8_info, slot 2: why the flag does nothing on a model
KH_GEMM16_Q8_REASONS = ("on", "flag not set", "fp32 model", "group size not 64", "geometry", "no class")
KH_Q4_CLASSES = KH_W16_CLASSES  # bit i of a class mask (kh_model_q4_info, kh_plan_q4, hook KH_Q4_CLASSES)
KH_LOGPROBS_MAX_TOP = 20
KH_SEQ_BIAS_MAX = 64


class KhError(RuntimeError):
    def __init__(self, code: int, what: str):
        self.code = code
        super().__init__(f"{what}: kh error {code} ({error_string(code)})")


class ModelOpts(C.Structure):
    _fields_ = [("family", C.c_int32), ("is_quant", C.c_int32), ("rope_mode", C.c_int32),
                ("rope_theta", C.c_float), ("rms_eps", C.c_float), ("max_seq_len", C.c_int32),
                ("device", C.c_int32), ("flags", C.c_int32)]


class FirstSample(C.Structure):
    _fields_ = [("pos", C.c_int32), ("prefill_mode", C.c_int32), ("top1_id", C.c_int32), ("top2_id", C.c_int32),
                ("top1", C.c_float), ("top2", C.c_float)]


class Sampling(C.Structure):
    """kh_sampling: temperature <= 0 is greedy, top_k 0 and top_p 1 are off (include/kuiper_hip.h)."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("seed", C.c_uint64)]

    def as_dict(self) -> dict:
        return {"temperature": float(self.temperature), "top_k": int(self.top_k), "top_p": float(self.top_p),
                "seed": int(self.seed)}


def sampling(temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> Sampling:
    return Sampling(float(temperature), int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF)


class Penalties(C.Structure):
    """kh_penalties: repetition 1, presence 0 and frequency 0 are off; last_n 0 is the whole sequence."""
    _fields_ = [("repetition", C.c_float), ("presence", C.c_float), ("frequency", C.c_float), ("last_n", C.c_int32)]

    def as_dict(self) -> dict:
        return {"repetition": float(self.repetition), "presence": float(self.presence),
                "frequency": float(self.frequency), "last_n": int(self.last_n)}


def penalties(repetition: float = 1.0, presence: float = 0.0, frequency: float = 0.0, last_n: int = 0) -> Penalties:
    return Penalties(float(repetition), float(presence), float(frequency), int(last_n))


class Fsm(C.Structure):
    """kh_fsm: a token automaton in CSR form (row_ptr int64 [n_states + 1], tokens / next int32 [n_edges])."""
    _fields_ = [("n_states", C.c_int32), ("start", C.c_int32), ("row_ptr", C.POINTER(C.c_int64)),
                ("tokens", C.POINTER(C.c_int32)), ("next", C.POINTER(C.c_int32))]


def fsm(start, row_ptr, tokens, nxt, n_states=None):
    """(Fsm, keepalive) over numpy arrays; the arrays are converted to the struct's dtypes and must outlive the call."""
    import numpy as np
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    tk = np.ascontiguousarray(tokens, dtype=np.int32)
    nx = np.ascontiguousarray(nxt, dtype=np.int32)
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a.size else C.POINTER(t)()
    n = int(n_states) if n_states is not None else len(rp) - 1
    return Fsm(n, int(start), ptr(rp, C.c_int64), ptr(tk, C.c_int32), ptr(nx, C.c_int32)), (rp, tk, nx)


class SeqOpts(C.Structure):
    """kh_seq_opts: per-sequence arrays of an _ex call (NULL: the neutral value for everyone); logprobs_top_n -1 off."""
    _fields_ = [("samplings", C.POINTER(Sampling)), ("penalties", C.POINTER(Penalties)), ("n_bias", C.POINTER(C.c_int32)),
                ("bias_ids", C.POINTER(C.c_int32)), ("bias", C.POINTER(C.c_float)), ("logprobs_top_n", C.c_int32)]


class LookupOpts(C.Structure):
    """kh_lookup_opts: 0 = the default of a field (ngram_max 4, ngram_min 1, miss_steps 8); hint optional."""
    _fields_ = [("ngram_max", C.c_int32), ("ngram_min", C.c_int32), ("miss_steps", C.c_int32),
                ("h_hint", C.POINTER(C.c_int32)), ("n_hint", C.c_int32)]


class LookupStats(C.Structure):
    _fields_ = [("passes", C.c_int32), ("drafted", C.c_int32), ("accepted", C.c_int32), ("plain_steps", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dim", "hidden_dim", "layer_num", "head_num", "kv_head_num", "vocab_size", "seq_len",
        "kv_dim", "kv_mul", "head_size", "is_shared_weight", "is_quant", "group_size", "family",
        "rope_mode", "cache_len")] + [("rope_theta", C.c_float), ("rms_eps", C.c_float),
                                      ("weight_bytes", C.c_int64), ("launches_per_token", C.c_int32),
                                      ("ring_selftest", C.c_int32), ("attn_merge_selftest", C.c_int32)]


_lib: Optional[C.CDLL] = None
_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


def lib() -> C.CDLL:
    """Load the HIP library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles the HIP runtime (libamdhip64.so.7); loading it before our
    # library makes both bind to ONE runtime, so torch-owned device pointers/streams are valid
    # inside libkuiper_hip.so.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m kuiperllama_amd.build` "
            "(there is no CPU fallback for the HIP path)")
    L = C.CDLL(LIB_PATH)
    L.kh_error_string.argtypes = [C.c_int]
    L.kh_error_string.restype = C.c_char_p
    L.kh_version.restype = C.c_int
    L.kh_device_count.restype = C.c_int
    L.kh_add_f32.argtypes = [_vp, _vp, _vp, _i32, _vp]
    L.kh_matmul_f32.argtypes = [_vp, _vp, _vp, _i32, _i32, _f32, _vp]
    L.kh_matmul_q8.argtypes = [_vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp]
    L.kh_embedding_f32.argtypes = [_vp, _i32, _vp, _vp, _i32, _i32, _vp]
    L.kh_embedding_f32_host.argtypes = [_vp, _i32, _vp, _vp, _i32, _i32, _vp]
    L.kh_swiglu_f32.argtypes = [_vp, _vp, _vp, _i32, _vp]
    L.kh_rmsnorm_f32.argtypes = [_vp, _vp, _vp, _i32, _f32, _vp]
    L.kh_rope_f32.argtypes = [_i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp]
    L.kh_sincos_cache_f32.argtypes = [_i32, _i32, _f32, _vp, _vp, _vp]
    L.kh_mha_f32.argtypes = [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                             _vp, _vp]
    L.kh_mha_decode_workspace_bytes.argtypes = [_i32, _i32, _i32]
    L.kh_mha_decode_workspace_bytes.restype = _i64
    L.kh_mha_prefill_f32.argtypes = [_i32] * 8 + [_vp, _vp, _vp, _vp, _vp]
    L.kh_mha_prefill_layout_f32.argtypes = [_i32] * 10 + [_vp, _vp, _vp, _vp, _vp]
    L.kh_mha_prefill_tiles_f32.argtypes = [_i32, _vp] + [_i32] * 8 + [_vp, _vp, _vp, _vp, _vp]
    L.kh_mha_decode_f32.argtypes = [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                    _vp, _vp, _i64, _vp]
    L.kh_argmax_f32.argtypes = [_vp, _i64, _vp, _vp]
    L.kh_argmax_rows_f32.argtypes = [_vp, _i64, _i64, _i32, _vp, _vp]
    L.kh_argmax_f32_host.argtypes = [_vp, _i64, C.POINTER(_i64), _vp]
    L.kh_sample_f32.argtypes = [_vp, _i64, C.POINTER(Sampling), _i64, _i32, _vp, _vp]
    L.kh_sample_f32_host.argtypes = [_vp, _i64, C.POINTER(Sampling), _i64, C.POINTER(_i64), _vp]
    L.kh_logit_process_workspace_bytes.argtypes = [_i64]
    L.kh_logit_process_workspace_bytes.restype = _i64
    L.kh_logit_process_f32.argtypes = [_vp, _i64, _vp, _vp, _i32, C.POINTER(Penalties), _vp, _vp, _i32, _vp, _vp]
    L.kh_logprobs_f32.argtypes = [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]
    L.kh_softmax_f32.argtypes = [_vp, _i32, _vp]
    L.kh_scale_f32.argtypes = [_f32, _vp, _i32, _vp]
    L.kh_scale_sum_f32.argtypes = [_vp, _vp, _vp, _i32, _i32, _i32, _vp]
    L.kh_model_create_from_file.argtypes = [C.c_char_p, C.POINTER(ModelOpts), C.POINTER(_vp)]
    L.kh_model_create_from_host_image.argtypes = [_vp, C.c_size_t, C.POINTER(ModelOpts),
                                                  C.POINTER(_vp)]
    L.kh_model_create_from_device_weights.argtypes = [C.POINTER(_i32), _vp, C.c_size_t,
                                                      C.POINTER(ModelOpts), C.POINTER(_vp)]
    L.kh_model_destroy.argtypes = [_vp]
    L.kh_model_destroy.restype = None
    L.kh_model_get_config.argtypes = [_vp, C.POINTER(Config)]
    L.kh_model_stream.argtypes = [_vp]
    L.kh_model_stream.restype = _vp
    L.kh_model_get_load_ms.argtypes = [_vp]
    L.kh_model_get_load_ms.restype = _f32
    L.kh_model_predict.argtypes = [_vp, _i32, _i32, _i32, _i32, C.POINTER(_i32)]
    L.kh_model_get_logits.argtypes = [_vp, _vp]
    L.kh_model_cls_screen_info.argtypes = [_vp, C.POINTER(_i64)]
    L.kh_model_cls_screen_probe.argtypes = [_vp, _vp, _vp, _vp, C.POINTER(_i64)]
    L.kh_model_cls_screen_read.argtypes = [_vp, _vp, _vp]
    L.kh_model_cls_screen_q8_info.argtypes = [_vp, C.POINTER(_i64)]
    L.kh_model_cls_screen_q8_probe.argtypes = [_vp, _vp, _i32, _vp, _vp, C.POINTER(_i64)]
    L.kh_model_cls_screen_q8_read.argtypes = [_vp, _vp, _vp, _vp]
    L.kh_model_w16_info.argtypes = [_vp, C.POINTER(_i64)]
    L.kh_plan_w16.argtypes = [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64)]
    L.kh_model_q4_info.argtypes = [_vp, C.POINTER(_i64)]
    L.kh_model_gemm16_info.argtypes = [_vp, C.POINTER(_i64)]
    L.kh_plan_gemm16.argtypes = [_i32, _i32, _i32, _i32, _i32, C.POINTER(_i64)]
    L.kh_gemm_w16_f32.argtypes = [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]
    L.kh_model_gemm16_q8_info.argtypes = [_vp, C.POINTER(_i64)]
    L.kh_plan_gemm16_q8.argtypes = [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64)]
    L.kh_gemm_q8_bf16_f32.argtypes = [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]
    L.kh_plan_q4.argtypes = [_i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64)]
    L.kh_model_get_kv.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_vp)]
    L.kh_model_kv_bytes.argtypes = [_vp, C.POINTER(_i64), C.POINTER(_i64)]
    L.kh_model_read_kv.argtypes = [_vp, _i32, _i32, _i32, _vp, _vp]
    L.kh_model_write_kv.argtypes = [_vp, _i32, _i32, _i32, _vp, _vp]
    L.kh_model_generate.argtypes = [_vp, C.POINTER(_i32), _i32, _i32, _i32, C.POINTER(_i32),
                                    C.POINTER(_i32), C.POINTER(_f32)]
    L.kh_model_generate_until.argtypes = [_vp, C.POINTER(_i32), _i32, _i32, _i32, C.POINTER(_i32),
                                          _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_f32)]
    L.kh_model_first_sample.argtypes = [_vp, C.POINTER(FirstSample)]
    L.kh_model_set_sampling.argtypes = [_vp, C.POINTER(Sampling)]
    L.kh_model_get_sampling.argtypes = [_vp, C.POINTER(Sampling)]
    L.kh_model_set_penalties.argtypes = [_vp, C.POINTER(Penalties)]
    L.kh_model_get_penalties.argtypes = [_vp, C.POINTER(Penalties)]
    L.kh_model_set_logit_bias.argtypes = [_vp, C.POINTER(_i32), C.POINTER(_f32), _i32]
    L.kh_model_set_logprobs.argtypes = [_vp, _i32]
    L.kh_model_get_logprobs_setting.argtypes = [_vp, C.POINTER(_i32)]
    L.kh_model_get_logprobs.argtypes = [_vp, _i32, _i32, _vp, _vp, _vp, _vp]
    L.kh_model_time_step.argtypes = [_vp, _i32, _i32, C.POINTER(_f32)]
    L.kh_plan_decode_shapes.argtypes = [_i32, _i32, _i32, _i32, _i32, C.POINTER(_i32)]
    L.kh_plan_decode_ring.argtypes = [_i32, _i32, _i32, _i32, _i32, C.POINTER(_i32)]
    L.kh_plan_prefill_shape.argtypes = [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i32)]
    L.kh_plan_attention.argtypes = [_i32, _i32, _i32, _i32, _i32, C.POINTER(_i32)]
    L.kh_plan_attention_launch.argtypes = [_i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, C.POINTER(_i32)]
    L.kh_spm_create_from_file.argtypes = [C.c_char_p, C.POINTER(_vp)]
    L.kh_spm_create_from_memory.argtypes = [_vp, C.c_int64, C.POINTER(_vp)]
    L.kh_spm_destroy.argtypes = [_vp]
    L.kh_spm_destroy.restype = None
    for fn in (L.kh_spm_vocab_size, L.kh_spm_bos_id, L.kh_spm_eos_id, L.kh_spm_unk_id):
        fn.argtypes = [_vp]
        fn.restype = _i32
    L.kh_spm_encode.argtypes = [_vp, C.c_char_p, C.c_int64, _i32, _i32, C.POINTER(_i32), _i32,
                                C.POINTER(_i32)]
    L.kh_spm_decode.argtypes = [_vp, C.POINTER(_i32), _i32, C.c_char_p, C.c_int64,
                                C.POINTER(C.c_int64)]
    L.kh_bpe_create_from_file.argtypes = [C.c_char_p, _i32, C.POINTER(_vp)]
    L.kh_bpe_create_from_memory.argtypes = [_vp, C.c_int64, _i32, C.POINTER(_vp)]
    L.kh_bpe_destroy.argtypes = [_vp]
    L.kh_bpe_destroy.restype = None
    for fn in (L.kh_bpe_vocab_size, L.kh_bpe_bos_id, L.kh_bpe_eos_id):
        fn.argtypes = [_vp]
    L.kh_bpe_stop_id.argtypes = [_vp, _i32]
    L.kh_bpe_encode.argtypes = [_vp, C.c_char_p, C.c_int64, _i32, _i32, _i32, C.POINTER(_i32), _i32,
                                C.POINTER(_i32)]
    L.kh_bpe_decode.argtypes = [_vp, C.POINTER(_i32), _i32, _i32, C.c_char_p, C.c_int64,
                                C.POINTER(C.c_int64)]
    L.kh_model_prefill.argtypes = [_vp, C.POINTER(_i32), _i32, _i32]
    L.kh_model_score.argtypes = [_vp, C.POINTER(_i32), _i32, _i32]
    L.kh_model_verify_width.argtypes = [_vp, C.POINTER(_i32)]
    L.kh_model_verify.argtypes = [_vp, C.POINTER(_i32), _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]
    L.kh_model_generate_lookup.argtypes = [_vp, C.POINTER(_i32), _i32, _i32, C.POINTER(_i32), _i32,
                                           C.POINTER(LookupOpts), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_f32),
                                           C.POINTER(LookupStats)]
    L.kh_model_verify_as_set.argtypes = L.kh_model_verify.argtypes
    L.kh_model_generate_lookup_as_set.argtypes = L.kh_model_generate_lookup.argtypes
    L.kh_lookup_draft.argtypes = [C.POINTER(_i32), _i32, C.POINTER(_i32), _i32, _i32, _i32, C.POINTER(_i32), _i32]
    L.kh_lookup_draft_fsm.argtypes = [C.POINTER(Fsm), _i32] + L.kh_lookup_draft.argtypes + [C.POINTER(_i32)]
    L.kh_model_verify_fsm.argtypes = L.kh_model_verify.argtypes
    L.kh_model_generate_lookup_fsm.argtypes = L.kh_model_generate_lookup.argtypes + [C.POINTER(_i32)]
    L.kh_model_seq_slots.argtypes = [_vp, _i32, C.POINTER(_i32)]
    L.kh_plan_seq_slots.argtypes = [_i32, _i32, C.POINTER(_i32)]
    L.kh_model_seq_slots_var.argtypes = [_vp, _i32, C.POINTER(_i32)]
    L.kh_plan_seq_slots_var.argtypes = [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]
    L.kh_model_seq_share.argtypes = [_vp, _i32, _i32, _i32]
    L.kh_model_seq_row.argtypes = [_vp, _i32, _i32, C.POINTER(_i32)]
    L.kh_model_seq_width.argtypes = [_vp, C.POINTER(_i32)]
    L.kh_model_seq_prefill.argtypes = [_vp, _i32, C.POINTER(_i32), _i32, _i32]
    L.kh_model_seq_fork.argtypes = [_vp, _i32, _i32, _i32]
    L.kh_model_seq_step.argtypes = [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(Sampling),
                                    C.POINTER(_i32)]
    L.kh_model_generate_batch.argtypes = [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32),
                                          C.POINTER(Sampling), C.POINTER(_i32), _i32, C.POINTER(_i32), _i32,
                                          C.POINTER(_i32), C.POINTER(_f32)]
    L.kh_model_generate_batch_from.argtypes = [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32),
                                               C.POINTER(_i32), C.POINTER(Sampling), C.POINTER(_i32), _i32,
                                               C.POINTER(_i32), _i32, C.POINTER(_i32), C.POINTER(_f32)]
    L.kh_model_seq_step_ex.argtypes = [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(SeqOpts),
                                       C.POINTER(_i32)]
    L.kh_model_generate_batch_ex.argtypes = [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32),
                                             C.POINTER(_i32), C.POINTER(SeqOpts), C.POINTER(_i32), _i32,
                                             C.POINTER(_i32), _i32, C.POINTER(_i32), C.POINTER(_f32)]
    L.kh_model_seq_set_history.argtypes = [_vp, _i32, _i32, C.POINTER(_i32), _i32]
    L.kh_model_seq_get_logprobs.argtypes = [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]
    L.kh_seq_rank.argtypes = [_i32, C.POINTER(_f32), _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32),
                              C.POINTER(C.c_double)]
    L.kh_plan_seq_batch.argtypes = [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32, C.POINTER(_i32)]
    L.kh_plan_seq_batch_wide.argtypes = L.kh_plan_seq_batch.argtypes
    L.kh_model_seq_width_gemm.argtypes = [_vp, C.POINTER(_i32)]
    L.kh_model_seq_step_gemm.argtypes = L.kh_model_seq_step_ex.argtypes
    L.kh_model_generate_batch_gemm.argtypes = L.kh_model_generate_batch_ex.argtypes
    L.kh_model_seq_gemm_logits.argtypes = [_vp, _i32, C.POINTER(_f32)]
    L.kh_plan_seq_prefill_gemm.argtypes = [_i32, C.POINTER(_i32), C.POINTER(_i32), _i32, C.POINTER(_i32), C.POINTER(_i32)]
    L.kh_model_seq_prefill_gemm.argtypes = [_vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]
    L.kh_model_prefill_gemm.argtypes = [_vp, C.POINTER(_i32), _i32, _i32]
    L.kh_model_time_prefill.argtypes = [_vp, C.POINTER(_i32), _i32, _i32, _i32, C.POINTER(_f32)]
    L.kh_model_profile_kernel.argtypes = [_vp, _i32, _i32, _i32, C.POINTER(_f32)]
    L.kh_model_profile_step.argtypes = [_vp, _i32, _i32, C.POINTER(_f32), C.POINTER(_i32)]
    L.kh_kclass_name.argtypes = [C.c_int]
    L.kh_kclass_name.restype = C.c_char_p
    L.kh_debug_set.argtypes = [C.c_char_p, C.c_char_p]
    L.kh_debug_get.argtypes = [C.c_char_p]
    L.kh_debug_get.restype = C.c_char_p
    L.kh_debug_list.argtypes = [C.c_char_p, _i64]
    L.kh_debug_list.restype = _i64
    L.kh_debug_launch_log.argtypes = [C.c_char_p, _i64]
    L.kh_debug_launch_log.restype = _i64
    L.kh_debug_alloc_stats.argtypes = [C.POINTER(_i64)]
    L.kh_fsm_check.argtypes = [C.POINTER(Fsm), _i64]
    L.kh_fsm_walk.argtypes = [C.POINTER(Fsm), _i32, C.POINTER(_i32), _i64, C.POINTER(_i32), C.POINTER(_i64)]
    L.kh_token_mask_f32.argtypes = [_vp, _i64, _vp, _vp]
    L.kh_model_set_constraint.argtypes = [_vp, C.POINTER(Fsm)]
    L.kh_model_get_constraint_state.argtypes = [_vp, C.POINTER(_i32)]
    L.kh_model_set_constraint_state.argtypes = [_vp, _i32]
    L.kh_model_seq_set_constraint.argtypes = [_vp, C.POINTER(Fsm)]
    L.kh_model_seq_set_constraint_state.argtypes = [_vp, _i32, _i32]
    L.kh_model_seq_get_constraint_state.argtypes = [_vp, _i32, C.POINTER(_i32)]
    L.kh_fsm_components.argtypes = [C.POINTER(Fsm), C.POINTER(_i32)]
    L.kh_fsm_bias_empties.argtypes = [C.POINTER(Fsm), _i32, C.POINTER(_i32), C.POINTER(C.c_float), _i32, C.POINTER(_i32)]
    for name in EXPORTS:  # fail at load time, not at first call, if a symbol is missing
        getattr(L, name)
    _lib = L
    return L


def debug_set(key: str, value: Optional[str]) -> None:
    """Set (or with None: clear) one tuning / test hook of the library (kh_debug_set).  A hook set here stays
    until it is cleared here: sync_env() only manages the hooks it mirrored from os.environ itself."""
    _ENV_MIRRORED.pop(key, None)  # from now on the key belongs to the caller, not to the environment mirror
    check(lib().kh_debug_set(key.encode(), None if value is None else str(value).encode()), "kh_debug_set")


def debug_get(key: str) -> Optional[str]:
    v = lib().kh_debug_get(key.encode())
    return None if v is None else v.decode()


def launch_log() -> set:
    """Kernel instantiations launched since the hook KH_LAUNCH_LOG was last set (kh_debug_launch_log), e.g.
    {"k_qkv<false,8,4,2>", "k_pf_ffn13<true,4>"}.  debug_set("KH_LAUNCH_LOG", "1") starts an empty log, None ends it."""
    L = lib()
    n = L.kh_debug_launch_log(None, 0)
    buf = C.create_string_buffer(int(n) + 1)
    L.kh_debug_launch_log(buf, int(n) + 1)
    return {k for k in buf.value.decode().split("\n") if k}


def alloc_stats() -> dict:
    """The library's allocation accounting (kh_debug_alloc_stats): device and pinned-host buffers alive and their
    bytes, process-wide; allocations made and failures injected since debug_set("KH_ALLOC_FAIL", k | None)."""
    out = (_i64 * 4)()
    check(lib().kh_debug_alloc_stats(out), "kh_debug_alloc_stats")
    return {"live": int(out[0]), "live_bytes": int(out[1]), "allocs": int(out[2]), "injected": int(out[3])}


_HOOK_PREFIXES = ("KH_SHAPE_", "KH_ATTN_", "KH_PG_", "KH_PREFILL", "KH_RING", "KH_SELFTEST", "KH_KV_", "KH_W16", "KH_Q4", "KH_GEMM16")
_ENV_MIRRORED = {}  # hook -> value, as last written into the table FROM os.environ by sync_env()
_ENV_SEEDED = False


def _seed_mirror(L) -> None:
    """First sync: the library seeded its table from the KH_* environment when it was loaded.  Hooks that are in
    the table AND were in the environment then are environment-owned from the start (value as in the table), so
    that a variable removed from os.environ before the first sync_env() - monkeypatch.delenv - is cleared like
    any other; a key that is in the table only (kh_debug_set before the first sync) stays the caller's."""
    global _ENV_SEEDED
    _ENV_SEEDED = True
    n = L.kh_debug_list(None, 0)
    if n <= 0:
        return
    buf = C.create_string_buffer(int(n) + 1)
    L.kh_debug_list(buf, int(n) + 1)
    for k in buf.value.decode().split("\n"):
        if k and k.startswith(_HOOK_PREFIXES) and k in _ENV_AT_IMPORT:
            v = L.kh_debug_get(k.encode())
            if v is not None and v.decode() == _ENV_AT_IMPORT[k]:
                _ENV_MIRRORED.setdefault(k, _ENV_AT_IMPORT[k])


_ENV_AT_IMPORT = {k: v for k, v in os.environ.items() if k.startswith(_HOOK_PREFIXES)}


def sync_env() -> None:
    """Mirror the KH_* hook variables of os.environ into the library's hook table.

    The library reads the environment once, when it is loaded; afterwards hooks change only through
    kh_debug_set.  The Python binding calls this before every entry point that reads a hook, so
    `os.environ[...] = ...` / `monkeypatch.setenv` keep working in tests and tools.  Only keys that came from
    the environment are managed: a variable that disappears from os.environ is cleared in the table, a hook
    set through debug_set() is left alone (an environment variable of the same name overrides it)."""
    if not _ENV_SEEDED:
        _seed_mirror(lib())
    want = {k: v for k, v in os.environ.items() if k.startswith(_HOOK_PREFIXES)}
    if want == _ENV_MIRRORED:  # nothing changed since the last call: no table walk per generate()
        return
    L = lib()
    for k in set(_ENV_MIRRORED) - set(want):
        L.kh_debug_set(k.encode(), None)
        del _ENV_MIRRORED[k]
    for k, v in want.items():
        if _ENV_MIRRORED.get(k) != v:
            L.kh_debug_set(k.encode(), v.encode())
            _ENV_MIRRORED[k] = v


def error_string(code: int) -> str:
    return lib().kh_error_string(int(code)).decode()


def check(code: int, what: str) -> None:
    if code != 0:
        raise KhError(int(code), what)


def plan_decode_shapes(dim: int, hidden_dim: int, kv_dim: int, vocab_size: int, quant: bool) -> dict:
    """{kernel: {split, u, grid, wg}} of the five decode GEMV kernels for a geometry (host-only)."""
    sync_env()
    out = (_i32 * 20)()
    rc = lib().kh_plan_decode_shapes(dim, hidden_dim, kv_dim, vocab_size, int(quant), out)
    if rc != 0:
        raise KhError(rc, "kh_plan_decode_shapes")
    names = ("qkv", "wo", "ffn13", "w2", "cls")
    return {n: dict(zip(("split", "u", "grid", "wg"), out[4 * i:4 * i + 4])) for i, n in enumerate(names)}


def plan_decode_ring(dim: int, hidden_dim: int, vocab_size: int, quant: bool, group_size: int = 64) -> dict:
    """Which int8 decode GEMVs run on the LDS-DMA ring kernels: {ffn13: {slots, grid}, cls: {slots, grid}};
    slots 0 = the register-tile kernel of plan_decode_shapes (host-only, kh_plan_decode_ring)."""
    sync_env()
    out = (_i32 * 4)()
    rc = lib().kh_plan_decode_ring(dim, hidden_dim, vocab_size, int(quant), group_size, out)
    if rc != 0:
        raise KhError(rc, "kh_plan_decode_ring")
    return {"ffn13": {"slots": out[0], "grid": out[1]}, "cls": {"slots": out[2], "grid": out[3]}}


def plan_w16(dim: int, hidden_dim: int, kv_dim: int, vocab_size: int, n_layers: int, quant: bool) -> dict:
    """The 16-bit weight copy of KH_FLAG_W16 for a geometry (host-only, kh_plan_w16): {"classes": the decode launch
    classes that run on it ([]: not applicable, e.g. int8), "bytes": HBM the copy takes}."""
    out = (_i64 * 2)()
    rc = lib().kh_plan_w16(dim, hidden_dim, kv_dim, vocab_size, n_layers, int(quant), out)
    if rc != 0:
        raise KhError(rc, "kh_plan_w16")
    return {"classes": [n for i, n in enumerate(KH_W16_CLASSES) if out[0] >> i & 1], "bytes": int(out[1])}


def plan_gemm16(dim: int, hidden_dim: int, kv_dim: int, vocab_size: int, quant: bool) -> dict:
    """KH_FLAG_GEMM16 for a geometry (host-only, kh_plan_gemm16): {"classes": the launch classes whose GEMMs of the GEMM
    pass run on the bf16 matrix cores - [] for int8 and for dims the GEMM prefill does not take -, "kblock": 32}."""
    out = (_i64 * 2)()
    rc = lib().kh_plan_gemm16(dim, hidden_dim, kv_dim, vocab_size, int(quant), out)
    if rc != 0:
        raise KhError(rc, "kh_plan_gemm16")
    return {"classes": [n for i, n in enumerate(KH_W16_CLASSES) if out[0] >> i & 1], "kblock": int(out[1])}


def plan_gemm16_q8(dim: int, hidden_dim: int, kv_dim: int, vocab_size: int, quant: bool, group_size: int = 64) -> dict:
    """KH_FLAG_GEMM16_Q8 for a geometry (host-only, kh_plan_gemm16_q8): {"classes": the launch classes whose GEMMs of the
    GEMM pass run on the bf16 matrix cores from the int8 image by default - [] for fp32, for a group size other than 64
    and for dims the int8 GEMM prefill does not take -, "kblock": 64}."""
    out = (_i64 * 2)()
    rc = lib().kh_plan_gemm16_q8(dim, hidden_dim, kv_dim, vocab_size, int(quant), group_size, out)
    if rc != 0:
        raise KhError(rc, "kh_plan_gemm16_q8")
    return {"classes": [n for i, n in enumerate(KH_W16_CLASSES) if out[0] >> i & 1], "kblock": int(out[1])}


def plan_q4(dim: int, hidden_dim: int, kv_dim: int, vocab_size: int, n_layers: int, quant: bool,
            group_size: int = 64) -> dict:
    """The 4-bit weight copy of KH_FLAG_Q4 for a geometry (host-only, kh_plan_q4): {"classes": the decode launch classes
    that run on it by default, "bytes": HBM the copy takes (0: not applicable, e.g. fp32)}."""
    out = (_i64 * 2)()
    rc = lib().kh_plan_q4(dim, hidden_dim, kv_dim, vocab_size, n_layers, int(quant), group_size, out)
    if rc != 0:
        raise KhError(rc, "kh_plan_q4")
    return {"classes": [n for i, n in enumerate(KH_Q4_CLASSES) if out[0] >> i & 1], "bytes": int(out[1])}


def plan_attention(head_num: int, kv_mul: int, head_size: int, seq_len: int, pos: int) -> dict:
    """Decode-attention geometry for a cache of seq_len rows at position pos (host-only, kh_plan_attention)."""
    sync_env()
    out = (_i32 * 8)()
    rc = lib().kh_plan_attention(head_num, kv_mul, head_size, seq_len, pos, out)
    if rc != 0:
        raise KhError(rc, "kh_plan_attention")
    return dict(zip(("ns", "ns_g", "stride", "t_long", "group_path", "active_splits", "split_len", "workgroups"),
                    list(out)))


def plan_attention_launch(head_num: int, kv_mul: int, head_size: int, seq_len: int, positions) -> dict:
    """One decode-attention launch over the tokens at `positions` (empty: a device-positioned launch) of the geometry
    of plan_attention (host-only, kh_plan_attention_launch)."""
    sync_env()
    n = len(positions)
    pos = (_i32 * max(n, 1))(*positions)
    out = (_i32 * 6)()
    rc = lib().kh_plan_attention_launch(head_num, kv_mul, head_size, seq_len, pos, n, out)
    if rc != 0:
        raise KhError(rc, "kh_plan_attention_launch")
    return dict(zip(("G", "KVM", "grid", "lds", "head_splits", "group_splits"), list(out)))


def plan_prefill_shape(epi: str, T: int, rows: int, K: int, quant: bool, r2_ok: bool = True) -> dict:
    """Launch plan of one GEMM of a T-token prefill pass (epi: qkv | resid | swiglu); host-only."""
    sync_env()
    out = (_i32 * 7)()
    rc = lib().kh_plan_prefill_shape({"qkv": 0, "resid": 1, "swiglu": 2}[epi], T, rows, K, int(quant),
                                     int(r2_ok), out)
    if rc != 0:
        raise KhError(rc, "kh_plan_prefill_shape")
    return dict(zip(("R", "NT", "ks", "slices", "solo", "kz", "workgroups"), out[:]))
