"""Operator-level Python mirror of the reference's kernel interface
(kuiper/source/op/kernels/kernels_interface.h:6-68) over libkuiper_hip.so.

Arguments are torch tensors living on the GPU (torch is only the owner of device memory and
streams here); every call goes through the C-ABI and launches a hand-written HIP kernel on
torch's current stream.  There is no eager/CPU fallback: a CPU tensor is an error.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _ffi

ROPE_INTERLEAVED, ROPE_HALF = 0, 1


def _p(t: Optional[torch.Tensor], dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("kuiperllama_amd.ops: tensors must be on the GPU (no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError("kuiperllama_amd.ops: tensors must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def add(in1, in2, out):
    _ffi.check(_ffi.lib().kh_add_f32(_p(in1, torch.float32), _p(in2, torch.float32),
                                     _p(out, torch.float32), in1.numel(), _stream()), "kh_add_f32")
    return out


def matmul(x, w, out, scale: float = 1.0):
    K, M = w.shape
    _ffi.check(_ffi.lib().kh_matmul_f32(_p(x, torch.float32), _p(w, torch.float32),
                                        _p(out, torch.float32), M, K, scale, _stream()),
               "kh_matmul_f32")
    return out


def gemm_w16(x, w16, out=None):
    """out[T, M] = x[T, K] @ w16[M, K]^T on the bf16 matrix cores, fp32-accurate (kh_gemm_w16_f32): w16 holds bf16 bits
    (torch.bfloat16, or int16 / uint16 words); M % 16 == 0, K % 32 == 0, T <= 512."""
    T, K = x.shape
    M, K2 = w16.shape
    if K2 != K or w16.element_size() != 2:
        raise ValueError("gemm_w16: w16 must be [M, K] 16-bit words")
    if out is None:
        out = torch.empty((T, M), dtype=torch.float32, device=x.device)
    _ffi.check(_ffi.lib().kh_gemm_w16_f32(_p(x, torch.float32), _p(w16), _p(out, torch.float32), T, M, K,
                                          out.stride(0), _stream()), "kh_gemm_w16_f32")
    return out


def gemm_q8_bf16(x, w8, scales, out=None):
    """out[T, M] = x[T, K] @ (scales * w8)[M, K]^T on the bf16 matrix cores, fp32-accurate (kh_gemm_q8_bf16_f32): w8 is
    int8 [M, K] in groups of 64 columns, scales fp32 [M, K / 64]; M % 16 == 0, K % 64 == 0, T <= 512.  out may be a
    [T, ldy >= M] buffer: columns past M keep their bytes."""
    T, K = x.shape
    M, K2 = w8.shape
    if K2 != K or tuple(scales.shape) != (M, K // 64):
        raise ValueError("gemm_q8_bf16: w8 must be [M, K] int8 and scales [M, K / 64]")
    if out is None:
        out = torch.empty((T, M), dtype=torch.float32, device=x.device)
    _ffi.check(_ffi.lib().kh_gemm_q8_bf16_f32(_p(x, torch.float32), _p(w8, torch.int8), _p(scales, torch.float32),
                                              _p(out, torch.float32), T, M, K, out.stride(0), _stream()),
               "kh_gemm_q8_bf16_f32")
    return out


def matmul_q8(x, w8, scales, group_size: int, out):
    K, M = w8.shape
    _ffi.check(_ffi.lib().kh_matmul_q8(_p(x, torch.float32), _p(w8, torch.int8),
                                       _p(scales, torch.float32), group_size,
                                       _p(out, torch.float32), M, K, _stream()), "kh_matmul_q8")
    return out


def embedding(tokens, w, out):
    V, dim = w.shape
    _ffi.check(_ffi.lib().kh_embedding_f32(_p(tokens, torch.int32), tokens.numel(),
                                           _p(w, torch.float32), _p(out, torch.float32), dim, V,
                                           _stream()), "kh_embedding_f32")
    return out


def embedding_host_tokens(tokens, w, out):
    """EmbeddingKernel as the reference calls it: `tokens` is a HOST int32 array (numpy); the ids
    travel in the kernel arguments, 64 per launch (kh_embedding_f32_host)."""
    import numpy as np
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    _ffi.check(_ffi.lib().kh_embedding_f32_host(t.ctypes.data, t.size, _p(w), _p(out), w.shape[1],
                                                w.shape[0], _stream()), "kh_embedding_f32_host")


def swiglu(a, b, out):
    _ffi.check(_ffi.lib().kh_swiglu_f32(_p(a, torch.float32), _p(b, torch.float32),
                                        _p(out, torch.float32), a.numel(), _stream()),
               "kh_swiglu_f32")
    return out


def rmsnorm(x, w, out, eps: float):
    _ffi.check(_ffi.lib().kh_rmsnorm_f32(_p(x, torch.float32), _p(w, torch.float32),
                                         _p(out, torch.float32), x.numel(), eps, _stream()),
               "kh_rmsnorm_f32")
    return out


def rope(q, k, pos, sin_cache, cos_cache, head_size: int, mode: int):
    """pos: python int, or a 1-element int32 GPU tensor (graph-capturable form)."""
    d_pos, ipos = (None, int(pos)) if not torch.is_tensor(pos) else (_p(pos, torch.int32), 0)
    _ffi.check(_ffi.lib().kh_rope_f32(q.numel(), k.numel(), head_size, _p(q, torch.float32),
                                      _p(k, torch.float32), d_pos, ipos,
                                      _p(sin_cache, torch.float32), _p(cos_cache, torch.float32),
                                      mode, _stream()), "kh_rope_f32")
    return q, k


def sincos_cache(head_size: int, seq_len: int, theta: float, sin_cache, cos_cache):
    _ffi.check(_ffi.lib().kh_sincos_cache_f32(head_size, seq_len, theta,
                                              _p(sin_cache, torch.float32),
                                              _p(cos_cache, torch.float32), _stream()),
               "kh_sincos_cache_f32")
    return sin_cache, cos_cache


def mha(pos, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, mha_out, q, score,
        kcache, vcache):
    d_pos, ipos = (None, int(pos)) if not torch.is_tensor(pos) else (_p(pos, torch.int32), 0)
    _ffi.check(_ffi.lib().kh_mha_f32(d_pos, ipos, head_num, layer_index, seq_len, kv_dim, kv_mul,
                                     head_size, _p(mha_out, torch.float32), _p(q, torch.float32),
                                     _p(score, torch.float32) if score is not None else None,
                                     _p(kcache, torch.float32),
                                     _p(vcache, torch.float32), _stream()), "kh_mha_f32")
    return mha_out


def mha_prefill(pos0, n_tokens, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, mha_out, q,
                kcache, vcache):
    """Causal attention of n_tokens consecutive queries (rows of q) on the matrix cores."""
    _ffi.sync_env()  # KH_PG_ATTN_QT
    _ffi.check(_ffi.lib().kh_mha_prefill_f32(
        int(pos0), int(n_tokens), head_num, layer_index, seq_len, kv_dim, kv_mul, head_size,
        _p(mha_out, torch.float32), _p(q, torch.float32), _p(kcache, torch.float32),
        _p(vcache, torch.float32), _stream()), "kh_mha_prefill_f32")
    return mha_out


PA_TILED_F32, PA_TILED_Q8, PA_ROWS = 0, 1, 2  # output layouts of the prompt-slice attention (csrc/kh_pattn.h)


def mha_prefill_layout(pos0, n_tokens, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, layout, tcap,
                       mha_out, q, kcache, vcache):
    """mha_prefill in the output layout of a model pass (kh_mha_prefill_layout_f32): PA_TILED_F32 / PA_TILED_Q8 write
    the tiled slab of dim * tcap floats the wo GEMM reads, PA_ROWS row-major [n_tokens][dim]."""
    _ffi.sync_env()  # KH_PG_ATTN_QT
    _ffi.check(_ffi.lib().kh_mha_prefill_layout_f32(
        int(pos0), int(n_tokens), head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, int(layout), int(tcap),
        _p(mha_out, torch.float32), _p(q, torch.float32), _p(kcache, torch.float32),
        _p(vcache, torch.float32), _stream()), "kh_mha_prefill_layout_f32")
    return mha_out


def mha_prefill_tiles(tiles, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, layout, tcap, mha_out, q,
                      kcache, vcache):
    """The slot prefill's attention (kh_mha_prefill_tiles_f32).  tiles: host int32 array [5][n_tiles] - pos0, nvalid,
    base, pfx_len, pfx_row0 per 16-token query tile; q is [16 * n_tiles][dim]."""
    import numpy as np
    t = np.ascontiguousarray(tiles, dtype=np.int32)
    if t.ndim != 2 or t.shape[0] != 5:
        raise ValueError("mha_prefill_tiles: tiles must be [5][n_tiles]")
    _ffi.check(_ffi.lib().kh_mha_prefill_tiles_f32(
        t.shape[1], t.ctypes.data, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, int(layout), int(tcap),
        _p(mha_out, torch.float32), _p(q, torch.float32), _p(kcache, torch.float32),
        _p(vcache, torch.float32), _stream()), "kh_mha_prefill_tiles_f32")
    return mha_out


def mha_decode_workspace(head_num: int, head_size: int, seq_len: int, device):
    """Zeroed workspace tensor for mha_decode (None when no time split is needed)."""
    _ffi.sync_env()  # KH_ATTN_TLONG
    n = int(_ffi.lib().kh_mha_decode_workspace_bytes(head_num, head_size, seq_len))
    if n < 0:
        _ffi.check(n, "kh_mha_decode_workspace_bytes")
    return torch.zeros(n, dtype=torch.uint8, device=device) if n else None


def mha_decode(pos, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size, mha_out, q, kcache,
               vcache, workspace):
    d_pos, ipos = (None, int(pos)) if not torch.is_tensor(pos) else (_p(pos, torch.int32), 0)
    _ffi.check(_ffi.lib().kh_mha_decode_f32(
        d_pos, ipos, head_num, layer_index, seq_len, kv_dim, kv_mul, head_size,
        _p(mha_out, torch.float32), _p(q, torch.float32), _p(kcache, torch.float32),
        _p(vcache, torch.float32), _p(workspace) if workspace is not None else None,
        workspace.numel() if workspace is not None else 0, _stream()), "kh_mha_decode_f32")
    return mha_out


def argmax(logits, out_index):
    _ffi.check(_ffi.lib().kh_argmax_f32(_p(logits, torch.float32), logits.numel(),
                                        _p(out_index, torch.int32), _stream()), "kh_argmax_f32")
    return out_index


def argmax_rows(logits, n: int, out_index):
    """out_index[r] = first maximum of logits[r, :n] for every row of the contiguous 2-d fp32 tensor `logits`, whose
    row stride - logits.shape[1] - is at least n and a multiple of 4 (kh_argmax_rows_f32; asynchronous)."""
    rows, stride = logits.shape
    assert out_index.numel() >= rows
    _ffi.check(_ffi.lib().kh_argmax_rows_f32(_p(logits, torch.float32), int(n), int(stride), int(rows),
                                             _p(out_index, torch.int32), _stream()), "kh_argmax_rows_f32")
    return out_index


def argmax_host(logits) -> int:
    import ctypes as C
    r = C.c_int64(-1)
    _ffi.check(_ffi.lib().kh_argmax_f32_host(_p(logits, torch.float32), logits.numel(),
                                             C.byref(r), _stream()), "kh_argmax_f32_host")
    return int(r.value)


def _sampling(params):
    if isinstance(params, _ffi.Sampling):
        return params
    return _ffi.sampling(**params)


def sample(logits, out, params, counter0: int = 0):
    """out.numel() seeded draws from one logit vector (kh_sample_f32): draw d uses counter counter0 + d.
    params: an _ffi.Sampling or a dict with temperature / top_k / top_p / seed (temperature <= 0: argmax)."""
    p = _sampling(params)
    _ffi.check(_ffi.lib().kh_sample_f32(_p(logits, torch.float32), logits.numel(), p, int(counter0), out.numel(),
                                        _p(out, torch.int32), _stream()), "kh_sample_f32")
    return out


def sample_host(logits, params, counter: int = 0) -> int:
    """One draw with the index returned to the host (kh_sample_f32_host; synchronises the stream)."""
    import ctypes as C
    r = C.c_int64(-1)
    _ffi.check(_ffi.lib().kh_sample_f32_host(_p(logits, torch.float32), logits.numel(), _sampling(params),
                                             int(counter), C.byref(r), _stream()), "kh_sample_f32_host")
    return int(r.value)


def logit_process_workspace(n: int, device):
    """Zeroed counter table for logit_process (zeroed once: the kernel leaves it zero)."""
    nb = int(_ffi.lib().kh_logit_process_workspace_bytes(int(n)))
    if nb < 0:
        _ffi.check(nb, "kh_logit_process_workspace_bytes")
    return torch.zeros(nb // 4, dtype=torch.int32, device=device)


def logit_process(logits, tokens, pos, penalties=None, bias_ids=None, bias=None, workspace=None):
    """Penalties and logit bias in place on `logits` (kh_logit_process_f32).  tokens: int32 GPU tensor, the token fed
    at every position up to `pos` (a python int, or a 1-element int32 GPU tensor: graph-capturable form); penalties: an
    _ffi.Penalties or a dict with repetition / presence / frequency / last_n; bias_ids / bias: int32 / float32 GPU
    tensors of equal length; workspace: logit_process_workspace(logits.numel())."""
    p = penalties if isinstance(penalties, _ffi.Penalties) or penalties is None else _ffi.penalties(**penalties)
    d_pos, ipos = (None, int(pos)) if not torch.is_tensor(pos) else (_p(pos, torch.int32), 0)
    nb = 0 if bias_ids is None else bias_ids.numel()
    if nb and (bias is None or bias.numel() != nb):
        raise ValueError("bias_ids and bias must have the same length")
    _ffi.check(_ffi.lib().kh_logit_process_f32(_p(logits, torch.float32), logits.numel(), _p(tokens, torch.int32),
                                               d_pos, ipos, p, _p(bias_ids, torch.int32) if nb else None,
                                               _p(bias, torch.float32) if nb else None, nb,
                                               _p(workspace, torch.int32), _stream()), "kh_logit_process_f32")
    return logits


def token_mask(logits, mask):
    """logits[v] = -inf in place wherever bit v & 31 of word v >> 5 of `mask` is clear (kh_token_mask_f32).  logits:
    float32 GPU tensor [V]; mask: int32 GPU tensor of at least ceil(V / 32) words (the bits, whatever the sign); bits
    past V are ignored."""
    n = logits.numel()
    if mask.numel() < (n + 31) // 32:
        raise ValueError("mask needs ceil(V / 32) words")
    _ffi.check(_ffi.lib().kh_token_mask_f32(_p(logits, torch.float32), n, _p(mask, torch.int32), _stream()),
               "kh_token_mask_f32")
    return logits


def logprobs(logits, ids, top_n: int = 0) -> dict:
    """Log-probability of ids[r] under the softmax of logits[r] and the top_n alternatives of every row
    (kh_logprobs_f32).  logits: float32 GPU tensor [V] or [rows, V]; ids: int32 GPU tensor [rows] (an id outside [0, V)
    reports NaN); 0 <= top_n <= 20.  Returns {"lse": [rows], "logprob": [rows], "top_ids": [rows, top_n],
    "top_logprobs": [rows, top_n]} as GPU tensors, in the sampler's order (logit descending, index ascending)."""
    rows = 1 if logits.dim() == 1 else logits.shape[0]
    V = logits.shape[-1]
    if ids.numel() != rows:
        raise ValueError("one id per row of logits")
    dev = logits.device
    out = {"lse": torch.empty(rows, dtype=torch.float32, device=dev),
           "logprob": torch.empty(rows, dtype=torch.float32, device=dev),
           "top_ids": torch.empty((rows, max(int(top_n), 0)), dtype=torch.int32, device=dev),
           "top_logprobs": torch.empty((rows, max(int(top_n), 0)), dtype=torch.float32, device=dev)}
    _ffi.check(_ffi.lib().kh_logprobs_f32(_p(logits, torch.float32), V, rows, _p(ids, torch.int32), int(top_n),
                                          _p(out["lse"]), _p(out["logprob"]), _p(out["top_ids"]),
                                          _p(out["top_logprobs"]), _stream()), "kh_logprobs_f32")
    return out


def softmax_(x):
    _ffi.check(_ffi.lib().kh_softmax_f32(_p(x, torch.float32), x.numel(), _stream()),
               "kh_softmax_f32")
    return x


def scale_(scale: float, x):
    _ffi.check(_ffi.lib().kh_scale_f32(scale, _p(x, torch.float32), x.numel(), _stream()),
               "kh_scale_f32")
    return x


def scale_sum(value, scale, out, pos: int, size: int, stride: int):
    _ffi.check(_ffi.lib().kh_scale_sum_f32(_p(value, torch.float32), _p(scale, torch.float32),
                                           _p(out, torch.float32), pos, size, stride, _stream()),
               "kh_scale_sum_f32")
    return out
