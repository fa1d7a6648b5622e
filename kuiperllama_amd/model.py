"""Model-level Python mirror of model::LLama2Model / Qwen2Model for the decode path
(kuiper/include/model/model.h:20-56, kuiper/source/model/llama3.cpp:107-167, 642-650,
733-745; demo/main.cpp:5-47) over libkuiper_hip.so.  All compute is in the HIP library.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ffi, binfmt
from ._ffi import KH_EXEC_FUSED, KH_EXEC_GRAPH, KH_EXEC_UNFUSED  # noqa: F401

EXEC = {"graph": KH_EXEC_GRAPH, "fused": KH_EXEC_FUSED, "unfused": KH_EXEC_UNFUSED}



def _opts(spec: binfmt.ModelSpec, max_seq_len: int, device: int, flags: int = 0) -> _ffi.ModelOpts:
    return _ffi.ModelOpts(spec.family, int(spec.quant), spec.rope_mode, spec.rope_theta,
                          spec.rms_eps, max_seq_len, device, flags)


def _i32_array(tokens):
    return (C.c_int32 * max(len(tokens), 1))(*[int(t) for t in tokens])


def _sampling_array(samplings, n: int, what: str):
    """[n] kh_sampling from a list of None (greedy) | dict of _ffi.sampling()'s fields | _ffi.Sampling; None stays None"""
    if samplings is None:
        return None
    samplings = list(samplings)
    if len(samplings) != n:
        raise ValueError(f"{what}: {len(samplings)} sampling entries for {n} sequences")
    arr = (_ffi.Sampling * max(n, 1))()
    for i, sp in enumerate(samplings):
        v = _ffi.sampling() if sp is None else sp if isinstance(sp, _ffi.Sampling) else _ffi.sampling(**sp)
        arr[i] = _ffi.Sampling(v.temperature, v.top_k, v.top_p, v.seed)
    return arr


def plan_seq_slots(cache_len: int, n_slots: int) -> int:
    """slot_len of a cache of cache_len rows cut into n_slots sequence slots (kh_plan_seq_slots; host only)."""
    out = C.c_int32(0)
    _ffi.check(_ffi.lib().kh_plan_seq_slots(int(cache_len), int(n_slots), C.byref(out)), "kh_plan_seq_slots")
    return int(out.value)


def plan_seq_slots_var(cache_len: int, lens: Sequence[int]) -> List[int]:
    """First row of every slot of a cache of cache_len rows cut into slots of lens[s] rows (kh_plan_seq_slots_var;
    host only)."""
    out = (C.c_int32 * max(len(lens), 1))()
    _ffi.check(_ffi.lib().kh_plan_seq_slots_var(int(cache_len), len(lens), _i32_array(lens), out),
               "kh_plan_seq_slots_var")
    return [int(out[s]) for s in range(len(lens))]


def plan_shared_layout(cache_len: int, n_seq: int, n_prefix: int, total_steps) -> List[int]:
    """Slot lengths for n_seq sequences of which slot 0 holds a prompt prefix of n_prefix positions and the others read
    it from there (seq_share): the parent owns all of its total_steps positions, a sharer only those from n_prefix on,
    every slot at least 8 rows.  total_steps: one int for all or one per sequence.  Raises ValueError where the
    lengths do not fit cache_len rows (host only)."""
    n_seq, n_prefix = int(n_seq), int(n_prefix)
    totals = [int(total_steps)] * n_seq if isinstance(total_steps, (int, np.integer)) else [int(t) for t in total_steps]
    if n_seq < 1 or len(totals) != n_seq or n_prefix < 0 or any(t < n_prefix for t in totals):
        raise ValueError(f"plan_shared_layout: {n_seq} sequences, prefix {n_prefix}, totals {totals}")
    lens = [max(8, totals[0])] + [max(8, t - n_prefix) for t in totals[1:]]
    if n_seq > 64 or sum(lens) > int(cache_len):
        raise ValueError(f"plan_shared_layout: {sum(lens)} rows in {n_seq} slots do not fit a cache of {cache_len}")
    return lens


def _seq_opts(n: int, sp, penalties, logit_bias, logprobs, what: str):
    """kh_seq_opts of an _ex call and the arrays it points to (keep both alive across the call): penalties = None | [n]
    of None | dict of set_penalties()'s keys | _ffi.Penalties; logit_bias = None | [n] of None | {id: value};
    logprobs = None | top_n.  Wrong lengths are refused here, before the library is called."""
    keep = [sp]
    o = _ffi.SeqOpts()
    o.samplings = sp if sp is not None else None
    if penalties is not None:
        penalties = list(penalties)
        if len(penalties) != n:
            raise ValueError(f"{what}: {len(penalties)} penalty entries for {n} sequences")
        pa = (_ffi.Penalties * max(n, 1))()
        for i, p in enumerate(penalties):
            v = _ffi.penalties() if p is None else p if isinstance(p, _ffi.Penalties) else _ffi.penalties(**p)
            pa[i] = _ffi.Penalties(v.repetition, v.presence, v.frequency, v.last_n)
        keep.append(pa)
        o.penalties = pa
    if logit_bias is not None:
        logit_bias = list(logit_bias)
        if len(logit_bias) != n:
            raise ValueError(f"{what}: {len(logit_bias)} logit-bias entries for {n} sequences")
        items = [sorted((int(k), float(v)) for k, v in (b or {}).items()) for b in logit_bias]
        nb = _i32_array([len(it) for it in items])
        flat = [kv for it in items for kv in it]
        ids = _i32_array([k for k, _ in flat])
        vals = (C.c_float * max(len(flat), 1))(*[v for _, v in flat])
        keep += [nb, ids, vals]
        o.n_bias, o.bias_ids, o.bias = nb, ids, vals
    o.logprobs_top_n = -1 if logprobs is None else int(logprobs)
    return o, keep


def seq_rank(lp_rows, first: Sequence[int], n_words: Sequence[int]) -> Tuple[List[int], np.ndarray]:
    """The ranking of best-of-n (kh_seq_rank; host only): lp_rows[s] holds sequence s's per-position log-probs, of which
    positions [first[s], n_words[s]) count.  Returns (order, mean): mean[s] the float64 mean of those log-probs (NaN
    where there are none), order the sequences by it - descending, ties by index, NaN last."""
    rows = [np.asarray(r, np.float32).ravel() for r in lp_rows]
    n = len(rows)
    first, n_words = list(first), list(n_words)
    if len(first) != n or len(n_words) != n:
        raise ValueError(f"seq_rank: {n} rows, {len(first)} first positions, {len(n_words)} word counts")
    stride = max([len(r) for r in rows] + [1])
    lp = np.full((max(n, 1), stride), np.nan, np.float32)
    for s, r in enumerate(rows):
        if int(n_words[s]) > len(r):
            raise ValueError(f"seq_rank: row {s} holds {len(r)} log-probs, n_words says {n_words[s]}")
        lp[s, :len(r)] = r
    order = (C.c_int32 * max(n, 1))()
    mean = np.empty(max(n, 1), np.float64)
    _ffi.check(_ffi.lib().kh_seq_rank(n, lp.ctypes.data_as(C.POINTER(C.c_float)), stride, _i32_array(first),
                                      _i32_array(n_words), order, mean.ctypes.data_as(C.POINTER(C.c_double))),
               "kh_seq_rank")
    return list(order[:n]), mean[:n]


def plan_seq_batch(first_pos: Sequence[int], total_steps: Sequence[int], width: int,
                   wide: bool = False) -> List[List[int]]:
    """The passes generate_batch runs while no sequence stops early (kh_plan_seq_batch; host only): per pass the
    sequences in its lanes.  first_pos[s] = len(prompt s) - 1, the first position a pass feeds.  wide: the passes of
    generate_batch(gemm=True), width up to 64 (kh_plan_seq_batch_wide)."""
    first_pos, total_steps = list(first_pos), list(total_steps)
    if len(first_pos) != len(total_steps):
        raise ValueError(f"plan_seq_batch: {len(first_pos)} positions for {len(total_steps)} totals")
    n, L = C.c_int32(0), _ffi.lib()
    name = "kh_plan_seq_batch_wide" if wide else "kh_plan_seq_batch"
    plan = getattr(L, name)
    rc = plan(len(first_pos), int(width), _i32_array(first_pos), _i32_array(total_steps), None, 0, C.byref(n))
    if rc not in (0, _ffi.KH_ERR_RANGE):
        raise _ffi.KhError(rc, name)
    out = (C.c_int32 * max(n.value * int(width), 1))()
    _ffi.check(plan(len(first_pos), int(width), _i32_array(first_pos), _i32_array(total_steps), out, n.value,
                    C.byref(n)), name)
    return [[int(x) for x in out[p * width:(p + 1) * width] if x >= 0] for p in range(n.value)]


def plan_seq_prefill_gemm(n_tokens: Sequence[int]) -> List[Tuple[int, int, int, int]]:
    """The runs seq_prefill_many's passes are made of (kh_plan_seq_prefill_gemm; host only): per placed run (pass,
    segment, first token offset, count).  A pass has 32 token tiles of 16; a segment that fits in what is left of the
    pass is placed whole, else its first 16 x free tokens fill the pass and the rest continues in the next."""
    n_tokens = [int(n) for n in n_tokens]
    n, L = C.c_int32(0), _ffi.lib()
    rc = L.kh_plan_seq_prefill_gemm(len(n_tokens), _i32_array(n_tokens), None, 0, C.byref(n), None)
    if rc not in (0, _ffi.KH_ERR_RANGE):
        raise _ffi.KhError(rc, "kh_plan_seq_prefill_gemm")
    out = (C.c_int32 * max(4 * n.value, 1))()
    _ffi.check(L.kh_plan_seq_prefill_gemm(len(n_tokens), _i32_array(n_tokens), out, n.value, C.byref(n), None),
               "kh_plan_seq_prefill_gemm")
    return [tuple(int(x) for x in out[4 * r:4 * r + 4]) for r in range(n.value)]


def lookup_draft(seq: Sequence[int], hint: Optional[Sequence[int]] = None, ngram_max: int = 4, ngram_min: int = 1,
                 cap: int = 7) -> List[int]:
    """The drafter of generate_lookup (kh_lookup_draft; host only, no device): up to `cap` tokens that followed the
    longest suffix of `seq` (ngram_max .. ngram_min tokens) at its earliest occurrence in `hint`, else at its most
    recent earlier occurrence in `seq` itself; [] when nothing matches."""
    seq, hint = list(seq), list(hint or [])
    out = (C.c_int32 * max(int(cap), 1))()
    n = _ffi.lib().kh_lookup_draft(_i32_array(seq), len(seq), _i32_array(hint), len(hint), int(ngram_max),
                                   int(ngram_min), out, int(cap))
    if n < 0:
        raise _ffi.KhError(n, "kh_lookup_draft")
    return list(out[:n])


def lookup_draft_fsm(automaton, state: int, seq: Sequence[int], hint: Optional[Sequence[int]] = None,
                     ngram_max: int = 4, ngram_min: int = 1, cap: int = 7) -> Tuple[List[int], int]:
    """The drafter of generate_lookup(constrained=True) (kh_lookup_draft_fsm; host only, no device): from `state` of
    the constraint.TokenAutomaton, the tokens of single-edge rows - forced, whatever the model says - and, where a row
    holds more, lookup_draft's proposal cut to what the automaton can follow.  Returns (tokens, n_forced)."""
    seq, hint = list(seq), list(hint or [])
    a, keep = _ffi.fsm(automaton.start, automaton.row_ptr, automaton.tokens, automaton.next)
    out = (C.c_int32 * max(int(cap), 1))()
    forced = C.c_int32(0)
    n = _ffi.lib().kh_lookup_draft_fsm(C.byref(a), int(state), _i32_array(seq), len(seq), _i32_array(hint), len(hint),
                                       int(ngram_max), int(ngram_min), out, int(cap), C.byref(forced))
    del keep
    if n < 0:
        raise _ffi.KhError(n, "kh_lookup_draft_fsm")
    return list(out[:n]), int(forced.value)


class KuiperModel:
    """Owns a kh_model handle.  Construct with one of the from_* classmethods."""

    def __init__(self, handle: int, spec: binfmt.ModelSpec, keepalive=None):
        self._h = C.c_void_p(handle)
        self.spec = spec
        self._keep = keepalive
        self._seq_slots = 1      # seq_slots(): the partition best_of() widens when it is too small
        self._seq_top_n = None   # the logprobs= of the last seq_step / generate_batch that had one: seq_logprobs' width
        cfg = _ffi.Config()
        _ffi.check(_ffi.lib().kh_model_get_config(self._h, C.byref(cfg)), "kh_model_get_config")
        self.cfg = cfg

    # ---- construction ------------------------------------------------------------------
    @classmethod
    def from_file(cls, path: str, spec: binfmt.ModelSpec, max_seq_len: int = 0,
                  device: int = 0, flags: int = 0) -> "KuiperModel":
        _ffi.sync_env()
        h = C.c_void_p()
        o = _opts(spec, max_seq_len, device, flags)
        _ffi.check(_ffi.lib().kh_model_create_from_file(path.encode(), C.byref(o), C.byref(h)),
                   "kh_model_create_from_file")
        return cls(h.value, spec)

    @classmethod
    def from_host_image(cls, image: np.ndarray, spec: binfmt.ModelSpec, max_seq_len: int = 0,
                        device: int = 0, flags: int = 0) -> "KuiperModel":
        assert image.dtype == np.uint8 and image.flags["C_CONTIGUOUS"]
        _ffi.sync_env()
        h = C.c_void_p()
        o = _opts(spec, max_seq_len, device, flags)
        _ffi.check(_ffi.lib().kh_model_create_from_host_image(image.ctypes.data, image.size,
                                                              C.byref(o), C.byref(h)),
                   "kh_model_create_from_host_image")
        return cls(h.value, spec)

    @classmethod
    def from_device_image(cls, image: torch.Tensor, spec: binfmt.ModelSpec, max_seq_len: int = 0,
                          device: int = 0, flags: int = 0) -> "KuiperModel":
        """image: uint8 GPU tensor with the .bin bytes (header included), resident on `device`.
        The library needs the bytes after the 28 / 32-byte header at a 16-byte aligned address:
        they are used in place when they already are, otherwise copied once into an aligned
        tensor (which transiently doubles the weight memory).  Not owned by the library."""
        assert image.is_cuda and image.dtype == torch.uint8
        if image.device.index != device:
            raise ValueError(f"image lives on cuda:{image.device.index} but the model is created on "
                             f"device {device}: kernels would dereference another GPU's pointers")
        hb = spec.header_bytes()
        header = np.frombuffer(image[:32].cpu().numpy().tobytes(), dtype=np.int32).copy()
        if (image.data_ptr() + hb) % 16 == 0:
            weights = image[hb:]
            keep = image
        else:
            weights = torch.empty(image.numel() - hb, dtype=torch.uint8, device=image.device)
            weights.copy_(image[hb:])
            keep = weights
        torch.cuda.synchronize()
        _ffi.sync_env()
        h = C.c_void_p()
        o = _opts(spec, max_seq_len, device, flags)
        hdr = (C.c_int32 * 8)(*header.tolist()[:8])
        _ffi.check(_ffi.lib().kh_model_create_from_device_weights(hdr, weights.data_ptr(),
                                                                  weights.numel(), C.byref(o),
                                                                  C.byref(h)),
                   "kh_model_create_from_device_weights")
        return cls(h.value, spec, keepalive=keep)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _ffi.lib().kh_model_destroy(self._h)
            self._h = C.c_void_p()
        self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- Model::predict / forward ----------------------------------------------------------
    def predict(self, token: int, pos: int, is_prompt: bool = False, exec: str = "fused") -> int:
        nxt = C.c_int32(-1)
        _ffi.check(_ffi.lib().kh_model_predict(self._h, token, pos, int(is_prompt), EXEC[exec],
                                               C.byref(nxt)), "kh_model_predict")
        return int(nxt.value)

    def set_sampling(self, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0) -> None:
        """Sampler of predict / generate (kh_model_set_sampling): temperature <= 0 is greedy (the default), top_k 0
        and top_p 1 are off; the draw at position p uses Philox counter p, so tokens do not depend on the exec mode
        or on how the steps were run."""
        _ffi.check(_ffi.lib().kh_model_set_sampling(self._h, _ffi.sampling(temperature, top_k, top_p, seed)),
                   "kh_model_set_sampling")

    @property
    def sampling(self) -> dict:
        s = _ffi.Sampling()
        _ffi.check(_ffi.lib().kh_model_get_sampling(self._h, C.byref(s)), "kh_model_get_sampling")
        return s.as_dict()

    def set_penalties(self, repetition: float = 1.0, presence: float = 0.0, frequency: float = 0.0,
                      last_n: int = 0) -> None:
        """Penalties of predict / generate over the last_n fed tokens (0: all of them), prompt included
        (kh_model_set_penalties): l = l / repetition (l > 0) or l * repetition, then l -= count * frequency + presence,
        for every token in the window, ahead of the greedy or sampled pick.  The defaults turn them off."""
        _ffi.check(_ffi.lib().kh_model_set_penalties(self._h, _ffi.penalties(repetition, presence, frequency, last_n)),
                   "kh_model_set_penalties")

    @property
    def penalties(self) -> dict:
        p = _ffi.Penalties()
        _ffi.check(_ffi.lib().kh_model_get_penalties(self._h, C.byref(p)), "kh_model_get_penalties")
        return p.as_dict()

    def set_logit_bias(self, bias: Optional[dict] = None) -> None:
        """{token id: value} added to the logits after the penalties (kh_model_set_logit_bias); -inf bans a token,
        None or {} clears the list."""
        items = sorted((int(k), float(v)) for k, v in (bias or {}).items())
        ids = (C.c_int32 * max(len(items), 1))(*[k for k, _ in items])
        vals = (C.c_float * max(len(items), 1))(*[v for _, v in items])
        _ffi.check(_ffi.lib().kh_model_set_logit_bias(self._h, ids, vals, len(items)), "kh_model_set_logit_bias")

    def set_logprobs(self, top_n: Optional[int] = None) -> None:
        """Per-token log-probs of predict / generate (kh_model_set_logprobs): None turns them off (the default), 0
        records the picked token's log-prob, 1 .. 20 also that many top alternatives.  No token changes."""
        _ffi.check(_ffi.lib().kh_model_set_logprobs(self._h, -1 if top_n is None else int(top_n)),
                   "kh_model_set_logprobs")

    @property
    def logprobs_setting(self) -> Optional[int]:
        n = C.c_int32(-1)
        _ffi.check(_ffi.lib().kh_model_get_logprobs_setting(self._h, C.byref(n)), "kh_model_get_logprobs_setting")
        return None if n.value < 0 else int(n.value)

    def logprobs(self, pos0: int, n: int) -> dict:
        """Records of positions [pos0, pos0 + n) (kh_model_get_logprobs): {"token": [n], "logprob": [n], "top_ids":
        [n, top_n], "top_logprobs": [n, top_n]} with top_n the current setting.  A position that was fed but not
        sampled holds token -1, ids -1 and NaN."""
        w = self.logprobs_setting or 0
        out = {"token": np.empty(max(n, 0), np.int32), "logprob": np.empty(max(n, 0), np.float32),
               "top_ids": np.empty((max(n, 0), w), np.int32), "top_logprobs": np.empty((max(n, 0), w), np.float32)}
        _ffi.check(_ffi.lib().kh_model_get_logprobs(self._h, int(pos0), int(n), out["token"].ctypes.data,
                                                    out["logprob"].ctypes.data, out["top_ids"].ctypes.data,
                                                    out["top_logprobs"].ctypes.data), "kh_model_get_logprobs")
        return out

    def set_constraint(self, automaton=None) -> None:
        """Constrained decoding (kh_model_set_constraint): a constraint.TokenAutomaton - every sampled position of
        predict / generate picks among the tokens its state allows and moves the state along the pick, inside the
        graph loop.  None turns it off (the default).  The library copies the automaton."""
        if automaton is None:
            _ffi.check(_ffi.lib().kh_model_set_constraint(self._h, None), "kh_model_set_constraint")
            return
        a, keep = _ffi.fsm(automaton.start, automaton.row_ptr, automaton.tokens, automaton.next)
        _ffi.check(_ffi.lib().kh_model_set_constraint(self._h, C.byref(a)), "kh_model_set_constraint")
        del keep

    @property
    def constraint_state(self) -> int:
        """The automaton state behind the last sampled step (kh_model_get_constraint_state; synchronises)."""
        s = C.c_int32(-1)
        _ffi.check(_ffi.lib().kh_model_get_constraint_state(self._h, C.byref(s)), "kh_model_get_constraint_state")
        return int(s.value)

    @constraint_state.setter
    def constraint_state(self, state: int) -> None:
        _ffi.check(_ffi.lib().kh_model_set_constraint_state(self._h, int(state)), "kh_model_set_constraint_state")

    def logits(self) -> np.ndarray:
        out = np.empty(self.cfg.vocab_size, np.float32)
        _ffi.check(_ffi.lib().kh_model_get_logits(self._h, out.ctypes.data), "kh_model_get_logits")
        return out

    def cls_screen_info(self) -> dict:
        """The screened classifier of the greedy generate loop (kh_model_cls_screen_info): whether it is on, its
        creation-time self-test, the HBM bytes and creation time of the bf16 copy, and counters since creation."""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().kh_model_cls_screen_info(self._h, out), "kh_model_cls_screen_info")
        keys = ("on", "selftest", "bytes", "build_us", "steps", "candidates", "overflow_steps", "capacity")
        return dict(zip(keys, (int(v) for v in out)))

    def w16_info(self) -> dict:
        """The 16-bit weight copy of _ffi.KH_FLAG_W16 (kh_model_w16_info): state (0 off or not applicable, 1 on, -1 some
        matrix is not bf16-exact, -2 the creation-time self-check failed), the copy's HBM bytes and build time, the
        decode launch classes that stream it, and the first inexact tensor (7 * layer + index into wq, wk, wv, wo, w1,
        w2, w3; 7 * n_layers: the classifier matrix; -1: none)."""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().kh_model_w16_info(self._h, out), "kh_model_w16_info")
        return {"state": int(out[0]), "bytes": int(out[1]), "build_us": int(out[2]),
                "classes": [n for i, n in enumerate(_ffi.KH_W16_CLASSES) if out[3] >> i & 1],
                "first_inexact": int(out[4])}

    def q4_info(self) -> dict:
        """The 4-bit weight copy of _ffi.KH_FLAG_Q4 (kh_model_q4_info): state (0 off or not applicable, 1 on, -1 some
        int8 value lies outside [-8, 7], -2 the creation-time self-check failed), the copy's HBM bytes and build time,
        the decode launch classes that stream it, and the first inexact tensor (7 * layer + index into wq, wk, wv, wo,
        w1, w2, w3; 7 * n_layers: wcls; -1: none)."""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().kh_model_q4_info(self._h, out), "kh_model_q4_info")
        return {"state": int(out[0]), "bytes": int(out[1]), "build_us": int(out[2]),
                "classes": [n for i, n in enumerate(_ffi.KH_Q4_CLASSES) if out[3] >> i & 1],
                "first_inexact": int(out[4])}

    def q4_pass_info(self) -> dict:
        """The B-token passes of a KH_FLAG_Q4 model (kh_model_q4_info, slot 5): {"classes": the launch classes whose
        passes - prefill, score, verify / generate_lookup, seq_* and generate_batch* - stream the 4-bit copy}.  The
        mask is the hook KH_Q4_PASS's at creation, whatever q4_info()["classes"] says (the copy holds every matrix);
        [] when the passes stream the int8 matrices, and always when the copy is not live."""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().kh_model_q4_info(self._h, out), "kh_model_q4_info")
        return {"classes": [n for i, n in enumerate(_ffi.KH_Q4_CLASSES) if out[5] >> i & 1]}

    def gemm16_info(self) -> dict:
        """_ffi.KH_FLAG_GEMM16 on this model (kh_model_gemm16_info): {"on": some launch class of the GEMM pass runs on
        the bf16 matrix cores, "classes": those classes, "reason": why the flag does nothing (one of
        _ffi.KH_GEMM16_REASONS; "on" where it does), "plan": the classes kh_plan_gemm16 adopts for the geometry}."""
        out = (_ffi._i64 * 8)()
        _ffi.check(_ffi.lib().kh_model_gemm16_info(self._h, out), "kh_model_gemm16_info")
        return {"on": bool(out[0]),
                "classes": [n for i, n in enumerate(_ffi.KH_W16_CLASSES) if out[1] >> i & 1],
                "reason": _ffi.KH_GEMM16_REASONS[out[2]],
                "plan": [n for i, n in enumerate(_ffi.KH_W16_CLASSES) if out[3] >> i & 1]}

    def gemm16_q8_info(self) -> dict:
        """_ffi.KH_FLAG_GEMM16_Q8 on this model (kh_model_gemm16_q8_info): {"on": some launch class of the GEMM pass runs
        on the bf16 matrix cores from the int8 image, "classes": those classes, "reason": why the flag does nothing (one
        of _ffi.KH_GEMM16_Q8_REASONS; "on" where it does), "plan": the classes kh_plan_gemm16_q8 adopts for the geometry}."""
        out = (_ffi._i64 * 8)()
        _ffi.check(_ffi.lib().kh_model_gemm16_q8_info(self._h, out), "kh_model_gemm16_q8_info")
        return {"on": bool(out[0]),
                "classes": [n for i, n in enumerate(_ffi.KH_W16_CLASSES) if out[1] >> i & 1],
                "reason": _ffi.KH_GEMM16_Q8_REASONS[out[2]],
                "plan": [n for i, n in enumerate(_ffi.KH_W16_CLASSES) if out[3] >> i & 1]}

    def w16_pass_info(self) -> dict:
        """The B-token passes of a KH_FLAG_W16 model (kh_model_w16_info, slot 5): {"classes": the launch classes whose
        passes - prefill, score, verify / generate_lookup, seq_* and generate_batch* - stream the 16-bit copy}, a
        subset of w16_info()["classes"] (hook KH_W16_PASS at creation); [] when the passes stream the fp32 matrices."""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().kh_model_w16_info(self._h, out), "kh_model_w16_info")
        return {"classes": [n for i, n in enumerate(_ffi.KH_W16_CLASSES) if out[5] >> i & 1]}

    def w16_format(self) -> dict:
        """The format of the 16-bit weight copy (kh_model_w16_info, slots 6 and 7): {"format": None (no live copy),
        "bf16" or "fp16" (_ffi.KH_FLAG_W16_F16 on an image that is fp16-exact but not bf16-exact),
        "first_inexact_fp16": the first tensor that is not fp16-exact, indexed as w16_info()["first_inexact"]; -1 when
        fp16 was not tried or every tensor passed}."""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().kh_model_w16_info(self._h, out), "kh_model_w16_info")
        return {"format": None if out[0] != 1 else ("fp16" if out[6] else "bf16"), "first_inexact_fp16": int(out[7]) - 1}

    def cls_screen_probe(self, x: np.ndarray) -> dict:
        """One screened step and one full-classifier step on the residual vector x[dim], without advancing
        (kh_model_cls_screen_probe, tests): the two tokens, the candidate rows re-scored, whether the step overflowed,
        and the interval [lb, ub] the screen gave every row.  logits() afterwards returns k_cls's logits of x."""
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (self.cfg.dim,)
        lb = np.empty(self.cfg.vocab_size, np.float32)
        ub = np.empty(self.cfg.vocab_size, np.float32)
        out = (C.c_int64 * 4)()
        _ffi.check(_ffi.lib().kh_model_cls_screen_probe(self._h, x.ctypes.data, lb.ctypes.data, ub.ctypes.data, out),
                   "kh_model_cls_screen_probe")
        return {"token": int(out[0]), "full_token": int(out[1]), "candidates": int(out[2]), "overflow": int(out[3]),
                "lb": lb, "ub": ub}

    def cls_screen_read(self) -> Tuple[np.ndarray, np.ndarray]:
        """(bf16 copy of the classifier as uint16 [vocab, dim], per-row error table [vocab]): kh_model_cls_screen_read."""
        wbf = np.empty((self.cfg.vocab_size, self.cfg.dim), np.uint16)
        err = np.empty(self.cfg.vocab_size, np.float32)
        _ffi.check(_ffi.lib().kh_model_cls_screen_read(self._h, wbf.ctypes.data, err.ctypes.data),
                   "kh_model_cls_screen_read")
        return wbf, err

    def cls_screen_q8_info(self) -> dict:
        """The int8 tier ahead of the bf16 screen (kh_model_cls_screen_q8_info): whether it is on, its creation-time
        self-test, the HBM bytes and creation time of the int8 copy, and counters since creation."""
        out = (C.c_int64 * 8)()
        _ffi.check(_ffi.lib().kh_model_cls_screen_q8_info(self._h, out), "kh_model_cls_screen_q8_info")
        keys = ("on", "selftest", "bytes", "build_us", "steps", "survivors", "spill_steps", "rows_per_workgroup")
        return dict(zip(keys, (int(v) for v in out)))

    def cls_screen_q8_probe(self, x: np.ndarray, grid: int = 0) -> dict:
        """One three-launch screened tail (tier 1 on `grid` workgroups, 0 = as planned) and one full-classifier step on
        the residual vector x[dim], without advancing (kh_model_cls_screen_q8_probe, tests): the two tokens, the rows
        that survived tier 1, whether tier 1 spilled, the candidate rows re-scored, whether the step overflowed, and the
        interval [lb, ub] tier 1 gave every row.  logits() afterwards returns k_cls's logits of x."""
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (self.cfg.dim,)
        lb = np.empty(self.cfg.vocab_size, np.float32)
        ub = np.empty(self.cfg.vocab_size, np.float32)
        out = (C.c_int64 * 6)()
        _ffi.check(_ffi.lib().kh_model_cls_screen_q8_probe(self._h, x.ctypes.data, int(grid), lb.ctypes.data,
                                                           ub.ctypes.data, out), "kh_model_cls_screen_q8_probe")
        return {"token": int(out[0]), "full_token": int(out[1]), "survivors": int(out[2]), "spill": int(out[3]),
                "candidates": int(out[4]), "overflow": int(out[5]), "lb": lb, "ub": ub}

    def cls_screen_q8_read(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(int8 copy [vocab, dim], scales [vocab, dim / 64], per-row error table [vocab]): kh_model_cls_screen_q8_read."""
        V, D = self.cfg.vocab_size, self.cfg.dim
        q = np.empty((V, D), np.int8)
        sc = np.empty((V, D // 64), np.float32)
        e8 = np.empty(V, np.float32)
        _ffi.check(_ffi.lib().kh_model_cls_screen_q8_read(self._h, q.ctypes.data, sc.ctypes.data, e8.ctypes.data),
                   "kh_model_cls_screen_q8_read")
        return q, sc, e8

    def kv_bytes(self) -> Tuple[int, int]:
        """(reserved, committed) bytes of the KV cache: the address range of the reference's up-front allocation and
        the HBM backing it right now (mapped on demand, kh_model_kv_bytes)."""
        r, c = C.c_int64(0), C.c_int64(0)
        _ffi.check(_ffi.lib().kh_model_kv_bytes(self._h, C.byref(r), C.byref(c)), "kh_model_kv_bytes")
        return int(r.value), int(c.value)

    def kv_cache_ptrs(self) -> Tuple[int, int]:
        k, v = C.c_void_p(), C.c_void_p()
        _ffi.check(_ffi.lib().kh_model_get_kv(self._h, C.byref(k), C.byref(v)), "kh_model_get_kv")
        return k.value, v.value

    def read_kv(self, layer: int, row0: int, nrows: int):
        k = np.empty((nrows, self.cfg.kv_dim), np.float32)
        v = np.empty((nrows, self.cfg.kv_dim), np.float32)
        _ffi.check(_ffi.lib().kh_model_read_kv(self._h, layer, row0, nrows, k.ctypes.data,
                                               v.ctypes.data), "kh_model_read_kv")
        return k, v

    def write_kv(self, layer: int, row0: int, k: np.ndarray, v: np.ndarray) -> None:
        """Overwrite cache rows [row0, row0 + len(k)) of `layer` (rotated keys / raw values)."""
        k = np.ascontiguousarray(k, np.float32)
        v = np.ascontiguousarray(v, np.float32)
        assert k.shape == v.shape and k.ndim == 2 and k.shape[1] == self.cfg.kv_dim
        _ffi.check(_ffi.lib().kh_model_write_kv(self._h, layer, row0, k.shape[0], k.ctypes.data,
                                                v.ctypes.data), "kh_model_write_kv")

    def write_kv_device(self, layer: int, row0: int, k: torch.Tensor, v: torch.Tensor) -> None:
        """write_kv from contiguous fp32 GPU tensors [nrows, kv_dim] on the model's device."""
        assert k.is_cuda and v.is_cuda and k.dtype == v.dtype == torch.float32
        assert k.is_contiguous() and v.is_contiguous() and k.shape == v.shape
        assert k.dim() == 2 and k.shape[1] == self.cfg.kv_dim
        torch.cuda.current_stream(k.device).synchronize()  # the copy runs on the model's own stream
        _ffi.check(_ffi.lib().kh_model_write_kv(self._h, layer, row0, k.shape[0], k.data_ptr(),
                                                v.data_ptr()), "kh_model_write_kv")

    # ---- demo/main.cpp generate() ---------------------------------------------------------
    def generate(self, prompt: Sequence[int], total_steps: int, exec: str = "graph",
                 stop: Optional[Sequence[int]] = None) -> Tuple[List[int], float]:
        """Returns (words, elapsed_ms of the step loop measured with HIP events).  `stop` = the
        reference's sentence-ending token ids (demo/main.cpp:30-32); the stop token itself is not
        part of `words`."""
        _ffi.sync_env()  # KH_PREFILL, KH_PG_*
        pr = (C.c_int32 * len(prompt))(*[int(t) for t in prompt])
        st = list(stop or [])
        sp = (C.c_int32 * max(len(st), 1))(*[int(t) for t in st])
        words = (C.c_int32 * total_steps)()
        n = C.c_int32(0)
        ms = C.c_float(0.0)
        _ffi.check(_ffi.lib().kh_model_generate_until(self._h, pr, len(prompt), total_steps,
                                                      EXEC[exec], sp, len(st), words,
                                                      C.byref(n), C.byref(ms)),
                   "kh_model_generate_until")
        return list(words[: n.value]), float(ms.value)

    def first_sample(self) -> Optional[dict]:
        """Near-tie report of the last generate() whose prompt ran as a prefill: the two largest logits of its
        first sampled step (kh_model_first_sample).  None when that generate had no prefill phase."""
        fs = _ffi.FirstSample()
        rc = _ffi.lib().kh_model_first_sample(self._h, C.byref(fs))
        if rc == -2:  # KH_ERR_UNSUPPORTED: no prefill phase
            return None
        _ffi.check(rc, "kh_model_first_sample")
        return {"pos": fs.pos, "prefill_mode": {1: "gemv", 2: "gemm"}.get(fs.prefill_mode, str(fs.prefill_mode)),
                "top1_id": fs.top1_id, "top2_id": fs.top2_id, "top1": float(fs.top1), "top2": float(fs.top2),
                "margin": float(fs.top1) - float(fs.top2)}

    def prefill(self, tokens: Sequence[int], pos0: int = 0) -> None:
        """Forward of `tokens` at positions pos0.. without logits, 8 (fp32) / 4 (int8) tokens per
        weight pass on the VALU; the K/V rows are bit-identical to token-by-token
        predict(is_prompt=True)."""
        t = (C.c_int32 * len(tokens))(*[int(x) for x in tokens])
        _ffi.check(_ffi.lib().kh_model_prefill(self._h, t, len(tokens), pos0), "kh_model_prefill")
        torch.cuda.synchronize()

    @staticmethod
    def score_totals(rec: dict) -> dict:
        """`rec` (the four keys of .logprobs() for the n positions of a score call) plus "sum_logprob", the float64
        sum of the n - 1 targets' log-probs (the last position has no target: token -1), and "perplexity" =
        exp(-sum / (n - 1)) - NaN for a single token, which predicts nothing inside the call."""
        lp = np.asarray(rec["logprob"], np.float64)[np.asarray(rec["token"]) >= 0]
        total = float(lp.sum())
        out = dict(rec)
        out["sum_logprob"] = total
        out["perplexity"] = float(np.exp(-total / len(lp))) if len(lp) else float("nan")
        return out

    def score(self, tokens: Sequence[int], pos0: int = 0) -> dict:
        """log P(token | prefix) of given text (kh_model_score; needs set_logprobs(top_n)): feeds `tokens` at
        positions pos0.. like prefill() and returns the records of those n positions - "token": the token that
        followed (-1 at the last position), "logprob": its log-prob under the raw logits (NaN at the last),
        "top_ids" / "top_logprobs": [n, top_n] - plus "sum_logprob" and "perplexity" (score_totals).  Bit-identical
        to ops.logprobs on the logits a loop of predict() leaves."""
        t = (C.c_int32 * len(tokens))(*[int(x) for x in tokens])
        _ffi.check(_ffi.lib().kh_model_score(self._h, t, len(tokens), int(pos0)), "kh_model_score")
        return self.score_totals(self.logprobs(int(pos0), len(tokens)))

    def verify_width(self) -> int:
        """Tokens per verify pass of this model (kh_model_verify_width): 8 for fp32, 4 for int8 and wide fp32."""
        w = C.c_int32(0)
        _ffi.check(_ffi.lib().kh_model_verify_width(self._h, C.byref(w)), "kh_model_verify_width")
        return int(w.value)

    def verify(self, tokens: Sequence[int], pos0: int, as_set: bool = False,
               constrained: bool = False) -> Tuple[np.ndarray, int]:
        """One verify pass (kh_model_verify): feeds tokens[0] - known - and the drafts tokens[1:] at positions pos0 ..
        in one sweep of the weights.  Returns (next, n_accept): next[i] is the greedy pick at position pos0 + i given
        tokens[:i + 1]; the caller owns next[:n_accept + 1], exactly the tokens a loop of predict() returns, and the
        decode state stands behind them.  as_set (kh_model_verify_as_set): the picks are made under the model's
        sampler, penalties, logit bias and log-probs - what a loop of predict() returns under the same settings -
        and with log-probs on the records of the accepted positions are written.  constrained (kh_model_verify_fsm):
        as_set under set_constraint() as well - every row is masked to the row of the automaton state behind the fed
        tokens ahead of it, next[i] is -1 behind a token the automaton cannot follow, and constraint_state stands
        behind next[n_accept] afterwards."""
        n = len(tokens)
        nxt = np.full(max(n, 1), -1, np.int32)
        a = C.c_int32(-1)
        name = "kh_model_verify_fsm" if constrained else "kh_model_verify_as_set" if as_set else "kh_model_verify"
        _ffi.check(getattr(_ffi.lib(), name)(self._h, _i32_array(tokens), n, int(pos0),
                                             nxt.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(a)), name)
        return nxt[:n], int(a.value)

    def generate_lookup(self, prompt: Sequence[int], total_steps: int, stop: Sequence[int] = (), ngram_max: int = 4,
                        ngram_min: int = 1, miss_steps: int = 8,
                        hint: Optional[Sequence[int]] = None,
                        as_set: bool = False, constrained: bool = False) -> Tuple[List[int], float, dict]:
        """generate(exec="graph") with the sampled part driven by draft + verify (kh_model_generate_lookup): the same
        words, several per sweep of the weights wherever lookup_draft's guess - from the text so far and the optional
        `hint`, the expected output - is right.  Greedy only, unless as_set (kh_model_generate_lookup_as_set): then the
        passes pick under the model's sampler, penalties, logit bias and log-probs, and the words and records are
        generate()'s under the same settings.  Returns (words, elapsed_ms, stats) with stats = {"passes", "drafted",
        "accepted", "plain_steps"}.  constrained (kh_model_generate_lookup_fsm): as_set under set_constraint() as well -
        the automaton drafts (lookup_draft_fsm: the tokens of single-edge rows first), the words are generate()'s under
        the same constraint and settings, and stats gains "forced", the drafted tokens that were forced ones."""
        _ffi.sync_env()  # KH_PREFILL, KH_PG_*
        st, hn = list(stop or []), list(hint or [])
        hint_arr = _i32_array(hn)
        opts = _ffi.LookupOpts(int(ngram_max), int(ngram_min), int(miss_steps),
                               C.cast(hint_arr, C.POINTER(C.c_int32)) if hn else None, len(hn))
        words = (C.c_int32 * max(total_steps, 1))()
        n = C.c_int32(0)
        ms = C.c_float(0.0)
        stats = _ffi.LookupStats()
        args = (self._h, _i32_array(prompt), len(prompt), total_steps, _i32_array(st), len(st), C.byref(opts), words,
                C.byref(n), C.byref(ms), C.byref(stats))
        if constrained:
            forced = C.c_int32(0)
            _ffi.check(_ffi.lib().kh_model_generate_lookup_fsm(*args, C.byref(forced)), "kh_model_generate_lookup_fsm")
            return list(words[: n.value]), float(ms.value), dict(stats.as_dict(), forced=int(forced.value))
        name = "kh_model_generate_lookup_as_set" if as_set else "kh_model_generate_lookup"
        _ffi.check(getattr(_ffi.lib(), name)(*args), name)
        return list(words[: n.value]), float(ms.value), stats.as_dict()

    # ---- sequence slots: several independent sequences per pass over the weights ---------------------------------
    def seq_slots(self, n_slots: int) -> int:
        """Cut the cache rows into n_slots equal sequence slots (kh_model_seq_slots); returns slot_len.  Slot s is
        rows [s * slot_len, (s + 1) * slot_len): read_kv(layer, s * slot_len + p, ..) is position p of its sequence."""
        out = C.c_int32(0)
        _ffi.check(_ffi.lib().kh_model_seq_slots(self._h, int(n_slots), C.byref(out)), "kh_model_seq_slots")
        self._seq_slots = int(n_slots)
        return int(out.value)

    def seq_slots_var(self, lens: Sequence[int]) -> None:
        """Cut the cache rows into len(lens) slots of lens[s] rows, slot 0 from row 0 (kh_model_seq_slots_var).  Resets
        every sharing relation, as seq_slots() does."""
        _ffi.check(_ffi.lib().kh_model_seq_slots_var(self._h, len(lens), _i32_array(lens)), "kh_model_seq_slots_var")
        self._seq_slots = len(lens)

    def seq_share(self, src_slot: int, dst_slot: int, n_rows: int) -> None:
        """Positions [0, n_rows) of dst_slot become src_slot's rows [0, n_rows) (kh_model_seq_share): nothing is
        copied, dst_slot stores only what follows them and holds n_rows + its own length positions.  0 detaches."""
        _ffi.check(_ffi.lib().kh_model_seq_share(self._h, int(src_slot), int(dst_slot), int(n_rows)),
                   "kh_model_seq_share")

    def seq_row(self, slot: int, pos: int) -> int:
        """The cache row that holds position pos of sequence slot `slot` (kh_model_seq_row): read_kv's row."""
        out = C.c_int32(0)
        _ffi.check(_ffi.lib().kh_model_seq_row(self._h, int(slot), int(pos), C.byref(out)), "kh_model_seq_row")
        return int(out.value)

    def seq_width(self, gemm: bool = False) -> int:
        """Lanes (sequences) per pass of this model (kh_model_seq_width): 8 for fp32, 4 for int8 and wide fp32.
        gemm=True: of the wide pass on the matrix cores (kh_model_seq_width_gemm): 64, or KhError where it does not
        run."""
        w = C.c_int32(0)
        name = "kh_model_seq_width_gemm" if gemm else "kh_model_seq_width"
        _ffi.check(getattr(_ffi.lib(), name)(self._h, C.byref(w)), name)
        return int(w.value)

    def seq_gemm_logits(self, lane: int) -> np.ndarray:
        """The logits row of lane `lane` of the last seq_step(gemm=True) / generate_batch(gemm=True) pass
        (kh_model_seq_gemm_logits): what its pick was made from - after penalties and bias where the call had any."""
        out = np.empty(int(self.cfg.vocab_size), np.float32)
        _ffi.check(_ffi.lib().kh_model_seq_gemm_logits(self._h, int(lane), out.ctypes.data_as(C.POINTER(C.c_float))),
                   "kh_model_seq_gemm_logits")
        return out

    def seq_prefill(self, slot: int, tokens: Sequence[int], pos0: int = 0, gemm: bool = False) -> None:
        """prefill() on the rows of sequence slot `slot` (kh_model_seq_prefill).
        gemm=True: as one segment of seq_prefill_many - the MFMA GEMM pass, prefill_gemm()'s contract, not bit-exact."""
        if gemm:
            return self.seq_prefill_many([slot], [tokens], [pos0])
        _ffi.check(_ffi.lib().kh_model_seq_prefill(self._h, int(slot), _i32_array(tokens), len(tokens), int(pos0)),
                   "kh_model_seq_prefill")
        torch.cuda.synchronize()

    def seq_prefill_many(self, slots: Sequence[int], prompts: Sequence[Sequence[int]],
                         pos0: Optional[Sequence[int]] = None) -> None:
        """Prompt segments of several slots in shared GEMM passes on the matrix cores (kh_model_seq_prefill_gemm):
        prompts[i] is fed at positions pos0[i] .. (None: 0) of slot slots[i], up to 512 slab tokens - 32 tiles of 16,
        a tile belongs to one segment - per sweep of the weights (plan_seq_prefill_gemm shows the passes).  Distinct
        slots; a sharer is fed from its shared length on and not together with its parent.  prefill_gemm()'s contract:
        K/V rows equal the token-by-token ones to fp32 round-off; no logits.  KhError where the pass does not run
        (there is no fallback to seq_prefill)."""
        slots, prompts = [int(s) for s in slots], [list(p) for p in prompts]
        pos0 = [0] * len(slots) if pos0 is None else [int(p) for p in pos0]
        if len(prompts) != len(slots) or len(pos0) != len(slots):
            raise ValueError(f"seq_prefill_many: {len(slots)} slots, {len(prompts)} prompts, {len(pos0)} positions")
        if not slots or any(len(p) == 0 for p in prompts):
            raise ValueError("seq_prefill_many: no segment, or an empty one")
        _ffi.sync_env()  # KH_PG_*
        _ffi.check(_ffi.lib().kh_model_seq_prefill_gemm(
            self._h, len(slots), _i32_array(slots), _i32_array([t for p in prompts for t in p]),
            _i32_array([len(p) for p in prompts]), _i32_array(pos0)), "kh_model_seq_prefill_gemm")

    plan_seq_prefill_gemm = staticmethod(plan_seq_prefill_gemm)

    def seq_fork(self, src_slot: int, dst_slot: int, n_rows: int) -> None:
        """Copy K/V rows [0, n_rows) of every layer from one slot to another (kh_model_seq_fork)."""
        _ffi.check(_ffi.lib().kh_model_seq_fork(self._h, int(src_slot), int(dst_slot), int(n_rows)),
                   "kh_model_seq_fork")
        torch.cuda.synchronize()

    def seq_set_constraint(self, automaton=None) -> None:
        """Constrained decoding for sequences in slots (kh_model_seq_set_constraint): ONE constraint.TokenAutomaton for
        all slots - constraint.union() lays different ones side by side - and one state per slot, all -1
        (unconstrained) after this call.  seq_set_constraint_state(slot, s) puts a sequence under the constraint; from
        then on every pass of seq_step / generate_batch / best_of masks that lane's logits to the row of its slot's
        state ahead of penalties, bias, pick and record and moves the state along the pick, exactly as a batch-1 model
        under set_constraint() does.  None turns it off.  One of this and set_constraint() is on at a time."""
        if automaton is None:
            _ffi.check(_ffi.lib().kh_model_seq_set_constraint(self._h, None), "kh_model_seq_set_constraint")
            return
        a, keep = _ffi.fsm(automaton.start, automaton.row_ptr, automaton.tokens, automaton.next)
        _ffi.check(_ffi.lib().kh_model_seq_set_constraint(self._h, C.byref(a)), "kh_model_seq_set_constraint")
        del keep
        torch.cuda.synchronize()

    def seq_constraint_state(self, slot: int) -> int:
        """The automaton state of sequence slot `slot`, -1: unconstrained (kh_model_seq_get_constraint_state;
        synchronises)."""
        s = C.c_int32(0)
        _ffi.check(_ffi.lib().kh_model_seq_get_constraint_state(self._h, int(slot), C.byref(s)),
                   "kh_model_seq_get_constraint_state")
        return int(s.value)

    def seq_set_constraint_state(self, slot: int, state: int) -> None:
        """Slot `slot` continues from `state` of the automaton (kh_model_seq_set_constraint_state); -1: unconstrained.
        Fed-only positions do not move a state: walk forced text with TokenAutomaton.walk() and set the result."""
        _ffi.check(_ffi.lib().kh_model_seq_set_constraint_state(self._h, int(slot), int(state)),
                   "kh_model_seq_set_constraint_state")

    def _seq_constrain(self, constraints) -> None:
        """constraints= of generate_batch / best_of: the union of the given automata, set, every slot at its start."""
        from . import constraint as _constraint
        a, starts = _constraint.union(constraints)
        self.seq_set_constraint(a)
        for s, st in enumerate(starts):
            if st >= 0:
                self.seq_set_constraint_state(s, st)

    def seq_step(self, slots: Sequence[int], tokens: Sequence[int], pos: Sequence[int],
                 samplings: Optional[Sequence] = None, penalties: Optional[Sequence] = None,
                 logit_bias: Optional[Sequence] = None, logprobs: Optional[int] = None,
                 gemm: bool = False) -> List[int]:
        """One pass over len(slots) <= seq_width() lanes in distinct slots (kh_model_seq_step): lane i feeds tokens[i]
        at position pos[i] of slot slots[i]; returns the picks - greedy, or sampled where samplings[i] (None | dict of
        temperature / top_k / top_p / seed) has a temperature > 0 - exactly a predict loop's on a batch-1 model.
        penalties (per lane None | dict of set_penalties()'s keys), logit_bias (per lane None | {id: value}) and
        logprobs (None | top_n for every lane) go through kh_model_seq_step_ex: the pick is then the batch-1 model's
        under those settings over the slot's fed-token history (seq_prefill, seq_fork, seq_set_history, earlier
        passes), the record of the lane's position is read with seq_logprobs(); the model's own set_* values are not
        consulted.  With all three None this is the plain call.
        gemm=True: the wide pass on the matrix cores (kh_model_seq_step_gemm), up to seq_width(gemm=True) = 64 lanes.
        Not bit-identical to the batch-1 loop: logits and K/V rows agree to fp32 round-off, every pick is exact on the
        pass's own logits (seq_gemm_logits).
        Under seq_set_constraint() a lane whose slot holds a state >= 0 is masked to that state's row and moves it."""
        slots, tokens, pos = list(slots), list(tokens), list(pos)
        n = len(slots)
        if len(tokens) != n or len(pos) != n:
            raise ValueError(f"seq_step: {n} slots, {len(tokens)} tokens, {len(pos)} positions")
        sp = _sampling_array(samplings, n, "seq_step")
        nxt = (C.c_int32 * max(n, 1))()
        if gemm:
            _ffi.sync_env()  # KH_PG_*
        if gemm or penalties is not None or logit_bias is not None or logprobs is not None:
            o, keep = _seq_opts(n, sp, penalties, logit_bias, logprobs, "seq_step")
            name = "kh_model_seq_step_gemm" if gemm else "kh_model_seq_step_ex"
            _ffi.check(getattr(_ffi.lib(), name)(self._h, n, _i32_array(slots), _i32_array(tokens), _i32_array(pos),
                                                 C.byref(o), nxt), name)
            del keep
            if logprobs is not None:
                self._seq_top_n = int(logprobs)
            return list(nxt[:n])
        _ffi.check(_ffi.lib().kh_model_seq_step(self._h, n, _i32_array(slots), _i32_array(tokens), _i32_array(pos), sp,
                                                nxt), "kh_model_seq_step")
        return list(nxt[:n])

    def generate_batch(self, prompts: Sequence[Sequence[int]], total_steps, samplings: Optional[Sequence] = None,
                       stop: Sequence[int] = (), cached: Optional[Sequence[int]] = None,
                       penalties: Optional[Sequence] = None, logit_bias: Optional[Sequence] = None,
                       logprobs: Optional[int] = None, gemm: bool = False,
                       gemm_prefill: bool = False,
                       constraints: Optional[Sequence] = None) -> Tuple[List[List[int]], float]:
        """generate() for len(prompts) <= n_slots sequences at once, sequence s in slot s (kh_model_generate_batch):
        seq_width() sequences share every pass over the weights.  total_steps: one int for all or one per sequence;
        samplings: None (all greedy) or one entry per sequence (None | dict of temperature / top_k / top_p / seed).
        cached: None, or per sequence how many leading prompt positions seq_prefill / seq_fork already left in its
        slot (kh_model_generate_batch_from).  Returns (words per sequence, elapsed_ms); every word list is exactly
        generate(prompt, total, stop=stop)'s on a batch-1 model with that entry set through set_sampling().
        penalties / logit_bias (one entry per sequence: None | dict of set_penalties()'s keys, None | {id: value}) and
        logprobs (None | top_n) go through kh_model_generate_batch_ex: the words are then that model's under
        set_penalties / set_logit_bias / set_logprobs too, and seq_logprobs(s, 0, len(words[s])) its records.  The
        model's own set_* values are not consulted.  With all three None this is the plain call.
        gemm=True: the sampled part runs as wide passes on the matrix cores (kh_model_generate_batch_gemm), up to 64
        sequences per pass over the weights.  Not bit-identical: greedy words can differ from generate()'s at
        near-ties, sampled words are the sampler's on the pass's own logits.
        gemm_prefill=True (orthogonal to gemm=): the fed-only part of every prompt that is not cached yet goes through
        one seq_prefill_many first - GEMM passes shared between the sequences instead of seq_prefill's passes per
        sequence - and the call then runs with cached = len(prompt) - 1.  prefill_gemm()'s contract for those rows.
        constraints: None, or one entry per sequence (None | constraint.TokenAutomaton): sequence s is sampled under
        its automaton from the automaton's start state - constraint.union() of the entries is set with
        seq_set_constraint(), every slot gets its start, and the constraint is turned off again behind the call.
        Sequence s's words and records are then generate()'s of a batch-1 model under set_constraint(constraints[s]).
        Without constraints= the call samples from whatever state seq_set_constraint_state() left in each slot."""
        if constraints is not None and any(a is not None for a in constraints):
            if len(constraints) != len(prompts):
                raise ValueError(f"generate_batch: {len(constraints)} constraints for {len(prompts)} prompts")
            self._seq_constrain(constraints)
            try:
                return self.generate_batch(prompts, total_steps, samplings, stop=stop, cached=cached,
                                           penalties=penalties, logit_bias=logit_bias, logprobs=logprobs, gemm=gemm,
                                           gemm_prefill=gemm_prefill)
            finally:
                self.seq_set_constraint(None)
        prompts = [list(p) for p in prompts]
        n = len(prompts)
        totals = [int(total_steps)] * n if isinstance(total_steps, (int, np.integer)) else [int(t) for t in total_steps]
        if len(totals) != n:
            raise ValueError(f"generate_batch: {len(totals)} totals for {n} prompts")
        if n == 0 or any(len(p) == 0 for p in prompts):
            raise ValueError("generate_batch: no prompt, or an empty one")
        sp = _sampling_array(samplings, n, "generate_batch")
        if cached is not None and len(cached) != n:
            raise ValueError(f"generate_batch: {len(cached)} cached counts for {n} prompts")
        st = list(stop or [])
        if gemm_prefill:
            have = [0] * n if cached is None else [int(c) for c in cached]
            fed = [min(len(p) - 1, t) for p, t in zip(prompts, totals)]
            todo = [s for s in range(n) if fed[s] > have[s]]
            if todo:
                self.seq_prefill_many(todo, [prompts[s][have[s]:fed[s]] for s in todo], [have[s] for s in todo])
            cached = [max(f, h) for f, h in zip(fed, have)]
        stride = max(max(totals), 1)
        words = (C.c_int32 * (n * stride))()
        nw = (C.c_int32 * n)()
        ms = C.c_float(0.0)
        flat = [t for p in prompts for t in p]
        if gemm:
            _ffi.sync_env()  # KH_PG_*
        if gemm or penalties is not None or logit_bias is not None or logprobs is not None:
            o, keep = _seq_opts(n, sp, penalties, logit_bias, logprobs, "generate_batch")
            name = "kh_model_generate_batch_gemm" if gemm else "kh_model_generate_batch_ex"
            _ffi.check(getattr(_ffi.lib(), name)(
                self._h, n, _i32_array(flat), _i32_array([len(p) for p in prompts]),
                None if cached is None else _i32_array(cached), _i32_array(totals), C.byref(o), _i32_array(st), len(st),
                words, stride, nw, C.byref(ms)), name)
            del keep
            if logprobs is not None:
                self._seq_top_n = int(logprobs)
            return [list(words[s * stride:s * stride + nw[s]]) for s in range(n)], float(ms.value)
        _ffi.check(_ffi.lib().kh_model_generate_batch_from(
            self._h, n, _i32_array(flat), _i32_array([len(p) for p in prompts]),
            None if cached is None else _i32_array(cached), _i32_array(totals), sp, _i32_array(st), len(st), words,
            stride, nw, C.byref(ms)), "kh_model_generate_batch")
        return [list(words[s * stride:s * stride + nw[s]]) for s in range(n)], float(ms.value)

    def seq_set_history(self, slot: int, tokens: Sequence[int], pos0: int = 0) -> None:
        """The fed-token history of positions pos0 .. of sequence slot `slot` (kh_model_seq_set_history): what the
        penalties of a later seq_step / generate_batch on that slot count, for rows that were not fed through
        seq_prefill (write_kv, a restored cache)."""
        _ffi.check(_ffi.lib().kh_model_seq_set_history(self._h, int(slot), int(pos0), _i32_array(tokens), len(tokens)),
                   "kh_model_seq_set_history")

    def seq_logprobs(self, slot: int, pos0: int, n: int, top_n: Optional[int] = None) -> dict:
        """logprobs() on the rows of sequence slot `slot` (kh_model_seq_get_logprobs): the records of positions
        [pos0, pos0 + n) that seq_step / generate_batch with logprobs= left.  The width of the top lists is that of
        the last such call (top_n, when given, must state the same)."""
        w = self._seq_top_n if top_n is None else int(top_n)
        if w is None or w != self._seq_top_n:
            raise ValueError(f"seq_logprobs: the last call with logprobs= on this model said {self._seq_top_n}")
        out = {"token": np.empty(max(n, 0), np.int32), "logprob": np.empty(max(n, 0), np.float32),
               "top_ids": np.empty((max(n, 0), w), np.int32), "top_logprobs": np.empty((max(n, 0), w), np.float32)}
        _ffi.check(_ffi.lib().kh_model_seq_get_logprobs(self._h, int(slot), int(pos0), int(n), out["token"].ctypes.data,
                                                        out["logprob"].ctypes.data, out["top_ids"].ctypes.data,
                                                        out["top_logprobs"].ctypes.data), "kh_model_seq_get_logprobs")
        return out

    seq_rank = staticmethod(seq_rank)

    def best_of(self, prompt: Sequence[int], n: int, total_steps: int, sampling: dict, stop: Sequence[int] = (),
                penalties: Optional[dict] = None, logit_bias: Optional[dict] = None, top_n: int = 0,
                share: bool = False, gemm: bool = False, gemm_prefill: bool = False,
                constraints=None) -> List[dict]:
        """n samples of one prompt, best first: one seq_prefill of the prompt's fed-only part into slot 0, n - 1
        seq_forks, one generate_batch(cached=..) with seeds seed, seed + 1, .. of `sampling` (and the shared penalties
        / logit_bias), then seq_rank on the sampled positions' log-probs.  Returns [{"words", "mean_logprob", "seed"}]
        in rank order; sample i is exactly generate() of a batch-1 model under seed + i.  Cuts the cache into n slots
        when the model has fewer.
        share=True: the samples read the prompt's rows from slot 0 instead of holding copies - one prefill, n - 1
        seq_share calls on plan_shared_layout(cfg.cache_len, ..) - so n samples need prompt + n * generated rows, not
        n * (prompt + generated).  Same words and records; penalties are refused on sharing slots.
        gemm=True: the samples decode as wide passes (generate_batch(gemm=True)), up to 64 per pass over the weights;
        sample i is then the sampler's on the wide pass's logits, equal to generate()'s to fp32 round-off.
        gemm_prefill=True: the one prefill is seq_prefill(.., gemm=True), the GEMM pass on the matrix cores.
        constraints: None | one constraint.TokenAutomaton for all samples (generate_batch's constraints=, the same
        entry n times): every sample is generate()'s of a batch-1 model under set_constraint() and its seed."""
        prompt, n, total_steps = [int(t) for t in prompt], int(n), int(total_steps)
        if n <= 0 or not prompt:
            raise ValueError("best_of: no sample, or an empty prompt")
        seed0 = int(sampling.get("seed", 0))
        fed = min(len(prompt) - 1, total_steps)
        share = bool(share) and fed > 0 and n > 1
        if share:
            if penalties is not None:
                raise ValueError("best_of: penalties on slots that share a prefix are not supported")
            self.seq_slots_var(plan_shared_layout(int(self.cfg.cache_len), n, fed, total_steps))
        elif self._seq_slots < n:
            self.seq_slots(n)
        if fed > 0:
            self.seq_prefill(0, prompt[:fed], gemm=bool(gemm_prefill))
            for s in range(1, n):
                if share:
                    self.seq_share(0, s, fed)
                else:
                    self.seq_fork(0, s, fed)
        words, _ = self.generate_batch([prompt] * n, total_steps, [dict(sampling, seed=seed0 + s) for s in range(n)],
                                       stop=stop, cached=[fed] * n, penalties=[penalties] * n,
                                       logit_bias=[logit_bias] * n, logprobs=int(top_n), gemm=gemm,
                                       constraints=None if constraints is None else [constraints] * n)
        rows = [self.seq_logprobs(s, 0, len(w))["logprob"] if w else np.empty(0, np.float32) for s, w in enumerate(words)]
        order, mean = seq_rank(rows, [min(fed, len(w)) for w in words], [len(w) for w in words])
        return [{"words": words[s], "mean_logprob": float(mean[s]), "seed": seed0 + s} for s in order]

    def prefill_gemm(self, tokens: Sequence[int], pos0: int = 0) -> None:
        """Forward of `tokens` at positions pos0.. as fp32-MFMA GEMMs (up to 128 tokens per weight
        pass); K/V rows equal the token-by-token ones to fp32 round-off."""
        _ffi.sync_env()
        t = (C.c_int32 * len(tokens))(*[int(x) for x in tokens])
        _ffi.check(_ffi.lib().kh_model_prefill_gemm(self._h, t, len(tokens), pos0),
                   "kh_model_prefill_gemm")
        torch.cuda.synchronize()

    PREFILL_MODES = {"token": 0, "gemv": 1, "gemm": 2}

    def time_prefill(self, tokens: Sequence[int], pos0: int = 0, mode: str = "gemm") -> float:
        """Milliseconds (HIP events on the model stream) of the prompt phase alone for `tokens`:
        "token" = one forward pass per token (the reference), "gemv" = B-token VALU kernels,
        "gemm" = fp32-MFMA GEMM prefill."""
        _ffi.sync_env()
        t = (C.c_int32 * len(tokens))(*[int(x) for x in tokens])
        ms = C.c_float(0.0)
        _ffi.check(_ffi.lib().kh_model_time_prefill(self._h, t, len(tokens), pos0,
                                                    self.PREFILL_MODES[mode], C.byref(ms)),
                   "kh_model_time_prefill")
        return float(ms.value)

    def time_step(self, pos: int, reps: int = 9) -> List[float]:
        """Microseconds of one graph-replayed decode step at `pos`, `reps` samples."""
        us = (C.c_float * reps)()
        _ffi.check(_ffi.lib().kh_model_time_step(self._h, pos, reps, us), "kh_model_time_step")
        return [float(v) for v in us]

    def profile_kernels(self, pos: int, reps: int = 8):
        """Back-to-back average launch duration (us) of every kernel class at position `pos`
        (kh_model_profile_kernel); clobbers activations and KV row `pos`."""
        out = {}
        for i in range(_ffi.KH_NUM_KCLASS):
            us = C.c_float(0.0)
            _ffi.check(_ffi.lib().kh_model_profile_kernel(self._h, i, pos, reps, C.byref(us)),
                       "kh_model_profile_kernel")
            out[_ffi.lib().kh_kclass_name(i).decode()] = float(us.value)
        return out

    def profile_kernel(self, name: str, pos: int, reps: int = 8) -> float:
        """Back-to-back average launch duration (us) of ONE kernel class ("attn", "ffn13", ...)."""
        names = [_ffi.lib().kh_kclass_name(i).decode() for i in range(_ffi.KH_NUM_KCLASS)]
        us = C.c_float(0.0)
        _ffi.check(_ffi.lib().kh_model_profile_kernel(self._h, names.index(name), pos, reps,
                                                      C.byref(us)), "kh_model_profile_kernel")
        return float(us.value)

    def profile_step(self, start_pos: int, n_steps: int):
        """Per-kernel-class average launch duration (us) of the fused step, HIP events."""
        avg = (C.c_float * _ffi.KH_NUM_KCLASS)()
        cnt = (C.c_int32 * _ffi.KH_NUM_KCLASS)()
        _ffi.check(_ffi.lib().kh_model_profile_step(self._h, start_pos, n_steps, avg, cnt),
                   "kh_model_profile_step")
        names = [_ffi.lib().kh_kclass_name(i).decode() for i in range(_ffi.KH_NUM_KCLASS)]
        return {n: {"avg_us": float(avg[i]), "launches_per_step": int(cnt[i])}
                for i, n in enumerate(names)}

    @property
    def load_ms(self) -> float:
        """Host image -> HBM upload time of the loader (pinned double-buffered chunks)."""
        return float(_ffi.lib().kh_model_get_load_ms(self._h))

    @property
    def stream(self) -> int:
        return int(_ffi.lib().kh_model_stream(self._h) or 0)
