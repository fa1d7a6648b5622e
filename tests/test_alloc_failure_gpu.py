"""Every allocation of the model level under an injected failure (hook KH_ALLOC_FAIL, kh_debug_alloc_stats).

An injected failure is an error return of the library's one allocation function: the runtime is not called, the GPU is
not touched.  What is checked is the host code around it: nothing leaks, nothing is left half built, and a call that
failed can simply be made again.

Models: dim 256, hidden 512, 2 layers, 4 heads, 2 KV heads (head size 64), vocab 512 - fp32 (tied), the same image
with bf16-exact matrices under KH_FLAG_W16, and int8 with group 64 (untied: an int8 model has no tied classifier).
Cache 128 rows, except where a call needs more: generate() refuses more steps than cache rows, so the 300-step run
that grows the step buffers past their first 256 entries uses 1024 rows, and so does the GEMM prefill with
KH_PG_ATTN=0 - a 128-row cache has one attention split and therefore no split workspace to allocate.

  1. create: for k = 1 .. N (N = the allocations of a hook-free create, from the counter) a create with the k-th
     allocation failing either fails, with no model and nothing alive, or - only where the failed allocation is one
     of the int8 screen tier's own Q8_TIER_ALLOCS = 8 (cls_screen_q8_create: "no room: the tier is off") - succeeds
     with the tier off and the hook-free model's tokens.
  2. lazy paths: for each call and each k = 1 .. n (n = the allocations of the call on a fresh model) the call fails on
     a fresh model, succeeds when repeated, and then yields the bits of a model that never failed.
  3. normal use leaks nothing: the cycles of tools/stress_destroy.py, one of them with two models alive.
"""
import numpy as np
import pytest
import torch

from kuiperllama_amd import _ffi, binfmt

pytestmark = pytest.mark.gpu

OOM = 2            # hipErrorOutOfMemory
Q8_TIER_ALLOCS = 8  # cls_screen_q8_create: q, sc, e8, p_lb, p_spill, p_ub, p_idx, stats
PROMPT = [5, 17, 300, 41]


def _spec(cache, quant=False, name="af"):
    return binfmt.ModelSpec(256, 512, 2, 4, 2, 512, cache, not quant, binfmt.FAMILY_LLAMA, quant, 64, binfmt.ROPE_HALF,
                            500000.0, 1e-5, f"{name}-{cache}{'-q8' if quant else ''}")


@pytest.fixture(scope="module")
def images(gpu):
    """kind -> (spec, device image, host image, flags)"""
    out = {}
    for kind, cache, quant, w16 in (("fp32", 128, False, False), ("w16", 128, False, True), ("int8", 128, True, False),
                                    ("fp32-long", 1024, False, False)):
        spec = _spec(cache, quant)
        img = binfmt.synth_image(spec, seed=11, device=gpu, final_norm_std=1.0)
        if w16:
            binfmt.round_matrices_bf16(img, spec)
        torch.cuda.synchronize()
        out[kind] = (spec, img, np.ascontiguousarray(img.cpu().numpy()), _ffi.KH_FLAG_W16 if w16 else 0)
    yield out
    _ffi.debug_set("KH_ALLOC_FAIL", None)


def _create(images, kind, host=False):
    from kuiperllama_amd.model import KuiperModel
    spec, dev, hst, flags = images[kind]
    return KuiperModel.from_host_image(hst, spec, flags=flags) if host else KuiperModel.from_device_image(dev, spec, flags=flags)


def _live():
    s = _ffi.alloc_stats()
    return s["live"], s["live_bytes"]


def _same(a, b):
    """bit for bit, NaN included"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, float, np.floating)):
        a, b = np.asarray(a), np.asarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


# ---- 1. create ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,host,plain_kv", [("fp32", False, False), ("w16", False, False), ("int8", False, False),
                                                ("fp32", True, False), ("fp32", False, True)])
def test_create_under_injected_failure(images, kind, host, plain_kv):
    base = _live()
    _ffi.debug_set("KH_KV_VMM", "0" if plain_kv else None)  # plain: the two halves of the cache are counted too
    try:
        _ffi.debug_set("KH_ALLOC_FAIL", None)  # restarts the count
        m = _create(images, kind, host)
        n_create = _ffi.alloc_stats()["allocs"]
        tier = m.cls_screen_q8_info()["on"]
        assert tier == (0 if kind == "int8" else 1)
        if kind == "w16":
            assert m.w16_info()["state"] == 1
        words = m.generate(PROMPT, 16)[0]
        m.close()
        assert _live() == base
        assert n_create >= (12 if plain_kv else 10), n_create
        print(f"{kind} host={host} plain_kv={plain_kv}: {n_create} allocations per create")
        tolerated = []
        for k in range(1, n_create + 1):
            _ffi.debug_set("KH_ALLOC_FAIL", k)
            try:
                m = _create(images, kind, host)
            except _ffi.KhError as e:
                assert e.code == OOM, (k, e)
                assert _ffi.alloc_stats()["injected"] == 1, k
                assert _live() == base, (k, _live(), base)
                continue
            # KH_OK: only the int8 tier may shrug a failed allocation off
            assert _ffi.alloc_stats()["injected"] == 1, k
            _ffi.debug_set("KH_ALLOC_FAIL", None)
            tolerated.append(k)
            assert tier and m.cls_screen_q8_info()["on"] == 0 and m.cls_screen_info()["on"] == 1, k
            assert m.generate(PROMPT, 16)[0] == words, k
            m.close()
            assert _live() == base, (k, _live(), base)
        print(f"  tolerated at k = {tolerated}")
        # a condition, not a measurement: each of the tier's own allocations turns it off, nothing else is shrugged off
        assert len(tolerated) == (Q8_TIER_ALLOCS if tier else 0), tolerated
        assert len(tolerated) == 0 or tolerated == list(range(tolerated[0], tolerated[0] + len(tolerated)))  # one block
    finally:
        _ffi.debug_set("KH_ALLOC_FAIL", None)
        _ffi.debug_set("KH_KV_VMM", None)


# ---- 2. lazy paths ------------------------------------------------------------------------------------------------
def _kv_rows(n):
    return lambda m: [m.read_kv(layer, 0, n) for layer in range(m.cfg.layer_num)]


def _gen(steps=16):
    return lambda m: m.generate(PROMPT, steps, exec="graph")[0]


def _gen_records(m):
    return m.generate(PROMPT, 16, exec="graph")[0], m.logprobs(0, 16)


def _bias_setup(m):
    m.set_logit_bias({3: 0.25})  # the first capacity: 64 entries
    m.generate(PROMPT, 16, exec="graph")  # captured k_sample_proc launches hold the lists' addresses


def _seq_ex_read(m):
    return [m.seq_logprobs(s, 0, 1) for s in (0, 1)]


TOKS = [(37 * i + 11) % 512 for i in range(16)]
BIAS65 = {i: 0.01 * (i % 7) for i in range(65)}
# name -> (model kind, hooks, setup, call, read)
LAZY = {
    "prefill": ("fp32", {}, None, lambda m: m.prefill(TOKS[:8]), _kv_rows(8)),
    "prefill-int8": ("int8", {}, None, lambda m: m.prefill(TOKS[:8]), _kv_rows(8)),
    "prefill_gemm": ("fp32", {}, None, lambda m: m.prefill_gemm(TOKS), _kv_rows(16)),
    "prefill_gemm-int8": ("int8", {}, None, lambda m: m.prefill_gemm(TOKS), _kv_rows(16)),
    "prefill_gemm-long": ("fp32-long", {}, None, lambda m: m.prefill_gemm(TOKS), _kv_rows(16)),
    "prefill_gemm-fallback-attn": ("fp32-long", {"KH_PG_ATTN": "0"}, None, lambda m: m.prefill_gemm(TOKS), _kv_rows(16)),
    "score": ("fp32", {}, lambda m: m.set_logprobs(2), lambda m: m.score(TOKS[:8]), None),
    "generate_lookup": ("fp32", {}, None, lambda m: m.generate_lookup(PROMPT, 24)[::2], None),
    "seq_step": ("fp32", {}, lambda m: m.seq_slots(2), lambda m: m.seq_step([0, 1], [5, 9], [0, 0]), None),
    "seq_step_ex": ("fp32", {}, lambda m: m.seq_slots(2), lambda m: m.seq_step([0, 1], [5, 9], [0, 0], logprobs=2),
                    _seq_ex_read),
    "set_logprobs": ("fp32", {}, None, lambda m: m.set_logprobs(2), _gen_records),
    "set_penalties": ("fp32", {}, None, lambda m: m.set_penalties(repetition=1.3, presence=0.1), _gen()),
    "set_sampling": ("fp32", {}, None, lambda m: m.set_sampling(temperature=0.8, top_k=40, seed=7), _gen()),
    "set_logit_bias-grow": ("fp32", {}, _bias_setup, lambda m: m.set_logit_bias(BIAS65), _gen()),
    "generate-grow": ("fp32-long", {}, lambda m: m.generate(PROMPT, 16, exec="graph"), _gen(300), _gen(32)),
}


def _run(m, setup, call, read):
    if setup:
        setup(m)
    _ffi.debug_set("KH_ALLOC_FAIL", None)
    out = call(m)
    n = _ffi.alloc_stats()["allocs"]
    return n, (out, read(m) if read else None)


@pytest.mark.parametrize("name", sorted(LAZY))
def test_lazy_path_under_injected_failure(images, name):
    kind, hooks, setup, call, read = LAZY[name]
    base = _live()
    try:
        for k, v in hooks.items():
            _ffi.debug_set(k, v)
        m = _create(images, kind)
        n, want = _run(m, setup, call, read)  # the model that never failed
        m.close()
        assert _live() == base
        assert n >= 1, "the call allocates nothing: not a lazy path"
        print(f"{name}: {n} allocations")
        for k in range(1, n + 1):
            m = _create(images, kind)
            if setup:
                setup(m)
            _ffi.debug_set("KH_ALLOC_FAIL", k)
            with pytest.raises(_ffi.KhError) as ei:
                call(m)
            assert ei.value.code == OOM, (k, ei.value)
            assert _ffi.alloc_stats()["injected"] == 1, k
            _ffi.debug_set("KH_ALLOC_FAIL", None)
            got = (call(m), read(m) if read else None)
            assert _same(got, want), (name, k)
            m.close()
            assert _live() == base, (k, _live(), base)
    finally:
        _ffi.debug_set("KH_ALLOC_FAIL", None)
        for k in hooks:
            _ffi.debug_set(k, None)


def test_fallback_attention_of_the_gemm_prefill_allocates_its_workspace(images):
    """KH_PG_ATTN=0 on a cache with several attention splits: one allocation more than the MFMA attention (pg_ws)."""
    counts = {}
    try:
        for hook in (None, "0"):
            _ffi.debug_set("KH_PG_ATTN", hook)
            m = _create(images, "fp32-long")
            counts[hook], _ = _run(m, None, lambda m: m.prefill_gemm(TOKS), None)
            m.close()
    finally:
        _ffi.debug_set("KH_PG_ATTN", None)
    assert counts["0"] == counts[None] + 1, counts


# ---- 3. no leak in normal use -------------------------------------------------------------------------------------
def test_normal_use_leaks_nothing(images):
    """One cycle of each mode of tools/stress_destroy.py (scaled to the 1024-row model), the generate cycle with a
    second model alive across the first one's destruction."""
    rng = np.random.default_rng(3)
    toks = [int(t) for t in rng.integers(0, 512, 601)]
    base = _live()
    _ffi.debug_set("KH_ALLOC_FAIL", None)
    for mode in range(4):
        m = _create(images, "fp32-long")
        assert _live()[0] > base[0]
        if mode == 0:
            m.prefill_gemm(toks[:600], 0)
            m.predict(toks[600], 600, exec="fused")
        elif mode == 1:
            m.generate(toks[:5], 64, exec="graph")
        elif mode == 2:
            m.prefill(toks[:37], 0)
            m.predict(toks[37], 37, exec="fused")
            m.read_kv(0, 0, 38)
        else:
            m.prefill_gemm(toks[:200], 0)
            m.prefill_gemm(toks[200:530], 200)
            m.logits()
        if mode == 1:
            m2 = _create(images, "int8")
            mid = _live()
            m.close()
            assert base[0] < _live()[0] < mid[0]
            m2.generate([1, 2, 3], 16, exec="graph")
            m2.close()
        else:
            m.close()
        assert _live() == base, (mode, _live(), base)
    assert _ffi.alloc_stats()["injected"] == 0
