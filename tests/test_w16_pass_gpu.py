"""The B-token passes of W16 models on the GPU (kh_w16_pass.h): prefill, score, verify / generate_lookup and the
sequence-slot calls of a KH_FLAG_W16 model stream the 16-bit copy and leave the BITS of the same image streamed as
fp32 - K/V rows, records, picks and words compared as raw words / bytes, never with a tolerance.

Models: 2 layers, 1024 cache rows, synth_image(seed fixed, final_norm_std=1.0) with its matrices rounded to bf16
(binfmt.round_matrices_bf16) at the four geometries of test_w16_gpu.py: 8 tokens per pass at dim 448 / 960 / 1152,
4 at dim 4224 (eight vectors exceed 80 KiB), 2 for w2 at hidden 10368.  The two models of a comparison share one
device image.

  1. state and launches: flag on with every class's pass on the copy (KH_W16_PASS=0x1f) -> a prefill, a score and a
     seq_step log only _w16 stems for the five pass classes; the default mask (ffn13, w2: DESIGN 3.1c's adoption) and
     any other class mask -> exactly their classes; KH_W16_PASS=0 -> the fp32 stems while a predict still logs the
     decode _w16 kernels; an unrounded image (state -1) and int8 -> the flag-off launches.  w16_pass_info() agrees in
     each case.  Tests 2 - 4 run under KH_W16_PASS=0x1f: all five classes are compared, adopted by default or not.
  2. bit identity under forced shapes: per geometry every (split, workgroup width) KH_SHAPE_* accept and
     prefill_supported admits, plus a shape with small odd grids; prefill of 1, width and 2 width + 1 tokens, a
     prefill across position 256 over random rows, a verify whose first wrong draft sits in the middle, a score with
     top-5 records and a seq_step over lanes at unequal positions in shuffled slots.  After every call the whole
     cache of both models is compared, and every row the call does not own against what it held before.
  3. the copy is what is read: NaN over the fp32 matrices of layer 1 and the classifier leaves a flag-on model's
     score records and generate_batch words as they were and turns a flag-off model's log-probs into NaN.
  4. loops: generate_batch (width + 1 sequences, sampled, a stop token; penalties, bias and records), best_of over a
     shared prefix and generate_lookup with a truthful hint, flag off against flag on; one sequence against generate
     of a flag-on batch-1 model.
  5. coverage gate: every compiled instantiation of the five stems was launched and compared by (2).
"""
import numpy as np
import pytest
import torch

import code_objects as co
from kuiperllama_amd import _ffi, binfmt, build

pytestmark = pytest.mark.gpu

CACHE = 1024
W16 = _ffi.KH_FLAG_W16
EXACT = _ffi.KH_FLAG_PREFILL_EXACT
L, Q2 = binfmt.FAMILY_LLAMA, binfmt.FAMILY_QWEN2
HALF, INTER = binfmt.ROPE_HALF, binfmt.ROPE_INTERLEAVED


def _spec(dim, hidden, heads, kv_heads, vocab, rope, family, name, tied=False, quant=False):
    q = family == Q2
    return binfmt.ModelSpec(dim, hidden, 2, heads, kv_heads, vocab, CACHE, tied, family, quant, 64, rope,
                            1000000.0 if q else 10000.0, 1e-6 if q else 1e-5, name)


GEOMETRIES = {
    "1152-h10368": _spec(1152, 10368, 18, 6, 1001, HALF, L, "w16-1152"),          # w2: 2 tokens per pass
    "4224-h3072": _spec(4224, 3072, 33, 3, 777, INTER, L, "w16-4224"),            # 4 tokens per pass
    "qwen-960-hs80": _spec(960, 1600, 12, 2, 1537, HALF, Q2, "w16-qwen"),         # bias, 240 units: masked lanes
    "448-tied": _spec(448, 1216, 7, 7, 999, INTER, L, "w16-tied", tied=True),     # the copy of tok_emb
}
WIDTH = {"1152-h10368": 8, "4224-h3072": 4, "qwen-960-hs80": 8, "448-tied": 8}
TIED = GEOMETRIES["448-tied"]
QWEN = GEOMETRIES["qwen-960-hs80"]
STEMS = {"k_pf_qkv_w16", "k_seq_qkv_w16", "k_pf_ffn13_w16", "k_pf_gemv_res_w16", "k_pf_cls_w16"}
FP32_STEMS = {"k_pf_qkv", "k_seq_qkv", "k_pf_ffn13", "k_pf_gemv_res", "k_pf_cls"}
DECODE_W16 = {"k_qkv_w16", "k_gemv_res_w16", "k_wo_comb_w16", "k_ffn13_w16", "k_cls_w16"}
ALL = list(_ffi.KH_W16_CLASSES)
DEFAULT = ["ffn13", "w2"]  # the classes whose pass reads the copy unless KH_W16_PASS says otherwise

_LAUNCHED = {}  # geometry -> _w16 pass instantiations its shapes launched (test_bit_identity -> test_coverage_gate)


def _model(img, spec, flags=0, passes=None):
    """passes: the value of the hook KH_W16_PASS while the model is created (None: unset)"""
    from kuiperllama_amd.model import KuiperModel
    _ffi.debug_set("KH_W16_PASS", passes)
    try:
        return KuiperModel.from_device_image(img, spec, flags=flags)
    finally:
        _ffi.debug_set("KH_W16_PASS", None)


def _rounded(spec, gpu, seed=4242):
    img = binfmt.synth_image(spec, seed=seed, device=gpu, final_norm_std=1.0)
    binfmt.round_matrices_bf16(img, spec)
    torch.cuda.synchronize()
    return img


@pytest.fixture(scope="module")
def tied_img(gpu):
    return _rounded(TIED, gpu)


def _pass_log(log):
    return {k for k in log if k.split("<")[0] in STEMS | FP32_STEMS}


def _stems(log):
    return {k.split("<")[0] for k in log}


def _rec_bytes(rec):
    return b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in ("token", "logprob", "top_ids", "top_logprobs"))


# ---- 1. state and launches --------------------------------------------------------------------
def _logged_passes(m, spec):
    """(stems of the pass launches of a prefill of 3 tokens, a score of 9 and a seq_step of 3 lanes; stems a predict
    launched)"""
    toks = [int(t) for t in np.random.default_rng(3).integers(0, spec.vocab_size, 9)]
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        m.prefill(toks[:3], 0)
        m.set_logprobs(5)
        m.score(toks, 0)
        m.set_logprobs(None)
        m.seq_slots(4)
        m.seq_step([2, 0, 3], toks[:3], [0, 4, 1])
        passes = _stems(_pass_log(_ffi.launch_log()))
        _ffi.debug_set("KH_LAUNCH_LOG", "1")  # an empty log
        m.predict(5, 0, exec="fused")
        return passes, _stems(_ffi.launch_log())
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)


def test_state_and_launches(gpu, tied_img):
    m0 = _model(tied_img, TIED)
    m1 = _model(tied_img, TIED, W16, passes="0x1f")
    md = _model(tied_img, TIED, W16)
    try:
        # fails on a library without the feature: no such entry point
        assert m0.w16_pass_info() == {"classes": []}
        assert m1.w16_info()["state"] == 1 and m1.w16_pass_info() == {"classes": ALL}
        assert md.w16_info()["classes"] == ALL and md.w16_pass_info() == {"classes": DEFAULT}
        p0, d0 = _logged_passes(m0, TIED)
        p1, d1 = _logged_passes(m1, TIED)
        pd, dd = _logged_passes(md, TIED)
        assert p0 == FP32_STEMS, sorted(p0)
        assert p1 == STEMS, sorted(p1)
        # wo and w2 share a stem: the default mask launches both forms of it
        assert pd == {"k_pf_qkv", "k_seq_qkv", "k_pf_gemv_res", "k_pf_gemv_res_w16", "k_pf_ffn13_w16", "k_pf_cls"}, sorted(pd)
        assert not d0 & DECODE_W16, sorted(d0)
        assert d1 & DECODE_W16 == dd & DECODE_W16 == DECODE_W16 - {"k_wo_comb_w16"}, (sorted(d1), sorted(dd))
    finally:
        m0.close()
        m1.close()
        md.close()


def test_hook_keeps_the_passes_on_fp32_or_picks_classes(gpu, tied_img):
    m = _model(tied_img, TIED, W16, passes="0")
    try:
        assert m.w16_info()["classes"] == ALL and m.w16_pass_info() == {"classes": []}
        p, d = _logged_passes(m, TIED)
        assert p == FP32_STEMS, sorted(p)
        assert d & DECODE_W16 == DECODE_W16 - {"k_wo_comb_w16"}, sorted(d)  # decode still reads the copy
    finally:
        m.close()
    m = _model(tied_img, TIED, W16, passes="0x11")  # qkv and cls
    try:
        assert m.w16_pass_info() == {"classes": ["qkv", "cls"]}
        p, _ = _logged_passes(m, TIED)
        assert p == {"k_pf_qkv_w16", "k_seq_qkv_w16", "k_pf_gemv_res", "k_pf_ffn13", "k_pf_cls_w16"}, sorted(p)
    finally:
        m.close()
    m = _model(tied_img, TIED, W16, passes="1")
    try:
        assert m.w16_pass_info() == {"classes": DEFAULT}
    finally:
        m.close()
    m = _model(tied_img, TIED, passes="0x1f")  # the hook does not switch the copy on
    try:
        assert m.w16_info()["state"] == 0 and m.w16_pass_info() == {"classes": []}
    finally:
        m.close()


def test_inexact_and_int8_images_launch_what_they_launch_today(gpu):
    plain = binfmt.synth_image(TIED, seed=4242, device=gpu, final_norm_std=1.0)
    torch.cuda.synchronize()
    q8 = _spec(512, 1408, 8, 8, 501, INTER, L, "w16-q8", quant=True)
    qimg = binfmt.synth_image(q8, seed=7, device=gpu)
    torch.cuda.synchronize()
    for img, spec, state in ((plain, TIED, -1), (qimg, q8, 0)):
        m0, m1 = _model(img, spec), _model(img, spec, W16, passes="0x1f")
        try:
            assert m1.w16_info()["state"] == state and m1.w16_pass_info() == {"classes": []}
            p0, d0 = _logged_passes(m0, spec)
            p1, d1 = _logged_passes(m1, spec)
            assert p0 == p1 == FP32_STEMS, (sorted(p0), sorted(p1))
            assert d0 == d1 and not d1 & DECODE_W16, sorted(d1)
        finally:
            m0.close()
            m1.close()


# ---- 2. bit identity under forced shapes ------------------------------------------------------
def _shapes(spec):
    """{hook suffix: (split, u, grid, wg)}: per workgroup width the three split combinations that walk every split
    each pass kernel has (qkv: 1, 2; wo / w2: 1, 2, 4; ffn13 / cls: 1), grids of one pair per wave; then one shape with
    small odd grids.  u is the decode kernels' own (a pass does not read it)."""
    pairs = {"QKV": (spec.dim + 2 * spec.kv_dim) // 2, "WO": spec.dim // 2, "FFN": spec.hidden_dim,
             "W2": spec.dim // 2, "CLS": (spec.vocab_size + 1) // 2}
    out = []
    for wg in (256, 512):
        for q, wo, w2 in ((1, 1, 1), (2, 2, 2), (1, 4, 4)):
            sp = {"QKV": q, "WO": wo, "FFN": 1, "W2": w2, "CLS": 1}
            out.append({k: (sp[k], 4, min(1024, -(-pairs[k] // ((wg // 64) // sp[k]))), wg) for k in pairs})
    out.append({k: (s[0], s[1], g, s[3]) for (k, s), g in zip(out[4].items(), (3, 5, 2, 7, 1))})
    return out


def _set_shape_hooks(sh):
    for k in ("QKV", "WO", "FFN", "W2", "CLS"):
        _ffi.debug_set(f"KH_SHAPE_{k}", ",".join(map(str, sh[k])) if k in sh else None)


def _dump(m, spec):
    """the whole cache as raw words: [layer, K / V, row, kv_dim]"""
    return np.stack([np.stack(m.read_kv(layer, 0, CACHE)) for layer in range(spec.n_layers)]).view(np.uint32)


class _Pair:
    """the flag-off and the flag-on model of one shape, driven through the same calls"""

    def __init__(self, m0, m1, spec, what):
        self.ms, self.spec, self.what = (m0, m1), spec, what
        self.before = [_dump(m, spec) for m in self.ms]
        assert np.array_equal(self.before[0], self.before[1]), f"{what}: the caches differ before the first call"

    def call(self, name, fn, owned):
        """fn(model) -> bytes on both models; the results, the whole caches and every row outside `owned` (against
        what it held before the call) must be equal"""
        res = [fn(m) for m in self.ms]
        assert res[0] == res[1], f"{self.what} {name}: results differ"
        after = [_dump(m, self.spec) for m in self.ms]
        bad = np.flatnonzero((after[0] != after[1]).any(axis=(0, 1, 3)))
        assert bad.size == 0, f"{self.what} {name}: K/V rows differ: {bad[:8]}"
        other = np.ones(CACHE, bool)
        other[list(owned)] = False
        for i in (0, 1):
            assert np.array_equal(after[i][:, :, other], self.before[i][:, :, other]), \
                f"{self.what} {name}: model {i} wrote a row the call does not own"
            assert not np.array_equal(after[i][:, :, ~other], self.before[i][:, :, ~other]), \
                f"{self.what} {name}: model {i} left its own rows as they were"
        self.before = after
        return res[0]


def _run_shape(m0, m1, spec, width, what, rng_seed):
    rng = np.random.default_rng(rng_seed)
    tok = lambda n: [int(t) for t in rng.integers(0, spec.vocab_size, n)]  # noqa: E731
    rows = rng.standard_normal((spec.n_layers, 2, CACHE, spec.kv_dim), dtype=np.float32)
    rows[:, 0, rng.integers(0, CACHE, 16)] *= 6.0  # a few dominant keys: the splits' maxima differ
    for m in (m0, m1):
        for layer in range(spec.n_layers):
            m.write_kv(layer, 0, rows[layer, 0], rows[layer, 1])
    p = _Pair(m0, m1, spec, what)
    none = lambda fn: (lambda m: fn(m) or b"")  # noqa: E731
    for n in (1, width, 2 * width + 1):
        t = tok(n)
        p.call(f"prefill {n}", none(lambda m: m.prefill(t, 0)), range(n))
    t = tok(width)
    p.call("prefill at 250", none(lambda m: m.prefill(t, 250)), range(250, 250 + width))
    t = tok(width)  # a pass that crosses position 256 whatever the width is
    p.call("prefill across 256", none(lambda m: m.prefill(t, 257 - width)), range(257 - width, 257))
    # verify at 300: the greedy chain of a predict loop, then a first wrong draft in the middle
    k = (width - 1) // 2
    t0 = tok(1)[0]
    chains = []
    for m in (m0, m1):
        c, cur = [], t0
        for i in range(k + 1):
            cur = m.predict(cur, 300 + i, exec="fused")
            c.append(cur)
        chains.append(c)
    assert chains[0] == chains[1], f"{what}: the predict loops differ"
    p.before = [_dump(m, spec) for m in p.ms]
    chain = chains[0]
    drafts = [t0] + chain[:k] + [(chain[k] + 1) % spec.vocab_size] + tok(width - k - 2)
    assert len(drafts) == width

    def verify(m):
        nxt, acc = m.verify(drafts, 300)
        assert acc == k and list(nxt[:k + 1]) == chain, f"{what}: verify accepted {acc} of {k}"
        return nxt.tobytes() + bytes([acc])

    # rows 300 .. 300 + k hold the predict loop's values already: the pass rewrites them with the same bits
    p.call("verify", verify, range(300 + k + 1, 300 + width))
    t = tok(width + 1)

    def score(m):
        m.set_logprobs(5)
        rec = m.score(t, 600)
        assert np.isfinite(rec["logprob"][:-1]).all(), f"{what}: score log-probs not finite"
        return _rec_bytes(rec)

    p.call("score", score, range(600, 600 + width + 1))
    slots = [int(s) for s in rng.permutation(8)[:width]]
    pos = [0, 5, 17, 100, 3, 64, 127, 31][:width]
    t = tok(width)

    def seq_step(m):
        assert m.seq_slots(8) == CACHE // 8 and m.seq_width() == width
        picks = m.seq_step(slots, t, pos, logprobs=5)
        recs = b"".join(_rec_bytes(m.seq_logprobs(s, q, 1)) for s, q in zip(slots, pos))
        return np.asarray(picks, np.int32).tobytes() + recs

    p.call("seq_step", seq_step, [s * (CACHE // 8) + q for s, q in zip(slots, pos)])


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_bit_identity_under_forced_shapes(gpu, name):
    spec, width = GEOMETRIES[name], WIDTH[name]
    img = _rounded(spec, gpu)
    assert binfmt.matrices_bf16_exact(img, spec)
    launched, n_ran = set(), 0
    try:
        for i, sh in enumerate(_shapes(spec)):
            what = f"{name} shape {i} {sh}"
            _set_shape_hooks(sh)
            m0, m1 = _model(img, spec), _model(img, spec, W16, passes="0x1f")
            try:
                assert m1.w16_info()["state"] == 1 and m1.w16_pass_info() == {"classes": ALL}, what
                try:
                    assert m1.verify_width() == width == m0.verify_width(), what
                except _ffi.KhError as e:
                    assert e.code == _ffi.KH_ERR_UNSUPPORTED, e  # the shape is outside prefill_supported
                    continue
                _ffi.debug_set("KH_LAUNCH_LOG", "1")  # after creation; m0 logs into it too: only _w16 names are kept
                _run_shape(m0, m1, spec, width, what, 7 + i)
                log = _ffi.launch_log()
                _ffi.debug_set("KH_LAUNCH_LOG", None)
                launched |= {k for k in log if k.split("<")[0] in STEMS}
                n_ran += 1
            finally:
                m0.close()
                m1.close()
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        _set_shape_hooks({})
    assert n_ran >= 4, f"{name}: only {n_ran} shapes ran the B-token pass"
    _LAUNCHED[name] = launched
    print(f"{name}: {n_ran} of {len(_shapes(spec))} shapes, {len(launched)} W16 pass instantiations launched")


def test_a_flag_on_pass_launches_no_fp32_twin_under_forced_shapes(gpu, tied_img):
    """the log of test 2 is shared by its two models; here the flag-on model runs alone"""
    try:
        _set_shape_hooks(_shapes(TIED)[1])
        m = _model(tied_img, TIED, W16, passes="0x1f")
        try:
            p, _ = _logged_passes(m, TIED)
            assert p == STEMS, sorted(p)
        finally:
            m.close()
    finally:
        _set_shape_hooks({})


# ---- 3. the copy is what is read --------------------------------------------------------------
def test_the_copy_is_what_is_read(gpu):
    spec = QWEN
    names = {f"{n}.1" for n in ("wq", "wk", "wv", "wo", "w1", "w2", "w3")} | {"wcls"}

    def poison(img):
        hit = 0
        for e in binfmt.layout(spec)[0]:
            if e.name in names:
                binfmt.tensor_from_image(img, e).fill_(float("nan"))
                hit += 1
        assert hit == len(names)
        torch.cuda.synchronize()

    rng = np.random.default_rng(5)
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, 9)]
    prompts = [toks[:1], toks[2:5], toks[4:9]]
    for flags in (W16, 0):
        img = _rounded(spec, gpu)
        assert (img.data_ptr() + spec.header_bytes()) % 16 == 0  # from_device_image uses the image in place
        m = _model(img, spec, flags, passes="0x1f")
        try:
            m.seq_slots(4)
            w0, _ = m.generate_batch(prompts, [12, 10, 14])
            m.set_logprobs(5)
            r0 = m.score(toks, 0)
            assert np.isfinite(r0["logprob"][:-1]).all()
            poison(img)
            r1 = m.score(toks, 0)
            if flags:
                assert _rec_bytes(r0) == _rec_bytes(r1)
                m.set_logprobs(None)
                w1, _ = m.generate_batch(prompts, [12, 10, 14])
                assert w0 == w1 and all(w0)
            else:  # the check of this test: the poison is in what a flag-off model streams
                assert np.isnan(r1["logprob"][:-1]).all()
        finally:
            m.close()


# ---- 4. loops ---------------------------------------------------------------------------------
def _loops(m, width, log_out):
    """every compared result of one model, as a dict"""
    rng = np.random.default_rng(21)
    ns = width + 1
    lens = [1, 2, 3, 2 * width + 1]
    prompts = [[int(t) for t in rng.integers(0, TIED.vocab_size, lens[s % 4])] for s in range(ns)]
    totals = [len(p) + 6 + (5 * s) % 11 for s, p in enumerate(prompts)]
    samp = [None if s == 1 else {"temperature": 0.8, "top_k": 50, "top_p": 0.95, "seed": 1000 + s} for s in range(ns)]
    r = {"prompts": prompts, "totals": totals, "samp": samp}
    assert m.seq_slots(ns) >= max(totals)
    r["batch"], _ = m.generate_batch(prompts, totals, samp)
    sampled = [w[len(p) - 1:] for w, p in zip(r["batch"], prompts)]
    pick = None
    for t in sorted(range(ns), key=lambda s: len(sampled[s])):
        for i in range(2, len(sampled[t]) - 2):
            tok = sampled[t][i]
            if tok not in sampled[t][:i] and all(tok not in sampled[s] for s in range(ns) if s != t):
                pick = (t, tok)
                break
        if pick:
            break
    assert pick, "no sequence emits a token of its own a few steps in: choose other seeds"
    r["stop"], _ = m.generate_batch(prompts, totals, samp, stop=[pick[1]])
    assert len(r["stop"][pick[0]]) < totals[pick[0]]  # that sequence left at the stop token
    assert all(len(r["stop"][s]) == totals[s] for s in range(ns) if s != pick[0])
    pen = [None if s % 3 == 0 else {"repetition": 1.3, "presence": 0.2, "frequency": 0.1, "last_n": 16}
           for s in range(ns)]
    bias = [None if s % 2 else {int(t): float(v) for t, v in zip(rng.integers(0, TIED.vocab_size, 3), (-3.0, 2.5, 4.0))}
            for s in range(ns)]
    r["ex"], _ = m.generate_batch(prompts, totals, samp, penalties=pen, logit_bias=bias, logprobs=5)
    r["ex records"] = [_rec_bytes(m.seq_logprobs(s, 0, len(w))) for s, w in enumerate(r["ex"])]
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        r["best_of"] = m.best_of(prompts[3], 4, len(prompts[3]) + 12, {"temperature": 0.8, "top_k": 50, "top_p": 0.95,
                                                                       "seed": 9}, top_n=3, share=True)
        log_out |= _stems(_ffi.launch_log())
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
    return r


def test_loops_match(gpu, tied_img):
    width = WIDTH["448-tied"]
    res, logs = {}, {}
    for flags in (EXACT, EXACT | W16):
        m = _model(tied_img, TIED, flags, passes="0x1f")
        try:
            assert m.w16_pass_info() == {"classes": ALL if flags & W16 else []}
            logs[flags] = set()
            res[flags] = _loops(m, width, logs[flags])
        finally:
            m.close()
    a, b = res[EXACT], res[EXACT | W16]
    for key in a:
        assert a[key] == b[key], f"{key}: flag off and on differ"
    assert len({tuple(w) for w in a["batch"]}) > width // 2  # the sequences wander apart
    assert "k_seq_attn_pfx" in logs[EXACT | W16] and "k_seq_qkv_w16" in logs[EXACT | W16], sorted(logs[EXACT | W16])
    assert "k_seq_qkv" not in logs[EXACT | W16] and "k_seq_qkv" in logs[EXACT]
    # generate_lookup with the truth as hint, and one sequence of the batch against a flag-on batch-1 model
    prompt = a["prompts"][3]
    total = len(prompt) + 40
    out = {}
    for flags in (EXACT, EXACT | W16):
        m = _model(tied_img, TIED, flags, passes="0x1f")
        try:
            truth, _ = m.generate(prompt, total, exec="graph")
            _ffi.debug_set("KH_LAUNCH_LOG", "1")
            words, _, stats = m.generate_lookup(prompt, total, hint=truth)
            log = _stems(_ffi.launch_log())
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            assert words == truth and stats["accepted"] > 0, stats
            if flags & W16:
                assert log & (STEMS | FP32_STEMS) == STEMS - {"k_seq_qkv_w16"}, sorted(log)
                for s in (0, 2):
                    m.set_sampling(**a["samp"][s])
                    got, _ = m.generate(a["prompts"][s], a["totals"][s], exec="graph")
                    assert got == b["batch"][s], f"sequence {s} of the batch against generate"
                m.set_sampling()
            out[flags] = (words, stats)
        finally:
            _ffi.debug_set("KH_LAUNCH_LOG", None)
            m.close()
    assert out[EXACT] == out[EXACT | W16]


# ---- 5. coverage gate -------------------------------------------------------------------------
def test_coverage_gate(gpu):
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    compiled = co.instantiations(co.code_object_notes(_ffi.LIB_PATH), STEMS)
    missing = [g for g in GEOMETRIES if g not in _LAUNCHED]
    assert not missing, f"geometries that did not run to the end (run the whole module): {missing}"
    seen = set().union(*_LAUNCHED.values())
    for stem in sorted(STEMS):
        assert any(k.split("<")[0] == stem for k in compiled), f"no {stem} instantiation in the library"
    assert seen <= compiled, f"launched but not found in the code objects: {sorted(seen - compiled)}"
    gap = compiled - seen
    print(f"{len(seen)} of {len(compiled)} compiled W16 pass instantiations launched and compared")
    assert not gap, f"compiled and never launched: {sorted(gap)}"
