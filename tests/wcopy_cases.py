"""Shared by the tests of the narrow exact weight copies - W16 (bf16), H16 (fp16) and Q4 (packed 4-bit) - and of the
decode-instantiation gate they grew from: test_w16_gpu.py, test_w16_f16_gpu.py, test_q4_gpu.py, test_w16_pass_gpu.py,
test_w16_f16_pass_gpu.py, test_decode_instantiations_gpu.py and, for the stem tables, the CPU modules test_w16.py,
test_w16_f16.py, test_q4.py and test_w16_pass.py.

Plain functions with explicit arguments: the geometries and stem tables, the hooks, the forced launch shapes, the
teacher-forced step loop and the comparison of two models over it, the exact image of a source, the B-token call
sequence of the pass tests, the generate loops and the coverage gate.  What only one source needs stays in its
module."""
import contextlib
import itertools

import numpy as np
import torch

import code_objects as co
from kuiperllama_amd import _ffi, binfmt, build

# ---- geometries -------------------------------------------------------------------------------
CACHE = 1024
DEEP_POS = 300  # 2 (head size 64) or 3 (128) attention time splits: k_wo_comb merges them where it can
L, Q2 = binfmt.FAMILY_LLAMA, binfmt.FAMILY_QWEN2
HALF, INTER = binfmt.ROPE_HALF, binfmt.ROPE_INTERLEAVED


def spec(dim, hidden, heads, kv_heads, vocab, quant, group, rope, family, name, tied=False):
    """2 layers, CACHE rows; theta and eps follow the family"""
    q = family == Q2
    return binfmt.ModelSpec(dim, hidden, 2, heads, kv_heads, vocab, CACHE, tied, family, quant, group, rope,
                            1000000.0 if q else 10000.0, 1e-6 if q else 1e-5, name)


# the fp32 geometries of the 16-bit copies (decode: w2 staging depths 6 / 0 and 4 / 0; passes: tokens per pass in WIDTH)
GEOMETRIES_F32 = {
    "1152-h10368": spec(1152, 10368, 18, 6, 1001, False, 64, HALF, L, "w16-1152"),      # w2 depth 6 / 0; 2 tokens
    "4224-h3072": spec(4224, 3072, 33, 3, 777, False, 64, INTER, L, "w16-4224"),        # hs 128, depth 4 / 0
    "qwen-960-hs80": spec(960, 1600, 12, 2, 1537, False, 64, HALF, Q2, "w16-qwen"),     # bias, 240 units: masked lanes
    "448-tied": spec(448, 1216, 7, 7, 999, False, 64, INTER, L, "w16-tied", tied=True),  # the copy of tok_emb
}
WIDTH = {"1152-h10368": 8, "4224-h3072": 4, "qwen-960-hs80": 8, "448-tied": 8}  # tokens per B-token pass
TIED = GEOMETRIES_F32["448-tied"]
QWEN = GEOMETRIES_F32["qwen-960-hs80"]

# ---- stems ------------------------------------------------------------------------------------
MATRICES = ("wq", "wk", "wv", "wo", "w1", "w2", "w3")  # per layer, in tensor-index order
LAYER1 = {f"{n}.1" for n in MATRICES}
DECODE_F32 = {"k_qkv", "k_gemv_res", "k_wo_comb", "k_ffn13", "k_cls"}  # what streams an fp32 image
DECODE_INT8 = DECODE_F32 | {"k_ffn13_ring", "k_cls_ring"}               # ... an int8 image
PASS_F32 = {"k_pf_qkv", "k_seq_qkv", "k_pf_ffn13", "k_pf_gemv_res", "k_pf_cls"}
DECODE = {src: {f"{s}_{src}" for s in DECODE_F32} for src in ("w16", "h16", "q4")}  # the five stems on a copy
PASS = {src: {f"{s}_{src}" for s in PASS_F32} for src in ("w16", "h16")}
# the decode GEMV launches of one fused step at position 0 of the 448-tied geometry under its heuristic shapes
# (qkv / wo / ffn13: u 2, 256 threads, staging depth 1; w2: u 4, 512 threads; cls: u 2, 512 threads; no split)
TIED_STEP_F32 = {"k_qkv<false,2,1,1>", "k_gemv_res<false,2,1,1>", "k_ffn13<false,2,1>", "k_gemv_res<false,4,1,1>",
                 "k_cls<false,2,1>"}
TIED_STEP = {src: {f"k_qkv_{src}<2,1,1>", f"k_gemv_res_{src}<2,1,1>", f"k_ffn13_{src}<2,1>",
                   f"k_gemv_res_{src}<4,1,1>", f"k_cls_{src}<2,1>"} for src in ("w16", "h16")}
# the compiled pass kernels (test_w16_pass.py, test_w16_f16.py): the _w16 products of the fp32 lists ...
PASS_W16_COMPILED = {
    "k_pf_qkv_w16": {f"k_pf_qkv_w16<{sp},{b}>" for sp in (2, 1) for b in (8, 4)},
    "k_seq_qkv_w16": {f"k_seq_qkv_w16<{sp},{b}>" for sp in (2, 1) for b in (8, 4)},
    "k_pf_ffn13_w16": {f"k_pf_ffn13_w16<{b}>" for b in (8, 4)},
    "k_pf_gemv_res_w16": {f"k_pf_gemv_res_w16<{sp},{b}>" for sp in (4, 2, 1) for b in (8, 4, 2)},
    "k_pf_cls_w16": {f"k_pf_cls_w16<{b}>" for b in (8, 4)},
}
# ... and what the parent of the W16 passes compiled for the kernels whose bodies became templates over the matrix view
PASS_COMPILED_BEFORE = {
    "k_pf_qkv": {"k_pf_qkv<false,1,4>", "k_pf_qkv<false,1,8>", "k_pf_qkv<false,2,4>", "k_pf_qkv<false,2,8>",
                 "k_pf_qkv<true,1,4>", "k_pf_qkv<true,2,4>"},
    "k_seq_qkv": {"k_seq_qkv<false,1,4>", "k_seq_qkv<false,1,8>", "k_seq_qkv<false,2,4>", "k_seq_qkv<false,2,8>",
                  "k_seq_qkv<true,1,4>", "k_seq_qkv<true,2,4>"},
    "k_pf_ffn13": {"k_pf_ffn13<false,4>", "k_pf_ffn13<false,8>", "k_pf_ffn13<true,4>"},
    "k_pf_gemv_res": {"k_pf_gemv_res<false,1,2>", "k_pf_gemv_res<false,1,4>", "k_pf_gemv_res<false,1,8>",
                      "k_pf_gemv_res<false,2,2>", "k_pf_gemv_res<false,2,4>", "k_pf_gemv_res<false,2,8>",
                      "k_pf_gemv_res<false,4,2>", "k_pf_gemv_res<false,4,4>", "k_pf_gemv_res<false,4,8>",
                      "k_pf_gemv_res<true,1,2>", "k_pf_gemv_res<true,1,4>", "k_pf_gemv_res<true,2,2>",
                      "k_pf_gemv_res<true,2,4>", "k_pf_gemv_res<true,4,2>", "k_pf_gemv_res<true,4,4>"},
    "k_pf_cls": {"k_pf_cls<false,4>", "k_pf_cls<false,8>", "k_pf_cls<true,4>"},
}


def stem(k):
    return k.split("<")[0]


def stems(log):
    return {stem(k) for k in log}


# ---- hooks ------------------------------------------------------------------------------------
@contextlib.contextmanager
def hook(key, value):
    _ffi.debug_set(key, value)
    try:
        yield
    finally:
        _ffi.debug_set(key, None)


@contextlib.contextmanager
def launch_log():
    """`with launch_log() as read:` starts an empty launch log; read() is what was launched since.  Setting
    KH_LAUNCH_LOG to "1" again inside empties the log."""
    with hook("KH_LAUNCH_LOG", "1"):
        yield _ffi.launch_log


# ---- forced shapes ----------------------------------------------------------------------------
def pairs(spec):
    """Work items (row pairs; ffn13: rows of w1/w3) of qkv, wo, ffn13, w2, cls: pick_shape's `pairs`."""
    return {"QKV": (spec.dim + 2 * spec.kv_dim) // 2, "WO": spec.dim // 2, "FFN": spec.hidden_dim,
            "W2": spec.dim // 2, "CLS": (spec.vocab_size + 1) // 2}


def decode_shapes(spec, second_odd_grids=(3, 5, 2, 7, 1), ring_shape=False):
    """Forced decode shapes of one geometry: a list of {hook suffix: (split, u, grid, wg)}.  For each workgroup width,
    nine shapes walk every (u, split) each kernel accepts (qkv: split <= 2, ffn13 / cls: 1; fp32 u 2, 4, 8, int8 u 2, 4
    and for w2 also 3).  Grid: one pair per wave, at most 1024 workgroups.  Then shapes 0 and 13 with only the grids
    changed to small odd ones, and with ring_shape one shape without the ffn13 / cls hooks (the int8 ring kernels take
    those launches)."""
    us = (2, 4) if spec.quant else (2, 4, 8)
    combos = {"QKV": list(itertools.product(us, (1, 2))), "WO": list(itertools.product(us, (1, 2, 4))),
              "FFN": list(itertools.product(us, (1,))), "CLS": list(itertools.product(us, (1,))),
              "W2": list(itertools.product((2, 3, 4) if spec.quant else us, (1, 2, 4)))}
    n = pairs(spec)
    out = []
    for wg in (256, 512):
        for i in range(9):
            sh = {}
            for k, c in combos.items():
                u, sp = c[i % len(c)]
                sh[k] = (sp, u, min(1024, -(-n[k] // ((wg // 64) // sp))), wg)
            out.append(sh)
    for base, grids in ((0, (3, 5, 2, 7, 1)), (13, second_odd_grids)):
        out.append({k: (s[0], s[1], g, s[3]) for (k, s), g in zip(out[base].items(), grids)})
    if ring_shape:
        out.append({k: v for k, v in out[4].items() if k not in ("FFN", "CLS")})
    return out


def pass_shapes(spec):
    """{hook suffix: (split, u, grid, wg)}: per workgroup width the three split combinations that walk every split
    each pass kernel has (qkv: 1, 2; wo / w2: 1, 2, 4; ffn13 / cls: 1), grids of one pair per wave; then one shape with
    small odd grids.  u is the decode kernels' own (a pass does not read it)."""
    n = pairs(spec)
    out = []
    for wg in (256, 512):
        for q, wo, w2 in ((1, 1, 1), (2, 2, 2), (1, 4, 4)):
            sp = {"QKV": q, "WO": wo, "FFN": 1, "W2": w2, "CLS": 1}
            out.append({k: (sp[k], 4, min(1024, -(-n[k] // ((wg // 64) // sp[k]))), wg) for k in n})
    out.append({k: (s[0], s[1], g, s[3]) for (k, s), g in zip(out[4].items(), (3, 5, 2, 7, 1))})
    return out


def set_shape_hooks(sh):
    for k in ("QKV", "WO", "FFN", "W2", "CLS"):
        _ffi.debug_set(f"KH_SHAPE_{k}", ",".join(map(str, sh[k])) if k in sh else None)


# ---- images and models ------------------------------------------------------------------------
_MAKE_EXACT = {"w16": binfmt.round_matrices_bf16, "h16": binfmt.round_matrices_fp16,
               "q4": binfmt.requantize_matrices_q4}


def _plant(img, spec):
    """-8, 7 and -1 in low (even column) and high (odd column) nibbles of the first and the last 16-column unit of the
    first two rows and the last row of every covered tensor"""
    pat = torch.tensor([-8, 7, -1, -8, 7, -8, -1, 7, -1, -1, 7, 7, -8, -8, 7, -1], dtype=torch.int8, device=img.device)
    for e, _ in binfmt.q4_tensors(spec):
        q = binfmt.tensor_from_image(img, e)
        for r in (0, 1, e.shape[0] - 1):
            q[r, :16] = pat
            q[r, -16:] = pat.flip(0)


def exact_image(source, spec, gpu, seed=4242, plant=False):
    """synth_image(final_norm_std=1.0) made exact for the source's copy: matrices rounded to bf16 ("w16") or fp16
    ("h16"), or requantised to 4 bits ("q4", plant: with the edge nibbles of _plant)"""
    img = binfmt.synth_image(spec, seed=seed, device=gpu, final_norm_std=1.0)
    _MAKE_EXACT[source](img, spec)
    if plant:
        _plant(img, spec)
    torch.cuda.synchronize()
    return img


def model(img, spec, flags=0, passes=None, q4_classes=None):
    """passes / q4_classes: the values of the hooks KH_W16_PASS / KH_Q4_CLASSES while the model is created (None: the
    hook is left as the caller has it)"""
    from kuiperllama_amd.model import KuiperModel
    with contextlib.ExitStack() as hooks:
        for key, value in (("KH_W16_PASS", passes), ("KH_Q4_CLASSES", q4_classes)):
            if value is not None:
                hooks.enter_context(hook(key, value))
        return KuiperModel.from_device_image(img, spec, flags=flags)


def planned_w16_bytes(spec):
    return _ffi.plan_w16(spec.dim, spec.hidden_dim, spec.kv_dim, spec.vocab_size, spec.n_layers, spec.quant)["bytes"]


def poison_layer1(img, spec, names, value):
    """fill the tensors `names` of the image (LAYER1: the matrices of layer 1; the scales of an int8 image stay)"""
    hit = 0
    for e in binfmt.layout(spec)[0]:
        if e.name in names:
            binfmt.tensor_from_image(img, e).fill_(value)
            hit += 1
    assert hit == len(names), (hit, sorted(names))
    torch.cuda.synchronize()


def rec_bytes(rec):
    return b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in ("token", "logprob", "top_ids", "top_logprobs"))


# ---- logged calls -----------------------------------------------------------------------------
def logged_step(m, keep, tok=5, pos=0):
    """(launches of one fused step whose stem is in `keep`, logits)"""
    with launch_log() as read:
        m.predict(tok, pos, exec="fused")
        lg = m.logits()
        return {k for k in read() if stem(k) in keep}, lg


def logged_passes(m, spec, keep):
    """(stems in `keep` of the launches of a prefill of 3 tokens, a score of 9 and a seq_step of 3 lanes; stems a
    predict launched)"""
    toks = [int(t) for t in np.random.default_rng(3).integers(0, spec.vocab_size, 9)]
    with launch_log() as read:
        m.prefill(toks[:3], 0)
        m.set_logprobs(5)
        m.score(toks, 0)
        m.set_logprobs(None)
        m.seq_slots(4)
        m.seq_step([2, 0, 3], toks[:3], [0, 4, 1])
        passes = stems(read()) & keep
        _ffi.debug_set("KH_LAUNCH_LOG", "1")  # an empty log
        m.predict(5, 0, exec="fused")
        return passes, stems(read())


# ---- teacher-forced decode steps --------------------------------------------------------------
def steps(spec, rng):
    toks = [int(t) for t in rng.integers(0, spec.vocab_size, 4)]
    return list(zip(toks, (0, 1, 2, DEEP_POS)))


def deep_rows(spec, rng):
    kr = rng.standard_normal((spec.n_layers, DEEP_POS, spec.kv_dim), dtype=np.float32)
    vr = rng.standard_normal((spec.n_layers, DEEP_POS, spec.kv_dim), dtype=np.float32)
    kr[:, rng.integers(0, DEEP_POS, 8)] *= 6.0  # a few dominant keys: the splits' maxima differ
    return kr, vr


def run_steps(m, spec, steps, rows, check=None):
    """teacher-forced steps into NaN rows (at DEEP_POS: behind `rows`) -> [(logits, K rows [layers, kv], V rows,
    token)], floats as raw words; check(i, tok, pos, token, logits, K rows, V rows) sees the floats of step i"""
    nan = np.full((1, spec.kv_dim), np.nan, np.float32)
    res = []
    for i, (tok, pos) in enumerate(steps):
        if pos == DEEP_POS:
            for layer in range(spec.n_layers):
                m.write_kv(layer, 0, rows[0][layer], rows[1][layer])
        for layer in range(spec.n_layers):
            m.write_kv(layer, pos, nan, nan)
        nxt = m.predict(tok, pos, exec="fused")
        lg = m.logits()
        kv = [m.read_kv(layer, pos, 1) for layer in range(spec.n_layers)]
        ks, vs = np.stack([k[0] for k, _ in kv]), np.stack([v[0] for _, v in kv])
        if check:
            check(i, tok, pos, nxt, lg, ks, vs)
        res.append((lg.view(np.uint32), ks.view(np.uint32), vs.view(np.uint32), nxt))
    return res


def compare_steps(m0, m1, spec, steps, rows, what, only_stems, keep_stems):
    """the teacher-forced steps on the image-streaming model m0 and the copy-streaming m1: equal words and tokens, and
    of the stems in `keep_stems` m1 launched `only_stems` alone -> (those launches, m0's results, m1's)"""
    want = run_steps(m0, spec, steps, rows)
    with launch_log() as read:  # after creation: the self-check's launches are not compared ones
        got = run_steps(m1, spec, steps, rows)
        log = {k for k in read() if stem(k) in keep_stems}
    assert log and all(stem(k) in only_stems for k in log), f"{what}: a GEMV off the copy was launched: {sorted(log)}"
    for (tok, pos), (la, ka, va, ta), (lb, kb, vb, tb) in zip(steps, want, got):
        assert not np.isnan(la.view(np.float32)).any(), f"{what} pos {pos}: NaN logits"
        assert np.array_equal(la, lb), f"{what} pos {pos}: logits differ in {int((la != lb).sum())} words"
        assert np.array_equal(ka, kb) and np.array_equal(va, vb), f"{what} pos {pos}: K/V rows differ"
        assert ta == tb, f"{what} pos {pos}: token {ta} vs {tb}"
    return log, want, got


# ---- the B-token calls of a pass model --------------------------------------------------------
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


def run_pass_shape(m0, m1, spec, width, what, rng_seed):
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
        return rec_bytes(rec)

    p.call("score", score, range(600, 600 + width + 1))
    slots = [int(s) for s in rng.permutation(8)[:width]]
    pos = [0, 5, 17, 100, 3, 64, 127, 31][:width]
    t = tok(width)

    def seq_step(m):
        assert m.seq_slots(8) == CACHE // 8 and m.seq_width() == width
        picks = m.seq_step(slots, t, pos, logprobs=5)
        recs = b"".join(rec_bytes(m.seq_logprobs(s, q, 1)) for s, q in zip(slots, pos))
        return np.asarray(picks, np.int32).tobytes() + recs

    p.call("seq_step", seq_step, [s * (CACHE // 8) + q for s, q in zip(slots, pos)])


def pass_loops(m, width, log_out):
    """every compared result of one model of the TIED geometry, as a dict: generate_batch (width + 1 sequences) plain,
    with a stop token and with penalties, bias and records; best_of over a shared prefix, its stems into log_out"""
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
    r["ex records"] = [rec_bytes(m.seq_logprobs(s, 0, len(w))) for s, w in enumerate(r["ex"])]
    with launch_log() as read:
        r["best_of"] = m.best_of(prompts[3], 4, len(prompts[3]) + 12, {"temperature": 0.8, "top_k": 50, "top_p": 0.95,
                                                                       "seed": 9}, top_n=3, share=True)
        log_out |= stems(read())
    return r


# ---- the batch-1 generate loops ---------------------------------------------------------------
def loop_prompt(spec, rng=None):
    """the 250 tokens generate_loops starts from (the modules' oracle anchors use the first two)"""
    rng = rng or np.random.default_rng(11)
    return [int(t) for t in rng.integers(0, spec.vocab_size, 250)]


def generate_loops(m):
    """greedy and sampled (penalties, a logit bias, log-probs) words of exec graph and fused across positions 250 ..
    270, and the records' bytes, as a dict.  Leaves the sampler, penalties, bias and records set."""
    rng = np.random.default_rng(11)
    prompt = loop_prompt(m.spec, rng)  # sampled steps at positions 249 .. 270
    total = 272
    bias = dict(zip((int(t) for t in rng.integers(0, m.spec.vocab_size, 6)), (-3.0, 2.5, -np.inf, 1.0, -1.5, 4.0)))
    r = {}
    for ex in ("graph", "fused"):
        r["greedy", ex] = m.generate(prompt, total, exec=ex)[0]  # the screened tail, as it is
    m.set_sampling(temperature=0.8, top_k=50, top_p=0.95, seed=17)
    m.set_penalties(repetition=1.3, presence=0.2, frequency=0.1, last_n=64)
    m.set_logit_bias(bias)
    m.set_logprobs(5)
    for ex in ("graph", "fused"):
        r["sampled", ex] = m.generate(prompt, total, exec=ex)[0]
        r["records", ex] = rec_bytes(m.logprobs(248, 24))
    return r


def assert_loops_equal(a, b):
    """a: the flag-off model's generate_loops (plus whatever its module added), b: the flag-on model's"""
    assert len(a["greedy", "graph"]) > 256 and len(a["sampled", "graph"]) > 256  # the runs cross position 256
    for key in a:
        assert a[key] == b[key], f"{key}: flag off and on differ"
    assert a["sampled", "graph"] == a["sampled", "fused"] and a["records", "graph"] == a["records", "fused"]
    assert len(set(a["sampled", "graph"][-20:])) > 4  # the run wanders: equality is not that of one repeated token


# ---- coverage gate ----------------------------------------------------------------------------
def coverage_gate(stems, geometries, launched, label):
    """every compiled instantiation of `stems` is in `launched` ({geometry: names}, filled by the module's
    bit-identity test), and every launched name is in the code objects -> the compiled set"""
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    compiled = co.instantiations(co.code_object_notes(_ffi.LIB_PATH), stems)
    missing = [g for g in geometries if g not in launched]
    assert not missing, f"geometries that did not run to the end (run the whole module): {missing}"
    seen = set().union(*launched.values())
    for s in sorted(stems):
        assert any(stem(k) == s for k in compiled), f"no {s} instantiation in the library"
    assert seen <= compiled, f"launched but not found in the code objects: {sorted(seen - compiled)}"
    gap = compiled - seen
    print(f"{len(seen)} of {len(compiled)} compiled {label} instantiations launched and compared")
    assert not gap, f"compiled and never launched: {sorted(gap)}"
    return compiled
