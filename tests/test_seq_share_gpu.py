"""A prompt prefix shared between sequence slots on the GPU: kh_model_seq_slots_var / _share / _row, and the passes,
prefill and batched loop over slots that read positions [0, P) from another slot's rows (csrc/kh_attn.h:
k_seq_attn_pfx; csrc/kh_model_seq.hip).

Every comparison is EXACT, as in tests/test_seq_gpu.py: token ids as integers, K/V rows and log-prob records as raw
bytes.  The reference is a batch-1 twin of the same image and the same cache length (so the split counts agree): a
fused predict loop for single passes, its prefill (KH_FLAG_PREFILL_EXACT) and its generate() for the loop; the loop is
also held against the same call on a FORKED layout (copies of the prompt rows) of a second model.  k_seq_attn_pfx is
k_seq_attn with another row address for the timesteps below P, so a differing byte is a bug.

Models: score_cases (a) fp32 GQA (head size 64: split quantum 256) and (b) int8 with caches of up to 640 rows, and the
small geometries tests/test_seq_gpu.py uses to reach every (G, KVM), among them head size 128 (quantum 128)."""
import dataclasses

import numpy as np
import pytest
import torch

import code_objects as co
import score_cases as S
from kuiperllama_amd import _ffi, binfmt, build
from kuiperllama_amd.model import KuiperModel, plan_shared_layout

pytestmark = pytest.mark.gpu

EXACT = _ffi.KH_FLAG_PREFILL_EXACT
SAMP = {"temperature": 0.8, "top_k": 50, "top_p": 0.95}
REC = ("token", "logprob", "top_ids", "top_logprobs")
STEM = "k_seq_attn_pfx"
CACHE = 640
_LAUNCHED = set()


@pytest.fixture(autouse=True)
def _launch_log():
    """every test of this file runs with the launch log on; what it launched is kept for the gate"""
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        yield
    finally:
        _LAUNCHED.update(_ffi.launch_log())
        _ffi.debug_set("KH_LAUNCH_LOG", None)


def _new_log():
    _LAUNCHED.update(_ffi.launch_log())
    _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log


_IMG = {}


def _image(gpu, which, seq_len=CACHE):
    spec = dataclasses.replace(S.SPECS[which] if isinstance(which, str) else which, seq_len=seq_len)
    key = (spec.name, spec.seq_len)
    if key not in _IMG:
        _IMG[key] = (spec, binfmt.synth_image(spec, seed=S.SEEDS.get(which, 13) if isinstance(which, str) else 13,
                                              device=gpu))
        torch.cuda.synchronize()
    return _IMG[key]


def _mk(spec, img, **kw):
    return KuiperModel.from_device_image(img, spec, max_seq_len=spec.seq_len, **kw)


def _sampling(seed):
    return dict(SAMP, seed=seed)


def _geometry(dim, heads, kv_heads, name):
    return binfmt.ModelSpec(dim, 512, 2, heads, kv_heads, 2048, 64, True, binfmt.FAMILY_LLAMA, False, 64,
                            binfmt.ROPE_HALF, 500000.0, 1e-5, name)


def _code(call):
    with pytest.raises(_ffi.KhError) as ei:
        call()
    return ei.value.code


# ---- 1, 2. single passes ---------------------------------------------------------------------------------------------
N_TXT = 304   # the long text: the parent holds all of it, its own lane sits at its last position
POS_FAR = 300  # a sharer's lane well behind every P: two per-head splits at quantum 256, three at 128
N_SHORT = 8   # the slot that shares nothing


class Loop:
    """a batch-1 twin after a fused predict loop over `text`: G[p] its greedy picks, KV[layer] the rows it left;
    sampled(p, sp): its pick at position p under a sampler (the rows of the loop are still in its cache)"""

    def __init__(self, spec, img, text):
        self.text, self.twin = text, _mk(spec, img)
        self.G = [self.twin.predict(t, p, exec="fused") for p, t in enumerate(text)]
        self.KV = [self.twin.read_kv(layer, 0, len(text)) for layer in range(spec.n_layers)]

    def sampled(self, p, sp):
        self.twin.set_sampling(**sp)
        tok = self.twin.predict(self.text[p], p, exec="fused")
        self.twin.set_sampling()
        return tok


# (geometry, hooks read at creation, shared lengths, the instantiations the passes must launch)
PQ256 = [1, 7, 200, 255, 256, 257, 270]  # inside split 0, on the boundary, inside split 1; P = pos: only the own token
PQ128 = [127, 128, 129]
TL = {"KH_ATTN_TLONG": "8"}  # the GQA group path from position 7 on: one group split below 256, two from there
SINGLE = [
    ("a", {}, PQ256, {"k_seq_attn_pfx<16,0>"}),
    (_geometry(512, 4, 2, "seq-32-2"), {}, PQ128, {"k_seq_attn_pfx<32,0>"}),
    ("a", TL, PQ256[1:], {"k_seq_attn_pfx<16,2>"}),
    (_geometry(512, 4, 2, "seq-32-2"), TL, PQ128 + [256], {"k_seq_attn_pfx<32,2>"}),
    (_geometry(256, 4, 1, "seq-16-4"), TL, [255, 256, 257], {"k_seq_attn_pfx<16,4>"}),
    (_geometry(448, 7, 1, "seq-16-7"), TL, [255, 256, 257], {"k_seq_attn_pfx<16,7>"}),
    (_geometry(512, 8, 1, "seq-16-8"), TL, [255, 256, 257], {"k_seq_attn_pfx<16,8>"}),
    (_geometry(512, 4, 1, "seq-32-4"), TL, [255, 256, 257], {"k_seq_attn_pfx<32,4>"}),
    (_geometry(512, 2, 2, "seq-64-0"), {}, [128, 257], {"k_seq_attn_pfx<64,0>"}),
]


@pytest.mark.parametrize("case", range(len(SINGLE)))
def test_a_pass_over_sharers_is_a_predict_loop_per_lane(gpu, case):
    """per P one pass of five lanes, greedy and sampled: sharers at P (its own range holds the current token only),
    P + 1 and POS_FAR, the parent at its last position (>= every P) and a slot that shares nothing at position 5 (below
    KH_ATTN_TLONG: with the hook one launch takes both paths).  Behind P the sharers continue with ANOTHER text than
    the parent's, so a timestep read from the wrong one of the two bases is a wrong row, on either side of P."""
    which, hooks, Ps, must = SINGLE[case]
    spec, img = _image(gpu, which)
    rng = np.random.default_rng(900 + case)
    text = [int(t) for t in rng.integers(0, spec.vocab_size, N_TXT)]
    short = [int(t) for t in rng.integers(0, spec.vocab_size, N_SHORT)]
    alt = [(t + 1 + int(d)) % spec.vocab_size for t, d in zip(text, rng.integers(0, 7, N_TXT))]  # differs everywhere
    try:
        for k, v in hooks.items():
            _ffi.debug_set(k, v)  # read by kh_model_create_*: the twins are shaped by them too
        ref, ref_s = Loop(spec, img, text), Loop(spec, img, short)
        m = _mk(spec, img)
        refs = {P: Loop(spec, img, text[:P] + alt[P:]) for P in Ps}  # what a sharer of P positions continues with
    finally:
        for k in hooks:
            _ffi.debug_set(k, None)
    nl = spec.n_layers
    poison = np.full((1, spec.kv_dim), np.nan, np.float32)
    _new_log()
    for P in Ps:
        far = P + 1 < POS_FAR
        lens = [N_TXT, N_SHORT, 8, 8] + ([POS_FAR + 1 - P] if far else [])
        assert sum(lens) <= CACHE
        m.seq_slots_var(lens)
        for layer in range(nl):  # the parent's and the short slot's rows: the twins'
            m.write_kv(layer, m.seq_row(0, 0), *ref.KV[layer])
            m.write_kv(layer, m.seq_row(1, 0), *ref_s.KV[layer])
        for dst in range(2, len(lens)):
            m.seq_share(0, dst, P)
            assert [m.seq_row(dst, p) for p in (0, P - 1, P)] == [0, P - 1, sum(lens[:dst])]
        # lanes: (slot, position, reference)
        rp = refs[P]
        for layer in range(nl):  # the shared rows are the parent's, bit for bit; behind them the two texts part
            assert rp.KV[layer][0][:P].tobytes() == ref.KV[layer][0][:P].tobytes()
            assert rp.KV[layer][0][P].tobytes() != ref.KV[layer][0][P].tobytes()
        lanes = [(2, P, rp), (1, 5, ref_s), (0, N_TXT - 1, ref), (3, P + 1, rp)]
        for layer in range(nl):  # what lies between P and a lane's position: the twin's rows, at the slot's own rows
            k, v = rp.KV[layer]
            m.write_kv(layer, m.seq_row(3, P), k[P:P + 1], v[P:P + 1])
            if far:
                m.write_kv(layer, m.seq_row(4, P), k[P:POS_FAR], v[P:POS_FAR])
        if far:
            lanes.insert(0, (4, POS_FAR, rp))
        slots, pos = [ln[0] for ln in lanes], [ln[1] for ln in lanes]
        rows = [m.seq_row(s, p) for s, p in zip(slots, pos)]
        assert len(set(rows)) == len(rows) and all(r >= N_TXT for r, s in zip(rows, slots) if s >= 2)
        for samplings in (None, [_sampling(70 + i) for i in range(len(lanes))]):
            what = (spec.name, tuple(hooks), P, samplings is not None)
            for layer in range(nl):
                for r in rows:
                    m.write_kv(layer, r, poison, poison)
            before = [m.read_kv(layer, 0, CACHE) for layer in range(nl)]
            got = m.seq_step(slots, [r.text[p] for _, p, r in lanes], pos, samplings)
            want = [r.G[p] if samplings is None else r.sampled(p, samplings[i]) for i, (_, p, r) in enumerate(lanes)]
            assert got == want, what
            other = np.ones(CACHE, bool)
            other[rows] = False
            for layer in range(nl):
                k, v = m.read_kv(layer, 0, CACHE)
                for (_, p, r), row in zip(lanes, rows):
                    wk, wv = r.KV[layer]
                    assert k[row].tobytes() == wk[p].tobytes() and v[row].tobytes() == wv[p].tobytes(), \
                        what + (layer, row, p)
                bk, bv = before[layer]
                assert k[other].tobytes() == bk[other].tobytes() and v[other].tobytes() == bv[other].tobytes(), \
                    what + (layer, "a row that is no lane's was written (the parent's included)")
    log = _ffi.launch_log()
    assert must <= log and any(k.startswith("seq_attn_pfx_launch<") for k in log), (must, sorted(log))
    assert not any(k.startswith("k_seq_attn<") for k in log), sorted(log)  # every pass here had a sharer
    if hooks:
        assert any(k.startswith("seq_attn_pfx_launch<") and k.endswith(",1>") for k in log), sorted(log)  # group grid
    m.close()
    for r in [ref, ref_s] + list(refs.values()):
        r.twin.close()


# ---- 3. prefill into a sharer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,P", [("a", 250), ("b", 20), ("a", 256)])
def test_prefill_into_a_sharer_leaves_the_twins_rows(gpu, name, P):
    """a suffix of 1, width and 2 width + 1 tokens at pos0 = P (from 250: across the split boundary at 256)"""
    spec, img = _image(gpu, name)
    w = S.BATCH[name]
    rng = np.random.default_rng(950 + P)
    N = P + 2 * w + 1
    text = [int(t) for t in rng.integers(0, spec.vocab_size, N)]
    twin = _mk(spec, img, flags=EXACT)
    twin.prefill(text)
    KV = [twin.read_kv(layer, 0, N) for layer in range(spec.n_layers)]
    twin.close()
    m = _mk(spec, img)
    m.seq_slots_var([P + 8, 8, 8, 2 * w + 1])  # the slot behind the parent is not the sharer: its base is not row P
    m.seq_prefill(0, text[:P])
    for n, dst in ((1, 1), (w, 2), (2 * w + 1, 3)):
        m.seq_share(0, dst, P)
        before = [m.read_kv(layer, 0, CACHE) for layer in range(spec.n_layers)]
        _new_log()
        m.seq_prefill(dst, text[P:P + n], P)
        log = _ffi.launch_log()
        assert any(k.startswith("k_seq_attn_pfx<") for k in log) and not any(k.startswith("k_attn_decode<") for k in log), \
            sorted(log)
        r0 = m.seq_row(dst, P)
        assert r0 == m.seq_row(dst, P + n - 1) - (n - 1) and m.seq_row(dst, P - 1) == P - 1
        other = np.ones(CACHE, bool)
        other[r0:r0 + n] = False
        for layer in range(spec.n_layers):
            k, v = m.read_kv(layer, 0, CACHE)
            wk, wv = KV[layer]
            assert k[r0:r0 + n].tobytes() == wk[P:P + n].tobytes() and v[r0:r0 + n].tobytes() == wv[P:P + n].tobytes(), \
                (name, P, n, layer)
            bk, bv = before[layer]
            assert k[other].tobytes() == bk[other].tobytes() and v[other].tobytes() == bv[other].tobytes(), \
                (name, P, n, layer, "a row outside the suffix was written")
    # the parent's rows are the twin's too
    for layer in range(spec.n_layers):
        k, v = m.read_kv(layer, 0, P)
        assert k.tobytes() == KV[layer][0][:P].tobytes() and v.tobytes() == KV[layer][1][:P].tobytes()
    m.close()


# ---- 4. the loop -----------------------------------------------------------------------------------------------------
def _rec_same(got, want, what):
    for k in REC:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), what + (k,)


class LoopCase:
    """n_seq sequences: a common prefix of P tokens and a suffix of 1 .. 3 of their own, unequal totals, a setting
    each.  W / R: the twin's generate() words and records per sequence."""

    def __init__(self, spec, img, P, n_seq, extra, seed, top_n, bias, sampled, stop=()):
        rng = np.random.default_rng(seed)
        V = spec.vocab_size
        self.P, self.n, self.top_n, self.stop = P, n_seq, top_n, list(stop)
        self.prefix = [int(t) for t in rng.integers(0, V, P)]
        self.prompts = [self.prefix + [int(t) for t in rng.integers(0, V, 1 + s % 3)] for s in range(n_seq)]
        self.totals = [len(p) - 1 + extra + (5 * s) % 11 for s, p in enumerate(self.prompts)]
        self.samplings = [(_sampling(3000 + s) if sampled and s != 1 else None) for s in range(n_seq)]
        self.bias = [({int(rng.integers(0, V)): 3.0, int(rng.integers(0, V)): -np.inf} if bias and s % 2 else None)
                     for s in range(n_seq)]
        self.spec, self.img = spec, img

    def kw(self):
        kw = dict(samplings=self.samplings, stop=self.stop, cached=[self.P] * self.n)
        if self.top_n is not None or any(self.bias):
            kw.update(logit_bias=self.bias, logprobs=self.top_n)
        return kw

    def twin_run(self):
        twin = _mk(self.spec, self.img, flags=EXACT)
        self.W, self.R, self.KV = [], [], []
        for s in range(self.n):
            twin.set_sampling(**(self.samplings[s] or {}))
            twin.set_logit_bias(self.bias[s])
            twin.set_logprobs(self.top_n)
            words, _ = twin.generate(self.prompts[s], self.totals[s], exec="graph", stop=self.stop)
            self.W.append(words)
            self.R.append(twin.logprobs(0, len(words)) if self.top_n is not None and words else None)
            self.KV.append([twin.read_kv(layer, 0, max(len(words), 1)) for layer in range(self.spec.n_layers)])
        twin.close()

    def check(self, m, got, shared, what):
        assert [len(g) for g in got] == [len(w) for w in self.W], what
        for s, words in enumerate(got):
            assert words == self.W[s], what + (s,)
            if self.top_n is not None and words:
                rec = m.seq_logprobs(s, 0, len(words))
                _rec_same(rec, self.R[s], what + (s,))
                fed = min(len(self.prompts[s]) - 1, len(words))
                assert (rec["token"][:fed] == -1).all() and (rec["token"][fed:] >= 0).all(), what + (s,)
            lo = self.P if shared and s else 0  # the rows the sequence owns
            for layer in range(self.spec.n_layers):
                k, v = m.read_kv(layer, m.seq_row(s, lo), len(words) - lo)
                wk, wv = self.KV[s][layer]
                assert k.tobytes() == wk[lo:len(words)].tobytes() and v.tobytes() == wv[lo:len(words)].tobytes(), \
                    what + (s, layer)


def _shared_model(c):
    m = _mk(c.spec, c.img)
    m.seq_slots_var(plan_shared_layout(CACHE, c.n, c.P, c.totals))
    m.seq_prefill(0, c.prefix)
    for s in range(1, c.n):
        m.seq_share(0, s, c.P)
    return m


@pytest.mark.parametrize("variant", ["greedy", "sampled+bias+top5", "sampled+top0+stop"])
def test_the_loop_over_sharers_is_generate_until_and_the_forked_call(gpu, variant):
    """one parent and width - 1, width, width + 1 sharers; the same call on copies of the prefix in a second model"""
    spec, img = _image(gpu, "a")
    w = S.BATCH["a"]
    P, n_seq = 40, {"greedy": w, "sampled+bias+top5": w + 1, "sampled+top0+stop": w + 2}[variant]
    top_n = {"greedy": None, "sampled+bias+top5": 5, "sampled+top0+stop": 0}[variant]
    c = LoopCase(spec, img, P, n_seq, 6, 1200 + n_seq, top_n, bias="bias" in variant, sampled="sampled" in variant)
    c.twin_run()
    assert all(len(c.W[s]) == c.totals[s] for s in range(n_seq)) and len(set(c.totals)) > 2
    if "stop" in variant:  # a token one sequence emits a few steps in and no other does: that one ends early
        sampled = [c.W[s][len(c.prompts[s]) - 1:] for s in range(n_seq)]
        pick = next(((t, i, sampled[t][i]) for t in range(1, n_seq) for i in range(2, len(sampled[t]) - 2)
                     if sampled[t][i] not in sampled[t][:i] and all(sampled[t][i] not in p for p in c.prompts)
                     and all(sampled[t][i] not in sampled[s] for s in range(n_seq) if s != t)), None)
        assert pick, "no sequence emits a token of its own a few steps in: choose other seeds"
        c.stop = [pick[2]]
        c.twin_run()
        assert len(c.W[pick[0]]) == len(c.prompts[pick[0]]) - 1 + pick[1] < c.totals[pick[0]]
        assert all(len(c.W[s]) == c.totals[s] for s in range(n_seq) if s != pick[0])
    m = _shared_model(c)
    _new_log()
    got, ms = m.generate_batch(c.prompts, c.totals, **c.kw())
    log = _ffi.launch_log()
    assert ms > 0 and any(k.startswith("k_seq_attn_pfx<") for k in log), sorted(log)
    assert ("k_seq_tail" in log) == (variant != "greedy"), sorted(log)
    c.check(m, got, True, (variant, "shared"))
    # sharers have no records below their shared length, whatever the parent's say there
    if top_n is not None:
        rec = m.seq_logprobs(1, 0, P + 1)
        assert (rec["token"][:P] == -1).all() and np.isnan(rec["logprob"][:P]).all() and (rec["top_ids"][:P] == -1).all()
    m.close()
    f = _mk(spec, img)  # copies: CACHE / (w + 2) = 64 rows per slot hold P + 3 + 6 + 10
    assert f.seq_slots(w + 2) == CACHE // (w + 2) >= max(c.totals)
    f.seq_prefill(0, c.prefix)
    for s in range(1, n_seq):
        f.seq_fork(0, s, P)
    _new_log()
    got_f, _ = f.generate_batch(c.prompts, c.totals, **c.kw())
    assert not any(k.startswith("k_seq_attn_pfx<") for k in _ffi.launch_log())
    assert got_f == got
    c.check(f, got_f, False, (variant, "forked"))
    f.close()


def test_samples_that_fit_no_equal_partition_fit_the_shared_layout(gpu):
    """the capability: 4 sequences of up to 310 positions behind a prefix of 200 need 1240 rows as copies - an equal
    slot of this cache holds 160 - and 640 with the prefix shared; the totals cross the split boundary at 256"""
    spec, img = _image(gpu, "a")
    c = LoopCase(spec, img, 200, 4, 100, 1300, None, bias=False, sampled=True)
    c.totals = [310, 296, 305, 270]
    assert sum(plan_shared_layout(CACHE, 4, 200, c.totals)) <= CACHE < 4 * max(c.totals)
    f = _mk(spec, img)
    assert f.seq_slots(4) == 160
    assert _code(lambda: f.generate_batch(c.prompts, c.totals, c.samplings)) == _ffi.KH_ERR_RANGE
    f.close()
    c.twin_run()
    m = _shared_model(c)
    got, _ = m.generate_batch(c.prompts, c.totals, **c.kw())
    c.check(m, got, True, ("capability",))
    assert len({tuple(g[200:]) for g in got}) > 1  # distinct seeds, distinct continuations
    m.close()


def test_best_of_with_a_shared_prefix_ranks_the_same_samples(gpu):
    spec, img = _image(gpu, "a")
    rng = np.random.default_rng(1400)
    prompt = [int(t) for t in rng.integers(0, spec.vocab_size, 150)]
    m = _mk(spec, img)
    with pytest.raises(ValueError):
        m.best_of(prompt, 4, 170, _sampling(5), share=True, penalties={"repetition": 1.2})
    _new_log()
    shared = m.best_of(prompt, 4, 170, _sampling(5), top_n=2, share=True)  # 4 x 170 rows as copies: 680 > 640
    assert any(k.startswith("k_seq_attn_pfx<") for k in _ffi.launch_log())
    m.close()
    twin = _mk(spec, img, flags=EXACT)
    for r in shared:
        twin.set_sampling(**_sampling(r["seed"]))
        assert twin.generate(prompt, 170, exec="graph")[0] == r["words"], r["seed"]
    twin.close()
    assert sorted(r["seed"] for r in shared) == [5, 6, 7, 8]
    assert [r["mean_logprob"] for r in shared] == sorted((r["mean_logprob"] for r in shared), reverse=True)


def test_demo_cli_share_prefix_prints_the_same_lines(gpu, tmp_path):
    """--parallel N --share-prefix: the ids of N batch-1 generates, from a cache too short for N copies"""
    import subprocess
    spec, img = _image(gpu, "a", seq_len=320)
    P, T, N, seed = S.tokens("a", 90), 110, 4, 41  # 4 x 110 rows as copies: 440 > 320; shared: 110 + 3 x 21
    twin = _mk(spec, img, flags=EXACT)
    want = []
    for s in range(N):
        twin.set_sampling(**_sampling(seed + s))
        want.append(twin.generate(P, T, exec="graph")[0])
    twin.close()
    path = tmp_path / "m.bin"
    img.cpu().numpy().tofile(path)
    exe = build.build_demo()
    args = [exe, str(path), "--rope", "half", "--theta", str(spec.rope_theta), "--eps", str(spec.rms_eps),
            "--max-seq-len", str(spec.seq_len), "--steps", str(T), "--prompt", ",".join(map(str, P)),
            "--temperature", "0.8", "--top-k", "50", "--top-p", "0.95", "--seed", str(seed), "--parallel", str(N)]
    out = subprocess.run(args + ["--share-prefix"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    at = lines.index("Generating...")
    assert [[int(t) for t in ln.split()] for ln in lines[at + 1:at + 1 + N]] == want
    assert subprocess.run(args, capture_output=True, text=True, timeout=120).returncode != 0  # copies do not fit


# ---- 5. rules --------------------------------------------------------------------------------------------------------
def test_rules_are_checked_before_any_launch(gpu):
    spec, img = _image(gpu, "a")
    m = _mk(spec, img)
    bad, rng_, uns = _ffi.KH_ERR_INVALID_ARG, _ffi.KH_ERR_RANGE, _ffi.KH_ERR_UNSUPPORTED
    for lens in ([], [8] * 65, [7, 8], [CACHE - 7, 8]):
        assert _code(lambda: m.seq_slots_var(lens)) == bad, lens
    m.seq_slots_var([100, 40, 40, 8, 8])
    text = list(range(1, 61))
    m.seq_prefill(0, text)
    m.seq_prefill(3, [1, 2, 3])
    torch.cuda.synchronize()
    _new_log()

    def refused(code, call):
        assert _code(call) == code, call
        assert not _ffi.launch_log(), _ffi.launch_log()

    refused(bad, lambda: m.seq_share(1, 1, 4))
    refused(bad, lambda: m.seq_share(0, 1, -1))
    refused(bad, lambda: m.seq_share(1, 0, 4))          # slot 0 is the batch-1 sequence: never a sharer
    refused(rng_, lambda: m.seq_share(0, 5, 4))
    refused(rng_, lambda: m.seq_share(5, 1, 4))
    refused(rng_, lambda: m.seq_share(3, 1, 9))         # more rows than the source owns
    m.seq_share(0, 1, 50)
    m.seq_share(0, 2, 30)
    assert not _ffi.launch_log()                         # sharing launches nothing
    assert [m.seq_row(1, p) for p in (0, 49, 50, 89)] == [0, 49, 100, 139]
    assert [m.seq_row(2, p) for p in (29, 30, 69)] == [29, 140, 179]
    refused(rng_, lambda: m.seq_row(1, 90))              # capacity: 50 shared + 40 own
    refused(rng_, lambda: m.seq_row(3, 8))
    refused(uns, lambda: m.seq_share(1, 3, 4))          # a sharer of a sharer
    refused(uns, lambda: m.seq_share(2, 4, 1))
    # dst with dependants: slot 0 cannot be a dst at all, so make slot 3 a parent of 4 first
    m.seq_share(3, 4, 3)
    refused(uns, lambda: m.seq_share(0, 3, 10))
    m.seq_share(3, 4, 0)
    # the parent's rows below Pmax = 50 are immutable
    refused(bad, lambda: m.seq_prefill(0, [1, 2], 49))
    refused(bad, lambda: m.seq_prefill(0, [1, 2], 0))
    refused(bad, lambda: m.seq_step([0], [5], [49]))
    refused(bad, lambda: m.seq_step([0, 3], [5, 6], [10, 3], logprobs=0))
    refused(bad, lambda: m.seq_set_history(0, [1, 2], 48))
    refused(bad, lambda: m.generate_batch([text + [7]], 70))                      # nothing cached: would feed position 0
    refused(bad, lambda: m.generate_batch([text + [7]], 70, cached=[49]))
    refused(bad, lambda: m.generate_batch([text + [7]], 70, cached=[49], logprobs=0))
    refused(bad, lambda: m.seq_fork(3, 0, 3))            # a fork into the parent
    refused(uns, lambda: m.seq_fork(1, 3, 3))            # ... from or into a sharer
    refused(uns, lambda: m.seq_fork(3, 1, 3))
    # a sharer is fed from its shared length on
    refused(bad, lambda: m.seq_prefill(1, [1, 2], 49))
    refused(bad, lambda: m.seq_prefill(2, [1, 2], 0))
    refused(bad, lambda: m.seq_step([1], [5], [49]))
    refused(bad, lambda: m.seq_step([3, 2], [5, 6], [3, 29]))
    refused(bad, lambda: m.seq_set_history(1, [1, 2], 49))
    refused(bad, lambda: m.generate_batch([text + [7], text + [8]], 70, cached=[50, 49]))
    refused(bad, lambda: m.generate_batch([text + [7], text + [8]], 70, cached=None))
    refused(rng_, lambda: m.seq_prefill(1, [1] * 41, 50))                         # past its capacity of 90
    refused(rng_, lambda: m.seq_step([1], [5], [90]))
    refused(rng_, lambda: m.generate_batch([text + [7], text + [8]], [70, 91], cached=[50, 50]))
    # penalties on a sharer; bias and log-probs are fine there, penalties on the others too
    pen = {"repetition": 1.2}
    refused(uns, lambda: m.seq_step([1], [5], [50], penalties=[pen]))
    refused(uns, lambda: m.seq_step([3, 2], [5, 6], [3, 30], penalties=[None, pen]))
    refused(uns, lambda: m.generate_batch([text + [7], text + [8]], 70, cached=[50, 50], penalties=[None, pen]))
    # what is allowed: the parent from Pmax on, sharers from their length on, mixed with a slot that shares nothing
    nxt = m.seq_step([0, 1, 2, 3], [5, 6, 7, 8], [50, 50, 30, 3], penalties=[pen, None, None, pen],
                     logit_bias=[None, {9: 2.0}, None, None], logprobs=0)
    assert len(nxt) == 4
    m.generate_batch([text + [7], text + [8]], 70, cached=[50, 50])
    m.seq_fork(0, 3, 8)                                   # the source may be a parent
    m.seq_set_history(1, [1, 2], 50)
    # n_rows = 0 detaches; seq_slots and seq_slots_var reset every relation
    _new_log()
    m.seq_share(0, 1, 0)
    assert m.seq_row(1, 0) == 100
    refused(bad, lambda: m.seq_prefill(0, [1, 2], 29))   # slot 2 still holds 30
    m.seq_share(0, 2, 0)
    m.seq_prefill(0, [1, 2], 0)
    m.seq_share(0, 1, 50)
    m.seq_slots_var([100, 40, 40, 8, 8])
    assert m.seq_row(1, 0) == 100
    m.seq_prefill(0, [1, 2], 0)
    m.seq_share(0, 1, 50)
    assert m.seq_slots(8) == CACHE // 8
    assert [m.seq_row(s, 1) for s in range(8)] == [s * (CACHE // 8) + 1 for s in range(8)]
    m.seq_prefill(0, [1, 2], 0)
    m.close()


# ---- 6. nothing changes when unused ----------------------------------------------------------------------------------
def test_a_pass_without_a_sharer_launches_the_plain_kernel(gpu):
    spec, img = _image(gpu, "a")
    m = _mk(spec, img)
    m.seq_slots_var([60, 20, 8])  # unequal slots, nobody shares
    m.seq_prefill(0, list(range(1, 41)))
    m.seq_share(0, 1, 40)
    m.seq_share(0, 1, 0)          # ... any more
    _new_log()
    m.seq_step([0, 1, 2], [5, 6, 7], [40, 0, 0])
    m.generate_batch([[1, 2, 3], [4], [5, 6]], [20, 20, 8], [None, _sampling(1), None])
    m.seq_prefill(1, [1, 2, 3])
    log = _ffi.launch_log()
    assert "k_seq_attn<16,0>" in log and any(k.startswith("seq_attn_launch<") for k in log), sorted(log)
    assert not any(k.startswith(("k_seq_attn_pfx", "seq_attn_pfx_launch")) for k in log), sorted(log)
    # the equal layout through the new tables: words of a plain call as on a model that was never cut unequally
    m.seq_slots(4)
    a, _ = m.generate_batch([[1, 2, 3], [4], [5, 6]], [20, 20, 8], [None, _sampling(1), None])
    n = _mk(spec, img)
    n.seq_slots(4)
    b, _ = n.generate_batch([[1, 2, 3], [4], [5, 6]], [20, 20, 8], [None, _sampling(1), None])
    assert a == b
    n.close()
    m.close()


# ---- 7. every instantiation ------------------------------------------------------------------------------------------
def test_instantiation_gate(gpu):
    """every compiled k_seq_attn_pfx was launched (and checked) by this file; names only"""
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    _new_log()
    compiled = co.kernels(co.code_object_notes(_ffi.LIB_PATH), {STEM})
    launched = {k for k in _LAUNCHED if k.split("<")[0] == STEM}
    assert len(compiled) == 9, sorted(compiled)
    assert launched <= compiled, f"launched but not found in the code objects: {sorted(launched - compiled)}"
    gap = compiled - launched
    assert not gap, f"compiled and never launched (run the whole module): {sorted(gap)}"
