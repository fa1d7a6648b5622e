"""The GEMM prefill into sequence slots on the GPU: kh_model_seq_prefill_gemm (csrc/kh_seq_prefill.h: k_rg_gemm,
k_rg_rope, k_rg_attn; the passes of csrc/kh_model_gemm.hip) and the Python calls on top of it.

The contract is kh_model_prefill_gemm's, not the bit-exact one of seq_prefill: K/V rows are held to the project's
tolerances against the CPU ORACLE fed the same tokens one by one (seq_gemm_cases.kv_atol: 5e-6, int8 4x), and so are
the logits of an exact step on the slot's next token (logit_atol: 2e-5 / 5e-5).  The pass has no logits of its own and
the 8-lane pass no accessor for its rows, so that step runs on a batch-1 twin that holds the slot's very K/V bytes
(either because equality (a) below was just asserted, or because the rows were copied over); the slot's own exact
seq_step then has to make the twin's pick.  On top of the tolerances two equalities hold on RAW BYTES, because the
arithmetic is one text with kh_model_prefill_gemm and slab columns are independent:
  (a) a lone segment leaves the bytes a batch-1 twin's prefill_gemm(tokens, pos0) leaves in rows [pos0, pos0 + n);
  (b) a multi-segment call leaves, per slot, the bytes of the same segments fed one call each, under every (R, NT)
      tile forced on the three GEMMs of the pass.
Geometries, the layout (2048 cache rows: three slots of 300 rows, 61 of 8) and the bounds are tests/seq_gemm_cases.py.

Worst errors against the oracle measured on an MI355X (the tests print them as "worst[...]"; DESIGN 3.3i repeats
them), all inside the bounds:
    geometry     K/V rows (bound)     next-step logits (bound)
    mha-inter    1.71e-6 (5e-6)       1.13e-6 (2e-5)
    gqa-half     2.74e-6 (5e-6)       1.19e-6 (2e-5)
    half-hs48    1.67e-6 (5e-6)       1.01e-6 (2e-5)
    qwen-bias    1.67e-6 (5e-6)       9.54e-7 (2e-5)
    int8         2.62e-6 (2e-5)       1.01e-6 (5e-5)"""
import ctypes as C

import numpy as np
import pytest

import code_objects as co
import seq_gemm_cases as G
from kuiperllama_amd import _ffi, build
from kuiperllama_amd.model import KuiperModel, plan_seq_prefill_gemm

pytestmark = pytest.mark.gpu

STEMS = {"k_rg_gemm", "k_rg_rope", "k_rg_attn"}
_LAUNCHED = set()  # what the calls whose rows were compared launched (the gate at the end reads it)
_WORST = {}
HOOKS = ("KH_PG_SHAPE_QKV", "KH_PG_SHAPE_RESID", "KH_PG_SHAPE_SWIGLU")
TILES = ((2, 8), (2, 4), (2, 2), (1, 4))  # the register tiles of the prefill GEMMs


@pytest.fixture(autouse=True)
def _clean_hooks():
    try:
        yield
    finally:
        for k in HOOKS + ("KH_LAUNCH_LOG", "KH_PG_ATTN"):
            _ffi.debug_set(k, None)


def _model(spec, lens=G.LENS):
    m = KuiperModel.from_host_image(G.host_image(spec), spec, max_seq_len=spec.seq_len)
    m.seq_slots_var(lens)
    return m


def _twin(spec):
    return KuiperModel.from_host_image(G.host_image(spec), spec, max_seq_len=spec.seq_len)


def _read_all(m, spec):
    return [m.read_kv(layer, 0, spec.seq_len) for layer in range(spec.n_layers)]


def _poison(m, spec, row0, n):
    nan = np.full((n, spec.kv_dim), np.nan, np.float32)
    for layer in range(spec.n_layers):
        m.write_kv(layer, row0, nan, nan)


def _logged(call):
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    call()
    log = set(_ffi.launch_log())
    _ffi.debug_set("KH_LAUNCH_LOG", None)
    return log


class Ref:
    """the oracle fed a text token by token: the logits of every position and the K/V rows [layer][pos]"""

    def __init__(self, oracle, spec, text):
        om = oracle.OracleModel.from_spec(G.host_image(spec), spec, cache_len=G.LONG)
        self.text = text
        self.logits = [om.forward(t, p).copy() for p, t in enumerate(text)]
        k, v = om.kv_cache()
        self.k, self.v = k[:, :len(text)].copy(), v[:, :len(text)].copy()


_REF = {}


def _ref(oracle, spec, key, text):
    if (spec.name, key) not in _REF:
        _REF[(spec.name, key)] = Ref(oracle, spec, text)
    return _REF[(spec.name, key)]


def _note(spec, kv=0.0, lg=0.0):
    w = _WORST.setdefault(spec.name, [0.0, 0.0])
    w[0], w[1] = max(w[0], kv), max(w[1], lg)


def _report(spec):
    w = _WORST[spec.name]
    print(f"worst[{spec.name}]: K/V {w[0]:.2e} (bound {G.kv_atol(spec):.0e}), "
          f"next-step logits {w[1]:.2e} (bound {G.logit_atol(spec):.0e})")


def _rows_vs_oracle(spec, after, rows, ref, pos0, what):
    """rows[i] holds position pos0 + i of ref's text: contract (1)"""
    n = len(rows)
    for layer in range(spec.n_layers):
        k, v = after[layer]
        ek = float(np.abs(k[rows] - ref.k[layer, pos0:pos0 + n]).max())
        ev = float(np.abs(v[rows] - ref.v[layer, pos0:pos0 + n]).max())
        _note(spec, kv=max(ek, ev))
        assert ek <= G.kv_atol(spec) and ev <= G.kv_atol(spec), what + (layer, ek, ev)  # (NaN: a row was not written)


def _others_untouched(spec, before, after, rows, what):
    other = np.ones(spec.seq_len, bool)
    other[rows] = False
    for layer in range(spec.n_layers):
        (bk, bv), (k, v) = before[layer], after[layer]
        assert k[other].tobytes() == bk[other].tobytes() and v[other].tobytes() == bv[other].tobytes(), \
            what + (layer, "a row that is no segment's was written")


def _next_step(m, twin, spec, slot, ref, n, what, copy_rows=None):
    """contract (2): the exact step on the slot's next token.  The twin holds the slot's K/V bytes in rows [0, n) -
    copy_rows: (layer -> (k, v)) to put there first; m's own exact seq_step makes the same pick"""
    if copy_rows is not None:
        for layer in range(spec.n_layers):
            twin.write_kv(layer, 0, *copy_rows[layer])
    pick = twin.predict(ref.text[n], n, exec="fused")
    e = float(np.abs(twin.logits() - ref.logits[n]).max())
    _note(spec, lg=e)
    assert e <= G.logit_atol(spec), what + ("next-step logits", e)
    assert m.seq_step([slot], [ref.text[n]], [n]) == [pick], what + ("the slot's own step",)


def _rope_follows(spec, R, NT):
    """does k_rg_rope follow the QKV GEMM?  Not where its epilogue rotates: interleaved pairs always, half mode when the
    head size is a multiple of 32 and the tile holds the partner rows (R = 2) and can keep them (NT <= 4)"""
    return spec.rope_mode != G.INTER and (spec.head_size % 32 != 0 or R != 2 or NT > 4)


def _rope_kernel(spec, T):
    """_rope_follows for the tile the cost model plans for a T-token pass (test_seq_gemm_gpu.py's rule)"""
    out = (C.c_int32 * 7)()
    r2 = spec.dim % 32 == 0 and spec.kv_dim % 32 == 0
    assert _ffi.lib().kh_plan_prefill_shape(0, T, spec.dim + 2 * spec.kv_dim, spec.dim, int(spec.quant), int(r2), out) == 0
    return _rope_follows(spec, out[0], out[1])


def _rope_planned(spec, n_tokens):
    """does k_rg_rope follow in ANY pass of a call with these segments, no hook set: _rope_kernel for the T = 16 x
    tiles of each planned pass"""
    tiles = {}
    for p, _, _, n in plan_seq_prefill_gemm(n_tokens):
        tiles[p] = tiles.get(p, 0) + (n + 15) // 16
    return any(_rope_kernel(spec, 16 * t) for t in tiles.values())


def _check_log(spec, log, T=None, rope=None):
    hb, nw = spec.head_size // 16, 4 if spec.head_size == 128 else 8
    assert f"k_rg_attn<{hb},{nw}>" in log and any(k.startswith("k_rg_gemm<") for k in log), sorted(log)
    assert ("k_rg_rope" in log) == (_rope_kernel(spec, T) if rope is None else rope), (T, sorted(log))
    assert not any(k.startswith(("k_pg_attn", "k_pg_rope", "k_pf_", "k_seq_", "k_attn")) for k in log), sorted(log)
    q = "true" if spec.quant else "false"
    assert not any(k.startswith("k_pg_gemm<") and k.endswith(",0>") for k in log), sorted(log)  # QKV is k_rg_gemm's
    assert any(k.startswith(f"k_pg_gemm<{q},") and k.endswith(",1>") for k in log), sorted(log)
    assert any(k.startswith(f"k_pg_gemm<{q},") and k.endswith(",2>") for k in log), sorted(log)


# ---- 1. single segments ----------------------------------------------------------------------------------------------
SINGLE = [(1, 0), (15, 0), (16, 0), (17, 0), (33, 0), (290, 0), (28, 5), (17, 16), (40, 37)]  # (tokens, pos0)


@pytest.mark.parametrize("name", sorted(G.SPECS))
def test_single_segments(gpu, oracle, name):
    """one segment into slot 1 (rows 300 ..): 1 / 15 / 16 / 17 / 33 / 290 tokens at position 0, continuations at
    positions 5, 16 and 37 behind exactly fed rows.  The target rows are poisoned first; contract (1) and (2), every
    other cache row byte-identical, equality (a) against a batch-1 twin's prefill_gemm."""
    spec = G.SPECS[name]
    text = [int(t) for t in np.random.default_rng(17).integers(0, spec.vocab_size, G.LONG)]
    ref = _ref(oracle, spec, "single", text)
    m, twin = _model(spec), _twin(spec)
    row0 = m.seq_row(1, 0)
    assert row0 == G.LONG
    for n, pos0 in SINGLE:
        what = (name, n, pos0)
        if pos0 == 5:  # the continuations stand behind exact rows, in the slot and in the twin
            m.seq_prefill(1, text[:37])
            twin.prefill(text[:37])
        toks = text[pos0:pos0 + n]
        rows = list(range(row0 + pos0, row0 + pos0 + n))
        _poison(m, spec, rows[0], n)
        _poison(twin, spec, pos0, n)
        before = _read_all(m, spec)
        log = _logged(lambda: m.seq_prefill(1, toks, pos0=pos0, gemm=True))
        after = _read_all(m, spec)
        _rows_vs_oracle(spec, after, rows, ref, pos0, what)
        _others_untouched(spec, before, after, rows, what)
        _check_log(spec, log, T=16 * ((n + 15) // 16))
        _LAUNCHED.update(log)
        twin.prefill_gemm(toks, pos0)
        for layer in range(spec.n_layers):
            tk, tv = twin.read_kv(layer, pos0, n)
            k, v = after[layer]
            assert k[rows].tobytes() == tk.tobytes() and v[rows].tobytes() == tv.tobytes(), \
                what + (layer, "equality (a): not the bytes of the batch-1 twin")
        _next_step(m, twin, spec, 1, ref, pos0 + n, what)
    _report(spec)
    m.close()
    twin.close()


# ---- 2. ragged calls -------------------------------------------------------------------------------------------------
def _ragged(spec):
    """(slots in call order, {slot: tokens}): 290 / 300 / 17 tokens in the long slots, 1 .. 8 in 20 short ones,
    shuffled - 60 token tiles, two passes, and the order puts a long segment across them"""
    rng = np.random.default_rng(20)  # (this shuffle cuts a long segment behind its token 112)
    lens = {0: 290, 1: 300, 2: 17}
    lens.update({s: 1 + (3 * s) % 8 for s in range(3, 23)})
    order = [int(s) for s in rng.permutation(sorted(lens))]
    return order, {s: [int(t) for t in rng.integers(0, spec.vocab_size, lens[s])] for s in sorted(lens)}


def test_the_ragged_case_splits_a_segment():
    order, segs = _ragged(G.SPECS["gqa-half"])
    runs = plan_seq_prefill_gemm([len(segs[s]) for s in order])
    assert max(r[0] for r in runs) == 1 and len(runs) == len(order) + 1, runs  # two passes, one segment in both
    assert sum(len(t) for t in segs.values()) > 64 * 8


def _slot_rows(m, segs):
    return {s: list(range(m.seq_row(s, 0), m.seq_row(s, 0) + len(t))) for s, t in segs.items()}


@pytest.mark.parametrize("name", ["gqa-half", "int8", "half-hs48"])
def test_ragged_calls(gpu, oracle, name):
    """23 segments in shuffled slot order in ONE call: oracle bounds per slot, untouched rows identical, the next step
    of three slots; then equality (b) - against the same segments fed one call each - without hooks and under each
    (R, NT) tile forced on all three GEMMs, the residual GEMMs with K split across 2 and 4 workgroups in turn."""
    spec = G.SPECS[name]
    order, segs = _ragged(spec)
    # (one more token where the slot has room for it: the next step's)
    refs = {s: _ref(oracle, spec, ("ragged", s), segs[s] + ([7] if len(segs[s]) < G.LENS[s] else [])) for s in order}
    a, b, twin = _model(spec), _model(spec), _twin(spec)
    rows = _slot_rows(a, segs)
    every = [r for s in order for r in rows[s]]
    q = "true" if spec.quant else "false"
    forced = [None] + [(R, NT, (1, 2, 1, 2)[i], (2, 4, 1, 2)[i]) for i, (R, NT) in enumerate(TILES)]
    for cfg in forced:
        what = (name, "ragged", cfg)
        for k in HOOKS:
            _ffi.debug_set(k, None if cfg is None else
                           f"{cfg[0]},{cfg[1]},{cfg[2]}" + (f",{cfg[3]}" if k.endswith("RESID") else ""))
        for mm in (a, b):
            for s in order:
                _poison(mm, spec, rows[s][0], len(rows[s]))
        before = _read_all(a, spec)
        log = _logged(lambda: a.seq_prefill_many(order, [segs[s] for s in order]))
        after = _read_all(a, spec)
        for s in order:
            _rows_vs_oracle(spec, after, rows[s], refs[s], 0, what + (s,))
        _others_untouched(spec, before, after, every, what)
        if cfg is None:
            _check_log(spec, log, rope=_rope_planned(spec, [len(segs[s]) for s in order]))
        else:
            R, NT = cfg[:2]
            _check_log(spec, log, rope=_rope_follows(spec, R, NT))
            assert {f"k_rg_gemm<{q},{R},{NT},0>", f"k_pg_gemm<{q},{R},{NT},1>", f"k_pg_gemm<{q},{R},{NT},2>"} <= log, \
                sorted(log)
            assert not any(k.startswith(("k_rg_gemm<", "k_pg_gemm<")) and f",{R},{NT}," not in k for k in log), sorted(log)
        _LAUNCHED.update(log)
        for s in order:  # equality (b): one call per segment, the same order
            b.seq_prefill(s, segs[s], gemm=True)
        other = _read_all(b, spec)
        for layer in range(spec.n_layers):
            for s in order:
                r = rows[s]
                assert after[layer][0][r].tobytes() == other[layer][0][r].tobytes() and \
                    after[layer][1][r].tobytes() == other[layer][1][r].tobytes(), \
                    what + (layer, s, "equality (b): not the bytes of the segment fed alone")
        if cfg is None:
            for s in (0, 2, next(s for s in order if s > 2 and len(segs[s]) < G.SHORT)):
                n = len(segs[s])
                _next_step(a, twin, spec, s, refs[s], n, what + (s,),
                           copy_rows=[(after[layer][0][rows[s]], after[layer][1][rows[s]])
                                      for layer in range(spec.n_layers)])
    _report(spec)
    for mm in (a, b, twin):
        mm.close()


# ---- 3. sharers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gqa-half", "int8"])
@pytest.mark.parametrize("P", [32, 37])
def test_sharers_are_fed_from_their_shared_length_on(gpu, oracle, name, P):
    """slots 1 and 2 share P rows of slot 0 (P = 32: on a tile edge; 37: inside a tile), the parent fed by an earlier
    call; the two sharers and a plain slot are fed in one call from P on.  Their rows equal, as bytes, those of a
    forked, non-sharing layout fed the same tokens by the same call, and lie within the bounds of the oracle; the
    parent's rows are unchanged; the attention is k_rg_attn."""
    spec = G.SPECS[name]
    rng = np.random.default_rng(41)
    parent = [int(t) for t in rng.integers(0, spec.vocab_size, 48)]
    own = {1: [int(t) for t in rng.integers(0, spec.vocab_size, 40)], 2: [int(t) for t in rng.integers(0, spec.vocab_size, 17)]}
    plain = [int(t) for t in rng.integers(0, spec.vocab_size, 7)]
    tail = int(rng.integers(0, spec.vocab_size))
    refs = {s: _ref(oracle, spec, ("share", P, s), parent[:P] + own[s] + [tail]) for s in (1, 2)}
    refs[5] = _ref(oracle, spec, ("share", "plain"), plain + [tail])
    sh, fk, twin = _model(spec), _model(spec), _twin(spec)
    for mm in (sh, fk):
        mm.seq_prefill(0, parent, gemm=True)
    for s in (1, 2):
        sh.seq_share(0, s, P)
        fk.seq_fork(0, s, P)
    slots, toks, pos0 = [2, 5, 1], [own[2], plain, own[1]], [P, 0, P]
    rows_sh = {s: [sh.seq_row(s, p) for p in range(p0, p0 + len(t))] for s, t, p0 in zip(slots, toks, pos0)}
    rows_fk = {s: [fk.seq_row(s, p) for p in range(p0, p0 + len(t))] for s, t, p0 in zip(slots, toks, pos0)}
    assert rows_sh[1][0] == G.LONG and rows_fk[1][0] == G.LONG + P  # a sharer owns only what follows the prefix
    for s in slots:
        _poison(sh, spec, rows_sh[s][0], len(rows_sh[s]))
        _poison(fk, spec, rows_fk[s][0], len(rows_fk[s]))
    before = _read_all(sh, spec)
    log = _logged(lambda: sh.seq_prefill_many(slots, toks, pos0))
    after = _read_all(sh, spec)
    fk.seq_prefill_many(slots, toks, pos0)
    forked = _read_all(fk, spec)
    what = (name, "share", P)
    _check_log(spec, log, rope=_rope_planned(spec, [len(t) for t in toks]))
    _LAUNCHED.update(log)
    for s, p0 in zip(slots, pos0):
        _rows_vs_oracle(spec, after, rows_sh[s], refs[s], p0, what + (s,))
        for layer in range(spec.n_layers):
            assert after[layer][0][rows_sh[s]].tobytes() == forked[layer][0][rows_fk[s]].tobytes() and \
                after[layer][1][rows_sh[s]].tobytes() == forked[layer][1][rows_fk[s]].tobytes(), \
                what + (layer, s, "not the bytes of the forked layout")
    _others_untouched(spec, before, after, [r for s in slots for r in rows_sh[s]], what)  # the parent's rows too
    # the next step of sharer 1: the twin takes the forked slot's rows [0, P + 40), which are one run
    n = P + len(own[1])
    r0 = fk.seq_row(1, 0)
    _next_step(sh, twin, spec, 1, refs[1], n, what,
               copy_rows=[(forked[layer][0][r0:r0 + n], forked[layer][1][r0:r0 + n]) for layer in range(spec.n_layers)])
    _report(spec)
    for mm in (sh, fk, twin):
        mm.close()


# ---- 4. RoPE paths ---------------------------------------------------------------------------------------------------
def test_rope_kernel_follows_exactly_where_the_epilogue_cannot_rotate(gpu, oracle):
    """half-hs48 (no multiple of 32: k_rg_rope always) and gqa-half under forced QKV tiles - (2,4) / (2,2) rotate in the
    epilogue, (2,8) and (1,4) leave it to k_rg_rope - with 17 and 21 tokens: a partial last tile, whose padding tokens
    repeat a row that must be rotated once.  k_rg_rope runs over T = 16 x tiles slab tokens of the pass."""
    for name, n in (("half-hs48", 17), ("gqa-half", 21)):
        spec = G.SPECS[name]
        text = [int(t) for t in np.random.default_rng(17).integers(0, spec.vocab_size, G.LONG)]
        ref = _ref(oracle, spec, "single", text)
        m = _model(spec)
        row0 = m.seq_row(2, 0)
        for R, NT in TILES:
            _ffi.debug_set("KH_PG_SHAPE_QKV", f"{R},{NT},1")
            _poison(m, spec, row0, n)
            log = _logged(lambda: m.seq_prefill(2, text[:n], gemm=True))
            _rows_vs_oracle(spec, _read_all(m, spec), list(range(row0, row0 + n)), ref, 0, (name, "rope", R, NT))
            assert ("k_rg_rope" in log) == _rope_follows(spec, R, NT), (name, R, NT, sorted(log))
            assert f"k_rg_gemm<false,{R},{NT},0>" in log, sorted(log)
            _LAUNCHED.update(log)
        _ffi.debug_set("KH_PG_SHAPE_QKV", None)
        m.close()


# ---- 5. the Python loop ----------------------------------------------------------------------------------------------
def test_generate_batch_and_best_of_with_gemm_prefill(gpu):
    """generate_batch(.., gemm_prefill=True) returns exactly the words of a model that does seq_prefill_many by hand
    and then generate_batch(.., cached=len - 1); best_of(.., share=True, gemm_prefill=True) runs and ranks."""
    spec = G.SPECS[G.LOOP_SPEC]
    img = G.host_image(spec, wander=True)
    prompts, totals = G.loop_case(spec)
    sp = [None if s % 3 == 0 else {"temperature": 0.8, "top_k": 40, "top_p": 0.95, "seed": 900 + s}
          for s in range(len(prompts))]
    a = KuiperModel.from_host_image(img, spec, max_seq_len=spec.seq_len)
    b = KuiperModel.from_host_image(img, spec, max_seq_len=spec.seq_len)
    a.seq_slots(32)
    b.seq_slots(32)
    res = []
    log = _logged(lambda: res.append(a.generate_batch(prompts, totals, sp, gemm_prefill=True)))
    assert any(k.startswith("k_rg_gemm<") for k in log) and any(k.startswith("k_rg_attn<") for k in log), sorted(log)
    assert not any(k.startswith("k_pf_qkv<") for k in log), sorted(log)  # no VALU prefill pass behind the GEMM one
    todo = [s for s, p in enumerate(prompts) if len(p) > 1]
    b.seq_prefill_many(todo, [prompts[s][:-1] for s in todo])
    want, _ = b.generate_batch(prompts, totals, sp, cached=[len(p) - 1 for p in prompts])
    assert res[0][0] == want
    assert all(len(w) == t for w, t in zip(want, totals))
    a.close()
    b.close()
    m = KuiperModel.from_host_image(img, spec, max_seq_len=spec.seq_len)
    prompt = [int(t) for t in np.random.default_rng(6).integers(0, spec.vocab_size, 41)]
    best = []
    log = _logged(lambda: best.extend(m.best_of(prompt, 4, 52, {"temperature": 0.9, "top_k": 50, "seed": 5},
                                                share=True, gemm_prefill=True)))
    assert any(k.startswith("k_rg_attn<") for k in log) and not any(k.startswith("k_pf_qkv<") for k in log), sorted(log)
    assert sorted(r["seed"] for r in best) == [5, 6, 7, 8] and all(len(r["words"]) == 52 for r in best)
    means = [r["mean_logprob"] for r in best]
    assert means == sorted(means, reverse=True) and all(np.isfinite(means))
    assert all(r["words"][:40] == prompt[1:] for r in best)
    m.close()


# ---- 5b. the fed-token record -----------------------------------------------------------------------------------------
def test_the_call_leaves_the_fed_token_record_of_seq_prefill(gpu):
    """what penalties count after the call is what seq_prefill would have recorded: a wide step with a strong
    repetition penalty on every lane leaves, in model A (fed by ONE ragged call: a second segment, a segment cut by
    the pass boundary, a sharer), the processed logits rows - raw bytes - of model B, which is fed by the same call
    and then has every slot's record stated again by seq_set_history; in model C, whose records are stated one token
    off, the rows differ.  The sharer is detached first (penalties are refused on sharing slots): its own rows then
    hold positions 0 .. of the slot, and so do their entries of the record."""
    spec = G.SPECS["gqa-half"]
    rng = np.random.default_rng(3)
    draw = lambda n: [int(t) for t in rng.integers(0, spec.vocab_size, n)]
    P, shorts = 16, list(range(4, 23))
    text = {0: draw(40), 1: draw(299), 2: draw(17), 3: draw(5)}
    text.update({s: draw(1 + (3 * s) % 7) for s in shorts})
    # 14 tiles of short slots, then the 19 tiles of slot 1: the pass boundary cuts it; the sharer last
    order = shorts[:14] + [1] + shorts[14:] + [2, 3]
    assert any(off > 0 for _, _, off, _ in plan_seq_prefill_gemm([len(text[s]) for s in order]))
    pen = {"repetition": 1.8, "presence": 0.5, "frequency": 0.25, "last_n": 0}
    rows = {}
    for which in "ABC":
        m = _model(spec)
        m.seq_prefill(0, text[0], gemm=True)  # the parent, fed by an earlier call
        m.seq_share(0, 3, P)  # slot 3 reads its positions [0, P) from slot 0 and is fed from P on
        m.seq_prefill_many(order, [text[s] for s in order], [P if s == 3 else 0 for s in order])
        m.seq_share(0, 3, 0)  # detached: slot 3's rows and record entries are now its positions 0 .. 4
        if which != "A":
            for s, t in text.items():
                m.seq_set_history(s, t if which == "B" else [(x + 1) % spec.vocab_size for x in t])
        lanes = [0] + order
        toks = [text[s][0] for s in lanes]  # a token of the slot's own history: the penalty bites
        m.seq_step(lanes, toks, [len(text[s]) for s in lanes], penalties=[pen] * len(lanes), gemm=True)
        rows[which] = [m.seq_gemm_logits(i).copy() for i in range(len(lanes))]
        m.close()
    for i, s in enumerate(lanes):
        assert rows["A"][i].tobytes() == rows["B"][i].tobytes(), (s, "not the record seq_set_history states")
        assert rows["A"][i].tobytes() != rows["C"][i].tobytes(), (s, "the penalties did not read the record")


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_an_empty_launch_log_and_the_cache_alone(gpu):
    spec = G.SPECS["gqa-half"]
    m = _model(spec)
    m.seq_prefill(0, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
    m.seq_share(0, 3, 8)  # slot 3 reads its positions [0, 8) from slot 0, whose rows below 8 are now immutable
    V = spec.vocab_size
    before = _read_all(m, spec)
    cases = [
        (dict(slots=[4, 7, 4], prompts=[[1], [2], [3]]), _ffi.KH_ERR_INVALID_ARG),                    # a slot twice
        (dict(slots=[3, 0], prompts=[[1], [2]], pos0=[8, 10]), _ffi.KH_ERR_INVALID_ARG),              # sharer + parent
        (dict(slots=[3], prompts=[[1, 2]], pos0=[7]), _ffi.KH_ERR_INVALID_ARG),                       # sharer below P
        (dict(slots=[0], prompts=[[1, 2]], pos0=[7]), _ffi.KH_ERR_INVALID_ARG),                       # shared rows
        (dict(slots=[4, 5], prompts=[[1], [1] * (G.SHORT + 1)]), _ffi.KH_ERR_RANGE),                  # over capacity
        (dict(slots=[4, 5], prompts=[[1], [2, 3]], pos0=[0, G.SHORT - 1]), _ffi.KH_ERR_RANGE),
        (dict(slots=[4, 64], prompts=[[1], [2]]), _ffi.KH_ERR_RANGE),                                 # no such slot
        (dict(slots=[4, 5], prompts=[[1], [2, V]]), _ffi.KH_ERR_RANGE),                               # no such token
        (dict(slots=list(range(64)) + [0], prompts=[[1]] * 65), _ffi.KH_ERR_RANGE),                   # n_seq = 65
    ]
    for kw, code in cases:
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        with pytest.raises(_ffi.KhError) as e:
            m.seq_prefill_many(**kw)
        assert e.value.code == code and not _ffi.launch_log(), (kw, e.value.code, _ffi.launch_log())
    _ffi.debug_set("KH_PG_ATTN", "0")  # no fallback to the decode-attention slices
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    with pytest.raises(_ffi.KhError) as e:
        m.seq_prefill(4, [1, 2, 3], gemm=True)
    assert e.value.code == _ffi.KH_ERR_UNSUPPORTED and not _ffi.launch_log(), (e.value.code, _ffi.launch_log())
    _ffi.debug_set("KH_PG_ATTN", None)
    after = _read_all(m, spec)
    for (bk, bv), (k, v) in zip(before, after):
        assert bk.tobytes() == k.tobytes() and bv.tobytes() == v.tobytes()
    m.seq_prefill(4, [1, 2, 3], gemm=True)  # the same call runs once the hook is gone
    m.close()
    bad = G.SMALL_HEAD  # head size 32: refused like prefill_gemm, and not rerouted to the VALU pass
    m = KuiperModel.from_host_image(G.host_image(bad), bad)
    m.seq_slots(4)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    with pytest.raises(_ffi.KhError) as e:
        m.seq_prefill_many([0, 1], [[1, 2], [3]])
    assert e.value.code == _ffi.KH_ERR_UNSUPPORTED and not _ffi.launch_log(), (e.value.code, _ffi.launch_log())
    m.close()


# ---- 7. gates --------------------------------------------------------------------------------------------------------
def test_a_model_that_never_asks_launches_and_allocates_nothing_new(gpu):
    """the calls of the existing paths log no k_rg_* launch and settle to a fixed allocation count; the first GEMM
    prefill into a slot then makes the six slabs of the GEMM prefill and nothing else, the second call nothing; a
    model that has run prefill_gemm already has those slabs: its first call allocates nothing"""
    spec = G.SPECS["gqa-half"]
    m = _model(spec)
    _ffi.debug_set("KH_LAUNCH_LOG", "1")

    def existing():
        m.seq_prefill(4, [1, 2, 3])
        m.seq_step([3, 4, 5], [1, 2, 3], [0, 3, 0])
        m.generate_batch([[1, 2], [3]], 4)

    existing()
    a0 = _ffi.alloc_stats()
    existing()
    a1 = _ffi.alloc_stats()
    assert a1["allocs"] == a0["allocs"] and a1["live"] == a0["live"]
    log = _ffi.launch_log()
    assert not any(k.startswith(("k_rg_", "k_pg_")) for k in log), sorted(log)
    m.seq_prefill(4, [1, 2, 3], gemm=True)
    a2 = _ffi.alloc_stats()
    assert a2["live"] - a1["live"] == 6 and a2["allocs"] - a1["allocs"] == 6, (a1, a2)
    m.seq_prefill_many([4, 5], [[1, 2, 3], [4]])
    assert _ffi.alloc_stats()["allocs"] == a2["allocs"]
    m.close()
    m = _model(spec)
    m.prefill_gemm([1, 2, 3, 4])
    a3 = _ffi.alloc_stats()
    m.seq_prefill(0, [1, 2, 3], gemm=True)
    assert _ffi.alloc_stats()["allocs"] == a3["allocs"]
    m.close()


def test_every_compiled_instantiation_of_the_new_stems_was_launched_and_compared(gpu):
    """runs last: what the compared calls above launched against the code objects - k_rg_gemm for fp32 / int8 x the
    four register tiles, k_rg_rope, k_rg_attn for head sizes 48 / 64 / 128"""
    if not co.tools_present():
        pytest.skip("LLVM tools of the ROCm install not found")
    compiled = co.kernels(co.code_object_notes(build.build_lib()), STEMS)
    assert len(compiled) == 12, sorted(compiled)
    launched = {k for k in _LAUNCHED if k.split("<")[0] in STEMS}
    assert compiled == launched, (sorted(compiled - launched), sorted(launched - compiled))
