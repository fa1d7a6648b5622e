"""Prompt attention: every compiled k_pg_attn<HB, NW, QT> and k_rg_attn<HB, NW> instantiation, every output layout
and every tile seam of csrc/kh_pattn_body.h, launched at operator level and checked against an fp64 gold.

k_pg_attn (csrc/kh_pattn.h) runs under every default prompt path, k_rg_attn (csrc/kh_seq_prefill.h) under the slot
prefill; both are ONE text.  HB = head size / 16 (48 / 64 / 128), NW = 8 waves (4 at head size 128) that take the
16-position tiles wave, wave + NW, ... in a two-deep register ring, QT = 1 / 2 / 4 query tiles of 16 tokens per
workgroup (the launch's own choice from start position 2048 on with >= 256 workgroups; hook KH_PG_ATTN_QT; head size
128 stops at 2).  The model-level gates see this kernel through the next layer's rows and the next step's logits only;
here the attention output itself is compared: EVERY token and head of every launch.

Gold: _gold() below, plain NumPy fp64 - per head S = Q K^T / sqrt(hs), the causal mask, a softmax, P V - over the K/V
rows gathered through the position-to-row map of the case; cross-checked at a few tokens per geometry against
oracle.mha(..., ACC_F64).  That oracle keeps its scores, softmax and P V in fp32 after an fp64 dot product, so the two
agree to its own round-off, bounded here by a tenth of the kernel's bound.

Data: layer 1 of a two-layer cache of 2700 rows (layer 0 all NaN); every K and V row no query column of the launch may
attend to is NaN (k_pg_attn: rows past pos0 + T - 1; k_rg_attn: every row outside the union of the tiles' readable
rows), and so are the query rows of k_rg_attn's padding columns.  `out` is filled with a sentinel bit pattern and has
guard space behind it (16 extra rows; the whole dim x tcap slab plus a guard); after the launch every stored output is
finite and every element no stored column owns keeps the sentinel.  The un-tiling is the test's own statement of
pg_tiled_index.  The three layouts of one launch configuration give the same bits.

k_pg_attn: GEOMETRIES x PG_CASES x KH_PG_ATTN_QT unset / 1 / 2 / 4 x three layouts; the logged instantiation must be
the one _pg_qt() and the head-size table predict.  k_rg_attn: one tile; lone aligned segments (32 full tiles at 2085,
100 tokens at 5) whose bits must equal k_pg_attn<HB, NW, 1>'s on the same tokens; the mixed pass of MIXED (segments of
1, 16, 17, 40 and 20 tokens at positions 0, 7, 300, 2085 and 48 = its shared length; distinct positive bases, one
negative base, shared prefixes of 37 and 48 rows) whose sharers must give the bits of the same segment run unshared
with the prefix rows copied in front of its own; every padding column has the bits of the column it repeats.

Seam probes (the under- and over-read check of the decode gate): one key is made dominant (score 20 against N(0, 1);
the gold's probability must exceed 0.99 - an assertion, not a skip) for a (token, head), so that the head's output is
that V row and a dropped or doubled timestep is an O(1) error: timestep 0, the token's own position, the row below
pos0 and pos0, both sides of a 16-position tile seam, of the seam between wave rounds (16 NW - 1, 16 NW), of the ring
swap (32 NW - 1, 32 NW), the last position tile of a group of QT > 1 tiles, for k_rg_attn both sides of the shared
length; the causal-leak probe puts the key at the token's position + 1: the token keeps its gold, its neighbour (given
the same query) becomes that V row.  Probes of one launch sit in different KV heads.

Gates: every k_pg_attn and k_rg_attn instantiation in the code objects was launched and checked, and the cell table
(PG_CELLS, RG_CELLS per instantiation: each layout; a single position tile, waves without a tile, more than one ring
round; a partial last query tile; a wholly padded query tile; each probe class; for k_rg_attn a prefix, a negative
base, a padding twin, 32 tiles, the bits of k_pg_attn) has no missing cell; UNREACHABLE lists the cells no launch can
reach.

The int8 tiled layout needs dim % 64 == 0 (the entry refuses it otherwise: a partial 64-column block would leave the
dim x tcap slab), so (6, 6, 48) runs two layouts; (8, 2, 48) gives k_pg_attn<3,8,*> its third.

Bound: |out - gold| <= 3e-5 + 2e-5 |gold| (the decode gate's).  Measured on an MI355X, worst |out - gold| (probed
heads included, whose output is a V row of magnitude up to 4.5): k_pg_attn head size 48: 2.1e-6, 64: 1.9e-6, 128:
1.7e-6; k_rg_attn head size 48: 1.7e-6, 64: 1.8e-6, 128: 2.3e-6 - a tenth of the bound; no case needed the
fp32-reference clause.  |oracle fp64 - gold| <= 4.1e-7.  Module wall time: 6.1 s (about 2300 checked launches).
Mutants the module was seen to reject, each in every geometry: the skip test with `>=` (by the pos0 % 16 == 1 slices
alone), a ring reload skipped for the last round, the prefix translation with `p <= pfx_len`, the causal mask with
`<= my_pos + 1`.
"""
import numpy as np
import pytest
import torch

import code_objects as co
from kuiperllama_amd import _ffi, build

pytestmark = pytest.mark.gpu

SEQ = 2700
LAYER = 1
TMAX = 512
ATOL, RTOL = 3e-5, 2e-5
PROBE_SCORE = 20.0
SENT = 0x7FC5A5A5     # a NaN with a payload: an output never stored is not finite, an element never owned keeps these bits
GUARD = 4096          # floats behind a tiled slab
L_F32, L_Q8, L_ROWS = 0, 1, 2
LAYOUTS = (L_ROWS, L_F32, L_Q8)

GEOMETRIES = [(6, 6, 48), (8, 2, 48), (6, 3, 64), (8, 2, 64), (14, 2, 64), (16, 4, 64), (4, 4, 128), (6, 3, 128)]
NWAVES = {48: 8, 64: 8, 128: 4}   # the test's own statement of launch_pg_attn's / launch_rg_attn's head-size table
QTS = (None, 1, 2, 4)
# (pos0, T): module docstring.  T = 16 QT k + {1, 17} at QT 2 and 4: 33, 49, 65, 81
# (1, 81) and (2049, 65): pos0 % 16 == 1 puts every query tile's last column on the first position of a tile, the
# one case in which the QT > 1 skip test `pt * 16 > tile_pos0 + 15` decides about a tile with a single visible key
PG_CASES = [(0, 1), (0, 16), (0, 17), (0, 37), (0, 512), (5, 100), (5, 129), (3, 33), (3, 49), (3, 65), (3, 81),
            (1, 81), (2049, 65), (2047, 512), (2048, 512), (2085, 512), (2085, 480), (SEQ - 16, 16), (SEQ - 1, 1)]
PROBE_CASE = (2085, 100)
# the mixed k_rg_attn pass: (tokens, pos0, base, pfx_len, pfx_row0); rows: S3 2..281, parents 300..347 and 350..386,
# S1 400, S2 410..432, S4 568..2644 (its unshared twin also 520..567), S5 2648..2667
MIXED = [(1, 0, 400, 0, 0), (16, 7, 410, 0, 0), (17, 300, -35, 37, 350), (40, 2085, 520, 48, 300),
         (20, 48, 2600, 48, 300)]

PG_CELLS = ("layout0", "layout1", "layout2", "single-tile", "idle-waves", "ring>1", "partial-q-tile", "padded-q-tile",
            "p:t0", "p:own", "p:below-pos0", "p:pos0", "p:tile-lo", "p:tile-hi", "p:round-lo", "p:round-hi",
            "p:ring-lo", "p:ring-hi", "p:group-last-tile", "p:leak")
RG_CELLS = ("layout0", "layout1", "layout2", "single-tile", "idle-waves", "ring>1", "partial-q-tile",
            "p:t0", "p:own", "p:below-pos0", "p:pos0", "p:tile-lo", "p:tile-hi", "p:round-lo", "p:round-hi",
            "p:ring-lo", "p:ring-hi", "p:pfx-lo", "p:pfx-hi", "p:leak", "prefix", "negative-base", "padding-twin",
            "32-tiles", "bits=k_pg_attn")
UNREACHABLE = {  # (stem, QT, cell) -> reason
    ("k_pg_attn", 1, "padded-q-tile"): "QT = 1: a group is one query tile, and a tile past T is no workgroup",
    ("k_pg_attn", 1, "p:group-last-tile"): "QT = 1: a group is one query tile",
}

_LAUNCHED = set()
_CELLS = {}
_WORST = {}    # (stem, head size) -> worst |out - gold|
_DONE = set()
_GEOS = {}


def _cell(inst, cell):
    _CELLS[(inst, cell)] = _CELLS.get((inst, cell), 0) + 1


def _tcap(T):
    return (T + 127) // 128 * 128


def _pg_qt(forced, heads, hs, pos0, T):
    """The test's own statement of pg_attn_qt (csrc/kh_pattn.h)."""
    maxqt = 2 if hs == 128 else 4
    if forced in (1, 2, 4):
        return min(forced, maxqt)
    if pos0 < 2048:
        return 1
    qt = 1
    while qt < maxqt and heads * ((T + 32 * qt - 1) // (32 * qt)) >= 256:
        qt *= 2
    return qt


def _tiled_index(quant, k, t, tcap):
    """The test's own statement of pg_tiled_index (csrc/kh_gemm.h): float index of (token t, column k)."""
    if not quant:
        return ((k >> 4) * tcap + t) * 16 + (k & 15)
    b, r = k >> 6, k & 63
    h, q, e = r >> 4, (r >> 2) & 3, r & 3
    return (((b * 4 + q) * tcap + t) * 4 + h) * 4 + e


def _gold(q, pos, K, V, heads, kvh, hs):
    """fp64 causal attention: q [n, dim], pos [n] (the last timestep of each column), K / V [P, kv_dim] indexed by
    POSITION.  Returns (out [n, dim], largest probability [n, heads])."""
    n, P, kv_mul = q.shape[0], K.shape[0], heads // kvh
    qd, Kd, Vd = q.astype(np.float64), K.astype(np.float64), V.astype(np.float64)
    masked = np.arange(P)[None, :] > np.asarray(pos)[:, None]
    out, pmax = np.empty((n, heads * hs)), np.empty((n, heads))
    for h in range(heads):
        g = h // kv_mul
        S = qd[:, h * hs:(h + 1) * hs] @ Kd[:, g * hs:(g + 1) * hs].T / np.sqrt(hs)
        S[masked] = -np.inf
        S -= S.max(axis=1, keepdims=True)
        np.exp(S, out=S)
        S /= S.sum(axis=1, keepdims=True)
        out[:, h * hs:(h + 1) * hs] = S @ Vd[:, g * hs:(g + 1) * hs]
        pmax[:, h] = S.max(axis=1)
    return out, pmax


def _close(got, gold):
    return np.abs(got - gold) <= ATOL + RTOL * np.abs(gold)


def _n_pt_cells(inst, n_pts, NW):
    if any(n == 1 for n in n_pts):
        _cell(inst, "single-tile")
    if any(n < NW for n in n_pts):
        _cell(inst, "idle-waves")
    if any(n > 2 * NW for n in n_pts):
        _cell(inst, "ring>1")


class _Geo:
    """One geometry: seeded data, device caches, the golds its configurations share."""

    def __init__(self, gpu, heads, kvh, hs):
        self.gpu, self.heads, self.kvh, self.hs = gpu, heads, kvh, hs
        self.kv_mul, self.kv_dim, self.dim, self.NW, self.HB = heads // kvh, kvh * hs, heads * hs, NWAVES[hs], hs // 16
        rng = np.random.default_rng(heads * 1000 + kvh * 100 + hs)
        self.kb = rng.standard_normal((SEQ, self.kv_dim), dtype=np.float32)
        self.vb = rng.standard_normal((SEQ, self.kv_dim), dtype=np.float32)
        self.q = rng.standard_normal((TMAX, self.dim), dtype=np.float32)
        self.kw = torch.full((LAYER + 1, SEQ, self.kv_dim), float("nan"), device=gpu)
        self.vw = torch.full((LAYER + 1, SEQ, self.kv_dim), float("nan"), device=gpu)
        self.layouts = [l for l in LAYOUTS if l != L_Q8 or self.dim % 64 == 0]
        self._idx, self._gold_pg = {}, {}

    def what(self):
        return f"({self.heads},{self.kvh},{self.hs})"

    def key(self, q, t, h):
        """c * q[t, head h] with c such that q . key / sqrt(hs) = PROBE_SCORE."""
        qh = q[t, h * self.hs:(h + 1) * self.hs].astype(np.float64)
        return (qh * (PROBE_SCORE * np.sqrt(self.hs) / float(qh @ qh))).astype(np.float32)

    def upload(self, readable, kmods=()):
        """Layer 1 := the base rows where `readable`, NaN elsewhere, with the probe keys (row, KV head, key) set.
        Returns the host copies."""
        k, v = self.kb.copy(), self.vb.copy()
        k[~readable] = np.nan
        v[~readable] = np.nan
        for row, g, vec in kmods:
            assert readable[row], row
            k[row, g * self.hs:(g + 1) * self.hs] = vec
        self.kw[LAYER].copy_(torch.from_numpy(k))
        self.vw[LAYER].copy_(torch.from_numpy(v))
        return k, v

    def index(self, layout, tcap):
        """[tcap, dim] float index of (token, column) in `out`; a bijection onto its range (asserted)."""
        if (layout, tcap) not in self._idx:
            t, k = np.arange(tcap, dtype=np.int64)[:, None], np.arange(self.dim, dtype=np.int64)[None, :]
            idx = t * self.dim + k if layout == L_ROWS else _tiled_index(layout == L_Q8, k, t, tcap)
            assert idx.min() == 0 and idx.max() == tcap * self.dim - 1 and np.unique(idx).size == idx.size
            self._idx[(layout, tcap)] = idx
        return self._idx[(layout, tcap)]

    def launch(self, kind, where, layout, nstored, tcap, qd, expect):
        """One launch into a sentinel-filled `out`; returns the stored columns [nstored, dim] as float32 bits."""
        from kuiperllama_amd import ops
        size = (nstored + 16) * self.dim if layout == L_ROWS else self.dim * tcap + GUARD
        buf = torch.full((size,), SENT, dtype=torch.int32, device=self.gpu)
        out = buf.view(torch.float32)
        geo = (self.heads, LAYER, SEQ, self.kv_dim, self.kv_mul, self.hs, layout, tcap, out, qd, self.kw, self.vw)
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        if kind == "pg":
            ops.mha_prefill_layout(where[0], where[1], *geo)
        else:
            ops.mha_prefill_tiles(where, *geo)
        log = _ffi.launch_log()
        assert log == {expect}, f"{self.what()} {kind} {where if kind == 'pg' else ''}: log {sorted(log)}, predicted {expect}"
        raw = buf.cpu().numpy()
        idx = self.index(layout, tcap)[:nstored]
        free = np.ones(size, bool)
        free[idx.ravel()] = False
        bad = np.flatnonzero(free & (raw != SENT))
        assert bad.size == 0, f"{self.what()} {expect} layout {layout}: {bad.size} elements no stored column owns " \
                              f"were written, the first at float {bad[0]} of {size}"
        _LAUNCHED.add(expect)
        _cell(expect, f"layout{layout}")
        return raw.view(np.float32)[idx]

    def check(self, got, gold, what, stem):
        assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} outputs are not finite " \
                                       "(a NaN row was read, or a stored column was not written)"
        err = np.abs(got - gold)
        key = (stem, self.hs)
        _WORST[key] = max(_WORST.get(key, 0.0), float(err.max()))
        ok = _close(got, gold)
        if not ok.all():
            t, c = np.argwhere(~ok)[0]
            raise AssertionError(f"{what}: |out - gold| {err.max():.3e}; first at token {t} head {c // self.hs}: "
                                 f"{got[t, c]!r} vs {gold[t, c]!r} ({int((~ok).sum())} elements)")

    # ---- k_pg_attn -----------------------------------------------------------------------------------------------------
    def gold_pg(self, pos0):
        """Gold of the longest slice of PG_CASES that starts at pos0; a shorter slice is its first rows."""
        if pos0 not in self._gold_pg:
            n = max(T for p, T in PG_CASES if p == pos0)
            self._gold_pg[pos0] = _gold(self.q[:n], pos0 + np.arange(n), self.kb[:pos0 + n], self.vb[:pos0 + n],
                                        self.heads, self.kvh, self.hs)[0]
        return self._gold_pg[pos0]

    def pg_inst(self, forced, pos0, T):
        return f"k_pg_attn<{self.HB},{self.NW},{_pg_qt(forced, self.heads, self.hs, pos0, T)}>"

    def pg_record(self, inst, qt, pos0, T):
        n_pts = [((pos0 + min(t0 + 16 * qt - 1, T - 1)) >> 4) + 1 for t0 in range(0, T, 16 * qt)]
        _n_pt_cells(inst, n_pts, self.NW)
        if T % 16:
            _cell(inst, "partial-q-tile")
        if qt > 1 and -(-T // 16) % qt:
            _cell(inst, "padded-q-tile")

    def run_pg(self, pos0, T, gold, q=None, qd=None, kmods=(), qts=QTS, layouts=None, tag=""):
        """The slice (pos0, T) under every KH_PG_ATTN_QT of `qts` and layout: log, sentinel, finite, gold, bits."""
        readable = np.arange(SEQ) < pos0 + T
        self.upload(readable, kmods)
        if qd is None:
            qd = torch.from_numpy(np.ascontiguousarray(self.q[:T])).to(self.gpu)
        res = {}
        for forced in qts:
            _ffi.debug_set("KH_PG_ATTN_QT", None if forced is None else str(forced))
            qt = _pg_qt(forced, self.heads, self.hs, pos0, T)
            inst = self.pg_inst(forced, pos0, T)
            first = None
            for layout in layouts or self.layouts:
                got = self.launch("pg", (pos0, T), layout, T, _tcap(T), qd, inst)
                what = f"{self.what()} {tag}pos0 {pos0} T {T} KH_PG_ATTN_QT {forced} {inst} layout {layout}"
                self.check(got, gold, what, "k_pg_attn")
                if first is None:
                    first = got
                else:
                    assert np.array_equal(got.view(np.int32), first.view(np.int32)), f"{what}: bits differ between layouts"
            self.pg_record(inst, qt, pos0, T)
            res[forced] = first
        _ffi.debug_set("KH_PG_ATTN_QT", None)
        return res

    def pg_probes(self, qt):
        pos0, T = PROBE_CASE
        NW = self.NW
        pr = [("t0", 0, 0), ("own", 15, pos0 + 15), ("own", T - 1, pos0 + T - 1), ("below-pos0", 16, pos0 - 1),
              ("pos0", 17, pos0), ("tile-lo", 31, 1023), ("tile-hi", 32, 1024),
              ("tile-lo", 40, ((pos0 + 40) >> 4) * 16 - 1), ("tile-hi", 41, ((pos0 + 41) >> 4) * 16),
              ("round-lo", 47, 16 * NW - 1), ("round-hi", 48, 16 * NW), ("ring-lo", 63, 32 * NW - 1),
              ("ring-hi", 64, 32 * NW), ("leak", 70, pos0 + 71), ("leak", 79, pos0 + 80)]
        for m in (2, 4):  # the last position tile of group 0 at QT = m: its first query tile skips it
            r = ((pos0 + 16 * m - 1) >> 4) * 16
            assert r > pos0 + 15
            pr.append(("group-last-tile" if m == qt else "tile-hi", 16 * m - 1, r))
        return pr

    def run_pg_probes(self):
        pos0, T = PROBE_CASE
        kvh, kv_mul, hs = self.kvh, self.kv_mul, self.hs
        maxqt = 2 if hs == 128 else 4
        P = pos0 + T
        n_launch = 0
        # the probe list depends on QT only through the class names of the group probes: place by the longest list
        base = self.pg_probes(maxqt)
        for i in range(-(-len(base) // kvh)):
            q = self.q[:T].copy()
            mine, kmods = [], []
            for g, (cls, t, r) in enumerate(base[i * kvh:(i + 1) * kvh]):
                h = g * kv_mul + (i + g) % kv_mul
                if cls == "leak":  # the neighbour asks the same question: it must see the key the token must not
                    q[t + 1, h * hs:(h + 1) * hs] = q[t, h * hs:(h + 1) * hs]
                    assert r == pos0 + t + 1 < P
                else:
                    assert 0 <= r <= pos0 + t
                kmods.append((r, g, self.key(q, t, h)))
                mine.append((i * kvh + g, t, h, r))
            k, v = self.kb[:P].copy(), self.vb[:P]
            for r, g, vec in kmods:
                k[r, g * hs:(g + 1) * hs] = vec
            gold, pmax = _gold(q, pos0 + np.arange(T), k, v, self.heads, kvh, hs)
            for j, t, h, r in mine:
                tt = t + 1 if base[j][0] == "leak" else t
                assert pmax[tt, h] > 0.99, f"{self.what()} probe {base[j]}: probability {pmax[tt, h]} in the gold"
                assert np.abs(gold[tt, h * hs:(h + 1) * hs] - self.vb[r, (h // kv_mul) * hs:(h // kv_mul + 1) * hs]).max() < 0.1
            qd = torch.from_numpy(q).to(self.gpu)
            for forced in (1, 2, 4):
                lay = [self.layouts[(i + forced) % len(self.layouts)]]
                self.run_pg(pos0, T, gold, q=q, qd=qd, kmods=kmods, qts=(forced,), layouts=lay, tag=f"probes {i} ")
                qt = min(forced, maxqt)
                names = self.pg_probes(qt)
                for j, t, h, r in mine:
                    _cell(f"k_pg_attn<{self.HB},{self.NW},{qt}>", "p:" + names[j][0])
                n_launch += 1
        return n_launch

    # ---- k_rg_attn -----------------------------------------------------------------------------------------------------
    def rg_inst(self):
        return f"k_rg_attn<{self.HB},{self.NW}>"

    @staticmethod
    def rows_of(seg, P):
        """The position-to-row map of a segment (RgAttnAddr::row) for positions 0 .. P - 1."""
        n, pos0, base, pfx, prow = seg
        p = np.arange(P)
        return np.where(p < pfx, prow + p, base + p)

    def run_rg(self, segs, tag, probes=(), layouts=None, copy_from=None):
        """One k_rg_attn pass of `segs` (tokens, pos0, base, pfx_len, pfx_row0; segment s takes the query rows that
        follow segment s - 1's) in every layout.  probes: (class, segment, token, timestep).  copy_from: (rows, K, V)
        host rows written over the base data first (the unshared twin's copied prefix).  Returns
        (stored bits [16 tiles, dim], the slab columns of every segment's valid tokens)."""
        hs, kvh, kv_mul = self.hs, self.kvh, self.kv_mul
        tiles, cols, qrow, twin = [], [], [], []
        q0 = 0
        for n, pos0, base, pfx, prow in segs:
            mine = []
            for o in range(0, n, 16):
                nv = min(16, n - o)
                k = len(tiles)
                tiles.append((pos0 + o, nv, base, pfx, prow))
                mine += [16 * k + i for i in range(nv)]
                twin += [16 * k + min(i, nv - 1) for i in range(16)]
            cols.append(np.array(mine))
            qrow.append(q0 + np.arange(n))
            q0 += n
        nt = len(tiles)
        assert nt <= 32 and q0 <= TMAX
        table = np.array(tiles, dtype=np.int32).T   # [5][n_tiles]
        twin = np.array(twin)
        q = self.q.copy()
        readable = np.zeros(SEQ, bool)
        for seg in segs:
            rows = self.rows_of(seg, seg[1] + seg[0])
            assert rows.min() >= 0 and rows.max() < SEQ
            readable[rows] = True
        kmods, placed = [], []
        for g, (cls, s, t, r) in enumerate(probes):
            assert g < kvh
            h = g * kv_mul + (len(probes) + g) % kv_mul
            n, pos0 = segs[s][0], segs[s][1]
            tq = qrow[s][t]
            if cls == "leak":
                assert r == pos0 + t + 1 < pos0 + n
                q[tq + 1, h * hs:(h + 1) * hs] = q[tq, h * hs:(h + 1) * hs]
            else:
                assert 0 <= r <= pos0 + t
            kmods.append((int(self.rows_of(segs[s], r + 1)[r]), g, self.key(q, tq, h)))
            placed.append((cls, s, t + 1 if cls == "leak" else t, h, r))
        if copy_from is not None:
            saved = self.kb[copy_from[0]].copy(), self.vb[copy_from[0]].copy()
            self.kb[copy_from[0]], self.vb[copy_from[0]] = copy_from[1], copy_from[2]
        try:
            k, v = self.upload(readable, kmods)
        finally:
            if copy_from is not None:
                self.kb[copy_from[0]], self.vb[copy_from[0]] = saved
        # the slab: valid columns hold their query, the padding columns' own query rows are read by nobody
        slab = np.full((16 * nt, self.dim), np.nan, np.float32)
        gold = np.empty((16 * nt, self.dim))
        for s, seg in enumerate(segs):
            n, pos0 = seg[0], seg[1]
            slab[cols[s]] = q[qrow[s]]
            rows = self.rows_of(seg, pos0 + n)
            if not probes and copy_from is None and seg[2:] == (0, 0, 0) and qrow[s][0] == 0:
                gs = self.gold_pg(pos0)[:n]   # k_pg_attn's slice: the same tokens over the same rows
            else:
                gs, pmax = _gold(q[qrow[s]], pos0 + np.arange(n), k[rows], v[rows], self.heads, kvh, hs)
                for cls, ps, t, h, r in placed:
                    if ps == s:
                        assert pmax[t, h] > 0.99, f"{self.what()} {tag} probe {cls} segment {s} token {t} timestep {r}: " \
                                                  f"probability {pmax[t, h]} in the gold"
                        vrow = v[rows[r], (h // kv_mul) * hs:(h // kv_mul + 1) * hs]
                        assert np.abs(gs[t, h * hs:(h + 1) * hs] - vrow).max() < 0.1
            assert np.isfinite(gs).all(), f"{tag}: the gold read a row outside the readable set"
            gold[cols[s]] = gs
        gold = gold[twin]
        qd = torch.from_numpy(slab).to(self.gpu)
        inst = self.rg_inst()
        first = None
        for layout in layouts or self.layouts:
            got = self.launch("rg", table, layout, 16 * nt, _tcap(16 * nt), qd, inst)
            what = f"{self.what()} {inst} {tag} layout {layout}"
            self.check(got, gold, what, "k_rg_attn")
            bits = got.view(np.int32)
            assert np.array_equal(bits, bits[twin]), f"{what}: a padding column differs from the column it repeats"
            if first is None:
                first = bits
            else:
                assert np.array_equal(bits, first), f"{what}: bits differ between layouts"
        _n_pt_cells(inst, [((t[0] + t[1] - 1) >> 4) + 1 for t in tiles], self.NW)
        if any(t[1] < 16 for t in tiles):
            _cell(inst, "partial-q-tile")
            _cell(inst, "padding-twin")
        if any(t[3] > 0 for t in tiles):
            _cell(inst, "prefix")
        if any(t[2] < 0 for t in tiles):
            _cell(inst, "negative-base")
        if nt == 32:
            _cell(inst, "32-tiles")
        for cls, s, t, h, r in placed:
            _cell(inst, "p:" + cls)
        return first, cols

    def rg_probes(self):
        NW = self.NW
        s3, s4 = 2, 3
        p4 = MIXED[s4][1]
        return [("t0", s4, 0, 0), ("own", s4, 15, p4 + 15), ("own", s4, 39, p4 + 39), ("below-pos0", s4, 16, p4 - 1),
                ("pos0", s4, 17, p4), ("tile-lo", s4, 20, 1023), ("tile-hi", s4, 21, 1024),
                ("round-lo", s4, 22, 16 * NW - 1), ("round-hi", s4, 23, 16 * NW), ("ring-lo", s4, 24, 32 * NW - 1),
                ("ring-hi", s4, 25, 32 * NW), ("pfx-lo", s4, 26, 47), ("pfx-hi", s4, 27, 48), ("leak", s4, 30, p4 + 31),
                ("leak", s4, 15, p4 + 16), ("pfx-lo", s3, 3, 36), ("pfx-hi", s3, 4, 37), ("own", s3, 16, 316),
                ("t0", s3, 1, 0), ("tile-hi", s3, 9, 304)]


def _geo(gpu, heads, kvh, hs):
    if (heads, kvh, hs) not in _GEOS:
        _GEOS[(heads, kvh, hs)] = _Geo(gpu, heads, kvh, hs)
    return _GEOS[(heads, kvh, hs)]


def _clear_hooks():
    for k in ("KH_PG_ATTN_QT", "KH_LAUNCH_LOG"):
        _ffi.debug_set(k, None)


@pytest.mark.parametrize("heads,kvh,hs", GEOMETRIES)
def test_gold_agrees_with_the_oracle(gpu, oracle, heads, kvh, hs):
    """_gold() against oracle.mha(..., ACC_F64) at a handful of tokens of a deep and a shallow slice.  The oracle
    rounds its scores to fp32 and runs softmax and P V in fp32, so it stands about 1e-6 from a full fp64 result; the
    two must agree within a tenth of the kernel's bound."""
    geo = _geo(gpu, heads, kvh, hs)
    worst = 0.0
    for pos0, toks in ((2085, (0, 17, 300, 511)), (5, (0, 31, 128)), (0, (0,))):
        gold = geo.gold_pg(pos0)
        for t in toks:
            oo, _ = oracle.mha(pos0 + t, heads, 0, SEQ, geo.kv_dim, geo.kv_mul, hs, geo.q[t], geo.kb[None], geo.vb[None],
                               acc=oracle.ACC_F64)
            err = np.abs(oo - gold[t])
            worst = max(worst, float(err.max()))
            assert (err <= 0.1 * (ATOL + RTOL * np.abs(gold[t]))).all(), f"pos0 {pos0} token {t}: {err.max():.3e}"
    print(f"({heads},{kvh},{hs}): worst |oracle fp64 - gold| {worst:.3e}")


@pytest.mark.parametrize("heads,kvh,hs", GEOMETRIES)
def test_pg_attn_geometry(gpu, heads, kvh, hs):
    """k_pg_attn: PG_CASES under every KH_PG_ATTN_QT and layout, then the seam probes (module docstring)."""
    geo = _geo(gpu, heads, kvh, hs)
    try:
        if (heads, kvh, hs) == (16, 4, 64):  # the launch's own choice of QT > 1
            assert geo.pg_inst(None, 2047, 512).endswith(",1>") and geo.pg_inst(None, 2048, 512).endswith(",2>")
            assert geo.pg_inst(None, 2085, 512).endswith(",2>") and geo.pg_inst(None, 2085, 480).endswith(",1>")
        if hs == 128:
            assert geo.pg_inst(4, 0, 512) == "k_pg_attn<8,4,2>"
        n = 0
        for pos0, T in PG_CASES:
            geo.run_pg(pos0, T, geo.gold_pg(pos0)[:T])
            n += len(QTS) * len(geo.layouts)
        n += geo.run_pg_probes()
    finally:
        _clear_hooks()
    _DONE.add(("pg", heads, kvh, hs))
    print(f"({heads},{kvh},{hs}): {n} launches, worst |out - gold| at head size {hs} so far "
          f"{_WORST[('k_pg_attn', hs)]:.3e}")


@pytest.mark.parametrize("heads,kvh,hs", GEOMETRIES)
def test_rg_attn_geometry(gpu, heads, kvh, hs):
    """k_rg_attn: one tile, lone aligned segments against k_pg_attn<HB, NW, 1>'s bits, the mixed pass with its
    unshared twins, padding columns, seam probes (module docstring)."""
    geo = _geo(gpu, heads, kvh, hs)
    inst = geo.rg_inst()
    try:
        geo.run_rg([(5, 7, 100, 0, 0)], "one tile")
        for n, pos0 in ((512, 2085), (100, 5)):
            bits, cols = geo.run_rg([(n, pos0, 0, 0, 0)], f"lone aligned segment at {pos0}")
            pg = geo.run_pg(pos0, n, geo.gold_pg(pos0)[:n], qts=(1,), layouts=(L_ROWS,))[1]
            assert np.array_equal(bits[cols[0]], pg.view(np.int32)), \
                f"{geo.what()} {inst}: lone aligned segment of {n} tokens at {pos0} differs from k_pg_attn<..,1>"
            _cell(inst, "bits=k_pg_attn")
        mixed, cols = geo.run_rg(MIXED, "mixed pass")
        for s in (2, 3, 4):  # the sharers, unshared: the prefix rows copied in front of the segment's own rows
            n, pos0, base, pfx, prow = MIXED[s]
            b2 = max(base, 3)   # the sharer with the negative base has no room in front of its own rows: moved
            rows = _Geo.rows_of(MIXED[s], pos0 + n)
            dst = b2 + np.arange(pos0 + n)
            qoff = sum(m[0] for m in MIXED[:s])
            saved_q = geo.q.copy()
            geo.q[:n] = saved_q[qoff:qoff + n]
            try:
                bits, c2 = geo.run_rg([(n, pos0, b2, 0, 0)], f"segment {s} unshared", layouts=(L_ROWS,),
                                      copy_from=(dst, geo.kb[rows].copy(), geo.vb[rows].copy()))
            finally:
                geo.q[:] = saved_q
            assert np.array_equal(bits[c2[0]], mixed[cols[s]]), \
                f"{geo.what()} {inst}: segment {s} of the mixed pass differs from its unshared run"
        pr = geo.rg_probes()
        for i in range(0, len(pr), kvh):
            lay = [geo.layouts[(i // kvh) % len(geo.layouts)]]
            geo.run_rg(MIXED, f"mixed pass, probes {pr[i:i + kvh]}", probes=pr[i:i + kvh], layouts=lay)
    finally:
        _clear_hooks()
    _DONE.add(("rg", heads, kvh, hs))
    print(f"({heads},{kvh},{hs}): worst |out - gold| of k_rg_attn at head size {hs} so far {_WORST[('k_rg_attn', hs)]:.3e}")


def test_argument_errors(gpu):
    """One case per validation rule of kh_mha_prefill_layout_f32 and kh_mha_prefill_tiles_f32: each raises, with the
    error kind kh_mha_prefill_f32 has for that fault, before anything is launched."""
    from kuiperllama_amd import ops
    heads, kvh, hs, seq = 4, 2, 64, 256
    dim, kv_dim, kv_mul = heads * hs, kvh * hs, heads // kvh
    out = torch.zeros(dim * 512 + 8, device=gpu)
    q = torch.zeros(512 * dim + 8, device=gpu)
    kc = torch.zeros(2 * seq * kv_dim + 8, device=gpu)

    def layout(pos0=0, T=16, layout=L_F32, tcap=128, heads=heads, hs=hs, kv_dim=kv_dim, o=out):
        ops.mha_prefill_layout(pos0, T, heads, 0, seq, kv_dim, kv_mul, hs, layout, tcap, o, q, kc, kc)

    def tiles(t, layout=L_F32, tcap=128, hs=hs, kv_dim=kv_dim, heads=heads, o=out, qq=q):
        ops.mha_prefill_tiles(np.array(t, dtype=np.int32).reshape(-1, 5).T, heads, 0, seq, kv_dim, kv_mul, hs, layout,
                              tcap, o, qq, kc, kc)

    _ffi.debug_set("KH_LAUNCH_LOG", "1")
    try:
        layout()                           # the valid twins of everything below
        tiles([7, 5, 10, 3, 100])
        assert len(_ffi.launch_log()) == 2
        _ffi.debug_set("KH_LAUNCH_LOG", "1")
        INV, UNS, RNG = _ffi.KH_ERR_INVALID_ARG, _ffi.KH_ERR_UNSUPPORTED, _ffi.KH_ERR_RANGE
        cases = [
            ("n_tokens > tcap", INV, lambda: layout(T=129)),
            ("tcap > 512", INV, lambda: layout(tcap=528)),
            ("tcap % 16", INV, lambda: layout(tcap=120)),
            ("layout 3", INV, lambda: layout(layout=3)),
            ("int8 slab, dim % 64", INV, lambda: layout(layout=L_Q8, heads=6, hs=48, kv_dim=3 * 48)),
            ("n_tokens 0", INV, lambda: layout(T=0)),
            ("slice past the cache", RNG, lambda: layout(pos0=seq - 8)),
            ("head size 32", UNS, lambda: layout(hs=32, kv_dim=kvh * 32)),
            ("misaligned out", INV, lambda: layout(o=out[1:])),
            ("no tile", INV, lambda: tiles([])),
            ("33 tiles", INV, lambda: tiles([0, 16, 0, 0, 0] * 33, tcap=512)),
            ("nvalid 0", INV, lambda: tiles([7, 0, 10, 0, 0])),
            ("nvalid 17", INV, lambda: tiles([7, 17, 10, 0, 0])),
            ("pfx_len < 0", INV, lambda: tiles([7, 5, 10, -1, 100])),
            ("pfx_len > pos0", INV, lambda: tiles([7, 5, 10, 8, 100])),
            ("pos0 < 0", INV, lambda: tiles([-1, 5, 10, 0, 0])),
            ("prefix rows below 0", RNG, lambda: tiles([7, 5, 10, 3, -1])),
            ("prefix rows past the cache", RNG, lambda: tiles([7, 5, 10, 3, seq - 2])),
            ("own rows below 0", RNG, lambda: tiles([7, 5, -4, 3, 100])),
            ("own rows past the cache", RNG, lambda: tiles([7, 5, seq - 11, 3, 100])),
            ("a later tile's rows past the cache", RNG, lambda: tiles([7, 5, 10, 3, 100, 7, 5, seq - 11, 3, 100])),
            ("16 n_tiles > tcap", INV, lambda: tiles([0, 16, 0, 0, 0] * 9, tcap=128)),
            ("tiles: tcap % 16", INV, lambda: tiles([7, 5, 10, 3, 100], tcap=120)),
            ("tiles: misaligned q", INV, lambda: tiles([7, 5, 10, 3, 100], qq=q[1:])),
            ("tiles: head size 32", UNS, lambda: tiles([7, 5, 10, 3, 100], hs=32, kv_dim=kvh * 32)),
            ("tiles: kv_dim", INV, lambda: tiles([7, 5, 10, 3, 100], kv_dim=kv_dim + 16)),
        ]
        for name, code, call in cases:
            with pytest.raises(_ffi.KhError) as ei:
                call()
            assert ei.value.code == code, f"{name}: {ei.value}"
        assert _ffi.launch_log() == set(), "a refused call launched something"
        with pytest.raises(ValueError):
            ops.mha_prefill_tiles(np.zeros((4, 1), np.int32), heads, 0, seq, kv_dim, kv_mul, hs, 0, 128, out, q, kc, kc)
    finally:
        _clear_hooks()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- gates
@pytest.fixture(scope="module")
def compiled():
    assert co.tools_present(), "the LLVM tools of the ROCm install are needed to read the library's code objects"
    build.build_lib()
    return co.kernels(co.code_object_notes(_ffi.LIB_PATH), {"k_pg_attn", "k_rg_attn"})


def _all_ran():
    want = {(k,) + g for g in GEOMETRIES for k in ("pg", "rg")}
    missing = sorted(map(str, want - _DONE))
    assert not missing, f"tests that did not run to the end (run the whole module): {missing}"


def test_coverage_gate(gpu, compiled):
    """Every compiled k_pg_attn and k_rg_attn instantiation was launched and checked, and nothing launched is missing
    from the code objects."""
    _all_ran()
    for stem in ("k_pg_attn", "k_rg_attn"):
        comp = {k for k in compiled if k.split("<")[0] == stem}
        assert comp, f"no {stem} instantiation in the library"
        print(f"{stem}: {len({k for k in _LAUNCHED if k.split('<')[0] == stem})} of {len(comp)} compiled "
              "instantiations launched and checked")
    print("worst |out - gold| per kernel and head size: " +
          ", ".join(f"{k} hs {hs}: {e:.3e}" for (k, hs), e in sorted(_WORST.items())))
    assert _LAUNCHED <= compiled, f"launched but not found in the code objects: {sorted(_LAUNCHED - compiled)}"
    gap = compiled - _LAUNCHED
    assert not gap, f"compiled and never launched: {sorted(gap)}"


def test_cell_gate(gpu, compiled):
    """The cell table (module docstring) has no missing cell; a cell listed unreachable was not reached."""
    _all_ran()
    missing, lines = [], []
    for inst in sorted(compiled):
        stem = inst.split("<")[0]
        qt = int(inst[:-1].split(",")[2]) if stem == "k_pg_attn" else 1
        for cell in PG_CELLS if stem == "k_pg_attn" else RG_CELLS:
            n = _CELLS.get((inst, cell), 0)
            why = UNREACHABLE.get((stem, qt, cell))
            lines.append(f"  {inst:18s} {cell:20s} {'UNREACHABLE: ' + why if why else str(n) + ' checked launches'}")
            if why:
                assert n == 0, f"{inst} {cell}: documented unreachable ({why}) but reached {n} times"
            elif n == 0:
                missing.append(f"{inst} {cell}")
    print("cell table:\n" + "\n".join(lines))
    assert not missing, f"cells never launched: {missing}"
