"""Gate of the sampler core (csrc/kh_sample.h: kh_sample_core) and of the top-N selection built on its machinery
(csrc/kh_logprobs.h): exact picks on rows where the device's arithmetic has no rounding, at every edge of its control
flow, through the operators ops.sample / ops.sample_host / ops.logprobs and through the decode step's sampled tails.

Exact rows.  fx_of_e weighs a token with exactly 2^sb at e == 0 and exactly 0 at e <= -104 (or l = -inf), so on a
TWO-LEVEL row - a set A at the maximum, everything else at a zero-weight level - the kept set and the pick are integers
(tests/sampling_ref.py: two_level_pick) and every draw is compared with ==: no Checker, no tolerance.  A third, weighted
level appears only where 0 < K <= |A| cuts it off.  Each configuration is 64 consecutive counters plus the two
counters with the smallest and the largest u among the first 2^20 of the seed (the first and the last index of S),
drawn twice (bit-reproducible).  Vocabulary sizes 1 .. 2^19 + 19 (V % 16 in {0, 1, 15}, V < 16, both sides of every
index-digit seam and of KH_SAMP_CAP); |A| in 1, 2, 255 .. 257, 4095 .. 4097, V; A at the first indices (a), the last -
the scalar tail of the 16-wide loads - (b), across index 256 (c), across 2^19 (d), every 16th index (e), random (f);
the low level at h - 128 T and at -inf; T in 1, 0.02, 50; K in 0, 1, |A| - 1, |A|, |A| + 1, V - 1, V; P in 1, 0.5,
0.999, 1e-6, a P with P32 * n an exact integer, and the two fp32 neighbours of (n - 1) / n (P32 * n just above n - 1:
m = n, the only way to m == ties with top-p on more than 1000 tokens; just below or at it: m = n - 1).

Table.  tests/sampling_ref.py: predict_path states, from the header's rules alone, which branches a row takes.  Every
cell of {candidates in LDS, in global memory} x {top-k only, top-p only, both, neither} x {index cut runs, does not} x
{1, 2, 3 index levels} is populated by checked draws, except the 14 cells of UNREACHABLE (each with its reason):
34 populated cells.

Natural rows (the unchanged Checker): both candidate sources on one row at the K where the candidate count crosses
KH_SAMP_CAP - picks equal wherever the fp64 threshold is farther than 1e-4 Z (ten times Checker.TOL) from every
boundary of both kept sets; the share of draws this leaves out is computed by the reference alone and must be at most
10 % - and the tail of the weight function: T = 0.02 and 0.005, where the K-th token falls into the last first-pass bin
and most weights underflow to zero.

Top-N of the log-prob operator on the same two-level rows (ids exact, floats within logprobs_ref.tol), and one
model-level test: real logits with five bit-equal rows across the index seam, the three sampled step tails
(k_sample_topp, k_sample_proc, k_sample_lp) token by token against ops.sample_host on the model's own logits.

Measured on an MI355X: 128 exact configurations and the six unaligned / shifted runs, 8844 draws compared with ==
in 536 launches, no mismatch and no call that drew other tokens the second time; 34 cells populated, 14 unreachable.
Source equivalence: K = 4062 (4062 candidates, LDS) against 4063 (4121, global), 512 draws, 1.2 % left out.  Model:
top-k 3 cuts inside the five-way tie in 34 of the 44 sampled steps of the two runs without processors.  Module wall
time: 3.4 s (32 tests, about 640 launches).  What the gate notices, tried once with one-line, memory-safe changes to the
kernels: the tie cut `i < i_cut` in kh_sample_core's in_s, index i + 14 for the last lane of the 16-wide load, and
"exceeds P" for "reaches P" in the top-p count m each fail test_exact_rows (the last one passes every operator test of
test_sampling_gpu.py: only a P with P32 * n an exact integer tells the two apart); `i < i_cut` among the survivors of
kh_logprobs_core fails every row of test_top_n_cuts_inside_the_tie_run.
"""
import itertools
import time
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest
import torch

import logprobs_ref as L
import sampling_ref as R
from kuiperllama_amd import _ffi, binfmt, ops
from test_logprobs_gpu import FLAT_SPEC
from test_sampling_gpu import _logits

pytestmark = pytest.mark.gpu

INF = float("inf")
H = 3.0  # the maximum of every two-level row
V19 = (1 << 19) + 19
VS = [1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 4111, 32000, 151936, V19]
SIZES = [1, 2, 255, 256, 257, 4095, 4096, 4097]  # |A|; and V where it fits
TS = (1.0, 0.02, 50.0)
K_KINDS = ("0", "1", "|A|-1", "|A|", "|A|+1", "V-1", "V")
P_KINDS = ("1", "0.5", "0.999", "1e-6", "exact", "above", "below")
PLACES = {"a": "first indices", "b": "last indices", "c": "across index 256", "d": "across index 2^19",
          "e": "every 16th index", "f": "random"}
SEEDS = (0x5EED_0123_4567_89AB, 77)
N_DRAWS = 64

SOURCES, MODES, LEVELS = ("LDS", "global"), ("top-k only", "top-p only", "both", "neither"), (1, 2, 3)
# cells of the table no input can reach, with the reason
UNREACHABLE = {}
for _s, _l in itertools.product(SOURCES, LEVELS):
    UNREACHABLE[(_s, "neither", True, _l)] = "without top-k and top-p nothing bounds S: no boundary key, no index cut"
for _m, _c in itertools.product(MODES, (True, False)):
    UNREACHABLE[("global", _m, _c, 1)] = ("one index level means V < 256, and at most V <= KH_SAMP_CAP candidates "
                                          "always fit into LDS")
UNREACHABLE[("LDS", "neither", False, 3)] = ("three index levels mean V >= 2^19 > KH_SAMP_CAP, and without top-k and "
                                             "top-p every token is a candidate")

_CELLS = Counter()    # cell -> exact draws checked in it (filled by test_exact_rows, read by the gate)
_COVER = Counter()    # ("|A|" | "place" | "K" | "P" | "T" | "low" | "descent" | ..., value) -> configurations
_RAN = set()          # vocabulary sizes whose test ran to the end
_STATS = Counter()    # configurations, draws, launches of the exact rows
_T0 = time.perf_counter()


# ---- two-level rows ---------------------------------------------------------------------------------------------------
def _place(V, nA, place):
    """ascending indices of A, or None where the placement does not exist at this (V, |A|)"""
    if nA == V:
        return np.arange(V) if place == "a" else None
    if place == "a":
        return np.arange(nA)
    if place == "b":
        return np.arange(V - nA, V)
    if place == "c":
        s = 256 - nA // 2
        return np.arange(s, s + nA) if s >= 0 and s + nA <= V and V > 256 else None
    if place == "d":  # centred where the row is long enough behind 2^19, else ending at the row's end
        s = min((1 << 19) - nA // 2, V - nA)
        return np.arange(s, s + nA) if V > (1 << 19) and 0 <= s < (1 << 19) else None
    if place == "e":  # one token per 16-index run of a thread: the histogram's run merging never merges
        return 16 * np.arange(nA) + 5 if 16 * nA <= V else None
    return np.sort(np.random.default_rng(31 * V + nA).choice(V, nA, replace=False))


def _resolve(V, nA, k_kind, p_kind):
    K = {"0": 0, "1": 1, "|A|-1": nA - 1, "|A|": nA, "|A|+1": nA + 1, "V-1": V - 1, "V": V}[k_kind]
    n = R.two_level_kept(nA, V, K, 1.0)[0]
    if p_kind in ("1", "0.5", "0.999", "1e-6"):
        P = float(p_kind)
    elif p_kind == "exact":  # P32 * n an exact integer: the >= edge of the top-p prefix (odd n: no such P below 1)
        P = 0.75 if n % 4 == 0 else 0.5
    elif n == 1:
        P = 0.5
    else:  # the fp32 neighbours of (n - 1) / n
        p = np.float32((n - 1) / n)
        over = Fraction(float(p)) * n > n - 1
        if p_kind == "above":
            p = p if over else np.nextafter(p, np.float32(1))
            assert p < 1 and Fraction(float(p)) * n > n - 1 and R.two_level_kept(nA, V, K, p)[1] == n
        else:
            p = np.nextafter(p, np.float32(0)) if over else p
            assert n - 2 < Fraction(float(p)) * n <= n - 1 and R.two_level_kept(nA, V, K, p)[1] == n - 1
        P = float(p)
    return K, P


def _row(V, A, T, low_inf, third):
    """fp32 two-level row: A at H, the rest at H - 128 T (e = -128) or -inf; `third`: the first, the middle and the
    last token outside A at H - 3 T (weight about e^-3)"""
    lg = np.full(V, -INF if low_inf else H - 128.0 * T, np.float32)
    lg[A] = H
    if third:
        rest = np.setdiff1d(np.arange(V), A)
        lg[rest[[0, rest.size // 2, -1]]] = H - 3.0 * T
    return lg


def _build_configs():
    """-> {V: [(|A|, place, low_inf, T, k_kind, p_kind), ...]}: a rotation over the pairs (V, |A|) that walks the
    7 x 7 (K, P) kinds, the placements, T and the low level; one configuration per reachable table cell and index-level
    count; and the named edges.  No full product."""
    out = {V: [] for V in VS}
    i = 0

    def add(V, nA, place, k_kind, p_kind, T=None, low_inf=None):
        nonlocal i
        cfg = (nA, place, bool((i // 3) % 2) if low_inf is None else low_inf, TS[i % 3] if T is None else T, k_kind,
               p_kind)
        assert _place(V, nA, place) is not None, (V, nA, place)
        if cfg not in out[V]:
            out[V].append(cfg)
        i += 1

    # 1. rotation: every V with the sizes that fit (four of them per V from 4095 on), the (K, P) kinds on a walk of
    #    stride 3 over the 49 pairs, the placements that exist in turn
    for vi, V in enumerate(VS):
        sizes = sorted({a for a in SIZES + [V] if a <= V})
        if len(sizes) > 5:
            sizes = [sizes[(vi + 2 * j) % len(sizes)] for j in range(4)] + [V]
        for nA in sorted(set(sizes)):
            feas = [p for p in PLACES if _place(V, nA, p) is not None]
            kp = (3 * i) % 49
            add(V, nA, feas[i % len(feas)], K_KINDS[kp % 7], P_KINDS[kp // 7])
    # 2. the table: per index-level count and source, every (mode, index cut) - (K kind, P kind) that produce it
    fill = {("top-k only", True): ("|A|-1", "1"), ("top-k only", False): ("|A|", "1"),
            ("top-p only", True): ("0", "0.5"), ("top-p only", False): ("0", "above"),
            ("both", True): ("|A|-1", "exact"), ("both", False): ("|A|", "above"), ("neither", False): ("0", "1")}
    for V, nA, place in ((255, 255, "a"), (4111, 257, "c"), (4111, 4097, "b"), (V19, 257, "d"), (V19, 4097, "d")):
        for k_kind, p_kind in fill.values():
            add(V, nA, place, k_kind, p_kind)
    # 3. named edges
    for V in (15, 17, 255, 257, 4097, 4111, 151936, V19):  # the interesting tokens in the scalar tail of the loads
        add(V, 2, "b", "1", "1")
        add(V, 2, "b", "|A|+1", "0.5")
    for V, nA in ((257, 2), (4111, 256), (151936, 257)):  # across index 255 / 256
        add(V, nA, "c", "|A|-1", "1")
        add(V, nA, "c", "0", "0.5")
    for nA in (2, 256):  # across index 2^19 - 1 / 2^19: the two bins of the top index level
        add(V19, nA, "d", "|A|-1", "1")
        add(V19, nA, "d", "0", "below")
    for V in (4096, 4097):  # every token a candidate (K beyond the weighted tokens, or no top-k): LDS up to V = 4096
        add(V, 2, "f", "|A|+1", "1", low_inf=False)
        add(V, 2, "f", "V-1", "0.999", low_inf=True)
        add(V, V, "a", "0", "1")
    for nA in (4095, 4096, 4097):  # the compaction switch at ncand == KH_SAMP_CAP
        add(151936, nA, "e", "|A|", "0.5")
        add(32000, nA, "b", "|A|-1", "0.999")
    return out


CONFIGS = _build_configs()
_EXTREME = {}


def _extreme(seed):
    if seed not in _EXTREME:
        _EXTREME[seed] = R.extreme_counters(seed)
    return _EXTREME[seed]


def _third(V, nA, K):
    return 0 < K <= nA and K < V and V - nA >= 3 and (V + nA + K) % 2 == 0


def _cell(path):
    return ("LDS" if path["in_lds"] else "global", path["mode"], path["index_cut"], path["levels"])


def _draw(lg_d, T, K, P, seed, n, counter0=0):
    out = torch.empty(n, dtype=torch.int32, device=lg_d.device)
    ops.sample(lg_d, out, dict(temperature=T, top_k=K, top_p=P, seed=seed), counter0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _exact_config(lg_d, A, V, T, K, P, seed, counter0):
    """the 64 + 2 draws of one configuration, twice -> (counters, picks, two_level_pick's picks)"""
    c_lo, c_hi = _extreme(seed)
    counters = list(range(counter0, counter0 + N_DRAWS)) + [c_lo, c_hi]
    params = _ffi.sampling(T, K, P, seed)
    got = _draw(lg_d, T, K, P, seed, N_DRAWS, counter0).tolist()
    again = _draw(lg_d, T, K, P, seed, N_DRAWS, counter0).tolist()
    assert again == got, f"V={V} |A|={len(A)} T={T} K={K} P={P}: a second call drew other tokens"
    got += [ops.sample_host(lg_d, params, c_lo), ops.sample_host(lg_d, params, c_hi)]
    want = [R.two_level_pick(A, V, K, P, seed, c) for c in counters]
    if V > 1:  # the two extreme counters are the first and the last index of S
        m = R.two_level_kept(len(A), V, K, P)[1]
        assert want[-2:] == [int(A[0]), int(A[m - 1])], (V, len(A), K, P, want[-2:])
    _STATS["launches"] += 4
    return counters, got, want


@pytest.mark.parametrize("V", VS)
def test_exact_rows(gpu, V):
    bad, n_cfg = [], 0
    for ci, (nA, place, low_inf, T, k_kind, p_kind) in enumerate(CONFIGS[V]):
        A = _place(V, nA, place)
        K, P = _resolve(V, nA, k_kind, p_kind)
        third = _third(V, nA, K)
        lg = _row(V, A, T, low_inf, third)
        path = R.predict_path(lg, T, K, P)
        seed = SEEDS[ci % 2]
        counters, got, want = _exact_config(torch.from_numpy(lg).to(gpu), A, V, T, K, P, seed, 1000 * ci + V % 997)
        what = (f"V={V} |A|={nA} {PLACES[place]} low={'-inf' if low_inf else 'h-128T'} T={T} K={K} ({k_kind}) P={P!r} "
                f"({p_kind}){' third level' if third else ''} {path}")
        for c, g, w in zip(counters, got, want):
            if g != w:
                bad.append(f"{what}: counter {c} drew {g}, the exact pick is {w}")
        if not path["trivial"]:
            _CELLS[_cell(path)] += len(counters)
            for d in path["descents"]:
                _COVER[("descent", d)] += 1
            _COVER[("m_key < ties", path["m_key_lt_ties"])] += 1
            if path["mode"] == "top-k only":
                _COVER[("top-k m_key vs ties", "==" if path["m_key"] == path["ties"] else "<")] += 1
                _COVER[("top-k beyond the weighted tokens", K > nA)] += 1
        for k, v in (("|A|", "V" if nA == V else nA), ("place", place), ("K", k_kind), ("P", p_kind), ("T", T),
                     ("low", low_inf), ("third", third)):
            _COVER[(k, v)] += 1
        _STATS["draws"] += len(counters)
        n_cfg += 1
    _STATS["configs"] += n_cfg
    _RAN.add(V)
    assert not bad, f"{len(bad)} exact draws differ:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("src", SOURCES)
def test_exact_rows_unaligned_and_shifted(gpu, src):
    """the same configuration with the row at lg_d[1:] (no 16-byte alignment: the scalar loop reads everything) and at
    lg_d[4:] (aligned, shifted: 16-wide loads and a 15-token tail that holds the end of A)"""
    V, nA = 4111, 257 if src == "LDS" else 4097
    A = _place(V, nA, "b")
    K, P = _resolve(V, nA, "|A|-1", "0.5")
    lg = _row(V, A, 0.02, False, True)
    path = R.predict_path(lg, 0.02, K, P)
    assert _cell(path) == (src, "both", True, 2)
    ref = None
    for off in (0, 1, 4):
        buf = torch.full((V + 4,), 7.0, dtype=torch.float32, device=gpu)  # a larger value around the row: never read
        buf[off:off + V] = torch.from_numpy(lg).to(gpu)
        view = buf[off:off + V]
        assert (view.data_ptr() % 16 == 0) == (off != 1)
        counters, got, want = _exact_config(view, A, V, 0.02, K, P, SEEDS[0], 500)
        assert got == want, (src, off, [(c, g, w) for c, g, w in zip(counters, got, want) if g != w][:10])
        ref = got if ref is None else ref
        assert got == ref
        _STATS["draws"] += len(counters)


# ---- natural rows: the unchanged Checker ------------------------------------------------------------------------------
def _ncand(b, K):
    """candidates of top-k K from the first-pass bins b: the tokens of the bins up to the K-th token's"""
    cum = np.cumsum(np.bincount(b, minlength=R.SAMP_NB))
    return int(cum[np.searchsorted(cum, K, side="left")])


def _boundary_distance(lg, T, K, us):
    """per draw: distance of the fp64 threshold u * Z_S from the nearest boundary of the index-order walk over the
    kept set of top-k K, in units of Z_S"""
    S, w, _ = R.kept_set(lg, T, K, 1.0)
    cum = np.cumsum(w[np.argsort(S, kind="stable")])
    edges = np.concatenate([[0.0], cum])
    thr = us * cum[-1]
    j = np.searchsorted(edges, thr)
    below, above = edges[np.maximum(j - 1, 0)], edges[np.minimum(j, edges.size - 1)]
    return np.minimum(np.abs(thr - below), np.abs(above - thr)) / cum[-1]


def test_both_candidate_sources_draw_the_same_tokens(gpu):
    """One natural row, top-k at the K where the candidate count crosses KH_SAMP_CAP: K (compacted into LDS) and K + 1
    (re-read from global memory) with the same counters.  T = 0.5 makes the row peaked enough that the reference alone
    leaves at most 10 % of the draws within 1e-4 Z of a boundary."""
    V, T, seed, n = 32000, 0.5, 0xBEEF, 512
    lg = _logits("peaked", V)
    _, b = R.bins_f32(lg, T)
    K = max(k for k in range(3000, R.SAMP_CAP + 1) if _ncand(b, k) <= R.SAMP_CAP)
    assert _ncand(b, K) <= R.SAMP_CAP < _ncand(b, K + 1)
    lg_d = torch.from_numpy(lg).to(gpu)
    ch = R.Checker(lg)
    counters = np.arange(40, 40 + n)
    us = np.array([R.uniform(seed, int(c)) for c in counters])
    picks = {}
    for k in (K, K + 1):
        picks[k] = _draw(lg_d, T, k, 1.0, seed, n, counter0=40)
        ok = ch.accepts(T, k, 1.0, seed, counters, picks[k])
        assert ok.all(), f"K={k}: {int((~ok).sum())} draws rejected, first counter {40 + int(np.argmin(ok))}"
    far = (_boundary_distance(lg, T, K, us) > 1e-4) & (_boundary_distance(lg, T, K + 1, us) > 1e-4)
    left_out = 1.0 - far.mean()
    print(f"source equivalence: K = {K} ({_ncand(b, K)} candidates, LDS) and {K + 1} ({_ncand(b, K + 1)}, global); "
          f"{n} draws, {100 * left_out:.1f} % within 1e-4 Z of a boundary and left out")
    assert left_out <= 0.10
    assert (picks[K][far] == picks[K + 1][far]).all(), np.flatnonzero(far & (picks[K] != picks[K + 1]))[:10]


@pytest.mark.parametrize("kind", ["peaked", "tied"])
@pytest.mark.parametrize("T", [0.02, 0.005])
def test_tail_of_the_weight_function(gpu, kind, T):
    """(l_max - l) / T beyond 64 (the last first-pass bin) and beyond 104 (weight zero) on natural rows"""
    V, seed, n = 32000, 0x7A11 + int(1000 * T), 128
    lg = _logits(kind, V)
    e, b = R.bins_f32(lg, T)
    kth = R.order(lg)[999]
    assert b[kth] == R.SAMP_NB - 1 and e[kth] <= -64, "the 1000th token is not in the last first-pass bin"
    assert (e <= -104).sum() > V // 2
    lg_d = torch.from_numpy(lg).to(gpu)
    ch = R.Checker(lg)
    counters = np.arange(5, 5 + n)
    for K in (0, 1000):
        for P in (1.0, 0.95):
            got = _draw(lg_d, T, K, P, seed, n, counter0=5)
            ok = ch.accepts(T, K, P, seed, counters, got)
            assert ok.all(), (f"{kind} T={T} K={K} P={P}: {int((~ok).sum())} draws rejected, first counter "
                              f"{5 + int(np.argmin(ok))} pick {got[np.argmin(ok)]}")


def test_all_but_three_tokens_weigh_nothing(gpu):
    V, T, seed, n = 32000, 1.0, 31337, 256
    rng = np.random.default_rng(12)
    lg = (rng.normal(0.0, 1.0, V) - 120.0).astype(np.float32)
    heavy = np.array([17, 255 * 16 + 15, V - 1])
    lg[heavy] = (5.0, 4.5, 4.0)
    e, _ = R.bins_f32(lg, T)
    assert (e < -104).sum() == V - 3
    lg_d = torch.from_numpy(lg).to(gpu)
    ch = R.Checker(lg)
    counters = np.arange(n)
    for K, P in ((0, 1.0), (0, 0.9), (2, 1.0), (3, 0.5), (50, 0.999)):
        got = _draw(lg_d, T, K, P, seed, n)
        assert np.isin(got, heavy).all(), (K, P, "a token of weight zero was drawn")
        assert ch.accepts(T, K, P, seed, counters, got).all(), (K, P)
        if (K, P) == (0, 1.0):
            assert set(got.tolist()) == set(heavy.tolist())


# ---- top-N of the log-prob operator -----------------------------------------------------------------------------------
def _check_floats(got, want, V, lse, what, is_lse=False):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    assert not np.isnan(got).any(), what
    ninf = np.isneginf(want)
    assert (np.isneginf(got) == ninf).all(), what
    for g, w in zip(got[~ninf], want[~ninf]):
        assert abs(g - w) <= L.tol(V, lse, 0.0 if is_lse else w), (what, g, w)


LP_ROWS = [(4111, 257, "b", False), (4111, 4097, "b", True), (4097, 257, "c", True), (32000, 256, "c", False),
           (V19, 257, "d", False), (V19, 4097, "d", True), (4097, 3, "f", True)]  # the last: fewer than N finite logits


@pytest.mark.parametrize("V,nA,place,low_inf", LP_ROWS)
def test_top_n_cuts_inside_the_tie_run(gpu, V, nA, place, low_inf):
    A = _place(V, nA, place)
    lg = _row(V, A, 1.0, low_inf, False)
    rest = np.setdiff1d(np.arange(V), A)
    order = np.concatenate([A, rest])  # logit descending, index ascending
    lse, lp, _, _ = L.logprobs(lg, 0)
    lg_d = torch.from_numpy(lg).to(gpu)
    ids_d = torch.tensor([int(A[-1])], dtype=torch.int32, device=gpu)
    for N in (1, 5, 20):
        outs = []
        for _ in range(2):
            out = ops.logprobs(lg_d, ids_d, N)
            torch.cuda.synchronize()
            outs.append({k: v.cpu().numpy() for k, v in out.items()})
        what = (V, nA, place, low_inf, N)
        for k in outs[0]:
            assert outs[0][k].tobytes() == outs[1][k].tobytes(), (what, k)
        got = outs[0]
        assert got["top_ids"][0].tolist() == order[:N].tolist(), (what, got["top_ids"][0], order[:N])
        _check_floats(got["lse"], lse, V, lse, what, is_lse=True)
        _check_floats(got["logprob"], lp[A[-1]], V, lse, what)
        _check_floats(got["top_logprobs"][0], lp[order[:N]], V, lse, what)


# ---- the decode step's sampled tails ----------------------------------------------------------------------------------
TIED = (0, 255, 256, 257, 2047)
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2, last_n=16)
BIAS = {5: -INF, 11: 1.0}
MODEL_SAMP = (0.5, 3, 0.9, 0xC0FFEE)
MODEL_CONFIGS = {"sampled": (None, None, None, "k_sample_topp"),
                 "sampled+penalties+bias": (PEN, BIAS, None, "k_sample_proc"),
                 "sampled+logprobs": (None, None, 5, "k_sample_lp")}
TAILS = {"k_sample_topp", "k_sample_proc", "k_sample_lp"}


def test_model_sampled_tails_on_logits_tied_across_the_seam(gpu):
    """A 2-layer synthetic model whose classifier rows 0, 255, 256, 257 and 2047 are one row: real logits with five
    bit-equal entries on both sides of the index seam.  The classifier is tied to the embedding, so feeding one of the
    five lifts all of them to the top of the next logits and top-k 3 cuts inside the run.  24 steps of the graph loop
    per tail; every sampled token is ops.sample_host's on the logits predict() leaves for that position."""
    from kuiperllama_amd.model import KuiperModel
    spec = FLAT_SPEC
    assert spec.vocab_size == 2048 and spec.shared_classifier
    img_d = binfmt.synth_image(spec, seed=3, device=gpu)
    ents, _ = binfmt.layout(spec)
    emb = binfmt.tensor_from_image(img_d, next(e for e in ents if e.name == "tok_emb"))
    emb[list(TIED)] = emb[256].clone()
    torch.cuda.synchronize()
    m = KuiperModel.from_device_image(img_d, spec, max_seq_len=128)
    T, K, P, seed = MODEL_SAMP
    prompt, steps = [1, 263, 256], 24
    n0 = len(prompt) - 1
    ws = ops.logit_process_workspace(spec.vocab_size, gpu)
    bias_ids = torch.tensor(sorted(BIAS), dtype=torch.int32, device=gpu)
    bias_val = torch.tensor([BIAS[k] for k in sorted(BIAS)], dtype=torch.float32, device=gpu)
    cut_in_run = 0
    try:
        for name, (pen, bias, top_n, tail) in MODEL_CONFIGS.items():
            m.set_penalties(**pen) if pen else m.set_penalties()
            m.set_logit_bias(bias)
            m.set_logprobs(top_n)
            m.set_sampling(T, K, P, seed)
            _ffi.debug_set("KH_LAUNCH_LOG", "1")  # a new, empty log
            words, _ = m.generate(prompt, steps, exec="graph")
            log = _ffi.launch_log()
            assert len(words) == steps and words[:n0] == prompt[1:]
            assert log & TAILS == {tail}, (name, sorted(log & TAILS))
            # replay: processors and records off, the same fed tokens one position at a time
            m.set_penalties()
            m.set_logit_bias(None)
            m.set_logprobs(None)
            fed = prompt + [int(w) for w in words[n0:]]
            fed_d = torch.tensor(fed, dtype=torch.int32, device=gpu)
            for p in range(steps):
                m.predict(fed[p], p, is_prompt=p < n0, exec="fused")
                if p < n0:
                    continue
                lg = m.logits()
                assert len(set(lg[list(TIED)].view(np.uint32).tolist())) == 1, (name, p, lg[list(TIED)])
                lg_d = torch.from_numpy(lg).to(gpu)
                if pen or bias:
                    ops.logit_process(lg_d, fed_d, p, pen, bias_ids, bias_val, ws)
                want = ops.sample_host(lg_d, _ffi.sampling(T, K, P, seed), p)
                assert words[p] == want, (name, p, words[p], want)
                if not (pen or bias):
                    cut_in_run += int((lg > lg[256]).sum() < K < (lg >= lg[256]).sum())
    finally:
        _ffi.debug_set("KH_LAUNCH_LOG", None)
        m.close()
    print(f"model: top-k cut inside the five-way tie in {cut_in_run} of {2 * (steps - n0)} sampled steps")
    assert cut_in_run > 0


# ---- the gate (last: it reads what the tests above recorded) --------------------------------------------------------
def test_table_gate(gpu):
    """every cell of the table was populated by checked exact draws or is documented unreachable, and every named kind
    of input took part"""
    missing_v = [V for V in VS if V not in _RAN]
    assert not missing_v, f"vocabulary sizes that did not run to the end (run the whole module): {missing_v}"
    lines, missing = [], []
    for cell in itertools.product(SOURCES, MODES, (True, False), LEVELS):
        n, why = _CELLS.get(cell, 0), UNREACHABLE.get(cell)
        src, mode, cut, lv = cell
        lines.append(f"  {src:6s} {mode:10s} {'index cut' if cut else 'no cut   '} {lv} level{'s' if lv > 1 else ' '}  "
                     f"{'UNREACHABLE: ' + why if why else str(n) + ' exact draws'}")
        if why:
            assert n == 0, f"{cell}: documented unreachable ({why}) but reached by {n} draws"
        elif n == 0:
            missing.append(cell)
    print("sampler table:\n" + "\n".join(lines))
    assert not missing, f"table cells no configuration reached: {missing}"
    assert len(UNREACHABLE) == 14 and sum(1 for c in _CELLS if _CELLS[c]) == 48 - 14
    want = ([("|A|", a) for a in SIZES + ["V"]] + [("place", p) for p in PLACES] + [("K", k) for k in K_KINDS] +
            [("P", p) for p in P_KINDS] + [("T", t) for t in TS] + [("low", b) for b in (False, True)] +
            [("third", True), ("m_key < ties", True), ("m_key < ties", False), ("top-k m_key vs ties", "=="),
             ("top-k m_key vs ties", "<"), ("top-k beyond the weighted tokens", True)] +
            [("descent", d) for d in ("top-k key", "top-p key", "index cut", "pick")])
    assert not [w for w in want if not _COVER[w]], [w for w in want if not _COVER[w]]
    print(f"exact rows: {_STATS['configs']} configurations, {_STATS['draws']} draws checked with ==, "
          f"{_STATS['launches']} launches; {sum(1 for c in _CELLS if _CELLS[c])} cells populated, "
          f"{len(UNREACHABLE)} unreachable")
    print(f"module wall time {time.perf_counter() - _T0:.1f} s")
