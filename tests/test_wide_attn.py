"""The plan of the wide pass's one-launch attention (csrc/kh_wide_attn_plan.h through kh_plan_wide_attn, host only): one
share item per distinct (pfx_row0, pfx_len), one own item per lane; every (lane, position) in exactly one (item, chunk)."""
import numpy as np
import pytest

from kuiperllama_amd import _ffi

SEQ = 8192


def _table(rows):
    """rows of (pos, base, pfx_len, pfx_row0) -> int32 [4][n]"""
    return np.array(rows, np.int32).T.copy()


def _unrelated(positions, row=0):
    out = []
    for p in positions:
        out.append((p, row, 0, 0))
        row += p + 1
    return out


TABLES = {
    "no sharing": _unrelated([0, 15, 16, 17, 255, 256, 257, 511, 512, 1500]),
    # parent rows from 100, P = 300: sharers at P, P + 1 and far behind, the parent's own lane beside them
    "one share group": [(300, 1000 - 300, 300, 100), (301, 1010 - 300, 300, 100), (900, 1100 - 300, 300, 100),
                        (305, 100, 0, 0), (7, 2000, 0, 0)],
    "two parents": [(40, 3000 - 33, 33, 0), (50, 3100 - 33, 33, 0), (600, 4000 - 600, 600, 1000),
                    (601, 4100 - 600, 600, 1000), (3, 5000, 0, 0)],
    "two P under one parent": [(20, 3000 - 16, 16, 64), (40, 3100 - 17, 17, 64), (41, 3200 - 17, 17, 64)],
    # the sharer's own rows start at row 0: base = 0 - P
    "negative base": [(45, -40, 40, 500), (44, 100 - 40, 40, 500), (60, 500, 0, 0)],
    "64 lanes": _unrelated([(37 * i) % 120 for i in range(64)]),
    # all 64 lanes share, 64 distinct prefixes: 128 items, the chunk cap on a long range
    "128 items": [(130 + i, 70 * i, 100 + i, 4480 + i) for i in range(63)] + [(8100, 0, 90, 7000)],
}


@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("kv_mul,head_size", [(4, 64), (7, 64), (1, 128)])
def test_every_position_of_every_lane_is_in_exactly_one_chunk(name, kv_mul, head_size):
    lanes = _table(TABLES[name])
    n = lanes.shape[1]
    items = _ffi.plan_wide_attn(lanes, kv_mul, head_size, SEQ)
    shares = [it for it in items if it["kind"] == "share"]
    assert len(items) == len(shares) + n <= 128
    assert [it["kind"] for it in items] == ["share"] * len(shares) + ["own"] * n
    hits = [np.zeros(int(lanes[0, i]) + 1, int) for i in range(n)]
    qt = 2 if head_size == 128 else 4
    for it in items:
        tiles = (it["len"] + 15) // 16
        ct, ns = it["chunk_tiles"], it["chunks"]
        assert 1 <= ns <= 8 and (ns - 1) * ct < tiles <= ns * ct, it  # whole tiles, and none of the chunks is empty
        assert ns == 1 or ct >= 16, it
        col_tiles = -(-len(it["lanes"]) * kv_mul // 16)  # 16 query columns (lane, head of the kv group) per tile
        assert it["units"] == ns * -(-col_tiles // qt), it
        for ln in it["lanes"]:
            pos, base, pfx, prow = (int(x) for x in lanes[:, ln])
            # the positions of lane ln that live in the item's rows
            p0, first = (0, prow) if it["kind"] == "share" else (pfx, base + pfx)
            assert first == it["row0"], (it, ln)
            assert it["len"] == (pfx if it["kind"] == "share" else pos - pfx + 1), (it, ln)
            for c in range(ns):
                lo, hi = 16 * ct * c, min(16 * ct * (c + 1), it["len"])
                hits[ln][p0 + lo:p0 + hi] += 1
    for i in range(n):
        assert (hits[i] == 1).all(), (name, i, np.flatnonzero(hits[i] != 1)[:8])
    # a share item carries exactly the lanes with its (pfx_row0, pfx_len); the own item of lane i is item n_share + i
    for it in shares:
        want = [i for i in range(n) if lanes[2, i] > 0 and (lanes[3, i], lanes[2, i]) == (it["row0"], it["len"])]
        assert it["lanes"] == want, it
    assert len({(it["row0"], it["len"]) for it in shares}) == len(shares)
    assert [it["lanes"] for it in items[len(shares):]] == [[i] for i in range(n)]


def test_a_long_range_is_cut_and_a_short_one_is_not():
    for length, chunks in ((1, 1), (496, 1), (497, 2), (1024, 4), (4096, 8), (8192, 8)):
        (it,) = _ffi.plan_wide_attn(_table([(length - 1, 0, 0, 0)]), 4, 64, SEQ)
        assert it["chunks"] == chunks, (length, it)
