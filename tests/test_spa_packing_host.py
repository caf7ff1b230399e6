"""CPU tests of the fp64 sum-product decoder's bin tables (mercury_amd/csrc/tables.cpp: pack_spa_bins and what load_graph derives from it),
read back through mgpu_debug_spa_bins for every rate of the built-in table blob: the number of bins is the minimum whole checks allow, every
check sits whole in one bin, the bin heads and walk masks say what the slot table says, the product walks are no longer than first-fit
decreasing's, long bins come first, and the placement is deterministic."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

from fp32_decoders_ref import blob_codes
from mercury_amd import load_library

N = 1600
# K -> bins: ceil(E / 64) wherever whole checks allow it; at rate 14/16 the 108 checks of more than 32 edges take a bin each and the 15 of
# exactly 32 edges eight more
BINS = {100: 56, 200: 61, 300: 70, 400: 73, 500: 85, 600: 88, 800: 95, 1400: 116}


@functools.lru_cache(maxsize=None)
def _blob():
    """K -> (check degrees, the checks' variable rows)"""
    out = {}
    for k, c in blob_codes().items():
        assert c["N"] == N
        cdeg = [int(d) for d in c["cdeg"]]
        rows, e = [], 0
        for d in cdeg:
            rows.append(tuple(int(v) for v in c["cflat"][e:e + d]))
            e += d
        out[k] = (cdeg, rows)
    return out


def _build(K):
    lib = load_library()
    dims = (C.c_int * 6)()
    assert lib.mgpu_debug_spa_bins(K, dims, None, None, None) == 0
    S, DM, rounds = dims[0], dims[1], dims[2]
    sadr = np.zeros((rounds + 1) * 1024 * 2, np.uint32)
    bhead = np.zeros((rounds + 1) * 64, np.uint64)
    bmask = np.zeros(rounds * 16 * DM, np.uint64)
    assert lib.mgpu_debug_spa_bins(K, dims, sadr.ctypes.data, bhead.ctypes.data, bmask.ctypes.data) == 0
    return {"S": S, "DM": DM, "rounds": rounds, "N": dims[3], "E": dims[4], "P": dims[5],
            "sadr": sadr.reshape(-1, 2), "bhead": bhead.reshape(-1, 4), "bmask": bmask.reshape(-1, DM)}


@functools.lru_cache(maxsize=None)
def _tables(K):
    return _build(K)


def _checks_of(t):
    """[(bin, first lane, degree, variables)] in slot order, from the slot table alone; asserts what every slot must satisfy on the way"""
    sadr = t["sadr"]
    ones = int(sadr[0, 1]) - 8 * N                         # slot 0 opens a check: its check's first message is the message array's first
    assert ones >= 48 * 8 and ones % 8 == 0
    out = []
    for b in range(t["S"] // 64):
        lane = 0
        while lane < 64 and sadr[b * 64 + lane, 1] != 0:
            cs = b * 64 + lane
            assert int(sadr[cs, 1]) == ones + 8 * N + 8 * cs      # a check starts where the previous one ended
            d = 1
            while lane + d < 64 and int(sadr[cs + d, 1]) == int(sadr[cs, 1]):
                d += 1
            row = []
            for p in range(cs, cs + d):
                a = int(sadr[p, 0]) - ones
                assert a >= 0 and a % 8 == 0 and a // 8 < N
                row.append(a // 8)
            out.append((b, lane, d, tuple(row)))
            lane += d
        assert not sadr[b * 64 + lane:(b + 1) * 64].any()         # padding: the rest of the bin, all zeros
    assert not sadr[t["S"]:].any()
    return out


def _ffd(cdeg):
    fill, mx = [], []
    for d in sorted(cdeg, reverse=True):
        for i in range(len(fill)):
            if fill[i] + d <= 64:
                fill[i] += d
                break
        else:
            fill.append(d)
            mx.append(d)
    return mx                                              # a bin's first check is its largest


@pytest.mark.parametrize("K", sorted(BINS))
def test_bins_are_the_minimum(K):
    cdeg, _ = _blob()[K]
    t = _tables(K)
    assert t["E"] == sum(cdeg) and t["P"] == len(cdeg) and t["N"] == N
    assert t["S"] == 64 * BINS[K]
    if K != 1400:
        assert BINS[K] == -(-sum(cdeg) // 64)
    assert t["rounds"] == max(4, -(-t["S"] // 1024))      # the kernel instance (NE) follows from this
    assert t["rounds"] == {100: 4, 200: 4, 300: 5, 400: 5, 500: 6, 600: 6, 800: 6, 1400: 8}[K]


@pytest.mark.parametrize("K", sorted(BINS))
def test_every_check_sits_whole_in_one_bin_in_row_order(K):
    cdeg, rows = _blob()[K]
    found = _checks_of(_tables(K))
    assert all(lane + d <= 64 for _b, lane, d, _row in found)
    # every check of the code exactly once, its variables in the blob's row order
    assert collections.Counter(row for _b, _lane, _d, row in found) == collections.Counter(r for r in rows if r)
    assert sum(d for _b, _lane, d, _row in found) == sum(cdeg)


@pytest.mark.parametrize("K", sorted(BINS))
def test_heads_and_walk_masks_follow_the_slot_table(K):
    t = _tables(K)
    bins = t["S"] // 64
    used = [0] * bins
    ends = [0] * bins
    maxdeg = [0] * bins
    masks = [[0] * t["DM"] for _ in range(bins)]
    for b, lane, d, _row in _checks_of(t):
        assert d <= t["DM"]
        for pos in range(d):
            used[b] |= 1 << (lane + pos)
            for j in range(d):
                if j != pos:
                    masks[b][j] |= 1 << (lane + pos)
        ends[b] |= 1 << (lane + d - 1)
        maxdeg[b] = max(maxdeg[b], d)
    bh, bm = t["bhead"], t["bmask"]
    for b in range(bins):
        assert [int(x) for x in bh[b]] == [used[b], ends[b], maxdeg[b], 0]
        assert [int(x) for x in bm[b]] == masks[b]
    assert not bh[bins:].any() and not bm[bins:].any()


@pytest.mark.parametrize("K", sorted(BINS))
def test_walks_are_no_longer_than_first_fit_decreasing_and_long_bins_come_first(K):
    cdeg, _ = _blob()[K]
    t = _tables(K)
    q = 4 if K == 1400 else 2                               # the walk runs in step quads at rate 14/16 (48 steps), in pairs elsewhere (16)
    mx = [int(x) for x in t["bhead"][:t["S"] // 64, 2]]
    assert sum(-(-m // q) for m in mx) <= sum(-(-m // q) for m in _ffd(cdeg))
    assert mx == sorted(mx, reverse=True)
    assert max(mx) == max(cdeg) and max(cdeg) <= (48 if K == 1400 else 16)


@pytest.mark.parametrize("K", [600, 1400])
def test_two_builds_are_identical(K):
    a, b = _tables(K), _build(K)
    for key in ("S", "DM", "rounds"):
        assert a[key] == b[key]
    for key in ("sadr", "bhead", "bmask"):
        assert np.array_equal(a[key], b[key])
