"""The cutoff set of grade-tonnage curves, geobodies and drill intercepts (DESIGN.md sections 17 to 19) has one definition per layer.
Without a GPU: resources.cutoff_query against hand-computed values and its errors, and the one verdict of csrc/cutoff_set.h behind
the three C entry points."""
import ctypes as C

import numpy as np
import pytest

from geobo_amd import resources as R

GRID = (8, 10, 6)                                                  # (yN, xN, zN) of the 10 x 8 x 6 survey
SCALE = (2.0, 4.0, 0.5)
INF, NAN = float("inf"), float("nan")


def query(prop="drill", cutoffs=(1.0,), offset=0.0, require=None, has_drill=True, block=None, region=None, n=4, start=0):
    return R.cutoff_query(prop, cutoffs, offset, require, SCALE, has_drill, GRID, block, region, n, start)


# ---- 1. the host query -----------------------------------------------------------------------------------------------------------
def test_cutoff_query_by_hand():
    q = query(cutoffs=[1.5, 0.5, 1.0, 0.5], offset=0.5, require={"density": 3.0}, n=7, start=2)
    assert q.p == 2 and q.n == 7 and q.start == 2
    assert np.array_equal(q.cut, [1.5, 0.5, 1.0, 0.5])
    assert np.array_equal(q.t, [0.0, 0.0, 1.0, 2.0])                # (c - 0.5) / 0.5, ascending
    assert np.array_equal(q.order, [1, 3, 2, 0])                    # stable: the two equal cutoffs keep their order
    assert np.array_equal(q.inverse, [3, 0, 2, 1])
    assert np.array_equal(q.t[q.inverse], (q.cut - 0.5) / 0.5)
    assert np.array_equal(q.lo, [1.5, -INF, -INF])                  # 3.0 / 2.0, cube units without the offset
    assert q.scale == [2.0, 4.0, 0.5] and all(type(v) is float for v in q.scale)
    assert q.box is None and tuple(q.shape) == GRID and q.mask is None
    assert np.array_equal(R.caller_order(np.arange(8).reshape(2, 4), q.order), np.arange(8).reshape(2, 4)[:, q.inverse])


def test_cutoff_query_block_and_region():
    q = query(block=(4, 3, 4))                                      # (bx, by, bz) as block_statistics takes it
    assert q.box == (3, 4, 4) and tuple(q.shape) == (3, 3, 2)
    region = np.zeros((3, 3, 2), dtype=bool)
    region[1, 2, 0] = True
    m = query(block=(4, 3, 4), region=region).mask
    assert m.dtype == np.uint8 and m.shape == (18,) and m.flags.c_contiguous and np.flatnonzero(m).tolist() == [10]
    full = np.ones(GRID, dtype=bool)
    assert query(region=full).mask.sum() == 480
    for bad in (np.ones((6, 10, 8), dtype=bool), full.astype(np.uint8), full[:, :, :5]):
        with pytest.raises(ValueError, match="region"):
            query(region=bad)
    with pytest.raises(ValueError, match="region"):                 # at block support the region has the block shape
        query(block=(4, 3, 4), region=full)


def test_cutoff_query_errors():
    with pytest.raises(ValueError, match="require"):
        query(prop="drill", require={"drill": 0.0})
    with pytest.raises(ValueError, match="require"):
        query(prop=2, require={2: 0.0})
    with pytest.raises(ValueError, match="require"):
        query(require={"magsus": NAN})
    with pytest.raises(ValueError, match="NaN"):
        query(cutoffs=[0.0, NAN])
    for c in ([], list(range(33))):
        with pytest.raises(ValueError, match="between 1 and 32 cutoffs"):
            query(cutoffs=c)
    assert query(cutoffs=list(range(32))).t.size == 32
    with pytest.raises(ValueError, match="n >= 1"):
        query(n=0)
    with pytest.raises(ValueError, match="start >= 0"):
        query(start=-1)
    with pytest.raises(ValueError, match="drill"):
        query(prop="drill", has_drill=False)
    with pytest.raises(ValueError, match="drill"):
        query(prop="density", require={"drill": 0.0}, has_drill=False)
    assert query(prop="density", require={"magsus": 0.0}, has_drill=False).p == 0
    with pytest.raises(ValueError, match="property"):
        query(prop="gold")


# ---- 2. one verdict, three entries -------------------------------------------------------------------------------------------------
def _dbl(v):
    return None if v is None else (C.c_double * len(v))(*v)


N = 60                                                              # the grid (3, 4, 5): 12 columns of 5
OK3 = (-INF, -INF, -INF)
ASC32 = tuple(float(i) for i in range(32))
# (p, C, t, lo, pstride, sstride, S, expected); C None = len(t)
ROWS = [
    (0, None, (0.0,), OK3, N, 3 * N, 0, 0),
    (2, None, (-INF, 0.0, 0.0, 1.5), (0.5, -INF, -INF), N + 4, 3 * N + 100, 0, 0),
    (1, None, ASC32, (-INF, -INF, INF), N, 3 * N, 0, 0),
    (-1, None, (0.0,), OK3, N, 3 * N, 0, -1),
    (3, None, (0.0,), OK3, N, 3 * N, 0, -1),
    (0, 0, (0.0,), OK3, N, 3 * N, 0, -1),
    (0, None, ASC32 + (32.0,), OK3, N, 3 * N, 0, -1),
    (0, None, (0.0, NAN, 1.0), OK3, N, 3 * N, 0, -1),
    (0, None, (0.0, 1.0, 0.5), OK3, N, 3 * N, 0, -1),
    (0, None, (0.0,), (-INF, NAN, -INF), N, 3 * N, 0, -1),
    (0, None, (0.0,), OK3, N - 1, 3 * N, 0, -1),
    (0, None, (0.0,), OK3, (1 << 61) + 1, (1 << 63) - 1, 0, -1),
    (0, None, (0.0,), OK3, N, 3 * N - 1, 0, -1),
    (0, None, (0.0,), OK3, N, 1 << 62, 3, -1),                      # S sstride beyond an int64
    (0, 1, None, OK3, N, 3 * N, 0, -1),
    (0, None, (0.0,), None, N, 3 * N, 0, -1),
]


def _three(L, S, F, ss, ps, prop, Cn, t, lo):
    """The codes of the three entries for one cutoff set on the grid (3, 4, 5), every other argument valid."""
    p = 16                                                          # (never dereferenced: S = 0, or the call fails its checks first)
    big = 1 << 40                                                   # workspace bytes: enough for every row
    return (L.geobo_cutoff_stats(S, F, ss, ps, N, prop, Cn, _dbl(t), _dbl(lo), None, None, p, p, None, p, big, None),
            L.geobo_bodies(S, F, ss, ps, 3, 4, 5, prop, Cn, _dbl(t), _dbl(lo), None, None, 6, 1, 0, None, p, p, None, None, None, p, 15, p, big,
                           None),
            L.geobo_trace_stats(S, F, ss, ps, 3, 4, 5, prop, Cn, _dbl(t), _dbl(lo), None, 12, None, None, 5, 1, 0, p, None, None, None, None, None,
                                None, None, None, None, p, big, None))


def test_one_verdict_three_entries():
    from geobo_amd import _lib
    L = _lib.load()
    for row in ROWS:
        prop, Cn, t, lo, ps, ss, S, want = row
        codes = _three(L, S, 16, ss, ps, prop, len(t) if Cn is None else Cn, t, lo)
        assert codes == (want, want, want), (row, codes)
    assert _three(L, 0, None, 3 * N, N, 0, 1, (0.0,), OK3) == (-1, -1, -1)          # a null F
