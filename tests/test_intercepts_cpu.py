"""Drill-intercept statistics without a GPU: the exported symbols and the argument checks of
geobo_trace_stats, the NumPy reference against hand-computed traces, and the host logic of geobo_amd/intercepts.py: trace
builders, the wrapper's validation of offsets and indices, metres to samples, quantiles from histograms, the unit conversion, the
CSV frames, the launch cuts and the YAML key."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _intercepts_ref as ref
from conftest import ROOT, settings_for


def _dbl(*v):
    return (C.c_double * len(v))(*v)


# ---- 1. C ABI without a GPU ------------------------------------------------------------------------------------------------------
def _header_args(name):
    src = open(os.path.join(ROOT, "include", "geobo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",") if a.strip()]


def test_symbols_and_signatures():
    from geobo_amd import _lib, build
    L = _lib.load()
    assert L.geobo_version() == 213
    assert "intercepts.hip" in build.SOURCES
    host = {"t", "lo"}                                         # host arrays travel as POINTER(c_double), device pointers as void*
    for name in ("geobo_trace_stats", "geobo_trace_stats_ws_bytes"):
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert getattr(L, name).argtypes == args and getattr(L, name).restype == res
        hres, hargs = _header_args(name)
        assert {"int": C.c_int, "size_t": C.c_size_t}[hres] == res
        assert len(hargs) == len(args), (name, len(hargs), len(args))
        for decl, ct in zip(hargs, args):
            pname = decl.split()[-1].lstrip("*")
            if "*" in decl:
                assert ct == (C.POINTER(C.c_double) if pname in host else C.c_void_p), decl
            else:
                assert ct == {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t}[decl.split()[-2]], decl
    assert len(_lib.SIGNATURES["geobo_trace_stats"][1]) == 31
    head = open(os.path.join(ROOT, "include", "geobo_hip.h")).read()
    assert "geobo_trace_stats_ws_bytes). */" in head and "validates them on the host" in head


def test_trace_stats_validates_without_gpu():
    from geobo_amd import _lib
    L = _lib.load()
    p = 16                                                     # (never dereferenced: every call below fails its checks first)
    grid = (3, 4, 5)
    n = 60
    wsb = L.geobo_trace_stats_ws_bytes
    inf = float("inf")

    def call(S=3, F=p, ss=3 * n, ps=n, grid=grid, prop=1, t=(-inf, 0.0, 0.0, 1.5), lo=(-inf, -inf, -inf), mask=None, K=12, offsets=None,
             voxels=None, Lmax=5, min_len=1, max_gap=0, tab=p, ws=p, nbytes=None, Cn=None):
        Cn = (4 if t is None else len(t)) if Cn is None else Cn
        nbytes = wsb(3, 12, 4) if nbytes is None else nbytes
        return L.geobo_trace_stats(S, F, ss, ps, *grid, prop, Cn, None if t is None else _dbl(*t), None if lo is None else _dbl(*lo), mask,
                                   K, offsets, voxels, Lmax, min_len, max_gap, tab, None, None, None, None, None, None, None, None, None,
                                   ws, nbytes, None)
    for name in ("F", "t", "lo", "tab", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(S=-1) == -1 and call(S=1 << 31) == -1
    assert call(K=0) == -1 and call(K=11) == -1 and call(K=13, nbytes=1 << 20) == -1      # columns: K = ny nx
    assert call(Lmax=4) == -1 and call(Lmax=6) == -1                                       # columns: Lmax = nz
    for axis in range(3):
        assert call(grid=tuple(0 if i == axis else v for i, v in enumerate(grid))) == -1
    assert call(grid=(2048, 2048, 2048), K=2048 * 2048, Lmax=2048, ps=1 << 40, ss=1 << 42, nbytes=1 << 40) == -1      # n > INT32_MAX
    assert call(grid=(1, 1, 4097), K=1, Lmax=4097, ps=4097, ss=3 * 4097) == -1            # a column of more than 4096
    assert call(Cn=0) == -1
    assert call(t=tuple(float(i) for i in range(33)), nbytes=1 << 30) == -1               # C = 33
    assert call(t=(0.0, 1.0, 0.5, 2.0)) == -1                                             # unsorted
    assert call(t=(0.0, float("nan"), 1.0, 2.0)) == -1 and call(t=(float("nan"), 0.0, 1.0, 2.0)) == -1
    assert call(lo=(-inf, float("nan"), -inf)) == -1
    assert call(prop=-1) == -1 and call(prop=3) == -1
    assert call(ps=n - 1) == -1 and call(ss=3 * n - 1) == -1
    assert call(min_len=0) == -1 and call(max_gap=-1) == -1 and call(max_gap=4097) == -1
    assert call(voxels=p, offsets=None, K=2) == -1                                        # voxels without offsets
    assert call(voxels=p, offsets=p, K=2, Lmax=0) == -1 and call(voxels=p, offsets=p, K=2, Lmax=4097) == -1
    assert call(nbytes=wsb(3, 12, 4) - 16) == -1 and call(nbytes=0) == -1
    assert call(ws=24) == -1                                                              # not 16-byte aligned
    # S == 0 is a no-op that touches nothing
    assert call(S=0) == 0 and call(S=0, voxels=p, offsets=p, K=7, Lmax=4096, max_gap=4096) == 0
    # the workspace size: 0 for invalid arguments, a multiple of 16 otherwise
    assert wsb(-1, 12, 4) == 0 and wsb(3, 0, 4) == 0 and wsb(3, 12, 0) == 0 and wsb(3, 12, 33) == 0
    for S in (0, 1, 3, 64, 100000):
        for K in (1, 7, 80, 4096, 128 * 128):
            for Cn in (1, 5, 16, 32):
                b = wsb(S, K, Cn)
                assert b >= max(16, 4 * S * K * Cn) and b % 16 == 0, (S, K, Cn, b)


# ---- 2. the reference against hand-computed traces -------------------------------------------------------------------------------
def _hand(text, max_gap, min_len=1):
    """'1' ore (value 1), '.' non-ore eligible, 'x' ineligible."""
    chars = text.split()
    ore = [ch == "1" for ch in chars]
    elig = [ch != "x" for ch in chars]
    return ref.trace_flags([1.0 if o else 0.25 for o in ore], ore, elig, min_len=min_len, max_gap=max_gap)


def test_reference_hand_cases():
    r = _hand("1 1 . 1 . . 1 x", 1)
    assert (r["start"], r["len"], r["n_int"], r["thick"], r["top"]) == (0, 4, 2, 4, 0)
    assert r["composite"] == [True, True, True, True, False, False, True, False]
    assert r["acc"] == 4.0 and r["run_sum"] == 3.25            # the filled waste counts with its own value
    r = _hand("1 1 . 1 . . 1 x", 2)
    assert (r["start"], r["len"], r["n_int"]) == (0, 7, 1) and r["run_sum"] == 4.75
    r = _hand("1 x 1", 5)
    assert (r["start"], r["len"], r["n_int"]) == (0, 1, 2) and r["composite"] == [True, False, True]
    r = _hand("1 1 . 1 1", 0)
    assert (r["start"], r["len"], r["n_int"]) == (0, 2, 2)     # a tie goes to the shallower
    assert _hand("1 1 . 1 1", 0, min_len=3)["n_int"] == 0
    r = _hand(". . x", 3)
    assert (r["thick"], r["top"], r["start"], r["len"], r["n_int"], r["acc"], r["run_sum"]) == (0, 3, 3, 0, 0, 0.0, 0.0)
    r = _hand(". 1 . .", 4)
    assert (r["start"], r["len"]) == (1, 1)                    # no ore after the gap, none before the first: nothing filled
    # trace_stats on a 1 x 2 x 4 grid, the second column read bottom up through CSR
    F = np.zeros((1, 3, 8))
    F[0, 0] = [1, 0, 1, 1, 0, 1, 1, 1]
    got = ref.trace_stats(F, 0, [0.5], [[0, 1, 2, 3], [7, 6, 5, 4]], max_gap=1, min_len=2)
    assert got["detail"][0, 0].tolist() == [[3, 0, 0, 4, 1, 0], [3, 0, 0, 3, 1, 0]]
    assert got["tab"][0, 0].tolist() == [2, 6, 4]
    m = ref.maps_of(got, 4, min_len=2)
    assert m["hist_len"][0].tolist() == [[0, 0, 0, 0, 1], [0, 0, 0, 1, 0]] and m["hits"].tolist() == [[1, 1]]


# ---- 3. host logic ---------------------------------------------------------------------------------------------------------------
def test_trace_builders():
    from geobo_amd import intercepts as ic
    from geobo_amd.acquisition import Acquisition
    grid = (3, 4, 5)
    off, vox = ic.column_traces(grid)
    assert off.tolist() == list(range(0, 61, 5)) and np.array_equal(vox, np.arange(60))
    assert [list(vox[off[k]:off[k + 1]]) for k in range(12)] == ref.column_traces(*grid)
    off, vox = ic.hole_traces([(3, 2), (0, 0), (3, 2)], grid)
    assert off.tolist() == [0, 5, 10, 15]
    assert vox[:5].tolist() == list(range((2 * 4 + 3) * 5, (2 * 4 + 3) * 5 + 5)) and vox[5:10].tolist() == [0, 1, 2, 3, 4]
    for bad in ([], [(4, 0)], [(0, 3)], [(-1, 0)], [(0.5, 1.0)], [(1, 2, 3)]):
        with pytest.raises(ValueError):
            ic.hole_traces(bad, grid)
    # a dipping path: the triplets of Acquisition.path_voxels at its own ranges, one entry per step, duplicates kept
    s = settings_for(10, 8, 6)
    acq = Acquisition(s, np.zeros((8, 10, 6)), np.ones((8, 10, 6)))
    x0, y0, az, dip = 310.0, 420.0, 35.0, 60.0
    want = acq.path_voxels(x0, y0, az, dip)
    got = ic.path_triplets(s, x0, y0, az, dip, acq._ranges)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    flat = ic.triplet_trace(want, (8, 10, 6))
    assert flat.size == acq._ranges.size and np.array_equal(flat, np.ravel_multi_index(want, (8, 10, 6)))
    assert (np.diff(flat) == 0).any()                          # half-voxel steps: some voxels are visited twice in a row
    with pytest.raises(ValueError, match="leaves"):
        ic.triplet_trace(acq.path_voxels(950.0, 420.0, 0.0, 30.0), (8, 10, 6))
    # at the ranges and with the length convention of predict_path
    off, vox, step = ic.path_traces(s, [(x0, y0, az, dip), (500.0, 400.0, 0.0, 0.0)], step=50.0)
    assert step == 50.0 and off[0] == 0 and off[-1] == vox.size
    rng, _ = ic.path_ranges(s, x0, y0, az, dip, step=50.0)
    assert rng[0] == 25.0 and np.allclose(np.diff(rng), 50.0) and off[1] == rng.size
    assert np.array_equal(vox[:off[1]], ic.triplet_trace(ic.path_triplets(s, x0, y0, az, dip, rng), (8, 10, 6)))
    assert off[2] - off[1] == 12                               # the vertical one: 600 m at 50 m
    assert np.array_equal(vox[off[1]:], np.ravel_multi_index((np.full(12, 5), np.full(12, 4), np.arange(12) // 2), (8, 10, 6)))
    short = ic.path_traces(s, [(700.0, 400.0, 0.0, 45.0)], step=50.0)                      # leaves the first axis at 800 m: cut there
    assert short[0][1] == 3
    for bad in ([], [(1.0, 2.0, 3.0)], [(-50.0, 400.0, 180.0, 45.0)]):
        with pytest.raises(ValueError):
            ic.path_traces(s, bad, step=50.0)
    with pytest.raises(ValueError, match="steps"):
        ic.path_traces(s, [(500.0, 400.0, 0.0, 0.0)], step=0.1)                           # 6000 steps


def test_wrapper_validates_offsets_and_indices():
    from geobo_amd import hip
    off, vox, K, Lmax = hip.check_traces([0, 1, 65, 130, 330], np.arange(330) % 100, 100)
    assert off.dtype == np.int32 and vox.dtype == np.int32 and (K, Lmax) == (4, 200)
    assert hip.check_traces([0, 4096], np.zeros(4096, dtype=np.int64), 1)[3] == 4096
    for o, v, n in (([0, 2, 2], [0, 1], 5),                    # an empty trace
                    ([0, 3, 2, 4], [0, 1, 2, 3], 5),           # not monotone
                    ([1, 4], [0, 1, 2, 3], 5),                 # does not start at 0
                    ([0, 3], [0, 1, 2, 3], 5),                 # does not end at the voxel count
                    ([0, 4], [0, 1, 5, 3], 5),                 # an index past the cube
                    ([0, 4], [0, -1, 2, 3], 5),                # a negative index
                    ([0, 4097], np.zeros(4097, dtype=np.int64), 5),
                    ([0], [], 5), ([[0, 1]], [0], 5), ([0.0, 1.0], [0], 5), ([0, 1], [0.5], 5)):
        with pytest.raises(ValueError):
            hip.check_traces(o, v, n)


def test_metres_to_samples():
    from geobo_amd import intercepts as ic
    assert ic.samples_of(None, 0.0, 100.0) == (1, 0)
    assert ic.samples_of(300.0, 100.0, 100.0) == (3, 1)
    assert ic.samples_of(250.0, 250.0, 100.0) == (3, 2)        # ceil for the length asked for, floor for the gap allowed
    assert ic.samples_of(1.0, 99.999, 100.0) == (1, 0)
    assert ic.samples_of(0.3, 0.3, 0.1) == (3, 3)              # 0.3 / 0.1 = 2.9999999999999996 counts as 3
    assert ic.samples_of(25.0, 4096 * 12.5, 12.5) == (2, 4096)
    for ml, mg, dz in ((0.0, 0.0, 100.0), (-1.0, 0.0, 100.0), (float("nan"), 0.0, 100.0), (1.0, -1.0, 100.0), (1.0, float("inf"), 100.0),
                       (1.0, 0.0, 0.0), (1.0, 4097 * 100.0, 100.0)):
        with pytest.raises(ValueError):
            ic.samples_of(ml, mg, dz)


def test_histogram_quantiles_against_numpy():
    from geobo_amd import intercepts as ic
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 10, 16, 255, 256):
        v = rng.integers(0, 17, size=(3, 5, n))
        v[0, 0] = 0
        v[0, 1] = 16
        h = np.zeros((3, 5, 17), dtype=np.int32)
        for i in range(3):
            for j in range(5):
                np.add.at(h[i, j], v[i, j], 1)
        q = (0.0, 0.1, 0.25, 0.5, 0.9, 1.0)
        got = ic.hist_quantiles(h, q)
        assert got.dtype == np.int64 and np.array_equal(got, np.quantile(v, q, axis=-1, method="inverted_cdf")), n
        assert np.allclose(ic.hist_mean(h), v.mean(-1), rtol=1e-15)
    empty = np.zeros((2, 4), dtype=np.int32)
    assert (ic.hist_quantiles(empty) == -1).all() and np.isnan(ic.hist_mean(empty)).all()
    s = ic.length_summary(np.array([[0, 3, 0, 1]]), 25.0)
    assert s["p10"].tolist() == [25.0] and s["p50"].tolist() == [25.0] and s["p90"].tolist() == [75.0] and s["mean"].tolist() == [37.5]


def test_unit_conversion():
    from geobo_amd import intercepts as ic
    n, Cn, K, B = 4, 2, 3, 6
    rng = np.random.default_rng(9)
    thick = rng.integers(0, B, size=(n, Cn, K))
    thick[:, 0, 2] = 0                                         # a hole that never meets ore
    length = np.minimum(thick, rng.integers(0, B, size=(n, Cn, K)))
    top = np.where(thick > 0, rng.integers(0, 3, size=(n, Cn, K)), B - 1)
    start = np.where(length > 0, top, B - 1)
    detail = np.stack([thick, top, start, length, (length > 1).astype(int), np.zeros_like(thick)], -1).astype(np.int32)
    dsum = rng.standard_normal((n, Cn, K, 2))
    scale, offset, dz = float(np.float32(2.5)), 10.0, 25.0
    r = ic.per_realisation(detail, dsum, scale, offset, dz)
    assert np.array_equal(r["thickness"], thick * dz) and np.array_equal(r["length"], length * dz)
    assert np.array_equal(np.isnan(r["depth_to_top"]), thick == 0) and np.array_equal(np.isnan(r["from"]), length == 0)
    assert np.array_equal(r["depth_to_top"][thick > 0], top[thick > 0] * dz)
    assert np.allclose(r["accumulation"], (scale * dsum[..., 0] + offset * thick) * dz, rtol=1e-15, atol=0)
    ok = length > 0
    assert np.allclose(r["grade"][ok], scale * dsum[..., 1][ok] / length[ok] + offset, rtol=1e-13) and np.isnan(r["grade"][~ok]).all()
    assert np.array_equal(r["n_intercepts"], length > 1)
    # maps
    maps = dict(hits_any=(thick > 0).sum(0), hits=(length >= 2).sum(0), thick_sum=thick.sum(0), top_sum=np.where(thick > 0, top, 0).sum(0),
                acc_sum=dsum[..., 0].sum(0))
    for name, col in (("hist_len", length), ("hist_thick", thick)):
        h = np.zeros((Cn, K, B), dtype=np.int32)
        for s in range(n):
            for c in range(Cn):
                np.add.at(h[c], (np.arange(K), col[s, c]), 1)
        maps[name] = h
    m = ic.intercept_maps(maps, n, scale, offset, dz)
    assert np.array_equal(m["probability"], (length >= 2).mean(0)) and np.array_equal(m["probability_any"], (thick > 0).mean(0))
    assert np.allclose(m["thickness"]["mean"], thick.mean(0) * dz, rtol=1e-15)
    assert np.array_equal(m["thickness"]["p50"], np.quantile(thick, 0.5, axis=0, method="inverted_cdf") * dz)
    assert np.array_equal(m["intercept_length"]["p90"], np.quantile(length, 0.9, axis=0, method="inverted_cdf") * dz)
    assert np.allclose(m["intercept_length"]["mean"], length.mean(0) * dz, rtol=1e-15)
    assert np.isnan(m["depth_to_top_mean"][0, 2])
    with np.errstate(all="ignore"):
        want = np.where(thick > 0, top, 0).sum(0) * dz / (thick > 0).sum(0)
    assert np.array_equal(np.isnan(m["depth_to_top_mean"]), (thick > 0).sum(0) == 0)
    assert np.allclose(m["depth_to_top_mean"], want, rtol=1e-15, equal_nan=True)
    assert np.allclose(m["accumulation_mean"], (scale * dsum[..., 0].sum(0) + offset * thick.sum(0)) * dz / n, rtol=1e-15, atol=0)
    # tables
    tab = np.stack([(length >= 2).sum(-1), thick.sum(-1), length.max(-1)], -1)
    t = ic.intercept_tables(tab, dz, column_area=100.0 * 50.0)
    assert np.array_equal(t["holes_hit"], tab[..., 0]) and np.array_equal(t["prospective_area"], tab[..., 0] * 5000.0)
    assert np.array_equal(t["longest"], tab[..., 2] * dz) and np.array_equal(t["count"], tab[..., 1])
    assert np.array_equal(t["quantiles"]["longest"], np.quantile(t["longest"], [0.1, 0.5, 0.9], axis=0))
    assert "prospective_area" not in ic.intercept_tables(tab, dz)


def test_csv_frames(tmp_path):
    from geobo_amd import intercepts as ic
    rng = np.random.default_rng(2)
    n, Cn, ny, nx = 5, 2, 3, 4
    out = dict(cutoffs=np.array([1.5, 0.5]))
    out.update(ic.intercept_tables(rng.integers(0, 9, size=(n, Cn, 3)), 25.0, column_area=100.0))
    frame = ic.curve_frame(out)
    assert list(frame.columns) == ["CUTOFF", "AREA_P10", "AREA_P50", "AREA_P90", "AREA_MEAN", "LONGEST_P10", "LONGEST_P50", "LONGEST_P90",
                                   "LONGEST_MEAN"] == list(ic.CSV_COLUMNS)
    assert np.array_equal(frame["CUTOFF"], out["cutoffs"]) and np.allclose(frame["AREA_MEAN"], out["prospective_area"].mean(0))
    assert np.array_equal(frame["LONGEST_P50"], out["quantiles"]["longest"][1])
    summary = dict(probability=rng.random((Cn, ny, nx)), probability_any=rng.random((Cn, ny, nx)), depth_to_top_mean=rng.random((Cn, ny, nx)),
                   accumulation_mean=rng.random((Cn, ny, nx)))
    for key in ("thickness", "intercept_length"):
        summary[key] = {q: rng.random((Cn, ny, nx)) for q in ("mean", "p10", "p50", "p90")}
    out.update(summary)
    x, y = np.array([50.0, 150.0, 250.0, 350.0]), np.array([10.0, 30.0, 50.0])
    mf = ic.map_frame(out, x, y)
    assert list(mf.columns) == list(ic.MAP_COLUMNS) and len(mf) == Cn * ny * nx
    row = mf.iloc[1 * ny * nx + 2 * nx + 3]                    # cutoff 1, iy = 2, ix = 3
    assert (row["X"], row["Y"], row["CUTOFF"]) == (350.0, 50.0, 0.5)
    assert row["PROBABILITY"] == out["probability"][1, 2, 3] and row["THICKNESS_P90"] == out["thickness"]["p90"][1, 2, 3]
    assert row["LENGTH_MEAN"] == out["intercept_length"]["mean"][1, 2, 3] and row["ACCUMULATION_MEAN"] == out["accumulation_mean"][1, 2, 3]
    mf.to_csv(tmp_path / "intercept_maps.csv", index=False)
    assert (tmp_path / "intercept_maps.csv").read_text().splitlines()[0].split(",") == list(ic.MAP_COLUMNS)
    holes = {k: ({q: a.reshape(Cn, -1)[:, :3] for q, a in v.items()} if isinstance(v, dict) else v.reshape(Cn, -1)[:, :3])
             for k, v in summary.items()}
    holes["cutoffs"] = out["cutoffs"]
    hf = ic.hole_frame(holes)
    assert list(hf.columns) == list(ic.HOLE_COLUMNS) and hf["HOLE"].tolist() == [0, 1, 2, 0, 1, 2] and hf["CUTOFF"].tolist() == [1.5] * 3 + [0.5] * 3
    assert hf["DEPTH_TO_TOP_MEAN"][4] == holes["depth_to_top_mean"][1, 1]
    del out["prospective_area"]
    assert np.isnan(ic.curve_frame(out)["AREA_P50"]).all()     # holes and paths have no area


def test_launch_cuts_and_yaml_key():
    from geobo_amd import intercepts as ic
    assert ic.launch_cuts(64, 16, 4096) == 64                                  # 16 MiB of workspace: one launch
    assert ic.launch_cuts(64, 16, 4096, detail=True) == 64 and ic.launch_cuts(1000, 16, 4096, detail=True) == (1 << 30) // (4096 * 16 * 44) == 372
    assert ic.launch_cuts(64, 32, 128 * 128, ws_bytes=1 << 20) == 1           # at least one sample
    assert ic.launch_cuts(0, 4, 10) == 1
    for S, Cn, K, det in ((64, 16, 4096, True), (7, 32, 100000, True), (256, 5, 80, False)):
        Sl = ic.launch_cuts(S, Cn, K, det)
        assert 1 <= Sl <= S and (Sl == 1 or Sl * K * Cn * (44 if det else 4) <= ic.WS_BYTES)
    kw, along = ic.parse_yaml(dict(cutoffs=[1, 2.5], property="density", samples=12, offset=0.5, min_length=200, max_gap=100))
    assert kw == dict(cutoffs=[1.0, 2.5], prop="density", n=12, offset=0.5, min_length=200.0, max_gap=100.0) and along is None
    assert ic.parse_yaml(dict(cutoffs=[0])) == (dict(cutoffs=[0.0], prop="drill", n=256, offset=0.0, min_length=None, max_gap=0.0), None)
    assert ic.parse_yaml(dict(cutoffs=[0], holes=[[1, 2], [3, 4]]))[1] == dict(holes=[(1, 2), (3, 4)])
    assert ic.parse_yaml(dict(cutoffs=[0], paths=[[1, 2, 30, 60]], step=25))[1] == dict(paths=[(1.0, 2.0, 30.0, 60.0)], step=25.0)
    for bad in (None, {}, dict(property="drill"), dict(cutoffs=[0], block=[2, 2, 2]), dict(cutoffs=[0], holes=[[1, 2]], paths=[[1, 2, 3, 4]])):
        with pytest.raises(ValueError):
            ic.parse_yaml(bad)
    # the key reaches the settings object run_geobo reads it from
    s = settings_for(4, 3, 2, drill_intercepts=dict(cutoffs=[0.0], samples=4))
    assert ic.parse_yaml(s.drill_intercepts)[0]["n"] == 4


def test_interface_is_there():
    import inspect

    from geobo_amd.engine import PosteriorEngine
    from geobo_amd.intercepts import InterceptMixin
    from geobo_amd.inversion import Inversion
    assert issubclass(PosteriorEngine, InterceptMixin) and callable(PosteriorEngine.trace_statistics)
    sig = inspect.signature(Inversion.drill_intercepts)
    assert list(sig.parameters)[1:] == ["cutoffs", "prop", "n", "seed", "start", "batch", "offset", "require", "region", "min_length", "max_gap",
                                        "holes", "paths", "step", "approximate", "write"]
    assert sig.parameters["prop"].default == "drill" and sig.parameters["n"].default == 256 and sig.parameters["batch"].default == 64
    assert list(inspect.signature(Inversion.column_intercepts).parameters)[1:] == ["cube", "cutoff", "min_length", "max_gap", "region"]
    assert list(inspect.signature(PosteriorEngine.trace_statistics).parameters)[1:11] == ["F", "p", "thresholds", "lo", "mask", "traces", "min_len",
                                                                                          "max_gap", "maps", "detail"]
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=settings_for(4, 3, 2)).drill_intercepts([0.0], prop="density")
