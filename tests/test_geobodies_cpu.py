"""Connected ore bodies without a GPU: the exported symbols and the argument checks of geobo_bodies, the host
logic of geobodies.py (seeds, block mapping, renumbering, tables, the CSV frame, the launch cuts), and the reference of the GPU tests
itself: scipy.ndimage.label against a plain breadth-first search on the small shapes."""
import ctypes as C
import os

import numpy as np
import pytest

import _geobodies_ref as ref
from conftest import settings_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dbl(*v):
    return (C.c_double * len(v))(*v)


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


# ---- 1. C ABI without a GPU ------------------------------------------------------------------------------------------------------
def test_symbols_and_signatures():
    from geobo_amd import _lib, build
    L = _lib.load()
    assert L.geobo_version() == 213
    assert "geobodies.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "geobodies.hip"))
    header = open(os.path.join(ROOT, "include", "geobo_hip.h")).read()
    for name in ("geobo_bodies", "geobo_bodies_ws_bytes"):
        assert name + "(" in header
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert "#define GEOBO_VERSION 213 " in header
    assert len(_lib.SIGNATURES["geobo_bodies"][1]) == 27 and len(_lib.SIGNATURES["geobo_bodies_ws_bytes"][1]) == 5


def test_bodies_validates_without_gpu():
    from geobo_amd import _lib
    L = _lib.load()
    p = 16                                                     # (never dereferenced: every call below fails its checks first)
    grid = (5, 7, 9)
    n = 315
    wsb = L.geobo_bodies_ws_bytes
    inf = float("inf")
    nan = float("nan")

    def call(S=3, F=p, ss=3 * n, ps=n, g=grid, prop=1, t=(-inf, 0.0, 0.0, 1.5), lo=(-inf, -inf, -inf), mask=None, weight=None, nb=6,
             min_count=1, seeds=(0, 17, n - 1), K=None, stats=p, sums=p, hl=None, hs=None, labels=None, info=p, phases=15, ws=p,
             nbytes=None, Cn=None):
        Cn = (4 if t is None else len(t)) if Cn is None else Cn
        nbytes = wsb(3, *grid, 4) if nbytes is None else nbytes
        K = (0 if seeds is None else len(seeds)) if K is None else K
        return L.geobo_bodies(S, F, ss, ps, *g, prop, Cn, None if t is None else _dbl(*t), None if lo is None else _dbl(*lo), mask, weight, nb,
                              min_count, K, None if seeds is None else _i32(*seeds), stats, sums, hl, hs, labels, info, phases, ws, nbytes, None)
    for name in ("F", "t", "lo", "stats", "sums", "info", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(seeds=None, K=2) == -1                                             # seeds announced and not given
    for nb in (0, 4, 8, 18, 27, -6):
        assert call(nb=nb) == -1, nb
    assert call(t=(0.0, 1.0, 0.5, 2.0)) == -1                                     # unsorted
    assert call(t=(0.0, nan, 1.0, 2.0)) == -1 and call(t=(nan, 0.0, 1.0, 2.0)) == -1
    assert call(lo=(-inf, nan, -inf)) == -1
    for bad in ((0, n), (-1, 3), (5, 2 ** 31 - 1)):                                # a seed index out of range
        assert call(seeds=bad) == -1, bad
    assert call(K=-1) == -1 and call(seeds=tuple(range(n)) + (0,)) == -1          # K < 0, K > n
    assert call(nbytes=wsb(3, *grid, 4) - 16) == -1 and call(nbytes=0) == -1      # a short workspace
    assert call(ws=24) == -1                                                      # not 16-byte aligned
    assert call(S=-1) == -1 and call(Cn=0) == -1 and call(min_count=0) == -1
    assert call(t=tuple(float(i) for i in range(33)), nbytes=1 << 30) == -1       # C = 33
    assert call(prop=-1) == -1 and call(prop=3) == -1
    assert call(phases=0) == -1 and call(phases=16) == -1 and call(phases=32) == -1 and call(phases=-1) == -1      # no stage, unknown bits
    assert call(ps=n - 1) == -1 and call(ss=3 * n - 1) == -1
    for axis in range(3):
        assert call(g=tuple(0 if i == axis else v for i, v in enumerate(grid))) == -1
    assert call(g=(2048, 2048, 2048), ps=1 << 40, ss=1 << 42) == -1               # n > INT32_MAX
    assert call(S=16384, ss=3 * n, nbytes=1 << 40) == -1                          # S C > 65535 volumes
    # the workspace size: 0 for invalid arguments, a multiple of 16 that grows with the volumes otherwise
    assert wsb(-1, *grid, 4) == 0 and wsb(3, 0, 7, 9, 4) == 0 and wsb(3, *grid, 0) == 0 and wsb(3, *grid, 33) == 0
    assert wsb(3, 2048, 2048, 2048, 4) == 0 and wsb(65536, *grid, 1) == 0
    for g in ((1, 1, 1), (1, 1, 70), grid, (64, 64, 64)):
        m = g[0] * g[1] * g[2]
        last = 0
        for S, Cn in ((0, 1), (1, 1), (1, 4), (3, 4), (64, 16)):
            b = wsb(S, *g, Cn)
            assert b >= 16 * max(S, 1) * Cn * m and b % 16 == 0 and b >= last, (g, S, Cn, b)
            last = b


# ---- 2. host logic ---------------------------------------------------------------------------------------------------------------
def test_seed_parsing_and_block_mapping():
    from geobo_amd import geobodies as G
    grid = (4, 5, 3)                                                              # (ny, nx, nz)
    assert G.parse_seeds(None, grid).size == 0 and G.parse_seeds(None, grid).dtype == np.int32
    cube = np.zeros(grid, dtype=bool)
    cube[1, 2, 0] = cube[3, 4, 2] = cube[0, 0, 1] = True
    want = np.array([1, (1 * 5 + 2) * 3 + 0, (3 * 5 + 4) * 3 + 2], dtype=np.int32)
    assert np.array_equal(G.parse_seeds(cube, grid), want)
    xyz = np.array([[4, 3, 2], [2, 1, 0], [0, 0, 1], [2, 1, 0]])                   # (ix, iy, iz), one of them twice
    got = G.parse_seeds(xyz, grid)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(G.parse_seeds("drill", grid, drill=np.array([59, 1, 21])), want)
    for bad in ("holes", np.zeros((5, 4, 3), dtype=bool), np.zeros((3, 2), dtype=int), np.zeros((3,), dtype=int), np.zeros((2, 3)),
                np.array([[5, 0, 0]]), np.array([[0, 4, 0]]), np.array([[0, 0, -1]])):
        with pytest.raises(ValueError):
            G.parse_seeds(bad, grid)
    with pytest.raises(ValueError):
        G.parse_seeds("drill", grid)
    with pytest.raises(ValueError):
        G.parse_seeds("drill", grid, drill=[60])
    # blocks of (by, bx, bz) = (2, 3, 2): 2 x 2 x 2 blocks
    box = (2, 3, 2)
    blocks = G.seeds_to_blocks(want, grid, box)
    by = lambda v: ((v // 15) // 2 * 2 + ((v // 3) % 5) // 3) * 2 + (v % 3) // 2
    assert blocks.dtype == np.int32 and np.array_equal(blocks, np.unique([by(int(v)) for v in want]))
    assert np.array_equal(G.seeds_to_blocks(np.arange(60), grid, box), np.arange(8))
    assert G.seeds_to_blocks(np.zeros(0, dtype=np.int32), grid, box).size == 0
    assert G.check_neighbours(6) == 6 and G.check_neighbours(np.int64(26)) == 26
    for bad in (0, 18, 27, "6", 6.0, True, None):
        with pytest.raises(ValueError):
            G.check_neighbours(bad)
    assert G.check_probability(None) == (False, False) and G.check_probability("both") == (True, True)
    assert G.check_probability("largest") == (True, False) and G.check_probability("seeded") == (False, True)
    with pytest.raises(ValueError):
        G.check_probability("all")


@pytest.mark.parametrize("neighbours", [6, 26])
def test_renumbering_is_scipys(neighbours):
    from scipy import ndimage

    from geobo_amd import geobodies as G
    rng = np.random.default_rng(neighbours)
    for grid in ((1, 1, 1), (1, 1, 9), (4, 5, 3), (6, 6, 6)):
        for occ in (0.0, 0.2, 0.5, 1.0):
            inset = rng.random(grid) < occ
            numbered, sizes = G.renumber(ref.label_scipy(inset, neighbours))
            lab, B = ndimage.label(inset, structure=ndimage.generate_binary_structure(3, 1 if neighbours == 6 else 3))
            assert numbered.dtype == np.int32 and numbered.shape == grid and np.array_equal(numbered, lab)
            assert sizes.dtype == np.int64 and np.array_equal(sizes, np.bincount(lab.reshape(-1), minlength=B + 1)[1:])


def test_tables_quantiles_and_csv(tmp_path):
    from geobo_amd import geobodies as G
    rng = np.random.default_rng(7)
    n, Cn = 9, 3
    stats = np.zeros((n, Cn, 6), dtype=np.int64)
    stats[..., 0] = rng.integers(40, 90, size=(n, Cn))
    stats[..., 1] = rng.integers(1, 9, size=(n, Cn))
    stats[..., 2] = rng.integers(5, 40, size=(n, Cn))
    stats[..., 3] = rng.integers(0, 100, size=(n, Cn))
    stats[..., 4] = rng.integers(0, 30, size=(n, Cn))
    stats[..., 5] = rng.integers(1, 3, size=(n, Cn))
    stats[:, 2, :] = 0                                                            # a cutoff nothing passes
    stats[:, 2, 3] = -1
    stats[4, 1, 4:] = 0                                                           # a realisation whose seeds all miss
    sums = rng.standard_normal((n, Cn, 3)) * stats[..., [0, 2, 4]]
    scale, offset, vv = float(np.float32(2.5)), 10.0, 100.0 * 50.0 * 25.0
    out = G.body_tables(stats, sums, scale, offset, vv)
    assert np.array_equal(out["count"], stats[..., 0]) and np.array_equal(out["n_bodies"], stats[..., 1]) and out["count"].dtype == np.int64
    assert np.array_equal(out["largest"]["label"], stats[..., 3]) and np.array_equal(out["seeded"]["bodies"], stats[..., 5])
    for key, k_cnt, k_sum in (("largest", 2, 1), ("seeded", 4, 2)):
        part = out[key]
        assert np.array_equal(part["count"], stats[..., k_cnt]) and np.array_equal(part["volume"], stats[..., k_cnt] * vv)
        assert np.allclose(part["quantity"], (scale * sums[..., k_sum] + offset * stats[..., k_cnt]) * vv, rtol=1e-15, atol=0)
        ok = stats[..., k_cnt] > 0
        assert np.isnan(part["grade"][~ok]).all() and np.allclose(part["grade"][ok], scale * sums[..., k_sum][ok] / stats[..., k_cnt][ok] + offset,
                                                                  rtol=1e-13)
    assert np.isnan(out["seeded"]["grade"][4, 1]) and np.isnan(out["largest"]["grade"][:, 2]).all()
    q = out["quantiles"]
    assert set(q) == {"n_bodies", "largest_volume", "seeded_volume"} and all(v.shape == (3, Cn) for v in q.values())
    assert np.array_equal(q["n_bodies"], np.quantile(stats[..., 1].astype(float), [0.1, 0.5, 0.9], axis=0))
    assert np.array_equal(q["largest_volume"], np.quantile(stats[..., 2] * vv, [0.1, 0.5, 0.9], axis=0))
    out["cutoffs"] = np.array([0.5, 1.5, 9.0])
    frame = G.bodies_frame(out)
    assert list(frame.columns) == list(G.CSV_COLUMNS) and frame.columns[0] == "CUTOFF" and len(frame) == Cn
    assert np.array_equal(frame["CUTOFF"], out["cutoffs"]) and np.allclose(frame["BODIES_MEAN"], stats[..., 1].mean(0))
    assert np.allclose(frame["SEEDED_VOLUME_P50"], q["seeded_volume"][1]) and np.isnan(frame["LARGEST_GRADE_MEAN"][2])
    assert np.isclose(frame["SEEDED_GRADE_MEAN"][1], np.nanmean(out["seeded"]["grade"][:, 1]))
    frame.to_csv(tmp_path / "geobodies.csv", index=False)
    assert (tmp_path / "geobodies.csv").read_text().splitlines()[0].split(",") == list(G.CSV_COLUMNS)


def test_launch_cuts():
    from geobo_amd import _lib, geobodies as G
    wsb = _lib.load().geobo_bodies_ws_bytes
    assert G.launch_cuts(64, 16, 64 ** 3) == (15, 16)                              # 1 GiB: 255 volumes of 4.2 MB
    assert G.launch_cuts(2, 5, 480, ws_bytes=16000) == (1, 2) and G.launch_cuts(2, 5, 480, ws_bytes=1) == (1, 1)
    assert G.launch_cuts(64, 5, 480) == (64, 5) and G.launch_cuts(100000, 1, 8) == (65535, 1)
    for S, Cn, grid, bound in ((64, 16, (64, 64, 64), 1 << 30), (7, 5, (8, 10, 6), 60000), (3, 32, (1, 1, 70), 1 << 14)):
        n = grid[0] * grid[1] * grid[2]
        Sl, Cl = G.launch_cuts(S, Cn, n, ws_bytes=bound)
        assert 1 <= Sl <= S and 1 <= Cl <= Cn and Sl * Cl <= 65535
        assert 0 < wsb(Sl, *grid, Cl) <= bound + 4 * n + 64                        # (the staged seeds are per launch, not per volume)


def test_interface_is_there():
    from geobo_amd.engine import PosteriorEngine
    from geobo_amd.geobodies import GeobodyMixin
    from geobo_amd.inversion import Inversion
    assert issubclass(PosteriorEngine, GeobodyMixin) and callable(PosteriorEngine.body_statistics)
    assert callable(Inversion.geobodies) and callable(Inversion.label_bodies)
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=settings_for(4, 3, 2)).geobodies([0.0], prop="density")


# ---- 3. the yardstick of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbours", [6, 26])
@pytest.mark.parametrize("grid", [(1, 1, 1), (1, 1, 70), (3, 1, 130), (5, 7, 9), (16, 16, 16)])
def test_scipy_reference_against_bfs(grid, neighbours):
    rng = np.random.default_rng(100 * grid[2] + neighbours)
    n = grid[0] * grid[1] * grid[2]
    for name, inset in ref.patterns(grid, rng):
        a, b = ref.label_scipy(inset, neighbours), ref.label_bfs(inset, neighbours)
        assert a.dtype == np.int32 and np.array_equal(a, b), name
        flat = a.reshape(-1)
        assert np.array_equal(flat >= 0, inset.reshape(-1)) and np.all(flat <= np.arange(n))
        roots = np.flatnonzero(flat == np.arange(n))
        if name == "full":
            assert roots.tolist() == [0]
        if name == "checkerboard" and neighbours == 6:
            assert roots.size == (n + 1) // 2
        if name == "checkerboard" and neighbours == 26 and sum(g > 1 for g in grid) >= 2:
            assert roots.size == 1
        if name in ("serpentine", "spiral", "comb_last_plane", "comb_last_row", "u_shape"):
            assert roots.tolist() == [0], name                                    # one body, labelled by its end of the chain
        if name == "corner_touch" and min(grid) > 1:
            assert roots.size == (2 if neighbours == 6 else 1)
        if name == "edge_touch" and grid[0] > 1 and grid[1] > 1:
            assert roots.size == (2 if neighbours == 6 else 1)


def test_reference_statistics_on_a_known_case():
    """Two bars and a speck on a 1 x 4 x 6 grid: counts, the tie-break, seeds and sums by hand."""
    grid = (1, 4, 6)
    F = np.full((1, 3, 24), -1.0)
    x = F[0, 0].reshape(4, 6)
    x[0, 0:3] = [1.0, 2.0, 3.0]                                                   # body 0: voxels 0, 1, 2
    x[2, 0:3] = [4.0, 5.0, 6.0]                                                   # body 12: voxels 12, 13, 14 (the same size)
    x[3, 5] = 7.0                                                                 # body 23, next to nothing
    x[1, 3] = 0.5                                                                 # voxel 9: diagonal to 2 and to 14, joins the bars at 26 alone
    r6 = ref.bodies(F, grid, 0, [0.0], neighbours=6, min_count=2, seeds=[13, 5, 23])
    assert r6["stats"][0, 0].tolist() == [8, 2, 3, 0, 4, 2]                       # the tie goes to label 0; seeds hit 12 and 23, 5 is outside
    assert r6["sums"][0, 0].tolist() == [28.5, 6.0, 22.0]
    assert np.flatnonzero(r6["in_seeded"][0, 0]).tolist() == [12, 13, 14, 23]
    assert np.unique(r6["labels"][0, 0]).tolist() == [-1, 0, 9, 12, 23]
    r26 = ref.bodies(F, grid, 0, [0.0], neighbours=26, min_count=2, seeds=[13, 5], labeller=ref.label_bfs)
    assert r26["stats"][0, 0].tolist() == [8, 1, 7, 0, 7, 1]
    assert r26["sums"][0, 0].tolist() == [28.5, 21.5, 21.5]
    w = np.arange(1, 25, dtype=np.int32)                                          # w[v] = v + 1
    rw = ref.bodies(F, grid, 0, [0.0, 4.5], neighbours=6, weight=w, seeds=[])
    assert rw["stats"][0, 0].tolist() == [1 + 2 + 3 + 10 + 13 + 14 + 15 + 24, 4, 42, 12, 0, 0]
    assert rw["stats"][0, 1].tolist() == [14 + 15 + 24, 2, 29, 13, 0, 0] and rw["sums"][0, 1, 1] == 14 * 5.0 + 15 * 6.0
