"""Prediction at arbitrary points on the device: geobo_ak_points by value against the oracle's covariance
functions and bit for bit against geobo_ak_fused, Inversion.predict_points against the oracle's dense posterior with the query
points stacked under the grid points (the construction tests/test_points_cpu.py checks on the host), against cubing() at voxel
centres, predict_path against hole_statistics(), and the error paths.

The values are raw: the reference's matern32 prior is slightly indefinite, so nothing here asserts a positive variance."""
import numpy as np
import pytest
import torch

from conftest import load_golden, normwise, settings_for
from oracle import geobo_oracle as O
from test_blockstats_gpu import _cubing, _host_operator, _inv
from test_points_cpu import extended_posterior, query_index

pytestmark = pytest.mark.gpu

TINY = dict(nx=10, ny=8, nz=6)
CUBE16 = dict(nx=16, ny=16, nz=16)


# ---- 1. the kernel by value ----------------------------------------------------------------------------------------------------------
def _soa(hip, P, n_pad):
    """Padded SoA of the points P (n, 3): copies of the last point behind n."""
    pad = lambda v: np.concatenate([v, np.full(n_pad - v.size, v[-1])])
    return tuple(hip.to_dev(pad(np.ascontiguousarray(P[:, d]))) for d in range(3))


def _query_pool(P, rng, n):
    """n query points: a grid point (d^2 = 0), a point farther than any sparse support from every voxel, the rest off the grid."""
    lo, hi = P.min(axis=0), P.max(axis=0)
    off = lo + rng.uniform(-0.3, 1.3, (n, 3)) * (hi - lo)
    off[0] = P[len(P) // 3]
    off[1] = hi + 5000.0
    return off


@pytest.mark.parametrize("kid", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("R_pad,rows", [(128, 48), (384, 300)])
@pytest.mark.parametrize("dims", [(8, 6, 5), (10, 8, 6)])            # N = 240 -> 256 and 480 -> 512
def test_ak_points_matches_oracle(dims, R_pad, rows, kid):
    from geobo_amd import hip
    hip.require_gpu()
    name, cross = ("exp", "matern32", "sparse")[(kid - 1) // 2], kid % 2 == 0
    assert hip.kernel_id(name, cross) == kid
    P = O.grid_points(dims, (100.0, 110.0, 90.0))
    N, Np = P.shape[0], hip.pad_n(P.shape[0])
    rng = np.random.default_rng(100 * kid + R_pad + N)
    A = np.zeros((R_pad, Np))
    A[:rows, :N] = rng.standard_normal((rows, N))
    Ad, xyz = hip.to_dev(A), _soa(hip, P, Np)
    l1, l2 = (210.0, 240.0) if cross else (210.0, 210.0)
    pool = _query_pool(P, rng, 130)
    for nq in (1, 127, 128, 130):                                     # 130 pads to 256: two column tiles
        Q = pool[:nq]
        nqp = hip.pad_n(nq)
        d2 = O.sqdist(P, Q)
        if nq >= 2:
            assert d2[:, 0].min() == 0.0 and np.sqrt(d2[:, 1].min()) > 240.0
        ref = A[:rows, :N] @ (0.4 * 1.1 * (O.k_cross(name, d2, l1, l2) if cross else O.k_auto(name, d2, l1)))
        out = torch.full((R_pad, nqp), float("nan"), dtype=torch.float64, device="cuda")
        hip.ak_points(kid, Ad, xyz, _soa(hip, Q, nqp), l1, l2, 0.4, 1.1, out)
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), (nq, "out arrives as NaN and comes back finite")
        err = np.abs(got[:rows, :nq] - ref).max() / np.abs(ref).max()
        assert err <= 5e-12, (nq, err)
        assert np.abs(got[rows:]).max() == 0.0                        # zero operator rows -> zero product rows


@pytest.mark.parametrize("name,cross", [("exp", False), ("matern32", True)])
def test_ak_points_is_the_generator_of_ak_fused(name, cross):
    """The column points set to a slice of the contraction points: the same bits as geobo_ak_fused on that slice."""
    from geobo_amd import hip
    hip.require_gpu()
    P = O.grid_points((10, 8, 6), (100.0, 110.0, 90.0))
    N, Np, Msp, Ms = P.shape[0], 512, 256, 200
    A = np.zeros((Msp, Np))
    A[:Ms, :N] = np.random.default_rng(5).standard_normal((Ms, N))
    Ad, xyz = hip.to_dev(A), _soa(hip, P, Np)
    l1, l2 = (210.0, 240.0) if cross else (210.0, 210.0)
    kid = hip.kernel_id(name, cross)
    fused = torch.full((Msp, 128), float("nan"), dtype=torch.float64, device="cuda")
    hip.ak_fused(kid, Ad, xyz, 128, 128, l1, l2, 0.4, 1.1, fused)
    points = torch.full((Msp, 128), float("nan"), dtype=torch.float64, device="cuda")
    hip.ak_points(kid, Ad, xyz, tuple(c[128:256] for c in xyz), l1, l2, 0.4, 1.1, points)
    assert torch.isfinite(fused).all() and torch.equal(points, fused)


# ---- 2. against the oracle's dense posterior ----------------------------------------------------------------------------------------
def _query_points(inv, rng):
    """About 150 points in the cube's own coordinates: the 8 corners of the box, 40 voxel centres (the drilled voxels among them),
    100 uniform points and a duplicate."""
    s = inv.settings
    lo, hi = np.array([0.0, 0.0, s.zmax - s.zLcube]), np.array([s.xLcube, s.yLcube, s.zmax])
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    N = inv.voxelpos.shape[1]
    drilled = inv._sel[:20]
    vox = np.concatenate([drilled, rng.choice(np.setdiff1d(np.arange(N), drilled), 40 - drilled.size, replace=False)])
    uniform = lo + rng.uniform(0.0, 1.0, (100, 3)) * (hi - lo)
    return np.vstack([corners, inv.voxelpos.T[vox], uniform, uniform[17:18]]), vox


# (golden case, grid, Inversion arguments, GEOBO_ROWS).  Streamed operators exist only where the spectral product runs (grid extents
# that are multiples of 16: the engine refuses them on the 10 x 8 x 6 cases), so that route is checked on the smallest such case.
ORACLE_CASES = [("tiny_exp", TINY, dict(method="auto"), False),
                ("tiny_matern32", TINY, dict(method="auto"), True),
                ("tiny_sparse", TINY, dict(method="auto"), False),
                ("cube16_matern32", CUBE16, dict(operators="streamed"), False)]


@pytest.mark.parametrize("name,dims,kw,rows", ORACLE_CASES, ids=["tiny_exp", "tiny_matern32-rows", "tiny_sparse", "cube16_matern32-streamed"])
def test_predict_points_match_oracle(name, dims, kw, rows, monkeypatch):
    if rows:
        monkeypatch.setenv("GEOBO_ROWS", "1")
    f = load_golden(name + ".npz")
    s = settings_for(**dims, kernelfunc=name.split("_")[1])
    inv = _inv(s, **kw)
    inv.gp_length = f["gp_length_in"].copy()
    _cubing(inv, f)
    eng = inv.engine
    if "operators" in kw:
        from geobo_amd.operators import StreamedOperator
        assert all(isinstance(A, StreamedOperator) for A in eng.last["ops"])
    pts, vox = _query_points(inv, np.random.default_rng(3))
    nq = pts.shape[0]
    assert 145 <= nq <= 155 and np.isin(inv._sel[:min(20, inv._sel.size)], vox).all()
    got = inv.predict_points(pts, full_cov=True)
    print("%s [%s] %d points" % (name, eng.step_route, nq))
    assert got["mean"].shape == got["var"].shape == got["std"].shape == (3, nq) and got["cov"].shape == (3 * nq, 3 * nq)
    # the oracle on the engine's own operators, query points stacked under the grid points
    A_g, A_m = (_host_operator(eng, A) for A in inv._operators())
    P = O.grid_points((s.xNcube, s.yNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize))
    Q = inv.to_covariance_frame(pts).T
    r, N1 = extended_posterior(P, Q, A_g, A_m, inv._sel, inv.Fs3, np.array(inv.gp_length, dtype=float), O.weight_matrix(inv.coeffm),
                               s.kernelfunc, inv.gp_sigma, gp_amp=inv.gp_amp)
    qi = query_index(P.shape[0], N1, nq)
    scale = np.array([float(v) for v in inv._cube_scale])
    mu, var, cov = r["mu"][qi].reshape(3, nq), r["var"][qi].reshape(3, nq), r["cov"][np.ix_(qi, qi)]
    for a in range(3):
        e_mu, e_var = normwise(got["mean"][a], mu[a] * scale[a]), normwise(got["var"][a], var[a] * scale[a] ** 2)
        print("    property %d: mean %.2e  var %.2e" % (a, e_mu, e_var))
        assert e_mu <= 1e-10 and e_var <= 1e-10, (name, a)
        for b in range(3):
            want = cov[a * nq:(a + 1) * nq, b * nq:(b + 1) * nq] * scale[a] * scale[b]
            err = normwise(got["cov"][a * nq:(a + 1) * nq, b * nq:(b + 1) * nq], want)
            print("    cov%d%d %.2e" % (a, b, err))
            assert err <= 1e-10, (name, a, b)
    assert np.array_equal(got["cov"], got["cov"].T)
    assert np.allclose(np.diag(got["cov"]), got["var"].reshape(-1), rtol=1e-12, atol=0)
    with np.errstate(all="ignore"):
        ok = got["var"] >= 0
        assert np.array_equal(np.isnan(got["std"]), ~ok) and np.allclose(got["std"][ok], np.sqrt(got["var"][ok]), rtol=1e-14, atol=0)
    # the voxel centres among the points: cubing()'s own values (to the cube tolerance: another route computed those)
    k0 = 8
    for a in range(3):
        assert normwise(got["mean"][a, k0:k0 + vox.size], inv.mu_rec.reshape(3, -1)[a][vox] * scale[a]) <= 1e-8
    # the duplicated point: two equal columns
    assert np.array_equal(got["mean"][:, -1], got["mean"][:, 8 + vox.size + 17]) and np.array_equal(got["var"][:, -1], got["var"][:, 8 + vox.size + 17])
    # batches of 64 points (the column unit rounds them up): the same values
    small = inv.predict_points(pts, full_cov=True, batch=64)
    for k in ("mean", "var", "cov"):
        assert normwise(small[k], got[k]) <= 1e-13, k
    if "operators" in kw:
        # the streamed operator in two row batches of 128 (the default holds its 256 rows in one): the same values
        from geobo_amd import hip
        from geobo_amd.engine import create_cov_lengths
        q = tuple(hip.to_dev(np.ascontiguousarray(c)) for c in inv.to_covariance_frame(pts))
        lengths = [float(v) for v in create_cov_lengths(np.array(inv.gp_length, dtype=float))]
        m2, v2 = eng.predict_points(q, s.kernelfunc, lengths, inv.coeffm, inv.gp_amp, op_rows=128)
        assert normwise(m2.cpu().numpy() * scale[:, None], got["mean"]) <= 1e-13
        assert normwise(v2.cpu().numpy() * scale[:, None] ** 2, got["var"]) <= 1e-13
        with pytest.raises(ValueError, match="op_rows"):
            eng.predict_points(q, s.kernelfunc, lengths, inv.coeffm, inv.gp_amp, op_rows=100)
    plain = inv.predict_points(pts)
    assert "cov" not in plain and normwise(plain["mean"], got["mean"]) <= 1e-13 and normwise(plain["var"], got["var"]) <= 1e-13


def test_no_drill_data_gives_nan_drill_entries():
    f = load_golden("tiny_exp_nodrill.npz")
    inv = _inv(settings_for(**TINY))
    inv.gp_length = f["gp_length_in"].copy()
    cubes = _cubing(inv, f)
    assert inv._sel.size == 0 and np.isnan(cubes[2]).all()
    idx = np.array([0, 17, 479])
    got = inv.predict_points(np.vstack([inv.voxelpos.T[idx], [[333.0, 410.0, -77.0]]]), full_cov=True)
    n = 4
    for k in ("mean", "var", "std"):
        assert np.isfinite(got[k][:2]).all() and np.isnan(got[k][2]).all()
    assert np.isfinite(got["cov"][:2 * n, :2 * n]).all() and np.isnan(got["cov"][2 * n:]).all() and np.isnan(got["cov"][:, 2 * n:]).all()
    for a in range(2):
        assert normwise(got["mean"][a, :3], np.asarray(cubes[a]).reshape(-1)[idx]) <= 1e-8
        assert normwise(got["var"][a, :3], np.asarray(cubes[3 + a]).reshape(-1)[idx]) <= 1e-8


# ---- 3. on the grid: cubing()'s own cubes -------------------------------------------------------------------------------------------
def _cube16(method):
    f = load_golden("cube16_matern32.npz")
    s = settings_for(**CUBE16, kernelfunc="matern32")
    inv = _inv(s, method=method)
    inv.gp_length = f["gp_length_in"].copy()
    return inv, _cubing(inv, f)


@pytest.fixture(scope="module")
def cube16_spectral():
    return _cube16("spectral")


def _spread_voxels(inv, n=300):
    """n voxel indices: the 8 corner voxels, rim voxels, the drilled voxels and an even spread."""
    ny, nx, nz = inv.settings.yNcube, inv.settings.xNcube, inv.settings.zNcube
    flat = lambda iy, ix, iz: (iy * nx + ix) * nz + iz
    corners = [flat(iy, ix, iz) for iy in (0, ny - 1) for ix in (0, nx - 1) for iz in (0, nz - 1)]
    rim = [flat(0, ix, 3) for ix in range(nx)] + [flat(iy, nx - 1, nz - 1) for iy in range(ny)] + [flat(5, 0, iz) for iz in range(nz)]
    first = np.unique(np.concatenate([corners, rim, inv._sel[:60]]))
    spread = np.setdiff1d(np.linspace(0, ny * nx * nz - 1, 2 * n).astype(np.int64), first)
    return np.concatenate([first, spread[:n - first.size]])


def _on_grid_identity(inv, cubes):
    idx = _spread_voxels(inv)
    assert idx.size == 300 and np.unique(idx).size == 300 and np.isin(inv._sel[:60], idx).all()
    before = inv.block_statistics((4, 4, 4))
    got = inv.predict_points(inv.voxelpos.T[idx])
    errs = [normwise(got["mean"][a], np.asarray(cubes[a]).reshape(-1)[idx]) for a in range(3)]
    errs += [normwise(got["var"][a], np.asarray(cubes[3 + a]).reshape(-1)[idx]) for a in range(3)]
    print("16^3 [%s] predict_points at 300 voxel centres vs cubing(): mean %s  var %s" % (inv.engine.step_route, errs[:3], errs[3:]))
    assert max(errs) <= 1e-8
    after = inv.block_statistics((4, 4, 4))
    assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before)
    for a in range(3):
        assert np.array_equal(inv.mu_rec.reshape(3, -1)[a][idx] * inv._cube_scale[a], np.asarray(cubes[a]).reshape(-1)[idx])


def test_voxel_centres_reproduce_the_cubes_spectral(cube16_spectral):
    _on_grid_identity(*cube16_spectral)


def test_voxel_centres_reproduce_the_cubes_dense():
    _on_grid_identity(*_cube16("dense"))


# ---- 4. path -------------------------------------------------------------------------------------------------------------------------
def test_vertical_path_matches_hole_statistics(cube16_spectral):
    """A hole straight down through the voxel centres of an inner column, one point per voxel.  In the convention of
    Acquisition.path_voxels the polar angle is 180 - dip degrees, so the vertical hole is dip = 0 (dip = 90 runs along the surface)."""
    inv, _ = cube16_spectral
    s = inv.settings
    iy, ix = 6, 9
    x0, y0 = (ix + 0.5) * s.xvoxsize, (iy + 0.5) * s.yvoxsize
    path = inv.predict_path(x0, y0, 0.0, 0.0, step=s.zvoxsize)
    n = s.zNcube
    assert path["points"].shape == (n, 3) and path["mean"].shape == path["std"].shape == (3, n) and path["range"].shape == (n,)
    centres = inv.voxelpos.reshape(3, s.yNcube, s.xNcube, s.zNcube)[:, iy, ix, :].T
    assert np.abs(path["points"] - centres).max() <= 1e-9
    want = inv.hole_statistics()["path_std"][iy, ix]
    got = path["path_mean_std"][2] * n
    print("vertical path: path_mean_std * n = %.12e, hole_statistics path_std = %.12e (rel %.2e)" % (got, want, abs(got / want - 1)))
    assert abs(got / want - 1) <= 1e-8
    pointwise = inv.predict_points(path["points"])
    assert np.allclose(path["mean"], pointwise["mean"], rtol=1e-13, atol=0) and np.allclose(path["std"], pointwise["std"], rtol=1e-13, atol=0, equal_nan=True)
    assert np.allclose(path["path_mean"], pointwise["mean"].mean(axis=1), rtol=1e-13, atol=0)
    # a dipping hole that leaves through the face x = xLcube is cut there and still returns
    dipping = inv.predict_path(s.xLcube - 2.5 * s.xvoxsize, y0, 0.0, 40.0)
    m = dipping["points"].shape[0]
    assert 0 < m < int(2 * s.zLcube / s.zvoxsize) and dipping["mean"].shape == (3, m) and dipping["range"].shape == (m,)
    assert (dipping["points"][:, 0] <= s.xLcube).all() and np.isfinite(dipping["mean"]).all() and np.isfinite(dipping["path_mean_std"]).all()
    assert np.allclose(np.diff(dipping["range"]), 0.5 * s.zvoxsize)


# ---- 5. workflow ---------------------------------------------------------------------------------------------------------------------
def test_yaml_keys_write_the_prediction_tables(tmp_path):
    """YAML keys predict_points / predict_path on the reference's first example (25 x 16 x 16, non-cubic voxels, sparse kernel)."""
    import json
    import os

    import pandas as pd
    import yaml
    from conftest import GOLDEN
    from geobo_amd import run_geobo
    f = load_golden("example1.npz")
    d = json.loads(str(f["settings_json"]))
    rng = np.random.default_rng(9)
    centres = np.array([[61.0, 61.0, -25.0], [61.0 + 122.0 * 24, 61.0 + 122.0 * 15, -775.0], [61.0 + 122.0 * 7, 61.0 + 122.0 * 3, -125.0]])
    pts = np.vstack([centres, rng.uniform(0.0, 1.0, (20, 3)) * np.array([3050.0, 1952.0, -800.0])])
    csv = tmp_path / "targets.csv"
    pd.DataFrame(dict(ID=np.arange(len(pts)), X=pts[:, 0], Y=pts[:, 1], Z=pts[:, 2])).to_csv(csv, index=False)
    d.update(inpath=os.path.join(GOLDEN, "data", "synthetic") + "/", outpath=str(tmp_path) + "/", predict_points=str(csv),
             predict_path=[1500.0, 900.0, 30.0, 25.0])
    y = tmp_path / "settings.yaml"
    y.write_text(yaml.safe_dump(d))
    out = run_geobo.run(str(y), bayesopt=False)
    tab = pd.read_csv(tmp_path / "points_prediction.csv")
    names = ("DENSITY", "MAGSUS", "DRILL")
    assert list(tab.columns) == ["X", "Y", "Z"] + ["MEAN_" + n for n in names] + ["STD_" + n for n in names] and len(tab) == len(pts)
    assert np.allclose(tab[["X", "Y", "Z"]].to_numpy(), pts, rtol=1e-15, atol=0)
    got = out["points_prediction"]
    for a, n in enumerate(names):
        assert np.allclose(tab["MEAN_" + n], got["mean"][a], rtol=1e-12, atol=0) and np.allclose(tab["STD_" + n], got["std"][a], rtol=1e-12, atol=0)
    # the three voxel centres: voxels (iy, ix, iz) = (0, 0, 0), (15, 24, 15), (3, 7, 2) of the cubes this run wrote
    cubes = [out[k] for k in ("cube_density", "cube_magsus", "cube_drill", "cube_density_variance", "cube_magsus_variance", "cube_drill_variance")]
    for a in range(3):
        for k, (iy, ix, iz) in enumerate(((0, 0, 0), (15, 24, 15), (3, 7, 2))):
            assert abs(got["mean"][a, k] - cubes[a][iy, ix, iz]) <= 1e-8 * np.abs(cubes[a]).max()
            assert abs(got["var"][a, k] - cubes[3 + a][iy, ix, iz]) <= 1e-8 * np.abs(cubes[3 + a]).max()
    path = pd.read_csv(tmp_path / "path_prediction.csv")
    assert len(path) == out["path_prediction"]["points"].shape[0] > 0 and np.isfinite(path["MEAN_DRILL"]).all()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------
def test_errors(cube16_spectral, monkeypatch):
    inv, _ = cube16_spectral
    s = inv.settings
    fresh = _inv(s)
    with pytest.raises(RuntimeError, match="cubing"):
        fresh.predict_points(np.array([[100.0, 100.0, -100.0]]))
    with pytest.raises(ValueError, match="point 1 "):
        inv.predict_points(np.array([[100.0, 100.0, -100.0], [100.0, s.yLcube + 1e-9, -100.0]]))
    with pytest.raises(ValueError):
        inv.predict_points(np.zeros((0, 3)))
    eng = inv.engine
    q = tuple(c[:5].clone() for c in eng.grid_points())
    args = (q, s.kernelfunc, [200.0, 204.0, 208.0], inv.coeffm, 1.0)
    with pytest.raises(MemoryError, match="bytes"):
        eng.predict_points(*args, full_cov=True, limit_bytes=1 << 10)
    monkeypatch.setattr(eng, "world", 2)
    with pytest.raises(NotImplementedError, match="one rank"):
        eng.predict_points(*args)
    monkeypatch.setattr(eng, "world", 1)
    monkeypatch.setattr(eng, "f32", True)
    with pytest.raises(NotImplementedError, match="fp64 assembly"):
        eng.predict_points(*args)
    monkeypatch.setattr(eng, "f32", False)
    monkeypatch.setattr(eng, "last", None)
    with pytest.raises(RuntimeError, match="posterior"):
        eng.predict_points(*args)
