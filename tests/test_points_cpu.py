"""Prediction at arbitrary points, the parts that need no device: the map from the cube's coordinates to the
covariance frame, the box check and the range ladder of a path, the argument validation of geobo_ak_points, and the construction
the GPU tests use as their reference (the oracle's dense posterior with the query points stacked under the grid points)."""
import ctypes

import numpy as np
import pytest

from conftest import normwise, settings_for
from oracle import geobo_oracle as O


def _inv(s):
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=s)
    inv.create_cubegeometry()
    return inv


def extended_posterior(P, Q, A_g, A_m, sel, y, lengths, W, name, gp_sigma, gp_amp=1.0):
    """oracle.posterior_dense with the query points Q (nq, 3) stacked under the grid points P (N, 3), P' = [P; Q], and nq zero columns
    appended to the operators: the query points are voxels that no sensor sees.  Entry a N' + N + i of the result is property a at
    query point i.  Returns (result, N')."""
    nq = Q.shape[0]
    wide = lambda A: np.hstack([A, np.zeros((A.shape[0], nq))])
    r = O.posterior_dense(np.vstack([P, Q]), wide(A_g), wide(A_m), sel, y, lengths, W, name, gp_sigma, gp_amp=gp_amp, return_cov=True)
    return r, P.shape[0] + nq


def query_index(N, N1, nq):
    """Indices of the 3 nq query entries [property][point] in the extended result."""
    return np.concatenate([a * N1 + N + np.arange(nq) for a in range(3)])


# ---- 1. frame ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ext,zmax", [((5, 4, 3), (550.0, 360.0, 150.0), 0.0), ((3, 7, 6), (90.0, 700.0, 1500.0), 40.0)])
def test_voxel_centres_map_onto_the_grid_points(dims, ext, zmax):
    nx, ny, nz = dims
    s = settings_for(nx, ny, nz, xmax=ext[0], ymax=ext[1], zLcube=ext[2], zmax=zmax)
    assert len({s.xvoxsize, s.yvoxsize, s.zvoxsize}) == 3
    inv = _inv(s)
    got = inv.to_covariance_frame(inv.voxelpos.T)
    want = O.grid_points((nx, ny, nz), (s.xvoxsize, s.yvoxsize, s.zvoxsize)).T
    assert got.shape == want.shape == (3, nx * ny * nz)
    assert np.abs(got / want - 1.0).max() <= 1e-12


# ---- 2. box and path -----------------------------------------------------------------------------------------------------------------
def _cubed(inv):
    """The attributes cubing() leaves, so that the argument checks in front of the engine can run without one."""
    inv.Fs3, inv._cube_scale = np.zeros(1), (1.0, 1.0, 1.0)
    return inv


def test_box_check():
    s = settings_for(5, 4, 3, xmax=550.0, ymax=360.0, zLcube=150.0, zmax=40.0)
    inv = _inv(s)
    with pytest.raises(RuntimeError, match="cubing"):
        inv.predict_points(np.zeros((1, 3)))
    with pytest.raises(RuntimeError, match="cubing"):
        inv.predict_path(100.0, 100.0, 0.0, 0.0)
    _cubed(inv)
    lo, hi = np.array([0.0, 0.0, 40.0 - 150.0]), np.array([550.0, 360.0, 40.0])
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    faces = np.array([[0.0, 100.0, 0.0], [550.0, 100.0, 0.0], [10.0, 0.0, -5.0], [10.0, 360.0, -5.0], [10.0, 10.0, 40.0], [10.0, 10.0, -110.0]])
    ok = inv._check_points(np.vstack([corners, faces, inv.voxelpos.T]))
    assert ok.shape == (14 + 60, 3) and ok.dtype == np.float64
    for axis in range(3):
        for side, sign in ((lo, -1.0), (hi, 1.0)):
            p = np.vstack([corners[:3], 0.5 * (lo + hi), 0.5 * (lo + hi)])
            p[3, axis] = side[axis] + sign * 1e-9
            p[4, axis] = side[axis] + sign * 1.0
            with pytest.raises(ValueError, match="point 3 "):            # the first offender is named
                inv.predict_points(p)
    bad = 0.5 * (lo + hi)[None, :].repeat(2, axis=0)
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="point 1 "):
        inv.predict_points(bad)
    for shape in ((0, 3), (3,), (4, 2), (2, 3, 1)):
        with pytest.raises(ValueError):
            inv.predict_points(np.zeros(shape))
    with pytest.raises(ValueError):
        inv.predict_points("somewhere")


def test_path_ladder():
    from geobo_amd.acquisition import Acquisition, spherical2cartes
    s = settings_for(8, 6, 5, xmax=800.0, ymax=660.0, zLcube=450.0)
    inv = _cubed(_inv(s))
    # default ladder: half the smallest voxel edge, length zLcube; a hole straight down (polar angle 180 - dip = 180 degrees) stays inside
    pts, rng = inv.path_points(250.0, 310.0, 35.0, 0.0)
    assert np.array_equal(rng, (np.arange(10) + 0.5) * 45.0) and pts.shape == (10, 3)
    x, y, z = spherical2cartes(250.0, 310.0, s.zmax, np.deg2rad(35.0), np.deg2rad(180.0), rng)
    assert np.array_equal(pts, np.stack([x, y, z], axis=1))
    assert np.abs(pts[:, 0] - 250.0).max() <= 1e-12 and np.abs(pts[:, 1] - 310.0).max() <= 1e-12
    assert np.allclose(pts[:, 2], -rng, rtol=1e-15, atol=0)
    # the convention of Acquisition.path_voxels: the same voxels
    acq = Acquisition(s, np.zeros((6, 8, 5)), np.zeros((6, 8, 5)))
    acq._ranges = rng
    ix, iy, iz = acq.path_voxels(250.0, 310.0, 35.0, 0.0)
    assert np.array_equal(ix, (pts[:, 0] / s.xvoxsize).astype(int)) and np.array_equal(iz, (-pts[:, 2] / s.zvoxsize).astype(int))
    # own step and length: ranges step/2, 3 step/2, ... <= length
    pts, rng = inv.path_points(250.0, 310.0, 0.0, 0.0, step=90.0, length=300.0)
    assert np.array_equal(rng, [45.0, 135.0, 225.0])
    # a dipping hole leaves through the face x = 800 and is cut there
    pts, rng = inv.path_points(700.0, 300.0, 0.0, 45.0, step=20.0, length=400.0)
    x, y, z = spherical2cartes(700.0, 300.0, s.zmax, 0.0, np.deg2rad(135.0), (np.arange(20) + 0.5) * 20.0)
    n = int(np.sum(x <= 800.0))
    assert 0 < n < 20 and pts.shape == (n, 3) and np.array_equal(pts, np.stack([x, y, z], axis=1)[:n]) and np.array_equal(rng, (np.arange(n) + 0.5) * 20.0)
    assert (pts[:, 0] <= 800.0).all() and x[n] > 800.0
    # collared outside: nothing inside
    pts, rng = inv.path_points(900.0, 300.0, 0.0, 0.0)
    assert pts.shape == (0, 3) and rng.shape == (0,)
    with pytest.raises(ValueError, match="no point inside"):
        inv.predict_path(900.0, 300.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        inv.path_points(250.0, 310.0, 0.0, 0.0, step=0.0)


# ---- 3. ABI --------------------------------------------------------------------------------------------------------------------------
def test_ak_points_validates_before_the_device():
    from geobo_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)

    def call(kid=1, A=p, R=128, N=256, lda=256, P=(p, p, p), Qp=(p, p, p), nq=128, out=p, ldo=128):
        return L.geobo_ak_points(kid, A, R, N, lda, P[0], P[1], P[2], Qp[0], Qp[1], Qp[2], nq, 1.0, 1.0, 1.0, 1.0, out, ldo, None)
    assert call(A=None, P=(None, None, None), Qp=(None, None, None), out=None) == -1
    assert call(A=None) == -1 and call(out=None) == -1
    for i in range(3):
        assert call(P=tuple(None if j == i else p for j in range(3))) == -1
        assert call(Qp=tuple(None if j == i else p for j in range(3))) == -1
    assert call(nq=100) == -2 and call(R=100) == -2
    assert call(N=250) == -2 and call(lda=257) == -2 and call(nq=0) == -2 and call(R=0) == -2


# ---- 4. the reference construction of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exp", "matern32", "sparse"])
def test_stacked_query_points_leave_the_grid_posterior_alone(name):
    nx, ny, nz = 10, 8, 6
    vox = (100.0, 110.0, 90.0)
    P = O.grid_points((nx, ny, nz), vox)
    N = P.shape[0]
    rng = np.random.default_rng(11)
    Ms = 24
    A_g, A_m = rng.standard_normal((Ms, N)), rng.standard_normal((Ms, N))
    sel = np.sort(rng.choice(N, 7, replace=False))
    y = rng.standard_normal(2 * Ms + sel.size)
    lengths = np.array([210.0, 236.0, 255.0])               # distinct: matern32's cross term is NaN at equal ones
    W = O.weight_matrix([0.3, 0.2, 0.4])
    sigma = np.array([0.1, 0.12, 0.08])
    plain = O.posterior_dense(P, A_g, A_m, sel, y, lengths, W, name, sigma, gp_amp=1.1, return_cov=True)
    on = np.concatenate([sel[:3], [0, N - 1, 137]])          # query points ON voxels (drilled ones among them) ...
    off = rng.uniform(0.5, 1.0, (9, 3)) * np.array([nx, ny, nz]) * np.array(vox)        # ... and off the grid
    Q = np.vstack([P[on], off])
    nq = Q.shape[0]
    ext, N1 = extended_posterior(P, Q, A_g, A_m, sel, y, lengths, W, name, sigma, gp_amp=1.1)
    grid = np.concatenate([a * N1 + np.arange(N) for a in range(3)])
    assert normwise(ext["mu"][grid], plain["mu"]) <= 1e-12
    assert normwise(ext["cov"][np.ix_(grid, grid)], plain["cov"]) <= 1e-12
    qi = query_index(N, N1, nq)
    k = len(on)
    at = np.concatenate([a * nq + np.arange(k) for a in range(3)])      # the on-voxel entries among the query entries
    vox_i = np.concatenate([a * N + on for a in range(3)])
    assert normwise(ext["mu"][qi][at], plain["mu"][vox_i]) <= 1e-12
    assert normwise(ext["cov"][np.ix_(qi, qi)][np.ix_(at, at)], plain["cov"][np.ix_(vox_i, vox_i)]) <= 1e-12
    assert normwise(ext["var"][qi][at], plain["var"][vox_i]) <= 1e-12
    assert np.isfinite(ext["mu"][qi]).all() and np.isfinite(ext["cov"][np.ix_(qi, qi)]).all()
