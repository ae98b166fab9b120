"""Cross-validation, host side: the fold builders, the NumPy identity against the brute force on the committed
matrices (which pins the reference of the GPU tests), the argument checks of the two C entry points before any device access, and
the order of the checks of Inversion.cross_validate."""
import numpy as np
import pytest

from conftest import load_golden, normwise, settings_for

import _crossval_ref as R

TINY = dict(nx=10, ny=8, nz=6)


def _lattice_xy(nx, ny, vox=100.0):
    """Sensor coordinates on the cube's x-y lattice, row-major in y (as the fixtures' surveys)."""
    x, y = np.meshgrid((np.arange(nx) + 0.5) * vox, (np.arange(ny) + 0.5) * vox)
    return np.stack([x.reshape(-1), y.reshape(-1)], axis=1)


# ---- 1. fold builders ------------------------------------------------------------------------------------------------------------
def test_loo_and_hole_folds():
    from geobo_amd.crossval import hole_folds, loo_folds
    assert [f.tolist() for f in loo_folds(4)] == [[0], [1], [2], [3]]
    nz, Ms = 6, 80
    # two whole z-columns (3 and 17), a run of three voxels in column 20, isolated voxels in columns 0, 20 (above the run), 41, 79
    sel = np.r_[2, 3 * nz + np.arange(nz), 17 * nz + np.arange(nz), 20 * nz + np.array([0, 2, 3, 4]), 41 * nz + 5, 79 * nz]
    assert np.all(np.diff(sel) > 0)
    folds = hole_folds(sel, nz, Ms)
    assert [f.tolist() for f in folds[:2 * Ms]] == [[i] for i in range(2 * Ms)]
    holes = [f - 2 * Ms for f in folds[2 * Ms:]]
    assert [h.tolist() for h in holes] == [[0], list(range(1, 7)), list(range(7, 13)), [13, 14, 15, 16], [17], [18]]
    assert np.array_equal(np.concatenate(folds), np.arange(2 * Ms + sel.size))
    assert [f.tolist() for f in hole_folds(np.array([], dtype=int), nz, 3)] == [[i] for i in range(6)]
    with pytest.raises(ValueError):
        hole_folds(np.array([5, 4]), nz, Ms)


@pytest.mark.parametrize("jitter", [0.0, 31.0])
def test_patch_folds_bin_by_coordinates(jitter):
    from geobo_amd.crossval import patch_folds
    nx, ny, nz = 10, 8, 6
    Ms = nx * ny
    xy = _lattice_xy(nx, ny)
    rng = np.random.default_rng(4)
    perm = rng.permutation(Ms)                                   # the row order carries no geometry
    xy = xy[perm] + jitter * (rng.random((Ms, 2)) - 0.5) + (0.0 if jitter == 0.0 else 40.0)
    sel = np.r_[3 * nz + np.arange(nz), 50 * nz + 1]
    folds = patch_folds(np.c_[xy, np.zeros(Ms)], 200.0, Ms, sel=sel, nz=nz)
    rows = np.concatenate(folds)
    assert np.array_equal(np.sort(rows), np.arange(2 * Ms + sel.size))      # every row in exactly one fold
    sensor = [f for f in folds if f.max() < 2 * Ms]
    grav = [f for f in sensor if f.max() < Ms]
    magn = [f - Ms for f in sensor if f.min() >= Ms]
    assert len(grav) + len(magn) == len(sensor)                             # no fold mixes the two types
    assert len(grav) == len(magn) and all(np.array_equal(a, b) for a, b in zip(grav, magn))
    cell = np.floor((xy - xy.min(axis=0)) / 200.0 + 1e-9).astype(int)
    for f in grav:
        assert len({tuple(c) for c in cell[f]}) == 1                        # one cell per fold ...
    assert len(grav) == len({tuple(c) for c in cell})                       # ... and one fold per cell
    if jitter == 0.0:
        assert len(grav) == (nx // 2) * (ny // 2) and all(f.size == 4 for f in grav)
        ix, iy = perm[grav[0]] % nx, perm[grav[0]] // nx
        assert sorted(zip(ix.tolist(), iy.tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [f.tolist() for f in folds[len(sensor):]] == [list(range(2 * Ms, 2 * Ms + nz)), [2 * Ms + nz]]
    assert len(patch_folds(xy, 200.0, Ms)) == len(sensor)                   # (Ms, 2) coordinates, no drill rows
    with pytest.raises(ValueError):
        patch_folds(xy[:-1], 200.0, Ms)


def test_fold_table_pads_and_rejects():
    from geobo_amd.crossval import fold_table
    tab = fold_table([[4], [0, 2, 1], [7, 3]], 8)
    assert tab.dtype == np.int64 and tab.tolist() == [[4, -1, -1], [0, 2, 1], [7, 3, -1]]
    assert fold_table([np.arange(128)], 200).shape == (1, 128)
    for bad in ([[1], []], [[1, 2, 1]], [[8]], [[-1, 2]], [np.arange(129)], [[1, 2], [3], [4, 2]], np.array([[1, 2], [2, -1]])):
        with pytest.raises(ValueError):
            fold_table(bad, 8 if len(bad[0]) < 100 else 200)


def test_padded_rows():
    from geobo_amd.crossval import padded_rows
    Ms, Msp = 80, 256
    idx = np.array([[0, 79, 80, 159], [160, 164, -1, -1]])
    assert padded_rows(idx, Ms, Msp).tolist() == [[0, 79, 256, 335], [512, 516, -1, -1]]
    assert np.array_equal(padded_rows(np.arange(165), Ms, Msp), np.r_[0:80, 256:336, 512:517])
    assert np.array_equal(padded_rows(np.arange(600), 256, 256), np.arange(600))


# ---- 2. the NumPy identity against the brute force -------------------------------------------------------------------------------
# deviation of the fp64 identity from the brute force on the committed AkA and Fs3 (residuals, variances, log density), measured
# on the CPU over "loo", "holes" and 2 x 2 sensor patches
E_NP = {"tiny_exp": (1.1e-13, 2.0e-12, 9.9e-13), "tiny_matern32": (2.9e-14, 1.3e-12, 6.4e-13), "tiny_sparse": (1.5e-14, 2.2e-13, 1.1e-13),
        "illcond_tiny_exp": (1.6e-11, 1.2e-9, 5.9e-10), "illcond_tiny_matern32": (3.3e-12, 2.6e-10, 5.8e-11)}


def tiny_fold_sets(f):
    from geobo_amd.crossval import hole_folds, loo_folds, patch_folds
    Ms, nz = TINY["nx"] * TINY["ny"], TINY["nz"]
    Mu = f["Fs3"].size
    return {"loo": loo_folds(Mu), "holes": hole_folds(f["sel"], nz, Ms),
            "patches": patch_folds(f["sensor_locations"], 200.0, Ms, sel=f["sel"], nz=nz),
            "mixed": [np.array([7, Ms + 31, 2 * Ms + 1, 2 * Ms + 3])]}


@pytest.mark.parametrize("name", sorted(E_NP))
def test_identity_matches_brute_force(name):
    f = load_golden(name + ".npz")
    K, y = f["AkA"], f["Fs3"]
    fac = R.identity_factor(K, y)
    for kind, folds in tiny_fold_sets(f).items():
        rows = np.concatenate(folds)
        pb, sb, lb = R.all_folds(R.brute_force, K, y, folds)
        pi, si, li = R.all_folds(R.identity, K, y, folds, factor=fac)
        errs = (normwise(y[rows] - pi, y[rows] - pb), normwise(si ** 2, sb ** 2), normwise(li, lb))
        print("%s %s: residuals %.1e variances %.1e log density %.1e" % (name, kind, *errs))
        assert all(e <= 16 * b for e, b in zip(errs, E_NP[name])), (kind, errs)


def test_long_double_reference_solves():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((9, 30))
    G, a = X @ X.T / 30 + 0.1 * np.eye(9), rng.standard_normal(9)
    logp, q, resid, var, white = R.loo_ld(G, a)
    Gi = np.linalg.inv(G)
    assert np.allclose(np.asarray(resid, dtype=float), Gi @ a, rtol=1e-12) and np.allclose(np.asarray(var, dtype=float), np.diag(Gi), rtol=1e-12)
    assert abs(float(q) - a @ Gi @ a) <= 1e-12 * float(q)
    assert abs(float(logp) - (-0.5 * a @ Gi @ a + 0.5 * np.linalg.slogdet(G)[1] - 4.5 * np.log(2 * np.pi))) <= 1e-12 * abs(float(logp))
    with pytest.raises(np.linalg.LinAlgError):
        R.cholesky_ld(G - 5.0 * np.eye(9))


# ---- 3. C ABI without a GPU ------------------------------------------------------------------------------------------------------
def test_crossval_entry_points_validate_without_gpu():
    from geobo_amd import _lib
    L = _lib.load()
    assert L.geobo_version() == 213
    p = 16                                                 # (never dereferenced: every call below fails its checks first)
    ws = lambda m: L.geobo_kinv_diag_ws_bytes(m)
    assert L.geobo_kinv_diag(256, None, 256, p, p, p, p, ws(256), None) == -1
    assert L.geobo_kinv_diag(256, p, 256, None, p, p, p, ws(256), None) == -1
    assert L.geobo_kinv_diag(256, p, 256, p, None, p, p, ws(256), None) == -1
    assert L.geobo_kinv_diag(256, p, 256, p, p, None, p, ws(256), None) == -1
    assert L.geobo_kinv_diag(256, p, 256, p, p, p, None, ws(256), None) == -1
    assert L.geobo_kinv_diag(300, p, 300, p, p, p, p, 1 << 30, None) == -1           # m % 256 != 0
    assert L.geobo_kinv_diag(0, p, 256, p, p, p, p, 1 << 30, None) == -1
    assert L.geobo_kinv_diag(512, p, 256, p, p, p, p, ws(512), None) == -1           # ldl < m
    assert L.geobo_kinv_diag(256, p, 257, p, p, p, p, ws(256), None) == -1           # odd ldl
    assert L.geobo_kinv_diag(256, 8, 256, p, p, p, p, ws(256), None) == -1           # Linv not 16-byte aligned
    assert L.geobo_kinv_diag(256, p, 256, p, p, p, p, ws(256) - 8, None) == -1       # workspace too small
    for m in (0, -256, 100, 257):
        assert ws(m) == 0
    # the header's formula: nb (nb + 1) slots of 2 x 256 doubles, nb = m / 256
    for m in (256, 8448):
        nb = m // 256
        assert ws(m) == nb * (nb + 1) * 2 * 256 * 8
    loo = lambda C, k, G=p, idx=p, alpha=p, n=64, out=p, resid=p, var=p, white=p, status=p: L.geobo_set_loo(
        C, k, G, idx, alpha, n, out, resid, var, white, status, None)
    for name in ("G", "idx", "alpha", "out", "resid", "var", "white", "status"):
        assert loo(4, 16, **{name: None}) == -1
    assert loo(4, 0) == -1 and loo(4, 129) == -1 and loo(-1, 16) == -1 and loo(4, 16, n=-1) == -1
    assert loo(0, 16) == 0                                 # nothing to do: no launch


# ---- 4. the public interface checks before it computes ---------------------------------------------------------------------------
def test_cross_validate_api_checks_order():
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=settings_for(10, 8, 6))
    with pytest.raises(RuntimeError, match="cubing"):
        inv.cross_validate()
    with pytest.raises(RuntimeError, match="cubing"):
        inv.cross_validate(folds="holes")
    with pytest.raises(ValueError, match="folds"):
        inv.cross_validate(folds="kfold")
    with pytest.raises(ValueError, match="folds"):
        inv.calc_cv([1.0, 2.0, 1.0, 0.2, 0.2], folds="kfold")
    from geobo_amd.engine import PosteriorEngine
    assert callable(PosteriorEngine.cross_validate)
