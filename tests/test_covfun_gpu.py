"""Covariances, length derivatives, exp_decay and the potentials by value against the multiprecision reference.  GPU only.

Four elementwise entry points (k_eval, cov_table, the generator inside ak_fused / ak_fused_grid, potential) at a few hundred
points each, compared with tests/_covfun_mp.py in units of its conditioned envelope: ulps(kernel) <= 4 K_ORACLE + 4, where
K_ORACLE is what the float64 oracle itself reaches (tests/test_covfun_cpu.py).  Every case prints its measured maximum (-s).

Measured on the MI355X (largest value over the six length pairs, in envelope units; the bound 4 K + 4 in brackets):
    exp        1.592 (12)   exp_x        2.362 (16)   matern32      2.207 (16)   matern32_x      1.995 (12)
    sparse     2.002 (16)   sparse_x     1.238 (12)
    exp_dl     3.521 (14)   exp_x_dl1    2.075 (14)   exp_x_dl2     1.605 (10)
    matern32_dl 4.828 (24)  matern32_x_dl1 1.997 (12) matern32_x_dl2 1.826 (8)
    sparse_dl  0.805 (6)    sparse_x_dl1 2.002 (6)    sparse_x_dl2  1.783 (6)
    grav       1.548 (12)   magn         1.232 (12)
    exp_decay  0.670 ulp at x = -696.2479... (claim 1.5); 0.680 units of 2^-1074 at x = -708.7429... (bound 2)
cov_table, ak_fused and ak_fused_grid: bit-equal to k_eval / k_block / the table for every id and family.

The fused generator is compared bit for bit: with A = the identity the MFMA contraction is 1 k + 0 ... in every association.
ak_fused_grid takes no lattice with nz < 16 (one carry per 16-deep chunk) or odd nz, so its 256 points are a 4 x 4 x 16 lattice;
the 8 x 8 x 4 lattice of the coordinate generator is asserted to be refused.
"""
import math

import numpy as np
import pytest
import torch

pytest.importorskip("mpmath")
import _covfun_mp as M  # noqa: E402

pytestmark = pytest.mark.gpu

VOX = (100.0, 120.0, 50.0)


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


def _k_eval(hip, kid, d2, l1, l2, w=M.W, amp=M.AMP):
    return hip.k_eval(kid, hip.to_dev(np.array(d2)), l1, l2, w, amp).cpu().numpy()   # np.array: the cached tables are read-only


def _report(what, l1, l2, k, where, d2, bound):
    print("%-14s (%.7g, %.7g): %.3f envelope units at d = %.6g (bound %.1f)"
          % (what, l1, l2, k, math.sqrt(d2[where]) if where >= 0 else 0.0, bound))


# ---- a. the six families ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", M.LENGTH_PAIRS, ids=lambda p: "%.7g-%.7g" % p)
@pytest.mark.parametrize("kid", [1, 2, 3, 4, 5, 6], ids=lambda k: M.NAMES[k])
def test_k_eval_values(hip, kid, pair):
    l1, l2 = pair
    d2, ref, env, _ = M.table(kid, l1, l2)
    got = _k_eval(hip, kid, d2, l1, l2)
    if kid == 4 and l1 == l2:
        # inf * 0: the NaN / inf pattern of the reference formula, as the float64 oracle produces it
        from oracle import geobo_oracle as O
        with np.errstate(all="ignore"):
            want = M.SCALE * O.k_cross("matern32", d2, l1, l2)
        assert not np.isfinite(want).any()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        return
    k, where, tiny = M.max_ulps(got, kid, l1, l2)
    _report(M.NAMES[kid], l1, l2, k, where, d2, M.tol(kid))
    assert np.isfinite(got[tiny]).all() and (got[tiny] >= 0).all() and (got[tiny] <= M.TINY_MAX).all()
    assert k <= M.tol(kid)
    if kid == 6 and l1 == l2:
        assert np.array_equal(got, _k_eval(hip, kid, d2, l1, l2 + 1e-3 * l2))     # the offset l2 += 1e-3 l2, and nothing else


# ---- b. the nine length derivatives ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", M.LENGTH_PAIRS, ids=lambda p: "%.7g-%.7g" % p)
@pytest.mark.parametrize("kid", [7, 8, 9, 10, 11, 12, 13, 14, 15], ids=lambda k: M.NAMES[k])
def test_k_eval_derivatives(hip, kid, pair):
    l1, l2 = pair
    d2, ref, env, keep = M.table(kid, l1, l2)
    got = _k_eval(hip, kid, d2, l1, l2)
    if kid in (11, 12) and l1 == l2:
        assert not np.isfinite(got).any()                                          # c = inf: no finite derivative either
        return
    assert (~keep).sum() <= M.DROP_CAP * keep.size
    k, where, tiny = M.max_ulps(got, kid, l1, l2)
    _report(M.NAMES[kid], l1, l2, k, where, d2, M.tol(kid))
    assert np.isfinite(got[tiny]).all() and (np.abs(got[tiny]) <= M.TINY_MAX).all()
    assert k <= M.tol(kid)


# ---- c. exp_decay alone -------------------------------------------------------------------------------------------------------------
def test_exp_decay(hip):
    """k_eval(exp, d2 = -2 x, l = 1) is exp_decay(x) exactly: c[0] = 1 and -0.5 d2 is exact.  The bound of 1.5 ulp is the claim of
    the function's own comment in covfun.h; a denormal result may carry ldexp's second rounding on top (2 units of 2^-1074)."""
    x = M.exp_arguments()
    got = _k_eval(hip, 1, -2.0 * x, 1.0, 1.0, 1.0, 1.0)
    assert np.isfinite(got).all()
    worst = {"ulp": (0.0, 0.0), "denormal": (0.0, 0.0)}
    for xi, g in zip(x, got):
        err, unit = M.exp_error(xi, g)
        if err > worst[unit][0]:
            worst[unit] = (err, xi)
    print("exp_decay: %.3f ulp at x = %.17g (bound 1.5); %.3f units of 2^-1074 at x = %.17g (bound 2)"
          % (worst["ulp"] + worst["denormal"]))
    assert worst["ulp"][0] <= 1.5
    assert worst["denormal"][0] <= 2.0
    assert got[0] == 1.0 and x[0] == 0.0 and got[1] == 1.0 and x[1] == -2.0 ** -60
    assert (got[x <= -800.0] == 0.0).all() and (x <= -800.0).sum() == 4
    assert (np.diff(got) <= 0).all()                                               # x descends: exp_decay does not rise


# ---- d. the lattice table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid", range(1, 16), ids=lambda k: M.NAMES[k])
def test_cov_table_is_k_eval_on_the_difference_lattice(hip, kid):
    """Bit equality with k_eval at d2 = (dx^2 + dy^2) + dz^2: the multiprecision bound of k_eval carries over to the table."""
    nx, ny, nz = 6, 5, 4
    l1, l2 = M.LENGTH_PAIRS[1]
    tab = hip.cov_table(kid, nx, ny, nz, *VOX, l1, l2, M.W, M.AMP).cpu().numpy()
    assert tab.shape == (2 * nx * ny * nz,)
    d2 = np.empty_like(tab)
    for diy in range(ny):
        for dix in range(nx):
            for dz in range(-(nz - 1), nz + 1):                                    # dz = nz: the padding entry of each row
                az = min(abs(dz), nz - 1)
                dx, dy, dzz = (dix + 1) * VOX[0] - 1.0 * VOX[0], (diy + 1) * VOX[1] - 1.0 * VOX[1], (az + 1) * VOX[2] - 1.0 * VOX[2]
                d2[(diy * nx + dix) * 2 * nz + (dz + nz - 1)] = (dx * dx + dy * dy) + dzz * dzz
    want = _k_eval(hip, kid, d2, l1, l2)
    assert np.isfinite(want).all() and np.unique(want).size > 8
    assert np.array_equal(tab, want)


# ---- e. the generator inside the fused product ----------------------------------------------------------------------------------------
def _identity(hip, n):
    return torch.eye(n, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("kid", [1, 2, 3, 4, 5, 6], ids=lambda k: M.NAMES[k])
def test_fused_generator_returns_rows_of_k_block(hip, kid):
    from oracle import geobo_oracle as O
    P = O.grid_points((8, 8, 4), VOX)                                              # N = 256: no padding column
    l1, l2 = M.LENGTH_PAIRS[1] if kid % 2 == 0 else M.LENGTH_PAIRS[0]
    xyz = tuple(hip.to_dev(P[:, d]) for d in range(3))
    want = torch.empty((256, 256), dtype=torch.float64, device="cuda")
    hip.k_block(kid, xyz, xyz, l1, l2, M.W, M.AMP, want)
    got = torch.full((256, 256), float("nan"), dtype=torch.float64, device="cuda")
    hip.ak_fused(kid, _identity(hip, 256), xyz, 0, 256, l1, l2, M.W, M.AMP, got)
    assert torch.isfinite(want).all() and want.unique().numel() > 8
    assert torch.equal(got, want)


@pytest.mark.parametrize("kid", [1, 2, 3, 4, 5, 6], ids=lambda k: M.NAMES[k])
def test_fused_grid_generator_returns_entries_of_cov_table(hip, kid):
    nx, ny, nz = 4, 4, 16
    l1, l2 = M.LENGTH_PAIRS[1] if kid % 2 == 0 else M.LENGTH_PAIRS[0]
    tab = hip.cov_table(kid, nx, ny, nz, *VOX, l1, l2, M.W, M.AMP)
    got = torch.full((256, 256), float("nan"), dtype=torch.float64, device="cuda")
    hip.ak_fused_grid(_identity(hip, 256), nx, ny, nz, tab, 0, 256, got)
    p = np.arange(256)
    iz, ix, iy = p % nz, (p // nz) % nx, p // (nz * nx)
    idx = ((np.abs(iy[:, None] - iy[None, :]) * nx + np.abs(ix[:, None] - ix[None, :])) * 2 * nz
           + (iz[:, None] - iz[None, :] + nz - 1))                                 # row = contraction voxel, column = output voxel
    want = tab.cpu().numpy()[idx]
    assert np.isfinite(want).all() and np.unique(want).size > 8
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(RuntimeError):                                              # nz = 4: refused, not computed
        hip.ak_fused_grid(_identity(hip, 256), 8, 8, 4, hip.cov_table(kid, 8, 8, 4, *VOX, l1, l2, M.W, M.AMP), 0, 256, got)


# ---- f. the potentials ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("func", ["grav", "magn"])
def test_potentials(hip, func):
    from geobo_amd import sensormodel as sm
    x, y, z = (np.array(a) for a in M.potential_points())                          # copies: the cached points are read-only
    got = hip.potential(func, M.B_FIELD, hip.to_dev(x), hip.to_dev(y), hip.to_dev(z)).cpu().numpy()
    k, where = M.max_ulps_potential(got, func)
    print("%s potential: %.3f envelope units at (%.6g, %.6g, %.6g) (bound %.1f)" % (func, k, x[where], y[where], z[where], M.tol(func)))
    assert k <= M.tol(func)
    # sensormodel's wrappers launch the same kernel
    same = sm.grav_func(x, y, z) if func == "grav" else sm.magn_func(x, y, z, *M.B_FIELD)
    assert np.array_equal(same, got)
