"""Appending drill rows to a factorised K_y, host side: the NumPy reference of the bordered factor against
np.linalg.cholesky of the whole matrix, the C ABI of the two kernels, the row ranges of the V tile generators, and the argument
checks and the frozen normalisation of Inversion.assimilate_drill -- all of it before any device is touched."""
import os
import re

import numpy as np
import pytest

import _append_ref as R
from conftest import settings_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want):
    return np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize("m,ks", [(1, (1,)), (9, (1, 5)), (40, (64,)), (150, (100, 3)), (60, (128, 16))])
def test_reference_bordered_factor_equals_the_whole_cholesky(m, ks):
    rng = np.random.default_rng(100 * m + sum(ks))
    n = m + sum(ks)
    K, y = R.spd(n, rng), rng.standard_normal(n)
    L = np.linalg.cholesky(K[:m, :m])
    Linv = R.tri_inv(L)
    u = Linv @ y[:m]
    logdet, uu = 2.0 * np.log(np.diag(L)).sum(), float(u @ u)
    for k in ks:                                        # chained appends
        e = m + k
        L, Linv, u, dl, du = R.bordered_append(L, Linv, u, K[:m, m:e], K[m:e, m:e], y[m:e])
        logdet, uu, m = logdet + dl, uu + du, e
    Lw = np.linalg.cholesky(K)
    uw = np.linalg.solve(Lw, y)
    assert _close(L, Lw) and _close(Linv, np.linalg.inv(Lw)) and _close(u, uw)
    assert _close(np.array([logdet, uu]), np.array([np.linalg.slogdet(K)[1], uw @ uw]))
    assert np.array_equal(L, np.tril(L)) and np.array_equal(Linv, np.tril(Linv))


def test_reference_downdate_is_the_posterior_of_the_union():
    """mu + V_P^T u_P and var - colsum(V_P^2) are mean and variance diagonal of the larger system: V = L^-1 C for any C."""
    rng = np.random.default_rng(3)
    m, k, n = 30, 7, 11
    K, y, C = R.spd(m + k, rng), rng.standard_normal(m + k), rng.standard_normal((m + k, n))
    L = np.linalg.cholesky(K[:m, :m])
    Linv = R.tri_inv(L)
    u = Linv @ y[:m]
    V = Linv @ C[:m]
    L2, Li2, u2, _, _ = R.bordered_append(L, Linv, u, K[:m, m:], K[m:, m:], y[m:])
    VP = Li2[m:] @ C
    mu, var = R.rows_downdate(VP, u2[m:], V.T @ u, 1.0 - (V ** 2).sum(axis=0))
    Vw = np.linalg.solve(np.linalg.cholesky(K), C)
    assert _close(mu, Vw.T @ np.linalg.solve(np.linalg.cholesky(K), y)) and _close(var, 1.0 - (Vw ** 2).sum(axis=0))


def test_kernels_are_declared_bound_and_built():
    from geobo_amd import _lib, build
    head = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "geobo_hip.h")).read(), flags=re.S)
    assert "append.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "append.hip"))
    for name, nargs in (("geobo_factor_append", 14), ("geobo_rows_downdate", 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, head)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r"%s\s*\((.*?)\)\s*;" % name, head, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs


def test_tile_row_ranges():
    from geobo_amd.information import _tile_range, _tile_rows
    assert _tile_range(None, 517) == (0, 517) and _tile_range((517, 530), 530) == (517, 530)
    for bad in ((-1, 4), (5, 4), (0, 531)):
        with pytest.raises(ValueError):
            _tile_range(bad, 530)
    V = [np.arange(12.0).reshape(6, 2)]
    assert _tile_rows(V, 6, 0)[0] is V and _tile_rows(V, 6, -128) == (V, 6)
    cut, n = _tile_rows(V, 5, 2)
    assert n == 3 and np.array_equal(cut[0], V[0][2:])


def _surveyed(drill=(1.5, 2.5, 4.0, 0.5), dtype=np.float64):
    """An Inversion as cubing() leaves its host side (no engine is ever built: every check comes before the device)."""
    from geobo_amd.inversion import Inversion
    s = settings_for(nx=10, ny=8, nz=6)
    inv = Inversion(settings=s)
    inv.drillfield = np.asarray(drill, dtype=dtype)
    inv._sel = np.array([3, 40, 41, 200])[:len(drill)]
    inv.Fs3 = np.zeros(160 + len(drill))
    inv._cube_scale = (1.0, 1.0, float(inv.drillfield.std()) if len(drill) else np.nan)
    return inv


def test_assimilate_drill_argument_checks():
    from geobo_amd.inversion import Inversion
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=settings_for(nx=10, ny=8, nz=6)).assimilate_drill([5], [1.0])
    inv = _surveyed()
    for vox, vals, what in (([5, 6, 5], [1.0, 2.0, 3.0], "repeat"), ([5, 40], [1.0, 2.0], "already"), ([480], [1.0], r"\[0, 480\)"),
                            ([-1], [1.0], r"\[0, 480\)"), ([5, 6], [1.0], "1 values for 2 voxels"), ([], [], "at least one"),
                            ([[8, 0, 0]], [1.0], "inside"), ([[0, 10, 0]], [1.0], "inside"), ([[0, 0, 6]], [1.0], "inside"),
                            ([[0, 0, -1]], [1.0], "inside"), ([[0, 0, 3]], [1.0], "already"), ([5.5], [1.0], "integer"),
                            (np.zeros((2, 2), dtype=int), [1.0, 1.0], "flat")):
        with pytest.raises(ValueError, match=what):
            inv.assimilate_drill(vox, vals)
    assert inv._engine is None and inv.Fs3.size == 164 and inv._sel.size == 4       # nothing was touched
    with pytest.raises(ValueError, match="spread"):
        _surveyed(drill=(2.0, 2.0))._new_drill_rows([5], [1.0])
    with pytest.raises(ValueError, match="update"):
        inv.propose_drill_campaign(1, update="rebuild")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_new_values_take_the_survey_normalisation(dtype):
    inv = _surveyed(dtype=dtype)
    d = np.asarray(inv.drillfield, dtype=np.float64)
    vox, vals = inv._new_drill_rows([[1, 2, 3], [0, 0, 0]], [3.0, d.mean()])
    assert vox.tolist() == [(1 * 10 + 2) * 6 + 3, 0] and vox.dtype == np.int64
    assert np.array_equal(vals, (np.array([3.0, d.mean()]) - d.mean()) / d.std()) and vals[1] == 0.0
    # the statistics are those of cubing()'s drillfield alone: not of the union, not of the values handed in
    assert not np.isclose(vals[0], (3.0 - np.append(d, 3.0).mean()) / np.append(d, 3.0).std())
    vox2, raw = inv._new_drill_rows(np.array([7, 9]), [0.25, -1.0], normalised=True)
    assert vox2.tolist() == [7, 9] and np.array_equal(raw, [0.25, -1.0])
    # the survey's own values come back as cubing() normalised them
    from geobo_amd.inversion import _zscore
    again = inv._new_drill_rows(np.array([7, 9, 11, 13])[:d.size], d)[1]
    assert np.allclose(again, _zscore(d)[0], rtol=1e-15, atol=1e-15)
