"""Drill-hole information gain and greedy campaigns, host side: the index tables of vertical and dipping holes,
the utilities against Acquisition, and argument checks of the two C entry points before any device access."""
import numpy as np
import pytest

from conftest import settings_for


def test_vertical_sets_follow_futility_vertical():
    from geobo_amd.acquisition import Acquisition
    from geobo_amd.campaign import column_table, vertical_sets
    ny, nx, nz = 8, 10, 6
    sets, ij = vertical_sets(ny, nx, nz)
    assert sets.shape == ((ny - 2) * (nx - 2), nz) and ij.shape == (sets.shape[0], 2)
    s = settings_for(nx, ny, nz)
    rng = np.random.default_rng(3)
    mean, var = rng.standard_normal((ny, nx, nz)), rng.random((ny, nx, nz))
    acq = Acquisition(s, mean, var)
    flat_mean, flat_var = mean.reshape(-1), var.reshape(-1)
    for c in range(sets.shape[0]):
        i0, i1 = ij[c]
        assert np.array_equal(flat_mean[sets[c]], mean[i0, i1, :])
        want = -acq.futility_vertical([i0, i1])
        got = flat_mean[sets[c]].sum() + s.kappa * np.sqrt(flat_var[sets[c]].sum())
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    t = column_table(np.arange(sets.shape[0], dtype=float), ij, ny, nx)
    assert np.isnan(t[0]).all() and np.isnan(t[-1]).all() and np.isnan(t[:, 0]).all() and np.isnan(t[:, -1]).all()
    assert np.isfinite(t[1:-1, 1:-1]).all()


def test_utilities_match_column_utility():
    from geobo_amd.acquisition import Acquisition
    from geobo_amd.campaign import utility, vertical_sets
    ny, nx, nz = 7, 9, 5
    s = settings_for(nx, ny, nz, kappa=1.7, beta=0.3)
    rng = np.random.default_rng(5)
    mean, var, cost = rng.standard_normal((ny, nx, nz)), rng.random((ny, nx, nz)), rng.random((ny, nx, nz))
    acq = Acquisition(s, mean, var, costs=cost)
    _, ij = vertical_sets(ny, nx, nz)
    zs = lambda a: np.ascontiguousarray(a).sum(axis=2)[ij[:, 0], ij[:, 1]]
    u = utility("ucb", zs(mean), zs(cost), s.kappa, s.beta, sum_var=zs(var))
    assert np.array_equal(u, acq.column_utility()[ij[:, 0], ij[:, 1]])
    pv = 3.0 * zs(var)
    assert np.allclose(utility("ucb_path", zs(mean), zs(cost), s.kappa, s.beta, path_var=pv), zs(mean) + 1.7 * np.sqrt(pv) - 0.3 * zs(cost))
    ig = rng.random(ij.shape[0])
    assert np.allclose(utility("information", zs(mean), zs(cost), s.kappa, s.beta, info_gain=ig), ig - 0.3 * zs(cost))
    with pytest.raises(ValueError):
        utility("ei", zs(mean), zs(cost), 1.0, 0.0)


def test_path_sets_unique_padding_and_leaving():
    from geobo_amd.acquisition import Acquisition
    from geobo_amd.campaign import path_sets
    shape = (8, 10, 6)
    s = settings_for(10, 8, 6)
    acq = Acquisition(s, np.zeros(shape), np.zeros(shape))
    inside = acq.path_voxels(350.0, 420.0, 30.0, 20.0)
    leaving = acq.path_voxels(50.0, 50.0, 200.0, 30.0)
    sets, valid = path_sets([inside, leaving, ([1, 1, 2], [3, 3, 3], [0, 1, 1])], shape)
    assert valid.tolist() == [True, False, True]
    flat = np.ravel_multi_index(inside, shape)
    _, first = np.unique(flat, return_index=True)
    want = flat[np.sort(first)]
    assert np.array_equal(sets[0, :want.size], want) and (sets[0, want.size:] == -1).all()
    assert (sets[1] == -1).all()
    assert sets[2, :3].tolist() == [np.ravel_multi_index(v, shape) for v in ((1, 3, 0), (1, 3, 1), (2, 3, 1))]
    big = (np.arange(129) // 60, (np.arange(129) // 6) % 10, np.arange(129) % 6)
    with pytest.raises(ValueError, match="distinct voxels"):
        path_sets([big], shape)


def test_set_entry_points_validate_without_gpu():
    from geobo_amd import _lib
    L = _lib.load()
    assert L.geobo_version() == 213
    p = 16                                                 # (never dereferenced: every call below fails its checks first)
    assert L.geobo_set_gram(4, 16, None, 8, p, 64, 64, 0, p, None) == -1
    assert L.geobo_set_gram(4, 129, p, 8, p, 64, 64, 0, p, None) == -1
    assert L.geobo_set_gram(-1, 16, p, 8, p, 64, 64, 0, p, None) == -1
    assert L.geobo_set_gram(4, 16, p, 8, p, 32, 64, 0, p, None) == -1
    assert L.geobo_set_logdet(4, 16, None, p, 0, 0.01, p, None, 64, p, p, None) == -1
    assert L.geobo_set_logdet(4, 129, p, p, 0, 0.01, p, None, 64, p, p, None) == -1
    assert L.geobo_set_logdet(-2, 16, p, p, 0, 0.01, p, None, 64, p, p, None) == -1
    assert L.geobo_set_logdet(4, 16, p, p, 0, 0.0, p, None, 64, p, p, None) == -1
    assert L.geobo_set_logdet(4, 16, p, p, 100, 0.01, p, None, 64, p, p, None) == -1
    assert L.geobo_set_gram(0, 16, p, 8, p, 64, 64, 0, p, None) == 0     # nothing to do: no launch


def test_campaign_api_exists_and_checks_order():
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=settings_for(10, 8, 6))
    with pytest.raises(RuntimeError, match="cubing"):
        inv.hole_statistics()
    with pytest.raises(RuntimeError, match="cubing"):
        inv.propose_drill_campaign(2)
