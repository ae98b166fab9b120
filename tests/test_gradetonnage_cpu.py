"""Grade-tonnage curves without a GPU: the exported symbols and the argument checks of geobo_box_means and
geobo_cutoff_stats, the host logic between the (n, C) tables of the device and the returned curves, and exceedance_probability."""
import ctypes as C

import numpy as np
import pytest

from conftest import settings_for


def _dbl(*v):
    return (C.c_double * len(v))(*v)


# ---- 1. C ABI without a GPU ------------------------------------------------------------------------------------------------------
def test_symbols_and_signatures():
    from geobo_amd import _lib, build
    L = _lib.load()
    assert L.geobo_version() == 213
    assert "gradetonnage.hip" in build.SOURCES
    for name in ("geobo_box_means", "geobo_cutoff_stats", "geobo_cutoff_stats_ws_bytes"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["geobo_cutoff_stats"][1]) == 17 and len(_lib.SIGNATURES["geobo_box_means"][1]) == 13


def test_cutoff_stats_validates_without_gpu():
    from geobo_amd import _lib
    L = _lib.load()
    p = 16                                                     # (never dereferenced: every call below fails its checks first)
    n = 481
    wsb = L.geobo_cutoff_stats_ws_bytes
    inf = float("inf")

    def call(S=3, F=p, ss=3 * n, ps=n, n_=n, prop=1, t=(-inf, 0.0, 0.0, 1.5), lo=(-inf, -inf, -inf), mask=None, weight=None, cnt=p,
             tot=p, hits=None, ws=p, nbytes=None, Cn=None):
        Cn = (4 if t is None else len(t)) if Cn is None else Cn
        nbytes = wsb(3, n, 4) if nbytes is None else nbytes
        return L.geobo_cutoff_stats(S, F, ss, ps, n_, prop, Cn, None if t is None else _dbl(*t), None if lo is None else _dbl(*lo), mask,
                                    weight, cnt, tot, hits, ws, nbytes, None)
    for name in ("F", "t", "lo", "cnt", "tot", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(S=-1) == -1
    assert call(Cn=0) == -1
    assert call(t=tuple(float(i) for i in range(33)), nbytes=1 << 30) == -1      # C = 33
    assert call(t=(0.0, 1.0, 0.5, 2.0)) == -1                                     # unsorted
    assert call(t=(0.0, float("nan"), 1.0, 2.0)) == -1
    assert call(t=(float("nan"), 0.0, 1.0, 2.0)) == -1
    assert call(lo=(-inf, float("nan"), -inf)) == -1
    assert call(prop=-1) == -1 and call(prop=3) == -1
    assert call(n_=0) == -1
    assert call(ps=n - 1) == -1 and call(ss=3 * n - 1) == -1
    assert call(nbytes=wsb(3, n, 4) - 8) == -1 and call(nbytes=0) == -1
    assert call(ws=24) == -1                                                      # not 16-byte aligned
    # the workspace size: 0 for invalid arguments, a multiple of 16 otherwise
    assert wsb(-1, n, 4) == 0 and wsb(3, 0, 4) == 0 and wsb(3, n, 0) == 0 and wsb(3, n, 33) == 0
    for S in (0, 1, 3, 64, 100000):
        for n_ in (1, 27, 420, 481, 32768, 64 ** 3, 128 ** 3):
            for Cn in (1, 4, 16, 32):
                b = wsb(S, n_, Cn)
                assert b > 0 and b % 16 == 0, (S, n_, Cn, b)


def test_box_means_validates_without_gpu():
    from geobo_amd import _lib
    L = _lib.load()
    p = 16
    N = 5 * 6 * 7

    def call(S=2, F=p, ss=3 * N, ps=N, grid=(5, 6, 7), box=(2, 3, 4), G=p, count=p):
        return L.geobo_box_means(S, F, ss, ps, *grid, *box, G, count, None)
    for name in ("F", "G", "count"):
        assert call(**{name: None}) == -1, name
    assert call(S=-1) == -1
    for axis in range(3):
        zero = lambda t: tuple(0 if i == axis else v for i, v in enumerate(t))
        assert call(grid=zero((5, 6, 7)), box=(1, 1, 1)) == -1
        assert call(box=zero((2, 3, 4))) == -1
        assert call(box=tuple(g + 1 if i == axis else 1 for i, g in enumerate((5, 6, 7)))) == -1     # a box larger than the grid
    assert call(ps=N - 1) == -1 and call(ss=3 * N - 1) == -1
    assert call(grid=(2048, 2048, 2048), box=(1, 1, 1), ps=1 << 40, ss=1 << 42) == -1                # N > INT32_MAX


# ---- 2. host logic ---------------------------------------------------------------------------------------------------------------
def test_threshold_conversion_and_order():
    from geobo_amd import resources as R
    scale = np.float32(0.37)
    cut = np.array([2.5, -np.inf, 1.0, 2.5, 4.0])
    t, order = R.normalised_thresholds(cut, 1.25, scale)
    assert np.all(np.diff(t) >= 0) and t[0] == -np.inf
    assert np.array_equal(t, np.sort((cut - 1.25) / float(scale)))            # float(scale): the float32's exact value, in fp64
    assert np.array_equal(t, ((cut - 1.25) / float(scale))[order])
    table = np.arange(10.0).reshape(2, 5)                                      # columns follow the sorted thresholds
    back = R.caller_order(table, order)
    for j in range(5):
        assert np.array_equal(back[:, order[j]], table[:, j])
    for bad in ([], list(range(33)), [0.0, float("nan")]):
        with pytest.raises(ValueError):
            R.normalised_thresholds(bad, 0.0, 1.0)
    assert [R.property_index(v) for v in ("density", "magsus", "drill", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
    for bad in ("gold", 3, -1, True, 1.0, None):
        with pytest.raises(ValueError):
            R.property_index(bad)


def test_tables_quantiles_and_csv(tmp_path):
    from geobo_amd import resources as R
    rng = np.random.default_rng(5)
    n, Cn = 7, 3
    count = rng.integers(1, 50, size=(n, Cn)).astype(np.int64)
    count[:, 2] = 0                                                            # a cutoff nobody passes
    count[3, 1] = 0                                                            # and one realisation that misses another
    total = rng.standard_normal((n, Cn)) * count
    scale, offset, vv = float(np.float32(2.5)), 10.0, 100.0 * 50.0 * 25.0
    out = R.tonnage_tables(count, total, scale, offset, vv)
    assert out["count"].dtype == np.int64 and np.array_equal(out["count"], count)
    assert np.array_equal(out["volume"], count * vv)
    assert np.allclose(out["quantity"], (scale * total + offset * count) * vv, rtol=1e-15, atol=0)
    assert np.all(out["volume"][:, 2] == 0) and np.isnan(out["grade"][:, 2]).all() and np.isnan(out["grade"][3, 1])
    ok = count > 0
    assert np.allclose(out["grade"][ok], (scale * total[ok] / count[ok] + offset), rtol=1e-13)
    q = out["quantiles"]
    assert set(q) == {"volume", "quantity", "grade"} and all(v.shape == (3, Cn) for v in q.values())
    assert np.array_equal(q["volume"], np.quantile(out["volume"], [0.1, 0.5, 0.9], axis=0))
    assert np.array_equal(q["grade"][:, 1], np.nanquantile(out["grade"][:, 1], [0.1, 0.5, 0.9]))
    assert np.isnan(q["grade"][:, 2]).all() and np.all(q["volume"][:, 2] == 0)
    out["cutoffs"] = np.array([0.5, 1.5, 9.0])
    frame = R.curve_frame(out)
    assert list(frame.columns) == ["CUTOFF", "VOLUME_P10", "VOLUME_P50", "VOLUME_P90", "VOLUME_MEAN", "QUANTITY_P10", "QUANTITY_P50",
                                   "QUANTITY_P90", "QUANTITY_MEAN", "GRADE_P10", "GRADE_P50", "GRADE_P90", "GRADE_MEAN"]
    assert len(frame) == Cn and np.array_equal(frame["CUTOFF"], out["cutoffs"])
    assert np.allclose(frame["VOLUME_MEAN"], out["volume"].mean(0)) and np.isnan(frame["GRADE_MEAN"][2])
    assert np.isclose(frame["GRADE_MEAN"][1], np.nanmean(out["grade"][:, 1]))
    frame.to_csv(tmp_path / "grade_tonnage.csv", index=False)
    assert (tmp_path / "grade_tonnage.csv").read_text().splitlines()[0].split(",") == list(R.CSV_COLUMNS)


# ---- 3. exceedance_probability -------------------------------------------------------------------------------------------------
def test_exceedance_probability_against_scipy():
    from scipy.stats import norm

    from geobo_amd.inversion import Inversion
    from geobo_amd import resources as R
    rng = np.random.default_rng(11)
    s = settings_for(4, 3, 2)
    N = 24
    inv = Inversion(settings=s)
    mu = rng.standard_normal(3 * N)
    var = rng.uniform(0.05, 2.0, 3 * N)
    var[5], var[N + 7] = 0.0, -1e-12
    inv.mu_rec, inv.cov_rec = mu, np.diag(var)
    inv._cube_scale = (np.float32(1.7), np.float64(0.4), np.float64(3.0))
    cut = np.array([0.3, -1.0, 2.0])
    for p, name in enumerate(("density", "magsus", "drill")):
        sc = inv._cube_scale[p]
        got = inv.exceedance_probability(cut, name, offset=0.25)
        assert got.shape == (3, 3, 4, 2)
        m = (mu[p * N:(p + 1) * N] * sc).reshape(3, 4, 2)
        v = (var[p * N:(p + 1) * N] * sc ** 2).reshape(3, 4, 2)
        good = v > 0
        with np.errstate(all="ignore"):
            ref = np.stack([norm.sf(c, loc=m + 0.25, scale=np.sqrt(np.where(good, v, np.nan))) for c in cut])
        assert np.array_equal(np.isnan(got), np.broadcast_to(~good, got.shape))
        assert np.abs(got - ref)[:, good].max() <= 1e-15
    assert np.isnan(inv.exceedance_probability(cut, 0)[:, 0, 2, 1]).all() and np.isnan(inv.exceedance_probability(cut, 1)[:, 0, 3, 1]).all()
    assert np.array_equal(R.exceedance_probability(np.zeros(2), np.ones(2), [0.0]), np.full((1, 2), 0.5))
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=s).exceedance_probability(cut, 0)


def test_interface_is_there():
    from geobo_amd.engine import PosteriorEngine
    from geobo_amd.inversion import Inversion
    from geobo_amd.resources import ResourceMixin
    assert issubclass(PosteriorEngine, ResourceMixin) and callable(PosteriorEngine.cutoff_statistics)
    assert callable(Inversion.grade_tonnage) and callable(Inversion._posterior_batches)
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=settings_for(4, 3, 2)).grade_tonnage([0.0], prop="density")
