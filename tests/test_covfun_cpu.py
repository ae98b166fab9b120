"""Calibration of the multiprecision reference (tests/_covfun_mp.py) on the CPU: no GPU, no torch.

Measures K_ORACLE -- the error of the float64 NumPy oracle (or, for the derivative ids the oracle does not have, of the same
mpmath formula at 53 bits) in units of the conditioned envelope -- and holds it to the table the GPU tests take their bound
from; proves the reference's analytic derivatives against mp.diff; and shows that the reference alone keeps the sparse
derivatives' dropped points under the cap.  Run with -s to see the measured figures.
"""
import math
import time

import numpy as np
import pytest

pytest.importorskip("mpmath")
from mpmath import mp, mpf  # noqa: E402

import _covfun_mp as M  # noqa: E402
from oracle import geobo_oracle as O  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def started():
    """The moment the module's first test starts (not its import: collection happens long before in a run of the whole suite)."""
    return time.perf_counter()


def _oracle(kid, d2, l1, l2):
    name, cross = M.ORACLE_FAMILY[kid]
    with np.errstate(all="ignore"):
        return M.SCALE * (O.k_cross(name, d2, l1, l2) if cross else O.k_auto(name, d2, l1))


@pytest.mark.parametrize("kid", [1, 2, 3, 4, 5, 6])
def test_oracle_stays_inside_its_tabulated_envelope(kid):
    worst = []
    for l1, l2 in M.LENGTH_PAIRS:
        d2, ref, env, _ = M.table(kid, l1, l2)
        got = _oracle(kid, d2, l1, l2)
        if kid == 4 and l1 == l2:
            assert np.isnan(got).all() and all(mp.isnan(r) for r in ref)      # inf * 0 at every distance
            continue
        k, where, tiny = M.max_ulps(got, kid, l1, l2)
        assert np.isfinite(got[tiny]).all() and (got[tiny] >= 0).all() and (got[tiny] <= M.TINY_MAX).all()
        worst.append(k)
        print("K_oracle %-10s (%.7g, %.7g): %.3f at d = %.6g" % (M.NAMES[kid], l1, l2, k, math.sqrt(d2[where])))
    print("K_oracle %-10s: %.3f (table %.1f)" % (M.NAMES[kid], max(worst), M.K_ORACLE[kid]))
    assert max(worst) <= M.K_ORACLE[kid]


@pytest.mark.parametrize("kid", [7, 8, 9, 10, 11, 12, 13, 14, 15])
def test_derivative_formula_at_53_bits_stays_inside_its_tabulated_envelope(kid):
    worst = []
    for l1, l2 in M.LENGTH_PAIRS:
        if kid in (11, 12) and l1 == l2:
            continue                                                          # no finite value: c = inf
        d2, ref, env, keep = M.table(kid, l1, l2)
        with mp.workprec(53):
            got = [float(mpf(M.SCALE) * M.evaluate(kid, x, l1, l2)[0]) for x in d2]
        k, where, tiny = M.max_ulps(got, kid, l1, l2)
        worst.append(k)
        print("K_53 %-14s (%.7g, %.7g): %.3f at d = %.6g" % (M.NAMES[kid], l1, l2, k, math.sqrt(d2[where])))
    print("K_53 %-14s: %.3f (table %.1f)" % (M.NAMES[kid], max(worst), M.K_ORACLE[kid]))
    assert max(worst) <= M.K_ORACLE[kid]


@pytest.mark.parametrize("func", ["grav", "magn"])
def test_potential_oracle_stays_inside_its_tabulated_envelope(func):
    x, y, z = M.potential_points()
    assert x.size == 256 and (np.abs(x[128:192]) >= 1e6).all() and (np.abs(y[192:]) >= 1e6).all()
    assert (x[160:192] < 0).all() and (y[224:] < 0).all() and set(z) == {0.5, 50.0, 3e3}
    got = O.grav_potential(x, y, z) if func == "grav" else O.magn_potential(x, y, z, *M.B_FIELD)
    k, where = M.max_ulps_potential(got, func)
    ref, env = M.potential_table(func)
    rel = max(abs((mpf(float(g)) - r) / r) for g, r in zip(got, ref))
    print("K_oracle %s: %.3f at (%.6g, %.6g, %.6g); raw relative error %.2e; table %.1f"
          % (func, k, x[where], y[where], z[where], float(rel), M.K_ORACLE[func]))
    assert k <= M.K_ORACLE[func]


@pytest.mark.parametrize("kid", [7, 8, 9, 10, 11, 12])
def test_analytic_reference_derivatives_agree_with_mp_diff(kid):
    base = M.BASE[kid]
    worst = 0.0
    for l1, l2 in M.LENGTH_PAIRS:
        if base == 4 and l1 == l2:
            continue
        L1, L2 = mpf(l1), mpf(l2)
        for x in M.sq(M.distances(l1, l2)):
            ref = M.evaluate(kid, x, l1, l2)[0]
            if kid in (9, 12):
                num = mp.diff(lambda b: M.value_mp(base, x, L1, b), L2)
            else:
                num = mp.diff(lambda a: M.value_mp(base, x, a, L2), L1)
            if ref == 0:
                assert num == 0
                continue
            worst = max(worst, float(abs(num - ref) / abs(ref)))
    print("%s: mp.diff against the analytic reference, largest relative difference %.2e" % (M.NAMES[kid], worst))
    assert worst <= 1e-30


@pytest.mark.parametrize("kid", M.SPARSE_DERIVS)
def test_sparse_derivative_drops_stay_under_the_cap(kid):
    for l1, l2 in M.LENGTH_PAIRS:
        drop = M.dropped(kid, l1, l2)
        print("%s (%.7g, %.7g): %d of %d points dropped" % (M.NAMES[kid], l1, l2, drop.sum(), drop.size))
        assert drop.sum() <= M.DROP_CAP * drop.size
        assert not drop[0]                                                    # d = 0 is kept


def test_point_sets():
    for l1, l2 in M.LENGTH_PAIRS:
        d = M.distances(l1, l2)
        assert d[0] == 0.0 and d.size <= 512 and (np.diff(d) > 0).all()
        for b in M.branch_points(l1, l2):
            assert {b, np.nextafter(b, np.inf)} <= set(d)
    assert M.LENGTH_PAIRS[1] == (230.0, 234.6)
    x = M.exp_arguments()
    assert x[0] == 0.0 and x[1] == -2.0 ** -60 and x[-1] == -1e300 and (np.diff(x) < 0).all()
    assert ((x <= -708.0) & (x >= -745.2)).sum() >= 64


def test_exp_metric_on_the_ieee_exponential():
    """The metric of the exp_decay test, applied to libm's exp: within 1 ulp where the result is normal, within one unit of
    2^-1074 where it is denormal."""
    for x in M.exp_arguments():
        err, unit = M.exp_error(x, math.exp(x))
        assert err <= 1.0, (x, err, unit)


def test_module_run_time(started):
    """The tables are cached (functools.lru_cache keyed by (id, l1, l2)): everything above runs in under 30 s."""
    assert time.perf_counter() - started < 30.0
