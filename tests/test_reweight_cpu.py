"""Down-weighting or dropping rows of a factorised K_y, host side: the NumPy reference of the fold update
against direct solves of the edited matrix, and the C ABI of the two kernels -- all of it before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import _reweight_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, tol=1e-12):
    return np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want)))


def _system(M, n, rng):
    Ky, y, AK = R.spd(M, rng), rng.standard_normal(M), rng.standard_normal((M, n))
    sigma2 = 0.05 + 0.1 * rng.random(M)              # (the reference needs only SOME positive noise variance per row)
    kdiag = 2.0 + rng.random(n)
    L = np.linalg.cholesky(Ky)
    Linv = R.tri_inv(L)
    u = Linv @ y
    V = Linv @ AK
    return dict(Ky=Ky, y=y, AK=AK, sigma2=sigma2, kdiag=kdiag, Linv=Linv, u=u, mu=V.T @ u, var=kdiag - (V ** 2).sum(axis=0),
                uu=float(u @ u), logdet=float(2.0 * np.log(np.diag(L)).sum()))


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("kind", ["drop", "finite", "mixed"])
def test_reference_equals_a_direct_solve_of_the_edited_matrix(k, kind):
    rng = np.random.default_rng(17 * k + len(kind))
    M, n = 40, 23
    s = _system(M, n, rng)
    D = np.sort(rng.choice(M, size=k, replace=False))
    scale = dict(drop=np.full(k, np.inf), finite=1.5 + 3.0 * rng.random(k),
                 mixed=np.where(np.arange(k) % 2 == 0, np.inf, 1.5 + 3.0 * rng.random(k)))[kind]
    dinv, logdelta = R.dinv_delta(scale, s["sigma2"][D])
    mu, var, uu, logdet, part = R.reweight(s["Linv"], s["u"], s["AK"], D, dinv, logdelta, s["mu"], s["var"], s["uu"], s["logdet"])
    mu_d, var_d, uu_d, logdet_d = R.direct(s["Ky"], s["y"], s["AK"], s["kdiag"], D, scale, s["sigma2"][D])
    assert _close(mu, mu_d) and _close(var, var_d)
    assert _close(np.array([uu, logdet]), np.array([uu_d, logdet_d]))
    assert _close(part, np.array([((mu_d - s["mu"]) ** 2).sum(), np.abs(mu_d - s["mu"]).max(), (var_d - s["var"]).sum()]), 1e-10)
    assert np.all(var >= s["var"] - 1e-14)           # less data never lowers a variance


def test_dropped_rows_logdet_is_the_logdet_of_the_kept_block():
    rng = np.random.default_rng(5)
    s = _system(40, 4, rng)
    D = np.array([0, 7, 39])
    W = s["Linv"][:, D]
    keep = np.setdiff1d(np.arange(40), D)
    want = np.linalg.slogdet(s["Ky"][np.ix_(keep, keep)])[1]
    assert abs(s["logdet"] + np.linalg.slogdet(W.T @ W)[1] - want) <= 1e-12 * abs(want)


def test_a_scale_below_one_is_indefinite():
    """S = P_DD + 1 / Delta with Delta < 0 beyond -1 / P_DD: no Cholesky factor (why scales < 1 are rejected)."""
    rng = np.random.default_rng(9)
    s = _system(40, 4, rng)
    D = np.array([3])
    W = s["Linv"][:, D]
    G = W.T @ W
    with pytest.raises(np.linalg.LinAlgError):
        R.fold_factor(G, np.array([-2.0 * G[0, 0]]), W.T @ s["u"])


def test_kernels_are_declared_bound_and_built():
    from geobo_amd import _lib, build
    head = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "geobo_hip.h")).read(), flags=re.S)
    assert "reweight.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "reweight.hip"))
    for name, nargs in (("geobo_fold_factor", 11), ("geobo_rows_reweight", 13), ("geobo_rows_reweight_ws_bytes", 1)):
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, head)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r"%s\s*\((.*?)\)\s*;" % name, head, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs


def test_argument_validation_without_gpu():
    """Both entry points validate before touching the device (nothing here is device memory)."""
    from geobo_amd import _lib
    L = _lib.load()
    d = 0x1000
    assert L.geobo_fold_factor(0, d, 8, d, d, d, 8, d, d, d, None) == -1
    assert L.geobo_fold_factor(129, d, 129, d, d, d, 129, d, d, d, None) == -1
    assert L.geobo_fold_factor(8, d, 7, d, d, d, 8, d, d, d, None) == -1
    assert L.geobo_fold_factor(8, d, 8, None, d, d, 8, d, d, d, None) == -1
    ws = L.geobo_rows_reweight_ws_bytes
    assert ws(1) == 24 and ws(256) == 24 and ws(257) == 48 and ws(4099) == 24 * 17 and ws(0) == 24
    big = 1 << 20
    assert L.geobo_rows_reweight(0, d, 64, 64, d, 8, d, d, d, d, d, big, None) == -1
    assert L.geobo_rows_reweight(129, d, 64, 64, d, 129, d, d, d, d, d, big, None) == -1
    assert L.geobo_rows_reweight(8, d, 63, 64, d, 8, d, d, d, d, d, big, None) == -1          # ldb < ncols
    assert L.geobo_rows_reweight(8, d, 64, 64, d, 7, d, d, d, d, d, big, None) == -1          # ldc < k
    assert L.geobo_rows_reweight(8, d, 64, 64, d, 8, d, d, None, d, d, big, None) == -1       # mu without var
    assert L.geobo_rows_reweight(8, d, 64, 64, d, 8, d, d, d, None, d, big, None) == -1       # no part
    assert L.geobo_rows_reweight(8, d, 512, 512, d, 8, d, d, d, d, d, 47, None) == -1         # ws too small
    assert L.geobo_rows_reweight(8, d, 64, 64, d, 8, d, d, d, d, d + 4, big, None) == -2      # ws misaligned
    assert isinstance(ctypes.c_size_t(ws(1 << 38)).value, int)
