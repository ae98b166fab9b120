"""References of the cross-validation tests.

brute_force  deletes the rows and columns of the fold, factorises the rest with SciPy and conditions on it: nothing of the identity
             the package uses.
identity     the G_B = [K_y^-1]_BB route of the package in plain fp64 NumPy: its deviation from brute_force on a matrix is the error
             level e_np that the device is measured against.
*_ld         Cholesky and triangular solves in np.longdouble, for the kernel tests.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, cholesky, solve_triangular

LOG2PI = float(np.log(2.0 * np.pi))


def _gauss_logpdf(r, cov):
    """log N(r; 0, cov) through SciPy's Cholesky."""
    L = cholesky(cov, lower=True)
    w = solve_triangular(L, r, lower=True)
    return float(-0.5 * w @ w - np.log(np.diag(L)).sum() - 0.5 * r.size * LOG2PI)


def brute_force(K_y, y, B):
    """y_B | y_-B by deleting the rows and columns of B: (mean, covariance, log density of y_B)."""
    B = np.asarray(B, dtype=np.int64)
    R = np.setdiff1d(np.arange(K_y.shape[0]), B)
    cf = cho_factor(K_y[np.ix_(R, R)], lower=True)
    K_BR = K_y[np.ix_(B, R)]
    mean = K_BR @ cho_solve(cf, y[R])
    cov = K_y[np.ix_(B, B)] - K_BR @ cho_solve(cf, K_BR.T)
    cov = 0.5 * (cov + cov.T)
    return mean, cov, _gauss_logpdf(y[B] - mean, cov)


def identity_factor(K_y, y):
    """(L^-1, alpha = K_y^-1 y) in fp64, as the step leaves them."""
    L = cholesky(K_y, lower=True)
    Linv = solve_triangular(L, np.eye(K_y.shape[0]), lower=True)
    return Linv, Linv.T @ (Linv @ y)


def identity(K_y, y, B, factor=None):
    """The same three through G_B = L^-1[:, B]^T L^-1[:, B]: mean = y_B - G_B^-1 alpha_B, covariance = G_B^-1."""
    B = np.asarray(B, dtype=np.int64)
    Linv, alpha = identity_factor(K_y, y) if factor is None else factor
    G = Linv[:, B].T @ Linv[:, B]
    Lg = cholesky(G, lower=True)
    white = solve_triangular(Lg, alpha[B], lower=True)
    resid = solve_triangular(Lg, white, lower=True, trans="T")
    X = solve_triangular(Lg, np.eye(B.size), lower=True)
    logp = float(-0.5 * white @ white + np.log(np.diag(Lg)).sum() - 0.5 * B.size * LOG2PI)
    return y[B] - resid, X.T @ X, logp


def all_folds(fn, K_y, y, folds, **kw):
    """fn over every fold: (predicted, std) per row in fold order, concatenated, and logp per fold."""
    pred, std, logp = [], [], []
    for B in folds:
        m, c, lp = fn(K_y, y, B, **kw)
        pred.append(m)
        std.append(np.sqrt(np.diag(c)))
        logp.append(lp)
    return np.concatenate(pred), np.concatenate(std), np.array(logp)


# ---- long double ----------------------------------------------------------------------------------------------------------------
def cholesky_ld(A):
    """Lower Cholesky factor of A in np.longdouble (LinAlgError on a non-positive pivot)."""
    A = np.array(A, dtype=np.longdouble)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("pivot %d" % j)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_ld(L, b, trans=False):
    """L x = b (trans: L^T x = b) in np.longdouble; b a vector or a matrix of columns."""
    L = np.asarray(L, dtype=np.longdouble)
    x = np.array(b, dtype=np.longdouble)
    n = L.shape[0]
    if not trans:
        for i in range(n):
            x[i] = (x[i] - L[i, :i] @ x[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def loo_ld(G, a):
    """What geobo_set_loo computes for one fold, in np.longdouble: (logp, mahalanobis, resid, var, white)."""
    L = cholesky_ld(G)
    white = solve_lower_ld(L, a)
    resid = solve_lower_ld(L, white, trans=True)
    X = solve_lower_ld(L, np.eye(L.shape[0], dtype=np.longdouble))
    q = white @ white
    logp = -0.5 * q + np.log(np.diag(L)).sum() - 0.5 * L.shape[0] * np.log(np.longdouble(8) * np.arctan(np.longdouble(1)))
    return logp, q, resid, (X * X).sum(axis=0), white
