"""NumPy reference of down-weighting or dropping rows of a factorised K_y: the arithmetic of
geobo_fold_factor and geobo_rows_reweight and the update of the posterior and of the likelihood statistics built on them.  No device,
no package import."""
import numpy as np

from _append_ref import spd, tri_inv  # noqa: F401  (spd: the well-conditioned random matrix of the append's tests)


def dinv_delta(scale, sigma2):
    """For rows with noise variances sigma2 and scales s in (1, inf]: dinv = 1 / Delta with Delta = (s^2 - 1) sigma2 (0 where s is
    inf), and sum over the finite rows of log Delta."""
    s = np.asarray(scale, dtype=np.float64)
    sigma2 = np.broadcast_to(np.asarray(sigma2, dtype=np.float64), s.shape)
    fin = np.isfinite(s)
    delta = np.where(fin, (np.where(fin, s, 2.0) ** 2 - 1.0) * sigma2, np.inf)
    dinv = np.where(fin, 1.0 / delta, 0.0)
    return dinv, float(np.log(delta[fin]).sum())


def fold_factor(G, dinv, a):
    """S = G + diag(dinv) = C C^T;  returns (Cinv = C^-1, g = C^-1 a, stats = (2 sum log diag C, g^T g))."""
    C = np.linalg.cholesky(np.tril(G) + np.tril(G, -1).T + np.diag(dinv))
    Cinv = tri_inv(C)
    g = Cinv @ a
    return Cinv, g, np.array([2.0 * np.log(np.diag(C)).sum(), g @ g])


def rows_reweight(B, Cinv, g, mu=None, var=None):
    """T = Cinv B;  dmu = -T^T g, dvar = sum_r T[r]^2;  returns (mu + dmu, var + dvar, part = (sum dmu^2, max |dmu|, sum dvar));
    mu = var = None: (None, None, part)."""
    T = Cinv @ B
    dmu, dvar = -(T.T @ g), (T ** 2).sum(axis=0)
    part = np.array([(dmu ** 2).sum(), np.abs(dmu).max() if dmu.size else 0.0, dvar.sum()])
    if mu is None:
        return None, None, part
    return mu + dmu, var + dvar, part


def reweight(Linv, u, AK, D, dinv, logdelta, mu, var, uu, logdet):
    """The posterior of the system with Delta added on the rows D (dinv = 0: the row deleted), from L^-1, u = L^-1 y and A K of the
    whole system: returns (mu', var', uu', logdet', part)."""
    W = Linv[:, D]
    G, a = W.T @ W, W.T @ u
    Cinv, g, stats = fold_factor(G, dinv, a)
    B = (W.T @ Linv) @ AK
    mu2, var2, part = rows_reweight(B, Cinv, g, mu, var)
    return mu2, var2, uu - stats[1], logdet + stats[0] + logdelta, part


def direct(Ky, y, AK, kdiag, D, scale, sigma2):
    """The same by a direct solve of the edited matrix: rows with an infinite scale deleted, the others with (s^2 - 1) sigma2 added on
    the diagonal.  Returns (mu, var, uu, logdet)."""
    s = np.asarray(scale, dtype=np.float64)
    D = np.asarray(D)
    K2 = Ky.copy()
    fin = np.isfinite(s)
    K2[D[fin], D[fin]] += (s[fin] ** 2 - 1.0) * np.broadcast_to(sigma2, s.shape)[fin]
    keep = np.setdiff1d(np.arange(Ky.shape[0]), D[~fin])
    L = np.linalg.cholesky(K2[np.ix_(keep, keep)])
    V = np.linalg.solve(L, AK[keep])
    w = np.linalg.solve(L, y[keep])
    return V.T @ w, kdiag - (V ** 2).sum(axis=0), float(w @ w), float(2.0 * np.log(np.diag(L)).sum())
