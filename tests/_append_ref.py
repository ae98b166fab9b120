"""NumPy reference of the bordered factor update: the arithmetic of geobo_factor_append, of the rows
append_drill_rows adds to L, L^-1 and u, and of geobo_rows_downdate.  No device, no package import."""
import numpy as np


def tri_inv(L):
    """Inverse of a lower triangular matrix by forward substitution, column by column."""
    n = L.shape[0]
    T = np.zeros_like(L)
    for j in range(n):
        T[j, j] = 1.0 / L[j, j]
        for i in range(j + 1, n):
            T[i, j] = -(L[i, j:i] @ T[j:i, j]) / L[i, i]
    return T


def factor_append(D, G, r):
    """S = D - G = Ls Ls^T, T = Ls^-1, uP = T r, sum log diag Ls."""
    Ls = np.linalg.cholesky(D - G)
    T = tri_inv(Ls)
    return Ls, T, T @ r, float(np.log(np.diag(Ls)).sum())


def bordered_append(L, Linv, u, B, D, yP):
    """The factor of [[K, B], [B^T, D]] from the factor L of K (Linv = L^-1, u = L^-1 y) and the new values yP:
    returns (L2, Linv2, u2, the increment of log det = 2 sum log diag Ls, the increment of u.u)."""
    m, k = B.shape
    W = Linv @ B
    Ls, T, uP, logsum = factor_append(D, W.T @ W, yP - W.T @ u)
    L2 = np.zeros((m + k, m + k))
    L2[:m, :m], L2[m:, :m], L2[m:, m:] = L, W.T, Ls
    Li2 = np.zeros((m + k, m + k))
    Li2[:m, :m], Li2[m:, :m], Li2[m:, m:] = Linv, -T @ W.T @ Linv, T
    return L2, Li2, np.concatenate([u, uP]), 2.0 * logsum, float(uP @ uP)


def rows_downdate(V, c, mu, var):
    """mu + V^T c, var - sum_r V[r]^2."""
    return mu + V.T @ c, var - (V ** 2).sum(axis=0)


def spd(n, rng):
    """A well-conditioned random symmetric positive definite matrix X X^T / n + I / 2."""
    X = rng.standard_normal((n, 3 * n))
    return X @ X.T / (3 * n) + 0.5 * np.eye(n)
