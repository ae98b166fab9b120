"""Drill-hole scoring by information gain and greedy drill campaigns.

Host side of the per-set posterior statistics of PosteriorEngine.set_statistics:
  * `vertical_sets` / `path_sets` turn holes into (C, k) voxel index tables (flat (iy, ix, iz) order, -1 = padding);
  * the three utilities of a hole, the reference's UCB score and two that see the correlation along the hole:
        "ucb"          sum mean + kappa sqrt(sum var)        - beta sum cost   (Acquisition.column_utility)
        "ucb_path"     sum mean + kappa sqrt(1^T Sigma_PP 1) - beta sum cost
        "information"  1/2 log det(I + Sigma_PP / sigma_d^2) - beta sum cost   (nats: the mutual information of log and field)
Inversion.hole_statistics and Inversion.propose_drill_campaign are the public entry points.
"""
import numpy as np

from .information import SET_K_MAX

UTILITIES = ("ucb", "ucb_path", "information")


def vertical_sets(ny, nx, nz):
    """Every inner vertical hole (cube axes 0 and 1 strictly inside the rim, as Acquisition.futility_vertical): (sets (C, nz) flat voxel
    indices of the z-column, ij (C, 2) its (axis-0, axis-1) indices), in row order of the (ny, nx) table."""
    i0, i1 = np.meshgrid(np.arange(1, ny - 1), np.arange(1, nx - 1), indexing="ij")
    ij = np.stack([i0.ravel(), i1.ravel()], axis=1).astype(np.int64)
    base = (ij[:, 0] * nx + ij[:, 1]) * nz
    return base[:, None] + np.arange(nz, dtype=np.int64)[None, :], ij


def path_sets(paths, shape):
    """Index tables of dipping holes: paths = [Acquisition.path_voxels(...) triplets of index arrays into the cube of `shape`]
    -> (sets (C, k) of the unique voxels of each path in path order, padded with -1; valid (C,) bool, False for a path that leaves the
    cube).  More than 128 unique voxels in one path raises ValueError."""
    shape = tuple(int(v) for v in shape)
    rows, valid = [], []
    for p in paths:
        a = [np.asarray(v, dtype=np.int64).reshape(-1) for v in p]
        inside = all(np.all((v >= 0) & (v < n)) for v, n in zip(a, shape))
        if not inside:
            rows.append(np.empty(0, dtype=np.int64))
            valid.append(False)
            continue
        flat = np.ravel_multi_index(tuple(a), shape)
        _, first = np.unique(flat, return_index=True)
        u = flat[np.sort(first)]
        if u.size > SET_K_MAX:
            raise ValueError("a path visits %d distinct voxels; at most %d per set" % (u.size, SET_K_MAX))
        rows.append(u)
        valid.append(True)
    k = max([1] + [r.size for r in rows])
    sets = np.full((len(rows), k), -1, dtype=np.int64)
    for c, r in enumerate(rows):
        sets[c, :r.size] = r
    return sets, np.asarray(valid, dtype=bool)


def utility(kind, mean_sum, cost_sum, kappa, beta, info_gain=None, path_var=None, sum_var=None):
    """Utility of holes from their sums (cubing() units for mean / variances) and statistics; see the module docstring."""
    if kind == "ucb":
        return mean_sum + kappa * np.sqrt(sum_var) - beta * cost_sum
    if kind == "ucb_path":
        return mean_sum + kappa * np.sqrt(path_var) - beta * cost_sum
    if kind == "information":
        return info_gain - beta * cost_sum
    raise ValueError("utility must be one of %s, got %r" % (UTILITIES, kind))


def column_table(values, ij, ny, nx):
    """(ny, nx) table with NaN on the rim from per-hole values in vertical_sets order."""
    t = np.full((ny, nx), np.nan)
    t[ij[:, 0], ij[:, 1]] = values
    return t
