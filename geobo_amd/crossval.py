"""Leave-one-out and leave-fold-out cross-validation of the fit: fold builders (host) and the mixin of
engine.PosteriorEngine that evaluates them from the factor of the last posterior() step.

With K_y = A3 K A3^T + D the matrix the step factorises, alpha = K_y^-1 y = L^-T u and, for a set B of data rows,
G_B = [K_y^-1]_BB = L^-1[:, B]^T L^-1[:, B]:

    y_B | y_-B  ~  N(y_B - G_B^-1 alpha_B, G_B^-1),    log p(y_B | y_-B) = -1/2 alpha_B^T G_B^-1 alpha_B + 1/2 log det G_B - |B|/2 log 2 pi

No refactorisation and no operator: geobo_kinv_diag gives alpha and the diagonal of K_y^-1 (all a single row needs) in one pass over
L^-1, folds of 2 .. 128 rows take their block G_B from geobo_set_gram over columns of L^-1 and are solved by geobo_set_loo.

Data rows are numbered in the order of the data vector [grav | magn | drill] (Mu = 2 Ms + Md rows).
"""
import math

import numpy as np
import torch

from . import hip

F64 = hip.F64
FOLD_K_MAX = 128
FOLD_SIZES = (16, 64, 128)          # padded fold sizes: one launch group each
GRAM_BYTES = 256 << 20              # bound of one batch's G


# ---- fold builders (host) -------------------------------------------------------------------------------------------------------
def loo_folds(Mu):
    """One fold per data row: the (Mu, 1) table of the rows."""
    return np.arange(int(Mu), dtype=np.int64)[:, None]


def _hole_runs(sel, nz, Ms):
    """Drill rows grouped by voxel column sel // nz (sel ascending: a hole is a contiguous run of drill rows)."""
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    if sel.size == 0:
        return []
    if np.any(np.diff(sel) <= 0):
        raise ValueError("sel must be strictly ascending")
    col = sel // int(nz)
    cuts = np.flatnonzero(np.diff(col)) + 1
    return [2 * int(Ms) + r for r in np.split(np.arange(sel.size, dtype=np.int64), cuts)]


def hole_folds(sel, nz, Ms):
    """Sensor rows as singletons, the drill rows of one voxel column (one hole) together."""
    return list(loo_folds(2 * int(Ms))) + _hole_runs(sel, nz, Ms)


def patch_folds(sensor_xy, cell, Ms, sel=None, nz=None):
    """The sensor rows of each data type binned by their coordinates into square cells of side `cell` (same units as sensor_xy,
    (Ms, 2+) array of x, y; the grid starts at the smallest x and y), gravity and magnetic rows alike; with `sel` the drill rows
    follow by hole.  Built from the coordinates, not the row index: it works off the lattice."""
    xy = np.asarray(sensor_xy, dtype=np.float64)
    Ms = int(Ms)
    if xy.ndim != 2 or xy.shape[0] != Ms or xy.shape[1] < 2:
        raise ValueError("sensor_xy must be (Ms, 2) or (Ms, 3)")
    if not cell > 0:
        raise ValueError("cell must be positive")
    b = np.floor((xy[:, :2] - xy[:, :2].min(axis=0)) / float(cell) + 1e-9).astype(np.int64)
    key = b[:, 1] * (b[:, 0].max() + 1) + b[:, 0]
    order = np.argsort(key, kind="stable")
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    bins = [np.sort(g) for g in np.split(order.astype(np.int64), cuts)]
    folds = [g + t * Ms for t in range(2) for g in bins]
    if sel is not None:
        folds += _hole_runs(sel, nz, Ms)
    return folds


def fold_table(folds, Mu=None):
    """(C, k) int64 table of the folds, padded with -1 (k = the largest fold).  folds: a list of index arrays, or a (C, k) table whose
    negative entries are padding.  ValueError for an empty fold, a duplicate inside a fold, a row in two folds (every row has one
    prediction: the folds are disjoint), an index outside [0, Mu) (Mu given) or, in a list, below 0, or more than 128 entries."""
    if isinstance(folds, np.ndarray) and folds.ndim == 2:
        if not np.issubdtype(folds.dtype, np.integer):
            raise ValueError("a fold table holds integer row indices")
        tab = np.where(folds < 0, -1, folds).astype(np.int64)
        tab = np.take_along_axis(tab, np.argsort(tab < 0, axis=1, kind="stable"), axis=1)      # live entries first, in their order
        size = (tab >= 0).sum(axis=1)
        tab = tab[:, :max(int(size.max(initial=1)), 1)]
    else:
        folds = [f if isinstance(f, np.ndarray) and f.ndim == 1 else np.asarray(f).reshape(-1) for f in folds]
        size = np.array([f.size for f in folds], dtype=np.int64)
        flat = np.concatenate(folds) if folds else np.zeros(0, dtype=np.int64)
        if flat.size and not np.issubdtype(flat.dtype, np.integer):
            raise ValueError("folds hold integer row indices")
        if flat.size and flat.min() < 0:
            raise ValueError("fold %d names a row below 0" % int(np.repeat(np.arange(size.size), size)[np.argmin(flat)]))
        tab = np.full((size.size, max(int(size.max(initial=1)), 1)), -1, dtype=np.int64)
        tab[np.repeat(np.arange(size.size), size), np.arange(flat.size) - np.repeat(np.cumsum(size) - size, size)] = flat
    if size.size and size.min() == 0:
        raise ValueError("fold %d is empty" % int(np.argmin(size)))
    if tab.shape[1] > FOLD_K_MAX:
        raise ValueError("fold %d holds %d rows: at most %d" % (int(np.argmax(size)), int(size.max()), FOLD_K_MAX))
    if Mu is not None and tab.size and tab.max() >= Mu:
        raise ValueError("fold %d names a row outside [0, %d)" % (int(np.argmax(tab.max(axis=1))), Mu))
    srt = np.sort(tab, axis=1)
    dup = (srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)
    if dup.any():
        raise ValueError("fold %d names a row twice" % int(np.argmax(dup.any(axis=1))))
    live = tab >= 0
    rows, count = np.unique(tab[live], return_counts=True)
    if count.size and count.max() > 1:
        fold = np.repeat(np.arange(tab.shape[0]), live.sum(axis=1))
        shared = rows[np.argmax(count > 1)]
        raise ValueError("row %d is in folds %s: a row has one prediction, so the folds must be disjoint"
                         % (int(shared), fold[tab[live] == shared].tolist()))
    return tab


def without_rows(tab, rows):
    """The fold table `tab` with the data rows `rows` (dropped by the engine's row scales, reweight.py) left out of every fold: they
    become padding, live entries first; a fold that loses all its rows stays in the table with size 0 (NaN outputs).  No rows: tab."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0 or tab.size == 0:
        return tab
    tab = np.where(np.isin(tab, rows), -1, tab)
    return np.take_along_axis(tab, np.argsort(tab < 0, axis=1, kind="stable"), axis=1)


def padded_rows(idx, Ms, Ms_pad):
    """Data indices ([grav | magn | drill]) -> rows of the padded matrix (i, Ms_pad + i, 2 Ms_pad + i); padding stays negative."""
    idx = np.asarray(idx, dtype=np.int64)
    seg = np.minimum(idx // int(Ms), 2)
    return np.where(idx < 0, idx, idx + seg * (int(Ms_pad) - int(Ms)))


# ---- engine ---------------------------------------------------------------------------------------------------------------------
class CrossValidationMixin:
    def cross_validate(self, folds):
        """Leave-fold-out prediction of the data from the factor of the last posterior() step (any one-rank route, any props, both
        assemblies: the factor is fp64).  folds: list of arrays of data rows (order [grav | magn | drill], Mu = 2 Ms + Md rows), or a
        (C, k) table padded with negative entries; at most 128 rows per fold, the folds disjoint (fold_table), rows in no fold stay NaN.
        Returns a dict of device tensors in normalised units: per row `resid` (y - E[y | rows outside its fold]), `var`, `white`,
        `fold_of_row` (-1: in no fold); per fold `logp`, `mahalanobis`, `size`, `status`
        (0, or 1 + the pivot at which G_B failed: NaN in that fold); `alpha` = K_y^-1 y per data row."""
        if self.world > 1:
            raise NotImplementedError("cross-validation runs on one rank (world = %d)" % self.world)
        last = self.last
        if last is None:
            raise RuntimeError("cross_validate() needs the factor of a posterior() step")
        Ms, Msp, Md = self.Ms, self.Ms_pad, len(last["sel"])
        Mu = 2 * Ms + Md
        tab = without_rows(fold_table(folds, Mu), self.dropped_rows(last["sel"]))
        with torch.cuda.device(self.device):
            return self._cross_validate(tab, last["Linv"], last["u"], Ms, Msp, Mu)

    def _cross_validate(self, tab, Linv, u, Ms, Msp, Mu):
        dev = self.device
        M_pad = Linv.shape[0]
        C_ = tab.shape[0]
        d, alpha = self._timed("cv_diag", 2.0 * M_pad * M_pad, lambda: hip.kinv_diag(
            Linv, u, ws=self._workspace("cv_diag_ws", (hip.kinv_diag_ws_doubles(M_pad),))))
        rows_all = torch.as_tensor(padded_rows(np.arange(Mu), Ms, Msp), device=dev)
        nan = float("nan")
        resid, var, white = (torch.full((Mu,), nan, dtype=F64, device=dev) for _ in range(3))
        fold_of_row = torch.full((Mu,), -1, dtype=torch.int64, device=dev)
        logp, maha = (torch.full((C_,), nan, dtype=F64, device=dev) for _ in range(2))
        status = torch.zeros(C_, dtype=torch.int32, device=dev)
        size = (tab >= 0).sum(axis=1)
        # singletons: the diagonal alone
        one = np.flatnonzero(size == 1)
        if one.size:
            fi = torch.as_tensor(one, device=dev)
            ri = torch.as_tensor(tab[one, 0], device=dev)
            dd, aa = d[rows_all[ri]], alpha[rows_all[ri]]
            ok = (dd > 0) & torch.isfinite(dd)
            dd = torch.where(ok, dd, torch.full_like(dd, nan))
            w = aa / torch.sqrt(dd)
            resid[ri], var[ri], white[ri], fold_of_row[ri] = aa / dd, 1.0 / dd, w, fi
            maha[fi] = w * w
            logp[fi] = -0.5 * w * w + 0.5 * torch.log(dd) - 0.5 * math.log(2 * math.pi)
            status[fi] = (~ok).to(torch.int32)
        # larger folds by padded size and by the block of their lowest row (rows of L^-1 above it are zero in a fold's columns: a
        # launch of drill folds starts its sweep behind the sensor rows)
        prow = padded_rows(tab, Ms, Msp)
        low = np.where(prow >= 0, prow, M_pad).min(axis=1)
        for prev, kp in zip((1,) + FOLD_SIZES[:-1], FOLD_SIZES):
            for seg in range(3):
                pick = np.flatnonzero((size > prev) & (size <= kp) & (np.minimum(low // Msp, 2) == seg))
                step = max(1, GRAM_BYTES // (8 * kp * kp))
                for b0 in range(0, pick.size, step):
                    sub = pick[b0:b0 + step]
                    self._cv_batch(sub, tab[sub, :kp], prow[sub, :kp], int(low[sub].min()), Linv, alpha,
                                   (resid, var, white, fold_of_row, logp, maha, status))
        return dict(resid=resid, var=var, white=white, fold_of_row=fold_of_row, logp=logp, mahalanobis=maha,
                    size=torch.as_tensor(size, device=dev), status=status, alpha=alpha[rows_all])

    def _cv_batch(self, folds, rows, prow, low, Linv, alpha, outs):
        """One launch pair over the folds `folds` (ids): rows / prow their (c, kp) tables of data rows / rows of the padded matrix."""
        resid, var, white, fold_of_row, logp, maha, status = outs
        dev = self.device
        M_pad = Linv.shape[0]
        c, kp = rows.shape
        idx = torch.as_tensor(np.ascontiguousarray(prow, dtype=np.int32), device=dev)
        G = torch.empty((c, kp, kp), dtype=F64, device=dev)
        r0 = low // hip.PAD_M * hip.PAD_M
        self._timed("cv_gram", 2.0 * c * kp * kp * (M_pad - r0), lambda: hip.set_gram(idx, Linv[r0:], M_pad - r0, G, ncols=M_pad))
        out, rs, vr, wh, st = self._timed("cv_loo", c * kp ** 3, lambda: hip.set_loo(G, idx, alpha, M_pad))
        fi = torch.as_tensor(folds, device=dev)
        keep = torch.as_tensor(rows >= 0, device=dev)
        ri = torch.as_tensor(np.maximum(rows, 0), device=dev)[keep]
        resid[ri], var[ri], white[ri] = rs[keep], vr[keep], wh[keep]
        fold_of_row[ri] = fi[:, None].expand(c, kp)[keep]
        logp[fi], maha[fi], status[fi] = out[0], out[1], st
