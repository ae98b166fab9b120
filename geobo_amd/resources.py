"""Grade-tonnage curves and exceedance probabilities from posterior realisations: host helpers and the mixin of
engine.PosteriorEngine.

A realisation f of the three property cubes and a cutoff c on property p select the set {v : f_p[v] >= c, f_q[v] >= lo_q, v in region}.
Its volume and the quantity sum_v f_p[v] it holds are non-linear in f: their law over the posterior comes from the realisations alone.
geobo_cutoff_stats reduces a device batch of realisations against C sorted cutoffs to one count and one sum per (realisation, cutoff)
and counts per voxel how often it passes; geobo_box_means first averages the realisations over the boxes of a block model (the support
of a selection block), whose voxel counts then weight the blocks.  Only the (n, C) tables and the C count cubes reach the host.

Units: the engine works in the GP's normalised units (cube / data std).  The host converts a cutoff c on (cube + offset) to
(c - offset) / scale_p and turns the tables back:  quantity = (scale_p * sum + offset * count) * voxel volume.
"""
import numpy as np
import torch

from . import hip

PROPS = ("density", "magsus", "drill")
CMAX = 32
QUANTILES = (0.1, 0.5, 0.9)


# ---- host helpers ---------------------------------------------------------------------------------------------------------------
def property_index(prop):
    """"density" | "magsus" | "drill" or 0 | 1 | 2 -> 0 | 1 | 2; ValueError otherwise."""
    if isinstance(prop, str):
        if prop in PROPS:
            return PROPS.index(prop)
    elif not isinstance(prop, bool) and isinstance(prop, (int, np.integer)) and 0 <= int(prop) <= 2:
        return int(prop)
    raise ValueError("a property is one of %r or 0, 1, 2, got %r" % (PROPS, prop))


def normalised_thresholds(cutoffs, offset, scale):
    """Cutoffs on (cube + offset) -> (t, order): t the ascending thresholds in normalised units, (c - offset) / float(scale), and
    order with t = converted[order], so that a table computed for t goes back to the caller's order as table[..., inverse(order)].
    ValueError for no cutoff, more than 32, or a NaN."""
    c = np.asarray(cutoffs, dtype=np.float64).reshape(-1)
    if c.size < 1 or c.size > CMAX:
        raise ValueError("between 1 and %d cutoffs, got %d" % (CMAX, c.size))
    if np.isnan(c).any():
        raise ValueError("a cutoff is NaN")
    t = (c - float(offset)) / float(scale)
    order = np.argsort(t, kind="stable")
    return t[order], order


def caller_order(table, order):
    """A table whose last axis follows the sorted thresholds -> the caller's cutoff order."""
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    return np.asarray(table)[..., inv]


def tonnage_tables(count, total, scale, offset, voxel_volume):
    """(n, C) counts (int64) and sums (normalised units) -> dict of count, volume = count * voxel volume, quantity = (scale * sum +
    offset * count) * voxel volume, grade = quantity / volume (NaN where nothing passes) and quantiles: the 10 / 50 / 90 % nanquantile
    over the realisations of volume, quantity and grade, (3, C) each."""
    count = np.asarray(count, dtype=np.int64)
    total = np.asarray(total, dtype=np.float64)
    vv = float(voxel_volume)
    volume = count * vv
    quantity = (float(scale) * total + float(offset) * count) * vv
    with np.errstate(all="ignore"):
        grade = np.where(count > 0, quantity / np.where(count > 0, volume, 1.0), np.nan)
    out = dict(count=count, volume=volume, quantity=quantity, grade=grade)

    def q3(a):
        res = np.full((3, a.shape[1]), np.nan)
        for j in range(a.shape[1]):
            col = a[:, j]
            if not np.isnan(col).all():
                res[:, j] = np.nanquantile(col, QUANTILES)
        return res
    out["quantiles"] = {k: q3(out[k]) for k in ("volume", "quantity", "grade")}
    return out


CSV_COLUMNS = ("CUTOFF",) + tuple("%s_%s" % (k, q) for k in ("VOLUME", "QUANTITY", "GRADE") for q in ("P10", "P50", "P90", "MEAN"))


def curve_frame(out):
    """One row per cutoff: CUTOFF, then P10 / P50 / P90 / MEAN of VOLUME, QUANTITY and GRADE (a pandas DataFrame)."""
    import pandas as pd
    cols = {"CUTOFF": np.asarray(out["cutoffs"], dtype=np.float64)}
    for k in ("volume", "quantity", "grade"):
        q = out["quantiles"][k]
        for i, name in enumerate(("P10", "P50", "P90")):
            cols["%s_%s" % (k.upper(), name)] = q[i]
        a = out[k]
        mean = np.full(a.shape[1], np.nan)
        for j in range(a.shape[1]):
            if not np.isnan(a[:, j]).all():
                mean[j] = np.nanmean(a[:, j])
        cols["%s_MEAN" % k.upper()] = mean
    return pd.DataFrame(cols)[list(CSV_COLUMNS)]


def exceedance_probability(mean, var, cutoffs, offset=0.0):
    """P(f + offset >= c) for independent normals f ~ N(mean, var): Phi((mean + offset - c) / sqrt(var)), shape (C,) + mean.shape;
    NaN where var is not positive."""
    from scipy.special import ndtr
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    c = np.asarray(cutoffs, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.where(var > 0, var, np.nan))
        z = (mean[None] + float(offset) - c.reshape((-1,) + (1,) * mean.ndim)) / sd[None]
        return ndtr(z)


# ---- engine ---------------------------------------------------------------------------------------------------------------------
class ResourceMixin:
    def cutoff_statistics(self, F, p, thresholds, lo=None, mask=None, box=None, hits=None):
        """Cutoff statistics of a device batch of realisations F (S, 3, N; normalised units, voxel order (iy, ix, iz)) for property p
        against the ascending `thresholds` (host, at most 32): device tensors (cnt (S, C) int64, sum (S, C) fp64) -- the number of
        voxels that pass each cutoff and the sum of their values -- and hits ((C, N) int32 device tensor or None) incremented per
        passing realisation.  lo: three lower bounds, -inf = none; mask: (N,) uint8 device tensor or None.
        box = (by, bx, bz): the statistics of the block means over that partition instead (geobo_box_means into a workspace, blocks
        weighted by their voxel counts); mask and hits are then per block, (nblocks,) and (C, nblocks)."""
        if self.world > 1:
            raise NotImplementedError("cutoff statistics run on one rank (world = %d)" % self.world)
        if not (isinstance(F, torch.Tensor) and F.dim() == 3 and F.shape[1] == 3 and F.shape[2] == self.N):
            raise ValueError("F must be a (S, 3, %d) device tensor" % self.N)
        with torch.cuda.device(self.device):
            S = F.shape[0]
            C_ = int(np.asarray(thresholds).size)
            weight = None
            if box is not None:
                from .blocksupport import block_counts, check_box
                grid = (self.ny, self.nx, self.nz)
                box = check_box(box, grid)
                nb = block_counts(grid, box)
                nblocks = nb[0] * nb[1] * nb[2]
                G = self._workspace("tonnage_means", (max(S, 1) * 3 * nblocks,))[:S * 3 * nblocks].view(S, 3, nblocks)
                weight = self._workspace("tonnage_count", (nblocks,), dtype=torch.int32)
                self._timed("box_means", 0.0, lambda: hip.box_means(F, grid, box, G=G, count=weight))
                F = G
            n = F.shape[2]
            ws = self._workspace("tonnage_ws", (hip.cutoff_stats_ws_doubles(S, n, C_),))
            return self._timed("cutoff_stats", 0.0, lambda: hip.cutoff_stats(F, p, thresholds, lo=lo, mask=mask, weight=weight, hits=hits, ws=ws))
