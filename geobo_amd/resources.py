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
import collections

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


def inverse_order(order):
    """The inverse of the permutation `order`: sorted[inverse] is in the caller's order again."""
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    return inv


def caller_order(table, order):
    """A table whose last axis follows the sorted thresholds -> the caller's cutoff order."""
    return np.asarray(table)[..., inverse_order(order)]


def region_mask(region, shape):
    """A boolean cube of `shape` restricting the voxels (or blocks) -> its flat uint8 vector; None for None.  ValueError for another
    dtype or shape."""
    if region is None:
        return None
    region = np.asarray(region)
    if region.dtype != np.bool_ or region.shape != tuple(shape):
        raise ValueError("region must be a boolean array of shape %r, got %r %r" % (tuple(shape), region.dtype, region.shape))
    return np.ascontiguousarray(region.reshape(-1)).astype(np.uint8)


CutoffQuery = collections.namedtuple("CutoffQuery", "p cut t order inverse lo scale box shape mask n start")


def cutoff_query(prop, cutoffs, offset, require, cube_scale, has_drill, grid, block=None, region=None, n=1, start=0):
    """The set that grade_tonnage(), geobodies() and drill_intercepts() reduce realisations against, from their common arguments, on
    the host: {v : f_p[v] >= t[c], f_q[v] >= lo[q] for the other two properties, mask[v] != 0} in the engine's normalised units.
    cube_scale: the three data stds of cubing(); has_drill: the survey has drill data; grid = (yN, xN, zN); block = (bx, by, bz)
    voxels or None.  Returns a CutoffQuery: p, cut (the cutoffs as given, (C,)), t = the ascending thresholds, order with
    t = converted[order] and its inverse permutation, lo (3,), scale (three floats), box = (by, bx, bz) or None, shape = the grid or
    the block grid, mask = region as a flat uint8 vector or None, n, start.  ValueError as those methods document."""
    from . import blocksupport
    p = property_index(prop)
    scale = [float(v) for v in cube_scale]
    bounds = {property_index(k): float(v) for k, v in (require or {}).items()}
    if p in bounds:
        raise ValueError("require names the other properties: %r is the one the cutoffs apply to" % (prop,))
    if not has_drill and (p == 2 or 2 in bounds):
        raise ValueError("the drill cubes are NaN without drill data: no cutoff on them")
    lo = np.full(3, -np.inf)
    for q, v in bounds.items():
        if np.isnan(v):
            raise ValueError("a lower bound of require is NaN")
        lo[q] = v / scale[q]
    cut = np.asarray(cutoffs, dtype=np.float64).reshape(-1)
    t, order = normalised_thresholds(cut, offset, cube_scale[p])
    yN, xN, zN = grid
    box, shape = None, tuple(grid)
    if block is not None:
        bx, by, bz = blocksupport.check_box(block, (xN, yN, zN))
        box = (by, bx, bz)
        shape = blocksupport.block_counts(grid, box)
    n, start = int(n), int(start)
    if n < 1 or start < 0:
        raise ValueError("n >= 1 realisations from start >= 0, got n = %r, start = %r" % (n, start))
    return CutoffQuery(p, cut, t, order, inverse_order(order), lo, scale, box, shape, region_mask(region, shape), n, start)


def nanquantile(a):
    """The 10 / 50 / 90 % nanquantile of every column of a (n, C) table, (3, C); NaN for a column of NaNs."""
    a = np.asarray(a, dtype=np.float64)
    res = np.full((3, a.shape[1]), np.nan)
    for j in range(a.shape[1]):
        col = a[:, j]
        if not np.isnan(col).all():
            res[:, j] = np.nanquantile(col, QUANTILES)
    return res


def nanmean(a):
    """The nanmean of every column of a (n, C) table, (C,); NaN for a column of NaNs."""
    a = np.asarray(a, dtype=np.float64)
    res = np.full(a.shape[1], np.nan)
    for j in range(a.shape[1]):
        if not np.isnan(a[:, j]).all():
            res[j] = np.nanmean(a[:, j])
    return res


def tonnage(count, total, scale, offset, voxel_volume):
    """Counts (int64) and sums (normalised units) of one shape -> dict of count, volume = count * voxel volume, quantity = (scale *
    sum + offset * count) * voxel volume and grade = quantity / volume (NaN where nothing passes)."""
    vv = float(voxel_volume)
    volume = count * vv
    quantity = (float(scale) * total + float(offset) * count) * vv
    with np.errstate(all="ignore"):
        grade = np.where(count > 0, quantity / np.where(count > 0, volume, 1.0), np.nan)
    return dict(count=count, volume=volume, quantity=quantity, grade=grade)


def tonnage_tables(count, total, scale, offset, voxel_volume):
    """(n, C) counts (int64) and sums (normalised units) -> dict of count, volume = count * voxel volume, quantity = (scale * sum +
    offset * count) * voxel volume, grade = quantity / volume (NaN where nothing passes) and quantiles: the 10 / 50 / 90 % nanquantile
    over the realisations of volume, quantity and grade, (3, C) each."""
    out = tonnage(np.asarray(count, dtype=np.int64), np.asarray(total, dtype=np.float64), scale, offset, voxel_volume)
    out["quantiles"] = {k: nanquantile(out[k]) for k in ("volume", "quantity", "grade")}
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
        cols["%s_MEAN" % k.upper()] = nanmean(out[k])
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
def _check_batch(engine, F, noun):
    """What cutoff_statistics, body_statistics and trace_statistics ask of the engine and of a batch of realisations F."""
    if engine.world > 1:
        raise NotImplementedError("%s run on one rank (world = %d)" % (noun, engine.world))
    if not (isinstance(F, torch.Tensor) and F.dim() == 3 and F.shape[1] == 3 and F.shape[2] == engine.N):
        raise ValueError("F must be a (S, 3, %d) device tensor" % engine.N)


def _block_support(engine, F, box):
    """(F, box) -> (F, grid, weight): the batch itself on the voxel grid for box None, else its block means over the partition
    `box` = (by, bx, bz) (geobo_box_means into a workspace), the block grid and the blocks' voxel counts."""
    grid = (engine.ny, engine.nx, engine.nz)
    if box is None:
        return F, grid, None
    from .blocksupport import block_counts, check_box
    box = check_box(box, grid)
    nb = block_counts(grid, box)
    S, nblocks = F.shape[0], nb[0] * nb[1] * nb[2]
    G = engine._workspace("tonnage_means", (max(S, 1) * 3 * nblocks,))[:S * 3 * nblocks].view(S, 3, nblocks)
    weight = engine._workspace("tonnage_count", (nblocks,), dtype=torch.int32)
    engine._timed("box_means", 0.0, lambda: hip.box_means(F, grid, box, G=G, count=weight))
    return G, nb, weight


class ResourceMixin:
    def cutoff_statistics(self, F, p, thresholds, lo=None, mask=None, box=None, hits=None):
        """Cutoff statistics of a device batch of realisations F (S, 3, N; normalised units, voxel order (iy, ix, iz)) for property p
        against the ascending `thresholds` (host, at most 32): device tensors (cnt (S, C) int64, sum (S, C) fp64) -- the number of
        voxels that pass each cutoff and the sum of their values -- and hits ((C, N) int32 device tensor or None) incremented per
        passing realisation.  lo: three lower bounds, -inf = none; mask: (N,) uint8 device tensor or None.
        box = (by, bx, bz): the statistics of the block means over that partition instead (geobo_box_means into a workspace, blocks
        weighted by their voxel counts); mask and hits are then per block, (nblocks,) and (C, nblocks)."""
        _check_batch(self, F, "cutoff statistics")
        with torch.cuda.device(self.device):
            F, _, weight = _block_support(self, F, box)
            ws = self._workspace("tonnage_ws", (hip.cutoff_stats_ws_doubles(F.shape[0], F.shape[2], int(np.asarray(thresholds).size)),))
            return self._timed("cutoff_stats", 0.0, lambda: hip.cutoff_stats(F, p, thresholds, lo=lo, mask=mask, weight=weight, hits=hits, ws=ws))
