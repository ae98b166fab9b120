"""Connected ore bodies (geobodies) of posterior realisations: host helpers and the mixin of
engine.PosteriorEngine.

A realisation and a cutoff select the set of resources.py (grade_tonnage); its connected components under 6- or 26-connectivity are
the BODIES.  How many there are, how large the largest is, what hangs together with the known intersections (the SEEDED body: the
union of the bodies that hold a seed voxel) and how often a voxel belongs to either are non-local functionals of the field: their
law comes from the joint realisations alone.  geobo_bodies labels a device batch by union-find and reduces it to small tables; only
those and the hit cubes reach the host.  Units and the cutoff conversion are those of resources.py.
"""
import numpy as np
import torch

from . import hip
from .resources import _block_support, _check_batch, nanmean, nanquantile, tonnage

NEIGHBOURS = (6, 26)
PROBABILITY = (None, "largest", "seeded", "both")
WS_BYTES = 1 << 30                  # workspace bound of one geobo_bodies launch: the engine cuts (samples, cutoffs) to stay below
VOLUMES = 65535                     # volumes (samples x cutoffs) of one launch at most


# ---- host helpers ---------------------------------------------------------------------------------------------------------------
def check_neighbours(neighbours):
    if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or int(neighbours) not in NEIGHBOURS:
        raise ValueError("neighbours is 6 (faces) or 26 (faces, edges and corners), got %r" % (neighbours,))
    return int(neighbours)


def check_probability(probability):
    if probability not in PROBABILITY:
        raise ValueError("probability is one of %r, got %r" % (PROBABILITY, probability))
    return probability in ("largest", "both"), probability in ("seeded", "both")


def parse_seeds(seeds, grid, drill=None):
    """Seed voxels -> ascending unique flat indices (int32) in voxel order (iy, ix, iz) of `grid` = (ny, nx, nz).  seeds: None (no
    seed), "drill" (`drill`: the flat indices of the drilled voxels), a boolean cube of shape `grid`, or a (K, 3) integer array of
    (ix, iy, iz).  ValueError for anything else or an index outside the grid."""
    ny, nx, nz = (int(v) for v in grid)
    if seeds is None:
        idx = np.zeros(0, dtype=np.int64)
    elif isinstance(seeds, str):
        if seeds != "drill":
            raise ValueError("seeds is None, \"drill\", a boolean cube or a (K, 3) array of (ix, iy, iz), got %r" % (seeds,))
        if drill is None:
            raise ValueError("seeds = \"drill\" needs the drilled voxels of cubing()")
        idx = np.asarray(drill, dtype=np.int64).reshape(-1)
    else:
        a = np.asarray(seeds)
        if a.dtype == np.bool_:
            if a.shape != (ny, nx, nz):
                raise ValueError("a boolean seeds cube has the shape %r, got %r" % ((ny, nx, nz), a.shape))
            idx = np.flatnonzero(a.reshape(-1))
        elif a.ndim == 2 and a.shape[1] == 3 and np.issubdtype(a.dtype, np.integer):
            ix, iy, iz = (a[:, k].astype(np.int64) for k in range(3))
            if ((ix < 0) | (ix >= nx) | (iy < 0) | (iy >= ny) | (iz < 0) | (iz >= nz)).any():
                raise ValueError("a seed (ix, iy, iz) lies outside the %d x %d x %d grid" % (nx, ny, nz))
            idx = (iy * nx + ix) * nz + iz
        else:
            raise ValueError("seeds is None, \"drill\", a boolean cube or a (K, 3) integer array of (ix, iy, iz), got shape %r %s"
                             % (a.shape, a.dtype))
    if idx.size and (idx.min() < 0 or idx.max() >= ny * nx * nz):
        raise ValueError("a seed index lies outside the grid")
    return np.unique(idx).astype(np.int32)


def seeds_to_blocks(idx, grid, box):
    """Flat voxel indices -> the ascending unique flat indices (int32) of their blocks (boxes of `box` = (by, bx, bz) voxels)."""
    from .blocksupport import block_partition
    index = block_partition(grid, box)[0]
    return np.unique(index[np.asarray(idx, dtype=np.int64)]).astype(np.int32)


def renumber(labels):
    """Canonical labels (the smallest flat index of each voxel's body, -1 outside) -> (numbered, sizes): bodies numbered 1 .. B in
    ascending order of that index, 0 outside (the numbering of scipy.ndimage.label), and the voxels of each body, (B,) int64."""
    lab = np.asarray(labels)
    flat = lab.reshape(-1)
    roots, inverse, sizes = np.unique(flat[flat >= 0], return_inverse=True, return_counts=True)
    out = np.zeros(flat.shape, dtype=np.int32)
    out[flat >= 0] = inverse.reshape(-1) + 1
    return out.reshape(lab.shape), sizes.astype(np.int64)


def body_tables(stats, sums, scale, offset, voxel_volume):
    """(n, C, 6) int64 statistics and (n, C, 3) sums (normalised units) of geobo_bodies -> dict: `count` (the whole set), `n_bodies`,
    `largest` and `seeded` = dicts of count, volume = count x voxel volume, quantity = (scale x sum + offset x count) x voxel volume
    and grade = quantity / volume (NaN when empty), `largest["label"]`, `seeded["bodies"]`, and `quantiles`: the 10 / 50 / 90 %
    quantiles over the realisations of n_bodies, the largest volume and the seeded volume, (3, C) each."""
    stats = np.asarray(stats, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    out = dict(count=stats[..., 0].copy(), n_bodies=stats[..., 1].copy())
    out["largest"] = tonnage(stats[..., 2].copy(), sums[..., 1], scale, offset, voxel_volume)
    out["largest"]["label"] = stats[..., 3].copy()
    out["seeded"] = tonnage(stats[..., 4].copy(), sums[..., 2], scale, offset, voxel_volume)
    out["seeded"]["bodies"] = stats[..., 5].copy()
    out["quantiles"] = dict(n_bodies=nanquantile(out["n_bodies"]), largest_volume=nanquantile(out["largest"]["volume"]),
                            seeded_volume=nanquantile(out["seeded"]["volume"]))
    return out


CSV_COLUMNS = ("CUTOFF",) + tuple("%s_%s" % (k, q) for k in ("BODIES", "LARGEST_VOLUME", "SEEDED_VOLUME") for q in ("P10", "P50", "P90", "MEAN")) \
    + ("LARGEST_GRADE_MEAN", "SEEDED_GRADE_MEAN", "SEEDED_BODIES_MEAN")


def bodies_frame(out):
    """One row per cutoff: CUTOFF, P10 / P50 / P90 / MEAN of the number of bodies, the largest and the seeded volume, and the mean
    grades of both bodies and the mean number of seeded bodies (a pandas DataFrame)."""
    import pandas as pd
    cols = {"CUTOFF": np.asarray(out["cutoffs"], dtype=np.float64)}
    for name, key, table in (("BODIES", "n_bodies", out["n_bodies"]), ("LARGEST_VOLUME", "largest_volume", out["largest"]["volume"]),
                             ("SEEDED_VOLUME", "seeded_volume", out["seeded"]["volume"])):
        q = out["quantiles"][key]
        for i, qn in enumerate(("P10", "P50", "P90")):
            cols["%s_%s" % (name, qn)] = q[i]
        cols["%s_MEAN" % name] = nanmean(table)
    cols["LARGEST_GRADE_MEAN"] = nanmean(out["largest"]["grade"])
    cols["SEEDED_GRADE_MEAN"] = nanmean(out["seeded"]["grade"])
    cols["SEEDED_BODIES_MEAN"] = nanmean(out["seeded"]["bodies"])
    return pd.DataFrame(cols)[list(CSV_COLUMNS)]


def launch_cuts(S, C, n, ws_bytes=WS_BYTES):
    """How the engine cuts a batch: (samples, cutoffs) per launch so that the launch's workspace (about 16.1 bytes per voxel of a
    volume) stays below ws_bytes and its volumes below 65535; at least one volume."""
    per = 16 * int(n) + 48 * ((int(n) + 511) // 512) + 64
    vols = max(1, min(VOLUMES, int(ws_bytes) // per))
    if vols >= C:
        return max(1, min(int(S), vols // C)), int(C)
    return 1, vols


# ---- engine ---------------------------------------------------------------------------------------------------------------------
class BodyStatisticsError(RuntimeError):
    """A bounded walk of the device union-find ran out of rounds (info: 1 find, 2 union, 3 flatten): the labels are not trusted."""


class GeobodyMixin:
    def body_statistics(self, F, p, thresholds, lo=None, mask=None, box=None, neighbours=6, min_count=1, seeds=None, hits_largest=None,
                        hits_seeded=None, labels=None, ws_bytes=WS_BYTES):
        """Connected-body statistics of a device batch of realisations F (S, 3, N; normalised units, voxel order (iy, ix, iz)) for
        property p against the ascending `thresholds` (host, at most 32), the sets being those of cutoff_statistics (lo, mask, box as
        there).  Returns device tensors (stats (S, C, 6) int64, sums (S, C, 3) fp64) with the columns hip.BODY_STATS / hip.BODY_SUMS.
        seeds: host array of flat voxel (with box: block) indices or None; hits_largest, hits_seeded: (C, n) int32 device tensors or
        None, incremented per realisation whose largest / seeded body holds the voxel; labels: (S, C, n) int32 device tensor or None.
        box = (by, bx, bz): geobo_box_means first, then the block grid is labelled with the blocks' voxel counts as weights.
        A batch is cut into launches of at most ws_bytes of workspace; the cut changes no bit.  BodyStatisticsError when a bounded
        walk of the union-find ran out (the call reads one word back from the device)."""
        _check_batch(self, F, "body statistics")
        neighbours = check_neighbours(neighbours)
        with torch.cuda.device(self.device):
            t = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
            C_ = int(t.size)
            F, grid, weight = _block_support(self, F, box)
            S, n = F.shape[0], F.shape[2]
            stats = torch.empty((S, C_, len(hip.BODY_STATS)), dtype=torch.int64, device=F.device)
            sums = torch.empty((S, C_, len(hip.BODY_SUMS)), dtype=torch.float64, device=F.device)
            info = torch.zeros(1, dtype=torch.int32, device=F.device)
            Sl, Cl = launch_cuts(S, C_, n, ws_bytes)
            ws = self._workspace("bodies_ws", (hip.bodies_ws_doubles(Sl, grid, Cl),))
            whole = Sl >= S and Cl >= C_

            def run():
                for s0 in range(0, S, Sl):
                    s1 = min(S, s0 + Sl)
                    for c0 in range(0, C_, Cl):
                        c1 = min(C_, c0 + Cl)
                        lab = None
                        if labels is not None:
                            lab = labels if whole else torch.empty((s1 - s0, c1 - c0, n), dtype=torch.int32, device=F.device)
                        st = stats if whole else torch.empty((s1 - s0, c1 - c0, stats.shape[2]), dtype=torch.int64, device=F.device)
                        sm = sums if whole else torch.empty((s1 - s0, c1 - c0, sums.shape[2]), dtype=torch.float64, device=F.device)
                        hip.bodies(F[s0:s1], grid, p, t[c0:c1], lo=lo, mask=mask, weight=weight, neighbours=neighbours, min_count=min_count,
                                   seeds=seeds, hits_largest=None if hits_largest is None else hits_largest[c0:c1],
                                   hits_seeded=None if hits_seeded is None else hits_seeded[c0:c1], labels=lab, info=info, ws=ws,
                                   stats=st, sums=sm)
                        if not whole:
                            stats[s0:s1, c0:c1] = st
                            sums[s0:s1, c0:c1] = sm
                            if labels is not None:
                                labels[s0:s1, c0:c1] = lab
            self._timed("bodies", 0.0, run)
            code = int(info.item())
            if code:
                raise BodyStatisticsError("the union-find of geobo_bodies ran out of rounds (info = %d)" % code)
            return stats, sums
