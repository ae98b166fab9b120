"""Block-support posterior statistics: the 3 x 3 covariance of the three properties' means over the boxes of a
block model, host helpers and the mixin of engine.PosteriorEngine.

With V_a = (L^-1 A3 K)[:, block a] (M x N, never stored) from the factor of the last posterior() step and a block B of n_B voxels,

    s_a[r, B] = sum_{v in B} V_a[r, v]
    cov(mean_B f_a, mean_B f_b | y) = kbar_ab(B) - (1 / n_B^2) sum_r s_a[r, B] s_b[r, B]
    kbar_ab(B) = (1 / n_B^2) sum_{v, v' in B} K_ab(v, v')

The tiles of the three V_a come in lockstep from the sweep of information.py (one forward transform of Z for the three outputs),
geobo_block_cov box-sums them and accumulates the six products per block.  The prior is stationary: kbar depends on the block's
shape alone (full or partial per axis, at most 8 shapes) and is the lattice table of geobo_cov_table contracted with the lag counts.

The raw entries are returned.  The reference's prior is not positive semidefinite for matern32 (create_cov's 1.02 l mutation and
cross weights), so a block's 3 x 3 matrix may have a slightly negative eigenvalue and a correlation slightly above 1 there: nothing
is factorised and nothing is clipped.

Blocks tile the grid from the origin, boxes of (by, bx, bz) voxels in the engine's (y, x, z) order, partial at the far edges;
block (jy, jx, jz) has index (jy nbx + jx) nbz + jz.
"""
import numpy as np
import torch

from . import hip

F64 = hip.F64
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))     # the order of geobo_block_cov's six sums


# ---- host helpers ---------------------------------------------------------------------------------------------------------------
def check_box(box, grid):
    """(b0, b1, b2) as ints: three integers >= 1, none beyond its extent of `grid` (same axis order); ValueError otherwise."""
    try:
        vals = list(box)
    except TypeError:
        raise ValueError("a block is three integers >= 1, got %r" % (box,)) from None
    if len(vals) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError("a block is three integers >= 1, got %r" % (box,))
    vals = tuple(int(v) for v in vals)
    if any(v < 1 for v in vals):
        raise ValueError("a block is three integers >= 1, got %r" % (box,))
    if any(v > n for v, n in zip(vals, grid)):
        raise ValueError("block %r exceeds the grid %r" % (vals, tuple(grid)))
    return vals


def block_counts(grid, box):
    """Blocks per axis: ceil(n / b)."""
    return tuple((int(n) + int(b) - 1) // int(b) for n, b in zip(grid, box))


def block_partition(grid, box):
    """(index, count): the block of every voxel, (N,) int64 in voxel order (iy, ix, iz), and the voxels of every block (nblocks,)."""
    nb = block_counts(grid, box)
    j = [np.arange(int(n)) // int(b) for n, b in zip(grid, box)]
    index = ((j[0][:, None, None] * nb[1] + j[1][None, :, None]) * nb[2] + j[2][None, None, :]).reshape(-1).astype(np.int64)
    return index, np.bincount(index, minlength=nb[0] * nb[1] * nb[2]).astype(np.int64)


def block_extents(grid, box):
    """(nblocks, 3) int64: the extent (m_y, m_x, m_z) of every block -- the box, cut at the far edges."""
    nb = block_counts(grid, box)
    m = [np.minimum(int(b), int(n) - np.arange(k) * int(b)) for n, b, k in zip(grid, box, nb)]
    out = np.empty(nb + (3,), dtype=np.int64)
    out[..., 0], out[..., 1], out[..., 2] = m[0][:, None, None], m[1][None, :, None], m[2][None, None, :]
    return out.reshape(-1, 3)


def lag_counts(m, signed=False):
    """How many ordered pairs of a run of m voxels lie d apart.  signed=False: c[d] = (m - d)(2 - [d = 0]) for d = 0 .. m - 1 (both
    signs of a lag folded onto |d|, as the table's y and x axes); signed=True: c[d] = m - |d| for d = -(m - 1) .. m - 1 (its z axis)."""
    m = int(m)
    if signed:
        return (m - np.abs(np.arange(-(m - 1), m))).astype(np.float64)
    c = 2.0 * (m - np.arange(m))
    c[0] = m
    return c


def mean_weights(extent):
    """W (m_y, m_x, 2 m_z - 1): kbar = sum W * table[:m_y, :m_x, nz - m_z : nz + m_z - 1] is the mean of K over all ordered voxel
    pairs of a block of that extent (the lag counts over (m_y m_x m_z)^2)."""
    my, mx, mz = (int(v) for v in extent)
    w = lag_counts(my)[:, None, None] * lag_counts(mx)[None, :, None] * lag_counts(mz, signed=True)[None, None, :]
    return w / float(my * mx * mz) ** 2


def prior_block_mean(table, grid, extent):
    """kbar of one covariance block for a block of `extent` = (m_y, m_x, m_z) voxels, from its lattice table (geobo_cov_table: index
    (dy nx + dx) 2 nz + dz + nz - 1; NumPy array or tensor of 2 N entries or more) on the grid (ny, nx, nz)."""
    ny, nx, nz = (int(v) for v in grid)
    my, mx, mz = (int(v) for v in extent)
    sub = table[:2 * ny * nx * nz].reshape(ny, nx, 2 * nz)[:my, :mx, nz - mz:nz + mz - 1]
    w = mean_weights(extent)
    if isinstance(table, torch.Tensor):
        return float((sub * torch.as_tensor(w, device=table.device)).sum())
    return float((np.asarray(sub) * w).sum())


# ---- engine ---------------------------------------------------------------------------------------------------------------------
class BlockSupportMixin:
    def block_covariance(self, box, kernelfunc, lengths, crossweights, gp_amp, source="auto"):
        """Posterior covariance of the three properties' block means, from the factor of the last posterior() step: device tensors
        cov (nblocks, 3, 3; symmetric, raw entries, the GP's normalised units) and count (nblocks, voxels per block).  box = (by, bx, bz)
        voxels in the engine's (y, x, z) order.  `lengths` carry the create_cov mutation.  source: "auto" (by the step's route),
        "spectral" or "generic".  One rank, fp64 assembly, a step over property blocks (0, 1, 2)."""
        from .engine import weight_matrix
        from .step import Prior
        if self.world > 1:
            raise NotImplementedError("set statistics run on one rank (world = %d)" % self.world)
        last = self.last
        if last is None or tuple(last["props"]) != (0, 1, 2):
            raise RuntimeError("block_covariance() needs the factor of a posterior() step over all three property blocks")
        AK = last["AK"] if last["AK_complete"] else last["AK_partial"]
        if self.f32 or (AK is not None and AK.dtype != F64):
            raise NotImplementedError("set statistics need the fp64 assembly")
        grid = (self.ny, self.nx, self.nz)
        box = check_box(box, grid)
        with torch.cuda.device(self.device):
            return self._block_covariance(box, grid, Prior(kernelfunc, lengths, weight_matrix(crossweights), float(gp_amp)), source, AK)

    def _block_covariance(self, box, grid, prior, source, AK):
        dev = self.device
        source = self._zsource(self.last["step"], AK, source)
        tiles = self._v_tiles(source, prior, AK, blocks=(0, 1, 2))
        ext = block_extents(grid, box)
        count = ext.prod(axis=1)
        C6 = torch.empty((count.size, 6), dtype=F64, device=dev)
        ws = self._workspace("block_ws", (hip.block_cov_ws_doubles(128 if source == "spectral" else 256, grid, box),))
        first = True
        while True:
            tile = self._timed("block_sweep", 0.0, lambda: next(tiles, None))
            if tile is None:
                break
            V, n = tile
            self._timed("block_cov", 12.0 * n * self.N, lambda: hip.block_cov(V, n, grid, box, C6, accumulate=not first, ws=ws), valu=12.0 * n * self.N)
            first = False
        # prior term: one value per block shape and property pair
        shapes, shape_of = np.unique(ext, axis=0, return_inverse=True)
        kbar = np.empty((len(shapes), 6))
        for p, (a, b) in enumerate(PAIRS):
            table = prior.table(self, a, b)
            for i, m in enumerate(shapes):
                kbar[i, p] = prior_block_mean(table, grid, m)
        cnt = torch.as_tensor(count, device=dev)
        c6 = torch.as_tensor(kbar[shape_of.reshape(-1)], device=dev) - C6 / (cnt.to(F64) ** 2)[:, None]
        cov = torch.empty((count.size, 3, 3), dtype=F64, device=dev)
        for p, (a, b) in enumerate(PAIRS):
            cov[:, a, b] = c6[:, p]
            cov[:, b, a] = c6[:, p]
        return cov, cnt
