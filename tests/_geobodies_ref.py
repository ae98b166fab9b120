"""Host reference of the connected-body statistics, shared by the tests and the timing tool: the sets of
_gradetonnage_ref.cutoff_stats, labelled by scipy.ndimage.label (or by a plain breadth-first search that pins it), with math.fsum for
the sums; and the test patterns."""
import math
from collections import deque

import numpy as np

import _gradetonnage_ref as gt

U = gt.U
sum_bound = gt.sum_bound


def _offsets(neighbours):
    if neighbours not in (6, 26):
        raise ValueError(neighbours)
    out = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = abs(dy) + abs(dx) + abs(dz)
                if k and (neighbours == 26 or k == 1):
                    out.append((dy, dx, dz))
    return out


def label_scipy(inset, neighbours):
    """Boolean (ny, nx, nz) -> int32 canonical labels: the smallest flat index of each voxel's body, -1 outside."""
    from scipy import ndimage
    inset = np.asarray(inset, dtype=bool)
    lab, B = ndimage.label(inset, structure=ndimage.generate_binary_structure(3, 1 if neighbours == 6 else 3))
    flat = lab.reshape(-1)
    first = np.full(B + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    out = np.where(flat > 0, first[flat], -1).astype(np.int32)
    return out.reshape(inset.shape)


def label_bfs(inset, neighbours):
    """The same labels by a breadth-first search from every unvisited in-set voxel in ascending flat order."""
    inset = np.asarray(inset, dtype=bool)
    ny, nx, nz = inset.shape
    offs = _offsets(neighbours)
    out = np.full(inset.shape, -1, dtype=np.int32)
    for iy in range(ny):
        for ix in range(nx):
            for iz in range(nz):
                if not inset[iy, ix, iz] or out[iy, ix, iz] >= 0:
                    continue
                root = (iy * nx + ix) * nz + iz
                out[iy, ix, iz] = root
                queue = deque([(iy, ix, iz)])
                while queue:
                    y, x, z = queue.popleft()
                    for dy, dx, dz in offs:
                        a, b, c = y + dy, x + dx, z + dz
                        if 0 <= a < ny and 0 <= b < nx and 0 <= c < nz and inset[a, b, c] and out[a, b, c] < 0:
                            out[a, b, c] = root
                            queue.append((a, b, c))
    return out


def bodies(F, grid, p, thresholds, lo=None, mask=None, weight=None, neighbours=6, min_count=1, seeds=None, labeller=label_scipy):
    """F (S, 3, n) host realisations on grid (ny, nx, nz) -> dict: stats (S, C, 6) int64 [count_total, n_bodies, largest count, largest
    label, seeded count, seeded bodies], sums (S, C, 3) by math.fsum [set, largest, seeded], abs (S, C, 3) = sum |w x| over the same
    members, labels (S, C, n) int32 canonical, in_largest and in_seeded (S, C, n) bool."""
    F = np.asarray(F, dtype=np.float64)
    cnt, _, _, _, passes = gt.cutoff_stats(F, p, thresholds, lo=lo, mask=mask, weight=weight)
    S, C, n = passes.shape
    w = np.ones(n, dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64)
    wx = F[:, p] * w[None, :]
    sd = np.zeros(0, dtype=np.int64) if seeds is None else np.asarray(seeds, dtype=np.int64).reshape(-1)
    stats = np.zeros((S, C, 6), dtype=np.int64)
    sums, ab = np.zeros((S, C, 3)), np.zeros((S, C, 3))
    labels = np.full((S, C, n), -1, dtype=np.int32)
    in_l, in_s = np.zeros((S, C, n), dtype=bool), np.zeros((S, C, n), dtype=bool)
    for s in range(S):
        for c in range(C):
            inset = passes[s, c]
            lab = labeller(inset.reshape(grid), neighbours).reshape(-1)
            labels[s, c] = lab
            size = np.zeros(n, dtype=np.int64)
            np.add.at(size, lab[inset], w[inset])
            roots = np.unique(lab[inset])
            assert np.array_equal(roots, np.flatnonzero(lab == np.arange(n)))
            stats[s, c, 0] = cnt[s, c]
            assert size.sum() == cnt[s, c]
            stats[s, c, 1] = (size[roots] >= min_count).sum()
            stats[s, c, 3] = -1
            if roots.size:
                big = roots[np.argmax(size[roots])]                      # (the first maximum: the smaller label of a tie)
                stats[s, c, 2], stats[s, c, 3] = size[big], big
                in_l[s, c] = lab == big
            hit = np.unique(lab[sd][lab[sd] >= 0]) if sd.size else np.zeros(0, dtype=np.int32)
            in_s[s, c] = inset & np.isin(lab, hit)
            stats[s, c, 4], stats[s, c, 5] = w[in_s[s, c]].sum(), hit.size
            for k, member in enumerate((inset, in_l[s, c], in_s[s, c])):
                sel = wx[s][member]
                sums[s, c, k], ab[s, c, k] = math.fsum(sel), math.fsum(np.abs(sel))
    return dict(stats=stats, sums=sums, abs=ab, labels=labels, in_largest=in_l, in_seeded=in_s)


def count_bodies(labels, weight, min_count):
    """(S, C, n) canonical labels -> (S, C) bodies of at least min_count weighted voxels."""
    S, C, n = labels.shape
    w = np.ones(n, dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64)
    out = np.zeros((S, C), dtype=np.int64)
    for s in range(S):
        for c in range(C):
            lab = labels[s, c]
            size = np.zeros(n, dtype=np.int64)
            np.add.at(size, lab[lab >= 0], w[lab >= 0])
            out[s, c] = (size[lab == np.arange(n)] >= min_count).sum()
    return out


# ---- patterns -------------------------------------------------------------------------------------------------------------------
def serpentine(grid):
    """One chain through the grid whose smallest index is at one end: the z-rows at even (iy, ix) in boustrophedon order, each joined
    to the next by one voxel at alternating ends."""
    ny, nx, nz = grid
    g = np.zeros(grid, dtype=bool)
    rows = []
    for jy in range(0, ny, 2):
        xs = list(range(0, nx, 2))
        rows += [(jy, x) for x in (xs if (jy // 2) % 2 == 0 else xs[::-1])]
    for k, (y, x) in enumerate(rows):
        g[y, x, :] = True
        if k + 1 < len(rows):
            y2, x2 = rows[k + 1]
            g[(y + y2) // 2, (x + x2) // 2, nz - 1 if k % 2 == 0 else 0] = True
    return g


def spiral(grid):
    """A square spiral in the plane iz = 0, walked inwards from voxel (0, 0): a chain with one-voxel gaps between its turns."""
    ny, nx, nz = grid
    g = np.zeros((ny, nx), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = True

    def free(a, b, py, px):
        if not (0 <= a < ny and 0 <= b < nx) or g[a, b]:
            return False
        for ey, ex in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            c, d = a + ey, b + ex
            if (c, d) != (py, px) and 0 <= c < ny and 0 <= d < nx and g[c, d]:
                return False
        return True
    while True:
        for _ in range(2):
            if free(y + dy, x + dx, y, x):
                y, x = y + dy, x + dx
                g[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            break
    out = np.zeros(grid, dtype=bool)
    out[:, :, 0] = g
    return out


def patterns(grid, rng):
    """Named boolean sets on the grid (tests)."""
    ny, nx, nz = grid
    iy, ix, iz = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(nz), indexing="ij")
    out = [("empty", np.zeros(grid, dtype=bool)), ("full", np.ones(grid, dtype=bool)), ("checkerboard", (iy + ix + iz) % 2 == 0),
           ("serpentine", serpentine(grid)), ("spiral", spiral(grid)),
           ("comb_last_plane", ((iy % 2 == 0) & (ix % 2 == 0)) | (iz == nz - 1)),
           ("comb_last_row", ((ix % 2 == 0) & (iz % 2 == 0)) | (iy == ny - 1)),
           ("u_shape", (ix == 0) | (ix == nx - 1) | ((iy == ny - 1) & (iz == nz - 1)))]
    hy, hx, hz = (ny + 1) // 2, (nx + 1) // 2, (nz + 1) // 2
    out.append(("corner_touch", ((iy < hy) & (ix < hx) & (iz < hz)) | ((iy >= hy) & (ix >= hx) & (iz >= hz))))
    out.append(("edge_touch", ((iy < hy) & (ix < hx)) | ((iy >= hy) & (ix >= hx)) if ny > 1 and nx > 1 else ((ix < hx) & (iz < hz)) | ((ix >= hx) & (iz >= hz))))
    for occ in (0.08, 0.12, 0.25, 0.31, 0.5):
        out.append(("random_%.2f" % occ, rng.random(grid) < occ))
    return out
