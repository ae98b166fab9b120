"""NumPy reference of the grade-tonnage reductions, shared by the tests and the timing tool: thresholding of host
realisations, cutoff by cutoff, with math.fsum for the sums, and the bound every summation order of the device has to meet."""
import math

import numpy as np

U = 2.0 ** -53


def cutoff_stats(F, p, thresholds, lo=None, mask=None, weight=None):
    """F (S, 3, n) host realisations -> (cnt (S, C) int64, sum (S, C) by math.fsum, abs (S, C) = sum |w x| over the passing elements,
    terms (S, C) = how many pass, passes (S, C, n) bool).  Element v passes cutoff c when F[s, p, v] >= t[c], F[s, q, v] >= lo[q] for
    q != p and mask[v] != 0; NaN fails; weight (n,) ints, default 1."""
    F = np.asarray(F, dtype=np.float64)
    S, _, n = F.shape
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    lo = np.full(3, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    w = np.ones(n, dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64)
    base = np.ones((S, n), dtype=bool)
    if mask is not None:
        base &= (np.asarray(mask).reshape(-1) != 0)[None, :]
    with np.errstate(invalid="ignore"):
        for q in range(3):
            if q != p and lo[q] > -np.inf:
                base &= F[:, q] >= lo[q]
        passes = base[:, None, :] & (F[:, p][:, None, :] >= t[None, :, None])
    cnt = (passes * w[None, None, :]).sum(-1).astype(np.int64)
    wx = F[:, p] * w[None, :]
    tot, ab = np.zeros((S, t.size)), np.zeros((S, t.size))
    for s in range(S):
        for c in range(t.size):
            sel = wx[s][passes[s, c]]
            tot[s, c], ab[s, c] = math.fsum(sel), math.fsum(np.abs(sel))
    return cnt, tot, ab, passes.sum(-1), passes


def sum_bound(n, abs_sum):
    """2 x (n - 1) 2^-53 sum |w x|: any order of adding n numbers is within (n - 1) u sum |.| of the exact sum; the factor 2 covers
    the rounding of w x and the reference's own last rounding."""
    return 2.0 * (np.asarray(n) - 1) * U * np.asarray(abs_sum)


def box_means(F, grid, box):
    """F (S, 3, N) -> (G (S, 3, nblocks) by math.fsum / count, abs (S, 3, nblocks) = sum |x| per block, count (nblocks,))."""
    from geobo_amd.blocksupport import block_partition
    F = np.asarray(F, dtype=np.float64)
    index, count = block_partition(grid, box)
    S = F.shape[0]
    G, A = np.zeros((S, 3, count.size)), np.zeros((S, 3, count.size))
    for b in range(count.size):
        sel = index == b
        for s in range(S):
            for a in range(3):
                x = F[s, a, sel]
                G[s, a, b], A[s, a, b] = math.fsum(x) / count[b], math.fsum(np.abs(x))
    return G, A, count
