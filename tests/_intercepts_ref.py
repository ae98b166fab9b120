"""Plain NumPy / Python reference of the drill-intercept statistics: a loop over the positions of a trace,
sums by math.fsum.  Nothing here shares code with geobo_amd/intercepts.py or the kernel.

Definitions, for the values x_j of property p along a trace (shallow to deep):
  eligible e_j: inside the mask and x_j not NaN;  ore o_j: e_j, x_j >= t and the other properties >= their lower bounds;
  a maximal run of non-ore positions is FILLED when its length is <= max_gap, all of it is eligible and an ore position lies
  immediately before and after it;  composite = ore or filled;  intercepts = maximal runs of composite;  BEST = the longest, a tie
  to the smaller start."""
import math

import numpy as np

U = 2.0 ** -53


def trace_flags(x, ore, eligible, min_len=1, max_gap=0):
    """One trace: x (L,) values, ore and eligible (L,) booleans -> dict(thick, top, start, len, n_int, acc, run_sum, acc_abs,
    run_abs, composite); acc_abs and run_abs are the sums of |x| behind the two sums (for the error bounds)."""
    L = len(x)
    ore = [bool(v) for v in ore]
    eligible = [bool(v) for v in eligible]
    comp = list(ore)
    j = 0
    while j < L:
        if ore[j]:
            j += 1
            continue
        g0 = j
        while j < L and not ore[j]:
            j += 1
        g1 = j                                                  # the maximal non-ore run [g0, g1)
        if g0 > 0 and g1 < L and g1 - g0 <= max_gap and all(eligible[g0:g1]):
            for i in range(g0, g1):
                comp[i] = True
    runs = []
    j = 0
    while j < L:
        if not comp[j]:
            j += 1
            continue
        r0 = j
        while j < L and comp[j]:
            j += 1
        runs.append((r0, j - r0))
    start, length = L, 0
    for r0, rl in runs:
        if rl > length:
            start, length = r0, rl
    best = range(start, start + length)
    ore_x = [float(x[i]) for i in range(L) if ore[i]]
    run_x = [float(x[i]) for i in best]
    return dict(thick=sum(ore), top=ore.index(True) if any(ore) else L, start=start, len=length,
                n_int=sum(1 for _, rl in runs if rl >= min_len), acc=math.fsum(ore_x), run_sum=math.fsum(run_x),
                acc_abs=math.fsum(abs(v) for v in ore_x), run_abs=math.fsum(abs(v) for v in run_x), composite=comp)


def column_traces(ny, nx, nz):
    return [list(range(k * nz, (k + 1) * nz)) for k in range(ny * nx)]


def trace_stats(F, p, t, traces, lo=None, mask=None, min_len=1, max_gap=0):
    """F (S, 3, n), thresholds t (C,), traces = list of voxel index lists -> dict: detail (S, C, K, 6) int32 = thick, top, start,
    len, n_int, 0; dsum (S, C, K, 2) = acc, run_sum; dabs (S, C, K, 2) = the sums of |x| behind them; tab (S, C, 3) int64."""
    F = np.asarray(F, dtype=np.float64)
    S = F.shape[0]
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    lo = np.full(3, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    K = len(traces)
    detail = np.zeros((S, t.size, K, 6), dtype=np.int32)
    dsum = np.zeros((S, t.size, K, 2))
    dabs = np.zeros((S, t.size, K, 2))
    for s in range(S):
        for k, tr in enumerate(traces):
            idx = np.asarray(tr, dtype=np.int64)
            x = F[s, p, idx]
            elig = ~np.isnan(x)
            if mask is not None:
                elig &= np.asarray(mask).reshape(-1)[idx] != 0
            other = np.ones(idx.size, dtype=bool)
            for q in range(3):
                if q != p and lo[q] > -np.inf:
                    with np.errstate(invalid="ignore"):
                        other &= F[s, q, idx] >= lo[q]
            for c in range(t.size):
                with np.errstate(invalid="ignore"):
                    ore = elig & other & (x >= t[c])
                r = trace_flags(x, ore, elig, min_len, max_gap)
                detail[s, c, k] = (r["thick"], r["top"], r["start"], r["len"], r["n_int"], 0)
                dsum[s, c, k] = (r["acc"], r["run_sum"])
                dabs[s, c, k] = (r["acc_abs"], r["run_abs"])
    hit = detail[..., 3] >= min_len
    tab = np.stack([hit.sum(-1), detail[..., 0].sum(-1, dtype=np.int64), detail[..., 3].max(-1)], -1).astype(np.int64)
    return dict(detail=detail, dsum=dsum, dabs=dabs, tab=tab)


def maps_of(r, Lmax, min_len=1):
    """The reference's (S, C, K) tables -> the maps and histograms the kernel accumulates over the samples."""
    d = r["detail"]
    S, C, K = d.shape[:3]
    thick, top, length = d[..., 0].astype(np.int64), d[..., 1].astype(np.int64), d[..., 3]
    present = thick > 0
    out = dict(hits_any=present.sum(0).astype(np.int32), hits=(length >= min_len).sum(0).astype(np.int32), thick_sum=thick.sum(0),
               top_sum=np.where(present, top, 0).sum(0))
    acc = np.zeros((C, K))
    for c in range(C):
        for k in range(K):
            acc[c, k] = math.fsum(r["dsum"][:, c, k, 0])
    out["acc_sum"] = acc
    out["acc_sum_abs"] = np.abs(r["dsum"][..., 0]).sum(0)
    for name, col in (("hist_len", length), ("hist_thick", thick)):
        h = np.zeros((C, K, Lmax + 1), dtype=np.int32)
        for s in range(S):
            for c in range(C):
                np.add.at(h[c], (np.arange(K), col[s, c]), 1)
        out[name] = h
    return out


def sum_bound(L, abs_sum):
    """Twice the bound of any summation order of L numbers against the exact sum: 2 (L - 1) 2^-53 sum |x|."""
    return 2.0 * np.maximum(np.asarray(L) - 1, 0) * U * np.asarray(abs_sum)
