"""Drill-intercept statistics along holes and columns from posterior realisations: host helpers and the mixin
of engine.PosteriorEngine.

What a drill hole would intersect -- how thick the material at or above a cutoff is along it, where it starts, how long the longest
continuous intercept is once short waste gaps are composited in, what accumulation (grade x metres) it returns -- depends on the
order of the samples along the hole and is not linear in the field: the law comes from the joint realisations alone.
geobo_trace_stats reduces a device batch of realisations along TRACES (ordered voxel lists, shallow to deep: every z-column of the
cube, or a CSR list built here from vertical holes and dipping paths) to small tables, maps over (cutoff, trace) and two
histograms per (cutoff, trace), from which exact order statistics follow without a sort.  Units and the cutoff conversion are
those of resources.py; lengths are counted in down-hole SAMPLES on the device (one voxel of a column, one step of a path) and
turned into metres here.
"""
import math

import numpy as np
import torch

from . import hip
from .resources import QUANTILES, _check_batch

WS_BYTES = 1 << 30                  # bound of the workspace plus the per-hole tables of one geobo_trace_stats launch
LMAX = hip.TRACE_LMAX


# ---- traces ---------------------------------------------------------------------------------------------------------------------
def column_traces(grid):
    """Every z-column of `grid` = (ny, nx, nz) as CSR (offsets (K + 1,), voxels (K nz,)), K = ny nx, column k = (iy nx + ix): what
    geobo_trace_stats walks when it is given no trace list."""
    ny, nx, nz = (int(v) for v in grid)
    K = ny * nx
    return np.arange(K + 1, dtype=np.int64) * nz, np.arange(K * nz, dtype=np.int64)


def hole_traces(holes, grid):
    """Vertical holes [(ix, iy), ...] -> CSR (offsets, voxels) of their z-columns, top to bottom.  ValueError for a hole outside the
    grid or an empty list."""
    ny, nx, nz = (int(v) for v in grid)
    try:
        h = np.asarray(holes)
    except (TypeError, ValueError):
        raise ValueError("holes is a list of (ix, iy) voxel indices") from None
    if h.ndim != 2 or h.shape[1] != 2 or h.shape[0] < 1 or not np.issubdtype(h.dtype, np.integer):
        raise ValueError("holes is a list of (ix, iy) integer voxel indices, got shape %r %s" % (h.shape, h.dtype))
    ix, iy = h[:, 0].astype(np.int64), h[:, 1].astype(np.int64)
    if ((ix < 0) | (ix >= nx) | (iy < 0) | (iy >= ny)).any():
        raise ValueError("a hole (ix, iy) lies outside the %d x %d columns" % (nx, ny))
    base = (iy * nx + ix) * nz
    return np.arange(h.shape[0] + 1, dtype=np.int64) * nz, (base[:, None] + np.arange(nz, dtype=np.int64)[None, :]).reshape(-1)


def path_triplets(settings, x0, y0, azimuth, dip, ranges):
    """The index triplets of Acquisition.path_voxels for a hole collared at (x0, y0, zmax), at the given ranges along it (the depth
    below zmax over the voxel height: path_voxels' -z / zvoxsize at its zmax = 0)."""
    from .acquisition import spherical2cartes
    s = settings
    x, y, z = spherical2cartes(x0, y0, s.zmax, np.deg2rad(azimuth), np.deg2rad(180. - dip), np.asarray(ranges, dtype=np.float64))
    return (x / s.xvoxsize).astype(int), (y / s.yvoxsize).astype(int), ((s.zmax - z) / s.zvoxsize).astype(int)


def triplet_trace(triplet, shape):
    """An Acquisition.path_voxels triplet (index arrays into the three axes of the cube of `shape`, as hole_statistics reads them) ->
    the flat voxel index of every step, in path order; consecutive steps inside one voxel stay separate entries.  ValueError for a
    path that leaves the cube."""
    shape = tuple(int(v) for v in shape)
    a = [np.asarray(v, dtype=np.int64).reshape(-1) for v in triplet]
    if not all(np.all((v >= 0) & (v < n)) for v, n in zip(a, shape)):
        raise ValueError("the path leaves the cube")
    return np.ravel_multi_index(tuple(a), shape).astype(np.int64)


def path_ranges(settings, x0, y0, azimuth, dip, step=None, length=None):
    """The ranges of predict_path: step / 2, 3 step / 2, ... up to `length`, cut where the path first leaves the cube's box or the
    index range of path_triplets.  step defaults to half the smallest voxel edge, length to zLcube.  Returns (ranges, step)."""
    from .acquisition import spherical2cartes
    s = settings
    step = 0.5 * min(s.xvoxsize, s.yvoxsize, s.zvoxsize) if step is None else float(step)
    length = float(s.zLcube) if length is None else float(length)
    if not (step > 0 and np.isfinite(step) and length > 0 and np.isfinite(length)):
        raise ValueError("step and length must be positive, got %r and %r" % (step, length))
    n = int(np.floor(length / step + 0.5 + 1e-12))
    rng = (np.arange(n) + 0.5) * step
    x, y, z = spherical2cartes(float(x0), float(y0), float(s.zmax), np.deg2rad(azimuth), np.deg2rad(180. - dip), rng)
    inside = (x >= 0) & (x <= s.xLcube) & (y >= 0) & (y <= s.yLcube) & (z >= s.zmax - s.zLcube) & (z <= s.zmax)
    for v, m in zip(path_triplets(s, float(x0), float(y0), azimuth, dip, rng), (s.yNcube, s.xNcube, s.zNcube)):
        inside &= (v >= 0) & (v < int(m))                       # (path_voxels' triplet indexes the cube's axes in their order)
    keep = n if inside.all() else int(np.argmin(inside))
    return rng[:keep], step


def path_traces(settings, paths, step=None, length=None):
    """Dipping holes [(x0, y0, azimuth, dip), ...] in the convention of Acquisition.path_voxels, sampled at the ranges of
    predict_path -> (offsets, voxels, step): one entry per step, duplicates kept.  ValueError for a path without a point inside the
    cube or with more than 4096 steps."""
    s = settings
    shape = (int(s.yNcube), int(s.xNcube), int(s.zNcube))
    offsets, voxels, used = [0], [], None
    if len(paths) < 1:
        raise ValueError("paths is a list of (x0, y0, azimuth, dip)")
    for path in paths:
        try:
            x0, y0, azimuth, dip = (float(v) for v in path)
        except (TypeError, ValueError):
            raise ValueError("a path is (x0, y0, azimuth, dip), got %r" % (path,)) from None
        rng, used = path_ranges(s, x0, y0, azimuth, dip, step, length)
        if rng.size < 1 or rng.size > LMAX:
            raise ValueError("the path from (%r, %r) with azimuth %r and dip %r has %d steps inside the cube; between 1 and %d"
                             % (x0, y0, azimuth, dip, rng.size, LMAX))
        voxels.append(triplet_trace(path_triplets(s, x0, y0, azimuth, dip, rng), shape))
        offsets.append(offsets[-1] + rng.size)
    return np.asarray(offsets, dtype=np.int64), np.concatenate(voxels), used


# ---- units ----------------------------------------------------------------------------------------------------------------------
def samples_of(min_length, max_gap, sample_length):
    """Metres down the hole -> samples: (min_len, max_gap) = (ceil(min_length / sample length), floor(max_gap / sample length)), a
    quotient within 1e-9 of an integer counting as that integer; min_length None = one sample.  ValueError for a negative or
    non-finite length, a min_length of 0 or a gap of more than 4096 samples."""
    dz = float(sample_length)
    if not (dz > 0 and np.isfinite(dz)):
        raise ValueError("the down-hole sample length must be positive, got %r" % (sample_length,))
    if min_length is None:
        min_len = 1
    else:
        m = float(min_length)
        if not (m > 0 and np.isfinite(m)):
            raise ValueError("min_length is a positive length in metres, got %r" % (min_length,))
        min_len = max(1, int(math.ceil(m / dz - 1e-9)))
    g = float(max_gap)
    if not (g >= 0 and np.isfinite(g)):
        raise ValueError("max_gap is a length >= 0 in metres, got %r" % (max_gap,))
    gap = int(math.floor(g / dz + 1e-9))
    if gap > LMAX:
        raise ValueError("max_gap spans %d samples; at most %d" % (gap, LMAX))
    return min_len, gap


def hist_quantiles(hist, q=QUANTILES):
    """Exact order statistics from histograms of integers: hist (..., B) counts of the values 0 .. B - 1 -> (len(q), ...) int64, the
    inverted-CDF quantiles np.quantile(values, q, method="inverted_cdf") of the samples behind each histogram (-1 for an empty
    one)."""
    h = np.asarray(hist, dtype=np.int64)
    cum = np.cumsum(h, axis=-1)
    n = cum[..., -1]
    out = np.empty((len(q),) + h.shape[:-1], dtype=np.int64)
    for i, qi in enumerate(q):
        target = np.clip(np.ceil(n * float(qi)), 1, np.maximum(n, 1)).astype(np.int64)
        out[i] = np.argmax(cum >= target[..., None], axis=-1)
        out[i][n == 0] = -1
    return out


def hist_mean(hist):
    """The mean of the samples behind histograms of the values 0 .. B - 1 (NaN for an empty one)."""
    h = np.asarray(hist, dtype=np.int64)
    n = h.sum(-1)
    tot = (h * np.arange(h.shape[-1], dtype=np.int64)).sum(-1)
    with np.errstate(all="ignore"):
        return np.where(n > 0, tot / np.where(n > 0, n, 1), np.nan)


def length_summary(hist, sample_length):
    """dict(mean, p10, p50, p90) in metres from histograms of lengths in samples."""
    q = hist_quantiles(hist) * float(sample_length)
    return dict(mean=hist_mean(hist) * float(sample_length), p10=q[0], p50=q[1], p90=q[2])


def _q3(a):
    a = np.asarray(a, dtype=np.float64)
    return np.quantile(a, QUANTILES, axis=0)


def intercept_tables(tab, sample_length, column_area=None):
    """(n, C, 3) int64 tab of geobo_trace_stats -> dict: holes_hit (n, C), count (n, C) = the ore samples of all traces, longest
    (n, C) metres, with column_area prospective_area = holes_hit x column_area, and quantiles (3, C) of longest (and the area)."""
    tab = np.asarray(tab, dtype=np.int64)
    out = dict(holes_hit=tab[..., 0].copy(), count=tab[..., 1].copy(), longest=tab[..., 2] * float(sample_length))
    out["quantiles"] = dict(longest=_q3(out["longest"]))
    if column_area is not None:
        out["prospective_area"] = out["holes_hit"] * float(column_area)
        out["quantiles"]["prospective_area"] = _q3(out["prospective_area"])
    return out


def intercept_maps(maps, n, scale, offset, sample_length):
    """The accumulators of geobo_trace_stats over n realisations (host arrays, (C, K) and (C, K, B)) -> dict of (C, K) arrays:
    probability, probability_any, thickness and intercept_length (dicts of mean, p10, p50, p90; metres), depth_to_top_mean (metres
    down the hole, given presence; NaN where never present) and accumulation_mean = (scale x acc_sum + offset x thick_sum) x sample
    length / n."""
    dz, n = float(sample_length), int(n)
    any_ = np.asarray(maps["hits_any"], dtype=np.int64)
    out = dict(probability=np.asarray(maps["hits"], dtype=np.float64) / n, probability_any=any_ / float(n))
    out["thickness"] = length_summary(maps["hist_thick"], dz)
    out["thickness"]["mean"] = np.asarray(maps["thick_sum"], dtype=np.float64) * dz / n
    out["intercept_length"] = length_summary(maps["hist_len"], dz)
    with np.errstate(all="ignore"):
        out["depth_to_top_mean"] = np.where(any_ > 0, np.asarray(maps["top_sum"], dtype=np.float64) * dz / np.where(any_ > 0, any_, 1), np.nan)
    out["accumulation_mean"] = (float(scale) * np.asarray(maps["acc_sum"], dtype=np.float64)
                                + float(offset) * np.asarray(maps["thick_sum"], dtype=np.float64)) * dz / n
    return out


def per_realisation(detail, dsum, scale, offset, sample_length):
    """detail (n, C, K, 6) and dsum (n, C, K, 2) of geobo_trace_stats -> dict of (n, C, K) arrays in metres and cube units: thickness,
    depth_to_top and `from` (NaN without ore / intercept), length, grade = (scale x run_sum + offset x len) / len (NaN without an
    intercept), accumulation = (scale x acc + offset x thick) x sample length, n_intercepts."""
    d = np.asarray(detail, dtype=np.int64)
    sums = np.asarray(dsum, dtype=np.float64)
    dz = float(sample_length)
    thick, top, start, length = d[..., 0], d[..., 1], d[..., 2], d[..., 3]
    with np.errstate(all="ignore"):
        grade = np.where(length > 0, (float(scale) * sums[..., 1] + float(offset) * length) / np.where(length > 0, length, 1), np.nan)
    return dict(thickness=thick * dz, depth_to_top=np.where(thick > 0, top * dz, np.nan), length=length * dz,
                grade=grade, accumulation=(float(scale) * sums[..., 0] + float(offset) * thick) * dz, n_intercepts=d[..., 4].copy(),
                **{"from": np.where(length > 0, start * dz, np.nan)})


# ---- CSV frames -------------------------------------------------------------------------------------------------------------------
CSV_COLUMNS = ("CUTOFF",) + tuple("%s_%s" % (k, q) for k in ("AREA", "LONGEST") for q in ("P10", "P50", "P90", "MEAN"))
MAP_COLUMNS = ("X", "Y", "CUTOFF", "PROBABILITY", "PROBABILITY_ANY", "THICKNESS_MEAN", "THICKNESS_P10", "THICKNESS_P50", "THICKNESS_P90",
               "LENGTH_MEAN", "LENGTH_P10", "LENGTH_P50", "LENGTH_P90", "DEPTH_TO_TOP_MEAN", "ACCUMULATION_MEAN")
HOLE_COLUMNS = ("HOLE",) + MAP_COLUMNS[2:]


def curve_frame(out):
    """One row per cutoff: CUTOFF, then P10 / P50 / P90 / MEAN of the prospective area and of the longest intercept."""
    import pandas as pd
    cols = {"CUTOFF": np.asarray(out["cutoffs"], dtype=np.float64)}
    for name, key in (("AREA", "prospective_area"), ("LONGEST", "longest")):
        if key in out:
            q, mean = out["quantiles"][key], np.asarray(out[key], dtype=np.float64).mean(0)
        else:
            q, mean = np.full((3, cols["CUTOFF"].size), np.nan), np.full(cols["CUTOFF"].size, np.nan)
        for i, qn in enumerate(("P10", "P50", "P90")):
            cols["%s_%s" % (name, qn)] = q[i]
        cols["%s_MEAN" % name] = mean
    return pd.DataFrame(cols)[list(CSV_COLUMNS)]


def _summary_columns(out, cols):
    flat = lambda a: np.asarray(a, dtype=np.float64).reshape(-1)
    cols["PROBABILITY"], cols["PROBABILITY_ANY"] = flat(out["probability"]), flat(out["probability_any"])
    for name, key in (("THICKNESS", "thickness"), ("LENGTH", "intercept_length")):
        for qn in ("mean", "p10", "p50", "p90"):
            cols["%s_%s" % (name, qn.upper())] = flat(out[key][qn])
    cols["DEPTH_TO_TOP_MEAN"], cols["ACCUMULATION_MEAN"] = flat(out["depth_to_top_mean"]), flat(out["accumulation_mean"])
    return cols


def map_frame(out, x, y):
    """One row per cutoff and column: X, Y (the columns' coordinates, (xN,) and (yN,)), CUTOFF and the map columns; rows in the
    order of the (C, yN, xN) maps."""
    import pandas as pd
    Cn, ny, nx = np.asarray(out["probability"]).shape
    cols = dict(X=np.broadcast_to(np.asarray(x, dtype=np.float64)[None, None, :], (Cn, ny, nx)).reshape(-1),
                Y=np.broadcast_to(np.asarray(y, dtype=np.float64)[None, :, None], (Cn, ny, nx)).reshape(-1),
                CUTOFF=np.repeat(np.asarray(out["cutoffs"], dtype=np.float64), ny * nx))
    return pd.DataFrame(_summary_columns(out, cols))[list(MAP_COLUMNS)]


def hole_frame(out):
    """One row per cutoff and hole: HOLE (its number in the caller's list), CUTOFF and the summary columns."""
    import pandas as pd
    Cn, K = np.asarray(out["probability"]).shape
    cols = dict(HOLE=np.tile(np.arange(K), Cn), CUTOFF=np.repeat(np.asarray(out["cutoffs"], dtype=np.float64), K))
    return pd.DataFrame(_summary_columns(out, cols))[list(HOLE_COLUMNS)]


def parse_yaml(d):
    """The YAML key drill_intercepts: {cutoffs, property, samples, offset, min_length, max_gap} and optionally holes: [[ix, iy], ...]
    or paths: [[x0, y0, azimuth, dip], ...] with step -> (keyword arguments of Inversion.drill_intercepts for the columns, the
    extra keyword arguments of a second call for the holes or paths, or None).  ValueError for an unknown key or missing cutoffs."""
    known = ("cutoffs", "property", "samples", "offset", "min_length", "max_gap", "holes", "paths", "step")
    if not isinstance(d, dict) or "cutoffs" not in d:
        raise ValueError("drill_intercepts needs cutoffs: [...]")
    extra = sorted(set(d) - set(known))
    if extra:
        raise ValueError("drill_intercepts: unknown keys %r (known: %r)" % (extra, known))
    if d.get("holes") and d.get("paths"):
        raise ValueError("drill_intercepts: give holes or paths, not both")
    ml = d.get("min_length")
    kw = dict(cutoffs=[float(v) for v in d["cutoffs"]], prop=d.get("property", "drill"), n=int(d.get("samples", 256)),
              offset=float(d.get("offset", 0.0)), min_length=None if ml is None else float(ml), max_gap=float(d.get("max_gap", 0.0)))
    along = None
    if d.get("holes"):
        along = dict(holes=[tuple(int(v) for v in h) for h in d["holes"]])
    elif d.get("paths"):
        along = dict(paths=[tuple(float(v) for v in h) for h in d["paths"]], step=None if d.get("step") is None else float(d["step"]))
    return kw, along


def launch_cuts(S, C, K, detail=False, ws_bytes=WS_BYTES):
    """How the engine cuts a batch: the samples of one launch, so that its workspace (4 bytes per (sample, trace, cutoff)) and, with
    detail, its per-hole tables (40 more) stay below ws_bytes; at least one sample."""
    per = int(K) * int(C) * (44 if detail else 4)
    return max(1, min(max(int(S), 1), int(ws_bytes) // per))


# ---- engine ---------------------------------------------------------------------------------------------------------------------
class InterceptMixin:
    def trace_statistics(self, F, p, thresholds, lo=None, mask=None, traces=None, min_len=1, max_gap=0, maps=None, detail=False,
                         ws_bytes=WS_BYTES):
        """Drill-intercept statistics of a device batch of realisations F (S, 3, N; normalised units, voxel order (iy, ix, iz)) for
        property p against the ascending `thresholds` (host, at most 32), the ore being the set of cutoff_statistics (lo, mask as
        there).  traces: a hip.TraceSet, or None for every z-column.  min_len, max_gap: in samples.  maps: dict of device
        accumulators (hip.trace_maps) incremented by the batch, or None.  Returns tab (S, C, 3) int64 (hip.TRACE_TAB) and with detail
        (tab, detail (S, C, K, 6) int32, dsum (S, C, K, 2) fp64) -- hip.TRACE_DETAIL, hip.TRACE_DSUM.  A batch is cut into launches
        whose workspace and per-hole tables stay below ws_bytes; the cut changes no bit."""
        _check_batch(self, F, "trace statistics")
        with torch.cuda.device(self.device):
            S = F.shape[0]
            t = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
            C_ = int(t.size)
            grid = (self.ny, self.nx, self.nz)
            K = grid[0] * grid[1] if traces is None else traces.K
            tab = torch.empty((S, C_, 3), dtype=torch.int64, device=F.device)
            det = torch.empty((S, C_, K, 6), dtype=torch.int32, device=F.device) if detail else None
            dsm = torch.empty((S, C_, K, 2), dtype=torch.float64, device=F.device) if detail else None
            Sl = launch_cuts(S, C_, K, detail, ws_bytes)
            ws = self._workspace("intercepts_ws", (hip.trace_stats_ws_doubles(Sl, K, C_),))

            def run():
                for s0 in range(0, S, Sl):
                    s1 = min(S, s0 + Sl)
                    hip.trace_stats(F[s0:s1], grid, p, t, lo=lo, mask=mask, traces=traces, min_len=min_len, max_gap=max_gap, maps=maps,
                                    detail=None if det is None else det[s0:s1], dsum=None if dsm is None else dsm[s0:s1],
                                    tab=tab[s0:s1], ws=ws)
            self._timed("trace_stats", 0.0, run)
            return (tab, det, dsm) if detail else tab
