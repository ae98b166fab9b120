"""Timing of the drill-intercept statistics -> profiles/intercepts.json.

    timeout -k 10 900 python tools/time_intercepts.py [--reps 2] [--out profiles/intercepts.json]

The configuration of sections 17 and 18: 64^3 on the sampling survey (tests/golden/oracle64_sample_matern32.npz, Matern-3/2, weights
(0.2, 0.2, 0.2)), C = 16 cutoffs on the density, batches of 64 realisations, n = 256, one process, medians after a warm-up:
  * geobo_trace_stats on one batch, every column of the cube, by device events: with all maps and both histograms, without the
    histograms, with nothing but tab, with the per-hole tables, each for max_gap 0 and 2 (min_len 3); the bytes the algorithm needs
    (one property of the batch) and the rate they give; beside them the time to produce that batch (prior draw and conditioning,
    host clock ended by a synchronise) and the share the reduction has of it;
  * the same kernel on a 64 x 64 x 16 grid (columns of a quarter wave), cut out of the same batch;
  * drill_intercepts(n = 256) end to end;
  * the host route: sample_posterior(256) and a NumPy loop down the columns (vectorised over the columns of a realisation, one
    pass per cutoff and depth) for thickness, depth to top and the longest run, with the same outputs at max_gap 0.
Every run of this tool belongs under its own `timeout -k 10 <s>` (it starts a GPU process and ends with it)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_campaign import timed  # noqa: E402
from time_gradetonnage import survey64, wall  # noqa: E402

STREAM_TBPS = 6.29                   # measured HBM stream rate of the device (float4 copy)
# what was measured earlier with this tool and dropped (recorded figures, MI355X; not re-measured by a run)
TRIED = {
 "wave_uniform_run_loop": {
  "what": "the first form: the run loop once per cutoff on scalar registers, wave-uniform, the carries of cutoff c read from lane c by v_readlane and written back under lane == c; the same results bit for bit (the same tests passed)",
  "columns_64x64x64_ms": {
   "maps_and_histograms_gap0": 3.0284,
   "maps_gap0": 3.0114,
   "tab_only_gap0": 2.7847,
   "maps_histograms_detail_gap0": 3.4332,
   "maps_and_histograms_gap2": 2.822,
   "maps_gap2": 2.8097,
   "tab_only_gap2": 2.5927,
   "maps_histograms_detail_gap2": 3.2156
  },
  "columns_64x64x16_ms": {
   "maps_and_histograms_gap0": 1.341,
   "maps_gap0": 1.3218,
   "tab_only_gap0": 1.1241,
   "maps_histograms_detail_gap0": 1.7985,
   "maps_and_histograms_gap2": 1.2882,
   "maps_gap2": 1.2725,
   "tab_only_gap2": 1.0769,
   "maps_histograms_detail_gap2": 1.7493
  },
  "batch_sampling_ms": 2247.7,
  "share_of_batch_sampling_64x64x64": 0.001347,
  "dropped_because": "4 waves per SIMD each spend a sample on 16 dependent chains of scalar instructions; one lane per cutoff runs the 16 chains side by side as vector code: 3.03 -> 0.78 ms with maps and histograms"
 },
 "packed_columns": {
  "what": "64 / L columns per wave for short traces, run masks cut at the segment borders",
  "not_built_because": "the criterion for it (reduction above 10 % of producing the batch at 64^3 or 64 x 64 x 16) is missed by a factor of about 300 and 80"
 }
}


def host_route(inv, cut, n, seed, min_len):
    """What a user does without the device reduction: every realisation to the host, then NumPy down the columns."""
    s = inv.settings
    ny, nx, nz = s.yNcube, s.xNcube, s.zNcube
    cubes = inv.sample_posterior(n, seed=seed)[0].reshape(n, ny, nx, nz)
    holes_hit = np.empty((n, cut.size), dtype=np.int64)
    count = np.empty((n, cut.size), dtype=np.int64)
    hits = np.zeros((cut.size, ny, nx), dtype=np.int64)
    top_sum = np.zeros((cut.size, ny, nx), dtype=np.int64)
    acc = np.zeros((cut.size, ny, nx))
    for k in range(n):
        for c, t in enumerate(cut):
            ore = cubes[k] >= t
            thick = ore.sum(-1)
            best = np.zeros((ny, nx), dtype=np.int64)
            run = np.zeros((ny, nx), dtype=np.int64)
            for z in range(nz):
                run = (run + 1) * ore[:, :, z]
                np.maximum(best, run, out=best)
            hit = best >= min_len
            holes_hit[k, c], count[k, c] = hit.sum(), thick.sum()
            hits[c] += hit
            top_sum[c] += np.where(thick > 0, ore.argmax(-1), 0)
            acc[c] += np.where(ore, cubes[k], 0.0).sum(-1)
    return holes_hit, count, hits / float(n), top_sum, acc


def kernel_times(F, grid, t_norm, reps, label, out):
    from geobo_amd import hip
    S, C = F.shape[0], t_norm.size
    K, L = grid[0] * grid[1], grid[2]
    ws = torch.empty(hip.trace_stats_ws_doubles(S, K, C), dtype=torch.float64, device=F.device)
    tab = torch.empty((S, C, 3), dtype=torch.int64, device=F.device)
    full = hip.trace_maps(C, K, L, device=F.device)
    nohist = {k: v for k, v in full.items() if not k.startswith("hist")}
    detail = torch.empty((S, C, K, 6), dtype=torch.int32, device=F.device)
    dsum = torch.empty((S, C, K, 2), dtype=torch.float64, device=F.device)
    nbytes = 8.0 * S * K * L                                       # one property of the batch
    rec = out[label] = dict(grid=list(grid), bytes=nbytes, kernels={})
    for gap in (0, 2):
        for name, kw in (("maps_and_histograms", dict(maps=full)), ("maps", dict(maps=nohist)), ("tab_only", dict()),
                         ("maps_histograms_detail", dict(maps=full, detail=detail, dsum=dsum))):
            ms = timed(lambda: hip.trace_stats(F, grid, 0, t_norm, min_len=3, max_gap=gap, tab=tab, ws=ws, **kw), 4 * reps, warm=2)
            rec["kernels"]["%s_gap%d" % (name, gap)] = dict(ms=ms, TBps=nbytes / (ms * 1e-3) / 1e12,
                                                           share_of_stream_rate=nbytes / (ms * 1e-3) / 1e12 / STREAM_TBPS)
    return rec


def measure(reps, S=64, C=16, n=256):
    inv = survey64()
    eng = inv.engine
    N, grid = eng.N, (64, 64, 64)
    mean = inv.mu_rec.reshape(3, N)[0]
    t_norm = np.quantile(mean, np.linspace(0.05, 0.95, C))
    cut = t_norm * float(inv._cube_scale[0])
    out = dict(route=eng.step_route, batch=S, cutoffs=C, realisations=n, min_len=3, stream_rate_TBps=STREAM_TBPS)

    def one_batch():
        return next(iter(inv._posterior_batches(S, seed=3)))[0]
    out["batch_sampling_ms"] = wall(one_batch, reps)               # prior draw + conditioning of the batch the kernel runs on
    F = one_batch()
    r64 = kernel_times(F, grid, t_norm, reps, "columns_64x64x64", out)
    # a flat grid: the first 64 x 64 x 16 voxels of each property of the same batch, columns of 16 (a quarter of a wave)
    flat = (64, 64, 16)
    r16 = kernel_times(F[:, :, :64 * 64 * 16], flat, t_norm, reps, "columns_64x64x16", out)
    for rec, share_of in ((r64, 1.0), (r16, 0.25)):                # (the flat grid holds a quarter of the voxels: a quarter of the batch)
        worst = max(v["ms"] for k, v in rec["kernels"].items() if "detail" not in k)
        rec["worst_ms_without_detail"] = worst
        rec["share_of_batch_sampling"] = worst / (out["batch_sampling_ms"] * share_of)
    r16["note"] = "share against a quarter of the 64^3 batch time: this grid has no survey of its own"
    del F
    out["drill_intercepts_ms"] = wall(lambda: inv.drill_intercepts(cut, prop="density", n=n, seed=5, min_length=300.0), reps)
    out["drill_intercepts_gap2_ms"] = wall(lambda: inv.drill_intercepts(cut, prop="density", n=n, seed=5, min_length=300.0, max_gap=200.0), 1)
    t0 = time.perf_counter()                                       # (once: sample_posterior is warm by now, NumPy needs no warm-up)
    host_route(inv, cut, n, 5, 3)
    torch.cuda.synchronize()
    out["host_route_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    inv.sample_posterior(n, seed=5)
    out["host_route_sample_posterior_ms"] = (time.perf_counter() - t0) * 1e3
    out["host_route_over_device_route"] = out["host_route_ms"] / out["drill_intercepts_ms"]
    # the two routes see the same intercepts
    dev = inv.drill_intercepts(cut, prop="density", n=4, seed=5, min_length=300.0)
    host = host_route(inv, cut, 4, 5, 3)
    out["routes_agree"] = bool(np.array_equal(dev["holes_hit"], host[0]) and np.array_equal(dev["count"], host[1])
                               and np.array_equal(dev["probability"], host[2]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intercepts.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0),
               note="kernels: device events around one geobo_trace_stats call (trace kernel and finish kernel) on a batch of 64 realisations "
                    "x 16 cutoffs, every column of the grid, min_len 3; bytes = one property of the batch; batch_sampling, drill_intercepts "
                    "and host route: host clock around the call, ended by a device synchronise; the host route runs once, max_gap 0")
    res["64"] = measure(a.reps)
    res["tried_and_dropped"] = TRIED
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
