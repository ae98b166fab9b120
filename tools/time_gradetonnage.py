"""Timing of the grade-tonnage reductions -> profiles/gradetonnage.json.

    timeout -k 10 900 python tools/time_gradetonnage.py [--reps 3] [--out profiles/gradetonnage.json]

At 64^3 on the sampling survey (tests/golden/oracle64_sample_matern32.npz, Matern-3/2, weights (0.2, 0.2, 0.2): a PSD prior), C = 16
cutoffs on the density and n = 256 realisations, in one process, medians of `reps` after a warm-up:
  * geobo_cutoff_stats alone on a batch of 64 realisations (with and without the hits cubes, and with one lower bound, which reads
    a second property), and geobo_box_means for the boxes (1, 1, 1), (4, 4, 4), (16, 16, 16): device events, bytes the algorithm
    needs (the property slices read, the hits and means written) and the rate they give;
  * grade_tonnage(n = 256) end to end, at voxel support with the probability cubes and at block support (4, 4, 4);
  * the host route: sample_posterior(256) and the NumPy thresholding of tests/_gradetonnage_ref.py's rule, cutoff by cutoff, with the
    same outputs (counts, sums, probability cubes).
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

BOXES = ((1, 1, 1), (4, 4, 4), (16, 16, 16))


def survey64():
    from geobo_amd.config_loader import Settings
    from geobo_amd.inversion import Inversion
    f = dict(np.load(os.path.join(ROOT, "tests", "golden", "oracle64_sample_matern32.npz")))
    n = 64
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc="matern32",
                      gp_coeff=[0.2, 0.2, 0.2]))
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    inv = Inversion(settings=s)
    inv.create_cubegeometry()
    inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    return inv


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_route(inv, cut, n, seed):
    """What a user does without the device reductions: every realisation to the host, then NumPy, cutoff by cutoff."""
    cubes = inv.sample_posterior(n, seed=seed)[0].reshape(n, -1)
    cnt = np.empty((n, cut.size), dtype=np.int64)
    tot = np.empty((n, cut.size))
    prob = np.empty((cut.size, cubes.shape[1]))
    for c, t in enumerate(cut):
        passes = cubes >= t
        cnt[:, c] = passes.sum(1)
        tot[:, c] = np.where(passes, cubes, 0.0).sum(1)
        prob[c] = passes.mean(0)
    return cnt, tot, prob


def measure(reps, S=64, C=16, n=256):
    from geobo_amd import hip
    inv = survey64()
    eng = inv.engine
    N, grid = eng.N, (64, 64, 64)
    mean = inv.mu_rec.reshape(3, N)[0]
    t_norm = np.quantile(mean, np.linspace(0.05, 0.95, C))
    cut = t_norm * float(inv._cube_scale[0])
    F = next(iter(inv._posterior_batches(S, seed=3)))[0]
    out = dict(grid=list(grid), route=eng.step_route, batch=S, cutoffs=C, realisations=n, kernels={})
    ws = torch.empty(hip.cutoff_stats_ws_doubles(S, N, C), dtype=torch.float64, device=eng.device)
    hits = torch.zeros((C, N), dtype=torch.int32, device=eng.device)

    def rec(name, fn, nbytes):
        ms = timed(fn, 4 * reps, warm=2)
        out["kernels"][name] = dict(ms=ms, bytes=nbytes, TBps=nbytes / (ms * 1e-3) / 1e12)
    rec("cutoff_stats", lambda: hip.cutoff_stats(F, 0, t_norm, ws=ws), 8.0 * S * N)
    rec("cutoff_stats_hits", lambda: hip.cutoff_stats(F, 0, t_norm, hits=hits, ws=ws), 8.0 * S * N + 8.0 * C * N)
    rec("cutoff_stats_lower_bound", lambda: hip.cutoff_stats(F, 0, t_norm, lo=[-np.inf, 0.0, -np.inf], ws=ws), 16.0 * S * N)
    for box in BOXES:
        nblocks = int(np.prod([-(-g // b) for g, b in zip(grid, box)]))
        G = torch.empty((S, 3, nblocks), dtype=torch.float64, device=eng.device)
        cnt = torch.empty(nblocks, dtype=torch.int32, device=eng.device)
        rec("box_means_" + "x".join(str(b) for b in box), lambda: hip.box_means(F, grid, box, G=G, count=cnt), 24.0 * S * (N + nblocks))
    del F
    out["grade_tonnage_ms"] = wall(lambda: inv.grade_tonnage(cut, prop="density", n=n, seed=5, voxel_probability=True), reps)
    out["grade_tonnage_block_4x4x4_ms"] = wall(lambda: inv.grade_tonnage(cut, prop="density", n=n, seed=5, block=(4, 4, 4)), reps)
    out["host_route_ms"] = wall(lambda: host_route(inv, cut, n, 5), reps)
    t0 = time.perf_counter()
    inv.sample_posterior(n, seed=5)
    out["host_route_sample_posterior_ms"] = (time.perf_counter() - t0) * 1e3
    # the two routes count the same voxels
    dev = inv.grade_tonnage(cut, prop="density", n=16, seed=5)
    out["counts_agree"] = bool(np.array_equal(dev["count"], host_route(inv, cut, 16, 5)[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradetonnage.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0),
               note="kernels: device events around one call on a batch of 64 realisations, bytes = what the algorithm reads and writes; "
                    "grade_tonnage and host route: host clock around the call, ended by a device synchronise")
    res["64"] = measure(a.reps)
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
