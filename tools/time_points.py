"""Timing of the prediction at arbitrary points -> profiles/points.json.

    timeout -k 10 900 python tools/time_points.py [--reps 5] [--out profiles/points.json]

In one process, medians of `reps` after a warm-up:
  * Inversion.predict_points at the 64^3 headline survey (tests/golden/oracle64_sample_matern32.npz; Matern-3/2) for Q = 256, 4096 and
    32768 uniform points: milliseconds per stage (points_ak, points_reduce) from the engine's kernel events, the executed flop and the
    rate of the fused product, the whole call against the step with the mean and variance; Q = 256 also with the joint covariance;
  * geobo_ak_points and geobo_ak_fused back to back on one operand set (R_pad = 4096, N_pad = 262144, 4096 columns; Matern-3/2 self
    block): every repeat of both, so that the difference can be read against the spread of geobo_ak_fused's own repeats.
Every run of this tool belongs under its own `timeout -k 10 <s>` (it starts a GPU process and ends with it)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_campaign import survey, timed  # noqa: E402

QS = (256, 4096, 32768)


def events(eng, fn):
    """Milliseconds and executed flop per stage name of one call."""
    eng.kernel_events = []
    fn()
    torch.cuda.synchronize()
    ms, flop = {}, {}
    for name, fl, _, _, e0, e1 in eng.kernel_events:
        ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
        flop[name] = flop.get(name, 0.0) + fl
    eng.kernel_events = None
    return ms, flop


def measure_calls(reps, qs):
    inv, _ = survey(64)
    eng, s = inv.engine, inv.settings
    t_step_mv = timed(lambda: inv._run(inv.gp_amp, inv.gp_length, None, False, True), reps)
    inv._run(inv.gp_amp, inv.gp_length, None, False, False)
    rng = np.random.default_rng(0)
    lo, hi = np.array([0.0, 0.0, s.zmax - s.zLcube]), np.array([s.xLcube, s.yLcube, s.zmax])
    out = dict(grid=[64, 64, 64], route=eng.step_route, rows=int(2 * eng.Ms_pad + len(inv._sel)), step_with_mean_var_ms=t_step_mv, Q={})
    for Q in qs:
        pts = lo + rng.uniform(0.0, 1.0, (Q, 3)) * (hi - lo)
        inv.predict_points(pts)
        runs = [events(eng, lambda: inv.predict_points(pts)) for _ in range(reps)]
        med = lambda name: float(np.median([r[0][name] for r in runs]))
        flop = runs[0][1]
        rec = dict(points_ak_ms=med("points_ak"), points_reduce_ms=med("points_reduce"), points_ak_flop=flop["points_ak"],
                   points_ak_TFps=flop["points_ak"] / (med("points_ak") * 1e-3) / 1e12,
                   points_reduce_TFps=flop["points_reduce"] / (med("points_reduce") * 1e-3) / 1e12,
                   call_ms=timed(lambda: inv.predict_points(pts), reps))
        rec["call_over_step"] = rec["call_ms"] / t_step_mv
        if Q <= 256:
            inv.predict_points(pts, full_cov=True)
            cov = [events(eng, lambda: inv.predict_points(pts, full_cov=True)) for _ in range(reps)]
            rec["points_cov_ms"] = float(np.median([r[0]["points_cov"] for r in cov]))
            rec["call_full_cov_ms"] = timed(lambda: inv.predict_points(pts, full_cov=True), reps)
        out["Q"][str(Q)] = rec
        print(json.dumps({str(Q): rec}, indent=1), flush=True)
    del inv
    torch.cuda.empty_cache()
    return out


def measure_kernels(reps, R=4096, N=262144, nq=4096):
    """geobo_ak_points against geobo_ak_fused: the same A, the same contraction points, 4096 columns each -- the first 4096 voxels for
    the fused entry, as many uniform points for the new one; interleaved repeats, each timed by its own event pair."""
    from geobo_amd import hip
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    A = torch.randn((R, N + 16), dtype=torch.float64, device=dev, generator=g)[:, :N]
    ax = np.arange(1, 65) * 100.0
    X, Y, Z = np.meshgrid(ax, ax, ax)
    xyz = tuple(hip.to_dev(v.ravel(), dev) for v in (X, Y, Z))
    q = tuple(100.0 + 6300.0 * torch.rand(nq, dtype=torch.float64, device=dev, generator=g) for _ in range(3))
    out = torch.empty((R, nq + 16), dtype=torch.float64, device=dev)[:, :nq]
    kid = hip.kernel_id("matern32", False)
    fused = lambda: hip.ak_fused(kid, A, xyz, 0, nq, 200.0, 200.0, 1.0, 1.0, out)
    points = lambda: hip.ak_points(kid, A, xyz, q, 200.0, 200.0, 1.0, 1.0, out)
    series = dict(ak_fused_ms=[], ak_points_ms=[])
    fused()
    points()
    for _ in range(reps):
        series["ak_fused_ms"].append(timed(fused, 1, warm=0))
        series["ak_points_ms"].append(timed(points, 1, warm=0))
    flop = 2.0 * R * N * nq
    f, p = np.array(series["ak_fused_ms"]), np.array(series["ak_points_ms"])
    series.update(R_pad=R, N_pad=N, nq_pad=nq, kernel="matern32", flop=flop, ak_fused_median_ms=float(np.median(f)),
                  ak_points_median_ms=float(np.median(p)), ak_fused_spread_ms=float(f.max() - f.min()),
                  ak_fused_TFps=flop / (np.median(f) * 1e-3) / 1e12, ak_points_TFps=flop / (np.median(p) * 1e-3) / 1e12,
                  difference_of_medians_ms=float(np.median(p) - np.median(f)))
    return series


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qs", default=",".join(str(q) for q in QS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0),
               note="stage times: HIP events around the engine's launches, medians; kernels: every repeat, fused and points interleaved")
    res["kernels"] = measure_kernels(a.reps)
    print(json.dumps(res["kernels"], indent=1), flush=True)
    res["predict_points_64"] = measure_calls(a.reps, [int(v) for v in a.qs.split(",")])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
