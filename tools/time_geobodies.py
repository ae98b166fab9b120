"""Timing of the connected-body labelling and statistics -> profiles/geobodies.json.

    timeout -k 10 900 python tools/time_geobodies.py [--reps 2] [--out profiles/geobodies.json]

The configuration of section 17: 64^3 on the sampling survey (tests/golden/oracle64_sample_matern32.npz, Matern-3/2, weights (0.2, 0.2,
0.2)), C = 16 cutoffs on the density, batches of 64 realisations, n = 256, one process, medians after a warm-up:
  * the stages of geobo_bodies on one batch (init, merge -- plain and with its tile-local LDS phase --, flatten, statistics with both
    hit cubes) for 6 and 26 neighbours: device
    events around each stage of each launch the engine's cut gives, added up over the batch; beside them the time to produce that
    batch (prior draw and conditioning), host clock ended by a synchronise, and the share labelling + statistics have of it;
  * geobodies(n = 256) end to end for 6 and 26 neighbours with both probability cubes;
  * the host route: sample_posterior(256) and scipy.ndimage.label per realisation and cutoff, with the same outputs.
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

from time_gradetonnage import survey64, wall  # noqa: E402

STAGES = ("init", "merge", "flatten", "statistics")


def stage_times(eng, F, t_norm, neighbours, seeds, reps, tiled):
    """Median over reps of the per-stage device time of one batch, ms, the launches of the engine's cut added up."""
    from geobo_amd import geobodies as gb, hip
    S, _, N = F.shape
    C = t_norm.size
    grid = (eng.ny, eng.nx, eng.nz)
    Sl, Cl = gb.launch_cuts(S, C, N)
    ws = torch.empty(hip.bodies_ws_doubles(Sl, grid, Cl), dtype=torch.float64, device=F.device)
    hl = torch.zeros((C, N), dtype=torch.int32, device=F.device)
    hs = torch.zeros((C, N), dtype=torch.int32, device=F.device)
    info = torch.zeros(1, dtype=torch.int32, device=F.device)
    runs = []
    for _ in range(reps + 1):
        marks = []
        for s0 in range(0, S, Sl):
            for c0 in range(0, C, Cl):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
                ev[0].record()
                for k, phase in enumerate((hip.BODIES_INIT, hip.BODIES_MERGE, hip.BODIES_FLATTEN, hip.BODIES_STATS)):
                    hip.bodies(F[s0:s0 + Sl], grid, 0, t_norm[c0:c0 + Cl], neighbours=neighbours, seeds=seeds, hits_largest=hl[c0:c0 + Cl],
                               hits_seeded=hs[c0:c0 + Cl], info=info, ws=ws, phases=phase, tiled=tiled)
                    ev[k + 1].record()
                marks.append(ev)
        torch.cuda.synchronize()
        runs.append([sum(ev[k].elapsed_time(ev[k + 1]) for ev in marks) for k in range(4)])
    assert int(info.item()) == 0
    med = np.median(np.array(runs[1:]), axis=0)                  # (the first run is the warm-up)
    return {name: float(v) for name, v in zip(STAGES, med)}, (Sl, Cl)


def host_route(inv, cut, n, seed, neighbours, seeds):
    """What a user does without the device labelling: every realisation to the host, then SciPy, volume by volume."""
    from scipy import ndimage
    s = inv.settings
    grid = (s.yNcube, s.xNcube, s.zNcube)
    structure = ndimage.generate_binary_structure(3, 1 if neighbours == 6 else 3)
    cubes = inv.sample_posterior(n, seed=seed)[0].reshape((n,) + grid)
    n_bodies = np.empty((n, cut.size), dtype=np.int64)
    largest = np.empty((n, cut.size), dtype=np.int64)
    seeded = np.empty((n, cut.size), dtype=np.int64)
    p_l, p_s = np.zeros((cut.size,) + grid), np.zeros((cut.size,) + grid)
    for k in range(n):
        for c, t in enumerate(cut):
            lab, B = ndimage.label(cubes[k] >= t, structure=structure)
            size = np.bincount(lab.reshape(-1), minlength=B + 1)
            size[0] = 0
            n_bodies[k, c] = B
            largest[k, c] = size.max() if B else 0
            if B:
                p_l[c] += lab == size.argmax()
            hit = np.unique(lab.reshape(-1)[seeds])
            member = np.isin(lab, hit[hit > 0])
            seeded[k, c] = member.sum()
            p_s[c] += member
    return n_bodies, largest, seeded, p_l / n, p_s / n


def measure(reps, S=64, C=16, n=256):
    inv = survey64()
    eng = inv.engine
    N, grid = eng.N, (64, 64, 64)
    mean = inv.mu_rec.reshape(3, N)[0]
    t_norm = np.quantile(mean, np.linspace(0.05, 0.95, C))
    cut = t_norm * float(inv._cube_scale[0])
    seeds = inv._drill_selection().astype(np.int32)
    out = dict(grid=list(grid), route=eng.step_route, batch=S, cutoffs=C, realisations=n, seeds=int(seeds.size))

    def one_batch():
        return next(iter(inv._posterior_batches(S, seed=3)))[0]
    out["batch_sampling_ms"] = wall(one_batch, reps)               # prior draw + conditioning of the batch the stages run on
    F = one_batch()
    for nb in (6, 26):
        rec = out["neighbours_%d" % nb] = {}
        for name, tiled in (("plain", False), ("tiled", True)):      # the merge without and with its tile-local phase in LDS
            stages, cuts = stage_times(eng, F, t_norm, nb, seeds, max(reps, 3), tiled)
            total = sum(stages.values())
            rec[name] = dict(stages_ms=stages, labelling_and_statistics_ms=total, share_of_batch_sampling=total / out["batch_sampling_ms"])
        rec["launch_cut"] = list(cuts)
    del F
    for nb in (6, 26):
        out["neighbours_%d" % nb]["geobodies_ms"] = wall(
            lambda: inv.geobodies(cut, prop="density", n=n, seed=5, neighbours=nb, seeds="drill", probability="both"), reps)
    t0 = time.perf_counter()                                       # (once: sample_posterior is warm by now, SciPy needs no warm-up)
    host_route(inv, cut, n, 5, 6, seeds)
    torch.cuda.synchronize()
    out["host_route_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    inv.sample_posterior(n, seed=5)
    out["host_route_sample_posterior_ms"] = (time.perf_counter() - t0) * 1e3
    # the two routes find the same bodies
    dev = inv.geobodies(cut, prop="density", n=4, seed=5, neighbours=6, seeds="drill", probability="both")
    host = host_route(inv, cut, 4, 5, 6, seeds)
    out["routes_agree"] = bool(np.array_equal(dev["n_bodies"], host[0]) and np.array_equal(dev["largest"]["count"], host[1])
                               and np.array_equal(dev["seeded"]["count"], host[2]) and np.array_equal(dev["probability_seeded"], host[4]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geobodies.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0),
               note="stages: device events around each stage of geobo_bodies on one batch of 64 realisations x 16 cutoffs (both hit cubes, the "
                    "drilled voxels as seeds), the launches of the engine's cut added up; batch_sampling, geobodies and host route: host "
                    "clock around the call, ended by a device synchronise; the host route labels with 6 neighbours and runs once")
    res["64"] = measure(a.reps)
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
