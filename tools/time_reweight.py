"""Timing of down-weighted or dropped data rows against whole steps -> profiles/reweight.json.

    timeout -k 10 900 python tools/time_reweight.py [--reps 3] [--folds 60] [--sizes 64] [--out profiles/reweight.json]

On the headline survey (tests/golden/oracle64_sample_matern32.npz; oracle32_matern32.npz at 32), in one process, wall-clock with the
device drained, `reps` runs after one warm-up:
  * the preview of one hole (the drill rows of one voxel column) and of one station, with cubes and statistics only, with the
    preview's split by its timed stages;
  * fold_influence over `folds` folds (the holes first, then stations);
  * the committed step (one hole dropped) against the same step with every scale at one and against the step with the attribute
    absent, in alternation: a whole step is what a user paid before for the same answer (edit the data, step again), and the
    all-ones step has to stay within the run-to-run spread of the plain one.
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

from time_campaign import survey      # noqa: E402  (the same surveys)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def measure(n, reps, nfolds):
    from geobo_amd import crossval
    inv, _ = survey(n)
    eng = inv.engine
    N, Ms = eng.N, eng.Ms
    step = lambda: inv._run(inv.gp_amp, inv.gp_length, None, True, True)
    step()
    out = dict(grid=[n, n, n], route=eng.step_route, rows=int(2 * eng.Ms_pad + len(inv._sel)), factor_rows=int(eng.last["step"].M_pad))
    holes = crossval._hole_runs(inv._sel, eng.nz, Ms)
    hole = max(holes, key=len)[:128]
    station = np.array([Ms // 2 + 3])
    prev = {}
    # (the headline survey's drill rows are scattered voxels: the k = 64 case is a patch of 8 x 8 gravity stations)
    patch = (np.arange(8)[:, None] * eng.nx + np.arange(8)[None, :]).reshape(-1) + (eng.ny // 2) * eng.nx + eng.nx // 2
    for name, rows in (("hole", hole), ("station", station), ("patch64", patch)):
        for want in ("cubes", "stats"):
            eng.reweight_preview(rows, np.inf, want=want)
            prev["%s_%s_ms" % (name, want)] = [wall(lambda: eng.reweight_preview(rows, np.inf, want=want))[0] for _ in range(reps)]
        prev[name + "_k"] = int(len(rows))
    eng.kernel_events = []
    eng.reweight_preview(patch, np.inf)
    torch.cuda.synchronize()
    split = {}
    for name, _, _, _, e0, e1 in eng.kernel_events:
        split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
    eng.kernel_events = None
    prev["patch64_split_ms"], prev["source"] = split, eng.set_source
    out["preview"] = prev
    folds = ([np.asarray(h)[:128] for h in holes] + [np.array([i]) for i in range(0, 2 * Ms, max(1, 2 * Ms // nfolds))])[:nfolds]
    inv.fold_influence(folds[:2])
    out["fold_influence"] = dict(folds=len(folds), ms=[wall(lambda: inv.fold_influence(folds))[0] for _ in range(reps)])
    # ---- the committed step against the step with every scale at one and the plain step, in alternation ---------------------------
    per_voxel = np.ones(N)
    per_voxel[inv._sel[hole - 2 * Ms]] = np.inf
    modes = dict(plain=None, ones=dict(grav=np.ones(Ms), magn=np.ones(Ms), drill=np.ones(N)),
                 dropped=dict(grav=np.ones(Ms), magn=np.ones(Ms), drill=per_voxel))
    runs = {m: [] for m in modes}
    for rep in range(reps + 1):
        for m, scales in modes.items():
            eng.row_scale = scales
            t = wall(step)[0]
            if rep:
                runs[m].append(t)
    eng.row_scale = None
    step()
    out["step"] = dict(plain_ms=runs["plain"], all_ones_ms=runs["ones"], hole_dropped_ms=runs["dropped"],
                       spread_ms={m: max(v) - min(v) for m, v in runs.items()},
                       note="whole steps with the likelihood, the mean and the variance, host read-back included; plain: the attribute "
                            "absent -- the launches of the parent commit's step, what editing the data and stepping again cost")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--folds", type=int, default=60)
    ap.add_argument("--sizes", default="64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reweight.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0))
    for n in [int(v) for v in a.sizes.split(",")]:
        res[str(n)] = measure(n, a.reps, a.folds)
        print(json.dumps(res[str(n)], indent=1), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
