"""Timing of the cross-validation of the fit -> profiles/crossval.json.

    timeout -k 10 900 python tools/time_crossval.py [--reps 5] [--out profiles/crossval.json]

At 32^3 and 64^3 on the headline surveys (tests/golden/oracle32_matern32.npz, oracle64_sample_matern32.npz; Matern-3/2) with eight whole
z-columns added to the drill data (so that "holes" has folds of nz rows), in one process, medians after a warm-up:
  * geobo_kinv_diag alone: time, bytes (the lower triangle of L^-1 once: 8 M (M + 1) / 2) and the fraction of a 5 TB/s stream;
  * the geobo_set_gram and geobo_set_loo launches of "holes" and "patches" (device events around the launches of one call);
  * the engine call (PosteriorEngine.cross_validate on prebuilt folds: launches and the scatter of the results, no read-back) and the
    whole Inversion.cross_validate call (fold building, read-back, units, summary) for each fold kind;
  * the step without mean and variance and the likelihood step (what calc_logl runs) at the headline lengths on the same box, and
    the ratio of cross_validate("loo") to the likelihood step.  calc_logl's and calc_cv's 5-parameter form puts two equal lengths into
    the Matern cross term (0/0: both return inf), so that pair is timed on the same data with the exp kernel (`exp_objectives`), by
    device events and by the host clock, after checking that calc_cv is finite and equals minus summary.logp of cross_validate("holes")
    at the same parameters; beside it the host time of the "holes" fold table and the engine call on it.
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

from geobo_amd.crossval import fold_table  # noqa: E402

STREAM = 5.0e12       # B/s, sustained HBM stream (profiles/r05_hbm_copy_runs.txt)
KINDS = ("loo", "holes", "patches")


def timed(fn, reps, warm=1, wall=False):
    """Median of device events around fn; wall=True: also the median of the host clock from the call to the device's last work."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts, ws = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ws.append(1e3 * (time.perf_counter() - t0))
        ts.append(e0.elapsed_time(e1))
    return (float(np.median(ts)), float(np.median(ws))) if wall else float(np.median(ts))


def wall_only(fn, reps):
    """Median host time of a function that does not touch the device."""
    ws = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        ws.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ws[1:]))


def survey(n, kern):
    from geobo_amd.config_loader import Settings
    from geobo_amd.inversion import Inversion
    name = "oracle32_matern32.npz" if n == 32 else "oracle64_sample_matern32.npz"
    f = dict(np.load(os.path.join(ROOT, "tests", "golden", name)))
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc=kern))
    rng = np.random.default_rng(n)
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    for iy, ix in zip(rng.choice(n - 2, 8, replace=False) + 1, rng.choice(n - 2, 8, replace=False) + 1):
        d0[iy, ix, :] = rng.standard_normal(n) * f["drillvalues"].std() + f["drillvalues"].mean()
    inv = Inversion(settings=s)
    inv.create_cubegeometry()
    if kern == "matern32":
        inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    torch.cuda.synchronize()
    return inv


def launches(eng, folds, reps):
    """Median device time of the cv_* launches of one engine call, by name."""
    runs = []
    for _ in range(reps):
        eng.kernel_events = []
        eng.cross_validate(folds)
        torch.cuda.synchronize()
        acc = {}
        for name, _, _, _, e0, e1 in eng.kernel_events:
            acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1)
        acc["launches"] = len(eng.kernel_events)
        runs.append(acc)
        eng.kernel_events = None
    return {k: float(np.median([r.get(k, 0.0) for r in runs])) for k in ("cv_diag", "cv_gram", "cv_loo", "launches")}


def objectives(n, reps):
    """calc_logl and calc_cv("holes") in their 5-parameter form, on the same data with the exp kernel; the value of calc_cv is checked
    against cross_validate("holes") at the same parameters before anything is timed."""
    inv = survey(n, "exp")
    xv = inv.settings.xvoxsize
    params = np.r_[inv.gp_amp, float(np.asarray(inv.gp_length, dtype=float)[0]) / xv, inv.coeffm]
    logl, cv = inv.calc_logl(params), inv.calc_cv(params)
    want = -inv.cross_validate("holes")["summary"]["logp"]
    assert np.isfinite(logl) and np.isfinite(cv), (logl, cv)
    assert abs(cv - want) <= 1e-10 * abs(want), (cv, want)
    table = fold_table(inv._cv_folds("holes", None), inv.Fs3.size)
    out = dict(route=inv.engine.step_route, calc_logl=float(logl), calc_cv_holes=float(cv))
    out["step_ms"], out["step_wall_ms"] = timed(lambda: inv._run(inv.gp_amp, inv.gp_length, None, False, False), reps, wall=True)
    out["calc_logl_ms"], out["calc_logl_wall_ms"] = timed(lambda: inv.calc_logl(params), reps, wall=True)
    out["calc_cv_holes_ms"], out["calc_cv_holes_wall_ms"] = timed(lambda: inv.calc_cv(params), reps, wall=True)
    out["holes_table_ms"] = wall_only(lambda: fold_table(inv._cv_folds("holes", None), inv.Fs3.size), reps)
    out["holes_engine_call_ms"] = timed(lambda: inv.engine.cross_validate(table), reps)
    out["calc_cv_over_calc_logl"] = out["calc_cv_holes_wall_ms"] / out["calc_logl_wall_ms"]
    return out


def measure(n, reps):
    from geobo_amd import hip
    inv = survey(n, "matern32")
    eng = inv.engine
    Linv, u = eng.last["Linv"], eng.last["u"]
    M_pad = Linv.shape[0]
    ws = torch.empty(hip.kinv_diag_ws_doubles(M_pad), dtype=torch.float64, device=eng.device)
    t_diag = timed(lambda: hip.kinv_diag(Linv, u, ws=ws), max(reps, 9), warm=2)
    diag_bytes = 8.0 * M_pad * (M_pad + 1) / 2
    out = dict(grid=[n, n, n], route=eng.step_route, rows=int(inv.Fs3.size), M_pad=int(M_pad), drill_rows=int(inv._sel.size),
               kinv_diag=dict(ms=t_diag, bytes=diag_bytes, frac_stream=diag_bytes / (t_diag * 1e-3) / STREAM))
    for kind in KINDS:
        folds = inv._cv_folds(kind, None)
        sizes = np.array([len(B) for B in folds])
        r = eng.cross_validate(folds)                               # warm-up
        assert int(r["status"].abs().max()) == 0 and bool(torch.isfinite(r["logp"]).all())
        ev = launches(eng, folds, reps)
        out[kind] = dict(folds=int(sizes.size), folds_over_one_row=int((sizes > 1).sum()), largest=int(sizes.max()),
                         set_gram_ms=ev["cv_gram"], set_loo_ms=ev["cv_loo"], kinv_diag_ms=ev["cv_diag"], timed_launches=int(ev["launches"]),
                         engine_call_ms=timed(lambda: eng.cross_validate(folds), reps),
                         cross_validate_ms=timed(lambda: inv.cross_validate(kind), reps))
    # the step calc_logl runs, at the headline lengths (the 5-parameter form itself is inf with matern32, see above)
    L = np.array(inv.gp_length, dtype=float)
    r = inv._run(inv.gp_amp, L.copy(), None, True, False)
    assert np.isfinite(r["uu"] + r["logdet"])
    out["step_ms"] = timed(lambda: inv._run(inv.gp_amp, L.copy(), None, False, False), reps)
    out["likelihood_step_ms"] = timed(lambda: inv._run(inv.gp_amp, L.copy(), None, True, False), reps)
    out["loo_over_likelihood_step"] = out["loo"]["cross_validate_ms"] / out["likelihood_step_ms"]
    out["loo_engine_call_over_likelihood_step"] = out["loo"]["engine_call_ms"] / out["likelihood_step_ms"]
    del inv, eng, Linv, u, r
    torch.cuda.empty_cache()
    out["exp_objectives"] = objectives(n, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossval.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), stream_Bps=STREAM)
    for n in [int(v) for v in a.sizes.split(",")]:
        res[str(n)] = measure(n, a.reps)
        print(json.dumps(res[str(n)], indent=1), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
