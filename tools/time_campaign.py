"""Timing of the per-hole information statistics -> profiles/campaign.json.

    timeout -k 10 900 python tools/time_campaign.py [--reps 3] [--out profiles/campaign.json]

At 32^3 and 64^3 on the headline surveys (tests/golden/oracle32_matern32.npz, oracle64_sample_matern32.npz; Matern-3/2), in one process:
  * the step (posterior() without the mean and variance, and cubing()'s step with them);
  * the table of every inner vertical hole (hole_statistics()), split into the V_d sweep (tiles of V_d through geobo_set_gram), the
    set_gram launches alone (timed on one stored tile of V_d rows, scaled to the rows of the sweep) and geobo_set_logdet;
  * one campaign hole (propose_drill_campaign(1): a step, a table, and the final step with the mean and variance and the restoring step);
  * rooflines of the two kernels: set_gram reads every row of V_d once (8 B per voxel of the holes) for 2 k^2 flop per row and set,
    of which the lower tiles run (kt (kt + 1) / 2 tiles of 16 x 16 of kt^2).
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

STREAM = 5.0e12       # B/s, sustained HBM stream (profiles/r05_hbm_copy_runs.txt)
F64_MFMA = 78.6e12    # flop/s, fp64 matrix peak of the part


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def survey(n):
    from geobo_amd.config_loader import Settings
    from geobo_amd.inversion import Inversion
    name = "oracle32_matern32.npz" if n == 32 else "oracle64_sample_matern32.npz"
    f = dict(np.load(os.path.join(ROOT, "tests", "golden", name)))
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc="matern32"))
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    inv = Inversion(settings=s)
    inv.create_cubegeometry()
    inv.gp_length = f["gp_length_in"].copy()
    t0 = time.perf_counter()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    torch.cuda.synchronize()
    return inv, (time.perf_counter() - t0) * 1e3


def measure(n, reps):
    from geobo_amd import hip
    from geobo_amd.campaign import vertical_sets
    inv, t_first = survey(n)
    eng = inv.engine
    t_step = timed(lambda: inv._run(inv.gp_amp, inv.gp_length, None, False, False), reps)
    t_step_mv = timed(lambda: inv._run(inv.gp_amp, inv.gp_length, None, False, True), reps)
    t_table = timed(lambda: inv.hole_statistics(), reps)
    eng.kernel_events = []
    inv.hole_statistics()
    torch.cuda.synchronize()
    ev = {name: e0.elapsed_time(e1) for name, _, _, _, e0, e1 in eng.kernel_events}
    eng.kernel_events = None
    sets, _ = vertical_sets(n, n, n)
    C, k = sets.shape
    Mv = 2 * eng.Ms_pad + len(inv._sel)
    idx = torch.as_tensor(sets.astype(np.int32), device=eng.device)
    V = torch.randn((256, eng.N + 16), dtype=torch.float64, device=eng.device)[:, :eng.N]
    G = torch.empty((C, k, k), dtype=torch.float64, device=eng.device)
    t_tile = timed(lambda: hip.set_gram(idx, V, 256, G, accumulate=True, ncols=eng.N), reps)
    t_gram = t_tile * Mv / 256.0
    kt = (k + 15) // 16
    gram_bytes = 8.0 * Mv * C * k
    gram_flop = 2.0 * Mv * C * (16 * 16) * kt * (kt + 1) / 2
    t_hole = timed(lambda: inv.propose_drill_campaign(1), 1, warm=0)
    return dict(
        grid=[n, n, n], route=eng.step_route, source=eng.set_source, holes=int(C), k=int(k), rows=int(Mv),
        first_cubing_ms=t_first, step_ms=t_step, step_with_mean_var_ms=t_step_mv,
        table_ms=t_table, table_over_step=t_table / t_step,
        split_ms=dict(vd_sweep_incl_gram=ev.get("set_sweep"), set_gram=t_gram, vd_sweep_excl_gram=(ev.get("set_sweep") or 0.0) - t_gram,
                      set_logdet=ev.get("set_logdet")),
        set_gram=dict(ms=t_gram, bytes=gram_bytes, flop=gram_flop, frac_stream=gram_bytes / (t_gram * 1e-3) / STREAM,
                      frac_mfma=gram_flop / (t_gram * 1e-3) / F64_MFMA,
                      note="timed on one 256-row tile of V_d (all %d holes), x %d rows / 256" % (C, Mv)),
        campaign_one_hole_ms=t_hole,
        campaign_note="propose_drill_campaign(1): step + table + step with mean and variance + the restoring step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "campaign.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), stream_Bps=STREAM, f64_mfma_flops=F64_MFMA)
    for n in [int(v) for v in a.sizes.split(",")]:
        res[str(n)] = measure(n, a.reps)
        print(json.dumps(res[str(n)], indent=1), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
