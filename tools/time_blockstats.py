"""Timing of the block-support statistics -> profiles/blockstats.json.

    timeout -k 10 900 python tools/time_blockstats.py [--reps 5] [--out profiles/blockstats.json]

At 32^3 and 64^3 on the headline surveys (tests/golden/oracle32_matern32.npz, oracle64_sample_matern32.npz; Matern-3/2), in one process,
medians of `reps` after a warm-up:
  * geobo_block_cov alone for the blocks (1, 1, 1), (4, 4, 4) and (16, 16, 16): one launch pair per tile of the sweep's row count over
    three stored tiles, scaled to the M rows of the sweep; bytes read (3 M N 8) and the rate against the bare read stream of the part
    (profiles/r03_hbm_copy_runs.txt, read-only runs: 5.7 TB/s), which is the kernel's roof;
  * the three-property V sweep (the block_sweep launches of block_statistics) against the one-property sweep of hole_statistics
    without its geobo_set_gram launches (profiles/campaign.json measures those the same way);
  * the whole block_statistics call against the step with the mean and variance.
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

READ_STREAM = 5.7e12      # B/s, read-only stream (profiles/r03_hbm_copy_runs.txt)
BOXES = ((1, 1, 1), (4, 4, 4), (16, 16, 16))


def events(eng, fn):
    eng.kernel_events = []
    fn()
    torch.cuda.synchronize()
    acc = {}
    for name, _, _, _, e0, e1 in eng.kernel_events:
        acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1)
    eng.kernel_events = None
    return acc


def measure(n, reps):
    from geobo_amd import hip
    from geobo_amd.campaign import vertical_sets
    inv, _ = survey(n)
    eng = inv.engine
    grid = (n, n, n)
    Mv = 2 * eng.Ms_pad + len(inv._sel)
    t_step_mv = timed(lambda: inv._run(inv.gp_amp, inv.gp_length, None, False, True), reps)
    inv._run(inv.gp_amp, inv.gp_length, None, False, False)
    out = dict(grid=list(grid), route=eng.step_route, rows=int(Mv), step_with_mean_var_ms=t_step_mv, boxes={})
    # the one-property sweep of hole_statistics, its set_gram launches timed apart on one stored tile
    inv.hole_statistics()
    hole = [events(eng, inv.hole_statistics) for _ in range(reps)]
    T = 128 if eng.set_source == "spectral" else 256
    sets, _ = vertical_sets(n, n, n)
    idx = torch.as_tensor(sets.astype(np.int32), device=eng.device)
    V = [torch.randn((T, eng.N + 16), dtype=torch.float64, device=eng.device)[:, :eng.N] for _ in range(3)]
    G = torch.empty((sets.shape[0], sets.shape[1], sets.shape[1]), dtype=torch.float64, device=eng.device)
    t_gram = timed(lambda: hip.set_gram(idx, V[0], T, G, accumulate=True, ncols=eng.N), reps) * Mv / T
    sweep1 = float(np.median([h["set_sweep"] for h in hole])) - t_gram
    out.update(source=eng.set_source, tile_rows=T, one_property_sweep_ms=sweep1)
    nbytes = 3.0 * Mv * eng.N * 8
    for box in BOXES:
        nblocks = int(np.prod([-(-g // b) for g, b in zip(grid, box)]))
        C6 = torch.zeros((nblocks, 6), dtype=torch.float64, device=eng.device)
        ws = torch.empty(hip.block_cov_ws_doubles(T, grid, box), dtype=torch.float64, device=eng.device)
        t_kernel = timed(lambda: hip.block_cov(V, T, grid, box, C6, accumulate=True, ws=ws), reps) * Mv / T
        inv.block_statistics(box)
        runs = [events(eng, lambda: inv.block_statistics(box)) for _ in range(reps)]
        sweep3 = float(np.median([r["block_sweep"] for r in runs]))
        t_call = timed(lambda: inv.block_statistics(box), reps)
        out["boxes"]["x".join(str(b) for b in box)] = dict(
            blocks=nblocks, block_cov_ms=t_kernel, bytes_read=nbytes, read_TBps=nbytes / (t_kernel * 1e-3) / 1e12,
            frac_read_stream=nbytes / (t_kernel * 1e-3) / READ_STREAM, block_cov_in_call_ms=float(np.median([r["block_cov"] for r in runs])),
            three_property_sweep_ms=sweep3, sweep_ratio=sweep3 / sweep1, call_ms=t_call, call_over_step=t_call / t_step_mv)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blockstats.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), read_stream_Bps=READ_STREAM,
               note="block_cov_ms: one launch pair per tile on three stored tiles, x rows / tile rows; the roof is the read of bytes_read")
    for n in [int(v) for v in a.sizes.split(",")]:
        res[str(n)] = measure(n, a.reps)
        print(json.dumps(res[str(n)], indent=1), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
