"""Timing of appended drill rows against whole steps -> profiles/append.json.

    timeout -k 10 900 python tools/time_append.py [--reps 3] [--q 8] [--sizes 64] [--out profiles/append.json]

On the headline survey (tests/golden/oracle64_sample_matern32.npz; oracle32_matern32.npz at 32), in one process:
  * a greedy campaign of q holes with update="refactor" (a step and a table per pick) against update="append" (one table, then per
    pick the hole's rows appended and their part added to the resident Grams), `reps` runs of each in alternation, wall-clock with the
    device drained; the picks of the two must coincide;
  * one assimilated hole (append_drill_rows with the mean and variance) against one step with the mean and variance, with the
    append's own split by its timed stages, the same append with B from each of its sources (None: the step does not offer it),
    and the result against the engine's step on the union of the rows;
  * the growth copy: the factor and A K reallocated with 256 more rows, and back.
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


def normwise(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def measure(n, reps, q):
    from geobo_amd.campaign import vertical_sets
    from geobo_amd.engine import create_cov_lengths
    inv, _ = survey(n)
    eng, s = inv.engine, inv.settings
    N = eng.N
    out = dict(grid=[n, n, n], route=eng.step_route, q=q, rows=int(2 * eng.Ms_pad + len(inv._sel)), factor_rows=int(eng.last["step"].M_pad))
    # ---- campaign: the two modes in alternation --------------------------------------------------------------------------------
    for mode in ("refactor", "append"):                      # (first-use allocations of both modes' workspaces)
        inv.propose_drill_campaign(q, update=mode)
    runs = dict(refactor=[], append=[])
    tables = {}
    for _ in range(reps):
        for mode in ("refactor", "append"):
            t, tab = wall(lambda: inv.propose_drill_campaign(q, update=mode))
            runs[mode].append(t)
            tables[mode] = tab
    same = bool(tables["refactor"][["NORTHING", "EASTING", "RANK"]].equals(tables["append"][["NORTHING", "EASTING", "RANK"]]))
    out["campaign"] = dict(
        refactor_ms=runs["refactor"], append_ms=runs["append"],
        refactor_per_pick_ms=[t / q for t in runs["refactor"]], append_per_pick_ms=[t / q for t in runs["append"]],
        spread_per_pick_ms=dict(refactor=(max(runs["refactor"]) - min(runs["refactor"])) / q, append=(max(runs["append"]) - min(runs["append"])) / q),
        faster_by_more_than_the_spread=bool(min(runs["refactor"]) - max(runs["append"]) > 0.0),
        same_picks=same, utility_difference=normwise(tables["append"].UTILITY.to_numpy(), tables["refactor"].UTILITY.to_numpy()),
        factor_rows_after=int(eng.last["step"].M_pad),
        note="whole propose_drill_campaign(q) calls, wall-clock; per pick = call / q (the append mode's one table sweep, its final "
             "truncation and the refactor mode's final and restoring steps are inside)")
    # ---- one hole: append against a step ---------------------------------------------------------------------------------------
    sets, _ = vertical_sets(n, n, n)
    seen = np.zeros(N, dtype=bool)
    seen[inv._sel] = True
    c = next(c for c in range(len(sets) // 2, len(sets)) if not seen[sets[c]].any())
    vox = sets[c].astype(np.int64)
    vals = np.asarray(inv.mu_rec)[2 * N + vox] + 0.3
    inv._run(inv.gp_amp, inv.gp_length, None, True, True)
    Md0 = eng.last["step"].Md
    t_step = [wall(lambda: inv._run(inv.gp_amp, inv.gp_length, None, True, True))[0] for _ in range(reps)]
    t_app, t_trunc = [], []
    for _ in range(reps):
        t, r = wall(lambda: eng.append_drill_rows(vox, vals))
        t_app.append(t)
        t_trunc.append(wall(lambda: eng.truncate_drill_rows(Md0))[0])
    by_source = {}
    for src in ("columns", "lattice", "points"):          # the whole append with B from each source the step offers (second of two runs)
        try:
            for _ in range(2):
                by_source[src] = wall(lambda: eng.append_drill_rows(vox, vals, _b_source=src))[0]
                eng.truncate_drill_rows(Md0)
        except RuntimeError:
            by_source[src] = None
    eng.kernel_events = []
    eng.append_drill_rows(vox, vals)
    torch.cuda.synchronize()
    split = {}
    for name, _, _, _, e0, e1 in eng.kernel_events:
        split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
    eng.kernel_events = None
    ng, nm = inv.gravfield.size, inv.magfield.size
    sel_u = np.concatenate([inv._sel, vox])
    y_u = np.concatenate([inv.Fs3[ng + nm:], vals])
    order = np.argsort(sel_u)
    lengths = [float(v) for v in create_cov_lengths(np.array(inv.gp_length, dtype=float))]
    A_g, A_m = inv._operators()
    ref = eng.posterior(A_g, A_m, sel_u[order], inv.Fs3[:ng], inv.Fs3[ng:ng + nm], y_u[order], lengths, inv.coeffm, s.kernelfunc, inv.gp_sigma,
                        gp_amp=inv.gp_amp, props=(0, 1, 2), calclogl=True, want_mean_var=True)
    out["one_hole"] = dict(
        k=int(vox.size), B_source=eng.append_B_source, step_with_mean_var_ms=t_step, append_ms=t_app, append_ms_by_B_source=by_source, truncate_ms=t_trunc, append_split_ms=split,
        against_step_on_union=dict(mean=[normwise(r["mu"][i * N:(i + 1) * N], ref["mu"][i * N:(i + 1) * N]) for i in range(3)],
                                   var=[normwise(r["var"][i * N:(i + 1) * N], ref["var"][i * N:(i + 1) * N]) for i in range(3)],
                                   logl=abs(r["logl"] - ref["logl"]) / abs(ref["logl"])),
        note="append_ms: append_drill_rows of one whole z-column with the mean and variance, host read-back included; the split is by "
             "the engine's timed stages (append_B: B; append_factor: W, S, the new rows of L^-1; append_downdate: geobo_rows_downdate); "
             "the rows of V between them are not timed separately")
    # ---- the growth copy -------------------------------------------------------------------------------------------------------
    inv._run(inv.gp_amp, inv.gp_length, None, True, True)
    last, AK = eng._append_ready("time_append")
    M0 = last["step"].M_pad
    t_grow, AK = wall(lambda: eng._factor_resize(last, AK, M0 + 256))
    t_back, AK = wall(lambda: eng._factor_resize(last, AK, M0))
    akb = 0 if AK is None else AK.shape[0] * eng._ws[last["step"].ak_slot].shape[1] * 8
    out["growth"] = dict(rows_from=int(M0), rows_to=int(M0 + 256), grow_ms=t_grow, shrink_ms=t_back,
                         bytes=dict(L=8 * M0 * M0, Linv=8 * M0 * M0, AK=int(akb)),
                         note="allocate-and-copy of L, L^-1, u and A K, allocation included")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--sizes", default="64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0))
    for n in [int(v) for v in a.sizes.split(",")]:
        res[str(n)] = measure(n, a.reps, a.q)
        print(json.dumps(res[str(n)], indent=1), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
