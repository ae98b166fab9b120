"""Timing of the exact log-likelihood gradient (HIP events after warm-up) -> profiles/logl_grad.json.

    timeout -k 10 900 python tools/time_logl_grad.py [--reps 5] [--out profiles/logl_grad.json]

  * calc_logl, calc_logl_grad (one directional Gram) and neg_logl_and_grad (three) on the synthetic survey of bench.py at 32^3 and on
    the 64^3 headline survey (50 drill rows).  calc_logl's 5-parameter form puts two equal lengths into the Matern cross term
    (0/0: inf), so the 5-parameter pair is timed with the exp kernel and the 7-parameter form with Matern-3/2 at the headline lengths
    (2.00, 2.02, 2.04) x 100 m, each against a likelihood-only step at the same parameters;
  * one geobo_kinv_dot launch at M = 8448 with T = 1 and T = 4 (random lower-triangular L^-1): time and fraction of the fp64 matrix
    peak for M^3/3 flop.
Every run of this tool belongs under its own `timeout -k 10 <s>` (it starts a GPU process and ends with it)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 78.6      # fp64 matrix peak of the MI355X, TF/s


def timed(fn, reps, warm=2):
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
    return float(np.median(ts)), [float(t) for t in ts]


def survey(n, kern):
    from bench import synthetic_inputs
    from geobo_amd.config_loader import Settings
    from geobo_amd.inversion import Inversion
    s = Settings(dict(xmin=0, xmax=100.0 * n, ymin=0, ymax=100.0 * n, zmax=0, zoff=1, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n,
                      gp_lengthscale=2, gp_err=[0.1, 0.1, 0.1], gp_coeff=[1.0, 0.2, 0.2], kernelfunc=kern, XMAG=0, YMAG=0, ZMAG=1))
    inv = Inversion(settings=s)
    grav, mag, loc, drill0 = synthetic_inputs(inv, 50)
    if kern == "matern32":
        inv.gp_length = np.array([2.00, 2.02, 2.04]) * s.xvoxsize
    inv.cubing(grav, mag, drill0[drill0 != 0], loc, drill0)
    return inv


def time_objectives(n, reps):
    out = {}
    inv = survey(n, "exp")
    p = np.array([1.0, 2.0, 1.0, 0.2, 0.2])
    t0, _ = timed(lambda: inv.calc_logl(p), reps)
    t1, _ = timed(lambda: inv.calc_logl_grad(p), reps)
    assert inv.calc_logl_grad(p)[0] == inv.calc_logl(p)
    out["exp"] = dict(calc_logl_ms=t0, calc_logl_grad_ms=t1, ratio=t1 / t0, route=inv.engine.step_route)
    del inv
    torch.cuda.empty_cache()
    inv = survey(n, "matern32")
    L = np.array(inv.gp_length, dtype=float)
    t0, _ = timed(lambda: inv._run(inv.gp_amp, L.copy(), None, True, False), reps)
    t1, _ = timed(lambda: inv.neg_logl_and_grad(inv.gp_amp, L, inv.coeffm), reps)
    v = inv.neg_logl_and_grad(inv.gp_amp, L, inv.coeffm)[0]
    out["matern32"] = dict(likelihood_step_ms=t0, neg_logl_and_grad_ms=t1, ratio=t1 / t0, value=float(v), route=inv.engine.step_route)
    del inv
    torch.cuda.empty_cache()
    return out


def time_kinv_dot(m, reps):
    from geobo_amd import hip
    rng = np.random.default_rng(1)
    L = hip.to_dev(np.tril(rng.standard_normal((m, m)) * 0.2 / np.sqrt(m)) + np.eye(m))
    alpha = hip.to_dev(rng.standard_normal(m))
    G = [hip.to_dev(rng.standard_normal((m, m))) for _ in range(4)]
    segs = ((0, 4096), (4096, 8192), (8192, 8242)) if m == 8448 else ((0, m // 2), (m // 2, m), (m, m))
    res = {}
    for T in (1, 4):
        ws = torch.empty(hip.kinv_dot_ws_doubles(m, T), dtype=torch.float64, device="cuda")
        out = torch.empty((T, 3, 3), dtype=torch.float64, device="cuda")
        ms, all_ms = timed(lambda: hip.kinv_dot(L, alpha, G[:T], segs, ws=ws, out=out), reps)
        flop = m ** 3 / 3.0
        res["T%d" % T] = dict(ms=ms, all_ms=all_ms, tflops=flop / ms / 1e9, frac_peak=flop / ms / 1e9 / PEAK_TF)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logl_grad.json"))
    ap.add_argument("--sizes", default="32,64")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), kinv_dot_M8448=time_kinv_dot(8448, a.reps))
    print(json.dumps(res["kinv_dot_M8448"]), flush=True)
    for n in [int(v) for v in a.sizes.split(",")]:
        res["cube%d" % n] = time_objectives(n, a.reps)
        print(n, json.dumps(res["cube%d" % n]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
