"""Timing of the posterior sampler (HIP events after warm-up) -> profiles/sampling.json.

    timeout -k 10 900 python tools/time_sampling.py [--reps 5] [--out profiles/sampling.json]

  * the kernels of sampling.hip at 64^3 x 3 (torus 128^3) and 128^3 x 3 (torus 256^3), Matern-3/2, lengths (2.00, 2.02, 2.04) x 100 m,
    weights (0.2, 0.2, 0.2): time, bytes moved (compulsory HBM traffic of each launch) and the fraction of a 5 TB/s stream;
  * prior-sample time per sample (64 samples), and at 64^3 on the headline survey (tests/golden/oracle64_sample_matern32.npz, 50 drill
    rows): conditioning time per sample (PosteriorEngine.condition, 64 samples) and the end-to-end sample_posterior(64).
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

STREAM = 5.0e12     # B/s


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
    return float(np.median(ts))


def kernels(n, reps, S=64):
    from geobo_amd import hip
    from geobo_amd.engine import weight_matrix
    from geobo_amd.sampling import PriorSampler
    smp = PriorSampler((n, n, n), (100.0, 100.0, 100.0), "matern32", [200.0, 202.0, 204.0], weight_matrix((0.2, 0.2, 0.2)))
    my, mx, mz = smp.ext
    M, P, npr, N = my * mx * mz, 3, len(smp.pairs), n ** 3
    no = (my // 2 + 1) * (mx // 2 + 1) * (mz // 2 + 1)
    npairs = S // 2
    dev = "cuda"
    tab = torch.empty(M * 2, dtype=torch.float64, device=dev)
    big = torch.empty(npr * M * 2, dtype=torch.float64, device=dev)
    big2 = torch.empty_like(big)
    z = torch.empty(npairs * P * my * mx * n * 2, dtype=torch.float64, device=dev)
    x = torch.empty(npairs * P * my * n * n * 2, dtype=torch.float64, device=dev)
    out = torch.empty((S, P, N), dtype=torch.float64, device=dev)
    ws = torch.empty(hip.sample_factor_ws_doubles(), dtype=torch.float64, device=dev)
    st = torch.empty(4, dtype=torch.float64, device=dev)
    F, lam = torch.empty(no * P * P, dtype=torch.float64, device=dev), torch.empty(no * npr, dtype=torch.float64, device=dev)
    mix_in = torch.zeros(2 * P * M * 2, dtype=torch.float64, device=dev)
    mix_out = torch.empty_like(mix_in)
    rows = {}

    def rec(name, fn, nbytes, note=""):
        t = timed(fn, reps)
        rows[name] = dict(ms=t, bytes=float(nbytes), frac_stream=nbytes / (t * 1e-3) / STREAM, note=note)
    rec("torus_table", lambda: hip.torus_table(hip.kernel_id("matern32", True), my, mx, mz, 100.0, 100.0, 100.0, 202.0, 200.0, 0.2, 1.0, tab),
        M * 16, "one block pair")
    rec("fft_axis_forward_z", lambda: hip.fft_axis(0, npr * my * mx, mz, 1, mz, mz, big, big2), 2 * npr * M * 16, "6 tables, contiguous axis")
    rec("fft_axis_forward_y", lambda: hip.fft_axis(0, npr, my, mx * mz, my, my, big, big2), 2 * npr * M * 16, "6 tables, strided axis")
    rec("sample_factor", lambda: hip.sample_factor(P, my, mx, mz, smp.spectra, F, lam, ws, st), no * (npr * 16 + (P * P + npr) * 8),
        "octant: gathers Re S, writes F and lambda")
    rec("sample_zpass", lambda: hip.sample_zpass(P, 0, npairs, my, mx, mz, n, smp.F, z, seed=1), npairs * P * my * mx * n * 16,
        "%d sample pairs: Philox + mixing + inverse z, writes the cropped lines" % npairs)
    rec("fft_axis_inverse_x", lambda: hip.fft_axis(hip.FFT_INVERSE, npairs * P * my, mx, n, mx, n, z, x),
        npairs * P * my * (mx + n) * n * 16, "%d sample pairs" % npairs)
    rec("fft_axis_inverse_y_pairs", lambda: hip.fft_axis(hip.FFT_INVERSE | hip.FFT_OUT_PAIRS, npairs * P, my, n * n, my, n, x, out, P=P, Q=N, S=S),
        npairs * P * my * n * n * 16 + S * P * N * 8, "%d samples written as fp64" % S)
    rec("spectral_mix", lambda: hip.spectral_mix(P, 2, my, mx, mz, smp.lam, 1.0 / M, mix_in, mix_out), 2 * 2 * P * M * 16,
        "2 pairs (conditioning)")
    t_prior = timed(lambda: smp.sample(0, S, seed=1, out=out), reps)
    res = dict(grid=[n, n, n], torus=list(smp.ext), kernels=rows, prior_sample_ms_per_sample=t_prior / S,
               min_max_eigenvalue_ratio=smp.ratio)
    del big, big2, z, x
    return res, smp


def conditioning64(reps, S=64):
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
    inv.sample_posterior(2)
    smp = inv._sampler_cache[1]
    eng = inv.engine
    A_g, A_m = inv._operators()
    ng = inv.gravfield.size
    y = inv.Fs3
    F = smp.sample(0, S, seed=3)
    e = torch.zeros((S, y.size), dtype=torch.float64, device=eng.device)
    t_cond = timed(lambda: eng.condition(F, e, A_g, A_m, y[:ng], y[ng:2 * ng], y[2 * ng:], smp), reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        inv.sample_posterior(S, seed=5)
    t_e2e = (time.perf_counter() - t0) / reps * 1e3
    return dict(route=eng.step_route, condition_ms_per_sample=t_cond / S, sample_posterior_64_ms=t_e2e,
                note="end-to-end: prior samples, observation noise, conditioning and the copy of 3 x 64 cubes to the host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), stream_Bps=STREAM)
    res["64"], _ = kernels(64, a.reps)
    torch.cuda.empty_cache()
    res["64"]["conditioning"] = conditioning64(a.reps)
    torch.cuda.empty_cache()
    res["128"], _ = kernels(128, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
