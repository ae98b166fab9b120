"""Drill-hole information gain and greedy campaigns on the device: the two kernels against torch / NumPy, the
per-hole statistics against the oracle's dense posterior covariance, consistency with cubing() and Acquisition at 32^3 and 64^3, the
greedy campaign against a NumPy greedy on the oracle, and the state the campaign leaves behind."""
import numpy as np
import pytest
import torch

from conftest import load_golden, normwise, settings_for
from oracle import geobo_oracle as O

pytestmark = pytest.mark.gpu

TINY = dict(nx=10, ny=8, nz=6)


def _inv(s, **kw):
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=s, **kw)
    inv.create_cubegeometry()
    return inv


def _cubing(inv, f):
    d0 = f["drilldata0"]
    return inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)


def _host_operator(eng, A):
    from geobo_amd.operators import StreamedOperator
    if not isinstance(A, StreamedOperator):
        return A[:eng.Ms, :eng.N].cpu().numpy()
    buf = torch.empty((256, eng.N_pad), dtype=torch.float64, device="cuda")
    return np.vstack([A.rows_into(buf, r0, min(256, eng.Ms - r0))[:, :eng.N].cpu().numpy() for r0 in range(0, eng.Ms, 256)])


def _oracle(inv, sel=None, y_d=None):
    """oracle.posterior_dense on the engine's own operators (selection / drill values: the survey's unless given)."""
    s, eng = inv.settings, inv.engine
    A_g, A_m = (_host_operator(eng, A) for A in inv._operators())
    ng, nm = inv.gravfield.size, inv.magfield.size
    sel = inv._sel if sel is None else sel
    y_d = inv.Fs3[ng + nm:] if y_d is None else y_d
    P3 = O.grid_points((s.xNcube, s.yNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize))
    y = np.concatenate([inv.Fs3[:ng + nm], y_d])
    return O.posterior_dense(P3, A_g, A_m, sel, y, np.array(inv.gp_length, dtype=float), O.weight_matrix(inv.coeffm), s.kernelfunc,
                             inv.gp_sigma, gp_amp=inv.gp_amp, return_cov=True)


def _stats(Sd, sets, sigma2, observed=None):
    out = np.full((3, len(sets)), np.nan)
    for c, P in enumerate(sets):
        P = P[P >= 0]
        if observed is not None:
            P = P[~observed[P]]
        S = Sd[np.ix_(P, P)]
        out[:, c] = 0.5 * np.linalg.slogdet(np.eye(P.size) + S / sigma2)[1], S.sum(), np.trace(S)
    return out


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [6, 16, 64, 100, 128])
def test_set_gram_matches_torch(k):
    from geobo_amd import hip
    rng = np.random.default_rng(k)
    ncols, ld, C = 700, 712, 5
    contiguous = np.stack([np.arange(k) + b for b in (0, 7, 128, 333, ncols - k)])
    scattered = np.stack([rng.choice(ncols, k, replace=False) for _ in range(C)])
    for R in (1, 37, 128):
        V = torch.as_tensor(rng.standard_normal((R, ld)), device="cuda")
        for tab in (contiguous, scattered):
            idx = torch.as_tensor(tab.astype(np.int32), device="cuda")
            want = torch.stack([V[:, idx[c].long()].t() @ V[:, idx[c].long()] for c in range(C)])
            G = torch.full((C, k, k), np.nan, dtype=torch.float64, device="cuda")
            hip.set_gram(idx, V, R, G, ncols=ncols)
            assert float((G - want).abs().max() / want.abs().max()) <= 1e-13
            G0 = torch.as_tensor(rng.standard_normal((C, k, k)), device="cuda")
            G0 = G0 + G0.transpose(1, 2)
            G = G0.clone()
            hip.set_gram(idx, V, R, G, accumulate=True, ncols=ncols)
            assert float((G - (G0 + want)).abs().max() / (G0 + want).abs().max()) <= 1e-13


def test_set_gram_tiles_are_bit_identical():
    from geobo_amd import hip
    rng = np.random.default_rng(11)
    V = torch.as_tensor(rng.standard_normal((256, 1024)), device="cuda")
    tab = np.concatenate([np.stack([np.arange(64) + 64 * c for c in range(8)]), np.stack([rng.choice(1024, 64, replace=False) for _ in range(8)])])
    idx = torch.as_tensor(tab.astype(np.int32), device="cuda")
    runs = []
    for cuts in ((0, 256), (0, 128, 256), (0, 32, 100, 144, 256), (0, 4, 8, 200, 256)):
        G = torch.empty((16, 64, 64), dtype=torch.float64, device="cuda")
        for a, b in zip(cuts[:-1], cuts[1:]):
            hip.set_gram(idx, V[a:], b - a, G, accumulate=a > 0)
        runs.append(G.cpu().numpy())
    assert all(np.array_equal(runs[0], r) for r in runs[1:])
    assert np.array_equal(runs[0], np.swapaxes(runs[0], 1, 2))


def test_set_logdet_matches_numpy():
    from geobo_amd import hip
    rng = np.random.default_rng(7)
    C, k, n_obs, s2 = 6, 40, 500, 0.05
    X = rng.standard_normal((k, 3 * k))
    Kpp = X @ X.T / (3 * k) + 0.5 * np.eye(k)
    sets = np.stack([rng.choice(n_obs, k, replace=False) for _ in range(C)])
    sets[1, 30:] = -1                                          # padding
    G = np.empty((C, k, k))
    for c in range(C):
        Y = rng.standard_normal((k, 2 * k)) * 0.2
        G[c] = Y @ Y.T / (2 * k)
    G[3] = Kpp + 50.0 * np.eye(k)                              # Kpp - G not PSD: pivot 0 fails
    observed = np.zeros(n_obs, dtype=bool)
    observed[sets[2, :5]] = True
    observed[sets[4, 10:12]] = True
    per = np.stack([Kpp * (1.0 + 0.1 * c) for c in range(C)])
    for Kx, mask in ((Kpp, None), (per, observed)):
        out, st = hip.set_logdet(torch.as_tensor(G, device="cuda"), torch.as_tensor(Kx, device="cuda"), s2,
                                 torch.as_tensor(sets.astype(np.int32), device="cuda"), n_obs,
                                 observed=None if mask is None else torch.as_tensor(mask.astype(np.uint8), device="cuda"))
        out, st = out.cpu().numpy(), st.cpu().numpy()
        assert st[3] == 1 and np.isnan(out[:, 3]).all()
        for c in (0, 1, 2, 4, 5):
            assert st[c] == 0
            Kc = Kx if Kx.ndim == 2 else Kx[c]
            keep = sets[c] >= 0
            if mask is not None:
                keep &= ~mask[np.maximum(sets[c], 0)]
            D = (Kc - G[c])[np.ix_(keep, keep)]
            Lc = np.linalg.cholesky(np.eye(D.shape[0]) + D / s2)
            want = np.array([np.log(np.diag(Lc)).sum(), D.sum(), np.trace(D)])
            assert np.all(np.abs(out[:, c] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), (c, out[:, c], want)


# ---- 2. against the oracle's dense covariance --------------------------------------------------------------------------------
def _dipping_paths(inv):
    from geobo_amd.acquisition import Acquisition
    s = inv.settings
    acq = Acquisition(s, np.zeros((s.yNcube, s.xNcube, s.zNcube)), np.zeros((s.yNcube, s.xNcube, s.zNcube)))
    ext = min(s.xmax, s.ymax)
    cands = [(fx * ext, fy * ext, az, dip) for fx, fy, az, dip in
             ((0.35, 0.5, 30, 20), (0.25, 0.38, 120, 15), (0.5, 0.6, 250, 25), (0.4, 0.45, 300, 10), (0.3, 0.3, 160, 5), (0.55, 0.4, 20, 12))]
    paths = [acq.path_voxels(*c) for c in cands] + [acq.path_voxels(50.0, 50.0, 200.0, 80.0)]     # the last one leaves the cube
    return paths


@pytest.mark.parametrize("name,dims,method,rows", [("tiny_exp", TINY, "auto", False), ("tiny_matern32", TINY, "auto", True),
                                                   ("cube16_matern32", dict(nx=16, ny=16, nz=16), "spectral", False),
                                                   ("cube16_matern32", dict(nx=16, ny=16, nz=16), "dense", False),
                                                   ("cube16_sparse", dict(nx=16, ny=16, nz=16), "spectral", True)])
def test_hole_statistics_match_oracle(name, dims, method, rows, monkeypatch):
    from geobo_amd.campaign import path_sets, vertical_sets
    if rows:
        monkeypatch.setenv("GEOBO_ROWS", "1")
    f = load_golden(name + ".npz")
    s = settings_for(**dims, kernelfunc=name.split("_")[1])
    inv = _inv(s, method=method)
    inv.gp_length = f["gp_length_in"].copy()
    _cubing(inv, f)
    N, ds = inv.engine.N, float(inv._cube_scale[2])
    Sd = _oracle(inv)["cov"][2 * N:3 * N, 2 * N:3 * N]
    s2 = float(inv.gp_sigma[2]) ** 2
    sets, ij = vertical_sets(s.yNcube, s.xNcube, s.zNcube)
    want = _stats(Sd, sets, s2)
    got = inv.hole_statistics()
    print("%s [%s, %s]" % (name, inv.engine.step_route, inv.engine.set_source))
    assert (got["status"][ij[:, 0], ij[:, 1]] == 0).all()
    assert normwise(got["info_gain"][ij[:, 0], ij[:, 1]], want[0]) <= 1e-10
    assert normwise(got["path_std"][ij[:, 0], ij[:, 1]], np.sqrt(want[1]) * ds) <= 1e-10
    assert normwise(got["sum_var"][ij[:, 0], ij[:, 1]], want[2] * ds ** 2) <= 1e-10
    assert np.isnan(got["info_gain"][0]).all() and np.isnan(got["sum_var"][:, -1]).all()
    paths = _dipping_paths(inv)
    psets, valid = path_sets(paths, (s.yNcube, s.xNcube, s.zNcube))
    assert valid.sum() >= 5 and not valid[-1]
    gp = inv.hole_statistics(paths)
    wp = _stats(Sd, psets[valid], s2)
    assert np.isnan(gp["info_gain"][~valid]).all()
    assert normwise(gp["info_gain"][valid], wp[0]) <= 1e-10
    assert normwise(gp["path_std"][valid], np.sqrt(wp[1]) * ds) <= 1e-10
    assert normwise(gp["sum_var"][valid], wp[2] * ds ** 2) <= 1e-10


# ---- 3. consistency at size --------------------------------------------------------------------------------------------------
def _consistency(inv, cubes):
    from geobo_amd.acquisition import Acquisition
    from geobo_amd.campaign import utility, vertical_sets
    s = inv.settings
    got = inv.hole_statistics()
    sets, ij = vertical_sets(s.yNcube, s.xNcube, s.zNcube)
    assert (got["status"][ij[:, 0], ij[:, 1]] == 0).all()
    zs = lambda a: np.ascontiguousarray(a).sum(axis=2)[ij[:, 0], ij[:, 1]]
    sv = got["sum_var"][ij[:, 0], ij[:, 1]]
    err = float(np.max(np.abs(sv - zs(cubes[5])) / np.abs(zs(cubes[5]))))
    u = utility("ucb", zs(cubes[2]), 0.0, s.kappa, s.beta, sum_var=sv)
    uerr = normwise(u, Acquisition(s, cubes[2], cubes[5]).column_utility()[ij[:, 0], ij[:, 1]])
    print("%d^3 [%s, %s]: sum_var vs cube z-sums %.2e, ucb table %.2e" % (s.xNcube, inv.engine.step_route, inv.engine.set_source, err, uerr))
    assert err <= 1e-12 and uerr <= 1e-12
    assert np.all(np.isfinite(got["info_gain"][1:-1, 1:-1])) and np.all(got["info_gain"][1:-1, 1:-1] > 0)
    return sets


def test_consistency_at_32():
    f = load_golden("oracle32_matern32.npz")
    d0 = np.zeros(32 ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(32, 32, 32)
    s = settings_for(32, 32, 32, kernelfunc="matern32")
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    cubes = inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    _consistency(inv, cubes)


def test_consistency_and_sources_agree_at_64():
    from geobo_amd.config_loader import Settings
    f = load_golden("oracle64_sample_matern32.npz")
    n = 64
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc="matern32"))
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    cubes = inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    sets = _consistency(inv, cubes)
    assert inv.engine.set_source == "spectral"
    from geobo_amd.engine import create_cov_lengths
    lengths = [float(v) for v in create_cov_lengths(np.array(inv.gp_length, dtype=float))]
    sub = sets[::37]
    res = {src: np.stack([t.cpu().numpy() for t in inv.engine.set_statistics(sub, s.kernelfunc, lengths, inv.coeffm, inv.gp_amp, inv.gp_sigma,
                                                                              source=src)[:3]]) for src in ("spectral", "generic")}
    errs = [normwise(res["spectral"][i], res["generic"][i]) for i in range(3)]
    print("64^3 spectral vs generic source: %s" % errs)
    assert max(errs) <= 1e-12


# ---- 4. greedy campaign ------------------------------------------------------------------------------------------------------
def test_campaign_matches_numpy_greedy():
    from geobo_amd.campaign import vertical_sets
    f = load_golden("tiny_exp.npz")
    s = settings_for(**TINY, kernelfunc="exp")
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    cubes = _cubing(inv, f)
    N, q = inv.engine.N, 3
    ng, nm = inv.gravfield.size, inv.magfield.size
    s2 = float(inv.gp_sigma[2]) ** 2
    sets, ij = vertical_sets(s.yNcube, s.xNcube, s.zNcube)
    r0 = _oracle(inv)
    mu_d = r0["mu"][2 * N:3 * N]
    values = np.zeros(N)
    values[inv._sel] = inv.Fs3[ng + nm:]
    sel, picks, utils = inv._sel.copy(), [], []
    r = r0
    for _ in range(q):
        observed = np.zeros(N, dtype=bool)
        observed[sel] = True
        u = _stats(r["cov"][2 * N:3 * N, 2 * N:3 * N], sets, s2, observed)[0] - s.beta * 0.0
        u[picks] = -np.inf
        c = int(np.argmax(u))
        picks.append(c)
        utils.append(u[c])
        new = sets[c][~observed[sets[c]]]
        values[new] = mu_d[new]
        sel = np.union1d(sel, new)
        r = _oracle(inv, sel, values[sel])
    table = inv.propose_drill_campaign(q)
    got_ij = [(int(round((a - s.ymin) / s.yvoxsize - 0.5)), int(round((b - s.xmin) / s.xvoxsize - 0.5))) for a, b in zip(table.NORTHING, table.EASTING)]
    assert got_ij == [tuple(ij[c]) for c in picks]
    assert table.RANK.tolist() == [1, 2, 3]
    assert normwise(table.UTILITY.to_numpy(), np.array(utils)) <= 1e-10
    assert np.allclose(table.INFO_GAIN.to_numpy(), table.UTILITY.to_numpy())
    info = inv.campaign_info
    assert np.array_equal(info["selection"], sel)
    scale = inv._cube_scale
    for i in range(3):
        want = r["var"][i * N:(i + 1) * N].reshape(s.yNcube, s.xNcube, s.zNcube) * scale[i] ** 2
        assert normwise(info["var"][i], want) <= 1e-10
        assert normwise(info["mean"][i], cubes[i]) <= 1e-12
    for kind in ("ucb", "ucb_path"):
        t = inv.propose_drill_campaign(2, utility=kind)
        assert len(t) == 2 and t.RANK.tolist() == [1, 2] and np.isfinite(t.UTILITY).all()


# ---- 5. state ----------------------------------------------------------------------------------------------------------------
def test_campaign_leaves_the_inversion_as_cubing_left_it():
    from geobo_amd.acquisition import Acquisition
    f = load_golden("tiny_matern32.npz")
    s = settings_for(**TINY, kernelfunc="matern32", gp_coeff=[0.2, 0.2, 0.2])
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    cubes = _cubing(inv, f)
    before = dict(Fs3=inv.Fs3.copy(), sel=inv._sel.copy(), d0=np.array(inv.drilldata0, copy=True), mu=inv.mu_rec.copy(),
                  var=np.diag(inv.cov_rec).copy())
    samples = inv.sample_posterior(8, seed=1)
    prop = Acquisition(s, cubes[2], cubes[5]).bayesopt_vert(write=False)
    inv.propose_drill_campaign(4)
    after = dict(Fs3=inv.Fs3, sel=inv._sel, d0=np.asarray(inv.drilldata0), mu=inv.mu_rec, var=np.diag(inv.cov_rec))
    assert all(np.array_equal(before[k], after[k]) for k in before)
    again = inv.sample_posterior(8, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(samples, again))
    assert prop.equals(Acquisition(s, cubes[2], cubes[5]).bayesopt_vert(write=False))
