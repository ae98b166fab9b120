"""Leave-one-out and leave-fold-out cross-validation on the device: the two kernels by value against long-double
references, the singleton and the set route against each other, Inversion.cross_validate and calc_cv against a brute force that
deletes the fold's rows and refactorises (tests/_crossval_ref.py) on the oracle's K_y, the state the calls leave behind, and 32^3 / 64^3.

The bound wherever a device value meets the brute force: normwise (conftest.normwise) within max(1e-10, 16 e_np), e_np the deviation
of the fp64 NumPy identity from the same brute force on the same matrix, computed in the test; 1e-10 is the project's tolerance for
hole statistics against the oracle's dense covariance.  Nothing of the device enters the bound."""
import numpy as np
import pytest
import torch

import _crossval_ref as R
from conftest import load_golden, normwise, settings_for
from oracle import geobo_oracle as O
from test_campaign_gpu import _host_operator, _inv

pytestmark = pytest.mark.gpu

TINY = dict(nx=10, ny=8, nz=6)
CUBE16 = dict(nx=16, ny=16, nz=16)
EPS = float(np.finfo(np.float64).eps)
MARGIN = 16.0
FLOOR = 1e-10
LD = np.longdouble


def _bound(e_np):
    return max(FLOOR, MARGIN * e_np)


def _dev(a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


# ---- 1. geobo_kinv_diag ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,pad", [(256, 0), (256, 16), (768, 0), (768, 16)])
def test_kinv_diag_by_value(m, pad):
    from geobo_amd import hip
    rng = np.random.default_rng(m + pad)
    Lh = np.tril(rng.standard_normal((m, m)))
    Lh[m - 40:] = 0.0                                          # the padding of a real factor: identity rows
    Lh[np.arange(m - 40, m), np.arange(m - 40, m)] = 1.0
    u = rng.standard_normal(m)
    buf = torch.full((m, m + pad), float("nan"), dtype=torch.float64, device="cuda")
    lower = torch.ones((m, m), dtype=torch.bool, device="cuda").tril()
    buf[:, :m] = torch.where(lower, _dev(Lh), torch.full_like(buf[:, :m], float("nan")))     # strict upper triangle: NaN
    Linv, ud = buf[:, :m], _dev(u)
    guard = torch.full((2, m + 128), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((hip.kinv_diag_ws_doubles(m),), float("nan"), dtype=torch.float64, device="cuda")
    d, alpha = hip.kinv_diag(Linv, ud, ws=ws, d=guard[0, 64:64 + m], alpha=guard[1, 64:64 + m])
    d2, alpha2 = hip.kinv_diag(Linv, ud)
    assert torch.equal(d, d2) and torch.equal(alpha, alpha2)                # bitwise, whatever ws held
    g = guard.cpu().numpy()
    assert np.isnan(g[:, :64]).all() and np.isnan(g[:, 64 + m:]).all() and not np.isnan(g[:, 64:64 + m]).any()
    Lt = _dev(Lh)
    torch_sums = ((Lt * Lt).sum(dim=0).cpu().numpy(), (Lt * ud[:, None]).sum(dim=0).cpu().numpy())
    Ll, ul = Lh.astype(LD), u.astype(LD)
    refs = ((Ll * Ll).sum(axis=0), (Ll * ul[:, None]).sum(axis=0))
    mags = ((Ll * Ll).sum(axis=0), np.abs(Ll * ul[:, None]).sum(axis=0))
    for name, got, ref, tsum, mag in zip(("d", "alpha"), (d.cpu().numpy(), alpha.cpu().numpy()), refs, torch_sums, mags):
        e_k = np.abs(got - ref).astype(np.float64)
        e_t = np.abs(tsum - ref).astype(np.float64)
        allowed = MARGIN * np.maximum(e_t, EPS * mag.astype(np.float64))
        print("kinv_diag m = %d ld = %d %s: worst error / allowed = %.3f" % (m, m + pad, name, float((e_k / allowed).max())))
        assert np.all(e_k <= allowed)
    assert np.array_equal(d.cpu().numpy()[m - 40:], np.ones(40))


# ---- 2. geobo_set_loo ------------------------------------------------------------------------------------------------------------
def _scipy_loo(G, a):
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    cf = cho_factor(G, lower=True)
    Lg = np.tril(cf[0])
    white = solve_triangular(Lg, a, lower=True)
    q = white @ white
    logp = -0.5 * q + np.log(np.diag(Lg)).sum() - 0.5 * a.size * R.LOG2PI
    return logp, q, cho_solve(cf, a), np.diag(cho_solve(cf, np.eye(a.size))).copy(), white


@pytest.mark.parametrize("k", [1, 5, 16, 17, 64, 100, 128])
def test_set_loo_by_value(k):
    from geobo_amd import hip
    rng = np.random.default_rng(100 + k)
    C, n = 6, 500
    G = np.empty((C, k, k))
    for c in range(C):
        X = rng.standard_normal((k, 3 * k + 2))
        G[c] = X @ X.T / X.shape[1] + 0.1 * np.eye(k)
    Q = np.linalg.qr(rng.standard_normal((k, k)))[0]
    G[1] = (Q * np.logspace(0, -6, k)) @ Q.T if k > 1 else G[1]                # condition about 1e6
    G[1] = 0.5 * (G[1] + G[1].T)
    idx = np.stack([rng.choice(n, k, replace=False) for _ in range(C)]).astype(np.int64)
    idx[5] += n                                                                # out of range on the far side: every entry padding but one
    idx[5, 0] = 3
    if k > 1:
        idx[2, k - max(1, k // 3):] = -1                                       # trailing padding
    if k > 2:
        idx[3, k // 2] = -1                                                    # interior padding
    piv = k // 2
    G[4, piv, piv] = -1.0                                                      # not positive definite: the pivot at k // 2 fails
    alpha = rng.standard_normal(n)
    out, resid, var, white, status = (t.cpu().numpy() for t in hip.set_loo(_dev(G), _dev(idx, np.int32), _dev(alpha), n))
    assert status.tolist() == [0, 0, 0, 0, 1 + piv, 0]
    assert np.isnan(out[:, 4]).all() and np.isnan(resid[4]).all() and np.isnan(var[4]).all() and np.isnan(white[4]).all()
    worst = 0.0
    for c in (0, 1, 2, 3, 5):
        live = (idx[c] >= 0) & (idx[c] < n)
        assert live.any()
        for arr in (resid, var, white):
            assert np.isnan(arr[c][~live]).all() and not np.isnan(arr[c][live]).any()
        Gl, al = G[c][np.ix_(live, live)], alpha[idx[c][live]]
        ref = R.loo_ld(Gl, al)
        sp = _scipy_loo(Gl, al)
        got = (out[0, c], out[1, c], resid[c][live], var[c][live], white[c][live])
        nl = int(live.sum())
        logp_scale = 0.5 * float(ref[1]) + float(np.abs(np.log(np.diag(R.cholesky_ld(Gl)))).sum()) + 0.5 * nl * R.LOG2PI
        scales = (logp_scale, float(ref[1]), float(np.abs(ref[2]).max()), float(np.abs(ref[3]).max()), float(np.abs(ref[4]).max()))
        for name, g, r, s, sc in zip(("logp", "mahalanobis", "resid", "var", "white"), got, ref, sp, scales):
            e_k = float(np.abs(np.asarray(g) - r).max())
            e_s = float(np.abs(np.asarray(s) - r).max())
            allowed = MARGIN * max(e_s, EPS * sc)
            worst = max(worst, e_k / allowed)
            assert e_k <= allowed, (k, c, name, e_k, e_s, sc)
    print("set_loo k = %d: worst error / allowed = %.3f" % (k, worst))


# ---- 3. the two device paths agree -----------------------------------------------------------------------------------------------
# (below m = 1024 the default schedule is the stream schedule: the 1024 case is the one that runs the tile DAG)
@pytest.mark.parametrize("schedule,m", [("default", 512), ("streams", 512), ("default", 1024)])
def test_singleton_and_set_routes_agree(schedule, m):
    from geobo_amd import hip
    rng = np.random.default_rng(5)
    X = rng.standard_normal((m, 2 * m))
    A = _dev(X @ X.T / (2 * m) + 0.05 * np.eye(m))
    Linv, info = hip.potrf_inv(A, ctx=hip.PotrfContext(), schedule="auto" if schedule == "default" else schedule)
    assert int(info.cpu()[0]) == 0
    assert float(torch.triu(Linv, 1).abs().max()) == 0.0                   # set_gram over columns of L^-1 relies on it
    u = Linv @ _dev(rng.standard_normal(m))
    d, alpha = hip.kinv_diag(Linv, u)
    resid, var = (alpha / d).cpu().numpy(), (1.0 / d).cpu().numpy()
    rows = np.arange(m)
    wide = np.full((m, 16), -1)
    wide[:, 0] = rows
    for tab in (rows[:, None], wide):
        idx = _dev(tab, np.int32)
        G = torch.empty((m, tab.shape[1], tab.shape[1]), dtype=torch.float64, device="cuda")
        hip.set_gram(idx, Linv, m, G, ncols=m)
        out, rs, vr, wh, st = hip.set_loo(G, idx, alpha, m)
        assert int(st.abs().max()) == 0
        errs = (normwise(rs[:, 0].cpu().numpy(), resid), normwise(vr[:, 0].cpu().numpy(), var))
        print("%s schedule, k = %d: resid %.2e var %.2e" % (schedule, tab.shape[1], *errs))
        assert max(errs) <= 1e-13
        assert normwise(out[1].cpu().numpy(), (alpha * alpha / d).cpu().numpy()) <= 1e-13


# ---- 4. end to end against the oracle --------------------------------------------------------------------------------------------
def _drilldata(f, dims, seed=9):
    """The fixture's drill voxels plus two whole z-columns and one run of three voxels, seeded normal values."""
    rng = np.random.default_rng(seed)
    d0 = np.array(f["drilldata0"], dtype=float)
    ny, nx, nz = d0.shape
    d0[ny // 4, nx // 3, :] = rng.standard_normal(nz)
    d0[(2 * ny) // 3, (3 * nx) // 4, :] = rng.standard_normal(nz)
    d0[ny // 2, nx // 2, 1:4] = rng.standard_normal(3)
    assert not np.any(d0[ny // 4, nx // 3] == 0)
    return d0


def _oracle_dense(inv, lengths=None, coeffm=None, gp_amp=None):
    """oracle.posterior_dense on the engine's own operators: K_y = AkA and the posterior mean."""
    s, eng = inv.settings, inv.engine
    A_g, A_m = (_host_operator(eng, A) for A in inv._operators())
    P3 = O.grid_points((s.xNcube, s.yNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize))
    r = O.posterior_dense(P3, A_g, A_m, inv._sel, inv.Fs3, np.array(inv.gp_length if lengths is None else lengths, dtype=float),
                          O.weight_matrix(inv.coeffm if coeffm is None else coeffm), s.kernelfunc, inv.gp_sigma,
                          gp_amp=inv.gp_amp if gp_amp is None else gp_amp)
    N, ng = eng.N, inv.gravfield.size
    A3mu = np.concatenate([A_g @ r["mu"][:N], A_m @ r["mu"][N:2 * N], r["mu"][2 * N:][inv._sel]])
    return r["AkA"], inv.Fs3 - A3mu, (A_g, A_m)


class _Brute:
    """Brute force and NumPy identity of folds on one (K_y, y), each fold computed once."""

    def __init__(self, K, y):
        self.K, self.y, self.fac, self.b, self.i = K, y, R.identity_factor(K, y), {}, {}

    def __call__(self, folds):
        """(predicted and std per row in fold order, logp per fold) of the brute force and of the identity, and the e_np of the three."""
        for B in folds:
            key = tuple(int(v) for v in B)
            if key not in self.b:
                self.b[key] = R.brute_force(self.K, self.y, B)
                self.i[key] = R.identity(self.K, self.y, B, factor=self.fac)
        pick = lambda store: R.all_folds(lambda K, y, B: store[tuple(int(v) for v in B)], self.K, self.y, folds)
        pb, pi = pick(self.b), pick(self.i)
        return pb, pi, tuple(normwise(a, b) for a, b in zip(pi, pb))


_SHARED = {}     # (fixture, drill seed) -> (operators, K_y, fit residual, _Brute): one oracle and one brute force per survey


def _reference(name, inv):
    ops = tuple(_host_operator(inv.engine, A) for A in inv._operators())
    hit = _SHARED.get(name)
    if hit is not None and all(normwise(a, b) <= 1e-13 for a, b in zip(ops, hit[0])):
        return hit[1:]
    K, fit, ops = _oracle_dense(inv)
    _SHARED[name] = (ops, K, fit, _Brute(K, inv.Fs3))
    return _SHARED[name][1:]


def _fold_sets(inv):
    Ms = inv.gravfield.size
    mixed = [np.array([7, Ms + 31, 2 * Ms + 1, 2 * Ms + 3]), np.array([0, 1, 2]), np.array([Ms + 5]), np.array([2 * Ms + 2, 11])]
    return {"loo": ("loo", inv._cv_folds("loo", None)), "holes": ("holes", inv._cv_folds("holes", None)),
            "patches": ("patches", inv._cv_folds("patches", None)), "mixed": (mixed, mixed)}


def _check_against_brute(inv, got, folds, brute, scale, label):
    """predicted, std and per-fold logp of one cross_validate() result against the brute force, within the bound."""
    Ms = inv.gravfield.size
    (pb, sb, lb), _, e_np = brute(folds)
    rows = np.concatenate(folds)
    sc = np.concatenate([np.full(Ms, scale[0]), np.full(Ms, scale[1]), np.full(inv.Fs3.size - 2 * Ms, scale[2])])
    pred = np.concatenate([got[t]["predicted"] for t in ("grav", "magn", "drill")])
    std = np.concatenate([got[t]["std"] for t in ("grav", "magn", "drill")])
    errs = (normwise(pred[rows] / sc[rows], pb), normwise(std[rows] / sc[rows], sb), normwise(got["folds"]["logp"], lb))
    print("%s: predicted %.2e std %.2e logp %.2e   (e_np %.1e %.1e %.1e)" % ((label,) + errs + e_np))
    assert (got["folds"]["status"] == 0).all()
    assert np.array_equal(got["folds"]["size"], [len(B) for B in folds])
    for e, b in zip(errs, e_np):
        assert e <= _bound(b), (label, errs, e_np)


CASES = [("tiny_exp", TINY, "auto", False, {}), ("tiny_matern32", TINY, "auto", True, {}),
         ("cube16_matern32", CUBE16, "spectral", False, {}), ("cube16_matern32", CUBE16, "dense", False, {}),
         ("cube16_sparse", CUBE16, "spectral", False, {}),
         ("illcond_tiny_exp", TINY, "auto", False, dict(gp_lengthscale=8, gp_err=[0.01, 0.01, 0.01]))]


@pytest.mark.parametrize("name,dims,method,rows,extra", CASES, ids=["%s-%s%s" % (c[0], c[2], "-rows" if c[3] else "") for c in CASES])
def test_cross_validate_matches_brute_force(name, dims, method, rows, extra, monkeypatch):
    if rows:
        monkeypatch.setenv("GEOBO_ROWS", "1")
    f = load_golden(name + ".npz")
    s = settings_for(**dims, kernelfunc=name.replace("illcond_", "").split("_")[1], **extra)
    inv = _inv(s, method=method)
    inv.gp_length = f["gp_length_in"].copy()
    if "gp_amp" in f:
        inv.gp_amp = float(f["gp_amp"])
    d0 = _drilldata(f, dims)
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    scale = [float(v) for v in inv._cube_scale]
    K, fit, brute = _reference(name, inv)
    sets = _fold_sets(inv)
    Ms = inv.gravfield.size
    # the in-sample misfit y - A3 mu = D alpha: the identity's own deviation from the oracle's is its e_np
    sig2 = np.concatenate([np.full(Ms, float(inv.gp_sigma[0])), np.full(Ms, float(inv.gp_sigma[1])), np.full(inv.Fs3.size - 2 * Ms, float(inv.gp_sigma[2]))]) ** 2
    e_fit = normwise(sig2 * brute.fac[1], fit)
    assert len(sets["holes"][1]) == 2 * Ms + np.unique(inv._sel // s.zNcube).size and max(len(B) for B in sets["holes"][1]) == s.zNcube
    for kind, (arg, folds) in sets.items():
        got = inv.cross_validate(folds=arg)
        _check_against_brute(inv, got, folds, brute, scale, "%s [%s] %s" % (name, inv.engine.step_route, kind))
        assert normwise(got["fit_residual"], fit) <= _bound(e_fit), (normwise(got["fit_residual"], fit), e_fit)
        # the summary is what the arrays give; z and std carry the scale of cubing()
        assert got["summary"]["logp"] == float(np.sum(got["folds"]["logp"]))
        a = 0
        for i, t in enumerate(("grav", "magn", "drill")):
            o, b = got[t], a + got[t]["observed"].size
            assert np.array_equal(o["observed"], inv.Fs3[a:b] * inv._cube_scale[i])
            seen = o["fold"] >= 0
            assert np.allclose(o["residual"][seen], (o["observed"] - o["predicted"])[seen], rtol=0, atol=1e-12 * np.abs(o["observed"]).max())
            assert np.isnan(o["predicted"][~seen]).all() and np.isnan(o["std"][~seen]).all()
            assert np.allclose(o["z"][seen], (o["residual"] / o["std"])[seen], rtol=1e-14)
            assert np.allclose(o["fit_residual"], got["fit_residual"][a:b] * inv._cube_scale[i], rtol=1e-14)
            if seen.any():
                assert got["summary"][t]["mean_z2"] == float(np.nanmean(o["z"] ** 2))
            inside = np.array([B.min() >= a and B.max() < b for B in folds])
            if inside.any():
                want = float(np.mean(got["folds"]["mahalanobis"][inside] / got["folds"]["size"][inside]))
                assert got["summary"][t]["mean_mahalanobis"] == want
            a = b
        if kind != "mixed":
            assert all((got[t]["fold"] >= 0).all() for t in ("grav", "magn", "drill"))
        else:
            assert (got["grav"]["fold"][[0, 1, 2]] == 1).all() and got["grav"]["fold"][7] == 0 and got["grav"]["fold"][11] == 3
            assert np.isnan(got["magn"]["predicted"][0]) and got["magn"]["fold"][0] == -1


# ---- 5. calc_cv ------------------------------------------------------------------------------------------------------------------
def test_calc_cv_matches_brute_force():
    from geobo_amd.engine import create_cov_lengths
    f = load_golden("tiny_exp.npz")
    s = settings_for(**TINY, kernelfunc="exp")
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    d0 = _drilldata(f, TINY)
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    before = np.array(inv.gp_length, copy=True)
    params = np.array([1.3, 2.6, 0.9, 0.3, 0.25])
    lengths = create_cov_lengths(params[1] * np.full(3, s.xvoxsize))
    K, _, _ = _oracle_dense(inv, lengths=lengths, coeffm=params[2:], gp_amp=params[0])
    brute = _Brute(K, inv.Fs3)
    for kind in ("holes", "loo"):
        (_, _, lb), (_, _, li), _ = brute(inv._cv_folds(kind, None))
        got, want = inv.calc_cv(params, folds=kind), -float(lb.sum())
        e_np = abs(-float(li.sum()) - want) / abs(want)
        print("calc_cv %s: %.12g against %.12g (e_np %.1e)" % (kind, got, want, e_np))
        assert abs(got - want) / abs(want) <= _bound(e_np)
    assert got == inv.calc_cv(params, folds="loo") and inv.calc_cv(params) == inv.calc_cv(params, folds="holes")
    assert np.array_equal(inv.gp_length, before)
    # an error of the folds is raised, not turned into an inf objective
    with pytest.raises(ValueError, match="at most 128"):
        inv.calc_cv(params, folds=[np.arange(129)])
    with pytest.raises(ValueError, match="disjoint"):
        inv.calc_cv(params, folds=[np.array([0, 1]), np.array([1, 2])])


def test_calc_cv_at_32_is_finite_and_the_sum_of_cross_validate():
    """calc_cv at 32^3 (exp kernel: the 5-parameter form makes matern32 singular) is finite and equals minus summary.logp of
    cross_validate("holes") at the same parameters.  The two values come from two factorisations of the same matrix through the same
    kernels, so the floor of this file's bound (1e-10, relative) is ample; the folds themselves meet the brute force at 32^3 in
    test_folds_at_32_match_brute_force."""
    f = load_golden("oracle32_matern32.npz")
    n = 32
    rng = np.random.default_rng(33)
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    d0[5, 9, :] = rng.standard_normal(n)
    d0[20, 14, :] = rng.standard_normal(n)
    s = settings_for(n, n, n, kernelfunc="exp")
    inv = _inv(s)
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    params = np.array([1.2, 2.5, 0.9, 0.3, 0.25])
    before = np.array(inv.gp_length, copy=True)
    got = inv.calc_cv(params)
    assert np.array_equal(inv.gp_length, before)
    inv.gp_amp, inv.gp_length, inv.coeffm = params[0], params[1] * np.full(3, s.xvoxsize), params[2:]
    cv = inv.cross_validate("holes")
    want = -cv["summary"]["logp"]
    print("calc_cv at 32^3: %.12g against %.12g, %d folds, largest %d" % (got, want, cv["folds"]["size"].size, cv["folds"]["size"].max()))
    assert (cv["folds"]["status"] == 0).all() and cv["folds"]["size"].max() == n
    assert np.isfinite(got) and abs(got - want) <= FLOOR * abs(want)


# ---- 6. state --------------------------------------------------------------------------------------------------------------------
def test_cross_validate_leaves_the_state_alone(monkeypatch):
    f = load_golden("tiny_matern32.npz")
    s = settings_for(**TINY, kernelfunc="matern32", gp_coeff=[0.2, 0.2, 0.2])
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    d0 = _drilldata(f, TINY)
    args = (f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    cubes = inv.cubing(*args)
    eng = inv.engine
    last = eng.last
    calls = []
    real = eng.posterior
    monkeypatch.setattr(eng, "posterior", lambda *a, **kw: (calls.append(kw.get("want_mean_var", True)), real(*a, **kw))[1])
    first = inv.cross_validate("holes")
    assert eng.last is last and calls == []                                  # no step ran
    again = inv.cubing(*args)
    assert all(np.array_equal(a, b) for a, b in zip(cubes, again))
    assert calls == [True]
    del calls[:]
    inv.gp_length = 1.5 * np.array(inv.gp_length)
    changed = inv.cross_validate("holes")
    assert calls == [False]                                                  # exactly one step, without mean and variance
    assert not np.array_equal(changed["drill"]["predicted"], first["drill"]["predicted"])
    assert np.array_equal(inv.cross_validate("holes")["drill"]["predicted"], changed["drill"]["predicted"]) and calls == [False]
    samples = inv.sample_posterior(2, seed=3)
    stats = inv.hole_statistics()
    assert all(np.isfinite(c).all() for c in samples) and np.isfinite(stats["info_gain"][1:-1, 1:-1]).all()
    assert calls == [False]
    # the 5-parameter form puts two equal lengths into the Matern cross term: the step fails, the objective is inf (as calc_logl's)
    assert inv.calc_cv([1.0, 2.0, 1.0, 0.2, 0.2]) == np.inf and inv.calc_logl([1.0, 2.0, 1.0, 0.2, 0.2]) == np.inf


# ---- 7. at size ------------------------------------------------------------------------------------------------------------------
def test_folds_at_32_match_brute_force():
    from geobo_amd.crossval import padded_rows
    f = load_golden("oracle32_matern32.npz")
    n = 32
    rng = np.random.default_rng(32)
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    d0[5, 9, :] = rng.standard_normal(n)
    d0[20, 14, :] = rng.standard_normal(n)
    d0[11, 3, 4:7] = rng.standard_normal(3)                                # (and two short runs: four holes of more than one voxel)
    d0[27, 27, 10:12] = rng.standard_normal(2)
    s = settings_for(n, n, n, kernelfunc="matern32")
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    eng = inv.engine
    Ms, Mu = eng.Ms, inv.Fs3.size
    rows = padded_rows(np.arange(Mu), Ms, eng.Ms_pad)
    L = np.tril(eng.last["L"].cpu().numpy())[rows]                         # (the padding rows are identity rows: no coupling)
    K = L @ L.T
    holes = [B for B in inv._cv_folds("holes", None) if len(B) > 1]
    patches = inv._cv_folds("patches", None)
    assert len(holes) >= 2 and all(len(B) == 4 for B in patches[:2 * (n // 2) ** 2])
    whole = [B for B in holes if len(B) == n]
    folds = [np.array([3]), np.array([Ms - 1]), np.array([Ms + 500]), np.array([2 * Ms + 2])]
    folds += [patches[0], patches[100], patches[(n // 2) ** 2 + 17], patches[2 * (n // 2) ** 2 - 1]]
    folds += whole[:2] + [B for B in holes if len(B) < n][:2]
    assert len(folds) == 12 and len(whole) == 2
    assert np.unique(np.concatenate(folds)).size == sum(len(B) for B in folds)          # (no row in two folds)
    got = inv.cross_validate(folds=folds)
    _check_against_brute(inv, got, folds, _Brute(K, inv.Fs3), [float(v) for v in inv._cube_scale], "32^3 [%s]" % eng.step_route)


def test_routes_agree_at_64():
    from geobo_amd import hip
    from geobo_amd.config_loader import Settings
    from geobo_amd.crossval import padded_rows
    f = load_golden("oracle64_sample_matern32.npz")
    n = 64
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc="matern32"))
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    eng = inv.engine
    last = eng.last
    loo = eng.cross_validate(inv._cv_folds("loo", None))
    patches = eng.cross_validate(inv._cv_folds("patches", None))
    assert eng.last is last
    assert int(loo["status"].abs().max()) == 0 and int(patches["status"].abs().max()) == 0
    assert bool(torch.isfinite(patches["resid"]).all()) and bool((patches["var"] >= loo["var"]).all())   # less data, no smaller variance
    Linv, M_pad = last["Linv"], last["Linv"].shape[0]
    assert float(torch.triu(Linv, 1).abs().max()) == 0.0                   # (the tile-DAG schedule of the factorisation, at size)
    sub = np.arange(inv.Fs3.size)[::37]
    idx = _dev(padded_rows(sub, eng.Ms, eng.Ms_pad)[:, None], np.int32)
    d, alpha = hip.kinv_diag(Linv, last["u"])
    G = torch.empty((sub.size, 1, 1), dtype=torch.float64, device="cuda")
    hip.set_gram(idx, Linv, M_pad, G, ncols=M_pad)
    out, rs, vr, wh, st = hip.set_loo(G, idx, alpha, M_pad)
    errs = (normwise(rs[:, 0].cpu().numpy(), loo["resid"].cpu().numpy()[sub]), normwise(vr[:, 0].cpu().numpy(), loo["var"].cpu().numpy()[sub]))
    print("64^3 singleton against set route on every 37th row: resid %.2e var %.2e" % errs)
    assert int(st.abs().max()) == 0 and max(errs) <= 1e-12


def test_csv_files_parse_back(tmp_path):
    import pandas as pd
    f = load_golden("tiny_exp.npz")
    s = settings_for(**TINY, kernelfunc="exp", outpath=str(tmp_path))
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    d0 = _drilldata(f, TINY)
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    got = inv.cross_validate("patches", write=True)
    loc = np.asarray(f["sensor_locations"], dtype=float)
    for t in ("grav", "magn", "drill"):
        tab = pd.read_csv(tmp_path / ("crossval_%s.csv" % t), float_precision="round_trip")
        want = ["EASTING", "NORTHING"] + (["DEPTH"] if t == "drill" else []) + ["OBSERVED", "PREDICTED", "STD", "Z", "FOLD"]
        assert list(tab.columns) == want and len(tab) == got[t]["observed"].size
        for col, key in (("OBSERVED", "observed"), ("PREDICTED", "predicted"), ("STD", "std"), ("Z", "z"), ("FOLD", "fold")):
            assert np.array_equal(tab[col].to_numpy(), got[t][key]), (t, col)
        if t == "drill":
            for col, row in (("EASTING", 0), ("NORTHING", 1), ("DEPTH", 2)):
                assert np.array_equal(tab[col].to_numpy(), inv.voxelpos[row][inv._sel])
        else:
            assert np.array_equal(tab["EASTING"].to_numpy(), loc[:, 0]) and np.array_equal(tab["NORTHING"].to_numpy(), loc[:, 1])
