"""Appending drill rows to the step's factor on the device: the two kernels against the NumPy reference and
torch, the engine's append against the oracle on the union of the rows, growth and chunks, truncation back to the bits of the step,
the products that read the factor afterwards, the campaign with update="append", and the state a failure leaves."""
import numpy as np
import pytest
import torch

import _append_ref as R
from conftest import load_golden, normwise, settings_for
from oracle import geobo_oracle as O

pytestmark = pytest.mark.gpu

TINY = dict(nx=10, ny=8, nz=6)
C16 = dict(nx=16, ny=16, nz=16)


def _inv(s, **kw):
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=s, **kw)
    inv.create_cubegeometry()
    return inv


def _cubing(inv, f):
    d0 = f["drilldata0"]
    return inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)


def _survey(name, dims, method="auto", **kw):
    f = load_golden(name + ".npz")
    inv = _inv(settings_for(**dims, kernelfunc=name.split("_")[1], **kw), method=method)
    inv.gp_length = f["gp_length_in"].copy()
    return inv, _cubing(inv, f)


def _host_operator(eng, A):
    from geobo_amd.operators import StreamedOperator
    if not isinstance(A, StreamedOperator):
        return A[:eng.Ms, :eng.N].cpu().numpy()
    buf = torch.empty((256, eng.N_pad), dtype=torch.float64, device="cuda")
    return np.vstack([A.rows_into(buf, r0, min(256, eng.Ms - r0))[:, :eng.N].cpu().numpy() for r0 in range(0, eng.Ms, 256)])


def _oracle(inv, sel, y_d, cov=True):
    """The oracle's posterior on the engine's own operators for the drill rows (sel, y_d), as tests/test_campaign_gpu.py calls it;
    cov=False: its matrix-free form (the same result without the 3N x 3N covariance)."""
    s, eng = inv.settings, inv.engine
    A_g, A_m = (_host_operator(eng, A) for A in inv._operators())
    ng, nm = inv.gravfield.size, inv.magfield.size
    P3 = O.grid_points((s.xNcube, s.yNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize))
    y = np.concatenate([inv.Fs3[:ng + nm], y_d])
    args = (P3, A_g, A_m, sel, y, np.array(inv.gp_length, dtype=float), O.weight_matrix(inv.coeffm), s.kernelfunc, inv.gp_sigma)
    if cov:
        return O.posterior_dense(*args, gp_amp=inv.gp_amp, return_cov=True)
    return O.posterior_blocked(*args, gp_amp=inv.gp_amp)


def _stats(Sd, sets, sigma2):
    out = np.full((3, len(sets)), np.nan)
    for c, P in enumerate(sets):
        S = Sd[np.ix_(P, P)]
        out[:, c] = 0.5 * np.linalg.slogdet(np.eye(P.size) + S / sigma2)[1], S.sum(), np.trace(S)
    return out


def _union(inv, vox, vals):
    """(sorted union of the survey's drill voxels and vox, their values in that order)."""
    ng, nm = inv.gravfield.size, inv.magfield.size
    sel = np.concatenate([inv._sel, vox])
    y = np.concatenate([inv.Fs3[ng + nm:], vals])
    order = np.argsort(sel)
    return sel[order], y[order]


def _new_rows(inv, scattered=3, column=True, seed=5):
    """One whole unobserved z-column plus `scattered` unobserved voxels elsewhere, with values off the posterior mean."""
    s = inv.settings
    ny, nx, nz = s.yNcube, s.xNcube, s.zNcube
    rng = np.random.default_rng(seed)
    seen = np.zeros(ny * nx * nz, dtype=bool)
    seen[inv._sel] = True
    vox = np.zeros(0, dtype=np.int64)
    if column:
        cols = [c for c in range(ny * nx) if not seen[c * nz:(c + 1) * nz].any() and 0 < c // nx < ny - 1 and 0 < c % nx < nx - 1]
        vox = cols[len(cols) // 2] * nz + np.arange(nz)
        seen[vox] = True
    vox = np.concatenate([vox, rng.choice(np.flatnonzero(~seen), scattered, replace=False)])
    vals = np.asarray(inv.mu_rec, dtype=np.float64)[2 * seen.size + vox] + 0.3 * rng.standard_normal(vox.size)
    return vox.astype(np.int64), vals


def _engine_state(eng):
    last = eng.last
    off_d = 2 * eng.Ms_pad
    AK = last["AK"] if last["AK_complete"] else last["AK_partial"]
    return dict(L=last["L"].cpu().numpy(), Linv=last["Linv"].cpu().numpy(), u=last["u"].cpu().numpy(), sel=np.array(last["sel"]),
                AKd=None if AK is None else AK[off_d:].cpu().numpy(), Md=last["step"].Md, M_pad=last["step"].M_pad,
                sel_t=None if last["step"].sel_t is None else last["step"].sel_t.cpu().numpy())


def _same_state(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in a)


# ---- 1. geobo_factor_append -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 64, 100, 128])
def test_factor_append_matches_reference(k):
    from geobo_amd import hip
    rng = np.random.default_rng(k)
    Kf = R.spd(2 * k, rng)
    D = Kf[k:, k:]
    Wt = np.linalg.solve(np.linalg.cholesky(Kf[:k, :k]), Kf[:k, k:])
    G, r = Wt.T @ Wt, rng.standard_normal(k)
    Ls_w, T_w, u_w, log_w = R.factor_append(D, G, r)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    ld = k + 6                                              # outputs inside larger buffers: nothing outside the k x k block moves
    Ls = torch.full((k + 2, ld), 7.0, dtype=torch.float64, device="cuda")
    T, uP = Ls.clone(), torch.full((k + 3,), 7.0, dtype=torch.float64, device="cuda")
    out, st = hip.factor_append(dev(D), dev(G), dev(r), Ls, T, uP)
    assert int(st.cpu()[0]) == 0
    close = lambda got, want: np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    Lh, Th = Ls.cpu().numpy(), T.cpu().numpy()
    print("k = %d: L %.2e  T %.2e  u %.2e  logsum %.2e" % (k, np.abs(Lh[:k, :k] - Ls_w).max(), np.abs(Th[:k, :k] - T_w).max(),
                                                           np.abs(uP.cpu().numpy()[:k] - u_w).max(), abs(float(out.cpu()[0]) - log_w)))
    assert close(Lh[:k, :k], Ls_w) and close(Th[:k, :k], T_w) and close(uP.cpu().numpy()[:k], u_w) and close(float(out.cpu()[0]), log_w)
    assert np.array_equal(Lh[:k, :k], np.tril(Lh[:k, :k])) and np.array_equal(Th[:k, :k], np.tril(Th[:k, :k]))
    for X in (Lh, Th):
        assert (X[k:] == 7.0).all() and (X[:, k:] == 7.0).all()
    assert (uP.cpu().numpy()[k:] == 7.0).all()
    # only the lower triangles of D and G are read
    Du, Gu = np.tril(D) + np.triu(np.full((k, k), np.nan), 1), np.tril(G) + np.triu(np.full((k, k), np.nan), 1)
    Ls2, T2, u2 = (torch.zeros((k, k), dtype=torch.float64, device="cuda"), torch.zeros((k, k), dtype=torch.float64, device="cuda"),
                   torch.zeros(k, dtype=torch.float64, device="cuda"))
    out2, st2 = hip.factor_append(dev(Du), dev(Gu), dev(r), Ls2, T2, u2)
    assert int(st2.cpu()[0]) == 0 and np.array_equal(Ls2.cpu().numpy(), Lh[:k, :k]) and np.array_equal(T2.cpu().numpy(), Th[:k, :k])


@pytest.mark.parametrize("k,pivot", [(1, 0), (40, 0), (40, 17), (128, 127)])
def test_factor_append_indefinite_leaves_outputs(k, pivot):
    from geobo_amd import hip
    rng = np.random.default_rng(k + pivot)
    S = R.spd(k, rng)
    Lw = np.linalg.cholesky(S)
    Lw[pivot, pivot] = 0.0
    S = Lw @ Lw.T                                           # the leading pivots are fine, pivot `pivot` is not
    S[pivot, pivot] -= 1.0
    G = rng.standard_normal((k, k))
    G = G @ G.T / k
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    Ls = torch.as_tensor(rng.standard_normal((k, k)), device="cuda")
    T, uP = Ls.clone() + 1.0, torch.as_tensor(rng.standard_normal(k), device="cuda")
    out = torch.full((1,), 3.25, dtype=torch.float64, device="cuda")
    st = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    before = [t.cpu().numpy().copy() for t in (Ls, T, uP, out)]
    hip.factor_append(dev(S + G), dev(G), dev(rng.standard_normal(k)), Ls, T, uP, out=out, status=st)
    assert int(st.cpu()[0]) == 1 + pivot
    assert all(np.array_equal(b, t.cpu().numpy()) for b, t in zip(before, (Ls, T, uP, out)))
    from geobo_amd import _lib
    lib = _lib.load()
    assert lib.geobo_factor_append(129, 1, 129, 1, 129, 1, 1, 129, 1, 129, 1, 1, 1, None) == -1      # checks before any access
    assert lib.geobo_factor_append(4, 1, 3, 1, 4, 1, 1, 4, 1, 4, 1, 1, 1, None) == -1
    assert lib.geobo_rows_downdate(1, 8, 2, 9, 1, 1, 1, None) == -1


# ---- 2. geobo_rows_downdate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 37, 128])
def test_rows_downdate_matches_torch(n):
    from geobo_amd import hip
    rng = np.random.default_rng(n)
    ncols, ld = 700, 712
    V = torch.as_tensor(rng.standard_normal((n, ld)), device="cuda")
    c = torch.as_tensor(rng.standard_normal(n), device="cuda")
    mu0, var0 = (torch.as_tensor(rng.standard_normal(ncols + 5), device="cuda") for _ in range(2))
    want_mu = mu0[:ncols] + V[:, :ncols].t() @ c
    want_var = var0[:ncols] - (V[:, :ncols] ** 2).sum(0)
    for off in (0, 1):                                     # 16-byte pairs, and the 8-byte form of an odd offset
        mu, var = mu0.clone(), var0.clone()
        hip.rows_downdate(V[:, off:], n, c, mu[off:], var[off:], ncols=ncols - off)
        assert float((mu[off:ncols] - want_mu[off:]).abs().max() / want_mu.abs().max()) <= 1e-13
        assert float((var[off:ncols] - want_var[off:]).abs().max() / want_var.abs().max()) <= 1e-13
        assert torch.equal(mu[ncols:], mu0[ncols:]) and torch.equal(var[ncols:], var0[ncols:])
        assert torch.equal(mu[:off], mu0[:off]) and torch.equal(var[:off], var0[:off])
    mu, var = mu0.clone(), var0.clone()
    hip.rows_downdate(V, n, c, mu, var, ncols=699)        # an odd column count: the last column on its own
    assert float((mu[:699] - want_mu[:699]).abs().max() / want_mu.abs().max()) <= 1e-13 and torch.equal(mu[699:], mu0[699:])
    assert float((var[:699] - want_var[:699]).abs().max() / want_var.abs().max()) <= 1e-13 and torch.equal(var[699:], var0[699:])


def test_rows_downdate_row_splits_are_bit_identical():
    from geobo_amd import hip
    rng = np.random.default_rng(2)
    ncols, ld = 700, 712
    V = torch.as_tensor(rng.standard_normal((128, ld)), device="cuda")
    c = torch.as_tensor(rng.standard_normal(128), device="cuda")
    mu0, var0 = (torch.as_tensor(rng.standard_normal(ncols), device="cuda") for _ in range(2))
    runs = []
    for cuts in ((0, 128), (0, 32, 100, 128), (0, 1, 2, 128)):
        mu, var = mu0.clone(), var0.clone()
        for a, b in zip(cuts[:-1], cuts[1:]):
            hip.rows_downdate(V[a:], b - a, c[a:], mu, var, ncols=ncols)
        runs.append((mu.cpu().numpy(), var.cpu().numpy()))
    assert all(np.array_equal(runs[0][0], r[0]) and np.array_equal(runs[0][1], r[1]) for r in runs[1:])
    mu, var = mu0.clone(), var0.clone()
    hip.rows_downdate(V[:, 1:], 128, c, mu[1:], var[1:], ncols=ncols - 1)       # the 8-byte form computes the same bits
    assert np.array_equal(mu.cpu().numpy()[1:], runs[0][0][1:]) and np.array_equal(var.cpu().numpy()[1:], runs[0][1][1:])


# ---- 3. the engine against the oracle on the union; 5. truncation -----------------------------------------------------------
@pytest.mark.parametrize("name,dims,method,rows", [("tiny_exp", TINY, "auto", False), ("tiny_matern32", TINY, "auto", True),
                                                   ("cube16_matern32", C16, "spectral", False), ("cube16_matern32", C16, "dense", False)])
def test_append_matches_oracle_and_truncates_to_the_step(name, dims, method, rows, monkeypatch):
    from geobo_amd.campaign import vertical_sets
    from geobo_amd.engine import create_cov_lengths
    if rows:
        monkeypatch.setenv("GEOBO_ROWS", "1")
    inv, _ = _survey(name, dims, method)
    s, eng = inv.settings, inv.engine
    N = eng.N
    # (the reference's matern32 prior at these weights is slightly indefinite: only the clipped sampler draws from it)
    draw = (lambda: inv.sample_posterior(8, seed=1, approximate=True)) if s.kernelfunc == "matern32" else (lambda: inv.sample_posterior(8, seed=1))
    samples = draw()
    state0 = _engine_state(eng)
    vox, vals = _new_rows(inv)
    assert vox.size == s.zNcube + 3
    r = eng.append_drill_rows(vox, vals)
    sel_u, y_u = _union(inv, vox, vals)
    want = _oracle(inv, sel_u, y_u)
    errs = [normwise(r["mu"][i * N:(i + 1) * N], want["mu"][i * N:(i + 1) * N]) for i in range(3)]
    errs += [normwise(r["var"][i * N:(i + 1) * N], want["var"][i * N:(i + 1) * N]) for i in range(3)]
    print("%s [%s, %s]: append vs oracle on the union: mean %s  var %s" % (name, eng.step_route, eng.set_source, errs[:3], errs[3:]))
    assert max(errs) <= 1e-10
    assert eng.last["step"].Md == state0["Md"] + vox.size and np.array_equal(eng.last["sel"], np.concatenate([state0["sel"], vox]))
    # the products that read the factor see the rows: hole statistics against the oracle covariance of the union
    sets, ij = vertical_sets(s.yNcube, s.xNcube, s.zNcube)
    ws = _stats(want["cov"][2 * N:3 * N, 2 * N:3 * N], sets, float(inv.gp_sigma[2]) ** 2)
    got = inv.hole_statistics()
    ds = float(inv._cube_scale[2])
    assert (got["status"][ij[:, 0], ij[:, 1]] == 0).all()
    assert normwise(got["info_gain"][ij[:, 0], ij[:, 1]], ws[0]) <= 1e-10
    assert normwise(got["path_std"][ij[:, 0], ij[:, 1]], np.sqrt(ws[1]) * ds) <= 1e-10
    assert normwise(got["sum_var"][ij[:, 0], ij[:, 1]], ws[2] * ds ** 2) <= 1e-10
    appended = _engine_state(eng)
    # truncation: the bits of the step
    eng.truncate_drill_rows(state0["Md"])
    assert _same_state(state0, _engine_state(eng))
    again = draw()
    assert all(np.array_equal(a, b) for a, b in zip(samples, again))
    # ... and the same append once more gives the same bits (the mean and variance came back with the rows)
    r2 = eng.append_drill_rows(vox, vals)
    assert _same_state(appended, _engine_state(eng)) and np.array_equal(r2["mu"], r["mu"]) and np.array_equal(r2["var"], r["var"])
    assert r2["logl"] == r["logl"]
    # the engine's own refactor on the union (last: it replaces the step)
    ng, nm = inv.gravfield.size, inv.magfield.size
    lengths = [float(v) for v in create_cov_lengths(np.array(inv.gp_length, dtype=float))]
    A_g, A_m = inv._operators()
    ref = eng.posterior(A_g, A_m, sel_u, inv.Fs3[:ng], inv.Fs3[ng:ng + nm], y_u, lengths, inv.coeffm, s.kernelfunc, inv.gp_sigma,
                        gp_amp=inv.gp_amp, props=(0, 1, 2), calclogl=True, want_mean_var=True)
    print("   vs the engine's refactor: logl %.2e  mean %.2e  var %.2e  (oracle logl %.2e)"
          % (abs(r["logl"] - ref["logl"]) / abs(ref["logl"]), normwise(r["mu"], ref["mu"]), normwise(r["var"], ref["var"]),
             abs(r["logl"] - want["logl"]) / abs(want["logl"])))
    assert abs(r["logl"] - ref["logl"]) <= 1e-10 * abs(ref["logl"])


def test_append_through_the_point_columns():
    """B from the column code of predict_points (the source of a step that keeps neither A K nor a lattice Gram), asked for by name."""
    inv, _ = _survey("tiny_exp", TINY)
    eng, N = inv.engine, inv.engine.N
    state0 = _engine_state(eng)
    vox, vals = _new_rows(inv)
    with pytest.raises(RuntimeError, match="not available"):
        eng.append_drill_rows(vox, vals, _b_source="lattice")
    assert _same_state(state0, _engine_state(eng))
    r = eng.append_drill_rows(vox, vals, _b_source="points")
    assert eng.append_B_source == "points"
    want = _oracle(inv, *_union(inv, vox, vals), cov=False)
    errs = [normwise(r[k][i * N:(i + 1) * N], want[k][i * N:(i + 1) * N]) for k in ("mu", "var") for i in range(3)]
    print("tiny_exp, B through geobo_ak_points: %s" % errs)
    assert max(errs) <= 1e-10
    eng.truncate_drill_rows(state0["Md"])
    r2 = eng.append_drill_rows(vox, vals)
    assert eng.append_B_source == "columns" and max(normwise(r2[k], r[k]) for k in ("mu", "var")) <= 1e-10


# ---- 4. growth and chunks ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cube16():
    return _survey("cube16_matern32", C16, "spectral")


def test_growth_and_chunks(cube16):
    inv, _ = cube16
    eng = inv.engine
    inv._ensure_factor()
    N = eng.N
    state0 = _engine_state(eng)
    vox, vals = _new_rows(inv, scattered=260, column=False, seed=9)
    assert (2 * eng.Ms_pad + state0["Md"]) // 256 < (2 * eng.Ms_pad + state0["Md"] + vox.size) // 256
    r = eng.append_drill_rows(vox, vals)
    assert eng.last["step"].M_pad > state0["M_pad"] and eng.last["Linv"].shape[0] == eng.last["step"].M_pad
    assert eng.last["step"].Md == state0["Md"] + 260 and eng.mean_var_known()
    want = _oracle(inv, *_union(inv, vox, vals), cov=False)
    errs = [normwise(r[k][i * N:(i + 1) * N], want[k][i * N:(i + 1) * N]) for k in ("mu", "var") for i in range(3)]
    print("16^3: 260 rows in three chunks, %d -> %d factor rows: %s" % (state0["M_pad"], eng.last["step"].M_pad, errs))
    assert max(errs) <= 1e-10
    eng.truncate_drill_rows(state0["Md"])
    assert _same_state(state0, _engine_state(eng))
    # two successive calls against one
    v19, y19 = _new_rows(inv, scattered=19, column=False, seed=10)
    one = eng.append_drill_rows(v19, y19)
    eng.truncate_drill_rows(state0["Md"])
    eng.append_drill_rows(v19[:3], y19[:3])
    two = eng.append_drill_rows(v19[3:], y19[3:])
    # back to where the second call began: its snapshot returns, and the call repeats bit for bit
    eng.truncate_drill_rows(state0["Md"] + 3)
    again = eng.append_drill_rows(v19[3:], y19[3:])
    assert all(np.array_equal(again[k], two[k]) for k in ("mu", "var")) and again["logl"] == two["logl"]
    # to a row count at which no call began: the statistics are formed again, the mean and variance are dropped
    eng.truncate_drill_rows(state0["Md"] + 1)
    assert not eng.mean_var_known() and eng.last["step"].Md == state0["Md"] + 1
    with pytest.raises(RuntimeError, match="no longer known"):
        eng.append_drill_rows(v19[3:], y19[3:])
    blind = eng.append_drill_rows(v19[1:], y19[1:], want_mean_var=False)
    assert "mu" not in blind and abs(blind["logl"] - one["logl"]) <= 1e-12 * abs(one["logl"])
    eng.truncate_drill_rows(state0["Md"])
    assert eng.mean_var_known()
    errs = [normwise(two[k][i * N:(i + 1) * N], one[k][i * N:(i + 1) * N]) for k in ("mu", "var") for i in range(3)]
    print("16^3: 3 + 16 rows against 19: %s, logl %.2e" % (errs, abs(two["logl"] - one["logl"]) / abs(one["logl"])))
    assert max(errs) <= 1e-12 and abs(two["logl"] - one["logl"]) <= 1e-12 * abs(one["logl"])
    assert _same_state(state0, _engine_state(eng))
    for bad, what in (([v19[0], v19[0]], "repeat"), ([N], "flat voxel"), ([int(inv._sel[0])], "already")):
        with pytest.raises(ValueError, match=what):
            eng.append_drill_rows(bad, [0.0] * len(bad))
    with pytest.raises(ValueError, match="values for"):
        eng.append_drill_rows(v19[:2], [0.0])
    with pytest.raises(ValueError, match="Md must lie"):
        eng.truncate_drill_rows(state0["Md"] - 1)
    assert _same_state(state0, _engine_state(eng))


# ---- 6. consumers after assimilate_drill ------------------------------------------------------------------------------------------
def test_consumers_see_assimilated_rows(cube16):
    inv, cubes = cube16
    eng = inv.engine
    N = eng.N
    before = dict(sel=inv._sel.copy(), Fs3=inv.Fs3.copy(), mu=inv.mu_rec, cov=inv.cov_rec, logl=inv.logl)
    vox, vals = _new_rows(inv, seed=12)
    scale = inv._cube_scale
    d = np.asarray(inv.drillfield, dtype=np.float64)
    data = vals * d.std() + d.mean()                                        # in data units: assimilate_drill normalises them again
    iyxz = np.stack(np.unravel_index(vox, (inv.settings.yNcube, inv.settings.xNcube, inv.settings.zNcube)), axis=1)
    try:
        new = inv.assimilate_drill(iyxz, data)
        assert np.allclose(inv.Fs3[before["Fs3"].size:], vals, rtol=1e-13, atol=1e-13) and np.array_equal(inv._sel, np.concatenate([before["sel"], vox]))
        want = _oracle(inv, *_union(dict_inv(inv, before), vox, inv.Fs3[before["Fs3"].size:]), cov=False)
        errs = [normwise(np.asarray(new[i]).reshape(-1), want["mu"][i * N:(i + 1) * N] * scale[i]) for i in range(3)]
        errs += [normwise(np.asarray(new[3 + i]).reshape(-1), want["var"][i * N:(i + 1) * N] * scale[i] ** 2) for i in range(3)]
        print("16^3 assimilate_drill vs oracle: %s, logl %.2e" % (errs, abs(inv.logl - want["logl"]) / abs(want["logl"])))
        assert max(errs) <= 1e-10 and inv.logl != before["logl"]
        assert np.array_equal(inv.mu_rec.reshape(3, -1)[2] * scale[2], np.asarray(new[2]).reshape(-1))
        idx = np.concatenate([vox[:10], np.linspace(0, N - 1, 40).astype(np.int64)])
        got = inv.predict_points(inv.voxelpos.T[idx])
        perr = [normwise(got["mean"][a], np.asarray(new[a]).reshape(-1)[idx]) for a in range(3)]
        perr += [normwise(got["var"][a], np.asarray(new[3 + a]).reshape(-1)[idx]) for a in range(3)]
        print("   predict_points at 50 voxel centres vs the updated cubes: %s" % perr)
        assert max(perr) <= 1e-8
        cv = inv.cross_validate("loo")
        assert cv["drill"]["observed"].size == before["sel"].size + vox.size and np.isfinite(cv["drill"]["z"]).all()
        assert np.array_equal(cv["drill"]["observed"], inv.Fs3[-cv["drill"]["observed"].size:] * scale[2])
        assert (cv["folds"]["status"] == 0).all()
        z = np.zeros((4, 3, N))
        post = inv.sample_posterior(4, prior=z, noise=np.zeros((4, inv.Fs3.size)))
        for a in range(3):
            for k in range(4):
                assert normwise(post[a][k].reshape(-1), np.asarray(new[a]).reshape(-1)) <= 1e-10
    finally:
        eng.truncate_drill_rows(before["sel"].size)
        inv._sel, inv.Fs3, inv.mu_rec, inv.cov_rec, inv.logl = before["sel"], before["Fs3"], before["mu"], before["cov"], before["logl"]


class dict_inv:
    """The survey of `inv` as it was before the rows were assimilated (what _union reads)."""

    def __init__(self, inv, before):
        self.gravfield, self.magfield, self._sel, self.Fs3 = inv.gravfield, inv.magfield, before["sel"], before["Fs3"]


# ---- 7. campaign -----------------------------------------------------------------------------------------------------------------
def test_campaign_append_matches_numpy_greedy():
    from geobo_amd.campaign import vertical_sets
    inv, cubes = _survey("tiny_exp", TINY)
    s = inv.settings
    N, q = inv.engine.N, 3
    ng, nm = inv.gravfield.size, inv.magfield.size
    s2 = float(inv.gp_sigma[2]) ** 2
    sets, ij = vertical_sets(s.yNcube, s.xNcube, s.zNcube)
    r = _oracle(inv, inv._sel, inv.Fs3[ng + nm:])
    mu_d = r["mu"][2 * N:3 * N]
    values = np.zeros(N)
    values[inv._sel] = inv.Fs3[ng + nm:]
    sel, picks, utils = inv._sel.copy(), [], []
    for _ in range(q):
        observed = np.zeros(N, dtype=bool)
        observed[sel] = True
        u = _stats(r["cov"][2 * N:3 * N, 2 * N:3 * N], [P[~observed[P]] for P in sets], s2)[0]
        u[picks] = -np.inf
        c = int(np.argmax(u))
        picks.append(c)
        utils.append(u[c])
        new = sets[c][~observed[sets[c]]]
        values[new] = mu_d[new]
        sel = np.union1d(sel, new)
        r = _oracle(inv, sel, values[sel])
    state0 = _engine_state(inv.engine)
    table = inv.propose_drill_campaign(q, update="append")
    got_ij = [(int(round((a - s.ymin) / s.yvoxsize - 0.5)), int(round((b - s.xmin) / s.xvoxsize - 0.5))) for a, b in zip(table.NORTHING, table.EASTING)]
    assert got_ij == [tuple(ij[c]) for c in picks] and table.RANK.tolist() == [1, 2, 3]
    print("campaign, append: utilities %.2e" % normwise(table.UTILITY.to_numpy(), np.array(utils)))
    assert normwise(table.UTILITY.to_numpy(), np.array(utils)) <= 1e-10
    info = inv.campaign_info
    assert np.array_equal(info["selection"], sel)
    scale = inv._cube_scale
    for i in range(3):
        want = r["var"][i * N:(i + 1) * N].reshape(s.yNcube, s.xNcube, s.zNcube) * scale[i] ** 2
        assert normwise(info["var"][i], want) <= 1e-10
        assert normwise(info["mean"][i], cubes[i]) <= 1e-12
    assert _same_state(state0, _engine_state(inv.engine))
    ref = inv.propose_drill_campaign(q)                       # the default: a step per pick
    assert ref[["NORTHING", "EASTING", "RANK"]].equals(table[["NORTHING", "EASTING", "RANK"]])
    assert normwise(table.UTILITY.to_numpy(), ref.UTILITY.to_numpy()) <= 1e-10


def test_campaign_append_leaves_the_inversion_as_cubing_left_it():
    from geobo_amd.acquisition import Acquisition
    inv, cubes = _survey("tiny_matern32", TINY, gp_coeff=[0.2, 0.2, 0.2])
    s = inv.settings
    before = dict(Fs3=inv.Fs3.copy(), sel=inv._sel.copy(), d0=np.array(inv.drilldata0, copy=True), mu=inv.mu_rec.copy(),
                  var=np.diag(inv.cov_rec).copy())
    samples = inv.sample_posterior(8, seed=1)
    prop = Acquisition(s, cubes[2], cubes[5]).bayesopt_vert(write=False)
    params = inv._step_params
    table = inv.propose_drill_campaign(4, update="append")
    assert len(table) == 4 and inv._step_params == params and params is not None
    after = dict(Fs3=inv.Fs3, sel=inv._sel, d0=np.asarray(inv.drilldata0), mu=inv.mu_rec, var=np.diag(inv.cov_rec))
    assert all(np.array_equal(before[k], after[k]) for k in before)
    again = inv.sample_posterior(8, seed=1)
    assert all(np.array_equal(a, b) for a, b in zip(samples, again))
    assert prop.equals(Acquisition(s, cubes[2], cubes[5]).bayesopt_vert(write=False))


# ---- 9. the loop: assimilate, propose, assimilate ---------------------------------------------------------------------------------
def test_assimilate_campaign_assimilate():
    """Drill, assimilate, propose, drill, assimilate: the campaign in append mode leaves the assimilated state (mean, variance,
    log-likelihood, rows) as it found it, a second assimilation and a second campaign follow, and a rebuild of the factor from the
    survey -- whose rows are no longer in ascending order -- contains every row."""
    inv, _ = _survey("tiny_exp", TINY)
    eng, N = inv.engine, inv.engine.N
    scale = inv._cube_scale
    ng, nm = inv.gravfield.size, inv.magfield.size
    sel0, y0 = inv._sel.copy(), inv.Fs3[ng + nm:].copy()
    v1, y1 = _new_rows(inv, seed=21)
    inv.assimilate_drill(v1, y1, normalised=True)
    kept = dict(mu=inv.mu_rec.copy(), var=np.diag(inv.cov_rec).copy(), logl=inv.logl, sel=inv._sel.copy(), Fs3=inv.Fs3.copy(),
                state=_engine_state(eng))
    t1 = inv.propose_drill_campaign(3, update="append")
    assert len(t1) == 3 and eng.mean_var_known()
    assert np.array_equal(inv.mu_rec, kept["mu"]) and np.array_equal(np.diag(inv.cov_rec), kept["var"]) and inv.logl == kept["logl"]
    assert np.array_equal(inv._sel, kept["sel"]) and np.array_equal(inv.Fs3, kept["Fs3"]) and _same_state(kept["state"], _engine_state(eng))
    v2, y2 = _new_rows(inv, seed=22, column=False, scattered=5)
    cubes = inv.assimilate_drill(v2, y2, normalised=True)
    sel = np.concatenate([sel0, v1, v2])
    y = np.concatenate([y0, y1, y2])
    order = np.argsort(sel)
    want = _oracle(inv, sel[order], y[order], cov=False)
    errs = [normwise(np.asarray(cubes[i]).reshape(-1), want["mu"][i * N:(i + 1) * N] * scale[i]) for i in range(3)]
    errs += [normwise(np.asarray(cubes[3 + i]).reshape(-1), want["var"][i * N:(i + 1) * N] * scale[i] ** 2) for i in range(3)]
    print("assimilate, campaign, assimilate vs oracle: %s, logl %.2e" % (errs, abs(inv.logl - want["logl"]) / abs(want["logl"])))
    assert max(errs) <= 1e-10 and np.array_equal(inv._sel, sel)
    t2 = inv.propose_drill_campaign(2, update="append")
    assert len(t2) == 2 and np.array_equal(inv.mu_rec.reshape(3, -1)[2] * scale[2], np.asarray(cubes[2]).reshape(-1))
    # a rebuild from the survey: one step over the rows in the order they arrived
    inv._step_params = None
    inv._ensure_factor()
    assert np.array_equal(eng.last["sel"], sel) and eng.last["step"].Md == sel.size and eng.last.get("append") is None
    post = inv.sample_posterior(2, prior=np.zeros((2, 3, N)), noise=np.zeros((2, inv.Fs3.size)))
    for a in range(3):
        assert normwise(post[a][0].reshape(-1), np.asarray(cubes[a]).reshape(-1)) <= 1e-10
    t3 = inv.propose_drill_campaign(2, update="append")          # (the rebuilt factor carries no mean: the campaign runs a step first)
    assert t3[["NORTHING", "EASTING", "RANK"]].equals(t2[["NORTHING", "EASTING", "RANK"]])
    assert normwise(t3.UTILITY.to_numpy(), t2.UTILITY.to_numpy()) <= 1e-10


# ---- 10. workflow -----------------------------------------------------------------------------------------------------------------
def test_yaml_assimilate_drill_writes_updated_cubes(tmp_path):
    """YAML key assimilate_drill on the reference's first example: the survey with three of its four holes, then the csv of all four --
    the voxels that carry a value already are left alone, the fourth hole goes in without a step."""
    import json
    import os

    import pandas as pd
    import yaml
    from conftest import GOLDEN
    from geobo_amd import dataio, run_geobo
    f = load_golden("example1.npz")
    d = json.loads(str(f["settings_json"]))
    inpath = os.path.join(GOLDEN, "data", "synthetic")
    drill = pd.read_csv(os.path.join(inpath, d["FNAME_drilldata"]))
    sites = sorted(drill.SiteID.unique())
    drill[drill.SiteID != sites[-1]].to_csv(tmp_path / "first.csv", index=False)
    drill.to_csv(tmp_path / "all.csv", index=False)
    d.update(inpath=inpath + "/", outpath=str(tmp_path) + "/", FNAME_drilldata=str(tmp_path / "first.csv"), assimilate_drill=str(tmp_path / "all.csv"))
    y = tmp_path / "settings.yaml"
    y.write_text(yaml.safe_dump(d))
    out = run_geobo.run(str(y), bayesopt=False)
    inv, new = out["inversion"], out["assimilated_voxels"]
    d0 = np.asarray(out["inputs"][4]).reshape(-1)
    assert new.size > 0 and not d0[new].any() and np.array_equal(inv._sel, np.concatenate([np.flatnonzero(d0), new]))
    names = ["cube_density", "cube_magsus", "cube_drill", "cube_density_variance", "cube_magsus_variance", "cube_drill_variance"]
    for n in names:
        cube = dataio.read_vtkcube(str(tmp_path / (n + "_updated.vtk")))[0]
        assert np.array_equal(np.asarray(cube).reshape(out[n + "_updated"].shape), out[n + "_updated"])
        assert os.path.exists(tmp_path / (n + ".vtk"))
    # the new hole is known better than before, and nothing is known worse
    var0, var1 = np.asarray(out["cube_drill_variance"]).reshape(-1), np.asarray(out["cube_drill_variance_updated"]).reshape(-1)
    noise = (float(inv.gp_sigma[2]) * float(inv._cube_scale[2])) ** 2      # (a voxel observed with noise sigma is known to sigma^2 at the least)
    assert (var1[new] <= noise * (1.0 + 1e-9)).all() and (var1 <= var0 + 1e-8 * var0.max()).all()
