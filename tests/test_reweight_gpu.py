"""Down-weighting or dropping rows of a finished step on the device: the two kernels against the NumPy
reference, the preview against a dense solve of the edited matrix, against the committed step and against the engine on physically
fewer rows, the spectral against the generic tile source, the products that read the factor after a commit, the state, and
fold_influence."""
import numpy as np
import pytest
import torch

import _reweight_ref as R
from conftest import load_golden, normwise, settings_for

pytestmark = pytest.mark.gpu

C16 = dict(nx=16, ny=16, nz=16)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _close(got, want, tol=1e-12):
    return np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want)))


def _dinv(kind, k, rng):
    return dict(zero=np.zeros(k), finite=0.2 + 5.0 * rng.random(k), mixed=np.where(np.arange(k) % 3 == 0, 0.0, 0.2 + 5.0 * rng.random(k)))[kind]


# ---- 1. geobo_fold_factor ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zero", "finite", "mixed"])
@pytest.mark.parametrize("k", [1, 3, 16, 17, 64, 128])
def test_fold_factor_matches_reference(k, kind):
    from geobo_amd import hip
    rng = np.random.default_rng(10 * k + len(kind))
    G, a, dinv = R.spd(k, rng), rng.standard_normal(k), _dinv(kind, k, rng)
    C_w, g_w, st_w = R.fold_factor(G, dinv, a)
    ld = k + 6                                              # outputs inside larger buffers: nothing outside the k x k block moves
    Cinv = torch.full((k + 2, ld), 7.0, dtype=torch.float64, device="cuda")
    g = torch.full((k + 3,), 7.0, dtype=torch.float64, device="cuda")
    Gu = np.tril(G) + np.triu(np.full((k, k), np.nan), 1)   # only the lower triangle of G is read
    stats, st = hip.fold_factor(_dev(Gu), _dev(dinv), _dev(a), Cinv, g)
    assert int(st.cpu()[0]) == 0
    Ch, gh, sh = Cinv.cpu().numpy(), g.cpu().numpy(), stats.cpu().numpy()
    print("k = %d, %s: Cinv %.2e  g %.2e  stats %.2e %.2e" % (k, kind, np.abs(Ch[:k, :k] - C_w).max(), np.abs(gh[:k] - g_w).max(),
                                                              abs(sh[0] - st_w[0]), abs(sh[1] - st_w[1])))
    assert _close(Ch[:k, :k], C_w) and _close(gh[:k], g_w) and _close(sh, st_w)
    assert np.array_equal(Ch[:k, :k], np.tril(Ch[:k, :k]))
    assert (Ch[k:] == 7.0).all() and (Ch[:, k:] == 7.0).all() and (gh[k:] == 7.0).all()


@pytest.mark.parametrize("k,pivot", [(1, 0), (17, 0), (40, 17), (128, 127)])
def test_fold_factor_indefinite_leaves_outputs(k, pivot):
    from geobo_amd import hip
    rng = np.random.default_rng(k + pivot)
    Lw = np.linalg.cholesky(R.spd(k, rng))
    Lw[pivot, pivot] = 0.0
    S = Lw @ Lw.T                                           # the leading pivots are fine, pivot `pivot` is not:
    S[pivot, pivot] -= 1.0                                  # one negative diagonal of the Schur complement
    dinv = _dinv("mixed", k, rng)
    Cinv = _dev(rng.standard_normal((k, k)))
    g, stats = _dev(rng.standard_normal(k)), _dev(np.array([3.25, -1.5]))
    st = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    before = [t.cpu().numpy().copy() for t in (Cinv, g, stats)]
    hip.fold_factor(_dev(S - np.diag(dinv)), _dev(dinv), _dev(rng.standard_normal(k)), Cinv, g, stats=stats, status=st)
    assert int(st.cpu()[0]) == 1 + pivot
    assert all(np.array_equal(b, t.cpu().numpy()) for b, t in zip(before, (Cinv, g, stats)))


# ---- 2. geobo_rows_reweight -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiles():
    """Per k: (B (k x 4112), Cinv, g, mu0, var0) on the host, and the reference of the whole 4099-column tile -- formed once."""
    out = {}
    for k in (1, 17, 128):
        rng = np.random.default_rng(1000 + k)
        Cinv, g, _ = R.fold_factor(R.spd(k, rng), _dinv("mixed", k, rng), rng.standard_normal(k))
        B = rng.standard_normal((k, 4112))
        mu0, var0 = rng.standard_normal(4112), 1.0 + rng.random(4112)
        out[k] = dict(B=B, Cinv=Cinv, g=g, mu0=mu0, var0=var0)
    return out


def _run(t, k, c0, ncols, cubes=True):
    """geobo_rows_reweight over the columns c0 .. c0 + ncols of the tile: (mu, var, part) as host arrays (whole guarded buffers)."""
    from geobo_amd import hip
    B, Cinv, g = _dev(t["B"]), _dev(t["Cinv"]), _dev(t["g"])
    mu, var = _dev(t["mu0"]), _dev(t["var0"])
    part = hip.rows_reweight(B[:, c0:], k, Cinv, g, mu[c0:] if cubes else None, var[c0:] if cubes else None, ncols=ncols)
    assert torch.equal(B, _dev(t["B"])) and torch.equal(Cinv, _dev(t["Cinv"])) and torch.equal(g, _dev(t["g"]))
    return mu.cpu().numpy(), var.cpu().numpy(), part.cpu().numpy()


@pytest.mark.parametrize("ncols,c0", [(1, 0), (2, 0), (127, 0), (4099, 1)])
@pytest.mark.parametrize("k", [1, 17, 128])
def test_rows_reweight_matches_reference(tiles, k, ncols, c0):
    t = tiles[k]
    cols = slice(c0, c0 + ncols)
    mu_w, var_w, part_w = R.rows_reweight(t["B"][:, cols], t["Cinv"], t["g"], t["mu0"][cols], t["var0"][cols])
    mu, var, part = _run(t, k, c0, ncols)
    errs = (np.abs(mu[cols] - mu_w).max() / np.abs(mu_w).max(), np.abs(var[cols] - var_w).max() / np.abs(var_w).max(),
            np.abs(part - part_w).max() / np.abs(part_w).max())
    print("k = %d, ncols = %d at column %d: mu %.2e  var %.2e  part %.2e" % ((k, ncols, c0) + errs))
    assert max(errs) <= 1e-13
    # the sentinels: nothing in front of the tile or behind it has moved
    for got, was in ((mu, t["mu0"]), (var, t["var0"])):
        assert np.array_equal(got[:c0], was[:c0]) and np.array_equal(got[c0 + ncols:], was[c0 + ncols:])
    # statistics only: the same part bits, and no cube is written
    mu_s, var_s, part_s = _run(t, k, c0, ncols, cubes=False)
    assert np.array_equal(part_s, part) and np.array_equal(mu_s, t["mu0"]) and np.array_equal(var_s, t["var0"])


@pytest.mark.parametrize("k", [1, 17, 128])
def test_rows_reweight_column_splits_are_bit_identical(tiles, k):
    t = tiles[k]
    whole = _run(t, k, 0, 4099)
    again = _run(t, k, 0, 4099)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))       # the sums too: no atomics
    for cut in (2, 1000, 4098):
        a, b = _run(t, k, 0, cut), _run(t, k, cut, 4099 - cut)
        for j in range(2):
            assert np.array_equal(a[j][:cut], whole[j][:cut]) and np.array_equal(b[j][cut:], whole[j][cut:])
    odd = _run(t, k, 1, 4098)                                            # the 8-byte form computes the same bits
    assert np.array_equal(odd[0][1:], whole[0][1:]) and np.array_equal(odd[1][1:], whole[1][1:])


# ---- 3. the engine: preview, committed step, reduced step -------------------------------------------------------------------------
HOLES = ((3, 4), (8, 9), (12, 5))            # (iy, ix) of three holes of four voxels each: 12 drill rows


def _drill16():
    rng = np.random.default_rng(4)
    d0 = np.zeros((16, 16, 16))
    for iy, ix in HOLES:
        d0[iy, ix, 2:6] = 2.5 + 0.3 * rng.standard_normal(4)
    return d0


def _survey16(method="dense"):
    from geobo_amd.inversion import Inversion
    f = load_golden("cube16_exp.npz")
    inv = Inversion(settings=settings_for(**C16, kernelfunc="exp"), method=method)
    inv.create_cubegeometry()
    inv.gp_length = f["gp_length_in"].copy()
    d0 = _drill16()
    cubes = inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    return inv, cubes


def _step(inv, sel=None, y_d=None, gp_sigma=None):
    """One engine step on the survey of inv with the drill rows (sel, y_d) (default: its own) and noise levels gp_sigma."""
    from geobo_amd.engine import create_cov_lengths
    ng, nm = inv.gravfield.size, inv.magfield.size
    lengths = [float(v) for v in create_cov_lengths(np.array(inv.gp_length, dtype=float))]
    A_g, A_m = inv._operators()
    sel = inv._sel if sel is None else sel
    y_d = inv.Fs3[ng + nm:] if y_d is None else y_d
    return inv.engine.posterior(A_g, A_m, sel, inv.Fs3[:ng], inv.Fs3[ng:ng + nm], y_d, lengths, inv.coeffm, inv.settings.kernelfunc,
                                inv.gp_sigma if gp_sigma is None else gp_sigma, gp_amp=inv.gp_amp, props=(0, 1, 2), calclogl=True,
                                want_mean_var=True)


def _reset(inv):
    """Back to the state cubing() left: no scales, the whole step."""
    inv.restore_data()
    r = inv._run(inv.gp_amp, inv.gp_length, None, True, True)
    from geobo_amd.inversion import DiagonalCovariance
    inv.mu_rec, inv.cov_rec, inv.logl = r["mu"], DiagonalCovariance(r["var"]), r["logl"]
    return r


def _errs(got_mu, got_var, want_mu, want_var, N):
    return [normwise(np.asarray(g).reshape(-1)[i * N:(i + 1) * N], np.asarray(w).reshape(-1)[i * N:(i + 1) * N])
            for g, w in ((got_mu, want_mu), (got_var, want_var)) for i in range(3)]


@pytest.fixture(scope="module")
def s16():
    inv, cubes = _survey16("dense")
    return inv, cubes, dict(mu=inv.mu_rec.copy(), var=np.diag(inv.cov_rec).copy(), logl=inv.logl)


@pytest.mark.parametrize("rows,scale", [([37], np.inf), ([516, 517, 518, 519], np.inf), ([100, 256 + 7, 512 + 9], (np.inf, 3.0, np.inf))])
def test_preview_matches_a_dense_solve_of_the_edited_matrix(s16, rows, scale):
    inv = s16[0]
    eng, N = inv.engine, inv.engine.N
    _reset(inv)
    last = eng.last
    assert last["AK_complete"] and eng.Ms_pad == 256 and last["step"].Md == 12
    Mv = 524
    L = np.tril(last["L"][:Mv, :Mv].cpu().numpy())
    y = L @ last["u"][:Mv].cpu().numpy()
    AK = np.concatenate([last["AK"][:Mv, a * eng.nc:a * eng.nc + N].cpu().numpy() for a in range(3)], axis=1)
    sig2 = np.repeat(np.asarray(inv.gp_sigma, dtype=float) ** 2, (256, 256, 12))
    rows = np.asarray(rows)
    sc = np.broadcast_to(np.asarray(scale, dtype=float), rows.shape)
    mu_w, var_w, uu_w, logdet_w = R.direct(L @ L.T, y, AK, float(inv.gp_amp), rows, sc, sig2[rows])
    before = (last["Linv"].clone(), last["u"].clone(), last["mv"][0].clone(), last["mv"][1].clone())
    p = eng.reweight_preview(rows, sc)
    assert eng.set_source == "generic"
    errs = _errs(p["mu"].cpu().numpy(), p["var"].cpu().numpy(), mu_w, var_w, N)
    e_uu, e_ld = abs(p["uu"] - uu_w) / abs(uu_w), abs(p["logdet"] - logdet_w) / abs(logdet_w)
    print("16^3 preview of rows %s vs dense solve: cubes %s  uu %.2e  logdet %.2e" % (rows.tolist(), " ".join("%.1e" % e for e in errs), e_uu, e_ld))
    assert max(errs) <= 1e-10 and e_uu <= 1e-10 and e_ld <= 1e-10
    d = p["mu"].cpu().numpy().reshape(3, N) - np.asarray(s16[2]["mu"]).reshape(3, N)
    assert np.allclose(p["sum_dmu2"], (d ** 2).sum(axis=1), rtol=1e-8, atol=1e-20) and np.allclose(p["max_dmu"], np.abs(d).max(axis=1), rtol=1e-8)
    # nothing of the engine's state has moved, and the statistics-only preview gives the same numbers without cubes
    assert all(torch.equal(a, b) for a, b in zip(before, (last["Linv"], last["u"], last["mv"][0], last["mv"][1]))) and eng.row_scale is None
    q = eng.reweight_preview(rows, sc, want="stats")
    assert "mu" not in q and q["logl"] == p["logl"] and all(np.array_equal(q[k], p[k]) for k in ("sum_dmu2", "max_dmu", "sum_dvar"))


def test_preview_committed_step_and_reduced_step_agree(s16):
    inv = s16[0]
    eng, N = inv.engine, inv.engine.N
    ng, nm = 256, 256
    _reset(inv)
    try:
        # one hole dropped
        hole = np.arange(4, 8)
        p = eng.reweight_preview(512 + hole, np.inf)
        pmu, pvar = p["mu"].cpu().numpy(), p["var"].cpu().numpy()
        per_voxel = np.ones(N)
        per_voxel[inv._sel[hole]] = np.inf
        eng.set_row_scale(drill=per_voxel)
        c = _step(inv)
        eng.set_row_scale()
        keep = np.setdiff1d(np.arange(12), hole)
        r = _step(inv, inv._sel[keep], inv.Fs3[ng + nm:][keep])
        e_pc, e_cr = _errs(pmu, pvar, c["mu"], c["var"], N), _errs(c["mu"], c["var"], r["mu"], r["var"], N)
        l_pc, l_cr = abs(p["logl"] - c["logl"]) / abs(c["logl"]), abs(c["logl"] - r["logl"]) / abs(r["logl"])
        print("16^3 hole dropped: preview vs committed %s logl %.2e; committed vs reduced %s logl %.2e"
              % (" ".join("%.1e" % e for e in e_pc), l_pc, " ".join("%.1e" % e for e in e_cr), l_cr))
        assert max(e_pc) <= 1e-10 and l_pc <= 1e-10 and max(e_cr) <= 1e-10 and l_cr <= 1e-12
        # a finite scale on a whole data type against the step whose gp_sigma carries it
        _reset(inv)
        p = eng.reweight_preview(512 + np.arange(12), 3.0)
        pmu, pvar = p["mu"].cpu().numpy(), p["var"].cpu().numpy()
        per_voxel = np.ones(N)
        per_voxel[inv._sel] = 3.0
        eng.set_row_scale(drill=per_voxel)
        c = _step(inv)
        eng.set_row_scale()
        sig = np.asarray(inv.gp_sigma, dtype=float) * np.array([1.0, 1.0, 3.0])
        r = _step(inv, gp_sigma=sig)
        e_pc, e_cr = _errs(pmu, pvar, c["mu"], c["var"], N), _errs(c["mu"], c["var"], r["mu"], r["var"], N)
        l_pc, l_cr = abs(p["logl"] - c["logl"]) / abs(c["logl"]), abs(c["logl"] - r["logl"]) / abs(r["logl"])
        print("16^3 drill noise x 3: preview vs committed %s logl %.2e; committed vs gp_sigma %s logl %.2e"
              % (" ".join("%.1e" % e for e in e_pc), l_pc, " ".join("%.1e" % e for e in e_cr), l_cr))
        assert max(e_pc) <= 1e-10 and l_pc <= 1e-10 and max(e_cr) <= 1e-10 and l_cr <= 1e-12
    finally:
        _reset(inv)


def test_spectral_source_matches_generic_source():
    """64 x 48 x 64 with 5 drill voxels on the transposed route: the preview of one station and of the drill rows, B from the
    spectral tile generator against the generic one."""
    import bench
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=settings_for(64, 48, 64, kernelfunc="matern32"))
    grav, mag, loc, drill0 = bench.synthetic_inputs(inv, 5)
    inv.gp_length = np.array([200.0, 202.0, 204.0])
    inv.cubing(grav, mag, drill0[drill0 != 0], loc, drill0)
    eng = inv.engine
    Mu = inv.Fs3.size
    for rows in ([1000], list(range(Mu - 5, Mu))):
        a = eng.reweight_preview(rows, np.inf, source="spectral")
        b = eng.reweight_preview(rows, np.inf, source="generic")
        errs = [normwise(a[k][i].cpu().numpy(), b[k][i].cpu().numpy()) for k in ("mu", "var") for i in range(3)]
        e_l = abs(a["logl"] - b["logl"]) / abs(b["logl"])
        print("64x48x64 rows %s: spectral vs generic source %s logl %.2e" % (rows[:2], " ".join("%.1e" % e for e in errs), e_l))
        assert max(errs) <= 1e-12 and e_l <= 1e-12


# ---- 4. consumers after a commit ---------------------------------------------------------------------------------------------------
def test_consumers_after_a_commit_see_the_reduced_system(s16):
    inv = s16[0]
    eng, N = inv.engine, inv.engine.N
    ng, nm = 256, 256
    hole = np.arange(4, 8)
    keep = np.setdiff1d(np.arange(12), hole)
    _reset(inv)
    ref, _ = _survey16("dense")                       # the same survey stepped on the physically reduced drill set
    ref._sel, ref.Fs3 = inv._sel[keep].copy(), np.concatenate([inv.Fs3[:ng + nm], inv.Fs3[ng + nm:][keep]])
    r = _reset(ref)
    rng = np.random.default_rng(8)
    s = inv.settings
    pts = np.stack([rng.uniform(s.xmin + 50, s.xmax - 50, 20), rng.uniform(s.ymin + 50, s.ymax - 50, 20),
                    inv.voxelpos[2].min() + rng.uniform(0.1, 0.9, 20) * (inv.voxelpos[2].max() - inv.voxelpos[2].min())], axis=1)
    first = inv.sample_posterior(2, seed=3)
    try:
        out = inv.reweight_data(drill=hole, commit=True)
        assert max(_errs(inv.mu_rec, np.diag(inv.cov_rec), r["mu"], r["var"], N)) <= 1e-10
        assert abs(out["logl"] - r["logl"]) <= 1e-12 * abs(r["logl"]) and inv.logl == out["logl"]
        hs, hr = inv.hole_statistics(), ref.hole_statistics()
        ok = hr["status"] == 0
        assert np.array_equal(hs["status"], hr["status"])
        assert max(normwise(hs[k][ok], hr[k][ok]) for k in ("info_gain", "path_std", "sum_var")) <= 1e-10
        pp, pr = inv.predict_points(pts), ref.predict_points(pts)
        assert max(normwise(pp[k], pr[k]) for k in ("mean", "var")) <= 1e-10
        bs, br = inv.block_statistics((4, 4, 4)), ref.block_statistics((4, 4, 4))
        assert max(normwise(bs[k], br[k]) for k in ("mean", "cov")) <= 1e-10
        cv, cr = inv.cross_validate("loo"), ref.cross_validate("loo")
        assert (cv["drill"]["fold"][hole] == -1).all() and np.isnan(cv["drill"]["z"][hole]).all() and np.isnan(cv["drill"]["residual"][hole]).all()
        assert (cv["drill"]["fold"][keep] >= 0).all()
        for name, pick in (("grav", slice(None)), ("magn", slice(None)), ("drill", keep)):
            assert normwise(cv[name]["residual"][pick], cr[name]["residual"]) <= 1e-10 and normwise(cv[name]["std"][pick], cr[name]["std"]) <= 1e-10
        with pytest.raises(ValueError, match="dropped already"):
            inv.reweight_data(drill=hole[:1])
        with pytest.raises(ValueError, match="dropped already"):
            inv.reweight_data(drill=hole[:1], commit=True)
        again = inv.sample_posterior(2, seed=3)
        vox = inv._sel[hole]
        assert not np.array_equal(again[2].reshape(2, -1)[:, vox], first[2].reshape(2, -1)[:, vox])
        # a fresh voxel still goes in by the append, on top of the reduced system
        new = np.array([[5, 11, 7]])
        flat = (5 * 16 + 11) * 16 + 7
        got = inv.assimilate_drill(new, [0.4], normalised=True)
        ref._sel, ref.Fs3 = np.concatenate([ref._sel, [flat]]), np.concatenate([ref.Fs3, [0.4]])
        want = ref._six_cubes(*[_reset(ref)[k] for k in ("mu", "var")])
        assert max(normwise(g, w) for g, w in zip(got, want)) <= 1e-10
    finally:
        if inv._sel.size > 12:
            eng.truncate_drill_rows(12)
            inv._sel, inv.Fs3 = inv._sel[:12], inv.Fs3[:ng + nm + 12]
        _reset(inv)


# ---- 5. state ------------------------------------------------------------------------------------------------------------------------
def test_restore_returns_the_bits_and_all_ones_launch_nothing_new(s16):
    inv, _, first = s16
    eng = inv.engine
    _reset(inv)
    try:
        inv.reweight_data(grav=[5, 9], magn=[17], drill=[[8, 9, 3]], scale=(np.inf, 2.0, np.inf, 4.0), commit=True)
        assert np.isinf(eng.row_scale["grav"][5]) and eng.row_scale["grav"][9] == 2.0 and eng.row_scale["drill"][(8 * 16 + 9) * 16 + 3] == 4.0
        assert not np.array_equal(inv.mu_rec, first["mu"])
        assert eng.dropped_rows().tolist() == [5, 256 + 17]
    finally:
        r = _reset(inv)
    assert eng.row_scale is None and np.array_equal(r["mu"], first["mu"]) and np.array_equal(r["var"], first["var"]) and r["logl"] == first["logl"]
    # the launches of a step: attribute absent, then present with every scale at one
    names = []
    for scales in (None, dict(grav=np.ones(256), magn=np.ones(256), drill=np.ones(eng.N))):
        eng.row_scale = scales
        eng.kernel_events = []
        try:
            r2 = _step(inv)
        finally:
            names.append([e[0] for e in eng.kernel_events])
            eng.kernel_events = None
            eng.row_scale = None
        assert np.array_equal(r2["mu"], first["mu"]) and np.array_equal(r2["var"], first["var"])
    assert names[0] == names[1] and len(names[0]) > 0 and not any(n.startswith("reweight") for n in names[0])
    _reset(inv)


def test_rejections(s16):
    inv = s16[0]
    eng = inv.engine
    _reset(inv)
    for rows, scale, what in (([3], 0.5, "below 1"), ([3], float("nan"), "below 1"), (list(range(129)), np.inf, "at most 128"),
                              ([3, 7, 3], np.inf, "twice"), ([], np.inf, "at least one"), ([524], np.inf, r"\[0, 524\)")):
        with pytest.raises(ValueError, match=what):
            eng.reweight_preview(rows, scale)
    with pytest.raises(ValueError, match="twice"):
        inv.reweight_data(grav=[3, 3])
    with pytest.raises(ValueError, match="no drill value"):
        inv.reweight_data(drill=[[0, 0, 0]])
    with pytest.raises(ValueError, match="below 1"):
        inv.reweight_data(grav=[3], scale=0.9, commit=True)
    assert eng.row_scale is None


# ---- 6. fold_influence ---------------------------------------------------------------------------------------------------------------
def test_fold_influence_ranks_the_planted_outlier_first():
    """An outlier is one against a background that fits: the drill values of this survey are the prior mean plus half a noise
    standard deviation of scatter (the z-scored random values of _drill16 differ by about one prior standard deviation from voxel
    to voxel, so every hole of that survey is as far off as a hole moved by 10 sigma_d = 1), then one hole is moved by 10 sigma_d."""
    inv, _ = _survey16("dense")
    sigma_d = float(inv.gp_sigma[2])
    inv.Fs3[512:] = 0.5 * sigma_d * np.random.default_rng(6).standard_normal(12)
    inv.Fs3[512 + 4:512 + 8] += 10.0 * sigma_d                            # hole 1 lies ten noise standard deviations off
    inv._step_params = None
    _reset(inv)
    table = inv.fold_influence("holes")
    print(table[table.SIZE == 4].to_string())
    assert len(table) == 512 + 3 and table.RANK.tolist() == list(range(1, 516))
    top = table.iloc[0]
    assert int(top.SIZE) == 4 and int(top.FIRST_ROW) == 512 + 4           # the hole that carries the outlier
    for h in range(3):
        one = inv.reweight_data(drill=np.arange(4 * h, 4 * h + 4))
        row = table[table.FIRST_ROW == 512 + 4 * h].iloc[0]
        assert abs(row.DELTA_LOGL - one["delta_logl"]) <= 1e-10 * abs(one["delta_logl"])
        got = np.array([row.RMS_DENSITY, row.RMS_MAGSUS, row.RMS_DRILL])
        assert np.all(np.abs(got - one["rms_change"]) <= 1e-10 * np.abs(one["rms_change"]))


# ---- 7. workflow ---------------------------------------------------------------------------------------------------------------------
def test_yaml_drop_data_writes_the_dropped_cubes(tmp_path):
    """YAML key drop_data on the reference's first example: the scales are committed after cubing() and the cubes are written."""
    import json
    import os

    import yaml
    from conftest import GOLDEN
    from geobo_amd import dataio, run_geobo
    d = json.loads(str(load_golden("example1.npz")["settings_json"]))
    d.update(inpath=os.path.join(GOLDEN, "data", "synthetic") + "/", outpath=str(tmp_path) + "/", drop_data=dict(grav=[3], drill=[0, 1]))
    y = tmp_path / "settings.yaml"
    y.write_text(yaml.safe_dump(d))
    out = run_geobo.run(str(y), bayesopt=False)
    inv = out["inversion"]
    ng, nm = inv.gravfield.size, inv.magfield.size
    assert inv.engine.dropped_rows().tolist() == [3, ng + nm, ng + nm + 1] and out["dropped_data"]["rows"].tolist() == [3, ng + nm, ng + nm + 1]
    for n in ["cube_density", "cube_magsus", "cube_drill", "cube_density_variance", "cube_magsus_variance", "cube_drill_variance"]:
        cube = dataio.read_vtkcube(str(tmp_path / (n + "_dropped.vtk")))[0]
        assert np.array_equal(np.asarray(cube).reshape(out[n + "_dropped"].shape), out[n + "_dropped"])
        assert os.path.exists(tmp_path / (n + ".vtk")) and not np.array_equal(out[n + "_dropped"], out[n])
    # less data: nothing is known better than before
    var0, var1 = np.asarray(out["cube_drill_variance"]).reshape(-1), np.asarray(out["cube_drill_variance_dropped"]).reshape(-1)
    assert (var1 >= var0 - 1e-8 * var0.max()).all()
