"""Grade-tonnage curves on the device: geobo_cutoff_stats and geobo_box_means against the NumPy reference of
_gradetonnage_ref, grade_tonnage against thresholding the host realisations of sample_posterior (voxel and block support, batching
and addressing), the empirical exceedance frequencies against the analytic ones, the region mean against block_statistics, a spectral
step at 32^3 and the error paths.

Sums: every order of adding n numbers is within (n - 1) 2^-53 sum |w x| of the exact sum; the tests ask for twice that (the rounding
of w x, of the scale and of the reference's own last rounding)."""
import numpy as np
import pytest
import torch

import _gradetonnage_ref as ref
from conftest import load_golden, settings_for

pytestmark = pytest.mark.gpu

SEED = 2026
PSD_W = (0.2, 0.2, 0.2)
TINY = dict(nx=10, ny=8, nz=6)
GRID = (8, 10, 6)                                             # (ny, nx, nz)
N = 480
VOXVOL = 100.0 ** 3


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype,
                                                                                                           device="cuda")


# ---- 1. geobo_cutoff_stats by value ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("n", [27, 420, 481, 32768])
def test_cutoff_stats_by_value(n, S):
    from geobo_amd import hip
    rng = np.random.default_rng(1000 * S + n)
    p = 1                                                      # (n = 481: the second property starts at an odd element)
    F = rng.standard_normal((S, 3, n))
    F[0, p, 5] = np.nan                                        # fails every cutoff, -inf included
    F[S - 1, 0, 11] = np.nan                                   # fails the lower bound
    F[0, 0, 17] = 0.0                                          # (element 17 of sample 0 meets the lower bound and the mask)
    exact = F[0, p, 17]                                        # a cutoff equal to an element bit for bit: >= counts it
    q = np.nanquantile(F[:, p], [0.25, 0.5])
    t = np.sort(np.array([-np.inf, q[0], q[1], q[1], exact, np.nanmax(F[:, p]) + 1.0]))
    lo = np.array([-0.8, -np.inf, -np.inf])
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    mask[17] = 1
    weight = rng.integers(1, 49, size=n).astype(np.int32)
    cnt_r, sum_r, abs_r, _, passes = ref.cutoff_stats(F, p, t, lo=lo, mask=mask, weight=weight)
    assert passes[0, list(t).index(exact), 17]                 # the tie is in the reference
    assert (cnt_r[:, -1] == 0).all() and (cnt_r[:, 0] > 0).all()

    Fd, md, wd = _dev(F), _dev(mask), _dev(weight)
    hits = torch.zeros((t.size, n), dtype=torch.int32, device="cuda")
    ws = torch.full((hip.cutoff_stats_ws_doubles(S, n, t.size),), float("nan"), dtype=torch.float64, device="cuda")
    cnt, tot = hip.cutoff_stats(Fd, p, t, lo=lo, mask=md, weight=wd, hits=hits, ws=ws)
    cnt, tot, h = cnt.cpu().numpy(), tot.cpu().numpy(), hits.cpu().numpy()
    err = np.abs(tot - sum_r)
    bound = ref.sum_bound(n, abs_r)
    print("cutoff_stats n = %d S = %d: max |sum - fsum| %.3e, bound there %.3e" % (n, S, err.max(), bound.reshape(-1)[err.argmax()]))
    assert np.array_equal(cnt, cnt_r)
    assert np.array_equal(h, passes.sum(0).astype(np.int32))
    assert np.all(err <= bound)
    # hits accumulate over calls; without hits, mask and weights the other kernel instance gives the plain counts
    hip.cutoff_stats(Fd, p, t, lo=lo, mask=md, weight=wd, hits=hits)
    assert np.array_equal(hits.cpu().numpy(), 2 * h)
    cnt1, tot1 = hip.cutoff_stats(Fd, p, t)
    c1, s1, a1, _, _ = ref.cutoff_stats(F, p, t)
    assert np.array_equal(cnt1.cpu().numpy(), c1) and np.all(np.abs(tot1.cpu().numpy() - s1) <= ref.sum_bound(n, a1))
    # one launch per sample: the same bits
    for s in range(S):
        c_s, t_s = hip.cutoff_stats(Fd[s:s + 1], p, t, lo=lo, mask=md, weight=wd)
        assert np.array_equal(c_s.cpu().numpy()[0], cnt[s])
        assert np.array_equal(t_s.cpu().numpy()[0].view(np.int64), tot[s].view(np.int64)), s


# ---- 2. geobo_box_means -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [(1, 1, 1), (3, 4, 4), (8, 10, 6)])
def test_box_means(box):
    from geobo_amd import hip
    from geobo_amd.blocksupport import block_partition
    rng = np.random.default_rng(7)
    S = 3
    F = rng.standard_normal((S, 3, N))
    F[1, 2, 40] = -0.0
    Fd = _dev(F)
    G, count = hip.box_means(Fd, GRID, box)
    G, count = G.cpu().numpy(), count.cpu().numpy()
    _, cnt_r = block_partition(GRID, box)
    assert count.dtype == np.int32 and np.array_equal(count, cnt_r)
    if box == (1, 1, 1):
        assert np.array_equal(G.view(np.int64), F.view(np.int64))             # bit for bit, the sign of -0.0 included
    G_r, A_r, _ = ref.box_means(F, GRID, box)
    err = np.abs(G - G_r)
    bound = ref.sum_bound(cnt_r, A_r) / cnt_r                                  # (n = the voxels of the box; 0 for a single voxel)
    print("box_means %s: max error %.3e" % (box, err.max()))
    assert np.all(err <= bound)
    for s in range(S):
        one, _ = hip.box_means(Fd[s:s + 1], GRID, box)
        assert np.array_equal(one.cpu().numpy()[0].view(np.int64), G[s].view(np.int64))


# ---- 3 .. 6: grade_tonnage on the 10 x 8 x 6 survey -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """The inversion after cubing() and its 16 host realisations (cube units), computed once and left unchanged."""
    from geobo_amd.inversion import Inversion
    f = load_golden("tiny_exp.npz")
    s = settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W))
    inv = Inversion(settings=s)
    inv.create_cubegeometry()
    inv.gp_length = np.array([200.0, 204.0, 208.0])
    d0 = f["drilldata0"]
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    host = np.stack([c.reshape(16, N) for c in inv.sample_posterior(16, seed=SEED)], 1)          # (16, 3, N)
    host.setflags(write=False)
    return dict(inv=inv, host=host)


def _midpoint_cutoffs(values, scale, k=5):
    """k cutoffs half way between neighbours of the sorted values, none within 1e-9 scale of a value."""
    v = np.sort(np.asarray(values).reshape(-1))
    idx = (np.linspace(0.1, 0.9, k) * (v.size - 1)).astype(int)
    cut = 0.5 * (v[idx] + v[idx + 1])
    assert np.abs(v[None, :] - cut[:, None]).min() > 1e-9 * float(scale)
    return cut


def test_grade_tonnage_matches_host_route(tiny):
    inv, host = tiny["inv"], tiny["host"]
    p = 2
    cut = _midpoint_cutoffs(host[:, p], inv._cube_scale[p])[[3, 0, 4, 1, 2]]                    # (the caller's order is kept)
    cnt_r, sum_r, abs_r, _, passes = ref.cutoff_stats(host, p, cut)
    out = inv.grade_tonnage(cut, prop="drill", n=16, seed=SEED, voxel_probability=True)
    assert np.array_equal(out["cutoffs"], cut)
    assert out["count"].dtype == np.int64 and np.array_equal(out["count"], cnt_r)
    err = np.abs(out["quantity"] - sum_r * VOXVOL)
    print("grade_tonnage: max quantity error %.3e of %.3e" % (err.max(), np.abs(sum_r * VOXVOL).max()))
    assert np.all(err <= ref.sum_bound(N, abs_r) * VOXVOL)
    assert np.array_equal(out["volume"], cnt_r * VOXVOL)
    assert out["probability"].shape == (5, 8, 10, 6)
    assert np.array_equal(out["probability"].reshape(5, N), passes.sum(0) / 16.0)
    assert out["quantiles"]["volume"].shape == (3, 5)
    # the batching changes no bit, and realisations are addressed by their absolute index
    two = inv.grade_tonnage(cut, prop=2, n=16, seed=SEED, batch=2)
    part = inv.grade_tonnage(cut, prop=2, n=8, seed=SEED, start=4)
    for k in ("count", "quantity"):
        assert np.array_equal(two[k], out[k]), k
        assert np.array_equal(part[k], out[k][4:12]), k
    # an offset moves the cutoffs and the values together
    off = inv.grade_tonnage(cut + 3.5, prop=2, n=16, seed=SEED, offset=3.5)
    assert np.array_equal(off["count"], cnt_r)
    assert np.allclose(off["quantity"], out["quantity"] + 3.5 * cnt_r * VOXVOL, rtol=1e-12, atol=0)
    # a region and a bound on another property, at voxel support
    region = np.zeros(GRID, dtype=bool)
    region[2:7, 1:9, :4] = True
    bound_d = float(np.median(host[:, 0]))
    c2, s2, a2, _, _ = ref.cutoff_stats(host, p, cut, lo=[bound_d, -np.inf, -np.inf], mask=region.reshape(-1))
    sub = inv.grade_tonnage(cut, prop=2, n=16, seed=SEED, region=region, require={"density": bound_d})
    assert np.abs(host[:, 0] - bound_d).min() > 1e-9 * float(inv._cube_scale[0])
    assert np.array_equal(sub["count"], c2) and np.all(np.abs(sub["quantity"] - s2 * VOXVOL) <= ref.sum_bound(N, a2) * VOXVOL)


def test_grade_tonnage_block_support(tiny):
    """Blocks of (bx, by, bz) = (4, 3, 4) voxels.  The device's block mean and the reference's (math.fsum / count) each lie within
    (n_B - 1) u sum_B |x| / n_B of the exact mean (n_B <= 48), the sum over the 18 blocks adds (18 - 1) u sum |w m|: in all
    (47 + 17) u sum |x| over the voxels of the passing blocks, asked for with the factor 2 of the other tests."""
    from geobo_amd.blocksupport import block_partition
    inv, host = tiny["inv"], tiny["host"]
    p = 1
    box = (3, 4, 4)                                            # (by, bx, bz)
    means, absb, count = ref.box_means(host, GRID, box)
    assert np.array_equal(count, block_partition(GRID, box)[1]) and count.size == 18
    cut = _midpoint_cutoffs(means[:, p], inv._cube_scale[p])
    cnt_r, sum_r, _, _, passes = ref.cutoff_stats(means, p, cut, weight=count)
    out = inv.grade_tonnage(cut, prop="magsus", n=16, seed=SEED, block=(4, 3, 4), voxel_probability=True)
    assert np.array_equal(out["count"], cnt_r)
    abs_vox = np.einsum("scb,sb->sc", passes.astype(np.float64), absb[:, p])
    err = np.abs(out["quantity"] - sum_r * VOXVOL)
    print("block support: max quantity error %.3e of %.3e" % (err.max(), np.abs(sum_r * VOXVOL).max()))
    assert np.all(err <= 2.0 * (47 + 17) * ref.U * abs_vox * VOXVOL)
    assert out["probability"].shape == (5, 3, 3, 2) and np.array_equal(out["probability"].reshape(5, 18), passes.sum(0) / 16.0)
    region = np.ones((3, 3, 2), dtype=bool)
    region[0] = False
    c2 = ref.cutoff_stats(means, p, cut, weight=count, mask=region.reshape(-1))[0]
    assert np.array_equal(inv.grade_tonnage(cut, prop=1, n=16, seed=SEED, block=(4, 3, 4), region=region)["count"], c2)


def test_empirical_against_analytic(tiny):
    inv = tiny["inv"]
    n = 512
    mean = inv.mu_rec.reshape(3, N)[0] * inv._cube_scale[0]
    cut = np.quantile(mean, [0.25, 0.5, 0.75])
    out = inv.grade_tonnage(cut, prop="density", n=n, seed=SEED, voxel_probability=True)
    pa = inv.exceedance_probability(cut, "density")
    assert pa.shape == out["probability"].shape == (3, 8, 10, 6) and np.isfinite(pa).all()
    dev = np.abs(out["probability"] - pa)
    bound = 5.0 * np.sqrt(pa * (1.0 - pa) / n) + 1.0 / n
    print("empirical vs analytic: worst deviation / bound %.3f" % (dev / bound).max())
    assert np.all(dev <= bound)


def test_region_mean_against_block_statistics(tiny):
    inv = tiny["inv"]
    n, a = 512, 0
    blocks = inv.block_statistics((4, 3, 4))
    jy, jx, jz = 1, 1, 0                                       # an interior box: 3 x 4 x 4 voxels
    assert blocks["count"][jy, jx, jz] == 48
    region = np.zeros(GRID, dtype=bool)
    region[3:6, 4:8, 0:4] = True
    out = inv.grade_tonnage([-np.inf], prop=a, n=n, seed=SEED, region=region)
    assert (out["count"] == 48).all()
    g = out["grade"][:, 0]                                     # the region's mean, one per realisation
    var, mu = blocks["cov"][jy, jx, jz, a, a], blocks["mean"][a, jy, jx, jz]
    ratio = g.var(ddof=1) / var
    print("region mean: variance ratio %.4f, mean off by %.2f standard errors" % (ratio, abs(g.mean() - mu) / np.sqrt(var / n)))
    assert abs(ratio - 1.0) <= 5.0 * np.sqrt(2.0 / (n - 1))
    assert abs(g.mean() - mu) <= 5.0 * np.sqrt(var / n)


# ---- 7. a spectral step at 32^3 -------------------------------------------------------------------------------------------------
def test_grade_tonnage_at_32():
    from geobo_amd.inversion import Inversion
    f = load_golden("oracle32_exp.npz")
    d0 = np.zeros((32, 32, 32))                                 # (this survey has no drill data)
    s = settings_for(32, 32, 32, kernelfunc="exp", gp_coeff=list(PSD_W))
    inv = Inversion(settings=s, method="spectral")
    inv.create_cubegeometry()
    inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    n, M = 8, 32 ** 3
    got = inv.sample_posterior(n, seed=SEED)
    host = np.stack([got[i].reshape(n, M) for i in range(2)] + [np.zeros((n, M))], 1)
    cut = _midpoint_cutoffs(host[:, 0], inv._cube_scale[0], k=4)
    cnt_r, sum_r, abs_r, _, passes = ref.cutoff_stats(host, 0, cut)
    out = inv.grade_tonnage(cut, prop="density", n=n, seed=SEED, voxel_probability=True)
    assert np.array_equal(out["count"], cnt_r)
    assert np.all(np.abs(out["quantity"] - sum_r * VOXVOL) <= ref.sum_bound(M, abs_r) * VOXVOL)
    assert np.array_equal(out["probability"].reshape(4, M), passes.sum(0) / float(n))
    with pytest.raises(ValueError, match="drill"):
        inv.grade_tonnage(cut, prop="drill", n=2)


# ---- workflow ---------------------------------------------------------------------------------------------------------------------
def test_yaml_key_writes_the_curve_and_the_cubes(tmp_path):
    """YAML key grade_tonnage on the reference's first example (25 x 16 x 16, non-cubic voxels), exponential kernel and the PSD weights."""
    import json
    import os

    import pandas as pd
    import yaml
    from conftest import GOLDEN
    from geobo_amd import dataio, resources, run_geobo
    f = load_golden("example1.npz")
    d = json.loads(str(f["settings_json"]))
    d.update(inpath=os.path.join(GOLDEN, "data", "synthetic") + "/", outpath=str(tmp_path) + "/", kernelfunc="exp", gp_coeff=list(PSD_W),
             sample_seed=3, grade_tonnage=dict(property="density", cutoffs=[0.05, -0.05, 0.0], samples=6, voxel_probability=True))
    y = tmp_path / "settings.yaml"
    y.write_text(yaml.safe_dump(d))
    out = run_geobo.run(str(y), bayesopt=False)
    got = out["grade_tonnage"]
    inv = out["inversion"]
    again = inv.grade_tonnage([0.05, -0.05, 0.0], prop="density", n=6, seed=3, voxel_probability=True)
    assert got["count"].shape == (6, 3) and np.array_equal(got["count"], again["count"]) and np.array_equal(got["quantity"], again["quantity"])
    assert np.all(got["count"][:, 1] >= got["count"][:, 2]) and np.all(got["count"][:, 2] >= got["count"][:, 0])
    tab = pd.read_csv(tmp_path / "grade_tonnage.csv")
    assert list(tab.columns) == list(resources.CSV_COLUMNS) and np.array_equal(tab["CUTOFF"], [0.05, -0.05, 0.0])
    assert np.allclose(tab["VOLUME_P50"], got["quantiles"]["volume"][1], rtol=1e-12, atol=0)
    s = inv.settings
    assert got["probability"].shape == (3, s.yNcube, s.xNcube, s.zNcube)
    for k in range(3):
        cube = dataio.read_vtkcube(str(tmp_path / ("cube_density_exceed_%d.vtk" % k)))[0]
        assert np.array_equal(cube, got["probability"][k])


# ---- 8. error paths -------------------------------------------------------------------------------------------------------------
def test_error_paths(tiny):
    from geobo_amd.inversion import Inversion
    inv = tiny["inv"]
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=settings_for(**TINY)).grade_tonnage([0.0], prop="density")
    with pytest.raises(ValueError):
        inv.grade_tonnage(np.arange(33.0), prop="density", n=2)
    with pytest.raises(ValueError, match="region"):
        inv.grade_tonnage([0.0], prop="density", n=2, region=np.ones((10, 8, 6), dtype=bool))
    with pytest.raises(ValueError, match="region"):
        inv.grade_tonnage([0.0], prop="density", n=2, block=(4, 3, 4), region=np.ones(GRID, dtype=bool))
    with pytest.raises(ValueError):
        inv.grade_tonnage([0.0], prop="density", n=2, block=(11, 3, 4))
    with pytest.raises(ValueError):
        inv.grade_tonnage([0.0], prop="density", n=2, require={"density": 0.0})
    f = load_golden("tiny_exp_nodrill.npz")
    nod = Inversion(settings=settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W)))
    nod.create_cubegeometry()
    nod.gp_length = np.array([200.0, 204.0, 208.0])
    d0 = f["drilldata0"]
    nod.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    with pytest.raises(ValueError, match="drill"):
        nod.grade_tonnage([0.0], prop="drill", n=2)
    with pytest.raises(ValueError, match="drill"):
        nod.grade_tonnage([0.0], prop="density", n=2, require={"drill": 0.0})
