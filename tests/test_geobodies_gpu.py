"""Connected ore bodies on the device: geobo_bodies against the SciPy reference of _geobodies_ref (labels, counts
and hit cubes exactly, sums within the bound of section 17), its reproducibility, Inversion.geobodies against thresholding and labelling
the host realisations of sample_posterior, label_bodies against scipy.ndimage.label, a spectral step at 32^3, the YAML key and the
error paths.

Sums: every order of adding n numbers is within (n - 1) 2^-53 sum |w x| of the exact sum; the tests ask for twice that (section 17).
No test provokes a fault: the bounded walks of the union-find are checked by reading that `info` stays 0."""
import numpy as np
import pytest
import torch

import _geobodies_ref as ref
import _gradetonnage_ref as gt
from conftest import load_golden, settings_for

pytestmark = pytest.mark.gpu

SEED = 2026
PSD_W = (0.2, 0.2, 0.2)
TINY = dict(nx=10, ny=8, nz=6)
GRID = (8, 10, 6)                                             # (ny, nx, nz)
N = 480
VOXVOL = 100.0 ** 3
GRIDS = [(1, 1, 1), (1, 1, 70), (3, 1, 130), (5, 7, 9), (16, 16, 16), (64, 64, 1), (1, 1, 4096)]


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype,
                                                                                                           device="cuda")


def _case(batch, rng, dressed):
    """A batch of boolean patterns -> (F (S, 3, n), p, t, lo, mask, weight, exact): property p is positive on the pattern and negative
    off it; the cutoffs are -inf (everything), 0 (the pattern), a value equal to an element bit for bit (a part of the pattern) and
    one above everything (nothing).  dressed: NaN values, a mask, a lower bound on another property and weights on top."""
    S, n = len(batch), batch[0].size
    p = 1
    F = rng.standard_normal((S, 3, n))
    for s, pat in enumerate(batch):
        F[s, p] = np.where(pat.reshape(-1), rng.uniform(0.5, 1.5, n), rng.uniform(-1.5, -0.5, n))
    lo, mask, weight = None, None, None
    if dressed:
        F[0, p, n // 3] = np.nan                               # outside every set, -inf included
        F[S - 1, 0, n // 2] = np.nan                           # fails the lower bound
        lo = np.array([-1.0, -np.inf, -np.inf])
        mask = (rng.random(n) < 0.9).astype(np.uint8)
        weight = rng.integers(1, 49, size=n).astype(np.int32)
    live = batch[0].reshape(-1) & ~np.isnan(F[0, p])
    if dressed:
        live &= (mask != 0) & (F[0, 0] >= lo[0])
    exact = F[0, p, np.flatnonzero(live)[live.sum() // 2]] if live.any() else 1.0
    t = np.sort(np.array([-np.inf, 0.0, exact, 9.0]))
    return F, p, t, lo, mask, weight, (int(np.flatnonzero(F[0, p] == exact)[0]) if live.any() else None)


# ---- 1. geobo_bodies by value ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("neighbours", [6, 26])
@pytest.mark.parametrize("grid", GRIDS)
def test_bodies_by_value(grid, neighbours, S):
    from geobo_amd import hip
    n = grid[0] * grid[1] * grid[2]
    rng = np.random.default_rng(1000 * n + 10 * neighbours + S)
    pats = ref.patterns(grid, rng)
    seeds = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, size=min(n, 6))])).astype(np.int32)
    Cn = 4
    hl = torch.zeros((Cn, n), dtype=torch.int32, device="cuda")
    hs = torch.zeros((Cn, n), dtype=torch.int32, device="cuda")
    hl_r, hs_r = np.zeros((Cn, n), dtype=np.int64), np.zeros((Cn, n), dtype=np.int64)
    ws = torch.full((hip.bodies_ws_doubles(S, grid, Cn),), float("nan"), dtype=torch.float64, device="cuda")
    worst = 0.0
    for b0 in range(0, len(pats), S):
        names = [pats[(b0 + i) % len(pats)][0] for i in range(S)]
        batch = [pats[(b0 + i) % len(pats)][1] for i in range(S)]
        for dressed in (False, True):
            what = "%s dressed %s" % (names, dressed)
            F, p, t, lo, mask, weight, at = _case(batch, rng, dressed)
            r = ref.bodies(F, grid, p, t, lo=lo, mask=mask, weight=weight, neighbours=neighbours, min_count=1, seeds=seeds)
            if at is not None:
                assert r["labels"][0, list(t).index(F[0, p, at]), at] >= 0        # the tie is in the reference: >= counts it
            Fd = _dev(F)
            md = None if mask is None else _dev(mask)
            wd = None if weight is None else _dev(weight)
            lab = torch.full((S, Cn, n), -7, dtype=torch.int32, device="cuda")
            st, sm, info = hip.bodies(Fd, grid, p, t, lo=lo, mask=md, weight=wd, neighbours=neighbours, min_count=1, seeds=seeds,
                                      hits_largest=hl, hits_seeded=hs, labels=lab, ws=ws)
            assert int(info.item()) == 0, what
            st_h, sm_h = st.cpu().numpy(), sm.cpu().numpy()
            assert np.array_equal(lab.cpu().numpy(), r["labels"]), what            # the canonical label: each body's smallest index
            assert np.array_equal(st_h, r["stats"]), what
            err, bound = np.abs(sm_h - r["sums"]), ref.sum_bound(n, r["abs"])
            worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
            assert np.all(err <= bound), what
            hl_r += r["in_largest"].sum(0)
            hs_r += r["in_seeded"].sum(0)
            assert np.array_equal(hl.cpu().numpy(), hl_r) and np.array_equal(hs.cpu().numpy(), hs_r), what    # accumulated over the calls
            # a second run (bodies of at least 5, no labels, no hits): the same bits, and its own body count
            st5, sm5, info5 = hip.bodies(Fd, grid, p, t, lo=lo, mask=md, weight=wd, neighbours=neighbours, min_count=5, seeds=seeds)
            assert int(info5.item()) == 0
            st5 = st5.cpu().numpy()
            assert np.array_equal(st5[..., 1], ref.count_bodies(r["labels"], weight, 5)), what
            assert np.array_equal(np.delete(st5, 1, axis=2), np.delete(st_h, 1, axis=2)) and np.array_equal(sm5.cpu().numpy(), sm_h), what
            # the merge without its tile-local phase: the same labels and tables
            lab_p = torch.full((S, Cn, n), -7, dtype=torch.int32, device="cuda")
            stp, smp, infop = hip.bodies(Fd, grid, p, t, lo=lo, mask=md, weight=wd, neighbours=neighbours, seeds=seeds, labels=lab_p, tiled=False)
            assert int(infop.item()) == 0 and np.array_equal(lab_p.cpu().numpy(), r["labels"]), what
            assert np.array_equal(stp.cpu().numpy(), st_h) and np.array_equal(smp.cpu().numpy(), sm_h), what
            # a sample alone, and a cutoff alone: the bits of the batch
            for s in range(S if S > 1 else 0):
                s1, m1, i1 = hip.bodies(Fd[s:s + 1], grid, p, t, lo=lo, mask=md, weight=wd, neighbours=neighbours, seeds=seeds)
                assert int(i1.item()) == 0 and np.array_equal(s1.cpu().numpy()[0], st_h[s]) and np.array_equal(m1.cpu().numpy()[0], sm_h[s]), what
            s2, m2, i2 = hip.bodies(Fd, grid, p, t[1:3], lo=lo, mask=md, weight=wd, neighbours=neighbours, seeds=seeds)
            assert int(i2.item()) == 0 and np.array_equal(s2.cpu().numpy(), st_h[:, 1:3]) and np.array_equal(m2.cpu().numpy(), sm_h[:, 1:3]), what
    # no seeds: zeros, and the seeded hits stay
    st0, sm0, _ = hip.bodies(Fd, grid, p, t, lo=lo, mask=md, weight=wd, neighbours=neighbours, hits_seeded=hs)
    assert (st0.cpu().numpy()[..., 4:] == 0).all() and (sm0.cpu().numpy()[..., 2] == 0).all() and np.array_equal(hs.cpu().numpy(), hs_r)
    print("bodies %s / %d / S = %d: %d patterns, worst |sum - fsum| / bound %.3f" % (grid, neighbours, S, len(pats), worst))


def test_patterns_are_what_they_claim():
    """The structural cases on the device itself: singletons, one body, the chain's end as its label, edge and corner contact."""
    from geobo_amd import hip
    for grid in ((16, 16, 16), (64, 64, 1)):
        n = grid[0] * grid[1] * grid[2]
        pats = dict(ref.patterns(grid, np.random.default_rng(3)))
        for nb in (6, 26):
            def run(name):
                F = torch.zeros((1, 3, n), dtype=torch.float64, device="cuda")
                F[0, 0] = _dev(np.where(pats[name].reshape(-1), 1.0, -1.0))
                lab = torch.empty((1, 1, n), dtype=torch.int32, device="cuda")
                st, _, info = hip.bodies(F, grid, 0, [0.0], neighbours=nb, labels=lab)
                assert int(info.item()) == 0
                return st.cpu().numpy()[0, 0], lab.cpu().numpy().reshape(-1), int(pats[name].sum())
            st, lab, m = run("checkerboard")
            assert st.tolist() == ([m, m, 1, 0, 0, 0] if nb == 6 else [m, 1, m, 0, 0, 0])
            for name in ("full", "serpentine", "spiral", "comb_last_plane", "comb_last_row", "u_shape"):
                st, lab, m = run(name)
                assert st.tolist() == [m, 1, m, 0, 0, 0] and set(lab.tolist()) <= {-1, 0}, (name, grid, nb)
            for name in ("corner_touch", "edge_touch"):
                if name == "corner_touch" and min(grid) == 1:
                    continue
                st, lab, m = run(name)
                assert st[1] == (2 if nb == 6 else 1) and st[0] == m, (name, grid, nb)
            assert run("empty")[0].tolist() == [0, 0, 0, -1, 0, 0]


# ---- 2. Inversion.geobodies on the 10 x 8 x 6 survey -----------------------------------------------------------------------------
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
    """k cutoffs half way between neighbours of the sorted values, none within 1e-9 scale of a value (section 17)."""
    v = np.sort(np.asarray(values).reshape(-1))
    idx = (np.linspace(0.1, 0.9, k) * (v.size - 1)).astype(int)
    cut = 0.5 * (v[idx] + v[idx + 1])
    assert np.abs(v[None, :] - cut[:, None]).min() > 1e-9 * float(scale)
    return cut


def _check(out, r, n, bound_abs, shape):
    """The returned tables against the reference dict r (cube units, offset 0); bound_abs: (n, C, 3) bounds on the three sums."""
    st = r["stats"]
    assert out["count"].dtype == np.int64 and np.array_equal(out["count"], st[..., 0])
    assert np.array_equal(out["n_bodies"], st[..., 1])
    for key, k_cnt, k_sum, member in (("largest", 2, 1, "in_largest"), ("seeded", 4, 2, "in_seeded")):
        part = out[key]
        assert np.array_equal(part["count"], st[..., k_cnt]), key
        assert np.array_equal(part["volume"], st[..., k_cnt] * VOXVOL), key
        err = np.abs(part["quantity"] - r["sums"][..., k_sum] * VOXVOL)
        assert np.all(err <= bound_abs[..., k_sum] * VOXVOL), key
        empty = st[..., k_cnt] == 0
        assert np.array_equal(np.isnan(part["grade"]), empty), key
        with np.errstate(all="ignore"):
            g = r["sums"][..., k_sum] / st[..., k_cnt]
        assert np.allclose(part["grade"][~empty], g[~empty], rtol=1e-9, atol=0), key
        prob = out["probability_" + key]
        assert prob.shape == (st.shape[1],) + tuple(shape)
        assert np.array_equal(prob.reshape(st.shape[1], -1), r[member].sum(0) / float(n)), key        # the hit frequencies, exactly
    assert np.array_equal(out["largest"]["label"], st[..., 3]) and np.array_equal(out["seeded"]["bodies"], st[..., 5])
    q = out["quantiles"]
    assert np.array_equal(q["n_bodies"], np.quantile(st[..., 1].astype(float), [0.1, 0.5, 0.9], axis=0))
    assert q["largest_volume"].shape == q["seeded_volume"].shape == (3, st.shape[1])


@pytest.mark.parametrize("neighbours", [6, 26])
def test_geobodies_matches_host_route(tiny, neighbours):
    inv, host = tiny["inv"], tiny["host"]
    p = 2
    cut = _midpoint_cutoffs(host[:, p], inv._cube_scale[p])[[3, 0, 4, 1, 2]]                    # (the caller's order is kept)
    drill = inv._drill_selection()
    assert drill.size > 0
    r = ref.bodies(host, GRID, p, cut, neighbours=neighbours, min_count=3, seeds=drill)
    out = inv.geobodies(cut, prop="drill", n=16, seed=SEED, neighbours=neighbours, min_voxels=3, seeds="drill", probability="both")
    assert np.array_equal(out["cutoffs"], cut)
    _check(out, r, 16, ref.sum_bound(N, r["abs"]), GRID)
    assert (r["stats"][..., 5] > 0).any()                                                        # (seeds that pass a cutoff are among the cases)
    print("geobodies / %d: bodies of 3 voxels or more between %d and %d" % (neighbours, r["stats"][..., 1].min(), r["stats"][..., 1].max()))
    assert np.array_equal(out["count"], inv.grade_tonnage(cut, prop="drill", n=16, seed=SEED)["count"])
    # the batching changes no bit, and realisations are addressed by their absolute index
    for batch in (2, 6):
        again = inv.geobodies(cut, prop=2, n=16, seed=SEED, batch=batch, neighbours=neighbours, min_voxels=3, seeds="drill", probability="both")
        for k in ("count", "n_bodies", "probability_largest", "probability_seeded"):
            assert np.array_equal(again[k], out[k]), (batch, k)
        for key in ("largest", "seeded"):
            for k in out[key]:
                assert np.array_equal(again[key][k], out[key][k], equal_nan=True), (batch, key, k)
    part = inv.geobodies(cut, prop=2, n=7, seed=SEED, start=5, batch=64, neighbours=neighbours, min_voxels=3, seeds=drill_xyz(drill))
    assert np.array_equal(part["n_bodies"], out["n_bodies"][5:12]) and np.array_equal(part["count"], out["count"][5:12])
    for key in ("largest", "seeded"):
        for k in out[key]:
            assert np.array_equal(part[key][k], out[key][k][5:12], equal_nan=True), (key, k)
    # a region and a bound on another property; a boolean seed cube
    region = np.zeros(GRID, dtype=bool)
    region[1:7, 1:9, :5] = True
    bound_d = float(np.median(host[:, 0]))
    assert np.abs(host[:, 0] - bound_d).min() > 1e-9 * float(inv._cube_scale[0])
    cube = np.zeros(GRID, dtype=bool)
    cube.reshape(-1)[drill] = True
    r2 = ref.bodies(host, GRID, p, cut, lo=[bound_d, -np.inf, -np.inf], mask=region.reshape(-1), neighbours=neighbours, seeds=drill)
    sub = inv.geobodies(cut, prop=2, n=16, seed=SEED, region=region, require={"density": bound_d}, neighbours=neighbours, seeds=cube,
                        probability="both")
    _check(sub, r2, 16, ref.sum_bound(N, r2["abs"]), GRID)
    assert np.array_equal(sub["count"], inv.grade_tonnage(cut, prop=2, n=16, seed=SEED, region=region, require={"density": bound_d})["count"])
    # an offset moves the cutoffs and the values together
    off = inv.geobodies(cut + 3.5, prop=2, n=16, seed=SEED, offset=3.5, neighbours=neighbours, min_voxels=3, seeds="drill")
    assert np.array_equal(off["n_bodies"], out["n_bodies"]) and np.array_equal(off["largest"]["count"], out["largest"]["count"])
    assert np.allclose(off["largest"]["quantity"], out["largest"]["quantity"] + 3.5 * out["largest"]["count"] * VOXVOL, rtol=1e-12, atol=0)
    assert "probability_largest" not in off and "probability_seeded" not in off


def drill_xyz(flat):
    """Flat voxel indices of the 10 x 8 x 6 survey -> (K, 3) rows (ix, iy, iz)."""
    flat = np.asarray(flat)
    return np.stack([(flat // GRID[2]) % GRID[1], flat // (GRID[1] * GRID[2]), flat % GRID[2]], 1)


@pytest.mark.parametrize("neighbours", [6, 26])
def test_geobodies_block_support(tiny, neighbours):
    """Blocks of (bx, by, bz) = (3, 4, 4) voxels: 2 x 4 x 2 blocks of at most 48 voxels.  The device's block mean and the reference's
    (math.fsum / count) each lie within (n_B - 1) u sum_B |x| / n_B of the exact mean, the sum over the 16 blocks adds (16 - 1) u
    sum |w m|: in all (47 + 15) u sum |x| over the voxels of the member blocks, asked for with the factor 2 of the other tests."""
    from geobo_amd import geobodies as G
    inv, host = tiny["inv"], tiny["host"]
    p = 1
    box = (4, 3, 4)                                            # (by, bx, bz)
    shape = (2, 4, 2)
    means, absb, count = gt.box_means(host, GRID, box)
    assert count.size == 16
    cut = _midpoint_cutoffs(means[:, p], inv._cube_scale[p])
    bseeds = G.seeds_to_blocks(inv._drill_selection(), GRID, box)
    r = ref.bodies(means, shape, p, cut, weight=count, neighbours=neighbours, min_count=49, seeds=bseeds)
    out = inv.geobodies(cut, prop="magsus", n=16, seed=SEED, block=(3, 4, 4), neighbours=neighbours, min_voxels=49, seeds="drill",
                        probability="both")
    members = np.stack([r["labels"] >= 0, r["in_largest"], r["in_seeded"]], -1).astype(np.float64)        # (n, C, blocks, 3)
    abs_vox = np.einsum("scbk,sb->sck", members, absb[:, p])
    _check(out, r, 16, 2.0 * (47 + 15) * ref.U * abs_vox, shape)
    assert np.array_equal(out["count"], inv.grade_tonnage(cut, prop="magsus", n=16, seed=SEED, block=(3, 4, 4))["count"])
    region = np.ones(shape, dtype=bool)
    region[:, 1] = False                                       # cuts the block grid in two along x
    r2 = ref.bodies(means, shape, p, cut, weight=count, mask=region.reshape(-1), neighbours=neighbours, seeds=bseeds)
    sub = inv.geobodies(cut, prop=1, n=16, seed=SEED, block=(3, 4, 4), region=region, neighbours=neighbours, seeds="drill", batch=6, start=0)
    assert np.array_equal(sub["n_bodies"], r2["stats"][..., 1]) and np.array_equal(sub["seeded"]["count"], r2["stats"][..., 4])
    assert np.array_equal(sub["largest"]["label"], r2["stats"][..., 3])


def test_limits(tiny):
    inv = tiny["inv"]
    out = inv.geobodies([np.inf, -np.inf], prop="density", n=4, seed=SEED, start=3, seeds="drill", probability="both", neighbours=26)
    assert (out["n_bodies"][:, 1] == 1).all() and (out["count"][:, 1] == N).all() and (out["largest"]["count"][:, 1] == N).all()
    assert (out["largest"]["label"][:, 1] == 0).all() and (out["seeded"]["count"][:, 1] == N).all() and (out["seeded"]["bodies"][:, 1] == 1).all()
    assert (out["probability_largest"][1] == 1.0).all() and (out["probability_seeded"][1] == 1.0).all()
    assert np.isfinite(out["largest"]["grade"][:, 1]).all()
    assert (out["n_bodies"][:, 0] == 0).all() and (out["count"][:, 0] == 0).all() and (out["largest"]["label"][:, 0] == -1).all()
    for key in ("largest", "seeded"):
        assert np.isnan(out[key]["grade"][:, 0]).all() and (out[key]["volume"][:, 0] == 0).all() and (out[key]["quantity"][:, 0] == 0).all()
    assert (out["probability_largest"][0] == 0.0).all() and (out["probability_seeded"][0] == 0.0).all()


@pytest.mark.parametrize("box", [None, (4, 3, 4)])
def test_launch_cuts_change_no_bit(tiny, box):
    """The engine cuts (samples, cutoffs) into launches to bound the workspace: every table, label and hit as in one launch."""
    from geobo_amd import geobodies as G
    eng = tiny["inv"].engine
    S, Cn = 5, 5
    F = torch.as_tensor(np.random.default_rng(9).standard_normal((S, 3, N)), device=eng.device)
    n = N if box is None else 16
    t = np.array([-np.inf, -0.6, 0.0, 0.5, 1.0]) if box is None else np.array([-np.inf, -0.1, 0.0, 0.05, 0.2])
    seeds = np.array([0, 7, n - 1], dtype=np.int32)

    def run(ws_bytes):
        hl = torch.zeros((Cn, n), dtype=torch.int32, device=eng.device)
        hs = torch.zeros((Cn, n), dtype=torch.int32, device=eng.device)
        lab = torch.full((S, Cn, n), -7, dtype=torch.int32, device=eng.device)
        st, sm = eng.body_statistics(F, 0, t, lo=[-np.inf, -1.0, -np.inf], box=box, neighbours=6, min_count=2, seeds=seeds, hits_largest=hl,
                                     hits_seeded=hs, labels=lab, ws_bytes=ws_bytes)
        return [x.cpu().numpy() for x in (st, sm, hl, hs, lab)]
    whole = run(G.WS_BYTES)
    assert whole[2].any() and whole[3].any() and (box is not None or (whole[0][..., 1] > 1).any())
    per = 16 * n + 48 + 64
    for bound, cuts in ((1, (1, 1)), (2 * per, (1, 2)), (5 * per, (1, 5)), (12 * per, (2, 5))):
        assert G.launch_cuts(S, Cn, n, bound) == cuts
        for a, b in zip(whole, run(bound)):
            assert np.array_equal(a, b), (bound, cuts)


# ---- 3. label_bodies ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbours", [6, 26])
def test_label_bodies_against_scipy(tiny, neighbours):
    from scipy import ndimage
    inv = tiny["inv"]
    structure = ndimage.generate_binary_structure(3, 1 if neighbours == 6 else 3)
    mean = (inv.mu_rec.reshape((3,) + GRID)[2] * inv._cube_scale[2]).astype(np.float64)
    real = tiny["host"][3, 2].reshape(GRID)
    for cube in (mean, real):
        for cutoff in np.quantile(cube, [0.3, 0.6, 0.85]):
            labels, sizes = inv.label_bodies(cube, cutoff, neighbours=neighbours)
            want, B = ndimage.label(cube >= cutoff, structure=structure)
            assert labels.dtype == np.int32 and np.array_equal(labels, want)
            assert np.array_equal(sizes, np.bincount(want.reshape(-1), minlength=B + 1)[1:])
    region = np.ones(GRID, dtype=bool)
    region[:, 4] = False
    cube = real.copy()
    cube[2, 3, 1] = np.nan
    labels, sizes = inv.label_bodies(cube, np.quantile(real, 0.4), neighbours=neighbours, region=region)
    with np.errstate(invalid="ignore"):
        want, B = ndimage.label((cube >= np.quantile(real, 0.4)) & region, structure=structure)
    assert np.array_equal(labels, want) and sizes.size == B and B >= 2
    assert inv.label_bodies(cube, np.inf)[1].size == 0 and inv.label_bodies(real, -np.inf)[1].tolist() == [N]


# ---- 4. a spectral step at 32^3 ----------------------------------------------------------------------------------------------------
def test_geobodies_at_32():
    from geobo_amd.inversion import Inversion
    f = load_golden("oracle32_exp.npz")
    d0 = np.zeros((32, 32, 32))                                 # (this survey has no drill data)
    s = settings_for(32, 32, 32, kernelfunc="exp", gp_coeff=list(PSD_W))
    inv = Inversion(settings=s, method="spectral")
    inv.create_cubegeometry()
    inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    n, M, grid = 4, 32 ** 3, (32, 32, 32)
    got = inv.sample_posterior(n, seed=SEED)
    host = np.stack([got[i].reshape(n, M) for i in range(2)] + [np.zeros((n, M))], 1)
    cut = _midpoint_cutoffs(host[:, 0], inv._cube_scale[0], k=5)[[3, 1, 2]]
    seeds = np.zeros(grid, dtype=bool)
    seeds[16, 16, :] = True                                     # a vertical hole through the middle
    r = ref.bodies(host, grid, 0, cut, neighbours=6, min_count=8, seeds=np.flatnonzero(seeds.reshape(-1)))
    out = inv.geobodies(cut, prop="density", n=n, seed=SEED, neighbours=6, min_voxels=8, seeds=seeds, probability="both")
    _check(out, r, n, ref.sum_bound(M, r["abs"]), grid)
    assert (r["stats"][..., 1] > 1).any()
    with pytest.raises(ValueError, match="drill"):
        inv.geobodies(cut, prop="drill", n=2)


# ---- 5. workflow -------------------------------------------------------------------------------------------------------------------
def test_yaml_key_writes_the_table_and_the_cubes(tmp_path):
    """YAML key geobodies on the reference's first example (25 x 16 x 16, non-cubic voxels), exponential kernel and the PSD weights."""
    import json
    import os

    import pandas as pd
    import yaml
    from conftest import GOLDEN
    from geobo_amd import dataio, geobodies, run_geobo
    f = load_golden("example1.npz")
    d = json.loads(str(f["settings_json"]))
    d.update(inpath=os.path.join(GOLDEN, "data", "synthetic") + "/", outpath=str(tmp_path) + "/", kernelfunc="exp", gp_coeff=list(PSD_W),
             sample_seed=3, geobodies=dict(property="density", cutoffs=[0.05, -0.05, 0.0], samples=6, neighbours=26, seeds="drill",
                                           probability="seeded"))
    y = tmp_path / "settings.yaml"
    y.write_text(yaml.safe_dump(d))
    out = run_geobo.run(str(y), bayesopt=False)
    got = out["geobodies"]
    inv = out["inversion"]
    again = inv.geobodies([0.05, -0.05, 0.0], prop="density", n=6, seed=3, neighbours=26, seeds="drill", probability="seeded")
    assert got["n_bodies"].shape == (6, 3) and np.array_equal(got["n_bodies"], again["n_bodies"])
    assert np.array_equal(got["seeded"]["quantity"], again["seeded"]["quantity"], equal_nan=True)
    assert np.array_equal(got["count"], inv.grade_tonnage([0.05, -0.05, 0.0], prop="density", n=6, seed=3)["count"])
    assert np.all(got["largest"]["count"] <= got["count"]) and np.all(got["seeded"]["count"] <= got["count"])
    tab = pd.read_csv(tmp_path / "geobodies.csv")
    assert list(tab.columns) == list(geobodies.CSV_COLUMNS) and np.array_equal(tab["CUTOFF"], [0.05, -0.05, 0.0])
    assert np.allclose(tab["BODIES_P50"], got["quantiles"]["n_bodies"][1], rtol=1e-12, atol=0)
    s = inv.settings
    assert got["probability_seeded"].shape == (3, s.yNcube, s.xNcube, s.zNcube) and "probability_largest" not in got
    for k in range(3):
        cube = dataio.read_vtkcube(str(tmp_path / ("cube_density_connected_%d.vtk" % k)))[0]
        assert np.array_equal(cube, got["probability_seeded"][k])


# ---- 6. error paths ----------------------------------------------------------------------------------------------------------------
def test_error_paths(tiny):
    from geobo_amd.inversion import Inversion
    inv = tiny["inv"]
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=settings_for(**TINY)).geobodies([0.0], prop="density")
    with pytest.raises(ValueError):
        inv.geobodies([0.0], prop="density", n=2, require={"density": 0.0})
    for bad in (np.ones((10, 8, 6), dtype=bool), np.zeros((4, 2), dtype=int), np.zeros(3, dtype=int), np.array([[10, 0, 0]]), "holes", 3.5):
        with pytest.raises(ValueError, match="seed"):
            inv.geobodies([0.0], prop="density", n=2, seeds=bad)
    for bad in (4, 18, 27, "6", None):
        with pytest.raises(ValueError, match="neighbours"):
            inv.geobodies([0.0], prop="density", n=2, neighbours=bad)
        with pytest.raises(ValueError, match="neighbours"):
            inv.label_bodies(np.zeros(GRID), 0.0, neighbours=bad)
    with pytest.raises(ValueError):
        inv.geobodies(np.arange(33.0), prop="density", n=2)
    with pytest.raises(ValueError, match="probability"):
        inv.geobodies([0.0], prop="density", n=2, probability="all")
    with pytest.raises(ValueError):
        inv.geobodies([0.0], prop="density", n=2, min_voxels=0)
    with pytest.raises(ValueError, match="region"):
        inv.geobodies([0.0], prop="density", n=2, region=np.ones((10, 8, 6), dtype=bool))
    with pytest.raises(ValueError):
        inv.geobodies([0.0], prop="density", n=2, block=(11, 3, 4))
    with pytest.raises(ValueError, match="shape"):
        inv.label_bodies(np.zeros((10, 8, 6)), 0.0)
    f = load_golden("tiny_exp_nodrill.npz")
    nod = Inversion(settings=settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W)))
    nod.create_cubegeometry()
    nod.gp_length = np.array([200.0, 204.0, 208.0])
    d0 = f["drilldata0"]
    nod.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    with pytest.raises(ValueError, match="drill"):
        nod.geobodies([0.0], prop="drill", n=2)
    with pytest.raises(ValueError, match="drill"):
        nod.geobodies([0.0], prop="density", n=2, require={"drill": 0.0})
    none = nod.geobodies([0.0], prop="density", n=2, seeds="drill")               # no drilled voxel: no seed
    assert (none["seeded"]["count"] == 0).all() and (none["seeded"]["bodies"] == 0).all()
