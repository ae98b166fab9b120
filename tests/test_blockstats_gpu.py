"""Block-support posterior statistics on the device: geobo_block_cov against torch, block_statistics against
the oracle's dense posterior covariance (all six entries of the 3 x 3 matrix), consistency with cubing() and hole_statistics() at
32^3 and 64^3, the two tile sources against each other, and the state the call leaves behind.

The entries are raw: the reference's matern32 prior is not positive semidefinite, so nothing here asserts PSD or |corr| <= 1."""
import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

from conftest import load_golden, normwise, settings_for
from oracle import geobo_oracle as O

pytestmark = pytest.mark.gpu

TINY = dict(nx=10, ny=8, nz=6)
CUBE16 = dict(nx=16, ny=16, nz=16)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


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


def _oracle(inv):
    """oracle.posterior_dense on the engine's own operators."""
    s, eng = inv.settings, inv.engine
    A_g, A_m = (_host_operator(eng, A) for A in inv._operators())
    P3 = O.grid_points((s.xNcube, s.yNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize))
    return O.posterior_dense(P3, A_g, A_m, inv._sel, inv.Fs3, np.array(inv.gp_length, dtype=float), O.weight_matrix(inv.coeffm),
                             s.kernelfunc, inv.gp_sigma, gp_amp=inv.gp_amp, return_cov=True)


def _partition(grid, box):
    """Block of every voxel and voxels per block, brute force: grid (ny, nx, nz), box (by, bx, bz)."""
    nb = [-(-n // b) for n, b in zip(grid, box)]
    iy, ix, iz = np.meshgrid(*(np.arange(n) for n in grid), indexing="ij")
    index = (((iy // box[0]) * nb[1] + ix // box[1]) * nb[2] + iz // box[2]).reshape(-1)
    return index, np.bincount(index), tuple(nb)


# ---- 1. the kernel against torch -------------------------------------------------------------------------------------------------
def _want6(V, N, index, nblocks):
    S = [torch.zeros((V[0].shape[0], nblocks), dtype=torch.float64, device="cuda").index_add_(1, index, v[:, :N]) for v in V]
    return torch.stack([torch.einsum("rb,rb->b", S[a], S[b]) for a, b in PAIRS], dim=1)


@pytest.mark.parametrize("R", [1, 37, 130])
@pytest.mark.parametrize("grid,boxes", [((5, 6, 7), [(1, 1, 1), (2, 3, 4), (3, 1, 2), (1, 1, 7), (5, 6, 7)]),     # odd nz: unaligned segments
                                        ((4, 4, 64), [(2, 2, 4), (1, 1, 64), (4, 4, 16)])])                      # aligned 16-byte loads
def test_block_cov_matches_torch(grid, boxes, R):
    from geobo_amd import hip
    rng = np.random.default_rng(R + grid[2])
    N = grid[0] * grid[1] * grid[2]
    ldv = N + 9

    def tile():
        t = torch.as_tensor(rng.standard_normal((R, ldv)), device="cuda")
        t[:, N:] = float("nan")                                # a NaN in the result: the padding columns were read
        return t
    V = [tile() for _ in range(3)]
    for box in boxes:
        index, count, _ = _partition(grid, box)
        nblocks = count.size
        want = _want6(V, N, torch.as_tensor(index, device="cuda"), nblocks)
        C6 = torch.full((nblocks, 6), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.full((hip.block_cov_ws_doubles(R, grid, box),), float("nan"), dtype=torch.float64, device="cuda")
        hip.block_cov(V, R, grid, box, C6, ws=ws)
        err = float((C6 - want).abs().max() / want.abs().max())
        print("block_cov grid %s box %s R = %d: %.2e" % (grid, box, R, err))
        assert err <= 1e-13, (grid, box, R)
        again = torch.full_like(C6, float("nan"))
        hip.block_cov(V, R, grid, box, again)                  # (its own workspace, whatever that holds)
        assert torch.equal(C6, again)
        C0 = torch.as_tensor(rng.standard_normal((nblocks, 6)), device="cuda")
        acc = C0.clone()
        hip.block_cov(V, R, grid, box, acc, accumulate=True, ws=ws)
        assert float((acc - (C0 + want)).abs().max() / (C0 + want).abs().max()) <= 1e-13
        same = torch.full_like(C6, float("nan"))
        hip.block_cov([V[1], V[1], V[1]], R, grid, box, same, ws=ws)
        assert torch.equal(same, same[:, :1].expand(-1, 6)) and torch.equal(same[:, 0], C6[:, 3])
    # no rows: zeroes, or leaves what is there
    C6 = torch.full((count.size, 6), float("nan"), dtype=torch.float64, device="cuda")
    hip.block_cov(V, 0, grid, boxes[-1], C6)
    assert float(C6.abs().max()) == 0.0
    hip.block_cov(V, 0, grid, boxes[-1], acc, accumulate=True)
    assert float((acc - (C0 + want)).abs().max() / (C0 + want).abs().max()) <= 1e-13


# ---- 2. against the oracle's dense covariance --------------------------------------------------------------------------------
_ORACLE = {}        # one dense posterior per golden case, shared by the routes that run on it


@pytest.mark.parametrize("name,dims,method,rows,blocks", [
    ("tiny_exp", TINY, "auto", False, [(1, 1, 1), (2, 2, 2), (4, 3, 4), (10, 8, 6)]),
    ("tiny_matern32", TINY, "auto", True, [(1, 1, 1), (2, 2, 2), (4, 3, 4), (10, 8, 6)]),
    ("cube16_matern32", CUBE16, "spectral", False, [(4, 4, 4), (1, 1, 16), (16, 16, 16)]),
    ("cube16_matern32", CUBE16, "dense", False, [(4, 4, 4), (1, 1, 16), (16, 16, 16)])])
def test_block_statistics_match_oracle(name, dims, method, rows, blocks, monkeypatch):
    if rows:
        monkeypatch.setenv("GEOBO_ROWS", "1")
    f = load_golden(name + ".npz")
    s = settings_for(**dims, kernelfunc=name.split("_")[1])
    inv = _inv(s, method=method)
    inv.gp_length = f["gp_length_in"].copy()
    _cubing(inv, f)
    N = inv.engine.N
    grid = (s.yNcube, s.xNcube, s.zNcube)
    if name not in _ORACLE:
        r = _oracle(inv)
        _ORACLE[name] = (r["cov"], r["mu"])
    Sigma, mu = _ORACLE[name]
    scale = [float(v) for v in inv._cube_scale]
    for bx, by, bz in blocks:
        index, count, nb = _partition(grid, (by, bx, bz))
        # the diagonal of W^T S W for the block-mean weights W (N x nblocks, 1 / n_B on the voxels of B)
        Wt = csr_matrix((1.0 / count[index], (index, np.arange(N))), shape=(count.size, N))
        wsw = lambda S: np.bincount(index, weights=(Wt @ S)[index, np.arange(N)]) / count
        wmean = lambda v: np.bincount(index, weights=v) / count
        got = inv.block_statistics((bx, by, bz))
        print("%s [%s, %s] block %s" % (name, inv.engine.step_route, inv.engine.set_source, (bx, by, bz)))
        assert got["cov"].shape == nb + (3, 3) and got["mean"].shape == (3,) + nb and np.array_equal(got["count"].reshape(-1), count)
        for a, b in PAIRS:
            want = wsw(Sigma[a * N:(a + 1) * N, b * N:(b + 1) * N]) * scale[a] * scale[b]
            err = normwise(got["cov"][..., a, b].reshape(-1), want)
            print("    cov%d%d %.2e   (corr range %.3f .. %.3f)" % (a, b, err, got["corr"][..., a, b].min(), got["corr"][..., a, b].max()))
            assert err <= 1e-10, (name, (bx, by, bz), a, b)
            assert np.array_equal(got["cov"][..., a, b], got["cov"][..., b, a])
        for a in range(3):
            assert normwise(got["mean"][a].reshape(-1), wmean(mu[a * N:(a + 1) * N]) * scale[a]) <= 1e-10
        with np.errstate(all="ignore"):
            var = np.einsum("...aa->...a", got["cov"])
            assert np.array_equal(np.isnan(got["std"]), np.moveaxis(var < 0, -1, 0))
            ok = var >= 0
            assert np.allclose(np.moveaxis(got["std"], 0, -1)[ok], np.sqrt(var[ok]), rtol=1e-14, atol=0)
            c01 = got["cov"][..., 0, 1] / np.sqrt(var[..., 0] * var[..., 1])
            assert np.allclose(got["corr"][..., 0, 1], c01, rtol=1e-12, atol=0, equal_nan=True)
    # centres: the mean of the voxel centres of a block
    index, count, nb = _partition(grid, (blocks[1][1], blocks[1][0], blocks[1][2]))
    got = inv.block_statistics(blocks[1])
    for i in range(3):
        assert np.allclose(got["centre"][..., i].reshape(-1), np.bincount(index, weights=inv.voxelpos[i]) / count, rtol=1e-14, atol=1e-9)


# ---- 3. consistency at size ------------------------------------------------------------------------------------------------------
def _consistency(inv, cubes):
    """Blocks of one voxel against cubing()'s variance cubes, whole z-columns against hole_statistics(), box means of the mean cubes."""
    s = inv.settings
    ny, nx, nz = s.yNcube, s.xNcube, s.zNcube
    scale = [float(v) for v in inv._cube_scale]
    one = inv.block_statistics((1, 1, 1))
    assert one["cov"].shape == (ny, nx, nz, 3, 3) and (one["count"] == 1).all()
    for a in range(3):
        prior_var = float(inv.gp_amp) * scale[a] ** 2
        err = float(np.abs(one["cov"][..., a, a] - cubes[3 + a]).max()) / prior_var
        print("%d^3 [%s, %s] voxel variance %d: %.2e of the prior variance" % (nx, inv.engine.step_route, inv.engine.set_source, a, err))
        assert err <= 1e-12
        assert normwise(one["mean"][a], cubes[a]) <= 1e-14
    holes = inv.hole_statistics()
    col = inv.block_statistics((1, 1, nz))
    assert col["cov"].shape == (ny, nx, 1, 3, 3) and (col["count"] == nz).all()
    got = col["cov"][1:-1, 1:-1, 0, 2, 2] * nz ** 2
    want = holes["path_std"][1:-1, 1:-1] ** 2
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    print("%d^3 column variance of the drill property vs hole_statistics: %.2e" % (nx, err))
    assert err <= 1e-12
    for a in range(3):
        assert normwise(col["mean"][a][:, :, 0], np.ascontiguousarray(cubes[a]).mean(axis=2)) <= 1e-14
    return holes


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
    part = inv.block_statistics((5, 3, 7))                     # partial blocks on every axis
    index, count, nb = _partition((32, 32, 32), (3, 5, 7))
    assert part["count"].shape == nb and np.array_equal(part["count"].reshape(-1), count)
    for a in range(3):
        assert normwise(part["mean"][a].reshape(-1), np.bincount(index, weights=np.asarray(cubes[a]).reshape(-1)) / count) <= 1e-14


def test_consistency_and_sources_agree_at_64():
    from geobo_amd.config_loader import Settings
    from geobo_amd.engine import create_cov_lengths
    f = load_golden("oracle64_sample_matern32.npz")
    n = 64
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc="matern32"))
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    cubes = inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    _consistency(inv, cubes)
    assert inv.engine.set_source == "spectral"
    lengths = [float(v) for v in create_cov_lengths(np.array(inv.gp_length, dtype=float))]
    res = {}
    for src in ("spectral", "generic"):
        cov, count = inv.engine.block_covariance((4, 4, 4), s.kernelfunc, lengths, inv.coeffm, inv.gp_amp, source=src)
        assert inv.engine.set_source == src and tuple(cov.shape) == (16 ** 3, 3, 3) and int(count.min()) == int(count.max()) == 64
        res[src] = cov.cpu().numpy()
    errs = [normwise(res["spectral"][:, a, b], res["generic"][:, a, b]) for a, b in PAIRS]
    print("64^3 spectral vs generic source, block (4, 4, 4): %s" % errs)
    assert max(errs) <= 1e-12


# ---- 4. state --------------------------------------------------------------------------------------------------------------------
def test_block_statistics_leave_the_engine_as_they_found_it():
    f = load_golden("tiny_matern32.npz")
    s = settings_for(**TINY, kernelfunc="matern32")
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    _cubing(inv, f)
    before = inv.hole_statistics()
    Linv, last = inv.engine.last["Linv"], inv.engine.last
    mu, var = inv.mu_rec.copy(), np.diag(inv.cov_rec).copy()
    first = inv.block_statistics((2, 3, 4))
    assert inv.engine.last is last and inv.engine.last["Linv"] is Linv
    after = inv.hole_statistics()
    assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before)
    assert np.array_equal(mu, inv.mu_rec) and np.array_equal(var, np.diag(inv.cov_rec))
    again = inv.block_statistics((2, 3, 4))
    assert all(np.array_equal(first[k], again[k], equal_nan=True) for k in first)
