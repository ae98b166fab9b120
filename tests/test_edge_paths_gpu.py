"""The boundary-slab paths of the lattice Gram (LatticeGram.edge_rows) and of L^-1 A (edge_apply_transpose, both slab layouts) against
the dense slab operator E[(jy, jx), (ix, iz)] = kappa_jy(ix - jx, iz), built in torch from the same random, non-even kappa.
Grids: 16 x 16 x 16 (nz = 16: the spare-slot case of edge_eigen_t) and 64 x 16 x 64 (the extents of the flagship grid's planes).
Row counts: 1, 5 and 1030 (crosses EDGE_ROWS = 1024, ragged against 128)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRIDS = [(16, 16, 16), (64, 16, 64)]
ROWS = [1, 5, 1030]
BOUND = 1e-12            # of max |result|


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64)


_cache = {}


def _slab(nx, ny, nz):
    """(gram, E, its two spectra): computed once per grid, shared by every case, never written to."""
    key = (nx, ny, nz)
    if key not in _cache:
        from geobo_amd import hip
        from geobo_amd.lattice_gram import LatticeGram
        from geobo_amd.spectral import SpectralProduct
        hip.require_gpu()
        gram = LatticeGram(SpectralProduct(nx, ny, nz, "cuda"), "cuda")
        kap = _rand((ny, 2 * nx - 1, nz), 71)                                            # kappa_jy(d, iz), d = -(nx-1) .. nx-1
        idx = (torch.arange(nx)[None, :] - torch.arange(nx)[:, None] + nx - 1).cuda()    # [jx][ix] -> d index
        E = kap[:, idx, :].reshape(ny * nx, nx * nz)                                     # row (jy, jx), column (ix, iz)
        Epad = torch.zeros((ny * nx + 256, nx * nz + 16), dtype=torch.float64, device="cuda")
        Epad[:ny * nx, :nx * nz] = E
        _cache[key] = (gram, E, gram.edge_eigen(Epad[:, :nx * nz]), gram.edge_eigen_t(Epad[:, :nx * nz]))
    return _cache[key]


@pytest.mark.parametrize("nrows", ROWS)
@pytest.mark.parametrize("grid", GRIDS)
def test_edge_rows_against_the_dense_slab(grid, nrows):
    nx, ny, nz = grid
    gram, E, V, _ = _slab(nx, ny, nz)
    pl = nx * nz
    for slack in (True, False):
        Xb = _rand((nrows + (1 if slack else 0), 3 * pl), 72 + nrows)
        X = Xb[:nrows, pl:] if slack else Xb[:, 2 * pl:]                   # without slack: the slab is the last thing in the buffer
        out = _rand((nrows + 2, ny * nx + 6), 73)                          # pre-filled: the product is ADDED, the padding stays
        before = out.clone()
        ref = out[:nrows, :ny * nx] + X[:nrows, :pl] @ E.t()
        gram.edge_rows(X, nrows, V, out)
        err = (out[:nrows, :ny * nx] - ref).abs().max().item() / ref.abs().max().item()
        print("edge_rows %s, %d rows, slack %s: %.2e" % (grid, nrows, slack, err))
        assert err <= BOUND
        out[:nrows, :ny * nx] = before[:nrows, :ny * nx]
        assert bool((_bits(out) == _bits(before)).all())


@pytest.mark.parametrize("zx", [False, True])
@pytest.mark.parametrize("nrows", ROWS)
@pytest.mark.parametrize("grid", GRIDS)
def test_edge_apply_transpose_against_the_dense_slab(grid, nrows, zx):
    nx, ny, nz = grid
    gram, E, _, Vt = _slab(nx, ny, nz)
    pl, Ms = nx * nz, nx * ny
    for slack in (True, False):
        Lb = _rand((nrows + (1 if slack else 0), 2 * Ms), 81 + nrows)
        L = Lb[:nrows, :Ms] if slack else Lb[:, Ms:]                       # without slack: the last row ends the buffer
        ref = L[:nrows] @ E                                                # [row][(ix, iz)]
        if zx:
            ref = ref.view(nrows, nx, nz).transpose(1, 2).reshape(nrows, pl)
        buf = _rand((nrows + 2, 3 * pl + 10), 82)                          # pre-filled: the slab is OVERWRITTEN, everything else stays
        before = buf.clone()
        out = buf[:, pl + 2:2 * pl + 2]
        gram.edge_apply_transpose(L, nrows, Vt, out, zx=zx)
        err = (out[:nrows] - ref).abs().max().item() / ref.abs().max().item()
        print("edge_apply_transpose %s, %d rows, zx %s, slack %s: %.2e" % (grid, nrows, zx, slack, err))
        assert err <= BOUND
        out[:nrows] = before[:nrows, pl + 2:2 * pl + 2]
        assert bool((_bits(buf) == _bits(before)).all())
