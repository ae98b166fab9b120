"""reduce_ss and product_two_term against the same quantities built from one-term storing products, at the smallest grid that reaches
each form of the y-stage join (SpectralProduct._join): one-pass pairs with and without the shared cross block, the odd last block of
a "y2t" grid, the accumulating and the three-transform forms, separate spectra, and the stored reduction with and without a join.
rows_per_batch = 4 with 9 rows of which the last 4 are two-term: a whole and a partial one-term batch, a whole two-term batch.
GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
ROWS, M_FIRST, BATCH = 9, 5, 4
TOL = 1e-11       # of the reference's maximum per block: the suite's figure for three- against four-product and transposed against fused


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=F64) * 2 - 1).cuda()


@pytest.mark.parametrize("nblocks", [2, 3])
@pytest.mark.parametrize("grid", [(64, 16, 64), (64, 32, 64), (64, 80, 64), (16, 16, 16), (32, 32, 32), (16, 80, 16)])
def test_two_term_rows_match_the_sum_of_one_term_products(grid, nblocks):
    from geobo_amd import hip
    from geobo_amd.spectral import SpectralProduct
    hip.require_gpu()
    nx, ny, nz = grid
    N = nx * ny * nz
    sp = SpectralProduct(nx, ny, nz, "cuda", rows_per_batch=BATCH)
    assert sp.R == BATCH and sp.dense_y
    ngen = ny * sp.Px * sp.Pz
    tg = [_rand((ngen,), 10 + j) for j in range(nblocks)]
    tm = [tg[1].clone()] + [_rand((ngen,), 20 + j) for j in range(1, nblocks)]         # K_10 = K_01: the three-product form applies
    Zg, Zm = _rand((ROWS, N), 1), _rand((ROWS - M_FIRST, N), 2)
    # reference: V_j = Zg K_0j (+ Zm K_1j on the two-term rows) from one-term storing products, added and squared in torch
    V = [torch.empty((ROWS, N), dtype=F64, device="cuda") for _ in range(nblocks)]
    W = [torch.empty((ROWS - M_FIRST, N), dtype=F64, device="cuda") for _ in range(nblocks)]
    sp.product(Zg, ROWS, tg, V)
    sp.product(Zm, ROWS - M_FIRST, tm, W)
    for j in range(nblocks):
        V[j][M_FIRST:] += W[j]
    y2s = sp.y2s_tables(tg, tm)
    assert (y2s is not None) == sp.forms.y2s
    ss = [torch.zeros((sp.ss_slots(), ny, nx * nz), dtype=F64, device="cuda") for _ in range(nblocks)]
    sp.reduce_ss(Zg, ROWS, tg, Zm, M_FIRST, tm, ss, y2s=y2s)
    err_ss = [float(((ss[j].sum(0).reshape(-1) - (V[j] ** 2).sum(0)).abs().max() / (V[j] ** 2).sum(0).abs().max())) for j in range(nblocks)]
    err_tt = None
    if sp.has_two_term_product(nblocks):
        out = [torch.full((BATCH, N), float("nan"), dtype=F64, device="cuda") for _ in range(nblocks)]
        sp.product_two_term(Zg[M_FIRST:], Zm, ROWS - M_FIRST, tg, tm, out, y2s=y2s)
        err_tt = [float((out[j] - V[j][M_FIRST:]).abs().max() / V[j][M_FIRST:].abs().max()) for j in range(nblocks)]
    if y2s is not None:
        assert float(sp.sym_residual) == 0.0
    print("two-term %dx%dx%d, %d blocks (%s, ss %s): reduce_ss %s, product_two_term %s"
          % (nx, ny, nz, nblocks, sp.forms.y_two_term, sp.forms.ss, ["%.2e" % e for e in err_ss], err_tt and ["%.2e" % e for e in err_tt]))
    assert max(err_ss) <= TOL, err_ss
    assert err_tt is None or max(err_tt) <= TOL, err_tt
