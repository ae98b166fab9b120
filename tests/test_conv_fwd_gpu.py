"""geobo_xz2d_fold_conv_fwd by value: the product-input inverse transform and the forward transform of every plane in one kernel, the
64 x 64 plane handed over on chip.  Two references on the same inputs: the pair of launches it replaces (geobo_xz2d_fold_inv_mul into a
dense buffer, rows 0 and n - 1 overwritten from the slab, geobo_xz2d_fold forward) and the same in torch float64 with
spectral.forward_matrix.  The fused kernel forms the same sums in at most a different order, so its deviation from the torch reference
may be at most twice the pair's own.  64 x 64 planes are the only shape the kernel exists for: small means few rows and few planes.
The last case has more planes (33 x 64 = 2112) than the launch has workgroups (2048): the plane loop and the reuse of the LDS plane
run a second time in some workgroups."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 64
P = 2 * N
TAIL = 4096


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


@pytest.fixture(scope="module")
def mats(hip):
    from geobo_amd.spectral import folded_matrices, forward_matrix
    G = torch.from_numpy(forward_matrix(N)).cuda()                               # (P, N)
    F = hip.to_dev(np.stack(folded_matrices(N), axis=2))
    return G, F


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).cuda()


def _inputs(R, ppr):
    lam, lh = _rand((ppr, P, P), 11 + R), _rand((R, P, P), 12 + ppr)
    slab = 8.0 * _rand((R, 2, ppr, N), 13 + R + ppr)          # another magnitude than the table's rows: a miss cannot hide
    return lam, lh, slab


def _fused(hip, F, lam, lh, slab, R, ppr):
    out = torch.full((R * ppr * P * P + TAIL,), float("nan"), dtype=torch.float64, device="cuda")
    hip.xz2d_fold_conv_fwd(N, R, ppr, lam, P * P, lh, P * P, slab, 0 if slab is None else 2 * ppr * N, F, F, out, ppr * P * P, P * P)
    torch.cuda.synchronize()
    body, tail = out[:R * ppr * P * P], out[R * ppr * P * P:]
    assert not bool(torch.isnan(body).any())                  # every element of every plane is written ...
    assert bool(torch.isnan(tail).all())                      # ... and nothing behind the last plane
    return body.view(R, ppr, P, P)


def _pair(hip, F, lam, lh, slab, R, ppr):
    Z = torch.empty((R, ppr, N, N), dtype=torch.float64, device="cuda")
    hip.xz2d_fold_inv_mul(N, R, ppr, lam, P * P, lh, P * P, F, F, Z, ppr * N * N, N * N, N)
    Z[:, :, 0, :] = 0.0 if slab is None else slab[:, 0]
    Z[:, :, N - 1, :] = 0.0 if slab is None else slab[:, 1]
    out = torch.empty((R, ppr, P, P), dtype=torch.float64, device="cuda")
    hip.xz2d_fold(False, N, R, ppr, Z, ppr * N * N, N * N, F, F, out, ppr * P * P, P * P)
    return out


def _torch_ref(G, lam, lh, slab):
    W = lam[None, :, :, :] * lh[:, None, :, :]                # (R, ppr, P, P)
    X = G.t() @ W @ G                                         # inverse: G^T S G
    X[:, :, 0, :] = 0.0 if slab is None else slab[:, 0]
    X[:, :, N - 1, :] = 0.0 if slab is None else slab[:, 1]
    return G @ X @ G.t()


@pytest.mark.parametrize("R,ppr,with_slab", [(1, 5, True), (1, 5, False), (3, 5, True), (3, 5, False), (33, 64, True)])
def test_fused_against_the_pair_and_torch(hip, mats, R, ppr, with_slab):
    G, F = mats
    lam, lh, slab = _inputs(R, ppr)
    if not with_slab:
        slab = None
    got = _fused(hip, F, lam, lh, slab, R, ppr)
    pair = _pair(hip, F, lam, lh, slab, R, ppr)
    ref = _torch_ref(G, lam, lh, slab)
    top = ref.abs().max().item()
    dev_fused, dev_pair = (got - ref).abs().max().item() / top, (pair - ref).abs().max().item() / top
    print("conv_fwd R = %d, ppr = %d, slab %s: fused vs torch %.3e, pair vs torch %.3e, fused vs pair %.3e"
          % (R, ppr, with_slab, dev_fused, dev_pair, (got - pair).abs().max().item() / top))
    assert 0.0 < dev_pair <= 1e-12                            # (the yardstick itself is sound: four contractions of <= 128 fp64 terms)
    assert dev_fused <= 2.0 * dev_pair


def test_boundary_rows_are_the_slab(hip, mats):
    """The transform is linear in the plane: (spectrum with a slab) - (spectrum with none) is the transform of a plane that holds the
    slab's two rows and nothing else -- not of what the stencil table would put there."""
    G, F = mats
    R, ppr = 3, 5
    lam, lh, slab = _inputs(R, ppr)
    with_, without = _fused(hip, F, lam, lh, slab, R, ppr), _fused(hip, F, lam, lh, None, R, ppr)
    E = torch.zeros((R, ppr, N, N), dtype=torch.float64, device="cuda")
    E[:, :, 0, :], E[:, :, N - 1, :] = slab[:, 0], slab[:, 1]
    ref = G @ E @ G.t()
    err = ((with_ - without) - ref).abs().max().item() / ref.abs().max().item()
    print("conv_fwd boundary rows: %.3e" % err)
    assert err <= 1e-12
    # ... and with no slab the two rows are zero, whatever the table gives: the plain inverse of the same inputs has them non-zero
    Z = torch.empty((R, ppr, N, N), dtype=torch.float64, device="cuda")
    hip.xz2d_fold_inv_mul(N, R, ppr, lam, P * P, lh, P * P, F, F, Z, ppr * N * N, N * N, N)
    assert Z[:, :, 0, :].abs().max().item() > 1.0
    Z[:, :, 0, :] = 0.0
    Z[:, :, N - 1, :] = 0.0
    ref0 = G @ Z @ G.t()
    assert (without - ref0).abs().max().item() <= 1e-12 * ref0.abs().max().item()
