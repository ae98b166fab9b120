"""The y stage on rows read as windows of a pool of distinct plane spectra (geobo_spectral_y_lattice) and the pooled feed of the A K
product built on it (SpectralProduct.plane_pool): the pooled route changes ADDRESSES only -- never operands or summation order -- so
every comparison here is bit for bit (torch.equal) against the same kernel on the materialised rows.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=F64) * 2 - 1).cuda()


def _windows(ny, R, seed):
    """Window starts (planes) into a pool of 3 ny planes: overlapping (neighbours shifted by one plane), repeated, and the two
    extreme ones whose never-read first / last plane lies one plane outside the pool."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 * ny + 1, size=R)
    if R >= 2:
        w[1] = w[0] + 1 if w[0] < 2 * ny else w[0] - 1        # overlap: the same window shifted by one plane
    if R >= 7:
        w[2], w[3], w[4] = w[0], -1, 2 * ny + 1               # a repeat; first plane in front of the pool; last plane behind it
    return w


def _case(hip, ny, C, S, R, nprop, y0, y1, perm, seed):
    P = 3 * ny
    # one NaN guard plane on either side of the pool, NaN in the padding columns: nothing of either may reach a result
    buf = torch.full((P + 2, S), float("nan"), dtype=F64, device="cuda")
    buf[1:P + 1, :C] = _rand((P, C), seed)
    pool = buf.reshape(-1)[S:]
    edge_row = 2 * S + 16
    edge = torch.full((R, edge_row), float("nan"), dtype=F64, device="cuda")
    e = _rand((R, 2, C), seed + 1)
    edge[:, :C], edge[:, S:S + C] = e[:, 0], e[:, 1]
    w = _windows(ny, R, seed + 2)
    row_off = torch.from_numpy(w.astype(np.int64) * S).cuda()
    order = torch.from_numpy(np.random.default_rng(seed + 3).permutation(R).astype(np.int32)).cuda() if perm else None
    tabs = [_rand((ny, C), seed + 4 + j).reshape(-1) for j in range(nprop)]
    # the materialised gather of the same windows
    rows = torch.full((R, ny, S), float("nan"), dtype=F64, device="cuda")
    for r in range(R):
        rows[r, 1:ny - 1] = buf[1 + w[r] + 1:1 + w[r] + ny - 1]
        rows[r, 0], rows[r, ny - 1] = edge[r, :S], edge[r, S:2 * S]
    ref = [torch.full((R, y1 - y0, S), 7.0, dtype=F64, device="cuda") for _ in range(nprop)]
    hip.spectral_y(ny, C, R, rows.reshape(-1), tabs, [o.reshape(-1) for o in ref], y0, y1, plane=S)
    out = [torch.full((R, y1 - y0, S), 7.0, dtype=F64, device="cuda") for _ in range(nprop)]
    hip.spectral_y_lattice(ny, C, R, pool, row_off, edge.reshape(-1), edge_row, order, tabs, [o.reshape(-1) for o in out], y0, y1, plane=S)
    torch.cuda.synchronize()
    for j in range(nprop):
        assert not bool(torch.isnan(ref[j]).any())
        assert torch.equal(out[j], ref[j]), (ny, C, S, R, nprop, y0, y1, perm, j)      # padding columns (7.0) included: not written


@pytest.mark.parametrize("nprop", [1, 2])
@pytest.mark.parametrize("C,S", [(64, 64), (64, 80), (128, 128), (128, 144)])
@pytest.mark.parametrize("ny", [32, 48, 64])
def test_windowed_rows_match_gathered_rows(hip, ny, C, S, nprop):
    # R = 1, 2, 7; the full height and a slab; identity order and a random permutation
    seed = 1000 * ny + C + S + nprop
    for R in (1, 2, 7):
        for y0, y1 in ((0, ny), (16, ny - 8)):
            for perm in (False, True):
                _case(hip, ny, C, S, R, nprop, y0, y1, perm, seed + 10 * R + y0 + perm)


@pytest.mark.parametrize("ny,R,nprop", [(64, 7, 1), (64, 7, 2), (64, 6, 1), (32, 5, 1), (48, 4, 2)])
def test_windowed_rows_several_rows_per_wave(hip, ny, R, nprop):
    # 16384 modes (the 64^3 plane): 256 workgroup columns, so that a row group sweeps SEVERAL positions -- one group of R rows for two
    # blocks, two groups (R = 7: 3 + 4, the odd and the even exit of the two-register-set loop; R = 6: 3 + 3) for one block -- with the
    # row-ahead prefetch following the order
    for perm in (False, True):
        _case(hip, ny, 16384, 16384, R, nprop, 0, ny, perm, 77 + ny + R + nprop + perm)
    _case(hip, ny, 16384, 16384 + 16, R, nprop, 8, ny - 3, True, 91 + ny + R)


def test_argument_validation(hip):
    from geobo_amd import _lib
    lib = _lib.load()
    ny, C, S, R = 32, 64, 64, 2
    pool, edge = _rand((3 * ny * S,), 1), _rand((R * 2 * S,), 2)
    row_off = torch.zeros(R, dtype=torch.int64, device="cuda")
    tab, out = _rand((ny * C,), 3), torch.zeros(R * ny * S, dtype=F64, device="cuda")
    basis = hip.spectral_y_basis(ny, pool.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(ny=ny, C=C, S=S, R=R, nprop=1, pool=pool, row_off=row_off, edge=edge, edge_row=2 * S, tab0=tab, tab1=None, out0=out, out1=None,
             y0=0, y1=None, basis=basis, pool_shift=0, edge_shift=0):
        pp = ctypes.c_void_p(pool.data_ptr() + pool_shift) if pool is not None else None
        pe = ctypes.c_void_p(edge.data_ptr() + edge_shift) if edge is not None else None
        return lib.geobo_spectral_y_lattice(ny, C, S, R, nprop, pp, p(row_off), pe, edge_row, None, p(tab0), p(tab1), p(out0), p(out1),
                                            y0, ny if y1 is None else y1, p(basis), None)

    E_ARG, E_ALIGN, E_UNSUPPORTED = -1, -2, -4
    for kw in (dict(pool=None), dict(row_off=None), dict(edge=None), dict(tab0=None), dict(out0=None), dict(basis=None),
               dict(nprop=2), dict(nprop=2, tab1=tab), dict(nprop=3), dict(nprop=0), dict(R=0), dict(y0=-1), dict(y1=ny + 1), dict(y0=8, y1=8),
               dict(S=C - 16)):
        assert call(**kw) == E_ARG, kw
    for kw in (dict(C=0), dict(C=72, S=80), dict(S=(1 << 31) // (8 * ny)), dict(edge_row=2 * S + 1), dict(S=C + 1), dict(pool_shift=8),
               dict(edge_shift=8)):
        assert call(**kw) == E_ALIGN, kw
    for bad in (16, 80, 128):
        assert call(ny=bad, y1=bad) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                  # no refused call touched the device
    assert call() == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        hip.spectral_y_lattice(ny, C, R, pool, row_off, edge, 2 * S + 1, None, [tab], [out])


# ---- the pooled feed of the product, 64 x 32 x 64 (the smallest grid it applies to) --------------------------------------------------
NX, NY, NZ = 64, 32, 64


@pytest.fixture(scope="module")
def product(hip):
    """SpectralProduct on its own + a synthetic lattice operator: random stencil table and boundary slabs (the product is linear in
    them; no geometry needed), 192 sensors in an order that is NOT row-major and that contains the windows at both ends of the pool."""
    from geobo_amd.spectral import LatticeRows, SpectralProduct
    sp = SpectralProduct(NX, NY, NZ, "cuda", rows_per_batch=16)
    assert sp.pool_applies() and sp.R == 16
    Ms, nqx = 192, 2 * NX - 1
    jy = np.concatenate([np.zeros(64), np.ones(64), np.full(64, NY - 1)]).astype(np.int64)       # rows 0 .. 127 row-major: jy 0, 1
    jx = np.concatenate([np.arange(64), np.arange(64), np.arange(64)[::-1]]).astype(np.int64)
    jy[128:] = np.where(np.arange(64) % 2 == 0, NY - 1, 0)                                       # then jx descending, jy at both extremes
    Q = _rand(((2 * NY - 3) * nqx * NZ,), 5)
    edge = _rand((Ms, 2 * NX * NZ), 6)
    row_off = torch.from_numpy(((NY - 2 - jy) * nqx + (NX - 1 - jx)) * NZ).cuda()
    lat = LatticeRows(Q, row_off, nqx * NZ, edge, jy=jy, jx=jx)
    gens = [_rand((NY * sp.Px * sp.Pz,), 7 + j) for j in range(2)]
    return sp, lat, Ms, gens


@pytest.mark.parametrize("nblocks", [2, 1])
@pytest.mark.parametrize("r0,R", [(0, 12), (58, 11), (120, 40)])
def test_pooled_product_matches_lattice_feed(product, r0, R, nblocks):
    # rows 0 .. 11; a batch that straddles the jy change at row 64; one that runs over several batches of the product (16 rows each)
    # and into the rows at the ends of the pool (jy = 0 / ny - 1 at jx' = 0: windows that start one plane in front of the pool)
    sp, lat, Ms, gens = product
    N = NX * NY * NZ
    ref = [torch.full((R, N), float("nan"), dtype=F64, device="cuda") for _ in range(nblocks)]
    sp.product(lat.rows(r0), R, gens[:nblocks], ref)
    pool = sp.plane_pool(lat, Ms, lat.jy, lat.jx)
    out = [torch.full((R, N), float("nan"), dtype=F64, device="cuda") for _ in range(nblocks)]
    sp.product(pool.rows(r0), R, gens[:nblocks], out)
    torch.cuda.synchronize()
    for j in range(nblocks):
        assert not bool(torch.isnan(ref[j]).any())
        assert torch.equal(out[j], ref[j])


def test_pooled_product_slab_and_accounting(product):
    # a y-slab of the output (the column-sharded engine's call) and the figures handed to the per-kernel timer: input bytes = the
    # batch's distinct planes once
    from geobo_amd.spectral import pool_distinct_planes
    sp, lat, Ms, gens = product
    r0, R, y0, y1 = 64, 16, 8, 24
    w = (y1 - y0) * NX * NZ
    ref = [torch.empty((R, w), dtype=F64, device="cuda") for _ in range(2)]
    sp.product(lat.rows(r0), R, gens, ref, y0, y1)
    pool = sp.plane_pool(lat, Ms, lat.jy, lat.jx)
    seen = []
    sp.kernel_timer = lambda name, nbytes, fn, valu=0.0, flop=0.0: (seen.append((name, nbytes)), fn())[1]
    try:
        out = [torch.empty((R, w), dtype=F64, device="cuda") for _ in range(2)]
        sp.product(pool.rows(r0), R, gens, out, y0, y1)
    finally:
        sp.kernel_timer = None
    torch.cuda.synchronize()
    assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])
    C = sp.Px * sp.Pz
    distinct = pool_distinct_planes(NY, lat.jy[r0:r0 + R], lat.jx[r0:r0 + R])
    assert distinct == 16 * (NY - 2) + 2 * 16                     # 16 rows of one jy, 16 different jx: nothing shared
    assert seen == [("kernel:toeplitz_y", 8.0 * C * (distinct + R * 2 * (y1 - y0)))]
    assert sp.flops(Ms, 2, NY, fwd_planes=sp.pool_planes(Ms)) < sp.flops(Ms, 2, NY)
