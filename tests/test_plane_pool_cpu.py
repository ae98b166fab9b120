"""Index tables of the distinct-plane pool of a lattice operator (geobo_amd/spectral.py: pool_row_off, pool_plane_source, pool_order,
pool_distinct_planes): pure arithmetic, checked against the description of the rows as windows of the stencil table
(operators.StreamedOperator.keep_stencil: plane y of row r at Q + row_off[r] + y q_plane).  No GPU."""
import numpy as np
import pytest

from geobo_amd.spectral import pool_distinct_planes, pool_layout, pool_order, pool_plane_source, pool_row_off


def _survey(nx, ny, seed):
    """Every node of the nx x ny lattice once, in a permuted sensor order (r != jy nx + jx)."""
    perm = np.random.default_rng(seed).permutation(nx * ny)
    return perm // nx, perm % nx


CASES = [(4, 5, 3, 1), (6, 4, 2, 2), (5, 7, 4, 3)]


@pytest.mark.parametrize("nx,ny,nz,seed", CASES)
def test_windows_resolve_to_the_rows_own_planes(nx, ny, nz, seed):
    jy, jx = _survey(nx, ny, seed)
    Cp = 4 * nx * nz + 6                                                  # any plane stride of the spectrum
    nqx, q_plane = 2 * nx - 1, (2 * nx - 1) * nz
    q_row_off = ((ny - 2 - jy) * nqx + (nx - 1 - jx)) * nz                # keep_stencil's windows of Q[2ny-3][2nx-1][nz]
    off = pool_row_off(nx, ny, Cp, jy, jx)
    assert off.dtype == np.int64 and off.shape == (nx * ny,)
    assert (off % Cp == 0).all()
    n_int = nx * (2 * ny - 3)
    for r in range(nx * ny):
        for y in range(1, ny - 1):
            p = off[r] // Cp + y                                          # pool plane the y stage reads for (r, y)
            assert 0 <= p < n_int                                         # inside the interior pool
            src = pool_plane_source(nx, ny, nz, p)                        # what the pool's forward launch transformed into it
            assert src == q_row_off[r] + y * q_plane
            assert 0 <= src and src + nx * nz <= (2 * ny - 3) * q_plane   # a whole window inside the table
    # (planes 0 and ny - 1 of a window are never read: they may fall one plane outside the pool, and only there)
    assert off.min() >= -Cp and off.max() + (ny - 1) * Cp <= n_int * Cp


@pytest.mark.parametrize("nx,ny,nz,seed", CASES)
def test_pool_source_is_one_strided_launch(nx, ny, nz, seed):
    # the interior pool is ONE forward launch with rows = nx, planes per row = 2ny-3, in_row = nz, in_plane = q_plane
    q_plane, nd = (2 * nx - 1) * nz, 2 * ny - 3
    p = np.arange(nx * nd)
    assert (pool_plane_source(nx, ny, nz, p) == (p // nd) * nz + (p % nd) * q_plane).all()


@pytest.mark.parametrize("nx,ny,nz,seed", CASES)
def test_edge_planes_are_the_rows_own(nx, ny, nz, seed):
    # the boundary pool is [Ms][2][Cp] in the operator's row order behind the interior pool: row r reads its planes 0 / ny - 1 at
    # r * edge_row (+ Cp) whatever (jy, jx) it has -- two rows with the same window still have distinct boundary planes -- and no
    # window's interior reaches into it
    jy, jx = _survey(nx, ny, seed)
    Ms, Cp = nx * ny, 2 * nx * 2 * nz
    n_int, edge_off, edge_row, planes = pool_layout(nx, ny, Ms, Cp)
    assert n_int == nx * (2 * ny - 3) and planes == n_int + 2 * Ms and edge_off == n_int * Cp and edge_row == 2 * Cp
    first = edge_off + np.arange(Ms) * edge_row
    both = np.concatenate([first, first + Cp])
    assert np.unique(both).size == 2 * Ms and both.min() == edge_off and both.max() + Cp == planes * Cp
    off = pool_row_off(nx, ny, Cp, jy, jx)
    assert (off + (ny - 2) * Cp + Cp <= edge_off).all()                    # last interior plane of every window ends in front of it


@pytest.mark.parametrize("nx,ny,nz,seed", CASES)
@pytest.mark.parametrize("r0,R", [(0, None), (3, 9), (5, 1)])
def test_order_sweeps_by_jx_then_jy(nx, ny, nz, seed, r0, R):
    jy, jx = _survey(nx, ny, seed)
    R = nx * ny - r0 if R is None else R
    by, bx = jy[r0:r0 + R], jx[r0:r0 + R]
    order = pool_order(by, bx)
    assert order.dtype == np.int32
    assert sorted(order.tolist()) == list(range(R))                       # a permutation of the batch's rows
    sx, sy = bx[order], by[order]
    for i in range(1, R):
        assert sx[i] > sx[i - 1] or (sx[i] == sx[i - 1] and sy[i] > sy[i - 1])     # equal jx consecutive, jy ascending inside


def test_distinct_planes_of_a_batch():
    # four jy x all jx of a 64 x 64 lattice: 62 + 3 interior planes per jx and 2 boundary planes per row
    ny, nx = 64, 64
    jy, jx = np.repeat(np.arange(8, 12), nx), np.tile(np.arange(nx), 4)
    assert pool_distinct_planes(ny, jy, jx) == nx * (62 + 3) + 2 * 4 * nx
    # one row: its own ny - 2 interior planes + 2; the same row twice: the interior planes once
    assert pool_distinct_planes(ny, [5], [7]) == 64
    assert pool_distinct_planes(ny, [5, 5], [7, 7]) == 62 + 4
    # a batch that straddles rows of different jx shares nothing between them
    assert pool_distinct_planes(ny, [5, 5], [7, 8]) == 2 * 62 + 4
