"""Block-support statistics without a GPU: the argument checks of geobo_block_cov, the host helpers (block
partition, lag-count weights of the prior term) against brute-force NumPy, and the checks block_statistics makes before it computes."""
import itertools

import numpy as np
import pytest

from conftest import settings_for

GRID = (8, 10, 6)                                             # (ny, nx, nz)
BOXES = [(1, 1, 1), (2, 2, 2), (4, 3, 4), GRID]               # (by, bx, bz); (4, 3, 4): partial edges on all three axes


# ---- 1. C ABI without a GPU ------------------------------------------------------------------------------------------------------
def test_block_cov_validates_without_gpu():
    from geobo_amd import _lib
    L = _lib.load()
    assert L.geobo_version() == 213
    p = 16                                                     # (never dereferenced: every call below fails its checks first)
    ws = L.geobo_block_cov_ws_bytes
    N = 5 * 6 * 7

    def call(R=37, V0=p, V1=p, V2=p, ldv=N, grid=(5, 6, 7), box=(2, 3, 4), C6=p, wsp=p, nbytes=None):
        nbytes = ws(37, 5, 6, 7, 2, 3, 4) if nbytes is None else nbytes
        return L.geobo_block_cov(R, V0, V1, V2, ldv, *grid, *box, 0, C6, wsp, nbytes, None)
    for name in ("V0", "V1", "V2", "C6", "wsp"):
        assert call(**{name: None}) == -1
    assert call(R=-1) == -1
    for axis in range(3):
        zero = lambda t: tuple(0 if i == axis else v for i, v in enumerate(t))
        assert call(grid=zero((5, 6, 7)), box=(1, 1, 1)) == -1        # an extent < 1
        assert call(box=zero((2, 3, 4))) == -1                        # a box edge < 1
        assert call(box=tuple(-1 if i == axis else v for i, v in enumerate((2, 3, 4)))) == -1
        assert call(box=tuple(g + 1 if i == axis else 1 for i, g in enumerate((5, 6, 7)))) == -1     # a box edge beyond its extent
    assert call(ldv=N - 1) == -1
    assert call(nbytes=ws(37, 5, 6, 7, 2, 3, 4) - 8) == -1            # workspace too small
    assert call(nbytes=0) == -1
    # the workspace size: 0 for invalid arguments, a multiple of 16 otherwise
    assert ws(-1, 5, 6, 7, 1, 1, 1) == 0
    assert ws(4, 0, 6, 7, 1, 1, 1) == 0 and ws(4, 5, 0, 7, 1, 1, 1) == 0 and ws(4, 5, 6, 0, 1, 1, 1) == 0
    assert ws(4, 5, 6, 7, 0, 1, 1) == 0 and ws(4, 5, 6, 7, 1, 0, 1) == 0 and ws(4, 5, 6, 7, 1, 1, 0) == 0
    assert ws(4, 5, 6, 7, 6, 1, 1) == 0 and ws(4, 5, 6, 7, 1, 7, 1) == 0 and ws(4, 5, 6, 7, 1, 1, 8) == 0
    for R in (0, 1, 37, 130, 8960):
        for grid, box in (((5, 6, 7), (1, 1, 1)), ((5, 6, 7), (2, 3, 4)), ((5, 6, 7), (5, 6, 7)), ((4, 4, 64), (2, 2, 4)),
                          ((64, 64, 64), (1, 1, 1)), ((64, 64, 64), (16, 16, 16)), ((64, 64, 64), (64, 64, 64)), ((3, 3, 300), (1, 1, 300))):
            b = ws(R, *grid, *box)
            assert b > 0 and b % 16 == 0, (R, grid, box, b)


# ---- 2. host helpers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", BOXES)
def test_block_partition_matches_brute_force(box):
    from geobo_amd.blocksupport import block_counts, block_extents, block_partition
    ny, nx, nz = GRID
    nb = block_counts(GRID, box)
    assert nb == tuple(-(-n // b) for n, b in zip(GRID, box))
    index, count = block_partition(GRID, box)
    want = np.empty(GRID, dtype=np.int64)
    for iy, ix, iz in itertools.product(range(ny), range(nx), range(nz)):
        want[iy, ix, iz] = ((iy // box[0]) * nb[1] + ix // box[1]) * nb[2] + iz // box[2]
    assert index.dtype == np.int64 and np.array_equal(index, want.reshape(-1))
    assert np.array_equal(count, np.array([(want == b).sum() for b in range(nb[0] * nb[1] * nb[2])]))
    assert count.sum() == ny * nx * nz and count.min() >= 1
    ext = block_extents(GRID, box)
    assert ext.shape == (count.size, 3) and np.array_equal(ext.prod(axis=1), count)
    for b in range(count.size):
        cells = np.argwhere(want == b)
        assert np.array_equal(ext[b], cells.max(axis=0) - cells.min(axis=0) + 1)


def test_lag_counts_count_ordered_pairs():
    from geobo_amd.blocksupport import lag_counts
    for m in (1, 2, 3, 4, 6, 10):
        i = np.arange(m)
        d = i[:, None] - i[None, :]
        assert np.array_equal(lag_counts(m), np.array([(np.abs(d) == k).sum() for k in range(m)]))
        assert np.array_equal(lag_counts(m, signed=True), np.array([(d == k).sum() for k in range(-(m - 1), m)]))
        assert lag_counts(m).sum() == m * m and lag_counts(m, signed=True).sum() == m * m


@pytest.mark.parametrize("box", BOXES)
def test_prior_block_mean_sums_all_pairs_of_a_block(box):
    """Every distinct block shape of the box, on a random table that is NOT symmetric in dz (the z axis of the table is signed)."""
    from geobo_amd.blocksupport import block_extents, mean_weights, prior_block_mean
    ny, nx, nz = GRID
    rng = np.random.default_rng(sum(box))
    table = rng.standard_normal(2 * ny * nx * nz + 5)          # (trailing entries, as a padded buffer, are ignored)
    T = table[:2 * ny * nx * nz].reshape(ny, nx, 2 * nz)
    for ext in np.unique(block_extents(GRID, box), axis=0):
        cells = np.array(list(itertools.product(*(range(int(m)) for m in ext))))
        d = cells[:, None, :] - cells[None, :, :]
        want = T[np.abs(d[..., 0]), np.abs(d[..., 1]), d[..., 2] + nz - 1].sum() / float(len(cells)) ** 2
        got = prior_block_mean(table, GRID, ext)
        assert abs(got - want) <= 1e-13 * np.abs(T).max(), (box, ext, got, want)
        assert abs(mean_weights(ext).sum() - 1.0) <= 1e-14


# ---- 3. the public interface checks before it computes ---------------------------------------------------------------------------
def test_block_statistics_checks_before_any_device_call():
    from geobo_amd.engine import PosteriorEngine
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=settings_for(10, 8, 6))
    with pytest.raises(RuntimeError, match="cubing"):
        inv.block_statistics((2, 2, 2))
    with pytest.raises(RuntimeError, match="cubing"):
        inv.block_statistics((10, 8, 6), write=True)
    inv.Fs3, inv._cube_scale = np.zeros(3), (1.0, 1.0, 1.0)    # as after cubing(): the box is still checked without a device
    for bad in ((0, 1, 1), (1, -2, 1), (1, 1), (1, 1, 1, 1), (1.5, 1, 1), ("2", 2, 2), (True, 1, 1), 4, None,
                (11, 1, 1), (1, 9, 1), (1, 1, 7)):                # the last three exceed an extent (x, y, z = 10, 8, 6)
        with pytest.raises(ValueError, match="block"):
            inv.block_statistics(bad)
    assert inv._engine is None                                 # nothing above built an engine
    assert callable(PosteriorEngine.block_covariance)
