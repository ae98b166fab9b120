"""The argument behind the mirrored magnetic block of AkA ("point mirror"), pinned with the NumPy oracle and no
device: on a row-major lattice survey with a sensor over every voxel column and a vertical ambient field, B = A_m K_11 A_m^T is
centrosymmetric, B[Ms-1-r, Ms-1-c] = B[r, c], so its second half is the flip of its first -- and the gravity block is NOT (the
+-1e6 m padding of A_sens, sensormodel.py:63-68, breaks the mirror of the gravity potential on the two padded planes), which is why
the engine measures the operator instead of trusting its name."""
import numpy as np
import pytest

from oracle import geobo_oracle as O


@pytest.fixture(scope="module")
def blocks16():
    """(MM, GG, A_m, A_g) of the 16^3 survey: the two diagonal blocks of AkA as full products, computed once."""
    G = O.Grid(nx=16, ny=16, nz=16, xmax=1600.0, ymax=1600.0, zLcube=1600.0, kernelfunc="matern32")
    loc, edges = G.sensor_locations(), G.edges()
    A_g = O.a_sens(G, G.B * 0.0, loc, edges, "grav")
    A_m = O.a_sens(G, G.B, loc, edges, "magn")
    lengths, W = np.array([200.0, 202.0, 204.0]), O.weight_matrix(G.gp_coeff)
    D2 = O.sqdist(O.grid_points((G.nx, G.ny, G.nz), (G.sx, G.sy, G.sz)))
    MM = A_m @ O.k_block("matern32", D2, lengths, W, 1, 1) @ A_m.T
    GG = A_g @ O.k_block("matern32", D2, lengths, W, 0, 0) @ A_g.T
    return MM, GG, A_m, A_g, G


def _rebuilt(B):
    """The block with its rows r >= ceil(n / 2) replaced by the point mirror of the first half (what geobo_centro_fill writes)."""
    n = B.shape[0]
    r0 = (n + 1) // 2
    out = B.copy()
    out[r0:] = B[:n - r0][::-1, ::-1]
    return out


def _operator_mirror(A, G):
    """A[Ms-1-r, flip(v)]: sensors reversed, voxels flipped in y and x, z kept."""
    return A[::-1].reshape(-1, G.ny, G.nx, G.nz)[:, ::-1, ::-1, :].reshape(A.shape)


def test_magnetic_block_is_its_own_point_mirror(blocks16):
    MM, _, A_m, _, G = blocks16
    dev_op = np.abs(A_m - _operator_mirror(A_m, G)).max() / np.abs(A_m).max()
    err = np.abs(_rebuilt(MM) - MM).max() / np.abs(MM).max()
    print("16^3 magnetic: operator mirror deviation %.2e (gate 2^-48 = %.2e), rebuilt block %.2e" % (dev_op, 2.0 ** -48, err))
    assert dev_op <= 2.0 ** -48
    assert err <= 1e-13


def test_gravity_block_is_not(blocks16):
    _, GG, _, A_g, G = blocks16
    dev_op = np.abs(A_g - _operator_mirror(A_g, G)).max() / np.abs(A_g).max()
    err = np.abs(_rebuilt(GG) - GG).max() / np.abs(GG).max()
    print("16^3 gravity: operator mirror deviation %.2e, rebuilt block %.2e" % (dev_op, err))
    assert dev_op > 2.0 ** -48
    assert not err <= 1e-13


def test_inclined_field_is_not():
    """The same survey under the field (0.3, 0.2, 0.9): the magnetic operator loses the mirror, the gate must see it."""
    G = O.Grid(nx=16, ny=16, nz=16, xmax=1600.0, ymax=1600.0, zLcube=1600.0, kernelfunc="matern32", mag=(0.3, 0.2, 0.9))
    rows = [0, 17, 100, 255]
    loc, edges = G.sensor_locations(), G.edges()
    A = O.a_sens(G, G.B, loc, edges, "magn", rows=rows)
    Am = O.a_sens(G, G.B, loc, edges, "magn", rows=[255 - r for r in rows])
    mirrored = Am.reshape(-1, G.ny, G.nx, G.nz)[:, ::-1, ::-1, :].reshape(A.shape)
    assert np.abs(A - mirrored).max() > 1e-3 * np.abs(A).max()


def test_fill_arguments_are_validated_before_any_device_call():
    """geobo_centro_fill / geobo_mirror_rows refuse a source row that would be written (2 r0 < n) and null pointers."""
    from geobo_amd import _lib
    L = _lib.load()
    assert L.geobo_centro_fill(None, 8, 6, 3, None) == -1
    assert L.geobo_centro_fill(4096, 8, 6, 2, None) == -1            # r0 = n/2 - 1: row 3 would be source and destination
    assert L.geobo_centro_fill(4096 + 8, 8, 6, 3, None) == -1        # not 16-byte aligned
    assert L.geobo_centro_fill(4096, 4, 6, 3, None) == -1            # ld < n
    assert L.geobo_centro_fill(4096, 7, 6, 3, None) == -2            # odd leading dimension
    assert L.geobo_mirror_rows(None, 64, 4, 2, 4, 16, None) == -1
    assert L.geobo_mirror_rows(4096, 64, 4, 1, 4, 16, None) == -1
    assert L.geobo_mirror_dev(None, 8, None, 8, 1, 2, 4, None, None, 0, None) == -1
