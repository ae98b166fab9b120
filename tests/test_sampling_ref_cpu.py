"""The references of tests/_sampling_ref.py checked on their own (no GPU): the long-double DFT against np.fft at every length the
sampler's FFT accepts, the real-pair layout round trips, the octant multiplicities, and psd_part on known decompositions."""
import numpy as np
import pytest

import _sampling_ref as R

LENGTHS = [2, 4, 8, 16, 32, 64, 128, 256, 512]          # every length geobo_fft_axis accepts
OTHER = [3, 5, 12, 100, 243]                             # the definition does not depend on the radix


def test_long_double_is_wider_than_fp64():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("m", LENGTHS + OTHER)
def test_dft_long_against_numpy(m, inverse):
    rng = np.random.default_rng(m + inverse)
    x = rng.standard_normal((5, m)) + 1j * rng.standard_normal((5, m))
    ref = R.dft_long(x, 1, inverse)
    assert ref.dtype == np.clongdouble and ref.shape == x.shape
    got = np.fft.ifft(x, axis=1) * m if inverse else np.fft.fft(x, axis=1)
    err = float((np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())
    # np.fft is an fp64 FFT: a handful of roundings per output.  The reference must agree with it to that, and no better than fp64
    # can: an error of the reference itself (angle, sign, index) would show as O(1) or O(1/m).
    assert err <= 16 * R.EPS, err
    # the definition on one output, summed term by term in long double
    k = m // 2 + (m > 2)
    j = np.arange(m)
    ang = 2 * R.PI_LD * ((j * k) % m).astype(np.longdouble) / m
    w = np.cos(ang) + (1j if inverse else -1j) * np.sin(ang)
    assert abs((x[2].astype(np.clongdouble) * w).sum() - ref[2, k]) <= 64 * float(np.finfo(np.longdouble).eps) * np.abs(x[2]).sum()


def test_dft_long_axis_and_round_trip():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 16, 5)) + 1j * rng.standard_normal((3, 16, 5))
    f = R.dft_long(x, 1)
    assert np.abs(f - np.fft.fft(x, axis=1)).max() <= 1e-13
    back = R.dft_long(f, 1, inverse=True) / 16
    assert np.abs(back - x).max() <= 1e-17
    # a unit impulse at j = 1: exp(-+2 pi i k / 8), whose values are 0, +-1 and +-sqrt(1/2) exactly
    e = np.zeros(8)
    e[1] = 1.0
    r = np.sqrt(np.longdouble(0.5))
    fwd = np.array([1, r - 1j * r, -1j, -r - 1j * r, -1, -r + 1j * r, 1j, r + 1j * r], dtype=np.clongdouble)
    tol = 4 * float(np.finfo(np.longdouble).eps)
    assert np.abs(R.dft_long(e) - fwd).max() <= tol
    assert np.abs(R.dft_long(e, inverse=True) - fwd.conj()).max() <= tol


@pytest.mark.parametrize("n_in,m,n_out", [(8, 8, 8), (5, 8, 4), (1, 8, 8), (8, 8, 1), (3, 64, 33), (1, 2, 1)])
def test_pad_crop_is_the_padded_transform_cropped(n_in, m, n_out):
    rng = np.random.default_rng(n_in * 100 + n_out)
    x = rng.standard_normal((2, n_in, 3)) + 1j * rng.standard_normal((2, n_in, 3))
    full = np.zeros((2, m, 3), dtype=complex)
    full[:, :n_in] = x
    for inverse in (False, True):
        want = R.dft_long(full, 1, inverse)[:, :n_out]
        got = R.pad_crop(x, n_in, m, n_out, axis=1, inverse=inverse)
        assert got.shape == (2, n_out, 3)
        assert np.abs(got - want).max() <= 1e-17 * m


@pytest.mark.parametrize("S", [1, 2, 3, 6, 7])
def test_pack_unpack_round_trip(S):
    rng = np.random.default_rng(S)
    P, Q = 3, 5
    K = (S + 1) // 2
    z = rng.standard_normal((K, P, Q)) + 1j * rng.standard_normal((K, P, Q))
    r = R.pack_pairs(z, S)
    assert r.shape == (S, P, Q) and r.dtype == np.float64
    for k in range(K):
        assert np.array_equal(r[2 * k], z[k].real)
        if 2 * k + 1 < S:
            assert np.array_equal(r[2 * k + 1], z[k].imag)
    back = R.unpack_pairs(r)
    assert back.shape == z.shape
    want = z.copy()
    if S % 2:
        want[-1] = want[-1].real              # the dropped imaginary sample reads as zero
    assert np.array_equal(back, want)
    assert np.array_equal(R.pack_pairs(back, S), r)
    # the flat address the header gives: element (s, p, q) of the real array at (s P + p) Q + q
    flat = r.reshape(-1)
    assert flat[((S - 1) * P + 2) * Q + 4] == (z[(S - 1) // 2, 2, 4].imag if (S - 1) % 2 else z[(S - 1) // 2, 2, 4].real)


@pytest.mark.parametrize("ext", [(2, 2, 2), (4, 2, 64), (16, 8, 32), (8, 16, 512)])
def test_multiplicity_counts_the_torus(ext):
    mult = R.multiplicity(ext)
    assert mult.shape == tuple(m // 2 + 1 for m in ext)
    assert int(mult.sum()) == ext[0] * ext[1] * ext[2]
    # the same count from the fold itself: how often every octant index occurs on the torus
    idx = R.octant_expand(np.arange(mult.size).reshape(mult.shape), ext)
    assert np.array_equal(np.bincount(idx.reshape(-1), minlength=mult.size).reshape(mult.shape), mult)


def test_octant_expand_is_even():
    ext = (4, 2, 8)
    rng = np.random.default_rng(0)
    a = rng.standard_normal((3, 2, 5, 2))
    full = R.octant_expand(a, ext)
    assert full.shape == (4, 2, 8, 2)
    for wy in range(4):
        for wx in range(2):
            for wz in range(8):
                assert np.array_equal(full[wy, wx, wz], a[min(wy, 4 - wy), min(wx, 2 - wx), min(wz, 8 - wz)])
                assert np.array_equal(full[wy, wx, wz], full[-wy % 4, -wx % 2, -wz % 8])


def test_psd_part_on_known_decompositions():
    th = 0.3
    c, s = np.cos(th), np.sin(th)
    V = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    cases = [(np.array([4.0, 1.0, 0.25]), V), (np.array([2.0, -3.0, 0.0]), V), (np.array([-1.0, -2.0, -3.0]), V),
             (np.array([5.0, 5.0, -1.0]), V), (np.zeros(3), np.eye(3))]
    S = np.stack([Vk @ np.diag(d) @ Vk.T for d, Vk in cases])
    psd, w, recon = R.psd_part(S)
    for k, (d, Vk) in enumerate(cases):
        want = Vk @ np.diag(np.maximum(d, 0.0)) @ Vk.T
        scale = max(np.abs(d).max(), 1.0)
        assert np.abs(psd[k] - want).max() <= 8 * R.EPS * scale
        assert np.abs(np.sort(w[k]) - np.sort(d)).max() <= 8 * R.EPS * scale
        assert recon[k] <= 8 * R.EPS * scale
    # batched shapes, P = 1 and P = 2
    assert R.psd_part(np.array([[[-2.0]], [[3.0]]]))[0].reshape(-1).tolist() == [0.0, 3.0]
    p2, w2, _ = R.psd_part(np.array([[0.0, 2.0], [2.0, 0.0]]))
    assert np.abs(p2 - np.ones((2, 2))).max() <= 4 * R.EPS and np.abs(w2 - [-2.0, 2.0]).max() <= 4 * R.EPS
