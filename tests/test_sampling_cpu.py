"""Prior sampler without a GPU: the padding rule against NumPy eigenvalues of the oracle's block tables, argument
validation of the new entry points, and the test suite's own Philox4x64-10 reference against NumPy's generator."""
import ctypes

import numpy as np
import pytest

from oracle import geobo_oracle as O

MASK = (1 << 64) - 1


def philox4x64_10(ctr, key):
    """Pure-Python Philox4x64-10 (Salmon et al., SC'11): 10 rounds, key bumped between rounds."""
    c = [int(v) for v in ctr]
    k0, k1 = int(key[0]), int(key[1])
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B97F4A7C15) & MASK, (k1 + 0xBB67AE8584CAA73B) & MASK
        p0, p1 = 0xD2E7470EE14C6C93 * c[0], 0xCA5A826395121157 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k0, p1 & MASK, (p0 >> 64) ^ c[3] ^ k1, p0 & MASK]
    return c


def numpy_block(seed, ctr):
    """The Philox block of counter ctr from NumPy: a generator started at counter ctr - 1 yields block ctr first."""
    v = sum(int(w) << (64 * i) for i, w in enumerate(ctr)) - 1
    v &= (1 << 256) - 1
    start = np.array([(v >> (64 * i)) & MASK for i in range(4)], dtype=np.uint64)
    return [int(w) for w in np.random.Philox(key=seed, counter=start).random_raw(4)]


@pytest.mark.parametrize("seed,ctr", [(0, (0, 0, 0, 0)), (7, (5, 3, 1, 0)), (123456789, (1 << 40, 17, 0, 1)), (2 ** 63 + 5, (MASK, 2, 1, 0))])
def test_numpy_philox_matches_pure_python(seed, ctr):
    assert numpy_block(seed, ctr) == philox4x64_10(ctr, (seed, 0))


def torus_ratio(name, m, lengths, w, h=1.0):
    """min/max eigenvalue over the frequencies of S(w) = [fftn(k_ij at the wrapped lags)] on the torus m (oracle block tables)."""
    ax = [np.minimum(np.arange(mm), mm - np.arange(mm)) * h for mm in m]
    dy, dx, dz = np.meshgrid(*ax, indexing="ij")
    d2 = dy ** 2 + dx ** 2 + dz ** 2
    W = O.weight_matrix(w)
    S = np.zeros(tuple(m) + (3, 3))
    for i in range(3):
        for j in range(i, 3):
            S[..., i, j] = S[..., j, i] = np.fft.fftn(O.k_block(name, d2, lengths, W, i, j)).real
    e = np.linalg.eigvalsh(S)
    return e.min() / e.max()


def test_torus_candidates():
    from geobo_amd.sampling import plan_torus
    assert plan_torus((8, 8, 8)) == [(16, 16, 16), (32, 32, 32), (64, 64, 64)]
    assert plan_torus((8, 10, 6)) == [(16, 32, 16), (32, 64, 32), (64, 128, 64)]
    assert plan_torus((64, 64, 64))[0] == (128, 128, 128)
    assert plan_torus((64, 64, 64), cap_bytes=1 << 30) == [(128, 128, 128)]      # the first candidate is always tried
    assert plan_torus((200, 64, 64)) == [(512, 128, 128)]                       # no axis above the FFT's 512
    with pytest.raises(ValueError):
        plan_torus((300, 8, 8))


@pytest.mark.parametrize("name,r16,r32", [("exp", -7.6e-5, -2.7e-17), ("matern32", -6.3e-4, 6.5e-5)])
def test_padding_rule_against_numpy_eigenvalues(name, r16, r32):
    """8^3, lengths (2, 2.04, 2.08) voxels, weights (0.2, 0.2, 0.2): the minimal 16^3 torus has negative eigenvalues, 32^3 is PSD to
    round-off; the rule stops at 32^3."""
    from geobo_amd.sampling import PSD_TOL, choose_torus
    lengths, w = np.array([2.0, 2.04, 2.08]), (0.2, 0.2, 0.2)
    seen = []

    def ratio_of(ext):
        seen.append(ext)
        return torus_ratio(name, ext, lengths, w)
    ext, r = choose_torus((8, 8, 8), ratio_of)
    assert ext == (32, 32, 32) and seen == [(16, 16, 16), (32, 32, 32)]
    assert r >= -PSD_TOL
    assert torus_ratio(name, (16, 16, 16), lengths, w) == pytest.approx(r16, rel=0.02)
    assert abs(r - r32) <= 0.02 * abs(r32) or abs(r32) < 1e-15


def test_indefinite_prior_is_not_fixed_by_the_torus():
    """Default weights (1.0, 0.2, 0.2) with distinct lengths: negative at every candidate torus."""
    from geobo_amd.sampling import PSD_TOL, choose_torus
    ext, r = choose_torus((8, 8, 8), lambda e: torus_ratio("exp", e, np.array([2.0, 2.04, 2.08]), (1.0, 0.2, 0.2)))
    assert ext == (64, 64, 64) and r < -PSD_TOL


@pytest.fixture(scope="module")
def lib():
    from geobo_amd.build import build
    from geobo_amd import _lib
    build()
    return _lib.load()


def test_sampling_entry_points_reject_bad_arguments_without_gpu(lib):
    """Every new entry point validates its arguments before it touches the device: -1 (GEOBO_E_ARG) on null pointers / bad extents."""
    fake = ctypes.c_void_p(16)
    assert lib.geobo_philox_fill(0, 1, 0, 0, 4, 0, 4, 0, None, None) == -1
    assert lib.geobo_philox_fill(2, 1, 0, 0, 4, 0, 4, 0, fake, None) == -1
    assert lib.geobo_torus_table(1, 16, 16, 16, 1.0, 1.0, 1.0, 2.0, 2.0, 1.0, 1.0, None, None) == -1
    assert lib.geobo_torus_table(1, 12, 16, 16, 1.0, 1.0, 1.0, 2.0, 2.0, 1.0, 1.0, fake, None) == -1    # not a power of two
    assert lib.geobo_torus_table(0, 16, 16, 16, 1.0, 1.0, 1.0, 2.0, 2.0, 1.0, 1.0, fake, None) == -1    # squared distance is no covariance
    assert lib.geobo_fft_axis(0, 4, 16, 1, 16, 16, None, fake, 0, 0, 0, None) == -1
    assert lib.geobo_fft_axis(0, 4, 1024, 1, 16, 16, fake, ctypes.c_void_p(32), 0, 0, 0, None) == -1   # above 512
    assert lib.geobo_fft_axis(0, 4, 16, 1, 17, 16, fake, ctypes.c_void_p(32), 0, 0, 0, None) == -1     # n_in > m
    assert lib.geobo_fft_axis(0, 4, 16, 1, 16, 16, fake, fake, 0, 0, 0, None) == -1                    # in place
    assert lib.geobo_fft_axis(2, 4, 16, 1, 16, 16, fake, ctypes.c_void_p(32), 0, 0, 0, None) == -1     # pairs without (P, Q, S)
    assert lib.geobo_sample_factor(3, 16, 16, 16, None, fake, fake, fake, 1 << 20, fake, None) == -1
    assert lib.geobo_sample_factor(4, 16, 16, 16, fake, fake, fake, fake, 1 << 20, fake, None) == -1
    assert lib.geobo_sample_factor(3, 16, 16, 16, fake, fake, fake, fake, 8, fake, None) == -1          # workspace too small
    assert lib.geobo_sample_zpass(3, 0, 1, 16, 16, 16, 8, None, None, 0, fake, None) == -1
    assert lib.geobo_sample_zpass(3, 0, 1, 16, 16, 16, 17, fake, None, 0, fake, None) == -1             # nz > mz
    assert lib.geobo_spectral_mix(3, 1, 16, 16, 16, None, 1.0, fake, ctypes.c_void_p(32), None) == -1
    assert lib.geobo_fft_lines(128, 1) == 32 and lib.geobo_fft_lines(256, 4096) == 16 and lib.geobo_fft_lines(100, 1) == 0
    assert lib.geobo_sample_factor_ws_bytes() > 0
