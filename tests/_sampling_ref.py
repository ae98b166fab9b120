"""Plain references of the prior sampler's kernels (csrc/sampling.hip), written from the text of
include/geobo_hip.h: a long-double DFT by the explicit matrix, the (S, P, Q) real-pair layout, the octant fold of the even torus
spectra with its multiplicities, and the positive semi-definite part of a batch of symmetric matrices.

np.longdouble is the x87 80-bit format where the tests run (eps 1.08e-19): three decimal digits below any fp64 FFT, which is what
makes dft_long a reference for one.  Nothing here touches the device."""
import functools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = float(np.finfo(np.float64).eps)
# pi to 40 digits: the string is parsed in long double (np.pi is only the fp64 value)
PI_LD = LD("3.141592653589793238462643383279502884197")


@functools.lru_cache(maxsize=None)
def dft_matrix(m, inverse=False):
    """(m, m) long-double cos and sin of 2 pi ((j k) mod m) / m: W = cos -+ i sin (forward -, inverse +), no scaling."""
    jk = np.outer(np.arange(m, dtype=np.int64), np.arange(m, dtype=np.int64)) % m
    ang = (2 * PI_LD) * jk.astype(LD) / LD(m)
    c, s = np.cos(ang), np.sin(ang)
    return c, (s if inverse else -s)


def _apply(c, s, x):
    """(c + i s) @ x along axis 0 of x, four real long-double products."""
    xr, xi = np.real(x).astype(LD), np.imag(x).astype(LD)
    tail = x.shape[1:]
    xr, xi = xr.reshape(x.shape[0], -1), xi.reshape(x.shape[0], -1)
    out = np.empty((c.shape[0], xr.shape[1]), dtype=CLD)
    out.real = c @ xr - s @ xi
    out.imag = c @ xi + s @ xr
    return out.reshape((c.shape[0],) + tail)


def dft_long(x, axis=-1, inverse=False):
    """Unscaled DFT of x along axis as the product with the explicit matrix, in long double: out[k] = sum_j x[j] exp(-+2 pi i jk/m)."""
    x = np.moveaxis(np.asarray(x), axis, 0)
    c, s = dft_matrix(x.shape[0], bool(inverse))
    return np.moveaxis(_apply(c, s, x), 0, axis)


def pad_crop(x, n_in, m, n_out, axis=-1, inverse=False):
    """What geobo_fft_axis computes along one axis: x holds n_in entries, the rest of the length-m line is zero, and the first n_out
    outputs are kept -- out[k] = sum_{j < n_in} x[j] exp(-+2 pi i jk/m), k < n_out (the sum as the header states it)."""
    x = np.moveaxis(np.asarray(x), axis, 0)
    assert x.shape[0] == n_in and 1 <= n_in <= m and 1 <= n_out <= m
    c, s = dft_matrix(m, bool(inverse))
    return np.moveaxis(_apply(c[:n_out, :n_in], s[:n_out, :n_in], x), 0, axis)


def pack_pairs(z, S):
    """Complex (K, P, Q) with K = ceil(S / 2) -> real (S, P, Q): sample 2k is the real part of pair k, sample 2k + 1 its imaginary
    part; with odd S the last imaginary part has no slot and is dropped."""
    z = np.asarray(z)
    K = z.shape[0]
    assert K == (S + 1) // 2
    out = np.empty((S,) + z.shape[1:], dtype=z.real.dtype)
    out[0::2] = z.real
    out[1::2] = z.imag[:S // 2]
    return out


def unpack_pairs(r):
    """Real (S, P, Q) -> complex (ceil(S / 2), P, Q); the missing imaginary part of an odd S reads as zero."""
    r = np.asarray(r)
    S = r.shape[0]
    out = np.zeros(((S + 1) // 2,) + r.shape[1:], dtype=np.result_type(r.dtype, np.complex64))
    out.real = r[0::2]
    out.imag[:S // 2] = r[1::2]
    return out


def fold_index(m):
    """min(w, m - w) for w < m: the octant coordinate of torus frequency w."""
    w = np.arange(m)
    return np.minimum(w, m - w)


def octant_expand(a, ext):
    """Octant array (my/2+1, mx/2+1, mz/2+1, ...) -> the full torus (my, mx, mz, ...), even in every axis."""
    my, mx, mz = ext
    a = np.asarray(a)
    assert a.shape[:3] == (my // 2 + 1, mx // 2 + 1, mz // 2 + 1)
    return a[np.ix_(fold_index(my), fold_index(mx), fold_index(mz))]


def multiplicity(ext):
    """Number of torus frequencies every octant point stands for: per axis 1 at f = 0 and at 2 f = m, else 2."""
    per = []
    for m in ext:
        f = np.arange(m // 2 + 1)
        per.append(np.where((f == 0) | (2 * f == m), 1, 2))
    return per[0][:, None, None] * per[1][None, :, None] * per[2][None, None, :]


def psd_part(S):
    """V max(D, 0) V^T of a batch (..., P, P) of symmetric matrices by np.linalg.eigh.  Returns (psd, w, recon): the eigenvalues and
    eigh's own reconstruction error max|V D V^T - S| per matrix, the yardstick of a decomposition in fp64."""
    S = np.asarray(S, dtype=np.float64)
    w, V = np.linalg.eigh(S)
    recon = np.abs(np.einsum("...ik,...k,...jk->...ij", V, w, V) - S).max(axis=(-2, -1))
    psd = np.einsum("...ik,...k,...jk->...ij", V, np.maximum(w, 0.0), V)
    return psd, w, recon
