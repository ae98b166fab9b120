"""Prior realisations of the three-property GP on the voxel grid by circulant embedding.

The prior K of create_cov (kernels.py:158-195) is stationary on the regular grid: block (i, j) is w_ij k(l1 = l_j, l2 = l_i) of the lag.
Embedded in a torus (my, mx, mz) of powers of two >= 2n per axis, every block becomes circulant, the 3-D FFT diagonalises it, and the
P x P matrix S(w) = [lambda_ij(w)] of each frequency carries the cross-covariance.  With F(w) F(w)^T = S(w),

    f = crop(IFFT(F xi)) / sqrt(my mx mz),   xi_q(w) complex standard normal,

has real and imaginary parts that are two independent N(0, K) samples.  The same spectra give K v = crop(IFFT(S FFT(pad v))) / M exactly
(no clipping), which the conditioning step uses (PosteriorEngine.condition).

plan_torus is the pure padding rule (CPU-tested); PriorSampler holds the device tables of one (grid, kernel, lengths, weights, amp).
"""
import numpy as np
import torch

from . import hip

F64 = hip.F64
PSD_TOL = 1e-12                 # min/max eigenvalue ratio accepted as round-off (clipped to 0)
MAX_DOUBLINGS = 2               # start >= 2n per axis: two doublings reach >= 8n
TORUS_BYTES_CAP = 6 << 30       # device bytes of the spectra build (tables + one transform buffer)


class SamplingError(RuntimeError):
    """The prior cannot be sampled exactly: its (3N)^2 covariance is not positive semi-definite."""


def _pow2_at_least(v):
    m = 2
    while m < v:
        m *= 2
    return m


def torus_bytes(ext, P=3):
    """Bytes of the spectra build on a torus: P(P+1)/2 complex tables and one transform buffer of the same size."""
    return 2 * (P * (P + 1) // 2) * int(np.prod(ext)) * 16


def plan_torus(grid, P=3, cap_bytes=TORUS_BYTES_CAP):
    """Candidate tori of the padding rule for grid (ny, nx, nz), smallest first: the smallest powers of two >= 2n per axis, then every
    axis doubled, at most MAX_DOUBLINGS times, while the spectra build fits in cap_bytes and every axis stays <= hip.FFT_MAX."""
    start = tuple(_pow2_at_least(2 * int(n)) for n in grid)
    out = []
    for t in range(MAX_DOUBLINGS + 1):
        ext = tuple(m << t for m in start)
        if max(ext) > hip.FFT_MAX or (out and torus_bytes(ext, P) > cap_bytes):
            break
        out.append(ext)
    if not out:
        raise ValueError("grid %s needs a torus axis above %d: larger than the sampler's FFT" % (tuple(grid), hip.FFT_MAX))
    return out


def choose_torus(grid, ratio_of, P=3, cap_bytes=TORUS_BYTES_CAP):
    """The padding rule: the first candidate torus whose min/max eigenvalue ratio (ratio_of(ext)) is >= -PSD_TOL, else the last one
    tried.  Returns (ext, ratio)."""
    for ext in plan_torus(grid, P, cap_bytes):
        r = ratio_of(ext)
        if r >= -PSD_TOL:
            return ext, r
    return ext, r


class PriorSampler:
    """Circulant-embedding sampler of N(0, K) for P <= 3 property blocks on an (ny, nx, nz) grid of voxel sizes (sx, sy, sz).
    kernelfunc, lengths (after create_cov's mutation), W (weight_matrix) and amp as create_cov / the engine's assembly use them."""

    def __init__(self, grid, vox, kernelfunc, lengths, W, amp=1.0, P=3, device="cuda", approximate=False, cap_bytes=TORUS_BYTES_CAP):
        self.grid = tuple(int(v) for v in grid)
        self.vox = tuple(float(v) for v in vox)
        self.name, self.P, self.device = kernelfunc, int(P), device
        self.lengths = [float(v) for v in lengths]
        self.W = [[float(W[i][j]) for j in range(3)] for i in range(3)]
        self.amp = float(amp)
        self.N = int(np.prod(self.grid))
        self.pairs = [(i, j) for i in range(self.P) for j in range(i, self.P)]
        self.ext, self.ratio = choose_torus(self.grid, self._build, self.P, cap_bytes)
        if self.ext != getattr(self, "_built", None):
            self._build(self.ext)
        st = self.status
        self.clipped_fraction = float(st[2] / st[3]) if st[3] > 0 else 0.0
        if self.ratio < -PSD_TOL and not approximate:
            w = self.W
            raise SamplingError("the prior covariance is not positive semi-definite: min/max eigenvalue ratio %.3e on the %s torus "
                                "(block weights w1 = %g (0-2), w2 = %g (1-2), w3 = %g (0-1), lengths %s); choose weights that make the "
                                "3 x 3 cross-spectra PSD, or pass approximate=True to clip the negative part (clipped fraction %.3e)"
                                % (self.ratio, "x".join(map(str, self.ext)), w[0][2], w[1][2], w[0][1], self.lengths, self.clipped_fraction))

    def key(self):
        return (self.grid, self.vox, self.name, tuple(self.lengths), tuple(map(tuple, self.W)), self.amp, self.P)

    def _build(self, ext):
        """Tables, spectra and per-frequency factors on the torus ext; returns the min/max eigenvalue ratio."""
        my, mx, mz = ext
        M, npr, P = my * mx * mz, len(self.pairs), self.P
        sx, sy, sz = self.vox
        self.spectra = self.F = self.lam = None
        tab = torch.empty(npr * M * 2, dtype=F64, device=self.device)
        tmp = torch.empty_like(tab)
        for p, (i, j) in enumerate(self.pairs):
            hip.torus_table(hip.kernel_id(self.name, i != j), my, mx, mz, sx, sy, sz, self.lengths[j], self.lengths[i], self.W[i][j], self.amp,
                            tab[p * M * 2:(p + 1) * M * 2])
        self.table = tab                                                        # (kept for the tests: the crop is K)
        hip.fft_axis(0, npr * my * mx, mz, 1, mz, mz, tab, tmp)                  # z
        spec = torch.empty_like(tab)
        hip.fft_axis(0, npr * my, mx, mz, mx, mx, tmp, spec)                     # x
        del tmp
        out = torch.empty_like(tab)
        hip.fft_axis(0, npr, my, mx * mz, my, my, spec, out)                     # y
        self.spectra = out
        no = (my // 2 + 1) * (mx // 2 + 1) * (mz // 2 + 1)
        self.F = torch.empty(no * P * P, dtype=F64, device=self.device)
        self.lam = torch.empty(no * npr, dtype=F64, device=self.device)
        ws = torch.empty(hip.sample_factor_ws_doubles(), dtype=F64, device=self.device)
        st = torch.empty(4, dtype=F64, device=self.device)
        hip.sample_factor(P, my, mx, mz, out, self.F, self.lam, ws, st)
        self.status = st.cpu().numpy()
        self._built = tuple(ext)
        emin, emax = float(self.status[0]), float(self.status[1])
        return emin / emax if emax > 0 else -np.inf

    def release_tables(self):
        """Drop what only set-up and the tests need (tables and full spectra); the factors and the octant spectra stay."""
        self.table = self.spectra = None

    def _pair_budget(self, per_pair_bytes, budget=1 << 30):
        return max(1, int(budget // max(per_pair_bytes, 1)))

    def sample(self, start, n, seed=0, noise=None, out=None):
        """Prior samples start .. start + n - 1: (n, P, N) fp64 device tensor.  Sample k is the real (k even) or imaginary (k odd) part of
        pair k // 2, so it is the same whatever batch it is drawn in.  noise (tests): complex (npairs, M, P) per pair of the samples'
        pairs, as a (npairs * M * P * 2,) fp64 device tensor, replacing Philox."""
        my, mx, mz = self.ext
        ny, nx, nz = self.grid
        P, N = self.P, self.N
        k0, k1 = start // 2, (start + n + 1) // 2        # pairs covering the samples
        res = out if out is not None else torch.empty((n, P, N), dtype=F64, device=self.device)
        per_pair = P * my * mx * nz * 16 + P * my * nx * nz * 16
        step = self._pair_budget(per_pair)
        M = my * mx * mz
        for a in range(k0, k1, step):
            b = min(k1, a + step)
            npairs = b - a
            z = torch.empty(npairs * P * my * mx * nz * 2, dtype=F64, device=self.device)
            nzv = None if noise is None else noise[(a - k0) * M * P * 2:(b - k0) * M * P * 2]
            hip.sample_zpass(P, a, npairs, my, mx, mz, nz, self.F, z, seed=seed, noise=nzv)
            x = torch.empty(npairs * P * my * nx * nz * 2, dtype=F64, device=self.device)
            hip.fft_axis(hip.FFT_INVERSE, npairs * P * my, mx, nz, mx, nx, z, x)
            del z
            blk = torch.empty((2 * npairs, P, N), dtype=F64, device=self.device)
            hip.fft_axis(hip.FFT_INVERSE | hip.FFT_OUT_PAIRS, npairs * P, my, nx * nz, my, ny, x, blk, P=P, Q=N, S=2 * npairs)
            # samples 2a .. 2b - 1 of this block, clipped to [start, start + n)
            s0, s1 = max(2 * a, start), min(2 * b, start + n)
            res[s0 - start:s1 - start].copy_(blk[s0 - 2 * a:s1 - 2 * a])
        return res

    def apply_K(self, V, out=None):
        """K v for every row v of V ((S, P, N) fp64 device tensor, property-major rows as the engine's blocks): exact circulant product on
        the torus (the unclipped spectra), two real rows per complex transform."""
        my, mx, mz = self.ext
        ny, nx, nz = self.grid
        P, N, S = self.P, self.N, V.shape[0]
        V = V.contiguous()
        res = out if out is not None else torch.empty((S, P, N), dtype=F64, device=self.device)
        M = my * mx * mz
        step = 2 * self._pair_budget(2 * P * M * 16)
        for a in range(0, S, step):
            b = min(S, a + step)
            s, np_ = b - a, (b - a + 1) // 2
            src = V[a:b]
            t1 = torch.empty(np_ * P * ny * nx * mz * 2, dtype=F64, device=self.device)
            hip.fft_axis(hip.FFT_IN_PAIRS, np_ * P * ny * nx, mz, 1, nz, mz, src, t1, P=P, Q=N, S=s)
            t2 = torch.empty(np_ * P * ny * mx * mz * 2, dtype=F64, device=self.device)
            hip.fft_axis(0, np_ * P * ny, mx, mz, nx, mx, t1, t2)
            t3 = torch.empty(np_ * P * M * 2, dtype=F64, device=self.device)
            hip.fft_axis(0, np_ * P, my, mx * mz, ny, my, t2, t3)
            t4 = torch.empty_like(t3)
            hip.spectral_mix(P, np_, my, mx, mz, self.lam, 1.0 / M, t3, t4)
            del t3
            hip.fft_axis(hip.FFT_INVERSE, np_ * P, my, mx * mz, my, ny, t4, t2)
            del t4
            hip.fft_axis(hip.FFT_INVERSE, np_ * P * ny, mx, mz, mx, nx, t2, t1[:np_ * P * ny * nx * mz * 2])
            hip.fft_axis(hip.FFT_INVERSE | hip.FFT_OUT_PAIRS, np_ * P * ny * nx, mz, 1, mz, nz, t1, res[a:b], P=P, Q=N, S=s)
        return res


def observation_noise(seed, start, n, M, device="cuda"):
    """(n, M) standard normals of the observation noise of samples start .. start + n - 1: element e of sample s is normal e % 4 of the
    Philox block (e // 4, s, RNG_OBS, 0)."""
    nb = (M + 3) // 4
    z = hip.philox_fill(seed, hip.RNG_OBS, start, n, 0, nb, device=device)
    return z.reshape(n, nb * 4)[:, :M]
