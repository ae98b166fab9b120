"""Spectral (real-DFT) form of the covariance x forward-operator product  AK = A_s K_sj  on a regular grid.

SURVEY.md section 8(f) row f2 ("structure-exploiting assembly: same results, fewer flops").  On the grid of
`calcGridPoints3D` (kernels.py:27-42) every block K_sj of `create_cov` (kernels.py:158-195) is a symmetric
three-level Toeplitz matrix: K(p,q) = k(|dy|,|dx|,|dz|).  Embedded in a symmetric three-level circulant of size
(2ny, 2nx, 2nz) it is diagonalised by the Kronecker product of the REAL transforms

    G_a  (P x n, P = 2n):   rows  sqrt(w_o) cos(2 pi o z / P), o = 0..P/2   and   sqrt(2) sin(2 pi o z / P), o = 1..P/2-1

(w_o = 1 for o in {0, P/2}, else 2):   K = crop[ (Gy x Gx x Gz)^T diag(Lambda / PyPxPz) (Gy x Gx x Gz) ],
Lambda(oy,ox,oz) = sum_d k(d) prod_a c_a(d_a) cos(2 pi o_a d_a / P_a)  (c = 1 for d = 0, 2 otherwise) -- all real, because
k is even in every coordinate.  One row of A_s (a ny x nx x nz volume) therefore costs three small-k GEMM passes forward
and three per property block backward (cropping on the way back) instead of an N x N contraction:
2.25e15 -> ~1.2e13 flop at 64^3.  Every pass is a batch of MFMA GEMMs against a fixed cosine/sine matrix
(`geobo_gemm_batched`); no FFT library, no complex arithmetic.

Numerics: the transform matrices are orthogonal up to scaling, so the result differs from the dense path by a few
1e-16 of max|A| max|K| per entry (normwise); the posterior cubes stay far inside the 1e-8 contract (tests).
"""
import math
import os

import numpy as np
import torch

from . import hip, plan
from .plan import INTEGER_BASIS_N, half_integer  # noqa: F401  (the basis of an extent is the planner's table; re-exported here)

F64 = hip.F64
SLACK = 4096  # doubles of slack behind every buffer: compute tiles may overhang the valid region (reads only)


def base_modes(n):
    """Base rows b = 0 .. n-1 of the real eigenvector basis of symmetric circulants of size P = 2n, as (kind, omega).  Every base row
    g_b comes with its MIRROR row (-1)^i g_b, which is the eigenvector of frequency n - omega (cos) / minus that eigenvector (sin); for
    the middle frequency n/2 the pair is (c + s, c - s) instead of (c, s) -- any rotation inside an eigenspace is as good a basis.
    Spectral position 2b holds base row b, position 2b+1 its mirror: the two rows differ only in the sign of the odd inputs, which is
    what the radix-2 (folded) transform kernels exploit -- per pair ONE even-input and ONE odd-input partial sum, outputs E + O and
    E - O (half the multiply-adds of the plain matrix product).

    ORDER (round 5): base rows come in groups of four, one per frequency omega = 0 .. n/4 - 1,
        b = 4 omega + (0: cos omega, 1: sin omega, 2: cos(n/2 - omega), 3: sin(n/2 - omega)),     omega >= 1
        b = 0 .. 3: cos 0, the middle pair (n/2), cos(n/4), sin(n/4)
    so that the eight spectral positions 8 omega .. 8 omega + 7 hold the frequencies omega, n - omega, n/2 - omega, n/2 + omega: the
    orbit of omega under a shift by a QUARTER period.  On the inputs i = 4j + rho of one residue class the rows of frequency
    n/2 -+ omega are +-(cos | sin) of frequency omega, so a transform needs only the cos / sin rows of omega < n/4 per class
    (RADIX 4: a quarter of the multiply-adds of the plain product; xz2d_fold.hip uses it for the synthesis along z).  The radix-2
    kernels see a pair-interleaved basis as before."""
    assert n % 4 == 0
    q = n // 4
    modes = [("cos", 0), ("mid", n // 2), ("cos", q), ("sin", q)]
    for om in range(1, q):
        modes += [("cos", om), ("sin", om), ("cos", n // 2 - om), ("sin", n // 2 - om)]
    return modes


def half_modes(n):
    """Base rows of the half-integer basis as (kind, 2 kappa): orbit omega = 0 .. n/4 - 1 (kappa = omega + 1/2) holds the base rows
    4 omega + (0: cos kappa, 1: sin kappa, 2: cos(n/2 + kappa), 3: sin(n/2 + kappa)); their mirrors (-1)^i g_b are the eigenvectors of
    n - kappa and n/2 - kappa: spectral positions 8 omega .. 8 omega + 7 = cos k, cos(n - k), sin k, -sin(n - k), cos(n/2 + k),
    cos(n/2 - k), sin(n/2 + k), -sin(n/2 - k)."""
    assert n % 4 == 0
    modes = []
    for om in range(n // 4):
        k2 = 2 * om + 1
        modes += [("cos", k2), ("sin", k2), ("cos", n + k2), ("sin", n + k2)]
    return modes


def _base_row(kind, om, n):
    P = 2 * n
    z = np.arange(n)
    ang = 2.0 * np.pi * ((om * z) % P) / P                        # exact integer phase index
    if kind == "cos":
        return (1.0 if om == 0 else math.sqrt(2.0)) * np.cos(ang)
    if kind == "sin":
        return math.sqrt(2.0) * np.sin(ang)
    return np.array([1.0, 1.0, -1.0, -1.0])[z % 4]                # cos(pi z / 2) + sin(pi z / 2), exactly


def _half_row(kind, k2, n):
    """sqrt(2) cos / sin(2 pi kappa z / P), kappa = k2 / 2, with the phase reduced in integers (index over 2P)."""
    P = 2 * n
    ang = 2.0 * np.pi * ((k2 * np.arange(n)) % (2 * P)) / (2 * P)
    return math.sqrt(2.0) * (np.cos(ang) if kind == "cos" else np.sin(ang))


def forward_matrix(n):
    """G (P x n): real eigenvector basis of symmetric circulants (integer basis) / skew-circulants (half-integer basis) of size P = 2n,
    restricted to the first n inputs, pair-interleaved: row 2b = base row b (base_modes / half_modes), row 2b+1 = (-1)^z times it."""
    assert n % 4 == 0
    G = np.empty((2 * n, n))
    alt = 1.0 - 2.0 * (np.arange(n) % 2)
    if half_integer(n):
        for b, (kind, k2) in enumerate(half_modes(n)):
            G[2 * b] = _half_row(kind, k2, n)
            G[2 * b + 1] = alt * G[2 * b]
        return G
    for b, (kind, om) in enumerate(base_modes(n)):
        G[2 * b] = _base_row(kind, om, n)
        G[2 * b + 1] = alt * G[2 * b]
    return G


def eigen_matrix(n):
    """E (P x n): Lambda' = E k for a half table k(d), d = 0..n-1, laid out on the same row index as G: row 2b carries the
    eigenvalue of the frequency of base row b, row 2b+1 that of its mirror n - frequency."""
    P = 2 * n
    d = np.arange(n)
    if half_integer(n):
        f2 = np.empty(P, dtype=np.int64)                          # twice the frequency
        for b, (kind, k2) in enumerate(half_modes(n)):
            f2[2 * b], f2[2 * b + 1] = k2, 2 * n - k2
        E = np.cos(2.0 * np.pi * ((f2[:, None] * d[None, :]) % (2 * P)) / (2 * P))
        E[:, 1:] *= 2.0
        return E
    om = np.empty(P, dtype=np.int64)
    for b, (kind, w) in enumerate(base_modes(n)):
        om[2 * b], om[2 * b + 1] = w, n - w
    E = np.cos(2.0 * np.pi * ((om[:, None] * d[None, :]) % P) / P)
    E[:, 1:] *= 2.0
    return E


def folded_matrices(n):
    """(Fe, Fo), each n x n/2: even / odd input columns of the base rows, Fe[b][j] = g_b[2j], Fo[b][j] = g_b[2j+1].
    forward:  out[2b] = E_b + O_b, out[2b+1] = E_b - O_b  with  E_b = sum_j Fe[b][j] x[2j], O_b = sum_j Fo[b][j] x[2j+1];
    inverse:  x[2j] = sum_b Fe[b][j] (s[2b] + s[2b+1]),   x[2j+1] = sum_b Fo[b][j] (s[2b] - s[2b+1])."""
    G = forward_matrix(n)
    return G[0::2, 0::2].copy(), G[0::2, 1::2].copy()


def _pad_rows(M, mult=128):
    r = (M.shape[0] + mult - 1) // mult * mult + mult      # one extra tile of zero rows: row-offset views may overhang
    out = np.zeros((r, M.shape[1]))
    out[:M.shape[0]] = M
    return out


def _buf(n, device):
    return torch.empty(int(n) + SLACK, dtype=F64, device=device)


class LatticeRows:
    """Operator rows of a lattice survey that are never materialised: plane y of row r is a window of the stencil table Q
    (hip.a_sens_lattice_stencil) at row_off[r] + y * q_plane, the two boundary planes come from `edge` ([rows][2][nx*nz]).
    forward_zx feeds the radix-2 forward kernel from this directly (geobo_xz2d_fold_lattice)."""

    def __init__(self, Q, row_off, q_plane, edge, r0=0, jy=None, jx=None):
        self.Q, self.row_off, self.q_plane, self.edge, self.r0 = Q, row_off, int(q_plane), edge, int(r0)
        self.jy, self.jx = jy, jx        # host copies of the survey plan's lattice indices per sensor (plane_pool)

    def rows(self, r0):
        return LatticeRows(self.Q, self.row_off, self.q_plane, self.edge, self.r0 + r0, self.jy, self.jx)


# ---- the distinct-plane pool of a lattice operator (pure index arithmetic: tests/test_plane_pool_cpu.py) ---------------------------------
# An interior plane y of row r sits at Q + row_off[r] + y q_plane with row_off[r] = ((ny-2-jy)(2nx-1) + (nx-1-jx)) nz: it depends on
# (d = y - jy + ny - 2, jx) only.  The pool holds the (x, z)-spectrum of every such plane ONCE, laid out [jx' = nx-1-jx][d][Cp], so that
# the ny planes of a row are contiguous: row r is the window at row_off'[r] = (jx' (2ny-3) + (ny-2-jy)) Cp.  (Planes 0 and ny - 1 of
# the window are not the row's -- those are its own boundary slabs -- and for jy = ny - 1 / jy = 0 they lie in front of / behind
# the block of jx': never read.)

def pool_row_off(nx, ny, Cp, jy, jx):
    """int64 window offsets row_off'[r] (doubles) into the interior pool [nx][2ny-3][Cp]."""
    jy, jx = np.asarray(jy, dtype=np.int64), np.asarray(jx, dtype=np.int64)
    return ((nx - 1 - jx) * (2 * ny - 3) + (ny - 2 - jy)) * int(Cp)


def pool_layout(nx, ny, Ms, Cp):
    """(interior planes, offset of the boundary pool, doubles between the boundary planes of consecutive rows, planes in all): the pool
    buffer is the interior pool [nx][2ny-3][Cp] followed by [Ms][2][Cp], row r's planes 0 and ny - 1 -- its own, whatever its window."""
    n_int = nx * (2 * ny - 3)
    return n_int, n_int * int(Cp), 2 * int(Cp), n_int + 2 * int(Ms)


def pool_plane_source(nx, ny, nz, p):
    """Offset (doubles) into the stencil table Q[2ny-3][2nx-1][nz] of the nx*nz window that pool plane p = jx' (2ny-3) + d transforms:
    what the pool's one forward launch reads with in_row = nz (rows = jx') and in_plane = (2nx-1) nz (planes = d)."""
    jxp, d = np.divmod(np.asarray(p, dtype=np.int64), 2 * ny - 3)
    return jxp * nz + d * ((2 * nx - 1) * nz)


def pool_order(jy, jx):
    """int32 permutation that sweeps a batch of rows by (jx, jy): rows of equal jx are consecutive with jy ascending -- neighbours are
    the same window shifted by one plane."""
    return np.lexsort((np.asarray(jy), np.asarray(jx))).astype(np.int32)


def pool_distinct_planes(ny, jy, jx):
    """Planes a batch of rows reads when every distinct one is read once: distinct interior (jx, d) + two boundary planes per row."""
    jy, jx = np.asarray(jy, dtype=np.int64), np.asarray(jx, dtype=np.int64)
    d = (ny - 2 - jy)[:, None] + np.arange(1, ny - 1, dtype=np.int64)[None, :]
    return int(np.unique(jx[:, None] * (2 * ny - 3) + d).size) + 2 * int(jy.size)


class PooledRows:
    """Operator rows of a lattice survey as windows of the pool of distinct plane SPECTRA (SpectralProduct.plane_pool): the y stage reads
    them in place (geobo_spectral_y_lattice), no forward transform per row.  pool: [nx][2ny-3][Cp] then the boundary planes [Ms][2][Cp]
    (`edge`, a view of the same buffer); row_off: int64 device offsets of the windows; jy / jx: host lattice indices (sweep order)."""

    def __init__(self, pool, row_off, edge, jy, jx, r0=0, geo=None, edge_row=None):
        self.pool, self.row_off, self.edge, self.jy, self.jx, self.r0 = pool, row_off, edge, jy, jx, int(r0)
        self.geo = geo if geo is not None else (jy.tobytes(), jx.tobytes())      # the survey's identity for the product's table cache
        self.edge_row = edge_row         # doubles between the boundary planes of consecutive rows (None: two planes, as plane_pool lays them out)

    def rows(self, r0):
        return PooledRows(self.pool, self.row_off, self.edge, self.jy, self.jx, self.r0 + r0, self.geo, self.edge_row)

    def interior(self, zero_planes):
        """The same rows restricted to their interior planes 1 .. ny-2 (A_i of DESIGN.md 2, "gravity block from half its rows"): every
        row reads zero_planes, two zero planes of the pool's stride, as its planes 0 and ny-1 (row stride 0)."""
        return PooledRows(self.pool, self.row_off, zero_planes, self.jy, self.jx, self.r0, self.geo, 0)


class ConvolvedRows:
    """Rows of L^-1 A of a lattice survey that are never materialised, for products whose Toeplitz axis is z (nx = ny = nz = 64): row r
    is the lattice convolution of Lview[r] (a sensor image, ny x nx) with the operator's stencil table, given by its eigen-data
    lam3[iz][ky][kx] (LatticeGram.transpose_tables3), boundary slabs iy = 0, ny - 1 apart in slab[r][k][iz][ix] (LatticeGram.
    edge_apply_transpose(..., zx=True)).  spectrum() hands the (y, x)-spectrum of every z channel to the y stage in ONE launch per batch
    (geobo_xz2d_fold_conv_fwd): the voxel-domain row is never written."""

    def __init__(self, gram, Lview, lam3, slab, r0=0):
        self.gram, self.Lview, self.lam3, self.slab, self.r0 = gram, Lview, lam3, slab, int(r0)

    def rows(self, r0):
        return ConvolvedRows(self.gram, self.Lview, self.lam3, self.slab, self.r0 + r0)

    def spectrum(self, sp, R, out_name):
        """[R][nz][Cp] planes (ky, kx) of the first R rows into sp's work buffer `out_name`."""
        nx, ny, nz, Px, Py, Cp = sp.nx, sp.ny, sp.nz, sp.Px, sp.Py, sp.Cp
        assert nx == ny == nz == 64 and Cp >= Py * Px
        a = self.r0
        lh = sp.buf("LG_Lh", R * Py * Px)
        self.gram._plane_yx(False, R, self.Lview[a:], self.Lview.stride(0), lh, Py * Px)
        t2 = sp.buf(out_name, R * nz * Cp)
        hip.xz2d_fold_conv_fwd(ny, R, nz, self.lam3, Py * Px, lh, Py * Px, self.slab[a:], self.slab.stride(0), sp.F["y"], sp.F["x"],
                               t2, nz * Cp, Cp)
        return t2


class SpectralProduct:
    """AK rows by the real-DFT route for one grid; holds the transform matrices and the work buffers."""

    def __init__(self, nx, ny, nz, device, rows_per_batch=None, plane_pad=0, opts=None, forms=None):
        if nx % 16 or ny % 16 or nz % 16:
            raise ValueError("spectral path needs grid extents that are multiples of 16")
        self.nx, self.ny, self.nz = nx, ny, nz
        # which kernel form carries each stage: decided ONCE by the planner (plan.stage_forms; the engine hands its route's record in); a
        # product built on its own (tests, tools) asks the planner, with the process environment unless `opts` (plan.switches) are given
        self.forms = f = forms or plan.stage_forms(nx, ny, nz, plan.switches(os.environ) if opts is None else opts)
        self.Px, self.Py, self.Pz = 2 * nx, 2 * ny, 2 * nz
        self.N, self.P3 = nx * ny * nz, self.Px * self.Py * self.Pz
        self.device = device
        dev = lambda a: hip.to_dev(a, device)
        axes = {"x": nx, "y": ny, "z": nz}
        self.G = {a: dev(_pad_rows(forward_matrix(n))) for a, n in axes.items()}
        self.GT = {a: dev(_pad_rows(forward_matrix(n).T.copy())) for a, n in axes.items()}
        self.E = {a: dev(_pad_rows(eigen_matrix(n))) for a, n in axes.items()}
        # folded (radix-2) matrices [n][n/2][(Fe, Fo)] of the axes whose stages run on the radix-2 kernels
        self.F = {a: dev(np.stack(folded_matrices(axes[a]), axis=2)) for a in f.folded_axes()}
        # 32 x 32 planes, "pair": two consecutive y-planes stacked along x through the (64, 32) instance with diag(Mx, Mx) (_paired): the z step
        # is row-wise anyway, the x step spends half its MFMAs on the zero blocks (cheap next to two GEMM passes through HBM); "quad": FOUR
        # y-planes as one 64 x 64 plane of the radix-2 kernels with the folded matrices of diag(G32, G32): no zero blocks in z, folded in both axes
        if f.xz == "quad":
            fe, fo = folded_matrices(32)
            fq = np.zeros((64, 32, 2))
            fq[:32, :16, 0], fq[:32, :16, 1] = fe, fo
            fq[32:, 16:, 0], fq[32:, 16:, 1] = fe, fo
            self.Fq = dev(fq)
        self._pairs = {}
        # plane stride of the (x, z)-spectrum work buffers [row][y][Px*Pz].  Px*Pz is a power of two at 64^3 (16384 doubles =
        # 128 KiB); a bare copy with the y stage's access pattern (512-byte runs, one per plane) streams 3.95 TB/s at that stride and
        # 5.2 TB/s with 2 KiB of padding (tools/hbm_copy_runs.hip, profiles/r03_hbm_copy_runs.txt) -- but the kernels of this
        # pipeline do not move: toeplitz_y 1.514 / 1.506 ms, inverse transform 0.372 / 0.375 ms, forward 0.571 / 0.573 ms with / without
        # the padding (profiles/r03_spectral_plane_pad_ab.txt): they are held by the fp64 VALU / the matrix pipe at the clock a
        # memory-bound launch runs at, not by channel aliasing.  The stride stays a parameter (`plane_pad`, doubles; the A/B switch
        # of round 3 is retired); default dense.  Fused kernels with the in-kernel y stage only (explicit strides); elsewhere Cp = Px*Pz.
        C, pad = self.Px * self.Pz, int(plane_pad)
        self.Cp = C + pad if (self.fused_xz and self.dense_y and C % 2048 == 0 and pad > 0) else C
        if rows_per_batch is None:
            per_row = (ny * self.Cp if self.dense_y else self.P3) * 8
            # ~3 GB per work buffer; ny = 128 (67 MB of spectrum per row): 48 rows.  Measured on the 128^3 rank step with the round-4 y
            # stage (several output chunks per staged row), A K -> AkA + posterior: 16 rows 1.69 + 2.94 s, 24: 1.62 + 2.92, 32: 1.58 + 2.82,
            # 48: 1.55 + 2.78, 64: 1.58 + 2.77, 96: 1.53 + 2.76, 128: 1.50 + 2.75 (flat from 48; 108 / 117 / 127 / 146 GB peak)
            cap = 3 << 30
            rows_per_batch = max(1, min(256 if self.dense_y else 128, cap // per_row))
        g = 128 // math.gcd(nx * ny, 128)
        self.R = max(g, rows_per_batch // g * g)
        self._bufs = {}
        self._pool_tabs = {}         # index tables of the pooled feed per survey geometry (constants of the survey, unlike the pool)
        self.kernel_timer = None     # callable(name, algorithmic_bytes, fn) -> fn(): the engine's HIP-event bracket for single kernels

    # lattice surveys: feed the A K y stage from the pool of distinct operator-plane spectra (plane_pool).  A plain attribute for A/B
    # runs and tests; results are bit-identical either way
    pooled_feed = True

    def pool_applies(self):
        """The pooled feed exists for one-term products on the in-kernel spectral y stage of ny <= 64 with the lattice forward kernel."""
        return bool(self.pooled_feed and self.forms.lattice_feed and self.forms.y == "mfma" and self.ny in (32, 48, 64))

    def pool_planes(self, Ms):
        """Planes the pool of an Ms-sensor operator holds (= forward transforms of plane_pool)."""
        return pool_layout(self.nx, self.ny, Ms, self.Cp)[3]

    def plane_pool(self, lattice, Ms, jy, jx):
        """(x, z)-spectra of every distinct plane of a lattice operator, each transformed once: the interior planes [nx][2ny-3][Cp] by ONE
        forward launch over the stencil table itself (row jx' = the window nz doubles further on, plane d = one table plane further: the
        windows overlap and are only read), the boundary slabs [Ms][2][Cp] by a second one.  Built per operator and step into a work
        buffer of its own -- the table workspace is overwritten by the next operator, nothing here is kept across steps."""
        assert self.pool_applies()
        nx, ny, nz, Cp = self.nx, self.ny, self.nz, self.Cp
        nd = 2 * ny - 3
        n_int, edge_off, edge_row, planes = pool_layout(nx, ny, Ms, Cp)
        buf = self.buf("Pool", planes * Cp)
        hip.xz2d_fold(False, nx, nx, nd, lattice.Q, nz, lattice.q_plane, self.F["x"], self.F["z"], buf, nd * Cp, Cp)
        e0 = lattice.edge[lattice.r0:]
        edge = buf[edge_off:planes * Cp]
        hip.xz2d_fold(False, nx, Ms, 2, e0, lattice.edge.stride(0), nx * nz, self.F["x"], self.F["z"], edge, edge_row, Cp)
        # (jy / jx: the lattice indices of the rows the lattice view starts at, in the operator's own row order -- not assumed row-major)
        jy, jx = np.ascontiguousarray(jy, dtype=np.int64)[:Ms], np.ascontiguousarray(jx, dtype=np.int64)[:Ms]
        rows = PooledRows(buf, None, edge, jy, jx)
        key = (rows.geo, Cp)
        row_off = self._pool_tabs.get(key)
        if row_off is None:
            row_off = self._pool_tabs[key] = torch.from_numpy(pool_row_off(nx, ny, Cp, jy, jx)).to(self.device)
        rows.row_off = row_off
        return rows

    def slab_spectra(self, A, Ms):
        """[Ms][2][Cp] (x, z)-spectra of the planes 0 and ny-1 of the first Ms rows of a resident operator: what plane_pool keeps behind
        the interior pool for an implicit one (the same forward launch on the same planes)."""
        nx, ny, nz, Cp = self.nx, self.ny, self.nz, self.Cp
        assert self.forms.xz == "fold" and A.stride(1) == 1
        spec = self.buf("SlabSpec", Ms * 2 * Cp)
        hip.xz2d_fold(False, nx, Ms, 2, A, A.stride(0), (ny - 1) * nx * nz, self.F["x"], self.F["z"], spec, 2 * Cp, Cp)
        return spec

    def slab_pair_rows(self, edge_spec, Ms, gen, out):
        """out[r, k nx nz:(k+1) nx nz] = plane (0, ny-1)[k] of (A_s K)[r] for r < Ms, A_s the rows of an operator restricted to their two
        boundary planes, given by those planes' spectra edge_spec [Ms][2][Cp] (PooledRows.edge, slab_spectra), K the block with
        generators gen: the 2 x 2 y stage (geobo_slab_pair_y), then the storing inverse transform of those 2 Ms planes.  (The other
        planes of A_s K are not computed: AkA's slab-slab term reads these two only.)"""
        nx, ny, nz, C, Cp = self.nx, self.ny, self.nz, self.Px * self.Pz, self.Cp
        assert self.forms.xz == "fold" and out.stride(1) == 1 and out.shape[1] >= 2 * nx * nz
        spec = self.buf("S", Ms * 2 * Cp)
        hip.slab_pair_y(ny, C, Ms, edge_spec, gen, spec, plane=Cp)
        hip.xz2d_fold(True, nx, Ms, 2, spec, 2 * Cp, Cp, self.F["x"], self.F["z"], out, out.stride(0), nx * nz)
        return out

    def _pool_batch(self, A, R):
        """(device int32 sweep order, distinct planes) of the first R rows of a pooled operator (constants of the survey: kept)."""
        a = A.r0
        key = (A.geo, a, R)
        hit = self._pool_tabs.get(key)
        if hit is None:
            jy, jx = A.jy[a:a + R], A.jx[a:a + R]
            hit = self._pool_tabs[key] = (torch.from_numpy(pool_order(jy, jx)).to(self.device), pool_distinct_planes(self.ny, jy, jx))
        return hit

    def _ystage_pooled(self, A, R, tabs, outs, y0, y1):
        """The y stage of the first R rows of a pooled operator, in place from the pool.  Algorithmic bytes for the per-kernel
        roofline: every distinct plane of the batch once + the output slabs."""
        ny, C, Cp = self.ny, self.Px * self.Pz, self.Cp
        order, distinct = self._pool_batch(A, R)
        a = A.r0
        er = 2 * Cp if A.edge_row is None else A.edge_row
        fn = lambda: hip.spectral_y_lattice(ny, C, R, A.pool, A.row_off[a:], A.edge[a * er:], er, order, tabs, outs, y0, y1, plane=Cp)
        name = "kernel:toeplitz_y" if len(tabs) >= 2 else "kernel:toeplitz_y_single"
        return self._launch(name, 8.0 * C * (distinct + R * len(tabs) * (y1 - y0)), R, self.y_stage_flop(1, len(tabs), y1 - y0), fn)

    # y per (x, z) mode inside one kernel (geobo_toeplitz_y), not by passes like x and z; there on the matrix pipe (round 6: geobo_spectral_y, same sums to rounding)
    dense_y = property(lambda self: self.forms.y != "spectrum")
    y_mfma = property(lambda self: self.forms.y == "mfma")
    fused_xz = property(lambda self: self.forms.xz in ("fold", "fused"))     # x and z of one whole plane inside one kernel (radix-2 or plain)

    def _ystage(self, R, src, tabs, outs, y0, y1, accumulate=False):
        """geobo_toeplitz_y launch, bracketed for the bench's per-kernel roofline when a timer is set: algorithmic bytes = the rows'
        (x, z)-spectrum read once + one output slab per property block (read as well when the launch accumulates)."""
        ny, C, plane = self.ny, self.Px * self.Pz, self.Cp
        # (the long-axis matrix-pipe kernel computes every output of a row whatever the slab; the windowed direct kernel only the chunks of
        # 16 that cover it: narrow slabs -- the y-slab shards of the column form -- stay with the direct kernel: 0.55 against 1.33 ms for 16
        # of 128 planes)
        if self.y_mfma and (ny > 64 or not accumulate) and (ny <= 64 or 2 * (y1 - y0) >= ny):
            fn = lambda: hip.spectral_y(ny, C, R, src, tabs, outs, y0, y1, plane=plane, accumulate=accumulate)
        else:
            fn = lambda: hip.toeplitz_y(ny, C, R, src, tabs, outs, y0, y1, plane=plane, accumulate=accumulate)
        # (one name per kernel symbol: single-block launches run toeplitz_y_kernel<ny, 2>, the others <ny, 1>)
        name = "kernel:toeplitz_y" if len(tabs) >= 2 or ny > 64 else "kernel:toeplitz_y_single"
        return self._launch(name, 8.0 * R * C * (ny + (2 if accumulate else 1) * len(tabs) * (y1 - y0)), R, self.y_stage_flop(1, len(tabs), y1 - y0), fn)

    def _launch(self, name, nbytes, rows, flop, fn):
        """fn(), bracketed by the engine's per-kernel timer when one is set; flop: (executed, its vector-pipe part) per row."""
        if self.kernel_timer is None:
            return fn()
        return self.kernel_timer(name, nbytes, fn, valu=rows * flop[1], flop=rows * flop[0])

    def _join(self, specs, gens, R, ylo, yhi, y2s=None, squaring=False):
        """The y stage of R rows for one group of property blocks: THE place that picks its kernel, timer name, bytes and flop.
        specs: one (x, z)-spectrum per term (work buffers of forward_zx; the PooledRows themselves where the rows' spectra are windows of
        the pool); gens[t][i]: generator of term t for block i of the group; y2s: the (D0, X, D1) tables of y2s_tables() when this group is
        their pair; squaring: the outputs feed the squaring inverse transform.  Returns (outs, outs2): one spectrum per block over the
        slab [ylo, yhi) in S / S1 / S2, and the second term's spectra in Sb / S1b where the terms do not meet here (y_two_term
        "separate", the odd last block of "y2t") -- [] where there are none, None where a block pair met in ONE pass."""
        ny, C, Cp, meet = self.ny, self.Px * self.Pz, self.Cp, self.forms.y_two_term
        nb = len(gens[0])
        outs = [self.buf(("S", "S1", "S2")[i], R * (yhi - ylo) * Cp) for i in range(nb)]
        if isinstance(specs[0], PooledRows):
            for i in range(0, nb, 2):       # (two blocks + one, each its own launch with its own bytes: what geobo_spectral_y3 does inside one call)
                self._ystage_pooled(specs[0], R, gens[0][i:i + 2], outs[i:i + 2], ylo, yhi)
            return outs, []
        if len(specs) == 1:
            self._ystage(R, specs[0], gens[0], outs, ylo, yhi)
            return outs, []
        assert (ylo, yhi) == (0, ny)
        (sg, sm), (gg, gm) = specs, gens
        # inherited, unmeasured: the squaring inverse is fed by two accumulating launches where the storing one takes geobo_spectral_y3t
        y3t = self.forms.y3t and not squaring
        if meet == "y2t" and nb == 2:
            # both terms in ONE pass: with the shared cross block three products per mode (geobo_toeplitz_y2s), otherwise four
            if y2s is not None:
                y2s_fn = hip.spectral_y2s if self.y_mfma else hip.toeplitz_y2s
                name, fn = "kernel:toeplitz_y2s", lambda: y2s_fn(ny, C, R, sg, sm, y2s[0], y2s[1], y2s[2], outs, plane=Cp)
            else:
                name, fn = "kernel:toeplitz_y2t", lambda: hip.toeplitz_y2t(ny, C, R, sg, sm, gg, gm, outs, plane=Cp)
            self._launch(name, 8.0 * R * C * 4 * ny, R, self.y_stage_flop(2, 2, shared=y2s is not None), fn)
            return outs, None
        if meet == "add" and y3t:
            # the terms meet in the y spectrum: 2 + nb transforms instead of 2 (1 + nb), no read-modify-write of the outputs
            fn = lambda: hip.spectral_y3t(ny, C, R, sg, sm, gg, gm, outs, plane=Cp)
            self._launch("kernel:toeplitz_y", 8.0 * R * C * ny * (2 + nb), R, self.y_stage_flop(2, nb), fn)
            return outs, []
        self._ystage(R, sg, gg, outs, ylo, yhi)
        if meet == "add":                   # the second y stage adds into the first one's output: ONE inverse transform per block
            self._ystage(R, sm, gm, outs, ylo, yhi, accumulate=True)
            return outs, []
        outs2 = [self.buf(("Sb", "S1b")[i], R * ny * Cp) for i in range(nb)]
        self._ystage(R, sm, gm, outs2, ylo, yhi)
        return outs, outs2

    def _rows_spectrum(self, A, r0, R, out_name):
        """(x, z)-spectrum of the rows r0 .. r0 + R of an operand: tensor rows, LatticeRows, PooledRows (nothing to transform) or
        ConvolvedRows (the (y, x)-spectrum of every z channel: the product's Toeplitz axis is z)."""
        if isinstance(A, PooledRows):
            return A.rows(r0)
        if isinstance(A, ConvolvedRows):
            return A.rows(r0).spectrum(self, R, out_name)
        if isinstance(A, LatticeRows):
            return self.forward_zx(A.rows(r0), R, self.G, out_name=out_name)
        return self.forward_zx(A[r0:], R, self.G, src_row_stride=A.stride(0), out_name=out_name)

    def _drive(self, batches, terms, sink, ylo, yhi, y2s=None, squaring=False):
        """Every dense-y product: forward transform each term, join, sink.  batches: [(r0, R, nterms)]; terms: [(rows, index of their
        first row, generators)]; sink(r0, R, js, outs, outs2) takes the joined spectra of the blocks js.  A sweep of the spectra feeds
        2 blocks where a pair is joined in one pass or squared, otherwise 3."""
        P_c = len(terms[0][2])
        for r0, R, nt in batches:
            specs = [self._rows_spectrum(A, r0 - first, R, name) for (A, first, _), name in zip(terms[:nt], ("T2", "T2b"))]
            step = 2 if squaring or (nt == 2 and self.forms.y_two_term == "y2t") else 3
            for j in range(0, P_c, step):
                js = range(j, min(j + step, P_c))
                tabs = y2s[1:] if y2s is not None and y2s[0] == j else None
                sink(r0, R, js, *self._join(specs, [[g[jj] for jj in js] for _, _, g in terms[:nt]], R, ylo, yhi, tabs, squaring))

    def _store(self, slabs, ylo, yhi, gx=None):
        """Sink: the storing inverse transform into rows r0 .. of every slab's targets.  gx (gx_applies; one slab, the whole y axis):
        the inverse transform also emits the lattice Gram's x analysis of every interior plane into the one-batch buffer "GX", and
        gx.rows(jj, r0, R, GX) consumes it before the next block overwrites it; gx.store_all False: of A K only the two boundary planes
        of every row are written."""
        def sink(r0, R, js, outs, _):
            for i, jj in enumerate(js):
                if gx is None:
                    self.backward_xz(outs[i], R, ylo, yhi, [(ya, yb, o[jj][r0:], o[jj].stride(0)) for ya, yb, o in slabs])
                    continue
                nx, ny, nz, Cp, gp = self.nx, self.ny, self.nz, self.Cp, self.Px * self.nz
                o = slabs[0][2][jj]
                GX = self.gx_buffer()
                hip.xz2d_fold_inv_gx(nx, R, ny, outs[i], ny * Cp, Cp, self.F["x"], self.F["z"], o[r0:], o.stride(0), nx * nz, gx.store_all,
                                     GX, ny * gp, gp)
                gx.rows(jj, r0, R, GX)
        return sink

    def gx_applies(self):
        """The storing inverse transform can emit the lattice Gram's x analysis (geobo_xz2d_fold_inv_gx): the radix-4 kernels of 64 x 64
        planes behind the dense y stage, at least one interior plane."""
        return self.forms.xz == "fold" and self.dense_y and self.nx == 64 and self.nz == 64 and self.ny >= 3

    def gx_buffer(self):
        """GX[R][ny][Px][nz] of one batch.  The inverse transform never writes the two boundary planes of a row and the Gram's y step
        multiplies them by the zero columns of its matrix: they are zeroed once per allocation, so that they stay finite."""
        gp = self.Px * self.nz
        b = self.buf("GX", self.R * self.ny * gp)
        if getattr(self, "_gx_zeroed", None) != b.data_ptr():
            v = b[:self.R * self.ny * gp].view(self.R, self.ny, gp)
            v[:, 0] = 0.0
            v[:, self.ny - 1] = 0.0
            self._gx_zeroed = b.data_ptr()
        return b

    def buf(self, name, n):
        b = self._bufs.get(name)
        if b is None or b.numel() < n + SLACK:
            b = self._bufs[name] = _buf(n, self.device)
        return b

    def _paired(self, Mx, rows, cols):
        """diag(Mx, Mx) for the stacked-pair form of the fused kernel (Mx: the valid rows x cols of a padded matrix)."""
        key = (Mx.data_ptr(), rows, cols)
        m2 = self._pairs.get(key)
        if m2 is None:
            m2 = torch.zeros((2 * rows, 2 * cols), dtype=Mx.dtype, device=Mx.device)
            m2[:rows, :cols] = Mx[:rows, :cols]
            m2[rows:, cols:] = Mx[:rows, :cols]
            self._pairs[key] = m2
        return m2

    # ---- axis passes, z (contiguous) then x [then y]: [R][ny][nx][nz] -> [R][ny][Px][Pz] [-> [R][Py][Px][Pz]] -----------------
    def forward_zx(self, src, R, M, src_row_stride=None, out_name="T2"):
        """src: R volumes of ny*nx*nz doubles, `src_row_stride` doubles apart (default: contiguous)."""
        nx, ny, nz, Px, Pz, Cp = self.nx, self.ny, self.nz, self.Px, self.Pz, self.Cp
        xz, analysis = self.forms.xz, M is self.G      # (the radix-2 forms hold G in their folded matrices: the eigen-matrices E take the plain twins)
        lds = self.N if src_row_stride is None else int(src_row_stride)
        t2 = self.buf(out_name, R * ny * Cp)           # planes Cp >= Px*Pz doubles apart (padded: see __init__)
        if isinstance(src, LatticeRows):               # operator rows read from the survey's stencil table by the radix-2 forward kernel
            assert self.forms.lattice_feed and analysis
            hip.xz2d_fold_lattice(nx, R, ny, src.Q, src.row_off[src.r0:], src.q_plane, src.edge[src.r0:], src.edge.stride(0),
                                  self.F["x"], self.F["z"], t2, ny * Cp, Cp)
        elif xz == "fold" and analysis:                # radix-2 kernels: half the MFMAs (xz2d_fold.hip)
            hip.xz2d_fold(False, nx, R, ny, src, lds, nx * nz, self.F["x"], self.F["z"], t2, ny * Cp, Cp)
        elif xz in ("fold", "fused"):
            hip.xz2d(False, nx, nz, R, ny, src, lds, nx * nz, M["x"], M["z"], t2, ny * Cp, Cp)
        elif xz == "quad" and analysis:
            hip.xz2d_fold_quad(False, nx, R, ny // 4, src, lds, nx * nz, self.Fq, self.Fq, t2, ny * Cp, Cp)
        elif xz in ("quad", "pair"):
            hip.xz2d(False, 2 * nx, nz, R, ny // 2, src, lds, 2 * nx * nz, self._paired(M["x"], Px, nx), M["z"], t2, ny * Cp, 2 * Cp)
        else:
            # any other extent: two batched passes, radix-2 (geobo_gemm_fold: half the multiply-adds) against the pair-interleaved basis
            fold = self.forms.fold and analysis
            t1 = self.buf("T1", R * ny * nx * Pz)
            hip.axis_pass(fold, False, False, hip.pad_n(ny * nx), hip.pad_n(Pz), nz, src, nz, lds, M["z"], nz, 0, t1, Pz, ny * nx * Pz, ny * nx, Pz, R)
            if self.forms.x_axis4 and analysis and Pz % 16 == 0:
                hip.spectral_axis(False, nx, Pz, Pz, Pz, nx * Pz, Px * Pz, R * ny, t1, t2)
            else:
                hip.axis_pass(fold, True, False, hip.pad_n(Px), hip.pad_n(Pz), nx, M["x"], nx, 0, t1, Pz, nx * Pz, t2, Pz, Px * Pz, Px, Pz, R * ny)
        return t2

    def forward(self, src, R, M, out_name="T3", src_row_stride=None):
        ny, Px, Py, Pz = self.ny, self.Px, self.Py, self.Pz
        t2 = self.forward_zx(src, R, M, src_row_stride)
        t3 = self.buf(out_name, R * self.P3)
        hip.gemm_batched(True, hip.pad_n(Py), hip.pad_n(Px * Pz), ny, M["y"], ny, 0, t2, Px * Pz, ny * Px * Pz, t3, Px * Pz,
                         self.P3, Py, Px * Pz, R)
        return t3

    # ---- back: y (crop to the slab [y0,y1)), x, z; writes rows of `out` (leading dimension ldo) -----------------------------
    def backward(self, spec, R, y0, y1, out, ldo):
        Px, Py, Pz = self.Px, self.Py, self.Pz
        slab = y1 - y0
        gyt = self.GT["y"][y0:]                                  # rows y0.. of G_y^T (padded rows behind are zero / slack)
        u2 = self.buf("U2", R * slab * Px * Pz)
        hip.gemm_batched(True, hip.pad_n(slab), hip.pad_n(Px * Pz), Py, gyt, Py, 0, spec, Px * Pz, self.P3, u2, Px * Pz,
                         slab * Px * Pz, slab, Px * Pz, R)
        self.backward_xz(u2, R, y0, y1, [(y0, y1, out, ldo)])

    def backward_xz(self, u2, R, ylo, yhi, targets):
        """u2: [R][yhi-ylo][Px][Pz] (y already in the space domain).  x pass over every (row, y), then one z pass per target
        (ya, yb, out, ldo): rows of `out` receive the y-slab [ya, yb) of every row."""
        nx, nz, Px, Pz, Cp = self.nx, self.nz, self.Px, self.Pz, self.Cp
        Ly, xz = yhi - ylo, self.forms.xz
        whole = lambda k: all((yb - ya) % k == 0 for ya, yb, _, _ in targets)      # every slab is a whole number of k-plane groups
        if xz == "fold":
            for ya, yb, out, ldo in targets:
                hip.xz2d_fold(True, nx, R, yb - ya, u2[(ya - ylo) * Cp:], Ly * Cp, Cp, self.F["x"], self.F["z"], out, ldo, nx * nz)
        elif xz == "fused":
            for ya, yb, out, ldo in targets:
                hip.xz2d(True, nx, nz, R, yb - ya, u2[(ya - ylo) * Cp:], Ly * Cp, Cp, self.GT["x"], self.GT["z"], out, ldo, nx * nz)
        elif xz == "quad" and whole(4):
            for ya, yb, out, ldo in targets:
                hip.xz2d_fold_quad(True, nx, R, (yb - ya) // 4, u2[(ya - ylo) * Cp:], Ly * Cp, Cp, self.Fq, self.Fq, out, ldo, nx * nz)
        elif xz in ("quad", "pair") and whole(2):
            for ya, yb, out, ldo in targets:
                hip.xz2d(True, 2 * nx, nz, R, (yb - ya) // 2, u2[(ya - ylo) * Cp:], Ly * Cp, 2 * Cp,
                         self._paired(self.GT["x"], nx, Px), self.GT["z"], out, ldo, 2 * nx * nz)
        else:
            fold = self.forms.fold
            u1 = self.buf("U1", R * Ly * nx * Pz)
            if self.forms.x_axis4 and Pz % 16 == 0:
                hip.spectral_axis(True, nx, Pz, Pz, Pz, Px * Pz, nx * Pz, R * Ly, u2, u1)
            else:
                hip.axis_pass(fold, True, True, hip.pad_n(nx), hip.pad_n(Pz), Px, self.GT["x"], Px, 0, u2, Pz, Px * Pz, u1, Pz, nx * Pz, nx, Pz, R * Ly)
            for ya, yb, out, ldo in targets:
                slab = yb - ya
                hip.axis_pass(fold, False, True, hip.pad_n(slab * nx), hip.pad_n(nz), Pz, u1[(ya - ylo) * nx * Pz:], Pz, Ly * nx * Pz,
                              self.GT["z"], Pz, 0, out, nz, ldo, slab * nx, nz, R)

    def flops(self, rows, nblocks, slab, fwd_planes=None):
        """Executed flop of product(): forward passes once, the rest per property block (compute extents).  fwd_planes: planes the
        forward transform runs over when that is not rows * ny (the pooled feed transforms pool_planes(Ms) distinct ones)."""
        nx, ny, nz, Px, Py, Pz = self.nx, self.ny, self.nz, self.Px, self.Py, self.Pz
        pn = hip.pad_n
        fwd = 2.0 * (ny * nx * pn(Pz) * nz + ny * pn(Px) * pn(Pz) * nx)
        bwd = 2.0 * (slab * pn(nx) * pn(Pz) * Px + pn(slab * nx) * pn(nz) * Pz)
        xz = self.forms.xz
        if xz == "gemm" and self.forms.fold:
            fwd, bwd = 0.5 * fwd, 0.5 * bwd         # radix-2 batched passes (geobo_gemm_fold)
        elif xz == "quad":                          # four planes per 64-point radix-2 plane: folded, both axes over the zero blocks
            fwd = 0.25 * ny * (64.0 * 64 * 128 + 128.0 * 64 * 128)
            bwd = 0.25 * slab * (128.0 * 128 * 64 + 64.0 * 128 * 64)
        elif xz == "pair":                          # diag(Mx, Mx) on stacked plane pairs: the x steps run over the zero blocks too
            fwd += 2.0 * ny * Px * Pz * nx
            bwd += 2.0 * slab * nx * Pz * Px
        elif xz == "fold":
            # radix-2 / radix-4 kernels (xz2d_fold.hip): forward z step one even- and one odd-input sum per spectral pair (half the plain
            # multiply-adds), forward x step and both inverse steps one cos / sin row per frequency group and residue class (a quarter)
            fwd = 2.0 * ny * (0.5 * nx * pn(Pz) * nz + 0.25 * pn(Px) * pn(Pz) * nx)
            bwd = 0.25 * bwd
        if not self.dense_y:
            fwd += 2.0 * pn(Py) * Px * Pz * ny
            bwd += 2.0 * pn(slab) * Px * Pz * Py
        if fwd_planes is not None:
            fwd *= float(fwd_planes) / (rows * ny)
        return rows * (fwd + nblocks * bwd + (self.y_stage_flop(1, nblocks, slab)[0] if self.dense_y else 0.0))

    def y_stage_flop(self, terms, nblocks, slab=None, shared=False):
        """(executed flop, its vector-pipe part) of the y stage per row: `terms` input spectra, `nblocks` output blocks.
        Direct kernels (toeplitz.hip): ny multiply-adds per output, block and term on the vector pipe (ny <= 64: every output y is
        computed and the slab stored; ny > 64: chunks of 16 outputs covering the slab); `shared`: the two-term rows of a block pair
        whose cross blocks coincide cost three products instead of four.
        In-kernel spectral product (spectral_y.hip): ny^2 / 2 multiply-adds per transform and mode on the matrix pipe -- one analysis
        per term, one synthesis per block -- plus the orbit butterflies on the vector pipe: 16 additions per orbit and analysis,
        4 mul + 8 fma + 8 add per orbit and block (one term) or 8 add + 8 mul + 16 fma + 32 add per orbit for a block pair of two-term
        rows (ny / 4 orbits per mode)."""
        ny, C = self.ny, self.Px * self.Pz
        if self.y_mfma and (ny <= 64 or slab is None or 2 * slab >= ny):
            valu = C * ny * (4.0 * terms + (7.0 * nblocks if terms == 1 else 10.0 * nblocks))
            return C * 1.0 * ny * ny * (terms + nblocks) + valu, valu
        outs = ny if (ny <= 64 or slab is None) else (slab + 15) // 16 * 16
        nprod = terms * nblocks * (0.75 if shared and terms == 2 and nblocks == 2 else 1.0)
        f = 2.0 * ny * outs * C * nprod
        return f, f

    def flops_valu(self, rows, nblocks, slab=None):
        """The part of flops() executed on the fp64 VALU (the y stage's vector-pipe work); everything else is MFMA."""
        return rows * self.y_stage_flop(1, nblocks, slab)[1] if self.dense_y else 0.0

    def eigenvalues(self, table_mirrored, toeplitz_z=False):
        """What product() needs of one covariance block, from the (z-mirrored) lattice table of geobo_cov_table:
        dense-y route: the Toeplitz generators t[d][ox][oz] = (E_x E_z k)(d, ox, oz) / (Px Pz)   ([ny][Px*Pz]);
        otherwise the full eigenvalue cube Lambda'/(Py Px Pz) on the G row index.
        toeplitz_z (dense-y route, nx = ny = nz): the half table k(dy, dx, dz) is permuted to [dz][dy][dx] first -- generators
        t[dz][oy][ox] of a product whose Toeplitz axis is z and whose planes are (y, x) (ConvolvedRows).  The TABLE is permuted, no
        isotropy is assumed: unequal voxel sizes stay exact; the transform matrices of equal extents are identical."""
        nx, ny, nz = self.nx, self.ny, self.nz
        T = table_mirrored[:ny * nx * 2 * nz].view(ny, nx, 2 * nz)[:, :, nz - 1:2 * nz - 1].contiguous()
        if toeplitz_z:
            assert self.dense_y and nx == ny == nz
            T = T.permute(2, 0, 1).contiguous()
        src = self.buf("Tsrc", self.N)
        src[:self.N] = T.reshape(-1)
        if self.dense_y:
            C, Cp = self.Px * self.Pz, self.Cp            # (Cp: plane stride of what forward_zx wrote)
            gen = self.forward_zx(src, 1, self.E, out_name="Lam")[:ny * Cp].view(ny, Cp)[:, :C].clone().view(-1)   # own dense [ny][C] table (the work buffer is reused)
            gen.mul_(1.0 / float(C))
            return gen
        lam = self.forward(src, 1, self.E, out_name="Lam")[:self.P3].clone()
        lam.mul_(1.0 / float(self.P3))
        return lam

    def product(self, A, Ms, lam_list, outs, y0=0, y1=None, slabs=None, gx=None):
        """outs[j][r, :] = (A[r, :N] convolved with block j) restricted to y-slab [y0,y1), r < Ms.
        A: (>=Ms x N) row-major; outs[j]: 2-D views (rows x (y1-y0)*nx*nz).
        `slabs` = [(y0, y1, outs), ...] crops the SAME scaled spectrum to several y-slabs (one per destination rank of the
        row-sharded multi-GPU form); the forward passes and the scaling are done once.
        gx: the lattice Gram takes the rows' x analysis straight from the inverse transform (_store; gx_applies(), whole y axis)."""
        y1 = self.ny if y1 is None else y1
        if slabs is None:
            slabs = [(y0, y1, outs)]
        N = self.N
        if isinstance(A, PooledRows):
            assert self.pool_applies() and self.dense_y
        elif isinstance(A, LatticeRows):
            assert self.forms.lattice_feed
        else:
            assert A.stride(1) == 1 and A.stride(0) >= N and A.stride(0) % 2 == 0
        if gx is not None:
            assert self.gx_applies() and len(slabs) == 1 and (slabs[0][0], slabs[0][1]) == (0, self.ny)
        if self.dense_y:
            return self._product_dense_y(A, Ms, lam_list, slabs, gx)
        for r0 in range(0, Ms, self.R):
            R = min(self.R, Ms - r0)
            spec = self.forward(A[r0:], R, self.G, src_row_stride=A.stride(0))
            n = R * self.P3
            j = 0
            while j < len(lam_list):
                if j + 1 < len(lam_list):      # two property blocks per read of the spectrum
                    s0, s1 = self.buf("S", n), self.buf("S1", n)
                    hip.scale_broadcast2(spec[:n], lam_list[j], lam_list[j + 1], s0[:n], s1[:n])
                    for ya, yb, o in slabs:
                        self.backward(s0, R, ya, yb, o[j][r0:], o[j].stride(0))
                        self.backward(s1, R, ya, yb, o[j + 1][r0:], o[j + 1].stride(0))
                    j += 2
                else:
                    s0 = self.buf("S", n)
                    hip.scale_broadcast(spec[:n], lam_list[j], s0[:n])
                    for ya, yb, o in slabs:
                        self.backward(s0, R, ya, yb, o[j][r0:], o[j].stride(0))
                    j += 1

    def _product_dense_y(self, A, Ms, gens, slabs, gx=None):
        """z and x through the spectrum, y as Toeplitz blocks: one read of the (x, z)-spectrum per three property blocks."""
        ylo, yhi = min(s[0] for s in slabs), max(s[1] for s in slabs)
        batches = [(r0, min(self.R, Ms - r0), 1) for r0 in range(0, Ms, self.R)]
        self._drive(batches, [(A, 0, gens)], self._store(slabs, ylo, yhi, gx), ylo, yhi)

    # ---- posterior variance in the transposed order (engine._posterior_zpath) ------------------------------------------------------
    def fused_ss(self):
        """True where the inverse transform itself squares and sums its output planes (geobo_xz2d_fold_inv_ss: the radix-2 kernels of
        nx = nz = 64 with the Toeplitz y stage); elsewhere reduce_ss stores a batch of V rows and geobo_sumsq_accum reduces it."""
        return self.forms.ss == "fused"

    GENERIC_SS_SLOTS = 8

    def ss_slots(self):
        """Partial cubes per property block that reduce_ss adds to (sum over them afterwards)."""
        return hip.xz2d_fold_inv_ss_slots(self.nx, self.R, self.ny) if self.fused_ss() else self.GENERIC_SS_SLOTS

    def y2s_tables(self, gens_g, gens_m, pair=(0, 1), check=True):
        """Tables of the three-product form of the two-term rows for the block pair (a, b) = `pair` (b = a + 1, a even), or None where
        the kernel does not apply.  The caller states that gens_g[b] and gens_m[a] are the SAME covariance block -- K_01 = K_10:
        create_cov's prior is symmetric (kernels.py:181-195) -- and the statement is verified on the device: `sym_residual`
        (max |gens_g[b] - gens_m[a]| over max |gens_g[b]|, a 0-d device tensor) is left for the caller to read at its next
        synchronisation (engine.posterior raises above 1e-12).  Returns (a, D0 = gens_g[a] - X, X = gens_g[b], D1 = gens_m[b] - X).
        check=False: tables only, for a second reader of blocks this step has already verified; `sym_residual` is left as it is."""
        a, b = pair
        applies = self.forms.y2s and b == a + 1 and a % 2 == 0 and b < len(gens_g)
        if not check:
            return (a, gens_g[a] - gens_g[b], gens_g[b], gens_m[b] - gens_g[b]) if applies else None
        self.sym_residual = None
        if not applies:
            return None
        x = gens_g[b]
        # (cross weight 0 -- gp_coeff = [.., .., 0], a legal prior -- makes both cross blocks exactly zero: 0 / 0 must not read as
        # "asymmetric", so the residual is the difference against a denominator that is never zero)
        den = torch.maximum(x.abs().max(), gens_m[a].abs().max())
        self.sym_residual = (x - gens_m[a]).abs().max() / den.clamp_min(torch.finfo(x.dtype).tiny)
        return (a, gens_g[a] - x, x, gens_m[b] - x)

    def reduce_ss(self, Zg, Mg, gens_g, Zm, m_first, gens_m, ss, y2s=None):
        """ss[j][slot][y][x*z] += sum_m V_j[m]^2  with  V_j[m] = Zg[m] * K_0j  (+ Zm[m - m_first] * K_1j for m >= m_first),  m < Mg:
        rows of L^-1 A_s carried through the covariance product and squared on the way out of the inverse transform -- V is never
        written.  Zg: (>= Mg x N) rows, Zm: (>= Mg - m_first x N) rows or None; gens_g[j] / gens_m[j]: Toeplitz generators of the
        blocks (0, j) / (1, j) (eigenvalues()); ss[j]: zeroed partial cubes (ss_slots() slots each).
        Batches never straddle m_first (a batch is entirely one-term or entirely two-term).  Grids without the fused reduction
        (fused_ss): the storing product of every batch into a scratch of R rows, then geobo_sumsq_accum.
        y2s: tables of y2s_tables() for a pair of blocks whose cross blocks coincide -- the two-term rows of that pair then cost three
        y-stage products instead of four (geobo_toeplitz_y2s)."""
        nx, ny, N, Cp, R = self.nx, self.ny, self.N, self.Cp, self.R
        P_c = len(gens_g)
        if Zm is None:
            m_first = Mg
        one = min(m_first, Mg)
        batches = [(r0, min(R, one - r0), 1) for r0 in range(0, one, R)] + [(r0, min(R, Mg - r0), 2) for r0 in range(m_first, Mg, R)]
        if self.fused_ss():
            def square(r0, Rb, js, outs, outs2):
                for i, jj in enumerate(js):
                    # (a pair joined in one pass -- outs2 None -- leaves the second input's row stride at its default; every other launch
                    # states it, second input or not: the kernel reads it beside src2 only, the launch arguments stay what they were)
                    second = {} if outs2 is None else dict(src2=outs2[i] if outs2 else None, in2_row=ny * Cp, r2_first=0)
                    hip.xz2d_fold_inv_ss(nx, Rb, ny, outs[i], ny * Cp, Cp, self.F["x"], self.F["z"], ss[jj], **second)
            return self._drive(batches, [(Zg, 0, gens_g), (Zm, m_first, gens_m)], square, 0, ny, y2s=y2s, squaring=True)
        # The stored reduction joins the terms of a row only where the second accumulates into the first ("add").  "separate" has no
        # join; "y2t" HAS one (product_two_term uses it on the same grids, 32 x 32 x 32 for one) and still runs two storing products
        # here: inherited and unmeasured -- joining them is a performance change that wants its own measurement.
        stored_join = self.dense_y and self.forms.y_two_term == "add"
        for r0, Rb, nt in batches:
            vg = [self.buf("SSV%d" % jj, R * N)[:R * N].view(R, N) for jj in range(P_c)]
            vm = None
            if nt == 2 and stored_join:
                self._drive([(0, Rb, 2)], [(Zg[r0:], 0, gens_g), (Zm[r0 - m_first:], 0, gens_m)], self._store([(0, ny, vg)], 0, ny), 0, ny)
            else:
                self.product(Zg[r0:], Rb, gens_g, vg)
                if nt == 2:
                    vm = [self.buf("SSW%d" % jj, R * N)[:R * N].view(R, N) for jj in range(P_c)]
                    self.product(Zm[r0 - m_first:], Rb, gens_m, vm)
            for jj in range(P_c):
                hip.sumsq_accum(vg[jj], vm[jj] if vm else None, Rb, ss[jj].view(ss[jj].shape[0], -1))

    def has_two_term_product(self, nblocks):
        """Whether the y stage of this grid joins the two terms of a row for `nblocks` property blocks (product_two_term): the
        one-pass kernels take the blocks in pairs, the accumulating form takes any number."""
        meet = self.forms.y_two_term
        return self.dense_y and ((meet == "y2t" and nblocks % 2 == 0) or meet == "add")

    def product_two_term(self, Zg, Zm, rows, gens_g, gens_m, outs, y2s=None):
        """outs[j][r, :] = Zg[r] * K_0j + Zm[r] * K_1j for r < rows <= R: the storing counterpart of reduce_ss's two-term rows.  The
        terms meet in the y stage (one pass for a pair of blocks -- with y2s tables three products per mode --, or the second term
        accumulating into the first one's spectrum), ONE storing inverse transform per block.  Grids: has_two_term_product."""
        assert self.has_two_term_product(len(gens_g)) and rows <= self.R
        self._drive([(0, rows, 2)], [(Zg, 0, gens_g), (Zm, 0, gens_m)], self._store([(0, self.ny, outs)], 0, self.ny), 0, self.ny, y2s=y2s)

    def flops_ss(self, rows_one, rows_two, nblocks, shared=False):
        """Executed flop of reduce_ss: rows_one one-term rows, rows_two two-term rows (forward transform per term, y stage, one second
        inverse step per row; the first inverse step per term)."""
        nx, ny, nz, Px, Pz = self.nx, self.ny, self.nz, self.Px, self.Pz
        fwd = 1.0 * ny * (nx * nz * Pz + 0.5 * Px * nx * Pz)           # radix 2 along z (half the plain products), radix 4 along x (a quarter)
        inv1, inv2 = 0.5 * ny * Px * Pz * nz, 0.5 * ny * nx * Px * nz  # radix 4 both ways
        terms = rows_one + 2 * rows_two
        y = rows_one * self.y_stage_flop(1, nblocks)[0] + rows_two * self.y_stage_flop(2, nblocks, shared=shared)[0]
        return terms * (fwd + nblocks * inv1) + (rows_one + rows_two) * nblocks * inv2 + y

    def valu_ss(self, rows_one, rows_two, nblocks, shared=False):
        """The vector-pipe part of flops_ss (the y stage's share on the fp64 VALU)."""
        return rows_one * self.y_stage_flop(1, nblocks)[1] + rows_two * self.y_stage_flop(2, nblocks, shared=shared)[1]
