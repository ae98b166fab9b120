"""The fp64 GEMM core (gemm_f64.hip) under each of its four workgroup -> tile maps, against a reference that is exact by construction.

Operands are small random integers (|x| <= 15 for the products, <= 3 for the posterior reduction), alpha and beta come from
{+-1, +-0.5, 2}: every product, partial sum and result is an integer or a dyadic rational far below 2^53, so every summation order
gives the same value and the fp64 product computed with torch on the CPU is THE result.  Comparison is bit for bit over the whole
C buffer: the region a call may write must hold the reference, everything else (padding columns of ldc > n, rows >= m_valid, tiles
strictly above the diagonal under lower_only) the bits it held before.  Where beta = 0, C starts as a NaN with a payload, so a
read of C shows.  The only bit patterns identified are +0 and -0: an exact zero's sign depends on whether a -0 term met a +0
(alpha = -1 times an all-zero sum), i.e. on the order, not on the value.

Every case first asserts, through hip.gemm_map (the function launch() itself calls), that it runs under the map it is listed for.
One further test uses real-valued operands (i 2^-26) with an int64-exact reference and the a-priori dot-product bound: small
integers are exact in fp32 too and would not notice a path that narrows an operand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8_0000_0000_1234
F64 = torch.float64


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


def _ints(shape, amp, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-amp, amp + 1, shape, generator=g, dtype=torch.int64).to(F64)


def _bits(t):
    b = t.detach().cpu().contiguous().view(torch.int64)
    return torch.where(b == torch.iinfo(torch.int64).min, torch.zeros_like(b), b)          # -0 -> +0, nothing else


def _same_bits(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _nan_like(shape):
    t = torch.empty(shape, dtype=F64)
    t.view(torch.int64).fill_(NAN_BITS)
    return t


def _assert_exact(X, Y, k, alpha=1.0, beta=0.0, C=None):
    """The bound that makes every summation order exact: max|X| max|Y| k max(|alpha|, |beta|, 1) < 2^53, here with C's share added
    and two bits to spare for the quarters that alpha, beta = +-0.5 bring (every partial sum is a multiple of 0.25 below 2^53)."""
    c = 0.0 if C is None else float(C.abs().max())
    assert (float(X.abs().max()) * float(Y.abs().max()) * k + c) * max(abs(alpha), abs(beta), 1.0) < 2.0 ** 51


def _strided(t, lead_extra, r0, c0):
    """A copy of t on the device as a view with a larger leading dimension and a nonzero origin (r0, c0 keep 16-byte alignment)."""
    buf = torch.zeros((t.shape[0] + r0 + 1, t.shape[1] + c0 + lead_extra), dtype=F64, device="cuda")
    v = buf[r0:r0 + t.shape[0], c0:c0 + t.shape[1]]
    v.copy_(t)
    return v


def _written(m, n, tm, lower_only, m_valid):
    """Mask of the elements of the m x n result a call stores: rows below m_valid, tiles with col0 < row0 + TM under lower_only."""
    r = torch.arange(m).unsqueeze(1)
    c = torch.arange(n).unsqueeze(0)
    w = (r < (m_valid if m_valid > 0 else m)) & (c >= 0)
    if lower_only:
        w = w & ((c // 128) * 128 < (r // tm) * tm + tm)
    return w


def _check_map(hip, want, **kw):
    info = hip.gemm_map(**kw)
    assert info["map"] == want, (kw, info)
    return info


def _product_case(hip, entry, m, n, k, alpha, beta, want_map, seed, lower_only=False, small_tiles=False, x_lower=False, y_lower=False,
                  m_valid=0, views=False, poison=False):
    """One gemm_nt / gemm_nn call against the exact reference, whole C buffer compared bit for bit."""
    nn = entry == "gemm_nn"
    info = _check_map(hip, want_map, m=m, n=n, small_tiles=small_tiles, lower_only=lower_only, x_lower=x_lower, y_lower=y_lower,
                      entry=entry)
    tm = info["tm"]
    X = _ints((m, k), 15, seed)
    Y = _ints((k, n) if nn else (n, k), 15, seed + 1)
    if x_lower:
        X = torch.tril(X)
    if y_lower:
        Y = torch.tril(Y)
    if m_valid:
        X[m_valid:] = 0.0                                     # the contract of m_valid: zero padding rows
    r0, c0 = (2, 3) if views else (0, 0)
    C0 = _nan_like((m + r0 + 1, n + c0 + 5)) if beta == 0.0 else _ints((m + r0 + 1, n + c0 + 5), 15, seed + 2)
    _assert_exact(X, Y, k, alpha, beta, None if beta == 0.0 else C0)
    prod = alpha * (X @ Y if nn else X @ Y.t())
    if beta != 0.0:
        prod = prod + beta * C0[r0:r0 + m, c0:c0 + n]
    want = C0.clone()
    w = _written(m, n, tm, lower_only, m_valid)
    want[r0:r0 + m, c0:c0 + n] = torch.where(w, prod, C0[r0:r0 + m, c0:c0 + n])

    def run(Xh, Yh):
        Xd = _strided(Xh, 6, 1, 2) if views else Xh.cuda()
        Yd = _strided(Yh, 10, 3, 4) if views else Yh.cuda()
        Cd = C0.cuda()
        Cv = Cd[r0:r0 + m, c0:c0 + n]
        if nn:
            hip.gemm_nn(Xd, Yd, Cv, alpha=alpha, beta=beta, x_lower=x_lower, y_lower=y_lower)
        else:
            hip.gemm_nt(Xd, Yd, Cv, alpha=alpha, beta=beta, lower_only=lower_only, m_valid=m_valid, small_tiles=small_tiles)
        return Cd.cpu()

    got = run(X, Y)
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), "%d elements differ, first at %s" % (int(bad.sum()), bad.nonzero()[0].tolist())
    if poison:
        # NaN exactly where the header says the operand is not contracted: the same bits must come out
        Xp, Yp = X.clone(), Y.clone()
        if x_lower:           # X at columns >= the end of its row tile
            Xp[torch.arange(k).unsqueeze(0) >= ((torch.arange(m) // tm + 1) * tm).unsqueeze(1)] = float("nan")
        if y_lower:           # Y at rows before the first column of its column tile
            Yp[torch.arange(k).unsqueeze(1) < ((torch.arange(n) // 128) * 128).unsqueeze(0)] = float("nan")
        assert bool(torch.isnan(Xp).any() or torch.isnan(Yp).any())
        assert _same_bits(run(Xp, Yp), got)


AB = [(1.0, 0.0), (-1.0, 1.0), (2.0, -0.5)]       # store / start-C-in-the-accumulators / general read-modify-write

# (m, n, k, small_tiles, map): [9 x 3] grid rounds nbi up to 16; [5 x 9] ragged supertiles; [9 x 8] one-row last band, 72 items;
# 128-row tiles [9 x 8] and, forced, [10 x 8]
NT_SHAPES = [(2304, 384, 48, False, 1), (1280, 1152, 32, False, 2), (2304, 1024, 64, False, 3), (1152, 1024, 16, False, 3),
             (1280, 1024, 128, True, 3)]


@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("m,n,k,small,want_map", NT_SHAPES)
def test_gemm_nt_every_map(hip, m, n, k, small, want_map, alpha, beta):
    _product_case(hip, "gemm_nt", m, n, k, alpha, beta, want_map, seed=m + n + k, small_tiles=small)


@pytest.mark.parametrize("m,n,k,want_map,alpha,beta", [(2304, 384, 32, 1, 2.0, -0.5), (1280, 1152, 48, 2, -1.0, 1.0),
                                                       (2304, 1024, 16, 3, 1.0, 0.0)])
def test_gemm_nt_strided_views(hip, m, n, k, want_map, alpha, beta):
    """ldx, ldy, ldc larger than the extents, every operand at a nonzero origin of its buffer."""
    _product_case(hip, "gemm_nt", m, n, k, alpha, beta, want_map, seed=7 + m + n, views=True)


@pytest.mark.parametrize("m,n,k,want_map", [(2304, 384, 32, 1), (1280, 1152, 16, 2), (2304, 1024, 48, 3), (1152, 1024, 32, 3)])
@pytest.mark.parametrize("short,alpha,beta", [(30, -1.0, 1.0), (150, 1.0, 0.0), (150, 0.5, 2.0)])
def test_gemm_nt_m_valid(hip, m, n, k, want_map, short, alpha, beta):
    """m_valid inside the last 64-row group of the last row tile (m - 30) and inside an earlier group (m - 150: with 256-row tiles
    an earlier group of the last tile, with 128-row tiles a group of the tile before, the last tile being all padding)."""
    _product_case(hip, "gemm_nt", m, n, k, alpha, beta, want_map, seed=11 + m + short, m_valid=m - short)


# lower_only: a different combination of tile height, map and square / rectangular shape each
LOWER_SHAPES = [(2304, 2304, 32, 3), (2304, 1024, 48, 3), (1152, 1152, 64, 3), (2048, 896, 16, 1), (1024, 1024, 128, 0)]


@pytest.mark.parametrize("alpha,beta", [(-1.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("m,n,k,want_map", LOWER_SHAPES)
def test_gemm_nt_lower_only(hip, m, n, k, want_map, alpha, beta):
    """The trailing update's form: exactly the tiles with col0 < row0 + TM are written, every other bit of C stays."""
    _product_case(hip, "gemm_nt", m, n, k, alpha, beta, want_map, seed=13 + m + n, lower_only=True)


@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("chunks", [1, 4])
@pytest.mark.parametrize("lower_only,m_valid", [(False, 0), (True, 0), (False, 2100)])
def test_gemm_nt_splitk(hip, splits, chunks, lower_only, m_valid):
    """Map 3 with batch = splits (72 or 60 items per slice: 216 = a partial last group).  Skipped tiles and rows >= m_valid of C
    come out as zero, as the header documents; the padding columns of C stay."""
    m, n, k = 2304, 1024, 16 * splits * chunks
    info = _check_map(hip, 3, m=m, n=n, lower_only=lower_only, batch=splits, entry="gemm_nt_splitk")
    assert info["ntiles"] == (60 if lower_only else 72) and info["grid_y"] == 1
    X = _ints((m, k), 15, 17 * splits + chunks)
    Y = _ints((n, k), 15, 19 * splits + chunks)
    if m_valid:
        X[m_valid:] = 0.0
    _assert_exact(X, Y, k)
    C0 = _nan_like((m, n + 6))
    want = C0.clone()
    want[:, :n] = torch.where(_written(m, n, info["tm"], lower_only, m_valid), X @ Y.t(), torch.zeros((), dtype=F64))
    Cd = C0.cuda()
    ws = _nan_like((splits * m * n,)).cuda()
    hip.gemm_nt_splitk(X.cuda(), Y.cuda(), Cd[:, :n], splits, ws, lower_only=lower_only, m_valid=m_valid)
    bad = _bits(Cd) != _bits(want)
    assert not bool(bad.any()), "%d elements differ, first at %s" % (int(bad.sum()), bad.nonzero()[0].tolist())


# (m, n, k, x_lower, y_lower, map, alpha, beta): rows descending + peeled diagonal chunks of the 3-stage path; 128-row tiles [5 x 4];
# map 0; y_lower [2 x 8]; both flags = map 2's triangular branch with a storing epilogue
NN_CASES = [(1024, 512, 1024, True, False, 3, 1.0, 0.0), (640, 512, 640, True, False, 3, -0.5, 1.0),
            (384, 256, 384, True, False, 0, 2.0, -1.0), (512, 1024, 1024, False, True, 3, -1.0, 1.0),
            (1024, 1024, 1024, True, True, 2, 0.5, 0.0)]


@pytest.mark.parametrize("m,n,k,xl,yl,want_map,alpha,beta", NN_CASES)
def test_gemm_nn_triangular_operands(hip, m, n, k, xl, yl, want_map, alpha, beta):
    """x_lower / y_lower clip the contraction range; for the single-flag cases a second pass with the operand poisoned by NaN where
    the header says it is not contracted (X: columns >= the end of the row tile; Y: rows before the column tile's first column)."""
    _product_case(hip, "gemm_nn", m, n, k, alpha, beta, want_map, seed=23 + m + n, x_lower=xl, y_lower=yl, poison=xl != yl)


@pytest.mark.parametrize("m,small,want_map", [(1280, False, 0), (1152, False, 1), (1280, True, 1)])
def test_in_place_panel_solve(hip, m, small, want_map):
    """P <- P L_kk^-T as the Cholesky issues it (C == X, n = k = 128): every workgroup reads its rows of P over the whole
    contraction before it stores them.  Bit-equal to the out-of-place call and to the reference."""
    _check_map(hip, want_map, m=m, n=128, small_tiles=small)
    P = _ints((m, 128), 15, 29 + m)
    Li = torch.tril(_ints((128, 128), 15, 31 + m))
    _assert_exact(P, Li, 128)
    want = P @ Li.t()
    Pd, Ld = P.cuda(), Li.cuda()
    out = _nan_like((m, 128)).cuda()
    hip.gemm_nt(Pd, Ld, out, small_tiles=small)
    hip.gemm_nt(Pd, Ld, Pd, small_tiles=small)
    assert _same_bits(out, want) and _same_bits(Pd, want)


# (m, n): the second shape is the first at which a batch of 64 takes map 3 and a batch of 65 map 2 (nbi >= 4, nbj >= 8 and
# nbi nbj >= 64 need 128-row tiles here); m = 512 has nbi = 2 and stays on map 0 at either batch -- kept as the map-0 batched case
@pytest.mark.parametrize("m,n,batch,want_map", [(1152, 1024, 65, 2), (1152, 1024, 64, 3), (512, 1024, 65, 0), (512, 1024, 64, 0)])
def test_gemm_batched_shared_operands(hip, m, n, batch, want_map):
    """Shared operands (stride 0): every slice bit-equal to the batch-1 call (compared on the device), one against the CPU."""
    k = 16
    _check_map(hip, want_map, m=m, n=n, batch=batch, entry="gemm_batched_nt")
    X, Y = _ints((m, k), 15, 37 + m), _ints((n, k), 15, 41 + m)
    _assert_exact(X, Y, k)
    Xd, Yd = X.cuda(), Y.cuda()
    C = _nan_like((1, m, n)).cuda().expand(batch, m, n).contiguous()
    one = _nan_like((m, n)).cuda()
    hip.gemm_batched(False, m, n, k, Xd, k, 0, Yd, k, 0, C, n, m * n, m, n, batch)
    hip.gemm_batched(False, m, n, k, Xd, k, 0, Yd, k, 0, one, n, m * n, m, n, 1)
    assert bool((C.view(torch.int64) == one.view(torch.int64).unsqueeze(0)).all())
    assert _same_bits(C[batch - 28], X @ Y.t())


# (m, ncols, m_valid, map): [4 x 9]; [4 x 33] -> two 32-column groups per row tile; row_shift = 128 (first tile starts in front of
# the matrix); map 1
@pytest.mark.parametrize("m,ncols,m_valid,want_map", [(1024, 1152, 0, 2), (1024, 4224, 0, 2), (1280, 1152, 1100, 2), (2048, 256, 0, 1)])
def test_posterior_reduce_exact(hip, m, ncols, m_valid, want_map):
    info = _check_map(hip, want_map, m=m, n=ncols, entry="posterior_reduce", m_valid=m_valid)
    mv = m_valid if m_valid else m
    assert info["nbi"] == (mv + 255) // 256
    Linv = torch.tril(_ints((m, m), 3, 43 + m))
    Linv[mv:] = 0.0
    AK = _ints((m, ncols), 3, 47 + ncols)
    u = _ints((m,), 3, 53 + m)
    V = Linv @ AK
    vmax = float(V.abs().max())
    assert 9.0 * m < 2.0 ** 51 and vmax * vmax * m < 2.0 ** 51 and vmax * 3.0 * m < 2.0 ** 51         # V, sum V^2, sum V u exact
    mu, var = hip.posterior_reduce(Linv.cuda(), AK.cuda(), u.cuda(), 5.0e7, m_valid=m_valid)
    assert _same_bits(mu, V.t() @ u)
    assert _same_bits(var, 5.0e7 - (V * V).sum(0))


@pytest.mark.parametrize("entry", ["ak_fused", "ak_fused_grid"])
def test_ak_fused_rows_under_map_1(hip, entry):
    """Ms_pad = 2304 [9 row tiles, map 1; the grid is rounded up to 16] on a 4 x 4 x 16 lattice: the rows are bit-equal to nine
    256-row calls, which run under map 0 (same tile, same contraction order)."""
    nx, ny, nz, N, Ms = 4, 4, 16, 256, 2304
    _check_map(hip, 1, m=Ms, n=N, entry=entry)
    _check_map(hip, 0, m=256, n=N, entry=entry)
    vox = (100.0, 90.0, 110.0)
    kid = hip.kernel_id("matern32", False)
    q = torch.arange(N)
    xyz = tuple(((idx + 1).to(F64) * s).cuda() for idx, s in zip(((q // nz) % nx, q // (nz * nx), q % nz), vox))
    tab = hip.cov_table(kid, nx, ny, nz, *vox, 260.0, 260.0, 0.3, 1.2)
    A = _ints((Ms, N), 15, 59).cuda()

    def call(Ad, out):
        if entry == "ak_fused":
            hip.ak_fused(kid, Ad, xyz, 0, N, 260.0, 260.0, 0.3, 1.2, out)
        else:
            hip.ak_fused_grid(Ad, nx, ny, nz, tab, 0, N, out)
    whole = _nan_like((Ms, N + 4)).cuda()
    call(A, whole[:, :N])
    parts = _nan_like((Ms, N + 4)).cuda()
    for r in range(0, Ms, 256):
        call(A[r:r + 256], parts[r:r + 256, :N])
    assert bool(torch.isfinite(whole[:, :N]).all()) and float(whole[:, :N].abs().max()) > 0.0
    assert bool((whole.view(torch.int64) == parts.view(torch.int64)).all())


def _exact_units(Xi, Yi):
    """int64 product of integer operands; overflow excluded by 2^52 k <= 2^62."""
    assert Xi.shape[1] * 2 ** 52 <= 2 ** 62 and max(np.abs(Xi).max(), np.abs(Yi).max()) < 2 ** 26
    return Xi @ Yi


@pytest.mark.parametrize("case", ["nt", "nn", "xkm_batched", "x_lower"])
def test_real_valued_operands_meet_the_dot_product_bound(hip, case):
    """Operands i 2^-26 (26 significant bits: a path that narrowed one to fp32 would lose two of them), exact result as an int64
    product in units of 2^-52, |C - ref| <= k 2^-53 (|X| |Y|^T) elementwise: the a-priori bound of a length-k fp64 dot product in any
    order (k u with u = 2^-53, first order; k <= 1024)."""
    m, n, k = {"nt": (256, 128, 1024), "nn": (256, 128, 256), "xkm_batched": (128, 128, 128), "x_lower": (512, 256, 512)}[case]
    rng = np.random.default_rng(61 + k)
    Xi = rng.integers(-2 ** 26 + 1, 2 ** 26, size=(m, k), dtype=np.int64)
    Yi = rng.integers(-2 ** 26 + 1, 2 ** 26, size=(k, n), dtype=np.int64)         # always k x n here; laid out per entry below
    if case == "x_lower":
        Xi = np.tril(Xi)
    ref = _exact_units(Xi, Yi)
    absref = _exact_units(np.abs(Xi), np.abs(Yi))
    X = torch.from_numpy(Xi.astype(np.float64) * 2.0 ** -26).cuda()
    Y = torch.from_numpy(Yi.astype(np.float64) * 2.0 ** -26).cuda()
    C = _nan_like((m, n)).cuda()
    if case == "nt":
        assert hip.gemm_map(m, n)["map"] == 0
        hip.gemm_nt(X, Y.t().contiguous(), C)
    elif case == "nn":
        hip.gemm_nn(X, Y, C)
    elif case == "x_lower":
        hip.gemm_nn(X, Y, C, x_lower=True)
    else:
        Xt, Yt = X.t().contiguous(), Y.t().contiguous()                            # X as k x m, Y as n x k
        C2 = _nan_like((2, m, n)).cuda()
        hip.gemm_batched(False, m, n, k, Xt, m, 0, Yt, k, 0, C2, n, m * n, m, n, 2, x_km=True)
        assert bool((C2[0].view(torch.int64) == C2[1].view(torch.int64)).all())
        C = C2[1]
    got = C.cpu().numpy()
    assert np.isfinite(got).all()
    if np.finfo(np.longdouble).nmant >= 63:
        # got 2^52 is exact in fp64 (a power-of-two scale); both terms are below 2^63, so the 64-bit mantissa holds ref exactly
        # and the difference of two values that agree to ~50 bits is exact as well
        diff = np.abs(got.astype(np.longdouble) * np.longdouble(2.0 ** 52) - ref.astype(np.longdouble))
        ratio = float((diff / (absref.astype(np.longdouble) * np.longdouble(k * 2.0 ** -53))).max())
    else:
        ratio = 0.0
        for g, r, a in zip(got.ravel().tolist(), ref.ravel().tolist(), absref.ravel().tolist()):
            num, den = g.as_integer_ratio()                                        # exact: g = num / den, den a power of two
            d = abs(num * 2 ** 52 - r * den)                                       # |g 2^52 - ref| den
            ratio = max(ratio, d * 2 ** 53 / (k * a * den))
    # ratio = max |C - ref| / (k 2^-53 |X||Y|^T), both sides in units of 2^-52 (|C 2^52 - ref| against k 2^-53 absref)
    print("%s: max |C - ref| = %.4f of the bound k 2^-53 |X||Y|^T (k = %d)" % (case, ratio, k))
    assert ratio <= 1.0
