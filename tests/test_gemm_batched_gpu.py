"""geobo_gemm_batched at valid extents well inside its 128-wide tiles (the boundary-slab products: 64, 16 or 5 valid rows / columns),
and with the left factor given transposed (GEOBO_GEMM_X_KM): by value against torch.matmul, the padding of C untouched, and bit for
bit against the same products through the entry points that existed before the transposed mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 1e-13            # normwise; k <= 128 products of values in [-1, 1] in fp64 sit three orders below it


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64)


def _operands(y_is_kn, m, n, k, batch, seed, x_km=False):
    """Padded operands (readable over the full 128-multiples the launch computes) and their strides."""
    X = _rand((batch, k, m) if x_km else (batch, m, k), seed)
    Y = _rand((batch, k, n) if y_is_kn else (batch, n, k), seed + 1)
    return X, Y


def _product(y_is_kn, X, Y, x_km=False):
    return torch.matmul(X.transpose(1, 2) if x_km else X, Y if y_is_kn else Y.transpose(1, 2))


def _run(hip, y_is_kn, X, Y, C, m, n, k, mv, nv, batch, x_km=False, **kw):
    return hip.gemm_batched(y_is_kn, m, n, k, X, X.stride(1), X.stride(0), Y, Y.stride(1), Y.stride(0), C, C.stride(1), C.stride(0),
                            mv, nv, batch, x_km=x_km, **kw)


@pytest.mark.parametrize("y_is_kn", [False, True])
@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("mv,nv", [(100, 64), (128, 16), (64, 200), (5, 128), (5, 16)])
def test_small_valid_extents_match_torch(hip, y_is_kn, k, mv, nv):
    m, n, batch = hip.pad_n(mv), hip.pad_n(nv), 3
    X, Y = _operands(y_is_kn, m, n, k, batch, 11 * k + mv + nv)
    ref = _product(y_is_kn, X, Y)[:, :mv, :nv]
    C = torch.full((batch, m + 3, n + 5), float("nan"), dtype=torch.float64, device="cuda")
    _run(hip, y_is_kn, X, Y, C, m, n, k, mv, nv, batch)
    err = (C[:, :mv, :nv] - ref).abs().max().item() / ref.abs().max().item()
    print("kn %s, k = %d, valid %d x %d: %.2e" % (y_is_kn, k, mv, nv, err))
    assert err <= BOUND
    pad = C.clone()
    pad[:, :mv, :nv] = float("nan")
    assert bool(torch.isnan(pad).all())                                        # nothing stored outside the valid region


@pytest.mark.parametrize("y_is_kn,x_km", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("mv,nv", [(100, 64), (5, 200), (200, 200)])
def test_accumulation_keeps_the_padding_bits(hip, y_is_kn, x_km, mv, nv):
    """beta = 1 into a C whose padding is NaN with a payload: valid region = C + X op(Y), every other bit of the buffer unchanged."""
    m, n, k, batch = hip.pad_n(mv), hip.pad_n(nv), 64, 3
    X, Y = _operands(y_is_kn, m, n, k, batch, 300 + mv + nv, x_km)
    C = torch.full((batch, m + 3, n + 5), 0.0, dtype=torch.float64, device="cuda")
    C.view(torch.int64).fill_(0x7FF8_0000_0000_1234)
    C0 = _rand((batch, mv, nv), 7)
    C[:, :mv, :nv] = C0
    before = C.clone()
    _run(hip, y_is_kn, X, Y, C, m, n, k, mv, nv, batch, x_km=x_km, beta=1.0)
    ref = C0 + _product(y_is_kn, X, Y, x_km)[:, :mv, :nv]
    err = (C[:, :mv, :nv] - ref).abs().max().item() / ref.abs().max().item()
    print("beta = 1, kn %s, x_km %s, valid %d x %d: %.2e" % (y_is_kn, x_km, mv, nv, err))
    assert err <= BOUND
    C[:, :mv, :nv] = C0
    assert bool((_bits(C) == _bits(before)).all())


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("mv,nv", [(128, 64), (100, 16), (1030, 64), (300, 200)])
def test_transposed_left_factor_matches_torch(hip, k, mv, nv):
    """X given as k x m: one and two column tiles, more than one row tile, ragged against the tile."""
    m, n, batch = hip.pad_n(mv), hip.pad_n(nv), 3
    X, Y = _operands(False, m, n, k, batch, 500 + mv + nv + k, x_km=True)
    ref = _product(False, X, Y, x_km=True)[:, :mv, :nv]
    C = torch.full((batch, m, n + 5), float("nan"), dtype=torch.float64, device="cuda")
    _run(hip, False, X, Y, C, m, n, k, mv, nv, batch, x_km=True)
    err = (C[:, :mv, :nv] - ref).abs().max().item() / ref.abs().max().item()
    print("transposed X, k = %d, valid %d x %d: %.2e" % (k, mv, nv, err))
    assert err <= BOUND
    # the same product with X transposed beforehand: the same k order, the same bits
    Xt = X.transpose(1, 2).contiguous()
    C2 = torch.zeros_like(C)
    _run(hip, False, Xt, Y, C2, m, n, k, mv, nv, batch)
    assert bool((_bits(C[:, :mv, :nv]) == _bits(C2[:, :mv, :nv])).all())


@pytest.mark.parametrize("y_is_kn", [False, True])
def test_existing_callers_keep_their_bits(hip, y_is_kn):
    """A shape the spectral route's callers use (128 x 128 tiles, k = 128, one product per plane): the batched launch agrees bit for
    bit with the unbatched GEMM entry on every plane (the 128 x 128 instantiation the batched entry has always run; an indirect pin:
    both go through the same, unchanged dispatch by rows), and a launch with smaller valid extents reproduces its bits on the part
    it stores."""
    m = n = k = 128
    batch = 3
    X, Y = _operands(y_is_kn, m, n, k, batch, 900)
    full = torch.zeros((batch, m, n), dtype=torch.float64, device="cuda")
    _run(hip, y_is_kn, X, Y, full, m, n, k, m, n, batch)
    for b in range(batch):
        one = torch.zeros((m, n), dtype=torch.float64, device="cuda")
        (hip.gemm_nn if y_is_kn else hip.gemm_nt)(X[b], Y[b], one)
        assert bool((_bits(one) == _bits(full[b])).all())
    for mv, nv in ((128, 64), (64, 128), (5, 128), (128, 16)):
        part = torch.zeros((batch, m, n), dtype=torch.float64, device="cuda")
        _run(hip, y_is_kn, X, Y, part, m, n, k, mv, nv, batch)
        assert bool((_bits(part[:, :mv, :nv]) == _bits(full[:, :mv, :nv])).all())
        assert bool((part[:, mv:] == 0).all()) and bool((part[:, :, nv:] == 0).all())


def test_operand_extent_check_covers_the_compute_extent(hip):
    """Operands are read over the 128-multiples whatever the valid extents: one that ends right behind its 64 valid columns (or, given
    transposed, its 64 valid rows) is refused before the launch."""
    k, batch = 64, 2
    X = _rand((batch, 128, k), 1)
    Yflat = _rand((batch * k * 64,), 2)                                          # [batch][k][64], nothing behind it
    C = torch.zeros((batch, 128, 64), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="past its allocation"):
        hip.gemm_batched(True, 128, 128, k, X, k, 128 * k, Yflat, 64, k * 64, C, 64, 128 * 64, 128, 64, batch)
    Y = _rand((batch, 128, k), 3)
    with pytest.raises(ValueError, match="past its allocation"):
        hip.gemm_batched(False, 128, 128, k, Yflat, 64, k * 64, Y, k, 128 * k, C, 64, 128 * 64, 64, 64, batch, x_km=True)
