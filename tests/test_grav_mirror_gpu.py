"""AkA's gravity block from half its rows ("gravity block from half its rows"; GEOBO_GRAV_MIRROR), by value.  GPU only.

  geobo_slab_pair_y         against float64 torch, elementwise inside the rounding of its own three operations: C = 64 and 16384, planes
                            further apart than C, three rows, a table whose rows 0 and ny-1 differ in sign; padding keeps its fill
  geobo_sym_add             B += E + E^T bit for bit against torch (the same additions in the same order): n = 5, 64, 130, views with row
                            strides > n, an asymmetric E; what lies behind column n keeps its fill
  geobo_spectral_y_lattice  rows restricted to their interior planes: edge_row = 0 and two zero planes against the same launch on rows
                            whose stored boundary planes are zero, bit for bit (ny = 32, five rows, one and two blocks)
  64 x 48 x 64              the smallest grid on which the pooled feed, the hand-over and both mirrors apply (Ms = 3072, 1536 gravity rows
                            run; at ny = 32 the lattice Gram has no fused column form and the symmetric plan does not exist): `on`
                            against `off` against the N-deep GEMM of the same build (GEOBO_AKA_LATTICE=0)

Bounds of the step.  Gravity block: distance to the GEMM block over max|AkA|, `on` at most TEN times `off` (both are rounding-level paths
to the same block; the cross block, the precedent, moved by a factor of four).  Cubes and log-likelihood: `on` at most twice as far from
the GEMM route as `off` is, the bound of tests/test_cross_rows_gpu.py for the same comparison.  Everything else bit for bit."""
import gc
import os

import numpy as np
import pytest
import torch

from conftest import normwise, settings_for

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


def _bits(t):
    return t.contiguous().view(torch.int64)


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=F64) * 2 - 1).cuda()


# ---- geobo_slab_pair_y ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,plane,ny", [(64, 80, 5), (16384, 16384 + 256, 64), (16384, 16384, 32)])
def test_slab_pair_y_against_float64_torch(hip, C, plane, ny):
    """out0 = t(0) e0 + t(ny-1) e1, out1 = t(ny-1) e0 + t(0) e1.  The kernel rounds one product and one fused multiply-add per output,
    torch two products and a sum: each is within 2 eps (|t e| + |t' e'|) of the exact value, so they differ by at most 4 eps of it."""
    rows = 3
    src = torch.full((rows, 2 * plane + 6), NAN, dtype=F64, device="cuda")
    e = _rand((rows, 2, C), C + ny)
    src[:, :C], src[:, plane:plane + C] = e[:, 0], e[:, 1]
    tab = _rand((ny, C), 7 * ny)
    tab[ny - 1] = -tab[0].abs() - 0.25                      # rows 0 and ny-1 of the table differ in sign (and in value)
    tab[0] = tab[0].abs() + 0.5
    out = torch.full((rows, 2 * plane + 10), NAN, dtype=F64, device="cuda")
    src0 = src.clone()
    hip.slab_pair_y(ny, C, rows, src[:, :2 * plane], tab.reshape(-1), out[:, :2 * plane], plane=plane)
    torch.cuda.synchronize()
    a, b = tab[0], tab[ny - 1]
    want = torch.stack([a * e[:, 0] + b * e[:, 1], b * e[:, 0] + a * e[:, 1]], 1)
    mag = torch.stack([(a * e[:, 0]).abs() + (b * e[:, 1]).abs(), (b * e[:, 0]).abs() + (a * e[:, 1]).abs()], 1)
    got = torch.stack([out[:, :C], out[:, plane:plane + C]], 1)
    excess = float(((got - want).abs() - 4.0 * EPS * mag).max())
    print("slab_pair_y C=%d plane=%d ny=%d: max|got - want| = %.3e" % (C, plane, ny, float((got - want).abs().max())))
    assert not bool(torch.isnan(got).any()) and excess <= 0.0
    assert float((got[:, 0] - (a * e[:, 0] - b * e[:, 1])).abs().max()) > 0.1          # (the sign of t(ny-1) is honoured)
    # modes behind C and the slack behind the two planes keep their fill; the input is not written
    assert bool(torch.isnan(out[:, C:plane]).all()) and bool(torch.isnan(out[:, plane + C:]).all())
    assert torch.equal(_bits(src), _bits(src0))


def test_slab_pair_y_flat_buffers_as_the_product_calls_it(hip):
    """Flat [rows][2][plane] buffers (row stride 2 plane) with an offset into the source, as SpectralProduct.slab_pair_rows passes them."""
    ny, C, rows = 32, 128, 3
    pool = _rand((5 * 2 * C,), 1)
    tab = _rand((ny * C,), 2)
    out = torch.zeros(rows * 2 * C, dtype=F64, device="cuda")
    hip.slab_pair_y(ny, C, rows, pool[2 * 2 * C:], tab, out)
    torch.cuda.synchronize()
    e = pool[2 * 2 * C:].view(rows, 2, C)
    a, b = tab[:C], tab[(ny - 1) * C:]
    want = torch.stack([a * e[:, 0] + b * e[:, 1], b * e[:, 0] + a * e[:, 1]], 1)
    assert float((out.view(rows, 2, C) - want).abs().max()) <= 8.0 * EPS


# ---- geobo_sym_add ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lde,ldb", [(5, 5, 5), (5, 8, 12), (64, 64, 80), (130, 136, 130), (130, 150, 146)])
def test_sym_add_against_torch(hip, n, lde, ldb):
    Ef, Bf = _rand((n + 1, lde), n), _rand((n + 1, ldb), n + 1)
    Ef[:, n:], Bf[:, n:], Ef[n], Bf[n] = NAN, NAN, NAN, NAN                           # what lies outside the n x n views
    E, B = Ef[:n, :n], Bf[:n, :n]
    assert float((E - E.t()).abs().max()) > 0.5                                       # E is not symmetric
    want = B + (E + E.t())
    E0 = Ef.clone()
    hip.sym_add(E, B, n)
    torch.cuda.synchronize()
    assert torch.equal(_bits(B), _bits(want))
    assert bool(torch.isnan(Bf[:, n:]).all()) and bool(torch.isnan(Bf[n]).all()) and torch.equal(_bits(Ef), _bits(E0))


# ---- geobo_spectral_y_lattice on interior-only rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nprop,C,perm", [(1, 64, False), (2, 64, True), (1, 128, True), (2, 128, False)])
def test_interior_only_rows_equal_rows_with_zero_boundary_planes(hip, nprop, C, perm):
    """edge_row = 0 with ONE pair of zero planes for every row against stored zero planes per row: the same operands at other
    addresses, so bit for bit.  ny = 32, five rows (windows overlap and repeat), one and two property blocks, one and two workgroups
    along the modes."""
    ny, R, S = 32, 5, C + 16
    P = 3 * ny
    pool = _rand((P * S,), 3 * C + nprop)
    w = np.array([0, 1, 2 * ny, 1, ny + 3])
    row_off = torch.from_numpy(w.astype(np.int64) * S).cuda()
    order = torch.from_numpy(np.array([3, 0, 4, 2, 1], dtype=np.int32)).cuda() if perm else None
    tabs = [_rand((ny * C,), 11 + j) for j in range(nprop)]
    stored = torch.zeros(R * 2 * S, dtype=F64, device="cuda")
    shared = torch.zeros(2 * S, dtype=F64, device="cuda")
    ref = [torch.full((R, ny, S), 7.0, dtype=F64, device="cuda") for _ in range(nprop)]
    out = [torch.full((R, ny, S), 7.0, dtype=F64, device="cuda") for _ in range(nprop)]
    hip.spectral_y_lattice(ny, C, R, pool, row_off, stored, 2 * S, order, tabs, [o.reshape(-1) for o in ref], plane=S)
    hip.spectral_y_lattice(ny, C, R, pool, row_off, shared, 0, order, tabs, [o.reshape(-1) for o in out], plane=S)
    torch.cuda.synchronize()
    for j in range(nprop):
        assert not bool(torch.isnan(ref[j]).any()) and float(ref[j][:, :, :C].abs().max()) > 0.0
        assert torch.equal(_bits(out[j]), _bits(ref[j]))
    # ... and it is the Toeplitz product of the window's interior planes alone, by value (row 0, block 0, fp64 torch)
    x = pool.view(P, S)[w[0]:w[0] + ny, :C].clone()
    x[0], x[ny - 1] = 0.0, 0.0
    t = tabs[0].view(ny, C)
    d = (torch.arange(ny)[:, None] - torch.arange(ny)[None, :]).abs().cuda()
    want = (t[d] * x[None, :, :]).sum(1)
    assert float((out[0][0, :, :C] - want).abs().max()) <= 64.0 * ny * EPS * float((t[d].abs() * x[None].abs()).sum(1).max())


# ---- whole steps, 64 x 48 x 64 ----------------------------------------------------------------------------------------------------------
_RUNS = {}
COMPUTED = (0, 1, 3, 4)          # mean and variance cubes of the two computed property blocks
GRID = (64, 48, 64)


class _Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(grav, lattice=True, keep_ak=False):
    """One cubing step at 64 x 48 x 64 (Matern-3/2, vertical field, 5 drill voxels, two property blocks, the cross block from the magnetic
    rows): host copies of what the tests compare.  lattice False: AkA by the N-deep GEMM.  Every combination runs once per session; what
    is kept lives on the host, except the three blocks of A K that keep_ak leaves on the device for the caller, who drops them (14.5 GB)."""
    key = (grav, lattice)
    if key in _RUNS:
        return _RUNS[key]
    import bench
    from geobo_amd.inversion import Inversion
    with _Env(GEOBO_GRAV_MIRROR=grav, GEOBO_CROSS_ROWS="magn", GEOBO_AKA_LATTICE="1" if lattice else "0"):
        s = settings_for(*GRID, kernelfunc="matern32", XMAG=0, YMAG=0, ZMAG=1)
        inv = Inversion(settings=s, props=(0, 1))
        grav_d, mag_d, loc, drill0 = bench.synthetic_inputs(inv, 5)
        inv.gp_length = np.array([200.0, 202.0, 204.0])
        keep = {}
        inv.engine.aka_hook = lambda AkA: keep.__setitem__("AkA", AkA.clone())
        cubes = inv.cubing(grav_d, mag_d, drill0[drill0 != 0], loc, drill0)
        eng = inv.engine
        step = eng.last["step"]
        Ms, Msp, nc = eng.Ms, eng.Ms_pad, eng.nc
        report = {f: dict(r) for f, r in eng.aka_mirror.items()}
        ak = None
        if keep_ak:
            AK = eng.last["AK"] if eng.last["AK_complete"] else eng.last["AK_partial"]
            ak = [AK[0:Ms, 0:eng.N].clone(), AK[0:Ms, nc:nc + eng.N].clone(), AK[Msp:Msp + Ms, nc:nc + eng.N].clone()]
            del AK
        res = dict(cubes=[np.array(c) for c in cubes], logl=float(inv.logl), AkA=keep.pop("AkA").cpu(), route=eng.step_route, fed=sorted(step.gram_S),
                   cross=step.cross_rows, mirror=step.mirror, grav_mirror=step.grav_mirror, fills=len(step.ak_fill), ak=ak, Ms=Ms, Msp=Msp,
                   report=report)
    inv.engine.aka_hook = None
    del inv, eng, step, keep
    gc.collect()
    torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The tests after this module get the device as they would without it."""
    yield
    _RUNS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _whole(A):
    """A symmetric matrix from its lower triangle (what every route defines)."""
    return torch.tril(A) + torch.tril(A, -1).t()


def test_gravity_block_against_the_gemm_route():
    """`on` runs 1536 of the 3072 gravity rows, interior part only, and builds the block from them, the mirror and the three slab terms;
    the N-deep GEMM of the same build is the reference.  Measured on one MI355X (printed by this test):
        gravity block, distance to the GEMM block / max|AkA|: on 1.110e-15, off 1.057e-15 (ratio 1.05); on, upper against lower
        triangle 5.7e-16; cubes (mean 0, mean 1, variance 0, variance 1) against the GEMM route: on 2.02e-13 5.20e-13 1.44e-13 2.89e-14,
        off 1.71e-13 4.72e-13 1.46e-13 2.71e-14; the log-likelihood is the same double in all three."""
    new, par, ref = _run("on", keep_ak=True), _run("off", keep_ak=True), _run("off", lattice=False)
    assert new["route"] == par["route"] == "single" and ref["route"] == "columns" and ref["fed"] == [] and ref["grav_mirror"] == 0
    Ms, Msp = new["Ms"], new["Msp"]
    assert Ms == 3072 and new["grav_mirror"] == 1536 and par["grav_mirror"] == 0 and new["mirror"] == par["mirror"] == 1536
    assert new["cross"] == par["cross"] == "magn" and new["fed"] == par["fed"] == [(0, 0), (1, 0), (1, 1)] and new["fills"] == par["fills"] == 2
    # what the step records: taken by the gate, the measurements beside it (gravity's slabs are far from their mirror -- not asked)
    assert new["report"]["grav"]["taken"] is True and par["report"]["grav"]["taken"] is False and new["report"]["magn"]["taken"] is True
    assert not new["report"]["grav"]["symmetric"] and new["report"]["grav"]["deviation"] > 2.0 ** -48
    R = _whole(ref["AkA"])
    top = float(R.abs().max())
    gg = (slice(0, Ms), slice(0, Ms))
    d_new, d_par = (float((_whole(r["AkA"][gg]) - R[gg]).abs().max()) / top for r in (new, par))
    # the block's full square is filled, and it is symmetric to the same rounding level
    up = float((new["AkA"][gg] - new["AkA"][gg].t()).abs().max()) / top
    msg = ("64x48x64 gravity block vs the N-deep GEMM / max|AkA|: on %.3e, off %.3e (ratio %.2f); on, upper vs lower triangle %.3e"
           % (d_new, d_par, d_new / d_par if d_par else float("inf"), up))
    print(msg)
    e_new = [normwise(new["cubes"][i], ref["cubes"][i]) for i in COMPUTED] + [abs(new["logl"] - ref["logl"]) / abs(ref["logl"])]
    e_par = [normwise(par["cubes"][i], ref["cubes"][i]) for i in COMPUTED] + [abs(par["logl"] - ref["logl"]) / abs(ref["logl"])]
    fmt = lambda e: " ".join("%.2e" % v for v in e)
    msg2 = "64x48x64 cubes (mean 0, mean 1, var 0, var 1), logl: on vs GEMM %s | off vs GEMM %s" % (fmt(e_new), fmt(e_par))
    print(msg2)
    # the other blocks: bit for bit
    blocks = {"cross (lower left)": (slice(Msp, Msp + Ms), slice(0, Ms)), "cross (upper right)": (slice(0, Ms), slice(Msp, Msp + Ms)),
              "magnetic": (slice(Msp, Msp + Ms), slice(Msp, Msp + Ms)), "drill rows": (slice(2 * Msp, None), slice(None))}
    for name, b in blocks.items():
        assert torch.equal(_bits(new["AkA"][b]), _bits(par["AkA"][b])), name
    # A K read through the completion hook after the step: the parent's buffer, bit for bit
    same = [torch.equal(_bits(a), _bits(b)) for a, b in zip(new["ak"], par["ak"])]
    new["ak"] = par["ak"] = None                                             # (the device copies: not kept for the session)
    gc.collect()
    torch.cuda.empty_cache()
    assert same == [True, True, True]
    assert 0.0 < d_par and d_new <= 10.0 * d_par, msg
    assert up <= 10.0 * d_par, msg
    for a, b in zip(e_new, e_par):
        assert a <= 2.0 * b, msg2


def test_refused_step_is_the_parents():
    """The route off: the step launches the parent's kernels -- every gravity row runs whole, the same hand-over, the same two fills --
    and says so.  (`off` here and in the test above is one cached run.)"""
    par = _run("off")
    assert par["grav_mirror"] == 0 and par["report"]["grav"]["taken"] is False
    assert par["fed"] == [(0, 0), (1, 0), (1, 1)] and par["fills"] == 2 and par["mirror"] == 1536
