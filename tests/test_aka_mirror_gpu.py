"""The mirrored magnetic block of AkA ("point mirror"): the native fill and row copy by value against torch.flip,
the deviation reduction against the same maxima in torch, and whole steps with the shortcut against GEOBO_AKA_MIRROR=0.  GPU only.

Grids of the end-to-end cases.  The shortcut lives in the symmetric plan of A K (step.sym), which needs the fused lattice Gram:
64 x 48 x 64 is the smallest grid that has it.  64 x 16 x 64 is planned "single" as well, but its AkA is a GEMM and its steps run as
"columns" (tests/test_logl_grad_gpu.py says the same): there the gate must say no and the switch must change nothing, which is
what its case checks."""
import gc
import os

import numpy as np
import pytest
import torch

from conftest import normwise, settings_for

pytestmark = pytest.mark.gpu

F64 = torch.float64


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=F64) * 2 - 1).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---- geobo_centro_fill ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld,r0", [(6, 6, 3), (7, 8, 4), (130, 136, 65), (130, 130, 100)])
def test_centro_fill_against_flip(hip, n, ld, r0):
    """B[r, c] = B[n-1-r, n-1-c] for r >= r0; rows below r0 and the padding columns (NaN) keep their bits; n = 7: the middle row 3
    is a source only."""
    B0 = torch.full((n, ld), float("nan"), dtype=F64, device="cuda")
    B0[:, :n] = _rand((n, n), 100 + n + r0)
    B = B0.clone()
    hip.centro_fill(B, n, r0)
    torch.cuda.synchronize()
    want = B0.clone()
    want[r0:, :n] = torch.flip(B0[:n - r0, :n], (0, 1))
    assert torch.equal(_bits(B), _bits(want))
    assert torch.equal(_bits(B[:r0]), _bits(B0[:r0])) and torch.equal(_bits(B[:, n:]), _bits(B0[:, n:]))
    if 2 * r0 == n:                 # filled from the middle of an even block: the whole block is its own point mirror
        assert torch.equal(B[:, :n], torch.flip(B[:, :n], (0, 1)))


def test_centro_fill_refuses_bad_arguments(hip):
    from geobo_amd import _lib
    L = _lib.load()
    n = 6
    flat = _rand((n * n + 2,), 7)
    B = flat[:n * n].view(n, n)
    keep = B.clone()
    with pytest.raises(RuntimeError, match="GEOBO_E_ARG"):
        hip.centro_fill(B, n, n // 2 - 1)                       # row n/2 would be read and written
    with pytest.raises(RuntimeError, match="GEOBO_E_ARG"):
        hip.centro_fill(flat[1:1 + n * n].view(n, n), n, 3)     # 8 bytes off the 16-byte boundary
    assert L.geobo_centro_fill(None, n, n, 3, None) == -1       # null
    torch.cuda.synchronize()
    assert torch.equal(B, keep)


def test_mirror_rows_against_flip(hip):
    """Rows of A K under the point mirror: voxel blocks (iy, ix) reversed, z kept; rows below r0 and the padding keep their bits."""
    m, nb, nz, ld, r0 = 10, 12, 6, 80, 6
    X0 = torch.full((m, ld), float("nan"), dtype=F64, device="cuda")
    X0[:, :nb * nz] = _rand((m, nb * nz), 11)
    X = X0.clone()
    hip.mirror_rows(X, m, r0, nb, nz)
    torch.cuda.synchronize()
    want = X0.clone()
    want[r0:, :nb * nz] = torch.flip(X0[:m - r0, :nb * nz].view(m - r0, nb, nz), (0, 1)).reshape(m - r0, nb * nz)
    assert torch.equal(_bits(X), _bits(want))
    with pytest.raises(RuntimeError, match="GEOBO_E_ARG"):
        hip.mirror_rows(X, m, 4, nb, nz)


# ---- geobo_mirror_dev -----------------------------------------------------------------------------------------------------------------
NX = NY = 8
NZ = 4


def _table_and_slabs(seed):
    Q = _rand((2 * NY - 3, 2 * NX - 1, NZ), seed)
    E = torch.full((NX * NY, 2 * NX * NZ + 8), float("nan"), dtype=F64, device="cuda")        # [sensor][slab 0 | slab 1 | padding]
    E[:, :2 * NX * NZ] = _rand((NX * NY, 2 * NX * NZ), seed + 1)
    return Q, E


def _measure(hip, Q, E):
    pl = NX * NZ
    Q2 = Q.view(2 * NY - 3, (2 * NX - 1) * NZ)
    out = torch.cat([hip.mirror_dev(Q2, Q2, 2 * NY - 3, 2 * NX - 1, NZ), hip.mirror_dev(E[:, :pl], E[:, pl:2 * pl], NX * NY, NX, NZ)])
    return out.tolist()


def _reference(Q, E):
    pl = NX * NZ
    E0, E1 = E[:, :pl].reshape(-1, NX, NZ), E[:, pl:2 * pl].reshape(-1, NX, NZ)
    return [float((Q - torch.flip(Q, (0, 1))).abs().max()), float(Q.abs().max()),
            float((E0 - torch.flip(E1, (0, 1))).abs().max()), float(torch.maximum(E0.abs().max(), E1.abs().max()))]


def test_mirror_dev_against_torch(hip):
    """Q[dy][dx][iz] against Q[-dy][-dx][iz]; slab 0 of sensor r at (ix, iz) against slab 1 of sensor Ms-1-r at (nx-1-ix, iz)."""
    Q, E = _table_and_slabs(31)
    assert _measure(hip, Q, E) == _reference(Q, E)


def test_mirror_dev_of_a_mirrored_operator_is_zero_and_sees_one_element(hip):
    pl = NX * NZ
    Q, E = _table_and_slabs(41)
    Q = Q + torch.flip(Q, (0, 1))
    E[:, pl:2 * pl] = torch.flip(E[:, :pl].reshape(-1, NX, NZ), (0, 1)).reshape(-1, pl)
    got = _measure(hip, Q, E)
    assert got[0] == 0.0 and got[2] == 0.0 and got[1] == float(Q.abs().max()) and got[3] == float(E[:, :pl].abs().max())
    for where in ("table", "slab"):
        Qp, Ep = Q.clone(), E.clone()
        if where == "table":
            x = float(Qp[3, 4, 1])
            Qp[3, 4, 1] = x + 1e-9
        else:
            x = float(Ep[5, pl + 7])
            Ep[5, pl + 7] = x + 1e-9
        got = _measure(hip, Qp, Ep)
        want = abs((x + 1e-9) - x)
        assert 0.9e-9 < want < 1.1e-9
        assert (got[0], got[2]) == ((want, 0.0) if where == "table" else (0.0, want))
    Ep = E.clone()
    Ep[9, 3] = float("nan")
    assert np.isnan(_measure(hip, Q, Ep)[2])                     # a NaN is not lost in the maxima: the gate then says no


# ---- whole steps ------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _run(shape, field, mirror):
    """One cubing step (Matern-3/2, 5 drill voxels, two property blocks) with the shortcut switched on / off: host copies of what the
    tests compare.  Every (grid, field, switch) runs once per session; the engine is dropped before the next one is built."""
    key = (shape, field, mirror)
    if key in _RUNS:
        return _RUNS[key]
    import bench
    from geobo_amd.inversion import Inversion
    before = os.environ.get("GEOBO_AKA_MIRROR")
    os.environ["GEOBO_AKA_MIRROR"] = "1" if mirror else "0"
    try:
        s = settings_for(*shape, kernelfunc="matern32", XMAG=field[0], YMAG=field[1], ZMAG=field[2])
        inv = Inversion(settings=s, props=(0, 1))
        grav, mag, loc, drill0 = bench.synthetic_inputs(inv, 5)
        inv.gp_length = np.array([200.0, 202.0, 204.0])
        keep = {}
        inv.engine.aka_hook = lambda AkA: keep.__setitem__("AkA", AkA.clone())
        cubes = inv.cubing(grav, mag, drill0[drill0 != 0], loc, drill0)
        eng = inv.engine
        res = dict(cubes=[np.array(c) for c in cubes], logl=float(inv.logl), AkA=keep["AkA"], route=eng.step_route, Msp=eng.Ms_pad, Ms=eng.Ms,
                   report={f: dict(r) for f, r in eng.aka_mirror.items()}, mirror_rows=eng.last["step"].mirror)
    finally:
        if before is None:
            os.environ.pop("GEOBO_AKA_MIRROR", None)
        else:
            os.environ["GEOBO_AKA_MIRROR"] = before
    del inv, eng
    gc.collect()
    torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


VERTICAL, INCLINED = (0, 0, 1), (0.3, 0.2, 0.9)
COMPUTED = (0, 1, 3, 4)          # mean and variance cubes of the two computed property blocks


def test_step_with_the_mirrored_block_against_the_full_one():
    """64 x 48 x 64, vertical field: the shortcut is taken for the magnetic operator by measurement and refused for gravity by
    measurement; the magnetic block agrees to 1e-12 max|AkA| (what the project asks between its AkA forms), everything else of AkA bit
    for bit, cubes and log-likelihood to 1e-13 (NOTES.md section 2: alternative Gram forms)."""
    on, off = _run((64, 48, 64), VERTICAL, True), _run((64, 48, 64), VERTICAL, False)
    print("mirror report:", on["report"])
    assert on["route"] == off["route"] == "single"
    assert on["report"]["magn"]["taken"] and on["report"]["magn"]["symmetric"] and on["report"]["magn"]["deviation"] <= 2.0 ** -48
    assert not on["report"]["grav"]["taken"] and not on["report"]["grav"]["symmetric"] and on["report"]["grav"]["deviation"] > 2.0 ** -48
    assert on["mirror_rows"] == on["Ms"] // 2 and off["mirror_rows"] == 0 and off["report"] == {}
    Msp, Ms = on["Msp"], on["Ms"]
    A1, A0 = on["AkA"], off["AkA"]
    mm = (slice(Msp, Msp + Ms), slice(Msp, Msp + Ms))
    e_mm = float((A1[mm] - A0[mm]).abs().max() / A0.abs().max())
    errs = [normwise(on["cubes"][i], off["cubes"][i]) for i in COMPUTED]
    e_logl = abs(on["logl"] - off["logl"]) / abs(off["logl"])
    print("64x48x64 mirrored vs full: MM block %.2e of max|AkA|, cubes %s, logl %.2e" % (e_mm, " ".join("%.2e" % e for e in errs), e_logl))
    assert e_mm <= 1e-12
    A1, A0 = A1.clone(), A0.clone()
    A1[mm], A0[mm] = 0.0, 0.0
    assert torch.equal(A1, A0)                                               # grav rows, cross block, drill rows, padding: the same bits
    assert max(errs) <= 1e-13
    assert e_logl <= 1e-13


def test_inclined_field_is_measured_and_refused():
    """The same grid under the field (0.3, 0.2, 0.9): the magnetic operator is not its own point mirror, the shortcut is not taken and
    the step is the one GEOBO_AKA_MIRROR=0 runs, bit for bit."""
    on, off = _run((64, 48, 64), INCLINED, True), _run((64, 48, 64), INCLINED, False)
    print("mirror report (inclined):", on["report"])
    assert on["route"] == off["route"] and on["mirror_rows"] == 0
    assert not on["report"]["magn"]["taken"] and not on["report"]["magn"]["symmetric"] and on["report"]["magn"]["deviation"] > 1e-3
    for i in COMPUTED:
        assert np.array_equal(on["cubes"][i], off["cubes"][i])
    assert on["logl"] == off["logl"] and torch.equal(on["AkA"], off["AkA"])


def test_grid_without_the_symmetric_plan_is_untouched():
    """64 x 16 x 64, vertical field: planned "single", but AkA is a GEMM there and the step runs as "columns" -- no symmetric plan, so
    the gate says no whatever the operator measures, and the switch changes nothing."""
    on, off = _run((64, 16, 64), VERTICAL, True), _run((64, 16, 64), VERTICAL, False)
    assert on["route"] == off["route"] == "columns" and on["mirror_rows"] == 0
    assert not any(r["taken"] for r in on["report"].values())
    for i in COMPUTED:
        assert np.array_equal(on["cubes"][i], off["cubes"][i])
    assert on["logl"] == off["logl"] and torch.equal(on["AkA"], off["AkA"])
