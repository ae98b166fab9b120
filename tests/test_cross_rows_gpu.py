"""AkA's cross block from the mirrored half of the magnetic rows (GEOBO_CROSS_ROWS), by value.  GPU only.

  geobo_mirror_planes   bit for bit against torch indexing: strides with slack, a partial row range, NaN-filled surroundings untouched,
                        argument rejections write nothing
  64 x 48 x 64          the smallest grid of the `single` family with the magnetic mirror: `magn` against `grav` (the parent's plan), both
                        against the N-deep GEMM of the same build (GEOBO_AKA_LATTICE=0: no Gram, no mirror)
  inclined field        the mirror is refused: `magn` and `grav` are the same step, bit for bit
  64^3                  the default option takes the new plan; mean and variance at the voxels of the independent oracle sample

Bounds.  The new plan and the parent's are rounding-level paths of similar length to the same matrix, so the new plan may be at most
TWICE as far from the GEMM route as the parent's plan is (AkA: max|delta| over the whole matrix / max|AkA|; every cube: normwise;
log-likelihood: relative); magn against grav is then bounded by the triangle inequality, three times the parent's distance.  All
figures are printed.  Measured on one MI355X: see the docstring of test_block_assembly_against_the_gemm_route."""
import gc
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, normwise, settings_for

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---- geobo_mirror_planes ----------------------------------------------------------------------------------------------------------------
def _planes(m, nx, nz, lds, ldd, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    src = (torch.rand((m, lds), generator=g, dtype=F64) * 2 - 1).cuda()
    dst = torch.full((m, ldd), NAN, dtype=F64, device="cuda")
    return src, dst


@pytest.mark.parametrize("m,nx,nz,r0,r1", [(6, 4, 2, 0, 3), (6, 4, 2, 0, 6), (7, 5, 6, 1, 4), (7, 5, 6, 0, 0), (9, 3, 4, 2, 9), (9, 3, 4, 4, 5),
                                           (300, 64, 64, 3, 290)])
def test_mirror_planes_against_torch_indexing(hip, m, nx, nz, r0, r1):
    """dst[m-1-r][(x, z)] = src[r][(nx-1-x, z)] for r0 <= r < r1 with row strides that leave slack behind the plane (different for
    source and destination); every other row and the slack keep their NaN fill.  The last case is the step's plane (64 x 64: several
    workgroups per row)."""
    pl = nx * nz
    lds, ldd = pl + 6, pl + 10
    src, dst = _planes(m, nx, nz, lds, ldd, 11 * m + nx)
    src0 = src.clone()
    hip.mirror_planes(src[:, :pl], dst[:, :pl], m, r0, r1, nx, nz)
    torch.cuda.synchronize()
    want = torch.full((m, ldd), NAN, dtype=F64, device="cuda")
    for r in range(r0, r1):
        want[m - 1 - r, :pl] = src0[r, :pl].view(nx, nz).flip(0).reshape(-1)
    assert torch.equal(_bits(dst), _bits(want))
    assert torch.equal(_bits(src), _bits(src0))
    written = torch.zeros(m, dtype=torch.bool)
    written[[m - 1 - r for r in range(r0, r1)]] = True
    assert bool(torch.isnan(dst[~written.cuda()]).all()) and bool(torch.isnan(dst[:, pl:]).all())
    assert not bool(torch.isnan(dst[written.cuda()][:, :pl]).any())


def test_mirror_planes_between_two_planes_of_one_buffer(hip):
    """As the step calls it: plane 0 from plane ny-1 and the other way round inside one buffer of rows, second half from the first."""
    m, nx, ny, nz = 8, 4, 3, 2
    pl = nx * nz
    X = _planes(m, nx, nz, ny * pl, ny * pl, 5)[0]
    X[m // 2:] = NAN
    X0 = X.clone()
    for d, s in ((0, ny - 1), (ny - 1, 0)):
        hip.mirror_planes(X[:, s * pl:(s + 1) * pl], X[:, d * pl:(d + 1) * pl], m, 0, m // 2, nx, nz)
    torch.cuda.synchronize()
    want = X0.clone()
    for r in range(m // 2):
        for d, s in ((0, ny - 1), (ny - 1, 0)):
            want[m - 1 - r, d * pl:(d + 1) * pl] = X0[r, s * pl:(s + 1) * pl].view(nx, nz).flip(0).reshape(-1)
    assert torch.equal(_bits(X), _bits(want))
    assert bool(torch.isnan(X[m // 2:, pl:(ny - 1) * pl]).all())                 # the interior plane of the mirrored rows: untouched


def test_mirror_planes_refuses_bad_arguments(hip):
    """Null pointers, a bad row range, planes wider than a row stride: GEOBO_E_ARG (-1); odd nz or strides, a misaligned pointer:
    GEOBO_E_ALIGN (-2).  Nothing is launched: the destination keeps its fill."""
    from geobo_amd import _lib
    L = _lib.load()
    m, nx, nz = 6, 4, 2
    pl = nx * nz
    src, dst = _planes(m, nx, nz, pl + 6, pl + 10, 3)
    p = lambda t: t.data_ptr()
    ok = [p(src), pl + 6, p(dst), pl + 10, m, 0, 3, nx, nz, None]
    bad = {"null src": ({0: None}, -1), "null dst": ({2: None}, -1), "negative m": ({4: -1}, -1), "negative r0": ({5: -1}, -1),
           "r0 > r1": ({5: 4}, -1), "r1 > m": ({6: m + 1}, -1), "nx = 0": ({7: 0}, -1), "nz = 0": ({8: 0}, -1), "short lds": ({1: pl - 2}, -1),
           "short ldd": ({3: pl - 2}, -1), "odd nz": ({8: 1}, -2), "odd lds": ({1: pl + 7}, -2), "odd ldd": ({3: pl + 11}, -2),
           "misaligned src": ({0: p(src) + 8}, -2), "misaligned dst": ({2: p(dst) + 8}, -2)}
    for what, (change, code) in bad.items():
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert L.geobo_mirror_planes(*args) == code, what
    with pytest.raises(RuntimeError):
        hip.mirror_planes(src[:, :pl], dst[:, :pl], m, 4, 3, nx, nz)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())
    assert L.geobo_mirror_planes(*ok) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dst[m - 3:, :pl]).any()) and bool(torch.isnan(dst[:m - 3]).all())


# ---- whole steps ------------------------------------------------------------------------------------------------------------------------
_RUNS = {}
VERTICAL, INCLINED = (0, 0, 1), (0.3, 0.2, 0.9)
COMPUTED = (0, 1, 3, 4)          # mean and variance cubes of the two computed property blocks


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


def _run(field, cross, lattice=True, keep_ak=False):
    """One cubing step at 64 x 48 x 64 (Matern-3/2, 5 drill voxels, two property blocks): host / device copies of what the tests compare.
    lattice False: AkA by the N-deep GEMM (GEOBO_AKA_LATTICE=0).  Every combination runs once per session.  What is kept between tests
    lives on the host; keep_ak leaves the three blocks of A K on the device for the caller, who drops them (14.5 GB)."""
    key = (field, cross, lattice)
    if key in _RUNS:
        return _RUNS[key]
    import bench
    from geobo_amd.inversion import Inversion
    with _Env(GEOBO_CROSS_ROWS=cross, GEOBO_AKA_LATTICE="1" if lattice else "0"):
        s = settings_for(64, 48, 64, kernelfunc="matern32", XMAG=field[0], YMAG=field[1], ZMAG=field[2])
        inv = Inversion(settings=s, props=(0, 1))
        grav, mag, loc, drill0 = bench.synthetic_inputs(inv, 5)
        inv.gp_length = np.array([200.0, 202.0, 204.0])
        keep = {}
        inv.engine.aka_hook = lambda AkA: keep.__setitem__("AkA", AkA.clone())
        cubes = inv.cubing(grav, mag, drill0[drill0 != 0], loc, drill0)
        eng = inv.engine
        step = eng.last["step"]
        Ms, Msp, nc = eng.Ms, eng.Ms_pad, eng.nc
        ak = None
        if keep_ak:
            AK = eng.last["AK"] if eng.last["AK_complete"] else eng.last["AK_partial"]
            ak = [AK[0:Ms, 0:eng.N].clone(), AK[0:Ms, nc:nc + eng.N].clone(), AK[Msp:Msp + Ms, nc:nc + eng.N].clone()]
            del AK
        res = dict(cubes=[np.array(c) for c in cubes], logl=float(inv.logl), AkA=keep.pop("AkA").cpu(), route=eng.step_route, fed=sorted(step.gram_S),
                   cross=step.cross_rows, mirror=step.mirror, fills=len(step.ak_fill), ak=ak, Ms=Ms, Msp=Msp, Mv=2 * Msp + 5)
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


def _whole(res):
    """The step's matrix with both triangles: the lower triangle (what every route defines) reflected."""
    A = res["AkA"]
    return torch.tril(A) + torch.tril(A, -1).t()


def test_block_assembly_against_the_gemm_route():
    """64 x 48 x 64, vertical field.  `magn` builds the cross block from the 1536 magnetic rows it runs anyway; the N-deep GEMM of the
    same build is the reference.  Measured on one MI355X (printed by this test):
        AkA, whole matrix, distance to the GEMM route / max|AkA|:  magn 1.328e-14, grav 1.328e-14 (the largest entry of either is outside
        the cross block); the cross block alone: magn 1.239e-15, grav 3.248e-16; magn against grav 1.230e-15
        cubes (mean 0, mean 1, variance 0, variance 1) against the GEMM route: magn 1.71e-13 4.72e-13 1.46e-13 2.71e-14,
        grav 1.70e-13 5.44e-13 1.46e-13 3.81e-14; magn against grav 2.29e-14 3.28e-13 7.95e-16 1.53e-14; the log-likelihood is the
        same double in all three; A K read afterwards: the three blocks equal the parent's bit for bit (0.0)."""
    new, par, ref = _run(VERTICAL, "magn", keep_ak=True), _run(VERTICAL, "grav", keep_ak=True), _run(VERTICAL, "grav", lattice=False)
    assert new["route"] == par["route"] == "single" and ref["route"] == "columns" and ref["fed"] == [] and ref["mirror"] == 0
    assert new["cross"] == "magn" and par["cross"] == "grav" and new["mirror"] == par["mirror"] == new["Ms"] // 2
    assert new["fed"] == [(0, 0), (1, 0), (1, 1)] and par["fed"] == [(0, 0), (0, 1), (1, 1)]
    assert new["fills"] == par["fills"] == 2
    Ms, Msp = new["Ms"], new["Msp"]
    # both triangles of the sensor blocks are filled: the upper-right block is the transpose of the lower-left, bit for bit
    for r in (new, par):
        assert torch.equal(_bits(r["AkA"][:Ms, Msp:Msp + Ms]), _bits(r["AkA"][Msp:Msp + Ms, :Ms].t()))
    R = _whole(ref)
    top = float(R.abs().max())
    d_new, d_par = float((_whole(new) - R).abs().max()) / top, float((_whole(par) - R).abs().max()) / top
    ll = (slice(Msp, Msp + Ms), slice(0, Ms))
    print("64x48x64 AkA vs the N-deep GEMM / max|AkA|: magn %.3e, grav %.3e; cross block alone: magn %.3e, grav %.3e; magn vs grav %.3e"
          % (d_new, d_par, float((new["AkA"][ll] - R[ll]).abs().max()) / top, float((par["AkA"][ll] - R[ll]).abs().max()) / top,
             float((_whole(new) - _whole(par)).abs().max()) / top))
    e_new = [normwise(new["cubes"][i], ref["cubes"][i]) for i in COMPUTED] + [abs(new["logl"] - ref["logl"]) / abs(ref["logl"])]
    e_par = [normwise(par["cubes"][i], ref["cubes"][i]) for i in COMPUTED] + [abs(par["logl"] - ref["logl"]) / abs(ref["logl"])]
    e_np = [normwise(new["cubes"][i], par["cubes"][i]) for i in COMPUTED] + [abs(new["logl"] - par["logl"]) / abs(par["logl"])]
    fmt = lambda e: " ".join("%.2e" % v for v in e)
    print("64x48x64 cubes (mean 0, mean 1, var 0, var 1), logl: magn vs GEMM %s | grav vs GEMM %s | magn vs grav %s" % (fmt(e_new), fmt(e_par), fmt(e_np)))
    # A K read through the completion hook: the three blocks the buffer owes its readers, against the parent's storing product
    e_ak = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(new["ak"], par["ak"]))
    new["ak"] = par["ak"] = None                                             # (the device copies: not kept for the session)
    gc.collect()
    torch.cuda.empty_cache()
    print("64x48x64 A K blocks (0,0), (0,1), (1,1) read afterwards, magn vs grav: %.2e" % e_ak)
    assert 0.0 < d_par and d_new <= 2.0 * d_par
    for a, b, c in zip(e_new, e_par, e_np):
        assert a <= 2.0 * b and c <= 3.0 * b
    assert e_ak <= 1e-13


def test_refused_mirror_leaves_the_parents_step():
    """The field (0.3, 0.2, 0.9): the magnetic operator is not its own point mirror, so `magn` has nothing to take and the two options
    run the same step, bit for bit."""
    new, par = _run(INCLINED, "magn"), _run(INCLINED, "grav")
    assert new["route"] == par["route"] and new["mirror"] == par["mirror"] == 0
    assert new["cross"] == par["cross"] == "grav" and new["fed"] == par["fed"] and new["fills"] == par["fills"]
    for i in COMPUTED:
        assert np.array_equal(new["cubes"][i], par["cubes"][i])
    assert new["logl"] == par["logl"] and torch.equal(_bits(new["AkA"]), _bits(par["AkA"]))


def test_default_step_at_64_cube_takes_the_new_plan_inside_the_contract():
    """64^3 (the headline configuration, default options): the step takes the cross block from the magnetic rows; mean and variance at
    the 3078 voxels of the independent oracle sample stay inside the 1e-8 contract.  The figures of a `grav` step are printed beside
    them.  Measured on one MI355X: mean 2.07e-12 / 1.19e-12 normwise, variance 1.82e-13 / 1.37e-14, log-likelihood 0.0 (the `grav`
    step: 2.06e-12 / 1.18e-12, 1.82e-13 / 1.35e-14, 1.2e-16)."""
    from geobo_amd.config_loader import Settings
    from geobo_amd.inversion import Inversion
    f = load_golden("oracle64_sample_matern32.npz")
    nx, ny, nz = (int(v) for v in f["dims"])
    n, N, q = nx, nx * ny * nz, f["voxels"]
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc="matern32"))
    d0 = np.zeros(N)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(ny, nx, nz)
    got = {}
    for opt in (None, "grav"):
        with _Env(**({} if opt is None else dict(GEOBO_CROSS_ROWS=opt))):
            inv = Inversion(settings=s, props=(0, 1))
            inv.gp_length = f["gp_length_in"].copy()
            inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
            step = inv.engine.last["step"]
            var = inv.cov_rec.diagonal()
            got[opt] = dict(cross=step.cross_rows, fed=sorted(step.gram_S), mirror=step.mirror,
                            e_mu=[normwise(inv.mu_rec[j * N + q], f["mu"][j]) for j in (0, 1)],
                            e_var=[float(np.abs(var[j * N + q] - f["var"][j]).max()) for j in (0, 1)],
                            e_logl=abs(inv.logl - float(f["logl"])) / abs(float(f["logl"])))
        del inv, step, var
        gc.collect()
        torch.cuda.empty_cache()
    for opt, g in got.items():
        print("64^3 [GEOBO_CROSS_ROWS=%s -> %s] vs the independent oracle sample: mean %s (normwise), variance %s (abs), logl %.2e"
              % (opt or "default", g["cross"], " ".join("%.2e" % e for e in g["e_mu"]), " ".join("%.2e" % e for e in g["e_var"]), g["e_logl"]))
    new, par = got[None], got["grav"]
    assert new["cross"] == "magn" and new["mirror"] == 2048 and new["fed"] == [(0, 0), (1, 0), (1, 1)]
    assert par["cross"] == "grav" and par["fed"] == [(0, 0), (0, 1), (1, 1)]
    assert max(new["e_mu"]) <= 1e-8 and max(new["e_var"]) <= 1e-8 and new["e_logl"] <= 1e-8
