"""The lattice Gram fed with x-analysed rows ("x step in the A K inverse"), by value.  GPU only.

  geobo_xz2d_fold_inv_gx   the storing inverse transform whose interior planes also leave as GX[o][z] = sum_x G_x[o][x] X[x][z]:
                           what it stores of the rows equals geobo_xz2d_fold bit for bit (all planes, or only the two boundary planes
                           of a row), GX against torch on the stored planes, untouched slots keep their NaN fill
  geobo_gram_yz            y step + eigenvalue scaling + channel sum on GX against torch and against the pair of launches it replaces
                           (geobo_ymul_fold + geobo_xcorr_reduce_fold on the rows themselves)
  whole steps              64 x 48 x 64 with the hand-over against GEOBO_GRAM_GX=0; 64 x 16 x 64 (no symmetric plan) is untouched

Bounds.  The new kernels form the sums of the launches they replace in another order, so each may deviate from the float64 torch
reference by at most TWICE what the replaced launch deviates by on the same data (both relative to the largest reference entry;
both figures are printed, DESIGN.md section 2 quotes them).  The kernels exist for 64 x 64 planes only: small means few rows and planes."""
import gc
import os

import numpy as np
import pytest
import torch

from conftest import normwise, settings_for

pytestmark = pytest.mark.gpu

F64 = torch.float64
N, P = 64, 128
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from geobo_amd import hip as h
    h.require_gpu()
    return h


@pytest.fixture(scope="module")
def mats(hip):
    from geobo_amd.spectral import folded_matrices, forward_matrix
    return torch.from_numpy(forward_matrix(N)).cuda(), hip.to_dev(np.stack(folded_matrices(N), axis=2))


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=F64) * 2 - 1).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---- geobo_xz2d_fold_inv_gx -------------------------------------------------------------------------------------------------------------
_INV = {}


def _inverse_runs(hip, F, ny):
    """Mode 0 and the two store modes of the new one on the same random spectra (R = 3 rows of ny planes), once per ny."""
    if ny in _INV:
        return _INV[ny]
    R = 3
    S = _rand((R, ny, P, P), 300 + ny)
    X0 = torch.full((R, ny, N, N), NAN, dtype=F64, device="cuda")
    hip.xz2d_fold(True, N, R, ny, S, ny * P * P, P * P, F, F, X0, ny * N * N, N * N)
    runs = {}
    for store_all in (True, False):
        X = torch.full((R, ny, N, N), NAN, dtype=F64, device="cuda")
        GX = torch.full((R * ny * P * N + 4096,), NAN, dtype=F64, device="cuda")
        hip.xz2d_fold_inv_gx(N, R, ny, S, ny * P * P, P * P, F, F, X, ny * N * N, N * N, store_all, GX, ny * P * N, P * N)
        torch.cuda.synchronize()
        assert bool(torch.isnan(GX[R * ny * P * N:]).all())                  # nothing behind the last plane
        runs[store_all] = (X, GX[:R * ny * P * N].view(R, ny, P, N))
    _INV[ny] = (X0, runs)
    return _INV[ny]


@pytest.mark.parametrize("ny", [4, 48])
def test_inverse_gx_stores_the_rows_of_mode_0_bit_for_bit(hip, mats, ny):
    _, F = mats
    X0, runs = _inverse_runs(hip, F, ny)
    assert not bool(torch.isnan(X0).any())
    X_all, X_edge = runs[True][0], runs[False][0]
    assert torch.equal(_bits(X_all), _bits(X0))
    for y in (0, ny - 1):
        assert torch.equal(_bits(X_edge[:, y]), _bits(X0[:, y]))
    assert bool(torch.isnan(X_edge[:, 1:ny - 1]).all())                      # the interior planes were not touched


@pytest.mark.parametrize("ny", [4, 48])
def test_inverse_gx_x_analysis_against_torch_and_xcorr(hip, mats, ny):
    """GX of the interior planes against G_x X in torch on the planes mode 0 stored.  The yardstick is the x analysis of
    geobo_xcorr_reduce_fold on the same planes, read out with one-hot eigenvalues: every stored plane is one "row" of that kernel, its
    64 "planes" all point at it (plane stride 0) and plane p scales channel z = p by one and the others by zero, so out[.][p][o] is its
    D[o][z = p] exactly."""
    G, F = mats
    X0, runs = _inverse_runs(hip, F, ny)
    R = X0.shape[0]
    ref = torch.einsum("ox,ryxz->ryoz", G, X0)[:, 1:ny - 1]
    top = ref.abs().max().item()
    for store_all in (True, False):
        GX = runs[store_all][1]
        assert bool(torch.isnan(GX[:, 0]).all()) and bool(torch.isnan(GX[:, ny - 1]).all())      # skipped boundary planes: the NaN fill
        assert not bool(torch.isnan(GX[:, 1:ny - 1]).any())
    onehot = torch.zeros((N, N, P), dtype=F64, device="cuda")                  # lamT[p][z][o]
    onehot[torch.arange(N), torch.arange(N), :] = 1.0
    Xp = X0.reshape(R * ny, N * N)
    out = torch.empty((R * ny, N, P), dtype=F64, device="cuda")
    hip.xcorr_reduce_fold(N, R * ny, N, Xp, N * N, 0, F, onehot.view(-1), out, N * P, P)
    xc = out.view(R, ny, N, P).transpose(2, 3)[:, 1:ny - 1]                    # [r][y][o][z]
    e_xc = (xc - ref).abs().max().item() / top
    e_gx = max((runs[sa][1][:, 1:ny - 1] - ref).abs().max().item() / top for sa in (True, False))
    print("inv_gx ny = %d: GX vs torch %.3e, xcorr_fold4's x analysis vs torch %.3e, GX vs xcorr %.3e"
          % (ny, e_gx, e_xc, (runs[True][1][:, 1:ny - 1] - xc).abs().max().item() / top))
    assert 0.0 < e_xc <= 1e-13                                               # (the yardstick itself is sound: 64 fp64 terms per sum)
    assert e_gx <= 2.0 * e_xc
    assert torch.equal(_bits(runs[True][1][:, 1:ny - 1]), _bits(runs[False][1][:, 1:ny - 1]))   # the store mode does not reach GX


# ---- geobo_gram_yz ----------------------------------------------------------------------------------------------------------------------
def _gy0(ny):
    """(128 x 64) pair-interleaved y matrix with the boundary columns zeroed (what LatticeGram.Gy0 is), columns scaled so that a swapped
    or transposed fragment shows; rows >= 2 ny and columns >= ny are zero (geobo_ymul_fold wants m = 128, k = 64)."""
    from geobo_amd.spectral import forward_matrix
    g = forward_matrix(ny) * (1.0 + 0.01 * np.arange(ny))[None, :]
    g[:, 0] = 0.0
    g[:, ny - 1] = 0.0
    full = np.zeros((128, 64))
    full[:2 * ny, :ny] = g
    return torch.from_numpy(full).cuda()


@pytest.mark.parametrize("R,ny", [(1, 48), (5, 48), (1, 64), (5, 64)])
def test_gram_yz_against_torch_and_the_pair(hip, mats, R, ny):
    Gx, F = mats
    Py = 2 * ny
    X = _rand((R, 64, N, N), 500 + R + ny)                                   # rows y >= ny meet zero columns of the y matrix
    GX = torch.einsum("ox,ryxz->ryoz", Gx, X).contiguous()                    # [r][y][o][z]
    Gy = _gy0(ny)
    lamT = _rand((Py, N, P), 600 + ny)                                       # [ky][z][o]: what geobo_xcorr_reduce_fold reads
    lam_oz = lamT.transpose(1, 2).contiguous()                                # [ky][o][z]: what geobo_gram_yz reads
    ref = torch.einsum("koz,ky,ryoz->rko", lam_oz, Gy[:Py, :ny], GX[:, :ny])
    top = ref.abs().max().item()
    # the pair on the rows themselves: y step into the y spectrum, then x step + scaling + channel sum
    Y1 = torch.empty((R, 128, N * N), dtype=F64, device="cuda")
    hip.ymul(128, 64, N * N, R, Gy, X.view(R, -1), 64 * N * N, Y1, 128 * N * N, fold=True)
    s_pair = torch.empty((R, Py, P), dtype=F64, device="cuda")
    hip.xcorr_reduce_fold(N, R, Py, Y1, 128 * N * N, N * N, F, lamT.view(-1), s_pair, Py * P, P)
    # the new kernel: rows beyond R, the padding between y-modes (s_plane > 128) and behind a row (s_row > Py * s_plane) keep their bits
    sp_, sr_ = P + 8, Py * (P + 8) + 24
    s = torch.full((R + 2, sr_), NAN, dtype=F64, device="cuda")
    hip.gram_yz(N, ny, R, GX[:, :ny].contiguous(), ny * P * N, P * N, Gy[:, :ny].contiguous(), lam_oz.view(-1), s, sr_, sp_)
    torch.cuda.synchronize()
    body = s[:R, :Py * sp_].view(R, Py, sp_)
    got = body[:, :, :P]
    assert not bool(torch.isnan(got).any())
    assert bool(torch.isnan(body[:, :, P:]).all()) and bool(torch.isnan(s[:R, Py * sp_:]).all()) and bool(torch.isnan(s[R:]).all())
    e_new, e_pair = (got - ref).abs().max().item() / top, (s_pair - ref).abs().max().item() / top
    print("gram_yz R = %d, ny = %d: vs torch %.3e, ymul + xcorr vs torch %.3e, vs the pair %.3e"
          % (R, ny, e_new, e_pair, (got - s_pair).abs().max().item() / top))
    assert 0.0 < e_pair <= 1e-12                                             # (three contractions of 64 fp64 terms)
    assert e_new <= 2.0 * e_pair


def test_gram_yz_refuses_bad_arguments(hip):
    """Null pointers, a misaligned GX, odd strides: GEOBO_E_ARG (-1), and nothing is launched (the result buffer keeps its fill)."""
    from geobo_amd import _lib
    L = _lib.load()
    ny, R = 48, 1
    gx = _rand((R * ny * P * N + 2,), 1)
    Gy, lam = _gy0(ny)[:, :ny].contiguous(), _rand((2 * ny * P * N,), 2)
    s = torch.full((R * 2 * ny * P,), NAN, dtype=F64, device="cuda")
    p = lambda t: t.data_ptr()
    ok = [N, ny, R, p(gx), ny * P * N, P * N, p(Gy), ny, p(lam), p(s), 2 * ny * P, P, None]
    bad = {"null gx": {3: None}, "null G": {6: None}, "null lam": {8: None}, "null s": {9: None}, "misaligned gx": {3: p(gx) + 8},
           "odd row stride": {4: ny * P * N + 1}, "odd plane stride": {5: P * N + 1}, "short plane stride": {5: P * N - 2},
           "odd ny": {1: 47}, "short s_plane": {11: P - 1}}
    for what, change in bad.items():
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert L.geobo_gram_yz(*args) == -1, what
    torch.cuda.synchronize()
    assert bool(torch.isnan(s).all())
    assert L.geobo_gram_yz(*ok) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(s).any())


# ---- whole steps ------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _run(shape, on):
    """One cubing step (Matern-3/2, vertical field, 5 drill voxels, two property blocks) with the hand-over switched on / off."""
    key = (shape, on)
    if key in _RUNS:
        return _RUNS[key]
    import bench
    from geobo_amd.inversion import Inversion
    before = os.environ.get("GEOBO_GRAM_GX")
    os.environ["GEOBO_GRAM_GX"] = "1" if on else "0"
    try:
        s = settings_for(*shape, kernelfunc="matern32", XMAG=0, YMAG=0, ZMAG=1)
        inv = Inversion(settings=s, props=(0, 1))
        grav, mag, loc, drill0 = bench.synthetic_inputs(inv, 5)
        inv.gp_length = np.array([200.0, 202.0, 204.0])
        keep = {}
        inv.engine.aka_hook = lambda AkA: keep.__setitem__("AkA", AkA.clone())
        cubes = inv.cubing(grav, mag, drill0[drill0 != 0], loc, drill0)
        eng = inv.engine
        step = eng.last["step"]
        hook = eng.last.complete is not None
        AK = eng.last["AK"] if eng.last["AK_complete"] else eng.last["AK_partial"]
        Ms, Msp, nc, mirror = eng.Ms, eng.Ms_pad, eng.nc, step.mirror
        # the blocks of A K the symmetric plan computes (sensor rows; the mirrored magnetic rows come from the completion hook)
        ak = None
        if step.sym:
            ak = [AK[0:Ms, 0:eng.N].clone(), AK[0:Ms, nc:nc + eng.N].clone(), AK[Msp:Msp + Ms, nc:nc + eng.N].clone()]
        res = dict(cubes=[np.array(c) for c in cubes], logl=float(inv.logl), AkA=keep["AkA"], route=eng.step_route, fed=sorted(step.gram_S), ak=ak,
                   hook=hook, fills=len(step.ak_fill))
    finally:
        if before is None:
            os.environ.pop("GEOBO_GRAM_GX", None)
        else:
            os.environ["GEOBO_GRAM_GX"] = before
    del inv, eng, step, AK
    gc.collect()
    torch.cuda.empty_cache()
    _RUNS[key] = res
    return res


COMPUTED = (0, 1, 3, 4)          # mean and variance cubes of the two computed property blocks


def test_step_with_the_hand_over_against_the_stored_y_spectrum():
    """64 x 48 x 64: the three blocks of the symmetric plan reach the Gram x-analysed; AkA agrees with the ymul / xcorr form to 1e-12
    max|AkA|, cubes and log-likelihood to 1e-13 (the project's figures for alternative Gram forms).  The step stored only the boundary
    planes of those rows; read through engine.last["AK_partial"] afterwards, the blocks equal the other run's stored A K to 1e-13."""
    on, off = _run((64, 48, 64), True), _run((64, 48, 64), False)
    assert on["route"] == off["route"] == "single"
    assert on["fed"] == [(0, 0), (0, 1), (1, 1)] and off["fed"] == []
    assert on["hook"] and on["fills"] == 2 and off["fills"] == 0             # one storing product per operator waits behind AK_partial
    e_aka = float((on["AkA"] - off["AkA"]).abs().max() / off["AkA"].abs().max())
    errs = [normwise(on["cubes"][i], off["cubes"][i]) for i in COMPUTED]
    e_logl = abs(on["logl"] - off["logl"]) / abs(off["logl"])
    e_ak = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(on["ak"], off["ak"]))
    print("64x48x64 hand-over vs stored y spectrum: AkA %.2e of max|AkA|, cubes %s, logl %.2e, A K %.2e"
          % (e_aka, " ".join("%.2e" % e for e in errs), e_logl, e_ak))
    assert e_aka <= 1e-12
    assert max(errs) <= 1e-13
    assert e_logl <= 1e-13
    assert e_ak <= 1e-13


def test_grid_without_the_symmetric_plan_is_untouched():
    """64 x 16 x 64 runs as "columns": no symmetric plan, no hand-over, and the switch changes no bit."""
    on, off = _run((64, 16, 64), True), _run((64, 16, 64), False)
    assert on["route"] == off["route"] == "columns" and on["fed"] == off["fed"] == []
    for i in COMPUTED:
        assert np.array_equal(on["cubes"][i], off["cubes"][i])
    assert on["logl"] == off["logl"] and torch.equal(on["AkA"], off["AkA"])
