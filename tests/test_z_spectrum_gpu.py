"""Rows of L^-1 A enter the posterior's covariance product as spectra (spectral.ConvolvedRows, GEOBO_Z_SPECTRUM): the product takes z as
its Toeplitz axis and the (iy, ix) plane the lattice convolution produces per (row, iz) goes through the product's forward transform
inside the same kernel -- Z in the voxel domain never exists.  Against the stored rows (TransposedPosteriorMixin._lattice_Z(...,
zx=True) + reduce_ss) on the same engine, against (L A) K evaluated from the covariance itself at sampled voxels, and one whole
64^3 step with the switch on and off.  The zx form exists for nx = ny = nz = 64 only."""
import gc

import numpy as np
import pytest
import torch

from conftest import normwise, settings_for

pytestmark = pytest.mark.gpu

n = 64


def _rand(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).cuda()


def _drop(*objs):
    del objs
    gc.collect()
    torch.cuda.empty_cache()


def test_reduce_ss_with_convolved_rows():
    """5 one-term rows and 5 two-term rows (m_first = 5, Mg = 10) in batches of 4 -- ragged, never straddling m_first."""
    from geobo_amd.engine import PosteriorEngine, weight_matrix
    from geobo_amd.spectral import SpectralProduct
    from geobo_amd.step import Prior
    s = settings_for(n, n, n)
    eng = PosteriorEngine(s, operators="resident")
    xe, ye, ze = eng.node_axes()
    X, Y = np.meshgrid(0.5 * (xe[:-1] + xe[1:]), 0.5 * (ye[:-1] + ye[1:]))
    loc = np.c_[X.ravel(), Y.ravel(), np.full(n * n, s.zmax + s.zoff)]
    N, Ms, Mg, m_first = n * n * n, n * n, 10, 5
    A_g = eng.operator("grav", loc, B=s.magneticField * 0.0)
    A_m = eng.operator("magn", loc, B=s.magneticField)
    gram = eng._gram
    assert gram.edge_supported() and gram.zx_supported()
    L = _rand((Mg + 1, 2 * Ms + 512), 91)[:Mg]
    L[:4, 1000:Ms] = 0.0                                                         # (a triangular corner like L^-1's)
    L[:8, Ms + 2000:] = 0.0
    Lg, Lm = L[:Mg, :Ms], L[m_first:Mg, Ms:2 * Ms]
    sp = SpectralProduct(n, n, n, "cuda", rows_per_batch=4, forms=eng._spectral_product().forms)
    f = sp.forms
    assert sp.R == 4 and sp.fused_ss() and f.z_mul and sp.y_mfma and f.y_two_term == "y2t"
    prior = Prior(s.kernelfunc, [200.0, 210.0, 220.0], weight_matrix(s.gp_coeff), 1.0)
    props = (0, 1)
    cubes = lambda: [torch.zeros((sp.ss_slots(), n, n * n), dtype=torch.float64, device="cuda") for _ in props]

    # today's path: rows stored as [iy][iz][ix], tables of transposed planes, y the Toeplitz axis
    Zg = torch.empty((Mg, N + 16), dtype=torch.float64, device="cuda")[:, :N]
    Zm = torch.empty((Mg - m_first, N + 16), dtype=torch.float64, device="cuda")[:, :N]
    eng._lattice_Z(Lg, Mg, "grav", A_g, Zg, zx=True)
    eng._lattice_Z(Lm, Mg - m_first, "magn", A_m, Zm, zx=True)
    swap = lambda g: g.view(n, sp.Px, sp.Pz).transpose(1, 2).contiguous().view(-1)
    tg, tm = ([swap(sp.eigenvalues(prior.table(eng, s_, j))) for j in props] for s_ in (0, 1))
    ss_ref = cubes()
    sp.reduce_ss(Zg, Mg, tg, Zm, m_first, tm, ss_ref, y2s=sp.y2s_tables(tg, tm))
    ref = [t.sum(0).view(n, n, n).transpose(1, 2).reshape(-1) for t in ss_ref]

    # the rows as spectra: z the Toeplitz axis, cubes come back as [iz][iy][ix]
    Cg, Cm = eng._convolved_rows(Lg, Mg, "grav", A_g), eng._convolved_rows(Lm, Mg - m_first, "magn", A_m)
    tgz, tmz = ([sp.eigenvalues(prior.table(eng, s_, j), toeplitz_z=True) for j in props] for s_ in (0, 1))
    ss_new = cubes()
    sp.reduce_ss(Cg, Mg, tgz, Cm, m_first, tmz, ss_new, y2s=sp.y2s_tables(tgz, tmz))
    new = [t.sum(0).view(n, n, n).permute(1, 2, 0).reshape(-1) for t in ss_new]
    for jj in range(len(props)):
        top = ref[jj].abs().max().item()
        err = (new[jj] - ref[jj]).abs().max().item() / top
        print("reduce_ss, block %d: convolved rows vs stored rows %.3e (max ss %.3e)" % (jj, err, top))
        assert top > 0.0 and err <= 1e-12

    # (L A) K from the covariance itself at sampled voxels: block (s, j)[:, sel] = block (j, s)[sel, :]^T
    g = torch.Generator(device="cpu").manual_seed(7)
    sel = torch.randperm(N, generator=g)[:300].sort().values.cuda()
    Zg_v, Zm_v = Lg @ A_g[:Ms, :N], Lm @ A_m[:Ms, :N]
    for jj, j in enumerate(props):
        K = torch.empty((sel.numel(), N), dtype=torch.float64, device="cuda")
        V = Zg_v @ eng._cov_rows(prior, j, 0, sel, 0, K).t()
        V[m_first:] += Zm_v @ eng._cov_rows(prior, j, 1, sel, 0, K).t()
        want = (V ** 2).sum(0)
        err = (new[jj][sel] - want).abs().max().item() / ref[jj].abs().max().item()
        print("reduce_ss, block %d: convolved rows vs (L A) K at %d voxels %.3e" % (jj, sel.numel(), err))
        assert err <= 1e-12
    _drop(eng, A_g, A_m)


def _inversion(md):
    import bench
    from geobo_amd.inversion import Inversion
    s = settings_for(n, n, n, kernelfunc="matern32")
    inv = Inversion(settings=s, props=(0, 1))
    grav, mag, loc, drill0 = bench.synthetic_inputs(inv, md)
    inv.gp_length = np.array([200.0, 202.0, 204.0])
    return inv, (grav, mag, drill0[drill0 != 0], loc, drill0)


def test_step_with_the_switch_on_and_off(monkeypatch):
    """One 64^3 step with 5 drill voxels: cubes to 1e-13 normwise, the log-likelihood (which no row of V enters) exactly; with
    GEOBO_Z_SPECTRUM=0 the launches are the parent's: Zg is written by the product-input inverse and the fused entry is never called."""
    from geobo_amd import hip
    fused, inv_mul = hip.xz2d_fold_conv_fwd, hip.xz2d_fold_inv_mul
    calls, outs = [], []
    monkeypatch.setattr(hip, "xz2d_fold_conv_fwd", lambda *a: calls.append(1) or fused(*a))
    monkeypatch.setattr(hip, "xz2d_fold_inv_mul", lambda *a: outs.append(a[9].data_ptr()) or inv_mul(*a))

    monkeypatch.setenv("GEOBO_Z_SPECTRUM", "1")
    inv, args = _inversion(5)
    on = [np.array(c) for c in inv.cubing(*args)]
    logl = float(inv.logl)
    eng = inv.engine
    assert eng.z_spectrum_on and eng.step_route == "single" and eng.last["step"].Md == 5
    assert calls and "Zg" not in eng._ws and "Zslab_grav" in eng._ws       # the rows went in as spectra; Z was never allocated
    _drop(inv, eng)

    monkeypatch.setenv("GEOBO_Z_SPECTRUM", "0")
    calls.clear()
    outs.clear()
    inv, args = _inversion(5)
    off = [np.array(c) for c in inv.cubing(*args)]
    eng = inv.engine
    assert not eng.z_spectrum_on and not calls
    assert eng._ws["Zg"].data_ptr() in outs and eng._ws["Zm"].data_ptr() in outs and "Zslab_grav" not in eng._ws
    errs = [normwise(on[i], off[i]) for i in (0, 1, 3, 4)]
    print("64^3 step, 5 drill voxels, rows as spectra vs stored rows: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) <= 1e-13 and float(inv.logl) == logl
    _drop(inv, eng)
