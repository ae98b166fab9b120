"""The drill rows of the transposed posterior (TransposedPosteriorMixin._drill_rows_ss): the short form -- sensor terms joined in the
y stage, drill term as an Md-deep product with the stored drill rows of A K, geobo_sumsq_accum -- against the three-product form it
replaces, which stays in the code for surveys off the lattice and serves as the reference here.  64 x 48 x 64 is the smallest grid whose
step runs the transposed posterior on the lattice (tests/test_aka_mirror_gpu.py).  Md = 5: a few rows of one tile; Md = 130: more than one
128-row tile, ragged."""
import gc

import numpy as np
import pytest
import torch

from conftest import normwise, settings_for

pytestmark = pytest.mark.gpu

SHAPE = (64, 48, 64)


def _inversion(md):
    import bench
    from geobo_amd.inversion import Inversion
    s = settings_for(*SHAPE, kernelfunc="matern32")
    inv = Inversion(settings=s, props=(0, 1))
    grav, mag, loc, drill0 = bench.synthetic_inputs(inv, md)
    inv.gp_length = np.array([200.0, 202.0, 204.0])
    return inv, (grav, mag, drill0[drill0 != 0], loc, drill0)


def _drop(*objs):
    del objs
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("md", [5, 130])
def test_short_form_against_the_three_products(md):
    inv, args = _inversion(md)
    inv.cubing(*args)
    eng = inv.engine
    last = eng.last
    step, Linv, (A_g, A_m) = last["step"], last["Linv"], last["ops"]
    AK = last["AK"] if last["AK"] is not None else last["AK_partial"]
    assert eng.step_route == "single" and step.Md == md
    Msp, P_c = eng.Ms_pad, len(step.props)
    assert eng._spectral.has_two_term_product(P_c)
    lattice_Z = lambda Lv, n, func, out: eng._lattice_Z(Lv, n, func, A_g if func == "grav" else A_m, out)
    Kd = [AK[2 * Msp:, jj * eng.nc:(jj + 1) * eng.nc] for jj in range(P_c)]
    new = eng._drill_rows_ss(step, Linv, 0, md, lattice_Z, None, None, Kd=Kd).clone()
    ref = eng._drill_rows_ss(step, Linv, 0, md, lattice_Z, None, None).clone()
    assert new.shape == ref.shape == (P_c, eng.N)
    err = float((new - ref).abs().max() / ref.abs().max())
    print("drill rows, Md = %d: short form vs three products %.2e (max sum %.3e)" % (md, err, float(ref.abs().max())))
    assert float(ref.abs().max()) > 0.0
    assert err <= 1e-12
    _drop(inv, eng, last)


def test_cubing_with_drill_voxels_against_the_long_way(monkeypatch):
    """One step with 5 drill voxels end to end, the short form against the same step with the drill rows sent the long way: cubes to
    1e-13 normwise, the log-likelihood (which no drill row of V enters) exactly."""
    from geobo_amd.spectral import SpectralProduct
    inv, args = _inversion(5)
    cubes = [np.array(c) for c in inv.cubing(*args)]
    logl = float(inv.logl)
    calls = []
    short = type(inv.engine)._drill_rows_ss_short
    monkeypatch.setattr(type(inv.engine), "_drill_rows_ss_short", lambda self, *a: calls.append(1) or short(self, *a))
    inv.cubing(*args)
    assert calls                                                        # the step does take the short form
    monkeypatch.setattr(SpectralProduct, "has_two_term_product", lambda self, nblocks: False)
    calls.clear()
    long_way = [np.array(c) for c in inv.cubing(*args)]
    assert not calls
    errs = [normwise(cubes[i], long_way[i]) for i in (0, 1, 3, 4)]
    print("cubing, 5 drill voxels, short form vs long way: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) <= 1e-13 and float(inv.logl) == logl
    _drop(inv)
