"""Log-likelihood gradient, host side: the new C-ABI entries (declared, bound, exported, argument checks before any device access),
the derivative covariance ids of hip.kernel_id and the chain rule between the reference's 5-parameter objective and the
7-parameter form.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("geobo_kinv_dot", "geobo_kinv_dot_ws_bytes")


@pytest.fixture(scope="module")
def lib():
    from geobo_amd import _lib
    from geobo_amd.build import build
    build()
    return _lib.load()


def test_new_symbols_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "geobo_hip.h")).read(), flags=re.S)
    from geobo_amd import _lib
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(lib, n), n


def test_kinv_dot_rejects_bad_arguments_without_a_device(lib):
    fake = C.c_void_p(4096)                  # never dereferenced: every check comes first
    seg = (C.c_int64 * 6)(0, 100, 256, 356, 512, 520)
    G = (C.c_void_p * 1)(4096)
    ws = lib.geobo_kinv_dot_ws_bytes(768, 1)
    assert ws == (6 * 7 // 2) * 1 * 6 * 8
    assert lib.geobo_kinv_dot_ws_bytes(300, 1) == 0 and lib.geobo_kinv_dot_ws_bytes(768, 5) == 0
    call = lambda m, L, a, T, g, sg, out, w, wsb: lib.geobo_kinv_dot(m, L, m, a, T, g, m, sg, out, w, wsb, None)
    assert call(768, None, fake, 1, G, seg, fake, fake, ws) == -1              # null Linv
    assert call(768, fake, None, 1, G, seg, fake, fake, ws) == -1              # null alpha
    assert call(768, fake, fake, 1, None, seg, fake, fake, ws) == -1           # null G array
    assert call(768, fake, fake, 1, (C.c_void_p * 1)(0), seg, fake, fake, ws) == -1   # null G[0]
    assert call(768, fake, fake, 1, G, None, fake, fake, ws) == -1             # null segments
    assert call(768, fake, fake, 1, G, seg, None, fake, ws) == -1              # null out
    assert call(768, fake, fake, 1, G, seg, fake, None, ws) == -1              # null workspace
    assert call(700, fake, fake, 1, G, seg, fake, fake, ws) == -1              # m not a multiple of 256
    assert call(768, fake, fake, 0, G, seg, fake, fake, ws) == -1              # T out of 1..4
    assert call(768, fake, fake, 5, G, seg, fake, fake, ws) == -1
    assert call(768, fake, fake, 1, G, seg, fake, fake, ws - 8) == -1          # workspace too small
    assert call(768, C.c_void_p(4104), fake, 1, G, seg, fake, fake, ws) == -1  # Linv not 16-byte aligned
    for bad in ((0, 100, 200, 356, 512, 520),      # segment start not a multiple of 256
                (0, 300, 256, 356, 512, 520),      # overlapping segments
                (0, 100, 256, 356, 512, 800),      # past m
                (256, 300, 0, 100, 512, 520)):     # out of order
        assert call(768, fake, fake, 1, G, (C.c_int64 * 6)(*bad), fake, fake, ws) == -1, bad


def test_kernel_id_derivatives():
    from geobo_amd import hip
    assert hip.kernel_id("exp", False) == 1 and hip.kernel_id("sparse", True) == 6      # unchanged
    assert [hip.kernel_id(n, False, 1) for n in ("exp", "matern32", "sparse")] == [7, 10, 13]
    assert [hip.kernel_id(n, True, d) for n in ("exp", "matern32", "sparse") for d in (1, 2)] == [8, 9, 11, 12, 14, 15]
    assert hip.KERNEL_IDS["matern32_x_dl2"] == 12 and len(set(hip.KERNEL_IDS.values())) == len(hip.KERNEL_IDS) == 16
    for bad in (0, 3, True, "1", 1.5):
        with pytest.raises(ValueError):
            hip.kernel_id("exp", True, bad)
    with pytest.raises(ValueError):
        hip.kernel_id("exp", False, 2)          # a self family has one length
    with pytest.raises(ValueError):
        hip.kernel_id("gauss", True, 1)


def test_five_to_seven_chain_rule():
    """calc_logl_grad's length component is ONE directional derivative along d = xvox (1, 1.02, 1): the Jacobian of create_cov's
    mutation of l xvox (1, 1, 1).  Against central differences of the mutation itself, and the 5-gradient as d . (7-gradient)."""
    from geobo_amd.engine import create_cov_lengths
    from geobo_amd.inversion import reference_length_direction
    xvox = 125.0
    d = reference_length_direction(xvox)
    assert np.array_equal(d, xvox * np.array([1.0, 1.02, 1.0]))
    for l in (0.5, 2.0, 7.3):
        h = 1e-6 * l
        jac = (create_cov_lengths((l + h) * np.full(3, xvox)) - create_cov_lengths((l - h) * np.full(3, xvox))) / (2 * h)
        assert np.allclose(jac, d, rtol=1e-8, atol=0)
    g7 = np.array([0.3, -1.5e-3, 2.0e-3, 4.0e-4, 1.1, -0.2, 0.05])        # (amp, l0, l1, l2, w1, w2, w3)
    g5 = np.r_[g7[0], d @ g7[1:4], g7[4:]]
    assert g5[1] == pytest.approx(xvox * (g7[1] + 1.02 * g7[2] + g7[3]), rel=1e-15)


def test_optimize_gp_method_selection(monkeypatch):
    """optimize_gp() keeps the reference's signature and runs SHGO unless the settings carry optimize_method: "L-BFGS-B"."""
    import scipy.optimize
    from scipy.optimize import OptimizeResult
    from conftest import settings_for
    from geobo_amd.inversion import Inversion
    used = []
    monkeypatch.setattr(scipy.optimize, "shgo", lambda *a, **k: used.append("shgo") or OptimizeResult(success=False, message="stub"))
    monkeypatch.setattr(Inversion, "_optimize_lbfgsb", lambda self, free: used.append(("L-BFGS-B", free)))
    for settings, want in ((settings_for(10, 8, 6), "shgo"), (settings_for(10, 8, 6, optimize_method="L-BFGS-B"), ("L-BFGS-B", False))):
        inv = Inversion(settings=settings)
        inv.gravfield = inv.magfield = inv.drillfield = np.ones(4)
        used.clear()
        inv.optimize_gp()
        assert used == [want]
    used.clear()
    inv.optimize_hyperparameters(method="L-BFGS-B", free_lengths=True)
    assert used == [("L-BFGS-B", True)]
    with pytest.raises(ValueError):
        inv.optimize_hyperparameters(method="SLSQP")
    with pytest.raises(ValueError):
        inv.optimize_hyperparameters(method="shgo", free_lengths=True)
