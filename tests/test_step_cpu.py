"""geobo_amd/step.py, host side: the terms of a plain and of a derivative Prior (kernel ids of include/geobo_hip.h and weights) and the
defaults of a Step.  No GPU needed."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

W = [[1.0, 0.3, 0.7], [0.3, 1.0, 0.4], [0.7, 0.4, 1.0]]        # engine.weight_matrix([0.7, 0.4, 0.3])
LENGTHS = [200.0, 204.0, 208.0]
# family ids (hip.KERNEL_IDS): covariance self / cross, d/dl of the self family, d/dl1 and d/dl2 of the cross family
IDS = {"exp": (1, 2, 7, 8, 9), "matern32": (3, 4, 10, 11, 12), "sparse": (5, 6, 13, 14, 15)}


def test_step_module_needs_no_torch():
    r = subprocess.run([sys.executable, "-c", "import sys; import geobo_amd.step; assert 'torch' not in sys.modules"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("name", sorted(IDS))
def test_plain_prior_has_one_term_per_block(name):
    from geobo_amd.engine import weight_matrix
    from geobo_amd.step import Prior
    assert weight_matrix([0.7, 0.4, 0.3]) == W
    p = Prior(name, LENGTHS, W, 1.3)
    assert p.deriv is None and (p.name, p.lengths, p.W, p.amp) == (name, LENGTHS, W, 1.3)
    k_self, k_cross = IDS[name][:2]
    for i in range(3):
        for j in range(3):
            assert p.terms(i, j) == [(k_cross if i != j else k_self, W[i][j])]


@pytest.mark.parametrize("name", sorted(IDS))
@pytest.mark.parametrize("d", [(100.0, 102.0, 100.0), (1.0, 0.0, 0.0), (0.0, -2.5, 0.5)])
def test_derivative_prior_terms(name, d):
    """Block (i, j) = w_ij k(l1 = l_j, l2 = l_i): its derivative along d is w_ij (d_j dk/dl1 + d_i dk/dl2); a self block has one
    length: w d_j dk/dl.  A zero component of d keeps its term (weight 0): the launches do not depend on the direction."""
    from geobo_amd.step import Prior
    p = Prior(name, LENGTHS, W, 1.3, deriv=np.asarray(d))
    assert p.deriv == list(d) and all(type(v) is float for v in p.deriv)
    _, _, k_dl, k_dl1, k_dl2 = IDS[name]
    for i in range(3):
        for j in range(3):
            if i == j:
                assert p.terms(i, j) == [(k_dl, W[i][j] * d[j])]
            else:
                assert p.terms(i, j) == [(k_dl1, W[i][j] * d[j]), (k_dl2, W[i][j] * d[i])]


def test_unit_weight_pair_prior_keeps_zero_self_blocks():
    """logl_grad's Gram of the pairs whose weight is 0: a plain Prior whose weight matrix has 0 on the diagonal."""
    from geobo_amd.step import Prior
    Wu = [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    p = Prior("exp", LENGTHS, Wu, 1.0)
    assert p.terms(2, 2) == [(1, 0.0)] and p.terms(0, 2) == [(2, 1.0)] and p.terms(2, 0) == [(2, 1.0)]


def test_unknown_kernel_is_an_error():
    from geobo_amd.step import Prior
    with pytest.raises(ValueError):
        Prior("gauss", LENGTHS, W, 1.0).terms(0, 1)


def test_step_defaults():
    from geobo_amd.step import Prior, Step
    p = Prior("exp", LENGTHS, W, 1.0)
    a, b = Step(p, (0, 1, 2), None, 0, 512), Step(p, (0, 1), None, 0, 512, noise=[0.1, 0.1, 0.1])
    assert (a.ak_slot, a.aka_slot) == ("AK", "AkA")
    assert a.noise is None                 # a derivative Gram: no noise diagonal, zero padding
    assert b.noise == [0.1, 0.1, 0.1]
    assert not a.keep_signal and not a.sym and not a.rowpath
    assert a.gens == {} and a.fullrows == {} and a.gens is not b.gens and a.fullrows is not b.fullrows      # products are per step
    g = Step(p, (0, 1, 2), None, 0, 512, ak_slot="dK_AK", aka_slot="dK_dir0")
    assert (g.ak_slot, g.aka_slot, g.noise) == ("dK_AK", "dK_dir0", None)
