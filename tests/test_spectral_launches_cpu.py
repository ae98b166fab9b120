"""Which wrappers SpectralProduct calls, in which order and under which timer names, for every y-stage form the planner can choose:
the table of the product's dispatch, as test_route_table is the planner's.  spectral.py reaches the device through its module
attribute `hip` only, so a recorder in its place runs reduce_ss and product_two_term on the CPU (no kernel runs; buffers are never
read).  Sequences are collapsed: consecutive calls of one wrapper count once."""
import numpy as np
import pytest
import torch

from geobo_amd import hip as real_hip
from geobo_amd import plan, spectral

F64 = torch.float64
Y_WRAPPERS = ("toeplitz_y", "toeplitz_y2t", "toeplitz_y2s", "spectral_y", "spectral_y2s", "spectral_y3t", "spectral_y_lattice")


class Recorder:
    F64, pad_n = F64, staticmethod(real_hip.pad_n)

    def __init__(self):
        self.calls, self.timers = [], []

    def to_dev(self, a, device=None):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))

    def xz2d_fold_inv_ss_slots(self, n, rows, ppr):
        return 4

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **kw: self.calls.append(name)

    def timer(self, name, nbytes, fn, valu=0.0, flop=0.0):
        assert nbytes > 0 and flop >= valu > 0
        self.timers.append(name)
        return fn()


def collapse(seq):
    return [s for i, s in enumerate(seq) if i == 0 or s != seq[i - 1]]


def launches(monkeypatch, grid, env, nblocks):
    """(reduce_ss calls, its timer names, product_two_term calls or None, its timer names) for 5 rows of which 3 are two-term, R = 2."""
    rec = Recorder()
    monkeypatch.setattr(spectral, "hip", rec)
    nx, ny, nz = grid
    sp = spectral.SpectralProduct(nx, ny, nz, "cpu", rows_per_batch=2, forms=plan.stage_forms(nx, ny, nz, plan.switches(env)))
    sp.kernel_timer = rec.timer
    assert sp.R == 2
    N = nx * ny * nz
    ngen = ny * sp.Px * sp.Pz if sp.dense_y else sp.P3
    tg = [torch.rand(ngen, dtype=F64) for _ in range(nblocks)]
    tm = [tg[1].clone()] + [torch.rand(ngen, dtype=F64) for _ in range(nblocks - 1)]
    Zg, Zm = torch.zeros(5, N, dtype=F64), torch.zeros(3, N, dtype=F64)
    y2s = sp.y2s_tables(tg, tm)
    assert (y2s is not None) == sp.forms.y2s and (y2s is None or float(sp.sym_residual) == 0.0)
    ss = [torch.zeros(sp.ss_slots(), ny, nx * nz, dtype=F64) for _ in range(nblocks)]
    sp.reduce_ss(Zg, 5, tg, Zm, 2, tm, ss, y2s=y2s)
    reduce, reduce_t = rec.calls, rec.timers
    two = two_t = None
    if sp.has_two_term_product(nblocks):
        rec.calls, rec.timers = [], []
        sp.product_two_term(Zg, Zm, 2, tg, tm, [torch.zeros(2, N, dtype=F64) for _ in range(nblocks)], y2s=y2s)
        two, two_t = rec.calls, rec.timers
    return reduce, reduce_t, two, two_t


FWD, INV_SS = "xz2d_fold", "xz2d_fold_inv_ss"
NO_MFMA, NO_Y2S, BY_PASSES = {"GEOBO_Y_MFMA": "0"}, {"GEOBO_Y2S": "0"}, {"GEOBO_SPECTRAL_DENSE_Y": "0"}
Y, Y1, Y2T, Y2S = "kernel:toeplitz_y", "kernel:toeplitz_y_single", "kernel:toeplitz_y2t", "kernel:toeplitz_y2s"

# (grid, environment, blocks): reduce_ss per batch -- one one-term batch, then two two-term batches --, its timer names per batch,
# product_two_term (None: the grid has none for that many blocks), its timer names
TABLE = [
    ((64, 16, 64), {}, 2, ([FWD, "toeplitz_y", INV_SS],) * 3, ([Y], [Y, Y], [Y, Y]), None, None),
    ((64, 32, 64), {}, 2, ([FWD, "spectral_y", INV_SS],) + ([FWD, "spectral_y2s", INV_SS],) * 2, ([Y], [Y2S], [Y2S]),
     [FWD, "spectral_y2s", FWD], [Y2S]),
    ((64, 32, 64), NO_Y2S, 2, ([FWD, "spectral_y", INV_SS],) + ([FWD, "toeplitz_y2t", INV_SS],) * 2, ([Y], [Y2T], [Y2T]),
     [FWD, "toeplitz_y2t", FWD], [Y2T]),
    ((64, 32, 64), NO_MFMA, 3, ([FWD, "toeplitz_y", INV_SS, "toeplitz_y", INV_SS],) + ([FWD, "toeplitz_y2s", INV_SS, "toeplitz_y", INV_SS],) * 2,
     ([Y, Y1], [Y2S, Y1, Y1], [Y2S, Y1, Y1]), None, None),
    ((64, 80, 64), {}, 3, ([FWD, "spectral_y", INV_SS, "spectral_y", INV_SS],) * 3, ([Y, Y], [Y] * 4, [Y] * 4), [FWD, "spectral_y3t", FWD], [Y]),
    ((64, 80, 64), NO_MFMA, 2, ([FWD, "toeplitz_y", INV_SS],) * 3, ([Y], [Y, Y], [Y, Y]), [FWD, "toeplitz_y", FWD], [Y, Y]),
    ((16, 80, 16), {}, 2, (["axis_pass", "spectral_y", "axis_pass", "sumsq_accum"],) + (["axis_pass", "spectral_y3t", "axis_pass", "sumsq_accum"],) * 2,
     ([Y], [Y], [Y]), ["axis_pass", "spectral_y3t", "axis_pass"], [Y]),
    ((16, 16, 16), {}, 2, (["axis_pass", "toeplitz_y", "axis_pass", "sumsq_accum"],)
     + (["axis_pass", "toeplitz_y", "axis_pass", "toeplitz_y", "axis_pass", "sumsq_accum"],) * 2, ([Y], [Y, Y], [Y, Y]), None, None),
    # the stored reduction does not join the terms of a "y2t" grid (spectral.reduce_ss: inherited); its storing product does
    ((32, 32, 32), {}, 2, (["xz2d_fold_quad", "spectral_y", "xz2d_fold_quad", "sumsq_accum"],)
     + (["xz2d_fold_quad", "spectral_y", "xz2d_fold_quad", "spectral_y", "xz2d_fold_quad", "sumsq_accum"],) * 2, ([Y], [Y, Y], [Y, Y]),
     ["xz2d_fold_quad", "toeplitz_y2t", "xz2d_fold_quad"], [Y2T]),
]


@pytest.mark.parametrize("grid,env,nblocks,reduce,reduce_t,two,two_t", TABLE)
def test_launch_table(monkeypatch, grid, env, nblocks, reduce, reduce_t, two, two_t):
    got = launches(monkeypatch, grid, env, nblocks)
    assert collapse(got[0]) == collapse(sum(reduce, []))
    assert got[1] == sum(reduce_t, [])
    assert (collapse(got[2]) if got[2] is not None else None) == two
    assert got[3] == two_t


def test_y_stage_by_passes_has_no_y_kernel_and_no_timer(monkeypatch):
    reduce, reduce_t, two, _ = launches(monkeypatch, (16, 16, 16), BY_PASSES, 2)
    assert two is None and reduce_t == []
    assert set(reduce) == {"axis_pass", "gemm_batched", "scale_broadcast2", "sumsq_accum"}


def test_every_y_wrapper_has_one_call_site():
    import inspect
    import re
    src = inspect.getsource(spectral)
    for name in Y_WRAPPERS:
        assert len(re.findall(r"hip\.%s\b" % name, src)) == 1, name
