"""The hand-over of x-analysed rows from the A K product to the lattice Gram, as far as it is host logic: the gate (plan.feed_options,
plan.gram_gx_route), what SpectralProduct launches with a feed (a recorder in place of `hip`, as in test_spectral_launches_cpu.py) and
the bookkeeping of engine.last's completion hook.  No device."""
import dataclasses

import pytest
import torch

from geobo_amd import plan, spectral
from test_spectral_launches_cpu import Recorder

F64 = torch.float64


def test_feed_options_are_their_own_table():
    assert dataclasses.asdict(plan.feed_options({})) == dict(gram_gx=True) == dataclasses.asdict(plan.feed_options(None))
    assert plan.feed_options({"GEOBO_GRAM_GX": "0"}).gram_gx is False and plan.feed_options({"GEOBO_GRAM_GX": "1"}).gram_gx is True
    names = {v for v, _, _ in plan.FEED_OPTIONS.values()}
    assert not names & set(plan.SWITCHES.values()) and not names & {v for v, _, _ in plan.ENGINE_OPTIONS.values()}
    assert "gram_gx" not in plan.SWITCHES and "gram_gx" not in {f.name for f in dataclasses.fields(plan.Forms)}
    # the planner does not see the variable: route, switches and forms are what they are without it
    assert plan.plan_route(64, 64, 64, env={"GEOBO_GRAM_GX": "0"}) == plan.plan_route(64, 64, 64, env={})
    with pytest.raises(dataclasses.FrozenInstanceError):
        plan.feed_options({}).gram_gx = False


GATE = dict(family="single", sym=True, f32=False, world=1, exchange=False, nx=64, ny=64, nz=64)


@pytest.mark.parametrize("change,want", [({}, True), (dict(ny=48), True), (dict(ny=16), True), (dict(ny=80), False), (dict(nx=32, nz=32), False),
                                         (dict(nz=32), False), (dict(sym=False), False), (dict(family="rows"), False), (dict(family="columns"), False),
                                         (dict(f32=True), False), (dict(world=2), False), (dict(exchange=True), False)])
def test_gate(change, want):
    a = dict(GATE, **change)
    forms = plan.stage_forms(a["nx"], a["ny"], a["nz"])
    assert plan.gram_gx_route(plan.feed_options({}), forms=forms, **a) is want
    assert plan.gram_gx_route(plan.feed_options({"GEOBO_GRAM_GX": "0"}), forms=forms, **a) is False


@pytest.mark.parametrize("env", [{"GEOBO_XZ_FOLD": "0"}, {"GEOBO_SPECTRAL_FUSED_XZ": "0"}, {"GEOBO_SPECTRAL_DENSE_Y": "0"}])
def test_gate_follows_the_kernel_forms(env):
    forms = plan.stage_forms(64, 64, 64, plan.switches(env))
    assert plan.gram_gx_route(plan.feed_options({}), forms=forms, **GATE) is False


class Feed:
    def __init__(self, store_all):
        self.store_all, self.got = store_all, []

    def rows(self, jj, r0, R, GX):
        self.got.append((jj, r0, R, GX.data_ptr()))


@pytest.mark.parametrize("store_all", [True, False])
def test_product_with_a_feed_launches_the_gx_inverse(monkeypatch, store_all):
    """5 rows in batches of 2, two blocks: every (batch, block) is ONE geobo_xz2d_fold_inv_gx with the feed's store mode, the feed gets
    the batch buffer right behind it, and the plain storing inverse is not launched; without a feed the product is what it was."""
    calls = []

    class Rec(Recorder):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return lambda *a, **kw: calls.append((name, a))
    monkeypatch.setattr(spectral, "hip", Rec())
    nx, ny, nz = 64, 16, 64
    sp = spectral.SpectralProduct(nx, ny, nz, "cpu", rows_per_batch=2, forms=plan.stage_forms(nx, ny, nz))
    assert sp.R == 2 and sp.gx_applies()
    N = nx * ny * nz
    gens = [torch.rand(ny * sp.Px * sp.Pz, dtype=F64) for _ in range(2)]
    A, outs = torch.zeros(5, N, dtype=F64), [torch.zeros(5, N, dtype=F64) for _ in range(2)]
    feed = Feed(store_all)
    sp.product(A, 5, gens, outs, gx=feed)
    inv = [a for n, a in calls if n == "xz2d_fold_inv_gx"]
    assert len(inv) == 6 and not [a for n, a in calls if n == "xz2d_fold" and a[0]]
    gp = sp.Px * nz
    GX = sp.gx_buffer()
    for a, (jj, r0, R, ptr), want in zip(inv, feed.got, [(0, 0, 2), (1, 0, 2), (0, 2, 2), (1, 2, 2), (0, 4, 1), (1, 4, 1)]):
        assert (jj, r0, R) == want and ptr == GX.data_ptr()
        assert a[:3] == (nx, R, ny) and a[8].data_ptr() == outs[jj][r0:].data_ptr() and a[9:11] == (N, nx * nz)
        assert a[11] is store_all and a[12].data_ptr() == GX.data_ptr() and a[13:] == (ny * gp, gp)
    # the two boundary planes of every row of the batch buffer are zeroed once per allocation: the Gram's y step multiplies them by zero
    v = GX[:2 * ny * gp].view(2, ny, gp)
    assert float(v[:, 0].abs().max()) == 0.0 and float(v[:, ny - 1].abs().max()) == 0.0
    del calls[:]
    sp.product(A, 5, gens, outs)
    assert not [n for n, _ in calls if n == "xz2d_fold_inv_gx"] and len([a for n, a in calls if n == "xz2d_fold" and a[0]]) == 6


def test_feed_is_refused_where_the_kernel_does_not_exist(monkeypatch):
    monkeypatch.setattr(spectral, "hip", Recorder())
    sp = spectral.SpectralProduct(32, 32, 32, "cpu", rows_per_batch=2, forms=plan.stage_forms(32, 32, 32))
    assert not sp.gx_applies()
    N = 32 ** 3
    with pytest.raises(AssertionError):
        sp.product(torch.zeros(2, N, dtype=F64), 2, [torch.rand(32 * sp.Px * sp.Pz, dtype=F64)], [torch.zeros(2, N, dtype=F64)], gx=Feed(True))


def test_completion_hook_runs_the_fills_once_in_order_on_the_first_read():
    from geobo_amd.engine import _LastStep
    ran = []
    last = _LastStep(AK_partial="buffer", AK_complete=False, L="L")
    assert _LastStep.chain([]) is None
    last.complete = _LastStep.chain([lambda: ran.append("product (0)"), lambda: ran.append("product (1)"), lambda: ran.append("mirror")])
    assert last["L"] == "L" and last["AK_complete"] is False and ran == []       # other keys do not trigger it
    assert last["AK_partial"] == "buffer" and ran == ["product (0)", "product (1)", "mirror"]
    assert last["AK_partial"] == "buffer" and len(ran) == 3 and last.complete is None
    plain = _LastStep(AK_partial="b")
    assert plain["AK_partial"] == "b"                                            # a step that left nothing unwritten: no hook
