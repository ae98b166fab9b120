"""AkA's cross block from the mirrored half of the magnetic rows, as far as it is host logic: the gate
(plan.cross_options, plan.cross_rows_route) as a literal table, what the symmetric plan hands the spectral product and the lattice
Gram under either choice (recorders in place of the product, the Gram and `hip`, as in test_spectral_launches_cpu.py: no kernel runs,
buffers are never read), and the order of engine.last's completion hook.  No device."""
import dataclasses
import types

import pytest
import torch

from geobo_amd import engine as engine_mod
from geobo_amd import plan, transposed
from geobo_amd.engine import PosteriorEngine, _GramFeed, _LastStep
from geobo_amd.step import Step

F64 = torch.float64


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
def test_cross_options_are_their_own_table():
    assert dataclasses.asdict(plan.cross_options({})) == dict(cross_rows="auto") == dataclasses.asdict(plan.cross_options(None))
    for v in ("auto", "magn", "grav"):
        assert plan.cross_options({"GEOBO_CROSS_ROWS": v}).cross_rows == v
    with pytest.raises(ValueError):
        plan.cross_options({"GEOBO_CROSS_ROWS": "1"})
    names = {v for v, _, _ in plan.CROSS_OPTIONS.values()}
    others = set(plan.SWITCHES.values()) | {v for v, _, _ in plan.ENGINE_OPTIONS.values()} | {v for v, _, _ in plan.FEED_OPTIONS.values()}
    assert not names & others
    assert "cross_rows" not in plan.SWITCHES and "cross_rows" not in {f.name for f in dataclasses.fields(plan.Forms)}
    # the other tables and the planner are what they were
    assert dataclasses.asdict(plan.feed_options({})) == dict(gram_gx=True)
    assert plan.plan_route(64, 64, 64, env={"GEOBO_CROSS_ROWS": "grav"}) == plan.plan_route(64, 64, 64, env={})
    with pytest.raises(dataclasses.FrozenInstanceError):
        plan.cross_options({}).cross_rows = "grav"


CUBE, SLAB, SMALL = (64, 64, 64), (64, 48, 64), (32, 32, 32)
# option, symmetric plan, mirror rows, grid -> taken
GATE = [("auto", True, 2048, CUBE, True), ("auto", True, 1536, SLAB, False), ("auto", True, 512, SMALL, False),
        ("auto", True, 0, CUBE, False), ("auto", False, 2048, CUBE, False), ("auto", False, 0, CUBE, False),
        ("auto", True, 0, SLAB, False), ("auto", False, 1536, SLAB, False),
        ("magn", True, 2048, CUBE, True), ("magn", True, 1536, SLAB, True), ("magn", True, 512, SMALL, True),
        ("magn", True, 0, CUBE, False), ("magn", True, 0, SLAB, False), ("magn", False, 2048, CUBE, False), ("magn", False, 1536, SLAB, False),
        ("grav", True, 2048, CUBE, False), ("grav", True, 1536, SLAB, False), ("grav", True, 512, SMALL, False),
        ("grav", True, 0, CUBE, False), ("grav", False, 2048, CUBE, False), ("grav", False, 0, SLAB, False)]


@pytest.mark.parametrize("opt,sym,mirror,grid,want", GATE)
def test_gate(opt, sym, mirror, grid, want):
    assert plan.cross_rows_route(plan.cross_options({"GEOBO_CROSS_ROWS": opt}), sym, mirror, *grid) is want


def test_auto_is_the_default_and_the_cube_is_the_grid_of_forms_zx():
    assert plan.cross_rows_route(plan.cross_options({}), True, 2048, *CUBE) is True
    assert plan.cross_rows_route(plan.cross_options({}), True, 1536, *SLAB) is False
    assert plan.stage_forms(*CUBE).zx and not plan.stage_forms(*SLAB).zx


# ---- what the plan launches -------------------------------------------------------------------------------------------------------------
NX, NY, NZ = 4, 4, 2
MS, N, MM, PL = NX * NY, NX * NY * NZ, NX * NY // 2, NX * NZ


class Calls:
    """Records (name, positional arguments) of every method called on it."""

    def __init__(self, log, **fixed):
        self._log, self._fixed = log, fixed

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name in self._fixed:
            return self._fixed[name]
        return lambda *a, **kw: self._log.append((name, a, kw))


class FakePrior:
    def table(self, eng, s_, j):
        return ("table", s_, j)


def _engine(log, feed_on):
    """What _assemble_AK_spectral, _assemble_AkA_sym and _ak_completion read of an engine, on a 4 x 4 x 2 grid."""
    sp = Calls(log, R=MM, eigenvalues=lambda tab: ("gen",) + tab[1:], pool_applies=lambda: False, flops=lambda *a, **kw: 1.0,
               flops_valu=lambda *a, **kw: 1.0)
    gram = Calls(log, flops=lambda rows, ny=None: float(rows), flops_back=lambda rows: 1000.0 * rows, flops_gx=lambda rows: 1.0, Py=2 * NY, Px=2 * NX)
    A_g, A_m = torch.zeros(MS, N, dtype=F64), torch.zeros(MS, N, dtype=F64)
    eng = types.SimpleNamespace(nx=NX, ny=NY, nz=NZ, N=N, nc=N, c0=0, c1=N, Ms=MS, Ms_pad=MS, exchange=False, f32=False, _gram=gram,
                                _lam={"grav": (A_g, "lam_g"), "magn": (A_m, "lam_m")}, flops=[])
    eng._spectral_product = lambda: sp
    eng._timed = lambda name, fl, fn, **kw: (eng.flops.append((name, fl)), fn())[1]
    eng._edge_spectrum = lambda func, k, cols: ("edge", func, k)
    eng._finish_AkA = lambda step, AkA: AkA

    def gram_feed(step, s_, blocks):
        if not feed_on:
            return None
        S = [torch.zeros(MS * 4 * NX * NY, dtype=F64) for _ in blocks]
        for j, Sj in zip(blocks, S):
            step.gram_S[(s_, j)] = Sj
        return _GramFeed(gram, [("lam_g", "lam_m")[j] for j in blocks], S, store_all=False)
    eng._gram_feed = gram_feed
    return eng, A_g, A_m


def _step(cross):
    step = Step(FakePrior(), (0, 1), None, 0, 3 * MS, None, sym=True, mirror=MM)
    step.cross_rows = cross
    return step


def _assemble(monkeypatch, cross, feed_on):
    log = []
    monkeypatch.setattr(transposed, "hip", Calls(log))
    monkeypatch.setattr(engine_mod, "hip", Calls(log))
    eng, A_g, A_m = _engine(log, feed_on)
    step = _step(cross)
    AK, AkA = torch.zeros(3 * MS, 2 * N, dtype=F64), torch.zeros(3 * MS, 3 * MS, dtype=F64)
    PosteriorEngine._assemble_AK_spectral(eng, step, AK, A_g, A_m)
    products = [(a[0], a[1], a[2], [o.data_ptr() for o in a[3]], kw.get("gx") is not None) for n, a, kw in log if n == "product"]
    del log[:]
    PosteriorEngine._assemble_AkA_sym(eng, step, AkA, AK, A_g, A_m)
    gram_calls = list(log)
    del log[:]
    return eng, step, AK, AkA, (A_g, A_m), products, gram_calls, log


G = lambda s_, j: ("gen", s_, j)
ptr = lambda AK, r0, jj: AK[r0:, jj * N:].data_ptr()


@pytest.mark.parametrize("feed_on", [True, False])
def test_magnetic_rows_run_both_blocks_and_gravity_rows_one(monkeypatch, feed_on):
    eng, step, AK, AkA, (A_g, A_m), products, _, _ = _assemble(monkeypatch, "magn", feed_on)
    assert [(p[0] is A_g, p[0] is A_m) for p in products] == [(True, False), (False, True)]
    assert products[0][1:] == (MS, [G(0, 0)], [ptr(AK, 0, 0)], feed_on)
    assert products[1][1:] == (MM, [G(1, 0), G(1, 1)], [ptr(AK, MS, 0), ptr(AK, MS, 1)], feed_on)
    assert step.gens == {(s_, j): G(s_, j) for s_ in (0, 1) for j in (0, 1)}        # the posterior needs all four
    assert sorted(step.gram_S) == ([(0, 0), (1, 0), (1, 1)] if feed_on else [])
    assert len(step.ak_fill) == (2 if feed_on else 1)


@pytest.mark.parametrize("feed_on", [True, False])
def test_the_parents_plan_is_what_it_was(monkeypatch, feed_on):
    eng, step, AK, AkA, (A_g, A_m), products, gram_calls, _ = _assemble(monkeypatch, "grav", feed_on)
    assert products[0][1:] == (MS, [G(0, 0), G(0, 1)], [ptr(AK, 0, 0), ptr(AK, 0, 1)], feed_on)
    assert products[1][1:] == (MM, [G(1, 1)], [ptr(AK, MS, 1)], feed_on)
    assert sorted(step.gram_S) == ([(0, 0), (0, 1), (1, 1)] if feed_on else [])
    assert len(step.ak_fill) == (2 if feed_on else 0)
    names = [n for n, _, _ in gram_calls]
    inner = "back_rows" if feed_on else "gram_rows"
    assert names == [inner, "edge_rows", "edge_rows"] * 3 + ["transpose", "centro_fill"] and "mirror_planes" not in names
    t = [a for n, a, _ in gram_calls if n == "transpose"][0]
    assert t[0].data_ptr() == AkA[:MS, MS:].data_ptr() and t[1].data_ptr() == AkA[MS:, :MS].data_ptr()
    assert [f for f in eng.flops if f[0].startswith("aka")] == [("aka_lattice", 1000.0 * (2 * MS + MM) if feed_on else float(2 * MS + MM)), ("aka_centro_fill", 0.0)]


@pytest.mark.parametrize("feed_on", [True, False])
def test_cross_block_comes_from_the_magnetic_rows_without_a_gravity_to_magnetic_gram(monkeypatch, feed_on):
    eng, step, AK, AkA, _, _, gram_calls, _ = _assemble(monkeypatch, "magn", feed_on)
    names = [n for n, _, _ in gram_calls]
    inner = "back_rows" if feed_on else "gram_rows"
    assert names == ([inner, "edge_rows", "edge_rows"] * 2                      # (grav, grav) and (magn, magn)
                     + [inner, "centro_fill", "mirror_planes", "mirror_planes", "edge_rows", "edge_rows", "transpose"]
                     + ["centro_fill"])                                         # (the magnetic block's own, behind its slabs)
    ll, ur = AkA[MS:, :MS], AkA[:MS, MS:]
    outs = [a[2 if n == "back_rows" else 3].data_ptr() for n, a, _ in gram_calls if n in ("back_rows", "gram_rows", "edge_rows")]
    assert ur.data_ptr() not in outs                                            # no Gram writes the upper-right block
    assert outs == [AkA.data_ptr()] * 3 + [AkA[MS:, MS:].data_ptr()] * 3 + [ll.data_ptr()] * 3
    cross = gram_calls[6:13]
    # interior of the computed rows against the GRAVITY table
    if feed_on:
        assert cross[0][1][0] is step.gram_S[(1, 0)] and cross[0][1][1] == MM
    else:
        assert cross[0][1][0].data_ptr() == ptr(AK, MS, 0) and cross[0][1][1:3] == (MM, "lam_g")
    assert all(a[2] != "lam_m" or a[0].data_ptr() != AK.data_ptr() for n, a, _ in gram_calls if n == "gram_rows")
    # the point mirror of the square block, from its middle row
    assert cross[1][1][0].data_ptr() == ll.data_ptr() and cross[1][1][1:] == (MS, (MS + 1) // 2)
    # boundary planes of the mirrored rows: plane 0 from plane ny-1 and the other way round, rows [0, Ms - Mm) of the source
    X = AK[MS:, 0:N]
    for (n, a, _), (dst, src) in zip(cross[2:4], ((0, NY - 1), (NY - 1, 0))):
        assert a[0].data_ptr() == X[:, src * PL:].data_ptr() and a[1].data_ptr() == X[:, dst * PL:].data_ptr()
        assert a[2:] == (MS, 0, MS - MM, NX, NZ)
    # gravity's boundary slabs for EVERY row, behind the fill; then the upper-right block by transpose
    for (n, a, _), (k, iy) in zip(cross[4:6], ((0, 0), (1, NY - 1))):
        assert a[0].data_ptr() == X[:, iy * PL:].data_ptr() and a[1] == MS and a[2] == ("edge", "grav", k)
    assert cross[6][1][0].data_ptr() == ll.data_ptr() and cross[6][1][1].data_ptr() == ur.data_ptr()
    rows = MS + 2 * MM
    assert [f for f in eng.flops if f[0].startswith("aka")] == [("aka_lattice", 1000.0 * rows if feed_on else float(rows)), ("aka_centro_fill", 0.0)]


@pytest.mark.parametrize("feed_on", [True, False])
def test_completion_chain_runs_gravity_magnetic_mirror_once(monkeypatch, feed_on):
    eng, step, AK, _, (A_g, A_m), _, _, log = _assemble(monkeypatch, "magn", feed_on)
    last = _LastStep(AK_partial=AK, AK_complete=False)
    last.complete = PosteriorEngine._ak_completion(eng, step, AK)
    assert log == []
    assert last["AK_partial"] is AK and last["AK_partial"] is AK and last.complete is None
    got = [(n, a[0], a[1], a[2] if n == "product" else None, kw.get("gx")) for n, a, kw in log]
    if feed_on:
        # the storing product of A_g K_00 and A_g K_01 (not the in-step product's single block), then A_m K_11, then the mirrored rows
        assert [g[0] for g in got] == ["product", "product", "mirror_rows"]
        assert got[0][1] is A_g and got[0][2:] == (MS, [G(0, 0), G(0, 1)], None)
        assert got[1][1] is A_m and got[1][2:] == (MM, [G(1, 1)], None)
    else:
        # the step stored what it ran whole: only A_g K_01 is owed
        assert [g[0] for g in got] == ["product", "mirror_rows"]
        assert got[0][1] is A_g and got[0][2:] == (MS, [G(0, 1)], None)
    m = log[-1][1]
    assert m[0].data_ptr() == AK[MS:, N:].data_ptr() and m[1:] == (MS, MM, NX * NY, NZ)


def test_mirror_planes_arguments_are_validated_before_any_device_call():
    """geobo_mirror_planes follows geobo_mirror_rows: a null pointer, a bad row range or planes wider than a row stride are GEOBO_E_ARG,
    odd nz / strides and pointers off the 16-byte boundary GEOBO_E_ALIGN."""
    from geobo_amd import _lib
    L = _lib.load()
    assert L.geobo_mirror_planes(None, 16, 8192, 16, 6, 0, 3, 4, 2, None) == -1
    assert L.geobo_mirror_planes(4096, 16, None, 16, 6, 0, 3, 4, 2, None) == -1
    assert L.geobo_mirror_planes(4096, 16, 8192, 16, 6, 4, 3, 4, 2, None) == -1       # r0 > r1
    assert L.geobo_mirror_planes(4096, 16, 8192, 16, 6, 0, 7, 4, 2, None) == -1       # r1 > m
    assert L.geobo_mirror_planes(4096, 6, 8192, 16, 6, 0, 3, 4, 2, None) == -1        # nx nz > lds
    assert L.geobo_mirror_planes(4096, 16, 8192, 6, 6, 0, 3, 4, 2, None) == -1        # nx nz > ldd
    assert L.geobo_mirror_planes(4096, 16, 8192, 16, 6, 0, 3, 4, 3, None) == -2       # odd nz
    assert L.geobo_mirror_planes(4096, 17, 8192, 16, 6, 0, 3, 4, 2, None) == -2       # odd lds
    assert L.geobo_mirror_planes(4096 + 8, 16, 8192, 16, 6, 0, 3, 4, 2, None) == -2   # not 16-byte aligned
    assert L.geobo_mirror_planes(4096, 16, 8192, 16, 6, 2, 2, 4, 2, None) == 0        # an empty range launches nothing
