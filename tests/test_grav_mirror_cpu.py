"""AkA's gravity block from half its rows ("gravity block from half its rows"; GEOBO_GRAV_MIRROR), as far as it runs
without a device:

  the identity      a dense NumPy model on a 6 x 5 x 3 grid: A_g = A_i + A_s (interior planes: windows of a point-even stencil table;
                    boundary slabs: random, no symmetry), K any symmetric lattice table.
                        centro(half the rows of A_i K A_i^T) + E + E^T + A_s K A_s^T  =  A K A^T,    E = A_i K A_s^T,
                    with the boundary planes of the mirrored rows of A_i K taken from their partners (x-reversed, opposite plane) and
                    the two planes of A_s K from the 2 x 2 Toeplitz product -- the data flow of transposed.grav_from_half.  It fails
                    as soon as the table is not point-even.
  the gate          plan.grav_options / plan.grav_mirror_route as a literal table
  the launches      what _assemble_AkA_sym asks of the Gram and of `hip` when step.grav_mirror is set (recorders, no kernel runs)
  the two entries   geobo_sym_add, geobo_slab_pair_y: arguments are validated before any device call

Tolerance of the identity: both sides are sums of products three factors deep over N = 90 voxels twice; fp64 summation in any order
differs from the exact value by at most gamma_2N |A| |K| |A|^T entrywise, so the two sides differ by at most twice that:
4 N eps max(|A| |K| |A|^T) bounds it with room for the 2 x 2 re-association."""
import dataclasses
import types

import numpy as np
import pytest
import torch

from geobo_amd import plan, transposed
from geobo_amd.engine import PosteriorEngine
from geobo_amd.step import Step

F64 = torch.float64
EPS = np.finfo(np.float64).eps


# ---- the identity -----------------------------------------------------------------------------------------------------------------------
GX, GY, GZ = 6, 5, 3
PLN, NV, NS = GX * GZ, GX * GY * GZ, GX * GY


def _model(seed, even=True):
    """(A_i, A_s, K): rows r = (jy, jx) row-major, voxels (iy, ix, iz)."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((2 * GY - 3, 2 * GX - 1, GZ))
    Q = 0.5 * (Q + Q[::-1, ::-1])                                   # point-even: Q[-dy, -dx, z] = Q[dy, dx, z]
    if not even:
        Q[0, 1, 0] += 0.25
    cy, cx = GY - 2, GX - 1
    A_i, A_s = np.zeros((NS, GY, GX, GZ)), np.zeros((NS, GY, GX, GZ))
    for jy in range(GY):
        for jx in range(GX):
            r = jy * GX + jx
            for iy in range(1, GY - 1):
                A_i[r, iy] = Q[iy - jy + cy, cx - jx:cx - jx + GX]
            A_s[r, 0], A_s[r, GY - 1] = rng.standard_normal((GX, GZ)), rng.standard_normal((GX, GZ))
    k = rng.standard_normal((GY, GX, GZ))                           # any symmetric lattice table: K[v, v'] = k(|dy|, |dx|, |dz|)
    iy, ix, iz = np.meshgrid(np.arange(GY), np.arange(GX), np.arange(GZ), indexing="ij")
    iy, ix, iz = iy.reshape(-1), ix.reshape(-1), iz.reshape(-1)
    K = k[np.abs(iy[:, None] - iy[None, :]), np.abs(ix[:, None] - ix[None, :]), np.abs(iz[:, None] - iz[None, :])]
    return A_i.reshape(NS, NV), A_s.reshape(NS, NV), K, k


def _from_half(A_i, A_s, K, k):
    """The block as grav_from_half assembles it, dense."""
    Mh = (NS + 1) // 2
    AiK = np.full((NS, GY, GX, GZ), np.nan)
    AiK[:Mh] = (A_i[:Mh] @ K).reshape(Mh, GY, GX, GZ)              # the rows the product runs
    B = np.full((NS, NS), np.nan)
    B[:Mh] = AiK[:Mh].reshape(Mh, NV) @ A_i.T                       # back_rows
    for r in range(Mh, NS):                                         # centro_fill
        B[r] = B[NS - 1 - r, ::-1]
    for dst, src in ((0, GY - 1), (GY - 1, 0)):                     # mirror_planes
        for r in range(NS - Mh):
            AiK[NS - 1 - r, dst] = AiK[r, src, ::-1]
    As4 = A_s.reshape(NS, GY, GX, GZ)
    E = np.zeros((NS, NS))
    for iy in (0, GY - 1):                                          # edge_rows into E
        E += AiK[:, iy].reshape(NS, PLN) @ As4[:, iy].reshape(NS, PLN).T
    B += E + E.T                                                    # sym_add
    # the slab pair: planes 0 and ny-1 of A_s K through the (x, z) blocks T(0), T(ny-1) of the Toeplitz-in-y matrix K
    T = lambda d: K.reshape(GY, PLN, GY, PLN)[0, :, d, :]
    e0, e1 = As4[:, 0].reshape(NS, PLN), As4[:, GY - 1].reshape(NS, PLN)
    o0, o1 = e0 @ T(0) + e1 @ T(GY - 1), e0 @ T(GY - 1) + e1 @ T(0)
    return B + o0 @ e0.T + o1 @ e1.T                                # edge_rows of the pair


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_block_from_half_its_rows_is_the_block(seed):
    A_i, A_s, K, k = _model(seed)
    A = A_i + A_s
    want, got = A @ K @ A.T, _from_half(A_i, A_s, K, k)
    tol = 4.0 * NV * EPS * float((np.abs(A) @ np.abs(K) @ np.abs(A).T).max())
    err = float(np.abs(got - want).max())
    print("6 x 5 x 3 dense model, seed %d: max|from half - A K A^T| = %.3e, bound %.3e, max|A K A^T| = %.3e" % (seed, err, tol, np.abs(want).max()))
    assert not np.isnan(got).any() and err <= tol
    # the slabs really are not symmetric: mirroring the whole operator would be wrong by far more than the bound
    Am = A.reshape(NS, GY, GX, GZ)[::-1, ::-1, ::-1].reshape(NS, NV)
    assert float(np.abs(Am - A).max()) > 0.1


def test_block_from_half_its_rows_needs_the_even_table():
    A_i, A_s, K, k = _model(0, even=False)
    A = A_i + A_s
    want, got = A @ K @ A.T, _from_half(A_i, A_s, K, k)
    tol = 4.0 * NV * EPS * float((np.abs(A) @ np.abs(K) @ np.abs(A).T).max())
    assert float(np.abs(got - want).max()) > 1e6 * tol


def test_interior_part_is_centrosymmetric_and_the_slab_part_is_not():
    A_i, A_s, K, _ = _model(3)
    Bi, Bs = A_i @ K @ A_i.T, A_s @ K @ A_s.T
    scale = float(np.abs(Bi).max())
    assert float(np.abs(Bi - Bi[::-1, ::-1]).max()) <= 4.0 * NV * EPS * float((np.abs(A_i) @ np.abs(K) @ np.abs(A_i).T).max())
    assert float(np.abs(Bs - Bs[::-1, ::-1]).max()) > 1e-3 * scale


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
def test_grav_options_are_their_own_table():
    assert dataclasses.asdict(plan.grav_options({})) == dict(grav_mirror="auto") == dataclasses.asdict(plan.grav_options(None))
    for v in ("auto", "on", "off"):
        assert plan.grav_options({"GEOBO_GRAV_MIRROR": v}).grav_mirror == v
    with pytest.raises(ValueError):
        plan.grav_options({"GEOBO_GRAV_MIRROR": "1"})
    names = {v for v, _, _ in plan.GRAV_OPTIONS.values()}
    others = (set(plan.SWITCHES.values()) | {v for v, _, _ in plan.ENGINE_OPTIONS.values()} | {v for v, _, _ in plan.FEED_OPTIONS.values()}
              | {v for v, _, _ in plan.CROSS_OPTIONS.values()})
    assert not names & others
    assert "grav_mirror" not in plan.SWITCHES and "grav_mirror" not in {f.name for f in dataclasses.fields(plan.Forms)}
    # the other tables and the planner are what they were
    assert dataclasses.asdict(plan.feed_options({})) == dict(gram_gx=True) and dataclasses.asdict(plan.cross_options({})) == dict(cross_rows="auto")
    assert plan.plan_route(64, 64, 64, env={"GEOBO_GRAV_MIRROR": "off"}) == plan.plan_route(64, 64, 64, env={})
    with pytest.raises(dataclasses.FrozenInstanceError):
        plan.grav_options({}).grav_mirror = "off"


CUBE, SLAB, SMALL = (64, 64, 64), (64, 32, 64), (32, 32, 32)
ALL = dict(sym=True, static=True, handover=True, pooled=True, even=True, alone=True)
# option, the condition that fails (None: all hold), grid -> taken
GATE = ([("auto", None, CUBE, True), ("auto", None, SLAB, False), ("auto", None, SMALL, False),
         ("on", None, CUBE, True), ("on", None, SLAB, True), ("on", None, SMALL, True),
         ("off", None, CUBE, False), ("off", None, SLAB, False), ("off", None, SMALL, False)]
        + [(opt, c, grid, False) for opt in ("auto", "on", "off") for c in ALL for grid in (CUBE, SLAB)])


@pytest.mark.parametrize("opt,fails,grid,want", GATE)
def test_gate(opt, fails, grid, want):
    cond = dict(ALL)
    if fails is not None:
        cond[fails] = False
    assert plan.grav_mirror_route(plan.grav_options({"GEOBO_GRAV_MIRROR": opt}), *[cond[c] for c in ALL], *grid) is want


def test_auto_is_the_default():
    assert plan.grav_mirror_route(plan.grav_options({}), *[True] * 6, *CUBE) is True
    assert plan.grav_mirror_route(plan.grav_options({}), *[True] * 6, *SLAB) is False
    assert Step(None, (0, 1), None, 0, 0, None).grav_mirror == 0            # (a derivative Gram's step sets nothing)


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


def test_gravity_block_is_assembled_from_half_its_rows(monkeypatch):
    log = []
    monkeypatch.setattr(transposed, "hip", Calls(log))
    gram = Calls(log, flops=lambda rows, ny=None: float(rows), flops_back=lambda rows: 1000.0 * rows)
    A_g, A_m = torch.zeros(MS, N, dtype=F64), torch.zeros(MS, N, dtype=F64)
    E = torch.ones(MS, MS, dtype=F64)
    eng = types.SimpleNamespace(nx=NX, ny=NY, nz=NZ, N=N, nc=N, Ms=MS, Ms_pad=MS, _gram=gram, _lam={"grav": (A_g, "lam_g"), "magn": (A_m, "lam_m")},
                                flops=[])
    eng._timed = lambda name, fl, fn, **kw: (eng.flops.append((name, fl)), fn())[1]
    eng._edge_spectrum = lambda func, k, cols: ("edge", func, k)
    eng._finish_AkA = lambda step, AkA: AkA
    eng._workspace2d = lambda name, rows, cols: {"grav_E": E}[name][:rows, :cols]
    step = Step(None, (0, 1), None, 0, 3 * MS, None, sym=True, mirror=MM)
    step.cross_rows, step.grav_mirror = "magn", MM
    step.gram_S = {b: torch.zeros(1, dtype=F64) for b in ((0, 0), (1, 0), (1, 1))}
    step.grav_slabs, step.grav_iplanes = torch.zeros(MS, 2 * PL, dtype=F64), torch.zeros(MS, 2 * PL, dtype=F64)
    AK, AkA = torch.zeros(3 * MS, 2 * N, dtype=F64), torch.zeros(3 * MS, 3 * MS, dtype=F64)
    PosteriorEngine._assemble_AkA_sym(eng, step, AkA, AK, A_g, A_m)
    names = [n for n, _, _ in log]
    grav = ["back_rows", "centro_fill", "mirror_planes", "mirror_planes", "edge_rows", "edge_rows", "sym_add", "edge_rows", "edge_rows"]
    assert names[:9] == grav and names[9:12] == ["back_rows", "edge_rows", "edge_rows"]            # then (magn, magn) as before
    assert names[12:] == ["back_rows", "centro_fill", "mirror_planes", "mirror_planes", "edge_rows", "edge_rows", "transpose", "centro_fill"]
    g = [a for _, a, _ in log[:9]]
    X = step.grav_iplanes                      # the two planes of A_i K, apart from the A K buffer (the completion hook overwrites that)
    assert g[0][0] is step.gram_S[(0, 0)] and g[0][1] == MM and g[0][2].data_ptr() == AkA.data_ptr()       # half the rows come back
    assert g[1][0].data_ptr() == AkA.data_ptr() and g[1][1:] == (MS, (MS + 1) // 2)
    for a, (dst, src) in zip(g[2:4], ((0, 1), (1, 0))):
        assert a[0].data_ptr() == X[:, src * PL:].data_ptr() and a[1].data_ptr() == X[:, dst * PL:].data_ptr() and a[2:] == (MS, 0, MS - MM, NX, NZ)
    assert float(E.abs().max()) == 0.0                                                                   # the scratch is zeroed before it is added to
    for a, (k, iy) in zip(g[4:6], ((0, 0), (1, NY - 1))):                                                # E: every row's planes of A_i K
        assert a[0].data_ptr() == X[:, k * PL:].data_ptr() and a[1] == MS and a[2] == ("edge", "grav", k) and a[3].data_ptr() == E.data_ptr()
    assert g[6][0].data_ptr() == E.data_ptr() and g[6][1].data_ptr() == AkA.data_ptr() and g[6][2] == MS
    for a, k in zip(g[7:9], (0, 1)):                                                                     # the slab pair, into the block itself
        assert a[0].data_ptr() == step.grav_slabs[:, k * PL:].data_ptr() and a[1] == MS and a[2] == ("edge", "grav", k)
        assert a[3].data_ptr() == AkA.data_ptr()
    assert eng.flops[0] == ("aka_lattice", 1000.0 * (MM + 2 * MM))                                       # the rows that ran


def test_resident_gravity_rows_run_their_interior_part_and_the_fill_runs_them_whole(monkeypatch):
    """A resident operator under step.grav_mirror: slab spectra of all Ms rows and the slab pair first, then the first MM rows as batch
    copies with planes 0 and ny-1 zeroed, handed to the Gram; the completion hook runs every gravity row whole from the operator itself."""
    from geobo_amd import engine as engine_mod
    from geobo_amd.engine import _GramFeed
    log = []
    monkeypatch.setattr(engine_mod, "hip", Calls(log))
    seen = []
    sp = Calls(log, R=MM // 2, eigenvalues=lambda tab: ("gen",) + tab[1:], pool_applies=lambda: False, flops=lambda *a, **kw: 1.0,
               flops_valu=lambda *a, **kw: 1.0, slab_spectra=lambda A, Ms: ("spectra", A.data_ptr(), Ms),
               product=lambda A, R, lams, outs, y0, y1, gx=None: seen.append((A.clone() if A is abuf else A, R, lams, [o.data_ptr() for o in outs], gx)))
    gram = Calls(log, flops_gx=lambda rows: 1.0, Py=2 * NY, Px=2 * NX)
    A_g, A_m = torch.ones(MS, N, dtype=F64), torch.ones(MS, N, dtype=F64)
    abuf, slabs, kept = torch.full((MM, N), 7.0, dtype=F64), torch.zeros(MS + 1, 2 * PL, dtype=F64), torch.full((MS + 1, 2 * PL), 5.0, dtype=F64)
    eng = types.SimpleNamespace(nx=NX, ny=NY, nz=NZ, N=N, nc=N, c0=0, c1=N, Ms=MS, Ms_pad=MS, exchange=False, f32=False, _gram=gram)
    eng._spectral_product = lambda: sp
    eng._timed = lambda name, fl, fn, **kw: fn()
    eng._op_rows_buffer = lambda: abuf
    eng._workspace2d = lambda name, rows, cols: {"grav_slabs": slabs, "grav_iplanes": kept}[name][:rows, :cols]

    def gram_feed(step, s_, blocks):
        S = [torch.zeros(MS * 4 * NX * NY, dtype=F64) for _ in blocks]
        for j, Sj in zip(blocks, S):
            step.gram_S[(s_, j)] = Sj
        return _GramFeed(gram, ["lam"] * len(blocks), S, store_all=False)
    eng._gram_feed = gram_feed

    class Prior:
        def table(self, eng, s_, j):
            return ("table", s_, j)
    step = Step(Prior(), (0, 1), None, 0, 3 * MS, None, sym=True, mirror=MM)
    step.cross_rows, step.grav_mirror = "magn", MM
    AK = torch.zeros(3 * MS, 2 * N, dtype=F64)
    PosteriorEngine._assemble_AK_spectral(eng, step, AK, A_g, A_m)
    pair = [a for n, a, _ in log if n == "slab_pair_rows"]
    assert len(pair) == 1 and pair[0][0] == ("spectra", A_g.data_ptr(), MS) and pair[0][1:3] == (MS, ("gen", 0, 0))
    assert pair[0][3].data_ptr() == slabs.data_ptr() and pair[0][3].shape == (MS, 2 * PL)
    grav = seen[:2]                                                         # two batches of MM / 2 rows, block K_00 alone, fed to the Gram
    for b, (rows, R, lams, outs, gx) in enumerate(grav):
        assert R == MM // 2 and lams == [("gen", 0, 0)] and outs == [AK[b * R:, 0:N].data_ptr()] and gx is not None
        x = rows[:R].view(R, NY, PL)
        assert float(x[:, 0].abs().max()) == 0.0 and float(x[:, NY - 1].abs().max()) == 0.0 and bool((x[:, 1:NY - 1] == 1.0).all())
    assert seen[2][0] is A_m and seen[2][1] == MM and len(seen) == 3        # the magnetic half, both blocks, as before
    # the stored planes 0 and ny-1 of the run rows are kept apart from the buffer (here: the zeros the fake product left in A K)
    assert step.grav_iplanes.data_ptr() == kept.data_ptr() and float(kept[:MM].abs().max()) == 0.0 and bool((kept[MM:] == 5.0).all())
    assert len(step.ak_fill) == 2
    step.ak_fill[0]()
    assert seen[3][0] is A_g and seen[3][1] == MS and seen[3][2] == [("gen", 0, 0), ("gen", 0, 1)] and seen[3][4] is None


def test_new_entries_validate_their_arguments_before_any_device_call():
    from geobo_amd import _lib
    L = _lib.load()
    assert L.geobo_sym_add(4, None, 8, 8192, 8, None) == -1 and L.geobo_sym_add(4, 4096, 8, None, 8, None) == -1
    assert L.geobo_sym_add(-1, 4096, 8, 8192, 8, None) == -1
    assert L.geobo_sym_add(9, 4096, 8, 8192, 16, None) == -1 and L.geobo_sym_add(9, 4096, 16, 8192, 8, None) == -1      # n > lde, ldb
    assert L.geobo_sym_add(0, 4096, 8, 8192, 8, None) == 0                                                              # nothing to launch
    ok = [4, 64, 64, 3, 4096, 128, 8192, 16384, 128, None]           # ny, C, plane, rows, in, in_row, tab, out, out_row, stream
    bad = {"null in": ({4: None}, -1), "null tab": ({6: None}, -1), "null out": ({7: None}, -1), "ny < 2": ({0: 1}, -1), "negative rows": ({3: -1}, -1),
           "C = 0": ({1: 0}, -1), "plane < C": ({2: 62}, -1), "short in_row": ({5: 126}, -1), "short out_row": ({8: 126}, -1),
           "odd C": ({1: 63}, -2), "odd plane": ({2: 65, 5: 130, 8: 130}, -2), "odd in_row": ({5: 129}, -2), "odd out_row": ({8: 129}, -2),
           "misaligned in": ({4: 4096 + 8}, -2), "misaligned tab": ({6: 8192 + 8}, -2), "misaligned out": ({7: 16384 + 8}, -2)}
    for what, (change, code) in bad.items():
        args = list(ok)
        for i, v in change.items():
            args[i] = v
        assert L.geobo_slab_pair_y(*args) == code, what
    args = list(ok)
    args[3] = 0
    assert L.geobo_slab_pair_y(*args) == 0                                                                               # no rows: nothing to launch
