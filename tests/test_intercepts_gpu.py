"""Drill-intercept statistics on the device: geobo_trace_stats by value against the NumPy reference of
_intercepts_ref (columns and CSR traces, the listed patterns, accumulation over calls, bitwise reproducibility), and
Inversion.drill_intercepts / column_intercepts against the same reference on the host realisations of sample_posterior.

Integers (detail, tab, the integer maps, both histograms) are asked for exactly.  Sums: every order of adding L numbers is within
(L - 1) 2^-53 sum |x| of the exact sum; the tests ask for twice that, as section 17 does, and for acc_sum add 2 S 2^-53 sum_s |acc_s|
for the S sequential additions over the samples.

The kernel test pairs every grid of the list with one S of {1, 3} and one C of {1, 5, 32} (each of the six pairs occurs) and runs
all four (min_len, max_gap) on it; the patterns get a test of their own on columns of 9, 70, 130 and 200 samples, one pattern per
column, so that every pattern meets every (min_len, max_gap), a word border and the second one."""
import numpy as np
import pytest
import torch

import _intercepts_ref as ref
from conftest import load_golden, settings_for

pytestmark = pytest.mark.gpu

SEED = 2026
PSD_W = (0.2, 0.2, 0.2)
TINY = dict(nx=10, ny=8, nz=6)
GRID = (8, 10, 6)                                             # (ny, nx, nz)
N = 480
DZ = 100.0
AREA = 100.0 * 100.0
LEN_GAP = [(1, 0), (3, 0), (2, 1), (4, 3)]
OCCUPANCY_SHIFT = (-1.2816, -0.5244, 0.0, 0.5244, 1.2816)     # the normal quantiles of 0.1, 0.3, 0.5, 0.7, 0.9


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype,
                                                                                                           device="cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _launch(Fd, grid, p, t, lo, mask, ml, mg, traces=None, maps=None):
    from geobo_amd import hip
    S, C_ = Fd.shape[0], len(t)
    K = grid[0] * grid[1] if traces is None else traces.K
    detail = torch.full((S, C_, K, 6), -7, dtype=torch.int32, device="cuda")
    dsum = torch.full((S, C_, K, 2), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((hip.trace_stats_ws_doubles(S, K, C_),), float("nan"), dtype=torch.float64, device="cuda")
    tab = hip.trace_stats(Fd, grid, p, t, lo=lo, mask=mask, traces=traces, min_len=ml, max_gap=mg, maps=maps, detail=detail, dsum=dsum, ws=ws)
    return dict(tab=tab.cpu().numpy(), detail=detail.cpu().numpy(), dsum=dsum.cpu().numpy())


def _host_maps(maps):
    return {k: v.cpu().numpy() for k, v in maps.items()}


def _check(F, grid, p, t, lo, mask, ml, mg, trace_lists=None, label=""):
    """One configuration against the reference: values, accumulation over calls, and the bitwise claims."""
    from geobo_amd import hip
    S, C_ = F.shape[0], len(t)
    n = F.shape[2]
    lists = ref.column_traces(*grid) if trace_lists is None else trace_lists
    K = len(lists)
    L = np.array([len(tr) for tr in lists])
    Lmax = int(L.max())
    traces = None
    if trace_lists is not None:
        traces = hip.TraceSet(np.concatenate([[0], np.cumsum(L)]), np.concatenate(lists), n)
    want = ref.trace_stats(F, p, t, lists, lo=lo, mask=mask, min_len=ml, max_gap=mg)
    wmaps = ref.maps_of(want, Lmax, min_len=ml)
    Fd = _dev(F)
    md = None if mask is None else _dev(mask.astype(np.uint8))
    maps = hip.trace_maps(C_, K, Lmax)
    got = _launch(Fd, grid, p, t, lo, md, ml, mg, traces, maps)
    m1 = _host_maps(maps)
    # exact integers
    assert np.array_equal(got["detail"], want["detail"]), label
    assert np.array_equal(got["tab"], want["tab"]), label
    for k in ("hits_any", "hits", "thick_sum", "top_sum", "hist_len", "hist_thick"):
        assert np.array_equal(m1[k], wmaps[k]), (label, k)
    # the two sums per (s, c, k), and the sum over the samples
    bound = ref.sum_bound(L[None, None, :, None], want["dabs"])
    err = np.abs(got["dsum"] - want["dsum"])
    print("%s: max |dsum - fsum| %.3e (bound there %.3e)" % (label, err.max(), bound.reshape(-1)[err.argmax()]))
    assert np.all(err <= bound), label
    abound = bound[..., 0].sum(0) + 2.0 * S * ref.U * wmaps["acc_sum_abs"]
    assert np.all(np.abs(m1["acc_sum"] - wmaps["acc_sum"]) <= abound), label
    # a second call accumulates: the integers double
    again = _launch(Fd, grid, p, t, lo, md, ml, mg, traces, maps)
    m2 = _host_maps(maps)
    for k in ("hits_any", "hits", "thick_sum", "top_sum", "hist_len", "hist_thick"):
        assert np.array_equal(m2[k], 2 * wmaps[k]), (label, k)
    # bit-identical: a second run ...
    for k in ("tab", "detail"):
        assert np.array_equal(again[k], got[k]), (label, k)
    assert np.array_equal(_bits(again["dsum"]), _bits(got["dsum"])), label
    # ... the samples in two calls (the accumulators too) ...
    if S > 1:
        maps_b = hip.trace_maps(C_, K, Lmax)
        a = _launch(Fd[:1], grid, p, t, lo, md, ml, mg, traces, maps_b)
        b = _launch(Fd[1:], grid, p, t, lo, md, ml, mg, traces, maps_b)
        assert np.array_equal(np.concatenate([a["detail"], b["detail"]]), got["detail"]) and np.array_equal(np.concatenate([a["tab"], b["tab"]]), got["tab"])
        assert np.array_equal(_bits(np.concatenate([a["dsum"], b["dsum"]])), _bits(got["dsum"])), label
        mb = _host_maps(maps_b)
        for k in m1:
            assert np.array_equal(_bits(mb[k]) if k == "acc_sum" else mb[k], _bits(m1[k]) if k == "acc_sum" else m1[k]), (label, k)
    # ... one-sample and one-cutoff launches
    for s in range(S):
        one = _launch(Fd[s:s + 1], grid, p, t, lo, md, ml, mg, traces)
        assert np.array_equal(one["detail"][0], got["detail"][s]) and np.array_equal(_bits(one["dsum"][0]), _bits(got["dsum"][s])), (label, s)
    for c in sorted({0, C_ // 2, C_ - 1}):
        one = _launch(Fd, grid, p, t[c:c + 1], lo, md, ml, mg, traces)
        assert np.array_equal(one["detail"][:, 0], got["detail"][:, c]) and np.array_equal(one["tab"][:, 0], got["tab"][:, c]), (label, c)
        assert np.array_equal(_bits(one["dsum"][:, 0]), _bits(got["dsum"][:, c])), (label, c)
    return got, want


def _thresholds(C_, exact):
    """C ascending thresholds around the cutoff 0: with more than one, -inf, one equal to an element bit for bit and one above all."""
    if C_ == 1:
        return np.array([0.0])
    base = np.array([-np.inf, -0.5, 0.0, exact, 40.0])
    if C_ > 5:
        base = np.concatenate([base, np.linspace(-2.0, 2.0, C_ - 6), [0.0]])                # (a repeated threshold too)
    return np.sort(base)


def _random_field(grid, S, seed):
    """Standard normal columns shifted so that the cutoff 0 meets the occupancies 0.1 .. 0.9 in turn, a few NaN, a region and values
    of the other properties that fail a lower bound here and there."""
    rng = np.random.default_rng(seed)
    ny, nx, nz = grid
    n = ny * nx * nz
    F = rng.standard_normal((S, 3, n))
    p = 1
    for s in range(S):
        for k in range(ny * nx):
            F[s, p, k * nz:(k + 1) * nz] += OCCUPANCY_SHIFT[(s + k) % 5]
    if n > 8:
        F[0, p, rng.integers(0, n, size=max(1, n // 40))] = np.nan
        F[S - 1, 2, rng.integers(0, n, size=max(1, n // 40))] = np.nan
    mask = rng.random(n) < 0.93 if n > 1 else np.ones(1, dtype=bool)
    lo = np.array([-1.6, -np.inf, -1.9])
    return F, p, lo, mask


# ---- 1. the kernel by value: grids, S, C, (min_len, max_gap) -----------------------------------------------------------------------
@pytest.mark.parametrize("grid,S,C_", [((1, 1, 1), 3, 32), ((1, 1, 63), 1, 5), ((1, 1, 64), 3, 1), ((1, 1, 65), 1, 32), ((2, 3, 70), 3, 5),
                                       ((3, 1, 130), 1, 1), ((5, 7, 9), 3, 32), ((16, 16, 16), 1, 5), ((2, 2, 128), 3, 5),
                                       ((1, 1, 4096), 3, 5)])
def test_trace_stats_by_value(grid, S, C_):
    F, p, lo, mask = _random_field(grid, S, seed=sum(grid) * 10 + S)
    j = 0 if F.shape[2] < 4 else 3
    F[0, p, j], F[0, 0, j], F[0, 2, j] = 0.37, 0.0, 0.0        # an element that passes the bounds: a cutoff equal to it counts it
    mask[j] = True
    t = _thresholds(C_, F[0, p, j])
    for ml, mg in LEN_GAP:
        got, want = _check(F, grid, p, t, lo, mask, ml, mg, label="grid %r S %d C %d len %d gap %d" % (grid, S, C_, ml, mg))
        if C_ > 1:
            c = list(t).index(0.37)
            k, pos = j // grid[2], j % grid[2]
            assert want["detail"][0, c, k, 0] >= 1 and want["detail"][0, c, k, 1] <= pos    # the tie is ore in the reference


# ---- 2. the patterns ---------------------------------------------------------------------------------------------------------------
def _patterns(L, g):
    """Named patterns for a column of L samples and max_gap g: each a dict(ore=positions, nan=, masked=, low=positions whose other
    property fails its bound); None when the column is too short."""
    def runs(*ab):
        return sorted({j for a, b in ab for j in range(a, b)})
    out = {"empty": dict(ore=[]), "full": dict(ore=list(range(L))), "alternating": dict(ore=list(range(0, L, 2))),
           "top": dict(ore=runs((0, min(3, L)))), "bottom": dict(ore=runs((max(0, L - 3), L)))}

    def gap_at(a, width):                                      # ore [a - 3, a), a gap of `width`, ore [a + width, a + width + 3)
        return dict(ore=runs((a - 3, a), (a + width, a + width + 3))) if a >= 3 and a + width + 3 <= L else None
    out["gap_exact"], out["gap_over"] = gap_at(3, g), gap_at(3, g + 1)
    for border in (64, 128):
        out["straddle_%d" % border] = dict(ore=runs((border - 4, border + 4))) if border + 4 <= L else None
        out["gap_exact_%d" % border] = gap_at(border - (g + 1) // 2, g)
        out["gap_over_%d" % border] = gap_at(border - (g + 2) // 2, g + 1)
    out["tie"] = dict(ore=runs((1, 3), (5 + g, 7 + g))) if 7 + g <= L else None
    w = max(g, 1)                                              # a gap that max_gap would fill (or, with max_gap 0, a plain gap) ...
    mid = 3 + w // 2
    if 6 + w <= L:
        out["nan_in_gap"] = dict(ore=runs((0, 3), (3 + w, 6 + w)), nan=[mid])             # ... holding a NaN,
        out["masked_in_gap"] = dict(ore=runs((0, 3), (3 + w, 6 + w)), masked=[mid])      # a voxel outside the region,
        out["bound_in_run"] = dict(ore=runs((0, 7)), low=[3])                             # and a run that a bound on another property cuts
    return {k: v for k, v in out.items() if v is not None}


@pytest.mark.parametrize("L", [9, 70, 130, 200])
def test_patterns(L):
    rng = np.random.default_rng(L)
    p, S = 0, 2
    for ml, mg in LEN_GAP:
        pats = _patterns(L, mg)
        names = sorted(pats)
        P = len(names)
        grid = (P, 1, L)
        F = np.zeros((S, 3, P * L))
        mask = np.ones(P * L, dtype=bool)
        F[:, p] = rng.uniform(-0.9, -0.1, size=(S, P * L))     # waste below the cutoff 0, ore above it
        for s in range(S):
            for k in range(P):
                d = pats[names[(k + s) % P]]                   # (the second sample meets the patterns one column on)
                base = k * L
                F[s, p, [base + j for j in d["ore"]]] = rng.uniform(0.1, 0.9, size=len(d["ore"]))
                for j in d.get("nan", []):
                    F[s, p, base + j] = np.nan
                for j in d.get("low", []):
                    F[s, 2, base + j] = -5.0
        for k in range(P):                                     # the region is shared by the samples: cut it where sample 0 asks
            for j in pats[names[k]].get("masked", []):
                mask[k * L + j] = False
        exact = F[0, p, names.index("full") * L + L // 2]
        t = _thresholds(5, exact)
        lo = np.array([-np.inf, -np.inf, -1.0])
        got, want = _check(F, grid, p, t, lo, mask, ml, mg, label="patterns L %d len %d gap %d" % (L, ml, mg))
        c0 = list(t).index(0.0)
        det = {names[k]: want["detail"][0, c0, k] for k in range(P)}                      # what the patterns mean, in the reference
        assert det["empty"].tolist() == [0, L, L, 0, 0, 0] and det["full"].tolist()[:4] == [L, 0, 0, L]
        assert det["top"].tolist()[:4] == [min(3, L)] * 1 + [0, 0, min(3, L)] and det["bottom"][2] == max(0, L - 3)
        if "gap_exact" in det:
            assert det["gap_exact"][3] == 6 + mg
        if "gap_over" in det:
            assert det["gap_over"][3] == 3 and det["gap_over"][2] == 0
        for border in (64, 128):
            if "straddle_%d" % border in det:
                assert det["straddle_%d" % border].tolist()[:4] == [8, border - 4, border - 4, 8]
            if "gap_exact_%d" % border in det:
                assert det["gap_exact_%d" % border][3] == 6 + mg
            if "gap_over_%d" % border in det:
                assert det["gap_over_%d" % border][3] == 3
        if "tie" in det:
            assert det["tie"].tolist()[:4] == [4, 1, 1, 2]
        if "nan_in_gap" in det:
            assert det["nan_in_gap"][3] == 3 and det["masked_in_gap"][3] == 3              # nothing is filled across them
            assert det["bound_in_run"][0] == 6 and det["bound_in_run"][3] == (7 if mg >= 1 else 3)


# ---- 3. CSR traces -----------------------------------------------------------------------------------------------------------------
def test_csr_traces():
    from geobo_amd import hip, intercepts as ic
    grid = (2, 3, 70)
    n = 420
    F, p, lo, mask = _random_field(grid, 3, seed=77)
    t = _thresholds(5, F[1, p, 9])
    ml, mg = 2, 1
    Fd, md = _dev(F), _dev(mask.astype(np.uint8))
    # the columns given explicitly equal the NULL form bit for bit
    off, vox = ic.column_traces(grid)
    ts = hip.TraceSet(off, vox, n)
    maps_a, maps_b = hip.trace_maps(5, 6, 70), hip.trace_maps(5, 6, 70)
    a = _launch(Fd, grid, p, t, lo, md, ml, mg, None, maps_a)
    b = _launch(Fd, grid, p, t, lo, md, ml, mg, ts, maps_b)
    assert np.array_equal(a["detail"], b["detail"]) and np.array_equal(a["tab"], b["tab"]) and np.array_equal(_bits(a["dsum"]), _bits(b["dsum"]))
    ha, hb = _host_maps(maps_a), _host_maps(maps_b)
    for k in ha:
        assert np.array_equal(_bits(ha[k]) if k == "acc_sum" else ha[k], _bits(hb[k]) if k == "acc_sum" else hb[k]), k
    # a reversed column, ragged lengths 1, 64, 65 and 200, and a trace that visits voxels twice
    rng = np.random.default_rng(5)
    lists = [list(range(139, 69, -1)), [417], list(range(100, 164)), list(range(7, 72)), [int(v) for v in rng.integers(0, n, size=200)],
             [30, 31, 31, 32, 33, 33, 33, 34, 30, 31]]
    got, want = _check(F, grid, p, t, lo, mask, ml, mg, trace_lists=lists, label="csr")
    col = ref.trace_stats(F, p, t, [list(range(70, 140))], lo=lo, mask=mask, min_len=ml, max_gap=mg)
    assert np.array_equal(want["detail"][:, :, 0, 0], col["detail"][:, :, 0, 0])           # read bottom up: the same thickness,
    assert np.array_equal(want["detail"][:, :, 0, 3], col["detail"][:, :, 0, 3])           # the same longest intercept
    for ml, mg in ((1, 0), (4, 3)):
        _check(F, grid, p, t, lo, mask, ml, mg, trace_lists=lists, label="csr len %d gap %d" % (ml, mg))


# ---- 4. drill_intercepts on the 10 x 8 x 6 survey ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """The inversion after cubing() and its 16 host realisations (cube units), computed once and left unchanged."""
    from geobo_amd.inversion import Inversion
    f = load_golden("tiny_exp.npz")
    s = settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W))
    inv = Inversion(settings=s)
    inv.create_cubegeometry()
    inv.gp_length = np.array([200.0, 204.0, 208.0])
    d0 = f["drilldata0"]
    cubes = inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    host = np.stack([c.reshape(16, N) for c in inv.sample_posterior(16, seed=SEED)], 1)          # (16, 3, N)
    host.setflags(write=False)
    return dict(inv=inv, host=host, mean=cubes[:3])


def _midpoint_cutoffs(values, scale, k=5):
    """k cutoffs half way between neighbours of the sorted values, none within 1e-9 scale of a value."""
    v = np.sort(np.asarray(values).reshape(-1))
    idx = (np.linspace(0.1, 0.9, k) * (v.size - 1)).astype(int)
    cut = 0.5 * (v[idx] + v[idx + 1])
    assert np.abs(v[None, :] - cut[:, None]).min() > 1e-9 * float(scale)
    return cut


def _compare_summaries(out, want, n, ml, lists, shape, label):
    """The integer side of a drill_intercepts result against the reference's (n, C, K) tables."""
    d = want["detail"]
    thick, top, length = d[..., 0], d[..., 1], d[..., 3]
    Cn = d.shape[1]
    assert np.array_equal(out["holes_hit"], want["tab"][..., 0]) and np.array_equal(out["count"], want["tab"][..., 1]), label
    assert np.array_equal(out["longest"], want["tab"][..., 2] * DZ), label
    assert np.array_equal(out["probability"].reshape(Cn, -1), (length >= ml).sum(0) / float(n)), label
    assert np.array_equal(out["probability_any"].reshape(Cn, -1), (thick > 0).sum(0) / float(n)), label
    for key, col in (("thickness", thick), ("intercept_length", length)):
        q = np.quantile(col, [0.1, 0.5, 0.9], axis=0, method="inverted_cdf")
        for i, name in enumerate(("p10", "p50", "p90")):
            assert out[key][name].shape == shape and np.array_equal(out[key][name].reshape(Cn, -1), q[i] * DZ), (label, key, name)
        assert np.allclose(out[key]["mean"].reshape(Cn, -1), col.mean(0) * DZ, rtol=1e-14, atol=0), (label, key)
    present = (thick > 0).sum(0)
    with np.errstate(all="ignore"):
        dtt = np.where(thick > 0, top, 0).sum(0) * DZ / present
    assert np.array_equal(np.isnan(out["depth_to_top_mean"].reshape(Cn, -1)), present == 0), label
    assert np.allclose(out["depth_to_top_mean"].reshape(Cn, -1), dtt, rtol=1e-14, atol=0, equal_nan=True), label


def test_drill_intercepts_matches_host_route(tiny):
    inv, host = tiny["inv"], tiny["host"]
    p, n = 2, 16
    scale = float(inv._cube_scale[p])
    cut = _midpoint_cutoffs(host[:, p], scale)[[3, 0, 4, 1, 2]]                                 # (the caller's order is kept)
    lists = ref.column_traces(*GRID)
    ml, mg = 2, 1                                                                               # 200 m, and a gap of one voxel
    want = ref.trace_stats(host, p, cut, lists, min_len=ml, max_gap=mg)
    out = inv.drill_intercepts(cut, prop="drill", n=n, seed=SEED, min_length=200.0, max_gap=100.0)
    assert np.array_equal(out["cutoffs"], cut) and (out["min_len"], out["max_gap_samples"], out["sample_length"]) == (ml, mg, DZ)
    _compare_summaries(out, want, n, ml, lists, (5, 8, 10), "columns")
    assert np.array_equal(out["prospective_area"], want["tab"][..., 0] * AREA) and out["quantiles"]["longest"].shape == (3, 5)
    assert np.array_equal(out["quantiles"]["prospective_area"], np.quantile(out["prospective_area"], [0.1, 0.5, 0.9], axis=0))
    # sum over the columns of the thickness = grade_tonnage's count, exactly; the accumulation = its quantity
    gt = inv.grade_tonnage(cut, prop="drill", n=n, seed=SEED)
    assert np.array_equal(out["count"], gt["count"])
    assert np.array_equal(np.rint(out["thickness"]["mean"].sum((1, 2)) * n / DZ).astype(np.int64), gt["count"].sum(0))
    total = out["accumulation_mean"].sum((1, 2)) * AREA
    # both are sums of the same S x N products scale x, each route within (terms - 1) u sum |x| per stage: the trace (L - 1), the
    # samples (S), grade_tonnage's voxels (N - 1), and the host's sums over columns (K - 1) and realisations (S - 1); twice that
    absx = np.array([np.abs(host[:, p])[host[:, p] >= c].sum() for c in cut])
    bound = 2.0 * ((6 - 1) + n + (N - 1) + (80 - 1) + (n - 1)) * ref.U * absx * DZ * AREA / n
    err = np.abs(total - gt["quantity"].mean(0))
    print("accumulation against grade_tonnage: max error %.3e, bound there %.3e" % (err.max(), bound[err.argmax()]))
    assert np.all(err <= bound)
    # the batching changes no bit, and realisations are addressed by their absolute index
    for batch in (2, 6):
        other = inv.drill_intercepts(cut, prop=2, n=n, seed=SEED, batch=batch, min_length=200.0, max_gap=100.0)
        for k in ("holes_hit", "count", "longest", "probability", "probability_any", "depth_to_top_mean", "accumulation_mean"):
            assert np.array_equal(other[k], out[k], equal_nan=True), (batch, k)
        for k in ("thickness", "intercept_length"):
            for q in ("mean", "p10", "p50", "p90"):
                assert np.array_equal(other[k][q], out[k][q]), (batch, k, q)
    part = inv.drill_intercepts(cut, prop=2, n=7, seed=SEED, start=3, min_length=200.0, max_gap=100.0)
    sub = dict(detail=want["detail"][3:10], tab=want["tab"][3:10])
    _compare_summaries(part, sub, 7, ml, lists, (5, 8, 10), "odd start")
    # an offset moves the cutoffs and the values together
    off = inv.drill_intercepts(cut + 3.5, prop=2, n=n, seed=SEED, offset=3.5, min_length=200.0, max_gap=100.0)
    assert np.array_equal(off["holes_hit"], out["holes_hit"]) and np.array_equal(off["probability"], out["probability"])
    assert np.allclose(off["accumulation_mean"], out["accumulation_mean"] + 3.5 * out["thickness"]["mean"], rtol=1e-12, atol=1e-9)


def test_drill_intercepts_require_region_and_limits(tiny):
    inv, host = tiny["inv"], tiny["host"]
    p, n = 2, 16
    cut = _midpoint_cutoffs(host[:, p], inv._cube_scale[p])
    lists = ref.column_traces(*GRID)
    region = np.zeros(GRID, dtype=bool)
    region[2:7, 1:9, :5] = True
    region[4, 4, 2] = False                                                                     # a hole in the region: no gap crosses it
    bound_d = float(np.median(host[:, 0]))
    assert np.abs(host[:, 0] - bound_d).min() > 1e-9 * float(inv._cube_scale[0])
    want = ref.trace_stats(host, p, cut, lists, lo=[bound_d, -np.inf, -np.inf], mask=region.reshape(-1), min_len=1, max_gap=1)
    out = inv.drill_intercepts(cut, prop="drill", n=n, seed=SEED, region=region, require={"density": bound_d}, max_gap=100.0)
    _compare_summaries(out, want, n, 1, lists, (5, 8, 10), "require and region")
    gt = inv.grade_tonnage(cut, prop="drill", n=n, seed=SEED, region=region, require={"density": bound_d})
    assert np.array_equal(out["count"], gt["count"])
    assert (out["probability_any"][:, 0] == 0).all() and (out["probability_any"][:, :, 0] == 0).all()
    # the limits: -inf takes every voxel, +inf none
    lim = inv.drill_intercepts([np.inf, -np.inf], prop="drill", n=4, seed=SEED, min_length=300.0)
    assert (lim["thickness"]["mean"][1] == 6 * DZ).all() and (lim["thickness"]["p10"][1] == 6 * DZ).all()
    assert (lim["depth_to_top_mean"][1] == 0).all() and (lim["probability"][1] == 1).all() and (lim["probability_any"][1] == 1).all()
    assert (lim["intercept_length"]["p90"][1] == 6 * DZ).all() and (lim["holes_hit"][:, 1] == 80).all() and (lim["longest"][:, 1] == 6 * DZ).all()
    assert (lim["probability_any"][0] == 0).all() and np.isnan(lim["depth_to_top_mean"][0]).all() and (lim["holes_hit"][:, 0] == 0).all()
    assert (lim["accumulation_mean"][0] == 0).all() and (lim["count"][:, 1] == N).all()


def test_drill_intercepts_holes_and_paths(tiny, tmp_path, monkeypatch):
    from geobo_amd import intercepts as ic
    inv, host = tiny["inv"], tiny["host"]
    monkeypatch.setattr(inv.settings, "outpath", str(tmp_path) + "/")
    p, n = 0, 16
    scale = float(inv._cube_scale[p])
    cut = _midpoint_cutoffs(host[:, p], scale, k=3)
    # two vertical holes
    holes = [(7, 2), (0, 5)]
    lists = [list(range((iy * 10 + ix) * 6, (iy * 10 + ix) * 6 + 6)) for ix, iy in holes]
    want = ref.trace_stats(host, p, cut, lists, min_len=2, max_gap=0)
    out = inv.drill_intercepts(cut, prop="density", n=n, seed=SEED, holes=holes, min_length=150.0)
    _compare_summaries(out, want, n, 2, lists, (3, 2), "holes")
    assert "prospective_area" not in out
    pr = out["per_realisation"]
    d = want["detail"]
    assert np.array_equal(pr["thickness"], d[..., 0] * DZ) and np.array_equal(pr["length"], d[..., 3] * DZ) and np.array_equal(pr["n_intercepts"], d[..., 4])
    assert np.array_equal(np.isnan(pr["from"]), d[..., 3] == 0) and np.array_equal(pr["from"][d[..., 3] > 0], d[..., 2][d[..., 3] > 0] * DZ)
    assert np.array_equal(pr["depth_to_top"][d[..., 0] > 0], d[..., 1][d[..., 0] > 0] * DZ)
    ok = d[..., 3] > 0
    gbound = ref.sum_bound(6, want["dabs"][..., 1])[ok] / d[..., 3][ok] + 4 * ref.U * np.abs(want["dsum"][..., 1][ok] / d[..., 3][ok])
    assert np.all(np.abs(pr["grade"][ok] - want["dsum"][..., 1][ok] / d[..., 3][ok]) <= gbound)          # (host values are in cube units)
    abound = (ref.sum_bound(6, want["dabs"][..., 0]) + 4 * ref.U * np.abs(want["dsum"][..., 0])) * DZ
    assert np.all(np.abs(pr["accumulation"] - want["dsum"][..., 0] * DZ) <= abound)
    both = inv.drill_intercepts(cut, prop="density", n=n, seed=SEED, min_length=150.0)
    for k, (ix, iy) in enumerate(holes):                                                        # a hole is its column of the map
        assert np.array_equal(out["probability"][:, k], both["probability"][:, iy, ix])
        assert np.array_equal(out["accumulation_mean"][:, k], both["accumulation_mean"][:, iy, ix])
    # one dipping path, 50 m steps: voxels repeat along it
    path = (310.0, 420.0, 35.0, 60.0)
    off, vox, step = ic.path_traces(inv.settings, [path], step=50.0)
    assert step == 50.0 and (np.diff(vox) == 0).any()
    wantp = ref.trace_stats(host, p, cut, [list(vox)], min_len=3, max_gap=2)
    outp = inv.drill_intercepts(cut, prop="density", n=n, seed=SEED, paths=[path], step=50.0, min_length=150.0, max_gap=100.0, write=True)
    assert (outp["min_len"], outp["max_gap_samples"], outp["sample_length"]) == (3, 2, 50.0) and outp["trace_lengths"].tolist() == [vox.size]
    dp = wantp["detail"]
    assert np.array_equal(outp["per_realisation"]["length"], dp[..., 3] * 50.0) and np.array_equal(outp["per_realisation"]["n_intercepts"], dp[..., 4])
    assert np.array_equal(outp["probability"], (dp[..., 3] >= 3).sum(0) / float(n))
    assert np.array_equal(outp["thickness"]["p50"], np.quantile(dp[..., 0], 0.5, axis=0, method="inverted_cdf") * 50.0)
    import os
    import pandas as pd
    tab = pd.read_csv(os.path.join(inv.settings.outpath, "hole_intercepts.csv"))
    assert list(tab.columns) == list(ic.HOLE_COLUMNS) and len(tab) == 3 and np.allclose(tab["PROBABILITY"], outp["probability"][:, 0])


def test_column_intercepts_of_the_mean_cube(tiny):
    inv = tiny["inv"]
    cube = np.asarray(tiny["mean"][0], dtype=np.float64)
    cutoff = float(_midpoint_cutoffs(cube, inv._cube_scale[0], k=3)[1])
    region = np.ones(GRID, dtype=bool)
    region[:, :, 5] = False
    F = np.zeros((1, 3, N))
    F[0, 0] = cube.reshape(-1)
    want = ref.trace_stats(F, 0, [cutoff], ref.column_traces(*GRID), mask=region.reshape(-1), min_len=2, max_gap=1)
    got = inv.column_intercepts(cube, cutoff, min_length=200.0, max_gap=100.0, region=region)
    d = want["detail"][0, 0].reshape(8, 10, 6)
    assert set(got) == {"thickness", "depth_to_top", "from", "length", "mean_value", "n_intercepts"}
    assert np.array_equal(got["thickness"], d[..., 0] * DZ) and np.array_equal(got["length"], d[..., 3] * DZ)
    assert np.array_equal(got["n_intercepts"], d[..., 4]) and (d[..., 0] > 0).any() and (d[..., 0] == 0).any()
    assert np.array_equal(np.isnan(got["depth_to_top"]), d[..., 0] == 0) and np.array_equal(got["depth_to_top"][d[..., 0] > 0], d[..., 1][d[..., 0] > 0] * DZ)
    assert np.array_equal(np.isnan(got["from"]), d[..., 3] == 0) and np.array_equal(got["from"][d[..., 3] > 0], d[..., 2][d[..., 3] > 0] * DZ)
    ok = d[..., 3] > 0
    mean_r = want["dsum"][0, 0, :, 1].reshape(8, 10)[ok] / d[..., 3][ok]
    bound = ref.sum_bound(6, want["dabs"][0, 0, :, 1].reshape(8, 10))[ok] / d[..., 3][ok] + 2 * ref.U * np.abs(mean_r)
    assert np.all(np.abs(got["mean_value"][ok] - mean_r) <= bound) and np.isnan(got["mean_value"][~ok]).all()
    with pytest.raises(ValueError):
        inv.column_intercepts(cube[:, :, :5], cutoff)
    with pytest.raises(ValueError):
        inv.column_intercepts(cube, float("nan"))


# ---- 5. a spectral step at 32^3 ------------------------------------------------------------------------------------------------------
def test_drill_intercepts_at_32():
    from geobo_amd.inversion import Inversion
    f = load_golden("oracle32_exp.npz")
    d0 = np.zeros((32, 32, 32))                                 # (this survey has no drill data)
    s = settings_for(32, 32, 32, kernelfunc="exp", gp_coeff=list(PSD_W))
    inv = Inversion(settings=s, method="spectral")
    inv.create_cubegeometry()
    inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    n = 4
    cut = np.quantile(np.asarray(inv.mu_rec).reshape(3, -1)[0] * float(inv._cube_scale[0]), [0.3, 0.6, 0.9]) + 1e-7
    out = inv.drill_intercepts(cut, prop="density", n=n, seed=SEED, min_length=300.0, max_gap=100.0)
    gt = inv.grade_tonnage(cut, prop="density", n=n, seed=SEED)
    assert out["probability"].shape == (3, 32, 32) and np.array_equal(out["count"], gt["count"]) and (gt["count"] > 0).all()
    assert np.all(out["holes_hit"] <= 32 * 32) and np.all(out["longest"] <= 32 * DZ) and np.all(np.diff(out["count"], axis=1) <= 0)
    assert np.all(out["probability"] <= out["probability_any"])
    with pytest.raises(ValueError, match="drill"):
        inv.drill_intercepts(cut, prop="drill", n=2)


# ---- workflow ---------------------------------------------------------------------------------------------------------------------
def test_yaml_key_writes_the_files(tmp_path):
    """YAML key drill_intercepts on the reference's first example (25 x 16 x 16, non-cubic voxels), exponential kernel and the PSD
    weights; the optional sub-key holes adds hole_intercepts.csv."""
    import json
    import os

    import pandas as pd
    import yaml
    from conftest import GOLDEN
    from geobo_amd import intercepts as ic, run_geobo
    f = load_golden("example1.npz")
    d = json.loads(str(f["settings_json"]))
    d.update(inpath=os.path.join(GOLDEN, "data", "synthetic") + "/", outpath=str(tmp_path) + "/", kernelfunc="exp", gp_coeff=list(PSD_W),
             sample_seed=3, drill_intercepts=dict(property="density", cutoffs=[0.05, -0.05, 0.0], samples=6, max_gap=0.0, holes=[[3, 4], [10, 9]]))
    y = tmp_path / "settings.yaml"
    y.write_text(yaml.safe_dump(d))
    out = run_geobo.run(str(y), bayesopt=False)
    got = out["drill_intercepts"]
    inv = out["inversion"]
    s = inv.settings
    again = inv.drill_intercepts([0.05, -0.05, 0.0], prop="density", n=6, seed=3)
    assert got["holes_hit"].shape == (6, 3) and np.array_equal(got["holes_hit"], again["holes_hit"])
    assert np.array_equal(got["accumulation_mean"], again["accumulation_mean"])
    assert np.all(got["count"][:, 1] >= got["count"][:, 2]) and np.all(got["count"][:, 2] >= got["count"][:, 0])
    tab = pd.read_csv(tmp_path / "intercepts.csv")
    assert list(tab.columns) == list(ic.CSV_COLUMNS) and np.array_equal(tab["CUTOFF"], [0.05, -0.05, 0.0])
    assert np.allclose(tab["AREA_P50"], got["quantiles"]["prospective_area"][1], rtol=1e-12, atol=0)
    maps = pd.read_csv(tmp_path / "intercept_maps.csv")
    assert list(maps.columns) == list(ic.MAP_COLUMNS) and len(maps) == 3 * s.yNcube * s.xNcube
    assert np.allclose(maps["PROBABILITY"].to_numpy().reshape(3, s.yNcube, s.xNcube), got["probability"], rtol=1e-12, atol=0)
    assert maps["X"][1] - maps["X"][0] == s.xvoxsize and got["sample_length"] == s.zvoxsize
    holes = pd.read_csv(tmp_path / "hole_intercepts.csv")
    assert list(holes.columns) == list(ic.HOLE_COLUMNS) and len(holes) == 6
    assert np.allclose(holes["PROBABILITY_ANY"].to_numpy().reshape(3, 2), got["probability_any"][:, [4, 9], [3, 10]], rtol=1e-12, atol=0)
    assert np.array_equal(out["drill_intercepts_holes"]["per_realisation"]["thickness"][:, :, 0] > 0,
                          out["drill_intercepts_holes"]["per_realisation"]["n_intercepts"][:, :, 0] > 0)


# ---- 6. error paths -------------------------------------------------------------------------------------------------------------
def test_error_paths(tiny, monkeypatch):
    from geobo_amd.inversion import Inversion
    inv = tiny["inv"]
    with pytest.raises(RuntimeError, match="cubing"):
        Inversion(settings=settings_for(**TINY)).drill_intercepts([0.0], prop="density")
    with pytest.raises(ValueError):
        inv.drill_intercepts(np.arange(33.0), prop="density", n=2)
    with pytest.raises(ValueError, match="region"):
        inv.drill_intercepts([0.0], prop="density", n=2, region=np.ones((10, 8, 6), dtype=bool))
    with pytest.raises(ValueError, match="require"):
        inv.drill_intercepts([0.0], prop="density", n=2, require={"density": 0.0})
    with pytest.raises(ValueError, match="holes or paths"):
        inv.drill_intercepts([0.0], prop="density", n=2, holes=[(1, 1)], paths=[(310.0, 420.0, 35.0, 60.0)])
    with pytest.raises(ValueError):
        inv.drill_intercepts([0.0], prop="density", n=2, holes=[(10, 1)])
    with pytest.raises(ValueError):
        inv.drill_intercepts([0.0], prop="density", n=2, min_length=0.0)
    with pytest.raises(ValueError):
        inv.drill_intercepts([0.0], prop="density", n=2, max_gap=-1.0)
    f = load_golden("tiny_exp_nodrill.npz")
    nod = Inversion(settings=settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W)))
    nod.create_cubegeometry()
    nod.gp_length = np.array([200.0, 204.0, 208.0])
    d0 = f["drilldata0"]
    nod.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    with pytest.raises(ValueError, match="drill"):
        nod.drill_intercepts([0.0], prop="drill", n=2)
    with pytest.raises(ValueError, match="drill"):
        nod.drill_intercepts([0.0], prop="density", n=2, require={"drill": 0.0})
    monkeypatch.setattr(inv.engine, "world", 2)
    with pytest.raises(NotImplementedError):
        inv.drill_intercepts([0.0], prop="density", n=2)
    with pytest.raises(NotImplementedError):
        inv.engine.trace_statistics(torch.zeros((1, 3, N), dtype=torch.float64, device="cuda"), 0, [0.0])
