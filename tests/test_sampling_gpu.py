"""Posterior realisations on the device: the Philox generator against NumPy, the torus tables and spectra against
the oracle's block tables, the sampler against a NumPy inverse FFT of the same noise, prior and posterior statistics against the oracle's
dense covariances, Matheron's rule against the oracle's dense formula, determinism, and the conditioning identity at 32^3 and 64^3.

Statistical tests: seed 2026, S = 8192 samples, 10 x 8 x 6 voxels of 100 m, gp_coeff (0.2, 0.2, 0.2) (a PSD prior)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, normwise, settings_for
from oracle import geobo_oracle as O
from test_sampling_cpu import numpy_block

pytestmark = pytest.mark.gpu

SEED = 2026
PSD_W = (0.2, 0.2, 0.2)
TINY = dict(nx=10, ny=8, nz=6)


def _inv(s, **kw):
    from geobo_amd.inversion import Inversion
    inv = Inversion(settings=s, **kw)
    inv.create_cubegeometry()
    return inv


def _sampler(s, lengths, w, amp=1.0, **kw):
    from geobo_amd.engine import weight_matrix
    from geobo_amd.sampling import PriorSampler
    return PriorSampler((s.yNcube, s.xNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize), s.kernelfunc, lengths, weight_matrix(w), amp, **kw)


def _oracle_K(s, lengths, w, amp=1.0):
    P3 = O.grid_points((s.xNcube, s.yNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize))
    D2 = O.sqdist(P3)
    W = O.weight_matrix(w)
    return amp * np.vstack([np.hstack([O.k_block(s.kernelfunc, D2, np.asarray(lengths), W, i, j) for j in range(3)]) for i in range(3)])


# ---- 1. RNG ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,purpose,sample0,elem0", [(0, 0, 0, 1), (SEED, 0, 7, 1000), (2 ** 40 + 3, 1, 3, 0), (5, 1, 0, 2 ** 33)])
def test_philox_words_and_normals_match_numpy(seed, purpose, sample0, elem0):
    from geobo_amd import hip
    ns, ne = 3, 37
    raw = hip.philox_fill(seed, purpose, sample0, ns, elem0, ne, raw=True).cpu().numpy().view(np.uint64)
    nrm = hip.philox_fill(seed, purpose, sample0, ns, elem0, ne).cpu().numpy()
    for s in range(ns):
        for e in range(ne):
            ref = numpy_block(seed, (elem0 + e, sample0 + s, purpose, 0))
            assert [int(v) for v in raw[s, e]] == ref
            u = (np.array(ref, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) + 0.5
            u *= 2.0 ** -53
            r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
            want = np.array([r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])])
            amp = np.array([r0, r0, r1, r1])
            assert np.all(np.abs(nrm[s, e] - want) <= 1e-15 * amp), (s, e)


# ---- 2. tables and spectra -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["exp", "matern32", "sparse"])
def test_torus_tables_and_spectra(kern):
    from geobo_amd import hip
    from geobo_amd.engine import PosteriorEngine, weight_matrix
    s = settings_for(**TINY, kernelfunc=kern)
    lengths = [200.0, 210.0, 220.0]
    smp = _sampler(s, lengths, PSD_W, 1.3, approximate=True)
    my, mx, mz = smp.ext
    M = my * mx * mz
    ny, nx, nz = smp.grid
    eng = PosteriorEngine(s)
    N = nx * ny * nz
    xyz = tuple(c[:N].contiguous() for c in eng.grid_points())
    W = weight_matrix(PSD_W)
    ax = [np.minimum(np.arange(m), m - np.arange(m)) * v for m, v in zip(smp.ext, (s.yvoxsize, s.xvoxsize, s.zvoxsize))]
    dy, dx, dz = np.meshgrid(*ax, indexing="ij")
    d2 = dy ** 2 + dx ** 2 + dz ** 2
    Wo = O.weight_matrix(PSD_W)
    spec = smp.spectra.view(len(smp.pairs), M, 2).cpu().numpy()
    tab = smp.table.view(len(smp.pairs), my, mx, mz, 2).cpu().numpy()
    for p, (i, j) in enumerate(smp.pairs):
        # crop of the torus table = the covariance from voxel 0 to every voxel: geobo_k_block's row 0, bit for bit
        row = torch.empty((1, N), dtype=torch.float64, device="cuda")
        hip.k_block(hip.kernel_id(kern, i != j), tuple(c[:1] for c in xyz), xyz, lengths[j], lengths[i], W[i][j], 1.3, row)
        assert np.array_equal(tab[p, :ny, :nx, :nz, 0].reshape(-1), row.cpu().numpy()[0]), (i, j)
        assert not tab[p, ..., 1].any()
        ref = np.fft.fftn(1.3 * O.k_block(kern, d2, np.asarray(lengths), Wo, i, j))
        assert np.abs(spec[p, :, 0] + 1j * spec[p, :, 1] - ref.reshape(-1)).max() <= 1e-12 * np.abs(ref).max(), (i, j)


# ---- 3. sampler with the caller's noise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(10, 8, 6), (16, 16, 16), (7, 12, 5)])
def test_sampler_equals_numpy_ifft_of_the_same_noise(dims):
    nx, ny, nz = dims
    s = settings_for(nx, ny, nz, kernelfunc="matern32")
    smp = _sampler(s, [200.0, 210.0, 220.0], PSD_W, approximate=True)
    my, mx, mz = smp.ext
    M, P, N = my * mx * mz, 3, nx * ny * nz
    rng = np.random.default_rng(11)
    npairs = 3
    xi = rng.standard_normal((npairs, M, P)) + 1j * rng.standard_normal((npairs, M, P))
    noise = torch.as_tensor(np.stack([xi.real, xi.imag], -1).reshape(-1), device="cuda")
    got = smp.sample(0, 2 * npairs - 1, noise=noise).cpu().numpy()            # odd count: the last pair's imaginary part is dropped
    Fo = smp.F.view(my // 2 + 1, mx // 2 + 1, mz // 2 + 1, P, P).cpu().numpy()
    fold = lambda m: np.minimum(np.arange(m), m - np.arange(m))
    Ff = Fo[np.ix_(fold(my), fold(mx), fold(mz))]                               # (my, mx, mz, P, P)
    for k in range(npairs):
        y = np.einsum("yxziq,yxzq->iyxz", Ff, xi[k].reshape(my, mx, mz, P)) / np.sqrt(M)
        f = np.fft.ifftn(y, axes=(1, 2, 3)) * M
        f = f[:, :ny, :nx, :nz].reshape(P, N)
        scale = np.abs(f).max()
        assert np.abs(got[2 * k] - f.real).max() <= 1e-12 * scale
        if 2 * k + 1 < got.shape[0]:
            assert np.abs(got[2 * k + 1] - f.imag).max() <= 1e-12 * scale


# ---- 4. prior statistics ---------------------------------------------------------------------------------------------------------
def test_prior_covariance_statistics():
    s = settings_for(**TINY, kernelfunc="exp")
    lengths = [200.0, 204.0, 208.0]
    S = 8192
    smp = _sampler(s, lengths, PSD_W)
    X = smp.sample(0, S, seed=SEED).reshape(S, -1).cpu().numpy()
    K = _oracle_K(s, lengths, PSD_W)
    C = X.T @ X / S
    d = np.diag(K)
    sd = np.sqrt((np.outer(d, d) + K ** 2) / S)
    assert np.all(np.abs(C - K) <= 6 * sd), float((np.abs(C - K) / sd).max())
    expect = np.sqrt(((np.outer(d, d) + K ** 2) / S).sum())
    fro = np.linalg.norm(C - K)
    print("prior: relative Frobenius error %.3e, expectation %.3e" % (fro / np.linalg.norm(K), expect / np.linalg.norm(K)))
    assert fro <= 1.5 * expect


# ---- 5. Matheron's rule is exact -------------------------------------------------------------------------------------------------
def _host_operator(eng, A):
    from geobo_amd.operators import StreamedOperator
    if not isinstance(A, StreamedOperator):
        return A[:eng.Ms, :eng.N].cpu().numpy()
    buf = torch.empty((256, eng.N_pad), dtype=torch.float64, device="cuda")
    return np.vstack([A.rows_into(buf, r0, min(256, eng.Ms - r0))[:, :eng.N].cpu().numpy() for r0 in range(0, eng.Ms, 256)])


def _matheron_case(inv, f, n=3, seed=4):
    """sample_posterior(prior=f, noise=eps) against f + K A3^T H^-1 (y - A3 f - eps) in float64 SciPy with the engine's own operators."""
    from scipy.linalg import cho_factor, cho_solve
    s = inv.settings
    d0 = f["drilldata0"]
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    eng = inv.engine
    A_g, A_m = (_host_operator(eng, A) for A in inv._operators())
    N, sel = eng.N, inv._sel
    rng = np.random.default_rng(seed)
    mg, mm, md = A_g.shape[0], A_m.shape[0], sel.size
    lengths = np.array(inv.gp_length, dtype=float)
    K = _oracle_K(s, lengths, inv.coeffm, inv.gp_amp)
    L = np.linalg.cholesky(K + 1e-9 * np.eye(3 * N)) if np.linalg.eigvalsh(K).min() > 0 else None
    fpr = (L @ rng.standard_normal((3 * N, n))).T if L is not None else rng.standard_normal((n, 3 * N))
    sig = O._noise(inv.gp_sigma, mg, mm, md)
    eps = rng.standard_normal((n, mg + mm + md)) * sig
    A3 = np.zeros((mg + mm + md, 3 * N))
    A3[:mg, :N], A3[mg:mg + mm, N:2 * N] = A_g, A_m
    A3[mg + mm + np.arange(md), 2 * N + sel] = 1.0
    H = A3 @ K @ A3.T + np.diag(sig ** 2)
    R = inv.Fs3[None, :] - fpr @ A3.T - eps
    want = fpr + (K @ A3.T @ cho_solve(cho_factor(H, lower=True), R.T)).T
    got = inv.sample_posterior(n, prior=fpr.reshape(n, 3, N), noise=eps)
    got = np.stack([got[i].reshape(n, N) / inv._cube_scale[i] for i in range(3)], 1)
    # (a survey without drill data has no drill std: cubing's drill cubes are NaN, and so are the samples' in data units)
    keep = [i for i in range(3) if np.isfinite(inv._cube_scale[i])]
    err = normwise(got[:, keep], want.reshape(n, 3, N)[:, keep])
    print("Matheron %s [%s]: %.2e" % (s.kernelfunc, eng.step_route, err))
    return err


@pytest.mark.parametrize("name,method,rows", [("tiny_exp", "auto", False), ("tiny_sparse", "auto", False), ("tiny_matern32", "auto", False),
                                              ("tiny_exp", "auto", True), ("cube16_matern32", "spectral", False),
                                              ("cube16_matern32", "dense", False), ("cube16_matern32", "spectral", True),
                                              ("cube16_exp", "spectral", True)])
def test_matheron_is_exact(name, method, rows, monkeypatch):
    if rows:
        monkeypatch.setenv("GEOBO_ROWS", "1")
    f = load_golden(name + ".npz")
    dims = TINY if name.startswith("tiny") else dict(nx=16, ny=16, nz=16)
    s = settings_for(**dims, kernelfunc=name.split("_")[1])
    inv = _inv(s, method=method)
    inv.gp_length = f["gp_length_in"].copy()
    assert _matheron_case(inv, f) <= 1e-10


# ---- 6. posterior statistics -----------------------------------------------------------------------------------------------------
def test_posterior_statistics_joint():
    f = load_golden("tiny_exp.npz")
    s = settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W))
    inv = _inv(s)
    inv.gp_length = np.array([200.0, 204.0, 208.0])
    d0 = f["drilldata0"]
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    N, S = 480, 8192
    got = inv.sample_posterior(S, seed=SEED, batch=256)
    X = np.stack([got[i].reshape(S, N) / inv._cube_scale[i] for i in range(3)], 1).reshape(S, 3 * N)
    # the oracle's dense posterior with the engine's operators
    eng = inv.engine
    A_g, A_m = (_host_operator(eng, A) for A in inv._operators())
    P3 = O.grid_points((10, 8, 6), (100.0, 100.0, 100.0))
    ref = O.posterior_dense(P3, A_g, A_m, inv._sel, inv.Fs3, np.array(inv.gp_length), O.weight_matrix(PSD_W), "exp", inv.gp_sigma,
                            return_cov=True)
    mu, cov = ref["mu"], ref["cov"]
    var = np.diag(cov)
    assert normwise(inv.mu_rec, mu) <= 1e-8
    m = X.mean(0)
    assert np.all(np.abs(m - mu) <= 6 * np.sqrt(var / S))
    v = X.var(0, ddof=1)
    assert np.all(np.abs(v - var) <= 6 * var * np.sqrt(2.0 / (S - 1)))
    # variance of the sum over a 3 x 3 x 3 block of density voxels: a joint property of the samples
    idx = np.array([(iy * 10 + ix) * 6 + iz for iy in range(3, 6) for ix in range(4, 7) for iz in range(1, 4)])
    one = np.zeros(3 * N)
    one[idx] = 1.0
    vb = float(one @ cov @ one)
    sums = X[:, idx].sum(1)
    vs = sums.var(ddof=1)
    print("block-sum variance %.4e vs oracle %.4e (marginals only: %.4e)" % (vs, vb, var[idx].sum()))
    assert abs(vs - vb) <= 6 * vb * np.sqrt(2.0 / (S - 1))
    assert abs(var[idx].sum() - vb) > 12 * vb * np.sqrt(2.0 / (S - 1))     # marginal-only sampling would fail this check


# ---- 7. determinism --------------------------------------------------------------------------------------------------------------
def test_determinism_and_addressing():
    f = load_golden("tiny_exp.npz")
    s = settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W))
    inv = _inv(s)
    inv.gp_length = np.array([200.0, 204.0, 208.0])
    d0 = f["drilldata0"]
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    a = inv.sample_posterior(64, seed=9)
    b = inv.sample_posterior(64, seed=9, batch=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for k in (0, 13, 63):
        one = inv.sample_posterior(1, seed=9, start=k)
        assert all(np.array_equal(x[k], y[0]) for x, y in zip(a, one)), k
    c = inv.sample_posterior(4, seed=10)
    assert not np.array_equal(a[0][:4], c[0])
    p = inv.sample_prior(8, seed=9)
    q = inv.sample_prior(3, seed=9, start=5)
    assert all(np.array_equal(x[5:], y) for x, y in zip(p, q))


def test_sample_posterior_needs_cubing():
    s = settings_for(**TINY, kernelfunc="exp", gp_coeff=list(PSD_W))
    with pytest.raises(RuntimeError, match="cubing"):
        _inv(s).sample_posterior(2)


# ---- 8. at size ------------------------------------------------------------------------------------------------------------------
def _identity_residual(inv, got):
    """||A3 f_post + eps + Sigma w - y|| / ||y|| per sample (device operators)."""
    eng = inv.engine
    A_g, A_m = inv._operators()
    info = inv.sample_info
    N, sel, y = eng.N, inv._sel, inv.Fs3
    ng, nm = inv.gravfield.size, inv.magfield.size
    sig = O._noise(inv.gp_sigma, ng, nm, sel.size)
    out = []
    for k in range(got[0].shape[0]):
        fk = [got[i][k].reshape(-1) / inv._cube_scale[i] for i in range(3)]
        a3f = np.concatenate([eng.apply_operator(A_g, fk[0]).cpu().numpy(), eng.apply_operator(A_m, fk[1]).cpu().numpy(), fk[2][sel]])
        out.append(np.linalg.norm(a3f + info["noise"][k] + sig ** 2 * info["w"][k] - y) / np.linalg.norm(y))
    return max(out)


def test_conditioning_identity_at_32_and_routes_agree():
    f = load_golden("oracle32_matern32.npz")
    d0 = np.zeros(32 ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(32, 32, 32)
    res = {}
    for method in ("spectral", "dense"):
        s = settings_for(32, 32, 32, kernelfunc="matern32", gp_coeff=list(PSD_W))
        inv = _inv(s, method=method)
        inv.gp_length = f["gp_length_in"].copy()
        inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
        got = inv.sample_posterior(4, seed=SEED)
        assert all(np.isfinite(g).all() for g in got)
        r = _identity_residual(inv, got)
        print("32^3 [%s]: identity residual %.2e" % (method, r))
        assert r <= 1e-9
        res[method] = got
    assert max(normwise(a, b) for a, b in zip(res["spectral"], res["dense"])) <= 1e-10


def test_conditioning_identity_and_prior_variance_at_64():
    from geobo_amd.config_loader import Settings
    f = load_golden("oracle64_sample_matern32.npz")
    n = 64
    s = Settings(dict(xmax=100.0 * n, ymax=100.0 * n, zLcube=100.0 * n, xNcube=n, yNcube=n, zNcube=n, kernelfunc="matern32",
                      gp_coeff=list(PSD_W)))
    d0 = np.zeros(n ** 3)
    d0[f["sel"]] = f["drillvalues"]
    d0 = d0.reshape(n, n, n)
    inv = _inv(s)
    inv.gp_length = f["gp_length_in"].copy()
    inv.cubing(f["gravfield"], f["magfield"], d0[d0 != 0], f["sensor_locations"], d0)
    got = inv.sample_posterior(2, seed=SEED)
    assert all(np.isfinite(g).all() for g in got)
    r = _identity_residual(inv, got)
    print("64^3: identity residual %.2e" % r)
    assert r <= 1e-9
    prior = inv.sample_prior(1, seed=SEED)
    for i in range(3):
        v = float(prior[i][0].var())
        print("64^3 prior block %d: spatial variance %.4f (K(0) = 1)" % (i, v))
        assert abs(v - 1.0) <= 0.05


# ---- 9. indefinite prior ---------------------------------------------------------------------------------------------------------
def test_indefinite_prior_raises_or_clips():
    from geobo_amd.sampling import SamplingError
    s = settings_for(8, 8, 8, kernelfunc="exp")                 # default gp_coeff (1.0, 0.2, 0.2)
    inv = _inv(s)
    inv.gp_length = np.array([200.0, 204.0, 208.0])
    with pytest.raises(SamplingError, match=r"ratio -[0-9.]+e-0[0-9].*w1 = 1"):
        inv.sample_prior(2)
    *cubes, frac = inv.sample_prior(4, approximate=True)
    assert len(cubes) == 3 and all(np.isfinite(c).all() and c.shape == (4, 8, 8, 8) for c in cubes)
    print("clipped fraction %.3e" % frac)
    assert frac > 0
