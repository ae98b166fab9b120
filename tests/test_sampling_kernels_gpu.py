"""The entry points of csrc/sampling.hip by value, against the plain references of tests/_sampling_ref.py:
geobo_fft_axis at every length it accepts and at its tile edges, geobo_sample_factor on constructed spectra, geobo_sample_zpass with
the caller's noise and with its own Philox addressing, geobo_spectral_mix, PriorSampler.apply_K against a dense covariance, and the
assembled sampler and its factors on tori of 128, 256 and 512 points per axis.

Tolerances are of two kinds only.  (a) Measured in the test: the error of the reference's own fp64 competitor (np.fft, np.linalg.eigh,
NumPy's circulant product) against the same high-precision reference, floored at the fp64 eps, times MARGIN = 16.  A radix-4 Stockham
FFT with exact sincospi twiddles has at most ceil(log4 m) + 1 rounding stages and pocketfft the same order; 16 covers a different
factorisation and stays below the smallest structural error (one twiddle index off at m = 512 is 2 pi / 512).  (b) The project's
existing bound 1e-12 on the spectra and the samples (tests/test_sampling_gpu.py), quoted as such.  spectral_mix alone has an analytic
bound: 4 eps sum_j |lambda_ij| |in_j|, the forward error of a three-term dot product and one scaling.

FFT errors are max-norm per line, relative to the maximum of the whole length-m reference line (also where only n_out < m outputs are
kept): an FFT's error bound is normwise over the transform, and a single kept output may be small by cancellation."""
import math

import numpy as np
import pytest
import torch

import _sampling_ref as R
from conftest import settings_for
from oracle import geobo_oracle as O
from test_sampling_gpu import PSD_W, _oracle_K, _sampler

pytestmark = pytest.mark.gpu

EPS = R.EPS
MARGIN = 16.0
GUARD = 64            # doubles of NaN in front of and behind every output
LENGTHS = [2, 4, 8, 16, 32, 64, 128, 256, 512]
LD = np.longdouble


def _interleave(z):
    z = np.asarray(z)
    return np.stack([z.real, z.imag], -1).astype(np.float64).reshape(-1)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _guarded(n, tail=0):
    """NaN buffer of GUARD + n + tail + GUARD doubles and its view of n (+ tail) doubles."""
    buf = torch.full((2 * GUARD + n + tail,), float("nan"), dtype=torch.float64, device="cuda")
    return buf, buf[GUARD:GUARD + n + tail]


def _untouched(buf, n):
    """Everything outside [GUARD, GUARD + n) of the guarded buffer is still NaN and everything inside was written."""
    h = buf.cpu().numpy()
    return bool(np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + n:]).all() and not np.isnan(h[GUARD:GUARD + n]).any())


def _complex(h, shape):
    h = np.asarray(h).reshape(shape + (2,))
    return h[..., 0] + 1j * h[..., 1]


def _line_errors(got, npf, full, n_out, axis):
    """Per line: (error of the kernel, error of np.fft), max-norm over the kept outputs relative to the max of the whole line."""
    ref = np.take(full, np.arange(n_out), axis=axis)
    scale = np.abs(full).max(axis=axis)
    scale = np.where(scale > 0, scale, LD(1))
    e_k = (np.abs(got - ref).max(axis=axis) / scale).astype(np.float64)
    e_np = (np.abs(npf - ref).max(axis=axis) / scale).astype(np.float64)
    return e_k, e_np


# ---- 1. geobo_fft_axis -----------------------------------------------------------------------------------------------------------
def _fft_layouts(m, hip):
    C = hip.require_gpu().geobo_fft_lines(m, 1)
    assert C == 4096 // m
    full = [(b0, 1) for b0 in (1, C, C + 3)]
    cols = []
    for b1 in (2, 3, C - 1, C, C + 5, 2 * C + 1):
        b1 = min(b1, 300)
        if b1 >= 2 and b1 not in cols:
            cols.append(b1)
    full += [(b0, b1) for b1 in cols for b0 in (1, 3)]
    cuts = [(C + 3, 1), (3, min(C + 5, 300)), (1, max(min(C - 1, 300), 2))]
    return full, cuts


def _fft_extents(m):
    ins = sorted({m, m // 2 + 1, 1}, reverse=True)
    outs = sorted({m, m // 2, 1}, reverse=True)
    return [(a, b) for a in ins for b in outs]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("m", LENGTHS)
def test_fft_axis_by_value(m, inverse):
    from geobo_amd import hip
    rng = np.random.default_rng(1000 + 2 * m + inverse)
    full, cuts = _fft_layouts(m, hip)
    cases = [(b0, b1, m, m) for b0, b1 in full]
    cases += [(b0, b1, n_in, n_out) for b0, b1 in cuts for n_in, n_out in _fft_extents(m) if (n_in, n_out) != (m, m)]
    assert any(n_in < m and n_out < m for _, _, n_in, n_out in cases) or m == 2
    worst, worst_np, bad = 0.0, 0.0, []
    for b0, b1, n_in, n_out in cases:
        x = rng.standard_normal((b0, n_in, b1)) + 1j * rng.standard_normal((b0, n_in, b1))
        n = 2 * b0 * n_out * b1
        buf, out = _guarded(n)
        hip.fft_axis(hip.FFT_INVERSE if inverse else 0, b0, m, b1, n_in, n_out, _dev(_interleave(x)), out)
        torch.cuda.synchronize()
        if not _untouched(buf, n):
            bad.append((b0, b1, n_in, n_out, "wrote outside its extent or left a hole"))
            continue
        got = _complex(out.cpu().numpy(), (b0, n_out, b1))
        ref_full = R.pad_crop(x, n_in, m, m, axis=1, inverse=inverse)
        xp = np.zeros((b0, m, b1), dtype=complex)
        xp[:, :n_in] = x
        npf = (np.fft.ifft(xp, axis=1) * m if inverse else np.fft.fft(xp, axis=1))[:, :n_out]
        e_k, e_np = _line_errors(got, npf, ref_full, n_out, 1)
        ratio = e_k / np.maximum(e_np, EPS)
        worst, worst_np = max(worst, float(ratio.max())), max(worst_np, float(e_np.max()))
        if not np.all(ratio <= MARGIN):
            bad.append((b0, b1, n_in, n_out, "ratio %.3g, error %.3g" % (ratio.max(), e_k.max())))
    print("fft_axis m = %d %s: worst error / max(e_np, eps) = %.2f over %d cases (largest e_np %.2e)"
          % (m, "inverse" if inverse else "forward", worst, len(cases), worst_np))
    assert not bad, bad


# the three passes that use the pair flags, on two small grids (ny, nx, nz) with their tori, and one pass with both flags
PAIR_GRIDS = [((5, 3, 6), (16, 8, 16)), ((3, 2, 40), (8, 4, 128))]


@pytest.mark.parametrize("S", [1, 2, 5, 6])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("grid,ext", PAIR_GRIDS, ids=["z16", "z128"])
@pytest.mark.parametrize("which", ["apply_K_first", "apply_K_last", "sample_last", "both"])
def test_fft_axis_pair_flags(which, grid, ext, P, S):
    from geobo_amd import hip
    (ny, nx, nz), (my, mx, mz) = grid, ext
    N, K = ny * nx * nz, (S + 1) // 2
    rng = np.random.default_rng([len(which), ny, P, S])
    slot = P * N                                              # doubles of one sample
    if which in ("apply_K_first", "both"):
        # real (S, P, N) in, zero padded along z; "both" writes the same packing, else complex [K P ny nx][mz]
        m, n_in, n_out = mz, nz, (nz if which == "both" else mz)
        flags = hip.FFT_IN_PAIRS | (hip.FFT_OUT_PAIRS if which == "both" else 0)
        v = rng.standard_normal((S, P, N))
        src = torch.full((S * slot + slot,), float("nan"), dtype=torch.float64, device="cuda")   # the missing sample's slot: NaN
        src[:S * slot] = _dev(v.reshape(-1))
        z = R.unpack_pairs(v).reshape(K * P * ny * nx, nz)
        inverse, b0, b1, axis = False, K * P * ny * nx, 1, 1
    elif which == "apply_K_last":
        m, n_in, n_out, flags = mz, mz, nz, hip.FFT_INVERSE | hip.FFT_OUT_PAIRS
        z = rng.standard_normal((K * P * ny * nx, mz)) + 1j * rng.standard_normal((K * P * ny * nx, mz))
        src = _dev(_interleave(z))
        inverse, b0, b1, axis = True, K * P * ny * nx, 1, 1
    else:
        m, n_in, n_out, flags = my, my, ny, hip.FFT_INVERSE | hip.FFT_OUT_PAIRS
        z = rng.standard_normal((K * P, my, nx * nz)) + 1j * rng.standard_normal((K * P, my, nx * nz))
        src = _dev(_interleave(z))
        inverse, b0, b1, axis = True, K * P, nx * nz, 1
    packed_out = bool(flags & hip.FFT_OUT_PAIRS)
    n = S * slot if packed_out else 2 * b0 * n_out * b1
    buf, out = _guarded(n, tail=slot if packed_out else 0)    # behind a packed output: room for the sample that must not be written
    hip.fft_axis(flags, b0, m, b1, n_in, n_out, src, out, P=P, Q=N, S=S)
    torch.cuda.synchronize()
    assert _untouched(buf, n), "wrote outside the (S, P, Q) extent (the missing sample's slot included) or left a hole"
    zz = z.reshape(b0, n_in, b1)
    full = R.pad_crop(zz, n_in, m, m, axis=axis, inverse=inverse)
    xp = np.zeros((b0, m, b1), dtype=complex)
    xp[:, :n_in] = zz
    npf = (np.fft.ifft(xp, axis=1) * m if inverse else np.fft.fft(xp, axis=1))[:, :n_out]
    ref = full[:, :n_out].copy()
    h = out[:n].cpu().numpy()
    if packed_out:
        got = R.unpack_pairs(h.reshape(S, P, N)).reshape(b0, n_out, b1)       # lines [K][P][...]: the layout of the complex side
        if S % 2:                                  # the last pair's imaginary part has no slot: its lines compare real parts only
            last = slice((K - 1) * (b0 // K), b0)
            ref[last], npf[last] = ref[last].real, npf[last].real
    else:
        got = _complex(h, (b0, n_out, b1))
    scale = np.abs(full).max(axis=1)
    e_k = (np.abs(got - ref).max(axis=1) / scale).astype(np.float64)
    e_np = (np.abs(npf - ref).max(axis=1) / scale).astype(np.float64)
    assert np.isfinite(e_k).all(), "the missing imaginary sample's slot was read into the result"
    ratio = e_k / np.maximum(e_np, EPS)
    print("fft_axis pairs %s m = %d P = %d S = %d: worst ratio %.2f" % (which, m, P, S, ratio.max()))
    assert np.all(ratio <= MARGIN), float(ratio.max())


# ---- 2. geobo_sample_factor ------------------------------------------------------------------------------------------------------
FAMILIES = ["decades", "rank2", "rank1", "diag", "zero", "cI", "two_equal", "indefinite", "tiny_off", "tiny_off_mixed", "mixed"]


def _rotation(rng, P):
    q, r = np.linalg.qr(rng.standard_normal((P, P)))
    return q * np.sign(np.diag(r))


def _family(name, P, n, rng):
    """n symmetric P x P matrices of one family."""
    out = np.zeros((n, P, P))
    for o in range(n):
        B = rng.standard_normal((P, P))
        if name == "decades":                      # magnitudes over ten decades from frequency to frequency
            S = (B @ B.T) * 10.0 ** rng.uniform(-5, 5)
        elif name in ("rank2", "rank1"):           # exactly singular for P = 3 (rank1 also for P = 2)
            Br = rng.standard_normal((P, 2 if name == "rank2" else 1))
            S = Br @ Br.T
        elif name == "diag":                       # no rotation at all: a[p][q] == 0 everywhere; negative and zero entries
            d = rng.standard_normal(P)
            d[o % P] = 0.0 if o % 3 == 0 else d[o % P]
            S = np.diag(d)
        elif name == "zero":                       # tot == 0
            S = np.zeros((P, P))
        elif name == "cI":
            S = rng.standard_normal() * np.eye(P)
        elif name == "two_equal":                  # a repeated eigenvalue and a rotated third
            a, b = rng.uniform(0.5, 2.0), rng.uniform(-1.0, 3.0)
            Q = _rotation(rng, P)
            S = Q @ np.diag(([a, a, b])[:P] if P == 3 else [a] * P) @ Q.T
        elif name == "indefinite":
            S = B @ B.T
            S = S - 0.5 * np.trace(S) / P * np.eye(P)
        elif name == "tiny_off":                   # tau = (a_qq - a_pp) / (2e-200): its square overflows
            S = np.diag(np.arange(1.0, P + 1) * rng.uniform(0.5, 2.0)) + 1e-200 * (1 - np.eye(P))
        elif name == "tiny_off_mixed":             # one rotation of order one keeps the sweep going over the 1e-200 pairs
            S = np.diag(np.arange(1.0, P + 1) * rng.uniform(0.5, 2.0)) + 1e-200 * (1 - np.eye(P))
            S[0, P - 1] = S[P - 1, 0] = 0.5 if P > 1 else S[0, 0]
        else:
            raise KeyError(name)
        out[o] = (S + S.T) / 2
    return out


def _octant_spectra(name, P, ext, rng):
    hy, hx, hz = (m // 2 + 1 for m in ext)
    n = hy * hx * hz
    if name != "mixed":
        return _family(name, P, n, rng).reshape(hy, hx, hz, P, P)
    fams = FAMILIES[:-1]
    S = np.zeros((n, P, P))
    pick = rng.permutation(n) % len(fams)
    for f, fam in enumerate(fams):
        idx = np.flatnonzero(pick == f)
        if idx.size:
            S[idx] = _family(fam, P, idx.size, rng)
    return S.reshape(hy, hx, hz, P, P)


def _run_factor(P, ext, S_full_real, S_full_imag=None):
    """geobo_sample_factor on spectra whose real parts are S_full_real (my, mx, mz, P, P); returns F (no, P, P), lam (no, NP), status."""
    from geobo_amd import hip
    my, mx, mz = ext
    M = my * mx * mz
    pairs = [(i, j) for i in range(P) for j in range(i, P)]
    spec = np.empty((len(pairs), M, 2))
    for p, (i, j) in enumerate(pairs):
        spec[p, :, 0] = S_full_real[..., i, j].reshape(-1)
        spec[p, :, 1] = np.nan if S_full_imag is None else S_full_imag[..., i, j].reshape(-1)
    no = (my // 2 + 1) * (mx // 2 + 1) * (mz // 2 + 1)
    bF, F = _guarded(no * P * P)
    bl, lam = _guarded(no * len(pairs))
    ws = torch.empty(hip.sample_factor_ws_doubles(), dtype=torch.float64, device="cuda")
    bs, st = _guarded(4)
    hip.sample_factor(P, my, mx, mz, _dev(spec.reshape(-1)), F, lam, ws, st)
    torch.cuda.synchronize()
    assert _untouched(bF, no * P * P) and _untouched(bl, no * len(pairs)) and _untouched(bs, 4), \
        "F, lam or status: NaN inside (an imaginary part was read) or a write outside the extent"
    return F.cpu().numpy().reshape(no, P, P), lam.cpu().numpy().reshape(no, len(pairs)), st.cpu().numpy(), pairs


def _check_factor(F, status, S_oct, S_full, extra=0.0, extra_sum=0.0, tag=""):
    """F F^T = psd_part(S) per octant frequency and the status word against eigvalsh: min and max over the octant, both traces over
    the FULL torus (unweighted), so the kernel's multiplicity weights are checked independently.  extra: added per frequency."""
    n, P = S_oct.shape[0], S_oct.shape[-1]
    psd, w, recon = R.psd_part(S_oct)
    smax = np.abs(S_oct).max(axis=(1, 2))
    tol = MARGIN * np.maximum(recon, EPS * smax) + extra
    err = np.abs(np.einsum("oik,ojk->oij", F, F) - psd).max(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    _, wf, reconf = R.psd_part(S_full.reshape(-1, P, P))
    tol_e = MARGIN * max(float(recon.max()), EPS * float(smax.max())) + extra
    tr, clip = math.fsum(wf.reshape(-1)), math.fsum(-wf[wf < 0])
    tol_t = MARGIN * max(P * math.fsum(reconf), EPS * math.fsum(np.abs(wf).reshape(-1))) + extra_sum
    d = [abs(status[0] - w.min()), abs(status[1] - w.max()), abs(status[2] - clip), abs(status[3] - tr)]
    r_st = [d[0] / tol_e if tol_e else d[0], d[1] / tol_e if tol_e else d[1], d[2] / tol_t if tol_t else d[2], d[3] / tol_t if tol_t else d[3]]
    print("sample_factor %s: F F^T worst error / tolerance %.3f; status (min, max, clipped, trace) error / tolerance %s"
          % (tag, ratio.max(), ", ".join("%.3f" % v for v in r_st)))
    assert np.all(err <= tol), (int(np.argmax(ratio)), float(ratio.max()))
    assert d[0] <= tol_e and d[1] <= tol_e, (status[:2], w.min(), w.max())
    assert d[2] <= tol_t and d[3] <= tol_t, (status[2:], clip, tr, tol_t)
    return float(ratio.max()), max(r_st)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("ext", [(16, 8, 32), (4, 2, 64), (2, 2, 2)], ids=lambda e: "x".join(map(str, e)))
def test_sample_factor_by_value(ext, P, family):
    """Constructed spectra, no covariance kernel involved.  The families "two_equal" and "mixed" are the ones that found the Jacobi
    loop rotating on rounding noise (1.0 to 1.6 times the tolerance before the negligible-entry rule, at most 0.67 with it)."""
    rng = np.random.default_rng([*ext, P, FAMILIES.index(family)])
    S_oct = _octant_spectra(family, P, ext, rng)
    S_full = R.octant_expand(S_oct, ext)
    F, lam, status, pairs = _run_factor(P, ext, S_full)           # imaginary parts NaN: only the real parts may be read
    S_oct = S_oct.reshape(-1, P, P)
    for p, (i, j) in enumerate(pairs):
        assert np.array_equal(lam[:, p], S_oct[:, i, j]), "lam is not the input's real part bit for bit (pair %d %d)" % (i, j)
    _check_factor(F, status, S_oct, S_full, tag="%s P = %d %s" % ("x".join(map(str, ext)), P, family))


# ---- 3. geobo_sample_zpass -------------------------------------------------------------------------------------------------------
def _zpass_lines_per_workgroup(P, mz):
    C = 1
    while 2 * C * P * mz <= 4096:
        C *= 2
    return C


ZPASS_TORI = {4: (16, 8), 64: (4, 2), 512: (2, 2)}                # mz -> (my, mx): 3 pairs give 384, 24 and 12 lines


def _zpass_reference(F, xi, ext, P, nz):
    """scale F(w) xi(w) in long double -> inverse DFT along z -> first nz; also the fp64 competitor (einsum + np.fft)."""
    my, mx, mz = ext
    M = my * mx * mz
    scale = 1.0 / math.sqrt(M)
    Ff = R.octant_expand(F.reshape(my // 2 + 1, mx // 2 + 1, mz // 2 + 1, P, P), ext)
    x5 = xi.reshape(-1, my, mx, mz, P)
    y = np.zeros((x5.shape[0], P, my, mx, mz), dtype=np.clongdouble)
    for i in range(P):
        for q in range(P):
            y[:, i] += Ff[None, ..., i, q].astype(LD) * x5[..., q].astype(np.clongdouble)
    y *= LD(1) / np.sqrt(LD(M))
    full = R.dft_long(y, 4, inverse=True)
    y64 = scale * np.einsum("yxziq,kyxzq->kiyxz", Ff, x5)
    npf = (np.fft.ifft(y64, axis=4) * mz)[..., :nz]
    return full, npf


@pytest.mark.parametrize("nz_of", ["1", "half", "full"])
@pytest.mark.parametrize("mz", [4, 64, 512])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_sample_zpass_with_callers_noise(P, mz, nz_of):
    from geobo_amd import hip
    my, mx = ZPASS_TORI[mz]
    ext, npairs = (my, mx, mz), 3
    nz = {"1": 1, "half": mz // 2, "full": mz}[nz_of]
    M, lines, C = my * mx * mz, npairs * my * mx, _zpass_lines_per_workgroup(P, mz)
    assert lines % C != 0 or C <= 4               # (lines are multiples of 4: only tiles of 8 and more can be partial)
    rng = np.random.default_rng(77 + 100 * P + mz + nz)
    no = (my // 2 + 1) * (mx // 2 + 1) * (mz // 2 + 1)
    F = rng.standard_normal((no, P, P))
    xi = rng.standard_normal((npairs, M, P)) + 1j * rng.standard_normal((npairs, M, P))
    n = 2 * npairs * P * my * mx * nz
    buf, out = _guarded(n)
    hip.sample_zpass(P, 0, npairs, my, mx, mz, nz, _dev(F.reshape(-1)), out, noise=_dev(_interleave(xi)))
    torch.cuda.synchronize()
    assert _untouched(buf, n)
    got = _complex(out.cpu().numpy(), (npairs, P, my, mx, nz))
    full, npf = _zpass_reference(F, xi, ext, P, nz)
    e_k, e_np = _line_errors(got, npf, full, nz, 4)
    ratio = e_k / np.maximum(e_np, EPS)
    print("sample_zpass P = %d mz = %d nz = %d (%d lines, %d per workgroup): worst ratio %.2f" % (P, mz, nz, lines, C, ratio.max()))
    assert np.all(ratio <= MARGIN), float(ratio.max())


@pytest.mark.parametrize("P", [1, 2, 3])
def test_sample_zpass_philox_addressing(P):
    """noise = NULL draws xi_q(w) of pair k from the Philox blocks (element w, sample pair0 + k, RNG_PRIOR, sub 0 and 1): normals
    (n[2q], n[2q+1]) of the eight of the two blocks -- the contract that makes sample k depend on (seed, k) only."""
    from geobo_amd import hip
    my, mx, mz, nz = 4, 2, 64, 20
    M, npairs, pair0, seed = my * mx * mz, 3, 5, 2 ** 40 + 7
    rng = np.random.default_rng(5 + P)
    no = (my // 2 + 1) * (mx // 2 + 1) * (mz // 2 + 1)
    F = _dev(rng.standard_normal(no * P * P))
    n = 2 * npairs * P * my * mx * nz
    a = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hip.sample_zpass(P, pair0, npairs, my, mx, mz, nz, F, a, seed=seed)
    blocks = [hip.philox_fill(seed, hip.RNG_PRIOR, pair0, npairs, 0, M, sub=sub) for sub in (0, 1)]
    normals = torch.cat(blocks, dim=-1)                                        # (npairs, M, 8)
    noise = normals[..., :2 * P].contiguous().reshape(-1)                      # [(k M + w) P + q] complex = (n[2q], n[2q+1])
    b = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hip.sample_zpass(P, 0, npairs, my, mx, mz, nz, F, b, noise=noise)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    d = float(np.abs(a - b).max() / np.abs(b).max())
    print("sample_zpass Philox P = %d: max difference %.2e of max|out|, bit for bit: %s" % (P, d, np.array_equal(a, b)))
    assert d <= 1e-14
    # a different pair0 or seed gives other noise (the comparison above is not vacuous)
    c = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hip.sample_zpass(P, pair0 + 1, npairs, my, mx, mz, nz, F, c, seed=seed)
    c = c.cpu().numpy()
    per = n // npairs
    assert np.array_equal(c[:2 * per], a[per:]) and not np.array_equal(c[:per], a[:per])


# ---- 4. geobo_spectral_mix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npairs", [1, 3])
@pytest.mark.parametrize("P", [1, 2, 3])
def test_spectral_mix_by_value(P, npairs):
    from geobo_amd import hip
    ext = my, mx, mz = 8, 4, 16
    M, NP = my * mx * mz, P * (P + 1) // 2
    rng = np.random.default_rng(31 + 10 * P + npairs)
    hy, hx, hz = my // 2 + 1, mx // 2 + 1, mz // 2 + 1
    # all entries of one frequency distinct and of different size per pair: a transposed or mis-indexed pair shows
    lam = rng.standard_normal((hy * hx * hz, NP)) + 3.0 * np.arange(1, NP + 1)
    x = rng.standard_normal((npairs, P, M)) + 1j * rng.standard_normal((npairs, P, M))
    scale = 0.37
    n = 2 * npairs * P * M
    buf, out = _guarded(n)
    hip.spectral_mix(P, npairs, my, mx, mz, _dev(lam.reshape(-1)), scale, _dev(_interleave(x)), out)
    torch.cuda.synchronize()
    assert _untouched(buf, n)
    got = _complex(out.cpu().numpy(), (npairs, P, M))
    pairs = [(i, j) for i in range(P) for j in range(i, P)]
    L = np.zeros((hy, hx, hz, P, P))
    for p, (i, j) in enumerate(pairs):
        L[..., i, j] = L[..., j, i] = lam[:, p].reshape(hy, hx, hz)
    Lf = R.octant_expand(L, ext).reshape(M, P, P).astype(LD)
    xl = x.astype(np.clongdouble)
    want = np.zeros((npairs, P, M), dtype=np.clongdouble)
    bound_re, bound_im = np.zeros((npairs, P, M)), np.zeros((npairs, P, M))
    for i in range(P):
        for j in range(P):
            want[:, i] += Lf[None, :, i, j] * xl[:, j]
            bound_re[:, i] += np.abs(Lf[None, :, i, j].astype(float) * x[:, j].real)
            bound_im[:, i] += np.abs(Lf[None, :, i, j].astype(float) * x[:, j].imag)
    want *= LD(scale)
    r = max(float((np.abs(got.real - want.real) / (4 * EPS * scale * bound_re)).max()),
            float((np.abs(got.imag - want.imag) / (4 * EPS * scale * bound_im)).max()))
    print("spectral_mix P = %d npairs = %d: worst error / (4 eps sum |lambda||in|) = %.3f" % (P, npairs, r))
    assert r <= 1.0


# ---- 5. and 7. the assembled sampler and its factors at the lengths the product uses ---------------------------------------------
# (nx, ny, nz) as settings_for takes them, and the torus (my, mx, mz) of the first candidate of the padding rule
PRODUCT_GRIDS = [((24, 40, 70), (128, 64, 256)), ((6, 4, 130), (8, 16, 512))]
LENGTHS3 = [200.0, 210.0, 220.0]


def _wrapped_tables(s, ext, kern, lengths, w, amp):
    """The oracle's covariance blocks at the wrapped lags of the torus: T[i][j] (my, mx, mz)."""
    ax = [R.fold_index(m) * v for m, v in zip(ext, (s.yvoxsize, s.xvoxsize, s.zvoxsize))]
    dy, dx, dz = np.meshgrid(*ax, indexing="ij")
    d2 = dy ** 2 + dx ** 2 + dz ** 2
    Wo = O.weight_matrix(w)
    return [[amp * O.k_block(kern, d2, np.asarray(lengths), Wo, i, j) for j in range(3)] for i in range(3)]


@pytest.mark.parametrize("kern", ["exp", "matern32", "sparse"])
@pytest.mark.parametrize("dims,ext", PRODUCT_GRIDS, ids=["128x64x256", "8x16x512"])
def test_tables_spectra_and_factor_at_product_lengths(dims, ext, kern):
    """test_torus_tables_and_spectra on tori with axes of 128, 256 and 512 points, and on the same sampler F F^T = psd_part(S(w)) with
    S(w) from np.fft.fftn of the oracle's wrapped-lag tables (not from smp.spectra): ties F, not only lam, to the oracle covariance.
    approximate = True with cap_bytes = 0: the padding rule stops at its first candidate whatever the PSD verdict."""
    from geobo_amd import hip
    from geobo_amd.engine import PosteriorEngine, weight_matrix
    nx, ny, nz = dims
    s = settings_for(nx, ny, nz, kernelfunc=kern)
    amp = 1.3
    smp = _sampler(s, LENGTHS3, PSD_W, amp, approximate=True, cap_bytes=0)
    assert smp.ext == ext
    my, mx, mz = ext
    M, N = my * mx * mz, nx * ny * nz
    eng = PosteriorEngine(s)
    xyz = tuple(c[:N].contiguous() for c in eng.grid_points())
    W = weight_matrix(PSD_W)
    T = _wrapped_tables(s, ext, kern, LENGTHS3, PSD_W, amp)
    spec = smp.spectra.view(len(smp.pairs), M, 2).cpu().numpy()
    tab = smp.table.view(len(smp.pairs), my, mx, mz, 2).cpu().numpy()
    S_full = np.empty((my, mx, mz, 3, 3))
    worst = 0.0
    for p, (i, j) in enumerate(smp.pairs):
        row = torch.empty((1, N), dtype=torch.float64, device="cuda")
        hip.k_block(hip.kernel_id(kern, i != j), tuple(c[:1] for c in xyz), xyz, LENGTHS3[j], LENGTHS3[i], W[i][j], amp, row)
        assert np.array_equal(tab[p, :ny, :nx, :nz, 0].reshape(-1), row.cpu().numpy()[0]), (i, j)
        assert not tab[p, ..., 1].any()
        ref = np.fft.fftn(T[i][j])
        e = np.abs(spec[p, :, 0] + 1j * spec[p, :, 1] - ref.reshape(-1)).max() / np.abs(ref).max()
        worst = max(worst, float(e))
        assert e <= 1e-12, (i, j)                                  # the existing bound on the spectra
        S_full[..., i, j] = S_full[..., j, i] = ref.real
    print("spectra %s %s: worst error %.2e of max|S|" % ("x".join(map(str, ext)), kern, worst))
    # ---- the factor and the status word on these spectra ----
    hy, hx, hz = my // 2 + 1, mx // 2 + 1, mz // 2 + 1
    S_oct = S_full[:hy, :hx, :hz].reshape(-1, 3, 3)
    F = smp.F.cpu().numpy().reshape(-1, 3, 3)
    smax = float(np.abs(S_full).max())
    # per frequency: the bound of test_sample_factor_by_value plus the spectra's 1e-12 max|S|; the traces: plus 1e-12 of sum |e|
    sum_abs = float(np.abs(np.linalg.eigvalsh(S_full.reshape(-1, 3, 3))).sum())
    _check_factor(F, smp.status, S_oct, S_full, extra=1e-12 * smax, extra_sum=1e-12 * sum_abs,
                  tag="%s %s" % ("x".join(map(str, ext)), kern))


@pytest.mark.parametrize("dims,ext", PRODUCT_GRIDS, ids=["128x64x256", "8x16x512"])
def test_sampler_equals_numpy_ifft_of_the_same_noise_at_product_lengths(dims, ext):
    """test_sampler_equals_numpy_ifft_of_the_same_noise with z, x and y transforms of 64 to 512 points (np.fft as the reference and the
    existing 1e-12 of the scale, as there)."""
    nx, ny, nz = dims
    s = settings_for(nx, ny, nz, kernelfunc="matern32")
    smp = _sampler(s, LENGTHS3, PSD_W, approximate=True, cap_bytes=0)
    assert smp.ext == ext
    my, mx, mz = ext
    M, P, N = my * mx * mz, 3, nx * ny * nz
    rng = np.random.default_rng(11)
    npairs = 2
    xi = rng.standard_normal((npairs, M, P)) + 1j * rng.standard_normal((npairs, M, P))
    got = smp.sample(0, 2 * npairs - 1, noise=_dev(_interleave(xi))).cpu().numpy()   # odd count: the last imaginary part is dropped
    Ff = R.octant_expand(smp.F.view(my // 2 + 1, mx // 2 + 1, mz // 2 + 1, P, P).cpu().numpy(), ext)
    worst = 0.0
    for k in range(npairs):
        y = np.einsum("yxziq,yxzq->iyxz", Ff, xi[k].reshape(my, mx, mz, P)) / np.sqrt(M)
        f = np.fft.ifftn(y, axes=(1, 2, 3)) * M
        f = f[:, :ny, :nx, :nz].reshape(P, N)
        scale = np.abs(f).max()
        worst = max(worst, float(np.abs(got[2 * k] - f.real).max() / scale))
        assert np.abs(got[2 * k] - f.real).max() <= 1e-12 * scale
        if 2 * k + 1 < got.shape[0]:
            worst = max(worst, float(np.abs(got[2 * k + 1] - f.imag).max() / scale))
            assert np.abs(got[2 * k + 1] - f.imag).max() <= 1e-12 * scale
    print("sampler vs np.fft on %s: worst error %.2e of the scale" % ("x".join(map(str, ext)), worst))


# ---- 6. apply_K against a dense covariance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", ["exp", "matern32", "sparse"])
@pytest.mark.parametrize("dims,ext", [((3, 5, 40), (16, 8, 128)), ((2, 3, 130), (8, 4, 512))], ids=["16x8x128", "8x4x512"])
def test_apply_K_against_dense_covariance(dims, ext, kern):
    """PriorSampler.apply_K (what condition() and the information gain use) against the oracle's dense K v, with the default weights
    (1.0, 0.2, 0.2): an indefinite prior, on which apply_K stays exact because it multiplies by the unclipped spectra.  The yardstick
    is NumPy's own circulant product crop(ifftn(S fftn(pad v))) against the same dense K v."""
    nx, ny, nz = dims
    w = (1.0, 0.2, 0.2)
    s = settings_for(nx, ny, nz, kernelfunc=kern)
    smp = _sampler(s, LENGTHS3, w, approximate=True, cap_bytes=0)
    assert smp.ext == ext
    my, mx, mz = ext
    N = nx * ny * nz
    K = _oracle_K(s, LENGTHS3, w)
    assert K.shape == (3 * N, 3 * N)
    T = _wrapped_tables(s, ext, kern, LENGTHS3, w, 1.0)
    Sp = [[np.fft.fftn(T[i][j]) for j in range(3)] for i in range(3)]
    rng = np.random.default_rng(3 + nz)
    for S in (1, 2, 5):                                           # odd counts: the last pair is half empty
        V = rng.standard_normal((S, 3, N))
        buf, out = _guarded(S * 3 * N)
        got = smp.apply_K(_dev(V), out=out.view(S, 3, N))
        torch.cuda.synchronize()
        assert _untouched(buf, S * 3 * N)
        got = got.cpu().numpy().reshape(S, 3 * N)
        want = V.reshape(S, 3 * N) @ K.T
        pad = np.zeros((S, 3, my, mx, mz))
        pad[:, :, :ny, :nx, :nz] = V.reshape(S, 3, ny, nx, nz)
        vh = np.fft.fftn(pad, axes=(2, 3, 4))
        mixed = np.stack([sum(Sp[i][j] * vh[:, j] for j in range(3)) for i in range(3)], 1)
        circ = np.fft.ifftn(mixed, axes=(2, 3, 4)).real[:, :, :ny, :nx, :nz].reshape(S, 3 * N)
        scale = np.abs(want).max(axis=1)
        e_dev = np.abs(got - want).max(axis=1) / scale
        e_np = np.abs(circ - want).max(axis=1) / scale
        print("apply_K %s %s S = %d: device %.2e, NumPy's circulant product %.2e (normwise, worst row), ratio %.2f"
              % ("x".join(map(str, ext)), kern, S, e_dev.max(), e_np.max(), (e_dev / np.maximum(e_np, EPS)).max()))
        assert np.all(e_dev <= MARGIN * np.maximum(e_np, EPS)), (S, e_dev, e_np)
