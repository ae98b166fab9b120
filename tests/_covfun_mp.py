"""Multiprecision reference of the covariance families, their length derivatives, exp_decay and the two potentials.

CPU only (mpmath at 50 digits, no torch).  Every function is written AS CODED in the kernel library (kernels.py of the
reference, make_cov / cov_eval of csrc/covfun.h, sensormodel.py:107-109 and :130-133), quirks included: the `cos` inside the `sin`
of sparse-cross branch A, `l2 += 1e-3 l2` at equal lengths, branch B winning at equality, the `res < 0 -> 0` clamps, pi and
sqrt(3) as the fp64 constants the code multiplies with, branches taken on the fp64 `sqrt(d2)` the code compares, and the scale
`w * amp` applied last.  Inputs enter with their exact fp64 value, `mpf(float(x))`.

Each reference returns (ref, env).  `env` is the conditioned error envelope: the first-order bound, in units of u = 2^-53, on
what a faithful fp64 evaluation of the same formula can lose,

    env = sum over the formula's terms of  |C| (|f(a)| + |a| |f'(a)|)        for a term C f(a), f in {exp, sin, cos}

which for f = exp is |term| (1 + |a|) -- rounding the argument a costs |a| u, and a difference loses relative to its terms, not
to its result.  For the trigonometric terms the derivative form is needed: |term| (1 + |a|) would vanish at a zero of sin while
the error of its rounded argument does not.  A denominator l1^2 - l2^2 that two cancelling terms share adds its own relative
error (l1^2 + l2^2) / |l1^2 - l2^2| times their sum.  For a derivative that is taken numerically (sparse ids 13-15) the same
rule on d/dl [C f(a)] = C' f + C f' a' gives (1 + |a|) (|C'| + |C a'|) with |f|, |f'| <= 1.

The unit of every comparison is  ulps(got, ref, env) = |got - ref| / (2^-53 env).

K_ORACLE holds, per function, the largest ulps(...) of the project's float64 NumPy oracle (ids 1-6, grav, magn) or of the
same mpmath formula evaluated at 53 bits (ids 7-15: the oracle has no derivatives) over the point sets below and every
length pair; tests/test_covfun_cpu.py re-measures it and the GPU tests allow 4 K + 4.  The derivative rows are the measurements
rounded up to the next half (mpmath is deterministic).  The oracle rows are rounded up to the next integer: NumPy's exp / sin /
log differ in the last bit between its SIMD code paths, which moved these figures by up to 0.25 (exp_x 2.28 .. 2.52,
matern32 2.21 .. 2.45) when the AVX-512 and AVX2 paths were switched off.
"""
import functools
import math

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

U = mpf(2) ** -53

# measured by tests/test_covfun_cpu.py (run it with -s); the measurement behind each entry is in the comment
K_ORACLE = {
    1: 2.0,      # exp              1.176
    2: 3.0,      # exp_x            2.515
    3: 3.0,      # matern32         2.452
    4: 2.0,      # matern32_x       1.485
    5: 3.0,      # sparse           2.242
    6: 2.0,      # sparse_x         1.238
    7: 2.5,      # exp_dl           2.490
    8: 2.5,      # exp_x_dl1        2.075
    9: 1.5,      # exp_x_dl2        1.306
    10: 5.0,     # matern32_dl      4.961
    11: 2.0,     # matern32_x_dl1   1.528
    12: 1.0,     # matern32_x_dl2   0.952
    13: 0.5,     # sparse_dl        0.391
    14: 0.5,     # sparse_x_dl1     0.296
    15: 0.5,     # sparse_x_dl2     0.448
    "grav": 2.0,  # grav_potential  1.548
    "magn": 2.0,  # magn_potential  1.232
}

NAMES = {1: "exp", 2: "exp_x", 3: "matern32", 4: "matern32_x", 5: "sparse", 6: "sparse_x", 7: "exp_dl", 8: "exp_x_dl1",
         9: "exp_x_dl2", 10: "matern32_dl", 11: "matern32_x_dl1", 12: "matern32_x_dl2", 13: "sparse_dl", 14: "sparse_x_dl1",
         15: "sparse_x_dl2"}
BASE = {7: 1, 8: 2, 9: 2, 10: 3, 11: 4, 12: 4, 13: 5, 14: 6, 15: 6}
ORACLE_FAMILY = {1: ("exp", False), 2: ("exp", True), 3: ("matern32", False), 4: ("matern32", True), 5: ("sparse", False),
                 6: ("sparse", True)}
SPARSE_DERIVS = (13, 14, 15)

# (230, 234.6) is the pair the workflow runs: create_cov turns [l, l, l] into [l, 1.02 l, l] in place
LENGTH_PAIRS = ((230.0, 230.0), (230.0, 1.02 * 230.0), (230.0, 255.0), (200.0, 600.0), (230.0, 230.0 * (1 + 1e-6)), (255.0, 230.0))
W, AMP = 0.7, 1.3
SCALE = W * AMP                  # make_cov: p.scale = w * amp, one fp64 product, applied last
TINY_ENV = 1e-290                # below this envelope a result is only required to be finite and at most TINY_MAX in size
TINY_MAX = 1e-289
DROP_RADIUS = 1e-9               # sparse derivatives: points this close (times lmax) to a branch point or clamp crossing are dropped
DROP_CAP = 0.03

PI = mpf(math.pi)                # the code's pi is the fp64 constant
SQRT3 = mpf(math.sqrt(3.0))      # make_cov: c[1] = sqrt(3.0)
B_FIELD = (0.2e-3, -0.1e-3, 1e-3)


def tol(key):
    """The GPU tests' bound in envelope units: the kernel replaces divisions by precomputed reciprocals and uses its own
    exponential, each at most one more rounding per term (factor 4); + 4 is the floor where the oracle's own error is near 0."""
    return 4.0 * K_ORACLE[key] + 4.0


def ulps(got, ref, env):
    got = float(got)
    if mp.isnan(ref):
        return 0.0 if math.isnan(got) else math.inf
    if not math.isfinite(got):
        return math.inf
    if env == 0:
        return 0.0 if got == ref else math.inf
    return float(abs(mpf(got) - ref) / (U * env))


# ---- points --------------------------------------------------------------------------------------------------------------------
def effective_l2(l1, l2):
    """kernels.py:125-126 / make_cov: the sparse cross family moves l2 off l1 (fp64 arithmetic)."""
    return l2 + 1e-3 * l2 if l1 == l2 else l2


def branch_points(l1, l2):
    pts = [abs(l2 - l1) / 2.0, (l1 + l2) / 2.0, l1, l2]
    if l1 == l2:
        e = effective_l2(l1, l2)
        pts += [abs(e - l1) / 2.0, (l1 + e) / 2.0, e]
    return pts


@functools.lru_cache(maxsize=None)
def distances(l1, l2):
    """The distances of a length pair (at most 512): 0, a geometric ladder over 7.6 decades up to 40 lmax (far tail), a linear
    ladder over the support of the sparse families, and every branch point with its two fp64 neighbours."""
    lmax = max(l1, l2)
    bp = np.array(branch_points(l1, l2))
    d = np.concatenate([[0.0], np.geomspace(1e-6 * lmax, 40 * lmax, 250), np.linspace(0, 1.2 * lmax, 200), bp,
                        np.nextafter(bp, np.inf), np.nextafter(bp, -np.inf)])
    d = np.unique(d[d >= 0])
    assert d.size <= 512
    d.setflags(write=False)
    return d


def sq(d):
    return d * d


# ---- term lists: a value is sum C f(a) --------------------------------------------------------------------------------------------
# kind None: C; 'sin' / 'cos': C sin(a), C cos(a); 'sincos': C sin(c5 cos(b)) with a = (c5, b)
def _term_value(C, kind, a):
    if kind is None:
        return C
    if kind == "sin":
        return C * mp.sin(a)
    if kind == "cos":
        return C * mp.cos(a)
    c5, b = a
    return C * mp.sin(c5 * mp.cos(b))


def _term_env(C, kind, a):
    if kind is None:
        return abs(C)
    if kind == "sin":
        return abs(C) * (abs(mp.sin(a)) + abs(a * mp.cos(a)))
    if kind == "cos":
        return abs(C) * (abs(mp.cos(a)) + abs(a * mp.sin(a)))
    c5, b = a
    t = c5 * mp.cos(b)
    return abs(C) * (abs(mp.sin(t)) + abs(mp.cos(t)) * (abs(t) + abs(c5 * b * mp.sin(b))))


def _term_env_d(t0, tp, tm, h):
    """(1 + |a|) (|C'| + |C a'|) with C', a' from a central difference at +-h (relative error h^2 ~ 1e-40: an envelope)."""
    (C, kind, a), (Cp, _, ap), (Cm, _, am) = t0, tp, tm
    dC = abs(Cp - Cm) / (2 * h)
    if kind is None:
        return dC
    if kind in ("sin", "cos"):
        return (1 + abs(a)) * (dC + abs(C * (ap - am) / (2 * h)))
    (c5, b), (c5p, bp), (c5m, bm) = a, ap, am
    return (1 + abs(c5 * mp.cos(b)) + abs(c5 * b)) * (dC + abs(C) * (abs(c5p - c5m) + abs(c5 * (bp - bm))) / (2 * h))


def _sparse_terms(l, d):
    """kernels.py:109-113 inside the support: (2 + cos t) / 3 (1 - d / l) + sin(t) / (2 pi), t = 2 pi d / l, multiplied out."""
    t = 2 * PI * d / l
    return [(mpf(2) / 3, None, 0), (-2 * d / (3 * l), None, 0), (mpf(1) / 3, "cos", t), (-d / (3 * l), "cos", t),
            (1 / (2 * PI), "sin", t)]


def _sparse_x_terms(l1, l2, d, branch):
    """kernels.py:121-137: branch 'B' (|l2 - l1| / 2 <= d <= (l1 + l2) / 2) or 'A' (d below that), constants as in make_cov."""
    pre = 2 / (3 * mp.sqrt(l1 * l2))
    if branch == "B":
        den = 2 * PI * (l1 * l1 - l2 * l2)
        return [(pre * (l1 + l2) / 2, None, 0), (-pre * d, None, 0), (pre * l1 ** 3 / den, "sin", PI * (l2 - 2 * d) / l1),
                (-pre * l2 ** 3 / den, "sin", PI * (l1 - 2 * d) / l2)]
    lmin, lmax = (l1, l2) if l1 < l2 else (l2, l1)
    c4 = 1 / PI * lmax ** 3 / (lmax * lmax - lmin * lmin)
    return [(pre * lmin, None, 0), (pre * c4, "sincos", (PI * lmin / lmax, 2 * PI * d / lmax))]


def _shared_denominator(terms, l1, l2):
    """Relative error of l1^2 - l2^2 times the sum of the terms that carry it (the trigonometric ones)."""
    s = sum(_term_value(*t) for t in terms if t[1] is not None)
    return abs(s) * (l1 * l1 + l2 * l2) / abs(l1 * l1 - l2 * l2)


def sparse_branch(l, d2):
    return "in" if math.sqrt(d2) < l else None


def sparse_x_branch(l1, l2, d2):
    """The branch the code takes: fp64 sqrt and fp64 limits (make_cov c[0], c[1]); B is tested first and wins at equality."""
    d = math.sqrt(d2)
    ca, cb = abs(l2 - l1) / 2.0, (l1 + l2) / 2.0
    if ca <= d <= cb:
        return "B"
    return "A" if d <= ca else None


def _sparse_any(kid, d2, l1, l2, which):
    """Value (which None) or d / d l_which of a sparse family at fp64 inputs: (ref, env, unclamped value)."""
    cross = BASE.get(kid, kid) == 6
    l2_in = l2
    if cross:
        l2 = effective_l2(l1, l2_in)
        branch = sparse_x_branch(l1, l2, d2)
    else:
        branch = sparse_branch(l1, d2)
    zero = mpf(0)
    if branch is None:
        return zero, zero, zero
    d = mp.sqrt(mpf(d2))
    L1, L2 = mpf(l1), mpf(l2)
    if cross:
        terms = lambda a, b: _sparse_x_terms(a, b, d, branch)
    else:
        terms = lambda a, b: _sparse_terms(a, d)
    value = lambda a, b: sum(_term_value(*t) for t in terms(a, b))
    t0 = terms(L1, L2)
    v0 = sum(_term_value(*t) for t in t0)
    if which is None:
        env = sum(_term_env(*t) for t in t0) + (_shared_denominator(t0, L1, L2) if cross else 0)
        return (v0 if v0 > 0 else zero), env, v0
    # the derivative follows the taken branch and the clamp; at equal lengths d l2_eff / d l2 = 1 + 1e-3 (make_cov c[0])
    chain = 1 + mpf(1e-3) if (which == 2 and l2 != l2_in) else 1
    h = (L1 if which == 1 else L2) * mpf(10) ** -20
    if which == 1:
        ref = mp.diff(lambda a: value(a, L2), L1)
        tp, tm = terms(L1 + h, L2), terms(L1 - h, L2)
    else:
        ref = mp.diff(lambda b: value(L1, b), L2)
        tp, tm = terms(L1, L2 + h), terms(L1, L2 - h)
    env = sum(_term_env_d(a, b, c, h) for a, b, c in zip(t0, tp, tm))
    return (chain * ref if v0 > 0 else zero), chain * env, v0


# ---- the sixteen functions (id 0 is d2 itself) -----------------------------------------------------------------------------------
def evaluate(kid, d2, l1, l2):
    """(ref, env) of family `kid` at the fp64 squared distance d2 and fp64 lengths, WITHOUT the scale; at the working precision
    of the mp context (50 digits for the reference; 53 bits when the CPU module calibrates the derivative ids)."""
    d2, l1, l2 = float(d2), float(l1), float(l2)
    if BASE.get(kid, kid) in (5, 6):
        which = {5: None, 6: None, 13: 1, 14: 1, 15: 2}[kid]
        return _sparse_any(kid, d2, l1, l2, which)[:2]
    D2, L1, L2 = mpf(d2), mpf(l1), mpf(l2)
    if kid == 0:                                        # the squared distance itself
        return D2, abs(D2)
    if kid in (1, 7):                                   # exp(-d2 / (2 l^2));  d/dl = k d2 / l^3
        a = D2 / (2 * L1 * L1)
        k = mp.exp(-a)
        v = k if kid == 1 else k * D2 / L1 ** 3
        return v, v * (1 + a)
    if kid in (2, 8, 9):                                # sqrt(2 l1 l2 / S) exp(-d2 / S), S = l1^2 + l2^2
        S = L1 * L1 + L2 * L2
        a = D2 / S
        k = mp.sqrt(2 * L1 * L2 / S) * mp.exp(-a)
        if kid == 2:
            return k, k * (1 + a)
        la = L1 if kid == 8 else L2                     # dk/dla = k (1/(2 la) - la/S + 2 la d2 / S^2)
        t = (1 / (2 * la), -la / S, 2 * la * D2 / (S * S))
        return k * sum(t), k * (1 + a) * sum(abs(x) for x in t)
    if kid in (3, 10):                                  # (1 + nu) exp(-nu), nu = sqrt(3) sqrt(d2) / l;  d/dl = nu^2 exp(-nu) / l
        nu = SQRT3 * mp.sqrt(D2) / L1
        v = (1 + nu) * mp.exp(-nu) if kid == 3 else nu * nu * mp.exp(-nu) / L1
        return v, v * (1 + nu)
    if kid in (4, 11, 12):                              # c (l1 e1 - l2 e2), c = 2 sqrt(l1 l2) / (l1^2 - l2^2), ei = exp(-r / li)
        if l1 == l2:
            return mp.nan, mp.nan                       # inf * 0, as coded
        r = mp.sqrt(3 * D2)
        q = 1 / (L1 * L1 - L2 * L2)
        c = 2 * mp.sqrt(L1 * L2) * q
        e1, e2 = mp.exp(-r / L1), mp.exp(-r / L2)
        diff = L1 * e1 - L2 * e2
        diff_env = L1 * e1 * (1 + r / L1) + L2 * e2 * (1 + r / L2)
        if kid == 4:
            return c * diff, abs(c) * diff_env
        if kid == 11:
            f = 1 / (2 * L1) - 2 * L1 * q
            fe = 1 / (2 * L1) + abs(2 * L1 * q)
            return c * (f * diff + e1 * (1 + r / L1)), abs(c) * (fe * diff_env + e1 * (1 + r / L1) ** 2)
        f = 1 / (2 * L2) + 2 * L2 * q
        fe = 1 / (2 * L2) + abs(2 * L2 * q)
        return c * (f * diff - e2 * (1 + r / L2)), abs(c) * (fe * diff_env + e2 * (1 + r / L2) ** 2)
    raise ValueError(kid)


def value_mp(kid, d2, l1, l2):
    """The value family `kid` (1-4) as a function of mpf lengths -- what mp.diff differentiates to prove the analytic ids 7-12."""
    D2 = mpf(float(d2))
    if kid == 1:
        return mp.exp(-D2 / (2 * l1 * l1))
    if kid == 2:
        S = l1 * l1 + l2 * l2
        return mp.sqrt(2 * l1 * l2 / S) * mp.exp(-D2 / S)
    if kid == 3:
        nu = SQRT3 * mp.sqrt(D2) / l1
        return (1 + nu) * mp.exp(-nu)
    r = mp.sqrt(3 * D2)
    return 2 * mp.sqrt(l1 * l2) / (l1 * l1 - l2 * l2) * (l1 * mp.exp(-r / l1) - l2 * mp.exp(-r / l2))


@functools.lru_cache(maxsize=None)
def table(kid, l1, l2):
    """Reference table of family `kid` over distances(l1, l2), scale w * amp applied last: (d2, ref, env, keep).
    keep[i] is False where a sparse derivative does not exist (see dropped())."""
    d2 = sq(distances(l1, l2))
    s = mpf(SCALE)
    ref, env = [], []
    for x in d2:
        r, e = evaluate(kid, x, l1, l2)
        ref.append(s * r)
        env.append(s * e)
    keep = ~dropped(kid, l1, l2) if kid in SPARSE_DERIVS else np.ones(d2.size, dtype=bool)
    return d2, ref, env, keep


@functools.lru_cache(maxsize=None)
def dropped(kid, l1, l2):
    """Points of distances(l1, l2) where the derivative of a sparse family does not exist as evaluated: within DROP_RADIUS lmax of
    a branch point, or of a zero crossing of the clamp -- the unclamped value changes sign inside that radius, or is so small
    that its fp64 sign is not determined (|value| below the value family's own tolerance)."""
    base = BASE[kid]
    d = distances(l1, l2)
    lmax = max(l1, l2)
    rad = DROP_RADIUS * lmax
    e2 = effective_l2(l1, l2) if base == 6 else l2
    bps = [l1] if base == 5 else [abs(e2 - l1) / 2.0, (l1 + e2) / 2.0]
    out = np.zeros(d.size, dtype=bool)
    for i, x in enumerate(d):
        if any(abs(x - b) <= rad for b in bps):
            out[i] = True
            continue
        _, env, v = _sparse_any(base, x * x, l1, l2, None)
        if env == 0:
            continue
        if abs(v) <= tol(base) * U * env:
            out[i] = True
            continue
        for y in (x - rad, x + rad):
            if y >= 0:
                _, _, vy = _sparse_any(base, y * y, l1, l2, None)
                if vy != 0 and (vy > 0) != (v > 0):
                    out[i] = True
    return out


def max_ulps(got, kid, l1, l2):
    """Largest ulps(...) of `got` over the kept points of table(kid, l1, l2) whose envelope is at least TINY_ENV, and the
    index where it occurs; the points below TINY_ENV are returned as a mask for the caller's finiteness assertions."""
    d2, ref, env, keep = table(kid, l1, l2)
    got = np.asarray(got, dtype=np.float64)
    tiny = np.array([not mp.isnan(e) and e < TINY_ENV for e in env])
    worst, where = 0.0, -1
    for i in np.flatnonzero(keep & ~tiny):
        u = ulps(got[i], ref[i], env[i])
        if u > worst:
            worst, where = u, int(i)
    return worst, where, tiny


# ---- exp_decay ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exp_arguments():
    """Arguments of exp_decay, sorted from 0 downwards: the reduction's multiples and half-way points of ln 2 with their fp64
    neighbours, the whole range, the denormal results and the clamp."""
    xs = [0.0, -2.0 ** -60]
    for n in (1, 2, 3, 10, 100, 511, 1000, 1022, 1023, 1074):
        for m in (mpf(n), mpf(n) + mpf(1) / 2):
            x = float(-m * mp.ln2)
            xs += [x, math.nextafter(x, 0.0), math.nextafter(x, -math.inf)]
    xs += list(-np.geomspace(1e-3, 745.2, 200))
    xs += list(-np.linspace(708.0, 745.2, 64))
    xs += [-800.0, -800.0000001, -1e4, -1e300]
    xs = np.array(sorted(set(xs), reverse=True))
    xs.setflags(write=False)
    return xs


def exp_error(x, got):
    """(error, unit): the error of `got` as exp(x) in ulps of the result ('ulp', normal results) or in units of 2^-1074
    ('denormal')."""
    ref = mp.exp(mpf(float(x)))
    got = mpf(float(got))
    if ref < mpf(2) ** -1022:
        return float(abs(got - ref) * mpf(2) ** 1074), "denormal"
    e = int(mp.floor(mp.log(ref, 2)))
    return float(abs(got - ref) / mpf(2) ** (e - 52)), "ulp"


# ---- potentials -----------------------------------------------------------------------------------------------------------------
def _log_env(s, r):
    """|log(s + r)| plus the amplified relative error of its argument: r carries its own rounding, the sum another."""
    return abs(mp.log(s + r)) + (abs(s) + 2 * r) / abs(s + r)


def _atan_env(num, den, den_abs):
    """|atan(q)| plus |q| / (1 + q^2) times the relative error of the quotient q = num / den: one rounding each for the two
    products and the division, and the denominator's own, amplified by den_abs / |den| like the arguments of the logs."""
    q = num / den
    return abs(mp.atan(q)) + abs(q) / (1 + q * q) * (3 + den_abs / abs(den))


def grav_mp(x, y, z):
    """sensormodel.py:107-109: x log(y + r) + y log(x + r) - z atan(x y / (z r + 1e-9)), with the 1e-9 of the code."""
    x, y, z = mpf(float(x)), mpf(float(y)), mpf(float(z))
    r = mp.sqrt(x * x + y * y + z * z)
    eps = mpf(1e-9)
    den = z * r + eps
    ref = x * mp.log(y + r) + y * mp.log(x + r) - z * mp.atan(x * y / den)
    env = abs(x) * _log_env(y, r) + abs(y) * _log_env(x, r) + abs(z) * _atan_env(x * y, den, abs(z * r) + eps)
    return ref, env


def magn_mp(x, y, z, bx, by, bz):
    """sensormodel.py:130-133: -(1 / |B|) (2 by bz log(x + r) + 2 bz bx log(y + r) + 2 by bx log(z + r)
    + (bz^2 - by^2) atan(x z / (y r)) + (bz^2 - bx^2) atan(y z / (x r)))."""
    x, y, z = mpf(float(x)), mpf(float(y)), mpf(float(z))
    bx, by, bz = mpf(float(bx)), mpf(float(by)), mpf(float(bz))
    r = mp.sqrt(x * x + y * y + z * z)
    nb = mp.sqrt(bx * bx + by * by + bz * bz)
    c = (2 * by * bz, 2 * bz * bx, 2 * by * bx, bz * bz - by * by, bz * bz - bx * bx)
    ca = (abs(c[0]), abs(c[1]), abs(c[2]), bz * bz + by * by, bz * bz + bx * bx)
    ref = -(c[0] * mp.log(x + r) + c[1] * mp.log(y + r) + c[2] * mp.log(z + r) + c[3] * mp.atan(x * z / (y * r))
            + c[4] * mp.atan(y * z / (x * r))) / nb
    env = (ca[0] * _log_env(x, r) + ca[1] * _log_env(y, r) + ca[2] * _log_env(z, r)
           + ca[3] * _atan_env(x * z, y * r, abs(y * r)) + ca[4] * _atan_env(y * z, x * r, abs(x * r))) / nb
    return ref, env


@functools.lru_cache(maxsize=None)
def potential_points():
    """(x, y, z): 128 generic corner offsets in +-3e3 and 128 with x or y on a 1e6-padded boundary plane, both signs (y + r of a
    large negative y cancels), z in {0.5, 50, 3e3}; no coordinate is exactly zero."""
    rng = np.random.default_rng(11)
    n = 256
    x, y = rng.uniform(-3e3, 3e3, n), rng.uniform(-3e3, 3e3, n)
    z = np.array([0.5, 50.0, 3e3])[np.arange(n) % 3]
    far = 1e6 + rng.uniform(0, 3e3, n)
    for k, (axis, sign) in enumerate(((x, 1.0), (x, -1.0), (y, 1.0), (y, -1.0))):
        sl = slice(128 + 32 * k, 128 + 32 * (k + 1))
        axis[sl] = sign * far[sl]
    assert (x != 0).all() and (y != 0).all()
    for a in (x, y, z):
        a.setflags(write=False)
    return x, y, z


@functools.lru_cache(maxsize=None)
def potential_table(func):
    x, y, z = potential_points()
    f = grav_mp if func == "grav" else (lambda a, b, c: magn_mp(a, b, c, *B_FIELD))
    out = [f(a, b, c) for a, b, c in zip(x, y, z)]
    return [o[0] for o in out], [o[1] for o in out]


def max_ulps_potential(got, func):
    ref, env = potential_table(func)
    u = [ulps(g, r, e) for g, r, e in zip(np.asarray(got, dtype=np.float64), ref, env)]
    i = int(np.argmax(u))
    return u[i], i
