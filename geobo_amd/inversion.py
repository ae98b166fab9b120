"""Joint GP inversion -- the reference's `geobo/inversion.py` `Inversion` class on the MI355X path.

Same constructor-less usage, attributes and method signatures as the reference:

    inv = Inversion()                       # settings: geobo_amd.config_loader.load(...) (or pass settings=)
    voxelpos = inv.create_cubegeometry()
    density_rec, magsus_rec, drill_rec, density_var, magsus_var, drill_var = \
        inv.cubing(gravfield, magfield, drillfield, sensor_locations, drilldata0)

`method` selects how A K is formed: "dense" = fused fp64-MFMA contraction with the covariance tile generated in the
kernel (any grid), "spectral" = real-DFT route on batched MFMA GEMMs (regular grids with extents % 16 == 0, ~40x
faster at 64^3, same results to ~1e-13), "auto" (default) = spectral when applicable.  `assembly="f32"` keeps the covariance
tables and A K in fp32 (BASELINE config 5: fp32 kernel assembly + fp64 Cholesky; results at fp32-storage accuracy, ~1e-5),
`operators="streamed"` generates the forward operators in batches instead of keeping them resident; "auto" (default) does so where it costs nothing (lattice survey on one device: the transforms read the stencil table, AkA is the lattice Gram), "resident" never.

`cubing`/`predict3`/`calc_logl` run matrix-free on the GPU (engine.PosteriorEngine): D2, the 3N x 3N prior
and the 3N x 3N posterior covariance of the reference (inversion.py:92,117) are never formed -- only the
posterior diagonal that `cubing` consumes (inversion.py:238).  No CPU fallback exists.
"""
import sys

import numpy as np
import torch

from . import config_loader, geometry
from . import kernels as kernel
from . import sensormodel as sm
from .engine import CholeskyError, FactorisationTimeout, PosteriorEngine, create_cov_lengths, weight_matrix
from .sampling import PriorSampler, SamplingError, observation_noise  # noqa: F401  (SamplingError: public)


class DiagonalCovariance:
    """What `predict3` returns in place of the (3N,3N) posterior covariance unless `full_cov=True`: only its diagonal exists.

    The reference consumes nothing but `np.diag(self.cov_rec)` (inversion.py:238).  That idiom works on this object:
    `np.diag(obj)` / `np.diagonal(obj)` are answered through NumPy's `__array_function__` protocol with the stored diagonal
    (no (3N)^2 array is ever built); `.diagonal()` and `.shape` behave like the matrix's.  Anything that needs off-diagonal
    entries (`np.asarray(obj)`, arithmetic) raises TypeError -- ask `predict3(full_cov=True)` for the matrix on small cubes."""

    def __init__(self, diag):
        self._d = np.asarray(diag)
        self.shape = (self._d.size, self._d.size)
        self.ndim = 2
        self.dtype = self._d.dtype

    def diagonal(self, offset=0):
        if offset != 0:
            raise TypeError("only the main diagonal of the posterior covariance is kept")
        return self._d

    def __array_function__(self, func, types, args, kwargs):
        if func in (np.diag, np.diagonal) and args and args[0] is self:
            k = kwargs.get("k", kwargs.get("offset", args[1] if len(args) > 1 else 0))
            return self.diagonal(k)
        if func is np.shape:
            return self.shape
        return NotImplemented

    def __array__(self, dtype=None, copy=None):
        raise TypeError("the MI355X path keeps only the diagonal of the posterior covariance; use np.diag(obj) / "
                        ".diagonal(), or predict3(full_cov=True) on a cube small enough to hold (3N)^2 doubles")


def reference_length_direction(xvoxsize):
    """d lengths / d l of calc_logl's single length scale: l xvox (1, 1, 1) becomes l xvox (1, 1.02, 1) in create_cov."""
    return xvoxsize * np.array([1.0, 1.02, 1.0])


def _zscore(v):
    """(v - mean) / std with the population std, and that std (inversion.py:209-214); NaN for an empty vector."""
    with np.errstate(all="ignore"):
        if not v.size:
            return v - np.nan, np.nan
        std = v.std()
        return (v - v.mean()) / std, std


def _hyper_key(gp_amp, lengths, coeffm):
    return (float(gp_amp), tuple(float(v) for v in np.asarray(lengths).reshape(-1)), tuple(float(v) for v in np.asarray(coeffm).reshape(-1)))


class Inversion:
    """Class for inversion and reconstruction of 3D cubes from 2D sensor data (inversion.py:23-248)."""

    def __init__(self, settings=None, props=(0, 1, 2), rank=0, world=1, group=None, device=None, profile=False,
                 method="auto", assembly="f64", operators="auto"):
        self.settings = s = settings or config_loader.active()
        # inversion.py:46-51 -- NB x voxel size for all three length scales
        self.gp_length = s.gp_lengthscale * np.asarray([s.xvoxsize, s.xvoxsize, s.xvoxsize])
        self.gp_sigma = np.asarray(s.gp_err)
        self.coeffm = np.asarray(s.gp_coeff)
        self.gp_amp = 1.
        self.props = tuple(props)
        self._engine_args = dict(rank=rank, world=world, group=group, device=device, profile=profile, method=method,
                                 assembly=assembly, operators=operators)
        self._engine = None

    # ---- geometry (host, inversion.py:54-74) -------------------------------------------------------------------
    def create_cubegeometry(self):
        """Node grid `Edges` (3, yN+1, xN+1, zN+1; z negated), voxel centres `xxx, yyy, zzz` (yN, xN, zN) and the (3, N)
        centre list `voxelpos` it returns, all expanded from the 1-D axes of geobo_amd.geometry."""
        s = self.settings
        self.Edges = geometry.expand(*geometry.node_axes(s))
        centres = geometry.expand(*geometry.centre_axes(s))
        self.xxx, self.yyy, self.zzz = centres[0], centres[1], centres[2]
        self.voxelpos = centres.reshape(3, -1).copy()
        return self.voxelpos

    # ---- engine --------------------------------------------------------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            self._engine = PosteriorEngine(self.settings, **self._engine_args)
        return self._engine

    def _operators(self):
        eng = self.engine
        axes = None
        if hasattr(self, "Edges"):
            # the meshgrid check of the node tensor costs a millisecond at 64^3: once per Edges object
            if getattr(self, "_axes_of", (None, None))[0] is not self.Edges:
                self._axes_of = (self.Edges, sm._edge_axes(self.Edges, eng.nx, eng.ny, eng.nz))
            axes = self._axes_of[1]
        A_g = eng.operator("grav", self.sensor_locations, B=self.settings.magneticField * 0., axes=axes)
        A_m = eng.operator("magn", self.sensor_locations, B=self.settings.magneticField, axes=axes)
        return A_g, A_m

    def _drill_selection(self):
        # inversion.py:219 + sensormodel.A_drill: rows = voxels with non-zero drill data, ascending flat index
        return np.flatnonzero(np.asarray(self.drilldata0).reshape(-1) != 0)

    def _run(self, gp_amp, gp_length, coeffm, calclogl, want_mean_var, directions=None):
        """One step of the engine: posterior(), or with `directions` (lists of three length components, metres) the likelihood
        and its exact gradient (PosteriorEngine.logl_grad)."""
        A_g, A_m = self._operators()
        lengths = create_cov_lengths(gp_length)  # in-place edit of the caller's array, like create_cov
        self._step_params = None   # (set below once the step has returned: what the engine's factor was built from)
        ng, nm = self.gravfield.size, self.magfield.size
        args = (A_g, A_m, self._sel, self.Fs3[:ng], self.Fs3[ng:ng + nm], self.Fs3[ng + nm:], [float(v) for v in lengths],
                self.coeffm if coeffm is None else coeffm, self.settings.kernelfunc, self.gp_sigma)
        if directions is None:
            step = lambda **kw: self.engine.posterior(*args, gp_amp=gp_amp, props=self.props, calclogl=calclogl,
                                                      want_mean_var=want_mean_var, **kw)
        else:
            step = lambda **kw: self.engine.logl_grad(*args, gp_amp, directions, **kw)
        try:
            r = step()
            self._step_params = _hyper_key(gp_amp, lengths, self.coeffm if coeffm is None else coeffm)
            return r
        except FactorisationTimeout:
            # (round-5 advisory) the tile DAG's bounded spins can trip on a device shared with other processes: once more, on the
            # stream schedule of rounds 2-4 (no inter-workgroup hand-offs), instead of returning an undefined factor
            import warnings
            warnings.warn("geobo_potrf_inv: tile-DAG hand-off timed out (info = -7); repeating the step on the stream schedule", RuntimeWarning)
            r = step(potrf_schedule="streams")
            self._step_params = _hyper_key(gp_amp, lengths, self.coeffm if coeffm is None else coeffm)
            return r

    # ---- inversion.py:77-122 ----------------------------------------------------------------------------------------
    def predict3(self, calclogl=False, full_cov=False):
        """Mean, covariance and log-likelihood of the GP with the 3x3 block kernel.
        The covariance is a diagonal-backed object (`np.diag(cov)` works, inversion.py:238) unless `full_cov=True`, which
        returns the (3N, 3N) matrix K - V^T V of inversion.py:117 -- only for cubes where 9 N^2 doubles fit (tests, small N)."""
        self.datastd = np.mean([np.nanstd(self.gravfield), np.nanstd(self.magfield), np.nanstd(self.drillfield)])
        try:
            r = self._run(self.gp_amp, self.gp_length, None, calclogl, True)
        except CholeskyError:
            if self.settings.kernelfunc == "matern32" and len(set(np.asarray(self.gp_length, dtype=float).tolist())) < 3:
                # the reference exits here too (its Matern cross term is 0/0 at equal lengths, kernels.py:148-156, and
                # create_cov turns the default [l,l,l] into [l,1.02l,l]); say why before the two reference lines
                print("matern32 needs three DISTINCT length scales: gp_length = %s has equal entries, which makes the "
                      "cross-covariance NaN. Set e.g. inv.gp_length = l * np.array([1.00, 1.02, 1.04])." % (self.gp_length,))
            print("Cholesky decompostion failed, AkA matrix i likely not positive semitive.")
            print("Change GP parameter settings")
            sys.exit(1)
        cov = DiagonalCovariance(r["var"])
        if full_cov:
            cov = self.engine.posterior_covariance(self.settings.kernelfunc, r["lengths"], self.coeffm, self.gp_amp)
        return r["mu"], cov, r["logl"]

    # ---- inversion.py:125-152 ---------------------------------------------------------------------------------------
    def calc_logl(self, params):
        """Negative marginal log-likelihood for hyper-parameters (amplitude, lengthscale, 3 correlation coefficients)."""
        s = self.settings
        gp_amp = params[0]
        gp_length = params[1] * np.asarray([s.xvoxsize, s.xvoxsize, s.xvoxsize])
        coeffm = params[2:]
        try:
            r = self._run(gp_amp, gp_length, coeffm, True, False)
            logl = -0.5 * (r["uu"] + r["logdet"])  # no N log 2pi term here (inversion.py:147-149)
            if not np.isfinite(logl):
                logl = -np.inf
        except Exception:
            logl = -np.inf
        return -logl

    def calc_logl_grad(self, params):
        """calc_logl(params) and its exact gradient in the same 5 parameters (amplitude, lengthscale in x-voxels, w1, w2, w3).
        The value comes from the same step as calc_logl's and equals it bit for bit; the gradient is <K^-1 - alpha alpha^T, dK>/2
        on the device (PosteriorEngine.logl_grad).  The lengths after create_cov's mutation are l xvox (1, 1.02, 1), so d/dl is ONE
        directional derivative along xvox (1, 1.02, 1).  Failure (as calc_logl's inf): (inf, NaN * ones(5))."""
        s = self.settings
        gp_amp = params[0]
        gp_length = params[1] * np.asarray([s.xvoxsize, s.xvoxsize, s.xvoxsize])
        coeffm = params[2:]
        try:
            r = self._run(gp_amp, gp_length, coeffm, True, False, directions=[reference_length_direction(s.xvoxsize)])
            logl = -0.5 * (r["uu"] + r["logdet"])
            grad = np.r_[r["d_amp"], r["d_dir"][0], r["d_w"]]
            if not np.isfinite(logl) or not np.isfinite(grad).all():
                raise FloatingPointError
        except Exception:
            return np.inf, np.full(5, np.nan)
        return -logl, grad

    def neg_logl_and_grad(self, gp_amp, gp_length, coeffm):
        """Negative log marginal likelihood (calc_logl's objective) and its gradient in the 7 parameters (amplitude, l0, l1, l2, w1, w2,
        w3) with three free length scales in metres, taken after create_cov's mutation (applied to a copy: gp_length is not edited).
        Three directional derivatives, one per length.  Failure: (inf, NaN * ones(7))."""
        lengths = np.array(gp_length, dtype=float).reshape(3)
        try:
            r = self._run(float(gp_amp), lengths, np.asarray(coeffm, dtype=float), True, False, directions=list(np.eye(3)))
            logl = -0.5 * (r["uu"] + r["logdet"])
            grad = np.r_[r["d_amp"], r["d_dir"], r["d_w"]]
            if not np.isfinite(logl) or not np.isfinite(grad).all():
                raise FloatingPointError
        except Exception:
            return np.inf, np.full(7, np.nan)
        return -logl, grad

    # ---- inversion.py:155-178 ---------------------------------------------------------------------------------------
    def hyper_bounds(self):
        """Search box of optimize_gp: amplitude, lengthscale (in x-voxels) and the three cross-correlation weights."""
        s = self.settings
        box = [(0.5, 2), (0.5 * s.gp_lengthscale, 10 * s.gp_lengthscale)]
        return tuple(box + [(0.5 * w, 1) for w in s.gp_coeff])

    def set_hyperparameters(self, x):
        """Adopt a hyper-parameter vector (amplitude, lengthscale in x-voxels, w1, w2, w3).
        The reference keeps the bare lengthscale scalar in gp_length at this point (inversion.py:175), which its own create_cov
        can no longer index; everywhere else gp_length is lengthscale * x-voxel size for all three blocks (:48, :137), so
        that is what is stored here."""
        x = np.asarray(x, dtype=float)
        self.gp_amp = x[0]
        self.gp_length = x[1] * np.full(3, self.settings.xvoxsize)
        self.coeffm = x[2:5].copy()

    def optimize_gp(self):
        """Maximise the marginal likelihood over the box of hyper_bounds() (the reference's entry point and signature): SHGO as the
        reference, or L-BFGS-B on the exact gradient where the settings carry optimize_method: "L-BFGS-B" (optional YAML key,
        default "shgo").  See optimize_hyperparameters."""
        return self.optimize_hyperparameters(method=getattr(self.settings, "optimize_method", "shgo"))

    def optimize_hyperparameters(self, method="shgo", free_lengths=False):
        """Maximise the marginal likelihood over the box of hyper_bounds().
        method "shgo" (default): SciPy's SHGO (10 Sobol points x 10 iterations, as the reference); every objective evaluation is one
        AkA + Cholesky + log-det on the device.
        method "L-BFGS-B": scipy.optimize.minimize with the exact gradient (calc_logl_grad), from the current parameters.
        free_lengths (L-BFGS-B only): the 7 parameters of neg_logl_and_grad -- three free length scales, each in the reference's length
        box -- which makes Matern-3/2 fittable; the result is stored in gp_length as three lengths."""
        print("Optimizing GP hyperparameters and correlation coefficients, this may take a while...")
        self.datastd = np.mean([np.nanstd(v) for v in (self.gravfield, self.magfield, self.drillfield)])
        if method == "L-BFGS-B":
            return self._optimize_lbfgsb(free_lengths)
        if method != "shgo":
            raise ValueError("optimize_hyperparameters: method must be 'shgo' or 'L-BFGS-B', got %r" % (method,))
        if free_lengths:
            raise ValueError("free_lengths needs method='L-BFGS-B'")
        from scipy.optimize import shgo
        found = shgo(self.calc_logl, bounds=self.hyper_bounds(), n=10, iters=10, sampling_method="sobol")
        if not found.success:
            print("WARNING: " + found.message)     # parameters stay as they were
            return found
        report = lambda title: print(title + "\n" + " ".join(str(v) for v in (self.gp_amp, self.gp_length, self.coeffm)))
        report("Initial parameter [amplitude, lengthscale, corr1, corr2, corr3]:")
        self.set_hyperparameters(found.x)
        report("Optimized parameter [amplitude, lengthscale, corr1, corr2, corr3]:")
        return found

    def _optimize_lbfgsb(self, free_lengths):
        """optimize_hyperparameters(method="L-BFGS-B"): bounded quasi-Newton on the exact gradient.  Lengths are optimised in x-voxel
        units (the 7-vector's gradient is scaled accordingly), which keeps the problem as well scaled as the reference's 5-vector."""
        from scipy.optimize import minimize
        s = self.settings
        xv = s.xvoxsize
        box = self.hyper_bounds()
        if free_lengths:
            bounds = [box[0]] + [box[1]] * 3 + list(box[2:])
            x0 = np.r_[self.gp_amp, np.asarray(self.gp_length, dtype=float) / xv, self.coeffm]

            def fun(x):
                f, g = self.neg_logl_and_grad(x[0], x[1:4] * xv, x[4:7])
                return f, np.r_[g[0], g[1:4] * xv, g[4:7]]
        else:
            bounds = list(box)
            x0 = np.r_[self.gp_amp, float(np.asarray(self.gp_length, dtype=float)[0]) / xv, self.coeffm]
            fun = self.calc_logl_grad
        x0 = np.clip(np.asarray(x0, dtype=float), [b[0] for b in bounds], [b[1] for b in bounds])
        found = minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=bounds)
        if not found.success:
            print("WARNING: " + str(found.message))     # parameters stay as they were
            return found
        report = lambda title: print(title + "\n" + " ".join(str(v) for v in (self.gp_amp, self.gp_length, self.coeffm)))
        if free_lengths:
            report("Initial parameter [amplitude, lengthscale, corr1, corr2, corr3]:")
            x = np.asarray(found.x, dtype=float)
            self.gp_amp, self.gp_length, self.coeffm = x[0], x[1:4] * xv, x[4:7].copy()
            report("Optimized parameter [amplitude, lengthscale, corr1, corr2, corr3]:")
        else:
            report("Initial parameter [amplitude, lengthscale, corr1, corr2, corr3]:")
            self.set_hyperparameters(found.x)
            report("Optimized parameter [amplitude, lengthscale, corr1, corr2, corr3]:")
        return found

    # ---- inversion.py:182-248 ---------------------------------------------------------------------------------------
    def cubing(self, gravfield, magfield, drillfield, sensor_locations, drilldata0):
        """Joint inversion and cubing of sensor data; returns the six cubes of the reference, each (yN, xN, zN)."""
        s = self.settings
        # no dtype cast: the reference z-scores the survey in the dtype it arrives in (float32 from a GeoTIFF
        # through scipy zoom, run_geobo.py:56-60) -- inversion.py:209-214
        self.gravfield = np.asarray(gravfield)
        self.magfield = np.asarray(magfield)
        self.drillfield = np.asarray(drillfield)
        self.sensor_locations = sensor_locations
        self.drilldata0 = drilldata0
        if not hasattr(self, "voxelpos"):
            self.create_cubegeometry()
        # population z-score of each data vector in the dtype it arrives in; an empty drill vector gives NaN statistics
        # (and NaN drill cubes), like the reference
        gravfield_norm, grav_std = _zscore(self.gravfield)
        magfield_norm, magn_std = _zscore(self.magfield)
        drillfield_norm, drill_std = _zscore(self.drillfield)
        gkey = (s.xNcube, s.yNcube, s.zNcube, s.xvoxsize, s.yvoxsize, s.zvoxsize)
        if getattr(self, "_points_key", None) != gkey:
            self._points_key, self._points3D = gkey, kernel.calcGridPoints3D(gkey[:3], gkey[3:])
        self.points3D = self._points3D
        self._sel = self._drill_selection()
        if self._sel.size != self.drillfield.size:
            raise ValueError("drillfield must hold one value per non-zero voxel of drilldata0")
        self.Fs3 = np.hstack((gravfield_norm, magfield_norm, drillfield_norm))
        if s.optimize_gp:
            self.optimize_gp()     # (optional YAML key optimize_method: "shgo", the default, or "L-BFGS-B")
        self.mu_rec, self.cov_rec, self.logl = self.predict3(calclogl=True)
        shape = (3, s.yNcube, s.xNcube, s.zNcube)
        mean_cubes = self.mu_rec.reshape(shape)
        var_cubes = np.diag(self.cov_rec).reshape(shape)           # the reference's own idiom (inversion.py:238)
        # deviations from the data means, back in data units (the means themselves are not restored, inversion.py:242-247)
        # (the std scalars keep the survey's dtype: a float32 survey squares its std in float32, as the reference does)
        scale = (grav_std, magn_std, drill_std)
        self._cube_scale = scale
        with np.errstate(all="ignore"):
            rec = [mean_cubes[i] * scale[i] for i in range(3)]
            var = [var_cubes[i] * scale[i] ** 2 for i in range(3)]
        return rec[0], rec[1], rec[2], var[0], var[1], var[2]

    # ---- new drill values without a new step --------------------------------------------------------------
    def _new_drill_rows(self, voxels, values, normalised=False):
        """(flat voxel indices, values in the GP's normalised units) of new drill observations, checked on the host: voxels as flat
        (iy, ix, iz) indices or a (k, 3) array of (iy, ix, iz); values in data units unless `normalised` -- then they are z-scored with
        the mean and population std of cubing()'s own drillfield (the survey's normalisation is frozen)."""
        if not hasattr(self, "Fs3") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("assimilate_drill() adds rows to the survey of cubing(): call cubing() first")
        s = self.settings
        ny, nx, nz = s.yNcube, s.xNcube, s.zNcube
        N = ny * nx * nz
        vox = np.asarray(voxels)
        if vox.size and not np.issubdtype(vox.dtype, np.integer):
            raise ValueError("voxels must be integer indices")
        if vox.ndim == 2 and vox.shape[1] == 3:
            if np.any(vox < 0) or np.any(vox >= np.array([ny, nx, nz])):
                raise ValueError("voxel indices (iy, ix, iz) must lie inside the (%d, %d, %d) cube" % (ny, nx, nz))
            vox = (vox[:, 0].astype(np.int64) * nx + vox[:, 1]) * nz + vox[:, 2]
        elif vox.ndim != 1:
            raise ValueError("voxels must be flat (iy, ix, iz) indices or a (k, 3) index array")
        vox = vox.astype(np.int64)
        vals = np.asarray(values, dtype=np.float64).reshape(-1)
        if vals.size != vox.size:
            raise ValueError("%d values for %d voxels" % (vals.size, vox.size))
        if vox.size < 1:
            raise ValueError("assimilate_drill() needs at least one voxel")
        if np.any(vox < 0) or np.any(vox >= N):
            raise ValueError("voxels must be flat voxel indices in [0, %d)" % N)
        if np.unique(vox).size != vox.size:
            raise ValueError("voxels repeat: one drill value per voxel")
        seen = np.intersect1d(vox, self._sel)
        if seen.size:
            raise ValueError("voxels %s carry a drill value already" % seen[:8])
        if not normalised:
            d = np.asarray(self.drillfield, dtype=np.float64)
            if not d.size or not d.std() > 0.0:
                raise ValueError("cubing()'s drillfield has no spread: new values cannot be normalised; pass normalised=True")
            vals = (vals - d.mean()) / d.std()
        return vox, vals

    def assimilate_drill(self, voxels, values, normalised=False):
        """New drill values after cubing(), without a new step: the factor of cubing()'s step is extended by one row per voxel
        (PosteriorEngine.append_drill_rows) and the six cubes are updated in place of recomputed.  voxels: flat (iy, ix, iz) indices or
        a (k, 3) index array of voxels that carry no drill value yet; values: in data units (normalised=True: already in the GP's units).
        The survey's normalisation is FROZEN: new values are z-scored with the mean and population std of cubing()'s drillfield, and
        the cubes come back in cubing()'s units.  A fresh cubing() on the union of the data re-normalises all three data vectors from
        the union and therefore returns (slightly) different cubes; this call gives what the reference's GP gives for the union at the
        survey's own normalisation.  The rows are appended to the survey (a later rebuild of the factor contains them), mu_rec,
        cov_rec and logl follow, and every product that works from the step's factor sees them.  Returns the six cubes."""
        vox, vals = self._new_drill_rows(voxels, values, normalised)
        self._ensure_factor()
        last = self.engine.last
        if last.get("uu") is None or not self.engine.mean_var_known():
            # the factor was rebuilt without the likelihood or the mean (after a refactoring campaign, a cross-validation at other
            # parameters), or rows went in or out without the mean: one whole step gives the state the rows are appended to
            self._run(self.gp_amp, self.gp_length, None, True, True)
        r = self.engine.append_drill_rows(vox, vals, want_mean_var=True)
        self._sel = np.concatenate([np.asarray(self._sel, dtype=np.int64), vox])
        self.Fs3 = np.hstack((self.Fs3, vals))
        self.mu_rec, self.cov_rec = r["mu"], DiagonalCovariance(r["var"])
        if "uu" in r:
            self.logl = r["logl"]
        s = self.settings
        shape = (3, s.yNcube, s.xNcube, s.zNcube)
        mean_cubes, var_cubes = self.mu_rec.reshape(shape), r["var"].reshape(shape)
        scale = self._cube_scale
        with np.errstate(all="ignore"):
            rec = [mean_cubes[i] * scale[i] for i in range(3)]
            var = [var_cubes[i] * scale[i] ** 2 for i in range(3)]
        return rec[0], rec[1], rec[2], var[0], var[1], var[2]

    # ---- down-weighting or dropping data rows -------------------------------------------------------------
    def _data_rows(self, grav=None, magn=None, drill=None):
        """Indices into the data vector [grav | magn | drill] of stations and drill rows named per data type: grav, magn: station
        indices; drill: drill row indices or a (k, 3) array of voxel indices (iy, ix, iz) that carry a drill value."""
        if not hasattr(self, "Fs3") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("the rows of a survey are those of cubing(): call cubing() first")
        s = self.settings
        ng, nm, nd = self.gravfield.size, self.magfield.size, self.Fs3.size - self.gravfield.size - self.magfield.size
        out = []
        for name, v, off, n in (("grav", grav, 0, ng), ("magn", magn, ng, nm), ("drill", drill, ng + nm, nd)):
            if v is None:
                continue
            v = np.asarray(v)
            if v.size and not np.issubdtype(v.dtype, np.integer):
                raise ValueError("%s must hold integer indices" % name)
            if name == "drill" and v.ndim == 2 and v.shape[1] == 3:
                if np.any(v < 0) or np.any(v >= np.array([s.yNcube, s.xNcube, s.zNcube])):
                    raise ValueError("voxel indices (iy, ix, iz) must lie inside the (%d, %d, %d) cube" % (s.yNcube, s.xNcube, s.zNcube))
                flat = (v[:, 0].astype(np.int64) * s.xNcube + v[:, 1]) * s.zNcube + v[:, 2]
                order = np.argsort(self._sel)
                pos = np.searchsorted(self._sel[order], flat)
                pos = np.minimum(pos, max(nd - 1, 0))
                if nd == 0 or np.any(self._sel[order][pos] != flat):
                    raise ValueError("a voxel named in drill carries no drill value")
                v = order[pos]
            v = v.reshape(-1).astype(np.int64)
            if np.any(v < 0) or np.any(v >= n):
                raise ValueError("%s indices must lie in [0, %d)" % (name, n))
            out.append(v + off)
        rows = np.concatenate(out) if out else np.zeros(0, dtype=np.int64)
        if rows.size < 1:
            raise ValueError("no data row is named")
        if np.unique(rows).size != rows.size:
            raise ValueError("a row is named twice")
        return rows

    def _stepped_with_mean(self):
        """The engine's factor at the current hyper-parameters with its likelihood, mean and variance (one whole step otherwise)."""
        self._ensure_factor()
        if self.engine.last.get("uu") is None or not self.engine.mean_var_known():
            self._run(self.gp_amp, self.gp_length, None, True, True)

    def _change_statistics(self, sum_dmu2, max_dmu, sum_dvar):
        """Per property, in cubing()'s units: RMS and largest change of the mean cube, mean increase of the variance."""
        N = self.engine.N
        sc = np.array([float(v) for v in self._cube_scale])
        with np.errstate(all="ignore"):
            return dict(rms_change=np.sqrt(np.asarray(sum_dmu2) / N) * sc, max_change=np.asarray(max_dmu) * sc,
                        mean_var_increase=np.asarray(sum_dvar) / N * sc ** 2)

    def _six_cubes(self, mu, var):
        s = self.settings
        shape = (3, s.yNcube, s.xNcube, s.zNcube)
        mean_cubes, var_cubes = np.asarray(mu).reshape(shape), np.asarray(var).reshape(shape)
        scale = self._cube_scale
        with np.errstate(all="ignore"):
            return tuple(mean_cubes[i] * scale[i] for i in range(3)) + tuple(var_cubes[i] * scale[i] ** 2 for i in range(3))

    def reweight_data(self, grav=None, magn=None, drill=None, scale=np.inf, commit=False, write=False):
        """The cubes without (scale=inf, the default) or with less weight on (scale > 1: that many times the noise standard
        deviation, a scalar or one per named row in the order grav, magn, drill) some data rows, after cubing().  grav, magn: station
        indices; drill: drill row indices or (k, 3) voxel indices (iy, ix, iz).
        commit=False: a preview from the factor the step left on the device -- no new step, nothing changes; at most 128 rows.
        commit=True: the scales are recorded (on top of those committed before; restore_data() clears them), ONE step runs with them,
        mu_rec, cov_rec and logl follow, and every later step and every product that works from the factor sees the reduced system;
        any number of rows.  The survey stays the full x-y lattice either way: the step keeps its lattice forms.
        Returns dict(cubes: the six cubes in cubing()'s units, logl, delta_logl, rows, and per property rms_change, max_change (of the
        mean cube) and mean_var_increase).  write=True: cube_<...>_dropped.vtk in outpath."""
        rows = self._data_rows(grav, magn, drill)
        from .reweight import check_scales
        sc = check_scales(scale, rows.size)
        eng = self.engine
        if not commit:
            self._stepped_with_mean()
        logl0 = float(self.logl)
        if not commit:
            r = eng.reweight_preview(rows, sc, want="cubes")
            h = eng._to_host(torch.cat([r["mu"].reshape(-1), r["var"].reshape(-1)]), 0)
            mu, var, logl = h[:3 * eng.N].copy(), h[3 * eng.N:].copy(), r["logl"]
            stats = self._change_statistics(r["sum_dmu2"], r["max_dmu"], r["sum_dvar"])
        else:
            if np.any(sc == 1.0):
                raise ValueError("a scale of 1 changes nothing: leave the row out")
            ng, nm = self.gravfield.size, self.magfield.size
            cur = eng._data_scales(self._sel)
            if np.any(np.isinf(cur[rows])):
                raise ValueError("rows %s are dropped already" % rows[np.isinf(cur[rows])][:8])
            cur[rows] = cur[rows] * sc
            rs = eng.row_scale
            per_voxel = np.ones(eng.N) if rs is None else rs["drill"].copy()
            per_voxel[self._sel] = cur[ng + nm:]
            mu0, var0 = np.asarray(self.mu_rec, dtype=np.float64), np.asarray(np.diag(self.cov_rec), dtype=np.float64)
            eng.set_row_scale(cur[:ng], cur[ng:ng + nm], per_voxel)
            try:
                r = self._run(self.gp_amp, self.gp_length, None, True, True)
            except Exception:
                eng.row_scale = rs
                self._step_params = None
                raise
            mu, var, logl = r["mu"], r["var"], r["logl"]
            self.mu_rec, self.cov_rec, self.logl = mu, DiagonalCovariance(var), logl
            d = (mu - mu0).reshape(3, -1)
            stats = self._change_statistics((d ** 2).sum(axis=1), np.abs(d).max(axis=1), (var - var0).reshape(3, -1).sum(axis=1))
        out = dict(cubes=self._six_cubes(mu, var), logl=float(logl), delta_logl=float(logl) - logl0, rows=rows, **stats)
        if write:
            self._write_dropped_cubes(out["cubes"])
        return out

    def _write_dropped_cubes(self, cubes):
        import os

        from . import dataio
        s = self.settings
        origin = (self.voxelpos[0].min(), self.voxelpos[1].min(), self.voxelpos[2].min())
        names = ["cube_density", "cube_magsus", "cube_drill", "cube_density_variance", "cube_magsus_variance", "cube_drill_variance"]
        for c, n in zip(cubes, names):
            dataio.create_vtkcube(c, origin, (s.xvoxsize, s.yvoxsize, s.zvoxsize), fname=os.path.join(s.outpath, n + "_dropped.vtk"))

    def restore_data(self):
        """Clear every committed row scale: the next step runs on the whole survey again and returns the bits it returned before
        the first reweight_data(commit=True).  The factor on the device is marked stale (the next product rebuilds it)."""
        self.engine.set_row_scale()
        self._step_params = None

    def _row_sigma(self):
        """Noise standard deviation per data row with the committed row scales (a dropped row: 0 -- it is not in the system)."""
        ng, nm = self.gravfield.size, self.magfield.size
        sig = np.concatenate([np.full(ng, float(self.gp_sigma[0])), np.full(nm, float(self.gp_sigma[1])),
                              np.full(self.Fs3.size - ng - nm, float(self.gp_sigma[2]))])
        if self._engine is None or self._engine.row_scale is None:
            return sig
        sc = self._engine._data_scales(self._sel)
        return np.where(np.isinf(sc), 0.0, sig * np.where(np.isinf(sc), 1.0, sc))

    def fold_influence(self, folds="holes", cell=None, write=False):
        """For every fold of cross_validate's fold definitions ("loo", "holes", "patches" or a list of index arrays into the data
        vector, at most 128 rows each), what the model would look like WITHOUT it, from the statistics-only preview (no step, no
        cube): a pandas table, one row per fold, with FOLD, SIZE, FIRST_ROW, DELTA_LOGL (log-likelihood of the remaining data minus
        that of all the data) and per property RMS_<p>, MAX_<p> (RMS and largest change of the mean cube) and DVAR_<p> (mean increase
        of the variance), in cubing()'s units, sorted by the summed relative RMS change (largest first; RANK).  Rows that are dropped
        already are in no fold.  write=True: fold_influence.csv in outpath."""
        import pandas as pd

        from .resources import PROPS
        self._check_cv_folds(folds)
        if not hasattr(self, "Fs3") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("fold_influence() works from the survey of cubing(): call cubing() first")
        eng = self.engine
        self._ensure_factor()
        if eng.last.get("uu") is None:
            self._run(self.gp_amp, self.gp_length, None, True, True)
        st = eng.last.get("append")
        uu, logdet = (st["uu"], st["logdet"]) if st is not None else (eng.last["uu"], eng.last["logdet"])
        logl0 = -0.5 * (uu + logdet + eng.N * np.log(2 * np.pi))
        rec = []
        for c, fold in enumerate(self._cv_folds(folds, cell)):
            fold = np.asarray(fold, dtype=np.int64).reshape(-1)
            fold = fold[fold >= 0]
            r = eng.reweight_preview(fold, np.inf, want="stats")
            ch = self._change_statistics(r["sum_dmu2"], r["max_dmu"], r["sum_dvar"])
            row = dict(FOLD=c, SIZE=fold.size, FIRST_ROW=int(fold.min()), DELTA_LOGL=r["logl"] - logl0)
            for i, p in enumerate(PROPS):
                row.update({"RMS_" + p.upper(): ch["rms_change"][i], "MAX_" + p.upper(): ch["max_change"][i],
                            "DVAR_" + p.upper(): ch["mean_var_increase"][i]})
            rec.append(row)
        table = pd.DataFrame(rec)
        if len(table):
            sc = np.array([float(v) for v in self._cube_scale])
            with np.errstate(all="ignore"):
                score = np.nansum(np.stack([table["RMS_" + p.upper()].to_numpy() / sc[i] for i, p in enumerate(PROPS)]), axis=0)
            table = table.iloc[np.argsort(-score, kind="stable")].reset_index(drop=True)
            table.insert(0, "RANK", np.arange(1, len(table) + 1))
        if write:
            import os
            table.to_csv(os.path.join(self.settings.outpath, "fold_influence.csv"), index=False)
        return table

    # ---- posterior realisations ---------------------------------------------------------------------------
    def _prior_sampler(self, approximate):
        """PriorSampler of the current hyper-parameters (cached per grid, kernel, lengths, weights, amplitude)."""
        s = self.settings
        lengths = create_cov_lengths(np.array(self.gp_length, dtype=float))
        args = ((s.yNcube, s.xNcube, s.zNcube), (s.xvoxsize, s.yvoxsize, s.zvoxsize), s.kernelfunc, [float(v) for v in lengths],
                weight_matrix(self.coeffm), float(self.gp_amp))
        key = (args[0], args[1], args[2], tuple(args[3]), tuple(map(tuple, args[4])), args[5], bool(approximate))
        hit = getattr(self, "_sampler_cache", None)
        if hit is None or hit[0] != key:
            hit = self._sampler_cache = (key, PriorSampler(*args, device=self.engine.device, approximate=approximate))
        return hit[1]

    def _sample_cubes(self, f, scale=(1.0, 1.0, 1.0)):
        s = self.settings
        h = f.cpu().numpy().reshape(f.shape[0], 3, s.yNcube, s.xNcube, s.zNcube)
        with np.errstate(all="ignore"):
            return tuple(h[:, i] * scale[i] for i in range(3))

    def sample_prior(self, n, seed=0, start=0, approximate=False):
        """n realisations of the prior N(0, K) of create_cov (current gp_amp, gp_length, coeffm), drawn on the device by circulant
        embedding: three arrays (n, yN, xN, zN) in the GP's normalised units.  Sample k (start <= k < start + n) depends only on (seed, k).
        A prior whose cross-spectra are indefinite (possible with three distinct lengths and large weights) raises SamplingError;
        approximate=True clips the negative eigenvalues of every frequency's 3 x 3 spectrum instead and returns the clipped fraction
        (clipped trace / trace) as a fourth element."""
        smp = self._prior_sampler(approximate)
        out = self._sample_cubes(smp.sample(int(start), int(n), seed=int(seed)))
        return out + (smp.clipped_fraction,) if approximate else out

    def sample_posterior(self, n, seed=0, start=0, approximate=False, batch=None, prior=None, noise=None):
        """n realisations of the joint posterior of the last cubing() survey, by Matheron's rule on the device:
            f_post = f + K A3^T H^-1 (y - A3 f - eps),   f ~ N(0, K) (sample_prior),  eps ~ N(0, Sigma),  H = A3 K A3^T + Sigma,
        which has exactly the posterior law N(mu, K - K A3^T H^-1 A3 K).  Returns three arrays (n, yN, xN, zN) in cubing()'s units (times
        the data std of each block), so their mean tends to cubing()'s first three cubes.  Sample k depends only on (seed, k): start
        addresses realisations, batch (default 64, at most 256) only bounds device memory.  The factor of the current hyper-parameters is reused, or
        rebuilt (without the mean and variance) when the last step used others.
        approximate=True (indefinite prior, see sample_prior): the clipped part E of the prior spectra leaves the samples' covariance off
        by (I - G A3) E (I - G A3)^T, G = K A3^T H^-1; the clipped fraction is returned as a fourth element.
        Tests: prior = (n, 3, N) array of f, noise = (n, M) array of eps (rows grav | magn | drill) replace the generators."""
        if not hasattr(self, "Fs3") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("sample_posterior() conditions on the survey of cubing(): call cubing() first")
        parts, ws, es = [], [], []
        for fp, w, e in self._posterior_batches(n, seed, start, approximate, batch, prior, noise):
            parts.append(self._sample_cubes(fp, self._cube_scale))
            ws.append(w.cpu().numpy())
            es.append(e.cpu().numpy())
        clipped = self._sampler_cache[1].clipped_fraction
        self.sample_info = dict(noise=np.concatenate(es), w=np.concatenate(ws), clipped_fraction=clipped)
        out = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
        return out + (clipped,) if approximate else out

    def _posterior_batches(self, n, seed=0, start=0, approximate=False, batch=None, prior=None, noise=None):
        """The realisations start .. start + n - 1 of sample_posterior() as device batches, in order: yields (f_post (k, 3, N) in
        normalised units, w (k, M), eps (k, M)) per batch, views of the batch's tensors cut to the requested realisations."""
        eng = self.engine
        self._ensure_factor()
        # (with the caller's f only the exact spectra of K are used: an indefinite prior is no obstacle there)
        smp = self._prior_sampler(approximate or prior is not None)
        A_g, A_m = self._operators()
        ng, nm = self.gravfield.size, self.magfield.size
        y_g, y_m, y_d = self.Fs3[:ng], self.Fs3[ng:ng + nm], self.Fs3[ng + nm:]
        M = ng + nm + y_d.size
        sig = self._row_sigma()
        sig_t = torch.as_tensor(sig, dtype=torch.float64, device=eng.device)
        n, start = int(n), int(start)
        # conditioning transforms two samples per complex line: sample k always shares it with sample k ^ 1 (batches start at even
        # absolute indices and hold an even count, at most 256 -- one GEMM tile of rows), so its bits do not depend on the batching
        batch = max(2, min(256, int(batch or 64)) // 2 * 2)
        lo, hi = start - start % 2, start + n + (start + n) % 2

        def given(a, b0, nb, shape):
            out = np.zeros((nb,) + shape)
            i0, i1 = max(b0, start), min(b0 + nb, start + n)
            out[i0 - b0:i1 - b0] = np.asarray(a, dtype=np.float64)[i0 - start:i1 - start].reshape((i1 - i0,) + shape)
            return torch.as_tensor(out, device=eng.device)
        for b0 in range(lo, hi, batch):
            nb = min(batch, hi - b0)
            f = given(prior, b0, nb, (3, eng.N)) if prior is not None else smp.sample(b0, nb, seed=int(seed))
            e = given(noise, b0, nb, (M,)) if noise is not None else observation_noise(int(seed), b0, nb, M, device=eng.device) * sig_t
            fp, w = eng.condition(f, e, A_g, A_m, y_g, y_m, y_d, smp)
            i0, i1 = max(b0, start) - b0, min(b0 + nb, start + n) - b0
            yield fp[i0:i1], w[i0:i1], e[i0:i1]

    # ---- grade-tonnage curves and exceedance probabilities ------------------------------------------------
    def grade_tonnage(self, cutoffs, prop="drill", n=256, seed=0, start=0, batch=64, offset=0.0, require=None, region=None, block=None,
                      voxel_probability=False, approximate=False, write=False):
        """Grade-tonnage curves of property `prop` ("density" | "magsus" | "drill" or 0 | 1 | 2) from the n posterior realisations
        sample_posterior(n, seed, start) of the last cubing() survey, reduced on the device: per realisation and cutoff the volume at
        or above the cutoff and the quantity it holds.  `cutoffs` (at most 32, any order) are in cubing()'s units after adding
        `offset`: the cubes are deviations from the data mean, so absolute grades take offset = drillfield.mean(); the value counted
        is cube + offset.  require = {property: lower bound} asks the other properties, at the same support and in cube units (no
        offset), to reach a bound as well; region is a boolean cube (yN, xN, zN) restricting the voxels.  block = (bx, by, bz) voxels
        (the order of block_statistics): the realisations are first averaged over the boxes of that block model (selection at block
        support; a block counts with its voxels) and region is (yB, xB, zB).  batch bounds device memory and changes no bit;
        approximate as in sample_posterior.
        Returns a dict: `cutoffs` (C,), `count` (n, C) int64 voxels, `volume` (n, C) m^3, `quantity` (n, C) = sum of value x voxel
        volume, `grade` (n, C) = quantity / volume (NaN where nothing passes), `quantiles` = {"volume", "quantity", "grade"}, each (3, C)
        with the 10 / 50 / 90 % quantiles over the realisations, with voxel_probability `probability` (C, yN, xN, zN) (or the block
        shape) = the fraction of realisations in which the voxel passes, with approximate `clipped_fraction`.  write=True:
        grade_tonnage.csv in outpath."""
        from . import resources
        q = self._cutoff_query("grade_tonnage() reduces realisations of the survey of cubing()", prop, cutoffs, offset, require, block, region,
                               n, start)
        eng = self.engine
        mask = self._on_device(q.mask)
        hits = torch.zeros((q.t.size, int(np.prod(q.shape))), dtype=torch.int32, device=eng.device) if voxel_probability else None
        cnts, sums = [], []
        for fp, _, _ in self._posterior_batches(q.n, seed, q.start, approximate, batch):
            c, v = eng.cutoff_statistics(fp, q.p, q.t, lo=q.lo, mask=mask, box=q.box, hits=hits)
            cnts.append(c)
            sums.append(v)
        out = dict(cutoffs=q.cut.copy())
        out.update(resources.tonnage_tables(torch.cat(cnts).cpu().numpy()[:, q.inverse], torch.cat(sums).cpu().numpy()[:, q.inverse],
                                            q.scale[q.p], offset, self._voxel_volume()))
        if voxel_probability:
            out["probability"] = self._probability(hits, q)
        if approximate:
            out["clipped_fraction"] = self._sampler_cache[1].clipped_fraction
        if write:
            import os
            resources.curve_frame(out).to_csv(os.path.join(self.settings.outpath, "grade_tonnage.csv"), index=False)
        return out

    def exceedance_probability(self, cutoffs, prop="drill", offset=0.0):
        """The analytic voxel-support counterpart of grade_tonnage()'s `probability`, from the mean and variance cubes of cubing():
        Phi((mu + offset - c) / sigma) per cutoff, shape (C, yN, xN, zN), in cubing()'s units.  NaN where the variance is not positive
        (and in the drill cubes without drill data); nothing is clipped.  Host only."""
        from . import resources
        p = resources.property_index(prop)
        if not hasattr(self, "mu_rec") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("exceedance_probability() reads the mean and variance cubes of cubing(): call cubing() first")
        s = self.settings
        shape = (3, s.yNcube, s.xNcube, s.zNcube)
        with np.errstate(all="ignore"):
            mean = np.asarray(self.mu_rec).reshape(shape)[p] * self._cube_scale[p]
            var = np.diag(self.cov_rec).reshape(shape)[p] * self._cube_scale[p] ** 2
        return resources.exceedance_probability(mean, var, cutoffs, offset)

    # ---- connected ore bodies -----------------------------------------------------------------------------
    def geobodies(self, cutoffs, prop="drill", n=256, seed=0, start=0, batch=64, offset=0.0, require=None, region=None, block=None,
                  neighbours=6, min_voxels=1, seeds=None, probability=None, approximate=False, write=False):
        """Connected bodies of the material at or above each cutoff, per posterior realisation, labelled and reduced on the device.
        cutoffs, prop, n, seed, start, batch, offset, require, region, block and approximate are those of grade_tonnage(): the sets are
        the same, so `count` equals grade_tonnage()'s.  neighbours: 6 (voxels joined by faces) or 26 (faces, edges, corners);
        min_voxels: the bodies counted in `n_bodies` hold at least that many voxels (at block support: voxels of their blocks).
        seeds: None, "drill" (the drilled voxels of cubing()), a boolean cube (yN, xN, zN) or a (K, 3) integer array of (ix, iy, iz);
        at block support a seed stands for its block.  The SEEDED body of a realisation is the union of the bodies that hold a seed
        which itself passes the cutoff.  probability: None, "largest", "seeded" or "both".
        Returns a dict with columns in the caller's cutoff order: `cutoffs` (C,), `n_bodies` (n, C), `count` (n, C), `largest` and
        `seeded` = dicts of `count`, `volume` (m^3), `quantity` and `grade` (n, C each; grade NaN when the body is empty),
        `largest["label"]` (the body's smallest flat voxel or block index, -1 when empty), `seeded["bodies"]` (how many bodies hold a
        seed), `quantiles` = {"n_bodies", "largest_volume", "seeded_volume"}, each (3, C) with the 10 / 50 / 90 % quantiles over
        the realisations, `probability_largest` / `probability_seeded` (C, yN, xN, zN) (or the block shape) = the fraction of
        realisations in which the voxel lies in that body, and with approximate `clipped_fraction`.  write=True: geobodies.csv in
        outpath."""
        from . import geobodies as gb
        s = self.settings
        q = self._cutoff_query("geobodies() labels realisations of the survey of cubing()", prop, cutoffs, offset, require, block, region, n, start)
        neighbours = gb.check_neighbours(neighbours)
        want_l, want_s = gb.check_probability(probability)
        grid = (s.yNcube, s.xNcube, s.zNcube)
        sd = gb.parse_seeds(seeds, grid, drill=self._drill_selection() if isinstance(seeds, str) and seeds == "drill" else None)
        if q.box is not None:
            sd = gb.seeds_to_blocks(sd, grid, q.box)
        min_voxels = int(min_voxels)
        if min_voxels < 1:
            raise ValueError("min_voxels >= 1, got %r" % (min_voxels,))
        eng = self.engine
        mask = self._on_device(q.mask)
        nel = int(np.prod(q.shape))
        hits_l = torch.zeros((q.t.size, nel), dtype=torch.int32, device=eng.device) if want_l else None
        hits_s = torch.zeros((q.t.size, nel), dtype=torch.int32, device=eng.device) if want_s else None
        stats, sums = [], []
        for fp, _, _ in self._posterior_batches(q.n, seed, q.start, approximate, batch):
            st, sm = eng.body_statistics(fp, q.p, q.t, lo=q.lo, mask=mask, box=q.box, neighbours=neighbours, min_count=min_voxels, seeds=sd,
                                         hits_largest=hits_l, hits_seeded=hits_s)
            stats.append(st)
            sums.append(sm)
        out = dict(cutoffs=q.cut.copy())
        out.update(gb.body_tables(torch.cat(stats).cpu().numpy()[:, q.inverse], torch.cat(sums).cpu().numpy()[:, q.inverse], q.scale[q.p], offset,
                                  self._voxel_volume()))
        for name, hits in (("probability_largest", hits_l), ("probability_seeded", hits_s)):
            if hits is not None:
                out[name] = self._probability(hits, q)
        if approximate:
            out["clipped_fraction"] = self._sampler_cache[1].clipped_fraction
        if write:
            import os
            gb.bodies_frame(out).to_csv(os.path.join(s.outpath, "geobodies.csv"), index=False)
        return out

    def label_bodies(self, cube, cutoff, neighbours=6, region=None):
        """Connected bodies of {cube >= cutoff} for any (yN, xN, zN) cube -- a mean cube, one realisation -- labelled on the device:
        (labels, sizes), labels (yN, xN, zN) int32 with the bodies numbered 1 .. B in ascending order of their smallest flat voxel
        index and 0 outside (the numbering of scipy.ndimage.label), sizes (B,) the voxels of each.  NaN is outside; region: a
        boolean cube restricting the voxels."""
        from . import geobodies as gb
        neighbours = gb.check_neighbours(neighbours)
        grid, F, cutoff, mask = self._cube_query(cube, cutoff, region)
        labels = torch.empty((1, 1, F.shape[2]), dtype=torch.int32, device=F.device)
        self.engine.body_statistics(F, 0, cutoff, mask=mask, neighbours=neighbours, labels=labels)
        numbered, sizes = gb.renumber(labels.cpu().numpy().reshape(grid))
        return numbered, sizes

    # ---- what grade_tonnage(), geobodies() and drill_intercepts() share -----------------------------------------------------------
    def _cutoff_query(self, what, prop, cutoffs, offset, require, block, region, n, start):
        """resources.cutoff_query for the survey of cubing(); `what` opens the sentence that asks for cubing() first."""
        from . import resources
        resources.property_index(prop)                            # (first, as before: a bad property is a ValueError even before cubing())
        if not hasattr(self, "Fs3") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("%s: call cubing() first" % what)
        s = self.settings
        return resources.cutoff_query(prop, cutoffs, offset, require, self._cube_scale, self.drillfield.size > 0, (s.yNcube, s.xNcube, s.zNcube),
                                      block, region, n, start)

    def _on_device(self, mask):
        """A host mask vector (or None) on the engine's device."""
        return None if mask is None else torch.as_tensor(mask, device=self.engine.device)

    def _voxel_volume(self):
        s = self.settings
        return float(s.xvoxsize) * float(s.yvoxsize) * float(s.zvoxsize)

    def _probability(self, hits, q):
        """(C, n) device counts over the q.n realisations -> the fractions in the caller's cutoff order, (C,) + q.shape."""
        return (hits.cpu().numpy().astype(np.float64) / q.n)[q.inverse].reshape((q.t.size,) + tuple(q.shape))

    def _cube_query(self, cube, cutoff, region):
        """One (yN, xN, zN) cube and one cutoff, for label_bodies() and column_intercepts(), as the engine's statistics take them:
        (grid, F (1, 3, N) device batch whose property 0 holds the cube, [cutoff], mask on the device or None), checked first."""
        from . import resources
        s = self.settings
        grid = (s.yNcube, s.xNcube, s.zNcube)
        cube = np.asarray(cube, dtype=np.float64)
        if cube.shape != grid:
            raise ValueError("cube must have the shape %r, got %r" % (grid, cube.shape))
        cutoff = float(cutoff)
        if np.isnan(cutoff):
            raise ValueError("the cutoff is NaN")
        mask = self._on_device(resources.region_mask(region, grid))
        F = torch.zeros((1, 3, cube.size), dtype=torch.float64, device=self.engine.device)
        F[0, 0] = torch.as_tensor(cube.reshape(-1).copy(), device=F.device)
        return grid, F, [cutoff], mask

    # ---- drill-intercept statistics ------------------------------------------------------------------------

    def drill_intercepts(self, cutoffs, prop="drill", n=256, seed=0, start=0, batch=64, offset=0.0, require=None, region=None,
                         min_length=None, max_gap=0.0, holes=None, paths=None, step=None, approximate=False, write=False):
        """What drill holes would intersect, from the n posterior realisations sample_posterior(n, seed, start) of the last cubing()
        survey, reduced on the device.  cutoffs, prop, n, seed, start, batch, offset, require, region and approximate are those of
        grade_tonnage(): the ORE of a realisation and a cutoff is the set that grade_tonnage() counts.  Along a hole, a run of
        non-ore samples no longer than max_gap that lies inside the region, holds no NaN and has ore immediately before and after it
        is composited in (internal dilution); the INTERCEPTS are the runs of the result and the BEST one is the longest (a tie goes
        to the shallower).  min_length and max_gap are metres down the hole and are converted to samples of the down-hole sample
        length -- zvoxsize for vertical holes, `step` for paths -- by min_len = ceil(min_length / sample length) and
        max_gap = floor(max_gap / sample length) (a quotient within 1e-9 of an integer counts as it); min_length=None is one sample.
        Default: every vertical column of the cube.  Returns a dict with the cutoffs in the caller's order:
          `cutoffs` (C,); per realisation, (n, C): `holes_hit` = the columns whose best intercept reaches min_length,
          `prospective_area` = holes_hit x xvoxsize x yvoxsize, `longest` = the longest intercept of any column (m), `count` = the ore
          samples of all columns (grade_tonnage()'s count), `quantiles` = {"prospective_area", "longest"}, each (3, C) at 10 / 50 /
          90 %; maps (C, yN, xN): `probability` (best intercept >= min_length), `probability_any` (any ore), `thickness` and
          `intercept_length` = dicts of `mean`, `p10`, `p50`, `p90` in metres (the quantiles are exact, by the inverted CDF of
          np.quantile(method="inverted_cdf"), from per-column histograms), `depth_to_top_mean` (m below the cube top, given
          presence; NaN where never present) and `accumulation_mean` = the mean of grade x metres, (scale x sum + offset x count) x
          sample length.
        holes = [(ix, iy), ...] (vertical holes at voxel columns) or paths = [(x0, y0, azimuth, dip), ...] (dipping holes in the
        convention of Acquisition.path_voxels, one sample per `step` at the ranges and with the length convention of predict_path(),
        steps inside one voxel repeating it): the same summaries per hole, (C, K) instead of (C, yN, xN), without the area, plus
        `per_realisation` = dict of (n, C, K) arrays: `thickness`, `depth_to_top`, `from`, `length` (m), `grade` = the mean value of
        the best intercept with its composited waste, `accumulation`, `n_intercepts`; and `trace_lengths` (K,) in samples.
        Always: `sample_length` (m) and the converted `min_len` and `max_gap_samples`.
        write=True: intercepts.csv and intercept_maps.csv (columns) or hole_intercepts.csv (holes, paths) in outpath.
        Block support, several ranks and a campaign utility built on these probabilities are out of scope."""
        from . import hip, intercepts as ic
        s = self.settings
        q = self._cutoff_query("drill_intercepts() reduces realisations of the survey of cubing()", prop, cutoffs, offset, require, None, region,
                               n, start)
        if holes is not None and paths is not None:
            raise ValueError("give holes or paths, not both")
        grid = q.shape
        eng = self.engine
        if eng.world > 1:
            raise NotImplementedError("drill intercepts run on one rank (world = %d)" % eng.world)
        mask = self._on_device(q.mask)
        dz, csr = float(s.zvoxsize), None
        if holes is not None:
            csr = ic.hole_traces(holes, grid)
        elif paths is not None:
            off, vox, dz = ic.path_traces(s, paths, step)
            csr = (off, vox)
        min_len, gap = ic.samples_of(min_length, max_gap, dz)
        traces = None if csr is None else hip.TraceSet(csr[0], csr[1], eng.N, device=eng.device)
        K, Lmax = (grid[0] * grid[1], grid[2]) if traces is None else (traces.K, traces.Lmax)
        maps = hip.trace_maps(q.t.size, K, Lmax, device=eng.device)
        tabs, dets, dsms = [], [], []
        for fp, _, _ in self._posterior_batches(q.n, seed, q.start, approximate, batch):
            r = eng.trace_statistics(fp, q.p, q.t, lo=q.lo, mask=mask, traces=traces, min_len=min_len, max_gap=gap, maps=maps,
                                     detail=traces is not None)
            if traces is None:
                tabs.append(r)
            else:
                tabs.append(r[0])
                dets.append(r[1].cpu())
                dsms.append(r[2].cpu())
        out = dict(cutoffs=q.cut.copy(), sample_length=dz, min_len=min_len, max_gap_samples=gap)
        out.update(ic.intercept_tables(torch.cat(tabs).cpu().numpy()[:, q.inverse], dz,
                                       float(s.xvoxsize) * float(s.yvoxsize) if traces is None else None))
        host = {k: v.cpu().numpy()[q.inverse] for k, v in maps.items()}
        summary = ic.intercept_maps(host, q.n, q.scale[q.p], offset, dz)
        if traces is None:
            shape = (q.t.size, grid[0], grid[1])
            summary = {k: ({name: a.reshape(shape) for name, a in v.items()} if isinstance(v, dict) else v.reshape(shape)) for k, v in summary.items()}
        out.update(summary)
        if traces is not None:
            out["per_realisation"] = ic.per_realisation(torch.cat(dets).numpy()[:, q.inverse], torch.cat(dsms).numpy()[:, q.inverse], q.scale[q.p],
                                                        offset, dz)
            out["trace_lengths"] = traces.lengths.copy()
        if approximate:
            out["clipped_fraction"] = self._sampler_cache[1].clipped_fraction
        if write:
            import os
            if traces is None:
                ic.curve_frame(out).to_csv(os.path.join(s.outpath, "intercepts.csv"), index=False)
                x = (np.arange(s.xNcube) + 0.5) * s.xvoxsize + s.xmin
                y = (np.arange(s.yNcube) + 0.5) * s.yvoxsize + s.ymin
                ic.map_frame(out, x, y).to_csv(os.path.join(s.outpath, "intercept_maps.csv"), index=False)
            else:
                ic.hole_frame(out).to_csv(os.path.join(s.outpath, "hole_intercepts.csv"), index=False)
        return out

    def column_intercepts(self, cube, cutoff, min_length=None, max_gap=0.0, region=None):
        """The deterministic companion of drill_intercepts() for any one (yN, xN, zN) cube -- a mean cube, one realisation -- on the
        device: per vertical column the material at or above `cutoff` (the cube's own units; NaN is outside, region a boolean cube
        restricting the voxels), min_length and max_gap in metres as there.  Returns a dict of (yN, xN) maps: `thickness` (m),
        `depth_to_top` (m below the cube top; NaN without ore), `from` and `length` of the best intercept (m; `from` NaN without
        one), `mean_value` = its mean with the composited waste (NaN without one), `n_intercepts` (of at least min_length)."""
        from . import intercepts as ic
        s = self.settings
        min_len, gap = ic.samples_of(min_length, max_gap, s.zvoxsize)
        grid, F, cutoff, mask = self._cube_query(cube, cutoff, region)
        _, det, dsm = self.engine.trace_statistics(F, 0, cutoff, mask=mask, min_len=min_len, max_gap=gap, detail=True)
        r = ic.per_realisation(det.cpu().numpy(), dsm.cpu().numpy(), 1.0, 0.0, s.zvoxsize)
        shape = (grid[0], grid[1])
        return {"thickness": r["thickness"].reshape(shape), "depth_to_top": r["depth_to_top"].reshape(shape), "from": r["from"].reshape(shape),
                "length": r["length"].reshape(shape), "mean_value": r["grade"].reshape(shape), "n_intercepts": r["n_intercepts"].reshape(shape)}

    # ---- drill-hole information gain and greedy campaigns ------------------------------------------------
    def _cubing_done(self, what):
        if not hasattr(self, "Fs3") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("%s scores holes against the posterior of cubing(): call cubing() first" % what)

    def _set_stats(self, sets, observed=None):
        """Engine set statistics of the current factor (normalised units), as host arrays."""
        lengths = create_cov_lengths(np.array(self.gp_length, dtype=float))
        r = self.engine.set_statistics(sets, self.settings.kernelfunc, [float(v) for v in lengths], self.coeffm, self.gp_amp, self.gp_sigma,
                                       observed=observed)
        return tuple(t.cpu().numpy() for t in r)

    def _ensure_factor(self):
        eng = self.engine
        want = _hyper_key(self.gp_amp, create_cov_lengths(np.array(self.gp_length, dtype=float)), self.coeffm)
        if getattr(self, "_step_params", None) != want or eng.last is None or tuple(eng.last["props"]) != (0, 1, 2):
            self._run(self.gp_amp, self.gp_length, None, False, False)

    # ---- cross-validation ----------------------------------------------------------------------------------
    CV_FOLDS = ("loo", "holes", "patches")

    def _cv_folds(self, folds, cell):
        """The fold list of a fold kind ("loo", "holes", "patches"), or the caller's own list of index arrays."""
        from . import crossval
        s = self.settings
        Ms = self.gravfield.size
        if not isinstance(folds, str):
            return folds
        if folds == "loo":
            out = crossval.loo_folds(self.Fs3.size)
        elif folds == "holes":
            out = crossval.hole_folds(self._sel, s.zNcube, Ms)
        else:
            cell = 2.0 * s.xvoxsize if cell is None else float(cell)
            out = crossval.patch_folds(np.asarray(self.sensor_locations, dtype=float)[:, :2], cell, Ms, sel=self._sel, nz=s.zNcube)
        dropped = self._engine.dropped_rows(self._sel) if self._engine is not None else np.zeros(0, dtype=np.int64)
        if dropped.size:
            # rows the committed row scales drop are in no fold; a fold that is left empty goes
            out = [f[~np.isin(f, dropped)] for f in (np.asarray(f, dtype=np.int64).reshape(-1) for f in out)]
            out = [f for f in out if f.size]
        return out

    def _check_cv_folds(self, folds):
        if isinstance(folds, str) and folds not in self.CV_FOLDS:
            raise ValueError("folds must be one of %s or a list of index arrays, got %r" % (self.CV_FOLDS, folds))

    def cross_validate(self, folds="loo", cell=None, write=False):
        """Leave-fold-out cross-validation of the fit, after cubing(): every data row is predicted from the rows outside its fold,
        from the factor the step left on the device (no refactorisation; one step without mean and variance when the hyper-parameters
        changed since).  folds: "loo" (one row each), "holes" (the drill rows of one voxel column together, sensors alone), "patches"
        (sensors in square cells of side `cell` metres, default two x-voxels, binned by their coordinates; drill rows by hole) or a
        list of disjoint index arrays into the data vector [grav | magn | drill], at most 128 rows each.  `cell` matters for "patches"
        alone and is ignored otherwise.
        Returns a dict: `grav`, `magn`, `drill` with `observed`, `predicted`, `residual`, `std`, `fit_residual` in the data units of
        that type (deviations from the data mean, as cubing()'s cubes), `z` = residual / std and `fold` (-1: row in no fold);
        `fit_residual`: the in-sample misfit y - A3 mu = D alpha of every row, normalised units; `folds`: `logp` (log predictive
        density of the fold), `mahalanobis`, `size`, `status` (0, or 1 + the pivot at which the fold's block failed); `summary`:
        `logp` (total) and per data type `mean_z2` and `mean_mahalanobis` (mean of mahalanobis / size over the folds that lie in that
        type), both about 1 for a calibrated model.  write=True: crossval_grav.csv, crossval_magn.csv, crossval_drill.csv in outpath."""
        self._check_cv_folds(folds)
        if not hasattr(self, "Fs3") or not hasattr(self, "_cube_scale"):
            raise RuntimeError("cross_validate() predicts the survey of cubing(): call cubing() first")
        eng = self.engine
        want = _hyper_key(self.gp_amp, create_cov_lengths(np.array(self.gp_length, dtype=float)), self.coeffm)
        if getattr(self, "_step_params", None) != want or eng.last is None:
            self._run(self.gp_amp, self.gp_length, None, False, False)
        r = {k: v.cpu().numpy() for k, v in eng.cross_validate(self._cv_folds(folds, cell)).items()}
        ng, nm, Mu = self.gravfield.size, self.magfield.size, self.Fs3.size
        fit = self._row_sigma() ** 2 * r["alpha"]
        out = dict(fit_residual=fit, folds={k: r[k] for k in ("logp", "mahalanobis", "size", "status")})
        summary = dict(logp=float(np.sum(r["logp"])))
        # the type of a fold: that of all its rows (a fold over several types counts for none)
        first = np.full(r["size"].size, Mu, dtype=np.int64)
        lastr = np.full(r["size"].size, -1, dtype=np.int64)
        rows = np.flatnonzero(r["fold_of_row"] >= 0)
        np.minimum.at(first, r["fold_of_row"][rows], rows)
        np.maximum.at(lastr, r["fold_of_row"][rows], rows)
        with np.errstate(all="ignore"):
            for i, (name, a, b) in enumerate((("grav", 0, ng), ("magn", ng, ng + nm), ("drill", ng + nm, Mu))):
                sc = self._cube_scale[i]
                obs, res, std = self.Fs3[a:b] * sc, r["resid"][a:b] * sc, np.sqrt(r["var"][a:b]) * sc
                out[name] = dict(observed=obs, predicted=obs - res, residual=res, std=std, z=res / std, fold=r["fold_of_row"][a:b],
                                 fit_residual=fit[a:b] * sc)
                inside = (first >= a) & (lastr < b) & (lastr >= 0)
                z = out[name]["z"]
                summary[name] = dict(mean_z2=float(np.nanmean(z ** 2)) if np.isfinite(z).any() else float("nan"),
                                     mean_mahalanobis=float(np.mean(r["mahalanobis"][inside] / r["size"][inside])) if inside.any() else float("nan"))
        out["summary"] = summary
        if write:
            self._write_crossval(out)
        return out

    def _write_crossval(self, out):
        """crossval_<type>.csv in outpath: sensor positions as passed to cubing() (voxel centres and DEPTH for the drill rows)."""
        import os

        import pandas as pd
        s = self.settings
        loc = np.asarray(self.sensor_locations, dtype=float)
        for name in ("grav", "magn", "drill"):
            o = out[name]
            cols = dict(OBSERVED=o["observed"], PREDICTED=o["predicted"], STD=o["std"], Z=o["z"], FOLD=o["fold"])
            if name == "drill":
                pos = dict(EASTING=self.voxelpos[0][self._sel], NORTHING=self.voxelpos[1][self._sel], DEPTH=self.voxelpos[2][self._sel])
            else:
                pos = dict(EASTING=loc[:, 0], NORTHING=loc[:, 1])
            pd.DataFrame({**pos, **cols}).to_csv(os.path.join(s.outpath, "crossval_%s.csv" % name), index=False)

    def calc_cv(self, params, folds="holes"):
        """Minus the total log predictive density of the folds (see cross_validate) for hyper-parameters (amplitude, lengthscale, 3
        correlation coefficients): calc_logl's signature and parameter handling, an objective for the derivative-free optimisers.  One
        step without mean and variance, then the folds; inf where the factorisation of the step fails (as calc_logl: with matern32 this
        5-parameter form puts two equal lengths into the cross term, so it is inf there for every params) and where a fold's block
        does not factorise.  Errors of the folds themselves (a hole of more than 128 voxels, a multi-rank engine) are raised.
        "patches" has no `cell` here: two x-voxels."""
        self._check_cv_folds(folds)
        s = self.settings
        gp_amp = params[0]
        gp_length = params[1] * np.asarray([s.xvoxsize, s.xvoxsize, s.xvoxsize])
        coeffm = params[2:]
        from . import crossval
        table = crossval.fold_table(self._cv_folds(folds, None), self.Fs3.size)
        try:
            self._run(gp_amp, gp_length, coeffm, False, False)
        except (CholeskyError, FactorisationTimeout):
            return np.inf
        total = float(self.engine.cross_validate(table)["logp"].sum())
        return -total if np.isfinite(total) else np.inf

    def hole_statistics(self, paths=None):
        """Posterior statistics of the drill property along holes, after cubing():
            info_gain = 1/2 log det(I + Sigma_PP / sigma_d^2)  (nats, scale-free),  path_std = sqrt(1^T Sigma_PP 1),  sum_var = trace Sigma_PP
        (the last two in cubing()'s drill units).  paths=None: (yN, xN) tables of every vertical hole (NaN on the rim); else a list of
        Acquisition.path_voxels triplets (dipping holes: the unique voxels of each path), one value per path (NaN for a path that
        leaves the cube).  Returns dict(info_gain, path_std, sum_var, status)."""
        from . import campaign
        self._cubing_done("hole_statistics()")
        s = self.settings
        self._ensure_factor()
        ds = float(self._cube_scale[2])
        if paths is None:
            sets, ij = campaign.vertical_sets(s.yNcube, s.xNcube, s.zNcube)
            ig, pv, sv, st = self._set_stats(sets)
            tab = lambda v: campaign.column_table(v, ij, s.yNcube, s.xNcube)
            st_t = np.full((s.yNcube, s.xNcube), -1, dtype=np.int64)
            st_t[ij[:, 0], ij[:, 1]] = st
            return dict(info_gain=tab(ig), path_std=tab(np.sqrt(pv) * ds), sum_var=tab(sv * ds ** 2), status=st_t)
        sets, valid = campaign.path_sets(paths, (s.yNcube, s.xNcube, s.zNcube))
        out = dict(info_gain=np.full(len(valid), np.nan), path_std=np.full(len(valid), np.nan), sum_var=np.full(len(valid), np.nan),
                   status=np.full(len(valid), -1, dtype=np.int64))
        if valid.any():
            ig, pv, sv, st = self._set_stats(sets[valid])
            out["info_gain"][valid], out["path_std"][valid], out["sum_var"][valid], out["status"][valid] = ig, np.sqrt(pv) * ds, sv * ds ** 2, st
        return out

    # ---- block-support statistics ---------------------------------------------------------------------------
    def block_statistics(self, block, write=False):
        """Posterior mean and 3 x 3 covariance of the three properties' averages over the boxes of a block model, after cubing():
        block = (bx, by, bz) voxels in the x, y, z order of the settings; the boxes tile the cube from its origin and are partial at the
        far edges.  The factor of the current hyper-parameters is reused, or rebuilt (without the mean and variance) when the last
        step used others.  Returns a dict of arrays in the cubes' (y, x, z) order and cubing()'s data units: `mean` (3, yB, xB, zB) the
        box means of the mean cubes, `cov` (yB, xB, zB, 3, 3) the covariance of the three block means, `std` (3, yB, xB, zB) the roots
        of its diagonal (NaN where an entry is negative), `corr` (yB, xB, zB, 3, 3), `count` (yB, xB, zB) voxels per block, `centre`
        (yB, xB, zB, 3) x, y, z of the block centres.  The entries are raw: the reference's matern32 prior is not positive semidefinite,
        so a block's matrix may be slightly indefinite and a correlation may pass 1 by a fraction of a percent; nothing is clipped.
        Drill entries are NaN without drill data, as cubing()'s.  write=True: block_model.csv in outpath."""
        from . import blocksupport
        s = self.settings
        bx, by, bz = blocksupport.check_box(block, (s.xNcube, s.yNcube, s.zNcube))
        self._cubing_done("block_statistics()")
        grid, box = (s.yNcube, s.xNcube, s.zNcube), (by, bx, bz)
        self._ensure_factor()
        lengths = create_cov_lengths(np.array(self.gp_length, dtype=float))
        cov, _ = self.engine.block_covariance(box, s.kernelfunc, [float(v) for v in lengths], self.coeffm, self.gp_amp)
        cov = cov.cpu().numpy()
        index, count = blocksupport.block_partition(grid, box)
        nb = blocksupport.block_counts(grid, box)
        box_mean = lambda v: np.bincount(index, weights=np.asarray(v, dtype=np.float64).reshape(-1), minlength=count.size) / count
        cs = self._cube_scale                               # (products in the survey's dtype, as cubing() squares them)
        scale, scale2 = np.array([float(v) for v in cs]), np.array([[float(a * b) for b in cs] for a in cs])
        with np.errstate(all="ignore"):
            mean = np.stack([box_mean(self.mu_rec.reshape(3, -1)[i] * self._cube_scale[i]) for i in range(3)])
            var = np.einsum("baa->ba", cov)
            std_n = np.sqrt(np.where(var >= 0, var, np.nan))
            corr = cov / np.sqrt(var[:, :, None] * var[:, None, :])
            cov = cov * scale2
            corr = np.where(np.isnan(cov), np.nan, corr)    # (NaN drill entries without drill data)
            std = (std_n * scale[None, :]).T
        out = dict(mean=mean.reshape((3,) + nb), cov=cov.reshape(nb + (3, 3)), std=std.reshape((3,) + nb), corr=corr.reshape(nb + (3, 3)),
                   count=count.reshape(nb), centre=np.stack([box_mean(self.voxelpos[i]) for i in range(3)], axis=-1).reshape(nb + (3,)))
        if write:
            self._write_block_model(out)
        return out

    def _write_block_model(self, out):
        """block_model.csv in outpath: one row per block."""
        import os

        import pandas as pd
        names = ("DENSITY", "MAGSUS", "DRILL")
        cols = dict(EASTING=out["centre"][..., 0], NORTHING=out["centre"][..., 1], DEPTH=out["centre"][..., 2], COUNT=out["count"])
        cols.update({"MEAN_" + n: out["mean"][i] for i, n in enumerate(names)})
        cols.update({"STD_" + n: out["std"][i] for i, n in enumerate(names)})
        cols.update({"CORR_%s_%s" % (names[a], names[b]): out["corr"][..., a, b] for a, b in ((0, 1), (0, 2), (1, 2))})
        pd.DataFrame({k: np.asarray(v).reshape(-1) for k, v in cols.items()}).to_csv(
            os.path.join(self.settings.outpath, "block_model.csv"), index=False)

    # ---- prediction at arbitrary points ---------------------------------------------------------------------
    def to_covariance_frame(self, points):
        """(Q, 3) points x, y, z in the cube's own coordinates (those of voxelpos) -> (3, Q) in the covariance frame, the frame of
        calcGridPoints3D: a voxel centre lands on its grid point (i + 1) * voxel size."""
        s = self.settings
        p = np.asarray(points, dtype=np.float64)
        return np.stack([p[:, 0] + s.xvoxsize / 2., p[:, 1] + s.yvoxsize / 2., (s.zmax - p[:, 2]) + s.zvoxsize / 2.])

    def _check_points(self, points):
        """`points` as a (Q, 3) float64 array inside the closed box of the cube; ValueError otherwise (naming the first offender)."""
        s = self.settings
        try:
            p = np.array(points, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("points must be a (Q, 3) array of x, y, z") from None
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError("points must be a (Q, 3) array of x, y, z with Q >= 1, got shape %r" % (p.shape,))
        lo = np.array([0., 0., s.zmax - s.zLcube])
        hi = np.array([s.xLcube, s.yLcube, s.zmax])
        bad = ~((p >= lo) & (p <= hi)).all(axis=1)              # (a NaN coordinate is outside too)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError("point %d = (%r, %r, %r) lies outside the cube [0, %r] x [0, %r] x [%r, %r]: no extrapolation"
                             % (i, p[i, 0], p[i, 1], p[i, 2], hi[0], hi[1], lo[2], hi[2]))
        return p

    def predict_points(self, points, full_cov=False, batch=4096):
        """Posterior of the three properties at arbitrary points inside the cube, after cubing(): `points` (Q, 3) x, y, z in the cube's
        own coordinates (those of voxelpos), inside the closed box [0, xLcube] x [0, yLcube] x [zmax - zLcube, zmax].  The factor of the
        current hyper-parameters is reused, or rebuilt when the last step used others.  Returns a dict in cubing()'s data units: `mean`
        (3, Q), `var` (3, Q), `std` (3, Q; NaN where var < 0) and with full_cov `cov` (3Q, 3Q), ordered [property][point].  The values
        are raw (the reference's matern32 prior is slightly indefinite); drill entries are NaN without drill data, as cubing()'s."""
        self._cubing_done("predict_points()")
        p = self._check_points(points)
        self._ensure_factor()
        eng = self.engine
        from . import hip
        q = tuple(hip.to_dev(np.ascontiguousarray(c), eng.device) for c in self.to_covariance_frame(p))
        lengths = create_cov_lengths(np.array(self.gp_length, dtype=float))
        r = eng.predict_points(q, self.settings.kernelfunc, [float(v) for v in lengths], self.coeffm, self.gp_amp, full_cov=full_cov,
                               batch=batch)
        Q = p.shape[0]
        cs = self._cube_scale                               # (products in the survey's dtype, as cubing() squares them)
        with np.errstate(all="ignore"):
            mean = r[0].cpu().numpy() * np.array([float(v) for v in cs])[:, None]
            var = r[1].cpu().numpy() * np.array([float(v * v) for v in cs])[:, None]
            out = dict(mean=mean, var=var, std=np.sqrt(np.where(var >= 0, var, np.nan)))
            if full_cov:
                scale2 = np.array([[float(a * b) for b in cs] for a in cs])
                out["cov"] = r[2].cpu().numpy() * np.repeat(np.repeat(scale2, Q, axis=0), Q, axis=1)
        return out

    def path_points(self, x0, y0, azimuth, dip, step=None, length=None):
        """Points and ranges of a hole collared at (x0, y0, zmax) with azimuth / dip in degrees (the convention of
        Acquisition.path_voxels): ranges step/2, 3 step/2, ... up to `length`, cut where the path first leaves the cube's box.
        step defaults to half the smallest voxel edge, length to zLcube.  Returns ((n, 3) points, (n,) ranges)."""
        from .acquisition import spherical2cartes
        s = self.settings
        step = 0.5 * min(s.xvoxsize, s.yvoxsize, s.zvoxsize) if step is None else float(step)
        length = float(s.zLcube) if length is None else float(length)
        if not (step > 0 and np.isfinite(step) and length > 0 and np.isfinite(length)):
            raise ValueError("step and length must be positive, got %r and %r" % (step, length))
        n = int(np.floor(length / step + 0.5 + 1e-12))          # ranges (k + 1/2) step <= length
        rng = (np.arange(n) + 0.5) * step
        x, y, z = spherical2cartes(float(x0), float(y0), float(s.zmax), np.deg2rad(azimuth), np.deg2rad(180. - dip), rng)
        pts = np.stack([x, y, z], axis=1) if n else np.empty((0, 3))
        lo = np.array([0., 0., s.zmax - s.zLcube])
        hi = np.array([s.xLcube, s.yLcube, s.zmax])
        inside = ((pts >= lo) & (pts <= hi)).all(axis=1)
        keep = n if inside.all() else int(np.argmin(inside))    # cut at the first point outside
        return pts[:keep], rng[:keep]

    def predict_path(self, x0, y0, azimuth, dip, step=None, length=None):
        """The prognosis log of a planned hole, after cubing(): the posterior at the points of path_points().  Returns dict(points
        (n, 3), range (n,), mean (3, n), std (3, n), path_mean (3,) the average of each property along the hole, path_mean_std (3,)
        = sqrt(1^T Sigma_aa 1) / n from the joint covariance of the points -- the uncertainty of the hole's average, which the
        pointwise stds cannot give; NaN where that sum is negative).  ValueError when no point lies inside the cube."""
        self._cubing_done("predict_path()")
        pts, rng = self.path_points(x0, y0, azimuth, dip, step, length)
        n = pts.shape[0]
        if n == 0:
            raise ValueError("the path from (%r, %r) with azimuth %r and dip %r has no point inside the cube" % (x0, y0, azimuth, dip))
        r = self.predict_points(pts, full_cov=True)
        with np.errstate(all="ignore"):
            tot = np.array([r["cov"][a * n:(a + 1) * n, a * n:(a + 1) * n].sum() for a in range(3)])
            pstd = np.sqrt(np.where(tot >= 0, tot, np.nan)) / n
        return dict(points=pts, range=rng, mean=r["mean"], std=r["std"], path_mean=r["mean"].mean(axis=1), path_mean_std=pstd)

    def _write_points_prediction(self, points, out, fname="points_prediction.csv"):
        """points_prediction.csv in outpath: one row per point."""
        import os

        import pandas as pd
        names = ("DENSITY", "MAGSUS", "DRILL")
        cols = dict(X=points[:, 0], Y=points[:, 1], Z=points[:, 2])
        cols.update({"MEAN_" + n: out["mean"][i] for i, n in enumerate(names)})
        cols.update({"STD_" + n: out["std"][i] for i, n in enumerate(names)})
        pd.DataFrame(cols).to_csv(os.path.join(self.settings.outpath, fname), index=False)

    def propose_drill_campaign(self, q, utility="information", costs=None, write=False, update="refactor"):
        """A greedy batch of q distinct vertical holes ("kriging believer"): pick the best inner hole by `utility` ("information",
        "ucb", "ucb_path"; see geobo_amd.campaign), add its voxels that carry no drill row yet as drill rows whose values are the
        posterior mean (which leaves the mean unchanged), refactor without the mean and variance, score again without the chosen holes.
        The statistics leave out voxels that already carry a drill row (they would not be measured again); the mean and cost sums run
        over the whole hole, as the reference's.  Returns a DataFrame (NORTHING, EASTING at voxel centres, RANK, UTILITY, INFO_GAIN,
        PATH_STD) and sets `campaign_info` (chosen voxel sets, the three variance cubes after all q holes in cubing()'s units, and the
        mean cubes of that step).  The Inversion is left as cubing() left it; the engine's factor is rebuilt from the real data.
        update="append": the same campaign without a step per pick -- the hole Grams of one sweep stay on the device, every pick's rows
        are appended to the factor at the posterior mean (PosteriorEngine.append_drill_rows; u_P = 0, the mean keeps its bits) and
        only their rows of V_d are added to the Grams; at the end the rows are dropped again (truncate_drill_rows) in place of the
        restoring step.  DESIGN.md section 20."""
        import os

        import pandas as pd
        from . import campaign
        self._cubing_done("propose_drill_campaign()")
        if utility not in campaign.UTILITIES:
            raise ValueError("utility must be one of %s, got %r" % (campaign.UTILITIES, utility))
        if update not in ("refactor", "append"):
            raise ValueError("update must be 'refactor' or 'append', got %r" % (update,))
        s = self.settings
        ny, nx, nz = s.yNcube, s.xNcube, s.zNcube
        N = nx * ny * nz
        q = int(q)
        if not 0 <= q <= (ny - 2) * (nx - 2):
            raise ValueError("q must be between 0 and the %d inner vertical holes" % ((ny - 2) * (nx - 2)))
        sets, ij = campaign.vertical_sets(ny, nx, nz)
        ds = float(self._cube_scale[2])
        scale = self._cube_scale
        zsum = lambda a: np.ascontiguousarray(a).sum(axis=2)[ij[:, 0], ij[:, 1]]
        drill_rec = self.mu_rec[2 * N:3 * N].reshape(ny, nx, nz) * scale[2]
        cost = np.zeros((ny, nx, nz)) if costs is None else np.asarray(costs, dtype=float).reshape(ny, nx, nz)
        mean_sum, cost_sum = zsum(drill_rec), zsum(cost)
        mu_d = np.asarray(self.mu_rec[2 * N:3 * N], dtype=np.float64)          # normalised posterior mean of the drill block
        ng, nm = self.gravfield.size, self.magfield.size
        y_g, y_m = self.Fs3[:ng], self.Fs3[ng:ng + nm]
        values = np.zeros(N)
        values[self._sel] = self.Fs3[ng + nm:]
        sel = np.asarray(self._sel, dtype=np.int64).copy()
        lengths = [float(v) for v in create_cov_lengths(np.array(self.gp_length, dtype=float))]
        eng = self.engine
        A_g, A_m = self._operators()

        def step(sel, want_mean_var):
            return eng.posterior(A_g, A_m, sel, y_g, y_m, values[sel], lengths, self.coeffm, s.kernelfunc, self.gp_sigma, gp_amp=self.gp_amp,
                                 props=(0, 1, 2), calclogl=False, want_mean_var=want_mean_var)
        picks, rows = [], []
        append = update == "append"
        if append:
            self._ensure_factor()
            if not eng.mean_var_known():
                self._run(self.gp_amp, self.gp_length, None, False, True)      # (a factor rebuilt without the mean: the appends carry it)
            params, Md0 = self._step_params, eng.last["step"].Md
            grams = eng.set_grams(sets, s.kernelfunc, lengths, self.coeffm, self.gp_amp, self.gp_sigma)
            r = dict(mu=np.asarray(self.mu_rec), var=np.asarray(np.diag(self.cov_rec)))
        try:
            self._step_params = None            # from here on the factor holds fantasised rows
            for rank in range(q):
                observed = np.zeros(N, dtype=bool)
                observed[sel] = True
                if append:
                    ig, pv, sv, st = (t.cpu().numpy() for t in eng.set_logdet_from(grams, observed=observed))
                else:
                    step(sel, False)
                    ig, pv, sv, st = (t.cpu().numpy() for t in eng.set_statistics(sets, s.kernelfunc, lengths, self.coeffm, self.gp_amp,
                                                                                     self.gp_sigma, observed=observed))
                u = campaign.utility(utility, mean_sum, cost_sum, s.kappa, s.beta, info_gain=ig, path_var=pv * ds ** 2, sum_var=sv * ds ** 2)
                u = np.where(np.isfinite(u), u, -np.inf)
                u[picks] = -np.inf
                c = int(np.argmax(u))
                if not np.isfinite(u[c]):
                    raise RuntimeError("no hole left to score (statistics status %s)" % np.unique(st))
                picks.append(c)
                rows.append((ij[c, 0], ij[c, 1], rank + 1, float(u[c]), float(ig[c]), float(np.sqrt(pv[c])) * ds))
                new = sets[c][~observed[sets[c]]]
                values[new] = mu_d[new]
                sel = np.union1d(sel, new)
                if append and new.size:
                    r = eng.append_drill_rows(new, None, want_mean_var=True, tile_hook=grams["add_rows"])
            if not append:
                r = step(sel, True)
            shape = (3, ny, nx, nz)
            with np.errstate(all="ignore"):
                var = [r["var"].reshape(shape)[i] * scale[i] ** 2 for i in range(3)]
                mean = [r["mu"].reshape(shape)[i] * scale[i] for i in range(3)]
            self.campaign_info = dict(sets=[sets[c].copy() for c in picks], holes=ij[picks].copy(), selection=sel.copy(), var=var, mean=mean,
                                      utility=utility)
        finally:
            # the engine's factor back to the real survey (sample_posterior must never condition on fantasised rows)
            if append:
                eng.truncate_drill_rows(Md0)
                self._step_params = params
            else:
                self._run(self.gp_amp, self.gp_length, None, False, False)
        table = pd.DataFrame(rows, columns=["I0", "I1", "RANK", "UTILITY", "INFO_GAIN", "PATH_STD"])
        table.insert(0, "NORTHING", table.pop("I0") * s.yvoxsize + s.ymin + 0.5 * s.yvoxsize)
        table.insert(1, "EASTING", table.pop("I1") * s.xvoxsize + s.xmin + 0.5 * s.xvoxsize)
        if write:
            table.to_csv(os.path.join(s.outpath, "newdrill_campaign_vertical.csv"), index=False)
        return table
