"""Matrix-free posterior engine on MI355X: the device pipeline behind `Inversion.predict3/cubing`.

Reference path replaced (file:line in the reference checkout):
    kernels.py:158-195 create_cov  +  inversion.py:92-117 predict3  (K, A K A^T + S, Cholesky, V, mu, diag cov)
    sensormodel.py:29-93 A_sens    (forward operators, built on the device)

Algorithm (same results as the reference, never holding an N x N object):
    1. AK[s-rows, j-cols] = A_s K_sj             spectral route on the regular grid (spectral.py: radix-2 real transforms over x, z,
                                                 Toeplitz blocks over y); fused fp64-MFMA contraction with the K tile generated in the
                                                 kernel for everything else
       AK[d-rows, j-cols] = K_2j[sel, :]         gather from the block's lattice table (k_block_grid) / k_block from coordinates
    2. AkA = AK A3^T + diag(sigma^2)             lattice Gram on a lattice survey (lattice_gram.py), else MFMA GEMM-NT
    3. L = chol(AkA), Linv = L^-1, u = Linv y    blocked Cholesky on MFMA tiles, wavefront-shuffle TRMV
    4. mu = AK^T (Linv^T u),  var = amp - colsum(V^2),  V = (Linv A3) K      transposed posterior (_posterior_zpath; round 3): rows of
                                                 Linv A3 through the kernels of step 1, squared and summed on the way out; V never stored
       or, where that path does not apply (grids without the radix-2 / Toeplitz-y kernels, padded sensor rows, fp32 assembly, dense method):
       mu = (Linv AK)^T u, var = amp - colsum((Linv AK)^2)                    MFMA GEMM fused with the column reductions

HBM layout (all fp64, row-major, zero padded -- include/geobo_hip.h "PADDING CONTRACT"):
    x,y,z      3 x N_pad                 voxel coordinates (SoA), N_pad = pad128(N)
    A_g, A_m   Ms_pad x N_pad            forward operators, Ms_pad = pad256(nx*ny)
    AK         M_pad x (P_c * nc)        nc = this rank's voxel columns; rows: [grav | mag | drill | pad]
    AkA/L      M_pad x M_pad             M_pad = pad256(2*Ms_pad + M_d); padding rows carry identity
    Linv       M_pad x M_pad

Which family a step runs in -- "single" (one rank, fused n = 64 kernels, transposed.py), "rows" (sharded by sensor rows over world >= 1
ranks, chunked, any grid of the spectral route: rowform.py) or "columns" (voxel-column shards, fused reduction, row exchange from 4
ranks: this file + columnform.py) -- is decided by plan.plan_route (pure, CPU-tested) and confirmed when the operators are built
(lattice survey, even stencils).  Multi-GPU: one process per GPU, torch.distributed / RCCL; row form: one all-gather of AkA row blocks +
one all-reduce of the partial sums of squares; column form: all-reduce of the partial AkA or all-to-all of A K block columns, mu / var
slices by one all-gather.  DESIGN.md sections 2 and 7.
"""
import math
import os
import time

import numpy as np
import torch

from . import geometry, hip
from .plan import (COLUMN_FORM_MAX_BYTES, cross_options, cross_rows_route, engine_options, feed_options, gram_gx_route, grav_mirror_route,
                   grav_options, plan_route)
from .columnform import ColumnExchangeMixin
from .rowform import RowFormMixin
from .operators import StreamedOperator
from .transposed import TransposedPosteriorMixin
from .information import SetStatisticsMixin
from .crossval import CrossValidationMixin
from .blocksupport import BlockSupportMixin
from .pointpred import PointPredictionMixin
from .resources import ResourceMixin
from .geobodies import GeobodyMixin
from .intercepts import InterceptMixin
from .append import AppendRowsMixin
from .reweight import ReweightMixin
from .step import Prior, Step
from .sharding import (EmulatedGroup, allreduce_sum_, assemble_columns, backend_of, exchange_blocks, exchange_blocks_finish,
                       exchange_blocks_start, gather_rows, gather_slices, shard_columns)

F64 = hip.F64


class _GramFeed:
    """What the spectral product hands the lattice Gram per batch and property block (spectral.SpectralProduct._store): the rows'
    x analysis GX goes through the Gram's y step, scaling and channel sum at once; the scaled spectra S[block] wait for the
    back-transform in _assemble_AkA_sym."""

    def __init__(self, gram, lams, S, store_all=True):
        self.gram, self.lams, self.S, self.store_all = gram, lams, S, store_all
        self.ld = gram.Py * gram.Px

    def rows(self, jj, r0, R, GX):
        self.gram.gx_rows(GX, R, self.lams[jj], self.S[jj][r0 * self.ld:])

    def at(self, r0):
        """The same hand-over for a product that starts at row r0 of the block."""
        return _GramFeed(self.gram, self.lams, [S[r0 * self.ld:] for S in self.S], self.store_all)


class CholeskyError(RuntimeError):
    """AkA not positive definite (first bad pivot in .info, 1-based like LAPACK dpotrf)."""

    def __init__(self, info):
        super().__init__("Cholesky failed at pivot %d" % info)
        self.info = info


class FactorisationTimeout(RuntimeError):
    """The persistent tile-DAG factorisation gave up on a hand-off (info = -7: a spin ran into its 4 s wall-clock bound -- a device
    shared with other processes can do that); the result is undefined.  Inversion retries the step once on the stream schedule."""


class _LastStep(dict):
    """engine.last.  `complete` (set by a mirrored step and by a step whose A K product fed the lattice Gram and stored only the
    boundary planes of its rows): writes what the step left unwritten of A K -- the storing product first, then the mirrored row copy;
    run on the first read of the buffer ("AK_partial"), never inside the step."""
    complete = None

    @staticmethod
    def chain(fills):
        """The completion hook that runs `fills` in order (None for none)."""
        fills = list(fills)
        return (lambda: [f() for f in fills] and None) if fills else None

    def __getitem__(self, key):
        if key == "AK_partial" and self.complete is not None:
            fill, self.complete = self.complete, None
            fill()
        return dict.__getitem__(self, key)


def create_cov_lengths(gplength):
    """kernels.py:174-180 -- create_cov edits the caller's length array IN PLACE: [l,l,l] -> [l,1.02l,l]."""
    p = np.asarray(gplength)
    if p[1] == p[0]:
        p[1] = 1.01 * p[0]
    if p[2] == p[0]:
        p[1] = 1.02 * p[0]
    if p[2] == p[1]:
        p[2] = 1.01 * p[1]
    return p


def weight_matrix(crossweights):
    """kernels.py:166-169,181 -- w1: 0<->2, w2: 1<->2, w3: 0<->1."""
    w1, w2, w3 = [float(v) for v in np.asarray(crossweights)]
    return [[1.0, w3, w1], [w3, 1.0, w2], [w1, w2, 1.0]]


# weight -> the block pair it multiplies (weight_matrix): w1 on (0, 2), w2 on (1, 2), w3 on (0, 1)
WEIGHT_PAIRS = ((0, 2), (1, 2), (0, 1))

_XGROUPS = {}


def _exchange_group(ranks, backend):
    """One extra communicator per rank tuple for the whole process (engines come and go; an RCCL communicator per engine would leak)."""
    key = (ranks, backend)
    if key not in _XGROUPS:
        _XGROUPS[key] = torch.distributed.new_group(ranks=list(ranks), backend=backend)
    return _XGROUPS[key]


def lattice_gram_form(exchange, chunked, world, Ms, c0, c1, plane, N):
    """Which form of the lattice Gram (AkA on a lattice survey) a rank can use -- pure shard arithmetic, tested on the CPU:
      "rows"     row exchange with rank-sized send buffers (>= 4 ranks, fp64, resident operators): before the all-to-all a rank holds
                 ALL voxels of its own Ms/world sensor rows, correlates those itself and AkA arrives as row blocks (all-gather);
      "columns"  every rank correlates its own y-slab of the A K rows (partial block columns add up in the all-reduce of AkA); the x
                 step and the back-transform are not divided, so from ~5 ranks the N/G-deep GEMM is cheaper; needs whole y-slabs in
                 multiples of 16;
      None       AkA by the N/G-deep GEMM.
    The CHUNKED exchange of the large-cube modes (fp32 assembly / streamed operators) keeps no full rows: it falls under the
    column rules (round-2 advisory: it used to get eigen-data under the row rule and then died in gram_rows' Ly % 16 assertion,
    e.g. 64^3 on 8 ranks with assembly="f32")."""
    if exchange and not chunked:
        return "rows" if (Ms // world) % 128 == 0 else None
    Ly = (c1 - c0) // plane
    if world > 4 or (c1 - c0) % plane or Ly % 16 or c1 > N or Ly <= 0:
        return None
    return "columns"


def _on_device(fn):
    """Entry points run with the engine's device current: every launch takes torch's current stream, and the C-ABI is
    handed raw pointers -- an engine on cuda:1 driven while cuda:0 is current would launch on the wrong device."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kw):
        with torch.cuda.device(self.device):
            return fn(self, *args, **kw)
    return wrapper


class PosteriorEngine(RowFormMixin, TransposedPosteriorMixin, ColumnExchangeMixin, SetStatisticsMixin, CrossValidationMixin, BlockSupportMixin,
                      PointPredictionMixin, ResourceMixin, GeobodyMixin, InterceptMixin, AppendRowsMixin, ReweightMixin):
    def __init__(self, settings, device=None, rank=0, world=1, group=None, profile=False, method="auto", assembly="f64",
                 operators="resident"):
        """assembly "f32": covariance tables rounded through fp32 and A K kept in fp32 in HBM (BASELINE config 5, "fp32 kernel
        assembly + fp64 Cholesky"); every contraction still accumulates in fp64 on fp64 panels converted on the fly.
        operators "streamed": A_g / A_m are generated in row batches / column slabs when needed instead of being resident."""
        hip.require_gpu()
        if assembly not in ("f64", "f32") or operators not in ("resident", "streamed", "auto"):
            raise ValueError("assembly must be 'f64' or 'f32', operators 'resident', 'streamed' or 'auto'")
        self.f32 = assembly == "f32"
        self.streamed = operators == "streamed"
        # "auto": streamed where that costs nothing -- a lattice survey on one device, whose transform reads the operator rows as
        # windows of the stencil table and whose AkA comes from the lattice Gram (no operator is ever materialised) -- else resident
        self.auto_ops = operators == "auto"
        self.s = settings
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError("PosteriorEngine needs a CUDA (ROCm) device, got %r" % (device,))
        if self.device.index is None:
            self.device = torch.device("cuda:%d" % torch.cuda.current_device())
        self.rank, self.world, self.group = rank, world, group
        self.profile = profile
        self.timings = {}
        s = settings
        self.nx, self.ny, self.nz = int(s.xNcube), int(s.yNcube), int(s.zNcube)
        self.N = self.nx * self.ny * self.nz
        self.N_pad = hip.pad_n(self.N)
        self.Ms = self.nx * self.ny
        self.Ms_pad = hip.pad_m(self.Ms)
        self.c0, self.c1 = shard_columns(self.N_pad, world, rank)
        self.nc = self.c1 - self.c0
        self._xyz = None
        self._A = {}
        self._ws = {}   # persistent device workspaces keyed by name (re-used across calls: no per-step allocation)
        self._host = {}  # pinned host staging buffers of the result read-back, keyed by slot
        self._auto_denied = set()       # operators="auto": (func, B) whose stencil turned out not to be even -> resident
        self._pending_exchange = None   # (A K, [(recv, work)], props) of a row exchange that has been started but not placed yet
        self.use_grid = self.nz >= 16 and self.nz % 2 == 0  # lattice-table generator (geobo_ak_fused_grid); coordinates otherwise
        # spectral (real-DFT) product: regular grid with extents % 16 == 0, unpadded voxel columns, shards on y-slab boundaries
        if method not in ("auto", "dense", "spectral"):
            raise ValueError("method must be 'auto', 'dense' or 'spectral'")
        self.method = method
        # every shape / rank-count / precision decision of a step comes from ONE pure function (plan.py, CPU-tested table); the
        # GEOBO_* switches are overrides into it.  What a step then actually ran is recorded in self.step_route.
        # The options the planner does not own (plan.ENGINE_OPTIONS) are resolved from the same mapping, here and nowhere else.
        env = os.environ
        self.route = plan_route(self.nx, self.ny, self.nz, world=world, rank=rank, assembly=assembly, operators=operators, method=method,
                                env=env)
        self.options = engine_options(env)
        self.feed = feed_options(env)       # (plan.FEED_OPTIONS: the A K product feeds the lattice Gram, _gram_feed)
        self.cross = cross_options(env)     # (plan.CROSS_OPTIONS: which rows give AkA's cross block, plan.cross_rows_route)
        self.grav = grav_options(env)       # (plan.GRAV_OPTIONS: AkA's gravity block from half its rows, plan.grav_mirror_route)
        self.use_spectral = self.route.spectral
        if method == "spectral" and not self.use_spectral:
            raise ValueError("spectral method needs grid extents % 16 == 0 and column shards on y-slab boundaries")
        if self.route.operators == "streamed":
            self.streamed = True            # (residency cannot fit: the planner's note says so)
        if self.route.note and self.N >= 32768:
            import warnings
            warnings.warn("geobo_amd route %s: %s" % (self.route.describe(), self.route.note), RuntimeWarning, stacklevel=3)
        self._spectral = None
        self._lattice_plan = None
        self._gram, self._lam, self._edgeV = None, {}, {}
        self._lamW, self._edgeVt = {}, {}     # transposed lattice application: permuted eigen-data, boundary-slab spectra
        # Mirrored magnetic block of AkA ("point mirror"): GEOBO_AKA_MIRROR=0 switches it off.  aka_mirror[func]: what the last
        # operator build measured and what the last step did with it -- dict(deviation, bound, symmetric, taken); _mirror: (operator, symmetric)
        self.aka_mirror_on = self.options.aka_mirror
        self.aka_mirror, self._mirror, self._mirror_meas = {}, {}, None
        # Rows of L^-1 A enter the posterior's covariance product as spectra, Z is never stored (transposed._posterior_zpath; DESIGN.md
        # section 2 item 4): GEOBO_Z_SPECTRUM=0 restores the stored rows
        self.z_spectrum_on = self.options.z_spectrum
        # Row form (plan.Route.family "rows", rowform.py): statically possible; whether a step takes it is decided when the operators
        # are built (lattice survey, even stencils).  Column form from 4 ranks: row-sharded transforms + one all-to-all of A K block
        # columns per operator (with 2 ranks the exchange would move a quarter of A K over ONE xGMI link, more than the forward passes
        # it saves: replicated forward passes + slab-cropped backward passes there).
        self.rows_static = self.route.rows
        self.exchange = self.route.exchange
        self._deny = {}                 # row form denied: "survey" -> (survey key, why), func -> ((survey key, B), why)
        self.step_route = None          # family the last step ran in: "rows" | "single" | "columns"
        self._step = None               # the Step of the last posterior() (step.py); self.last["step"] once it has completed
        self.last = None                # what the last completed posterior() left on the device
        if self.streamed and not self.use_spectral:
            raise ValueError("streamed operators feed the spectral product: needs the spectral method's grid conditions")
        # Communicator of the row exchange.  Default: the caller's own group -- collectives of one communicator run in issue order on
        # its stream, so the asynchronous all-to-all still overlaps with this rank's COMPUTE (second operator's transforms, row Gram)
        # and only the all-gather of the AkA row blocks queues up behind it; nothing about that can deadlock.
        # GEOBO_EXCHANGE_COMM=own gives the exchange a second communicator so that the all-gather overtakes it (the all-to-all then
        # also runs under the factorisation).  Two communicators with collectives in flight on one device are deadlock-prone unless
        # every rank issues them in the same order (they do) -- but that mode has never run on RCCL hardware (no multi-GPU box was
        # available to the builder), so it is opt-in.  GEOBO_ASYNC_EXCHANGE=0: blocking exchange on the caller's group.
        # (own: torch.distributed.new_group is a collective over the DEFAULT group -- every rank must build its engine at the same
        # point; the communicator is cached per rank tuple and shared by all engines of the process.)
        self._xgroup = group
        self.async_exchange = self.options.async_exchange
        if (self.exchange and self.options.exchange_comm == "own" and self.async_exchange
                and not isinstance(group, EmulatedGroup) and torch.distributed.is_available() and torch.distributed.is_initialized()):
            ranks = torch.distributed.get_process_group_ranks(group) if group is not None else list(range(torch.distributed.get_world_size()))
            if len(ranks) == world:
                self._xgroup = _exchange_group(tuple(ranks), torch.distributed.get_backend(group))
        self._Arows, self._Aedge, self._rowsrc, self._op_args = {}, {}, {}, {}
        self._slab_ops = set()      # data pointers of operators that hold only this rank's column slab
        self._potrf_ctx = None
        # one-rank runs issue no collective; bench.py --gpus 1 --check and the RCCL test set this so that the row form's all-gather,
        # all-reduce and agreement go through the backend with one rank (sharding._live)
        self.force_collectives = self.options.force_collectives
        self.kernel_events = None  # set to [] to record (name, flops, start, stop) HIP events per fused launch
        self.aka_hook = None       # callable(AkA) run between the assembly of AkA and its factorisation (emulation tool only)

    # ---- geometry --------------------------------------------------------------------------------------------
    def grid_points(self):
        """calcGridPoints3D((xN,yN,zN),(xvox,yvox,zvox)) as called at inversion.py:216 -> padded SoA on device."""
        if self._xyz is None:
            s = self.s
            xr = np.arange(1, self.nx + 1) * s.xvoxsize
            yr = np.arange(1, self.ny + 1) * s.yvoxsize
            zr = np.arange(1, self.nz + 1) * s.zvoxsize
            X, Y, Z = np.meshgrid(xr, yr, zr)
            out = []
            for a in (X, Y, Z):
                v = np.empty(self.N_pad)
                v[:self.N] = a.ravel()
                v[self.N:] = v[self.N - 1]
                out.append(hip.to_dev(v, self.device))
            self._xyz = tuple(out)
        return self._xyz

    def node_axes(self):
        """1-D node coordinates behind inversion.py:58-66 (Edges = meshgrid(xedge, yedge, zedge), z negated)."""
        return geometry.node_axes(self.s)

    # ---- forward operators -----------------------------------------------------------------------------------
    @_on_device
    def operator(self, func, sensor_locations, B=None, axes=None, full=False):
        """A_sens on the device: (Ms_pad x N_pad) zero padded tensor (sensormodel.py:29-93).
        In the row-sharded multi-GPU form (self.exchange) only what this rank needs is built unless `full`: the voxel
        columns of its y-slab for every sensor (AkA operand) and all voxels for its own sensor rows (transform input)."""
        s = self.s
        loc = np.ascontiguousarray(sensor_locations, dtype=np.float64)
        assert loc.shape == (self.Ms, 3), "A_sens handles exactly xNcube*yNcube sensors (sensormodel.py:54,58)"
        xe, ye, ze = self.node_axes() if axes is None else axes
        # survey on the cube's own x-y lattice (the reference's workflow): translation-invariant stencil, ~2000x fewer potentials
        # (the lattice analysis is always attempted; a survey off the lattice gets plan = None)
        skey = (loc.tobytes(), xe.tobytes(), ye.tobytes(), ze.tobytes())
        if self._lattice_plan is None or self._lattice_plan[0] != skey:
            self._lattice_plan = (skey, hip.lattice_plan(loc, xe, ye, ze, self.nx, self.ny, self.nz, self.device))
        plan = self._lattice_plan[1]
        # row form (rowform.py): this rank's sensor rows + the two boundary slabs of every sensor, nothing sharded by voxel columns.
        # Needs a row-major lattice survey and even stencils; a denial holds for exactly the survey / field it was found for.
        Bkey = None if B is None else tuple(np.asarray(B, dtype=float))
        if self._deny.get("survey", (skey,))[0] != skey:
            self._allow_rows("survey")
        if self._deny.get(func, ((skey, Bkey),))[0] != (skey, Bkey):
            self._allow_rows(func)
        if self.rows_static and not self._rows_denied and not full and (plan is None or not plan["rowmajor"]):
            self._deny_rows("survey", skey, "the survey is not a row-major x-y lattice of the cube")
        rows_mode = self.rows_static and not self._rows_denied and not full
        self._op_args[func] = (sensor_locations, B, axes)
        partial = self.exchange and not full and not rows_mode
        dkey = (func, Bkey, None if plan is None else self._lattice_plan[0])      # a stencil's evenness belongs to (field, survey geometry)
        stream_it = (self.streamed or (self.auto_ops and dkey not in self._auto_denied and self._implicit_operators_pay(plan))) and not full
        if rows_mode and self.auto_ops and not stream_it and self.world == 1 and not self.route.single:
            stream_it = True      # "auto" in the row form on one rank: rows are generated a transform batch at a time (a_sens on the lattice is a copy)
        key = (func, loc.tobytes(), Bkey, partial, stream_it, rows_mode)
        if key in self._A:
            return self._A[key]
        self._mirror.pop(func, None)        # (measured below where the mirrored block can apply: _mirror_static)
        self.aka_mirror.pop(func, None)
        rows_r = self.Ms // self.world if rows_mode else 0
        if rows_mode and not stream_it and self.world > 1:
            A = self._workspace2d("Arows_" + func, rows_r, self.N_pad)        # the handle of a row-form operator IS its row shard
        elif partial and not stream_it:
            # row-exchange form: only this rank's y-slab of every sensor row is ever read (AkA operand of the N/G-deep GEMM):
            # a compact (Ms_pad x nc) buffer, columns c0 .. c1 (the kernels address columns absolutely: col_origin)
            A = self._workspace2d("Aslab_" + func, self.Ms_pad, self.nc)
            if self.Ms_pad > self.Ms:
                A[self.Ms:].zero_()
            self._slab_ops.add(A.data_ptr())
        elif not stream_it:
            A = self._workspace2d("A_" + func, self.Ms_pad, self.N_pad)
            if self.Ms_pad > self.Ms:
                A[self.Ms:].zero_()
            if self.N_pad > self.N:
                A[:, self.N:].zero_()
        if func == "grav":
            Bv = np.zeros(3) if B is None else np.asarray(B, dtype=float)
            mul, div = s.c_MILLIGALS_UNITS, s.fcor_grav
        else:
            Bv = s.magneticField if B is None else np.asarray(B, dtype=float)
            mul, div = 1.0, s.fcor_mag
        locd, xed, yed, zed = (hip.to_dev(v, self.device) for v in (loc, xe, ye, ze))
        lws = None
        if plan is not None:
            lws = self._workspace("a_sens_lattice_ws", (hip.a_sens_lattice_ws_doubles(self.nx, self.ny, self.nz),))
        plane = self.nx * self.nz

        def boundary_slabs():
            """(Ms_pad x 2 nx nz): the two 1e6-padded boundary slabs of the operator for every sensor (their part of the Gram and of
            L^-1 A goes through the slabs' x-DFT spectra)."""
            E2 = self._workspace2d("Aedge_" + func, self.Ms_pad, 2 * plane)
            if self.Ms_pad > self.Ms:
                E2[self.Ms:].zero_()
            for k, iy in enumerate((0, self.ny - 1)):
                hip.a_sens(func, Bv, locd, self.nx, self.ny, self.nz, xed, yed, zed, mul, div, E2[:, k * plane:(k + 1) * plane], iy, iy + 1,
                           plan=plan, ws=lws, col_origin=iy * plane)
            return E2[:, :plane], E2[:, plane:2 * plane]
        if stream_it:
            A = StreamedOperator(self, func, Bv, mul, div, locd, (xed, yed, zed), plan, lws)
            lam = None
            if plan is not None:
                # one two-sensor call leaves the stencil table Q in the lattice workspace (the Gram's eigen-data come from it)
                tmp = self._workspace2d("op_rows2", 2, self.N_pad)
                self._timed("a_sens_" + func, 0.0, lambda: A.rows_into(tmp, 0, 2))
                feed = self.use_spectral and self._spectral_product().forms.lattice_feed and not self.f32
                mirror = None
                if feed and self._mirror_static(plan):
                    # the boundary slabs enter the mirror measurement, which shares the evenness check's host read: kept first
                    self._timed("a_sens_" + func, 0.0, lambda: A.keep_stencil(func))
                    mirror = (A.lattice.Q.view(2 * self.ny - 3, 2 * self.nx - 1, self.nz), A.edge[:, :plane], A.edge[:, plane:2 * plane])
                lam = self._gram_eigen(plan, lws, rows=rows_mode, mirror=mirror)
                self._mirror_record(func, A, mirror)
                if lam is None and rows_mode:
                    self._deny_rows(func, (skey, Bkey), "the %s stencil is not even in both lattice offsets" % func)
                    return self.operator(func, sensor_locations, B=B, axes=axes, full=full)
                if lam is None and not self.streamed:
                    # "auto" and the stencil is not even (no lattice Gram): AkA is an N-deep GEMM against the operator -- resident
                    self._auto_denied.add(dkey)
                    return self.operator(func, sensor_locations, B=B, axes=axes, full=full)
                if feed and A.lattice is None:
                    self._timed("a_sens_" + func, 0.0, lambda: A.keep_stencil(func))
            self._lam[func] = None if lam is None else (A, lam)
            if rows_mode:
                if A.lattice is not None:
                    self._rowsrc[func] = ("lattice", A.lattice, 0)
                    self._Aedge[func] = (A.edge[:, :plane], A.edge[:, plane:2 * plane])
                else:
                    self._rowsrc[func] = ("streamed", A, 0)
                    self._Aedge[func] = self._timed("a_sens_" + func, 0.0, boundary_slabs)
        elif rows_mode:
            g0 = self.rank * rows_r

            def build():
                if self.N_pad > self.N:
                    A[:, self.N:].zero_()
                if self.world > 1:
                    hip.a_sens(func, Bv, locd[g0:g0 + rows_r].contiguous(), self.nx, self.ny, self.nz, xed, yed, zed, mul, div, A, plan=plan,
                               rows=slice(g0, g0 + rows_r), ws=lws)
                    return boundary_slabs()
                hip.a_sens(func, Bv, locd, self.nx, self.ny, self.nz, xed, yed, zed, mul, div, A, plan=plan, ws=lws)
                return A[:, :plane], A[:, (self.ny - 1) * plane:self.ny * plane]     # (one rank: the slabs are columns of the operator itself)
            edges = self._timed("a_sens_" + func, 0.0, build)
            lam = self._gram_eigen(plan, lws, rows=True)
            if lam is None:
                self._deny_rows(func, (skey, Bkey), "the %s stencil is not even in both lattice offsets" % func)
                return self.operator(func, sensor_locations, B=B, axes=axes, full=full)
            self._lam[func] = (A, lam)
            self._rowsrc[func] = ("tensor", A, g0)
            self._Aedge[func] = edges
            if self.world > 1:
                self._Arows[func] = A
        elif partial:
            rows_r = self.Ms // self.world
            Ar = self._workspace2d("Arows_" + func, rows_r, self.N_pad)
            loc_r = locd[self.rank * rows_r:(self.rank + 1) * rows_r].contiguous()

            def build():
                hip.a_sens(func, Bv, locd, self.nx, self.ny, self.nz, xed, yed, zed, mul, div, A, self.c0 // plane, self.c1 // plane,
                           plan=plan, ws=lws, col_origin=self.c0)
                hip.a_sens(func, Bv, loc_r, self.nx, self.ny, self.nz, xed, yed, zed, mul, div, Ar, plan=plan,
                           rows=slice(self.rank * rows_r, (self.rank + 1) * rows_r), ws=lws)
            self._timed("a_sens_" + func, 0.0, build)
            self._Arows[func] = Ar
            lam = self._gram_eigen(plan, lws) if plan is not None else None
            self._lam[func] = None if lam is None else (A, lam)
            if lam is not None:
                # row-sharded lattice Gram: the two 1e6-padded boundary slabs of the operator, every sensor (their part of AkA is a GEMM)
                self._Aedge[func] = boundary_slabs()
        else:
            self._timed("a_sens_" + func, 0.0, lambda: hip.a_sens(func, Bv, locd, self.nx, self.ny, self.nz, xed, yed, zed, mul, div, A,
                                                                 plan=plan, ws=lws))
            mirror = None
            if self._mirror_static(plan):
                mirror = (hip.a_sens_lattice_stencil(lws, self.nx, self.ny, self.nz), A[:, :plane], A[:, (self.ny - 1) * plane:self.ny * plane])
            lam = self._gram_eigen(plan, lws, mirror=mirror) if plan is not None else None
            self._mirror_record(func, A, mirror)
            self._lam[func] = None if lam is None else (A, lam)      # valid for exactly this operator tensor
        self._A = {k: v for k, v in self._A.items() if k[0] != func}  # one operator per type stays resident
        self._edgeV = {k: v for k, v in self._edgeV.items() if k[0] != func}   # (spectra of the previous operator's boundary slabs)
        self._edgeVt = {k: v for k, v in self._edgeVt.items() if k[0] != func}
        self._lamW = {k: v for k, v in self._lamW.items() if k[0] != func}
        self._A[key] = A
        return A

    @property
    def _rows_denied(self):
        return bool(self._deny)

    def _deny_rows(self, what, key, why):
        """The row form is impossible for this survey / field: operator builds and steps take the column form (with the all-to-all only
        where it pays without the row posterior: from 4 ranks) until an operator build with another survey / field lifts the denial.
        Operators already built for the row form are dropped (posterior() rebuilds them from the recorded arguments)."""
        if self.route.rows_mandatory:
            # (round-4 advisory) the column form's A K does not fit this device: say so instead of running into the allocator
            raise RuntimeError("the row form is the only one that fits this grid (a materialised A K would take %.0f GB per rank) and it "
                               "cannot run here: %s" % (self.route.ak_bytes / 1e9, why))
        self._deny[what] = (key, why)
        self.exchange = self.route.exchange_without_rows
        self._A = {k: v for k, v in self._A.items() if not k[5]}
        self._rowsrc, self._Aedge = {}, {}

    def _allow_rows(self, what):
        if self._deny.pop(what, None) is not None and not self._deny:
            self.exchange = self.route.exchange

    def _implicit_operators_pay(self, plan):
        """operators="auto": True when neither the transforms nor AkA need a materialised operator."""
        if plan is None or self.world != 1 or self.f32 or not self.use_spectral or not plan["rowmajor"]:
            return False
        if not self.route.opt("aka_lattice"):
            return False
        from .lattice_gram import LatticeGram
        if not LatticeGram.supported(self.nx, self.ny, self.nz) or self.Ms_pad != self.Ms:
            return False
        return self._spectral_product().forms.lattice_feed

    def _spectral_product(self):
        """The grid's SpectralProduct, its per-kernel timer following the engine's kernel_events switch."""
        from .spectral import SpectralProduct
        if self._spectral is None:
            self._spectral = SpectralProduct(self.nx, self.ny, self.nz, self.device, forms=self.route.forms)
        self._spectral.kernel_timer = None if self.kernel_events is None else (
            lambda name, by, fn, valu=0.0, flop=0.0: self._timed(name, flop, fn, alg=by, valu=valu))
        return self._spectral

    def _timed(self, name, flops, fn, alg=0.0, valu=0.0):
        """Run fn(); when kernel_events is a list, bracket it with HIP events on the launch stream (torch's current one).
        flops = executed flop (padded compute extents), alg = algorithmic flop of SURVEY.md 8(d) for the same work (unpadded),
        valu = the part of `flops` that runs on the fp64 VALU instead of the matrix pipe."""
        if self.kernel_events is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        self.kernel_events.append((name, float(flops), float(alg), float(valu), e0, e1))
        return r

    def _workspace(self, name, shape, dtype=F64):
        """Persistent uninitialised device tensor; reallocated only when the shape changes (large hipMallocs are slow)."""
        t = self._ws.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            self._ws.pop(name, None)
            t = self._ws[name] = torch.empty(shape, dtype=dtype, device=self.device)
        return t

    def _to_host(self, t, slot=0):
        """Device vector -> host array through a persistent PINNED staging buffer (valid until the next call with the same slot).
        A pageable device-to-host copy pins its destination on the fly; on a busy host that now and then took 20-30 ms for the
        4 MB of a result vector (one 64^3 step in five came out 4 % slow)."""
        h = self._to_host_async(t, slot)
        torch.cuda.current_stream(self.device).synchronize()
        return h

    def _to_host_async(self, t, slot=0):
        """Queue the copy of _to_host without waiting for it: the returned array is valid after the caller's next synchronize of the
        current stream (one wait for all the read-backs of a step: status word, likelihood statistics, mean and variance)."""
        n = t.numel()
        buf = self._host.get(slot)
        if buf is None or buf.numel() < n or buf.dtype != t.dtype:
            buf = self._host[slot] = torch.empty(max(n, 1), dtype=t.dtype, pin_memory=True)
        buf[:n].copy_(t.detach().reshape(-1), non_blocking=True)
        return buf[:n].numpy()

    def _workspace2d(self, name, rows, cols, pad=16, dtype=F64):
        """(rows x cols) view of a persistent buffer whose leading dimension is cols + pad.  Power-of-two row strides
        (4 MiB for AK at 64^3) alias rows onto the same cache sets / channels and cost the GEMMs ~12 %; 128 bytes of
        padding per row remove it (profiles/r01_row_stride.txt)."""
        return self._workspace(name, (rows, cols + pad), dtype)[:, :cols]

    def _panel64(self, name, src, rows=None, cols=None):
        """fp64 view of a block of A K for the MFMA kernels: the block itself when A K is kept in fp64, else a conversion into a
        persistent scratch panel of capacity rows x cols (12 B of HBM traffic per element -- small beside the M-deep
        contraction that consumes it)."""
        if src.dtype == F64:
            return src
        buf = self._workspace2d(name, src.shape[0] if rows is None else rows, src.shape[1] if cols is None else cols)
        view = buf[:src.shape[0], :src.shape[1]]
        hip.convert(src, view)
        return view

    def _op_rows_buffer(self):
        """Row-batch buffer of the streamed operators: one size for every user (no reallocation between stages)."""
        return self._workspace2d("op_rows", max(256, self._spectral_product().R), self.N_pad)

    def _cov_table(self, kid, lj, ls, w, amp):
        """Lattice table of one covariance block; rounded through fp32 in the fp32-assembly mode."""
        sset = self.s
        tab = hip.cov_table(kid, self.nx, self.ny, self.nz, sset.xvoxsize, sset.yvoxsize, sset.zvoxsize, lj, ls, w, amp, self.device)
        return hip.round_f32_(tab) if self.f32 else tab

    @_on_device
    def apply_operator(self, A, v):
        """A @ v for a resident or streamed forward operator (the synthetic surveys of bench.py: data = A rho); v: (N,) host or
        device vector, returns the (Ms,) device vector.  Streamed operators are generated 256 rows at a time."""
        vd = v if isinstance(v, torch.Tensor) else hip.to_dev(np.asarray(v, dtype=np.float64).reshape(-1), self.device)
        if vd.numel() % 2 or vd.data_ptr() % 16:      # (geobo_rowgemv reads 16-byte pairs)
            vd = torch.cat([vd.reshape(-1), vd.new_zeros(2 - vd.numel() % 2)])
        n2 = self.N + self.N % 2                       # (an odd voxel count meets the zero column of the padding)
        if not isinstance(A, StreamedOperator):
            return hip.rowgemv(A[:self.Ms, :n2], vd)
        buf = self._op_rows_buffer()
        out = torch.empty(self.Ms, dtype=F64, device=self.device)
        for r0 in range(0, self.Ms, 256):
            R = min(256, self.Ms - r0)
            hip.rowgemv(A.rows_into(buf, r0, R)[:, :n2], vd, out=out[r0:r0 + R])
        return out

    def clear_operators(self):
        """Drop the resident forward operators (the benchmark rebuilds them inside every timed step)."""
        self._A = {}
        self._lam, self._mirror = {}, {}
        self._edgeV, self._edgeVt, self._lamW = {}, {}, {}
        self._rowsrc, self._Aedge, self._Arows = {}, {}, {}
        self._lattice_plan = None     # host analysis of the survey geometry + its device copies: part of the operator build

    def release(self):
        """Give the device memory back (workspaces, transform buffers, operators, eigen-data); the engine rebuilds what the next
        step needs.  bench.py --check: the ranks free their share before rank 0 runs the 1-rank comparison on the same device."""
        self.clear_operators()
        self._ws, self._spectral, self._gram = {}, None, None
        self._xyz = None
        self.last = None
        if self._step is not None:       # (which form the step took stays readable: _rowpath)
            self._step.gens, self._step.fullrows = {}, {}
        torch.cuda.empty_cache()

    # ---- stages ------------------------------------------------------------------------------------------------
    def _tick(self, name, t0=None):
        if not self.profile:
            return None
        torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        if t0 is not None:
            self.timings[name] = self.timings.get(name, 0.0) + (now - t0)
        return now

    @property
    def _rowpath(self):
        """The last posterior() step ran (or, after a failure, was going to run) the row-sharded form."""
        return self._step is not None and self._step.rowpath

    def _new_step(self, prior, props, sel_t, noise, **kw):
        """A Step over the drill voxels sel_t (int64 device tensor or None); kw: the remaining fields of step.Step."""
        Md = 0 if sel_t is None else sel_t.numel()
        step = Step(prior, tuple(props), sel_t, Md, hip.pad_m(2 * self.Ms_pad + Md), noise, **kw)
        if "row_scale" not in kw and self._row_scale_active():
            # committed row scales (reweight.py) of a step that was not handed them: a derivative Gram of logl_grad
            step.row_scale = self._step_row_scale(np.zeros(0, dtype=np.int64) if sel_t is None else sel_t.cpu().numpy())
        return step

    def _assemble_AK(self, step, A_g, A_m):
        """A K into the workspace step.ak_slot, or None in the row form (decided here: step.rowpath), which has no A K.
        step.sym (posterior() sets it when the step will run in the transposed order on a lattice survey): only the blocks AkA's
        LOWER triangle needs -- (grav rows, blocks 0 and 1), (magn rows, block 1), the drill rows; AkA[magn rows, grav columns] is the
        transpose of AkA[grav rows, magn columns], and nothing but AkA reads A K in that order (_mean_rows, _posterior_zpath)."""
        xyz = self.grid_points()
        props, sel_t, Md, M_pad = step.props, step.sel_t, step.Md, step.M_pad
        off_d = 2 * self.Ms_pad
        nc = self.nc
        step.rowpath = False
        if self.rows_static:
            self._spectral_product()
            if self._rows_agree(self._rows_ok(A_g, A_m)):
                # row form: no column shard of A K exists (and none is allocated) -- AkA comes straight from chunks of the rank's rows
                self._finish_exchange()  # (an exchange left over by a call that failed between its start and its factorisation)
                step.rowpath = True
                step.fullrows = {}
                return None
        # what THIS step would materialise (its own property count and element size; the planner's figure is for two blocks)
        ak_bytes = M_pad * len(props) * nc * (4 if self.f32 else 8)
        if ak_bytes > COLUMN_FORM_MAX_BYTES and self.use_spectral:
            raise RuntimeError("A K of this grid would take %.0f GB on this rank and only the row form avoids it (%s)"
                               % (ak_bytes / 1e9, self.route.note or "GEOBO_ROWS=0 / GEOBO_POSTERIOR=dense switch it off"))
        AK = self._workspace2d(step.ak_slot, M_pad, len(props) * nc, dtype=hip.F32 if self.f32 else F64)
        # every sensor/drill row is overwritten below; only the padding must be defined: rows behind each row block
        # (zero, so that AkA / V get zero rows) and voxel columns >= N of the last shard (finite: they meet zero A columns)
        for r0, r1 in ((self.Ms, self.Ms_pad), (self.Ms_pad + self.Ms, off_d), (off_d + Md, M_pad)):
            if r1 > r0:
                AK[r0:r1].zero_()
        if self.c1 > self.N:
            for jj in range(len(props)):
                AK[:, jj * nc + max(self.N - self.c0, 0):(jj + 1) * nc].zero_()
        if self.use_spectral:
            self._assemble_AK_spectral(step, AK, A_g, A_m)
        for jj, j in enumerate(props):
            cols = slice(jj * nc, (jj + 1) * nc)
            for s_, A in ((0, A_g), (1, A_m)):
                if self.use_spectral:
                    break
                # block (row-block s, col-block j) of create_cov is w * k2(l_j, l_s)  (kernels.py:183-195)
                out = AK[s_ * self.Ms_pad:(s_ + 1) * self.Ms_pad, cols]
                out64 = out if not self.f32 else self._workspace2d("ak_block64", self.Ms_pad, nc)
                if self.use_grid:
                    # regular grid: covariance = table on the index-difference lattice (built once per block, N doubles)
                    tab = step.prior.table(self, s_, j)
                    self._timed("ak_fused_grid", 2.0 * self.Ms_pad * self.N_pad * nc,
                                lambda: hip.ak_fused_grid(A, self.nx, self.ny, self.nz, tab, self.c0, nc, out64),
                                alg=2.0 * self.Ms * self.N * min(nc, max(self.N - self.c0, 0)))
                else:
                    self._timed("ak_fused", 2.0 * self.Ms_pad * self.N_pad * nc,
                                lambda: step.prior.ak_fused(self, s_, j, A, xyz, nc, out64),
                                alg=2.0 * self.Ms * self.N * min(nc, max(self.N - self.c0, 0)))
                if self.f32:
                    hip.convert(out64, out)
            if Md:
                self._cov_rows(step.prior, 2, j, sel_t, self.c0, AK[off_d:off_d + Md, cols])
        return AK

    def _cov_rows(self, prior, i, j, rows_t, col0, out):
        """out[r, c] = block (i, j) of the prior (create_cov, kernels.py:183-195: w_ij k2(l_j, l_i)) for the row voxels rows_t (flat indices,
        int64 device tensor) and the voxel columns col0 .. col0 + out.shape[1]: materialised covariance assembly.  On the regular
        grid a gather from the block's difference-lattice table (geobo_k_block_grid: bound by the HBM store), otherwise evaluated
        from coordinates (geobo_k_block)."""
        ncv = min(out.shape[1], max(self.N - col0, 0))       # columns behind N are voxel padding (zeroed by the caller)
        if ncv <= 0:
            return out
        if self.use_grid and col0 % 2 == 0:
            tab = prior.table(self, i, j)
            return hip.k_block_grid(tab, self.nx, self.ny, self.nz, rows_t, col0, out[:, :ncv])
        xyz = self.grid_points()
        rows = tuple(c[rows_t] for c in xyz)
        colc = tuple(c[col0:col0 + out.shape[1]] for c in xyz)
        return prior.k_block(self, i, j, rows, colc, out)

    def _assemble_AK_spectral(self, step, AK, A_g, A_m):
        """Sensor rows of AK through the real-DFT route (geobo_amd/spectral.py): same product, ~200x fewer flops."""
        sp, nc, props = self._spectral_product(), self.nc, step.props
        plane = self.nx * self.nz
        y0, y1 = self.c0 // plane, self.c1 // plane
        if self.exchange:
            return self._assemble_AK_spectral_exchange(step, AK)
        # the symmetric plan: the blocks the buffer keeps for its readers (engine.last["AK_partial"]), and the blocks the step runs -- the
        # same, or with AkA's cross block from the magnetic rows (step.cross_rows): A_m K_10 on the step.mirror rows the
        # magnetic block runs anyway in place of A_g K_01 on every gravity row
        kept = ((0, 0), (0, 1), (1, 1))
        run = ((0, 0), (1, 0), (1, 1)) if step.cross_rows == "magn" else kept
        for s_, A in ((0, A_g), (1, A_m)):
            gen_of, out_of = {}, {}
            for jj, j in enumerate(props):
                gen_of[j] = sp.eigenvalues(step.prior.table(self, s_, j))
                step.gens[(s_, j)] = gen_of[j]          # (the transposed posterior path applies the same blocks to L^-1 A_s)
                out_of[j] = AK[s_ * self.Ms_pad:s_ * self.Ms_pad + self.Ms, jj * nc:(jj + 1) * nc]
            blocks = [j for j in props if not step.sym or (s_, j) in run]
            lams, outs = [gen_of[j] for j in blocks], [out_of[j] for j in blocks]
            # lattice survey, fp64 assembly: the y stage reads the rows as windows of the pool of distinct operator-plane spectra, built
            # here once per operator and step (spectral.plane_pool) -- no forward transform per row
            pooled = (isinstance(A, StreamedOperator) and A.lattice is not None and A.lattice.jy is not None and not self.f32
                      and sp.pool_applies())
            # mirrored magnetic block (step.mirror): only the rows whose AkA rows are computed; the others are never written
            Mrun = step.mirror if (s_ == 1 and step.mirror) else self.Ms
            # gravity block from half its rows (step.grav_mirror): the interior part A_i of the first rows runs -- their windows
            # of the pool between two zero planes; resident rows: copies with the two planes zeroed --, the boundary slabs of every row are
            # still transformed (the slab-slab term)
            half = bool(s_ == 0 and step.grav_mirror)
            if half:
                Mrun = step.grav_mirror
            fl = sp.flops(Mrun, len(lams), y1 - y0, fwd_planes=sp.pool_planes(self.Ms if half else Mrun) if pooled else None)
            fv = sp.flops_valu(Mrun, len(lams), y1 - y0)
            feed = self._gram_feed(step, s_, blocks) if (y0, y1) == (0, self.ny) else None
            assert not half or ((pooled or not isinstance(A, StreamedOperator)) and feed is not None and not feed.store_all and blocks == [0])      # (the gate: _grav_mirror_rows)
            if feed is not None:
                fl += self._gram.flops_gx(Mrun * len(lams))

            def product_rows(gx, A=A, lams=lams, outs=outs, Mrun=Mrun, pooled=pooled, half=half):
                """The block's rows of A K (arguments bound now: the completion hook calls this after the step).  gx: the hand-over.
                half: the interior part of the rows only; planes 0 and ny-1 of the boundary part's product go to step.grav_slabs."""
                slabs_to = lambda: self._workspace2d("grav_slabs", self.Ms + 1, 2 * plane)[:self.Ms]      # (a row of slack: edge_rows)

                def keep_planes():
                    # planes 0 and ny-1 of the rows of A_i K the product just stored, compact and apart from the A K buffer: the
                    # completion hook overwrites the buffer's with the whole rows', and AkA may be assembled again after it
                    P = self._workspace2d("grav_iplanes", self.Ms + 1, 2 * plane)[:self.Ms]
                    P[:Mrun, :plane].copy_(outs[0][:Mrun, :plane])
                    P[:Mrun, plane:].copy_(outs[0][:Mrun, (self.ny - 1) * plane:self.ny * plane])
                    step.grav_iplanes = P
                if not self.f32 and not isinstance(A, StreamedOperator):
                    if not half:
                        return sp.product(A, Mrun, lams, [o[:Mrun] for o in outs], y0, y1, gx=gx)
                    # resident rows: the same operands as the pooled feed's -- the slab spectra of every row from the operator's own
                    # planes 0 and ny-1, the interior part as a batch copy of the rows with those two planes zeroed
                    step.grav_slabs = sp.slab_pair_rows(sp.slab_spectra(A, self.Ms), self.Ms, lams[0], slabs_to())
                    abuf = self._op_rows_buffer()
                    for r0 in range(0, Mrun, sp.R):
                        R = min(sp.R, Mrun - r0)
                        abuf[:R, :self.N].copy_(A[r0:r0 + R, :self.N])
                        abuf[:R, :plane].zero_()
                        abuf[:R, (self.ny - 1) * plane:self.ny * plane].zero_()
                        sp.product(abuf, R, lams, [o[r0:r0 + R] for o in outs], y0, y1, gx=gx and gx.at(r0))
                    return keep_planes()
                # row batches: operator rows generated on demand (streamed) and / or the product written to an fp64 scratch and
                # stored as fp32 (fp32 assembly); one batch = the spectral product's own batch size
                Rb = sp.R
                abuf = self._op_rows_buffer() if isinstance(A, StreamedOperator) else None
                scr = [self._workspace2d("ak_rows64_%d" % jj, Rb, nc) for jj in range(len(lams))] if self.f32 else None
                pool = sp.plane_pool(A.lattice, self.Ms if half else Mrun, A.lattice.jy, A.lattice.jx) if pooled else None
                if half:
                    step.grav_slabs = sp.slab_pair_rows(pool.edge, self.Ms, lams[0], slabs_to())
                    zero = self._workspace("pool_zero_planes", (2 * sp.Cp,))
                    zero.zero_()
                    pool = pool.interior(zero)
                for r0 in range(0, Mrun, Rb):
                    R = min(Rb, Mrun - r0)
                    if pool is not None:
                        src = pool.rows(r0)                   # no rows and no transform of them: the y stage reads the pool
                    elif abuf is not None and A.lattice is not None:
                        src = A.lattice.rows(r0)              # no rows at all: the forward transform reads the stencil table
                    else:
                        src = A.rows_into(abuf, r0, R) if abuf is not None else A[r0:r0 + R]
                    dst = [b[:R] for b in scr] if scr is not None else [o[r0:r0 + R] for o in outs]
                    sp.product(src, R, lams, dst, y0, y1, gx=gx and gx.at(r0))
                    if scr is not None:
                        for jj in range(len(lams)):
                            hip.convert(dst[jj], outs[jj][r0:r0 + R])
                if half:
                    keep_planes()
            self._timed("spectral_product", fl, lambda: product_rows(feed), valu=fv)
            # what the buffer's readers are owed of this operator's rows and the step did not store whole: the hand-over's interior planes,
            # and with the cross block from the magnetic rows A_g K_01, which the step did not run
            whole = feed is None or feed.store_all
            late = [j for j in props if (not step.sym or (s_, j) in kept) and not (whole and j in blocks)]
            if late:
                # (half: the fill runs every gravity row whole, with its own boundary planes -- the launches of a step without the shortcut)
                whole_rows = dict(Mrun=self.Ms, half=False) if half else {}
                step.ak_fill.append(lambda fill=product_rows, lams=[gen_of[j] for j in late], outs=[out_of[j] for j in late], kw=whole_rows:
                                    fill(None, lams=lams, outs=outs, **kw))

    def _gram_feed_applies(self, step, blocks):
        """The condition of _gram_feed for the blocks `blocks` of one operator's rows (nothing is allocated here)."""
        gram, sp = self._gram, self._spectral_product()
        funcs = ("grav", "magn")
        return bool(gram_gx_route(self.feed, self.route.family, step.sym, self.f32, self.world, self.exchange, self.nx, self.ny, self.nz, sp.forms)
                    and gram is not None and gram.gx_applies() and sp.gx_applies()
                    and all(j in (0, 1) and self._lam.get(funcs[j]) is not None for j in blocks))

    def _grav_mirror_rows(self, step, A_g):
        """Gravity rows whose interior part a step of the symmetric plan runs when the interior part of AkA's gravity block comes from
        half its rows ("gravity block from half its rows"): ceil(Ms / 2) rounded up to the spectral product's batch, as
        _mirror_rows; 0: every row runs whole.  plan.grav_mirror_route holds the gate."""
        if not step.sym:                                      # (no symmetric plan: nothing to ask, and no spectral product need exist)
            return 0
        sp = self._spectral_product()
        hit, lam = self._mirror.get("grav"), self._lam.get("grav")
        static = hit is not None and hit[0] is A_g            # (measured only where _mirror_static held; what it measured is not asked)
        even = lam is not None and lam[0] is A_g              # (LatticeGram.eigen accepted the stencil table of exactly this operator)
        # interior planes and boundary slabs of a row can be fed apart: the pooled feed of an implicit operator, or resident fp64 rows
        # (copied a batch at a time with their two boundary planes zeroed: the same operands, so the two forms agree bit for bit)
        if isinstance(A_g, StreamedOperator):
            pooled = A_g.lattice is not None and A_g.lattice.jy is not None and sp.pool_applies()
        else:
            pooled = not self.f32
        pooled = bool(pooled and (self.c0, self.c1) == (0, self.nx * self.ny * self.nz))
        handover = bool(step.sym and 0 in step.props and self._gram_feed_applies(step, [0]))
        alone = step.cross_rows == "magn"                     # (otherwise block K_01 needs every gravity row whole)
        if not grav_mirror_route(self.grav, step.sym, static, handover, pooled, even, alone, self.nx, self.ny, self.nz):
            return 0
        return min(self.Ms, ((self.Ms + 1) // 2 + sp.R - 1) // sp.R * sp.R)

    def _gram_feed(self, step, s_, blocks):
        """The hand-over of x-analysed rows from the A K product of operator s_ to the lattice Gram (options.gram_gx; DESIGN.md 2,
        "x step in the A K inverse"), or None where the route does not apply: the symmetric plan of the one-rank `single` family, fp64
        assembly, both operators' Gram on the stencil eigen-data, 64 x 64 (x, z) planes.  Block j of A K meets operator j in AkA."""
        gram, funcs = self._gram, ("grav", "magn")
        if not self._gram_feed_applies(step, blocks):
            return None
        S =[self._workspace("gram_S_%d%d" % (s_, j), (self.Ms * gram.Py * gram.Px,)) for j in blocks]
        for j, Sj in zip(blocks, S):
            step.gram_S[(s_, j)] = Sj
        # AkA is the only reader of these rows inside a step ("Unwritten rows"): of A K the product stores the two
        # boundary planes (the Gram's edge_rows reads them); the rest is written by step.ak_fill when somebody asks for the buffer
        return _GramFeed(gram, [self._lam[funcs[j]][1] for j in blocks], S, store_all=False)

    def _edge_spectrum(self, func, k, ycols):
        """Spectrum of boundary slab k (0: iy = 0, 1: iy = ny - 1) of operator `func` for the lattice Gram's x-correlation; built once
        per operator build (clear_operators drops it) from the slab's columns of the operator."""
        key = (func, k)
        hit = self._edgeV.get(key)
        if hit is None or hit[0] != ycols.data_ptr():
            hit = self._edgeV[key] = (ycols.data_ptr(), self._gram.edge_eigen(ycols))
        return hit[1]

    MIRROR_BOUND = 2.0 ** -48      # |a - mirror(a)| <= 2^-48 max|a|: a condition on the operator, not a tuning value

    def _mirror_static(self, plan):
        """What the mirrored magnetic block of AkA needs before anything is measured: the one-rank `single` family, fp64 assembly, a
        row-major lattice survey with a sensor over every voxel column (sensor r and sensor Ms - 1 - r are point mirrors)."""
        return bool(self.aka_mirror_on and plan is not None and plan["rowmajor"] and self.route.family == "single" and self.world == 1
                    and not self.exchange and not self.f32 and self.Ms_pad == self.Ms)

    def _mirror_record(self, func, A, mirror):
        """The measurement _gram_eigen's host read brought back for operator A (mirror: what was handed to it, None: not measured): the
        largest deviation of the stencil table and of the boundary slabs from their point mirror against the largest entry."""
        meas, self._mirror_meas = self._mirror_meas, None
        if mirror is None or meas is None:
            return
        dq, mq, de, me = meas
        scale = max(mq, me)
        ok = bool(dq <= self.MIRROR_BOUND * scale and de <= self.MIRROR_BOUND * scale and scale > 0.0)      # (a NaN anywhere: no)
        self._mirror[func] = (A, ok)
        self.aka_mirror[func] = dict(deviation=max(dq, de) / scale if scale > 0.0 else float("nan"), bound=self.MIRROR_BOUND,
                                     table=(dq, mq), slabs=(de, me), symmetric=ok, taken=False)

    def _mirror_rows(self, step, A_m):
        """Magnetic rows a step of the symmetric plan has to run when the rest of AkA's magnetic block is the point mirror of them:
        ceil(Ms / 2) rounded up to the spectral product's batch (0: all rows -- the operator did not measure symmetric, or no gate)."""
        hit = self._mirror.get("magn")
        if not (self.aka_mirror_on and step.sym and hit is not None and hit[0] is A_m and hit[1] and 1 in step.props):
            return 0
        R = self._spectral_product().R
        return min(self.Ms, ((self.Ms + 1) // 2 + R - 1) // R * R)

    def _gram_eigen(self, plan, lws, rows=False, mirror=None):
        """Eigen-data of the operator's stencil table for the lattice Gram (lattice_gram.py); None -> AkA by the N-deep GEMM.
        rows: the row form asks (no column-shard arithmetic applies: every rank correlates whole rows).
        mirror: (stencil table, boundary slab iy = 0, slab iy = ny - 1) of the operator -- their deviation from the point mirror is
        reduced on the device (geobo_mirror_dev) and read with the evenness check: no second synchronisation per operator build."""
        from .lattice_gram import LatticeGram
        plane = self.nx * self.nz
        Ly = (self.c1 - self.c0) // plane
        # column-sharded runs: every rank correlates its own y-slab of the A K rows (the partial results add up in the all-reduce
        # of AkA); the x step and the back-transform are not divided, so from ~5 ranks the N-deep GEMM over N/G columns is cheaper
        # (with the row exchange -- 4 ranks and more -- the GEMM over N/G columns is within a few ms of it: not used there)
        if (not self.use_spectral or not plan["rowmajor"] or self.Ms_pad != self.Ms
                or not LatticeGram.supported(self.nx, self.ny, self.nz) or not self.route.opt("aka_lattice")):
            return None
        if not rows:
            # the column forms of the Gram run on the fused n = 64 kernels' grids only (their batched-GEMM stand-ins pay in the row form)
            if not LatticeGram.fast(self.nx, self.ny, self.nz):
                return None
            form = lattice_gram_form(self.exchange, self.f32 or self.streamed, self.world, self.Ms, self.c0, self.c1, plane, self.N)
            if form is None:
                return None
        if self._gram is None:
            self._gram = LatticeGram(self._spectral_product(), self.device)
        if mirror is None:
            return self._timed("aka_lattice_eigen", 0.0, lambda: self._gram.eigen(hip.a_sens_lattice_stencil(lws, self.nx, self.ny, self.nz)))
        Q, E0, E1 = mirror

        def measured():
            nqx, ws = 2 * self.nx - 1, self._workspace("mirror_ws", (hip.mirror_dev_ws_doubles(),))
            out = self._workspace("mirror_out", (4,))
            Q2 = Q.view(2 * self.ny - 3, nqx * self.nz)
            hip.mirror_dev(Q2, Q2, 2 * self.ny - 3, nqx, self.nz, out=out[0:2], ws=ws)
            hip.mirror_dev(E0, E1, self.Ms, self.nx, self.nz, out=out[2:4], ws=ws)
            lam = self._gram.eigen(Q, extra=out)
            self._mirror_meas = tuple(self._gram.extra_host)
            return lam
        return self._timed("aka_lattice_eigen", 0.0, measured)

    def _assemble_AkA(self, step, AK, A_g, A_m):
        """AkA = A K A3^T (+ the noise variances) into the workspace step.aka_slot, from what _assemble_AK(step, ...) left."""
        nc = self.nc
        props, Md, M_pad = step.props, step.Md, step.M_pad
        off_d = 2 * self.Ms_pad
        AkA = self._workspace(step.aka_slot, (M_pad, M_pad))
        AkA.zero_()
        if step.rowpath or (self._row_gram() and step.fullrows):
            return self._assemble_AkA_rows(step, AkA)
        if step.sym:
            return self._assemble_AkA_sym(step, AkA, AK, A_g, A_m)
        # only the LOWER triangle of AkA is consumed (Cholesky, lower=True): block column s needs rows >= s*Ms_pad, and
        # tiles strictly above the diagonal are skipped inside the GEMM (47 % fewer tiles at 64^3)
        for s_, A in ((0, A_g), (1, A_m)):
            jj = props.index(s_)
            r0 = s_ * self.Ms_pad
            rows = M_pad - r0
            tiles = sum(min(2 * (bi + 1), self.Ms_pad // 128) for bi in range(rows // 256))  # lower-only 256x128 tiles
            # a few hundred long tiles do not fill 256 CUs evenly: split the contraction into concurrent slices
            splits = 1
            for cand in ((8, 4, 2) if tiles < 512 else (4, 2)):
                if nc % (16 * cand) == 0 and nc // cand >= 2048 and tiles < 4096:
                    splits = cand
                    break
            streamed = isinstance(A, StreamedOperator)
            Xv, Cv = AK[r0:, jj * nc:(jj + 1) * nc], AkA[r0:, r0:r0 + self.Ms_pad]
            Yv = None if streamed else (A if A.data_ptr() in self._slab_ops else A[:, self.c0:self.c1])
            mv = off_d + Md - r0                       # rows behind the last drill row are padding: not contracted
            pl = self.nx * self.nz
            ya, yb = self.c0 // pl, self.c1 // pl      # this rank's y-slab (slab-aligned shards only where it is used)

            def operand_cols(cs, ce):
                """Columns [cs, ce) of this rank's slice of the operator, for every sensor."""
                if Yv is not None:
                    return Yv[:, cs:ce]
                return A.slab_into(self._workspace2d("op_slab", self.Ms_pad, pw_stream), ya + cs // pl, ya + ce // pl)
            lam = self._lam.get(("grav", "magn")[s_])
            lam = lam[1] if lam is not None and lam[0] is A else None
            if lam is not None:
                # lattice survey, even stencil: interior y-slabs by the (y, x) correlation, the two padded slabs by a GEMM
                gram = self._gram
                pw_stream = pl
                edges = [c for iy, c in ((0, 0), (self.ny - 1, (self.ny - 1 - ya) * pl)) if ya <= iy < yb]
                fl = gram.flops(mv, yb - ya) + 2.0 * len(edges) * pl * 128 * sum(
                    min(2 * (bi + 1), self.Ms_pad // 128) * rv for bi, rv in enumerate(hip.tile_rows(rows, mv)))

                def lattice():
                    if Xv.dtype == F64:
                        gram.gram_rows(Xv, mv, lam, Cv, ya, yb)
                    else:
                        for rb in range(0, mv, gram.R):       # fp32 A K: the Gram's own row batches, converted on the way in
                            R = min(gram.R, mv - rb)
                            gram.gram_rows(self._panel64("gram_rows64", Xv[rb:rb + R], rows=gram.R), R, lam, Cv[rb:], ya, yb)
                    for c0 in edges:
                        k = 0 if ya + c0 // pl == 0 else 1
                        if streamed and A.lattice is not None:      # the two boundary slabs are kept with the stencil table
                            ycols = A.edge[:, k * pl:(k + 1) * pl]
                        else:
                            ycols = operand_cols(c0, c0 + pl)
                        if gram.edge_supported() and Xv.dtype == F64:
                            # x-Toeplitz slab: correlation through the full real DFT (three batched GEMMs) instead of a 4096-deep GEMM
                            gram.edge_rows(Xv[:, c0:], mv, self._edge_spectrum(("grav", "magn")[s_], k, ycols), Cv)
                        else:
                            hip.gemm_nt(self._panel64("aka_panel64", Xv[:, c0:c0 + pl]), ycols, Cv, alpha=1.0,
                                        beta=1.0, lower_only=True, m_valid=mv)
                self._timed("aka_lattice", fl, lattice)
                continue
            # executed flop: lower-only tiles, whole 64-row wavefront groups of the last row tile
            fl = 2.0 * 128 * nc * sum(min(2 * (bi + 1), self.Ms_pad // 128) * rv for bi, rv in enumerate(hip.tile_rows(rows, mv)))
            # 8(d): 2 M Ms N for the full block column; the lower triangle that is consumed is half of the square part
            nv = min(nc, max(self.N - self.c0, 0))
            alg = 2.0 * nv * (self.Ms * (self.Ms + 1) / 2.0 + (mv - self.Ms_pad) * self.Ms)
            if Xv.dtype != F64 or streamed:
                # column panels: A K converted to fp64 and / or the operator's columns generated panel by panel, accumulated
                unit = pl if streamed else 2048
                pw_stream = pw = max(unit, min(nc, int((3 << 30) // (8 * rows)) // unit * unit))

                def panels():
                    for cs in range(0, nc, pw):
                        ce = min(nc, cs + pw)
                        hip.gemm_nt(self._panel64("aka_panel64", Xv[:, cs:ce], cols=pw), operand_cols(cs, ce), Cv, alpha=1.0,
                                    beta=1.0, lower_only=True, m_valid=mv)
                self._timed("aka_gemm_nt", fl, panels, alg=alg)
            elif splits > 1:
                ws = self._workspace("aka_ws", (splits * rows * self.Ms_pad,))
                self._timed("aka_gemm_nt", fl, lambda: hip.gemm_nt_splitk(Xv, Yv, Cv, splits, ws, lower_only=True, m_valid=mv), alg=alg)
            else:
                self._timed("aka_gemm_nt", fl, lambda: hip.gemm_nt(Xv, Yv, Cv, lower_only=True, m_valid=mv), alg=alg)
        allreduce_sum_(AkA, self.world, self.group)
        return self._finish_AkA(step, AkA)

    def _finish_AkA(self, step, AkA):
        """Drill columns by symmetry, the drill-drill block, the noise variances on the diagonal (identity on the padding).
        A derivative Gram (step.noise None) gets no diagonal: its padding stays zero.  step.keep_signal: the matrix before the diagonal
        is copied into the "K_signal" workspace (the signal part of K, for the amplitude and weight derivatives)."""
        xyz = self.grid_points()
        sel_t, Md, gp_sigma = step.sel_t, step.Md, step.noise
        off_d = 2 * self.Ms_pad
        if gp_sigma is not None:
            dvec = torch.ones(step.M_pad, dtype=F64, device=self.device)
            dvec[0:self.Ms] = float(gp_sigma[0]) ** 2
            dvec[self.Ms_pad:self.Ms_pad + self.Ms] = float(gp_sigma[1]) ** 2
        if Md:
            AkA[:off_d, off_d:off_d + Md] = AkA[off_d:off_d + Md, :off_d].t()
            rows = tuple(c[sel_t] for c in xyz)
            # (create_cov's self blocks carry weight 1: weight_matrix; the unit-weight pair Gram of logl_grad has 0 there)
            step.prior.k_block(self, 2, 2, rows, rows, AkA[off_d:off_d + Md, off_d:off_d + Md])
            if gp_sigma is not None:
                dvec[off_d:off_d + Md] = float(gp_sigma[2]) ** 2
        drop = None
        if step.row_scale is not None:
            # committed row scales (reweight.py): s^2 on the noise variance; a dropped row leaves K_y as a zero row and column with a
            # unit diagonal (a derivative Gram: the zero row and column alone)
            s2, dropped = step.row_scale
            if dropped.size:
                drop = torch.as_tensor(dropped, device=self.device)
                AkA[drop, :] = 0.0
                AkA[:, drop] = 0.0
            if gp_sigma is not None:
                dvec.mul_(torch.as_tensor(s2, device=self.device))
                if drop is not None:
                    dvec[drop] = 1.0
        if gp_sigma is None:
            return AkA
        if step.keep_signal:
            self._workspace("K_signal", tuple(AkA.shape)).copy_(AkA)
        AkA.diagonal().add_(dvec)
        return AkA

    def _pad_y(self, y_g, y_m, y_d, M_pad, dropped=None):
        y = np.zeros(M_pad)
        y[0:self.Ms] = y_g
        y[self.Ms_pad:self.Ms_pad + self.Ms] = y_m
        if len(y_d):
            y[2 * self.Ms_pad:2 * self.Ms_pad + len(y_d)] = y_d
        if dropped is not None:
            y[dropped] = 0.0                    # (rows of the padded matrix that the committed row scales drop, reweight.py)
        return hip.to_dev(y, self.device)

    def _results_to_host(self, mu, var, props, queued=None):
        """(P_c N) device mean and variance, complete on this rank -> the reference's two (3N,) property-major host vectors (NaN: blocks
        not computed).  One device-to-host copy for both; queued: the staging array of a copy that was queued (and waited for) already."""
        N, P_c = self.N, len(props)
        h = queued if queued is not None else self._to_host(torch.cat([mu.reshape(-1)[:P_c * N], var.reshape(-1)[:P_c * N]]), 0)
        outs = []
        for k in range(2):
            out = np.empty(3 * N)
            for j in range(3):
                if j in props:
                    jj = props.index(j)
                    out[j * N:(j + 1) * N] = h[(k * P_c + jj) * N:(k * P_c + jj + 1) * N]
                else:
                    out[j * N:(j + 1) * N] = np.nan
            outs.append(out)
        return outs

    @_on_device
    def posterior(self, A_g, A_m, sel, y_g, y_m, y_d, lengths, crossweights, kernelfunc, gp_sigma, gp_amp=1.0,
                  props=(0, 1, 2), calclogl=True, want_mean_var=True, keep_K=False, potrf_schedule=None):
        """Posterior mean / variance / log-likelihood.  `lengths` must already carry the create_cov mutation.
        Returns dict(mu (3N, NaN for skipped property blocks), var, logl, info).
        potrf_schedule: the `schedule` of hip.potrf_inv for this step (None: the engine's resolved option, self.options.potrf).
        keep_K (internal, logl_grad): keep a copy of the assembled K without its diagonal (workspace "K_signal") before the
        in-place factorisation."""
        props = tuple(props)
        assert 0 in props and 1 in props, "gravity and magnetic blocks are needed for AkA"
        sel = np.asarray(sel, dtype=np.int64)
        sel_t = torch.as_tensor(sel, device=self.device) if sel.size else None
        t = self._tick("start")
        # the data vector goes up first: a pageable host-to-device copy blocks the host until the stream reaches it
        scales = self._step_row_scale(sel)
        y = self._pad_y(y_g, y_m, y_d, hip.pad_m(2 * self.Ms_pad + len(sel)), None if scales is None else scales[1])
        if self.rows_static and not self._rows_denied and not self._rows_ok(A_g, A_m) and all(f in self._op_args for f in ("grav", "magn")):
            # operators handed in from before a denial / a clear: rebuild them from the recorded arguments in the form this step takes
            A_g, A_m = (self.operator(f, *self._op_args[f][:1], B=self._op_args[f][1], axes=self._op_args[f][2]) for f in ("grav", "magn"))
        step = self._step = self._new_step(Prior(kernelfunc, lengths, weight_matrix(crossweights), gp_amp), props, sel_t, gp_sigma,
                                           keep_signal=bool(keep_K), row_scale=scales, sym=not self.rows_static and self._sym_ok(A_g, A_m))
        M_pad = step.M_pad
        step.mirror = self._mirror_rows(step, A_m)
        step.cross_rows = "magn" if cross_rows_route(self.cross, step.sym, step.mirror, self.nx, self.ny, self.nz) else "grav"
        step.grav_mirror = self._grav_mirror_rows(step, A_g)
        for f, rec in self.aka_mirror.items():
            # (magnetic: the whole block is the mirror of its first half, by measurement; gravity: the interior part only, by the Gram's
            # evenness check of the stencil table -- the record's table / slabs deviations are kept beside it, the slabs ungated)
            rec["taken"] = bool(step.mirror if f == "magn" else step.grav_mirror)
        AK = self._assemble_AK(step, A_g, A_m)
        self.step_route = "rows" if step.rowpath else ("single" if step.sym else "columns")
        t = self._tick("ak_fused", t)
        AkA = self._assemble_AkA(step, AK, A_g, A_m)
        if self.aka_hook is not None:          # tools/emulate_rank.py: keep the assembled matrix (1 rank) / put the true one in place
            self.aka_hook(AkA)                 # of what an emulated all-gather produced (a lone rank of G)
        t = self._tick("aka", t)
        if self._potrf_ctx is None:
            self._potrf_ctx = hip.PotrfContext()       # fork streams of the L^-1 build: per engine, on this engine's device
        Linv, info = self._timed("potrf_inv", 2.0 * M_pad ** 3 / 3.0, lambda: hip.potrf_inv(
            AkA, self._workspace("Linv", (M_pad, M_pad)), self._workspace("potrf_ws", (hip.potrf_ws_doubles(M_pad),)),
            ctx=self._potrf_ctx, schedule=potrf_schedule or self.options.potrf), alg=(2 * self.Ms + len(sel)) ** 3 * 2.0 / 3.0)  # AkA now holds L
        L = AkA
        if scales is not None and scales[1].size:
            # dropped rows: row and column of L^-1 are those of the identity; without the diagonal entry the row is gone from every
            # product that works from L^-1 (u_i = 0, a zero row of V), and its unit pivot adds nothing to logdet
            Linv.diagonal()[torch.as_tensor(scales[1], device=self.device)] = 0.0
        self._finish_exchange()
        u, stats = hip.trmv_stats(Linv, y, L)
        t = self._tick("cholesky", t)
        out = dict(info=0, M_pad=M_pad, lengths=[float(v) for v in lengths])

        def check_factor():
            # the status word and the likelihood statistics come back in one host read, AFTER the reduction has been queued:
            # a failed factorisation costs the wasted launch, a good one (every step of a survey) no idle gap in front of it
            # the long wait of a step is spent HERE, in the stream's own synchronize: a pageable device-to-host copy that has to wait
            # for a busy stream itself now and then returns 25-30 ms late (one step in five at 64^3)
            # ... and every read-back of the step is queued in front of that one wait (each further wait is a host wake-up: ~1 ms)
            h_info = self._to_host_async(info, "info")
            st = self._to_host_async(stats, "stats") if calclogl else None
            resid = getattr(self._spectral, "sym_residual", None)
            h_res = self._to_host_async(resid.reshape(1), "sym_residual") if resid is not None else None
            if resid is not None:
                self._spectral.sym_residual = None      # read (queued above) exactly once, whatever this step raises
            torch.cuda.current_stream(self.device).synchronize()
            info_h = int(h_info[0])
            if info_h == -7:
                raise FactorisationTimeout("geobo_potrf_inv: the tile DAG timed out on a hand-off (info = -7)")
            if info_h != 0:
                raise CholeskyError(info_h)
            if h_res is not None:
                if not float(h_res[0]) <= 1e-12:
                    # the three-product y stage (geobo_toeplitz_y2s) took blocks (0, 1) and (1, 0) of the prior for one block
                    raise RuntimeError("the covariance blocks (0, 1) and (1, 0) differ (relative %.3e): this prior is not symmetric; "
                                       "set GEOBO_Y2S=0 for the four-product y stage" % float(h_res[0]))
            if calclogl:
                out["uu"], out["logdet"] = float(st[0]), float(st[1])
                out["logl"] = -0.5 * (st[0] + st[1] + self.N * math.log(2 * math.pi))  # inversion.py:107-110
            else:
                out["logl"] = 0.0
        mv = None       # (device mean, device variance, elements between their property blocks): what append_drill_rows starts from
        if not want_mean_var:
            check_factor()
        if want_mean_var and step.rowpath:
            mu_f, var_f = self._posterior_rows(step, Linv, u)
            mv = (mu_f, var_f, self.N)
            N_ = len(props) * self.N
            hq = self._to_host_async(torch.cat([mu_f.reshape(-1)[:N_], var_f.reshape(-1)[:N_]]), 0)
            check_factor()
            t = self._tick("posterior", t)
            out["mu"], out["var"] = self._results_to_host(mu_f, var_f, props, queued=hq)
            self._tick("d2h", t)
        elif want_mean_var:
            # executed flop: every 64-row wavefront group g of the valid rows contracts the 64 g columns in front of its diagonal
            # block in full, and of the block itself the 16-row sub-groups' chunks at or below the diagonal (40 of 64 MFMA steps)
            Mv = 2 * self.Ms_pad + len(sel)
            fl = 2.0 * AK.shape[1] * sum(64.0 * 64 * g + 2560.0 for g in range((Mv + 63) // 64))
            Mu = 2 * self.Ms + len(sel)                                  # unpadded observation rows
            nv = len(props) * min(self.nc, max(self.N - self.c0, 0))     # this rank's voxel-property columns
            zp = self._zpath_ok(step, AK)
            if step.sym and not zp:
                raise RuntimeError("internal: A K was assembled for the transposed posterior, which is not available")
            if zp:
                mu_l, var_l = self._posterior_zpath(step, Linv, AK, u, A_g, A_m)
            elif AK.dtype == F64:
                mu_l, var_l = self._timed("posterior_reduce", fl, lambda: hip.posterior_reduce(
                    Linv, AK, u, gp_amp * 1.0, self._workspace("post_ws", (hip.posterior_ws_doubles(M_pad, AK.shape[1]),)), m_valid=Mv),
                    alg=(1.0 * Mu * Mu + 4.0 * Mu) * nv)
            else:
                ncols = AK.shape[1]
                pw = max(128, min(ncols, int((3 << 30) // (8 * M_pad)) // 128 * 128))

                def panels():
                    ws = self._workspace("post_ws", (hip.posterior_ws_doubles(M_pad, pw),))
                    parts = [hip.posterior_reduce(Linv, self._panel64("post_panel64", AK[:, cs:min(ncols, cs + pw)], cols=pw), u,
                                                  gp_amp * 1.0, ws, m_valid=Mv) for cs in range(0, ncols, pw)]
                    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
                mu_l, var_l = self._timed("posterior_reduce", fl, panels, alg=(1.0 * Mu * Mu + 4.0 * Mu) * nv)
            one = self.world == 1 and self.N == self.N_pad
            mv = (mu_l, var_l, self.nc) if self.world == 1 else None
            N_ = len(props) * self.N
            hq = self._to_host_async(torch.cat([mu_l.reshape(-1)[:N_], var_l.reshape(-1)[:N_]]), 0) if one else None
            check_factor()
            t = self._tick("posterior", t)
            if one:
                out["mu"], out["var"] = self._results_to_host(mu_l, var_l, props, queued=hq)
            else:
                mu = assemble_columns(gather_slices(mu_l, len(props), self.N_pad, self.world, self.group), props, self.N,
                                      self.N_pad, self.world, to_host=self._to_host)
                var = assemble_columns(gather_slices(var_l, len(props), self.N_pad, self.world, self.group), props, self.N,
                                       self.N_pad, self.world, to_host=self._to_host)
                out["mu"], out["var"] = mu, var
            self._tick("d2h", t)
        # A K is published only when it is whole; the symmetric plan leaves the blocks (magn rows, block 0) and (sensor rows, block 2)
        # unwritten: that buffer goes under AK_partial (the tests' oracle contacts read its assembled blocks); the row form has none
        whole = AK is not None and not step.sym
        self.last = _LastStep(L=L, Linv=Linv, u=u, AK=AK if whole else None, AK_partial=None if whole else AK, AK_complete=whole, props=props,
                              sel=sel, ops=(A_g, A_m), step=step, mv=mv, uu=out.get("uu"), logdet=out.get("logdet"))
        self.last.complete = self._ak_completion(step, AK)
        return out

    def _ak_completion(self, step, AK):
        """engine.last's completion hook for the A K buffer of a finished step (None: nothing was left unwritten)."""
        fills = list(step.ak_fill)           # the storing products of what the step did not store whole (_assemble_AK_spectral) first
        if step.mirror and step.mirror < self.Ms:
            # a mirrored step left the magnetic rows behind step.mirror unwritten.  Nothing of the engine reads them (AkA was their only
            # reader); whoever asks for the buffer gets them by the mirrored row copy, once, so that no stale row is ever seen
            jj, nc, Msp, Mm = step.props.index(1), self.nc, self.Ms_pad, step.mirror
            fills.append(lambda: hip.mirror_rows(AK[Msp:Msp + self.Ms, jj * nc:jj * nc + self.N], self.Ms, Mm, self.nx * self.ny, self.nz))
        return _LastStep.chain(fills)

    def _derivative_gram(self, A_g, A_m, sel_t, prior, slot):
        """A derivative Gram dK in workspace `slot`: posterior()'s own assembly (_assemble_AK / _assemble_AkA, whichever route the
        step takes) as a step of its own over `prior`, without the noise diagonal, zero padding, lower triangle valid.  Its A K and
        its Gram go to workspaces of their own; the step the factor came from (self.last) is not touched."""
        step = self._new_step(prior, (0, 1, 2), sel_t, None, ak_slot="dK_AK", aka_slot=slot,
                              sym=not self.rows_static and self._sym_ok(A_g, A_m))
        return self._assemble_AkA(step, self._assemble_AK(step, A_g, A_m), A_g, A_m)

    @_on_device
    def logl_grad(self, A_g, A_m, sel, y_g, y_m, y_d, lengths, crossweights, kernelfunc, gp_sigma, gp_amp, directions,
                  potrf_schedule=None):
        """Exact gradient of f = (u.u + log det K) / 2 (calc_logl without the N log 2 pi term), K = amp sum_ij W_ij B_ij + D:
            df/dtheta = <S, dK/dtheta> / 2,   S = K^-1 - alpha alpha^T,   alpha = L^-T u,   K^-1 = L^-T L^-1 (never stored).
        One posterior() step (likelihood only) keeps K's signal part; G_0 = that part, plus the unit-weight blocks amp (B_ab + B_ba) of
        any pair whose weight is 0 (its block of K is zero); G_t = the Gram of the directional derivative along directions[t - 1]
        (`lengths` carry the create_cov mutation; directions are in the same metres).  One geobo_kinv_dot launch gives the block
        sums of <S, G_t> per pair of row segments, from which
            d_amp = sum over the non-zero-weight pairs / amp,  d_w = pair (a, b) / w (or the unit block's sum where w = 0),
            d_dir[t] = all pairs of G_t,
        each halved.  Returns dict(uu, logdet, d_amp, d_w (3,), d_dir (len(directions),)).  One rank, fp64 assembly.
        potrf_schedule: as in posterior()."""
        if self.world > 1:
            raise ValueError("logl_grad runs on one rank (world = %d): the multi-rank gradient is not implemented" % self.world)
        if self.f32:
            raise ValueError("logl_grad needs the fp64 assembly (assembly='f32' keeps fp32 covariance tables)")
        directions = [np.asarray(d, dtype=float).reshape(3) for d in directions]
        if len(directions) > 3:
            raise ValueError("at most three length directions per evaluation")
        props = (0, 1, 2)
        r = self.posterior(A_g, A_m, sel, y_g, y_m, y_d, lengths, crossweights, kernelfunc, gp_sigma, gp_amp=gp_amp, props=props,
                           calclogl=True, want_mean_var=False, keep_K=True, potrf_schedule=potrf_schedule)
        W = weight_matrix(crossweights)
        Linv, u = self.last["Linv"], self.last["u"]
        M_pad = Linv.shape[0]
        sel = np.asarray(sel, dtype=np.int64)
        sel_t = torch.as_tensor(sel, device=self.device) if sel.size else None
        alpha = hip.colgemv(Linv, u, ws=self._workspace("grad_colgemv_ws", (hip.colgemv_ws_doubles(M_pad, M_pad),)))   # L^-T u
        G0 = self._workspace("K_signal", (M_pad, M_pad))
        wvals = [W[a][b] for a, b in WEIGHT_PAIRS]
        if any(w == 0.0 for w in wvals):
            Wu = [[0.0] * 3 for _ in range(3)]
            for (a, b), w in zip(WEIGHT_PAIRS, wvals):
                if w == 0.0:
                    Wu[a][b] = Wu[b][a] = 1.0
            G0.add_(self._derivative_gram(A_g, A_m, sel_t, Prior(kernelfunc, lengths, Wu, gp_amp), "dK_unit"))
        Gs = [G0] + [self._derivative_gram(A_g, A_m, sel_t, Prior(kernelfunc, lengths, W, gp_amp, deriv=d), "dK_dir%d" % t)
                     for t, d in enumerate(directions)]
        segs = ((0, self.Ms), (self.Ms_pad, self.Ms_pad + self.Ms), (2 * self.Ms_pad, 2 * self.Ms_pad + len(sel)))
        out = self._timed("kinv_dot", M_pad ** 3 / 3.0, lambda: hip.kinv_dot(
            Linv, alpha, Gs, segs, ws=self._workspace("kinv_dot_ws", (hip.kinv_dot_ws_doubles(M_pad, len(Gs)),))))
        o = self._to_host(out, "kinv_dot").reshape(len(Gs), 3, 3).copy()
        pair = lambda t, a, b: float(o[t, a, b])
        diag = sum(pair(0, a, a) for a in range(3))
        d_w = np.empty(3)
        off = 0.0
        for k, ((a, b), w) in enumerate(zip(WEIGHT_PAIRS, wvals)):
            if w == 0.0:
                d_w[k] = 0.5 * pair(0, a, b)
            else:
                d_w[k] = 0.5 * pair(0, a, b) / w
                off += pair(0, a, b)
        d_dir = np.array([0.5 * sum(pair(t, a, b) for a in range(3) for b in range(a, 3)) for t in range(1, len(Gs))])
        return dict(uu=r["uu"], logdet=r["logdet"], d_amp=0.5 * (diag + off) / gp_amp, d_w=d_w, d_dir=d_dir)

    @_on_device
    def posterior_covariance(self, kernelfunc, lengths, crossweights, gp_amp=1.0, limit_bytes=48 << 30):
        """Full (3N x 3N) posterior covariance  K - V^T V  (inversion.py:117) from the state the last posterior() call left on
        the device (A K, L^-1) -- what `predict3(full_cov=True)` returns.  Small cubes only: 9 N^2 doubles are built on the
        device and copied to the host, exactly the object the matrix-free path exists to avoid."""
        last = getattr(self, "last", None)
        if last is not None and not last.get("AK_complete", True):
            raise RuntimeError("full covariance needs A K from the last posterior(), and this step kept only the blocks AkA needs "
                               "(symmetric / row form of the transposed order): rerun with GEOBO_POSTERIOR=dense for predict3(full_cov=True)")
        if last is None or tuple(last["props"]) != (0, 1, 2) or self.world != 1 or last["AK"].dtype != F64:
            raise RuntimeError("full covariance needs a single-rank fp64 posterior() with all three property blocks")
        n3 = 3 * self.N_pad
        if n3 * n3 * 8 * 2 > limit_bytes:
            raise MemoryError("full posterior covariance of %d voxels needs %.1f GB; use the diagonal (np.diag(cov))"
                              % (self.N, n3 * n3 * 8 / 1e9))
        W = weight_matrix(crossweights)
        Linv, AK = last["Linv"], last["AK"]
        M_pad = Linv.shape[0]
        V = torch.empty((M_pad, n3), dtype=F64, device=self.device)
        hip.gemm_nn(Linv, AK, V, x_lower=True)                             # V = L^-1 (A K), block columns [prop][voxel]
        Vt = V.t().contiguous()
        del V
        C = torch.empty((n3, n3), dtype=F64, device=self.device)
        xyz = self.grid_points()
        for i in range(3):
            for j in range(3):
                hip.k_block(hip.kernel_id(kernelfunc, i != j), xyz, xyz, lengths[i], lengths[j], W[i][j], gp_amp,
                            C[i * self.N_pad:(i + 1) * self.N_pad, j * self.N_pad:(j + 1) * self.N_pad])
        hip.gemm_nt(Vt, Vt, C, alpha=-1.0, beta=1.0)
        idx = torch.cat([torch.arange(self.N, device=self.device) + j * self.N_pad for j in range(3)])
        return C[idx][:, idx].cpu().numpy()

    # ---- posterior realisations (Matheron's rule) ------------------------------------------------------------
    def _operator_rows(self, A, rows=256, slot="cond_op_rows"):
        """(r0, rows) batches of a forward operator: the resident matrix at once, a streamed one 256 zero-padded rows at a time
        (`rows`, a multiple of 128, at a time into workspace `slot` for a caller that wants another batch; never beyond row Ms_pad)."""
        if not isinstance(A, StreamedOperator):
            yield 0, A[:self.Ms_pad, :self.N_pad]
            return
        buf = self._workspace2d(slot, rows, self.N_pad)
        for r0 in range(0, self.Ms, rows):
            R = min(rows, self.Ms - r0)
            A.rows_into(buf, r0, R)
            if R < rows:
                buf[R:].zero_()
            yield r0, buf[:min(rows, self.Ms_pad - r0)]

    @_on_device
    def condition(self, F, eps, A_g, A_m, y_g, y_m, y_d, sampler):
        """Condition S prior samples on the data with the factor of the last posterior() step (Matheron's rule):
            f_post = f + K A3^T w,   w = H^-1 (y - A3 f - eps) = L^-T L^-1 r,   H = A3 K A3^T + Sigma.
        F: (S, 3, N) device prior samples (sampler.sample); eps: (S, M) device observation noise, rows [grav | magn | drill] unpadded.
        A3 F and A3^T W are MFMA GEMMs against the operator (row batches of 256 for a streamed one); K (A3^T W) is the sampler's exact
        circulant product, the same on every single-rank route.  Returns (f_post (S, 3, N), w (S, M))."""
        if self.world > 1:
            raise NotImplementedError("posterior sampling runs on one rank (world = %d)" % self.world)
        last = self.last
        if last is None or tuple(last["props"]) != (0, 1, 2):
            raise RuntimeError("condition() needs the factor of a posterior() step over all three property blocks")
        Linv = last["Linv"]
        sel = np.asarray(last["sel"], dtype=np.int64)
        M_pad, Ms, Msp, N, Np, Md = Linv.shape[0], self.Ms, self.Ms_pad, self.N, self.N_pad, len(sel)
        off_d = 2 * Msp
        S = F.shape[0]
        Sp = hip.pad_m(S)
        dev = self.device
        # residual r = y - A3 f - eps, one padded row per sample
        Rt = torch.zeros((Sp, M_pad), dtype=F64, device=dev)
        Fp = torch.zeros((Sp, Np), dtype=F64, device=dev)
        AF = torch.empty((Sp, Msp), dtype=F64, device=dev)
        for j, (A, r0) in enumerate(((A_g, 0), (A_m, Msp))):
            Fp[:S, :N] = F[:, j, :]
            for c0, rows in self._operator_rows(A):
                hip.gemm_nt(Fp, rows, AF[:, c0:c0 + rows.shape[0]])
            Rt[:S, r0:r0 + Ms] = -AF[:S, :Ms]
        Rt[:S, 0:Ms] += hip.to_dev(np.asarray(y_g, dtype=np.float64), dev)
        Rt[:S, Msp:Msp + Ms] += hip.to_dev(np.asarray(y_m, dtype=np.float64), dev)
        Rt[:S, 0:Ms] -= eps[:, 0:Ms]
        Rt[:S, Msp:Msp + Ms] -= eps[:, Ms:2 * Ms]
        if Md:
            sel_t = torch.as_tensor(sel, device=dev)
            Rt[:S, off_d:off_d + Md] = hip.to_dev(np.asarray(y_d, dtype=np.float64), dev) - F[:, 2, :][:, sel_t] - eps[:, 2 * Ms:2 * Ms + Md]
        # w = L^-T (L^-1 r): rows of Z^T = R^T L^-T, then W^T = Z^T L^-1 (L^-1 lower triangular, upper part zero)
        Zt = hip.gemm_nt(Rt, Linv, torch.empty((Sp, M_pad), dtype=F64, device=dev))
        Wt = hip.gemm_nn(Zt, Linv, Rt, y_lower=True)
        del Zt
        # A3^T w on the voxel grid, block by block, then K through the circulant spectra
        V = torch.zeros((S, 3, N), dtype=F64, device=dev)
        Vp = torch.empty((Sp, Np), dtype=F64, device=dev)
        for j, (A, r0) in enumerate(((A_g, 0), (A_m, Msp))):
            for c0, rows in self._operator_rows(A):
                hip.gemm_nn(Wt[:, r0 + c0:r0 + c0 + rows.shape[0]], rows, Vp, beta=1.0 if c0 else 0.0)
            V[:, j, :] = Vp[:S, :N]
        if Md:
            V[:, 2, :][:, sel_t] = Wt[:S, off_d:off_d + Md]
        f_post = sampler.apply_K(V)
        f_post.add_(F)
        w = torch.cat([Wt[:S, 0:Ms], Wt[:S, Msp:Msp + Ms], Wt[:S, off_d:off_d + Md]], dim=1)
        return f_post, w
