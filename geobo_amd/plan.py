"""Route planning: every shape / rank-count / precision decision of an inversion step as ONE pure function.

`plan_route` maps (grid extents, world size, assembly precision, operator mode, method, environment overrides) to a `Route`: which
algorithm family the engine runs (engine.py reads nothing else to decide) and which kernels carry each stage (`stage_forms`).  No device, no torch:
the whole table is tested on the CPU for every BASELINE.json configuration x world in {1, 2, 4, 8}
(tests/test_host_logic_cpu.py::test_route_table).  The behaviour-changing GEOBO_* environment switches are overrides INTO this
function; what a step then does is recorded as `engine.route` / `engine.step_route` and in the bench line.

Families (DESIGN.md sections 2 and 7):
  "rows"     the structured algorithm sharded by SENSOR ROWS over world >= 1 ranks: the three blocks of A K that AkA's lower triangle
             needs, row block by row block through the spectral product and straight on through the lattice Gram (A K is never held),
             replicated Cholesky, transposed posterior V = (L^-1 A3) K on the rank's rows of L^-1, one all-gather + one all-reduce.
             Needs a lattice survey with even stencils (decided per operator build: engine falls back to "columns").
  "single"   one rank, fp64, the fused n = 64 kernels: the same algorithm with A K materialised once (engine._posterior_zpath,
             _assemble_AkA_sym) and, with operators="auto", operator rows read as windows of the stencil table.
  "columns"  voxel-column shards of A K / V (rounds 1-2): fused reduction L^-1 (A K), AkA by the N/G-deep GEMM or the column form of
             the lattice Gram, row exchange (all-to-all) from 4 ranks.  What runs for surveys off the lattice, the dense method, padded
             shapes and small grids without fused kernels.
Reference call sites all of these replace: inversion.py:92-117 (predict3), kernels.py:158-195 (create_cov)."""
from dataclasses import asdict, dataclass, make_dataclass

PAD_M, PAD_N = 256, 128
XZ2D_SHAPES = ((48, 64), (64, 64), (64, 32))      # fused (x, z) transform instances (hip.XZ2D_SHAPES)
XZ2D_FOLD_N = (64,)                               # radix-2 instances (hip.XZ2D_FOLD_N)
TOEPLITZ_NY = (16, 32, 48, 64, 80, 96, 112, 128)               # Toeplitz y-stage instances (hip.TOEPLITZ_NY)
SPECTRAL_AXIS_N = (80, 96, 112, 128)              # radix-4 axis passes (hip.SPECTRAL_AXIS_N); extents on the half-integer basis only
SPECTRAL_Y_NY = (32, 48, 64, 80, 96, 112, 128)    # in-kernel spectral y stage on the matrix pipe (hip.SPECTRAL_Y_NY); > 64: geobo_spectral_y3 only
TOEPLITZ_Y2T_NY = (32, 48, 64)                    # two-term y stage in one pass (geobo_toeplitz_y2t / _y2s; hip.TOEPLITZ_Y2T_NY)
TOEPLITZ_ADD_NY = (80, 96, 112, 128)              # accumulating y stage (geobo_toeplitz_y3_add; hip.TOEPLITZ_ADD_NY)
SPECTRAL_Y3T_NY = (80, 96, 112, 128)              # two-term long-axis spectral y stage (geobo_spectral_y3t; hip.SPECTRAL_Y3T_NY)
YMUL_SHAPES = ((128, 64),)                        # (m, k) geobo_ymul is instantiated for (hip.YMUL_SHAPES)
INTEGER_BASIS_N = (32, 64)                        # extents whose fused kernels (xz2d_fold.hip: n = 64 and the four-plane form of 32 x 32 planes) build the
                                                  # integer basis of spectral.base_modes() internally; every other extent: half_integer()
ROWS_MIN_VOXELS = 1 << 18                         # batched-GEMM forms of the row algorithm pay from 64^3 voxels ...
ROWS_MIN_PLANE = 96 * 96                          # ... and (x, z) planes that fill the 128 x 128 GEMM tiles
ROWS_MIN_VOXELS_MID, ROWS_MIN_PLANE_MID = 3 << 17, 64 * 64   # ... or from 393 216 voxels with planes of 4096 modes: 80^3 3345 / 4733 ms (52 / 183 GB),
                                                  # 80x64x80 2026 / 2503; at the old threshold 96x32x96 786 / 741; below: 80x32x80 528 / 414, 112x16x112 290 / 212,
                                                  # 16x128x128 462 / 367 (2048-mode planes), 48^3 237 / 188, 32x32x128 100 / 63
COLUMN_FORM_MAX_BYTES = 160 << 30                 # a two-property A K of the column form beyond this does not fit beside its workspaces (80x128x80:
                                                  # 272 GB, out of memory; row form 8.8 s in 63 GB)
ROWS_MIN_VOXELS_FUSED = 1 << 17                   # with fused / four-plane (x, z) kernels and the Toeplitz y stage: from 2^17 voxels.  Measured
                                                  # (row form / column form, ms per step, one MI355X): 64x32x64 107 / 138, 32x128x32 379 / 482,
                                                  # 64x64x32 369 / 484, 48x64x64 341 / 424, 64x80x64 877 / 1736, 64x128x64 2365 / 6670 (50 / 235 GB);
                                                  # below: 64x32x32 101 / 80, 48x32x64 89 / 69, 32x64x32 87 / 77, 64x16x64 35 / 33


# Every behaviour switch of a step, in ONE table: option -> the environment override that turns it off ("0").  They are resolved ONCE
# (switches(); a product built on its own resolves the process environment the same way) into the kernel forms of stage_forms(): the spectral
# product, the lattice Gram and the transposed posterior decide nothing.  The environment is also read for plan_route's family overrides
# (GEOBO_ROWS, GEOBO_POSTERIOR, GEOBO_SPECTRAL_EXCHANGE) and for the engine's own options (ENGINE_OPTIONS below).  All are
# A/B and fallback-coverage switches: the default of every option is "on", every "off" path a complete, tested form of the same arithmetic.
SWITCHES = {"fused_xz": "GEOBO_SPECTRAL_FUSED_XZ",   # fused (x, z) transform kernels (else two batched passes)
            "fold": "GEOBO_XZ_FOLD",                 # radix-2 / radix-4 transform kernels (else the plain products)
            "quad": "GEOBO_XZ_QUAD",                 # 32 x 32 planes four at a time through the n = 64 radix-2 kernels (else stacked pairs)
            "dense_y": "GEOBO_SPECTRAL_DENSE_Y",     # y axis applied per mode inside one kernel (else carried through the spectrum by passes)
            "y_mfma": "GEOBO_Y_MFMA",                # ... as an in-kernel spectral product on the matrix pipe (else the direct vector-pipe kernels)
            "axis_mfma": "GEOBO_AXIS_MFMA",          # x passes of the unfused (x, z) transforms as radix-4 axis kernels (else radix-2 GEMM passes)
            "y2s": "GEOBO_Y2S",                      # two-term rows with the shared cross block K_01 = K_10 (else four products)
            "z_fused": "GEOBO_Z_FUSED",              # rows of L^-1 A: one fused inverse transform per (row, z) plane (else two GEMM passes)
            "z_mul": "GEOBO_Z_MUL",                  # ... its input product formed inside the kernel (else written and read back)
            "z_lattice": "GEOBO_Z_LATTICE",          # rows of L^-1 A as lattice convolutions (else triangular GEMMs against the operator)
            "aka_lattice": "GEOBO_AKA_LATTICE"}      # AkA by the lattice Gram (else the N-deep GEMM)


def switches(env=None):
    """{option: bool} from an environment-like mapping (None: every option on)."""
    env = {} if env is None else env
    return {k: env.get(v, "1") != "0" for k, v in SWITCHES.items()}


# The options of an engine that the planner does NOT own (they change no route and no kernel form, so they stay out of SWITCHES and of
# the pinned route table): field -> (environment variable, default, parser of the variable's text).  Resolved ONCE per engine by
# engine_options(), from the same mapping that plan_route gets; nothing else in the package reads them.
_on = lambda v: v != "0"
ENGINE_OPTIONS = {"aka_mirror": ("GEOBO_AKA_MIRROR", True, _on),               # magnetic block of AkA: one half computed, the other mirrored
                  "z_spectrum": ("GEOBO_Z_SPECTRUM", True, _on),               # rows of L^-1 A enter the posterior as spectra (else stored rows)
                  "async_exchange": ("GEOBO_ASYNC_EXCHANGE", True, _on),       # row exchange overlapped with compute (else blocking)
                  "exchange_comm": ("GEOBO_EXCHANGE_COMM", "shared", str),     # "own": a second communicator for the row exchange
                  "force_collectives": ("GEOBO_FORCE_COLLECTIVES", False, lambda v: v == "1"),   # one-rank runs go through the backend
                  "row_chunk": ("GEOBO_ROW_CHUNK", 0, int),                    # rows per batch of the row form (0: from the memory budget; tests)
                  "potrf": ("GEOBO_POTRF", "auto", lambda v: "dag" if v[:1] == "d" else "streams")}   # schedule of hip.potrf_inv
EngineOptions = make_dataclass("EngineOptions", [(k, type(d)) for k, (_, d, _p) in ENGINE_OPTIONS.items()], frozen=True)


def engine_options(env=None):
    """EngineOptions from an environment-like mapping (None: every default)."""
    env = {} if env is None else env
    return EngineOptions(**{k: parse(env[var]) if var in env else default for k, (var, default, parse) in ENGINE_OPTIONS.items()})


# The hand-over between the A K product and the lattice Gram (engine._gram_feed): resolved once per engine from the same mapping, beside
# engine_options().  A table of its own: ENGINE_OPTIONS is pinned entry by entry (tests/test_host_logic_cpu.py::test_engine_options_table),
# like SWITCHES and Forms, and none of the three moves for it.
FEED_OPTIONS = {"gram_gx": ("GEOBO_GRAM_GX", True, _on)}      # the A K inverse transform emits the Gram's x analysis; the y spectrum is never stored
FeedOptions = make_dataclass("FeedOptions", [(k, type(d)) for k, (_, d, _p) in FEED_OPTIONS.items()], frozen=True)


def feed_options(env=None):
    """FeedOptions from an environment-like mapping (None: every default)."""
    env = {} if env is None else env
    return FeedOptions(**{k: parse(env[var]) if var in env else default for k, (var, default, parse) in FEED_OPTIONS.items()})


def gram_gx_route(opts, family, sym, f32, world, exchange, nx, ny, nz, forms):
    """Whether a step hands x-analysed rows from the A K product to the lattice Gram: the option, the symmetric plan of the one-rank
    `single` family, fp64 assembly, and 64 x 64 (x, z) planes on the radix-4 kernels with the dense y stage (what the two kernels,
    geobo_xz2d_fold_inv_gx and geobo_gram_yz, are instantiated for)."""
    return bool(opts.gram_gx and sym and family == "single" and not f32 and world == 1 and not exchange
                and nx == 64 and nz == 64 and ny % 2 == 0 and 4 <= ny <= 64
                and forms.xz == "fold" and forms.gram_x == "fold" and forms.y != "spectrum")


# Which rows give AkA's cross block (engine._assemble_AK_spectral, transposed._assemble_AkA_sym): resolved once
# per engine from the same mapping.  Again a table of its own: ENGINE_OPTIONS, SWITCHES, Forms and FEED_OPTIONS are pinned entry by entry.
CROSS_ROWS = ("auto", "magn", "grav")


def _cross_rows(v):
    if v not in CROSS_ROWS:
        raise ValueError("GEOBO_CROSS_ROWS must be one of %s, got %r" % (", ".join(CROSS_ROWS), v))
    return v


CROSS_OPTIONS = {"cross_rows": ("GEOBO_CROSS_ROWS", "auto", _cross_rows)}     # "magn": the mirrored half of the magnetic rows; "grav": all gravity rows
CrossOptions = make_dataclass("CrossOptions", [(k, type(d)) for k, (_, d, _p) in CROSS_OPTIONS.items()], frozen=True)


def cross_options(env=None):
    """CrossOptions from an environment-like mapping (None: every default)."""
    env = {} if env is None else env
    return CrossOptions(**{k: parse(env[var]) if var in env else default for k, (var, default, parse) in CROSS_OPTIONS.items()})


def cross_rows_route(opts, sym, mirror_rows, nx, ny, nz):
    """Whether a step builds AkA's cross block from the magnetic rows A_m K_10 it runs anyway: the symmetric plan with the magnetic
    point mirror taken (mirror_rows > 0: the operator measured as its own mirror), and the option.  "auto" takes it on the planner's
    cube only (nx = ny = nz = 64, the grids of Forms.zx) -- a restriction of the roll-out, not of the method."""
    if not (sym and mirror_rows) or opts.cross_rows == "grav":
        return False
    return opts.cross_rows == "magn" or nx == ny == nz == 64


# AkA's gravity block from half its rows (engine._grav_mirror_rows, transposed._assemble_AkA_sym; DESIGN.md section 2, "gravity block
# from half its rows"): resolved once per engine from the same mapping, in a table of its own like the two above.
GRAV_MIRROR = ("auto", "on", "off")


def _grav_mirror(v):
    if v not in GRAV_MIRROR:
        raise ValueError("GEOBO_GRAV_MIRROR must be one of %s, got %r" % (", ".join(GRAV_MIRROR), v))
    return v


GRAV_OPTIONS = {"grav_mirror": ("GEOBO_GRAV_MIRROR", "auto", _grav_mirror)}     # "on": wherever the gate holds; "off": every gravity row runs
GravOptions = make_dataclass("GravOptions", [(k, type(d)) for k, (_, d, _p) in GRAV_OPTIONS.items()], frozen=True)


def grav_options(env=None):
    """GravOptions from an environment-like mapping (None: every default)."""
    env = {} if env is None else env
    return GravOptions(**{k: parse(env[var]) if var in env else default for k, (var, default, parse) in GRAV_OPTIONS.items()})


def grav_mirror_route(opts, sym, static, handover, pooled, even, alone, nx, ny, nz):
    """Whether a step builds the interior part of AkA's gravity block from the first half of the gravity rows and mirrors the rest.
    The gate is a set of conditions, none of them a tuning value: the symmetric plan (sym); the static conditions of the point
    mirror (static: engine._mirror_static held when the operator was built); the A K product hands its rows to the lattice Gram
    (handover: engine._gram_feed applies) and can feed interior and boundary planes apart (pooled: the plane pool of an implicit
    operator, or resident fp64 rows copied with their boundary planes zeroed -- the same operands, the same bits); the gravity stencil table passed the Gram's evenness check (even: LatticeGram.eigen returned eigen-data -- evenness in
    both offsets implies point evenness); the gravity rows run block K_00 alone (alone: the cross block comes from the magnetic
    rows, cross_rows_route -- block K_01 of the gravity rows would need every row whole).  The boundary slabs are not asked anything:
    their terms are computed with no symmetry assumed.  "auto" takes it on the planner's cube only (nx = ny = nz = 64), the
    roll-out convention of cross_rows_route."""
    if opts.grav_mirror == "off" or not (sym and static and handover and pooled and even and alone):
        return False
    return opts.grav_mirror == "on" or nx == ny == nz == 64


def half_integer(n):
    """True where the axis runs on the HALF-INTEGER (skew-circulant) basis (round 6): a symmetric Toeplitz block of size n is also the
    leading block of the skew-circulant of size P = 2n (first column k_0 .. k_{n-1}, *, -k_{n-1} .. -k_1), diagonalised by cos / sin of
    the frequencies kappa = 1/2 .. n - 1/2 with eigenvalues sum_d w_d k(d) cos(2 pi kappa d / P).  No frequency is its own mirror or
    quarter-period image, so all n frequencies fall into n/4 orbits {kappa, n - kappa, n/2 + kappa, n/2 - kappa} of ONE shape -- what
    the radix-4 axis kernels of spectral_y.hip want.  Every consumer of G / G^T / E treats the spectral index as opaque (the eigen-data
    go through the same matrices), and the pair structure row 2b+1 = (-1)^i row 2b of the radix-2 passes holds for every pair."""
    return n not in INTEGER_BASIS_N


@dataclass(frozen=True)
class Forms:
    """Which kernel form carries each stage of the spectral route on one grid (stage_forms): what SpectralProduct and LatticeGram run on."""
    xz: str              # (x, z) transform of the covariance product: "fold" (radix-2 / radix-4 fused kernels) | "fused" (plain fused kernel) |
                         # "quad" | "pair" (32 x 32 planes by fours on the radix-2 / by pairs on the (64, 32) fused kernel) | "gemm" (two passes).
                         # Per call the eigen-matrices take the plain twin (fold -> fused, quad -> pair); odd slabs step down quad -> pair -> gemm
    x_axis4: bool        # the x passes of "gemm" (and the x synthesis of the lattice rows) as radix-4 axis kernels (geobo_spectral_axis)
    y: str               # "mfma" (in-kernel spectral product on the matrix pipe) | "toeplitz" (direct vector-pipe kernels) | "spectrum" (by passes)
    y_two_term: str      # two-term rows: "y2t" (one pass for both terms) | "add" (the second term accumulates) | "separate" (two spectra, summed later)
    y3t: bool            # ... "add" in one pass of the long-axis spectral kernel (geobo_spectral_y3t)
    y2s: bool            # ... "y2t" with the shared cross block K_01 = K_10: three products instead of four
    fold: bool           # the radix-2 switch as the batched passes see it (hip.axis_pass)
    ss: str              # posterior sums of squares: "fused" (inside the inverse transform) | "stored" (a batch of V rows, then geobo_sumsq_accum)
    lattice_feed: bool   # operator rows read from a lattice survey's stencil table by the radix-2 forward kernel
    plane_yx: str        # the (ny, nx) two-axis transform of the lattice Gram / lattice rows: "fold" | "fused" | "gemm"
    gram_x: str          # the Gram's x step: "fold" (geobo_xcorr_reduce_fold) | "plain" (geobo_xcorr_reduce) | "fold_lamdot" | "gemm"
    gram_y_axis4: bool   # the Gram's y step over the whole axis as a radix-4 axis kernel
    zx: bool             # rows of L^-1 A by one fused inverse transform per (row, z) plane, written as [iy][iz][ix]
    z_mul: bool          # ... its input product formed inside the kernel
    ymul_slabs: tuple    # slab heights whose Gram y step runs on geobo_ymul

    def folded_axes(self):                # axes whose folded (radix-2) matrices some stage of this record reads
        xz = self.xz == "fold" or self.lattice_feed or self.ss == "fused"
        return tuple(a for a, used in (("x", xz or self.gram_x == "fold" or self.plane_yx == "fold"), ("y", self.plane_yx == "fold"), ("z", xz)) if used)


def stage_forms(nx, ny, nz, opts=None):
    """The kernel form of every stage on one grid; opts: {option: bool} of switches() (None: all on).  Priority: the order of each chain."""
    sw = switches(None) if opts is None else opts
    fold, fused = sw["fold"], (nx, nz) in XZ2D_SHAPES and sw["fused_xz"]
    folds = lambda a, b: fold and a == b and a in XZ2D_FOLD_N              # a square (a, b) plane on the radix-2 kernels
    pair = (nx, nz) == (32, 32) and (64, 32) in XZ2D_SHAPES and ny % 2 == 0 and sw["fused_xz"]
    quad = pair and ny % 4 == 0 and fold and 64 in XZ2D_FOLD_N and sw["quad"]
    xz = "fold" if (fused and folds(nx, nz)) else "fused" if fused else "quad" if quad else "pair" if pair else "gemm"
    axis4 = lambda n: n in SPECTRAL_AXIS_N and half_integer(n) and sw["axis_mfma"]
    dense_y = ny in TOEPLITZ_NY and sw["dense_y"]
    y = "spectrum" if not dense_y else "mfma" if (ny in SPECTRAL_Y_NY and sw["y_mfma"]) else "toeplitz"
    y_two_term = "y2t" if ny in TOEPLITZ_Y2T_NY else "add" if ny in TOEPLITZ_ADD_NY else "separate"
    fused_ss = xz == "fold" and dense_y                  # (any Toeplitz ny: the reduction in the inverse transform takes any plane count)
    zx = nx == ny == nz == 64 and folds(ny, nx) and sw["z_fused"]
    return Forms(xz=xz, x_axis4=axis4(nx), y=y, y_two_term=y_two_term, y3t=y == "mfma" and ny in SPECTRAL_Y3T_NY,
                 y2s=fused_ss and y_two_term == "y2t" and sw["y2s"], fold=fold, ss="fused" if fused_ss else "stored", lattice_feed=fused_ss and ny >= 3,
                 plane_yx="fold" if folds(ny, nx) else "fused" if (ny, nx) in XZ2D_SHAPES else "gemm",
                 gram_x="fold" if folds(nx, nz) else "plain" if (nx, nz) == (64, 64) else "fold_lamdot" if (fold and nz <= 128) else "gemm",
                 gram_y_axis4=axis4(ny), zx=zx, z_mul=zx and sw["z_mul"], ymul_slabs=tuple(k for m, k in YMUL_SHAPES if m == 2 * ny))


def _pad(v, m):
    return (int(v) + m - 1) // m * m


def shard_columns(n_pad, world, rank):
    units = n_pad // PAD_N
    return units * rank // world * PAD_N, units * (rank + 1) // world * PAD_N


@dataclass(frozen=True)
class Route:
    spectral: bool          # A K through the real-DFT route (regular grid, extents % 16, unpadded voxels, slab-aligned shards)
    family: str             # "rows" | "single" | "columns": what the engine attempts (a survey off the lattice demotes to "columns")
    rows: bool              # the row form is statically possible
    single: bool            # the one-rank fused-kernel form is statically possible
    exchange: bool          # column form: row-sharded transforms + all-to-all of A K block columns
    exchange_without_rows: bool   # ... when the row form is denied at operator-build time (off-lattice survey, uneven stencil)
    operators: str          # "resident" | "streamed" | "auto" as requested, resolved to "streamed" where residency cannot fit
    kernels: tuple          # (("xz", ...), ("y", ...), ("gram", ...), ("ss", ...)): which implementation carries each stage
    note: str               # why a faster family stepped aside for this shape ("" when nothing did)
    ak_bytes: int = 0       # what a materialised A K (column form / one-rank fused form) of this rank would take
    rows_mandatory: bool = False   # ak_bytes > COLUMN_FORM_MAX_BYTES: only the row form fits; a denied row form is an error, not a fallback
    switches: tuple = ()    # ((option, bool), ...) of SWITCHES as resolved from the environment handed to plan_route
    forms: object = None    # Forms: the record `kernels`, `single` and `rows` were derived from; what the spectral product and the lattice Gram run on

    def opt(self, name):
        return dict(self.switches).get(name, True)

    def opts(self):
        return dict(switches(None), **dict(self.switches))

    def describe(self):
        k = dict(self.kernels)
        return "%s/%s xz=%s y=%s gram=%s ss=%s%s" % ("spectral" if self.spectral else "dense", self.family, k["xz"], k["y"], k["gram"],
                                                      k["ss"], " exchange" if self.exchange and self.family == "columns" else "")

    def as_dict(self):
        d = asdict(self)
        d["kernels"] = dict(self.kernels)
        d["switches"] = dict(self.switches)
        return d


def lattice_gram_fast(nx, ny, nz):
    """Grids whose Gram x step / back-transform run on the fused kernels (lattice_gram.LatticeGram.fast)."""
    return nx == 64 and nz == 64 and ny in (48, 64)


def lattice_gram_supported(nx, ny, nz):
    return nx % 16 == 0 and ny % 16 == 0 and nz % 16 == 0 and ny >= 16


def plan_route(nx, ny, nz, world=1, rank=0, assembly="f64", operators="resident", method="auto", env=None, nprops=2):
    env = {} if env is None else env
    sw = switches(env)
    nx, ny, nz, world = int(nx), int(ny), int(nz), int(world)
    N, Ms = nx * ny * nz, nx * ny
    N_pad, Ms_pad = _pad(N, PAD_N), _pad(Ms, PAD_M)
    plane = nx * nz
    f32, streamed = assembly == "f32", operators == "streamed"
    notes = []
    # slab alignment is decided over ALL ranks' shards (round-4 advisory: decided per rank, 16^3 on 3 / 5 / 6 / 7 ranks gave some ranks
    # the spectral route and others the dense one -- same collectives, different arithmetic and bench lines per rank)
    shards = [shard_columns(N_pad, world, r) for r in range(world)]
    aligned = all(c0 % plane == 0 and c1 % plane == 0 and c1 > c0 for c0, c1 in shards)
    spectral = (method in ("auto", "spectral") and nx % 16 == 0 and ny % 16 == 0 and nz % 16 == 0 and N == N_pad and aligned)
    forms = stage_forms(nx, ny, nz, sw)
    fused_ss, dense_y, fast_xz = forms.ss == "fused", forms.y != "spectrum", forms.xz in ("fold", "fused", "quad")
    transposed = env.get("GEOBO_POSTERIOR", "zpath") == "zpath"
    unpadded = Ms == Ms_pad and N == N_pad
    gram_ok = lattice_gram_supported(nx, ny, nz) and sw["aka_lattice"]
    gram_fast = lattice_gram_fast(nx, ny, nz)
    single = world == 1 and not f32 and spectral and unpadded and transposed and fused_ss
    rows_mode = env.get("GEOBO_ROWS", "auto")           # "0": never; "1": wherever it is possible; "auto": where it pays
    # a materialised A K of this rank: nprops property blocks in the element size of the assembly (fp32 assembly stores A K as fp32); the
    # engine repeats the check with the step's own property count where it allocates (engine._assemble_AK)
    column_ak_bytes = (2 * Ms_pad + PAD_M) * int(nprops) * N_pad * (4 if f32 else 8) // max(world, 1)
    pays = ((gram_fast and fused_ss) or (fast_xz and dense_y and N >= ROWS_MIN_VOXELS_FUSED)
            or (N >= ROWS_MIN_VOXELS and plane >= ROWS_MIN_PLANE) or (N >= ROWS_MIN_VOXELS_MID and plane >= ROWS_MIN_PLANE_MID)
            or column_ak_bytes > COLUMN_FORM_MAX_BYTES)
    xmode = env.get("GEOBO_SPECTRAL_EXCHANGE", "auto")    # "0": replicated forward transforms, column shards (also switches the row form off for N > 1)
    rows = (spectral and unpadded and Ms % world == 0 and gram_ok and transposed and sw["z_lattice"] and rows_mode != "0"
            and (pays or rows_mode == "1") and not (single and gram_fast and rows_mode != "1") and (world == 1 or xmode != "0" or rows_mode == "1"))
    ncs = {shard_columns(N_pad, world, r)[1] - shard_columns(N_pad, world, r)[0] for r in range(world)}
    xbase = spectral and world > 1 and Ms % world == 0 and len(ncs) == 1 and xmode != "0"
    exchange_without_rows = xbase and (world >= 4 or xmode == "1")
    exchange = xbase and (world >= 4 or xmode == "1" or rows)
    family = "rows" if rows else ("single" if single else "columns")
    if spectral and family == "columns" and transposed:
        if not unpadded:
            notes.append("nx*ny = %d is not a multiple of %d (padded sensor rows): fused reduction L^-1 (A K) instead of the transposed order" % (Ms, PAD_M))
        elif not pays:
            notes.append("the structured algorithm pays from %d voxels with fused (x, z) kernels and from %d voxels with (x, z) planes of %d "
                         "modes (%d with %d) on the batched-GEMM forms (here %d x %d x %d: %d voxels, %d modes, %s (x, z) kernels): N-deep Gram "
                         "and fused reduction (2-6x the work of the structured forms at larger sizes)"
                         % (ROWS_MIN_VOXELS_FUSED, ROWS_MIN_VOXELS, ROWS_MIN_PLANE, ROWS_MIN_VOXELS_MID, ROWS_MIN_PLANE_MID, nx, ny, nz, N, plane,
                            "fused" if fast_xz else "no fused"))
        elif world > 1 and Ms % world:
            notes.append("%d sensor rows do not divide over %d ranks: column shards" % (Ms, world))
    if not spectral and method == "auto" and (nx % 16 or ny % 16 or nz % 16):
        notes.append("grid extents %d x %d x %d are not multiples of 16: dense route (2 Ms N^2 flop per block pair)" % (nx, ny, nz))
    # operator residency: one operator is Ms_pad x N_pad doubles; in the row form a rank only ever needs its rows + two boundary slabs
    ops = operators
    rows_r = Ms // world if Ms % world == 0 else Ms
    if family == "rows" and not streamed and rows_r * N_pad * 8 > (40 << 30):
        ops = "streamed"
        notes.append("operator rows of a rank (%.0f GB) are generated per batch instead of being resident" % (rows_r * N_pad * 8 / 1e9))
    kernels = (("xz", "gemm+axis4" if (forms.xz == "gemm" and forms.x_axis4) else forms.xz), ("y", forms.y),
               ("gram", ("fused" if gram_fast else "gemm") if (family in ("rows", "single") and gram_ok) else "per-step"),
               ("ss", ("fused" if fused_ss else "stored") if family in ("rows", "single") else "reduction"))
    if column_ak_bytes > COLUMN_FORM_MAX_BYTES and family != "rows":
        notes.append("a materialised A K of this grid takes %.0f GB per rank (limit %.0f): only the row form fits, and it is %s"
                     % (column_ak_bytes / 1e9, COLUMN_FORM_MAX_BYTES / 1e9, "switched off (GEOBO_ROWS=0)" if rows_mode == "0" else "not available here"))
    return Route(spectral=spectral, family=family, rows=rows, single=single, exchange=exchange, exchange_without_rows=exchange_without_rows,
                 operators=ops, kernels=kernels, note="; ".join(notes), ak_bytes=int(column_ak_bytes),
                 rows_mandatory=bool(column_ak_bytes > COLUMN_FORM_MAX_BYTES), switches=tuple(sorted(sw.items())), forms=forms)
