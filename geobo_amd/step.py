"""What one step of PosteriorEngine is made from, as two values handed from stage to stage instead of engine attributes:

  Prior   the covariance of a step -- create_cov's 3 x 3 block kernel (kernels.py:158-195), or its directional derivative in the three
          lengths (PosteriorEngine.logl_grad) -- and the three ways the assembly evaluates one of its blocks
  Step    what one assembly was asked for (prior, property blocks, drill rows, noise, workspace slots), what it decided (sym, rowpath)
          and what it left for the later stages (gens, fullrows)

Nothing here needs torch or a device at import; the evaluators take the engine whose workspaces and grid they use."""
from dataclasses import dataclass, field


class Prior:
    """Block (row property i, column property j) of create_cov is w_ij k(l1 = l_j, l2 = l_i) (kernels.py:183-195): ONE term.
    deriv = d: the derivative of that block along the direction d in the three lengths, w_ij (d_j dk/dl1 + d_i dk/dl2); a self block
    has one length: w d_j dk/dl.  The blocks (i, j) and (j, i) stay transposes of each other (k_ij(a, b) = k_ji(b, a)), so a
    derivative Gram is symmetric and runs through every route of the assembly unchanged.
    `lengths` carry the create_cov mutation; W is the 3 x 3 weight matrix (engine.weight_matrix)."""

    def __init__(self, name, lengths, W, amp, deriv=None):
        self.name, self.lengths, self.W, self.amp = name, lengths, W, amp
        self.deriv = None if deriv is None else [float(v) for v in deriv]

    def terms(self, i, j):
        """[(kernel id, weight)] whose sum is block (i, j)."""
        from .hip import kernel_id
        w, d = self.W[i][j], self.deriv
        if d is None:
            return [(kernel_id(self.name, i != j), w)]
        if i == j:
            return [(kernel_id(self.name, False, 1), w * d[j])]
        return [(kernel_id(self.name, True, 1), w * d[j]), (kernel_id(self.name, True, 2), w * d[i])]

    def table(self, eng, i, j):
        """Lattice table of block (i, j) on the engine's grid (each term rounded through fp32 in the fp32-assembly mode)."""
        tabs = [eng._cov_table(kid, self.lengths[j], self.lengths[i], w, self.amp) for kid, w in self.terms(i, j)]
        for t in tabs[1:]:
            tabs[0].add_(t)
        return tabs[0]

    def k_block(self, eng, i, j, rows, cols, out):
        """Block (i, j) evaluated from coordinates (geobo_k_block)."""
        from . import hip
        terms = self.terms(i, j)
        hip.k_block(terms[0][0], rows, cols, self.lengths[j], self.lengths[i], terms[0][1], self.amp, out)
        for kid, w in terms[1:]:
            tmp = eng._workspace2d("dcov_tmp", out.shape[0], out.shape[1])
            hip.k_block(kid, rows, cols, self.lengths[j], self.lengths[i], w, self.amp, tmp)
            out.add_(tmp)
        return out

    def ak_fused(self, eng, s, j, A, xyz, nc, out):
        """A_s K_sj with the covariance generated inside the fused product (coordinate route)."""
        from . import hip
        terms = self.terms(s, j)
        hip.ak_fused(terms[0][0], A, xyz, eng.c0, nc, self.lengths[j], self.lengths[s], terms[0][1], self.amp, out)
        for kid, w in terms[1:]:
            tmp = eng._workspace2d("dak_tmp", out.shape[0], nc)
            hip.ak_fused(kid, A, xyz, eng.c0, nc, self.lengths[j], self.lengths[s], w, self.amp, tmp)
            out[:, :nc].add_(tmp)
        return out

    def ak_points(self, eng, s, j, A, q_xyz, out):
        """A_s K_sj(grid, Q) for the column points q_xyz (padded SoA in the covariance frame): the same product off the grid."""
        from . import hip
        terms = self.terms(s, j)
        xyz = eng.grid_points()
        hip.ak_points(terms[0][0], A, xyz, q_xyz, self.lengths[j], self.lengths[s], terms[0][1], self.amp, out)
        for kid, w in terms[1:]:
            tmp = eng._workspace2d("dak_points_tmp", out.shape[0], out.shape[1])
            hip.ak_points(kid, A, xyz, q_xyz, self.lengths[j], self.lengths[s], w, self.amp, tmp)
            out.add_(tmp)
        return out


@dataclass
class Step:
    """One assembly A K -> AkA and what follows it.  Rows of AkA: [grav | magn | drill | pad], M_pad of them, Md drill rows at the
    voxels sel_t (int64 device tensor, None without drill rows)."""
    prior: Prior
    props: tuple
    sel_t: object
    Md: int
    M_pad: int
    noise: object = None        # gp_sigma (3,); None: a derivative Gram -- no noise diagonal, zero padding
    ak_slot: str = "AK"         # workspaces of A K and AkA (a derivative Gram keeps its own beside the step's)
    aka_slot: str = "AkA"
    keep_signal: bool = False   # copy AkA before its diagonal into workspace "K_signal" (the signal part of K: logl_grad)
    row_scale: object = None    # the engine's committed row scales for this step's rows (reweight._step_row_scale); None: all ones
    # decided by the A K assembly
    sym: bool = False           # only the blocks of A K that AkA's lower triangle needs (transposed order on a lattice survey)
    rowpath: bool = False       # the row-sharded form: no A K at all
    mirror: int = 0             # > 0 (sym only): magnetic rows the assembly runs; the rest of AkA's magnetic block is their point mirror
    cross_rows: str = "grav"    # rows behind AkA's cross block: "grav" (A_g K_01, all rows) | "magn" (A_m K_10, the step.mirror rows; plan.cross_rows_route)
    grav_mirror: int = 0        # > 0 (sym only): gravity rows whose interior part A_i K the assembly runs (plan.grav_mirror_route); 0: all rows, whole
    # left for the later stages
    gens: dict = field(default_factory=dict)        # Toeplitz generators of the covariance blocks (s, j)
    fullrows: dict = field(default_factory=dict)    # column form with the row exchange: this rank's whole rows of A K
    gram_S: dict = field(default_factory=dict)      # (s, j) -> the lattice Gram's scaled spectra of the block's rows (engine._gram_feed)
    grav_slabs: object = None                       # grav_mirror: planes 0 and ny-1 of A_s K_00, [Ms][2 nx nz] (engine._assemble_AK_spectral)
    grav_iplanes: object = None                     # grav_mirror: planes 0 and ny-1 of A_i K_00, [Ms][2 nx nz], the run rows stored, the rest mirrored in AkA
    ak_fill: list = field(default_factory=list)     # storing products that write the interior planes of A K the hand-over skipped (run by
                                                    # engine.last's completion hook, on the first read of the buffer)
