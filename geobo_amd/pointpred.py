"""Prediction at arbitrary points inside the cube: the mixin of engine.PosteriorEngine.

The prior covariance is a function of position, so the posterior of the three properties at query points Q that are no voxels
follows from the factor of the last posterior() step exactly as on the grid:

    C*_a = A3 K_{.a}(grid, Q)        (M x Q)   rows [A_g K_0a | A_m K_1a | K_2a(P_sel, Q)]
    V*_a = L^-1 C*_a
    mean_a = V*_a^T u,   cov_ab(Q, Q) = K_ab(Q, Q) - V*_a^T V*_b

The sensor rows of C* are geobo_ak_points -- the fused product A K with the covariance generated inside the fp64-MFMA contraction,
its column points taken from Q instead of the voxel set -- the drill rows geobo_k_block, mean and variance geobo_posterior_reduce
(V* is not stored unless the joint covariance is asked for).  Q is in the covariance frame, the frame of grid_points(): voxel
(ix, iy, iz) sits at ((ix + 1) sx, (iy + 1) sy, (iz + 1) sz).

Raw values are returned: the reference's matern32 prior is slightly indefinite, so a variance may come out slightly negative
and nothing is clipped.
"""
import torch

from . import hip

F64 = hip.F64
STREAM_ROWS_BYTES = 4 << 30     # row-batch buffer of a streamed operator in predict_points (the default batch of _operator_rows: 256 rows)


class PointPredictionMixin:
    def predict_points(self, q_xyz, kernelfunc, lengths, crossweights, gp_amp, full_cov=False, batch=4096, limit_bytes=48 << 30,
                       op_rows=None):
        """Posterior of the three properties at the points q_xyz (three device vectors of Q coordinates in the covariance frame), from
        the factor of the last posterior() step: device tensors mean (3, Q) and var (3, Q), and with full_cov also the joint
        covariance (3Q, 3Q) ordered [property][point] (symmetric; MemoryError above limit_bytes).  Normalised units, raw values.
        `lengths` carry the create_cov mutation.  The queries run in batches of `batch` points (rounded up to the column unit);
        op_rows: rows per batch of a streamed operator (a multiple of 128; default: what a STREAM_ROWS_BYTES buffer holds).
        One rank, fp64 assembly, a step over property blocks (0, 1, 2)."""
        from .engine import weight_matrix
        from .step import Prior
        if self.world > 1:
            raise NotImplementedError("point prediction runs on one rank (world = %d)" % self.world)
        if self.f32:
            raise NotImplementedError("point prediction needs the fp64 assembly")
        last = self.last
        if last is None or tuple(last["props"]) != (0, 1, 2):
            raise RuntimeError("predict_points() needs the factor of a posterior() step over all three property blocks")
        try:
            qx, qy, qz = q_xyz
        except (TypeError, ValueError):
            raise ValueError("q_xyz is three device vectors (x, y, z) of equal length") from None
        for t in (qx, qy, qz):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == F64 and t.dim() == 1 and t.numel() == qx.numel()):
                raise ValueError("q_xyz is three float64 device vectors (x, y, z) of equal length")
        if qx.numel() < 1 or int(batch) < 1:
            raise ValueError("predict_points() needs at least one point and batch >= 1")
        if op_rows is not None and (int(op_rows) < 128 or int(op_rows) % 128):
            raise ValueError("op_rows must be a multiple of 128, got %r" % (op_rows,))
        with torch.cuda.device(self.device):
            return self._predict_points((qx, qy, qz), Prior(kernelfunc, lengths, weight_matrix(crossweights), float(gp_amp)), bool(full_cov),
                                        hip.pad_n(batch), int(limit_bytes), None if op_rows is None else int(op_rows))

    def _points_op_batch(self, op_rows=None):
        """(rows per batch of a streamed operator, workspace slot of the batch) for _points_columns; None: what a STREAM_ROWS_BYTES
        buffer holds in whole 256-row tiles."""
        if op_rows is None:
            op_rows = min(self.Ms_pad, max(256, STREAM_ROWS_BYTES // (8 * self.N_pad) // 256 * 256))
        return op_rows, "cond_op_rows" if op_rows == 256 else "points_op_rows"

    def _points_columns(self, prior, qb, blocks, Cb, sel_xyz, Md, op_rows, slot, n_valid):
        """Cb[i] = C*_a = A3 K_{.a}(grid, Q) for a = blocks[i] and the column points qb (a whole number of 128-point units): the
        sensor rows through geobo_ak_points against the row batches of the last step's operators, the Md drill rows (voxel
        coordinates sel_xyz) through geobo_k_block, zero behind them.  Cb[i]: (M_pad x len(qb)) views.  n_valid: the points that
        are no padding (flop accounting only).  predict_points and append_drill_rows (append.py) share it."""
        Msp = self.Ms_pad
        off_d = 2 * Msp
        nb = qb[0].numel()
        for s_, A in enumerate(self.last["ops"]):
            # operator rows as condition() reads them: zero padded, so the padding rows of C* come out zero
            for r0, rows in self._operator_rows(A, op_rows, slot):
                R = rows.shape[0]
                for a, C_a in zip(blocks, Cb):
                    out = C_a[s_ * Msp + r0:s_ * Msp + r0 + R]
                    self._timed("points_ak", 2.0 * R * self.N_pad * nb, lambda: prior.ak_points(self, s_, a, rows, qb, out),
                                alg=2.0 * min(R, self.Ms - r0) * self.N * n_valid)
        for a, C_a in zip(blocks, Cb):
            C_a[off_d + Md:].zero_()
            if Md:
                prior.k_block(self, 2, a, sel_xyz, qb, C_a[off_d:off_d + Md])

    def _predict_points(self, q_xyz, prior, full_cov, batch, limit_bytes, op_rows):
        dev, last = self.device, self.last
        Linv, u = last["Linv"], last["u"]
        sel_t = last["step"].sel_t
        Md = 0 if sel_t is None else int(sel_t.numel())
        M_pad, Msp = Linv.shape[0], self.Ms_pad
        off_d = 2 * Msp
        Mv = off_d + Md                                       # rows behind Mv are zero padding
        Q = q_xyz[0].numel()
        Qp = hip.pad_n(Q)
        if full_cov:
            need = 8 * (2 * 3 * M_pad * Qp + 2 * (3 * Qp) ** 2)          # V*, its transpose, the matrix and its mirror
            if need > limit_bytes:
                raise MemoryError("the joint covariance of %d points needs %d bytes (limit %d); ask for fewer points or for the "
                                  "variances alone" % (Q, need, limit_bytes))
        # the query set padded with copies of its last point: finite columns that are never returned
        qp = tuple(torch.cat([c, c[-1:].expand(Qp - Q)]).contiguous() for c in q_xyz)
        batch = min(batch, Qp)
        xyz = self.grid_points()
        sel_xyz = tuple(c[sel_t] for c in xyz) if Md else None
        mean = torch.empty((3, Qp), dtype=F64, device=dev)
        var = torch.empty((3, Qp), dtype=F64, device=dev)
        V = torch.empty((3, M_pad, Qp), dtype=F64, device=dev) if full_cov else None
        C = self._workspace("points_C", (3, M_pad, batch + 16))
        ws = self._workspace("points_post_ws", (hip.posterior_ws_doubles(M_pad, batch),))
        # a streamed operator: each row batch is generated once per query batch and serves the three properties.  256 rows x one
        # query batch are a few dozen workgroups per launch, so the batch grows to what a fixed buffer holds (whole 256-row tiles)
        op_rows, slot = self._points_op_batch(op_rows)
        # executed flop of the reduction: as posterior() counts them (triangular L^-1, 64-row groups)
        tri = sum(64.0 * 64 * g + 2560.0 for g in range((Mv + 63) // 64))
        for b0 in range(0, Qp, batch):
            nb = min(batch, Qp - b0)
            qb = tuple(c[b0:b0 + nb] for c in qp)
            Cb = [C[a][:, :nb] for a in range(3)]
            self._points_columns(prior, qb, (0, 1, 2), Cb, sel_xyz, Md, op_rows, slot, min(nb, max(Q - b0, 0)))
            for a in range(3):
                m_a, v_a = self._timed("points_reduce", 2.0 * nb * tri, lambda: hip.posterior_reduce(
                    Linv, Cb[a], u, prior.W[a][a] * prior.amp, ws, m_valid=Mv))
                mean[a, b0:b0 + nb], var[a, b0:b0 + nb] = m_a, v_a
                if full_cov:
                    self._timed("points_cov", 2.0 * nb * tri, lambda: hip.gemm_nn(Linv, Cb[a], V[a][:, b0:b0 + nb], x_lower=True))
        if not full_cov:
            return mean[:, :Q], var[:, :Q]

        def joint():
            Vt = V.permute(0, 2, 1).reshape(3 * Qp, M_pad)     # rows [property][point]
            S = torch.empty((3 * Qp, 3 * Qp), dtype=F64, device=dev)
            for i in range(3):
                for j in range(3):
                    prior.k_block(self, i, j, qp, qp, S[i * Qp:(i + 1) * Qp, j * Qp:(j + 1) * Qp])
            return hip.gemm_nt(Vt, Vt, S, alpha=-1.0, beta=1.0)
        S = self._timed("points_cov", 2.0 * M_pad * (3 * Qp) ** 2, joint)
        del V
        idx = torch.cat([torch.arange(Q, device=dev) + a * Qp for a in range(3)])
        S = S[idx][:, idx]
        # one triangle, mirrored: blocks (a, b) and (b, a) are evaluated with their lengths in the other order
        S = torch.tril(S)
        cov = S + torch.tril(S, -1).t()
        return mean[:, :Q], var[:, :Q], cov
