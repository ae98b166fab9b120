"""New drill rows behind the last row of a factorised K_y, without a new step: mixin of engine.PosteriorEngine.

New drill observations always go behind the last drill row of K_y = A3 K A3^T + Sigma, so the factor of the larger matrix is the old
one with k rows added at the bottom; the leading part of L, of L^-1 and of u = L^-1 y stays bit for bit.  For k distinct voxels P that
carry no drill row yet and their values y_P (normalised units):

    B = A3 K[:, (2, P)]                 (Mv x k)   rows [A_g K_02(grid, P) | A_m K_12(grid, P) | K_22(sel, P)]: C*_2 of pointpred.py
    W = L^-1 B,   S = K_22(P, P) + sigma_d^2 I - W^T W = Ls Ls^T,   T = Ls^-1        (geobo_factor_append, one workgroup, k <= 128)
    new rows of L:     [W^T | Ls]
    new rows of L^-1:  [-T W^T L^-1 | T]
    u_P = T (y_P - W^T u),    uu += |u_P|^2,    logdet += 2 sum log diag Ls
    V_P = the new rows of V = L^-1 A3 K, from the new rows of L^-1 through the tile generators of information.py
    mu += V_P^T u_P,    var -= sum_r V_P[r, :]^2                                      (geobo_rows_downdate)

More than 128 voxels go through in chunks; every chunk is exact, so chained appends are.  Everything of a chunk is computed into
scratch first and the engine's buffers are written once its status word has come back 0: a failed pivot leaves the engine as it was.
truncate_drill_rows drops appended rows again (identity padding returns; every buffer a step over the remaining rows would hold has
the bits it had before the append).
"""
import math

import numpy as np
import torch

from . import hip

F64 = hip.F64
APPEND_K_MAX = 128


class AppendRowsMixin:
    def _append_ready(self, what):
        """The conditions of set_statistics, with its errors; returns (last, A K or its partial form or None)."""
        if self.world > 1:
            raise NotImplementedError("%s runs on one rank (world = %d)" % (what, self.world))
        last = self.last
        if last is None or tuple(last["props"]) != (0, 1, 2):
            raise RuntimeError("%s needs the factor of a posterior() step over all three property blocks" % what)
        AK = last["AK"] if last["AK_complete"] else last["AK_partial"]
        if self.f32 or (AK is not None and AK.dtype != F64):
            raise NotImplementedError("%s needs the fp64 assembly" % what)
        return last, AK

    def _append_state(self, last):
        """What the appends of one step carry beside the factor: the drill rows the step itself had (Md0), the two likelihood
        statistics and the (3, N) device mean and variance at the current row count (mu None: not formed yet, or `lost`: rows went
        in or out without them), and one snapshot of the four per append call, taken at its entry -- snaps[Md] is the state with Md
        rows, what truncate_drill_rows(Md) and a failed call restore."""
        st = last.get("append")
        if st is None:
            st = last["append"] = dict(Md0=last["step"].Md, uu=last.get("uu"), logdet=last.get("logdet"), mu=None, var=None, lost=False, snaps={})
        return st

    def mean_var_known(self):
        """Whether append_drill_rows(want_mean_var=True) has a mean and variance to start from: the step's own, or those the appends
        since have carried."""
        last = self.last
        if last is None:
            return False
        st = last.get("append")
        if st is None:
            return last.get("mv") is not None
        return st["mu"] is not None or (not st["lost"] and last.get("mv") is not None)

    def _append_mean_var(self, last, st, mean_var):
        """The (3, N) device mean and variance the downdates run on: carried from the last append, else the step's own (posterior()
        keeps them on the device), else the caller's host vectors `mean_var` = (mu, var), 3N each, property-major."""
        if st["mu"] is not None:
            return
        if st["lost"]:
            raise RuntimeError("append_drill_rows(want_mean_var=True) after an append or a truncation that did not carry the mean and "
                               "variance: they are no longer known; run a step")
        N = self.N
        if last.get("mv") is not None:
            mu_l, var_l, stride = last["mv"]
            mu = torch.stack([mu_l.reshape(-1)[j * stride:j * stride + N] for j in range(3)])
            var = torch.stack([var_l.reshape(-1)[j * stride:j * stride + N] for j in range(3)])
        elif mean_var is not None:
            mu, var = (hip.to_dev(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(3, N)), self.device) for a in mean_var)
        else:
            raise RuntimeError("append_drill_rows(want_mean_var=True) needs the mean and variance of the step: run posterior() with "
                               "want_mean_var=True or pass mean_var=(mu, var)")
        st["mu"], st["var"] = mu.contiguous(), var.contiguous()

    # ---- buffers ---------------------------------------------------------------------------------------------------------------
    def _factor_resize(self, last, AK, M_new):
        """L, L^-1, u and A K with M_new rows (a multiple of 256) by allocate-and-copy: the leading rows keep their bits, new padding is
        identity in L and L^-1 and zero in u and A K.  A free-memory check comes first.  Returns the A K view (None without one)."""
        step = last["step"]
        M_old = step.M_pad
        if M_new == M_old:
            return AK
        keep = min(M_old, M_new)
        akbuf = self._ws.get(step.ak_slot) if AK is not None else None
        need = 8 * (2 * M_new * M_new + M_new) + (0 if akbuf is None else akbuf.element_size() * M_new * akbuf.shape[1])
        free = torch.cuda.mem_get_info(self.device)[0] + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if need > free:
            raise MemoryError("%d factor rows instead of %d need %d bytes for the copies of L, L^-1 and A K; %d bytes are free"
                              % (M_new, M_old, need, free))
        if AK is not None:
            last["AK_partial"]         # (a mirrored step completes its rows on the first read: before the buffer is replaced)

        def square(old):
            new = torch.zeros((M_new, M_new), dtype=F64, device=self.device)
            new[:keep, :keep] = old[:keep, :keep]
            if M_new > keep:
                new.diagonal()[keep:].fill_(1.0)
            return new
        L, Linv = square(last["L"]), square(last["Linv"])
        u = torch.zeros(M_new, dtype=F64, device=self.device)
        u[:keep] = last["u"][:keep]
        # (the engine's workspaces follow: the next step finds buffers of the size it asks for or reallocates, as after any other step)
        self._ws[step.aka_slot], self._ws["Linv"] = L, Linv
        last["L"], last["Linv"], last["u"] = L, Linv, u
        if AK is not None:
            new = torch.zeros((M_new, akbuf.shape[1]), dtype=akbuf.dtype, device=self.device)
            new[:keep] = akbuf[:keep]
            self._ws[step.ak_slot] = new
            AK = new[:, :AK.shape[1]]
            last["AK" if last["AK_complete"] else "AK_partial"] = AK
        step.M_pad = M_new
        return AK

    # ---- B = A3 K[:, (2, P)] ---------------------------------------------------------------------------------------------------
    def _append_B(self, last, AK, P_t, pad, qp, sel_xyz, k, B, want=None):
        """B (M_pad x 128; columns behind k are padding) for the drill voxels P_t.  Its sensor rows are A_s K_s2(grid, P), s = 0, 1,
        from the cheapest source the step offers:
          "columns"  a whole A K (every one-rank step but the symmetric plan and the row form): the columns P of its drill block;
          "lattice"  the symmetric plan of a lattice survey: B^T = K_2s[P, :] A_s^T, the k rows K_2s[P, :] through the lattice Gram
                     and the boundary slabs' spectra -- what _assemble_AkA_sym does for the step's own drill rows;
          "points"   anything else: the fused product of geobo_ak_points at the voxel centres (pointpred._points_columns).
        want: one of the three by name (RuntimeError where the step does not offer it); append_B_source says which ran."""
        from .operators import StreamedOperator
        step = last["step"]
        prior, Md = step.prior, step.Md
        Msp, nc, kp = self.Ms_pad, self.nc, B.shape[1]
        off_d = 2 * Msp
        A_g, A_m = last["ops"]
        ok = dict(columns=AK is not None and last["AK_complete"], lattice=AK is not None and step.sym and self._sym_ok(A_g, A_m), points=True)
        if want and not ok.get(want, False):
            raise RuntimeError("the source %r of B is not available on this step" % (want,))
        src = want or next(n for n in ("columns", "lattice", "points") if ok[n])
        self.append_B_source = src
        if src == "points":
            op_rows, slot = self._points_op_batch()
            return self._points_columns(prior, qp, (2,), [B], sel_xyz, Md, op_rows, slot, k)
        if src == "columns":
            B[:off_d] = AK[:off_d].index_select(1, pad + step.props.index(2) * nc)
        else:
            gram, pl, ny = self._gram, self.nx * self.nz, self.ny
            Kd = self._workspace("append_Kd", (kp, nc + 16 + hip.pad_n(self.nz)))[:, :nc]     # (slack behind the last row: edge_rows)
            BT = self._workspace("append_BT", (kp, off_d + 16))[:, :off_d]
            BT.zero_()
            for s_, (func, A) in enumerate((("grav", A_g), ("magn", A_m))):
                self._cov_rows(prior, 2, s_, P_t, self.c0, Kd[:k])
                out = BT[:, s_ * Msp:(s_ + 1) * Msp]
                gram.gram_rows(Kd, k, self._lam[func][1], out, 0, ny)
                for e, iy in enumerate((0, ny - 1)):
                    if isinstance(A, StreamedOperator):
                        ycols = A.edge[:, e * pl:(e + 1) * pl] if A.lattice is not None else A.slab_into(self._workspace2d("op_slab", Msp, pl), iy, iy + 1)
                    else:
                        ycols = A[:, iy * pl:(iy + 1) * pl]
                    gram.edge_rows(Kd[:, iy * pl:], k, self._edge_spectrum(func, e, ycols), out)
            hip.transpose(BT, B[:off_d])
        B[off_d + Md:].zero_()
        if Md:
            prior.k_block(self, 2, 2, sel_xyz, qp, B[off_d:off_d + Md])

    # ---- one chunk -------------------------------------------------------------------------------------------------------------
    def _append_chunk(self, last, AK, vox, vals, b_source=None):
        """Rows for the k <= 128 voxels `vox` (int64 host array) with values `vals` behind the valid rows; M_pad has room.  Everything
        goes to scratch until the status word is back.  Returns (status, logsum, |u_P|^2); status != 0: nothing was written."""
        step = last["step"]
        prior, Md, M_pad = step.prior, step.Md, step.M_pad
        Linv, L, u = last["Linv"], last["L"], last["u"]
        Msp, N, dev = self.Ms_pad, self.N, self.device
        off_d = 2 * Msp
        Mv = off_d + Md
        k, kp = int(vox.size), APPEND_K_MAX
        assert 1 <= k <= kp and Mv + k <= M_pad
        xyz = self.grid_points()
        P_t = torch.as_tensor(vox, device=dev)
        pad = torch.cat([P_t, P_t[-1:].expand(kp - k)])                  # padded with copies of the last point: finite, never used
        qp = tuple(c[pad].contiguous() for c in xyz)
        sel_xyz = tuple(c[step.sel_t] for c in xyz) if Md else None
        B = self._workspace("append_B", (M_pad, kp + 16))[:, :kp]
        self._timed("append_B", 0.0, lambda: self._append_B(last, AK, P_t, pad, qp, sel_xyz, k, B, b_source))
        W = self._workspace("append_W", (M_pad, kp + 16))[:, :kp]
        WT = self._workspace("append_WT", (kp, M_pad + 16))[:, :M_pad]
        X2 = self._workspace("append_X2", (kp, M_pad + 16))[:, :M_pad]
        R = self._workspace("append_R", (kp, M_pad + 16))[:, :M_pad]
        small = self._workspace("append_small", (4, kp, kp))
        G, D, Ls, T = small[0], small[1], small[2], small[3]
        vec = self._workspace("append_vec", (3, kp))
        y_P, r, uP = vec[0], vec[1], vec[2]
        splits = 16                                                      # (M_pad is a multiple of 256 = 16 x 16)

        def run():
            hip.gemm_nn(Linv, B, W, x_lower=True)                        # W = L^-1 B; zero behind row Mv (identity rows x zero rows)
            hip.transpose(W, WT)
            hip.gemm_nt_splitk(WT, WT, G, splits, self._workspace("append_gram_ws", (splits * kp * kp,)))
            prior.k_block(self, 2, 2, qp, qp, D)
            D.diagonal().add_(float(step.noise[2]) ** 2)                 # the diagonal _finish_AkA gives drill rows
            if vals is None:
                r.zero_()                                                # values at the posterior mean W^T u: u_P = 0 exactly
            else:
                y_P.zero_()
                y_P[:k] = torch.as_tensor(np.asarray(vals, dtype=np.float64), device=dev)
                torch.sub(y_P, hip.colgemv(W, u, ws=self._workspace("append_colgemv_ws", (hip.colgemv_ws_doubles(M_pad, kp),))), out=r)
            Ls.zero_()
            T.zero_()
            uP.zero_()
            out, status = hip.factor_append(D, G, r[:k], Ls, T, uP)
            hip.gemm_nn(WT, Linv, X2, y_lower=True)                      # W^T L^-1
            hip.gemm_nn(T, X2, R, alpha=-1.0)                            # -T W^T L^-1 (T zero behind k: the padding rows come out zero)
            return out, status
        out, status = self._timed("append_factor", 2.0 * kp * M_pad * M_pad, run)
        h_st = self._to_host_async(status, "append_status")
        h_out = self._to_host_async(out, "append_logsum")
        h_u = self._to_host_async(uP[:k], "append_u")
        torch.cuda.current_stream(dev).synchronize()
        if int(h_st[0]) != 0:
            return int(h_st[0]), 0.0, 0.0
        logsum, upup = float(h_out[0]), float(np.dot(h_u, h_u))
        rows = slice(Mv, Mv + k)
        L[rows, :Mv] = WT[:k, :Mv]
        L[rows, rows] = Ls[:k, :k]
        Linv[rows, :Mv] = R[:k, :Mv]
        Linv[rows, rows] = T[:k, :k]
        u[rows] = uP[:k]
        if AK is not None:
            nc = self.nc
            for jj, j in enumerate(step.props):                          # K_2j[P, :]: the drill rows of A K, as _assemble_AK writes them
                self._cov_rows(prior, 2, j, P_t, self.c0, AK[off_d + Md:off_d + Md + k, jj * nc:(jj + 1) * nc])
        step.sel_t = P_t if step.sel_t is None else torch.cat([step.sel_t, P_t])
        step.Md = Md + k
        last["sel"] = np.concatenate([np.asarray(last["sel"], dtype=np.int64), vox])
        return 0, logsum, upup

    # ---- entry points ----------------------------------------------------------------------------------------------------------
    def append_drill_rows(self, voxels, values, want_mean_var=True, mean_var=None, tile_hook=None, _b_source=None):
        """Drill-property observations `values` (the GP's normalised units) at the voxels `voxels` (flat indices in (iy, ix, iz)
        order) as new rows behind the last row of the last posterior() step's factor; the engine's state (engine.last: L, L^-1, u,
        sel, step, the drill rows of A K) is updated in place and every product that works from the step's L^-1 sees the rows.
        values=None: the posterior mean at the voxels ("kriging believer" rows: u_P = 0, the mean keeps its bits).
        Returns dict(mu, var, logl, uu, logdet, info) as posterior() does (mu, var only with want_mean_var; logl 0 when the step
        computed no likelihood).  mean_var: host (mu, var) to start from when the step kept none on the device.  tile_hook(V, n):
        called with every tile of the new rows of V_d (information.set_gram's input), after every chunk has factorised.
        ValueError: voxels that repeat, lie outside [0, N) or carry a drill row already, len(values) != len(voxels).  CholeskyError: a
        pivot failed; the engine is as it was.  One rank, fp64 assembly, a completed step over property blocks (0, 1, 2)."""
        from .engine import CholeskyError
        last, AK = self._append_ready("append_drill_rows()")
        vox = np.asarray(voxels)
        vals = None if values is None else np.asarray(values, dtype=np.float64).reshape(-1)
        if vox.size and not np.issubdtype(vox.dtype, np.integer):
            raise ValueError("voxels must be integer flat voxel indices")
        vox = vox.reshape(-1).astype(np.int64)
        if vals is not None and vox.size != vals.size:
            raise ValueError("%d values for %d voxels" % (vals.size, vox.size))
        if vox.size < 1:
            raise ValueError("append_drill_rows() needs at least one voxel")
        if np.any(vox < 0) or np.any(vox >= self.N):
            raise ValueError("voxels must be flat voxel indices in [0, %d)" % self.N)
        if np.unique(vox).size != vox.size:
            raise ValueError("voxels repeat: one drill row per voxel")
        if np.intersect1d(vox, np.asarray(last["sel"], dtype=np.int64)).size:
            raise ValueError("voxels %s carry a drill row already" % np.intersect1d(vox, np.asarray(last["sel"], dtype=np.int64))[:8])
        if vals is not None and not np.all(np.isfinite(vals)):
            raise ValueError("values must be finite")
        with torch.cuda.device(self.device):
            st = self._append_state(last)
            if want_mean_var:
                self._append_mean_var(last, st, mean_var)
            step = last["step"]
            Md_start, Msp = step.Md, self.Ms_pad
            Mv_start = 2 * Msp + Md_start
            st["snaps"][Md_start] = (st["uu"], st["logdet"], None if st["mu"] is None else st["mu"].clone(),
                                     None if st["var"] is None else st["var"].clone(), st["lost"])
            uu, logdet = st["uu"], st["logdet"]
            AK = self._factor_resize(last, AK, max(step.M_pad, hip.pad_m(Mv_start + vox.size)))
            prior = step.prior
            # every chunk's factor first: a failed pivot finds the mean, the variance and the caller's Grams untouched
            for c0 in range(0, vox.size, APPEND_K_MAX):
                Mv = 2 * Msp + step.Md
                status, logsum, upup = self._append_chunk(last, AK, vox[c0:c0 + APPEND_K_MAX],
                                                          None if vals is None else vals[c0:c0 + APPEND_K_MAX], _b_source)
                if status != 0:
                    self._truncate(last, AK, Md_start)
                    raise CholeskyError(Mv + status)
                if uu is not None:
                    uu, logdet = uu + upup, logdet + 2.0 * logsum
            st["uu"], st["logdet"] = uu, logdet
            if want_mean_var or tile_hook is not None:
                blocks = (0, 1, 2) if want_mean_var else (2,)
                row, u = Mv_start, last["u"]
                source = self._zsource(step, AK, "auto")
                for Vs, n in self._v_tiles(source, prior, AK, blocks=blocks, rows=(Mv_start, Mv_start + vox.size)):
                    if want_mean_var:
                        self._timed("append_downdate", 4.0 * 3 * n * self.N, lambda: [
                            hip.rows_downdate(V, n, u[row:row + n], st["mu"][a], st["var"][a], ncols=self.N) for a, V in zip(blocks, Vs)])
                    if tile_hook is not None:
                        tile_hook(Vs[blocks.index(2)], n)
                    row += n
            if not want_mean_var:
                st["mu"] = st["var"] = None          # (rows went in without their downdate)
                st["lost"] = True
            out = dict(info=0, M_pad=step.M_pad, lengths=[float(v) for v in prior.lengths], logl=0.0)
            if uu is not None:
                out["uu"], out["logdet"] = uu, logdet
                out["logl"] = -0.5 * (uu + logdet + self.N * math.log(2 * math.pi))
            if want_mean_var:
                out["mu"], out["var"] = self._results_to_host(st["mu"].reshape(-1), st["var"].reshape(-1), (0, 1, 2))
            return out

    def _truncate(self, last, AK, Md):
        step = last["step"]
        Md_cur, Msp = step.Md, self.Ms_pad
        off_d = 2 * Msp
        if Md < Md_cur:
            r0, r1 = off_d + Md, off_d + Md_cur
            for X in (last["L"], last["Linv"]):
                X[r0:r1].zero_()
                X.diagonal()[r0:r1].fill_(1.0)
            last["u"][r0:r1].zero_()
            if AK is not None:
                AK[r0:r1].zero_()
            step.sel_t = step.sel_t[:Md] if Md else None
            step.Md = Md
            last["sel"] = np.asarray(last["sel"], dtype=np.int64)[:Md]
        return self._factor_resize(last, AK, hip.pad_m(off_d + Md))

    def truncate_drill_rows(self, Md):
        """Drop the drill rows behind the first `Md` again (rows that append_drill_rows added: Md is at least the step's own count).
        Identity rows return in L and L^-1; u, sel, step and the drill rows of A K are reset; buffers that had grown go back to
        pad256(2 Ms_pad + Md) rows.  Afterwards every buffer a step over Md rows would hold has the bits it had before the append.
        Where an append call began at Md rows (the step's own count among them) the mean, the variance and the two likelihood
        statistics return as they were then; at any other Md the statistics are formed again from u and the diagonal of L, and the
        mean and variance are dropped (mean_var_known() says so; a step brings them back)."""
        last, AK = self._append_ready("truncate_drill_rows()")
        st = self._append_state(last)
        Md = int(Md)
        if not st["Md0"] <= Md <= last["step"].Md:
            raise ValueError("Md must lie between the step's %d drill rows and the current %d" % (st["Md0"], last["step"].Md))
        with torch.cuda.device(self.device):
            if Md == last["step"].Md:
                return
            self._truncate(last, AK, Md)
            st["snaps"] = {m: v for m, v in st["snaps"].items() if m <= Md}
            if Md in st["snaps"]:
                uu, logdet, mu, var, lost = st["snaps"][Md]
                st.update(uu=uu, logdet=logdet, mu=None if mu is None else mu.clone(), var=None if var is None else var.clone(), lost=lost)
                return
            st.update(mu=None, var=None, lost=True)
            if st["uu"] is not None:          # (padding rows: u = 0 and a unit diagonal, so the sums run over the whole buffers)
                u = last["u"]
                st["uu"] = float((u * u).sum())
                st["logdet"] = float(2.0 * torch.log(last["L"].diagonal()).sum())
