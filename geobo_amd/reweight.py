"""Down-weighting or dropping data rows of a finished step, exactly: mixin of engine.PosteriorEngine.

The valid rows of K_y = A3 K A3^T + Sigma are [grav | magn | drill] and Sigma is diagonal.  With P = K_y^-1 = L^-T L^-1, alpha = P y =
L^-T u and D a set of k <= 128 rows, giving row i of D the noise s_i sigma (s_i in (1, inf]; inf drops the row) adds
Delta = diag((s_i^2 - 1) sigma_i^2) on D.  With dinv_i = 1 / Delta_i (0 for a dropped row):

    W  = L^-1[:, D]                     G = W^T W = P_DD,   a = W^T u = alpha_D
    S  = G + diag(dinv) = C C^T         (geobo_fold_factor: C^-1, g = C^-1 a, 2 sum log diag C, g^T g)
    P_D = W^T L^-1                      the rows D of K_y^-1: a DENSE left factor
    B  = P_D A3 K                       property by property: the tile generators of information.py with P_D in the place of L^-1
    mu' = mu - (C^-1 B)^T g,   var' = var + colsum((C^-1 B)^2)                  (geobo_rows_reweight, one pass over B)
    uu' = uu - g^T g,          logdet' = logdet + 2 sum log diag C + sum_{finite i} log Delta_i

reweight_preview computes this from engine.last and changes nothing.  The COMMITTED state is engine.row_scale (per gravity station,
per magnetic station, per drill voxel; None: all ones): a posterior() step multiplies a row's noise variance by s^2, and gives a dropped
row a zero row and column with a unit diagonal in AkA, a zero in y and a zero diagonal entry in L^-1 -- the rows of V for dropped rows
vanish, u_i = 0, the unit pivot adds nothing to logdet, and every consumer that works from L^-1 sees the reduced system.
"""
import math

import numpy as np
import torch

from . import hip
from .crossval import padded_rows

F64 = hip.F64
REWEIGHT_K_MAX = 128


def check_scales(scale, k):
    """`scale` broadcast to k rows as float64; ValueError below 1 or NaN (S would be indefinite)."""
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64), (k,)).copy()
    if np.any(np.isnan(s)) or np.any(s < 1.0):
        raise ValueError("a row scale lies in [1, inf] (inf drops the row); scales below 1 are not supported")
    return s


class ReweightMixin:
    row_scale = None        # dict(grav (Ms,), magn (Ms,), drill (N,)) of scales >= 1, inf: dropped; None: all ones

    # ---- the committed state -----------------------------------------------------------------------------------------------------
    def set_row_scale(self, grav=None, magn=None, drill=None):
        """The row scales every later posterior() step honours: per gravity station and per magnetic station (Ms each) and per drill
        VOXEL (N; it survives a change of the drill selection); None: ones.  All None: the attribute is cleared."""
        if grav is None and magn is None and drill is None:
            self.row_scale = None
            return
        out = {}
        for name, v, n in (("grav", grav, self.Ms), ("magn", magn, self.Ms), ("drill", drill, self.N)):
            out[name] = np.ones(n) if v is None else check_scales(np.asarray(v, dtype=np.float64).reshape(-1), n)
        self.row_scale = out

    def _data_scales(self, sel):
        """The scales of the data rows [grav | magn | drill at the voxels sel] (all ones without a committed state)."""
        sel = np.asarray(sel, dtype=np.int64)
        rs = self.row_scale
        if rs is None:
            return np.ones(2 * self.Ms + sel.size)
        return np.concatenate([rs["grav"], rs["magn"], rs["drill"][sel]])

    def _row_scale_active(self):
        rs = self.row_scale
        return rs is not None and any(np.any(v != 1.0) for v in rs.values())

    def _step_row_scale(self, sel):
        """What a step over the drill voxels `sel` does about the committed scales: None (all ones: nothing is launched), or
        (s2 (M_pad,) host array of noise-variance factors, 1 on dropped and padding rows; dropped: int64 rows of the padded matrix)."""
        if self.row_scale is None:
            return None
        s = self._data_scales(sel)
        if not np.any(s != 1.0):
            return None
        Ms, Msp = self.Ms, self.Ms_pad
        rows = padded_rows(np.arange(s.size), Ms, Msp)
        s2 = np.ones(hip.pad_m(2 * Msp + (s.size - 2 * Ms)))
        fin = np.isfinite(s)
        s2[rows[fin]] = s[fin] ** 2
        return s2, rows[~fin]

    def dropped_rows(self, sel=None):
        """Data rows ([grav | magn | drill]) the committed state drops, for the drill voxels `sel` (default: the last step's)."""
        if sel is None:
            sel = self.last["sel"] if self.last is not None else np.zeros(0, dtype=np.int64)
        return np.flatnonzero(np.isinf(self._data_scales(sel)))

    # ---- preview -----------------------------------------------------------------------------------------------------------------
    def _reweight_mean_var(self, last):
        """Copies of the (3, N) device mean and variance of the step as it stands (with the rows appended since), or None."""
        st = last.get("append")
        if st is not None and st["mu"] is not None:
            return st["mu"].clone(), st["var"].clone()
        if (st is not None and st["lost"]) or last.get("mv") is None:
            return None
        N = self.N
        mu_l, var_l, stride = last["mv"]
        return (torch.stack([mu_l.reshape(-1)[j * stride:j * stride + N] for j in range(3)]).contiguous(),
                torch.stack([var_l.reshape(-1)[j * stride:j * stride + N] for j in range(3)]).contiguous())

    def reweight_preview(self, rows, scale=np.inf, want="cubes", source="auto"):
        """What the last posterior() step would have given with the data rows `rows` (indices into [grav | magn | drill], at most
        128) at `scale` times their noise (a scalar or one per row, in (1, inf]; inf: the row dropped), without a new step and
        without touching the engine's state.  Returns dict(uu, logdet, logl, sum_dmu2, max_dmu, sum_dvar (three each, per property:
        sum and largest magnitude of the change of the mean, sum of the increase of the variance, normalised units), status) and,
        with want="cubes", mu and var: (3, N) device tensors, copies (the step's own stay).  want="stats": no cube is copied or
        written.  source: the tile source of B ("auto": by the step's route, "spectral", "generic").
        ValueError: no rows or more than 128, a row twice or outside the data, a scale below 1, a row that is dropped already.
        CholeskyError: S did not factorise.  One rank, fp64 assembly, a completed step over property blocks (0, 1, 2) with its
        likelihood; want="cubes" needs its mean and variance."""
        from .engine import CholeskyError
        if want not in ("cubes", "stats"):
            raise ValueError("want must be 'cubes' or 'stats'")
        last, AK = self._append_ready("reweight_preview()")
        step = last["step"]
        Ms, Msp, Md = self.Ms, self.Ms_pad, step.Md
        Mu = 2 * Ms + Md
        idx = np.asarray(rows)
        if idx.size and not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("rows must be integer indices into the data vector [grav | magn | drill]")
        idx = idx.reshape(-1).astype(np.int64)
        k = int(idx.size)
        if k < 1:
            raise ValueError("reweight_preview() needs at least one row")
        if k > REWEIGHT_K_MAX:
            raise ValueError("%d rows in one preview: at most %d (commit the scales and run a step)" % (k, REWEIGHT_K_MAX))
        if np.any(idx < 0) or np.any(idx >= Mu):
            raise ValueError("rows must lie in [0, %d)" % Mu)
        if np.unique(idx).size != k:
            raise ValueError("a row is named twice")
        s = check_scales(scale, k)
        if np.any(s == 1.0):
            raise ValueError("a scale of 1 changes nothing: leave the row out")
        current = self._data_scales(last["sel"])[idx]
        if np.any(np.isinf(current)):
            raise ValueError("rows %s are dropped already" % idx[np.isinf(current)][:8])
        uu, logdet = last.get("uu"), last.get("logdet")
        st = last.get("append")
        if st is not None:
            uu, logdet = st["uu"], st["logdet"]
        if uu is None:
            raise RuntimeError("reweight_preview() needs the likelihood statistics of the step: run posterior() with calclogl=True")
        # Delta on the row's CURRENT noise variance (a committed finite scale included)
        sig2 = np.repeat(np.asarray(step.noise, dtype=np.float64) ** 2, (Ms, Ms, Md))[idx] * current ** 2
        fin = np.isfinite(s)
        delta = (np.where(fin, s, 2.0) ** 2 - 1.0) * sig2
        dinv = np.where(fin, 1.0 / delta, 0.0)
        logdelta = float(np.log(delta[fin]).sum())
        with torch.cuda.device(self.device):
            mv = self._reweight_mean_var(last) if want == "cubes" else None
            if want == "cubes" and mv is None:
                raise RuntimeError("reweight_preview(want='cubes') needs the mean and variance of the step: run posterior() with "
                                   "want_mean_var=True")
            source = self._zsource(step, AK, source)
            out = self._reweight(last, AK, padded_rows(idx, Ms, Msp), dinv, mv, source)
        if out["status"] != 0:
            raise CholeskyError(out["status"])
        out["uu"] = uu - out.pop("gg")
        out["logdet"] = logdet + out.pop("logdetC") + logdelta
        out["logl"] = -0.5 * (out["uu"] + out["logdet"] + self.N * math.log(2 * math.pi))
        return out

    def _reweight(self, last, AK, prow, dinv, mv, source):
        """The device part of reweight_preview for the rows `prow` of the padded matrix: dict(status, logdetC, gg, sum_dmu2, max_dmu,
        sum_dvar[, mu, var]).  mv: the (mu, var) copies to update, or None (statistics only)."""
        step = last["step"]
        Linv, u = last["Linv"], last["u"]
        M_pad, N, dev = step.M_pad, self.N, self.device
        k, kp, T = int(prow.size), REWEIGHT_K_MAX, 256
        D_t = torch.as_tensor(prow, device=dev)
        WT = self._workspace("reweight_WT", (kp, M_pad + 16))[:, :M_pad]
        PD = self._workspace("reweight_PD", (T, M_pad + 16))[:, :M_pad]          # (padded to the generators' tile height)
        small = self._workspace("reweight_small", (2, kp, kp))
        G, Cinv = small[0], small[1]
        vec = self._workspace("reweight_vec", (3, kp))
        a, g, dv = vec[0], vec[1], vec[2]
        stats = self._workspace("reweight_stats", (2,))
        parts = self._workspace("reweight_part", (3, 3))
        status = self._workspace("reweight_status", (1,), dtype=torch.int32)
        splits = 16                                                              # (M_pad is a multiple of 256 = 16 x 16)

        def factor():
            WT.zero_()
            WT[:k] = Linv.t()[D_t]                                               # W^T: the columns D of L^-1 as rows
            hip.gemm_nt_splitk(WT, WT, G, splits, self._workspace("reweight_gram_ws", (splits * kp * kp,)))
            hip.rowgemv(WT, u, out=a)                                            # a = W^T u = alpha_D
            dv.zero_()
            dv[:k] = torch.as_tensor(dinv, device=dev)
            hip.fold_factor(G, dv[:k], a[:k], Cinv, g, stats=stats, status=status)
            PD[kp:].zero_()
            hip.gemm_nn(WT, Linv, PD[:kp], y_lower=True)                         # P_D = W^T L^-1
        self._timed("reweight_factor", 2.0 * kp * M_pad * M_pad, factor)
        h_st = self._to_host_async(status, "reweight_status")
        h_stats = self._to_host_async(stats, "reweight_stats")
        torch.cuda.current_stream(dev).synchronize()
        if int(h_st[0]) != 0:
            return dict(status=int(h_st[0]))
        out = dict(status=0, logdetC=float(h_stats[0]), gg=float(h_stats[1]))
        mu, var = mv if mv is not None else (None, None)
        ws = self._workspace("reweight_ws", (hip.rows_reweight_ws_doubles(N),))
        for Vs, n in self._v_tiles(source, step.prior, AK, blocks=(0, 1, 2), rows=(0, k), left=PD):
            assert n == k                                                        # (k <= 128: one tile of either generator)
            self._timed("reweight_rows", 1.0 * 3 * k * k * N, lambda: [
                hip.rows_reweight(V, k, Cinv, g, None if mu is None else mu[j], None if var is None else var[j], ncols=N,
                                  part=parts[j], ws=ws) for j, V in enumerate(Vs)])
        h = self._to_host(parts.reshape(-1), "reweight_part").reshape(3, 3).copy()
        out.update(sum_dmu2=h[:, 0], max_dmu=h[:, 1], sum_dvar=h[:, 2])
        if mv is not None:
            out["mu"], out["var"] = mu, var
        return out
