"""Per-set blocks of the drill-property posterior covariance: mixin of engine.PosteriorEngine.

For a voxel set P (a drill hole) the posterior covariance of the drill property is

    Sigma_PP = K_dd(P, P) - G_P,   G_P = V_d(:, P)^T V_d(:, P),   V_d = (L^-1 A3 K)[:, drill block]

from the factor of the last posterior() step.  V_d (M x N) is never stored: it is produced tile by tile of rows, and every tile goes
through geobo_set_gram, which adds V_tile(:, P_c)^T V_tile(:, P_c) to G[c] for every set c at once.  geobo_set_logdet then forms
S_c = Sigma_PP / sigma_d^2 + I and returns 1/2 log det S_c (the information gain of a drill log along P, nats), 1^T Sigma_PP 1 and
trace Sigma_PP.

Two sources of V_d tiles, by the route the step took:
  spectral  the transposed route (plan.Route.single): rows of Z = L^-1 A3 as the step makes them (lattice convolutions or MFMA GEMMs
            against the operators), times K through SpectralProduct.product with the generators of blocks (0, 2), (1, 2), (2, 2);
            the drill term only in the rows behind the sensor rows (L^-1 is lower triangular), as in _drill_rows_ss.
  generic   every other one-rank fp64 step: L^-1 (A K)[:, drill block] by MFMA GEMMs when A K is whole, otherwise rows of Z by
            GEMMs against the operator rows (as condition() forms A3^T W) and K through the prior sampler's exact circulant product.
Both generators yield the tiles of any list of property blocks in lockstep (the drill block alone by default): the block-support
statistics of blocksupport.py sweep all three, with one forward transform of Z per operator term.
"""
import numpy as np
import torch

from . import hip

F64 = hip.F64
SET_K_MAX = 128


def _vertical_bases(idx, nz):
    """Column bases when every set is one whole z-column (nz contiguous flat indices from a multiple of nz), else None."""
    idx = np.asarray(idx)
    if idx.shape[1] != nz:
        return None
    base = idx[:, 0]
    if np.any(base < 0) or np.any(base % nz) or not np.array_equal(idx, base[:, None] + np.arange(nz)[None, :]):
        return None
    return base


def _tile_range(rows, Mv):
    """The row range of a tile sweep: all Mv valid rows, or the caller's (r0, r1) within them."""
    if rows is None:
        return 0, Mv
    r0, r1 = int(rows[0]), int(rows[1])
    if not 0 <= r0 <= r1 <= Mv:
        raise ValueError("rows must lie within the %d valid rows, got %r" % (Mv, rows))
    return r0, r1


def _tile_rows(V, n, skip):
    """(Vs, n) of a tile whose first `skip` rows lie in front of the row range (tiles start at multiples of the tile height)."""
    if skip <= 0:
        return V, n
    return [v[skip:] for v in V], n - skip


class SetStatisticsMixin:
    def _set_sampler(self, prior):
        """PriorSampler whose exact circulant product applies K (generic source), cached per hyper-parameters."""
        from .sampling import PriorSampler
        s = self.s
        name, lengths, W, amp = prior.name, prior.lengths, prior.W, prior.amp
        key = (name, tuple(float(v) for v in lengths), tuple(map(tuple, W)), float(amp))
        hit = getattr(self, "_set_smp", None)
        if hit is None or hit[0] != key:
            smp = PriorSampler((self.ny, self.nx, self.nz), (s.xvoxsize, s.yvoxsize, s.zvoxsize), name, [float(v) for v in lengths], W,
                               float(amp), device=self.device, approximate=True)
            hit = self._set_smp = (key, smp)
        return hit[1]

    def _v_spectral(self, step, prior, Linv, A_g, A_m, blocks=(2,), rows=None, dense=False):
        """Tiles (Vs, n) of 128 rows of V_a for every property block a of `blocks` in lockstep (Vs: one tile per block) on the
        transposed route, voxel order (iy, ix, iz): the generators of the step whose factor Linv is where it kept them, the others
        from `prior`.  The rows of Z are formed once per tile and every operator term is ONE product for all the blocks (Z is
        transformed once).  rows = (r0, r1): the rows r0 .. r1 only (_tile_range).  dense: Linv is a dense left factor (rows of K_y^-1,
        reweight.py), not a lower triangular one: no operator term is skipped."""
        sel_t, Md = step.sel_t, step.Md
        sp, N, Msp, T = self._spectral, self.N, self.Ms_pad, 128
        lat = (self._gram is not None and self._gram.edge_supported() and Msp == self.nx * self.ny and self.route.opt("z_lattice")
               and all(self._lam.get(f) is not None and self._lam[f][0] is A for f, A in (("grav", A_g), ("magn", A_m))))
        if not lat:
            Ag = self._resident_operator(A_g, "grav")
            Am = self._resident_operator(A_m, "magn")
        gen = lambda s_, a: step.gens[(s_, a)] if (s_, a) in step.gens else sp.eigenvalues(prior.table(self, s_, a))
        gens = [[gen(s_, a) for a in blocks] for s_ in range(3)]
        Zg, Zm, Zd = (self._workspace2d(nm, T, N) for nm in ("set_Zg", "set_Zm", "set_Zd"))
        # (the drill block keeps the buffers it had before the other blocks came)
        V = [self._workspace2d("set_V" if a == 2 else "set_V%d" % a, T, N) for a in blocks]
        tmp = [self._workspace2d("set_Vt" if a == 2 else "set_Vt%d" % a, T, N) for a in blocks]
        r0, r1 = _tile_range(rows, 2 * Msp + Md)
        for b0 in range(r0 // T * T, r1, T):
            n = min(T, r1 - b0)
            terms = []
            for func, A, Ar, c0, Z, g in (("grav", A_g, None if lat else Ag, 0, Zg, gens[0]), ("magn", A_m, None if lat else Am, Msp, Zm, gens[1])):
                if not dense and b0 + n <= c0:
                    continue                                # L^-1 is lower triangular: these rows do not see this operator
                if lat:
                    self._lattice_Z(Linv[b0:b0 + n, c0:c0 + Msp], n, func, A, Z)
                else:
                    hip.gemm_nn(Linv[b0:b0 + T, c0:c0 + Msp], Ar[:Msp, :N], Z)
                terms.append((Z, g))
            if Md and (dense or b0 + n > 2 * Msp):
                Zd[:n].zero_()
                Zd[:n, sel_t] = Linv[b0:b0 + n, 2 * Msp:2 * Msp + Md]
                terms.append((Zd, gens[2]))
            sp.product(terms[0][0], n, terms[0][1], V)
            for Z, g in terms[1:]:
                sp.product(Z, n, g, tmp)
                for v, t in zip(V, tmp):
                    v[:n].add_(t[:n])
            yield _tile_rows(V, n, r0 - b0)

    def _v_generic(self, step, prior, Linv, A_g, A_m, AK, blocks=(2,), rows=None, dense=False):
        """Tiles (Vs, n) of 256 rows of V_a for every property block a of `blocks` on any one-rank fp64 step, voxel order
        (iy, ix, iz).  Vs[i] holds N columns or more.  rows = (r0, r1): the rows r0 .. r1 only (_tile_range).  dense: Linv is a dense
        left factor, not a lower triangular one: the contraction runs over every row of A K and no operator term is skipped."""
        sel_t, Md = step.sel_t, step.Md
        N, Np, Msp, T = self.N, self.N_pad, self.Ms_pad, 256
        r0, r1 = _tile_range(rows, 2 * Msp + Md)
        start = r0 // T * T
        if AK is not None:
            AKa = [AK[:, a * self.nc:a * self.nc + Np] for a in blocks]
            V = [self._workspace2d("set_V" if a == 2 else "set_V%d" % a, T, Np) for a in blocks]
            for b0 in range(start, r1, T):
                e = b0 + T                                  # (M_pad is a multiple of 256: whole tiles; columns >= e of L^-1 are zero)
                for AKd, v in zip(AKa, V):
                    if dense:
                        hip.gemm_nn(Linv[b0:e], AKd, v)
                    else:
                        hip.gemm_nn(Linv[b0:e, :e], AKd[:e], v)
                yield _tile_rows(V, min(T, r1 - b0), r0 - b0)
            return
        smp = self._set_sampler(prior)
        Zt = torch.empty((T, 3, N), dtype=F64, device=self.device)
        Zp = self._workspace2d("set_Zp", T, Np)
        for b0 in range(start, r1, T):
            n = min(T, r1 - b0)
            for j, A, a0 in ((0, A_g, 0), (1, A_m, Msp)):
                if not dense and b0 + n <= a0:
                    Zt[:, j, :].zero_()
                    continue
                for c0, arows in self._operator_rows(A):
                    hip.gemm_nn(Linv[b0:b0 + T, a0 + c0:a0 + c0 + arows.shape[0]], arows, Zp, beta=1.0 if c0 else 0.0)
                Zt[:, j, :] = Zp[:, :N]
            Zt[:, 2, :].zero_()
            if Md and (dense or b0 + n > 2 * Msp):
                Zt[:, 2, :][:, sel_t] = Linv[b0:b0 + T, 2 * Msp:2 * Msp + Md]
            KZ = smp.apply_K(Zt[:n])                        # (all three properties come out of the one circulant product)
            yield _tile_rows([KZ[:, a, :] for a in blocks], n, r0 - b0)

    def _zsource(self, step, AK, source):
        """The tile source of a sweep, "spectral" or "generic" ("auto": by the step's route); sets set_source."""
        spectral_ok = self._zpath_ok(step, AK)
        if source == "auto":
            source = "spectral" if spectral_ok else "generic"
        if source == "spectral" and not spectral_ok:
            raise RuntimeError("the spectral source needs a step on the transposed route")
        if source not in ("spectral", "generic"):
            raise ValueError("source must be 'auto', 'spectral' or 'generic'")
        self.set_source = source
        return source

    def _v_tiles(self, source, prior, AK, blocks=(2,), rows=None, left=None):
        """Generator of the V tiles of the last step's factor from `source` ("spectral" or "generic"); rows = (r0, r1): the rows
        r0 .. r1 of V only (default: all of them).  left: a dense left factor in the place of L^-1 (rows of K_y^-1 padded to the
        tile height, reweight.py): the tiles are rows of left A3 K and the short-cuts of a triangular factor are off."""
        last = self.last
        Linv, step = last["Linv"], last["step"]
        A_g, A_m = last["ops"]
        if left is not None:
            if source == "spectral":
                return self._v_spectral(step, prior, left, A_g, A_m, blocks, rows, dense=True)
            return self._v_generic(step, prior, left, A_g, A_m, AK if last["AK_complete"] else None, blocks, rows, dense=True)
        if source == "spectral":
            return self._v_spectral(step, prior, Linv, A_g, A_m, blocks, rows)
        return self._v_generic(step, prior, Linv, A_g, A_m, AK if last["AK_complete"] else None, blocks, rows)

    def set_statistics(self, sets, kernelfunc, lengths, crossweights, gp_amp, gp_sigma, observed=None, source="auto"):
        """Posterior statistics of the drill property over C voxel sets, from the factor of the last posterior() step:
            info_gain[c] = 1/2 log det(I + Sigma_PP / sigma_d^2)  (nats),  path_var[c] = 1^T Sigma_PP 1,  sum_var[c] = trace Sigma_PP,
        P = sets[c] (flat voxel indices in (iy, ix, iz) order; entries < 0 are padding), sigma_d = gp_sigma[2], all in the GP's
        normalised units.  observed: optional (N,) bool mask of voxels that already carry a drill row: they are left out (unit rows of
        S, not in the sums).  `lengths` carry the create_cov mutation.  source: "auto" (by the step's route), "spectral" or "generic".
        Returns device tensors (info_gain, path_var, sum_var, status), C each; status 1 + pivot marks a set whose S did not factorise
        (NaN outputs).  One rank, fp64 assembly, a step over property blocks (0, 1, 2)."""
        from .engine import weight_matrix
        from .step import Prior
        if self.world > 1:
            raise NotImplementedError("set statistics run on one rank (world = %d)" % self.world)
        last = self.last
        if last is None or tuple(last["props"]) != (0, 1, 2):
            raise RuntimeError("set_statistics() needs the factor of a posterior() step over all three property blocks")
        AK = last["AK"] if last["AK_complete"] else last["AK_partial"]
        if self.f32 or (AK is not None and AK.dtype != F64):
            raise NotImplementedError("set statistics need the fp64 assembly")
        sets = np.asarray(sets)
        if sets.ndim != 2 or not 1 <= sets.shape[1] <= SET_K_MAX:
            raise ValueError("sets must be a (C, k) index table with 1 <= k <= %d" % SET_K_MAX)
        if np.any(sets >= self.N):
            raise ValueError("set entries must be flat voxel indices below N = %d (negative: padding)" % self.N)
        with torch.cuda.device(self.device):
            return self._set_statistics(sets.astype(np.int64), Prior(kernelfunc, lengths, weight_matrix(crossweights), float(gp_amp)),
                                        float(gp_sigma[2]) ** 2, observed, source, AK)

    def _set_statistics(self, sets, prior, sigma2, observed, source, AK):
        return self._set_logdet(self._set_grams(sets, prior, sigma2, source, AK), observed)

    def _set_grams(self, sets, prior, sigma2, source, AK):
        """The sweep of _set_statistics on its own: dict(idx, G, Kpp, sigma2) with the Grams G[c] of every set over all rows of V_d and
        the prior blocks.  A caller that adds rows to the factor keeps it resident and adds the new rows' part (add_rows)."""
        C_, k = sets.shape
        dev = self.device
        idx = torch.as_tensor(sets.astype(np.int32), device=dev)
        G = torch.zeros((C_, k, k), dtype=F64, device=dev)
        tiles = self._v_tiles(self._zsource(self.last["step"], AK, source), prior, AK)

        def sweep():
            first = True
            for (V,), n in tiles:
                hip.set_gram(idx, V, n, G, accumulate=not first, ncols=self.N)
                first = False
        self._timed("set_sweep", 0.0, sweep)
        # prior block K_dd(P, P): one block for whole z-columns (the prior is stationary), else one per set
        xyz = self.grid_points()
        base = _vertical_bases(sets, self.nz)
        if base is not None:
            col = torch.as_tensor(np.arange(k) + int(base[0]) if C_ else np.arange(k), device=dev)
            Kpp = torch.empty((k, k), dtype=F64, device=dev)
            prior.k_block(self, 2, 2, tuple(c[col] for c in xyz), tuple(c[col] for c in xyz), Kpp)
        else:
            Kpp = torch.empty((C_, k, k), dtype=F64, device=dev)
            pts = torch.as_tensor(np.maximum(sets, 0), device=dev)
            for c in range(C_):
                p = tuple(x[pts[c]] for x in xyz)
                prior.k_block(self, 2, 2, p, p, Kpp[c])
        return dict(idx=idx, G=G, Kpp=Kpp, sigma2=sigma2,
                    add_rows=lambda V, n: hip.set_gram(idx, V, n, G, accumulate=True, ncols=self.N))

    def _set_logdet(self, grams, observed):
        """(info_gain, path_var, sum_var, status) of _set_statistics from the Grams of _set_grams."""
        obs = None
        if observed is not None:
            obs = torch.as_tensor(np.asarray(observed, dtype=bool).reshape(-1)[:self.N].astype(np.uint8), device=self.device)
        out, status = self._timed("set_logdet", 0.0, lambda: hip.set_logdet(grams["G"], grams["Kpp"], grams["sigma2"], grams["idx"], self.N,
                                                                            observed=obs))
        return out[0], out[1], out[2], status

    def set_grams(self, sets, kernelfunc, lengths, crossweights, gp_amp, gp_sigma, source="auto"):
        """set_statistics in two parts for a caller that appends drill rows in between (append.py): the Grams of `sets` over every row
        of V_d, kept on the device; grams["add_rows"] is append_drill_rows' tile_hook, set_logdet_from(grams, observed) the statistics.
        Arguments and conditions of set_statistics."""
        from .engine import weight_matrix
        from .step import Prior
        last, AK = self._append_ready("set_grams()")
        sets = np.asarray(sets)
        if sets.ndim != 2 or not 1 <= sets.shape[1] <= SET_K_MAX:
            raise ValueError("sets must be a (C, k) index table with 1 <= k <= %d" % SET_K_MAX)
        if np.any(sets >= self.N):
            raise ValueError("set entries must be flat voxel indices below N = %d (negative: padding)" % self.N)
        with torch.cuda.device(self.device):
            return self._set_grams(sets.astype(np.int64), Prior(kernelfunc, lengths, weight_matrix(crossweights), float(gp_amp)),
                                   float(gp_sigma[2]) ** 2, source, AK)

    def set_logdet_from(self, grams, observed=None):
        """The statistics of set_statistics from set_grams' resident Grams (observed as there)."""
        with torch.cuda.device(self.device):
            return self._set_logdet(grams, observed)
