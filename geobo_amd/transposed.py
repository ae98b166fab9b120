"""The one-rank structured step on the fused n = 64 kernels (plan.Route.family "single") and the pieces of the transposed posterior
every family shares: mixin of engine.PosteriorEngine.

  _sym_ok / _assemble_AkA_sym   AkA from the three blocks of A K its lower triangle needs, through the lattice Gram (inversion.py:96)
  _lattice_Z                    rows of L^-1 A as lattice convolutions with the operator's stencil table (inversion.py:114 re-associated)
  _posterior_zpath              V = (L^-1 A3) K through the covariance kernels, squared and summed on the way out (inversion.py:114-117,238)
  _mean_rows, _drill_rows_ss    the mean as three rows through the covariance product; the rows behind the sensor rows
"""

import torch

from . import hip
from .operators import StreamedOperator

F64 = hip.F64


class TransposedPosteriorMixin:
    def _sym_ok(self, A_g, A_m):
        """The symmetric plan of A K / AkA (see _assemble_AK): the step will run in the transposed order (_zpath_static_ok) and AkA is
        the lattice Gram for both operators, boundary slabs through their spectra."""
        if not self._zpath_static_ok():
            return False
        return (self._gram is not None and self._gram.edge_supported() and self.Ms_pad == self.nx * self.ny
                and all(self._lam.get(f) is not None and self._lam[f][0] is A for f, A in (("grav", A_g), ("magn", A_m))))

    def _assemble_AkA_sym(self, step, AkA, AK, A_g, A_m):
        """AkA on one device from the blocks of A K the symmetric plan keeps, row block by row block through the lattice Gram:
        [grav rows -> grav columns], [grav rows -> magn columns] (transposed into the lower-left block, which is what the
        factorisation reads), [magn rows -> magn columns], drill rows -> both.  A quarter of the Gram's and of A K's work less than the
        block-column form, which computes the lower-left block from A_m K_10 as well."""
        gram, pl, ny, Msp, nc = self._gram, self.nx * self.nz, self.ny, self.Ms_pad, self.nc
        Md, off_d, props = step.Md, 2 * self.Ms_pad, step.props
        lam = {0: self._lam["grav"][1], 1: self._lam["magn"][1]}
        ops = {0: A_g, 1: A_m}

        def edge_cols(sp_, k, iy):
            A = ops[sp_]
            if isinstance(A, StreamedOperator):
                return A.edge[:, k * pl:(k + 1) * pl] if A.lattice is not None else A.slab_into(self._workspace2d("op_slab", Msp, pl), iy, iy + 1)
            return A[:, iy * pl:(iy + 1) * pl]

        def interior(X, nrows, sp_, out, S=None):
            # S: the block's rows met the Gram's y and x steps on their way out of the A K product (engine._gram_feed)
            if S is not None:
                gram.back_rows(S, nrows, out)
            else:
                gram.gram_rows(X, nrows, lam[sp_], out, 0, ny)

        def slabs(X, nrows, sp_, out):
            for k, iy in enumerate((0, ny - 1)):
                gram.edge_rows(X[:, iy * pl:], nrows, self._edge_spectrum(("grav", "magn")[sp_], k, edge_cols(sp_, k, iy)), out)

        def rows_times_AT(X, nrows, sp_, out, S=None):
            interior(X, nrows, sp_, out, S)
            slabs(X, nrows, sp_, out)
        blk = lambda r0, j: AK[r0:, props.index(j) * nc:(props.index(j) + 1) * nc]

        # step.mirror: A K holds the first rows of the magnetic block only (engine._assemble_AK_spectral); the block is centrosymmetric
        # (operator measured: engine._mirror_record), so its remaining rows are the point mirror of the computed ones
        Mm = step.mirror or self.Ms
        cross = step.cross_rows == "magn"

        def cross_from_magn():
            """AkA[magn rows, grav columns] from the step.mirror rows of A_m K_10 ("cross block from the magnetic rows"): row
            Ms-1-r of A_m K_10 is the point mirror of row r.  The interior slabs meet the gravity stencil table, which the Gram models as
            even in both offsets, so that part of row Ms-1-r is row r's with the sensor index reversed: a point mirror of the square
            block.  Gravity's boundary slabs have no such symmetry: they take the mirrored rows' own boundary planes (the x-reversed
            opposite planes of their partners) and are added behind the fill, for every row.  Then the upper-right block by transpose."""
            X, out, Ms = blk(Msp, 0), AkA[Msp:, 0:Msp], self.Ms
            interior(X, Mm, 0, out, S.get((1, 0)))
            hip.centro_fill(out[:Ms, :Ms], Ms, (Ms + 1) // 2)
            for dst, src in ((0, ny - 1), (ny - 1, 0)):
                hip.mirror_planes(X[:, src * pl:(src + 1) * pl], X[:, dst * pl:(dst + 1) * pl], Ms, 0, Ms - Mm, self.nx, self.nz)
            slabs(X, Ms, 0, out)
            hip.transpose(AkA[Msp:2 * Msp, :Msp], AkA[:Msp, Msp:2 * Msp])

        # step.grav_mirror: A K holds the interior part A_i K of the first rows of the gravity block, boundary planes only
        Mg = step.grav_mirror or self.Ms

        def grav_from_half():
            """AkA[grav rows, grav columns] from A_g = A_i + A_s, interior planes and boundary slabs ("gravity block from half
            its rows"):  A_i K A_i^T + E + E^T + A_s K A_s^T  with  E = A_i K A_s^T.  The first term is centrosymmetric -- the stencil
            table is even, which the Gram's eigen-data require -- so the step.grav_mirror rows the product ran give it whole.  E takes the
            boundary planes of A_i K for every row (the mirrored rows': the x-reversed opposite planes of their partners) against the
            slab spectra, no symmetry assumed; the last term the two planes of A_s K the product left in step.grav_slabs."""
            P, out, Ms = step.grav_iplanes, AkA[0:, 0:Msp], self.Ms          # (P: the two planes of A_i K, kept apart from the A K buffer)
            gram.back_rows(S[(0, 0)], Mg, out)
            hip.centro_fill(out[:Ms, :Ms], Ms, (Ms + 1) // 2)
            for dst, src in ((0, 1), (1, 0)):
                hip.mirror_planes(P[:, src * pl:(src + 1) * pl], P[:, dst * pl:(dst + 1) * pl], Ms, 0, Ms - Mg, self.nx, self.nz)
            E = self._workspace2d("grav_E", Ms, Ms)
            E.zero_()
            for k, iy in enumerate((0, ny - 1)):
                gram.edge_rows(P[:, k * pl:], Ms, self._edge_spectrum("grav", k, edge_cols(0, k, iy)), E)
            hip.sym_add(E, out[:Ms, :Ms], Ms)
            for k, iy in enumerate((0, ny - 1)):
                gram.edge_rows(step.grav_slabs[:, k * pl:], Ms, self._edge_spectrum("grav", k, edge_cols(0, k, iy)), out)

        def run():
            if step.grav_mirror:
                grav_from_half()
            else:
                rows_times_AT(blk(0, 0), self.Ms, 0, AkA[0:, 0:Msp], S.get((0, 0)))
            if not cross:
                rows_times_AT(blk(0, 1), self.Ms, 1, AkA[0:, Msp:2 * Msp], S.get((0, 1)))
            rows_times_AT(blk(Msp, 1), Mm, 1, AkA[Msp:, Msp:2 * Msp], S.get((1, 1)))
            if cross:
                cross_from_magn()
            else:
                hip.transpose(AkA[:Msp, Msp:2 * Msp], AkA[Msp:2 * Msp, :Msp])
            if Md:
                rows_times_AT(blk(off_d, 0), Md, 0, AkA[off_d:, 0:Msp])
                rows_times_AT(blk(off_d, 1), Md, 1, AkA[off_d:, Msp:2 * Msp])
        S = step.gram_S
        nfed = sum(Mg if s_ == 0 else Mm for s_, _ in S)
        self._timed("aka_lattice", gram.flops((Mg + 2 * Mm if cross else 2 * self.Ms + Mm) + 2 * Md - nfed, ny) + gram.flops_back(nfed), run)
        if step.mirror:
            # (after gram_rows AND edge_rows of the block: the fill copies finished rows; same stream, so it is ordered behind them)
            self._timed("aka_centro_fill", 0.0, lambda: hip.centro_fill(AkA[Msp:Msp + self.Ms, Msp:Msp + self.Ms], self.Ms, (self.Ms + 1) // 2))
        return self._finish_AkA(step, AkA)

    def _zpath_static_ok(self):
        """The one-rank transposed posterior on the fused kernels (plan.Route.single): one rank, fp64 A K, the radix-2 transform kernels
        and the Toeplitz y stage of this grid, unpadded sensor rows and voxel columns."""
        if not self.route.single or self.exchange:
            return False
        self._spectral_product()
        return True

    def _zpath_ok(self, step, AK):
        """... and the covariance generators of the step's A K assembly."""
        return (self._zpath_static_ok() and AK is not None and AK.dtype == F64
                and all((s_, j) in step.gens for s_ in (0, 1) for j in step.props))

    def _resident_operator(self, A, func):
        """A materialised copy of a forward operator that the route so far only kept implicitly (stencil table + boundary slabs)."""
        if not isinstance(A, StreamedOperator):
            return A
        R = self._workspace2d("A_" + func, self.Ms_pad, self.N_pad)
        xed, yed, zed = A.axes_dev
        hip.a_sens(A.func, A.Bv, A.locd, self.nx, self.ny, self.nz, xed, yed, zed, A.mul, A.div, R, plan=A.plan, ws=A.lws)
        return R

    def _lattice_Z(self, Lview, nrows, func, A, out, zx=False, edge=None):
        """out[r, :N] = sum_c Lview[r, c] A[c, :]  for a lattice-survey operator, without touching A: interior slabs through the stencil
        table's eigen-data, the two boundary slabs through their x-DFT spectra (lattice_gram.apply_transpose / edge_apply_transpose)."""
        gram, pl, ny = self._gram, self.nx * self.nz, self.ny
        lam = self._lam[func][1]
        hit = self._lamW.get((func, zx))
        if hit is None or hit[0] is not lam:
            hit = self._lamW[(func, zx)] = (lam, gram.transpose_tables3(lam) if zx else gram.transpose_tables(lam))
        if zx:
            gram.apply_transpose_zx(Lview, nrows, hit[1], out)      # rows as [iy][iz][ix]
        else:
            gram.apply_transpose(Lview, nrows, hit[1], out)
        self._lattice_slabs(Lview, nrows, func, A, [out[:, iy * pl:(iy + 1) * pl] for iy in (0, ny - 1)], zx=zx, edge=edge)

    def _lattice_slabs(self, Lview, nrows, func, A, outs, zx=False, edge=None):
        """The two boundary slabs iy = 0, ny - 1 of the rows of _lattice_Z into outs[0], outs[1] ((>= nrows x nx*nz) views), through the
        slabs' x-DFT spectra (lattice_gram.edge_apply_transpose)."""
        gram, pl, ny = self._gram, self.nx * self.nz, self.ny
        for k, iy in enumerate((0, ny - 1)):
            if edge is not None:                      # (row form: the two boundary slabs of every sensor, engine.operator)
                ycols = edge[k]
            elif isinstance(A, StreamedOperator) and A.lattice is not None:
                ycols = A.edge[:, k * pl:(k + 1) * pl]
            elif isinstance(A, StreamedOperator):
                ycols = A.slab_into(self._workspace2d("op_slab", self.Ms_pad, pl), iy, iy + 1)
            else:
                ycols = A[:, iy * pl:(iy + 1) * pl]
            key = (func, k)
            vt = self._edgeVt.get(key)
            if vt is None or vt[0] != ycols.data_ptr():
                vt = self._edgeVt[key] = (ycols.data_ptr(), gram.edge_eigen_t(ycols))
            gram.edge_apply_transpose(Lview, nrows, vt[1], outs[k], zx=zx)

    def _z_spectrum_ok(self):
        """Rows of L^-1 A enter the posterior's covariance product as spectra (spectral.ConvolvedRows; GEOBO_Z_SPECTRUM, default on):
        the zx form of the lattice application with the product formed inside the inverse kernel, the squaring inverse fused, the y
        stage on the matrix pipe with the one-pass two-term join."""
        sp = self._spectral
        f = sp.forms
        return bool(self.z_spectrum_on and f.zx and f.z_mul and sp.fused_ss() and sp.y_mfma and f.y_two_term == "y2t")

    def _convolved_rows(self, Lview, nrows, func, A):
        """spectral.ConvolvedRows of  Lview A  (the rows _lattice_Z(..., zx=True) would store): only their boundary slabs are computed
        here, 64 KB per row, into a compact buffer [row][k][iz][ix] of the operator's own."""
        from .spectral import ConvolvedRows
        gram, pl = self._gram, self.nx * self.nz
        lam = self._lam[func][1]
        hit = self._lamW.get((func, True))
        if hit is None or hit[0] is not lam:
            hit = self._lamW[(func, True)] = (lam, gram.transpose_tables3(lam))
        slab = self._workspace2d("Zslab_" + func, nrows, 2 * pl)
        self._lattice_slabs(Lview, nrows, func, A, [slab[:, k * pl:(k + 1) * pl] for k in (0, 1)], zx=True)
        return ConvolvedRows(gram, Lview, hit[1], slab)

    def _posterior_zpath(self, step, Linv, AK, u, A_g, A_m):
        """Posterior mean and variance in the TRANSPOSED order (round 3).  V = L^-1 (A3 K) is (L^-1 A3) K as well, and A3 is block
        diagonal: applying L^-1 to the forward operators costs M x Ms x N per operator -- independent of the number of property blocks
        and only over the operator's own columns of L^-1 -- where applying it to A K costs M^2 / 2 x N per property block:
            Z_g = Linv[:, grav columns] A_g,   Z_m = Linv[:, magn columns] A_m                (fp64 MFMA GEMMs, triangular X: 1.8e13 flop
                                                                                               at 64^3 instead of 3.6e13)
            V_j = Z_g K_0j + Z_m K_1j  (+ the drill term in the last rows only: L^-1 is lower triangular)
        and the covariance products run through the same spectral kernels as A K, with the inverse transform squaring and summing
        its output planes over the rows instead of storing them (geobo_xz2d_fold_inv_ss): V is never written.  The mean needs no V
        at all: mu = (A K)^T (L^-T u), two weighted column sums.  Same arithmetic up to summation order (inversion.py:114-117)."""
        props, Md, M_pad, amp = step.props, step.Md, step.M_pad, step.prior.amp
        sp, N, Msp, P_c = self._spectral, self.N, self.Ms_pad, len(props)
        nx, ny, nz = self.nx, self.ny, self.nz
        cws = self._workspace("colgemv_ws", (max(hip.colgemv_ws_doubles(M_pad, M_pad), hip.colgemv_ws_doubles(Msp, self.N_pad)),))
        w = self._timed("posterior_mean", 0.0, lambda: hip.colgemv(Linv, u, ws=cws))
        Zg = Zm = None
        zs = False
        # Z = L^-1[:, operator columns] A: on a lattice survey a (y, x) convolution of every row's sensor image with the operator's
        # stencil table (lattice_gram.apply_transpose: 2e8 flop per row), otherwise two triangular MFMA GEMMs (2.1e9 flop per row)
        lat = (self._gram is not None and self._gram.edge_supported() and Msp == nx * ny and self.route.opt("z_lattice")
               and all(self._lam.get(f) is not None and self._lam[f][0] is A for f, A in (("grav", A_g), ("magn", A_m))))
        if lat:
            gram = self._gram
            fl_conv, fl_slab = 3 * Msp * gram.flops(1, ny), 3 * Msp * 2 * 3 * 2.0 * 128 * 128 * 64

            zx = gram.zx_supported()          # rows of Z as [iy][iz][ix]: the fused inverse transform writes them, the products below follow
            # ... or not at all: the covariance product takes z as its Toeplitz axis, and the (iy, ix) plane the convolution produces per
            # (row, iz) goes through the product's forward transform inside the same kernel (spectral.ConvolvedRows).  Only the
            # boundary slabs are computed ahead of the product
            zs = zx and self._z_spectrum_ok()

            def zlattice():
                nonlocal Zg, Zm
                if zs:
                    Zg = self._convolved_rows(Linv[:2 * Msp, :Msp], 2 * Msp, "grav", A_g)
                    Zm = self._convolved_rows(Linv[Msp:2 * Msp, Msp:2 * Msp], Msp, "magn", A_m)
                    return
                Zg, Zm = self._workspace2d("Zg", 2 * Msp, N), self._workspace2d("Zm", Msp, N)
                self._lattice_Z(Linv[:2 * Msp, :Msp], 2 * Msp, "grav", A_g, Zg, zx=zx)
                self._lattice_Z(Linv[Msp:2 * Msp, Msp:2 * Msp], Msp, "magn", A_m, Zm, zx=zx)
            self._timed("posterior_zlattice", fl_slab if zs else fl_conv + fl_slab, zlattice)
            Ag = Am = None
            vec_of = lambda func, wv, out: self._lattice_Z(wv.view(1, -1), 1, func, A_g if func == "grav" else A_m, out)
        else:
            Ag = self._timed("a_sens_grav", 0.0, lambda: self._resident_operator(A_g, "grav"))
            Am = self._timed("a_sens_magn", 0.0, lambda: self._resident_operator(A_m, "magn"))
            tri = sum(min(256 * (bi + 1), Msp) for bi in range(Msp // 256)) * 256.0      # executed k-extent x rows of a triangular block
            fl = 2.0 * N * (2 * tri + 1.0 * Msp * Msp)
            alg = 2.0 * N * (2 * (Msp * (Msp + 1) / 2.0) + 1.0 * Msp * Msp)

            Zg, Zm = self._workspace2d("Zg", 2 * Msp, N), self._workspace2d("Zm", Msp, N)

            def zgemm():
                hip.gemm_nn(Linv[:2 * Msp, :Msp], Ag[:Msp, :N], Zg, x_lower=True)
                hip.gemm_nn(Linv[Msp:2 * Msp, Msp:2 * Msp], Am[:Msp, :N], Zm, x_lower=True)
            self._timed("posterior_zgemm", fl, zgemm, alg=alg)
            vec_of = lambda func, wv, out: hip.colgemv((Ag if func == "grav" else Am)[:Msp, :N], wv, out=out[0], ws=cws)
        mu_l = self._timed("posterior_mean", 0.0, lambda: self._mean_rows(step, w, vec_of)).reshape(-1)
        zx = lat and zx
        zs = zx and zs
        ss, tg, tm, y2s, voxel_order = self._ss_cubes(step, zx, toeplitz_z=zs)
        shared = y2s is not None and P_c == 2
        self._timed("posterior_spectral", sp.flops_ss(Msp, Msp, P_c, shared) + (fl_conv if zs else 0.0),
                    lambda: sp.reduce_ss(Zg, 2 * Msp, tg, Zm, Msp, tm, ss, y2s=y2s), valu=sp.valu_ss(Msp, Msp, P_c, shared))
        ssum = torch.stack([voxel_order(t) for t in ss])                                  # (P_c, N)
        if Md:
            # K_2j[drill voxels, :]: the drill rows of A K, already there (fp64, every voxel column: _zpath_ok), zero rows behind them
            Kd = [AK[2 * Msp:, jj * self.nc:(jj + 1) * self.nc] for jj in range(P_c)] if self.nc >= N and self.c0 == 0 else None
            ssum = ssum + self._timed("posterior_drill_rows", 0.0, lambda: self._drill_rows_ss(
                step, Linv, 0, Md, (lambda Lv, n, func, out: self._lattice_Z(Lv, n, func, A_g if func == "grav" else A_m, out)) if lat else None, Ag, Am,
                Kd=Kd, y2s=None if zx else y2s))             # (zx: y2s holds the tables of the transposed planes)
        return mu_l, (amp * 1.0 - ssum).reshape(-1)

    def _ss_cubes(self, step, zx, toeplitz_z=False):
        """What both transposed posteriors hand to sp.reduce_ss, and the way back: (ss, tg, tm, y2s, voxel_order).  ss: the zeroed partial
        cubes post_ss_* (sp.ss_slots() slots per block); tg / tm: the step's generators of the blocks (0, j) / (1, j), as tables of
        transposed planes where the rows of Z come as [iy][iz][ix] (zx); y2s: their three-product tables -- blocks (0, 1) and (1, 0) of
        a symmetric prior coincide: three y-stage products per two-term row instead of four.  voxel_order(t): one block's cube summed
        over its slots, N values in voxel order (iy, ix, iz).
        toeplitz_z: the rows are spectral.ConvolvedRows -- generators of the permuted tables (one single-row transform per block:
        sp.eigenvalues(..., toeplitz_z=True)), cubes come back as [iz][iy][ix]."""
        props, sp, nx, ny, nz = step.props, self._spectral, self.nx, self.ny, self.nz
        ss = [self._workspace("post_ss_%d" % jj, (sp.ss_slots(), ny, nx * nz)) for jj in range(len(props))]
        for t in ss:
            t.zero_()
        if toeplitz_z:
            tg, tm = ([sp.eigenvalues(step.prior.table(self, s_, j), toeplitz_z=True) for j in props] for s_ in (0, 1))
            y2s = sp.y2s_tables(tg, tm) if tuple(props[:2]) == (0, 1) else None
            return ss, tg, tm, y2s, lambda t: t.sum(0).view(nz, ny, nx).permute(1, 2, 0).reshape(-1)
        swap = (lambda g: g.view(ny, sp.Px, sp.Pz).transpose(1, 2).contiguous().view(-1)) if zx else (lambda g: g)
        tg, tm = [swap(step.gens[(0, j)]) for j in props], [swap(step.gens[(1, j)]) for j in props]
        y2s = sp.y2s_tables(tg, tm) if tuple(props[:2]) == (0, 1) else None
        if zx:                                                                            # planes came out as [iz][ix]
            return ss, tg, tm, y2s, lambda t: t.sum(0).view(ny, nz, nx).transpose(1, 2).reshape(-1)
        return ss, tg, tm, y2s, lambda t: t.sum(0).reshape(-1)

    def _mean_rows(self, step, w, vec_of):
        """Posterior mean (P_c, N):  mu_j = (A3 K)[:, block j]^T w  re-associated as  K_.j (A3^T w)  -- the covariance blocks are
        symmetric, so three N-vectors (A_g^T w_g, A_m^T w_m, the drill weights scattered to their voxels) go through the covariance
        product as ONE row each (0.3 ms) where the weighted column sums of A K read all of it (35 GB at 64^3: 6 ms).
        vec_of(func, weights, out (1 x N)): out = A_func^T weights.  w = L^-T u (inversion.py:105,115)."""
        props, sel_t, Md = step.props, step.sel_t, step.Md
        sp, N, Msp, P_c = self._spectral, self.N, self.Ms_pad, len(props)
        V = self._workspace2d("mean_rows", 4, N)
        vec_of("grav", w[:Msp], V[0:1])
        vec_of("magn", w[Msp:2 * Msp], V[1:2])
        terms = [(V[0:1], 0), (V[1:2], 1)]
        if Md:
            V[2].zero_()
            V[2][sel_t] = w[2 * Msp:2 * Msp + Md]
            terms.append((V[2:3], 2))
        mu = torch.zeros((P_c, N), dtype=F64, device=self.device)
        tmp = [self._workspace2d("mean_tmp_%d" % jj, 2, N) for jj in range(P_c)]
        for rows, s_ in terms:
            gens = [step.gens[(s_, j)] if s_ < 2 else sp.eigenvalues(step.prior.table(self, s_, j)) for j in props]
            sp.product(rows, 1, gens, tmp)
            for jj in range(P_c):
                mu[jj].add_(tmp[jj][0])
        return mu

    DRILL_SS_SLOTS = 4      # partial sums per column of the drill rows' squares (geobo_sumsq_accum: one thread per slot and column pair)

    def _drill_rows_ss(self, step, Linv, d0, nd, lattice_Z, Ag, Am, Kd=None, y2s=None):
        """(P_c, N) sums of squares of V = L^-1 (A3 K) over the drill rows d0 .. d0 + nd of the row block behind the sensor rows:
        L^-1 is lower triangular, so only THESE rows see the drill columns.  Tiles of up to 128 rows, three terms (gravity, magnetic,
        drill block rows of K).  lattice_Z(Lview, n, func, out): rows of L^-1 A on a lattice survey; None: MFMA GEMMs against the
        resident operators Ag / Am (whole 128-row tiles).
        Kd[jj]: (>= Md rounded up to 16, >= N) view of K_2j[drill voxels, :] -- the drill rows of A K (engine._cov_rows), zero rows
        behind them.  With it, on a lattice survey whose y stage joins two terms (sp.has_two_term_product) in batches that hold a
        whole tile (sp.R >= 128): _drill_rows_ss_short.  Otherwise three storing products, added and squared here.
        y2s: sp.y2s_tables of the step's untransposed tables where the caller has them (the short form builds them otherwise)."""
        props, sel_t, Md = step.props, step.sel_t, step.Md
        sp, N, Msp, P_c, T = self._spectral, self.N, self.Ms_pad, len(props), 128
        if Kd is not None and lattice_Z is not None and sp.has_two_term_product(P_c) and sp.R >= T:
            return self._drill_rows_ss_short(step, Linv, d0, nd, lattice_Z, Kd, y2s)
        Zgd, Zmd = (self._workspace2d(nm, T, N) for nm in ("Zg_d", "Zm_d"))
        Vd = [self._workspace2d("Vd_%d" % jj, T, N) for jj in range(P_c)]
        tmp = [self._workspace2d("Vt_%d" % jj, T, N) for jj in range(P_c)]
        gens_g, gens_m = [step.gens[(0, j)] for j in props], [step.gens[(1, j)] for j in props]
        acc = torch.zeros((P_c, N), dtype=F64, device=self.device)
        Zdd = self._workspace2d("Zd_d", T, N)
        gens_d = [sp.eigenvalues(step.prior.table(self, 2, j)) for j in props]
        for c0 in range(d0, d0 + nd, T):
            n = min(T, d0 + nd - c0)
            b0 = 2 * Msp + c0
            if lattice_Z is not None:
                lattice_Z(Linv[b0:b0 + n, :Msp], n, "grav", Zgd)
                lattice_Z(Linv[b0:b0 + n, Msp:2 * Msp], n, "magn", Zmd)
            else:
                nt = min(T, Linv.shape[0] - b0)          # (M_pad is a multiple of 256: whole tiles unless the caller's share starts mid-tile)
                hip.gemm_nn(Linv[b0:b0 + nt, :Msp], Ag[:Msp, :N], Zgd)
                hip.gemm_nn(Linv[b0:b0 + nt, Msp:2 * Msp], Am[:Msp, :N], Zmd)
            Zdd[:n].zero_()
            Zdd[:n, sel_t] = Linv[b0:b0 + n, 2 * Msp:2 * Msp + Md]
            sp.product(Zgd, n, gens_g, Vd)
            for Zx, gx in ((Zmd, gens_m), (Zdd, gens_d)):
                sp.product(Zx, n, gx, tmp)
                for jj in range(P_c):
                    Vd[jj][:n].add_(tmp[jj][:n])
            for jj in range(P_c):
                acc[jj].add_((Vd[jj][:n] ** 2).sum(0))
        return acc

    def _drill_rows_ss_short(self, step, Linv, d0, nd, lattice_Z, Kd, y2s=None):
        """_drill_rows_ss without the third spectral product and without torch arithmetic: the two sensor terms meet in the y stage
        (sp.product_two_term: ONE stored V per block), the drill term is the small product L^-1[rows, drill columns] Kd[jj] (Md deep:
        K_2j[drill voxels, :] is already there), and geobo_sumsq_accum adds the two, squares and sums over the rows."""
        props, Md = step.props, step.Md
        sp, N, Msp, P_c, T = self._spectral, self.N, self.Ms_pad, len(props), 128
        Zgd, Zmd = (self._workspace2d(nm, T, N) for nm in ("Zg_d", "Zm_d"))
        Vd = [self._workspace2d("Vd_%d" % jj, T, N) for jj in range(P_c)]
        tmp = [self._workspace2d("Vt_%d" % jj, T, N) for jj in range(P_c)]
        gens_g, gens_m = [step.gens[(0, j)] for j in props], [step.gens[(1, j)] for j in props]
        if y2s is None and tuple(props[:2]) == (0, 1):
            y2s = sp.y2s_tables(gens_g, gens_m, check=False)   # (the caller's pass over these blocks has left their sym_residual)
        kd = (Md + 15) // 16 * 16
        Ld = self._workspace2d("Ld_d", T, kd)                  # the rows' drill columns of L^-1, zero padded to the GEMM's extents
        ss = self._workspace("drill_ss", (P_c, self.DRILL_SS_SLOTS, N))
        ss.zero_()
        for c0 in range(d0, d0 + nd, T):
            n = min(T, d0 + nd - c0)
            b0 = 2 * Msp + c0
            lattice_Z(Linv[b0:b0 + n, :Msp], n, "grav", Zgd)
            lattice_Z(Linv[b0:b0 + n, Msp:2 * Msp], n, "magn", Zmd)
            sp.product_two_term(Zgd, Zmd, n, gens_g, gens_m, Vd, y2s=y2s)
            Ld.zero_()
            Ld[:n, :Md] = Linv[b0:b0 + n, 2 * Msp:2 * Msp + Md]
            for jj in range(P_c):
                hip.gemm_batched(True, T, N, kd, Ld, Ld.stride(0), 0, Kd[jj], Kd[jj].stride(0), 0, tmp[jj], tmp[jj].stride(0), 0, n, N, 1)
                hip.sumsq_accum(Vd[jj], tmp[jj], n, ss[jj])
        return ss.sum(1)
