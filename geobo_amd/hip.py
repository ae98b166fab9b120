"""Tensor-level wrappers over the C ABI (include/geobo_hip.h).

PyTorch is plumbing here: device memory (torch.float64 CUDA tensors), the current HIP stream and
torch.distributed; every numerical operation of the hot path is a hand-written gfx950 kernel in
libgeobo_hip.so.  All functions are asynchronous on torch's current stream.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

F64 = torch.float64

KERNEL_IDS = {"d2": 0, "exp": 1, "exp_x": 2, "matern32": 3, "matern32_x": 4, "sparse": 5, "sparse_x": 6,
              # partial derivatives in the lengths (log-likelihood gradient): self families d/dl, cross families d/dl1, d/dl2
              "exp_dl": 7, "exp_x_dl1": 8, "exp_x_dl2": 9, "matern32_dl": 10, "matern32_x_dl1": 11, "matern32_x_dl2": 12,
              "sparse_dl": 13, "sparse_x_dl1": 14, "sparse_x_dl2": 15}
FUNC_IDS = {"grav": 0, "magn": 1}
# kernel-instance tables and padding units: ONE definition (plan.py, which decides routes from them on the CPU); re-exported here
from .plan import (PAD_M, PAD_N, SPECTRAL_AXIS_N, SPECTRAL_Y3T_NY, SPECTRAL_Y_NY, TOEPLITZ_ADD_NY, TOEPLITZ_NY, TOEPLITZ_Y2T_NY,  # noqa: E402,F401
                   XZ2D_FOLD_N, XZ2D_SHAPES, YMUL_SHAPES)


def kernel_id(name, cross, deriv=None):
    """(kernelfunc, is-cross-block) -> family id of include/geobo_hip.h (kernels.py:183-195).
    deriv: None = the covariance itself; 1 / 2 = its partial derivative in l1 / l2 (the self families have one length: deriv 1)."""
    if name not in ("exp", "matern32", "sparse"):
        raise ValueError("unknown kernelfunc %r (expected 'sparse', 'exp' or 'matern32')" % (name,))
    if deriv is None:
        return KERNEL_IDS[name + ("_x" if cross else "")]
    if isinstance(deriv, bool) or deriv not in (1, 2):
        raise ValueError("deriv must be None, 1 or 2, got %r" % (deriv,))
    if not cross:
        if deriv != 1:
            raise ValueError("the self family %r has one length: deriv must be 1" % (name,))
        return KERNEL_IDS[name + "_dl"]
    return KERNEL_IDS["%s_x_dl%d" % (name, deriv)]


def pad_m(m):
    return (int(m) + PAD_M - 1) // PAD_M * PAD_M


def pad_n(n):
    return (int(n) + PAD_N - 1) // PAD_N * PAD_N


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.GeoboHipUnavailable("no MI355X / ROCm device visible: the GeoBO hot path has no CPU fallback")
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _chk(t, name, dtype=F64):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype):
        raise TypeError("%s must be a CUDA %s tensor" % (name, dtype))
    return t


def _ptrs(ts, name):
    """The device pointers of the fp64 tensors `ts` as a C array of void*."""
    return (C.c_void_p * len(ts))(*[_chk(t, name).data_ptr() for t in ts])


def _rowmajor(t, name):
    _chk(t, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("%s must be 2-D with unit column stride" % name)
    return t.stride(0)


def version():
    return _lib.load().geobo_version()


F32 = torch.float32


def k_block(kid, rows_xyz, cols_xyz, l1, l2, w, amp, out):
    """out[r,c] = w*amp*k(|rows_r - cols_c|^2).  rows_xyz / cols_xyz: tuples of three 1-D tensors; out fp64 or fp32."""
    lib = require_gpu()
    rx, ry, rz = (_chk(t, "rows") for t in rows_xyz)
    cx, cy, cz = (_chk(t, "cols") for t in cols_xyz)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype in (F64, F32) and out.dim() == 2 and out.stride(1) == 1):
        raise TypeError("out must be a 2-D CUDA float64 / float32 tensor with unit column stride")
    ld = out.stride(0)
    nr, nc = rx.numel(), cx.numel()
    assert out.shape[0] >= nr and out.shape[1] >= nc
    fn, name = (lib.geobo_k_block, "geobo_k_block") if out.dtype == F64 else (lib.geobo_k_block_f32, "geobo_k_block_f32")
    _lib.check(fn(kid, _p(rx), _p(ry), _p(rz), nr, _p(cx), _p(cy), _p(cz), nc, float(l1), float(l2), float(w), float(amp),
                  _p(out), ld, _stream()), name)
    return out


def k_block_grid(table, nx, ny, nz, rows, col0, out, row0=0, nr=None):
    """Covariance block on the regular grid gathered from the lattice table of cov_table: out[r, c] for row voxels `rows` (int64
    device tensor of flat voxel indices, or None for the range row0 .. row0 + nr) and column voxels col0 .. col0 + out.shape[1]."""
    lib = require_gpu()
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype in (F64, F32) and out.dim() == 2 and out.stride(1) == 1):
        raise TypeError("out must be a 2-D CUDA float64 / float32 tensor with unit column stride")
    if rows is not None:
        assert rows.dtype == torch.int64 and rows.is_cuda and rows.is_contiguous()
        nr = rows.numel()
    nr = out.shape[0] if nr is None else int(nr)
    assert out.shape[0] >= nr and _chk(table, "table").numel() >= 2 * nx * ny * nz
    _lib.check(lib.geobo_k_block_grid(int(nx), int(ny), int(nz), _p(table), C.c_void_p(rows.data_ptr()) if rows is not None else None,
                                      int(row0), nr, int(col0), out.shape[1], 1 if out.dtype == F32 else 0, _p(out), out.stride(0),
                                      _stream()), "geobo_k_block_grid")
    return out


def lattice_wbuild(rows, Py, Px, nz, lamW, lhat, W):
    """W[r][kx][iz][ky] = lamW[kx][iz][ky] * lhat[r][ky][kx]  (geobo_lattice_wbuild)."""
    lib = require_gpu()
    done = 0
    while done < rows:
        nb = min(rows - done, 65535)
        _lib.check(lib.geobo_lattice_wbuild(nb, int(Py), int(Px), int(nz), _p(_chk(lamW, "lamW")),
                                            C.c_void_p(_chk(lhat, "lhat").data_ptr() + done * Py * Px * 8),
                                            C.c_void_p(_chk(W, "W").data_ptr() + done * Px * nz * Py * 8), _stream()), "geobo_lattice_wbuild")
        done += nb


def lattice_wplanes(rows, Py, Px, nz, lam3, lhat, W):
    """W[r][iz][ky][kx] = lam3[iz][ky][kx] * lhat[r][ky][kx]  (geobo_lattice_wplanes)."""
    lib = require_gpu()
    done = 0
    while done < rows:
        nb = min(rows - done, 65535)
        _lib.check(lib.geobo_lattice_wplanes(nb, int(Py), int(Px), int(nz), _p(_chk(lam3, "lam3")),
                                             C.c_void_p(_chk(lhat, "lhat").data_ptr() + done * Py * Px * 8),
                                             C.c_void_p(_chk(W, "W").data_ptr() + done * nz * Py * Px * 8), _stream()), "geobo_lattice_wplanes")
        done += nb


def xz2d_fold_inv_strided(n, rows, ppr, src, in_row, in_plane, Fx, Fz, out, out_row, out_plane, out_rowstride):
    """Inverse radix-2 transform with strided output rows (geobo_xz2d_fold_inv_strided)."""
    lib = require_gpu()
    _lib.check(lib.geobo_xz2d_fold_inv_strided(int(n), int(rows), int(ppr), _p(_chk(src, "src")), int(in_row), int(in_plane), _p(_chk(Fx, "Fx")),
                                               _p(_chk(Fz, "Fz")), _p(_chk(out, "out")), int(out_row), int(out_plane), int(out_rowstride),
                                               _stream()), "geobo_xz2d_fold_inv_strided")


def xz2d_fold_inv_mul(n, rows, ppr, a, a_plane, b, b_row, Fx, Fz, out, out_row, out_plane, out_rowstride):
    """Inverse radix-2 transform of the planes a[p] * b[r] (elementwise), strided output rows (geobo_xz2d_fold_inv_mul)."""
    lib = require_gpu()
    _lib.check(lib.geobo_xz2d_fold_inv_mul(int(n), int(rows), int(ppr), _p(_chk(a, "a")), int(a_plane), _p(_chk(b, "b")), int(b_row),
                                           _p(_chk(Fx, "Fx")), _p(_chk(Fz, "Fz")), _p(_chk(out, "out")), int(out_row), int(out_plane),
                                           int(out_rowstride), _stream()), "geobo_xz2d_fold_inv_mul")


def xz2d_fold_conv_fwd(n, rows, ppr, a, a_plane, b, b_row, slab, slab_row, Fx, Fz, out, out_row, out_plane):
    """Forward radix-2 spectrum of the inverse transform of the planes a[p] * b[r], rows 0 and n - 1 of every plane taken from
    slab[r][k][p][n] (None: zeros); the planes themselves are never stored (geobo_xz2d_fold_conv_fwd)."""
    lib = require_gpu()
    P = 4 * n * n
    room = lambda t, name: _chk(t, name).untyped_storage().nbytes() // 8 - t.storage_offset()      # doubles behind the first element
    assert room(a, "a") >= (ppr - 1) * a_plane + P and room(b, "b") >= (rows - 1) * b_row + P
    assert room(out, "out") >= (rows - 1) * out_row + (ppr - 1) * out_plane + P
    assert slab is None or room(slab, "slab") >= (rows - 1) * slab_row + 2 * ppr * n
    _lib.check(lib.geobo_xz2d_fold_conv_fwd(int(n), int(rows), int(ppr), _p(a), int(a_plane), _p(b), int(b_row),
                                            _p(slab) if slab is not None else None, int(slab_row), _p(_chk(Fx, "Fx")), _p(_chk(Fz, "Fz")),
                                            _p(out), int(out_row), int(out_plane), _stream()), "geobo_xz2d_fold_conv_fwd")


def colgemv(X, v, out=None, ws=None):
    """out[c] = sum_r X[r, c] v[r]  (X: 2-D row-major CUDA float64, unit column stride, even width)."""
    lib = require_gpu()
    ld = _rowmajor(X, "X")
    m, n = X.shape
    assert _chk(v, "v").numel() >= m
    if out is None:
        out = torch.empty(n, dtype=F64, device=X.device)
    nbytes = lib.geobo_colgemv_ws_bytes(m, n)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(max(nbytes // 8, 1), dtype=F64, device=X.device)
    _lib.check(lib.geobo_colgemv(m, n, _p(X), ld, _p(v), _p(_chk(out, "out")), _p(ws), ws.numel() * 8, _stream()), "geobo_colgemv")
    return out


def rowgemv(X, v, out=None):
    """out[r] = sum_c X[r, c] * v[c] (geobo_rowgemv): a forward operator applied to a model, data = A rho."""
    lib = require_gpu()
    ld = _rowmajor(X, "X")
    m, n = X.shape
    assert v.numel() >= n and v.dtype == F64 and v.is_cuda
    if out is None:
        out = torch.empty(m, dtype=F64, device=X.device)
    _lib.check(lib.geobo_rowgemv(int(m), int(n), _p(X), int(ld), _p(v), _p(out), _stream()), "geobo_rowgemv")
    return out


def sumsq_accum(a, b, rows, ss):
    """ss[slot][c] += sum over the rows r = slot (mod slots) of (a[r, c] + b[r, c])^2  (geobo_sumsq_accum); b may be None.
    a, b: 2-D row-major views (>= rows x n); ss: (slots, n) view with unit column stride."""
    lib = require_gpu()
    lda = _rowmajor(a, "a")
    n = ss.shape[1]
    assert a.shape[1] >= n and a.shape[0] >= rows and _rowmajor(ss, "ss") >= n
    _lib.check(lib.geobo_sumsq_accum(int(rows), int(n), _p(a), lda, _p(b) if b is not None else None,
                                     _rowmajor(b, "b") if b is not None else 0, ss.shape[0], _p(ss), ss.stride(0), _stream()),
               "geobo_sumsq_accum")
    return ss


def lamdot_z(batch, planes, px, nz, D, lam, out):
    """out[b][o] = sum_z D[b][o][z] * lam[b % planes][o][z]  (geobo_lamdot_z)."""
    lib = require_gpu()
    _lib.check(lib.geobo_lamdot_z(int(batch), int(planes), int(px), int(nz), _p(_chk(D, "D")), _p(_chk(lam, "lam")), _p(_chk(out, "out")),
                                  _stream()), "geobo_lamdot_z")
    return out


def centro_fill(B, n, r0):
    """B[r, c] = B[n-1-r, n-1-c] for r0 <= r < n (geobo_centro_fill): the second half of a centrosymmetric block from its first half.
    B: 2-D row-major view with at least n rows and columns."""
    lib = require_gpu()
    ld = _rowmajor(B, "B")
    assert B.shape[0] >= n and B.shape[1] >= n
    _lib.check(lib.geobo_centro_fill(_p(B), int(ld), int(n), int(r0), _stream()), "geobo_centro_fill")
    return B


def transpose(src, dst):
    """dst[c, r] = src[r, c] (geobo_transpose); src, dst: 2-D row-major views that do not overlap, dst at least src's shape transposed."""
    lib = require_gpu()
    lds, ldd = _rowmajor(src, "src"), _rowmajor(dst, "dst")
    rows, cols = src.shape
    assert dst.shape[0] >= cols and dst.shape[1] >= rows
    _lib.check(lib.geobo_transpose(int(rows), int(cols), _p(src), int(lds), _p(dst), int(ldd), _stream()), "geobo_transpose")
    return dst


def mirror_rows(X, m, r0, nb, nz):
    """X[r, (b, z)] = X[m-1-r, (nb-1-b, z)] for r0 <= r < m (geobo_mirror_rows): rows of A K under the point mirror of a lattice survey."""
    lib = require_gpu()
    ld = _rowmajor(X, "X")
    assert X.shape[0] >= m and X.shape[1] >= nb * nz
    _lib.check(lib.geobo_mirror_rows(_p(X), int(ld), int(m), int(r0), int(nb), int(nz), _stream()), "geobo_mirror_rows")
    return X


def mirror_planes(src, dst, m, r0, r1, nx, nz):
    """dst[m-1-r, (x, z)] = src[r, (nx-1-x, z)] for r0 <= r < r1 (geobo_mirror_planes): one (x, z) plane per row under the point mirror.
    src, dst: 2-D row-major views starting at the plane read / written, at least m rows and nx*nz columns; they must not overlap."""
    lib = require_gpu()
    lds, ldd = _rowmajor(src, "src"), _rowmajor(dst, "dst")
    assert src.shape[0] >= r1 and dst.shape[0] >= m and src.shape[1] >= nx * nz and dst.shape[1] >= nx * nz
    _lib.check(lib.geobo_mirror_planes(_p(src), int(lds), _p(dst), int(ldd), int(m), int(r0), int(r1), int(nx), int(nz), _stream()),
               "geobo_mirror_planes")
    return dst


def sym_add(E, B, n):
    """B[r, c] += E[r, c] + E[c, r] for r, c < n (geobo_sym_add).  E, B: 2-D row-major views of at least n x n that do not overlap."""
    lib = require_gpu()
    lde, ldb = _rowmajor(E, "E"), _rowmajor(B, "B")
    assert min(E.shape) >= n and min(B.shape) >= n
    _lib.check(lib.geobo_sym_add(int(n), _p(E), int(lde), _p(B), int(ldb), _stream()), "geobo_sym_add")
    return B


def slab_pair_y(ny, C, rows, src, tab, out, plane=None):
    """out[r, 0] = t(0) src[r, 0] + t(ny-1) src[r, 1], out[r, 1] = t(ny-1) src[r, 0] + t(0) src[r, 1] per mode c < C, t(d) = tab[d*C + c]
    (geobo_slab_pair_y): the y stage of rows that are zero between their boundary planes.  src, out: [rows][2][plane] (row-major
    (rows, >= 2 plane) views, or flat buffers of rows of 2 plane doubles); tab: the generator table [ny][C]."""
    lib = require_gpu()
    plane = int(C if plane is None else plane)
    ld = lambda t: t.stride(0) if t.dim() == 2 else 2 * plane
    room = lambda t: _chk(t, "planes").untyped_storage().nbytes() // 8 - t.storage_offset()
    assert all(t.dim() == 1 or t.stride(1) == 1 for t in (src, out)) and _chk(tab, "tab").is_contiguous() and tab.numel() >= ny * C
    assert rows == 0 or min(room(src) - (rows - 1) * ld(src), room(out) - (rows - 1) * ld(out)) >= plane + C
    _lib.check(lib.geobo_slab_pair_y(int(ny), int(C), plane, int(rows), _p(src), int(ld(src)), _p(tab), _p(out), int(ld(out)), _stream()),
               "geobo_slab_pair_y")
    return out


def mirror_dev_ws_doubles():
    return require_gpu().geobo_mirror_dev_ws_bytes() // 8


def mirror_dev(a, b, rows, nx, nz, out=None, ws=None):
    """out[0] = max |a[r, (x, z)] - b[rows-1-r, (nx-1-x, z)]|, out[1] = max(|a|, |b|)  (geobo_mirror_dev); a, b: 2-D row-major views
    of `rows` rows.  Returns the 2-element device tensor (no host read)."""
    lib = require_gpu()
    lda, ldb = _rowmajor(a, "a"), _rowmajor(b, "b")
    assert a.shape[0] >= rows and b.shape[0] >= rows
    nws = lib.geobo_mirror_dev_ws_bytes() // 8
    if ws is None:
        ws = torch.empty(nws, dtype=F64, device=a.device)
    if out is None:
        out = torch.empty(2, dtype=F64, device=a.device)
    _lib.check(lib.geobo_mirror_dev(_p(a), int(lda), _p(b), int(ldb), int(rows), int(nx), int(nz), _p(_chk(out, "out")), _p(_chk(ws, "ws")),
                                    ws.numel() * 8, _stream()), "geobo_mirror_dev")
    return out


def convert(src, dst):
    """dst[r, c] = src[r, c] across fp64 <-> fp32 (2-D views, unit column stride, even widths and leading dimensions)."""
    lib = require_gpu()
    assert src.shape == dst.shape and src.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1
    assert {src.dtype, dst.dtype} == {F64, F32}, "one side float64, the other float32"
    _lib.check(lib.geobo_convert(1 if dst.dtype == F32 else 0, _p(src), src.stride(0), _p(dst), dst.stride(0), src.shape[0],
                                 src.shape[1], _stream()), "geobo_convert")
    return dst


def round_f32_(x):
    """In place x <- (double)(float)x."""
    lib = require_gpu()
    assert _chk(x, "x").is_contiguous()
    _lib.check(lib.geobo_round_f32(_p(x), x.numel(), _stream()), "geobo_round_f32")
    return x


def k_eval(kid, d2, l1, l2, w=1.0, amp=1.0):
    lib = require_gpu()
    d2 = _chk(d2, "d2").contiguous()
    out = torch.empty_like(d2)
    _lib.check(lib.geobo_k_eval(kid, _p(d2), d2.numel(), float(l1), float(l2), float(w), float(amp), _p(out), _stream()),
               "geobo_k_eval")
    return out


def lattice_plan(loc, xe, ye, ze, nx, ny, nz, device="cuda"):
    """Host-side check for the lattice form of A_sens (geobo_a_sens_lattice): the sensors occupy every column of an nx x ny
    lattice at one height AND every node offset xe[j] - sx, ye[i] - sy (planes 1 .. ny-1) is bit-identical for all pairs with
    the same index difference -- then the lattice kernels reproduce geobo_a_sens exactly.  Returns None otherwise (irregular
    survey, or spacings whose differences round differently from pair to pair: the direct kernel is used)."""
    loc = np.asarray(loc, dtype=np.float64)
    xe, ye, ze = (np.asarray(v, dtype=np.float64) for v in (xe, ye, ze))
    if ny < 3 or nz % 2 or loc.shape != (nx * ny, 3) or np.unique(loc[:, 2]).size != 1:
        return None
    ux, uy = np.unique(loc[:, 0]), np.unique(loc[:, 1])
    if ux.size != nx or uy.size != ny:
        return None
    jx, jy = np.searchsorted(ux, loc[:, 0]), np.searchsorted(uy, loc[:, 1])
    if np.unique(jy * nx + jx).size != nx * ny:
        return None
    X = xe[:, None] - ux[None, :]                 # (nx+1, nx): offset of node j from lattice column t
    Y = ye[1:ny, None] - uy[None, :]              # (ny-1, ny): planes 1 .. ny-1 (planes 0 and ny carry the 1e6 padding)
    # every offset must depend on the index difference only, bit for bit: scatter by difference, then compare the whole matrix
    dix = np.arange(nx + 1)[:, None] - np.arange(nx)[None, :] + nx - 1            # d = j - t        -> 0 .. 2nx-1
    diy = np.arange(1, ny)[:, None] - np.arange(ny)[None, :] + ny - 2             # d = i - t, i>=1  -> 0 .. 2ny-3
    dxv, dyv = np.empty(2 * nx), np.empty(2 * ny - 2)
    dxv[dix.ravel()] = X.ravel()
    dyv[diy.ravel()] = Y.ravel()
    if not ((dxv[dix] == X).all() and (dyv[diy] == Y).all()):
        return None
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(device)
    return dict(dxv=dev(dxv, np.float64), dyv=dev(dyv, np.float64), dzv=dev(ze - loc[0, 2], np.float64),
                jx=dev(jx, np.int32), jy=dev(jy, np.int32), rowmajor=bool((jy * nx + jx == np.arange(nx * ny)).all()))


def a_sens(func, B, loc, nx, ny, nz, xe, ye, ze, scale_mul, scale_div, out, iy0=0, iy1=None, plan=None, rows=None, ws=None,
           col_origin=0):
    """Forward operator rows for the sensors in `loc`; optionally only the voxel slab iy0 <= iy < iy1.
    plan (lattice_plan) + rows (slice of the plan's sensors that `loc` holds): interior slabs by the lattice kernels, the
    two 1e6-padded boundary slabs by the direct kernel.
    col_origin: voxel column that out[:, 0] stands for: 0 (full-width operator) or the first column of a compact buffer that holds
    only a slab; the library checks that the requested columns lie inside a buffer row and applies the offset itself."""
    lib = require_gpu()
    ld = _rowmajor(out, "A")
    col_origin = int(col_origin)
    base = _p(out)
    loc = _chk(loc, "loc").contiguous()
    Bh = (C.c_double * 3)(*[float(b) for b in B])
    iy1 = int(ny if iy1 is None else iy1)

    def direct(a, b):
        _lib.check(lib.geobo_a_sens_slab(FUNC_IDS[func], Bh, _p(loc), loc.shape[0], int(nx), int(ny), int(nz), _p(_chk(xe, "xe")),
                                         _p(_chk(ye, "ye")), _p(_chk(ze, "ze")), float(scale_mul), float(scale_div), int(a),
                                         int(b), base, ld, col_origin, _stream()), "geobo_a_sens_slab")
    if plan is None:
        direct(iy0, iy1)
        return out
    rows = slice(0, loc.shape[0]) if rows is None else rows
    jx, jy = plan["jx"][rows].contiguous(), plan["jy"][rows].contiguous()
    assert jx.numel() == loc.shape[0]
    nbytes = lib.geobo_a_sens_lattice_ws_bytes(int(nx), int(ny), int(nz))
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(nbytes // 8, dtype=F64, device=out.device)
    _lib.check(lib.geobo_a_sens_lattice(FUNC_IDS[func], Bh, loc.shape[0], int(nx), int(ny), int(nz), _p(plan["dxv"]), _p(plan["dyv"]),
                                        _p(plan["dzv"]), C.c_void_p(jx.data_ptr()), C.c_void_p(jy.data_ptr()), float(scale_mul),
                                        float(scale_div), int(iy0), iy1, base, ld, col_origin, _p(ws), nbytes, _stream()),
               "geobo_a_sens_lattice")
    if iy0 == 0:
        direct(0, 1)
    if iy1 == ny:
        direct(ny - 1, ny)
    return out


def potential(func, B, x, y, z):
    lib = require_gpu()
    x, y, z = (_chk(t, "xyz").contiguous() for t in (x, y, z))
    out = torch.empty_like(x)
    Bh = (C.c_double * 3)(*[float(b) for b in B])
    _lib.check(lib.geobo_potential(FUNC_IDS[func], Bh, _p(x), _p(y), _p(z), x.numel(), _p(out), _stream()), "geobo_potential")
    return out


def ak_fused(kid, A, xyz, col0, ncols, l1, l2, w, amp, out):
    """out[:, :ncols] = A @ K[:, col0:col0+ncols] with K generated on the fly (never stored)."""
    lib = require_gpu()
    lda = _rowmajor(A, "A")
    ldo = _rowmajor(out, "AK")
    x, y, z = (_chk(t, "xyz") for t in xyz)
    Ms_pad, N_pad = A.shape
    assert x.numel() >= N_pad and out.shape[0] >= Ms_pad and out.shape[1] >= ncols
    _lib.check(lib.geobo_ak_fused(kid, _p(A), Ms_pad, N_pad, lda, _p(x), _p(y), _p(z), int(col0), int(ncols), float(l1),
                                  float(l2), float(w), float(amp), _p(out), ldo, _stream()), "geobo_ak_fused")
    return out


def ak_points(kid, A, grid_xyz, q_xyz, l1, l2, w, amp, out):
    """out[:, :nq] = A @ K(grid, Q): geobo_ak_fused's product against the nq column points q_xyz (three 1-D tensors, nq % 128 == 0)
    instead of a slice of the contraction points grid_xyz."""
    lib = require_gpu()
    lda = _rowmajor(A, "A")
    ldo = _rowmajor(out, "out")
    x, y, z = (_chk(t, "grid_xyz") for t in grid_xyz)
    qx, qy, qz = (_chk(t, "q_xyz") for t in q_xyz)
    R_pad, N_pad = A.shape
    nq = qx.numel()
    assert min(x.numel(), y.numel(), z.numel()) >= N_pad and qy.numel() == nq and qz.numel() == nq
    assert all(t.is_contiguous() for t in (x, y, z, qx, qy, qz)) and out.shape[0] >= R_pad and out.shape[1] >= nq
    _lib.check(lib.geobo_ak_points(kid, _p(A), R_pad, N_pad, lda, _p(x), _p(y), _p(z), _p(qx), _p(qy), _p(qz), nq, float(l1),
                                   float(l2), float(w), float(amp), _p(out), ldo, _stream()), "geobo_ak_points")
    return out


def cov_table(kid, nx, ny, nz, sx, sy, sz, l1, l2, w, amp, device="cuda"):
    """Covariance on the grid's difference lattice, z mirrored: (ny*nx*2nz,) tensor, index (diy*nx + dix)*2nz + (dz + nz-1)."""
    lib = require_gpu()
    tab = torch.empty(2 * int(nx) * int(ny) * int(nz), dtype=F64, device=device)
    _lib.check(lib.geobo_cov_table(kid, int(nx), int(ny), int(nz), float(sx), float(sy), float(sz), float(l1), float(l2),
                                   float(w), float(amp), _p(tab), _stream()), "geobo_cov_table")
    return tab


def ak_fused_grid(A, nx, ny, nz, table, col0, ncols, out):
    """out[:, :ncols] = A @ K[:, col0:col0+ncols], K gathered from the lattice table (regular grids, nz >= 16)."""
    lib = require_gpu()
    lda = _rowmajor(A, "A")
    ldo = _rowmajor(out, "AK")
    Ms_pad, N_pad = A.shape
    assert out.shape[0] >= Ms_pad and out.shape[1] >= ncols and _chk(table, "table").numel() >= 2 * nx * ny * nz
    _lib.check(lib.geobo_ak_fused_grid(_p(A), Ms_pad, N_pad, lda, int(nx), int(ny), int(nz), _p(table), int(col0), int(ncols),
                                       _p(out), ldo, _stream()), "geobo_ak_fused_grid")
    return out


def gemm_nt(X, Y, C_, alpha=1.0, beta=0.0, lower_only=False, m_valid=0, small_tiles=False):
    """C = alpha X Y^T + beta C.  m_valid > 0: rows >= m_valid of X are zero padding (not contracted, not stored).
    small_tiles: 128-row workgroup tiles even when 256-row tiles would fit."""
    lib = require_gpu()
    ldx, ldy, ldc = _rowmajor(X, "X"), _rowmajor(Y, "Y"), _rowmajor(C_, "C")
    m, k = X.shape
    n = Y.shape[0]
    assert Y.shape[1] == k and C_.shape[0] >= m and C_.shape[1] >= n
    _lib.check(lib.geobo_gemm_nt(m, n, k, float(alpha), _p(X), ldx, _p(Y), ldy, float(beta), _p(C_), ldc,
                                 (1 if lower_only else 0) | (2 if small_tiles else 0), int(m_valid), _stream()), "geobo_gemm_nt")
    return C_


def gemm_nt_splitk(X, Y, C_, splits, ws, lower_only=False, m_valid=0):
    """C = X Y^T with the contraction split into `splits` concurrent slices (ws: >= splits*m*n doubles)."""
    lib = require_gpu()
    ldx, ldy, ldc = _rowmajor(X, "X"), _rowmajor(Y, "Y"), _rowmajor(C_, "C")
    m, k = X.shape
    n = Y.shape[0]
    assert Y.shape[1] == k and C_.shape[0] >= m and C_.shape[1] >= n and ws.numel() >= splits * m * n
    _lib.check(lib.geobo_gemm_nt_splitk(m, n, k, int(splits), _p(X), ldx, _p(Y), ldy, _p(C_), ldc, 1 if lower_only else 0,
                                        int(m_valid), _p(ws), ws.numel() * 8, _stream()), "geobo_gemm_nt_splitk")
    return C_


def gemm_nn(X, Y, C_, alpha=1.0, beta=0.0, x_lower=False, y_lower=False):
    """C = alpha X Y + beta C."""
    lib = require_gpu()
    ldx, ldy, ldc = _rowmajor(X, "X"), _rowmajor(Y, "Y"), _rowmajor(C_, "C")
    m, k = X.shape
    n = Y.shape[1]
    assert Y.shape[0] == k and C_.shape[0] >= m and C_.shape[1] >= n
    _lib.check(lib.geobo_gemm_nn(m, n, k, float(alpha), _p(X), ldx, _p(Y), ldy, float(beta), _p(C_), ldc,
                                 1 if x_lower else 0, 1 if y_lower else 0, _stream()), "geobo_gemm_nn")
    return C_


# entry -> (ymode of the core, reduce epilogue); see geobo_gemm_map in include/geobo_hip.h
_GEMM_ENTRIES = {"ak_fused": (0, 0), "ak_points": (0, 0), "ak_fused_grid": (3, 0), "gemm_nt": (1, 0), "gemm_nt_splitk": (1, 0),
                 "gemm_nn": (2, 0), "gemm_batched_nt": (1, 0), "gemm_batched_nn": (2, 0), "gemm_batched_xkm": (4, 0),
                 "posterior_reduce": (2, 1)}


def gemm_map(m, n, small_tiles=False, lower_only=False, x_lower=False, y_lower=False, batch=1, entry="gemm_nt", m_valid=0):
    """The workgroup -> tile map the GEMM core takes for a call of `entry` (a key of _GEMM_ENTRIES) with these public arguments:
    dict(map, ntiles, nblocks, grid_y, nbi, nbj, tm).  Host arithmetic only (geobo_gemm_map), no GPU needed.  batch: the batch of
    gemm_batched_* or the splits of gemm_nt_splitk.  posterior_reduce: m, n = shape of AK, x_lower is implied, m_valid as there."""
    lib = _lib.load()
    ymode, reduce = _GEMM_ENTRIES[entry]
    m, n = int(m), int(n)
    if n % 128 or m % 128:
        raise ValueError("gemm_map: m and n must be multiples of 128")
    tri = (1 if lower_only else 0) | (2 if x_lower else 0) | (4 if y_lower else 0)
    if entry == "posterior_reduce":
        # 256-row tiles aligned to the END of the valid rows (row_shift of geobo_posterior_reduce)
        groups = ((m_valid if 0 < m_valid < m else m) + 63) // 64
        tm, nbi, tri = 256, (groups + 3) // 4, 2
    elif entry == "gemm_batched_xkm":
        tm, nbi = 128, m // 128
    elif m % 256 == 0 and not small_tiles:
        tm, nbi = 256, m // 256
    else:
        tm, nbi = 128, m // 128
    nbj = n // 128
    out = (C.c_int * 4)()
    _lib.check(lib.geobo_gemm_map(ymode, reduce, nbi, nbj, tm, 128, tri, int(batch), out), "geobo_gemm_map")
    return dict(map=out[0], ntiles=out[1], nblocks=out[2], grid_y=out[3], nbi=nbi, nbj=nbj, tm=tm)


def _check_extents(fn, ops, batch):
    """Operand tiles may overhang the valid rows -- by contract into slack of the same allocation: checked before the launch."""
    for T, lead, stride, rows, cols, what in ops:
        last = (batch - 1) * int(stride) + (int(rows) - 1) * int(lead) + int(cols)
        room = T.untyped_storage().nbytes() // T.element_size() - T.storage_offset()
        if last > room:
            raise ValueError("%s: operand %s (%d x %d, ld %d, batch %d x stride %d) reads %d elements past its allocation"
                             % (fn, what, rows, cols, lead, batch, stride, last - room))


def axis_pass(fold, y_is_kn, inverse, *args):
    """One batched axis pass of the spectral route against the basis G (analysis) or G^T (synthesis): the radix-2 kernel when `fold`
    (the matrix operand has the pair structure and the strides allow it), else the plain batched GEMM on the same operands."""
    even = (4, 5, 7, 8) + ((10, 11) if not (y_is_kn or inverse) else ())     # operand strides; pair stores of the contiguous analysis
    if fold and all(int(args[i]) % 2 == 0 for i in even):
        return gemm_fold(y_is_kn, inverse, *args)
    return gemm_batched(y_is_kn, *args)


def gemm_fold_lamdot(px, nz, k, G, ldg, Y, ldy, strideY, lam, planes, out, batch):
    """Gram x step in one launch (geobo_gemm_fold_lamdot): out[b][o] = sum_z (G Y_b)[o][z] * lam[b % planes][o][z]."""
    lib = require_gpu()
    _check_extents("geobo_gemm_fold_lamdot", ((G, ldg, 0, pad_n(px), k, "G"), (Y, ldy, strideY, k, pad_n(nz), "Y")), batch)
    done = 0
    while done < batch:
        nb = min(batch - done, 65535)
        _lib.check(lib.geobo_gemm_fold_lamdot(int(px), int(nz), int(k), _p(G), int(ldg), C.c_void_p(Y.data_ptr() + done * strideY * 8),
                                              int(ldy), int(strideY), _p(_chk(lam, "lam")), int(planes), int(done),
                                              C.c_void_p(out.data_ptr() + done * px * 8), int(nb), _stream()), "geobo_gemm_fold_lamdot")
        done += nb
    return out


def gemm_fold(y_is_kn, inverse, m, n, k, X, ldx, strideX, Y, ldy, strideY, C_, ldc, strideC, m_valid, n_valid, batch):
    """Radix-2 form of a gemm_batched axis pass against the pair-interleaved basis G / G^T (geobo_gemm_fold): same arguments as the
    gemm_batched call it replaces (alpha = 1, beta = 0), half the multiply-adds."""
    lib = require_gpu()
    _check_extents("geobo_gemm_fold", ((X, ldx, strideX, m, k, "X"), (Y, ldy, strideY, k if y_is_kn else n, n if y_is_kn else k, "Y")), batch)
    done = 0
    while done < batch:
        nb = min(batch - done, 65535)
        _lib.check(lib.geobo_gemm_fold(1 if y_is_kn else 0, int(inverse), int(m), int(n), int(k),
                                       C.c_void_p(X.data_ptr() + done * strideX * 8), int(ldx), int(strideX),
                                       C.c_void_p(Y.data_ptr() + done * strideY * 8), int(ldy), int(strideY),
                                       C.c_void_p(C_.data_ptr() + done * strideC * 8), int(ldc), int(strideC), int(m_valid), int(n_valid),
                                       int(nb), _stream()), "geobo_gemm_fold")
        done += nb
    return C_


X_KM = 2          # GEOBO_GEMM_X_KM


def gemm_batched(y_is_kn, m, n, k, X, ldx, strideX, Y, ldy, strideY, C_, ldc, strideC, m_valid, n_valid, batch, alpha=1.0,
                 beta=0.0, x_km=False):
    """Raw batched GEMM (see include/geobo_hip.h); X/Y/C are tensors whose data_ptr is the batch-0 origin.
    m, n are COMPUTE extents (multiples of 128: the MFMA tiles run without edge predication on their loads; only the stores look at
    m_valid / n_valid), so operand tiles may overhang the valid rows -- by contract into slack of the same allocation.  That contract
    is checked here (round 5: a per-slot operand of the boundary-slab convolution overhung its tensor by 64 KB at nz = 16, which only
    aborted once an unmapped page happened to follow it).  x_km: X is given transposed (k x m, m-contiguous; y_is_kn False only)."""
    lib = require_gpu()
    done = 0
    esz = 8
    _check_extents("geobo_gemm_batched", ((X, ldx, strideX, k if x_km else m, m if x_km else k, "X"),
                                          (Y, ldy, strideY, k if y_is_kn else n, n if y_is_kn else k, "Y")), batch)
    while done < batch:                      # gridDim.y limit
        nb = min(batch - done, 65535)
        _lib.check(lib.geobo_gemm_batched((1 if y_is_kn else 0) | (X_KM if x_km else 0), int(m), int(n), int(k), float(alpha),
                                          C.c_void_p(X.data_ptr() + done * strideX * esz), int(ldx), int(strideX),
                                          C.c_void_p(Y.data_ptr() + done * strideY * esz), int(ldy), int(strideY), float(beta),
                                          C.c_void_p(C_.data_ptr() + done * strideC * esz), int(ldc), int(strideC),
                                          int(m_valid), int(n_valid), int(nb), _stream()), "geobo_gemm_batched")
        done += nb
    return C_


def scale_broadcast(a, b, out):
    lib = require_gpu()
    _lib.check(lib.geobo_scale_broadcast(_p(_chk(a, "a")), _p(_chk(b, "b")), a.numel(), b.numel(), _p(out), _stream()),
               "geobo_scale_broadcast")
    return out


def scale_broadcast2(a, b0, b1, out0, out1):
    lib = require_gpu()
    _lib.check(lib.geobo_scale_broadcast2(_p(_chk(a, "a")), _p(_chk(b0, "b0")), _p(_chk(b1, "b1")), a.numel(), b0.numel(),
                                          _p(out0), _p(out1), _stream()), "geobo_scale_broadcast2")


# XZ2D_SHAPES (plan.py): (nx, nz) the fused (x, z) transform kernel is instantiated for


def xz2d(inverse, nx, nz, rows, ppr, src, in_row, in_plane, Mx, Mz, out, out_row, out_plane):
    """Fused two-axis transform of rows*ppr planes (geobo_xz2d): X -> Mx X Mz^T."""
    lib = require_gpu()
    _lib.check(lib.geobo_xz2d(1 if inverse else 0, int(nx), int(nz), int(rows), int(ppr), _p(_chk(src, "src")), int(in_row),
                              int(in_plane), _p(_chk(Mx, "Mx")), int(Mx.stride(0)), _p(_chk(Mz, "Mz")), int(Mz.stride(0)),
                              _p(_chk(out, "out")), int(out_row), int(out_plane), _stream()), "geobo_xz2d")


# XZ2D_FOLD_N (plan.py): extents the radix-2 kernels are instantiated for (both axes equal)


def xz2d_fold(inverse, n, rows, ppr, src, in_row, in_plane, Fx, Fz, out, out_row, out_plane):
    """Radix-2 form of xz2d on the pair-interleaved basis (geobo_xz2d_fold); Fx / Fz: (n, n/2, 2) folded matrices."""
    lib = require_gpu()
    _lib.check(lib.geobo_xz2d_fold(1 if inverse else 0, int(n), int(rows), int(ppr), _p(_chk(src, "src")), int(in_row), int(in_plane),
                                   _p(_chk(Fx, "Fx")), _p(_chk(Fz, "Fz")), _p(_chk(out, "out")), int(out_row), int(out_plane), _stream()),
               "geobo_xz2d_fold")


def xz2d_fold_quad(inverse, n, rows, groups, src, in_row, in_plane, Fx, Fz, out, out_row, out_plane):
    """geobo_xz2d_fold for n = 32 planes, four consecutive planes of a row per kernel plane (geobo_xz2d_fold_quad); Fx / Fz: folded
    matrices of diag(G_32, G_32), shape (64, 32, 2)."""
    lib = require_gpu()
    _lib.check(lib.geobo_xz2d_fold_quad(1 if inverse else 0, int(n), int(rows), int(groups), _p(_chk(src, "src")), int(in_row), int(in_plane),
                                        _p(_chk(Fx, "Fx")), _p(_chk(Fz, "Fz")), _p(_chk(out, "out")), int(out_row), int(out_plane), _stream()),
               "geobo_xz2d_fold_quad")


def xz2d_fold_inv_ss_slots(n, rows, ppr):
    return _lib.load().geobo_xz2d_fold_inv_ss_slots(int(n), int(rows), int(ppr))


def xz2d_fold_inv_ss(n, rows, ppr, src, in_row, in_plane, Fx, Fz, ss, src2=None, in2_row=0, r2_first=0):
    """Inverse radix-2 transform fused with the sum of squares over the rows (geobo_xz2d_fold_inv_ss): ss[slot][y][n*n] +=
    sum_r (inverse(src[r][y] (+ src2[r - r2_first][y] for r >= r2_first)))^2."""
    lib = require_gpu()
    assert _chk(ss, "ss").numel() >= xz2d_fold_inv_ss_slots(n, rows, ppr) * ppr * n * n
    _lib.check(lib.geobo_xz2d_fold_inv_ss(int(n), int(rows), int(ppr), _p(_chk(src, "src")), int(in_row), int(in_plane),
                                          _p(_chk(src2, "src2")) if src2 is not None else None, int(in2_row), int(r2_first),
                                          _p(_chk(Fx, "Fx")), _p(_chk(Fz, "Fz")), _p(ss), _stream()), "geobo_xz2d_fold_inv_ss")


def tile_rows(m, m_valid, tile=256, group=64):
    """Rows of each `tile`-row tile that take part in the contraction when rows >= m_valid are padding: whole `group`-row
    wavefront groups (flop accounting of the m_valid argument of geobo_gemm_nt / geobo_posterior_reduce)."""
    m_valid = m if not m_valid or m_valid > m else m_valid
    out = []
    for r0 in range(0, m, tile):
        v = min(max(m_valid - r0, 0), tile)
        out.append((v + group - 1) // group * group)
    return out


def xz2d_fold_lattice(n, rows, ppr, Q, row_off, q_plane, edge, edge_row, Fx, Fz, out, out_row, out_plane):
    """Forward radix-2 transform of operator rows read as windows of the lattice stencil table (geobo_xz2d_fold_lattice)."""
    lib = require_gpu()
    assert row_off.dtype == torch.int64 and row_off.is_contiguous() and row_off.numel() >= rows
    _lib.check(lib.geobo_xz2d_fold_lattice(int(n), int(rows), int(ppr), _p(_chk(Q, "Q")), row_off.data_ptr(), int(q_plane),
                                           _p(_chk(edge, "edge")), int(edge_row), _p(_chk(Fx, "Fx")), _p(_chk(Fz, "Fz")),
                                           _p(_chk(out, "out")), int(out_row), int(out_plane), _stream()), "geobo_xz2d_fold_lattice")


# YMUL_SHAPES (plan.py): (m, k) geobo_ymul is instantiated for


def ymul(m, k, C, rows, G, src, in_row, out, out_row, fold=False):
    """out[r] (m x C) = G (m x k) . src[r] (k x C) for every row (geobo_ymul); fold: G is pair-interleaved (row 2b+1 = (-1)^j row 2b) and
    the product runs in radix 2 (geobo_ymul_fold)."""
    lib = require_gpu()
    fn, name = (lib.geobo_ymul_fold, "geobo_ymul_fold") if fold else (lib.geobo_ymul, "geobo_ymul")
    _lib.check(fn(int(m), int(k), int(C), int(rows), _p(_chk(G, "G")), int(G.stride(0)), _p(_chk(src, "src")), int(in_row),
                  _p(_chk(out, "out")), int(out_row), _stream()), name)


def xz2d_fold_inv_gx(n, rows, ppr, src, in_row, in_plane, Fx, Fz, out, out_row, out_plane, store_all, gx, gx_row, gx_plane):
    """Inverse radix-4 transform that also emits the lattice Gram's x analysis GX[r][y][o][z] of every interior plane
    (geobo_xz2d_fold_inv_gx); store_all False: only the two boundary planes of a row are stored to out."""
    lib = require_gpu()
    _lib.check(lib.geobo_xz2d_fold_inv_gx(int(n), int(rows), int(ppr), _p(_chk(src, "src")), int(in_row), int(in_plane), _p(_chk(Fx, "Fx")),
                                          _p(_chk(Fz, "Fz")), _p(_chk(out, "out")), int(out_row), int(out_plane), 1 if store_all else 0,
                                          _p(_chk(gx, "gx")), int(gx_row), int(gx_plane), _stream()), "geobo_xz2d_fold_inv_gx")


def gram_yz(n, ny, rows, gx, gx_row, gx_plane, G, lam_oz, s, s_row, s_plane):
    """s[r][ky][o] = sum_z lam_oz[ky][o][z] (G gx[r])[ky][o][z]: y step, eigenvalue scaling and channel sum of the lattice Gram on
    x-analysed rows (geobo_gram_yz); G: (2 ny) x ny pair-interleaved."""
    lib = require_gpu()
    _lib.check(lib.geobo_gram_yz(int(n), int(ny), int(rows), _p(_chk(gx, "gx")), int(gx_row), int(gx_plane), _p(_chk(G, "G")), int(G.stride(0)),
                                 _p(_chk(lam_oz, "lam_oz")), _p(_chk(s, "s")), int(s_row), int(s_plane), _stream()), "geobo_gram_yz")


def xcorr_reduce(nx, nz, rows, planes, src, in_row, in_plane, Mx, lam, out, out_row, out_plane):
    """x step + eigenvalue scaling + channel sum of the lattice Gram (geobo_xcorr_reduce)."""
    lib = require_gpu()
    _lib.check(lib.geobo_xcorr_reduce(int(nx), int(nz), int(rows), int(planes), _p(_chk(src, "src")), int(in_row), int(in_plane),
                                      _p(_chk(Mx, "Mx")), int(Mx.stride(0)), _p(_chk(lam, "lam")), _p(_chk(out, "out")),
                                      int(out_row), int(out_plane), _stream()), "geobo_xcorr_reduce")


def xcorr_reduce_fold(n, rows, planes, src, in_row, in_plane, F, lam, out, out_row, out_plane):
    """Radix-2 form of xcorr_reduce on the pair-interleaved basis (geobo_xcorr_reduce_fold); F: (n, n/2, 2) folded x matrices."""
    lib = require_gpu()
    _lib.check(lib.geobo_xcorr_reduce_fold(int(n), int(rows), int(planes), _p(_chk(src, "src")), int(in_row), int(in_plane),
                                           _p(_chk(F, "F")), _p(_chk(lam, "lam")), _p(_chk(out, "out")), int(out_row), int(out_plane),
                                           _stream()), "geobo_xcorr_reduce_fold")


def a_sens_lattice_stencil(ws, nx, ny, nz):
    """View of the stencil table Q[(2ny-3)][(2nx-1)][nz] that geobo_a_sens_lattice left in its workspace."""
    np_ = (2 * ny - 2) * (2 * nx) * (nz + 1)
    return ws[np_:np_ + (2 * ny - 3) * (2 * nx - 1) * nz].view(2 * ny - 3, 2 * nx - 1, nz)


# TOEPLITZ_NY (plan.py): y extents geobo_toeplitz_y / _y3 are instantiated for


# TOEPLITZ_ADD_NY (plan.py): y extents of the accumulating form (geobo_toeplitz_y3_add)


def toeplitz_y(ny, C, R, src, tabs, outs, y0=0, y1=None, plane=None, accumulate=False):
    """outs[j][r, y - y0, c] = sum_y' tabs[j][|y - y'|, c] * src[r, y', c]  (geobo_toeplitz_y3); 1 to 3 property blocks per sweep.
    plane: stride in doubles between the y-planes of src and outs (default C: dense).  accumulate: outs[j] += (geobo_toeplitz_y3_add,
    ny in TOEPLITZ_ADD_NY)."""
    lib = require_gpu()
    y1 = ny if y1 is None else y1
    n = len(tabs)
    assert 1 <= n <= 3 and len(outs) == n
    tp, op = _ptrs(tabs, "tab"), _ptrs(outs, "out")
    fn, name = (lib.geobo_toeplitz_y3_add, "geobo_toeplitz_y3_add") if accumulate else (lib.geobo_toeplitz_y3, "geobo_toeplitz_y3")
    _lib.check(fn(int(ny), int(C), int(C if plane is None else plane), int(R), n, _p(_chk(src, "src")), tp, op, int(y0), int(y1), _stream()), name)


# TOEPLITZ_Y2T_NY (plan.py): y extents of the two-term kernel


def toeplitz_y2t(ny, C, R, src_g, src_m, tabs_g, tabs_m, outs, plane=None):
    """outs[j][r, y, c] = sum_y' tabs_g[j][|y - y'|, c] src_g[r, y', c] + tabs_m[j][|y - y'|, c] src_m[r, y', c],  j = 0, 1
    (geobo_toeplitz_y2t: the two-term rows of the transposed posterior in one pass)."""
    lib = require_gpu()
    assert len(tabs_g) == 2 and len(tabs_m) == 2 and len(outs) == 2
    _lib.check(lib.geobo_toeplitz_y2t(int(ny), int(C), int(C if plane is None else plane), int(R), _p(_chk(src_g, "src_g")), _p(_chk(src_m, "src_m")),
                                      _p(_chk(tabs_g[0], "tab")), _p(_chk(tabs_g[1], "tab")), _p(_chk(tabs_m[0], "tab")), _p(_chk(tabs_m[1], "tab")),
                                      _p(_chk(outs[0], "out")), _p(_chk(outs[1], "out")), _stream()), "geobo_toeplitz_y2t")


def toeplitz_y2s(ny, C, R, src_g, src_m, tab_d0, tab_x, tab_d1, outs, plane=None):
    """Two-term rows with a shared cross block (K_10 = K_01) as three products per mode instead of four:
    outs[0] = T(tab_d0) src_g + T(tab_x)(src_g + src_m),  outs[1] = T(tab_d1) src_m + T(tab_x)(src_g + src_m)   (geobo_toeplitz_y2s)."""
    lib = require_gpu()
    assert len(outs) == 2
    _lib.check(lib.geobo_toeplitz_y2s(int(ny), int(C), int(C if plane is None else plane), int(R), _p(_chk(src_g, "src_g")), _p(_chk(src_m, "src_m")),
                                      _p(_chk(tab_d0, "tab")), _p(_chk(tab_x, "tab")), _p(_chk(tab_d1, "tab")),
                                      _p(_chk(outs[0], "out")), _p(_chk(outs[1], "out")), _stream()), "geobo_toeplitz_y2s")


# SPECTRAL_Y_NY (plan.py): y extents of the in-kernel spectral y stage (geobo_spectral_y / _y2s)
_spectral_y_basis = {}              # (ny, device index) -> fragment blob (constant of ny: filled once per device)


def spectral_y_basis(ny, device=None):
    """Transform fragments of geobo_spectral_y for one y extent (a constant of ny: built once per device, kept for the process)."""
    lib = require_gpu()
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    b = _spectral_y_basis.get((ny, dev))
    if b is None:
        n = int(lib.geobo_spectral_y_basis_doubles(int(ny)))
        if n <= 0:
            raise RuntimeError("geobo_spectral_y: ny = %d is not instantiated" % ny)
        b = torch.empty(n, dtype=F64, device="cuda:%d" % dev)
        _lib.check(lib.geobo_spectral_y_basis(int(ny), _p(b), _stream()), "geobo_spectral_y_basis")
        _spectral_y_basis[(ny, dev)] = b
    return b


def spectral_y(ny, C, R, src, tabs, outs, y0=0, y1=None, plane=None, accumulate=False):
    """The sums of toeplitz_y (one to three property blocks; accumulate: outs[j] += ..., ny > 64) through the y axis's own spectrum on the
    matrix pipe (geobo_spectral_y3: ny <= 64 one wave per 16 modes, two blocks per sweep; ny > 64 four waves per 16 modes)."""
    lib = require_gpu()
    y1 = ny if y1 is None else y1
    n = len(tabs)
    assert 1 <= n <= 3 and len(outs) == n
    tp, op = _ptrs(tabs, "tab"), _ptrs(outs, "out")
    _lib.check(lib.geobo_spectral_y3(int(ny), int(C), int(C if plane is None else plane), int(R), n, _p(_chk(src, "src")), tp, op, int(y0), int(y1),
                                     1 if accumulate else 0, _p(spectral_y_basis(ny, src.device)), _stream()), "geobo_spectral_y3")


def spectral_y_lattice(ny, C, R, pool, row_off, edge, edge_row, order, tabs, outs, y0=0, y1=None, plane=None):
    """spectral_y on rows read as windows of a pool of (x, z)-spectrum planes (geobo_spectral_y_lattice; ny <= 64): row r = the planes at
    pool + row_off[r] + y * plane between its two boundary planes edge[r * edge_row:] (+ plane), swept in the order `order` (int32
    permutation or None).  One to three property blocks, two per sweep like spectral_y.  Bit-identical to spectral_y on the gather."""
    lib = require_gpu()
    y1 = ny if y1 is None else y1
    n = len(tabs)
    assert 1 <= n <= 3 and len(outs) == n
    assert row_off.is_cuda and row_off.dtype == torch.int64 and row_off.is_contiguous() and row_off.numel() >= R
    assert order is None or (order.is_cuda and order.dtype == torch.int32 and order.is_contiguous() and order.numel() == R)
    basis = spectral_y_basis(ny, pool.device)
    for j in range(0, n, 2):
        two = j + 1 < n
        _lib.check(lib.geobo_spectral_y_lattice(int(ny), int(C), int(C if plane is None else plane), int(R), 2 if two else 1, _p(_chk(pool, "pool")),
                                                row_off.data_ptr(), _p(_chk(edge, "edge")), int(edge_row), order.data_ptr() if order is not None else None,
                                                _p(_chk(tabs[j], "tab")), _p(_chk(tabs[j + 1], "tab")) if two else None,
                                                _p(_chk(outs[j], "out")), _p(_chk(outs[j + 1], "out")) if two else None,
                                                int(y0), int(y1), _p(basis), _stream()), "geobo_spectral_y_lattice")


# SPECTRAL_Y3T_NY (plan.py): y extents of the two-term long-axis form (geobo_spectral_y3t)


def spectral_y3t(ny, C, R, src_g, src_m, tabs_g, tabs_m, outs, plane=None):
    """outs[j] = T(tabs_g[j]) src_g + T(tabs_m[j]) src_m for up to three property blocks, the terms meeting in the y spectrum
    (geobo_spectral_y3t, ny in SPECTRAL_Y3T_NY)."""
    lib = require_gpu()
    n = len(outs)
    assert 1 <= n <= 3 and len(tabs_g) == n and len(tabs_m) == n
    _lib.check(lib.geobo_spectral_y3t(int(ny), int(C), int(C if plane is None else plane), int(R), n, _p(_chk(src_g, "src_g")), _p(_chk(src_m, "src_m")),
                                      _ptrs(tabs_g, "tab"), _ptrs(tabs_m, "tab"), _ptrs(outs, "out"), _p(spectral_y_basis(ny, src_g.device)), _stream()),
               "geobo_spectral_y3t")


# SPECTRAL_AXIS_N (plan.py): extents of the radix-4 axis passes (geobo_spectral_axis); half-integer basis only


def spectral_axis(inverse, n, C, plane_in, plane_out, item_in, item_out, items, src, dst, mask_ends=False):
    """One axis pass along a strided axis against the half-integer basis G of size n (geobo_spectral_axis): analysis n -> 2n planes or
    synthesis 2n -> n planes of C contiguous modes per item.  mask_ends (analysis): input planes 0 and n - 1 count as zero."""
    lib = require_gpu()
    _lib.check(lib.geobo_spectral_axis(1 if inverse else 0, int(n), int(C), int(plane_in), int(plane_out), int(item_in), int(item_out), int(items),
                                       _p(_chk(src, "src")), _p(_chk(dst, "dst")), _p(spectral_y_basis(n, src.device)), 1 if mask_ends else 0, _stream()),
               "geobo_spectral_axis")
    return dst


def spectral_y2s(ny, C, R, src_g, src_m, tab_d0, tab_x, tab_d1, outs, plane=None):
    """The sums of toeplitz_y2s (two-term rows, shared cross block) with the terms meeting in the y spectrum (geobo_spectral_y2s)."""
    lib = require_gpu()
    assert len(outs) == 2
    _lib.check(lib.geobo_spectral_y2s(int(ny), int(C), int(C if plane is None else plane), int(R), _p(_chk(src_g, "src_g")), _p(_chk(src_m, "src_m")),
                                      _p(_chk(tab_d0, "tab")), _p(_chk(tab_x, "tab")), _p(_chk(tab_d1, "tab")),
                                      _p(_chk(outs[0], "out")), _p(_chk(outs[1], "out")), _p(spectral_y_basis(ny, src_g.device)), _stream()),
               "geobo_spectral_y2s")


class PotrfContext:
    """Fork streams / events of geobo_potrf_inv on the device that is current at construction (owned by the caller: one per
    engine; never shared between concurrent factorisations)."""

    def __init__(self):
        lib = require_gpu()
        self._h = C.c_void_p()
        _lib.check(lib.geobo_potrf_ctx_create(C.byref(self._h)), "geobo_potrf_ctx_create")

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().geobo_potrf_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


POTRF_SCHEDULES = {"auto": 0, "streams": 1, "dag": 2}      # GEOBO_POTRF_AUTO / _STREAMS / _DAG of include/geobo_hip.h


def potrf_inv(A, Linv=None, ws=None, ctx=None, schedule="auto"):
    """In-place lower Cholesky of A (m x m, m % 128 == 0); returns (Linv, info_tensor).  Linv / ws may be caller-owned;
    ctx: PotrfContext (concurrent L^-1 subtrees) or None (serial on the current stream).  schedule: "auto" (the tile DAG from
    m = 1024, the stream schedule below), "streams" or "dag" (that one at any m)."""
    if schedule not in POTRF_SCHEDULES:
        raise ValueError("potrf_inv: schedule must be one of %s, not %r" % (", ".join(map(repr, POTRF_SCHEDULES)), schedule))
    lib = require_gpu()
    ld = _rowmajor(A, "A")
    m = A.shape[0]
    if Linv is None:
        Linv = torch.empty((m, m), dtype=F64, device=A.device)
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    nbytes = lib.geobo_potrf_ws_bytes(m)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(max(nbytes // 8, 1), dtype=F64, device=A.device)
    _lib.check(lib.geobo_potrf_inv(m, _p(A), ld, _p(Linv), Linv.stride(0), _p(info), _p(ws), nbytes,
                                   ctx.handle if ctx is not None else None, POTRF_SCHEDULES[schedule], _stream()), "geobo_potrf_inv")
    return Linv, info


def trmv_stats(Linv, y, L):
    """u = Linv y; stats = [u.u, sum log(L_ii^2)]."""
    lib = require_gpu()
    m = Linv.shape[0]
    u = torch.empty(m, dtype=F64, device=Linv.device)
    stats = torch.empty(2, dtype=F64, device=Linv.device)
    _lib.check(lib.geobo_trmv_stats(m, _p(Linv), _rowmajor(Linv, "Linv"), _p(_chk(y, "y")), _p(L), _rowmajor(L, "L"),
                                    _p(u), _p(stats), _stream()), "geobo_trmv_stats")
    return u, stats


def a_sens_lattice_ws_doubles(nx, ny, nz):
    return max(_lib.load().geobo_a_sens_lattice_ws_bytes(int(nx), int(ny), int(nz)) // 8, 1)


def potrf_ws_doubles(m):
    return max(_lib.load().geobo_potrf_ws_bytes(int(m)) // 8, 1)


def colgemv_ws_doubles(m, n):
    return max(_lib.load().geobo_colgemv_ws_bytes(int(m), int(n)) // 8, 1)


def posterior_ws_doubles(m, ncols):
    return max(_lib.load().geobo_posterior_ws_bytes(int(m), int(ncols)) // 8, 1)


def posterior_reduce(Linv, AK, u, prior_var, ws=None, m_valid=0):
    """mu[c] = sum_m (Linv AK)[m,c] u[m],  var[c] = prior_var - sum_m (Linv AK)[m,c]^2 (V never stored)."""
    lib = require_gpu()
    m, ncols = AK.shape
    mu = torch.empty(ncols, dtype=F64, device=AK.device)
    var = torch.empty(ncols, dtype=F64, device=AK.device)
    nbytes = lib.geobo_posterior_ws_bytes(m, ncols)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(max(nbytes // 8, 1), dtype=F64, device=AK.device)
    _lib.check(lib.geobo_posterior_reduce(m, ncols, _p(Linv), _rowmajor(Linv, "Linv"), _p(AK), _rowmajor(AK, "AK"),
                                          _p(_chk(u, "u")), float(prior_var), _p(mu), _p(var), int(m_valid), _p(ws), nbytes,
                                          _stream()),
               "geobo_posterior_reduce")
    return mu, var


def kinv_dot_ws_doubles(m, T):
    return max(_lib.load().geobo_kinv_dot_ws_bytes(int(m), int(T)) // 8, 1)


def kinv_dot(Linv, alpha, Gs, segs, ws=None, out=None):
    """out[t, a, b] = sum over rows i of segment a, columns j of segment b of (Linv^T Linv - alpha alpha^T)_ij Gs[t]_ij, Gs[t] given
    by its lower triangle (symmetric); segs: three (start, end) row ranges, starts multiples of 256.  K^-1 is never stored."""
    lib = require_gpu()
    m = Linv.shape[0]
    ldl = _rowmajor(Linv, "Linv")
    T = len(Gs)
    if not 1 <= T <= 4:
        raise ValueError("kinv_dot takes 1 to 4 matrices, got %d" % T)
    ldg = _rowmajor(Gs[0], "G")
    for g in Gs:
        if _rowmajor(g, "G") != ldg or tuple(g.shape) != (m, m):
            raise ValueError("every G must be (m x m) with the same leading dimension")
    alpha = _chk(alpha, "alpha")
    assert alpha.is_contiguous() and alpha.numel() >= m and Linv.shape[1] == m
    seg = (C.c_int64 * 6)(*[int(v) for ab in segs for v in ab])
    gp = (C.c_void_p * T)(*[g.data_ptr() for g in Gs])
    if out is None:
        out = torch.empty((T, 3, 3), dtype=F64, device=Linv.device)
    nbytes = lib.geobo_kinv_dot_ws_bytes(m, T)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(max(nbytes // 8, 1), dtype=F64, device=Linv.device)
    _lib.check(lib.geobo_kinv_dot(m, _p(Linv), ldl, _p(alpha), T, gp, ldg, seg, _p(_chk(out, "out")), _p(ws), nbytes, _stream()),
               "geobo_kinv_dot")
    return out


def set_gram(idx, V, R, G, accumulate=False, ncols=None):
    """G[c] = (accumulate ? G[c] : 0) + V[:R, idx[c]]^T V[:R, idx[c]] for the C sets of idx ((C, k) int32, k <= 128; entries outside
    [0, ncols) are padding).  V: 2-D fp64 rows of V_d (columns in voxel order); G: (C, k, k) fp64, written in full (fp64 MFMA)."""
    lib = require_gpu()
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 2 and idx.is_contiguous()):
        raise TypeError("idx must be a contiguous (C, k) CUDA int32 tensor")
    C_, k = idx.shape
    ldv = _rowmajor(V, "V")
    R = int(R)
    assert 0 <= R <= V.shape[0]
    ncols = V.shape[1] if ncols is None else int(ncols)
    assert ncols <= V.shape[1]
    _chk(G, "G")
    assert G.is_contiguous() and tuple(G.shape) == (C_, k, k)
    _lib.check(lib.geobo_set_gram(C_, k, _p(idx), R, _p(V), ldv, ncols, 1 if accumulate else 0, _p(G), _stream()), "geobo_set_gram")
    return G


def set_logdet(G, Kpp, sigma2, idx, n_obs, observed=None, out=None, status=None):
    """Per set c: D = Kpp_c - G[c], S = D / sigma2 + I (entries that are padding or `observed` become unit rows / columns), Cholesky:
    out (3, C) = [1/2 log det S, 1^T D 1, trace D] over the entries kept, status (C,) int32 = 0 or 1 + failing pivot (NaN outputs).
    Kpp: (k, k) shared by every set or (C, k, k) one per set; observed: (n_obs,) uint8 CUDA tensor or None."""
    lib = require_gpu()
    C_, k = idx.shape
    _chk(G, "G")
    _chk(Kpp, "Kpp")
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()):
        raise TypeError("idx must be a contiguous (C, k) CUDA int32 tensor")
    assert G.is_contiguous() and tuple(G.shape) == (C_, k, k) and Kpp.is_contiguous()
    if tuple(Kpp.shape) == (k, k):
        stride = 0
    elif tuple(Kpp.shape) == (C_, k, k):
        stride = k * k
    else:
        raise ValueError("Kpp must be (k, k) or (C, k, k)")
    obs = None
    if observed is not None:
        if not (isinstance(observed, torch.Tensor) and observed.is_cuda and observed.dtype == torch.uint8 and observed.is_contiguous()
                and observed.numel() >= int(n_obs)):
            raise TypeError("observed must be a contiguous CUDA uint8 tensor of n_obs entries")
        obs = _p(observed)
    if out is None:
        out = torch.empty((3, C_), dtype=F64, device=G.device)
    if status is None:
        status = torch.empty(C_, dtype=torch.int32, device=G.device)
    _lib.check(lib.geobo_set_logdet(C_, k, _p(G), _p(Kpp), stride, float(sigma2), _p(idx), obs, int(n_obs), _p(_chk(out, "out")),
                                    _p(status), _stream()), "geobo_set_logdet")
    return out, status


def factor_append(D, G, r, Ls, T, uP, out=None, status=None):
    """S = D - G (k x k, k <= 128, lower triangles read), S = Ls Ls^T, T = Ls^-1, uP = T r (geobo_factor_append, one workgroup).
    D, G, Ls, T: 2-D fp64 views with unit column stride (k rows and columns used); r, uP: k doubles.  Returns (out (1,) = sum log
    diag Ls, status (1,) int32 = 0, or 1 + the failing pivot -- then nothing else was written)."""
    lib = require_gpu()
    k = _chk(r, "r").numel()
    lds = [_rowmajor(t, nm) for t, nm in ((D, "D"), (G, "G"), (Ls, "Ls"), (T, "T"))]
    assert all(t.shape[0] >= k and t.shape[1] >= k for t in (D, G, Ls, T)) and r.is_contiguous()
    assert _chk(uP, "uP").numel() >= k and uP.is_contiguous()
    if out is None:
        out = torch.empty(1, dtype=F64, device=D.device)
    if status is None:
        status = torch.empty(1, dtype=torch.int32, device=D.device)
    _lib.check(lib.geobo_factor_append(int(k), _p(D), lds[0], _p(G), lds[1], _p(r), _p(Ls), lds[2], _p(T), lds[3], _p(uP),
                                       _p(_chk(out, "out")), _p(status), _stream()), "geobo_factor_append")
    return out, status


def rows_downdate(V, n, c, mu, var, ncols=None):
    """mu[j] += sum_{r < n} c[r] V[r, j], var[j] -= sum_{r < n} V[r, j]^2 for j < ncols (geobo_rows_downdate): rows in ascending
    order from the stored values, so a split of the rows over several calls gives the same bits."""
    lib = require_gpu()
    ld = _rowmajor(V, "V")
    n = int(n)
    ncols = V.shape[1] if ncols is None else int(ncols)
    assert 0 <= n <= V.shape[0] and ncols <= V.shape[1] and _chk(c, "c").numel() >= n and c.is_contiguous()
    assert _chk(mu, "mu").numel() >= ncols and _chk(var, "var").numel() >= ncols and mu.is_contiguous() and var.is_contiguous()
    _lib.check(lib.geobo_rows_downdate(_p(V), ld, n, ncols, _p(c), _p(mu), _p(var), _stream()), "geobo_rows_downdate")
    return mu, var


def fold_factor(G, dinv, a, Cinv, g, stats=None, status=None):
    """S = G + diag(dinv) (k x k, k <= 128, the lower triangle of G read), S = C C^T, Cinv = C^-1, g = C^-1 a (geobo_fold_factor, one
    workgroup).  G, Cinv: 2-D fp64 views with unit column stride (k rows and columns used); dinv, a, g: k doubles.  Returns (stats
    (2,) = [2 sum log diag C, g^T g], status (1,) int32 = 0, or 1 + the failing pivot -- then nothing else was written)."""
    lib = require_gpu()
    k = _chk(a, "a").numel()
    ldg, ldc = _rowmajor(G, "G"), _rowmajor(Cinv, "Cinv")
    assert all(t.shape[0] >= k and t.shape[1] >= k for t in (G, Cinv)) and a.is_contiguous()
    assert _chk(dinv, "dinv").numel() == k and dinv.is_contiguous() and _chk(g, "g").numel() >= k and g.is_contiguous()
    if stats is None:
        stats = torch.empty(2, dtype=F64, device=G.device)
    if status is None:
        status = torch.empty(1, dtype=torch.int32, device=G.device)
    assert _chk(stats, "stats").numel() >= 2 and stats.is_contiguous()
    _lib.check(lib.geobo_fold_factor(int(k), _p(G), ldg, _p(dinv), _p(a), _p(Cinv), ldc, _p(g), _p(stats), _p(status), _stream()),
               "geobo_fold_factor")
    return stats, status


def rows_reweight_ws_doubles(ncols):
    return max(_lib.load().geobo_rows_reweight_ws_bytes(int(ncols)) // 8, 1)


def rows_reweight(B, k, Cinv, g, mu=None, var=None, ncols=None, part=None, ws=None):
    """Per column c < ncols of the first k rows of B: t = Cinv B[:k, c], mu[c] -= t . g, var[c] += t . t (geobo_rows_reweight); returns
    part (3,) = [sum_c dmu^2, max_c |dmu|, sum_c dvar].  mu = var = None: statistics only, no cube is written.  A tile cut at an even
    column gives the same mu and var bits; part is summed in a fixed order (no atomics)."""
    lib = require_gpu()
    ldb, ldc = _rowmajor(B, "B"), _rowmajor(Cinv, "Cinv")
    k = int(k)
    ncols = B.shape[1] if ncols is None else int(ncols)
    assert 1 <= k <= B.shape[0] and ncols <= B.shape[1] and Cinv.shape[0] >= k and Cinv.shape[1] >= k
    assert _chk(g, "g").numel() >= k and g.is_contiguous()
    if (mu is None) != (var is None):
        raise ValueError("mu and var go together")
    if mu is not None:
        assert _chk(mu, "mu").numel() >= ncols and _chk(var, "var").numel() >= ncols and mu.is_contiguous() and var.is_contiguous()
    if part is None:
        part = torch.empty(3, dtype=F64, device=B.device)
    assert _chk(part, "part").numel() >= 3 and part.is_contiguous()
    need = rows_reweight_ws_doubles(ncols)
    if ws is None:
        ws = torch.empty(need, dtype=F64, device=B.device)
    assert _chk(ws, "ws").numel() >= need and ws.is_contiguous()
    _lib.check(lib.geobo_rows_reweight(k, _p(B), ldb, ncols, _p(Cinv), ldc, _p(g), None if mu is None else _p(mu),
                                       None if var is None else _p(var), _p(part), _p(ws), 8 * ws.numel(), _stream()),
               "geobo_rows_reweight")
    return part


def kinv_diag_ws_doubles(m):
    return max(_lib.load().geobo_kinv_diag_ws_bytes(int(m)) // 8, 1)


def kinv_diag(Linv, u, ws=None, d=None, alpha=None):
    """d[c] = sum_r Linv[r, c]^2 (the diagonal of K^-1 = Linv^T Linv) and alpha = Linv^T u, from the lower triangle of Linv alone
    (m x m, m % 256 == 0, even leading dimension); the strict upper triangle is never read.  Returns (d, alpha)."""
    lib = require_gpu()
    m = Linv.shape[0]
    ldl = _rowmajor(Linv, "Linv")
    u = _chk(u, "u")
    assert Linv.shape[1] == m and u.is_contiguous() and u.numel() >= m
    if d is None:
        d = torch.empty(m, dtype=F64, device=Linv.device)
    if alpha is None:
        alpha = torch.empty(m, dtype=F64, device=Linv.device)
    assert d.is_contiguous() and alpha.is_contiguous() and d.numel() >= m and alpha.numel() >= m
    nbytes = lib.geobo_kinv_diag_ws_bytes(m)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = torch.empty(max(nbytes // 8, 1), dtype=F64, device=Linv.device)
    _lib.check(lib.geobo_kinv_diag(m, _p(Linv), ldl, _p(u), _p(_chk(d, "d")), _p(_chk(alpha, "alpha")), _p(_chk(ws, "ws")), nbytes,
                                   _stream()), "geobo_kinv_diag")
    return d, alpha


def set_loo(G, idx, alpha, n=None):
    """Leave-fold-out prediction of the C folds idx ((C, k) int32 rows, entries outside [0, n) are padding) from G[c] = [K^-1]_BB
    (set_gram) and alpha = K^-1 y: returns (out (2, C) = [log p(y_B | y_-B), white.white], resid, var, white (C, k each, NaN at
    padding), status (C,) int32 = 0 or 1 + failing pivot (NaN in everything of that fold))."""
    lib = require_gpu()
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 2 and idx.is_contiguous()):
        raise TypeError("idx must be a contiguous (C, k) CUDA int32 tensor")
    C_, k = idx.shape
    _chk(G, "G")
    alpha = _chk(alpha, "alpha")
    n = alpha.numel() if n is None else int(n)
    assert G.is_contiguous() and tuple(G.shape) == (C_, k, k) and alpha.is_contiguous() and alpha.numel() >= n
    dev = G.device
    out = torch.empty((2, C_), dtype=F64, device=dev)
    resid, var, white = (torch.empty((C_, k), dtype=F64, device=dev) for _ in range(3))
    status = torch.empty(C_, dtype=torch.int32, device=dev)
    _lib.check(lib.geobo_set_loo(C_, k, _p(G), _p(idx), _p(alpha), n, _p(out), _p(resid), _p(var), _p(white), _p(status), _stream()),
               "geobo_set_loo")
    return out, resid, var, white, status


def block_cov_ws_doubles(R, grid, box):
    """Workspace of block_cov for R rows, grid (ny, nx, nz) and box (by, bx, bz), in doubles."""
    nbytes = _lib.load().geobo_block_cov_ws_bytes(int(R), *(int(v) for v in grid), *(int(v) for v in box))
    if nbytes == 0:
        raise ValueError("block_cov: invalid rows %r, grid %r or box %r" % (R, tuple(grid), tuple(box)))
    return nbytes // 8


def block_cov(V, R, grid, box, C6, accumulate=False, ws=None):
    """C6[B] = (accumulate ? C6[B] : 0) + sum_{r < R} s_a[r, B] s_b[r, B] in the order (00, 01, 02, 11, 12, 22), s_a[r, B] the sum of
    V[a][r] over the voxels of block B (boxes of `box` = (by, bx, bz) voxels tiling `grid` = (ny, nx, nz) from the origin, partial at
    the far edges; block index (jy nbx + jx) nbz + jz).  V: three 2-D fp64 tiles of one leading dimension, columns in voxel order
    (iy, ix, iz); C6: (nblocks, 6) fp64."""
    lib = require_gpu()
    ldv = _rowmajor(V[0], "V")
    R = int(R)
    grid, box = tuple(int(v) for v in grid), tuple(int(v) for v in box)
    N = grid[0] * grid[1] * grid[2]
    for t in V:
        if _rowmajor(t, "V") != ldv or t.shape[0] < R or t.shape[1] < N:
            raise ValueError("the three tiles must share a leading dimension and hold R x N elements")
    nblocks = 1
    for n, b in zip(grid, box):
        nblocks *= (n + max(b, 1) - 1) // max(b, 1)
    _chk(C6, "C6")
    assert C6.is_contiguous() and tuple(C6.shape) == (nblocks, 6)
    need = block_cov_ws_doubles(R, grid, box)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=F64, device=C6.device)
    _lib.check(lib.geobo_block_cov(R, _p(V[0]), _p(V[1]), _p(V[2]), ldv, *grid, *box, 1 if accumulate else 0, _p(C6), _p(_chk(ws, "ws")),
                                   ws.numel() * 8, _stream()), "geobo_block_cov")
    return C6


def _samples(F, name):
    """(S, 3, n) fp64 CUDA tensor with unit element stride -> (S, n, sample stride, property stride)."""
    _chk(F, name)
    if F.dim() != 3 or F.shape[1] != 3 or F.stride(2) != 1:
        raise ValueError("%s must be (S, 3, n) with unit element stride" % name)
    return F.shape[0], F.shape[2], F.stride(0), F.stride(1)


def _cutoff_batch(F, grid, thresholds, lo, mask, weight):
    """A batch of realisations F (S, 3, n) against a cutoff set: the checks and host arrays that cutoff_stats, bodies and trace_stats
    share.  grid: (ny, nx, nz) holding the n elements, or None.  Returns (S, n, sample stride, property stride, t, lo_h, C)."""
    S, n, ss, ps = _samples(F, "F")
    if grid is not None and (len(grid) != 3 or n != grid[0] * grid[1] * grid[2]):
        raise ValueError("F holds %d elements per property, the grid %r does not" % (n, grid))
    t = np.array(thresholds, dtype=np.float64).reshape(-1)         # (own copies: contiguous and writable, as _doubles needs them)
    lo_h = np.full(3, -np.inf) if lo is None else np.array(lo, dtype=np.float64).reshape(-1)
    if lo_h.size != 3:
        raise ValueError("lo holds one lower bound per property")
    for x, name, dtype in ((mask, "mask", torch.uint8), (weight, "weight", torch.int32)):
        if x is not None:
            _chk(x, name, dtype)
            assert x.is_contiguous() and x.numel() == n
    return S, n, ss, ps, t, lo_h, t.size


def _int32(h, name, shape):
    """An optional contiguous int32 tensor of the given shape (the kernels' uint32 counters travel so: torch has no arithmetic on uint32)."""
    if h is not None:
        _chk(h, name, torch.int32)
        assert h.is_contiguous() and tuple(h.shape) == tuple(shape), name


def _opt(x):
    """The device pointer of an optional tensor (NULL for None)."""
    return C.c_void_p(None) if x is None else _p(x)


def _doubles(a):
    """A contiguous writable fp64 host array as the C array the ABI takes for `const double*` (it keeps `a` alive)."""
    return (C.c_double * a.size).from_buffer(a)


def _ws_or_new(ws, need, device):
    """ws if it holds `need` doubles, a new workspace otherwise."""
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=F64, device=device)
    return _chk(ws, "ws")


def box_means(F, grid, box, G=None, count=None):
    """Means of the S realisations F (S, 3, N; voxel order (iy, ix, iz)) over the boxes of `box` = (by, bx, bz) voxels tiling `grid` =
    (ny, nx, nz) from the origin (partial at the far edges; block index (jy nbx + jx) nbz + jz): returns (G (S, 3, nblocks) fp64,
    count (nblocks,) int32).  With the box (1, 1, 1) G equals F bit for bit."""
    lib = require_gpu()
    S, n, ss, ps = _samples(F, "F")
    grid, box = tuple(int(v) for v in grid), tuple(int(v) for v in box)
    if n != grid[0] * grid[1] * grid[2]:
        raise ValueError("F holds %d elements per property, the grid %r has %d" % (n, grid, grid[0] * grid[1] * grid[2]))
    nblocks = 1
    for m, b in zip(grid, box):
        nblocks *= (m + max(b, 1) - 1) // max(b, 1)
    if G is None:
        G = torch.empty((S, 3, nblocks), dtype=F64, device=F.device)
    if count is None:
        count = torch.empty(nblocks, dtype=torch.int32, device=F.device)
    _chk(G, "G")
    _chk(count, "count", torch.int32)
    assert G.is_contiguous() and tuple(G.shape) == (S, 3, nblocks) and count.is_contiguous() and count.numel() == nblocks
    _lib.check(lib.geobo_box_means(S, _p(F), ss, ps, *grid, *box, _p(G), _p(count), _stream()), "geobo_box_means")
    return G, count


def cutoff_stats_ws_doubles(S, n, C):
    nbytes = _lib.load().geobo_cutoff_stats_ws_bytes(int(S), int(n), int(C))
    if nbytes == 0:
        raise ValueError("cutoff_stats: invalid samples %r, elements %r or cutoffs %r" % (S, n, C))
    return nbytes // 8


def cutoff_stats(F, p, thresholds, lo=None, mask=None, weight=None, hits=None, ws=None):
    """S cubes F (S, 3, n) against the ascending `thresholds` (host sequence of C <= 32 doubles, -inf allowed) of property p: element v
    of sample s passes cutoff c when F[s, p, v] >= thresholds[c], F[s, q, v] >= lo[q] for the other two properties (lo: three host
    doubles, -inf = not read; default all -inf) and mask[v] != 0 (mask: (n,) uint8 or None); NaN fails.  Returns (cnt (S, C) int64 =
    sum of the weights (weight: (n,) int32, None = 1) of the passing elements, sum (S, C) fp64 = sum of weight x value); hits
    ((C, n) int32 or None) is incremented by one per passing sample.  Bitwise reproducible, the same for any grouping of samples."""
    lib = require_gpu()
    S, n, ss, ps, t, lo_h, C_ = _cutoff_batch(F, None, thresholds, lo, mask, weight)
    _int32(hits, "hits", (C_, n))
    ws = _ws_or_new(ws, cutoff_stats_ws_doubles(S, n, C_), F.device)
    cnt = torch.empty((S, C_), dtype=torch.int64, device=F.device)
    tot = torch.empty((S, C_), dtype=F64, device=F.device)
    _lib.check(lib.geobo_cutoff_stats(S, _p(F), ss, ps, n, int(p), C_, _doubles(t), _doubles(lo_h), _opt(mask), _opt(weight), _p(cnt), _p(tot),
                                      _opt(hits), _p(ws), ws.numel() * 8, _stream()), "geobo_cutoff_stats")
    return cnt, tot


BODIES_INIT, BODIES_MERGE, BODIES_FLATTEN, BODIES_STATS, BODIES_ALL, BODIES_TILED = 1, 2, 4, 8, 15, 16
BODY_STATS = ("count_total", "n_bodies", "largest_count", "largest_label", "seeded_count", "seeded_bodies")     # columns of stats
BODY_SUMS = ("total", "largest", "seeded")                                                                       # columns of sums


def bodies_ws_doubles(S, grid, C):
    nbytes = _lib.load().geobo_bodies_ws_bytes(int(S), *[int(v) for v in grid], int(C))
    if nbytes == 0:
        raise ValueError("bodies: invalid samples %r, grid %r or cutoffs %r (samples x cutoffs <= 65535)" % (S, tuple(grid), C))
    return nbytes // 8


def bodies(F, grid, p, thresholds, lo=None, mask=None, weight=None, neighbours=6, min_count=1, seeds=None, hits_largest=None,
           hits_seeded=None, labels=None, info=None, ws=None, phases=BODIES_ALL, stats=None, sums=None, tiled=True):
    """Connected bodies of the cutoff sets of S cubes F (S, 3, n) on `grid` = (ny, nx, nz), n = ny nx nz: the set of (s, c) is that of
    cutoff_stats (same thresholds, lo, mask, weight); bodies are its components under `neighbours` = 6 or 26.  seeds: host sequence of
    K voxel indices or None.  Returns (stats (S, C, 6) int64 -- the columns BODY_STATS --, sums (S, C, 3) fp64 -- BODY_SUMS --, info
    (one int32 on the device: 0 unless a bounded walk ran out, which the caller turns into an error)).  hits_largest, hits_seeded:
    (C, n) int32 or None, incremented per sample whose largest / seeded body holds the voxel; labels: (S, C, n) int32 or None, the
    smallest voxel index of each voxel's body, -1 outside.  Exact counts, bitwise reproducible sums.  tiled=False: the merge stage
    without its tile-local phase in LDS (the same results, slower)."""
    lib = require_gpu()
    grid = tuple(int(v) for v in grid)
    S, n, ss, ps, t, lo_h, C_ = _cutoff_batch(F, grid, thresholds, lo, mask, weight)
    dev = F.device
    _int32(hits_largest, "hits_largest", (C_, n))
    _int32(hits_seeded, "hits_seeded", (C_, n))
    _int32(labels, "labels", (S, C_, n))
    sd = np.ascontiguousarray(np.zeros(0, dtype=np.int32) if seeds is None else np.asarray(seeds, dtype=np.int32).reshape(-1))
    ws = _ws_or_new(ws, bodies_ws_doubles(S, grid, C_), dev)
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=dev)
    _chk(info, "info", torch.int32)
    if stats is None:
        stats = torch.empty((S, C_, len(BODY_STATS)), dtype=torch.int64, device=dev)
    if sums is None:
        sums = torch.empty((S, C_, len(BODY_SUMS)), dtype=F64, device=dev)
    _chk(stats, "stats", torch.int64)
    _chk(sums, "sums")
    assert stats.is_contiguous() and tuple(stats.shape) == (S, C_, 6) and sums.is_contiguous() and tuple(sums.shape) == (S, C_, 3)
    _lib.check(lib.geobo_bodies(S, _p(F), ss, ps, *grid, int(p), C_, _doubles(t), _doubles(lo_h), _opt(mask), _opt(weight), int(neighbours),
                                int(min_count), sd.size, sd.ctypes.data_as(C.POINTER(C.c_int32)), _p(stats), _p(sums), _opt(hits_largest),
                                _opt(hits_seeded), _opt(labels), _p(info), int(phases) | (BODIES_TILED if tiled else 0), _p(ws), ws.numel() * 8,
                                _stream()), "geobo_bodies")
    if sd.size and (phases & BODIES_STATS):
        torch.cuda.current_stream().synchronize()     # the staging copy of the host seeds has been read before `sd` goes away
    return stats, sums, info


TRACE_LMAX = 4096
TRACE_DETAIL = ("thick", "top", "start", "len", "n_int", "zero")     # columns of detail
TRACE_DSUM = ("acc", "run_sum")                                       # columns of dsum
TRACE_TAB = ("holes_hit", "thick", "longest")                         # columns of tab
TRACE_MAPS = (("hits_any", torch.int32), ("hits", torch.int32), ("thick_sum", torch.int64), ("top_sum", torch.int64), ("acc_sum", F64),
              ("hist_len", torch.int32), ("hist_thick", torch.int32))


def check_traces(offsets, voxels, n):
    """Host validation of a CSR trace list for geobo_trace_stats (which cannot read the device copies): offsets (K + 1,) ascending from
    0 with lengths in 1 .. 4096, voxels (offsets[K],) in 0 .. n - 1.  Returns (offsets int32, voxels int32, K, Lmax); ValueError
    otherwise."""
    off = np.asarray(offsets)
    vox = np.asarray(voxels)
    if off.ndim != 1 or off.size < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("trace offsets are a 1-D integer array of K + 1 >= 2 entries")
    if vox.ndim != 1 or not np.issubdtype(vox.dtype, np.integer):
        raise ValueError("trace voxels are a 1-D integer array")
    off, vox = off.astype(np.int64), vox.astype(np.int64)
    if off[0] != 0 or off[-1] != vox.size or vox.size > np.iinfo(np.int32).max:
        raise ValueError("trace offsets run from 0 to the number of voxels (%d), got %d .. %d" % (vox.size, off[0], off[-1]))
    length = np.diff(off)
    if length.min() < 1 or length.max() > TRACE_LMAX:
        raise ValueError("a trace holds between 1 and %d positions, got %d .. %d" % (TRACE_LMAX, length.min(), length.max()))
    if vox.min() < 0 or vox.max() >= int(n):
        raise ValueError("a trace voxel lies outside 0 .. %d" % (int(n) - 1))
    return np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(vox, dtype=np.int32), int(off.size - 1), int(length.max())


class TraceSet:
    """A validated CSR trace list on the device (built once, used by every launch)."""

    def __init__(self, offsets, voxels, n, device="cuda"):
        off, vox, self.K, self.Lmax = check_traces(offsets, voxels, n)
        self.n = int(n)
        self.lengths = np.diff(off.astype(np.int64))
        require_gpu()
        self.offsets = torch.as_tensor(off, device=device)
        self.voxels = torch.as_tensor(vox, device=device)


def trace_stats_ws_doubles(S, K, C):
    nbytes = _lib.load().geobo_trace_stats_ws_bytes(int(S), int(K), int(C))
    if nbytes == 0:
        raise ValueError("trace_stats: invalid samples %r, traces %r or cutoffs %r" % (S, K, C))
    return nbytes // 8


def trace_maps(C, K, Lmax, device="cuda", hist=True):
    """The zeroed accumulators of trace_stats: dict of hits_any, hits (C, K) int32, thick_sum, top_sum (C, K) int64, acc_sum (C, K)
    fp64 and with hist hist_len, hist_thick (C, K, Lmax + 1) int32."""
    out = {}
    for name, dtype in TRACE_MAPS:
        if name.startswith("hist"):
            if hist:
                out[name] = torch.zeros((C, K, Lmax + 1), dtype=dtype, device=device)
        else:
            out[name] = torch.zeros((C, K), dtype=dtype, device=device)
    return out


def trace_stats(F, grid, p, thresholds, lo=None, mask=None, traces=None, min_len=1, max_gap=0, maps=None, detail=None, dsum=None,
                tab=None, ws=None):
    """Drill-intercept statistics of S cubes F (S, 3, n) on `grid` = (ny, nx, nz) along traces: `traces` = a TraceSet, or None for
    the ny nx z-columns.  The ore of (s, c) is the set of cutoff_stats (same thresholds, lo, mask); a run of non-ore positions of at
    most max_gap samples, all eligible, between two ore positions is filled; the longest run of the result is the BEST intercept
    and counts as a hit from min_len samples on.  Returns tab (S, C, 3) int64 -- the columns TRACE_TAB.  maps: dict of accumulators
    (trace_maps; any subset), incremented; detail (S, C, K, 6) int32 -- TRACE_DETAIL -- and dsum (S, C, K, 2) fp64 -- TRACE_DSUM --
    are written when given.  Exact integers, bitwise reproducible sums, the same for any grouping of samples."""
    lib = require_gpu()
    grid = tuple(int(v) for v in grid)
    S, n, ss, ps, t, lo_h, C_ = _cutoff_batch(F, grid, thresholds, lo, mask, None)
    dev = F.device
    if traces is None:
        K, Lmax, off_p, vox_p = grid[0] * grid[1], grid[2], _opt(None), _opt(None)
    else:
        if not isinstance(traces, TraceSet) or traces.n != n:
            raise ValueError("traces is a TraceSet validated for the %d voxels of F" % n)
        K, Lmax, off_p, vox_p = traces.K, traces.Lmax, _p(traces.offsets), _p(traces.voxels)
    maps = maps or {}
    ptr = {}
    for name, dtype in TRACE_MAPS:
        m = maps.get(name)
        if m is not None:
            _chk(m, name, dtype)                      # (the kernel's uint32 counters travel as int32: torch has no arithmetic on uint32)
            assert m.is_contiguous() and tuple(m.shape) == ((C_, K, Lmax + 1) if name.startswith("hist") else (C_, K)), name
        ptr[name] = _opt(m)
    if set(maps) - set(ptr):
        raise ValueError("unknown maps %r" % sorted(set(maps) - set(ptr)))
    _int32(detail, "detail", (S, C_, K, 6))
    if dsum is not None:
        _chk(dsum, "dsum")
        assert dsum.is_contiguous() and tuple(dsum.shape) == (S, C_, K, 2)
    if tab is None:
        tab = torch.empty((S, C_, 3), dtype=torch.int64, device=dev)
    _chk(tab, "tab", torch.int64)
    assert tab.is_contiguous() and tuple(tab.shape) == (S, C_, 3)
    ws = _ws_or_new(ws, trace_stats_ws_doubles(S, K, C_), dev)
    _lib.check(lib.geobo_trace_stats(S, _p(F), ss, ps, *grid, int(p), C_, _doubles(t), _doubles(lo_h), _opt(mask), K, off_p, vox_p, Lmax,
                                     int(min_len), int(max_gap), _p(tab), ptr["hits_any"], ptr["hits"], ptr["thick_sum"], ptr["top_sum"],
                                     ptr["acc_sum"], ptr["hist_len"], ptr["hist_thick"], _opt(detail), _opt(dsum), _p(ws), ws.numel() * 8,
                                     _stream()), "geobo_trace_stats")
    return tab


def mfma_f64_peak(blocks=1024, iters=20000):
    """Time the v_mfma_f64_16x16x4_f64 issue rate; returns TFLOP/s (4 waves/WG x 16 MFMA x 2048 flop per iter)."""
    lib = require_gpu()
    out = torch.empty(blocks * 256, dtype=F64, device="cuda")
    _lib.check(lib.geobo_mfma_f64_peak(blocks, 100, _p(out), _stream()), "geobo_mfma_f64_peak")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(lib.geobo_mfma_f64_peak(blocks, iters, _p(out), _stream()), "geobo_mfma_f64_peak")
    e1.record()
    torch.cuda.synchronize()
    secs = e0.elapsed_time(e1) * 1e-3
    return blocks * 4 * iters * 16 * 2048.0 / secs / 1e12


def to_dev(a, device="cuda"):
    require_gpu()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=F64).to(device)


# ---- prior sampler by circulant embedding (sampling.hip) ----------------------------------------------------------------------
RNG_PRIOR, RNG_OBS = 0, 1
FFT_INVERSE, FFT_IN_PAIRS, FFT_OUT_PAIRS, FFT_MAX = 1, 2, 4, 512


def philox_fill(seed, purpose, sample0, nsamples, elem0, nelem, sub=0, raw=False, out=None, device="cuda"):
    """(nsamples, nelem, 4) Philox4x64-10 blocks of counters (elem0 + e, sample0 + s, purpose, sub), key (seed, 0): raw 64-bit words
    (int64 tensor holding the uint64 bits) or fp64 Box-Muller normals."""
    lib = require_gpu()
    if out is None:
        out = torch.empty((int(nsamples), int(nelem), 4), dtype=torch.int64 if raw else F64, device=device)
    _lib.check(lib.geobo_philox_fill(1 if raw else 0, int(seed), int(purpose), int(sample0), int(nsamples), int(elem0), int(nelem), int(sub),
                                     _p(out), _stream()), "geobo_philox_fill")
    return out


def torus_table(kid, my, mx, mz, sx, sy, sz, l1, l2, w, amp, out):
    """out (my*mx*mz*2 fp64, complex interleaved) = w amp k at the wrapped lags of the (my, mx, mz) torus."""
    lib = require_gpu()
    assert out.numel() >= 2 * my * mx * mz
    _lib.check(lib.geobo_torus_table(int(kid), int(my), int(mx), int(mz), float(sx), float(sy), float(sz), float(l1), float(l2), float(w),
                                     float(amp), _p(_chk(out, "out")), _stream()), "geobo_torus_table")
    return out


def fft_axis(flags, b0, m, b1, n_in, n_out, src, out, P=0, Q=0, S=0):
    """Batched complex FFT along the middle axis of [b0][len][b1] (geobo_fft_axis).  Extents are checked against both allocations here."""
    lib = require_gpu()
    pairs_in, pairs_out = flags & FFT_IN_PAIRS, flags & FFT_OUT_PAIRS
    need_in = (S * P * Q) if pairs_in else 2 * b0 * n_in * b1
    need_out = (S * P * Q) if pairs_out else 2 * b0 * n_out * b1
    if pairs_in or pairs_out:
        assert (b0 * (n_in if pairs_in else n_out) * b1) == ((S + 1) // 2) * P * Q, "pair packing: extents do not match (S, P, Q)"
    if src.numel() < need_in or out.numel() < need_out:
        raise ValueError("geobo_fft_axis: operand smaller than its extents")
    _lib.check(lib.geobo_fft_axis(int(flags), int(b0), int(m), int(b1), int(n_in), int(n_out), _p(_chk(src, "src")), _p(_chk(out, "out")),
                                  int(P), int(Q), int(S), _stream()), "geobo_fft_axis")
    return out


def sample_factor(P, my, mx, mz, spectra, F, lam, ws, status):
    lib = require_gpu()
    no = (my // 2 + 1) * (mx // 2 + 1) * (mz // 2 + 1)
    assert spectra.numel() >= P * (P + 1) * my * mx * mz and F.numel() >= no * P * P and lam.numel() >= no * P * (P + 1) // 2
    _lib.check(lib.geobo_sample_factor(int(P), int(my), int(mx), int(mz), _p(_chk(spectra, "spectra")), _p(_chk(F, "F")), _p(_chk(lam, "lam")),
                                       _p(ws), ws.numel() * ws.element_size(), _p(_chk(status, "status")), _stream()), "geobo_sample_factor")
    return status


def sample_factor_ws_doubles():
    return int(_lib.load().geobo_sample_factor_ws_bytes()) // 8


def sample_zpass(P, pair0, npairs, my, mx, mz, nz, F, out, seed=0, noise=None):
    """Noise -> F / sqrt(M) -> inverse z FFT, cropped: out (npairs * P * my * mx * nz complex)."""
    lib = require_gpu()
    assert out.numel() >= 2 * npairs * P * my * mx * nz
    if noise is not None:
        assert _chk(noise, "noise").numel() >= 2 * npairs * my * mx * mz * P
    _lib.check(lib.geobo_sample_zpass(int(P), int(pair0), int(npairs), int(my), int(mx), int(mz), int(nz), _p(_chk(F, "F")),
                                      _p(noise) if noise is not None else None, int(seed), _p(_chk(out, "out")), _stream()), "geobo_sample_zpass")
    return out


def spectral_mix(P, npairs, my, mx, mz, lam, scale, src, out):
    lib = require_gpu()
    assert src.numel() >= 2 * npairs * P * my * mx * mz and out.numel() >= 2 * npairs * P * my * mx * mz
    _lib.check(lib.geobo_spectral_mix(int(P), int(npairs), int(my), int(mx), int(mz), _p(_chk(lam, "lam")), float(scale), _p(_chk(src, "src")),
                                      _p(_chk(out, "out")), _stream()), "geobo_spectral_mix")
    return out
