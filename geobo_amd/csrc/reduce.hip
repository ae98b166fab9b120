// reduce.hip -- the two streaming reductions of the shape-independent forms of the structured algorithm: what the fused n = 64
// kernels of xz2d_fold.hip do inside their epilogues, as stand-alone HBM-bound passes for every other grid extent.
//
//   geobo_sumsq_accum   ss[slot][c] += sum_{r = slot (mod slots)} (a[r][c] + b[r][c])^2
//                       diag(K - V^T V) of inversion.py:117,238 in the transposed order V = (L^-1 A3) K: a batch of rows of V comes out
//                       of the storing covariance product (any transform path), is squared and summed over the rows here.
//                       Deterministic: a (slot, column) pair is owned by one thread, rows are added in ascending order.
//   geobo_lamdot_z      out[b][o] = sum_z D[b][o][z] * lam[b % planes][o][z]
//                       x step of the lattice Gram (AkA on a lattice survey, inversion.py:96) behind a batched GEMM D = Gx X: the
//                       eigenvalue scaling and the channel (z) sum.  Eight lanes share one (plane, o) row of nz doubles: 16-byte loads,
//                       128 contiguous bytes per lane group, three shuffle steps.
//   geobo_rowgemv       out[r] = sum_c X[r][c] * v[c]
//                       a forward operator applied to a model, data = A rho (simcube.py:147-150; the synthetic surveys of bench.py and of
//                       the tests): one workgroup per row, 16-byte loads, a fixed reduction tree (deterministic).  HBM read bound.
//   geobo_centro_fill   B[r][c] = B[n-1-r][n-1-c] for r >= r0: the second half of a centrosymmetric block of AkA (inversion.py:96) from its
//                       first half -- the magnetic block of a row-major lattice survey under a vertical field.  Stream copy.
//   geobo_transpose     dst = src^T, tiled through LDS: the lower-left block of AkA from the upper-right one the lattice Gram computed.
//   geobo_sym_add       B += E + E^T on a square block, the transposed tiles through LDS: the two boundary-slab cross terms of AkA's
//                       gravity block from ONE sweep of the lattice Gram's slab stage ("gravity block from half its rows").
//   geobo_mirror_rows   the same point mirror on rows of A K (voxel blocks of nz doubles reversed, z kept): for readers of the rows
//                       the step did not compute.
//   geobo_mirror_planes ... on ONE (x, z) plane of every row, between two buffers: the boundary planes of the mirrored rows of A_m K_10
//                       (the lattice Gram's boundary-slab term reads nothing else of them).
//   geobo_mirror_dev    max |a - mirror(b)| and max |a|, |b| of a lattice operator's stencil table / boundary slabs: the measurement
//                       that decides whether geobo_centro_fill may stand for the product.  Slot-owned partial maxima + one finishing
//                       pass, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "geobo_hip.h"

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256) sumsq_accum_kernel(int64_t rows, int64_t n2, const double* __restrict__ a, int64_t lda,
                                                          const double* __restrict__ b, int64_t ldb, int slots, double* __restrict__ ss,
                                                          int64_t ld_ss) {
  const int64_t c2 = (int64_t)blockIdx.x * 256 + threadIdx.x;      // column pair
  if (c2 >= n2) return;
  const int slot = blockIdx.y;
  v2d acc = *reinterpret_cast<const v2d*>(ss + slot * ld_ss + 2 * c2);
  if (b) {
    for (int64_t r = slot; r < rows; r += slots) {
      const v2d x = *reinterpret_cast<const v2d*>(a + r * lda + 2 * c2) + *reinterpret_cast<const v2d*>(b + r * ldb + 2 * c2);
      acc.x = __builtin_fma(x.x, x.x, acc.x);
      acc.y = __builtin_fma(x.y, x.y, acc.y);
    }
  } else {
    for (int64_t r = slot; r < rows; r += slots) {
      const v2d x = *reinterpret_cast<const v2d*>(a + r * lda + 2 * c2);
      acc.x = __builtin_fma(x.x, x.x, acc.x);
      acc.y = __builtin_fma(x.y, x.y, acc.y);
    }
  }
  *reinterpret_cast<v2d*>(ss + slot * ld_ss + 2 * c2) = acc;
}

// 8 lanes per (batch plane, o) row; 32 rows per 256-thread workgroup
__global__ void __launch_bounds__(256) lamdot_z_kernel(int64_t nrows, int planes, int px, int nz, const double* __restrict__ D,
                                                       const double* __restrict__ lam, double* __restrict__ out) {
  const int sub = threadIdx.x & 7;
  for (int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3); row < nrows; row += (int64_t)gridDim.x * 32) {
    const int64_t bp = row / px;                                   // batch plane (r, p)
    const int o = (int)(row - bp * px);
    const double* d = D + row * nz;
    const double* l = lam + ((int64_t)(bp % planes) * px + o) * nz;
    double acc = 0.0;
    for (int z = 2 * sub; z < nz; z += 16) {
      const v2d x = *reinterpret_cast<const v2d*>(d + z), y = *reinterpret_cast<const v2d*>(l + z);
      acc = __builtin_fma(x.x, y.x, acc);
      acc = __builtin_fma(x.y, y.y, acc);
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    if (sub == 0) out[row] = acc;
  }
}

__global__ void __launch_bounds__(256) rowgemv_kernel(int64_t m, int64_t n2, const double* __restrict__ X, int64_t ld,
                                                      const double* __restrict__ v, double* __restrict__ out) {
  __shared__ double part[4];
  for (int64_t r = blockIdx.x; r < m; r += gridDim.x) {
    const v2d* x = reinterpret_cast<const v2d*>(X + r * ld);
    const v2d* w = reinterpret_cast<const v2d*>(v);
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < n2; c += 256) {
      const v2d a = x[c], b = w[c];
      acc = __builtin_fma(a.x, b.x, acc);
      acc = __builtin_fma(a.y, b.y, acc);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[r] = (part[0] + part[1]) + (part[2] + part[3]);
    __syncthreads();
  }
}

// ---- the point mirror of a lattice survey (inversion.py:96 on a centrosymmetric magnetic block) --------------------------------
// One thread per 16-byte pair of the SOURCE row n-1-r: loaded aligned, swapped in registers, stored at the mirrored columns
// (one 16-byte store when n is even, two 8-byte vector stores when n is odd: the mirrored pair then starts on an odd column).
__global__ void __launch_bounds__(256) centro_fill_kernel(double* __restrict__ B, int64_t ld, int64_t n, int64_t r0) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = 2 * p;
  if (c >= n) return;
  for (int64_t r = r0 + blockIdx.y; r < n; r += gridDim.y) {
    const double* src = B + (n - 1 - r) * ld;       // 2 r0 >= n: r >= r0 > n-1-r, a source row is never a destination
    double* dst = B + r * ld;
    if (c + 1 < n) {
      const v2d v = *reinterpret_cast<const v2d*>(src + c);
      if ((n & 1) == 0) {
        v2d w;
        w.x = v.y;
        w.y = v.x;
        *reinterpret_cast<v2d*>(dst + (n - 2 - c)) = w;
      } else {
        dst[n - 2 - c] = v.y;
        dst[n - 1 - c] = v.x;
      }
    } else {
      dst[0] = src[c];                              // n odd: the last column stands alone
    }
  }
}

// X[r][b][:] = X[m-1-r][nb-1-b][:] for r0 <= r < m: rows as nb blocks of nz doubles (voxel (iy, ix) blocks of a row of A K)
__global__ void __launch_bounds__(256) mirror_rows_kernel(double* __restrict__ X, int64_t ld, int64_t m, int64_t r0, int64_t nb, int nz2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // 16-byte pair of the destination row
  if (e >= nb * nz2) return;
  const int64_t b = e / nz2;
  const int64_t se = (nb - 1 - b) * nz2 + (e - b * nz2);
  for (int64_t r = r0 + blockIdx.y; r < m; r += gridDim.y)
    reinterpret_cast<v2d*>(X + r * ld)[e] = reinterpret_cast<const v2d*>(X + (m - 1 - r) * ld)[se];
}

// dst[m-1-r][x][:] = src[r][nx-1-x][:] for r0 <= r < r1: ONE (x, z) plane per row under the point mirror (the y index is the caller's:
// src and dst point at opposite boundary planes of the rows).  One thread per 16-byte pair of the destination plane.
__global__ void __launch_bounds__(256) mirror_planes_kernel(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd,
                                                            int64_t m, int64_t r0, int64_t r1, int nx, int nz2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)nx * nz2) return;
  const int64_t x = e / nz2;
  const int64_t se = (nx - 1 - x) * nz2 + (e - x * nz2);
  for (int64_t r = r0 + blockIdx.y; r < r1; r += gridDim.y)
    reinterpret_cast<v2d*>(dst + (m - 1 - r) * ldd)[e] = reinterpret_cast<const v2d*>(src + r * lds)[se];
}

// NaN-keeping maximum: a NaN anywhere makes the result NaN (the gate that reads it then says no)
__device__ __forceinline__ double max_keep_nan(double m, double v) { return (v > m || v != v) ? v : m; }

constexpr int MIRROR_SLOTS_X = 4, MIRROR_SLOTS_Y = 256;           // slot-owned partial maxima: [y][x][2]

__global__ void __launch_bounds__(256) mirror_dev_kernel(const double* __restrict__ a, int64_t lda, const double* __restrict__ b, int64_t ldb,
                                                         int64_t rows, int nx, int nz2, double* __restrict__ part) {
  __shared__ double sh[2][4];
  double dev = 0.0, mx = 0.0;
  const int pairs = nx * nz2;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const v2d* pa = reinterpret_cast<const v2d*>(a + r * lda);
    const v2d* pb = reinterpret_cast<const v2d*>(b + (rows - 1 - r) * ldb);
    for (int e = blockIdx.x * 256 + threadIdx.x; e < pairs; e += gridDim.x * 256) {
      const int x = e / nz2;
      const v2d u = pa[e], w = pb[(nx - 1 - x) * nz2 + (e - x * nz2)];
      dev = max_keep_nan(max_keep_nan(dev, __builtin_fabs(u.x - w.x)), __builtin_fabs(u.y - w.y));
      mx = max_keep_nan(max_keep_nan(mx, __builtin_fabs(u.x)), __builtin_fabs(u.y));
      mx = max_keep_nan(max_keep_nan(mx, __builtin_fabs(w.x)), __builtin_fabs(w.y));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    dev = max_keep_nan(dev, __shfl_xor(dev, o));
    mx = max_keep_nan(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = dev;
    sh[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double* s = sh[threadIdx.x];
    part[2 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = max_keep_nan(max_keep_nan(s[0], s[1]), max_keep_nan(s[2], s[3]));
  }
}

// the finishing pass: one workgroup folds the slots in a fixed order
__global__ void __launch_bounds__(256) mirror_dev_finish_kernel(const double* __restrict__ part, int slots, double* __restrict__ out) {
  __shared__ double sh[2][4];
  double dev = 0.0, mx = 0.0;
  for (int s = threadIdx.x; s < slots; s += 256) {
    dev = max_keep_nan(dev, part[2 * s]);
    mx = max_keep_nan(mx, part[2 * s + 1]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    dev = max_keep_nan(dev, __shfl_xor(dev, o));
    mx = max_keep_nan(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = dev;
    sh[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double* s = sh[threadIdx.x];
    out[threadIdx.x] = max_keep_nan(max_keep_nan(s[0], s[1]), max_keep_nan(s[2], s[3]));
  }
}

// dst[c][r] = src[r][c]: one 64 x 64 tile per workgroup through LDS (row stride 65: the transposed reads are conflict free), 512-byte
// runs on both sides
__global__ void __launch_bounds__(256) transpose_kernel(int64_t rows, int64_t cols, const double* __restrict__ src, int64_t lds,
                                                        double* __restrict__ dst, int64_t ldd) {
  __shared__ double t[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
#pragma unroll 4
  for (int i = ty; i < 64; i += 4)
    if (r0 + i < rows && c0 + tx < cols) t[i][tx] = src[(r0 + i) * lds + c0 + tx];
  __syncthreads();
#pragma unroll 4
  for (int i = ty; i < 64; i += 4)
    if (c0 + i < cols && r0 + tx < rows) dst[(c0 + i) * ldd + r0 + tx] = t[tx][i];
}

// B[r][c] += E[r][c] + E[c][r]: the tile (r0, c0) of B takes the tile of E in place and the tile (c0, r0) of E through LDS, as
// transpose_kernel reads it.  Every element of B has one owner: no atomics.
__global__ void __launch_bounds__(256) sym_add_kernel(int64_t n, const double* __restrict__ E, int64_t lde, double* __restrict__ B, int64_t ldb) {
  __shared__ double t[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
#pragma unroll 4
  for (int i = ty; i < 64; i += 4)
    if (c0 + i < n && r0 + tx < n) t[i][tx] = E[(c0 + i) * lde + r0 + tx];
  __syncthreads();
#pragma unroll 4
  for (int i = ty; i < 64; i += 4)
    if (r0 + i < n && c0 + tx < n) B[(r0 + i) * ldb + c0 + tx] += E[(r0 + i) * lde + c0 + tx] + t[tx][i];
}

}  // namespace

extern "C" int geobo_sym_add(int64_t n, const double* E, int64_t lde, double* B, int64_t ldb, void* stream) {
  if (!E || !B || n < 0 || lde < n || ldb < n || (n + 63) / 64 > 65535) return GEOBO_E_ARG;
  if (n == 0) return GEOBO_OK;
  const unsigned nt = (unsigned)((n + 63) / 64);
  hipLaunchKernelGGL(sym_add_kernel, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, n, E, lde, B, ldb);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_transpose(int64_t rows, int64_t cols, const double* src, int64_t lds, double* dst, int64_t ldd, void* stream) {
  if (!src || !dst || rows < 0 || cols < 0 || lds < cols || ldd < rows || (rows + 63) / 64 > 65535) return GEOBO_E_ARG;
  if (rows == 0 || cols == 0) return GEOBO_OK;
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64)), dim3(256), 0, (hipStream_t)stream,
                     rows, cols, src, lds, dst, ldd);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_centro_fill(double* B, int64_t ld, int64_t n, int64_t r0, void* stream) {
  if (!B || ((uintptr_t)B & 15) || n < 0 || r0 < 0 || r0 > n || 2 * r0 < n || ld < n) return GEOBO_E_ARG;
  if (ld & 1) return GEOBO_E_ALIGN;
  if (r0 == n) return GEOBO_OK;
  const int64_t gy = n - r0 < 65535 ? n - r0 : 65535;
  hipLaunchKernelGGL(centro_fill_kernel, dim3((unsigned)(((n + 1) / 2 + 255) / 256), (unsigned)gy), dim3(256), 0, (hipStream_t)stream, B, ld, n, r0);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_mirror_rows(double* X, int64_t ld, int64_t m, int64_t r0, int64_t nb, int nz, void* stream) {
  if (!X || m < 0 || r0 < 0 || r0 > m || 2 * r0 < m || nb <= 0 || nz <= 0 || nb * nz > ld) return GEOBO_E_ARG;
  if ((nz & 1) || (ld & 1) || ((uintptr_t)X & 15)) return GEOBO_E_ALIGN;
  if (r0 == m) return GEOBO_OK;
  const int64_t pairs = nb * (nz / 2), gy = m - r0 < 65535 ? m - r0 : 65535;
  hipLaunchKernelGGL(mirror_rows_kernel, dim3((unsigned)((pairs + 255) / 256), (unsigned)gy), dim3(256), 0, (hipStream_t)stream, X, ld, m, r0, nb,
                     nz / 2);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_mirror_planes(const double* src, int64_t lds, double* dst, int64_t ldd, int64_t m, int64_t r0, int64_t r1, int nx, int nz,
                                   void* stream) {
  if (!src || !dst || m < 0 || r0 < 0 || r0 > r1 || r1 > m || nx <= 0 || nz <= 0 || (int64_t)nx * nz > lds || (int64_t)nx * nz > ldd)
    return GEOBO_E_ARG;
  if ((nz & 1) || (lds & 1) || (ldd & 1) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return GEOBO_E_ALIGN;
  if (r0 == r1) return GEOBO_OK;
  const int64_t pairs = (int64_t)nx * (nz / 2), gy = r1 - r0 < 65535 ? r1 - r0 : 65535;
  hipLaunchKernelGGL(mirror_planes_kernel, dim3((unsigned)((pairs + 255) / 256), (unsigned)gy), dim3(256), 0, (hipStream_t)stream, src, lds, dst,
                     ldd, m, r0, r1, nx, nz / 2);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" size_t geobo_mirror_dev_ws_bytes(void) { return sizeof(double) * 2 * MIRROR_SLOTS_X * MIRROR_SLOTS_Y; }

extern "C" int geobo_mirror_dev(const double* a, int64_t lda, const double* b, int64_t ldb, int64_t rows, int nx, int nz, double* out2, void* ws,
                                size_t ws_bytes, void* stream) {
  if (!a || !b || !out2 || !ws || rows <= 0 || nx <= 0 || nz <= 0 || ws_bytes < geobo_mirror_dev_ws_bytes()) return GEOBO_E_ARG;
  if ((int64_t)nx * nz > lda || (int64_t)nx * nz > ldb || (int64_t)nx * nz >= (1LL << 31)) return GEOBO_E_ARG;
  if ((nz & 1) || (lda & 1) || (ldb & 1) || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)ws & 15)) return GEOBO_E_ALIGN;
  const int pairs = nx * (nz / 2);
  const int gx = (pairs + 255) / 256 < MIRROR_SLOTS_X ? (pairs + 255) / 256 : MIRROR_SLOTS_X;
  const int gy = rows < MIRROR_SLOTS_Y ? (int)rows : MIRROR_SLOTS_Y;
  hipLaunchKernelGGL(mirror_dev_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, rows, nx, nz / 2, (double*)ws);
  hipLaunchKernelGGL(mirror_dev_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, gx * gy, out2);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_rowgemv(int64_t m, int64_t n, const double* X, int64_t ld, const double* v, double* out, void* stream) {
  if (!X || !v || !out) return GEOBO_E_ARG;
  if (m <= 0 || n <= 0) return GEOBO_OK;
  if ((n & 1) || (ld & 1) || ld < n || ((uintptr_t)X & 15) || ((uintptr_t)v & 15)) return GEOBO_E_ALIGN;
  const int64_t nb = m < 256 * 16 ? m : 256 * 16;
  hipLaunchKernelGGL(rowgemv_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, m, n / 2, X, ld, v, out);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_sumsq_accum(int64_t rows, int64_t n, const double* a, int64_t lda, const double* b, int64_t ldb, int slots,
                                 double* ss, int64_t ld_ss, void* stream) {
  if (!a || !ss) return GEOBO_E_ARG;
  if (rows <= 0 || n <= 0) return GEOBO_OK;
  if (slots < 1 || slots > 65535) return GEOBO_E_ARG;
  if ((n & 1) || (lda & 1) || (ldb & 1) || (ld_ss & 1) || lda < n || (b && ldb < n) || ld_ss < n || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) ||
      ((uintptr_t)ss & 15))
    return GEOBO_E_ALIGN;
  const int64_t n2 = n / 2;
  hipLaunchKernelGGL(sumsq_accum_kernel, dim3((unsigned)((n2 + 255) / 256), (unsigned)slots), dim3(256), 0, (hipStream_t)stream, rows, n2, a,
                     lda, b, ldb, slots, ss, ld_ss);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_lamdot_z(int64_t batch, int planes, int px, int nz, const double* D, const double* lam, double* out, void* stream) {
  if (!D || !lam || !out) return GEOBO_E_ARG;
  if (batch <= 0) return GEOBO_OK;
  if (planes <= 0 || px <= 0 || nz <= 0) return GEOBO_E_ARG;
  if ((nz & 15) || ((uintptr_t)D & 15) || ((uintptr_t)lam & 15)) return GEOBO_E_ALIGN;
  const int64_t nrows = batch * px;
  int64_t nb = (nrows + 31) / 32;
  if (nb > 256 * 64) nb = 256 * 64;
  hipLaunchKernelGGL(lamdot_z_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, nrows, planes, px, nz, D, lam, out);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
