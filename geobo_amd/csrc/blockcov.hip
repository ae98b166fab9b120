// blockcov.hip -- block-support posterior statistics: products of box sums of three row tiles.
//
//   geobo_block_cov:  C6[B][ab] (+)= sum_{r < R} s_a[r, B] s_b[r, B],   s_a[r, B] = sum_{v in B} V_a[r, v],   ab = 00, 01, 02, 11, 12, 22
//
// for the blocks B that tile the (ny, nx, nz) grid from the origin in boxes of (by, bx, bz) voxels (partial at the far edges).  The
// three tiles are rows of V_a = (L^-1 A3 K)[:, block a], voxel order (iy, ix, iz): a z-column of the grid is one contiguous segment
// of nz doubles.  A streaming reduction: every element of the three tiles is read once, the roof is that read.
//
// Work item of ONE WAVE: (unit, slice).  A unit is a block column (jy, jx) cut along z into chunks of whole blocks, at most 128
// elements and 128 blocks each (one block per chunk from bz > 64 and where one block spans nz); a slice is RS consecutive rows, RS
// from the unit's size alone (32 rows for single voxels, down to 1 for units of 2048 elements and more, so that a handful of
// huge blocks still gives R waves).  Per row the wave walks the unit's z-segments: lane l owns the elements 2l, 2l + 1 (+ 128 t)
// of the chunk and sums them over the segments in registers (one 16-byte load per tile and segment where the address allows, two
// 8-byte loads where nz is odd or the row starts at an odd element); the sums along z within a box follow through the wave's own
// LDS rows (lane j adds the entries of blocks 2j, 2j + 1 in ascending order) or, with one block per chunk, by a butterfly over
// the lanes; then six FMAs per block.  The rows of a slice are added in ascending order, every (slice, block) leaves six partial
// sums in ws and the finish kernel adds the slices in slice order and then the old value when accumulating: no atomics, bitwise
// reproducible, and nothing of ws is read that this call did not write.  Waves never wait for each other: no workgroup barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "geobo_hip.h"

typedef double v2d __attribute__((ext_vector_type(2)));

namespace {

constexpr int ZC = 128;           // elements of a chunk held by one pass of the lanes (2 per lane)
constexpr int RS_MAX = 32;        // rows per slice for the smallest units
constexpr int64_t UNIT_ELEMS = 2048;    // a slice holds about this many elements of one tile

struct Shape {
  int ny, nx, nz, by, bx, bz;
  int nby, nbx, nbz;
  int kb;                         // blocks per chunk
  int nch;                        // chunks per block column
  int rs;                         // rows per slice
  int64_t nunits, nblocks, nsl;
};

bool shape_of(int64_t R, int ny, int nx, int nz, int by, int bx, int bz, Shape& s) {
  if (R < 0 || ny < 1 || nx < 1 || nz < 1 || by < 1 || bx < 1 || bz < 1 || by > ny || bx > nx || bz > nz) return false;
  if ((int64_t)ny * nx > INT32_MAX / nz) return false;        // N fits an int: block and unit counts do too
  s.ny = ny; s.nx = nx; s.nz = nz; s.by = by; s.bx = bx; s.bz = bz;
  s.nby = (ny + by - 1) / by; s.nbx = (nx + bx - 1) / bx; s.nbz = (nz + bz - 1) / bz;
  s.kb = bz > ZC / 2 ? 1 : ZC / bz;
  if (s.kb > s.nbz) s.kb = s.nbz;                               // (one block along z: the butterfly, whatever its size)
  s.nch = (s.nbz + s.kb - 1) / s.kb;
  const int64_t zlen = s.kb == 1 ? bz : (int64_t)s.kb * bz;
  const int64_t w = (int64_t)by * bx * (zlen < nz ? zlen : nz);
  const int64_t rs = UNIT_ELEMS / w;
  s.rs = (int)(rs < 1 ? 1 : rs > RS_MAX ? RS_MAX : rs);
  s.nunits = (int64_t)s.nby * s.nbx * s.nch;
  s.nblocks = (int64_t)s.nby * s.nbx * s.nbz;
  s.nsl = (R + s.rs - 1) / s.rs;
  return true;
}

struct Args {
  Shape s;
  int64_t R, ldv;
  const double* V[3];
  int vec;                        // the three tiles start at 16-byte addresses
  double* part;                   // [slice][block][6]
};

__device__ __forceinline__ void wave_sync() {    // LDS traffic of one wave: in order on the hardware, fenced for the compiler
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool ONE>   // ONE: one block per chunk (lane butterfly); else up to 128 blocks per chunk of at most 128 elements (LDS)
__global__ void __launch_bounds__(256) block_cov_kernel(const Args a) {
  __shared__ double zs[4][3][ZC];
  const Shape& s = a.s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t task = (int64_t)blockIdx.x * 4 + wave;
  if (task >= s.nunits * s.nsl) return;
  const int64_t sl = task / s.nunits;
  int64_t u = task - sl * s.nunits;
  const int c = (int)(u % s.nch);
  u /= s.nch;
  const int jx = (int)(u % s.nbx), jy = (int)(u / s.nbx);
  const int y0 = jy * s.by, x0 = jx * s.bx;
  const int my = min(s.by, s.ny - y0), mx = min(s.bx, s.nx - x0);
  const int zb0 = c * s.kb;
  const int z_lo = zb0 * s.bz;
  const int zlen = min(s.nz, (zb0 + s.kb) * s.bz) - z_lo;     // (ONE: the block's own extent, which may pass 128)
  const int kb = min(s.kb, s.nbz - zb0);
  const int64_t r0 = sl * s.rs, r1 = min(a.R, r0 + s.rs);
  double (*z)[ZC] = zs[wave];

  double acc[2][6];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[q][i] = 0.0;

  for (int64_t r = r0; r < r1; ++r) {
    const int64_t row = r * a.ldv;
    // a 16-byte load needs an even element offset: all segments of the row share its parity when nz is even
    const bool vec = a.vec && !(s.nz & 1) && !((row + z_lo) & 1);
    double x[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
    for (int sy = 0; sy < my; ++sy) {
      const int64_t seg0 = row + ((int64_t)(y0 + sy) * s.nx + x0) * s.nz + z_lo;
      if (vec) {
#pragma unroll 4
        for (int sx = 0; sx < mx; ++sx) {
          const int64_t seg = seg0 + (int64_t)sx * s.nz;
          for (int e = 2 * lane; e < zlen; e += ZC) {
            if (e + 1 < zlen) {
#pragma unroll
              for (int t = 0; t < 3; ++t) {
                const v2d v = *reinterpret_cast<const v2d*>(a.V[t] + seg + e);
                x[t][0] += v.x;
                x[t][1] += v.y;
              }
            } else {                                   // the last element of the chunk alone: its neighbour is not ours to read
#pragma unroll
              for (int t = 0; t < 3; ++t) x[t][0] += a.V[t][seg + e];
            }
          }
        }
      } else {
#pragma unroll 4
        for (int sx = 0; sx < mx; ++sx) {
          const int64_t seg = seg0 + (int64_t)sx * s.nz;
          for (int e = 2 * lane; e < zlen; e += ZC) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
              x[t][0] += a.V[t][seg + e];
              if (e + 1 < zlen) x[t][1] += a.V[t][seg + e + 1];
            }
          }
        }
      }
    }
    if (ONE) {
      double b[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        b[t] = x[t][0] + x[t][1];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) b[t] += __shfl_xor(b[t], off, 64);
      }
      acc[0][0] = __builtin_fma(b[0], b[0], acc[0][0]);
      acc[0][1] = __builtin_fma(b[0], b[1], acc[0][1]);
      acc[0][2] = __builtin_fma(b[0], b[2], acc[0][2]);
      acc[0][3] = __builtin_fma(b[1], b[1], acc[0][3]);
      acc[0][4] = __builtin_fma(b[1], b[2], acc[0][4]);
      acc[0][5] = __builtin_fma(b[2], b[2], acc[0][5]);
    } else {
#pragma unroll
      for (int t = 0; t < 3; ++t) *reinterpret_cast<v2d*>(&z[t][2 * lane]) = v2d{x[t][0], x[t][1]};
      wave_sync();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = 2 * lane + q;
        if (j < kb) {
          const int lo = j * s.bz, hi = min(lo + s.bz, zlen);
          double b[3] = {0.0, 0.0, 0.0};
          for (int i = lo; i < hi; ++i) {
#pragma unroll
            for (int t = 0; t < 3; ++t) b[t] += z[t][i];
          }
          acc[q][0] = __builtin_fma(b[0], b[0], acc[q][0]);
          acc[q][1] = __builtin_fma(b[0], b[1], acc[q][1]);
          acc[q][2] = __builtin_fma(b[0], b[2], acc[q][2]);
          acc[q][3] = __builtin_fma(b[1], b[1], acc[q][3]);
          acc[q][4] = __builtin_fma(b[1], b[2], acc[q][4]);
          acc[q][5] = __builtin_fma(b[2], b[2], acc[q][5]);
        }
      }
      wave_sync();                                     // the next row overwrites what the neighbours have just read
    }
  }

  const int64_t blk0 = ((int64_t)jy * s.nbx + jx) * s.nbz + zb0;
  double* p = a.part + (sl * s.nblocks + blk0) * 6;
  if (ONE) {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 6; ++i) p[i] = acc[0][i];
    }
  } else {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = 2 * lane + q;
      if (j < kb) {
#pragma unroll
        for (int i = 0; i < 6; ++i) p[(int64_t)j * 6 + i] = acc[q][i];
      }
    }
  }
}

// the slices in ascending row order, then the old value
__global__ void __launch_bounds__(256) block_cov_finish_kernel(const double* __restrict__ part, int64_t n6, int64_t nsl, int accumulate,
                                                               double* __restrict__ C6) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n6) return;
  double v = 0.0;
  for (int64_t sl = 0; sl < nsl; ++sl) v += part[sl * n6 + i];
  C6[i] = accumulate ? C6[i] + v : v;
}

size_t ws_bytes_of(const Shape& s) {
  const size_t b = (size_t)s.nsl * (size_t)s.nblocks * 6 * sizeof(double);     // (a multiple of 48, so of 16)
  return b < 16 ? 16 : b;
}

}  // namespace

extern "C" size_t geobo_block_cov_ws_bytes(int64_t R, int ny, int nx, int nz, int by, int bx, int bz) {
  Shape s;
  if (!shape_of(R, ny, nx, nz, by, bx, bz, s)) return 0;
  return ws_bytes_of(s);
}

extern "C" int geobo_block_cov(int64_t R, const double* V0, const double* V1, const double* V2, int64_t ldv, int ny, int nx, int nz,
                               int by, int bx, int bz, int accumulate, double* C6, void* ws, size_t ws_bytes, void* stream) {
  // every check before any device access
  Shape s;
  if (!V0 || !V1 || !V2 || !C6 || !ws) return GEOBO_E_ARG;
  if (!shape_of(R, ny, nx, nz, by, bx, bz, s)) return GEOBO_E_ARG;
  if (ldv < (int64_t)ny * nx * nz || ws_bytes < ws_bytes_of(s)) return GEOBO_E_ARG;
  if (R > 0 && ldv > INT64_MAX / R) return GEOBO_E_ARG;
  const int64_t wgs = (s.nunits * s.nsl + 3) / 4;
  if (wgs > INT32_MAX) return GEOBO_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n6 = s.nblocks * 6;
  if (R == 0) {
    if (accumulate) return GEOBO_OK;
    return hipMemsetAsync(C6, 0, (size_t)n6 * sizeof(double), st) == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
  }
  Args a{};
  a.s = s; a.R = R; a.ldv = ldv;
  a.V[0] = V0; a.V[1] = V1; a.V[2] = V2;
  a.vec = !(((uintptr_t)V0 | (uintptr_t)V1 | (uintptr_t)V2) & 15);
  a.part = (double*)ws;
  if (s.kb == 1)
    hipLaunchKernelGGL(block_cov_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(block_cov_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, st, a);
  hipLaunchKernelGGL(block_cov_finish_kernel, dim3((unsigned)((n6 + 255) / 256)), dim3(256), 0, st, (const double*)ws, n6, s.nsl,
                     accumulate ? 1 : 0, C6);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
