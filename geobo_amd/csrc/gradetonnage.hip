// gradetonnage.hip -- reductions over posterior realisations for grade-tonnage curves.
//
//   geobo_box_means:    G[s][a][B] = (1 / n_B) sum_{v in B} F[s][a][v],   count[B] = n_B
//   geobo_cutoff_stats: cnt[s][c] = sum_v w[v] [v passes c in sample s],   sum[s][c] = sum_v w[v] F[s][p][v] [..],   hits[c][v] += [..]
//
// for S realisations F[s][a][v] (a = 0, 1, 2; sample and property strides given), the boxes of blockcov.hip's partition and C sorted
// thresholds.  Both are streams: every element is read once.
//
// box means: ONE LANE per output (s, a, B), B fastest, so the lanes of a wave read neighbouring runs of the same z-columns and
// write consecutive doubles.  A lane adds the z-run of a segment in ascending z, then the segments in ascending (iy, ix); the first
// term starts each sum (no 0.0 + x, which would lose the sign of -0.0), so a box of one voxel returns its input bit for bit.
//
// cutoff statistics: a workgroup of 256 lanes owns a CHUNK of 512 consecutive elements, lane i the elements 2i, 2i + 1 (one 16-byte
// load per sample and property that is read where the address allows, two 8-byte loads otherwise), and walks the S samples.  Per
// sample a lane finds the BIN of each of its elements -- how many thresholds lie at or below the value, by bisection over the
// thresholds in LDS, 0 for an element that fails the mask, a lower bound or is NaN -- and leaves (bin, w, w x) in the chunk's LDS
// image.  "At or above cutoff c" is "bin > c": lane (c, part) = (i & 31, i >> 5) adds the entries 64 part .. 64 part + 63 with
// bin > c in ascending order (broadcast reads), lane c then adds the eight parts in ascending order and writes one partial count
// and sum per (sample, chunk, c) into ws; the finish kernel adds the chunks in ascending order.  The order is fixed by n alone:
// no floating-point atomics, bitwise reproducible, independent of S and of what ws held.  hits: a lane keeps the histogram of its
// two elements' bins over the samples of the launch in a lane-private LDS column (16-bit counters, at most 32768 samples a launch),
// and adds its suffix sums to hits[c][v] once at the end: no atomics, each hits entry has one owner.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "cutoff_set.h"
#include "geobo_hip.h"

typedef double v2d __attribute__((ext_vector_type(2)));

namespace {

constexpr int WG = 256;             // lanes of a cutoff workgroup
constexpr int CHUNK = 2 * WG;       // elements of a chunk
constexpr int64_t S_LAUNCH = 32768; // samples per launch (16-bit histogram counters)

// ---- box means -----------------------------------------------------------------------------------------------------------------
struct BoxShape {
  int ny, nx, nz, by, bx, bz, nby, nbx, nbz;
  int64_t N, nblocks;
};

bool box_shape_of(int ny, int nx, int nz, int by, int bx, int bz, BoxShape& s) {
  if (ny < 1 || nx < 1 || nz < 1 || by < 1 || bx < 1 || bz < 1 || by > ny || bx > nx || bz > nz) return false;
  if ((int64_t)ny * nx > INT32_MAX / nz) return false;        // N fits an int: block counts do too
  s.ny = ny; s.nx = nx; s.nz = nz; s.by = by; s.bx = bx; s.bz = bz;
  s.nby = (ny + by - 1) / by; s.nbx = (nx + bx - 1) / bx; s.nbz = (nz + bz - 1) / bz;
  s.N = (int64_t)ny * nx * nz;
  s.nblocks = (int64_t)s.nby * s.nbx * s.nbz;
  return true;
}

__global__ void __launch_bounds__(256) box_means_kernel(const BoxShape s, int64_t S, const double* __restrict__ F, int64_t sstride,
                                                        int64_t pstride, double* __restrict__ G, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= S * 3 * s.nblocks) return;
  const int64_t B = i % s.nblocks, sa = i / s.nblocks;
  const int a = (int)(sa % 3);
  const int64_t smp = sa / 3;
  const int jz = (int)(B % s.nbz), jx = (int)((B / s.nbz) % s.nbx), jy = (int)(B / ((int64_t)s.nbz * s.nbx));
  const int y0 = jy * s.by, x0 = jx * s.bx, z0 = jz * s.bz;
  const int my = min(s.by, s.ny - y0), mx = min(s.bx, s.nx - x0), mz = min(s.bz, s.nz - z0);
  const double* f = F + smp * sstride + a * pstride;
  double total = 0.0;
  for (int sy = 0; sy < my; ++sy) {
    for (int sx = 0; sx < mx; ++sx) {
      const double* seg = f + ((int64_t)(y0 + sy) * s.nx + (x0 + sx)) * s.nz + z0;
      double run = seg[0];
      int e = 1;
      if (((uintptr_t)(seg + e) & 15) && e < mz) run += seg[e++];     // pairs from the first 16-byte address on
      for (; e + 1 < mz; e += 2) {
        const v2d v = *reinterpret_cast<const v2d*>(seg + e);
        run += v.x;
        run += v.y;
      }
      if (e < mz) run += seg[e];
      total = (sy | sx) ? total + run : run;
    }
  }
  const int nB = my * mx * mz;
  G[i] = total / (double)nB;
  if (sa == 0) count[B] = nB;
}

// ---- cutoff statistics -----------------------------------------------------------------------------------------------------------
struct CutArgs {
  const double* F;
  int64_t sstride, pstride, n, S;
  int C;
  int64_t off[3];                   // element offsets of the properties p, (p + 1) % 3, (p + 2) % 3 within a sample
  int read[3];                      // the property of that slot is read: slot 0 always, the others when their bound is > -inf
  double lo[3];                     // lower bound of that slot (slot 0: not used)
  double t[CMAX];
  const uint8_t* mask;
  const int32_t* weight;
  double* psum;                     // [sample][chunk][C]
  int64_t* pcnt;                    // [sample][chunk][C]
  uint32_t* hits;                   // [C][n], or NULL
  int64_t nchunks;
};

struct Entry {                      // 16 bytes: one element of the chunk in one sample
  int32_t bin, w;
  double wx;
};

__device__ __forceinline__ void load2(const double* base, int64_t e0, int64_t n, double& x0, double& x1) {
  const double* q = base + e0;
  x0 = 0.0; x1 = 0.0;
  if (e0 + 1 < n) {
    if (!((uintptr_t)q & 15)) {
      const v2d v = *reinterpret_cast<const v2d*>(q);
      x0 = v.x; x1 = v.y;
    } else {
      x0 = q[0]; x1 = q[1];
    }
  } else if (e0 < n) {
    x0 = q[0];
  }
}

template <bool HITS>
__global__ void __launch_bounds__(WG) cutoff_kernel(const CutArgs a) {
  __shared__ double ts[CMAX];
  __shared__ Entry ent[CHUNK];
  __shared__ double part_sum[WG / 32][CMAX];
  __shared__ int64_t part_cnt[WG / 32][CMAX];
  __shared__ uint16_t hist[HITS ? 2 * (CMAX + 1) * WG : 1];   // [element][bin][lane]: a lane touches its own column alone

  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int64_t e0 = chunk * CHUNK + 2 * tid;                 // this lane's elements e0, e0 + 1
  const int C = a.C;
  if (tid < CMAX) ts[tid] = tid < C ? a.t[tid] : 0.0;
  if (HITS) {
    for (int j = 0; j < 2 * (CMAX + 1); ++j) hist[j * WG + tid] = 0;
  }
  // what does not change from sample to sample: the mask and the weights of the two elements
  bool live[2];
  int32_t w[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    live[k] = e0 + k < a.n && (!a.mask || a.mask[e0 + k] != 0);
    w[k] = (e0 + k < a.n && a.weight) ? a.weight[e0 + k] : 1;
  }
  __syncthreads();

  const int c = tid & 31, part = tid >> 5;
  // the values of the next sample are loaded before the current one is reduced
  double nxt[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (a.read[j]) load2(a.F + a.off[j], e0, a.n, nxt[j][0], nxt[j][1]);       // (uniform: the whole grid reads the property or not)
  }
  for (int64_t s = 0; s < a.S; ++s) {
    const double x[2] = {nxt[0][0], nxt[0][1]};
    bool ok[2] = {live[0], live[1]};
#pragma unroll
    for (int j = 1; j < 3; ++j) {
      if (a.read[j]) {
        ok[0] = ok[0] && nxt[j][0] >= a.lo[j];                 // (NaN fails)
        ok[1] = ok[1] && nxt[j][1] >= a.lo[j];
      }
    }
    if (s + 1 < a.S) {
      const double* f = a.F + (s + 1) * a.sstride;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (a.read[j]) load2(f + a.off[j], e0, a.n, nxt[j][0], nxt[j][1]);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int b = 0;                                               // thresholds at or below x: ts[b - 1] <= x < ts[b]; NaN gives 0
#pragma unroll
      for (int step = CMAX; step >= 1; step >>= 1) {
        const int j = b + step;
        if (j <= C && ts[j - 1] <= x[k]) b = j;
      }
      if (!ok[k]) b = 0;
      Entry en;
      en.bin = b; en.w = w[k]; en.wx = (double)w[k] * x[k];
      ent[2 * tid + k] = en;
      if (HITS) hist[(k * (CMAX + 1) + b) * WG + tid] += 1;
    }
    __syncthreads();
    {
      const Entry* run = ent + part * 64;
      double sum = 0.0;
      int64_t cnt = 0;
#pragma unroll 16
      for (int i = 0; i < 64; ++i) {                           // (unrolled: sixteen LDS reads in flight, the adds stay in order)
        const Entry en = run[i];
        if (en.bin > c) {                                      // (an entry that does not pass is not added at all: it may be inf or NaN)
          sum += en.wx;
          cnt += en.w;
        }
      }
      part_sum[part][c] = sum;
      part_cnt[part][c] = cnt;
    }
    __syncthreads();                                           // (the next sample's entries are written after this barrier too)
    if (tid < C) {
      double sum = 0.0;
      int64_t cnt = 0;
#pragma unroll
      for (int pt = 0; pt < WG / 32; ++pt) {
        sum += part_sum[pt][tid];
        cnt += part_cnt[pt][tid];
      }
      const int64_t o = (s * a.nchunks + chunk) * C + tid;
      a.psum[o] = sum;
      a.pcnt[o] = cnt;
    }
  }

  if (HITS) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (e0 + k < a.n) {
        uint32_t above = 0;
        for (int b = C; b >= 1; --b) {                         // bin b passes the cutoffs 0 .. b - 1
          above += hist[(k * (CMAX + 1) + b) * WG + tid];
          if (above) a.hits[(int64_t)(b - 1) * a.n + e0 + k] += above;
        }
      }
    }
  }
}

// the chunks in ascending order
__global__ void __launch_bounds__(256) cutoff_finish_kernel(const double* __restrict__ psum, const int64_t* __restrict__ pcnt, int64_t S,
                                                            int64_t nchunks, int C, double* __restrict__ sum, int64_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= S * C) return;
  const int64_t s = i / C;
  const int c = (int)(i - s * C);
  double v = 0.0;
  int64_t k = 0;
#pragma unroll 16
  for (int64_t ch = 0; ch < nchunks; ++ch) {                   // (unrolled: sixteen loads in flight, the adds stay in order)
    const int64_t o = (s * nchunks + ch) * C + c;
    v += psum[o];
    k += pcnt[o];
  }
  sum[i] = v;
  cnt[i] = k;
}

bool cut_shape_ok(int64_t S, int64_t n, int C) {
  if (S < 0 || n < 1 || C < 1 || C > CMAX) return false;
  if (n > (int64_t)INT32_MAX * CHUNK / 2) return false;
  return true;
}

size_t cut_ws_bytes_of(int64_t S, int64_t n, int C) {
  const int64_t nchunks = (n + CHUNK - 1) / CHUNK;
  const int64_t per = nchunks * C * 16;                        // a double and an int64 per (chunk, c)
  const int64_t Sl = S < S_LAUNCH ? S : S_LAUNCH;              // launches reuse the workspace
  if (Sl > 0 && per > INT64_MAX / Sl) return 0;
  const size_t b = (size_t)(Sl * per);
  return b < 16 ? 16 : b;
}

}  // namespace

extern "C" int geobo_box_means(int64_t S, const double* F, int64_t sstride, int64_t pstride, int ny, int nx, int nz, int by, int bx,
                               int bz, double* G, int32_t* count, void* stream) {
  // every check before any device access
  BoxShape s;
  if (!F || !G || !count) return GEOBO_E_ARG;
  if (S < 0 || !box_shape_of(ny, nx, nz, by, bx, bz, s)) return GEOBO_E_ARG;
  if (pstride < s.N || pstride > INT64_MAX / 4 || sstride < 2 * pstride + s.N) return GEOBO_E_ARG;
  if (S > 0 && (sstride > INT64_MAX / S || 3 * s.nblocks > INT64_MAX / S)) return GEOBO_E_ARG;
  const int64_t wgs = (S * 3 * s.nblocks + 255) / 256;
  if (wgs > INT32_MAX) return GEOBO_E_ARG;
  if (S == 0) return GEOBO_OK;
  hipLaunchKernelGGL(box_means_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, s, S, F, sstride, pstride, G, count);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" size_t geobo_cutoff_stats_ws_bytes(int64_t S, int64_t n, int C) {
  if (!cut_shape_ok(S, n, C)) return 0;
  return cut_ws_bytes_of(S, n, C);
}

extern "C" int geobo_cutoff_stats(int64_t S, const double* F, int64_t sstride, int64_t pstride, int64_t n, int p, int C, const double* t,
                                  const double* lo, const uint8_t* mask, const int32_t* weight, int64_t* cnt, double* sum,
                                  uint32_t* hits, void* ws, size_t ws_bytes, void* stream) {
  // every check before any device access (t and lo are host arrays)
  CutArgs a{};
  if (!cnt || !sum || !ws || !cut_shape_ok(S, n, C)) return GEOBO_E_ARG;
  if (!cutoff_set_of(S, F, sstride, pstride, n, p, C, t, lo, mask, a)) return GEOBO_E_ARG;
  const size_t need = cut_ws_bytes_of(S, n, C);
  if (need == 0 || ws_bytes < need || ((uintptr_t)ws & 15)) return GEOBO_E_ARG;
  if (S == 0) return GEOBO_OK;

  a.pstride = pstride; a.weight = weight; a.hits = hits;
  a.nchunks = (n + CHUNK - 1) / CHUNK;
  hipStream_t st = (hipStream_t)stream;
  for (int64_t s0 = 0; s0 < S; s0 += S_LAUNCH) {              // stream order lets the launches share ws
    const int64_t Sl = S - s0 < S_LAUNCH ? S - s0 : S_LAUNCH;
    a.F = F + s0 * sstride;
    a.S = Sl;
    a.psum = (double*)ws;
    a.pcnt = (int64_t*)((double*)ws + Sl * a.nchunks * C);
    if (hits)
      hipLaunchKernelGGL(cutoff_kernel<true>, dim3((unsigned)a.nchunks), dim3(WG), 0, st, a);
    else
      hipLaunchKernelGGL(cutoff_kernel<false>, dim3((unsigned)a.nchunks), dim3(WG), 0, st, a);
    hipLaunchKernelGGL(cutoff_finish_kernel, dim3((unsigned)((Sl * C + 255) / 256)), dim3(256), 0, st, (const double*)a.psum,
                       (const int64_t*)a.pcnt, Sl, a.nchunks, C, sum + s0 * C, cnt + s0 * C);
  }
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
