// kinv_dot.hip -- block sums of <K^-1 - alpha alpha^T, G_t> for the exact log-likelihood gradient, K^-1 never stored.
//
//   P = Linv^T Linv  (= K^-1, Linv lower triangular)           lower 128 x 128 tiles only, fp64 MFMA (v_mfma_f64_16x16x4)
//   S = P - alpha alpha^T                                       in the epilogue
//   out[t][a][b] = sum_{i in seg a, j in seg b} S_ij G_t[i][j]  G_t symmetric, read from its LOWER triangle only
//
// Tile (bi >= bj) is a TN product over the rows k >= 128 bi of Linv (the rows above are zero in both operands): both operands are
// row runs of Linv, so every k step loads two contiguous 1 KiB runs.  Workgroup = 4 waves (2 x 2), each a 64 x 64 block as a 4 x 4
// grid of 16 x 16 f64 accumulators; k walked in chunks of 16 rows, double-buffered in LDS (one barrier per chunk), next chunk
// prefetched into registers while the matrix pipe works on the current one.  f64 MFMA layout: A[i = lane&15][k = lane>>4],
// B[k = lane>>4][j = lane&15], D: col = lane&15, row = (lane>>4) + 4 reg.
// Epilogue: strictly-lower elements count twice (the upper half by symmetry), diagonal ones once; each product goes to its pair of
// row segments (a >= b).  The sums leave each workgroup through a fixed-order wave / LDS tree into a per-tile workspace slot and
// are added up tile by tile in a fixed order by the finish kernel: no atomics, bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "geobo_hip.h"

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

namespace {

constexpr int KT = 128;       // output tile edge
constexpr int KC = 16;        // rows of Linv per chunk
constexpr int LS = KT + 16;   // LDS row stride (doubles): rows k and k+1 land 128 bytes apart -> a wave's 4 k rows in 2 passes
constexpr int NPAIR = 6;      // segment pairs (a >= b): (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)

struct KinvArgs {
  const double* L; int64_t ldl;
  const double* alpha;
  const double* G[4]; int64_t ldg;
  int64_t seg[6];             // [s0, e0, s1, e1, s2, e2]
  int64_t m; int nb;
  double* part;               // [tile][T][NPAIR]
};

__device__ __forceinline__ void tile_of(int t, int& bi, int& bj) {   // lower tiles in row order: t = bi (bi + 1) / 2 + bj
  int b = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((b + 1) * (b + 2) / 2 <= t) ++b;
  while (b * (b + 1) / 2 > t) --b;
  bi = b; bj = t - b * (b + 1) / 2;
}

__device__ __forceinline__ int seg_of(const KinvArgs& a, int64_t i) {
  if (i >= a.seg[0] && i < a.seg[1]) return 0;
  if (i >= a.seg[2] && i < a.seg[3]) return 1;
  if (i >= a.seg[4] && i < a.seg[5]) return 2;
  return -1;
}

// 16 x 128 run of Linv rows k0.., columns c0.. into registers (8 doubles per thread), zero above the diagonal (k < column)
__device__ __forceinline__ void load_chunk(const KinvArgs& a, int64_t k0, int64_t c0, int tid, v2d (&r)[4]) {
  const int row = tid >> 4, col = (tid & 15) * 8;
  const int64_t k = k0 + row;
  const double* src = a.L + k * a.ldl + c0 + col;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v2d v = *reinterpret_cast<const v2d*>(src + 2 * q);
    const int64_t c = c0 + col + 2 * q;
    if (k < c) v.x = 0.0;
    if (k < c + 1) v.y = 0.0;
    r[q] = v;
  }
}

__device__ __forceinline__ void store_chunk(double* lds, int tid, const v2d (&r)[4]) {
  const int row = tid >> 4, col = (tid & 15) * 8;
#pragma unroll
  for (int q = 0; q < 4; ++q) *reinterpret_cast<v2d*>(lds + row * LS + col + 2 * q) = r[q];
}

template <int T>
__global__ void __launch_bounds__(256, 2) kinv_dot_kernel(const KinvArgs a) {
  __shared__ double lds[2][2][KC * LS];   // [stage][operand i / j][k][column]
  __shared__ double red[4][T * NPAIR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int bi, bj;
  tile_of(blockIdx.x, bi, bj);
  const bool diag = bi == bj;
  const int64_t I0 = (int64_t)bi * KT, J0 = (int64_t)bj * KT;
  const bool active = !(diag && wn > wm);          // the upper 64 x 64 block of a diagonal tile is not needed
  v4d acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = v4d{0, 0, 0, 0};

  const int64_t nchunks = (a.m - I0) / KC;
  v2d ri[4], rj[4];
  load_chunk(a, I0, I0, tid, ri);
  if (!diag) load_chunk(a, I0, J0, tid, rj);
  for (int64_t c = 0; c < nchunks; ++c) {
    const int st = (int)(c & 1);
    store_chunk(lds[st][0], tid, ri);
    if (!diag) store_chunk(lds[st][1], tid, rj);
    __syncthreads();
    if (c + 1 < nchunks) {
      const int64_t k0 = I0 + (c + 1) * KC;
      load_chunk(a, k0, I0, tid, ri);
      if (!diag) load_chunk(a, k0, J0, tid, rj);
    }
    if (active) {
      const double* Xi = lds[st][0];
      const double* Xj = diag ? lds[st][0] : lds[st][1];
#pragma unroll
      for (int s = 0; s < KC / 4; ++s) {
        const int k = 4 * s + (lane >> 4);
        double av[4], bv[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) av[x] = Xi[k * LS + wm * 64 + x * 16 + (lane & 15)];
#pragma unroll
        for (int y = 0; y < 4; ++y) bv[y] = Xj[k * LS + wn * 64 + y * 16 + (lane & 15)];
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[y], acc[x][y], 0, 0, 0);
      }
    }
  }

  // epilogue: S = P - alpha alpha^T against the G_t tiles, summed per segment pair
  double sums[T][NPAIR];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int q = 0; q < NPAIR; ++q) sums[t][q] = 0.0;
  if (active) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int64_t j = J0 + wn * 64 + y * 16 + (lane & 15);
      const int sj = seg_of(a, j);
      const double aj = a.alpha[j];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t i = I0 + wm * 64 + x * 16 + (lane >> 4) + 4 * r;
          const int si = seg_of(a, i);
          if (i < j || si < 0 || sj < 0) continue;
          const double wgt = (i == j) ? 1.0 : 2.0;
          const double sv = wgt * (acc[x][y][r] - a.alpha[i] * aj);
          const int pq = si * (si + 1) / 2 + sj;        // si >= sj: segments are ordered and i >= j
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const double g = a.G[t][i * a.ldg + j];
#pragma unroll
            for (int q = 0; q < NPAIR; ++q)
              if (q == pq) sums[t][q] = __builtin_fma(sv, g, sums[t][q]);
          }
        }
      }
    }
  }
  // fixed-order reduction: butterfly over the wave, then the four waves in order
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int q = 0; q < NPAIR; ++q) {
      double v = sums[t][q];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) red[wave][t * NPAIR + q] = v;
    }
  __syncthreads();
  if (tid < T * NPAIR) {
    const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    a.part[(int64_t)blockIdx.x * T * NPAIR + tid] = v;
  }
}

// out[t][a][b] (3 x 3, symmetric) = sum over tiles in index order of the pair sums
__global__ void kinv_dot_finish_kernel(const double* __restrict__ part, int ntiles, int T, double* __restrict__ out) {
  const int idx = threadIdx.x;
  if (idx >= T * NPAIR) return;
  double s = 0.0;
  for (int b = 0; b < ntiles; ++b) s += part[(int64_t)b * T * NPAIR + idx];
  const int t = idx / NPAIR, q = idx % NPAIR;
  const int pa[NPAIR] = {0, 1, 1, 2, 2, 2}, pb[NPAIR] = {0, 0, 1, 0, 1, 2};
  out[t * 9 + pa[q] * 3 + pb[q]] = s;
  out[t * 9 + pb[q] * 3 + pa[q]] = s;
}

int64_t ntiles_of(int64_t m) {
  const int64_t nb = m / KT;
  return nb * (nb + 1) / 2;
}

}  // namespace

extern "C" size_t geobo_kinv_dot_ws_bytes(int64_t m, int T) {
  if (m <= 0 || m % GEOBO_PAD_M || T < 1 || T > 4) return 0;
  return (size_t)ntiles_of(m) * T * NPAIR * sizeof(double);
}

extern "C" int geobo_kinv_dot(int64_t m, const double* Linv, int64_t ldl, const double* alpha, int T, const double* const* G,
                              int64_t ldg, const int64_t* seg, double* out, void* ws, size_t ws_bytes, void* stream) {
  // every check before any device access
  if (!Linv || !alpha || !G || !seg || !out || !ws) return GEOBO_E_ARG;
  if (m <= 0 || m % GEOBO_PAD_M || T < 1 || T > 4 || ldl < m || ldg < m || (ldl & 1)) return GEOBO_E_ARG;
  if ((uintptr_t)Linv & 15) return GEOBO_E_ARG;     // 16-byte loads of column pairs
  for (int t = 0; t < T; ++t)
    if (!G[t]) return GEOBO_E_ARG;
  int64_t prev = 0;
  for (int s = 0; s < 3; ++s) {
    const int64_t s0 = seg[2 * s], s1 = seg[2 * s + 1];
    if (s0 < prev || s0 % GEOBO_PAD_M || s1 < s0 || s1 > m) return GEOBO_E_ARG;
    prev = s1;
  }
  if (ws_bytes < geobo_kinv_dot_ws_bytes(m, T)) return GEOBO_E_ARG;
  KinvArgs a{};
  a.L = Linv; a.ldl = ldl; a.alpha = alpha; a.ldg = ldg; a.m = m; a.nb = (int)(m / KT);
  for (int t = 0; t < 4; ++t) a.G[t] = t < T ? G[t] : nullptr;
  for (int s = 0; s < 6; ++s) a.seg[s] = seg[s];
  a.part = (double*)ws;
  const int64_t nt = ntiles_of(m);
  hipStream_t st = (hipStream_t)stream;
  switch (T) {
    case 1: hipLaunchKernelGGL(kinv_dot_kernel<1>, dim3((unsigned)nt), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL(kinv_dot_kernel<2>, dim3((unsigned)nt), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(kinv_dot_kernel<3>, dim3((unsigned)nt), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(kinv_dot_kernel<4>, dim3((unsigned)nt), dim3(256), 0, st, a); break;
  }
  hipLaunchKernelGGL(kinv_dot_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, (int)nt, T, out);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
