// information.hip -- per-set blocks of the drill-property posterior covariance and their information gain.
//
//   geobo_set_gram:    G[c] (+)= V(:, P_c)^T V(:, P_c)   for C voxel sets P_c of k <= 128 entries (one tile of rows of V_d at a time)
//   geobo_set_logdet:  S_c = (Kpp - G[c]) / sigma^2 + I, Cholesky in LDS:  1/2 log det S_c, 1^T (Kpp - G[c]) 1, trace (Kpp - G[c])
//
// set_gram: one workgroup (4 waves) per set.  The rows of the tile are walked in chunks of 16; each chunk's gathered 16 x k block is
// staged through LDS (double-buffered, next chunk prefetched into registers, one barrier per chunk) and every wave multiplies its
// share of the lower 16 x 16 tiles of the k x k result on the fp64 matrix pipe (v_mfma_f64_16x16x4).  A set whose entries are one
// contiguous run of columns (a vertical hole: 64 x 8 B) is read as whole row segments, others are gathered through the index table.
// Rows are consumed in groups of 4 per MFMA in row order, and the accumulators start from G itself when accumulating: a split of the
// same rows into tiles at multiples of 4 rows gives the same bits.  No atomics.
// f64 MFMA layout: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15], D: col = lane&15, row = (lane>>4) + 4 reg.
//
// set_logdet: one workgroup per set, S_c in LDS (k = 128: 132 KiB), unblocked right-looking Cholesky with two barriers per column.
// Entries whose index is negative (padding) or whose voxel is marked in `observed` become unit rows / columns and are left out of the
// two sums.  A pivot that is not positive gives status 1 + pivot and NaN outputs for that set only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "geobo_hip.h"

typedef double v4d __attribute__((ext_vector_type(4)));

namespace {

constexpr int KMAX = 128;
constexpr int RC = 16;            // rows per chunk
constexpr int LDX = KMAX + 8;     // LDS row stride of a chunk (doubles)
constexpr int TPW = 9;            // lower 16 x 16 tiles per wave: 8 x 9 / 2 = 36 tiles over 4 waves

struct GramArgs {
  const int32_t* idx; int k;
  const double* V; int64_t ldv; int64_t R; int64_t ncols;
  int accumulate;
  double* G;
};

__device__ __forceinline__ void tile_of(int t, int& ti, int& tj) {   // lower tiles in row order: t = ti (ti + 1) / 2 + tj
  int b = 0;
  while ((b + 1) * (b + 2) / 2 <= t) ++b;
  ti = b; tj = t - b * (b + 1) / 2;
}

// the 16 x kp chunk of rows r0.. into registers: element e = tid + 256 q  ->  (row e / kp, column e % kp)
__device__ __forceinline__ void load_chunk(const GramArgs& a, const int* sidx, int kp, int64_t base, int64_t r0, int tid, double (&reg)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = tid + 256 * q;
    const int row = e / kp, col = e - row * kp;
    double v = 0.0;
    const int64_t r = r0 + row;
    if (row < RC && col < a.k && r < a.R) {
      if (base >= 0) {
        v = a.V[r * a.ldv + base + col];                // contiguous run: whole row segments
      } else {
        const int c = sidx[col];
        if (c >= 0) v = a.V[r * a.ldv + c];             // gathered; padding entries (c < 0) read nothing
      }
    }
    reg[q] = v;
  }
}

__device__ __forceinline__ void store_chunk(double* X, int kp, int tid, const double (&reg)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = tid + 256 * q;
    const int row = e / kp, col = e - row * kp;
    if (row < RC) X[row * LDX + col] = reg[q];
  }
}

__global__ void __launch_bounds__(256) set_gram_kernel(const GramArgs a) {
  __shared__ double X[2][RC * LDX];
  __shared__ int sidx[KMAX];
  __shared__ int contiguous;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = blockIdx.x;
  const int k = a.k, kt = (k + 15) >> 4, kp = kt * 16, ntiles = kt * (kt + 1) / 2;
  const int32_t* ic = a.idx + c * k;
  if (tid == 0) contiguous = 1;
  __syncthreads();
  if (tid < KMAX) {
    int v = -1;
    if (tid < k) {
      v = ic[tid];
      if (v < 0 || (int64_t)v >= a.ncols) v = -1;                  // out-of-range entries count as padding
    }
    sidx[tid] = v;
  }
  __syncthreads();
  if (tid < k && (sidx[tid] < 0 || sidx[tid] != sidx[0] + tid)) contiguous = 0;   // (benign race: every writer stores 0)
  __syncthreads();
  const int64_t base = contiguous ? (int64_t)sidx[0] : -1;

  double* Gc = a.G + c * (int64_t)k * k;
  v4d acc[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    acc[q] = v4d{0, 0, 0, 0};
    const int t = wave + 4 * q;
    if (a.accumulate && t < ntiles) {
      int ti, tj;
      tile_of(t, ti, tj);
      const int j = tj * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * 16 + (lane >> 4) + 4 * r;
        if (i < k && j < k) acc[q][r] = Gc[(int64_t)i * k + j];
      }
    }
  }

  const int64_t nch = (a.R + RC - 1) / RC;
  double reg[8];
  if (nch > 0) load_chunk(a, sidx, kp, base, 0, tid, reg);
  for (int64_t ch = 0; ch < nch; ++ch) {
    const int st = (int)(ch & 1);
    store_chunk(X[st], kp, tid, reg);
    __syncthreads();
    if (ch + 1 < nch) load_chunk(a, sidx, kp, base, (ch + 1) * RC, tid, reg);
    const double* Xs = X[st];
#pragma unroll
    for (int s = 0; s < RC / 4; ++s) {
      const int kk = 4 * s + (lane >> 4);
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const int t = wave + 4 * q;
        if (t < ntiles) {
          int ti, tj;
          tile_of(t, ti, tj);
          const double av = Xs[kk * LDX + ti * 16 + (lane & 15)];
          const double bv = Xs[kk * LDX + tj * 16 + (lane & 15)];
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
        }
      }
    }
  }

  // lower tiles out, mirrored: diagonal tiles write their lower half (i >= j) to both places
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const int t = wave + 4 * q;
    if (t >= ntiles) continue;
    int ti, tj;
    tile_of(t, ti, tj);
    const int j = tj * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ti * 16 + (lane >> 4) + 4 * r;
      if (i < k && j < k && i >= j) {
        Gc[(int64_t)i * k + j] = acc[q][r];
        Gc[(int64_t)j * k + i] = acc[q][r];
      }
    }
  }
}

struct LogdetArgs {
  int k; int64_t C;
  const double* G; const double* Kpp; int64_t kpp_stride;
  double s2;
  const int32_t* idx; const uint8_t* observed; int64_t n_obs;
  double* out; int* status;
};

template <int KM>
__global__ void __launch_bounds__(256) set_logdet_kernel(const LogdetArgs a) {
  constexpr int LS = KM + 1;
  __shared__ double S[KM * LS];
  __shared__ double col[KM];
  __shared__ int live[KM];
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const int k = a.k;
  const int64_t c = blockIdx.x;
  if (tid < KM) {
    int v = 0;
    if (tid < k) {
      const int32_t e = a.idx[c * k + tid];
      v = e >= 0 && (int64_t)e < a.n_obs;
      if (v && a.observed && a.observed[e]) v = 0;
    }
    live[tid] = v;
  }
  __syncthreads();
  const double* Gc = a.G + c * (int64_t)k * k;
  const double* Kc = a.Kpp + c * a.kpp_stride;
  double ps = 0.0, ts = 0.0;
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    const double d = Kc[e] - Gc[e];
    const bool on = live[i] && live[j];
    if (on) {
      ps += d;
      if (i == j) ts += d;
    }
    S[i * LS + j] = on ? d / a.s2 + (i == j ? 1.0 : 0.0) : (i == j ? 1.0 : 0.0);
  }
  red[0][tid] = ps;
  red[1][tid] = ts;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {             // fixed-order tree
    if (tid < h) {
      red[0][tid] += red[0][tid + h];
      red[1][tid] += red[1][tid + h];
    }
    __syncthreads();
  }
  const double path = red[0][0], trace = red[1][0];

  double logsum = 0.0;
  int fail = -1;
  for (int j = 0; j < k; ++j) {
    const double d = S[j * LS + j];                // every thread reads the same pivot: the branch below is uniform
    if (!(d > 0.0) || !isfinite(d)) {
      fail = j;
      break;
    }
    logsum += log(d);
    const double rd = 1.0 / sqrt(d);
    for (int i = j + 1 + tid; i < k; i += 256) col[i] = S[i * LS + j] * rd;
    __syncthreads();
    const int w = k - j - 1;
    for (int e = tid; e < w * w; e += 256) {
      const int ii = e / w, ll = e - ii * w;
      if (ll <= ii) {
        const int i = j + 1 + ii, l = j + 1 + ll;
        S[i * LS + l] -= col[i] * col[l];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double nan = __builtin_nan("");
    const bool ok = fail < 0;
    a.out[c] = ok ? 0.5 * logsum : nan;
    a.out[a.C + c] = ok ? path : nan;
    a.out[2 * a.C + c] = ok ? trace : nan;
    a.status[c] = ok ? 0 : 1 + fail;
  }
}

}  // namespace

extern "C" int geobo_set_gram(int64_t C, int k, const int32_t* idx, int64_t R, const double* V, int64_t ldv, int64_t ncols,
                              int accumulate, double* G, void* stream) {
  // every check before any device access
  if (!idx || !G || (R > 0 && !V)) return GEOBO_E_ARG;
  if (C < 0 || C > INT32_MAX || k < 1 || k > KMAX || R < 0 || ncols < 0 || ldv < ncols) return GEOBO_E_ARG;
  if (C == 0) return GEOBO_OK;
  GramArgs a{};
  a.idx = idx; a.k = k; a.V = V; a.ldv = ldv; a.R = R; a.ncols = ncols; a.accumulate = accumulate ? 1 : 0; a.G = G;
  hipLaunchKernelGGL(set_gram_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_set_logdet(int64_t C, int k, const double* G, const double* Kpp, int64_t kpp_stride, double sigma2,
                                const int32_t* idx, const uint8_t* observed, int64_t n_obs, double* out, int* status, void* stream) {
  if (!G || !Kpp || !idx || !out || !status) return GEOBO_E_ARG;
  if (C < 0 || C > INT32_MAX || k < 1 || k > KMAX || n_obs < 0) return GEOBO_E_ARG;
  if (kpp_stride != 0 && kpp_stride < (int64_t)k * k) return GEOBO_E_ARG;
  if (!(sigma2 > 0.0) || !isfinite(sigma2)) return GEOBO_E_ARG;
  if (C == 0) return GEOBO_OK;
  LogdetArgs a{};
  a.k = k; a.C = C; a.G = G; a.Kpp = Kpp; a.kpp_stride = kpp_stride; a.s2 = sigma2;
  a.idx = idx; a.observed = observed; a.n_obs = n_obs; a.out = out; a.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (k <= 64)
    hipLaunchKernelGGL(set_logdet_kernel<64>, dim3((unsigned)C), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(set_logdet_kernel<128>, dim3((unsigned)C), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
