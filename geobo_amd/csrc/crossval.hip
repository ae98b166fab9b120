// crossval.hip -- leave-fold-out cross-validation from the step's L^-1.
//
//   geobo_kinv_diag:  d[c] = sum_{r >= c} Linv[r,c]^2 = [K_y^-1]_cc,   alpha[c] = sum_{r >= c} Linv[r,c] u[r] = [K_y^-1 y]_c
//   geobo_set_loo:    per fold B (k <= 128 rows), G = [K_y^-1]_BB:  Cholesky G = Lg Lg^T in LDS, white = Lg^-1 alpha_B,
//                     resid = Lg^-T white = y_B - E[y_B | y_-B],  var_a = (G^-1)_aa,  log p(y_B | y_-B)
//
// kinv_diag is one pass over the lower triangle of Linv (m^2 / 2 doubles).  Tiles of 256 columns x slices of 128 rows, the first
// slice of a tile starting at the tile's diagonal; one workgroup (256 threads) per (tile, slice).  A thread owns two adjacent columns
// (one 16-byte load per row: a wave reads 1 KiB of a row) and every second row of the slice, in ascending order; the two row
// phases are added in LDS.  The strict upper triangle is never loaded: in the two slices that cross the diagonal a pair is read
// whole, as its first element alone, or not at all.  Each (tile, slice) leaves 2 x 256 partial sums in ws and the finish kernel adds
// the slices of a tile in ascending order: no atomics, bitwise reproducible, nothing of ws is read that this call did not write.
//
// set_loo: one workgroup per fold, the matrix in LDS with a padded row (k = 128: 129 KiB), as set_logdet_kernel.  Right-looking
// Cholesky that keeps the factor (the forward substitution of alpha_B rides along, one column at a time), then thread j inverts
// column j of Lg into ROW j of the unused upper triangle (X_ij at S[j][i]; the diagonal of X apart), so nothing a neighbour still
// reads is overwritten and no barrier is needed; var and resid are sums along that row, in ascending order.  Entries whose index is
// outside [0, n) are padding: unit rows / columns, NaN outputs.  A pivot that is not positive gives status 1 + pivot and NaN in
// everything of that fold alone; every thread reads the same pivot, so the branch is uniform.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "geobo_hip.h"

typedef double v2d __attribute__((ext_vector_type(2)));

namespace {

constexpr int CT = 256;       // columns per tile
constexpr int RS = 128;       // rows per slice
constexpr int KMAX = 128;

struct DiagArgs {
  const double* L; int64_t ldl;
  const double* u;
  int64_t m; int nb;          // nb = m / CT column tiles; tile t has 2 (nb - t) slices
  double* part;               // [slot][2][CT]; slots of tile t start at t (2 nb - t + 1)
};

__global__ void __launch_bounds__(256) kinv_diag_kernel(const DiagArgs a) {
  __shared__ double sd[2 * CT];
  int t = 0, s = (int)blockIdx.x;
  while (s >= 2 * (a.nb - t)) {      // (tile, slice) of this workgroup: tiles in order, their slices in row order
    s -= 2 * (a.nb - t);
    ++t;
  }
  const int tid = threadIdx.x, tx = tid & 127, ph = tid >> 7;
  const int64_t c = (int64_t)t * CT + 2 * tx;
  const int64_t r0 = (int64_t)t * CT + (int64_t)s * RS;
  const double* src = a.L + c;
  double d0 = 0.0, d1 = 0.0, a0 = 0.0, a1 = 0.0;
  if (s >= 2) {                      // wholly below the diagonal block
#pragma unroll 8
    for (int q = 0; q < RS / 2; ++q) {
      const int64_t r = r0 + 2 * q + ph;
      const v2d v = *reinterpret_cast<const v2d*>(src + r * a.ldl);
      const double ur = a.u[r];
      d0 = __builtin_fma(v.x, v.x, d0);
      d1 = __builtin_fma(v.y, v.y, d1);
      a0 = __builtin_fma(v.x, ur, a0);
      a1 = __builtin_fma(v.y, ur, a1);
    }
  } else {
    for (int q = 0; q < RS / 2; ++q) {
      const int64_t r = r0 + 2 * q + ph;
      if (r < c) continue;           // both elements above the diagonal
      const double ur = a.u[r];
      if (r > c) {
        const v2d v = *reinterpret_cast<const v2d*>(src + r * a.ldl);
        d0 = __builtin_fma(v.x, v.x, d0);
        d1 = __builtin_fma(v.y, v.y, d1);
        a0 = __builtin_fma(v.x, ur, a0);
        a1 = __builtin_fma(v.y, ur, a1);
      } else {                       // r == c: the second element of the pair is above the diagonal
        const double x = src[r * a.ldl];
        d0 = __builtin_fma(x, x, d0);
        a0 = __builtin_fma(x, ur, a0);
      }
    }
  }
  if (ph == 1) {
    sd[2 * tx] = d0;
    sd[2 * tx + 1] = d1;
    sd[CT + 2 * tx] = a0;
    sd[CT + 2 * tx + 1] = a1;
  }
  __syncthreads();
  if (ph == 0) {
    const int64_t slot = (int64_t)t * (2 * a.nb - t + 1) + s;
    double* p = a.part + slot * 2 * CT;
    *reinterpret_cast<v2d*>(p + 2 * tx) = v2d{d0 + sd[2 * tx], d1 + sd[2 * tx + 1]};
    *reinterpret_cast<v2d*>(p + CT + 2 * tx) = v2d{a0 + sd[CT + 2 * tx], a1 + sd[CT + 2 * tx + 1]};
  }
}

// the slices of a tile in ascending row order
__global__ void __launch_bounds__(256) kinv_diag_finish_kernel(const double* __restrict__ part, int nb, double* __restrict__ d,
                                                               double* __restrict__ alpha) {
  const int t = (int)blockIdx.x, j = threadIdx.x;
  const double* p = part + (int64_t)t * (2 * nb - t + 1) * 2 * CT;
  double sd = 0.0, sa = 0.0;
  for (int s = 0; s < 2 * (nb - t); ++s) {
    sd += p[(int64_t)s * 2 * CT + j];
    sa += p[(int64_t)s * 2 * CT + CT + j];
  }
  d[(int64_t)t * CT + j] = sd;
  alpha[(int64_t)t * CT + j] = sa;
}

struct LooArgs {
  int k; int64_t C;
  const double* G; const int32_t* idx; const double* alpha; int64_t n;
  double* out; double* resid; double* var; double* white; int* status;
};

template <int KM>
__global__ void __launch_bounds__(256) set_loo_kernel(const LooArgs a) {
  constexpr int LS = KM + 1;
  __shared__ double S[KM * LS];
  __shared__ double col[KM];
  __shared__ double rhs[KM];       // alpha_B, forward-substituted in place: white once the factorisation is through
  __shared__ double xd[KM];        // diagonal of Lg^-1
  __shared__ int live[KM];
  const int tid = threadIdx.x;
  const int k = a.k;
  const int64_t c = blockIdx.x;
  if (tid < KM) {
    int v = 0;
    double r = 0.0;
    if (tid < k) {
      const int32_t e = a.idx[c * k + tid];
      v = e >= 0 && (int64_t)e < a.n;
      if (v) r = a.alpha[e];
    }
    live[tid] = v;
    rhs[tid] = r;
  }
  __syncthreads();
  const double* Gc = a.G + c * (int64_t)k * k;
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    S[i * LS + j] = (live[i] && live[j]) ? Gc[e] : (i == j ? 1.0 : 0.0);
  }
  __syncthreads();

  double logsum = 0.0;
  int fail = -1;
  for (int j = 0; j < k; ++j) {
    const double d = S[j * LS + j];                // every thread reads the same pivot: the branch below is uniform
    if (!(d > 0.0) || !isfinite(d)) {
      fail = j;
      break;
    }
    logsum += log(d);
    const double sq = sqrt(d), rd = 1.0 / sq;
    const double wj = rhs[j] * rd;                 // (final: row j took its last update in column j - 1)
    for (int i = j + 1 + tid; i < k; i += 256) {
      const double l = S[i * LS + j] * rd;
      col[i] = l;
      S[i * LS + j] = l;
      rhs[i] -= l * wj;
    }
    __syncthreads();
    if (tid == 0) {
      S[j * LS + j] = sq;
      xd[j] = rd;
      rhs[j] = wj;
    }
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
  const double nan = __builtin_nan("");
  double* rc = a.resid + c * (int64_t)k;
  double* vc = a.var + c * (int64_t)k;
  double* wc = a.white + c * (int64_t)k;
  if (fail >= 0) {
    if (tid < k) rc[tid] = vc[tid] = wc[tid] = nan;
    if (tid == 0) {
      a.out[c] = nan;
      a.out[a.C + c] = nan;
      a.status[c] = 1 + fail;
    }
    return;
  }
  // X = Lg^-1, column j by thread j into row j of the upper triangle: X_jj = 1 / L_jj,  X_ij = -(sum_{j <= l < i} L_il X_lj) / L_ii
  if (tid < k) {
    const int j = tid;
    double* Xj = S + j * LS;                       // Xj[i] = X_ij for i > j
    const double xjj = xd[j];
    for (int i = 1; i < k; ++i) {                  // (i and l run alike in every lane: L_il is one broadcast read)
      double s = 0.0;
      for (int l = 0; l < i; ++l) {
        const double lil = S[i * LS + l];
        if (l > j) s = __builtin_fma(lil, Xj[l], s);
        else if (l == j) s = lil * xjj;
      }
      if (i > j) Xj[i] = -s * xd[i];
    }
    double v = xjj * xjj, r = xjj * rhs[j];
    for (int i = j + 1; i < k; ++i) {
      const double x = Xj[i];
      v = __builtin_fma(x, x, v);
      r = __builtin_fma(x, rhs[i], r);
    }
    const bool on = live[j] != 0;
    rc[j] = on ? r : nan;
    vc[j] = on ? v : nan;
    wc[j] = on ? rhs[j] : nan;
  }
  if (tid == 0) {
    double q = 0.0;
    int nl = 0;
    for (int i = 0; i < k; ++i) {                  // (padding entries carry white = 0 and a unit pivot)
      q = __builtin_fma(rhs[i], rhs[i], q);
      nl += live[i];
    }
    a.out[c] = -0.5 * q + 0.5 * logsum - 0.5 * nl * 1.8378770664093453;   // log 2 pi
    a.out[a.C + c] = q;
    a.status[c] = 0;
  }
}

int64_t diag_slots(int64_t m) {
  const int64_t nb = m / CT;
  return nb * (nb + 1);
}

}  // namespace

extern "C" size_t geobo_kinv_diag_ws_bytes(int64_t m) {
  if (m <= 0 || m % GEOBO_PAD_M) return 0;
  return (size_t)diag_slots(m) * 2 * CT * sizeof(double);
}

extern "C" int geobo_kinv_diag(int64_t m, const double* Linv, int64_t ldl, const double* u, double* d, double* alpha, void* ws,
                               size_t ws_bytes, void* stream) {
  // every check before any device access
  if (!Linv || !u || !d || !alpha || !ws) return GEOBO_E_ARG;
  if (m <= 0 || m % GEOBO_PAD_M || m > (int64_t)1 << 20 || ldl < m || (ldl & 1)) return GEOBO_E_ARG;
  if (((uintptr_t)Linv & 15) || ((uintptr_t)ws & 15)) return GEOBO_E_ARG;     // 16-byte loads of column pairs
  if (ws_bytes < geobo_kinv_diag_ws_bytes(m)) return GEOBO_E_ARG;
  DiagArgs a{};
  a.L = Linv; a.ldl = ldl; a.u = u; a.m = m; a.nb = (int)(m / CT); a.part = (double*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kinv_diag_kernel, dim3((unsigned)diag_slots(m)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(kinv_diag_finish_kernel, dim3((unsigned)a.nb), dim3(CT), 0, st, (const double*)ws, a.nb, d, alpha);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_set_loo(int64_t C, int k, const double* G, const int32_t* idx, const double* alpha, int64_t n, double* out,
                             double* resid, double* var, double* white, int* status, void* stream) {
  if (!G || !idx || !alpha || !out || !resid || !var || !white || !status) return GEOBO_E_ARG;
  if (C < 0 || C > INT32_MAX || k < 1 || k > KMAX || n < 0) return GEOBO_E_ARG;
  if (C == 0) return GEOBO_OK;
  LooArgs a{};
  a.k = k; a.C = C; a.G = G; a.idx = idx; a.alpha = alpha; a.n = n;
  a.out = out; a.resid = resid; a.var = var; a.white = white; a.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (k <= 64)
    hipLaunchKernelGGL(set_loo_kernel<64>, dim3((unsigned)C), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(set_loo_kernel<128>, dim3((unsigned)C), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
