// append.hip -- new drill rows behind the last row of a factorised K_y, without a new factorisation.
//
//   geobo_factor_append:  S = D - G (k <= 128), Cholesky S = Ls Ls^T in LDS, T = Ls^-1 in place, uP = T r, sum log diag Ls
//   geobo_rows_downdate:  mu[j] += sum_r c[r] V[r, j],  var[j] -= sum_r V[r, j]^2   over the n new rows of V = L^-1 A3 K
//
// factor_append: one workgroup, S in LDS (k = 128: 129 KiB -- one k x k matrix fits, not two, so the inverse overwrites the factor
// column by column once the factor has gone out).  The factorisation is the unblocked right-looking one of set_logdet_kernel (two
// barriers per column); the inverse is the unblocked lower-triangular one from the last column to the first,
//     T[j+1:, j] = -T[j+1:, j+1:] Ls[j+1:, j] / Ls[j][j],
// one thread per row.  The diagonal lives in an array of its own while the columns are being scaled (every thread reads the pivot
// its column is divided by).  A pivot that is not positive (or not finite) gives status 1 + pivot and NOTHING else is written.
//
// rows_downdate: a stream of n x ncols doubles; a thread owns two adjacent columns (16-byte loads where the addresses allow, one
// column and 8-byte loads otherwise -- the same arithmetic) and walks the rows in ascending order from the stored values with one
// fma per row and sum: cutting the rows into several calls gives the same bits.  No atomics, no LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "geobo_hip.h"

namespace {

constexpr int KMAX = 128;

struct AppendArgs {
  int k;
  const double* D; int64_t ldd;
  const double* G; int64_t ldg;
  const double* r;
  double* Ls; int64_t ldl;
  double* T; int64_t ldt;
  double* uP; double* logsum; int* status;
};

template <int KM>
__global__ void __launch_bounds__(256) factor_append_kernel(const AppendArgs a) {
  constexpr int LS = KM + 1;
  __shared__ double S[KM * LS];
  __shared__ double col[KM];
  __shared__ double diag[KM];
  const int tid = threadIdx.x;
  const int k = a.k;
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    if (j <= i) S[i * LS + j] = a.D[i * a.ldd + j] - a.G[i * a.ldg + j];
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
    const double sd = sqrt(d);
    logsum += log(sd);
    if (tid == 0) diag[j] = sd;                    // (S[j][j] itself stays: other threads may still be reading it)
    for (int i = j + 1 + tid; i < k; i += 256) {
      const double v = S[i * LS + j] / sd;
      col[i] = v;
      S[i * LS + j] = v;
    }
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
  if (fail >= 0) {
    if (tid == 0) a.status[0] = 1 + fail;
    return;
  }
  if (tid < k) S[tid * LS + tid] = diag[tid];
  __syncthreads();
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    a.Ls[i * a.ldl + j] = j <= i ? S[i * LS + j] : 0.0;
  }
  __syncthreads();

  // T = Ls^-1 in place: the diagonal first, then the columns from the last to the first against the inverted trailing block
  if (tid < k) {
    S[tid * LS + tid] = 1.0 / diag[tid];
    diag[tid] = a.r[tid];                          // (the factor's diagonal is done with: the array now holds r for uP = T r)
  }
  __syncthreads();
  for (int j = k - 2; j >= 0; --j) {
    if (tid > j && tid < k) col[tid] = S[tid * LS + j];
    __syncthreads();
    if (tid > j && tid < k) {
      double s = 0.0;
      for (int l = j + 1; l <= tid; ++l) s = fma(S[tid * LS + l], col[l], s);
      S[tid * LS + j] = -s * S[j * LS + j];
    }
    __syncthreads();
  }
  if (tid < k) {
    double s = 0.0;
    for (int l = 0; l <= tid; ++l) s = fma(S[tid * LS + l], diag[l], s);
    a.uP[tid] = s;
  }
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    a.T[i * a.ldt + j] = j <= i ? S[i * LS + j] : 0.0;
  }
  if (tid == 0) {
    a.logsum[0] = logsum;
    a.status[0] = 0;
  }
}

struct DowndateArgs {
  const double* V; int64_t ld; int64_t n; int64_t ncols;
  const double* c;
  double* mu; double* var;
};

template <bool PAIR>
__global__ void __launch_bounds__(256) rows_downdate_kernel(const DowndateArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (PAIR) {
    const int64_t j = 2 * t;
    if (j + 1 < a.ncols) {
      double2 m = *reinterpret_cast<const double2*>(a.mu + j);
      double2 s = *reinterpret_cast<const double2*>(a.var + j);
      const double* p = a.V + j;
#pragma unroll 4
      for (int64_t r = 0; r < a.n; ++r) {
        const double2 v = *reinterpret_cast<const double2*>(p + r * a.ld);
        const double cr = a.c[r];
        m.x = fma(cr, v.x, m.x);
        m.y = fma(cr, v.y, m.y);
        s.x = fma(-v.x, v.x, s.x);
        s.y = fma(-v.y, v.y, s.y);
      }
      *reinterpret_cast<double2*>(a.mu + j) = m;
      *reinterpret_cast<double2*>(a.var + j) = s;
      return;
    }
    if (j >= a.ncols) return;
    // (an odd column count: the last column on its own)
    double m = a.mu[j], s = a.var[j];
    for (int64_t r = 0; r < a.n; ++r) {
      const double v = a.V[r * a.ld + j];
      m = fma(a.c[r], v, m);
      s = fma(-v, v, s);
    }
    a.mu[j] = m;
    a.var[j] = s;
  } else {
    if (t >= a.ncols) return;
    double m = a.mu[t], s = a.var[t];
#pragma unroll 4
    for (int64_t r = 0; r < a.n; ++r) {
      const double v = a.V[r * a.ld + t];
      m = fma(a.c[r], v, m);
      s = fma(-v, v, s);
    }
    a.mu[t] = m;
    a.var[t] = s;
  }
}

}  // namespace

extern "C" int geobo_factor_append(int k, const double* D, int64_t ldd, const double* G, int64_t ldg, const double* r, double* Ls,
                                   int64_t ldl, double* T, int64_t ldt, double* uP, double* logsum, int* status, void* stream) {
  // every check before any device access
  if (!D || !G || !r || !Ls || !T || !uP || !logsum || !status) return GEOBO_E_ARG;
  if (k < 1 || k > KMAX || ldd < k || ldg < k || ldl < k || ldt < k) return GEOBO_E_ARG;
  AppendArgs a{};
  a.k = k; a.D = D; a.ldd = ldd; a.G = G; a.ldg = ldg; a.r = r; a.Ls = Ls; a.ldl = ldl; a.T = T; a.ldt = ldt;
  a.uP = uP; a.logsum = logsum; a.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (k <= 64)
    hipLaunchKernelGGL(factor_append_kernel<64>, dim3(1), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(factor_append_kernel<128>, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_rows_downdate(const double* V, int64_t ld, int64_t n, int64_t ncols, const double* c, double* mu, double* var,
                                   void* stream) {
  if (!mu || !var || (n > 0 && (!V || !c))) return GEOBO_E_ARG;
  if (n < 0 || ncols < 0 || ld < ncols || ncols > ((int64_t)1 << 38)) return GEOBO_E_ARG;
  if (n == 0 || ncols == 0) return GEOBO_OK;
  DowndateArgs a{};
  a.V = V; a.ld = ld; a.n = n; a.ncols = ncols; a.c = c; a.mu = mu; a.var = var;
  hipStream_t st = (hipStream_t)stream;
  const bool pair = ((uintptr_t)V % 16 == 0) && ((uintptr_t)mu % 16 == 0) && ((uintptr_t)var % 16 == 0) && ld % 2 == 0;
  if (pair) {
    const int64_t threads = (ncols + 1) / 2;
    hipLaunchKernelGGL(rows_downdate_kernel<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(rows_downdate_kernel<false>, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
