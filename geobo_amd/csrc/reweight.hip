// reweight.hip -- down-weight or drop rows of a factorised K_y, exactly, without a new factorisation.
//
//   geobo_fold_factor:    S = G + diag(dinv) (k <= 128), Cholesky S = C C^T in LDS, C^-1 in place, g = C^-1 a,
//                         stats = (2 sum log diag C, g^T g)
//   geobo_rows_reweight:  per column c of a k x ncols tile of B:  t = C^-1 B[:, c],  mu[c] -= t . g,  var[c] += t . t,
//                         and sum_c dmu^2, max_c |dmu|, sum_c dvar of the tile
//
// fold_factor is geobo_factor_append (append.hip) with another matrix in front and other products behind: one workgroup, S in LDS
// with row stride k + 1, the unblocked right-looking factorisation of set_logdet_kernel (two barriers per column), the unblocked
// lower-triangular inverse from the last column to the first, one thread per row.  A pivot that is not positive (or not finite) gives
// status 1 + pivot and NOTHING else is written.
//
// rows_reweight: a stream of k x ncols doubles with k^2 / 2 fma per column.  C^-1 (packed lower triangle) and g sit in LDS, staged
// once per workgroup; every lane of a wave reads the same entry (a broadcast: no bank conflict whatever the layout).  A thread owns two
// adjacent columns (16-byte loads where the addresses allow, one column and 8-byte loads otherwise -- the same arithmetic) and walks
// the rows of C^-1 in blocks of 16: the 16 sums t_r of a block live in registers and take their terms in ascending q, so B[q, c] is
// loaded once per block of rows (the first load comes from HBM, the k / 16 - 1 later ones from cache).  A column's result depends on
// nothing but the column: a tile cut at any even column gives the same mu and var bits.  The three tile sums go through one partial
// per workgroup (a fixed butterfly inside a wave, the four waves in order) and a finishing launch that adds the partials in index
// order: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "geobo_hip.h"

namespace {

constexpr int KMAX = 128;

struct FoldArgs {
  int k;
  const double* G; int64_t ldg;
  const double* dinv;
  const double* a;
  double* Cinv; int64_t ldc;
  double* g; double* stats; int* status;
};

template <int KM>
__global__ void __launch_bounds__(256) fold_factor_kernel(const FoldArgs a) {
  constexpr int LS = KM + 1;
  __shared__ double S[KM * LS];
  __shared__ double col[KM];
  __shared__ double diag[KM];
  const int tid = threadIdx.x;
  const int k = a.k;
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    if (j < i) S[i * LS + j] = a.G[i * a.ldg + j];
    if (j == i) S[i * LS + j] = a.G[i * a.ldg + j] + a.dinv[i];
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

  // C^-1 in place: the diagonal first, then the columns from the last to the first against the inverted trailing block
  if (tid < k) {
    S[tid * LS + tid] = 1.0 / diag[tid];
    diag[tid] = a.a[tid];                          // (the factor's diagonal is done with: the array now holds a for g = C^-1 a)
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
    col[tid] = s;
    a.g[tid] = s;
  }
  for (int e = tid; e < k * k; e += 256) {
    const int i = e / k, j = e - i * k;
    a.Cinv[i * a.ldc + j] = j <= i ? S[i * LS + j] : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double gg = 0.0;
    for (int l = 0; l < k; ++l) gg = fma(col[l], col[l], gg);
    a.stats[0] = 2.0 * logsum;
    a.stats[1] = gg;
    a.status[0] = 0;
  }
}

struct ReweightArgs {
  int k;
  const double* B; int64_t ldb; int64_t ncols;
  const double* Cinv; int64_t ldc;
  const double* g;
  double* mu; double* var;
  double* ws;
};

constexpr int RB = 16;                             // rows of C^-1 whose sums a thread holds at a time

__device__ __forceinline__ int tri(int r) { return r * (r + 1) / 2; }

template <int KM, bool PAIR>
__global__ void __launch_bounds__(256) rows_reweight_kernel(const ReweightArgs a) {
  static_assert(KM % RB == 0, "whole row blocks");
  __shared__ double Cs[KM * (KM + 1) / 2];
  __shared__ double gs[KM];
  __shared__ double red[3 * 4];
  const int tid = threadIdx.x;
  const int k = a.k;
  const int kp = (k + RB - 1) / RB * RB;           // rows behind k: zero rows of C^-1 and zero entries of g (they add nothing)
  for (int e = tid; e < kp * kp; e += 256) {
    const int r = e / kp, q = e - r * kp;
    if (q <= r) Cs[tri(r) + q] = r < k ? a.Cinv[r * a.ldc + q] : 0.0;
  }
  if (tid < kp) gs[tid] = tid < k ? a.g[tid] : 0.0;
  __syncthreads();

  const int64_t c = ((int64_t)blockIdx.x * 256 + tid) * (PAIR ? 2 : 1);
  const bool have0 = c < a.ncols;
  const bool have1 = PAIR && c + 1 < a.ncols;
  double dm0 = 0.0, dm1 = 0.0, dv0 = 0.0, dv1 = 0.0;
  if (have0) {
    const double* p = a.B + c;
    for (int r0 = 0; r0 < kp; r0 += RB) {
      double t0[RB], t1[RB];
#pragma unroll
      for (int j = 0; j < RB; ++j) t0[j] = t1[j] = 0.0;
      for (int q = 0; q < r0; ++q) {               // the columns in front of the block: every row of the block takes the term
        double b0, b1 = 0.0;
        if (have1) {
          const double2 v = *reinterpret_cast<const double2*>(p + q * a.ldb);
          b0 = v.x;
          b1 = v.y;
        } else {
          b0 = p[q * a.ldb];
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          const double cv = Cs[tri(r0 + j) + q];
          t0[j] = fma(cv, b0, t0[j]);
          if (PAIR) t1[j] = fma(cv, b1, t1[j]);
        }
      }
#pragma unroll
      for (int jq = 0; jq < RB; ++jq) {            // the block's own triangle
        const int q = r0 + jq;
        if (q < k) {
          double b0, b1 = 0.0;
          if (have1) {
            const double2 v = *reinterpret_cast<const double2*>(p + q * a.ldb);
            b0 = v.x;
            b1 = v.y;
          } else {
            b0 = p[q * a.ldb];
          }
#pragma unroll
          for (int j = jq; j < RB; ++j) {
            const double cv = Cs[tri(r0 + j) + q];
            t0[j] = fma(cv, b0, t0[j]);
            if (PAIR) t1[j] = fma(cv, b1, t1[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const double gr = gs[r0 + j];
        dm0 = fma(-t0[j], gr, dm0);
        dv0 = fma(t0[j], t0[j], dv0);
        if (PAIR) {
          dm1 = fma(-t1[j], gr, dm1);
          dv1 = fma(t1[j], t1[j], dv1);
        }
      }
    }
    if (a.mu) {
      if (have1) {
        double2 m = *reinterpret_cast<const double2*>(a.mu + c);
        double2 s = *reinterpret_cast<const double2*>(a.var + c);
        m.x += dm0; m.y += dm1;
        s.x += dv0; s.y += dv1;
        *reinterpret_cast<double2*>(a.mu + c) = m;
        *reinterpret_cast<double2*>(a.var + c) = s;
      } else {
        a.mu[c] += dm0;
        a.var[c] += dv0;
      }
    }
  }

  // the workgroup's partial of the three tile sums: a fixed butterfly per wave, then the four waves in order
  double s2 = fma(dm1, dm1, dm0 * dm0), mx = fmax(fabs(dm0), fabs(dm1)), sv = dv0 + dv1;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s2 += __shfl_xor(s2, off, 64);
    mx = fmax(mx, __shfl_xor(mx, off, 64));
    sv += __shfl_xor(sv, off, 64);
  }
  if ((tid & 63) == 0) {
    red[3 * (tid >> 6) + 0] = s2;
    red[3 * (tid >> 6) + 1] = mx;
    red[3 * (tid >> 6) + 2] = sv;
  }
  __syncthreads();
  if (tid == 0) {
    double r2 = red[0], rm = red[1], rv = red[2];
    for (int w = 1; w < 4; ++w) {
      r2 += red[3 * w + 0];
      rm = fmax(rm, red[3 * w + 1]);
      rv += red[3 * w + 2];
    }
    double* o = a.ws + 3 * (int64_t)blockIdx.x;
    o[0] = r2; o[1] = rm; o[2] = rv;
  }
}

// part = the partials of ws in index order: staged 256 at a time, added by one thread
__global__ void __launch_bounds__(256) reweight_finish_kernel(int64_t nblocks, const double* ws, double* part) {
  __shared__ double buf[3 * 256];
  const int tid = threadIdx.x;
  double r2 = 0.0, rm = 0.0, rv = 0.0;
  for (int64_t b0 = 0; b0 < nblocks; b0 += 256) {
    const int64_t n = nblocks - b0 < 256 ? nblocks - b0 : 256;
    for (int64_t e = tid; e < 3 * n; e += 256) buf[e] = ws[3 * b0 + e];
    __syncthreads();
    if (tid == 0) {
      for (int64_t i = 0; i < n; ++i) {
        r2 += buf[3 * i + 0];
        rm = fmax(rm, buf[3 * i + 1]);
        rv += buf[3 * i + 2];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[0] = r2; part[1] = rm; part[2] = rv;
  }
}

bool reweight_pair(const ReweightArgs& a) {
  return ((uintptr_t)a.B % 16 == 0) && ((uintptr_t)a.mu % 16 == 0) && ((uintptr_t)a.var % 16 == 0) && a.ldb % 2 == 0;
}

int64_t reweight_blocks(int64_t ncols, bool pair) {
  const int64_t threads = pair ? (ncols + 1) / 2 : ncols;
  return (threads + 255) / 256;
}

}  // namespace

extern "C" int geobo_fold_factor(int k, const double* G, int64_t ldg, const double* dinv, const double* a, double* Cinv, int64_t ldc,
                                 double* g, double* stats, int* status, void* stream) {
  // every check before any device access
  if (!G || !dinv || !a || !Cinv || !g || !stats || !status) return GEOBO_E_ARG;
  if (k < 1 || k > KMAX || ldg < k || ldc < k) return GEOBO_E_ARG;
  FoldArgs f{};
  f.k = k; f.G = G; f.ldg = ldg; f.dinv = dinv; f.a = a; f.Cinv = Cinv; f.ldc = ldc; f.g = g; f.stats = stats; f.status = status;
  hipStream_t st = (hipStream_t)stream;
  if (k <= 64)
    hipLaunchKernelGGL(fold_factor_kernel<64>, dim3(1), dim3(256), 0, st, f);
  else
    hipLaunchKernelGGL(fold_factor_kernel<128>, dim3(1), dim3(256), 0, st, f);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" size_t geobo_rows_reweight_ws_bytes(int64_t ncols) {
  if (ncols < 0) return 0;
  const int64_t nb = reweight_blocks(ncols, false);             // (the one-column form has the most workgroups)
  return (size_t)(3 * 8 * (nb > 1 ? nb : 1));
}

extern "C" int geobo_rows_reweight(int k, const double* B, int64_t ldb, int64_t ncols, const double* Cinv, int64_t ldc, const double* g,
                                   double* mu, double* var, double* part, void* ws, size_t ws_bytes, void* stream) {
  if (!B || !Cinv || !g || !part || !ws) return GEOBO_E_ARG;
  if ((mu == nullptr) != (var == nullptr)) return GEOBO_E_ARG;
  if (k < 1 || k > KMAX || ncols < 0 || ldb < ncols || ldc < k || ncols > ((int64_t)1 << 38)) return GEOBO_E_ARG;
  if ((uintptr_t)ws % 8 != 0) return GEOBO_E_ALIGN;
  if (ws_bytes < geobo_rows_reweight_ws_bytes(ncols)) return GEOBO_E_ARG;
  ReweightArgs a{};
  a.k = k; a.B = B; a.ldb = ldb; a.ncols = ncols; a.Cinv = Cinv; a.ldc = ldc; a.g = g; a.mu = mu; a.var = var; a.ws = (double*)ws;
  hipStream_t st = (hipStream_t)stream;
  const bool pair = reweight_pair(a);
  const int64_t nb = reweight_blocks(ncols, pair);
  if (nb > 0) {
    const dim3 grid((unsigned)nb), block(256);
    if (pair) {
      if (k <= 64)
        hipLaunchKernelGGL((rows_reweight_kernel<64, true>), grid, block, 0, st, a);
      else
        hipLaunchKernelGGL((rows_reweight_kernel<128, true>), grid, block, 0, st, a);
    } else {
      if (k <= 64)
        hipLaunchKernelGGL((rows_reweight_kernel<64, false>), grid, block, 0, st, a);
      else
        hipLaunchKernelGGL((rows_reweight_kernel<128, false>), grid, block, 0, st, a);
    }
    if (hipGetLastError() != hipSuccess) return GEOBO_E_LAUNCH;
  }
  hipLaunchKernelGGL(reweight_finish_kernel, dim3(1), dim3(256), 0, st, nb, (const double*)ws, part);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
