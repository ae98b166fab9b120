// sampling.hip -- prior realisations of the three-property GP on the voxel grid by circulant embedding.
//
//   geobo_philox_fill      Philox4x64-10 blocks of counter (element, sample, purpose, sub), key (seed, 0): raw words or fp64
//                          Box-Muller normals
//   geobo_torus_table      w amp k(wrapped lag) of one block pair on the (my, mx, mz) torus, complex interleaved (imaginary 0)
//   geobo_fft_axis         batched complex fp64 Stockham FFT along one axis of a [b0][m][b1] array, whole lines in LDS, radix 4
//                          (one radix-2 stage for odd log2 m); zero-pads the n_in inputs and keeps the first n_out outputs; optional
//                          real-pair packing of the input / output (sample 2k = real part, 2k+1 = imaginary part)
//   geobo_sample_factor    per frequency of the octant: S(w) = [lambda_ij(w)] -> Jacobi eigen-decomposition -> F = V sqrt(max(D, 0));
//                          status = (min eigenvalue, max eigenvalue, clipped trace, trace), traces weighted by the octant multiplicity
//   geobo_sample_zpass     fused: noise (Philox or caller's) -> F(w) / sqrt(M) -> inverse z FFT -> first nz outputs
//   geobo_spectral_mix     out_i(w) = scale sum_j lambda_ij(w) in_j(w): the covariance product K v on the torus (conditioning)
//
// Layouts: voxel p = (iy nx + ix) nz + iz; torus frequency (wy my... ) flat index (wy mx + wx) mz + wz; octant index
// (fy (mx/2+1) + fx) (mz/2+1) + fz with f = min(w, m - w); block pairs i <= j in row order (0,0),(0,1),...,(P-1,P-1).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covfun.h"
#include "geobo_hip.h"

namespace {

constexpr int FFT_LDS = 4096;   // complex elements of one workgroup's lines (64 KiB)
constexpr int FFT_THREADS = 256;
constexpr uint64_t PH_M0 = 0xD2E7470EE14C6C93ull, PH_M1 = 0xCA5A826395121157ull;
constexpr uint64_t PH_W0 = 0x9E3779B97F4A7C15ull, PH_W1 = 0xBB67AE8584CAA73Bull;

__device__ __forceinline__ void philox4x64_10(uint64_t c[4], uint64_t k0, uint64_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += PH_W0; k1 += PH_W1; }
    const uint64_t lo0 = PH_M0 * c[0], hi0 = __umul64hi(PH_M0, c[0]);
    const uint64_t lo1 = PH_M1 * c[2], hi1 = __umul64hi(PH_M1, c[2]);
    const uint64_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
  }
}

// uniforms ((x >> 11) + 0.5) 2^-53 in (0, 1); normals r cos(2 pi u1), r sin(2 pi u1), r = sqrt(-2 log u0) (NumPy's operation order)
__device__ __forceinline__ void box_muller(uint64_t a, uint64_t b, double& n0, double& n1) {
  const double u0 = ((double)(a >> 11) + 0.5) * 0x1p-53, u1 = ((double)(b >> 11) + 0.5) * 0x1p-53;
  const double r = sqrt(-2.0 * log(u0));
  const double t = 6.283185307179586 * u1;
  n0 = r * cos(t);
  n1 = r * sin(t);
}

__device__ __forceinline__ void philox_normals4(uint64_t seed, uint64_t elem, uint64_t sample, uint64_t purpose, uint64_t sub,
                                                double n[4]) {
  uint64_t c[4] = {elem, sample, purpose, sub};
  philox4x64_10(c, seed, 0);
  box_muller(c[0], c[1], n[0], n[1]);
  box_muller(c[2], c[3], n[2], n[3]);
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// one Stockham stage of radix R over C lines of length m held in LDS at lds[c sc + j sj]: every thread reads all of its butterflies'
// inputs, the workgroup synchronises, then every thread writes (one buffer suffices).  Forward: exp(-2 pi i jk / m); inverse: +.
template <int R>
__device__ __forceinline__ void stockham_stage(double2* lds, int m, int C, int sc, int sj, int Ns, bool inverse) {
  constexpr int MAXB = FFT_LDS / R / FFT_THREADS;
  const int mq = m / R, W = C * mq;
  double2 v[MAXB][R];
  int cidx[MAXB], jidx[MAXB];
#pragma unroll
  for (int t = 0; t < MAXB; ++t) {
    const int w = threadIdx.x + t * FFT_THREADS;
    cidx[t] = -1;
    if (w < W) {
      const int c = sj == 1 ? w / mq : w % C, j = sj == 1 ? w % mq : w / C;
      cidx[t] = c; jidx[t] = j;
#pragma unroll
      for (int r = 0; r < R; ++r) v[t][r] = lds[c * sc + (j + r * mq) * sj];
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < MAXB; ++t) {
    if (cidx[t] < 0) continue;
    const int c = cidx[t], j = jidx[t], jm = j % Ns;
#pragma unroll
    for (int r = 1; r < R; ++r) {
      // angle 2 pi jm r / (Ns R): an exact binary fraction for sincospi
      double s, co;
      sincospi(2.0 * (double)(jm * r) / (double)(Ns * R), &s, &co);
      v[t][r] = cmul(v[t][r], make_double2(co, inverse ? s : -s));
    }
    double2 y[R];
    if constexpr (R == 2) {
      y[0] = cadd(v[t][0], v[t][1]);
      y[1] = csub(v[t][0], v[t][1]);
    } else {
      const double2 a0 = cadd(v[t][0], v[t][2]), a1 = csub(v[t][0], v[t][2]), a2 = cadd(v[t][1], v[t][3]);
      const double2 d = csub(v[t][1], v[t][3]);
      const double2 a3 = inverse ? make_double2(-d.y, d.x) : make_double2(d.y, -d.x);   // (+-i) (v1 - v3)
      y[0] = cadd(a0, a2); y[2] = csub(a0, a2); y[1] = cadd(a1, a3); y[3] = csub(a1, a3);
    }
    const int base = (j / Ns) * Ns * R + jm;
#pragma unroll
    for (int r = 0; r < R; ++r) lds[c * sc + (base + r * Ns) * sj] = y[r];
  }
  __syncthreads();
}

__device__ void fft_lds(double2* lds, int m, int C, int sc, int sj, bool inverse) {
  int Ns = 1;
  if (__builtin_ctz(m) & 1) {
    stockham_stage<2>(lds, m, C, sc, sj, Ns, inverse);
    Ns = 2;
  }
  for (; Ns < m; Ns *= 4) stockham_stage<4>(lds, m, C, sc, sj, Ns, inverse);
}

// real-pair packing: complex element f of a [kq][Q] array <-> reals of samples 2k, 2k+1 in an (S, P, Q) array, kq = k P + q
__device__ __forceinline__ void pair_addr(int64_t f, int P, int64_t Q, int64_t& re, int64_t& im, int& k2) {
  const int64_t kq = f / Q, rem = f - kq * Q, k = kq / P, q = kq - k * P;
  k2 = (int)(2 * k);
  re = ((2 * k) * P + q) * Q + rem;
  im = ((2 * k + 1) * P + q) * Q + rem;
}

__global__ void __launch_bounds__(FFT_THREADS) fft_axis_kernel(int flags, int64_t B0, int m, int64_t B1, int n_in, int n_out, int C,
                                                               const double* __restrict__ in, double* __restrict__ out, int P,
                                                               int64_t Q, int64_t S) {
  __shared__ double2 lds[FFT_LDS];
  const bool inverse = flags & GEOBO_FFT_INVERSE, in_pairs = flags & GEOBO_FFT_IN_PAIRS, out_pairs = flags & GEOBO_FFT_OUT_PAIRS;
  const bool contig = B1 == 1;
  int64_t b0_first, b1_first;
  if (contig) {
    b0_first = (int64_t)blockIdx.x * C; b1_first = 0;
  } else {
    const int64_t tiles = (B1 + C - 1) / C;
    b0_first = (int64_t)blockIdx.x / tiles; b1_first = ((int64_t)blockIdx.x % tiles) * C;
  }
  const int sc = contig ? m : 1, sj = contig ? 1 : C;
  for (int e = threadIdx.x; e < C * m; e += FFT_THREADS) {
    const int c = contig ? e / m : e % C, j = contig ? e % m : e / C;
    const int64_t b0 = contig ? b0_first + c : b0_first, b1 = contig ? 0 : b1_first + c;
    double2 v = make_double2(0.0, 0.0);
    if (j < n_in && b0 < B0 && b1 < B1) {
      const int64_t f = (b0 * n_in + j) * B1 + b1;
      if (in_pairs) {
        int64_t re, im; int k2;
        pair_addr(f, P, Q, re, im, k2);
        v.x = k2 < S ? in[re] : 0.0;
        v.y = k2 + 1 < S ? in[im] : 0.0;
      } else {
        v = reinterpret_cast<const double2*>(in)[f];
      }
    }
    lds[c * sc + j * sj] = v;
  }
  __syncthreads();
  fft_lds(lds, m, C, sc, sj, inverse);
  for (int e = threadIdx.x; e < C * n_out; e += FFT_THREADS) {
    const int c = contig ? e / n_out : e % C, j = contig ? e % n_out : e / C;
    const int64_t b0 = contig ? b0_first + c : b0_first, b1 = contig ? 0 : b1_first + c;
    if (b0 >= B0 || b1 >= B1) continue;
    const double2 v = lds[c * sc + j * sj];
    const int64_t f = (b0 * n_out + j) * B1 + b1;
    if (out_pairs) {
      int64_t re, im; int k2;
      pair_addr(f, P, Q, re, im, k2);
      if (k2 < S) out[re] = v.x;
      if (k2 + 1 < S) out[im] = v.y;
    } else {
      reinterpret_cast<double2*>(out)[f] = v;
    }
  }
}

template <int ID>
__global__ void __launch_bounds__(256) torus_table_kernel(int my, int mx, int mz, double sx, double sy, double sz, const CovParams p,
                                                          double2* __restrict__ out) {
  const int64_t n = (int64_t)my * mx * mz;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int wz = (int)(i % mz);
    const int64_t t = i / mz;
    const int wx = (int)(t % mx), wy = (int)(t / mx);
    const int dz = wz < mz - wz ? wz : mz - wz, dx = wx < mx - wx ? wx : mx - wx, dy = wy < my - wy ? wy : my - wy;
    // the coordinate differences of geobo_cov_table / geobo_k_block: (d + 1) s - 1 s per axis
    const double d2 = sqdist3(1.0 * sx, 1.0 * sy, 1.0 * sz, (double)(dx + 1) * sx, (double)(dy + 1) * sy, (double)(dz + 1) * sz);
    out[i] = make_double2(p.scale * cov_eval<ID>(p, d2), 0.0);
  }
}

__device__ __forceinline__ int pair_index(int i, int j, int P) {   // i <= j, row order of the upper triangle
  return i * P - i * (i - 1) / 2 + (j - i);
}

// cyclic Jacobi on a symmetric P x P matrix (P <= 3): a -> diag(eigenvalues), v -> eigenvectors (columns)
template <int P>
__device__ void jacobi_eig(double a[3][3], double v[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j) {
        tot += a[i][j] * a[i][j];
        if (i != j) off += a[i][j] * a[i][j];
      }
    if (!(off > 1e-34 * tot)) break;
    for (int p = 0; p < P - 1; ++p)
      for (int q = p + 1; q < P; ++q) {
        // an off-diagonal below the rounding of its two diagonal entries is zero: rotating on it (repeated eigenvalues: a large
        // angle set by noise) never converges and every such rotation costs V an eps of orthogonality
        if (fabs(a[p][q]) <= 0x1p-54 * (fabs(a[p][p]) + fabs(a[q][q]))) {
          a[p][q] = a[q][p] = 0.0;
          continue;
        }
        const double tau = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
        for (int k = 0; k < P; ++k) {   // columns p, q
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < P; ++k) {   // rows p, q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
        }
        a[p][q] = a[q][p] = 0.0;   // what the rotation was chosen for
        for (int k = 0; k < P; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

constexpr int FACTOR_BLOCKS = 256;

template <int P>
__global__ void __launch_bounds__(256) sample_factor_kernel(int my, int mx, int mz, const double2* __restrict__ spectra,
                                                            double* __restrict__ F, double* __restrict__ lam, double* __restrict__ part) {
  const int hy = my / 2 + 1, hx = mx / 2 + 1, hz = mz / 2 + 1;
  const int64_t M = (int64_t)my * mx * mz, n = (int64_t)hy * hx * hz;
  constexpr int NP = P * (P + 1) / 2;
  double emin = INFINITY, emax = -INFINITY, clip = 0.0, tr = 0.0;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) {
    const int fz = (int)(o % hz);
    const int64_t t = o / hz;
    const int fx = (int)(t % hx), fy = (int)(t / hx);
    const int64_t w = ((int64_t)fy * mx + fx) * mz + fz;
    double a[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, v[3][3];
    for (int i = 0; i < P; ++i)
      for (int j = i; j < P; ++j) {
        const double l = spectra[(int64_t)pair_index(i, j, P) * M + w].x;
        a[i][j] = a[j][i] = l;
        lam[o * NP + pair_index(i, j, P)] = l;
      }
    jacobi_eig<P>(a, v);
    const double mult = (fy == 0 || 2 * fy == my ? 1.0 : 2.0) * (fx == 0 || 2 * fx == mx ? 1.0 : 2.0) * (fz == 0 || 2 * fz == mz ? 1.0 : 2.0);
    for (int k = 0; k < P; ++k) {
      const double e = a[k][k];
      emin = fmin(emin, e); emax = fmax(emax, e);
      tr += mult * e;
      if (e < 0) clip -= mult * e;
      const double r = e > 0 ? sqrt(e) : 0.0;
      for (int i = 0; i < P; ++i) F[o * P * P + i * P + k] = v[i][k] * r;
    }
  }
  __shared__ double red[4][256];
  red[0][threadIdx.x] = emin; red[1][threadIdx.x] = emax; red[2][threadIdx.x] = clip; red[3][threadIdx.x] = tr;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] = fmin(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + s]);
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
      red[3][threadIdx.x] += red[3][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) part[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void __launch_bounds__(256) factor_status_kernel(const double* __restrict__ part, int nparts, double* __restrict__ status) {
  __shared__ double red[4][256];
  double v[4] = {INFINITY, -INFINITY, 0.0, 0.0};
  for (int b = threadIdx.x; b < nparts; b += 256) {
    v[0] = fmin(v[0], part[b * 4 + 0]); v[1] = fmax(v[1], part[b * 4 + 1]);
    v[2] += part[b * 4 + 2]; v[3] += part[b * 4 + 3];
  }
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] = fmin(red[0][threadIdx.x], red[0][threadIdx.x + s]);
      red[1][threadIdx.x] = fmax(red[1][threadIdx.x], red[1][threadIdx.x + s]);
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
      red[3][threadIdx.x] += red[3][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) status[threadIdx.x] = red[threadIdx.x][0];
}

__device__ __forceinline__ int64_t octant_index(int wy, int wx, int wz, int my, int mx, int mz) {
  const int fy = wy < my - wy ? wy : my - wy, fx = wx < mx - wx ? wx : mx - wx, fz = wz < mz - wz ? wz : mz - wz;
  return ((int64_t)fy * (mx / 2 + 1) + fx) * (mz / 2 + 1) + fz;
}

// C lines (pair k, wy, wx) of P components each: noise -> F(w) xi / sqrt(M) in LDS -> inverse z FFT -> outputs iz < nz
template <int P>
__global__ void __launch_bounds__(FFT_THREADS) sample_zpass_kernel(int64_t kp0, int64_t npairs, int my, int mx, int mz, int nz, int C,
                                                                   const double* __restrict__ F, const double2* __restrict__ noise,
                                                                   uint64_t seed, double scale, double2* __restrict__ out) {
  __shared__ double2 lds[FFT_LDS];
  const int64_t lines = npairs * my * mx, M = (int64_t)my * mx * mz;
  const int64_t g0 = (int64_t)blockIdx.x * C;
  for (int e = threadIdx.x; e < C * mz; e += FFT_THREADS) {
    const int c = e / mz, wz = e % mz;
    const int64_t g = g0 + c;
    double2 y[P];
    for (int i = 0; i < P; ++i) y[i] = make_double2(0.0, 0.0);
    if (g < lines) {
      const int64_t k = g / ((int64_t)my * mx), rem = g % ((int64_t)my * mx);
      const int wy = (int)(rem / mx), wx = (int)(rem % mx);
      const int64_t w = rem * mz + wz;
      double2 xi[P];
      if (noise) {
        for (int q = 0; q < P; ++q) xi[q] = noise[(k * M + w) * P + q];
      } else {
        double n[8];
        philox_normals4(seed, (uint64_t)w, (uint64_t)(kp0 + k), GEOBO_RNG_PRIOR, 0, n);
        if (P > 2) philox_normals4(seed, (uint64_t)w, (uint64_t)(kp0 + k), GEOBO_RNG_PRIOR, 1, n + 4);
        for (int q = 0; q < P; ++q) xi[q] = make_double2(n[2 * q], n[2 * q + 1]);
      }
      const double* f = F + octant_index(wy, wx, wz, my, mx, mz) * P * P;
      for (int i = 0; i < P; ++i) {
        double2 s = make_double2(0.0, 0.0);
        for (int q = 0; q < P; ++q) {
          const double fq = f[i * P + q];
          s.x += fq * xi[q].x; s.y += fq * xi[q].y;
        }
        y[i] = make_double2(scale * s.x, scale * s.y);
      }
    }
    for (int i = 0; i < P; ++i) lds[(c * P + i) * mz + wz] = y[i];
  }
  __syncthreads();
  fft_lds(lds, mz, C * P, mz, 1, true);
  for (int e = threadIdx.x; e < C * P * nz; e += FFT_THREADS) {
    const int L = e / nz, iz = e % nz, c = L / P, i = L % P;
    const int64_t g = g0 + c;
    if (g >= lines) continue;
    const int64_t k = g / ((int64_t)my * mx), rem = g % ((int64_t)my * mx);
    // intermediate [k][i][wy][wx][iz]: the x pass reads lines of mx along its middle axis
    out[((k * P + i) * my * mx + rem) * nz + iz] = lds[L * mz + iz];
  }
}

template <int P>
__global__ void __launch_bounds__(256) spectral_mix_kernel(int64_t npairs, int my, int mx, int mz, const double* __restrict__ lam, double scale,
                                                           const double2* __restrict__ in, double2* __restrict__ out) {
  constexpr int NP = P * (P + 1) / 2;
  const int64_t M = (int64_t)my * mx * mz, n = npairs * M;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t k = t / M, w = t % M;
    const int wz = (int)(w % mz), wx = (int)((w / mz) % mx), wy = (int)(w / ((int64_t)mz * mx));
    const double* l = lam + octant_index(wy, wx, wz, my, mx, mz) * NP;
    double2 x[P];
    for (int j = 0; j < P; ++j) x[j] = in[(k * P + j) * M + w];
    for (int i = 0; i < P; ++i) {
      double2 s = make_double2(0.0, 0.0);
      for (int j = 0; j < P; ++j) {
        const double lij = l[i <= j ? pair_index(i, j, P) : pair_index(j, i, P)];
        s.x += lij * x[j].x; s.y += lij * x[j].y;
      }
      out[(k * P + i) * M + w] = make_double2(scale * s.x, scale * s.y);
    }
  }
}

__global__ void __launch_bounds__(256) philox_fill_kernel(int mode, uint64_t seed, uint64_t purpose, int64_t sample0, int64_t nsamples,
                                                          int64_t elem0, int64_t nelem, uint64_t sub, double* __restrict__ out) {
  const int64_t n = nsamples * nelem;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t s = t / nelem, e = t % nelem;
    uint64_t c[4] = {(uint64_t)(elem0 + e), (uint64_t)(sample0 + s), purpose, sub};
    philox4x64_10(c, seed, 0);
    if (mode == 1) {
      uint64_t* o = reinterpret_cast<uint64_t*>(out) + t * 4;
      o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
    } else {
      double* o = out + t * 4;
      box_muller(c[0], c[1], o[0], o[1]);
      box_muller(c[2], c[3], o[2], o[3]);
    }
  }
}

bool pow2(int64_t m) { return m >= 2 && (m & (m - 1)) == 0; }

unsigned grid_of(int64_t n, int64_t cap = 4096) {
  int64_t nb = (n + 255) / 256;
  if (nb > cap) nb = cap;
  return (unsigned)(nb < 1 ? 1 : nb);
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

extern "C" int geobo_philox_fill(int mode, uint64_t seed, uint64_t purpose, int64_t sample0, int64_t nsamples, int64_t elem0,
                                 int64_t nelem, uint64_t sub, double* out, void* stream) {
  if (!out || (mode != 0 && mode != 1) || sample0 < 0 || nsamples < 0 || elem0 < 0 || nelem < 0) return GEOBO_E_ARG;
  if (!nsamples || !nelem) return GEOBO_OK;
  hipLaunchKernelGGL(philox_fill_kernel, dim3(grid_of(nsamples * nelem)), dim3(256), 0, (hipStream_t)stream, mode, seed, purpose, sample0,
                     nsamples, elem0, nelem, sub, out);
  return launched() ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_torus_table(int kernel_id, int my, int mx, int mz, double sx, double sy, double sz, double l1, double l2, double w,
                                 double amp, double* out, void* stream) {
  if (!out || !pow2(my) || !pow2(mx) || !pow2(mz) || kernel_id < GEOBO_K_EXP || kernel_id > GEOBO_K_SPARSE_X) return GEOBO_E_ARG;
  const CovParams p = make_cov(kernel_id, l1, l2, w, amp);
  hipStream_t st = (hipStream_t)stream;
  double2* o = reinterpret_cast<double2*>(out);
#define GEOBO_TT(ID) hipLaunchKernelGGL(torus_table_kernel<ID>, dim3(grid_of((int64_t)my * mx * mz)), dim3(256), 0, st, my, mx, mz, sx, sy, sz, p, o)
  COV_DISPATCH(kernel_id, GEOBO_TT);
#undef GEOBO_TT
  return launched() ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_fft_lines(int m, int64_t b1) {
  if (!pow2(m) || m > GEOBO_FFT_MAX || b1 < 1) return 0;
  int C = FFT_LDS / m;
  if (b1 > 1) {
    int c = 1;
    while (c < C && c < b1) c *= 2;
    C = c;
  }
  return C;
}

extern "C" int geobo_fft_axis(int flags, int64_t b0, int m, int64_t b1, int n_in, int n_out, const double* in, double* out, int P,
                              int64_t Q, int64_t S, void* stream) {
  if (!in || !out || !pow2(m) || m > GEOBO_FFT_MAX || b0 < 1 || b1 < 1 || n_in < 1 || n_in > m || n_out < 1 || n_out > m ||
      (flags & ~(GEOBO_FFT_INVERSE | GEOBO_FFT_IN_PAIRS | GEOBO_FFT_OUT_PAIRS)))
    return GEOBO_E_ARG;
  if ((flags & (GEOBO_FFT_IN_PAIRS | GEOBO_FFT_OUT_PAIRS)) && (P < 1 || Q < 1 || S < 1)) return GEOBO_E_ARG;
  if (in == out) return GEOBO_E_ARG;   // lines of one workgroup are another's inputs
  const int C = geobo_fft_lines(m, b1);
  const int64_t nwg = b1 == 1 ? (b0 + C - 1) / C : b0 * ((b1 + C - 1) / C);
  if (nwg > 0x7fffffff) return GEOBO_E_UNSUPPORTED;
  hipLaunchKernelGGL(fft_axis_kernel, dim3((unsigned)nwg), dim3(FFT_THREADS), 0, (hipStream_t)stream, flags, b0, m, b1, n_in, n_out, C, in,
                     out, P, Q, S);
  return launched() ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" size_t geobo_sample_factor_ws_bytes(void) { return (size_t)FACTOR_BLOCKS * 4 * sizeof(double); }

extern "C" int geobo_sample_factor(int P, int my, int mx, int mz, const double* spectra, double* F, double* lam, void* ws, size_t ws_bytes,
                                   double* status, void* stream) {
  if (!spectra || !F || !lam || !ws || !status || P < 1 || P > 3 || !pow2(my) || !pow2(mx) || !pow2(mz)) return GEOBO_E_ARG;
  if (ws_bytes < geobo_sample_factor_ws_bytes()) return GEOBO_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)(my / 2 + 1) * (mx / 2 + 1) * (mz / 2 + 1);
  const unsigned nb = grid_of(n, FACTOR_BLOCKS);
  const double2* s2 = reinterpret_cast<const double2*>(spectra);
  double* part = static_cast<double*>(ws);
  switch (P) {
    case 1: hipLaunchKernelGGL(sample_factor_kernel<1>, dim3(nb), dim3(256), 0, st, my, mx, mz, s2, F, lam, part); break;
    case 2: hipLaunchKernelGGL(sample_factor_kernel<2>, dim3(nb), dim3(256), 0, st, my, mx, mz, s2, F, lam, part); break;
    default: hipLaunchKernelGGL(sample_factor_kernel<3>, dim3(nb), dim3(256), 0, st, my, mx, mz, s2, F, lam, part); break;
  }
  if (!launched()) return GEOBO_E_LAUNCH;
  hipLaunchKernelGGL(factor_status_kernel, dim3(1), dim3(256), 0, st, part, (int)nb, status);
  return launched() ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_sample_zpass(int P, int64_t pair0, int64_t npairs, int my, int mx, int mz, int nz, const double* F, const double* noise,
                                  uint64_t seed, double* out, void* stream) {
  if (!F || !out || P < 1 || P > 3 || pair0 < 0 || npairs < 1 || !pow2(my) || !pow2(mx) || !pow2(mz) || mz > GEOBO_FFT_MAX ||
      P * mz > FFT_LDS || nz < 1 || nz > mz)
    return GEOBO_E_ARG;
  int C = 1;
  while (2 * C * P * mz <= FFT_LDS) C *= 2;
  const int64_t lines = npairs * my * mx, nwg = (lines + C - 1) / C;
  if (nwg > 0x7fffffff) return GEOBO_E_UNSUPPORTED;
  const double scale = 1.0 / sqrt((double)my * mx * mz);
  hipStream_t st = (hipStream_t)stream;
  const double2* nz2 = reinterpret_cast<const double2*>(noise);
  double2* o = reinterpret_cast<double2*>(out);
  switch (P) {
    case 1: hipLaunchKernelGGL(sample_zpass_kernel<1>, dim3((unsigned)nwg), dim3(FFT_THREADS), 0, st, pair0, npairs, my, mx, mz, nz, C, F, nz2, seed, scale, o); break;
    case 2: hipLaunchKernelGGL(sample_zpass_kernel<2>, dim3((unsigned)nwg), dim3(FFT_THREADS), 0, st, pair0, npairs, my, mx, mz, nz, C, F, nz2, seed, scale, o); break;
    default: hipLaunchKernelGGL(sample_zpass_kernel<3>, dim3((unsigned)nwg), dim3(FFT_THREADS), 0, st, pair0, npairs, my, mx, mz, nz, C, F, nz2, seed, scale, o); break;
  }
  return launched() ? GEOBO_OK : GEOBO_E_LAUNCH;
}

extern "C" int geobo_spectral_mix(int P, int64_t npairs, int my, int mx, int mz, const double* lam, double scale, const double* in, double* out,
                                  void* stream) {
  if (!lam || !in || !out || in == out || P < 1 || P > 3 || npairs < 1 || !pow2(my) || !pow2(mx) || !pow2(mz)) return GEOBO_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = grid_of(npairs * my * mx * (int64_t)mz, 8192);
  const double2* i2 = reinterpret_cast<const double2*>(in);
  double2* o2 = reinterpret_cast<double2*>(out);
  switch (P) {
    case 1: hipLaunchKernelGGL(spectral_mix_kernel<1>, dim3(nb), dim3(256), 0, st, npairs, my, mx, mz, lam, scale, i2, o2); break;
    case 2: hipLaunchKernelGGL(spectral_mix_kernel<2>, dim3(nb), dim3(256), 0, st, npairs, my, mx, mz, lam, scale, i2, o2); break;
    default: hipLaunchKernelGGL(spectral_mix_kernel<3>, dim3(nb), dim3(256), 0, st, npairs, my, mx, mz, lam, scale, i2, o2); break;
  }
  return launched() ? GEOBO_OK : GEOBO_E_LAUNCH;
}
