// potrf.hip -- blocked lower Cholesky + explicit L^-1 on gfx950 (replaces scipy.linalg.cholesky /
// solve_triangular, inversion.py:100,105,114), plus u = L^-1 y and the log-likelihood statistics
// (inversion.py:105-110).
//
// From m = 1024: ONE persistent launch, the tile DAG further down (round 5; round 6: the diagonal block's pivot tile in a row layout
// without LDS memory, and up to 40 block columns one workgroup walking the latency chain).  Below, and with schedule = GEOBO_POTRF_STREAMS, the
// stream schedule of rounds 2-4 -- right-looking, block size 128:
//   potf2_inv_kernel  one workgroup factors the 128x128 diagonal block in registers (2-D cyclic over 256 threads),
//                     carrying the inverse along by forward substitution, and writes L_kk and L_kk^-1 (the latter
//                     straight into the diagonal block of Linv);
//   panel solve       P = A[k+1:,k] * (L_kk^-1)^T           -> geobo_gemm_nt on the fp64 MFMA core (in place)
//   trailing update   A[k+1:,k+1:] -= P P^T (lower tiles)   -> geobo_gemm_nt, lower_only
// L^-1 is assembled by recursive halving, two MFMA GEMMs per merge, every node queued on a worker stream as soon as the columns of L
// it reads are final (the EAGER tree below):
//   Linv[hi,lo] = -Linv[hi,hi] * (L[hi,lo] * Linv[lo,lo]).
#include <hip/hip_runtime.h>
#include <atomic>
#include <new>
#include <stdint.h>
#include <type_traits>
#include "geobo_hip.h"
#include "lds_optin.h"

namespace {

constexpr int NB = 128;

// The 128x128 diagonal block AND the running inverse live in registers: thread (ti, tj) of a 16 x 16 grid owns the
// 2-D cyclic elements (ti + 16 p, tj + 16 q), p, q < 8.  Column step j broadcasts column j of the block and row j of
// the inverse through a double-buffered 2 KiB LDS line (ONE barrier per column), then every thread applies the
// rank-1 updates   A[i][c] -= l_i l_c  (i, c > j)   and   X[i][c] -= l_i X[j][c]  (i > j >= c)   on its registers.
// X starts as the identity, so after the last column X = L_kk^-1 (forward substitution fused into the
// factorisation).  The outer loop over 16-column groups is unrolled, so all register indices are static and the
// update ranges shrink with the group index.  (A version with the block in LDS spent ~90 % of its 0.35 ms in
// ~640 barriers and LDS round trips.)
template <int JB>
__device__ __forceinline__ void potf2_group(double (&a)[8][8], double (&x)[8][8], double (&colbuf)[2][NB],
                                            double (&rowbuf)[2][NB], int tid, int ti, int tj, int kb_global,
                                            int* __restrict__ info, bool& bad_seen) {
#pragma unroll 1
  for (int jj = 0; jj < 16; ++jj) {
    const int j = JB * 16 + jj, buf = jj & 1;
    if (tj == jj) {
#pragma unroll
      for (int p = JB; p < 8; ++p) colbuf[buf][ti + 16 * p] = a[p][JB];
    }
    if (ti == jj) {
#pragma unroll
      for (int q = 0; q <= JB; ++q) rowbuf[buf][tj + 16 * q] = x[JB][q];
    }
    __syncthreads();
    const double d = colbuf[buf][j];
    // every LDS read of the step is issued HERE, unconditionally, so that their latency runs under the pivot's reciprocal square
    // root instead of behind it (they used to sit under the predicates below: the compiler placed them after the sqrt / division
    // chain); -19 us per 128 x 128 block
    double cv[8], cc[8], xr[8];
#pragma unroll
    for (int p = JB; p < 8; ++p) cv[p] = colbuf[buf][ti + 16 * p];
#pragma unroll
    for (int q = JB; q < 8; ++q) cc[q] = colbuf[buf][tj + 16 * q];
#pragma unroll
    for (int q = 0; q <= JB; ++q) xr[q] = rowbuf[buf][tj + 16 * q];
    if (!(d > 0.0) && !bad_seen) {  // non-positive or NaN pivot: LAPACK dpotrf's info = j (1-based)
      bad_seen = true;
      if (tid == 0 && *info == 0) *info = kb_global + j + 1;
    }
    // (IEEE sqrt and division kept: a v_rsq_f64 + Newton form saves another 3 us per block, but its last-bit differences move
    //  optimize_gp's SHGO / SLSQP iterates -- forward differences with h = 1.5e-8 -- to a different point of the flat valley)
    const double r = sqrt(d);
    const double rinv = 1.0 / r;
    double li[8], lc[8], xj[8];
#pragma unroll
    for (int p = JB; p < 8; ++p) li[p] = (ti + 16 * p > j) ? cv[p] * rinv : 0.0;
#pragma unroll
    for (int q = JB; q < 8; ++q) lc[q] = (tj + 16 * q > j) ? cc[q] * rinv : 0.0;
#pragma unroll
    for (int q = 0; q <= JB; ++q) xj[q] = (tj + 16 * q <= j) ? xr[q] * rinv : 0.0;
    if (tj == jj) {  // column j of L: scaled sub-diagonal, sqrt on the diagonal
#pragma unroll
      for (int p = JB; p < 8; ++p) {
        const int i = ti + 16 * p;
        a[p][JB] = (i > j) ? li[p] : (i == j ? r : a[p][JB]);
      }
    }
    if (ti == jj) {  // row j of the inverse is final
#pragma unroll
      for (int q = 0; q <= JB; ++q) x[JB][q] = xj[q];
    }
#pragma unroll
    for (int p = JB; p < 8; ++p) {
#pragma unroll
      for (int q = JB; q < 8; ++q) a[p][q] = __builtin_fma(-li[p], lc[q], a[p][q]);
#pragma unroll
      for (int q = 0; q <= JB; ++q) x[p][q] = __builtin_fma(-li[p], xj[q], x[p][q]);
    }
  }
}

__global__ void __launch_bounds__(256) potf2_inv_kernel(double* __restrict__ A, int64_t ld, double* __restrict__ Linv,
                                                        int64_t ldi, int kb_global, int* __restrict__ info) {
  __shared__ double colbuf[2][NB], rowbuf[2][NB];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  double a[8][8], x[8][8];
#pragma unroll
  for (int p = 0; p < 8; ++p)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = ti + 16 * p, c = tj + 16 * q;
      a[p][q] = (c <= i) ? A[(int64_t)i * ld + c] : 0.0;
      x[p][q] = (c == i) ? 1.0 : 0.0;
    }
  bool bad_seen = false;
  potf2_group<0>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  potf2_group<1>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  potf2_group<2>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  potf2_group<3>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  potf2_group<4>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  potf2_group<5>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  potf2_group<6>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  potf2_group<7>(a, x, colbuf, rowbuf, tid, ti, tj, kb_global, info, bad_seen);
  // L_kk with the upper part zeroed (like scipy's lower=True result) and L_kk^-1
#pragma unroll
  for (int p = 0; p < 8; ++p)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = ti + 16 * p, c = tj + 16 * q;
      A[(int64_t)i * ld + c] = (c <= i) ? a[p][q] : 0.0;
      Linv[(int64_t)i * ldi + c] = (c <= i) ? x[p][q] : 0.0;
    }
}

// ---- blocked diagonal-block kernel (round 4) ------------------------------------------------------------------------------------
// The kernel above is 128 barrier-separated column steps (70-85 us, of which ~70 us is the floor of 128 x (barrier + LDS round trip +
// dependent sqrt / division)).  Here the 128 x 128 block is factorised in 8 steps of 16 columns, two barriers per step:
//   * the trailing matrix and the running inverse live in REGISTERS as 16 x 16 fp64 MFMA accumulator tiles (D layout), owned by
//     COLUMN: wave w of the four holds the tiles (i, c), i >= c, of columns c = w and c = w + 4 of both A and Y (12 - 2 w tiles each);
//   * step s: the owner of column s puts its tiles (i, s), i >= s, into LDS (one of two panel buffers);  barrier;
//     EVERY wave factorises and inverts the 16 x 16 pivot tile redundantly, without LDS memory or barriers (round 6: row layout, the
//     four 16-lane groups of the wave sharing the columns, partners' values through v_readlane and the LDS crossbar -- see step (2) of
//     potf2b_body);  the panel tiles L_is = A_is X_ss^T (i > s; 4 MFMAs each, spread over the waves) go back to the same
//     LDS rows and to memory;  barrier;  every wave updates its own tiles:  A_ic -= L_is L_cs^T (c > s)  and -- forward substitution
//     of the inverse fused in, as in the column kernel --  X_sc = X_ss Y_sc (c < s; its own register tile is the B operand),
//     Y_ic -= L_is X_sc (i > s, c <= s; B operand = the X_sc tile the same wave has just finished: column ownership keeps it local).
// Same recurrences as the column kernel up to summation order; the pivot's sqrt(d) and 1 / sqrt(d) come from one v_rsq_f64 seed (an
// ulp or two from the IEEE pair of the column kernel).
constexpr int PS = 17;   // LDS row stride of a 16-wide panel in doubles (conflict-free b64 fragment reads)

template <int I, int E, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (I < E) {
    f(std::integral_constant<int, I>{});
    sfor<I + 1, E>(f);
  }
}

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

// result stores of the diagonal-block kernel: plain as a kernel of its own; write-through (agent-scope relaxed atomic = `sc1`) inside
// the persistent tile-DAG kernel below, where another workgroup on another XCD reads them within the same launch
template <bool PUB>
__device__ __forceinline__ void stg(double* p, double v) {
  if constexpr (PUB) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// 1 / sqrt(d) and sqrt(d) from one v_rsq_f64 seed y (good to ~ 2^-26): ONE third-order step, y (1 + e / 2 + 3 e^2 / 8) with
// e = 1 - d y^2 -- four dependent operations where the coupled Newton form needs ten and the IEEE sqrt + division about thirty (the
// reciprocal is what the column step's chain waits for); sqrt(d) = d y' with one residual correction, off that chain.  Both within an ulp
// or two of the IEEE pair.  d <= 0 or NaN gives NaN (the caller raises info).
__device__ __forceinline__ void rsqrt_pair(double d, double& rt, double& rinv) {
  const double y = __builtin_amdgcn_rsq(d);
  const double t = d * y;
  const double e = __builtin_fma(-t, y, 1.0);
  const double p = __builtin_fma(0.375, e, 0.5), q = y * e;
  const double ri = __builtin_fma(q, p, y);
  double g = d * ri;
  g = __builtin_fma(__builtin_fma(-g, g, d), 0.5 * ri, g);
  rt = g;
  rinv = ri;
}

// v of the lane whose byte index (4 x lane) is given: the LDS crossbar, no memory access
__device__ __forceinline__ double bperm(double v, int byte_lane) {
  const int lo = __builtin_amdgcn_ds_bpermute(byte_lane, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(byte_lane, __double2hiint(v));
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double rdlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// number of tiles wave W owns per matrix, and the (i, c) of its slot q: columns W (rows W..7) then W + 4 (rows W+4..7)
template <int W> struct Own {
  static constexpr int N0 = 8 - W, N1 = 4 - W, NT = N0 + N1;
  static constexpr int row(int q) { return q < N0 ? W + q : W + 4 + (q - N0); }
  static constexpr int col(int q) { return q < N0 ? W : W + 4; }
  static constexpr int slot(int i, int c) { return c == W ? i - W : N0 + (i - W - 4); }   // valid for c in {W, W+4}, i >= c
};

template <int W, bool PUB>
__device__ __forceinline__ void potf2b_body(double* __restrict__ A, int64_t ld, double* __restrict__ Linv, int64_t ldi, int kb_global,
                                            int* __restrict__ info, double (&pan)[2][NB][PS], double (&xss)[4][16][PS]) {
  using O = Own<W>;
  constexpr int NT = O::NT;
  const int lane = threadIdx.x & 63, lr = lane & 15, q4 = lane >> 4;
  v4d a[NT], y[NT];
  // ---- load: tile (i, c) element (16 i + q4 + 4 r, 16 c + lr); strictly upper entries of the diagonal tiles are not part of the matrix
  sfor<0, NT>([&](auto qq) {
    constexpr int q = decltype(qq)::value, i = O::row(q), c = O::col(q);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * i + q4 + 4 * r, col = 16 * c + lr;
      a[q][r] = (col <= row) ? A[(int64_t)row * ld + col] : 0.0;
      y[q][r] = (col == row) ? 1.0 : 0.0;
    }
  });
  bool bad_seen = false;
  sfor<0, 8>([&](auto ss) {
    constexpr int s = decltype(ss)::value, buf = s & 1;
    // (1) the owner of column s publishes its tiles (i, s), i >= s
    if constexpr (s % 4 == W) {
      sfor<s, 8>([&](auto ii) {
        constexpr int i = decltype(ii)::value, q = O::slot(i, s);
#pragma unroll
        for (int r = 0; r < 4; ++r) pan[buf][16 * i + q4 + 4 * r][lr] = a[q][r];
      });
    }
    __syncthreads();
    // (2) pivot tile, redundantly in every wave.
    // ROW layout (round 6), the four 16-lane groups of the wave sharing the columns -- lane (g, i) = 16 g + i holds the entries
    // T_i[4 k + g], k < 4, of row i of the tile and the same entries of the running inverse: 2 x 4 registers, every lane does a quarter of
    // a row's updates (the accumulator-layout pivot of round 4 went through two LDS round trips and ~ 100 instructions per column step, the
    // same count as a row-per-lane form in which the four groups repeat each other: 250 ns per column, 128 columns per diagonal block,
    // on the chain of the whole factorisation).  Column step j: the pivot out of lane (j % 4, j) by v_readlane; 1 / sqrt(d) from
    // v_rsq_f64 (one third-order step: no IEEE sqrt, no division); the scaled column j, which lives in group j % 4,
    // reaches every lane that needs an entry of it -- its own row's l_ij, and l_cj for the columns c it holds -- by ds_bpermute (the LDS
    // crossbar: no memory, no barrier); rows of the inverse are kept UNSCALED (Y_j, with X_j = Y_j / l_jj applied once at the end), so a
    // step's inverse update is one fused multiply-add per held column against Y_j[c] fetched from lane (g, j).
    const int g4 = q4, byte_i = 4 * lr, byte_g = 64 * q4;
    double T[4], Yr[4], rinv_mine = 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      T[k] = pan[buf][16 * s + lr][4 * k + g4];
      Yr[k] = (4 * k + g4 == lr) ? 1.0 : 0.0;
    }
    // Software-pipelined: the step's crossbar fetches are issued first, and while they are in flight the pivot of the NEXT column is
    // formed beside them instead of being fetched back through the updates -- d_{j+1} = t - l^2 with t, the entry (j+1, j+1) as the
    // previous step left it (read ahead by v_readlane), and l = l_{j+1,j} read out of the scaled column the same way: the same fused
    // multiply-add the owning lane applies to its own copy (identical bits) -- and its reciprocal square root is taken.  What remains on
    // the loop-carried chain is scale -> crossbar -> one multiply-add.  A non-positive / NaN pivot is recorded without a branch and raised
    // after the tile.
    double d = rdlane(T[0], 0);
    int badj = (d > 0.0) ? -1 : 0;
    double rt, rinv;
    rsqrt_pair(d, rt, rinv);
    double tn = rdlane(T[0], 17);                              // entry (1, 1)
    sfor<0, 16>([&](auto jj) {
      constexpr int j = decltype(jj)::value, gj = j % 4, kj = j / 4;
      const double lsrc = (lr > j) ? T[kj] * rinv : 0.0;       // column j below the diagonal, scaled (meaningful in group gj; 0 in the rows <= j)
      const double li = bperm(lsrc, 64 * gj + byte_i);         // l_ij of this lane's row
      double lc[4], yj[4];
      sfor<kj, 4>([&](auto kk) {                               // l_cj of the held column c = 4 k + g (0 for c <= j: the update is a no-op there)
        constexpr int k = decltype(kk)::value;
        lc[k] = bperm(lsrc, 64 * gj + 16 * k + 4 * g4);
      });
      sfor<0, kj + 1>([&](auto kk) {                           // Y_jc of the held columns (c > j: zero)
        constexpr int k = decltype(kk)::value;
        yj[k] = bperm(Yr[k], byte_g + 4 * j);
      });
      double rt_n = rt, rinv_n = rinv;
      if constexpr (j < 15) {
        const double ln = rdlane(lsrc, 16 * gj + j + 1);
        d = __builtin_fma(-ln, ln, tn);
        badj = (badj < 0 && !(d > 0.0)) ? j + 1 : badj;
        rsqrt_pair(d, rt_n, rinv_n);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (g4 == gj) T[kj] = (lr == j) ? rt : lsrc;             // column j is final (rows < j: above the diagonal, zero)
      sfor<kj, 4>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        T[k] = __builtin_fma(-li, lc[k], T[k]);
      });
      const double li2 = li * rinv;
      sfor<0, kj + 1>([&](auto kk) {
        constexpr int k = decltype(kk)::value;
        Yr[k] = __builtin_fma(-li2, yj[k], Yr[k]);             // Y_ic -= l_ij / l_jj Y_jc  (rows <= j: l = 0)
      });
      rinv_mine = (lr == j) ? rinv : rinv_mine;
      if constexpr (j < 14) tn = rdlane(T[(j + 2) / 4], 16 * ((j + 2) % 4) + j + 2);
      rt = rt_n;
      rinv = rinv_n;
    });
    if (badj >= 0 && !bad_seen) {      // non-positive or NaN pivot: LAPACK dpotrf's info (1-based), the first one wins
      bad_seen = true;
      if (threadIdx.x == 0 && *info == 0) *info = kb_global + 16 * s + badj + 1;
    }
    // back to the accumulator (D) layout through this wave's own 16 x 16 LDS tile (wave-local: program order, no barrier)
    double xt[4];
    if constexpr (s % 4 == W) {                                // L_ss to memory (upper part zero) by the column's owner
#pragma unroll
      for (int k = 0; k < 4; ++k) xss[W][lr][4 * k + g4] = T[k];
      __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        stg<PUB>(A + (int64_t)(16 * s + q4 + 4 * r) * ld + 16 * s + lr, (lr <= q4 + 4 * r) ? xss[W][q4 + 4 * r][lr] : 0.0);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) xss[W][lr][4 * k + g4] = Yr[k] * rinv_mine;     // row-major X_ss, this wave's own copy
    __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll
    for (int r = 0; r < 4; ++r) xt[r] = xss[W][q4 + 4 * r][lr];
    __builtin_amdgcn_s_waitcnt(0xc07f);                        // lgkmcnt(0): this wave's xss copy is written (wave-local: no barrier)
    // MFMA fragments of X_ss: A[i = lr][k = 4 t + q4] (also B[k][j] = X_ss^T: the same addresses)
    double xf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) xf[t] = xss[W][lr][4 * t + q4];
    // (3) X row block s: X_sc = X_ss Y_sc for the own columns c < s; the diagonal tile is X_ss itself
    sfor<0, 2>([&](auto hh) {
      constexpr int c = W + 4 * decltype(hh)::value;
      if constexpr (c < s) {
        constexpr int q = O::slot(s, c);
        v4d acc = (v4d){0., 0., 0., 0.};
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xf[t], y[q][t], acc, 0, 0, 0);
        y[q] = acc;
      } else if constexpr (c == s) {
        constexpr int q = O::slot(s, s);
#pragma unroll
        for (int r = 0; r < 4; ++r) y[q][r] = xt[r];
      }
    });
    // (4) panel tiles L_is = A_is X_ss^T for i > s, i = W (mod 4): back into the panel rows and to memory
    sfor<s + 1, 8>([&](auto ii) {
      constexpr int i = decltype(ii)::value;
      if constexpr (i % 4 == W) {
        v4d acc = (v4d){0., 0., 0., 0.};
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pan[buf][16 * i + lr][4 * t + q4], xf[t], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pan[buf][16 * i + q4 + 4 * r][lr] = acc[r];
          stg<PUB>(A + (int64_t)(16 * i + q4 + 4 * r) * ld + 16 * s + lr, acc[r]);
        }
      }
    });
    if constexpr (s < 7) {
      __syncthreads();
      // (5) updates of the own tiles
      sfor<0, NT>([&](auto qq) {
        constexpr int q = decltype(qq)::value, i = O::row(q), c = O::col(q);
        if constexpr (i > s) {
          double li[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) li[t] = -pan[buf][16 * i + lr][4 * t + q4];
          if constexpr (c > s) {                               // A_ic -= L_is L_cs^T
#pragma unroll
            for (int t = 0; t < 4; ++t) a[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(li[t], pan[buf][16 * c + lr][4 * t + q4], a[q], 0, 0, 0);
          } else {                                             // Y_ic -= L_is X_sc   (X_sc: this wave's finished tile of row block s)
            constexpr int qs = O::slot(s, c);
#pragma unroll
            for (int t = 0; t < 4; ++t) y[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(li[t], y[qs][t], y[q], 0, 0, 0);
          }
        }
      });
    }
  });
  // ---- L^-1 tiles to memory (the lower tiles; Linv was zeroed by the caller), zeros into the strictly upper tiles of L ------------
  sfor<0, NT>([&](auto qq) {
    constexpr int q = decltype(qq)::value, i = O::row(q), c = O::col(q);
#pragma unroll
    for (int r = 0; r < 4; ++r) stg<PUB>(Linv + (int64_t)(16 * i + q4 + 4 * r) * ldi + 16 * c + lr, y[q][r]);
    if constexpr (i > c) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // mirror tile (c, i): strictly above the diagonal.  Inside the tile DAG the zeros of D_j ARE read by other workgroups (the
        // whole 128 x 128 tile is the operand of L_ij = S D_j^T): published like the rest; the zeros of L_jj are read by no one
        A[(int64_t)(16 * c + q4 + 4 * r) * ld + 16 * i + lr] = 0.0;
        stg<PUB>(Linv + (int64_t)(16 * c + q4 + 4 * r) * ldi + 16 * i + lr, 0.0);
      }
    }
  });
}

__global__ void __launch_bounds__(256) potf2b_inv_kernel(double* __restrict__ A, int64_t ld, double* __restrict__ Linv, int64_t ldi,
                                                         int kb_global, int* __restrict__ info) {
  __shared__ double pan[2][NB][PS];
  __shared__ double xss[4][16][PS];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  switch (w) {     // four specialisations: the tile lists differ per wave, every register index is static; all hit the same barriers
    case 0: potf2b_body<0, false>(A, ld, Linv, ldi, kb_global, info, pan, xss); break;
    case 1: potf2b_body<1, false>(A, ld, Linv, ldi, kb_global, info, pan, xss); break;
    case 2: potf2b_body<2, false>(A, ld, Linv, ldi, kb_global, info, pan, xss); break;
    default: potf2b_body<3, false>(A, ld, Linv, ldi, kb_global, info, pan, xss); break;
  }
}

// ---- persistent tile-DAG factorisation + inverse (round 5) ------------------------------------------------------------------------
// ONE launch, one 256-thread workgroup per CU, no host-side schedule: the 128 x 128 tiles of L and of X = L^-1 are tasks of a
// dependency graph, drawn IN ORDER from one global counter (a task only ever depends on tasks with a smaller index, so whatever is
// claimed can always finish: no residency assumption, no deadlock), synchronised through agent-scope counters in global memory.
//   Cholesky tile (i, j), i >= j  (LEFT-looking: the tile is accumulated in registers over the whole contraction, C is touched once
//   instead of once per 128 columns -- the rank-128 trailing updates of the stream schedule moved 16 flop per byte of C):
//       S = A_ij - sum_{k<j} L_ik L_jk^T ;   i == j:  L_jj = chol(S), D_j = L_jj^-1 (potf2b_body) ;   i > j:  L_ij = S D_j^T
//   inverse tile (i, c), c < i  (forward substitution by block rows, so that row i of X follows row i of L):
//       X_ic = -D_i sum_{k=c}^{i-1} L_ik X_kc ,   X_cc = D_c
// A task waits (one lane polls, relaxed agent-scope loads + s_sleep; one agent-scope acquire after the match; barrier) only where its
// next 128 columns of the contraction are not final yet, runs the contraction over everything that is (LDS-DMA ring + fp64 MFMA, as in
// gemm_f64.hip), and publishes its tile with write-through stores, a per-wave vmcnt(0) drain, a barrier and ONE flag store
// (MI355X_MICROARCH.md "inter-workgroup visibility", form R1).  Task order: column step s = the tiles (s..nb-1, s) of L, diagonal first,
// then row s - XD of X (its inputs were final XD steps ago: filler work under the latency chain diag -> sub-diagonal tile -> next diag).
// Summation order is fixed by the tile, not by timing: bit-reproducible.  Every spin is bounded (abort flag + wall-clock limit).
constexpr int DBK = 16, DXS = 16, DNST = 4;   // (the task loop's segments rotate three stages; the walker's use four)
constexpr int DXBUF = NB * DXS;                  // X chunk [128 rows][16 k], 128-byte rows, XOR-swizzled 16-byte slots
constexpr int DYS_NN = NB + 4;                   // row stride of a [16 k][128 cols] chunk (the X_kc operand of the inverse tiles)
constexpr int DYBUF = DBK * DYS_NN;              // >= NB * DXS: also holds a [128 cols][16 k] chunk
constexpr int DSTAGE = DXBUF + DYBUF;
constexpr int DAG_LDS_DOUBLES = DNST * DSTAGE;   // 133 120 bytes: one workgroup per CU
constexpr size_t DAG_LDS_BYTES = (size_t)DAG_LDS_DOUBLES * sizeof(double) + 64;
constexpr int DAG_CTL = 16;                      // control words in front of the counters: [0] task head, [1] abort
constexpr int DAG_XDELAY = 6;

// -DGEOBO_DAG_TRACE (tools/potrf_dag_trace.py builds it): every task logs 8 x int64 behind the counters --
// [0] (type << 40 | i << 20 | j), [1] workgroup << 8 | XCC, [2] claimed, [3] contraction complete, [4] last dependency seen,
// [5] published (100 MHz wall clock), [6] ticks spent polling, [7] segments run
#ifdef GEOBO_DAG_TRACE
#define DAG_T(slot, val) do { if (threadIdx.x == 0) trace[(slot)] = (val); } while (0)
#define DAG_NOW() ((long long)wall_clock64())
#else
#define DAG_T(slot, val) do { } while (0)
#define DAG_NOW() 0ll
#endif

struct DagArgs {
  double* A; int64_t ld; double* Linv; int64_t ldi; int* info;
  int* ctl;          // [0] head, [1] abort, [DAG_CTL .. +nb) rows of L final up to (count), then nb x nb flags of X, then 2 nb flags of the parked tiles
  int nb, xdelay;
};

__device__ __forceinline__ int dswz(int row) {
  const int p = (row >> 1) & 7;
  return (p & 1) | (((p >> 2) & 1) * 6);
}
__device__ __forceinline__ int ld_flag(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_flag(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// bounded spin of ONE lane: true = give up (someone aborted, or this lane did after ~4 s of wall clock: 100 MHz counter)
struct Spin {
  unsigned n = 0; uint64_t t0 = 0;
  __device__ __forceinline__ bool fail(int* ctl, int* info) {
    __builtin_amdgcn_s_sleep(4);
    if ((++n & 255u) != 0) return false;
    if (ld_flag(ctl + 1)) return true;
    const uint64_t t = wall_clock64();
    if (t0 == 0) { t0 = t; return false; }
    if (t - t0 < 400000000ull) return false;
    st_flag(ctl + 1, 1);
    if (*info == 0) *info = -7;
    return true;
  }
};

// acc += X[128 rows][klen] * Y^T (NT: Y [128 cols][klen], both k-contiguous) or X * Y (NN: Y [klen][128 cols]); klen % 16 == 0.
// The 3-stage LDS-DMA ring and the fragment rotation of gemm_f64.hip, 2 x 2 waves of 64 x 64.
template <bool NN>
__device__ __forceinline__ void dag_segment(v4d (&acc)[4][4], const double* Xp, int64_t ldx, const double* Yp, int64_t ldy, int klen,
                                            double* smem) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* glb_ptr_t;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lg = lane >> 4, srow = tid >> 3;
  const char* const Xb = reinterpret_cast<const char*>(Xp);
  const char* const Yb = reinterpret_cast<const char*>(Yp);
  int64_t xsrc[4], ysrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 32 + srow;
    xsrc[i] = ((int64_t)row * ldx + 2 * ((tid & 7) ^ dswz(row))) * 8;
    ysrc[i] = NN ? ((int64_t)(i * 4 + wave) * ldy + 2 * lane) * 8 : ((int64_t)row * ldy + 2 * ((tid & 7) ^ dswz(row))) * 8;
  }
  auto stage = [&](int k0, int st) {
    double* const xs = smem + st * DSTAGE;
    double* const ys = xs + DXBUF;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(Xb + xsrc[i] + (int64_t)k0 * 8), (lds_ptr_t)(xs + (i * 32 + wave * 8) * DXS), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (NN)
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(Yb + ysrc[i] + (int64_t)k0 * ldy * 8), (lds_ptr_t)(ys + (i * 4 + wave) * DYS_NN), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((glb_ptr_t)(Yb + ysrc[i] + (int64_t)k0 * 8), (lds_ptr_t)(ys + (i * 32 + wave * 8) * DXS), 16, 0, 0);
    }
  };
  const int xoff0 = 2 * ((2 * lg + 0) ^ dswz(lr)), xoff1 = 2 * ((2 * lg + 1) ^ dswz(lr));
  const double* const xfrag = smem + (wm * 64 + lr) * DXS;
  const double* const yfrag = smem + DXBUF + (NN ? (wn * 64 + lr) : (wn * 64 + lr) * DXS);
  auto read_half = [&](int st, int h, v2d (&av)[4], v2d (&bv)[4]) {
    const double* xb = xfrag + st * DSTAGE + (h ? xoff1 : xoff0);
#pragma unroll
    for (int m = 0; m < 4; ++m) av[m] = *reinterpret_cast<const v2d*>(xb + m * 16 * DXS);
    if constexpr (NN) {
      const double* yb = yfrag + st * DSTAGE + (4 * lg + 2 * h) * DYS_NN;
#pragma unroll
      for (int n = 0; n < 4; ++n) { bv[n][0] = yb[n * 16]; bv[n][1] = yb[DYS_NN + n * 16]; }
    } else {
      const double* yb = yfrag + st * DSTAGE + (h ? xoff1 : xoff0);
#pragma unroll
      for (int n = 0; n < 4; ++n) bv[n] = *reinterpret_cast<const v2d*>(yb + n * 16 * DXS);
    }
  };
  stage(0, 0);
  stage(klen > DBK ? DBK : 0, 1);
  __syncthreads();
  int s0 = 0, s1 = 1, s2 = 2;
  v2d a0[4], b0[4], a1[4], b1[4];
  read_half(0, 0, a0, b0);
  for (int k0 = 0; k0 < klen; k0 += DBK) {
    int kn = k0 + 2 * DBK;
    if (kn >= klen) kn = klen - DBK;          // the tail re-stages the last chunk instead of branching
    stage(kn, s2);
    read_half(s0, 1, a1, b1);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t == 2) read_half(s1, 0, a0, b0);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(t < 2 ? a0[m][t & 1] : a1[m][t & 1], t < 2 ? b0[n][t & 1] : b1[n][t & 1],
                                                           acc[m][n], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x126, 4, 0);
    }
    __syncthreads();
    const int ts = s0; s0 = s1; s1 = s2; s2 = ts;
  }
}

// tile <-> accumulators (D layout of v_mfma_f64_16x16x4: col = lane & 15, row = (lane >> 4) + 4 reg)
template <bool PUB>
__device__ __forceinline__ void dag_store(const v4d (&acc)[4][4], double* T, int64_t ld, double sgn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* const tw = T + (int64_t)((wave >> 1) * 64 + (lane >> 4)) * ld + (wave & 1) * 64 + (lane & 15);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) stg<PUB>(tw + (int64_t)(m * 16 + 4 * r) * ld + n * 16, sgn * acc[m][n][r]);
}
__device__ __forceinline__ void dag_load_neg(v4d (&acc)[4][4], const double* T, int64_t ld) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* const tw = T + (int64_t)((wave >> 1) * 64 + (lane >> 4)) * ld + (wave & 1) * 64 + (lane & 15);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[m][n][r] = -tw[(int64_t)(m * 16 + 4 * r) * ld + n * 16];
}
// ---- the chain in ONE workgroup (round 6, second half) -----------------------------------------------------------------------------
// Task log of the round-5 DAG: a column's chain is diag (44 us) -> hand-off -> L_{j+1,j} = S D_j^T (22) -> hand-off -> last update of
// the next diagonal tile (22); halving the MFMAs of the two tile products changed the launch by 1.3 %: the links wait for a tile another
// XCD has just published, chunk by chunk (NOTES.md section 14).  Now workgroup 0 WALKS the chain and never hands off: it factorises
// S_jj, forms L_{j+1,j} with D_j still in its own L2, publishes it, applies it to the next diagonal tile itself, factorises again.  What
// it needs from others are two PARKED partial sums per column -- S_{j+1,j} (all k < j) and S_{j+1,j+1} (all k < j) -- which the former
// sub-diagonal and diagonal tasks now park and flag instead of waiting for D_j; their inputs are final one column earlier, so the tiles
// are old by the time the walker reads them.  Everything else (the tiles (i >= j + 2, j), the rows of X) is unchanged.  (The same
// four-stage counted-wait ring in the task loop's segments was measured and is NOT used there: 8448 8.64 -> 9.09 ms -- their chunks are
// not latency-bound, and the hand-scheduled fragment prefetch of dag_segment is worth more than the depth.)  No new wait
// cycle: the walker at column j waits for helpers whose inputs are tiles of columns < j, published by ordinary tasks that wait for D_k,
// k < j, which the walker has already published.  Needs a second resident workgroup (grids of one keep the round-5 roles).
// With the latency gone the two products are bound by their MFMAs (13.7 us each on one CU), and both are half empty:
//   * L_{j+1,j} = S D_j^T: D_j is lower triangular -- the 16-deep chunk kc only reaches the 16-column tiles ct >= kc; the column tiles
//     are dealt {0, 1, 6, 7} | {2, 3, 4, 5} to the two wave columns (18 of 32 chunk-tiles each instead of 10 | 26);
//   * the diagonal tile is only read below its diagonal (potf2b_body loads col <= row): its 36 lower 16 x 16 tiles are dealt
//     10 | 8 | 8 | 10 to the waves for the walker's update.
// A map names the tiles of a wave's accumulators: acc[m][n] = tile (rb + m, ct[n]), bit 4 m + n of `act` set where it exists.  Staging
// and barriers are those of dag_segment (every wave stages, every wave meets): only MFMAs are skipped.
#ifndef DAG_WALKER
#define DAG_WALKER 1     // 0: the round-5 roles (every link of the chain a task of its own): the A/B
#endif
// The walker pays where the launch is chain-bound: M = 1024 0.81 -> 0.77 ms, 2048 1.72 -> 1.54, 4224 3.55 -> 3.40.  From ~ 40 block
// columns the middle of the factorisation is work-bound, the parked sums arrive late (the walker waited 21 us per column for the diagonal
// tile's at M = 8448) and a workgroup that does not take tiles is missed: 8448 8.58 -> 8.64 ms, 16 640 48.1 -> 48.9.  Larger matrices
// keep the round-5 roles.
#ifndef DAG_WALK_NB
#define DAG_WALK_NB 40
#endif
struct DagMap { int rb, ct[4]; unsigned act; };
__device__ __forceinline__ DagMap dag_map_tri(int wave) {      // L = S D^T
  const int wm = wave >> 1, wn = wave & 1;
  return wn ? DagMap{4 * wm, {2, 3, 4, 5}, 0xFFFFu} : DagMap{4 * wm, {0, 1, 6, 7}, 0xFFFFu};
}
__device__ __forceinline__ DagMap dag_map_lower(int wave) {    // the lower tiles of a diagonal tile (m >= n: 0xF731; m < 2: 0x00FF)
  switch (wave) {
    case 0: return DagMap{0, {0, 1, 2, 3}, 0xF731u};
    case 1: return DagMap{4, {0, 1, 2, 3}, 0x00FFu};
    case 2: return DagMap{6, {0, 1, 2, 3}, 0x00FFu};
    default: return DagMap{4, {4, 5, 6, 7}, 0xF731u};
  }
}
// NT segment on a map; TRI: Y is lower triangular
template <bool TRI>
__device__ __forceinline__ void dag_segment_map(v4d (&acc)[4][4], const double* Xp, int64_t ldx, const double* Yp, int64_t ldy, int klen,
                                                double* smem, const DagMap& mp) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* glb_ptr_t;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4, srow = tid >> 3;
  const char* const Xb = reinterpret_cast<const char*>(Xp);
  const char* const Yb = reinterpret_cast<const char*>(Yp);
  int64_t xsrc[4], ysrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 32 + srow;
    xsrc[i] = ((int64_t)row * ldx + 2 * ((tid & 7) ^ dswz(row))) * 8;
    ysrc[i] = ((int64_t)row * ldy + 2 * ((tid & 7) ^ dswz(row))) * 8;
  }
  auto stage = [&](int k0, int st) {
    double* const xs = smem + st * DSTAGE;
    double* const ys = xs + DXBUF;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(Xb + xsrc[i] + (int64_t)k0 * 8), (lds_ptr_t)(xs + (i * 32 + wave * 8) * DXS), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(Yb + ysrc[i] + (int64_t)k0 * 8), (lds_ptr_t)(ys + (i * 32 + wave * 8) * DXS), 16, 0, 0);
  };
  const int xoff0 = 2 * ((2 * lg + 0) ^ dswz(lr)), xoff1 = 2 * ((2 * lg + 1) ^ dswz(lr));
  const double* const xfrag = smem + (mp.rb * 16 + lr) * DXS;
  const double* const yfrag = smem + DXBUF + lr * DXS;
  auto read_half = [&](int st, int h, v2d (&av)[4], v2d (&bv)[4]) {
    const double* xb = xfrag + st * DSTAGE + (h ? xoff1 : xoff0);
#pragma unroll
    for (int m = 0; m < 4; ++m) av[m] = *reinterpret_cast<const v2d*>(xb + m * 16 * DXS);
    const double* yb = yfrag + st * DSTAGE + (h ? xoff1 : xoff0);
#pragma unroll
    for (int n = 0; n < 4; ++n) bv[n] = *reinterpret_cast<const v2d*>(yb + mp.ct[n] * 16 * DXS);
  };
  // FOUR stages, three chunks in flight, counted waits (the walker's segments read tiles that an acquire has just pushed out of this
  // XCD's caches: ~ 2.5 us per access; with the task loop's ring -- every chunk barrier a full drain, __syncthreads -- each of the
  // eight chunks of a 128-deep product waited that long: 20-27 us per product, measured per phase).  klen = 8 chunks exactly.
  static_assert(DNST >= 4, "stages");
  stage(0, 0);
  stage(DBK, 1);
  stage(2 * DBK, 2);
  sfor<0, NB / DBK>([&](auto cc) {
    constexpr int c = decltype(cc)::value, NCH = NB / DBK;
    constexpr int after = (NCH - 1 - c) < 2 ? (NCH - 1 - c) : 2;        // stages issued behind chunk c that may stay in flight
    // chunk c has landed (this wave's part; the barrier covers the others'), and every wave is past its reads of chunk c - 1
    if constexpr (after == 2) asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else if constexpr (after == 1) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if constexpr (c + 3 < NCH) stage((c + 3) * DBK, (c + 3) % 4);        // into the slot chunk c - 1 has just left
    v2d a0[4], b0[4], a1[4], b1[4];
    read_half(c % 4, 0, a0, b0);
    read_half(c % 4, 1, a1, b1);
    unsigned on = mp.act;
    if constexpr (TRI) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (c > mp.ct[n]) on &= ~(0x1111u << n);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          if (on & (1u << (4 * m + n)))
            acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(t < 2 ? a0[m][t & 1] : a1[m][t & 1], t < 2 ? b0[n][t & 1] : b1[n][t & 1],
                                                             acc[m][n], 0, 0, 0);
    }
  });
  __syncthreads();                                                      // (the ring is free for whoever stages next)
}
template <bool PUB>
__device__ __forceinline__ void dag_store_map(const v4d (&acc)[4][4], double* T, int64_t ld, double sgn, const DagMap& mp) {
  const int lane = threadIdx.x & 63;
  double* const tw = T + (int64_t)(mp.rb * 16 + (lane >> 4)) * ld + (lane & 15);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
      if (mp.act & (1u << (4 * m + n))) {
#pragma unroll
        for (int r = 0; r < 4; ++r) stg<PUB>(tw + (int64_t)(m * 16 + 4 * r) * ld + mp.ct[n] * 16, sgn * acc[m][n][r]);
      }
}
__device__ __forceinline__ void dag_load_neg_map(v4d (&acc)[4][4], const double* T, int64_t ld, const DagMap& mp) {
  const int lane = threadIdx.x & 63;
  const double* const tw = T + (int64_t)(mp.rb * 16 + (lane >> 4)) * ld + (lane & 15);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[m][n][r] = (mp.act & (1u << (4 * m + n))) ? -tw[(int64_t)(m * 16 + 4 * r) * ld + mp.ct[n] * 16] : 0.0;
}
__device__ __forceinline__ void dag_zero(v4d (&acc)[4][4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = (v4d){0., 0., 0., 0.};
}
// every wave has stored write-through: drain, meet, ONE flag store
__device__ __forceinline__ void dag_publish(int* flag, int value) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) st_flag(flag, value);
}
// broadcast of a value found by thread 0 (which has also issued the agent-scope acquire): all threads return it
// (round-5 advisory: EVERY wave issues its own agent-scope acquire behind the broadcast barrier -- one buffer_inv per wave -- instead of
// relying on thread 0's invalidate covering the whole CU, which holds on gfx942 / gfx950 (the vector L1 is per CU) but is outside the
// HIP memory model.  The producer side stays what MI355X_MICROARCH.md's form R1 prescribes: write-through tile stores, per-wave
// vmcnt(0), barrier, one relaxed flag store -- an agent-scope RELEASE there would add an L2 write-back to every hand-off of the chain.)
__device__ __forceinline__ int dag_bcast(int* sh, int v) {
  if (threadIdx.x == 0) sh[0] = v;
  __syncthreads();
  const int r = sh[0];
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __syncthreads();
  return r;
}

// the diagonal block as a function of its own: inlined into the task loop its 230 + 100 registers (four wave specialisations) spilled
// (640 scratch accesses on the latency chain: 135 us per block instead of 49)
__device__ __noinline__ void potf2b_dag(double* T, int64_t ld, double* D, int64_t ldi, int kb_global, int* info, double* smem) {
  double (&pan)[2][NB][PS] = *reinterpret_cast<double (*)[2][NB][PS]>(smem);
  double (&xss)[4][16][PS] = *reinterpret_cast<double (*)[4][16][PS]>(smem + 2 * NB * PS);
  switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {
    case 0: potf2b_body<0, true>(T, ld, D, ldi, kb_global, info, pan, xss); break;
    case 1: potf2b_body<1, true>(T, ld, D, ldi, kb_global, info, pan, xss); break;
    case 2: potf2b_body<2, true>(T, ld, D, ldi, kb_global, info, pan, xss); break;
    default: potf2b_body<3, true>(T, ld, D, ldi, kb_global, info, pan, xss); break;
  }
}

// the chain walker as a function of its own (inlined into the task loop it raised the kernel's spills from 38 to 101 registers)
__device__ __noinline__ bool dag_walk(const DagArgs& a, double* smem) {
  int* const sh = reinterpret_cast<int*>(smem + DAG_LDS_DOUBLES);
  int* const ready = a.ctl + DAG_CTL;
  const int nb = a.nb, tid = threadIdx.x;
  int* const pd = ready + nb + (int64_t)nb * nb;
  int* const pl = pd + nb;
  v4d acc[4][4];
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const DagMap mlow = dag_map_lower(wv), mtri = dag_map_tri(wv);
  auto wait_flag = [&](const int* f) {
    int ok = 1;
    if (tid == 0) {
      Spin sp;
      while (ld_flag(f) < 1)
        if (sp.fail(a.ctl, a.info)) { ok = 0; break; }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    return dag_bcast(sh, ok);
  };
#ifdef DAG_WALK_STATS
  long long ws_t[6] = {0, 0, 0, 0, 0, 0};
#define WS_MARK(i) do { const long long n_ = (long long)wall_clock64(); ws_t[i] += n_ - ws_last; ws_last = n_; } while (0)
  long long ws_last = (long long)wall_clock64();
#else
#define WS_MARK(i) do { } while (0)
#endif
  for (int s = 0; s < nb; ++s) {
    double* const Tss = a.A + (int64_t)s * NB * a.ld + (int64_t)s * NB;
    double* const Ds = a.Linv + (int64_t)s * NB * a.ldi + (int64_t)s * NB;
    // S_ss is complete and visible here (s = 0: the input; else stored below behind vmcnt(0), a fence and a barrier)
    potf2b_dag(Tss, a.ld, Ds, a.ldi, s * NB, a.info, smem);
    dag_publish(ready + s, s + 1);
    WS_MARK(0);
    if (s + 1 == nb) break;
    double* const Tl = a.A + (int64_t)(s + 1) * NB * a.ld + (int64_t)s * NB;          // tile (s + 1, s)
    double* const Tn = a.A + (int64_t)(s + 1) * NB * a.ld + (int64_t)(s + 1) * NB;    // tile (s + 1, s + 1)
    if (!wait_flag(pl + s + 1)) return false;
    WS_MARK(1);
    dag_zero(acc);
    dag_segment_map<true>(acc, Tl, a.ld, Ds, a.ldi, NB, smem, mtri);                   // L_{s+1,s} = S D_s^T
    dag_store_map<true>(acc, Tl, a.ld, 1.0, mtri);
    dag_publish(ready + s + 1, s + 1);
    WS_MARK(2);
    if (!wait_flag(pd + s + 1)) return false;
    WS_MARK(3);
    dag_load_neg_map(acc, Tn, a.ld, mlow);
    dag_segment_map<false>(acc, Tl, a.ld, Tl, a.ld, NB, smem, mlow);                   // ... + L_{s+1,s} L_{s+1,s}^T, lower tiles
    dag_store_map<false>(acc, Tn, a.ld, -1.0, mlow);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __syncthreads();
    WS_MARK(4);
  }
#ifdef DAG_WALK_STATS
  if (tid == 0) for (int q = 0; q < 5; ++q) a.ctl[2 + q] = (int)ws_t[q];
#endif
  return true;
}

// WALK: the chain walker's roles (chosen at launch: <= DAG_WALK_NB block columns and a second workgroup); false = exactly the round-5 kernel
template <bool WALK>
__global__ void __launch_bounds__(256) potrf_dag_kernel(const DagArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  int* const sh = reinterpret_cast<int*>(smem + DAG_LDS_DOUBLES);
  int* const ready = a.ctl + DAG_CTL;
  int* const xflag = ready + a.nb;
  const int nb = a.nb, XD = a.xdelay, total = nb * nb;
  const int tid = threadIdx.x;
  int* const pd = xflag + (int64_t)nb * nb;      // pd[j] = 1: S_jj with every column k < j - 1 applied is parked in the tile's place
  int* const pl = pd + nb;                        // pl[i] = 1: S_{i,i-1} with every column k < i - 1 applied is parked
  constexpr bool walk = WALK;
  if (walk && blockIdx.x == 0) {
    if (!dag_walk(a, smem)) return;
  }
  int cur_s = 0, cur_base = 0;     // claimed indices grow: decode incrementally
  auto step_tasks = [&](int s) { return (s < nb ? nb - s : 0) + ((s >= XD && s - XD < nb) ? s - XD : 0); };
  for (;;) {
    v4d acc[4][4];
    int t = 0;
    if (tid == 0) t = atomicAdd(a.ctl, 1);
    t = dag_bcast(sh, t);
    if (t >= total) return;
#ifdef GEOBO_DAG_TRACE
    long long* const trace = reinterpret_cast<long long*>((reinterpret_cast<uintptr_t>(xflag + (int64_t)nb * nb + 2 * nb) + 7) & ~(uintptr_t)7) + (int64_t)t * 8;
    long long t_poll = 0, t_p0 = 0;
    int n_seg = 0;
    DAG_T(1, ((long long)blockIdx.x << 8) | (__builtin_amdgcn_s_getreg(6164) & 7));   // hwreg(HW_REG_XCC_ID = 20, 0, 4)
    DAG_T(2, DAG_NOW());
#endif
    while (t >= cur_base + step_tasks(cur_s)) { cur_base += step_tasks(cur_s); ++cur_s; }
    const int r = t - cur_base, nchol = cur_s < nb ? nb - cur_s : 0;
    if (r < nchol) {
      // ---------------- tile (i, j) of L ----------------
      const int j = cur_s, i = cur_s + r;
      double* const Tij = a.A + (int64_t)i * NB * a.ld + (int64_t)j * NB;
      DAG_T(0, (0ll << 40) | ((long long)i << 20) | j);
      dag_load_neg(acc, Tij, a.ld);
      int have = 0;
      bool fin = false;
      // with the walker: the diagonal task stops one column early (the walker applies column j - 1 itself), and it and the task of the
      // tile under the diagonal PARK their sums instead of finishing the tile
      const bool park = walk && i <= j + 1;
      const int lim = (walk && i == j) ? (j > 0 ? j - 1 : 0) : j;
      for (;;) {
        const double *Xp, *Yp;
        int64_t ldy;
        int klen;
        if (have < lim) {
          int f = 0;
          if (tid == 0) {
            Spin sp;
#ifdef GEOBO_DAG_TRACE
            t_p0 = DAG_NOW();
#endif
            for (;;) {
              const int ri = ld_flag(ready + i), rj = (i == j) ? ri : ld_flag(ready + j);
              f = ri < rj ? ri : rj;
              if (f > lim) f = lim;
              if (f > have) break;
              if (sp.fail(a.ctl, a.info)) { f = -1; break; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#ifdef GEOBO_DAG_TRACE
            t_poll += DAG_NOW() - t_p0;
#endif
          }
          f = dag_bcast(sh, f);
          if (f < 0) return;
          Xp = a.A + (int64_t)i * NB * a.ld + (int64_t)have * NB;
          Yp = a.A + (int64_t)j * NB * a.ld + (int64_t)have * NB;
          ldy = a.ld;
          klen = (f - have) * NB;
          have = f;
        } else {
          if (i == j || park) { DAG_T(1, (DAG_NOW() << 16) | ((long long)blockIdx.x << 8)); break; }
          DAG_T(3, DAG_NOW());
          // S is complete: park it in the tile's own place, then L_ij = S D_j^T as one more contraction (X = S from memory)
          dag_store<false>(acc, Tij, a.ld, -1.0);
          int ok = 1;
          if (tid == 0) {
            Spin sp;
            while (ld_flag(ready + j) < j + 1)
              if (sp.fail(a.ctl, a.info)) { ok = 0; break; }
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          ok = dag_bcast(sh, ok);
          if (!ok) return;
          DAG_T(4, DAG_NOW());
          dag_zero(acc);
          Xp = Tij;
          Yp = a.Linv + (int64_t)j * NB * a.ldi + (int64_t)j * NB;
          ldy = a.ldi;
          klen = NB;
          fin = true;
        }
        dag_segment<false>(acc, Xp, a.ld, Yp, ldy, klen, smem);
#ifdef GEOBO_DAG_TRACE
        ++n_seg;
#endif
        if (fin) break;
      }
      if (park) {
        if (i == j) {
          if (j > 0) {                                         // (S_00 is the input itself: the walker starts on it at once)
            dag_store<true>(acc, Tij, a.ld, -1.0);
            dag_publish(pd + j, 1);
          }
        } else {
          dag_store<true>(acc, Tij, a.ld, -1.0);
          dag_publish(pl + i, 1);
        }
        DAG_T(3, DAG_NOW()); DAG_T(4, DAG_NOW()); DAG_T(5, DAG_NOW()); DAG_T(6, t_poll); DAG_T(7, n_seg);
      } else if (i == j) {
        dag_store<false>(acc, Tij, a.ld, -1.0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __syncthreads();
        DAG_T(3, DAG_NOW());      // (diagonal tasks: [3] = S parked and visible, [4] = factorised and inverted)
        potf2b_dag(Tij, a.ld, a.Linv + (int64_t)j * NB * a.ldi + (int64_t)j * NB, a.ldi, j * NB, a.info, smem);
        DAG_T(4, DAG_NOW());
        dag_publish(ready + j, j + 1);
        DAG_T(5, DAG_NOW()); DAG_T(6, t_poll); DAG_T(7, n_seg);
      } else {
        dag_store<true>(acc, Tij, a.ld, 1.0);
        dag_publish(ready + i, j + 1);
        DAG_T(5, DAG_NOW()); DAG_T(6, t_poll); DAG_T(7, n_seg);
      }
    } else {
      // ---------------- tile (i, c) of X = L^-1 ----------------
      const int i = cur_s - XD, c = r - nchol;
      double* const Tic = a.Linv + (int64_t)i * NB * a.ldi + (int64_t)c * NB;
      DAG_T(0, (1ll << 40) | ((long long)i << 20) | c);
      dag_zero(acc);
      int have = c;
      bool fin = false;
      for (;;) {
        const double *Xp, *Yp;
        int64_t ldx;
        int klen;
        if (have < i) {
          int f = 0;
          if (tid < 64) {       // wave 0: lane l looks at contraction block have + l
            Spin sp;
            const int k = have + tid;
#ifdef GEOBO_DAG_TRACE
            t_p0 = DAG_NOW();
#endif
            for (;;) {
              int okl = 0;
              if (k < i) okl = (k == c) ? (ld_flag(ready + c) >= c + 1) : (ld_flag(xflag + (int64_t)k * nb + c) != 0);
              // row i of L (and D_i for the last step) must be final as well
              const int li = ld_flag(ready + i) >= i + 1;
              const unsigned long long m = __ballot(okl && li);
              f = m == ~0ull ? 64 : __builtin_ctzll(~m);
              if (f > 0) break;
              if (sp.fail(a.ctl, a.info)) { f = -1; break; }
            }
            f = __builtin_amdgcn_readfirstlane(f);
            if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#ifdef GEOBO_DAG_TRACE
            t_poll += DAG_NOW() - t_p0;
#endif
          }
          f = dag_bcast(sh, f);
          if (f < 0) return;
          Xp = a.A + (int64_t)i * NB * a.ld + (int64_t)have * NB;
          ldx = a.ld;
          Yp = a.Linv + (int64_t)have * NB * a.ldi + (int64_t)c * NB;
          klen = f * NB;
          have += f;
        } else {
          // X_ic = -D_i S: S parked in the tile's own place, one more contraction with X = D_i, Y = S
          DAG_T(3, DAG_NOW()); DAG_T(4, DAG_NOW());
          dag_store<false>(acc, Tic, a.ldi, 1.0);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          __syncthreads();
          dag_zero(acc);
          Xp = a.Linv + (int64_t)i * NB * a.ldi + (int64_t)i * NB;
          ldx = a.ldi;
          Yp = Tic;
          klen = NB;
          fin = true;
        }
        dag_segment<true>(acc, Xp, ldx, Yp, a.ldi, klen, smem);
#ifdef GEOBO_DAG_TRACE
        ++n_seg;
#endif
        if (fin) break;
      }
      dag_store<true>(acc, Tic, a.ldi, -1.0);
      {   // the mirror tile (c, i) of the result is zero (nothing reads it inside the launch)
        double* const Z = a.Linv + (int64_t)c * NB * a.ldi + (int64_t)i * NB;
        for (int e = tid; e < NB * NB / 2; e += 256) *reinterpret_cast<v2d*>(Z + (int64_t)(e >> 6) * a.ldi + 2 * (e & 63)) = (v2d){0., 0.};
      }
      dag_publish(xflag + (int64_t)i * nb + c, 1);
      DAG_T(5, DAG_NOW()); DAG_T(6, t_poll); DAG_T(7, n_seg);
    }
  }
}

// u[i] = sum_{k<=i} Linv[i,k] y[k]: one wavefront per row, shuffle-tree reduction
__global__ void __launch_bounds__(256) trmv_lower_kernel(int64_t m, const double* __restrict__ Linv, int64_t ldi,
                                                         const double* __restrict__ y, double* __restrict__ u) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const double* Lr = Linv + row * ldi;
  double acc = 0.0;
  for (int64_t k = lane; k <= row; k += 64) acc = __builtin_fma(Lr[k], y[k], acc);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) u[row] = acc;
}

// stats[0] = u.u, stats[1] = sum log(L_ii^2); single workgroup, fixed summation order (deterministic)
__global__ void __launch_bounds__(256) logl_stats_kernel(int64_t m, const double* __restrict__ u,
                                                         const double* __restrict__ L, int64_t ld,
                                                         double* __restrict__ stats) {
  __shared__ double s0[256], s1[256];
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int64_t i = tid; i < m; i += 256) {
    const double ui = u[i], d = L[i * ld + i];
    a = __builtin_fma(ui, ui, a);
    b += log(d * d);
  }
  s0[tid] = a; s1[tid] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { s0[tid] += s0[tid + w]; s1[tid] += s1[tid + w]; }
    __syncthreads();
  }
  if (tid == 0) { stats[0] = s0[0]; stats[1] = s1[0]; }
}

// L^-1 by recursive halving, two MFMA GEMMs per merge:
//   node [lo, hi) split at mid:   T = L[mid:hi, lo:mid] * Linv[lo:mid, lo:mid],   Linv[mid:hi, lo:mid] = -Linv[mid:hi, mid:hi] * T.
// (rounds 2-3 launched the left child of every node of the right spine as one serial recursion when the factorisation passed its last
//  column and kept the rest for the end; round 4 schedules every node on its own: see the EAGER tree below.)
struct InvCtx {
  const double* L; int64_t ld; double* Linv; int64_t ldi; hipStream_t st;
};

int split_point(int lo, int hi) {
  // split on a multiple of two 128-blocks where possible: the merge GEMMs then run on 256-row tiles
  int mid = (lo + hi) / 2;
  if (hi - lo > 2 && ((mid - lo) & 1)) ++mid;
  return mid;
}

// T (r x cc, leading dimension cc) = L[mid:hi, lo:mid] * Linv[lo:mid, lo:mid]   (Y lower triangular)
int form_T(const InvCtx& c, int lo, int mid, int hi, double* T) {
  const int64_t r = (int64_t)(hi - mid) * NB, cc = (int64_t)(mid - lo) * NB;
  const int64_t o_lo = (int64_t)lo * NB, o_mid = (int64_t)mid * NB;
  return geobo_gemm_nn(r, cc, cc, 1.0, c.L + o_mid * c.ld + o_lo, c.ld, c.Linv + o_lo * c.ldi + o_lo, c.ldi, 0.0, T, cc, 0, 1, c.st);
}

// Linv[mid:hi, lo:mid] = -Linv[mid:hi, mid:hi] * T         (X lower triangular)
int merge_T(const InvCtx& c, int lo, int mid, int hi, const double* T) {
  const int64_t r = (int64_t)(hi - mid) * NB, cc = (int64_t)(mid - lo) * NB;
  const int64_t o_lo = (int64_t)lo * NB, o_mid = (int64_t)mid * NB;
  return geobo_gemm_nn(r, cc, r, -1.0, c.Linv + o_mid * c.ldi + o_mid, c.ldi, T, cc, 0.0, c.Linv + o_mid * c.ldi + o_lo, c.ldi, 1, 0,
                       c.st);
}

// EAGER tree (round 4).  Measured: the factorisation loop alone takes 11.2 ms at M = 8448 and the call 17.2 -- the L^-1 tree, two thirds
// of it the serial inversion of the root's left child (128 launches of a few tiles each) queued at the half-way point, was the critical
// path of the second half.  Every node [lo, mid, hi) of the tree needs
//     T      = L[mid:hi, lo:mid] * Linv[lo:mid, lo:mid]       -- final once the factorisation has passed block mid - 1 and the left child is merged
//     merge:   Linv[mid:hi, lo:mid] = -Linv[mid:hi, mid:hi] * T -- once block hi - 1 is through and the right child is merged
// so after block c of the factorisation a worker stream receives, in post-order, the merges of all nodes with hi = c + 1 and then the T
// products of all nodes with mid = c + 1 (in-order stream: children before parents).  The work is spread along the loop, every node has its
// own T buffer, and what is left behind the last diagonal block is the right spine's merges.  Same GEMMs per node as the serial recursion:
// identical bits.
constexpr int MAX_NODES = 2048;
struct TreeNode { int lo, mid, hi; int64_t t_off; };
struct TreePlan { int n; int64_t total; TreeNode node[MAX_NODES]; };
void plan_tree_rec(int lo, int hi, TreePlan& p) {
  if (hi - lo <= 1 || p.n >= MAX_NODES) return;
  const int mid = split_point(lo, hi);
  plan_tree_rec(lo, mid, p);
  plan_tree_rec(mid, hi, p);
  if (p.n >= MAX_NODES) return;
  p.node[p.n++] = TreeNode{lo, mid, hi, p.total};
  p.total += (int64_t)(hi - mid) * (mid - lo) * NB * NB;
}
int64_t tree_doubles(int nb) {      // = sum over the nodes of (hi - mid)(mid - lo) blocks: closed recursion, no plan needed
  if (nb <= 1) return 0;
  const int mid = split_point(0, nb);
  return (int64_t)(nb - mid) * mid * NB * NB + tree_doubles(mid) + tree_doubles(nb - mid);
}

// Fork context (geobo_potrf_ctx_create): three streams + a few events on the device that was current at creation, owned by
// the caller.  Nothing here is process-global: two engines (or two devices, or two threads) each bring their own.
constexpr int NEV = 8 + 5;   // 2 x 4 for the look-ahead rings of the factorisation, 4 + 1 for the L^-1 tree (step ring, join)
struct PotrfCtx { int dev; hipStream_t s[3]; hipEvent_t ev[NEV]; };

size_t dag_ctl_bytes(int64_t nb) {
#ifdef GEOBO_DAG_TRACE
  return (size_t)(DAG_CTL + 3 * nb + nb * nb + 2) * sizeof(int) + (size_t)nb * nb * 8 * sizeof(long long);
#else
  return (size_t)(DAG_CTL + 3 * nb + nb * nb) * sizeof(int);
#endif
}

// one persistent launch (the tile DAG above): counters zeroed on the stream, grid = one workgroup per CU
int potrf_inv_dag(int64_t m, double* A, int64_t ld, double* Linv, int64_t ldi, int* info, int* ctl, hipStream_t st) {
  static std::atomic<uint64_t> attr_done{0}, attr_done_walk{0};   // > 64 KiB dynamic LDS (lds_optin.h): one mask per kernel, both set
  if (int rc = ensure_lds_attr(attr_done, potrf_dag_kernel<false>, DAG_LDS_BYTES)) return rc;
  if (int rc = ensure_lds_attr(attr_done_walk, potrf_dag_kernel<true>, DAG_LDS_BYTES)) return rc;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return GEOBO_E_LAUNCH;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return GEOBO_E_LAUNCH;
  const int nb = (int)(m / NB);
  if (hipMemsetAsync(ctl, 0, dag_ctl_bytes(nb), st) != hipSuccess) return GEOBO_E_LAUNCH;
  DagArgs a;
  a.A = A; a.ld = ld; a.Linv = Linv; a.ldi = ldi; a.info = info; a.ctl = ctl; a.nb = nb;
  a.xdelay = DAG_XDELAY;
  int grid = cus < nb * nb ? cus : nb * nb;
  if (DAG_WALKER && grid >= 2 && nb <= DAG_WALK_NB) hipLaunchKernelGGL(potrf_dag_kernel<true>, dim3(grid), dim3(256), DAG_LDS_BYTES, st, a);
  else hipLaunchKernelGGL(potrf_dag_kernel<false>, dim3(grid), dim3(256), DAG_LDS_BYTES, st, a);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}

}  // namespace

extern "C" size_t geobo_potrf_ws_bytes(int64_t m) {
  const int64_t nb = (m + NB - 1) / NB;
  // one T buffer per node of the L^-1 tree (stream schedule), then the counters of the tile DAG
  return (size_t)tree_doubles((int)nb) * sizeof(double) + dag_ctl_bytes(nb);
}

extern "C" int geobo_potrf_ctx_create(void** ctx) {
  if (!ctx) return GEOBO_E_ARG;
  PotrfCtx* c = new (std::nothrow) PotrfCtx();
  if (!c) return GEOBO_E_LAUNCH;
  int ns = 0, ne = 0;   // streams / events created so far
  bool ok = hipGetDevice(&c->dev) == hipSuccess;
  while (ok && ns < 3) { ok = hipStreamCreateWithFlags(&c->s[ns], hipStreamNonBlocking) == hipSuccess; ns += ok; }
  while (ok && ne < NEV) { ok = hipEventCreateWithFlags(&c->ev[ne], hipEventDisableTiming) == hipSuccess; ne += ok; }
  if (!ok) {
    for (int i = 0; i < ne; ++i) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < ns; ++i) (void)hipStreamDestroy(c->s[i]);
    delete c;
    return GEOBO_E_LAUNCH;
  }
  *ctx = c;
  return GEOBO_OK;
}

extern "C" int geobo_potrf_ctx_destroy(void* ctx) {
  if (!ctx) return GEOBO_OK;
  PotrfCtx* c = (PotrfCtx*)ctx;
  for (int i = 0; i < NEV; ++i) (void)hipEventDestroy(c->ev[i]);
  for (int i = 0; i < 3; ++i) (void)hipStreamDestroy(c->s[i]);
  delete c;
  return GEOBO_OK;
}

extern "C" int geobo_potrf_inv(int64_t m, double* A, int64_t ld, double* Linv, int64_t ldi, int* info, void* ws,
                               size_t ws_bytes, void* ctx, int schedule, void* stream) {
  if (schedule != GEOBO_POTRF_AUTO && schedule != GEOBO_POTRF_STREAMS && schedule != GEOBO_POTRF_DAG) return GEOBO_E_ARG;
  if (!A || !Linv || !info || !ws) return GEOBO_E_ARG;
  if (ctx) {   // the fork streams belong to one device: refuse a context made for another one
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != ((PotrfCtx*)ctx)->dev) return GEOBO_E_ARG;
  }
  if (m <= 0 || m % NB || (ld & 1) || (ldi & 1) || ld < m || ldi < m) return GEOBO_E_ALIGN;
  if (ws_bytes < geobo_potrf_ws_bytes(m)) return GEOBO_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(info, 0, sizeof(int), st) != hipSuccess) return GEOBO_E_LAUNCH;
  // From m = 1024: the persistent tile DAG (one launch; every tile of Linv is written by it, no memset).  Below -- the tiny grids of
  // optimize_gp's search, see the note at blocked_potf2 -- and with schedule = GEOBO_POTRF_STREAMS: the stream schedule that follows.
  if (schedule == GEOBO_POTRF_AUTO ? m >= 1024 : schedule == GEOBO_POTRF_DAG) {
    const int64_t nbd = m / NB;
    return potrf_inv_dag(m, A, ld, Linv, ldi, info, reinterpret_cast<int*>((char*)ws + (size_t)tree_doubles((int)nbd) * sizeof(double)), st);
  }
  if (hipMemset2DAsync(Linv, (size_t)ldi * sizeof(double), 0, (size_t)m * sizeof(double), (size_t)m, st) != hipSuccess)
    return GEOBO_E_LAUNCH;
  // Right-looking factorisation with ONE STEP OF LOOK-AHEAD when a fork context is given.  The trailing update of step c is
  // split into (a) the next panel's column block and (b) everything right of it; (b) runs on the context's first stream while
  // the caller's stream already factors the next diagonal block and solves the next panel, which need (a)_c and (b)_(c-2) only:
  //     caller's stream:  [wait (b)_(c-2)] potf2(c), panel(c) -> event P_c;  [wait (b)_(c-1): same column block] (a)_c
  //     side stream:      [wait P_c] (b)_c -> event B_c
  // The first half of the loop is bound by (b) (250 us per step at M = 8448: a K = 128 rank update moves 16 flop per byte of C),
  // the second half by the chain potf2 + panel + (a) = ~175 us per step.  Every element still receives the same updates in the
  // same order: bit-identical to the serial schedule.
  const PotrfCtx* pc = (const PotrfCtx*)ctx;
  hipStream_t side = pc ? pc->s[0] : st;
  const hipEvent_t* Pev = pc ? pc->ev : nullptr;
  const hipEvent_t* Bev = pc ? pc->ev + 4 : nullptr;
  const hipEvent_t* Sev = pc ? pc->ev + 8 : nullptr;     // L^-1 tree: [c & 3] block c is through, [4] the worker has finished
  const int nb = (int)(m / NB);
  if (nb - 1 > MAX_NODES) return GEOBO_E_ARG;
  InvCtx ic;
  ic.L = A; ic.ld = ld; ic.Linv = Linv; ic.ldi = ldi;
  double* const wsd = (double*)ws;
  TreePlan tp;
  tp.n = 0; tp.total = 0;
  plan_tree_rec(0, nb, tp);
  hipStream_t wtree = pc ? pc->s[1] : st;
  // after block c (diagonal block factorised, panel below it solved): merges with hi = c + 1, then T products with mid = c + 1
  auto tree_after_step = [&](int c) -> int {
    if (tp.n == 0) return GEOBO_OK;
    bool any = false;
    for (int i = 0; i < tp.n && !any; ++i) any = tp.node[i].hi == c + 1 || tp.node[i].mid == c + 1;
    if (!any) return GEOBO_OK;
    if (pc && (hipEventRecord(Sev[c & 3], st) != hipSuccess || hipStreamWaitEvent(wtree, Sev[c & 3], 0) != hipSuccess)) return GEOBO_E_LAUNCH;
    InvCtx tc = ic;
    tc.st = wtree;
    for (int i = 0; i < tp.n; ++i) {
      const TreeNode& nd = tp.node[i];
      if (nd.hi == c + 1) { const int rc = merge_T(tc, nd.lo, nd.mid, nd.hi, wsd + nd.t_off); if (rc) return rc; }
    }
    for (int i = 0; i < tp.n; ++i) {
      const TreeNode& nd = tp.node[i];
      if (nd.mid == c + 1) { const int rc = form_T(tc, nd.lo, nd.mid, nd.hi, wsd + nd.t_off); if (rc) return rc; }
    }
    return GEOBO_OK;
  };
  // TWO-LEVEL blocking (round 3): outer panels of OB x 128 columns.  A panel is factorised by the 128-block steps above restricted
  // to the panel's own columns (diagonal block, panel solve, update of the panel columns to the right of it: tall and narrow, a
  // few tens of microseconds), and the trailing matrix receives ONE rank-(OB x 128) update per panel instead of OB rank-128 ones:
  // a rank-128 update moves 16 flop per byte of C and ran at 34 TF/s (the first half of the loop was bound by it, 250 us per
  // 128 columns at M = 8448); at rank 512 it is a matrix-pipe-bound GEMM again.  The look-ahead is the same, one level up:
  //     caller's stream:  [wait (b)_(K-2)] factorise panel K -> event P_K;  [wait (b)_(K-1)] (a)_K = the next panel's columns
  //     side stream:      [wait P_K] (b)_K = everything right of the next panel -> event B_K
  // OB = 1 is the round-2 schedule exactly.  Fixed summation orders for a given OB: ranks that
  // factorise the same matrix get the same bits.  Measured (tools/run_potrf_once.py): M = 33024 (128^3 x 3 properties) 547 -> 408 ms
  // with OB = 4; M = 8448 17.5 -> 18.2 ms -- there the loop is bound by the chain potf2 (98 us) -> panel solve -> panel update of
  // every 128 columns, not by the trailing update, and the longer (a) of a 512-wide panel sits on that chain.  Hence by size:
  // diagonal blocks: the blocked kernel (49 us alone on the chip against 66) from m = 1024; below that -- the tiny grids on which
  // optimize_gp's SHGO / SLSQP search runs, whose forward differences (h = 1.5e-8) amplify last-bit differences of the objective into
  // a different path through a flat valley -- the column kernel, whose rounding the reference-optimum fixture was recorded against.
  const bool blocked_potf2 = m >= 1024;
  const int OB = nb >= 96 ? 4 : 1;
  // Error paths (round-4 advisory): once a tree GEMM or a look-ahead update is queued on a context stream, a non-OK return must not leave
  // that work running behind the caller's back (a retry with jitter on `stream` would race with GEMMs still writing Linv and the T
  // buffers): every early return below first makes `stream` wait for both context streams.
  auto fail = [&](int rc) -> int {
    if (pc) {
      if (hipEventRecord(Sev[4], wtree) == hipSuccess) (void)hipStreamWaitEvent(st, Sev[4], 0);
      if (hipEventRecord(Bev[0], side) == hipSuccess) (void)hipStreamWaitEvent(st, Bev[0], 0);
    }
    return rc;
  };
  int step = 0, ostep = 0, last_b = -1, prev_b = -1;   // step: global 128-block index; outer steps whose (b) was launched most recently
  if (pc) {   // the side stream starts after everything already queued on the caller's stream (the memsets above, the producer of A)
    if (hipEventRecord(Pev[3], st) != hipSuccess || hipStreamWaitEvent(side, Pev[3], 0) != hipSuccess) return fail(GEOBO_E_LAUNCH);
  }
  // panel and (a) are short and run next to (b) of the previous step: 128-row tiles find room as soon as HALF a CU drains
  // (a 512-thread workgroup waits for a whole CU: behind 256-thread (b) tiles that only happens when (b) ends)
  const int crit = pc ? GEOBO_GEMM_SMALL_TILES : 0;
  for (int64_t k0 = 0; k0 < m; ++ostep) {
    const int64_t W = (m - k0) < (int64_t)OB * NB ? (m - k0) : (int64_t)OB * NB;
    if (pc && prev_b >= 0 && hipStreamWaitEvent(st, Bev[prev_b & 3], 0) != hipSuccess) return fail(GEOBO_E_LAUNCH);
    for (int64_t kb = k0; kb < k0 + W; kb += NB, ++step) {
      if (blocked_potf2) hipLaunchKernelGGL(potf2b_inv_kernel, dim3(1), dim3(256), 0, st, A + kb * ld + kb, ld, Linv + kb * ldi + kb, ldi, (int)kb, info);
      else hipLaunchKernelGGL(potf2_inv_kernel, dim3(1), dim3(256), 0, st, A + kb * ld + kb, ld, Linv + kb * ldi + kb, ldi, (int)kb, info);
      if (hipGetLastError() != hipSuccess) return fail(GEOBO_E_LAUNCH);
      const int64_t rem = m - kb - NB;
      if (rem <= 0) {
        const int rt = tree_after_step(step);
        if (rt) return fail(rt);
        continue;
      }
      double* P = A + (kb + NB) * ld + kb;
      int rc = geobo_gemm_nt(rem, NB, NB, 1.0, P, ld, Linv + kb * ldi + kb, ldi, 0.0, P, ld, crit, 0, stream);
      if (rc) return fail(rc);
      rc = tree_after_step(step);
      if (rc) return fail(rc);
      const int64_t cols_left = k0 + W - (kb + NB);
      if (cols_left > 0) {   // the panel's own columns to the right of this block: rows >= kb + NB, lower tiles from the diagonal on
        rc = geobo_gemm_nt(rem, cols_left, NB, -1.0, P, ld, P, ld, 1.0, A + (kb + NB) * ld + (kb + NB), ld, GEOBO_GEMM_LOWER_ONLY | crit, 0, stream);
        if (rc) return fail(rc);
      }
    }
    const int64_t remo = m - k0 - W;   // rows / columns behind the panel
    if (remo > 0) {
      double* Pp = A + (k0 + W) * ld + k0;   // the panel below its diagonal part: remo x W
      double* C0 = A + (k0 + W) * ld + (k0 + W);
      if (!pc) {
        int rc = geobo_gemm_nt(remo, remo, W, -1.0, Pp, ld, Pp, ld, 1.0, C0, ld, GEOBO_GEMM_LOWER_ONLY, 0, stream);
        if (rc) return fail(rc);
      } else {
        if (hipEventRecord(Pev[ostep & 3], st) != hipSuccess) return fail(GEOBO_E_LAUNCH);
        if (last_b >= 0 && hipStreamWaitEvent(st, Bev[last_b & 3], 0) != hipSuccess) return fail(GEOBO_E_LAUNCH);
        const int64_t Wn = remo < (int64_t)OB * NB ? remo : (int64_t)OB * NB;
        // (a)_K: the next panel's columns, rows >= its diagonal
        int rc = geobo_gemm_nt(remo, Wn, W, -1.0, Pp, ld, Pp, ld, 1.0, C0, ld, (OB > 1 ? GEOBO_GEMM_LOWER_ONLY : 0) | crit, 0, stream);
        if (rc) return fail(rc);
        prev_b = last_b;
        if (remo > Wn) {
          // (b)_K: columns behind the next panel, lower tiles
          if (hipStreamWaitEvent(side, Pev[ostep & 3], 0) != hipSuccess) return fail(GEOBO_E_LAUNCH);
          double* P2 = Pp + Wn * ld;
          rc = geobo_gemm_nt(remo - Wn, remo - Wn, W, -1.0, P2, ld, P2, ld, 1.0, C0 + Wn * ld + Wn, ld, GEOBO_GEMM_LOWER_ONLY, 0, side);
          if (rc) return fail(rc);
          if (hipEventRecord(Bev[ostep & 3], side) != hipSuccess) return fail(GEOBO_E_LAUNCH);
          last_b = ostep;
        }
      }
    }
    k0 += W;
  }
  if (pc && last_b >= 0 && hipStreamWaitEvent(st, Bev[last_b & 3], 0) != hipSuccess) return fail(GEOBO_E_LAUNCH);
  // everything is queued; what is left on the worker behind the last diagonal block are the merges of the tree's right spine
  if (pc && tp.n > 0 && (hipEventRecord(Sev[4], wtree) != hipSuccess || hipStreamWaitEvent(st, Sev[4], 0) != hipSuccess)) return GEOBO_E_LAUNCH;
  return GEOBO_OK;
}

extern "C" int geobo_trmv_stats(int64_t m, const double* Linv, int64_t ldi, const double* y, const double* L,
                                int64_t ld, double* u, double* stats, void* stream) {
  if (!Linv || !y || !L || !u || !stats || m <= 0) return GEOBO_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(trmv_lower_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, m, Linv, ldi, y, u);
  hipLaunchKernelGGL(logl_stats_kernel, dim3(1), dim3(256), 0, st, m, u, L, ld, stats);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
