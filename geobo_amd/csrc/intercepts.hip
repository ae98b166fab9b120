// intercepts.hip -- drill-intercept statistics along traces through posterior realisations.
//
//   geobo_trace_stats: for S realisations F[s][a][v], C sorted thresholds on property p and K TRACES (ordered lists of voxels, shallow
//   to deep: the z-columns of the grid, or a CSR list) the thickness, depth to top, accumulation and the longest composited intercept
//   of every (sample, cutoff, trace), reduced to tab[s][c][3], to maps over (c, k) that accumulate over calls, to two histograms and,
//   on request, written out per (s, c, k).
//
// A WAVE owns a trace and walks the samples of the launch, so every map and histogram entry has one owner and needs no atomics.  A
// trace is cut into WORDS of 64 positions, lane i holding position 64 w + i.  Per sample and word the wave loads its 64 values once
// (for a column one 512-byte read; word 0 of the next sample is loaded before the current sample is reduced).  One __ballot per word
// gives the ELIGIBLE word, one per cutoff the ORE word of that cutoff, which LANE c keeps for cutoff c.  Everything that depends on
// the order of the positions is then 64-bit arithmetic that lane c does on its own word, all cutoffs side by side: thickness by
// popcount, top by count-trailing-zeros, the ore runs of the word one after the other (each turn of that loop clears a run, at most
// 32 turns) with three carries from word to word -- start and end of the open intercept and whether every position since its last
// ore is eligible -- which decide whether the gap in front of a run is filled.  The longest intercept is known only at the end of
// the trace, so its sum is a second pass over the words it touches.
// The two floating-point sums are butterfly reductions over the 64 lanes of a word (positions outside the set add +0.0), the words
// added in ascending order: the order depends on the trace length alone, never on S, C or the launch.  No floating-point atomics,
// no LDS, no loop that is not bounded by L, C or S, nothing waits on another workgroup.
// tab: lane c leaves (len, thick, hit) of (s, k, c) packed in one int32 of the workspace; the finish kernel reduces them over k.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "cutoff_set.h"
#include "geobo_hip.h"

namespace {

constexpr int LCAP = 4096;          // positions of a trace at most (13 bits of the packed partial hold 0 .. 4096)
constexpr int WAVES = 4;            // traces of a workgroup

struct TraceArgs {
  const double* F;
  int64_t sstride, n, S, K;
  int C, nz, Lmax, min_len, max_gap;
  int64_t off[3];                   // element offsets of the properties p, (p + 1) % 3, (p + 2) % 3 within a sample
  int read[3];                      // the property of that slot is read: slot 0 always, the others when their bound is > -inf
  double lo[3];                     // lower bound of that slot (slot 0: not used)
  double t[CMAX];
  const uint8_t* mask;
  const int32_t* offsets;           // [K + 1], or unused for columns
  const int32_t* voxels;            // CSR voxel list, or NULL for columns
  uint32_t* hits_any;               // maps [C][K], each may be NULL
  uint32_t* hits;
  int64_t* thick_sum;
  int64_t* top_sum;
  double* acc_sum;
  uint32_t* hist_len;               // [C][K][Lmax + 1], or NULL
  uint32_t* hist_thick;
  int32_t* detail;                  // [S][C][K][6], or NULL
  double* dsum;                     // [S][C][K][2], or NULL
  int32_t* part;                    // [S][K][C]: len | thick << 13 | hit << 26
};

__device__ __forceinline__ uint64_t below(int nbits) {        // the bits 0 .. nbits - 1, nbits in 0 .. 64
  return nbits >= 64 ? ~0ull : ((1ull << nbits) - 1ull);
}

__device__ __forceinline__ double wave_sum(double v) {        // butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the voxel of position 64 w + lane of the trace that starts at element o0 (of `voxels`, or of the grid) and whether it can be read
__device__ __forceinline__ void trace_word(const TraceArgs& a, int64_t o0, int L, int w, int lane, int64_t& v, bool& live) {
  const int j = w * 64 + lane;
  v = 0;
  live = false;
  if (j < L) {
    v = a.voxels ? (int64_t)a.voxels[o0 + j] : o0 + j;
    live = v >= 0 && v < a.n && (!a.mask || a.mask[v] != 0);   // (an index outside the cube is never read)
  }
}

__device__ __forceinline__ void load_word(const TraceArgs& a, const double* f, int64_t v, bool live, double x[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) x[j] = (live && a.read[j]) ? f[a.off[j] + v] : 0.0;
}

__global__ void __launch_bounds__(64 * WAVES) trace_kernel(const TraceArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (k >= a.K) return;                                        // (a whole wave leaves)
  int64_t o0;
  int L;
  if (a.voxels) {
    const int b0 = __builtin_amdgcn_readfirstlane(a.offsets[k]), b1 = __builtin_amdgcn_readfirstlane(a.offsets[k + 1]);
    o0 = b0;
    L = b1 - b0;
  } else {
    o0 = k * a.nz;
    L = a.nz;
  }
  L = L < 0 ? 0 : (L > a.Lmax ? a.Lmax : L);                   // (the histograms hold Lmax + 1 bins: no length can leave them)
  const int nw = (L + 63) >> 6;
  const int C = a.C;
  const bool own = lane < C;                                   // lane c owns cutoff c of this trace
  const int64_t ck = (int64_t)lane * a.K + k;
  const bool want_acc = a.acc_sum || a.dsum, want_run = a.dsum != nullptr;

  uint32_t m_any = 0, m_hit = 0;
  int64_t m_thick = 0, m_top = 0;
  double m_acc = (own && a.acc_sum) ? a.acc_sum[ck] : 0.0;

  int64_t v0;
  bool live0;
  trace_word(a, o0, L, 0, lane, v0, live0);
  double nxt[3] = {0.0, 0.0, 0.0};
  if (a.S > 0) load_word(a, a.F, v0, live0, nxt);

  for (int64_t s = 0; s < a.S; ++s) {
    const double* f = a.F + s * a.sstride;
    int thick = 0, top = L, best_len = 0, best_start = L, n_int = 0;      // lane c: the results of cutoff c
    int cur_start = -1, cur_end = 0, gap_ok = 1;                           // lane c: the carries of cutoff c from word to word
    double acc = 0.0, rsum = 0.0, x0 = 0.0;
    for (int w = 0; w < nw; ++w) {
      int64_t v = v0;
      bool live = live0;
      double x[3];
      if (w == 0) {
        x[0] = nxt[0]; x[1] = nxt[1]; x[2] = nxt[2];
        if (s + 1 < a.S) load_word(a, f + a.sstride, v0, live0, nxt);
        x0 = x[0];
      } else {
        trace_word(a, o0, L, w, lane, v, live);
        load_word(a, f, v, live, x);
      }
      const bool e = live && x[0] == x[0];                     // eligible: inside the mask and not NaN
      bool eb = e;
#pragma unroll
      for (int j = 1; j < 3; ++j) {
        if (a.read[j]) eb = eb && x[j] >= a.lo[j];             // (NaN fails)
      }
      const int base = w * 64;
      const uint64_t bad = ~__ballot(e) & below(L - base);     // the positions of the word that no gap may hold
      uint64_t om = 0;                                         // lane c: the ore word of cutoff c
      for (int c = 0; c < C; ++c) {
        const bool o = eb && x[0] >= a.t[c];
        const uint64_t b = __ballot(o);
        if (lane == c) om = b;
        if (want_acc) {
          const double part = wave_sum(o ? x[0] : 0.0);
          if (lane == c) acc += part;
        }
      }
      // from here every lane works on its own cutoff (the lanes from C on hold an empty word)
      if (om) {
        thick += __popcll(om);
        if (top == L) top = base + (int)__builtin_ctzll(om);
      }
      uint64_t m = om;
      int pos = 0;                                             // the word is consumed up to here
      while (m) {                                              // one ore run per turn
        const int r0 = (int)__builtin_ctzll(m);                // (pos <= r0 < 64)
        if (bad & below(r0) & ~below(pos)) gap_ok = 0;
        const uint64_t rest = ~(m >> r0);
        const int len = rest ? (int)__builtin_ctzll(rest) : 64;
        const int g0 = base + r0;
        if (!(cur_start >= 0 && gap_ok && g0 - cur_end <= a.max_gap)) {    // the gap in front is not filled: the open intercept ends
          if (cur_start >= 0) {
            const int il = cur_end - cur_start;
            if (il > best_len) { best_len = il; best_start = cur_start; }
            if (il >= a.min_len) n_int += 1;
          }
          cur_start = g0;
        }
        cur_end = g0 + len;
        gap_ok = 1;
        pos = r0 + len;
        m &= ~below(pos);
      }
      if (bad & ~below(pos)) gap_ok = 0;
    }
    if (cur_start >= 0) {                                      // lane c ends the intercept that is still open
      const int il = cur_end - cur_start;
      if (il > best_len) { best_len = il; best_start = cur_start; }
      if (il >= a.min_len) n_int += 1;
    }
    if (want_run) {                                            // the sum over the longest intercept, its filled waste included
      for (int c = 0; c < C; ++c) {
        const int bs = __builtin_amdgcn_readlane(best_start, c), bl = __builtin_amdgcn_readlane(best_len, c);
        if (bl > 0) {
          double tot = 0.0;
          for (int w = bs >> 6; w <= (bs + bl - 1) >> 6; ++w) {
            double xv = x0;
            if (w > 0) {
              int64_t v;
              bool live;
              trace_word(a, o0, L, w, lane, v, live);
              xv = live ? f[a.off[0] + v] : 0.0;
            }
            const int j = w * 64 + lane;
            tot += wave_sum((j >= bs && j < bs + bl) ? xv : 0.0);
          }
          if (lane == c) rsum = tot;
        }
      }
    }
    if (own) {
      const int hit = best_len >= a.min_len ? 1 : 0;
      m_any += thick > 0 ? 1u : 0u;
      m_hit += (uint32_t)hit;
      m_thick += thick;
      m_top += thick > 0 ? top : 0;
      m_acc += acc;
      if (a.hist_len) a.hist_len[ck * (a.Lmax + 1) + best_len] += 1u;
      if (a.hist_thick) a.hist_thick[ck * (a.Lmax + 1) + thick] += 1u;
      a.part[(s * a.K + k) * C + lane] = best_len | (thick << 13) | (hit << 26);
      if (a.detail) {
        int32_t* d = a.detail + ((s * C + lane) * a.K + k) * 6;
        d[0] = thick; d[1] = top; d[2] = best_start; d[3] = best_len; d[4] = n_int; d[5] = 0;
      }
      if (a.dsum) {
        double* d = a.dsum + ((s * C + lane) * a.K + k) * 2;
        d[0] = acc; d[1] = rsum;
      }
    }
  }
  if (own) {
    if (a.hits_any) a.hits_any[ck] += m_any;
    if (a.hits) a.hits[ck] += m_hit;
    if (a.thick_sum) a.thick_sum[ck] += m_thick;
    if (a.top_sum) a.top_sum[ck] += m_top;
    if (a.acc_sum) a.acc_sum[ck] = m_acc;
  }
}

// tab[s][c] = (sum_k hit, sum_k thick, max_k len): a workgroup per sample, a lane keeps one cutoff
__global__ void __launch_bounds__(256) trace_finish_kernel(const int32_t* __restrict__ part, int64_t K, int C, int64_t* __restrict__ tab) {
  __shared__ int64_t r_hit[256], r_thick[256];
  __shared__ int32_t r_len[256];
  const int tid = threadIdx.x;
  const int stride = (256 / C) * C;                            // a multiple of C: lane tid always meets cutoff tid % C
  const int32_t* p = part + (int64_t)blockIdx.x * K * C;
  int64_t hit = 0, thick = 0;
  int32_t len = 0;
  if (tid < stride) {
    for (int64_t i = tid; i < K * C; i += stride) {
      const int32_t v = p[i];
      hit += (v >> 26) & 1;
      thick += (v >> 13) & 8191;
      len = max(len, v & 8191);
    }
  }
  r_hit[tid] = hit; r_thick[tid] = thick; r_len[tid] = len;
  __syncthreads();
  if (tid < C) {
    for (int u = tid + C; u < stride; u += C) {
      hit += r_hit[u];
      thick += r_thick[u];
      len = max(len, r_len[u]);
    }
    int64_t* o = tab + ((int64_t)blockIdx.x * C + tid) * 3;
    o[0] = hit; o[1] = thick; o[2] = len;
  }
}

bool trace_shape_ok(int64_t S, int64_t K, int C) {
  return S >= 0 && S <= INT32_MAX && K >= 1 && K <= INT32_MAX && C >= 1 && C <= CMAX;
}

size_t trace_ws_bytes_of(int64_t S, int64_t K, int C) {
  const int64_t per = K * C * 4;                               // one int32 per (trace, cutoff); K C < 2^36
  if (S > 0 && per > INT64_MAX / S) return 0;
  const int64_t b = (S * per + 15) / 16 * 16;
  return (size_t)(b < 16 ? 16 : b);
}

}  // namespace

extern "C" size_t geobo_trace_stats_ws_bytes(int64_t S, int64_t K, int C) {
  if (!trace_shape_ok(S, K, C)) return 0;
  return trace_ws_bytes_of(S, K, C);
}

extern "C" int geobo_trace_stats(int64_t S, const double* F, int64_t sstride, int64_t pstride, int ny, int nx, int nz, int p, int C,
                                 const double* t, const double* lo, const uint8_t* mask, int64_t K, const int32_t* offsets,
                                 const int32_t* voxels, int Lmax, int min_len, int max_gap, int64_t* tab, uint32_t* hits_any,
                                 uint32_t* hits, int64_t* thick_sum, int64_t* top_sum, double* acc_sum, uint32_t* hist_len,
                                 uint32_t* hist_thick, int32_t* detail, double* dsum, void* ws, size_t ws_bytes, void* stream) {
  // every check before any device access (t and lo are host arrays; offsets and voxels are on the device and are not read here)
  if (!tab || !ws || !trace_shape_ok(S, K, C)) return GEOBO_E_ARG;
  if (ny < 1 || nx < 1 || nz < 1 || (int64_t)ny * nx > INT32_MAX / nz) return GEOBO_E_ARG;
  TraceArgs a{};
  if (!cutoff_set_of(S, F, sstride, pstride, (int64_t)ny * nx * nz, p, C, t, lo, mask, a)) return GEOBO_E_ARG;
  if (min_len < 1 || max_gap < 0 || max_gap > LCAP || Lmax < 1 || Lmax > LCAP) return GEOBO_E_ARG;
  if (voxels) {
    if (!offsets) return GEOBO_E_ARG;
  } else if (K != (int64_t)ny * nx || Lmax != nz) {            // the columns of the grid
    return GEOBO_E_ARG;
  }
  const size_t need = trace_ws_bytes_of(S, K, C);
  if (need == 0 || ws_bytes < need || ((uintptr_t)ws & 15)) return GEOBO_E_ARG;
  if (S == 0) return GEOBO_OK;

  a.S = S; a.K = K;
  a.nz = nz; a.Lmax = Lmax; a.min_len = min_len; a.max_gap = max_gap;
  a.offsets = offsets; a.voxels = voxels;
  a.hits_any = hits_any; a.hits = hits; a.thick_sum = thick_sum; a.top_sum = top_sum; a.acc_sum = acc_sum;
  a.hist_len = hist_len; a.hist_thick = hist_thick; a.detail = detail; a.dsum = dsum;
  a.part = (int32_t*)ws;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(trace_kernel, dim3((unsigned)((K + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, st, a);
  hipLaunchKernelGGL(trace_finish_kernel, dim3((unsigned)S), dim3(256), 0, st, (const int32_t*)a.part, K, C, tab);
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
