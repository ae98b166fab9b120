// geobodies.hip -- connected bodies of the cutoff sets of posterior realisations.
//
// For S realisations F[s][a][v] on the (ny, nx, nz) grid (z fastest) and C ascending thresholds, volume (s, c) holds the SET of
// gradetonnage.hip's geobo_cutoff_stats: F_p >= t[c], the other properties at their lower bounds, the mask set, NaN out.  A BODY is a
// connected component of the set under 6- or 26-connectivity.  Labelling is a union-find on one int32 parent array L per volume:
//
//   init     L[v] = v in the set, -1 outside; the body sizes are zeroed.
//   merge    one lane per voxel unites it with its in-set FORWARD neighbours (3 or 13: the offsets that are positive in (y, x, z)
//            order).  find() follows parents and halves the path with atomicMin; unite() hooks the larger root under the smaller
//            with old = atomicMin(&L[hi], lo): done when old == hi, else it goes on from (old, lo).  INVARIANT: L[x] <= x, L[x] is
//            a voxel of x's body, and values only decrease -- a stale read is still an ancestor, the larger index of the pair
//            falls in every round, and the one root a body ends with is its smallest voxel index, whatever the arrival order.
//            Every access to L in this kernel is a relaxed agent-scope atomic (load, min); no fence, no flag, no waiting on
//            another workgroup: the only hand-offs are the launch boundaries.
//            TILED (the default): a tile-local phase first -- a workgroup labels a tile of at most 512 voxels (8 x 8 x 8 in a cube)
//            in LDS with the same find / unite on workgroup-scope atomics and leaves L[v] = the tile's root of v; tile-local
//            index order is global index order, so the invariant holds on.  The merge then unites across tile faces only, from
//            trees of depth one.  Same labels either way; 64^3, 1024 volumes: see DESIGN.md section 18 for both timings.
//   flatten  label[v] = root(v) (read-only walk), and the weighted size of each body by integer atomics on its root's counter
//            (exact, order-free), added up within the wave first where lanes share a root.
//
// Every loop is bounded: a walk or a unite that has not ended after 2 n + 64 rounds writes a code into *info and leaves.
//
// Statistics per volume: a marking pass sets mark[root] for the bodies that hold an in-set seed; one workgroup per volume counts the
// bodies of at least min_count, finds the largest (ties to the smaller label) and counts the seeded bodies; the floating-point sums
// (whole set, largest body, seeded body) use the scheme of geobo_cutoff_stats -- a workgroup owns 512 consecutive voxels, eight
// runs of 64 are added in ascending order, then the runs, then the chunks by a finish pass -- so the order follows from n alone:
// no floating-point atomics, bitwise reproducible, a sample alone gives the bits it gives in a batch, and the whole-set sum is
// geobo_cutoff_stats's bit for bit.  hits: one lane owns (c, v) and walks the samples of the call -- no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "cutoff_set.h"
#include "geobo_hip.h"

namespace {

constexpr int WG = 256;
constexpr int TILE = 512;             // voxels of a tile of the tile-local phase at most
constexpr int CHUNK = 2 * WG;       // voxels of a sum chunk (as in gradetonnage.hip)
constexpr int64_t VMAX = 65535;     // volumes of a call (grid y extent)
constexpr int NSTAT = 6;            // count_total, n_bodies, largest count, largest label, seeded count, seeded bodies
constexpr int NSUM = 3;             // whole set, largest body, seeded body

struct Grid {
  int ny, nx, nz;
  int64_t n;
};

bool grid_of(int ny, int nx, int nz, Grid& g) {
  if (ny < 1 || nx < 1 || nz < 1) return false;
  if ((int64_t)ny * nx > INT32_MAX / nz) return false;         // a voxel index fits an int32
  g.ny = ny; g.nx = nx; g.nz = nz;
  g.n = (int64_t)ny * nx * nz;
  return true;
}

// the tile of the tile-local phase: up to 8 x 8 x 8, grown along z, x, y (in that order) while the grid has room and the tile stays
// within TILE voxels -- (1, 1, 4096) gets (1, 1, 512), (64, 64, 1) gets (8, 64, 1)
void tile_of(const Grid& g, int& ty, int& tx, int& tz) {
  ty = g.ny < 8 ? g.ny : 8; tx = g.nx < 8 ? g.nx : 8; tz = g.nz < 8 ? g.nz : 8;
  while (tz < g.nz && 2 * ty * tx * tz <= TILE) tz *= 2;
  while (tx < g.nx && 2 * ty * tx * tz <= TILE) tx *= 2;
  while (ty < g.ny && 2 * ty * tx * tz <= TILE) ty *= 2;
}

bool shape_ok(int64_t S, int C) { return S >= 0 && C >= 1 && C <= CMAX && S * C <= VMAX; }

struct Layout {                     // workspace of V = max(S, 1) * C volumes: byte offsets, each a multiple of 16
  size_t L, label, size, seeds, psum, pcnt, total;
};

Layout layout_of(int64_t S, int64_t n, int C) {
  const size_t V = (size_t)(S < 1 ? 1 : S) * C;
  const size_t nchunks = (size_t)((n + CHUNK - 1) / CHUNK);
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  Layout l;
  size_t o = 0;
  l.L = o; o += up(V * n * 4);
  l.label = o; o += up(V * n * 4);
  l.size = o; o += up(V * n * 8);
  l.seeds = o; o += up((size_t)n * 4);
  l.psum = o; o += up(V * nchunks * NSUM * 8);
  l.pcnt = o; o += up(V * nchunks * NSUM * 8);
  l.total = o;
  return l;
}

struct BodyArgs {
  const double* F;
  int64_t sstride, pstride, n;
  int S, C, ny, nx, nz, cap;
  int ty, tx, tz;                   // tile of the tile-local phase
  int64_t off[3];                   // element offsets of the properties p, (p + 1) % 3, (p + 2) % 3 within a sample
  int read[3];
  double lo[3];
  double t[CMAX];
  const uint8_t* mask;
  const int32_t* weight;
  int32_t* L;                       // parents; after flatten: the seed marks of the roots
  int32_t* label;
  int64_t* size;
  int32_t* info;
};

struct Agent {                      // parents in global memory, shared by every workgroup of the launch
  static __device__ __forceinline__ int32_t ld(const int32_t* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ int32_t amin(int32_t* q, int32_t v) {
    return __hip_atomic_fetch_min(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
struct Group {                      // parents of one tile in LDS, shared by the lanes of one workgroup
  static __device__ __forceinline__ int32_t ld(const int32_t* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ int32_t amin(int32_t* q, int32_t v) {
    return __hip_atomic_fetch_min(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
__device__ __forceinline__ void flag(int32_t* info, int32_t code) {
  __hip_atomic_fetch_max(info, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- init ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) init_kernel(const BodyArgs a) {
  const int64_t v = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (v >= a.n) return;
  const int64_t s = blockIdx.y;
  const double* f = a.F + s * a.sstride;
  const double x = f[a.off[0] + v];
  bool ok = !a.mask || a.mask[v] != 0;
#pragma unroll
  for (int j = 1; j < 3; ++j) {
    if (a.read[j]) ok = ok && f[a.off[j] + v] >= a.lo[j];      // (NaN fails)
  }
  for (int c = 0; c < a.C; ++c) {
    const bool in = ok && x >= a.t[c];                          // (NaN fails)
    const int64_t o = (s * a.C + c) * a.n + v;
    a.L[o] = in ? (int32_t)v : -1;
    a.size[o] = 0;
  }
}

// ---- merge -----------------------------------------------------------------------------------------------------------------------
template <class M>
__device__ int32_t find_halving(int32_t* L, int32_t x, int cap, int32_t* info) {
  for (int it = 0; it < cap; ++it) {
    const int32_t p = M::ld(L + x);
    if (p == x) return x;
    const int32_t g = M::ld(L + p);
    if (g != p) M::amin(L + x, g);                                // path halving: only ever lowers L[x], to an ancestor
    x = g;
  }
  flag(info, 1);
  return x;
}

template <class M>
__device__ void unite(int32_t* L, int32_t a, int32_t b, int cap, int32_t* info) {
  a = find_halving<M>(L, a, cap, info);
  b = find_halving<M>(L, b, cap, info);
  for (int it = 0; it < cap; ++it) {
    if (a == b) return;
    if (a < b) { const int32_t h = a; a = b; b = h; }          // a = hi, b = lo
    const int32_t old = M::amin(L + a, b);
    if (old == a) return;                                      // a was a root and now hangs under b
    a = old;                                                   // a had the parent old < a: old and b remain to be united
  }
  flag(info, 2);
}

// a forward offset: positive in (y, x, z) order; with 6 neighbours the three face offsets alone
template <int NB>
__device__ __forceinline__ constexpr bool forward_offset(int dy, int dx, int dz) {
  return (dy > 0 || (dy == 0 && (dx > 0 || (dx == 0 && dz > 0)))) && (NB == 26 || (dy != 0) + (dx != 0) + (dz != 0) == 1);
}

// tile-local phase: a workgroup labels one tile of at most 512 voxels in LDS with the same find / unite (local index order is
// global index order, so the invariant carries over) and leaves L[v] = the tile-local root; the merge then unites across tile
// faces only.
template <int NB>
__global__ void __launch_bounds__(TILE) tile_kernel(const BodyArgs a) {
  __shared__ int32_t lab[TILE];
  const int i = threadIdx.x;
  const int ty = a.ty, tx = a.tx, tz = a.tz;
  const int ntx = (a.nx + tx - 1) / tx, ntz = (a.nz + tz - 1) / tz;
  const int t = blockIdx.x;
  const int y0 = (t / (ntx * ntz)) * ty, x0 = ((t / ntz) % ntx) * tx, z0 = (t % ntz) * tz;
  const int lz = i % tz, lx = (i / tz) % tx, ly = i / (tz * tx);
  const int gy = y0 + ly, gx = x0 + lx, gz = z0 + lz;
  const bool inside = ly < ty && gy < a.ny && gx < a.nx && gz < a.nz;
  int32_t* L = a.L + (int64_t)blockIdx.y * a.n;
  const int32_t g = inside ? (gy * a.nx + gx) * a.nz + gz : 0;
  const bool in = inside && L[g] >= 0;
  lab[i] = in ? i : -1;
  __syncthreads();
  if (in) {
#pragma unroll
    for (int dy = 0; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
          if (!forward_offset<NB>(dy, dx, dz)) continue;
          const int my = ly + dy, mx = lx + dx, mz = lz + dz;
          if (my >= ty || mx < 0 || mx >= tx || mz < 0 || mz >= tz) continue;
          const int j = (my * tx + mx) * tz + mz;
          if (Group::ld(lab + j) >= 0) unite<Group>(lab, i, j, 2 * TILE + 64, a.info);
        }
      }
    }
  }
  __syncthreads();
  if (in) {
    int32_t r = i;
    int it = 0;
    for (; it < TILE; ++it) {
      const int32_t p = lab[r];
      if (p == r) break;
      r = p;
    }
    if (it == TILE) flag(a.info, 4);
    if (r != i) L[g] = ((y0 + r / (tz * tx)) * a.nx + x0 + (r / tz) % tx) * a.nz + z0 + r % tz;
  }
}

template <int NB, bool TILED>
__global__ void __launch_bounds__(WG) merge_kernel(const BodyArgs a) {
  const int64_t v64 = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (v64 >= a.n) return;
  const int32_t v = (int32_t)v64;
  int32_t* L = a.L + (int64_t)blockIdx.y * a.n;
  if (Agent::ld(L + v) < 0) return;
  const int iz = v % a.nz, ix = (v / a.nz) % a.nx, iy = v / (a.nz * a.nx);
  const int ly = TILED ? iy % a.ty : 0, lx = TILED ? ix % a.tx : 0, lz = TILED ? iz % a.tz : 0;
#pragma unroll
  for (int dy = 0; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz) {
        if (!forward_offset<NB>(dy, dx, dz)) continue;
        const int jy = iy + dy, jx = ix + dx, jz = iz + dz;
        if (jy >= a.ny || jx < 0 || jx >= a.nx || jz < 0 || jz >= a.nz) continue;
        if (TILED && ly + dy < a.ty && lx + dx >= 0 && lx + dx < a.tx && lz + dz >= 0 && lz + dz < a.tz) continue;    // united in the tile
        const int32_t u = (jy * a.nx + jx) * a.nz + jz;
        if (Agent::ld(L + u) >= 0) unite<Agent>(L, v, u, a.cap, a.info);
      }
    }
  }
}

// ---- flatten ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) flatten_kernel(const BodyArgs a) {
  const int64_t v = (int64_t)blockIdx.x * WG + threadIdx.x;
  const int64_t o = (int64_t)blockIdx.y * a.n;
  const int32_t* L = a.L + o;
  int32_t r = -1;
  int64_t w = 0;
  if (v < a.n) {
    int32_t x = L[v];
    if (x >= 0) {
      int it = 0;
      for (; it < a.cap; ++it) {
        const int32_t p = L[x];
        if (p == x) break;
        x = p;
      }
      if (it == a.cap) flag(a.info, 3);
      r = x;
      w = a.weight ? a.weight[v] : 1;
    }
    a.label[o + v] = r;
  }
  // sizes: lanes of a wave that share a root add up first (two rounds), the rest add alone.  (every lane of the wave gets here)
  const int lane = threadIdx.x & 63;
  unsigned long long* size = reinterpret_cast<unsigned long long*>(a.size + o);
  bool todo = r >= 0;
  for (int round = 0; round < 2; ++round) {
    const unsigned long long act = __ballot(todo);
    if (!act) break;                                           // (wave-uniform)
    const int leader = __ffsll((long long)act) - 1;
    const int32_t lr = __shfl(r, leader);
    const bool same = todo && r == lr;
    long long sum = same ? w : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    if (lane == leader) atomicAdd(size + lr, (unsigned long long)sum);
    if (same) todo = false;
  }
  if (todo) atomicAdd(size + r, (unsigned long long)w);
}

// ---- seeds -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) seed_kernel(int64_t n, int64_t K, const int32_t* __restrict__ seeds, const int32_t* __restrict__ label,
                                                  int32_t* __restrict__ mark) {
  const int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (k >= K) return;
  const int64_t o = (int64_t)blockIdx.y * n;
  const int32_t sd = seeds[k];
  if (sd < 0 || sd >= n) return;                               // (checked on the host; never trusted with an address)
  const int32_t lab = label[o + sd];
  if (lab >= 0) atomicOr(mark + o + lab, 1);
}

// ---- per-volume body statistics ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) stats_kernel(int64_t n, int64_t min_count, const int32_t* __restrict__ label, const int64_t* __restrict__ size,
                                                   const int32_t* __restrict__ mark, int64_t* __restrict__ stats) {
  __shared__ int64_t s_nb[WG], s_sb[WG], s_cnt[WG];
  __shared__ int32_t s_lab[WG];
  const int tid = threadIdx.x;
  const int64_t o = (int64_t)blockIdx.x * n;
  int64_t nb = 0, sb = 0, best = 0;
  int32_t blab = -1;
  for (int64_t v = tid; v < n; v += WG) {                      // ascending v: a tie keeps the smaller label
    if (label[o + v] == (int32_t)v) {
      const int64_t sz = size[o + v];
      nb += sz >= min_count;
      sb += mark[o + v] != 0;
      if (sz > best) { best = sz; blab = (int32_t)v; }
    }
  }
  s_nb[tid] = nb; s_sb[tid] = sb; s_cnt[tid] = best; s_lab[tid] = blab;
  __syncthreads();
  for (int h = WG / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      s_nb[tid] += s_nb[tid + h];
      s_sb[tid] += s_sb[tid + h];
      const int64_t c2 = s_cnt[tid + h];
      const int32_t l2 = s_lab[tid + h];
      if (l2 >= 0 && (c2 > s_cnt[tid] || (c2 == s_cnt[tid] && (s_lab[tid] < 0 || l2 < s_lab[tid])))) {
        s_cnt[tid] = c2; s_lab[tid] = l2;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    int64_t* st = stats + (int64_t)blockIdx.x * NSTAT;
    st[1] = s_nb[0]; st[2] = s_cnt[0]; st[3] = s_lab[0]; st[5] = s_sb[0];
  }
}

// ---- sums ------------------------------------------------------------------------------------------------------------------------
struct Entry {                      // 16 bytes: one voxel of the chunk
  int32_t in, w;                    // in: bit 0 the set, bit 1 the largest body, bit 2 the seeded body
  double wx;
};

__global__ void __launch_bounds__(WG) sums_kernel(const BodyArgs a, const int32_t* __restrict__ mark, const int64_t* __restrict__ stats,
                                                  int64_t nchunks, double* __restrict__ psum, int64_t* __restrict__ pcnt) {
  __shared__ Entry ent[CHUNK];
  __shared__ double part_sum[NSUM][8];
  __shared__ int64_t part_cnt[NSUM][8];
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.x, vol = blockIdx.y;
  const int64_t s = vol / a.C;
  const int64_t o = vol * a.n;
  const int32_t big = (int32_t)stats[vol * NSTAT + 3];
  const double* f = a.F + s * a.sstride + a.off[0];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int64_t v = chunk * CHUNK + 2 * tid + k;
    Entry en;
    en.in = 0; en.w = 0; en.wx = 0.0;
    if (v < a.n) {
      const int32_t lab = a.label[o + v];
      if (lab >= 0) {
        en.w = a.weight ? a.weight[v] : 1;
        en.wx = (double)en.w * f[v];
        en.in = 1 | (lab == big ? 2 : 0) | (mark[o + lab] != 0 ? 4 : 0);
      }
    }
    ent[2 * tid + k] = en;
  }
  __syncthreads();
  if (tid < NSUM * 8) {
    const int q = tid >> 3, part = tid & 7;
    const Entry* run = ent + part * 64;
    double sum = 0.0;
    int64_t cnt = 0;
#pragma unroll 16
    for (int i = 0; i < 64; ++i) {
      const Entry en = run[i];
      if ((en.in >> q) & 1) {                                  // (a voxel outside is not added at all: it may be inf or NaN)
        sum += en.wx;
        cnt += en.w;
      }
    }
    part_sum[q][part] = sum;
    part_cnt[q][part] = cnt;
  }
  __syncthreads();
  if (tid < NSUM) {
    double sum = 0.0;
    int64_t cnt = 0;
#pragma unroll
    for (int pt = 0; pt < 8; ++pt) {
      sum += part_sum[tid][pt];
      cnt += part_cnt[tid][pt];
    }
    const int64_t i = (vol * nchunks + chunk) * NSUM + tid;
    psum[i] = sum;
    pcnt[i] = cnt;
  }
}

// the chunks in ascending order
__global__ void __launch_bounds__(WG) sums_finish_kernel(const double* __restrict__ psum, const int64_t* __restrict__ pcnt, int64_t V, int64_t nchunks,
                                                         double* __restrict__ sums, int64_t* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= V * NSUM) return;
  const int64_t vol = i / NSUM;
  const int q = (int)(i - vol * NSUM);
  double v = 0.0;
  int64_t k = 0;
#pragma unroll 16
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    const int64_t j = (vol * nchunks + ch) * NSUM + q;
    v += psum[j];
    k += pcnt[j];
  }
  sums[i] = v;
  if (q == 0) stats[vol * NSTAT + 0] = k;
  if (q == 2) stats[vol * NSTAT + 4] = k;
}

// ---- hits: one owner per (c, v) -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG) hits_kernel(int64_t n, int S, int C, const int32_t* __restrict__ label, const int32_t* __restrict__ mark,
                                                  const int64_t* __restrict__ stats, uint32_t* __restrict__ hits_largest,
                                                  uint32_t* __restrict__ hits_seeded) {
  const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= (int64_t)C * n) return;
  const int64_t c = i / n, v = i - c * n;
  uint32_t hl = 0, hs = 0;
  for (int s = 0; s < S; ++s) {
    const int64_t vol = (int64_t)s * C + c;
    const int32_t lab = label[vol * n + v];
    if (lab >= 0) {
      hl += lab == (int32_t)stats[vol * NSTAT + 3];
      if (hits_seeded) hs += mark[vol * n + lab] != 0;
    }
  }
  if (hits_largest && hl) hits_largest[i] += hl;
  if (hits_seeded && hs) hits_seeded[i] += hs;
}

}  // namespace

extern "C" size_t geobo_bodies_ws_bytes(int64_t S, int ny, int nx, int nz, int C) {
  Grid g;
  if (!grid_of(ny, nx, nz, g) || !shape_ok(S, C)) return 0;
  return layout_of(S, g.n, C).total;
}

extern "C" int geobo_bodies(int64_t S, const double* F, int64_t sstride, int64_t pstride, int ny, int nx, int nz, int p, int C, const double* t,
                            const double* lo, const uint8_t* mask, const int32_t* weight, int neighbours, int64_t min_count, int64_t K,
                            const int32_t* seeds, int64_t* stats, double* sums, uint32_t* hits_largest, uint32_t* hits_seeded, int32_t* labels,
                            int32_t* info, int phases, void* ws, size_t ws_bytes, void* stream) {
  // every check before any device access (t, lo and seeds are host arrays)
  Grid g;
  if (!stats || !sums || !info || !ws) return GEOBO_E_ARG;
  if (!grid_of(ny, nx, nz, g) || !shape_ok(S, C)) return GEOBO_E_ARG;
  if (neighbours != 6 && neighbours != 26) return GEOBO_E_ARG;
  if (min_count < 1 || K < 0 || K > g.n || (K > 0 && !seeds)) return GEOBO_E_ARG;
  if (phases < 1 || phases > (GEOBO_BODIES_ALL | GEOBO_BODIES_TILED) || !(phases & GEOBO_BODIES_ALL)) return GEOBO_E_ARG;
  for (int64_t k = 0; k < K; ++k) {
    if (seeds[k] < 0 || seeds[k] >= g.n) return GEOBO_E_ARG;
  }
  const int64_t n = g.n;
  BodyArgs a{};
  if (!cutoff_set_of(S, F, sstride, pstride, n, p, C, t, lo, mask, a)) return GEOBO_E_ARG;
  const Layout l = layout_of(S, n, C);
  if (ws_bytes < l.total || ((uintptr_t)ws & 15)) return GEOBO_E_ARG;
  if (S == 0) return GEOBO_OK;

  const int64_t V = S * C;
  char* w8 = (char*)ws;
  a.pstride = pstride; a.S = (int)S; a.ny = ny; a.nx = nx; a.nz = nz;
  a.cap = (int)(2 * n + 64 > INT32_MAX ? INT32_MAX : 2 * n + 64);
  a.weight = weight; a.info = info;
  a.L = (int32_t*)(w8 + l.L);
  a.label = labels ? labels : (int32_t*)(w8 + l.label);
  a.size = (int64_t*)(w8 + l.size);
  int32_t* mark = a.L;
  int32_t* dseeds = (int32_t*)(w8 + l.seeds);
  double* psum = (double*)(w8 + l.psum);
  int64_t* pcnt = (int64_t*)(w8 + l.pcnt);
  const int64_t nchunks = (n + CHUNK - 1) / CHUNK;
  const unsigned gx = (unsigned)((n + WG - 1) / WG);
  hipStream_t st = (hipStream_t)stream;

  if (phases & GEOBO_BODIES_INIT) hipLaunchKernelGGL(init_kernel, dim3(gx, (unsigned)S), dim3(WG), 0, st, a);
  if (phases & GEOBO_BODIES_MERGE) {
    if (phases & GEOBO_BODIES_TILED) {
      tile_of(g, a.ty, a.tx, a.tz);
      const unsigned tiles = (unsigned)(((ny + a.ty - 1) / a.ty) * ((nx + a.tx - 1) / a.tx) * ((nz + a.tz - 1) / a.tz));
      if (neighbours == 6) {
        hipLaunchKernelGGL(tile_kernel<6>, dim3(tiles, (unsigned)V), dim3(TILE), 0, st, a);
        hipLaunchKernelGGL((merge_kernel<6, true>), dim3(gx, (unsigned)V), dim3(WG), 0, st, a);
      } else {
        hipLaunchKernelGGL(tile_kernel<26>, dim3(tiles, (unsigned)V), dim3(TILE), 0, st, a);
        hipLaunchKernelGGL((merge_kernel<26, true>), dim3(gx, (unsigned)V), dim3(WG), 0, st, a);
      }
    } else if (neighbours == 6) {
      hipLaunchKernelGGL((merge_kernel<6, false>), dim3(gx, (unsigned)V), dim3(WG), 0, st, a);
    } else {
      hipLaunchKernelGGL((merge_kernel<26, false>), dim3(gx, (unsigned)V), dim3(WG), 0, st, a);
    }
  }
  if (phases & GEOBO_BODIES_FLATTEN) hipLaunchKernelGGL(flatten_kernel, dim3(gx, (unsigned)V), dim3(WG), 0, st, a);
  if (phases & GEOBO_BODIES_STATS) {
    if (hipMemsetAsync(mark, 0, (size_t)V * n * 4, st) != hipSuccess) return GEOBO_E_LAUNCH;      // the parents are done with
    if (K > 0) {
      if (hipMemcpyAsync(dseeds, seeds, (size_t)K * 4, hipMemcpyHostToDevice, st) != hipSuccess) return GEOBO_E_LAUNCH;
      hipLaunchKernelGGL(seed_kernel, dim3((unsigned)((K + WG - 1) / WG), (unsigned)V), dim3(WG), 0, st, n, K, (const int32_t*)dseeds,
                         (const int32_t*)a.label, mark);
    }
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)V), dim3(WG), 0, st, n, min_count, (const int32_t*)a.label, (const int64_t*)a.size,
                       (const int32_t*)mark, stats);
    hipLaunchKernelGGL(sums_kernel, dim3((unsigned)nchunks, (unsigned)V), dim3(WG), 0, st, a, (const int32_t*)mark, (const int64_t*)stats, nchunks,
                       psum, pcnt);
    hipLaunchKernelGGL(sums_finish_kernel, dim3((unsigned)((V * NSUM + WG - 1) / WG)), dim3(WG), 0, st, (const double*)psum, (const int64_t*)pcnt, V,
                       nchunks, sums, stats);
    if (hits_largest || hits_seeded)
      hipLaunchKernelGGL(hits_kernel, dim3((unsigned)(((int64_t)C * n + WG - 1) / WG)), dim3(WG), 0, st, n, (int)S, C, (const int32_t*)a.label,
                         (const int32_t*)mark, (const int64_t*)stats, hits_largest, hits_seeded);
  }
  return hipGetLastError() == hipSuccess ? GEOBO_OK : GEOBO_E_LAUNCH;
}
