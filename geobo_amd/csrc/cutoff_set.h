// cutoff_set.h -- the set that grade-tonnage curves, geobodies and drill intercepts reduce realisations against (DESIGN.md
// sections 17 to 19), defined once:
//
//   {v : F[s][p][v] >= t[c],  F[s][q][v] >= lo[q] for the other two properties q,  mask[v] != 0,  NaN fails}
//
// for S realisations F[s][a][v] (a = 0, 1, 2; sample and property strides given) and C ascending thresholds.  A kernel's argument
// struct says so in the fields
//
//   const double* F;  int64_t sstride, n;  int C;
//   int64_t off[3];                   element offsets of the properties p, (p + 1) % 3, (p + 2) % 3 within a sample
//   int read[3];                      the property of that slot is read: slot 0 always, the others when their bound is > -inf
//   double lo[3];                     lower bound of that slot (slot 0: not used)
//   double t[CMAX];  const uint8_t* mask;
//
// which CutArgs, BodyArgs and TraceArgs each declare in the order their kernels were compiled and measured with (a common base
// struct would move them: the device code of the three sources is instruction for instruction that of their own structs).
// cutoff_set_of validates the arguments and fills those fields, for any of the three, on the host before any device access.
#pragma once
#include <math.h>
#include <stdint.h>

namespace {

constexpr int CMAX = 32;            // thresholds at most

// false for a null F, t or lo, p outside 0 .. 2, C outside 1 .. CMAX, a NaN or descending threshold, a NaN bound, strides that let
// the properties of a sample or the samples overlap, or S sstride beyond an int64.  t and lo are host arrays.
template <class Args>
bool cutoff_set_of(int64_t S, const double* F, int64_t sstride, int64_t pstride, int64_t n, int p, int C, const double* t,
                   const double* lo, const uint8_t* mask, Args& a) {
  if (!F || !t || !lo || p < 0 || p > 2 || C < 1 || C > CMAX) return false;
  for (int c = 0; c < C; ++c) {
    if (t[c] != t[c] || (c > 0 && t[c] < t[c - 1])) return false;           // NaN, or not ascending
  }
  for (int q = 0; q < 3; ++q) {
    if (lo[q] != lo[q]) return false;
  }
  if (pstride < n || pstride > INT64_MAX / 4 || sstride < 2 * pstride + n) return false;
  if (S > 0 && sstride > INT64_MAX / S) return false;
  a.F = F; a.sstride = sstride; a.n = n;
  a.C = C;
  for (int j = 0; j < 3; ++j) {
    const int q = (p + j) % 3;
    a.off[j] = q * pstride;
    a.lo[j] = lo[q];
    a.read[j] = j == 0 || lo[q] > -INFINITY;
  }
  for (int c = 0; c < CMAX; ++c) a.t[c] = c < C ? t[c] : 0.0;
  a.mask = mask;
  return true;
}

}  // namespace
