// The three passes of the exact anisotropic squared Euclidean distance transform, shared by surface.hip (the full field) and
// morph.hip (the field up to a radius).  d2 = ((sx2 dx^2 + sy2 dy^2) + sz2 dz^2) in float64, every product and sum rounded on its own: both
// files are compiled with fp contraction off.  Float64 addition and multiplication by a positive constant are monotone, so the minimum is
// taken axis by axis and has the bits of the brute-force minimum.
//
// `cap` bounds the two scans: they return min(cap, the exact minimum).  +inf gives the full transform.  A finite cap above a radius r2 makes
// every value <= r2 exact and every other value "far" (> r2), and ends a scan once the step alone costs cap or more: O(r / spacing) per voxel.
#pragma once
#include "common.h"

#pragma clang fp contract(off)                              // from here to the end of the including file: the scans must not fuse

constexpr int EDT_NONE = 0xFFFF;                            // no feature in this row of the box (a real distance is <= 8191)

// Rows: one wave per row of bw voxels, 64 columns at a time; feat(xb) tells whether column xb of the row is a feature (called for xb < bw
// only).  A ballot and one count-leading-zeros give every lane the nearest feature at or left of it, the last feature column is carried
// from chunk to chunk (wave-uniform); a second sweep from the right end (a feature is where the left distance is 0) takes the smaller one.
// g[xb] = the distance in columns, EDT_NONE in a row without a feature.  Returns whether the row has one (wave-uniform).  All 64 lanes call it.
template <class Feat>
__device__ __forceinline__ bool edt_row_pass(uint16_t* __restrict__ g, int bw, int lane, Feat feat) {
  const int chunks = (bw + 63) >> 6;
  int last = -1;                                            // wave-uniform: the last feature column seen so far
#pragma unroll 1
  for (int c = 0; c < chunks; ++c) {
    const int xb = c * 64 + lane;
    const bool live = xb < bw;
    const bool f = live && feat(xb);
    const unsigned long long m = __ballot(f);
    const unsigned long long below = m & (~0ull >> (63 - lane));
    const int dl = below ? lane - (63 - __clzll((long long)below)) : (last >= 0 ? xb - last : EDT_NONE);
    if (live) g[xb] = (uint16_t)dl;
    if (m) last = c * 64 + 63 - __clzll((long long)m);
  }
  if (last < 0) return false;                               // every element is EDT_NONE already
  int next = -1;                                            // the first feature column right of the chunk
#pragma unroll 1
  for (int c = chunks - 1; c >= 0; --c) {
    const int xb = c * 64 + lane;
    const bool live = xb < bw;
    const int dl = live ? (int)g[xb] : EDT_NONE;            // this lane's own store of the first sweep
    const unsigned long long m = __ballot(live && dl == 0);
    const unsigned long long above = m >> lane;
    const int dr = above ? __ffsll((long long)above) - 1 : (next >= 0 ? next - xb : EDT_NONE);
    if (live && dr < dl) g[xb] = (uint16_t)dr;
    if (m) next = c * 64 + __ffsll((long long)m) - 1;
  }
  return true;
}

// Columns: min(cap, min over y' of (sx2 g[y']^2 + sy2 (y' - yb)^2)); col[y' * bw] is element y' of the voxel's column.  Candidates in order
// of increasing |dy|; the scan stops once sy2 dy^2 is not below the best so far -- exact: the other term is >= 0 and rounding is monotone, so
// every later candidate is >= sy2 dy^2 >= best.
__device__ __forceinline__ double edt_scan_y(const uint16_t* __restrict__ col, int bw, int yb, int bh, double sx2, double sy2, double cap) {
  const int reach = max(yb, bh - 1 - yb);
  double best = cap;
#pragma unroll 1
  for (int k = 0; k <= reach; ++k) {
    const double dy2 = sy2 * ((double)k * (double)k);
    if (!(dy2 < best)) break;
    if (yb - k >= 0) {
      const int gx = col[(int64_t)(yb - k) * bw];
      if (gx != EDT_NONE) best = fmin(best, sx2 * ((double)gx * (double)gx) + dy2);
    }
    if (k > 0 && yb + k < bh) {
      const int gx = col[(int64_t)(yb + k) * bw];
      if (gx != EDT_NONE) best = fmin(best, sx2 * ((double)gx * (double)gx) + dy2);
    }
  }
  return best;
}

// z: min(cap, min over z' of (col[z' * plane] + sz2 (z' - zb)^2)), the same pruned scan
__device__ __forceinline__ double edt_scan_z(const double* __restrict__ col, int64_t plane, int zb, int bd, double sz2, double cap) {
  const int reach = max(zb, bd - 1 - zb);
  double best = cap;
#pragma unroll 1
  for (int k = 0; k <= reach; ++k) {
    const double dz2 = sz2 * ((double)k * (double)k);
    if (!(dz2 < best)) break;
    if (zb - k >= 0) best = fmin(best, col[(zb - k) * plane] + dz2);
    if (k > 0 && zb + k < bd) best = fmin(best, col[(zb + k) * plane] + dz2);
  }
  return best;
}
