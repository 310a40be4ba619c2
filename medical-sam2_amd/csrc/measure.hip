// Measurement step of the 3-D path: per-organ geometry, surface and intensity tables from a uint8 label volume [D, H, W] and, optionally, the
// image it was segmented from (int16 Hounsfield units or the uint8 grey of the intake), in one pass, gfx950.
//
// The host alternative copies both volumes to the host and runs one boolean mask plus a handful of numpy reductions per organ.  Here one
// kernel reads the labels (and the image under the organs) once and fills five small integer tables; volume, centroid, covariance, principal
// axes, surface area, mean / spread / percentiles follow from them on the host (volume_labels.measurements_from_tables).  Every table is an
// integer and the partials of the workgroups meet in global memory through integer add / min / max only, so no table depends on scheduling.
//
// msam2_label_measure, for the n <= LABEL_MAX_OBJ listed ids (a value not in ids is "not an organ", like the background):
//   moments int64 [n, 14]: count, Sz, Sy, Sx, Szz, Syy, Sxx, Szy, Szx, Syx, Sv, Svv, below, above  (sums over the organ's voxels of the
//                          voxel indices z, y, x, their products, the image value v and v^2; below / above = voxels with v < hist_lo /
//                          v >= hist_lo + bins; columns 10 - 13 are 0 without an image)
//   extent  int32 [n, 6]:  inclusive (z0, z1, y0, y1, x0, x1), all -1 when the organ is absent: label_stats' pre-set and unsigned-min trick
//                          (the table is pre-set to -1, the lower ends are minimised as UNSIGNED numbers, the upper ends maximised as signed)
//   vrange  int32 [n, 2]:  (min v, max v); (INT32_MAX, INT32_MIN) when the organ is absent or there is no image
//   faces   int64 [n, 6]:  (optional) interior faces per axis z, y, x -- pairs of axis neighbours of which exactly one is the organ; a face
//                          between two listed organs counts once for each -- then frame faces per axis z, y, x: faces of the organ's voxels
//                          on the first or on the last index of the axis that look out of the volume (a voxel of an axis of length 1 has two)
//   hist    int32 [n, bins]: (optional) voxels of the organ with v == hist_lo + b
//
// Bounds (D <= 65535, H, W <= 8192, D H W <= 2^31 - 2: LABEL_AT_MOST_2G_VOXELS; |v| <= 2^15):
//   Szz is the largest coordinate sum: at most H W (D - 1) D (2 D - 1) / 6 < D H W D^2 / 3 < 2^31 2^32 / 3 < 2^63;  Syy, Sxx <= 2^31 2^26.
//   Svv <= 2^31 2^30 = 2^61, |Sv| <= 2^46.  A band (below) has fewer than 2^15 voxels: its count, below / above, face counts and extents fit
//   32 bits; its Syy, Sxx, Syx (up to 2^15 2^26), Svv (2^15 2^30) and, for simplicity, every other sum are 64-bit from the lane up: a run's
//   and a lane's partials are 64-bit (a wave's Sv and tail counts, at most 2^25 and 2^10, travel as 32-bit words), the workgroup's tables
//   are 64-bit LDS counters, the global tables take 64-bit adds.
//
// Structure (label_stats_kernel's, csrc/prompts.hip): a workgroup owns a band of whole rows of one slice (about 16 KiB of labels).
//   * bytes in front of the first 16-byte boundary of the LABELS and behind the last one go through a scalar path (one thread each); in
//     between every lane loads 16 voxels at once.  W is arbitrary, so a lane's 16 voxels may straddle rows.
//   * a "plain" lane holds one value inside one row; neighbouring plain lanes of the same row and value form a segment, found by a ballot of
//     the segment heads, and only the head adds the run's geometry to LDS: the sums of y, x, yy, xx, yx over a run are closed forms in the
//     run's row, first column and length (z is the slice: its sums are products taken when the band leaves).  A wave of background costs
//     one ballot and no LDS access (with faces: plus the three neighbour compares below).
//   * the image is read only under listed organs.  Its alignment is independent of the labels': the 16 values of a plain lane come as
//     16-byte loads when the image address of the band's first chunk is 16-byte aligned (then every chunk's is), else element by element.
//     A segment's intensity partials (Sv, Svv, min, max, below, above) meet in its head by a segmented shuffle reduction over the wave.
//   * faces (compile-time option) need the +x, +y and +z neighbours only, each differing pair counted for both sides.  A plain lane whose
//     +y and +z chunks (unaligned 16-byte loads; the +y neighbour of the band's last row and the +z neighbour belong to another workgroup's
//     band or slice and are simply read) and whose next byte in the row repeat its value has no face; where a chunk differs, the lane adds the
//     faces run by run of the neighbour's values, from registers.  Any other lane walks its voxels and reads their neighbours byte by byte.
//   * histogram (compile-time option): private to the workgroup in LDS, HIST_LDS_WORDS counters (16 KiB: eight workgroups
//     still fit a CU) for `group` = HIST_LDS_WORDS / bins organs at a time: after the main pass the band is read again (from the cache) once
//     per group of organs that has a voxel in the band, and the non-zero bins leave with global adds; only the bins between the organ's
//     (min v, max v) in the band are cleared and looked at.  256 bins: 16 organs per pass.  4096 bins, 13 organs: one organ per pass, so a
//     band takes as many passes as it holds organs.  More than HIST_LDS_WORDS bins: global adds per voxel.
//   * the band's partials leave with one atomic per non-zero table element; an extent or range the band cannot move (a look first) costs none.
// All tables are pre-set by one small kernel on the caller's stream: no allocation, no host synchronisation, no workspace.
#include <limits.h>

#include "common.h"

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_BAND_BYTES = 16384;      // a band is the fewest whole rows that reach this: fewer than 16384 + 8192 voxels
constexpr int HIST_LDS_WORDS = 4096;      // 16 KiB of private histogram per workgroup
constexpr int MS_MAX_BINS = 65536;
constexpr int IMG_NONE = 0, IMG_I16 = 1, IMG_U8 = 2;   // kernel variants; the ABI's image_type is volume_prep's: 0 uint8, 1 int16

enum { S_CNT, S_Y, S_X, S_YY, S_XX, S_YX, S_V, S_VV, S_N };

struct MeasureTables {                    // LDS of one workgroup
  unsigned long long s[LABEL_MAX_OBJ][S_N];
  int y0[LABEL_MAX_OBJ], y1[LABEL_MAX_OBJ], x0[LABEL_MAX_OBJ], x1[LABEL_MAX_OBJ];
  int vmin[LABEL_MAX_OBJ], vmax[LABEL_MAX_OBJ], below[LABEL_MAX_OBJ], above[LABEL_MAX_OBJ];
  int faces[LABEL_MAX_OBJ][6];            // interior z, y, x; frame: unused, y, x (z follows from the count)
  signed char lut[256];                   // label value -> object index, -1 = not listed
};

struct MeasureArgs {
  const uint8_t* labels;
  const uint8_t* ids;
  const void* image;
  int n, D, H, W, band_rows, hist_lo, bins, hist_group;   // hist_group: organs per LDS histogram pass, 0 = global adds per voxel
  unsigned long long* moments;
  int* extent;
  int* vrange;
  unsigned long long* faces;
  int* hist;
};

template <int IMG>
__device__ __forceinline__ int image_value(const void* image, int64_t i) {
  if constexpr (IMG == IMG_I16) return reinterpret_cast<const int16_t*>(image)[i];
  else return reinterpret_cast<const uint8_t*>(image)[i];
}

// the intensity partial of some voxels of one organ
struct Intensity {
  long long sv = 0, svv = 0;
  int vmin = INT_MAX, vmax = INT_MIN, below = 0, above = 0;
  __device__ __forceinline__ void add(int v, int hist_lo, int bins) {
    sv += v;
    svv += (long long)(v * v);                               // |v| <= 2^15: the product fits
    vmin = min(vmin, v);
    vmax = max(vmax, v);
    const long long b = (long long)v - hist_lo;
    below += b < 0;
    above += b >= bins;
  }
};

__device__ __forceinline__ void add_intensity(MeasureTables& t, int j, const Intensity& q) {
  atomicAdd(&t.s[j][S_V], (unsigned long long)q.sv);
  atomicAdd(&t.s[j][S_VV], (unsigned long long)q.svv);
  atomicMin(&t.vmin[j], q.vmin);
  atomicMax(&t.vmax[j], q.vmax);
  if (q.below) atomicAdd(&t.below[j], q.below);
  if (q.above) atomicAdd(&t.above[j], q.above);
}

// a run of len voxels of object j in row y (of the slice) from column x on
template <bool FACES>
__device__ __forceinline__ void add_run(MeasureTables& t, int j, int y, int x, int len, int H, int W) {
  if (j < 0 || len <= 0) return;
  const unsigned long long L = len, X = x, Y = y;
  const unsigned long long sx = L * X + L * (L - 1) / 2;                                     // sum of x .. x + L - 1
  const unsigned long long sxx = L * X * X + X * L * (L - 1) + (L - 1) * L * (2 * L - 1) / 6;  // sum of their squares
  atomicAdd(&t.s[j][S_CNT], L);
  atomicAdd(&t.s[j][S_Y], Y * L);
  atomicAdd(&t.s[j][S_X], sx);
  atomicAdd(&t.s[j][S_YY], Y * Y * L);
  atomicAdd(&t.s[j][S_XX], sxx);
  atomicAdd(&t.s[j][S_YX], Y * sx);
  atomicMin(&t.y0[j], y);
  atomicMax(&t.y1[j], y);
  atomicMin(&t.x0[j], x);
  atomicMax(&t.x1[j], x + len - 1);
  if constexpr (FACES) {
    const int fy = (y == 0 ? len : 0) + (y == H - 1 ? len : 0), fx = (x == 0) + (x + len == W);
    if (fy) atomicAdd(&t.faces[j][4], fy);
    if (fx) atomicAdd(&t.faces[j][5], fx);
  }
}

__device__ __forceinline__ void add_face(MeasureTables& t, int ja, int jb, int axis) {
  if (ja == jb) return;
  if (ja >= 0) atomicAdd(&t.faces[ja][axis], 1);
  if (jb >= 0) atomicAdd(&t.faces[jb][axis], 1);
}

// what the walks need of the band: p = its first voxel, voxel0 = that voxel's index in the volume, y0 = its row
struct Band {
  const uint8_t* p;
  int64_t voxel0, plane;                  // plane = H * W
  int z, y0;
};

// the interior faces behind the voxels [o, o + len) of the band (their +x, +y and +z neighbours, read from memory)
__device__ __forceinline__ void walk_faces(MeasureTables& t, const MeasureArgs& a, const Band& b, int o, int len) {
  int row = o / a.W, col = o - row * a.W;
  for (int e = 0; e < len; ++e) {
    const uint8_t* q = b.p + o + e;
    const int j = t.lut[q[0]];
    if (col + 1 < a.W) add_face(t, j, t.lut[q[1]], 2);
    if (b.y0 + row + 1 < a.H) add_face(t, j, t.lut[q[a.W]], 1);
    if (b.z + 1 < a.D) add_face(t, j, t.lut[q[b.plane]], 0);
    if (++col == a.W) col = 0, ++row;
  }
}

// The voxels [o, o + len) of the band (len <= 16): runs of one object inside one row are added whole, with their intensity partial.
template <int IMG, bool FACES>
__device__ __forceinline__ void walk_voxels(MeasureTables& t, const MeasureArgs& a, const Band& b, int o, int len) {
  int row = o / a.W, col = o - row * a.W;
  int cj = -1, crow = 0, ccol = 0, clen = 0;
  Intensity q;
  for (int e = 0; e < len; ++e) {
    const int j = t.lut[b.p[o + e]];
    if (j == cj && col != 0) {
      ++clen;
    } else {
      add_run<FACES>(t, cj, b.y0 + crow, ccol, clen, a.H, a.W);
      if (IMG != IMG_NONE && cj >= 0) add_intensity(t, cj, q);
      q = Intensity();
      cj = j, crow = row, ccol = col, clen = 1;
    }
    if constexpr (IMG != IMG_NONE) {
      if (j >= 0) q.add(image_value<IMG>(a.image, b.voxel0 + o + e), a.hist_lo, a.bins);
    }
    if (++col == a.W) col = 0, ++row;
  }
  add_run<FACES>(t, cj, b.y0 + crow, ccol, clen, a.H, a.W);
  if (IMG != IMG_NONE && cj >= 0) add_intensity(t, cj, q);
  if constexpr (FACES) walk_faces(t, a, b, o, len);
}

__device__ __forceinline__ uint4 load16_unaligned(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
__device__ __forceinline__ bool same16(const uint4& a, const uint4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

__device__ __forceinline__ unsigned byte_of(const uint4& v, int e) {
  const unsigned w = e < 8 ? (e < 4 ? v.x : v.y) : (e < 12 ? v.z : v.w);
  return (w >> ((e & 3) << 3)) & 0xffu;
}

// the 16 image values from voxel i of the volume on; wide: their address is 16-byte aligned
template <int IMG>
__device__ __forceinline__ void values16(int (&val)[16], const MeasureArgs& a, int64_t i, bool wide) {
  if (wide) {
    if constexpr (IMG == IMG_I16) {
      const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const int16_t*>(a.image) + i);
      const uint4 lo = src[0], hi = src[1];
      const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        val[2 * e] = (int)(int16_t)(w[e] & 0xffffu);
        val[2 * e + 1] = (int)(int16_t)(w[e] >> 16);
      }
    } else {
      const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.image) + i);
#pragma unroll
      for (int e = 0; e < 16; ++e) val[e] = (int)byte_of(u, e);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) val[e] = image_value<IMG>(a.image, i + e);
  }
}

// the faces between the 16 voxels of a plain lane (value `first`, object j) and their neighbours nb along one axis, runs of one
// neighbour value added whole
__device__ __forceinline__ void faces_vs_chunk(MeasureTables& t, int j, unsigned first, const uint4& nb, int axis) {
  unsigned cur = first;
  int run = 0;
  auto flush = [&]() {
    if (cur == first || run == 0) return;
    const int jn = t.lut[cur];
    if (jn == j) return;
    if (j >= 0) atomicAdd(&t.faces[j][axis], run);
    if (jn >= 0) atomicAdd(&t.faces[jn][axis], run);
  };
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const unsigned v = byte_of(nb, e);
    if (v == cur) {
      ++run;
    } else {
      flush();
      cur = v, run = 1;
    }
  }
  flush();
}

// One histogram pass over the band's `bytes` voxels for the objects [g0, g1): add(j, bin) for every voxel of them inside the range.
// 16 voxels per lane from the band's first voxel on (the labels by unaligned loads), the rest one by one.
template <int IMG, typename Add>
__device__ __forceinline__ void hist_pass(const MeasureTables& t, const MeasureArgs& a, const Band& b, int bytes, int g0, int g1, Add add) {
  auto count = [&](int j, int v) {
    const long long bin = (long long)v - a.hist_lo;
    if (bin >= 0 && bin < a.bins) add(j, (int)bin);
  };
  const int nchunk = bytes >> 4;
  const bool wide = (((uintptr_t)a.image + (uintptr_t)b.voxel0 * (IMG == IMG_I16 ? 2 : 1)) & 15) == 0;
  for (int c = threadIdx.x; c < nchunk; c += MS_THREADS) {
    const int o = c << 4;
    const uint4 v = load16_unaligned(b.p + o);
    const unsigned first = v.x & 0xffu;
    const bool uniform = v.x == first * 0x01010101u && v.y == v.x && v.z == v.x && v.w == v.x;
    const int jf = t.lut[first];
    if (uniform && (jf < g0 || jf >= g1)) continue;
    int val[16];
    if (uniform) {
      values16<IMG>(val, a, b.voxel0 + o, wide);
#pragma unroll
      for (int e = 0; e < 16; ++e) count(jf, val[e]);
    } else {
      for (int e = 0; e < 16; ++e) {
        const int j = t.lut[byte_of(v, e)];
        if (j >= g0 && j < g1) count(j, image_value<IMG>(a.image, b.voxel0 + o + e));
      }
    }
  }
  for (int i = (nchunk << 4) + threadIdx.x; i < bytes; i += MS_THREADS) {
    const int j = t.lut[b.p[i]];
    if (j >= g0 && j < g1) count(j, image_value<IMG>(a.image, b.voxel0 + i));
  }
}

// Min / max into a global table element that only ever moves one way: a look first (any value the element has held since the call's
// pre-set will do) spares the atomic wherever the band cannot move it -- most bands of an organ.
__device__ __forceinline__ int peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lower_unsigned(int* p, int v) {
  if ((unsigned)peek(p) > (unsigned)v) atomicMin(reinterpret_cast<unsigned*>(p), (unsigned)v);
}
__device__ __forceinline__ void lower_signed(int* p, int v) {
  if (peek(p) > v) atomicMin(p, v);
}
__device__ __forceinline__ void raise_signed(int* p, int v) {
  if (peek(p) < v) atomicMax(p, v);
}

__global__ __launch_bounds__(MS_THREADS) void measure_init_kernel(MeasureArgs a) {
  const int n = a.n;
  const int64_t nh = a.hist ? (int64_t)n * a.bins : 0;
  const int64_t total = nh > n * 14 ? nh : n * 14;
  for (int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * MS_THREADS) {
    if (i < n * 14) a.moments[i] = 0;
    if (i < n * 6) a.extent[i] = -1;
    if (i < n * 2) a.vrange[i] = (i & 1) ? INT_MIN : INT_MAX;
    if (a.faces && i < n * 6) a.faces[i] = 0;
    if (i < nh) a.hist[i] = 0;
  }
}

// blockIdx.x = band of `band_rows` rows, blockIdx.y = slice
template <int IMG, bool FACES, bool HIST>
__global__ __launch_bounds__(MS_THREADS) void label_measure_kernel(MeasureArgs a) {
  static_assert(!HIST || IMG != IMG_NONE, "a histogram needs an image");
  __shared__ MeasureTables t;
  const int tid = threadIdx.x, lane = tid & 63, z = blockIdx.y, n = a.n, H = a.H, W = a.W;
  const int y0 = blockIdx.x * a.band_rows, nrows = min(a.band_rows, H - y0);
  for (int i = tid; i < LABEL_MAX_OBJ * S_N; i += MS_THREADS) (&t.s[0][0])[i] = 0;
  for (int i = tid; i < LABEL_MAX_OBJ * 6; i += MS_THREADS) (&t.faces[0][0])[i] = 0;
  if (tid < LABEL_MAX_OBJ) {
    t.y0[tid] = t.x0[tid] = t.vmin[tid] = INT_MAX;
    t.y1[tid] = t.x1[tid] = -1;
    t.vmax[tid] = INT_MIN;
    t.below[tid] = t.above[tid] = 0;
  }
  ids_to_object_table(t.lut, a.ids, n, tid);

  Band b;
  b.plane = (int64_t)H * W;
  b.voxel0 = (int64_t)z * b.plane + (int64_t)y0 * W;
  b.p = a.labels + b.voxel0;
  b.z = z;
  b.y0 = y0;
  const uint8_t* p = b.p;                                   // the band: `bytes` consecutive voxels
  const int bytes = nrows * W;                              // < MS_BAND_BYTES + W
  const int head = min(bytes, (int)((16 - ((uintptr_t)p & 15)) & 15));
  const int nvec = (bytes - head) >> 4, tail = bytes - head - (nvec << 4);
  if (tid == 0 && head > 0) walk_voxels<IMG, FACES>(t, a, b, 0, head);
  if (tid == 64 && tail > 0) walk_voxels<IMG, FACES>(t, a, b, head + (nvec << 4), tail);
  bool wide = false;                                        // every chunk's image address is 16-byte aligned iff the first one's is
  if constexpr (IMG != IMG_NONE)
    wide = (((uintptr_t)a.image + (uintptr_t)(b.voxel0 + head) * (IMG == IMG_I16 ? 2 : 1)) & 15) == 0;
  const uint4* pv = reinterpret_cast<const uint4*>(p + head);
  for (int base = 0; base < nvec; base += MS_THREADS) {     // wave-uniform bound: the shuffle and the ballot below see whole waves
    const int c = base + tid;
    const bool live = c < nvec;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (live) v = pv[c];
    const int o = head + (c << 4);
    const int row = live ? o / W : 0, col = o - row * W;
    const unsigned first = v.x & 0xffu;
    const bool plain = live && col + 16 <= W && v.x == first * 0x01010101u && v.y == v.x && v.z == v.x && v.w == v.x;
    // segments of neighbouring plain lanes with the same (row, value): consecutive lanes hold consecutive voxels, so a segment of m lanes
    // is one run of 16 m voxels that starts at its head's column
    const int key = plain ? (int)((row << 8) | first) : -1;
    const int prev = __shfl_up(key, 1);
    const unsigned long long heads = __ballot(lane == 0 || key < 0 || key != prev);
    const int j = plain ? t.lut[first] : -1;
    const bool is_head = (heads >> lane) & 1;
    if constexpr (IMG != IMG_NONE) {
      // the intensity partials of a segment's lanes meet in its head by a segmented reduction over the wave (lane l takes lane l + d's
      // partial iff no segment starts in (l, l + d]): one set of LDS updates per segment here too.  A wave without an organ skips it.
      const bool organ = plain && j >= 0;
      if (__ballot(organ)) {
        Intensity q;
        if (organ) {
          int val[16];
          values16<IMG>(val, a, b.voxel0 + o, wide);
#pragma unroll
          for (int e = 0; e < 16; ++e) q.add(val[e], a.hist_lo, a.bins);
        }
        int sv = (int)q.sv, tails = q.below | (q.above << 16);          // a wave's |Sv| <= 2^10 2^15, its tail counts <= 2^10 each
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const int o_sv = __shfl_down(sv, d), o_min = __shfl_down(q.vmin, d), o_max = __shfl_down(q.vmax, d), o_tails = __shfl_down(tails, d);
          const long long o_svv = __shfl_down(q.svv, d);
          if (lane + d < 64 && ((heads >> (lane + 1)) & ((1ull << d) - 1ull)) == 0) {
            sv += o_sv, q.svv += o_svv, tails += o_tails;
            q.vmin = min(q.vmin, o_min), q.vmax = max(q.vmax, o_max);
          }
        }
        if (organ && is_head) {
          q.sv = sv, q.below = tails & 0xffff, q.above = tails >> 16;
          add_intensity(t, j, q);
        }
      }
    }
    if (plain) {
      if (is_head) add_run<FACES>(t, j, y0 + row, col, run_length(heads, lane) << 4, H, W);
      if constexpr (FACES) {
        if (col + 16 < W) {                                 // the +x neighbour of the lane's last voxel (the others are in v)
          const unsigned nb = p[o + 16];
          if (nb != first) add_face(t, j, t.lut[nb], 2);
        }
        if (y0 + row + 1 < H) {
          const uint4 nb = load16_unaligned(p + o + W);
          if (!same16(v, nb)) faces_vs_chunk(t, j, first, nb, 1);
        }
        if (z + 1 < a.D) {
          const uint4 nb = load16_unaligned(p + o + b.plane);
          if (!same16(v, nb)) faces_vs_chunk(t, j, first, nb, 0);
        }
      }
    } else if (live) {
      walk_voxels<IMG, FACES>(t, a, b, o, 16);
    }
  }
  __syncthreads();

  // the band's partials: one atomic per non-zero element.  The sums that involve z are products with the slice index.
  const unsigned long long Z = (unsigned long long)z;
  for (int i = tid; i < n * 14; i += MS_THREADS) {
    const int j = i / 14, k = i - j * 14;
    const unsigned long long* s = t.s[j];
    if (s[S_CNT] == 0) continue;
    unsigned long long x = 0;
    switch (k) {
      case 0: x = s[S_CNT]; break;
      case 1: x = Z * s[S_CNT]; break;
      case 2: x = s[S_Y]; break;
      case 3: x = s[S_X]; break;
      case 4: x = Z * Z * s[S_CNT]; break;
      case 5: x = s[S_YY]; break;
      case 6: x = s[S_XX]; break;
      case 7: x = Z * s[S_Y]; break;
      case 8: x = Z * s[S_X]; break;
      case 9: x = s[S_YX]; break;
      case 10: x = s[S_V]; break;
      case 11: x = s[S_VV]; break;
      case 12: x = (unsigned long long)t.below[j]; break;
      default: x = (unsigned long long)t.above[j]; break;
    }
    if (x) atomicAdd(a.moments + i, x);
  }
  for (int i = tid; i < n * 6; i += MS_THREADS) {
    const int j = i / 6, k = i - j * 6;
    if (t.s[j][S_CNT] == 0) continue;
    int* e = a.extent + i;
    switch (k) {
      case 0: lower_unsigned(e, z); break;
      case 1: raise_signed(e, z); break;
      case 2: lower_unsigned(e, t.y0[j]); break;
      case 3: raise_signed(e, t.y1[j]); break;
      case 4: lower_unsigned(e, t.x0[j]); break;
      default: raise_signed(e, t.x1[j]); break;
    }
    if constexpr (IMG != IMG_NONE) {
      if (k == 0) lower_signed(a.vrange + 2 * j, t.vmin[j]);
      if (k == 1) raise_signed(a.vrange + 2 * j + 1, t.vmax[j]);
    }
  }
  if constexpr (FACES) {                                    // (an organ without a voxel in the band can own faces of it: its +y / +z side)
    for (int i = tid; i < n * 6; i += MS_THREADS) {
      const int j = i / 6, k = i - j * 6;
      const unsigned long long f = k == 3 ? t.s[j][S_CNT] * (unsigned long long)((z == 0) + (z == a.D - 1)) : (unsigned long long)t.faces[j][k];
      if (f) atomicAdd(a.faces + i, f);
    }
  }

  if constexpr (HIST) {
    __shared__ int hist[HIST_LDS_WORDS];
    const int bins = a.bins, G = a.hist_group;
    if (G == 0) {
      int* out = a.hist;
      hist_pass<IMG>(t, a, b, bytes, 0, n, [&](int j, int bin) { atomicAdd(out + (int64_t)j * bins + bin, 1); });
    } else {
      for (int g0 = 0; g0 < n; g0 += G) {                   // everything below branches on values the whole workgroup shares
        const int g1 = min(n, g0 + G);
        bool any = false;
        for (int j = g0; j < g1; ++j) any |= t.s[j][S_CNT] != 0;
        if (!any) continue;
        // organ j's voxels of the band lie in the bins [b0, b1) of its (min v, max v): only those are cleared, and looked at afterwards
        auto first_bin = [&](int j) { return (int)min(max((long long)t.vmin[j] - a.hist_lo, 0ll), (long long)bins); };
        auto end_bin = [&](int j) { return (int)min(max((long long)t.vmax[j] - a.hist_lo + 1, 0ll), (long long)bins); };
        for (int j = g0; j < g1; ++j)                       // (g1 - g0) * bins <= HIST_LDS_WORDS
          for (int i = first_bin(j) + tid; i < end_bin(j); i += MS_THREADS) hist[(j - g0) * bins + i] = 0;
        __syncthreads();
        hist_pass<IMG>(t, a, b, bytes, g0, g1, [&](int j, int bin) { atomicAdd(&hist[(j - g0) * bins + bin], 1); });
        __syncthreads();
        for (int j = g0; j < g1; ++j)
          for (int i = first_bin(j) + tid; i < end_bin(j); i += MS_THREADS) {
            const int c = hist[(j - g0) * bins + i];
            if (c) atomicAdd(a.hist + (int64_t)j * bins + i, c);
          }
        __syncthreads();
      }
    }
  }
}

template <int IMG, bool FACES, bool HIST>
void launch_measure(const MeasureArgs& a, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((label_measure_kernel<IMG, FACES, HIST>), grid, dim3(MS_THREADS), 0, s, a);
}
template <int IMG>
void launch_measure_image(const MeasureArgs& a, dim3 grid, hipStream_t s) {
  if constexpr (IMG == IMG_NONE) {
    if (a.faces) launch_measure<IMG, true, false>(a, grid, s);
    else launch_measure<IMG, false, false>(a, grid, s);
  } else {
    if (a.faces && a.hist) launch_measure<IMG, true, true>(a, grid, s);
    else if (a.faces) launch_measure<IMG, true, false>(a, grid, s);
    else if (a.hist) launch_measure<IMG, false, true>(a, grid, s);
    else launch_measure<IMG, false, false>(a, grid, s);
  }
}

}  // namespace

// image: NULL (geometry only) or the volume the labels belong to, image_type 0 uint8, 1 int16 (2-byte aligned).  faces and hist may be NULL.
// below / above (moments columns 12, 13) split at hist_lo and hist_lo + bins whether or not hist is given (bins = 0: at hist_lo alone).
extern "C" int msam2_label_measure(const uint8_t* labels, const uint8_t* ids, const void* image, int image_type, int64_t D, int64_t H, int64_t W,
                                   int64_t n, int hist_lo, int64_t bins, int64_t* moments, int* extent, int* vrange, int64_t* faces, int* hist,
                                   void* stream) {
  MSAM2_REQUIRE(labels && ids && moments && extent && vrange, "label_measure: null labels / ids / moments / extent / vrange");
  LABEL_REQUIRE_OBJECTS("label_measure", n);
  LABEL_REQUIRE_SIZES("label_measure", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(!image || image_type == 0 || image_type == 1, "label_measure: image_type %d (0 uint8, 1 int16)", image_type);
  MSAM2_REQUIRE(!image || image_type == 0 || ((uintptr_t)image & 1) == 0, "label_measure: an int16 image must be 2-byte aligned");
  MSAM2_REQUIRE(bins >= (hist ? 1 : 0) && bins <= MS_MAX_BINS, "label_measure: bins = %lld (1 .. %d with a histogram, 0 .. %d without)",
                (long long)bins, MS_MAX_BINS, MS_MAX_BINS);
  MSAM2_REQUIRE(!hist || image, "label_measure: a histogram needs an image");
  hipStream_t s = (hipStream_t)stream;
  int64_t band = cdiv(MS_BAND_BYTES, W);
  band = band < H ? band : H;
  MeasureArgs a;
  a.labels = labels, a.ids = ids, a.image = image;
  a.n = (int)n, a.D = (int)D, a.H = (int)H, a.W = (int)W, a.band_rows = (int)band, a.hist_lo = hist_lo, a.bins = (int)bins;
  a.hist_group = hist ? (int)(HIST_LDS_WORDS / bins) : 0;
  a.moments = reinterpret_cast<unsigned long long*>(moments), a.extent = extent, a.vrange = vrange;
  a.faces = reinterpret_cast<unsigned long long*>(faces), a.hist = hist;
  const int64_t cells = hist ? n * bins : n * 14;
  hipLaunchKernelGGL(measure_init_kernel, dim3(grid1d(cells > n * 14 ? cells : n * 14, 1024)), dim3(MS_THREADS), 0, s, a);
  if (const int rc = msam2_check_launch("label_measure (init)")) return rc;
  const dim3 grid(cdiv(H, band), (unsigned)D);
  if (!image) launch_measure_image<IMG_NONE>(a, grid, s);
  else if (image_type == 1) launch_measure_image<IMG_I16>(a, grid, s);
  else launch_measure_image<IMG_U8>(a, grid, s);
  return msam2_check_launch("label_measure");
}
