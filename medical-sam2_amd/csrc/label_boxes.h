// What the label-volume entries that work per organ inside a host-supplied bounding box share (surface.hip, holes.hip, morph.hip; the
// neighbour rows and the run heads also components.hip): one definition each.  DESIGN 7.19 states the contract.
//   * A box is six HOST integers (z0, z1, y0, y1, x0, x1), inclusive, inside the D x H x W volume; the kernels get it by value as a
//     LabelBox (first voxel and extent), the first sub-object of every organ job, so the jobs of all three files start alike.
//   * An entry with an out volume (holes, morph) first makes out a copy of labels; when out IS labels the copy goes to the workspace
//     instead and every launch reads the input from there: in place gives the bytes of the out-of-place call.
//   * Organs go through in groups whose tables fit the workspace, in the order of ids; one organ alone always fits.
#pragma once
#include "common.h"

namespace {

struct LabelBox {
  int z0, y0, x0, bd, bh, bw;                               // first voxel and extent
};

// Is the box upright and inside a D x H x W volume?
static inline bool label_box_ok(const int32_t* b, int64_t D, int64_t H, int64_t W) {
  return b[0] >= 0 && b[0] <= b[1] && b[1] < D && b[2] >= 0 && b[2] <= b[3] && b[3] < H && b[4] >= 0 && b[4] <= b[5] && b[5] < W;
}
// (of a box that label_box_ok accepted)
static inline LabelBox label_box(const int32_t* b) { return {b[0], b[2], b[4], b[1] - b[0] + 1, b[3] - b[2] + 1, b[5] - b[4] + 1}; }
__host__ __device__ __forceinline__ int64_t label_box_rows(const LabelBox& b) { return (int64_t)b.bd * b.bh; }
__host__ __device__ __forceinline__ int64_t label_box_voxels(const LabelBox& b) { return (int64_t)b.bd * b.bh * b.bw; }

// Box voxel i in the box's raster order: position in the box, index in the volume.  I: int64_t, or int where the entry holds a voxel
// index in an int32 anyway (holes.hip: a voxel of the volume is below 2^31 - 2, and 32-bit divisions are what its kernels are made of).
template <typename I>
struct LabelBoxVoxel {
  int zb, yb, xb;
  I g;
  __device__ __forceinline__ LabelBoxVoxel(I i, const LabelBox& o, int H, int W) {
    const I r = i / o.bw;
    xb = (int)(i - r * o.bw);
    zb = (int)(r / o.bh);
    yb = (int)(r - (I)zb * o.bh);
    g = ((I)(o.z0 + zb) * H + o.y0 + yb) * W + o.x0 + xb;
  }
};

// A spacing is usable iff its square is a normal float64 and 2^36 times it is finite: the largest squared index difference is below 2^33, so
// no product or sum overflows (inf * 0 would be NaN at a feature voxel) and no square flushes to 0 or loses bits as a subnormal.  False for NaN.
constexpr double LABEL_MIN_SPACING2 = 2.2250738585072014e-308, LABEL_MAX_SPACING2 = 1.7976931348623157e308 / 68719476736.0;
static inline bool label_spacing_ok(double s) { return s > 0.0 && s * s >= LABEL_MIN_SPACING2 && s * s <= LABEL_MAX_SPACING2; }
// The row pass of edt_passes.h runs one wave per row of the box in one launch: 64 threads per row must stay below 2^32 in all (2^25 rows:
// half of that).
constexpr int64_t LABEL_MAX_BOX_ROWS = 1ll << 25;

__host__ __device__ __forceinline__ long long label_round8(long long b) { return (b + 7) & ~7ll; }
static inline size_t label_round16(size_t b) { return (b + 15) & ~(size_t)15; }

// ---- the out volume, the snapshot of an in-place call and the counters ------------------------------------------------------------------
// For the sources that define LABEL_BOXES_OUT before the include (holes.hip, morph.hip): a __global__ function goes into the code object of
// every source that sees it, called or not.
#ifdef LABEL_BOXES_OUT
// (a kernel, not hipMemcpyAsync: see fill_kernel in common.h)
__global__ void label_copy_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t n, int vec) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {                                                // both 16-byte aligned: the tail by bytes
    const int64_t n16 = n / 16;
    for (int64_t i = t; i < n16; i += step) ((int4*)dst)[i] = ((const int4*)src)[i];
    for (int64_t i = n16 * 16 + t; i < n; i += step) dst[i] = src[i];
  } else {
    for (int64_t i = t; i < n; i += step) dst[i] = src[i];
  }
}

// The workspace of such an entry: LABEL_WS_HEAD_BYTES (it is never empty), the snapshot of the input when the call is in place, then
// what the entry adds.  Everything is 16-byte granular.
constexpr size_t LABEL_WS_HEAD_BYTES = 16;
static inline size_t label_input_bytes(int64_t N, bool in_place) { return LABEL_WS_HEAD_BYTES + (in_place ? label_round16((size_t)N) : 0); }

// Makes out the copy of labels (in place: the workspace's snapshot) and zeroes the n x 4 counters of info.  Returns the input every later
// launch reads: labels, or its snapshot.  The workspace holds label_input_bytes(N, out == labels) for it.
static inline const uint8_t* label_begin_out(const uint8_t* labels, uint8_t* out, int64_t N, char* ws, int32_t* info, int64_t n, hipStream_t s) {
  const bool in_place = out == labels;
  uint8_t* copy_to = in_place ? (uint8_t*)(ws + LABEL_WS_HEAD_BYTES) : out;
  hipLaunchKernelGGL(label_copy_kernel, dim3(grid1d(N, 4096, 256 * 16)), dim3(256), 0, s, labels, copy_to, N,
                     (int)((((uintptr_t)labels | (uintptr_t)copy_to) & 15) == 0));
  fill_on(s, info, n * 4, 0);
  return in_place ? copy_to : labels;
}
#endif

// ---- groups ---------------------------------------------------------------------------------------------------------------------------
// bytes[j]: the tables of organ j, 0 for an organ that has nothing to do (it joins no group).  What all organs need at once, or the
// largest one alone:
static inline size_t label_tables_bytes(const size_t* bytes, int64_t n, bool all_at_once) {
  size_t sum = 0, largest = 0;
  for (int64_t j = 0; j < n; ++j) sum += bytes[j], largest = bytes[j] > largest ? bytes[j] : largest;
  return all_at_once ? sum : largest;
}
// The next group: the live organs from j on, as long as their tables fit `room` (one alone always fits: the entry refused a workspace
// below its largest).  take(j, offset) for every member, offset: where its tables start within the room.  Returns the organ the
// group after this one starts at, n after the last group.
template <typename F>
static inline int label_next_group(const size_t* bytes, int n, int j, size_t room, F&& take) {
  size_t used = 0;
  for (; j < n; ++j) {
    if (!bytes[j]) continue;
    if (used > 0 && used + bytes[j] > room) break;
    take(j, used);
    used += bytes[j];
  }
  return j;
}

// ---- refusals, in the style of LABEL_REQUIRE_SIZES (entry, name: string literals) ---------------------------------------------------------
#define LABEL_REQUIRE_BOX(entry, j, bx, D, H, W)                                                                                            \
  MSAM2_REQUIRE(label_box_ok(bx, D, H, W), entry ": box %d (%d..%d, %d..%d, %d..%d) is inverted or outside the %lld x %lld x %lld volume", j, \
                (bx)[0], (bx)[1], (bx)[2], (bx)[3], (bx)[4], (bx)[5], (long long)(D), (long long)(H), (long long)(W))
// ids[j] of the HOST bytes ids is not the background and none of ids[0 .. j): in a loop over j, ids are non-zero and pairwise distinct
#define LABEL_REQUIRE_DISTINCT_ID(entry, name, ids, j)                                                                                      \
  do {                                                                                                                                      \
    MSAM2_REQUIRE((ids)[j] != 0, entry ": " name "[%d] is 0, the background", j);                                                           \
    for (int k_ = 0; k_ < (j); ++k_)                                                                                                        \
      MSAM2_REQUIRE((ids)[k_] != (ids)[j], entry ": " name "[%d] and " name "[%d] are both %d", k_, j, (int)(ids)[j]);                      \
  } while (0)
#define LABEL_REQUIRE_SPACING(entry, sz, sy, sx)                                                                                            \
  MSAM2_REQUIRE(label_spacing_ok(sz) && label_spacing_ok(sy) && label_spacing_ok(sx),                                                       \
                entry ": spacing (%g, %g, %g): every value must be positive with a square in 2.3e-308 .. 2.6e297", sz, sy, sx)
#define LABEL_REQUIRE_OUT(entry, labels, out, N) \
  MSAM2_REQUIRE((out) == (labels) || (out) + (N) <= (labels) || (labels) + (N) <= (out), entry ": out overlaps labels without being labels")

// ---- runs and the neighbour rows of a connectivity (components.hip, holes.hip) -------------------------------------------------------------
struct LabelRows {                                          // the backward neighbour rows of a connectivity
  int count;
  int dd[4], dr[4], wide[4];                                // slice and row offset; wide: the overlap reaches one column further
};
static inline bool label_connectivity_ok(int c) { return c == 4 || c == 8 || c == 6 || c == 18 || c == 26; }
static inline bool label_connectivity_in_plane(int c) { return c == 4 || c == 8; }
// (slice offset, row offset, widened by a column): in plane first
static inline LabelRows label_rows(int connectivity) {
  LabelRows rows = {};
  const bool diag2 = connectivity == 8 || connectivity == 18 || connectivity == 26;     // offsets that differ in two coordinates
  auto add = [&](int dd, int dr, bool wide) {
    rows.dd[rows.count] = dd, rows.dr[rows.count] = dr, rows.wide[rows.count] = wide ? 1 : 0;
    ++rows.count;
  };
  add(0, -1, diag2);
  if (!label_connectivity_in_plane(connectivity)) {
    add(-1, 0, diag2);
    if (diag2) {
      add(-1, -1, connectivity == 26);
      add(-1, 1, connectivity == 26);
    }
  }
  return rows;
}

// Lane of the first voxel of this lane's run among the wave's 64 voxels.  b: the voxel's class, 0 = belongs to no run (such voxels are
// runs of their own); a run starts where the class differs from the left lane's, at column 0 (of the volume, or of the box) and at
// lane 0.  differs(class of the left lane): `b != left` for label bytes, `left == 0` for a binary class -- the same for 0 / 1, but `!=`
// moves instructions in holes.hip.  *heads: the lanes that start a run.  All 64 lanes call it.
template <typename F>
__device__ __forceinline__ int label_run_first(int b, int col, int lane, unsigned long long* heads, F&& differs) {
  const int left = __shfl_up(b, 1);
  const bool head = lane == 0 || b == 0 || col == 0 || differs(left);
  *heads = __ballot(head);                                  // bit 0 is always set
  return 63 - __clzll((long long)(*heads & (~0ull >> (63 - lane))));
}

}  // namespace
