// Start of the 3-D path: box and click prompts from a uint8 label volume [D, H, W] (volume_labels.labels_from_pack), gfx950.
//
// The reference's dataset builds its prompts per (slice, object) pair on the host (func_3d/dataset/btcv.py:88-104 calling
// func_3d/utils.py:89-137): every pair runs np.argwhere over a full-resolution mask.  Here one pass over the label volume gives, per
// (slice, object), the voxel count and the inclusive row / column extent (the box), plus the count of every row; a second, tiny kernel
// turns an index k into the k-th voxel of the object in raster order (np.argwhere's order: the click).  Everything is an integer, and the
// partials of the workgroups meet in global memory through integer add / min / max only, so the tables do not depend on scheduling.
//
// msam2_label_stats: a workgroup owns a band of whole rows of one slice (a contiguous byte range: up to STAT_ROWS rows, about 16 KiB).
//   * bytes in front of the first 16-byte boundary and behind the last one go through a scalar path (one thread each); in between every
//     lane loads 16 voxels at once.  W is arbitrary, so a lane's 16 voxels may straddle rows.
//   * per lane: labels are spatially coherent, so the 16 voxels are usually one run of one value inside one row ("plain" lane: two
//     compares).  Any other lane walks its voxels, maps each through the 256-entry label -> object table in LDS and adds whole runs.
//   * per wave: neighbouring plain lanes of the same row and value form one segment; a ballot of the segment heads gives every head its
//     segment's length, and only the head touches LDS (one add to the row count, one min and one max on the column extent).  A wave of
//     background costs one ballot and no LDS access.
//   * the band's row counts leave with plain stores (each row of the table has exactly one owner), and (count, r0, r1, c0, c1) of the
//     objects the band contains with one atomic each.  stats is pre-set to -1 by fill_kernel on the caller's stream: r0 / c0 are minimised
//     as UNSIGNED numbers (0xffffffff is the neutral element and reads back as -1 when the object is absent), r1 / c1 maximised as signed
//     ones, and the first band of every slice adds 1 to every count, so an absent object ends at (0, -1, -1, -1, -1).
// msam2_label_pick: one workgroup per (slice, object): a prefix scan over the object's row counts (rows r0 .. r1, 256 at a time) finds
//   the row that holds voxel k, a ballot scan over that row of the volume (columns c0 .. c1) finds the column.
#include <limits.h>

#include "common.h"

namespace {

constexpr int STAT_THREADS = 256;
constexpr int STAT_ROWS = 64;            // most rows of a band (LDS: LABEL_MAX_OBJ x STAT_ROWS row counts)
constexpr int STAT_BAND_BYTES = 16384;   // a band is the fewest whole rows that reach this, at most STAT_ROWS

struct BandTables {                      // LDS of one workgroup
  int rowcnt[LABEL_MAX_OBJ * STAT_ROWS]; // [object][row of the band]
  int c0[LABEL_MAX_OBJ], c1[LABEL_MAX_OBJ], r0[LABEL_MAX_OBJ], r1[LABEL_MAX_OBJ], cnt[LABEL_MAX_OBJ];
  signed char lut[256];                  // label value -> object index, -1 = ignored
};

__device__ __forceinline__ void add_run(BandTables& t, int j, int row, int col, int len) {
  if (j < 0 || len <= 0) return;
  atomicAdd(&t.rowcnt[j * STAT_ROWS + row], len);
  atomicMin(&t.c0[j], col);
  atomicMax(&t.c1[j], col + len - 1);
}

// The voxels [o, o + len) of the band (len <= 16), value of voxel e = byte(e): runs of one object inside one row are added whole.
template <typename Byte>
__device__ __forceinline__ void walk_voxels(BandTables& t, int W, int o, int len, Byte byte) {
  int row = o / W, col = o - row * W;
  int cj = -1, crow = 0, ccol = 0, clen = 0;
  for (int e = 0; e < len; ++e) {
    const int j = t.lut[byte(e)];
    if (j == cj && col != 0) {
      ++clen;
    } else {
      add_run(t, cj, crow, ccol, clen);
      cj = j, crow = row, ccol = col, clen = 1;
    }
    if (++col == W) col = 0, ++row;
  }
  add_run(t, cj, crow, ccol, clen);
}

// blockIdx.x = band of `band_rows` rows, blockIdx.y = slice
__global__ __launch_bounds__(STAT_THREADS) void label_stats_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ ids, int n,
                                                                   int H, int W, int band_rows, int* __restrict__ stats,
                                                                   int* __restrict__ rows) {
  __shared__ BandTables t;
  const int tid = threadIdx.x, lane = tid & 63, d = blockIdx.y;
  const int y0 = blockIdx.x * band_rows, nrows = min(band_rows, H - y0);
  for (int i = tid; i < LABEL_MAX_OBJ * STAT_ROWS; i += STAT_THREADS) t.rowcnt[i] = 0;
  if (tid < LABEL_MAX_OBJ) {
    t.c0[tid] = t.r0[tid] = INT_MAX;
    t.c1[tid] = t.r1[tid] = -1;
    t.cnt[tid] = 0;
  }
  t.lut[tid] = -1;                                          // STAT_THREADS == 256.  (ids_to_object_table spelled out: with the call
  __syncthreads();                                          //  this kernel's listing comes out three lines shorter)
  if (tid < n) t.lut[ids[tid]] = (signed char)tid;
  __syncthreads();

  const uint8_t* p = labels + ((int64_t)d * H + y0) * W;    // the band: `bytes` consecutive voxels
  const int bytes = nrows * W;                              // <= STAT_BAND_BYTES + W
  const int head = min(bytes, (int)((16 - ((uintptr_t)p & 15)) & 15));
  const int nvec = (bytes - head) >> 4, tail = bytes - head - (nvec << 4);
  if (tid == 0 && head > 0) walk_voxels(t, W, 0, head, [&](int e) { return p[e]; });
  if (tid == 64 && tail > 0) {
    const int o = head + (nvec << 4);
    walk_voxels(t, W, o, tail, [&](int e) { return p[o + e]; });
  }
  const uint4* pv = reinterpret_cast<const uint4*>(p + head);
  for (int base = 0; base < nvec; base += STAT_THREADS) {   // wave-uniform bound: the shuffle and the ballot below see whole waves
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
    if (plain) {
      if ((heads >> lane) & 1) {
        add_run(t, t.lut[first], row, col, run_length(heads, lane) << 4);
      }
    } else if (live) {
      const unsigned long long lo = v.x | ((unsigned long long)v.y << 32), hi = v.z | ((unsigned long long)v.w << 32);
      walk_voxels(t, W, o, 16, [&](int e) { return (unsigned)(((e < 8 ? lo : hi) >> ((e & 7) << 3)) & 0xffu); });
    }
  }
  __syncthreads();

  // the band's rows of the table (zeros included: nothing pre-sets it), and the band's row extent and count per object
  for (int i = tid; i < n * STAT_ROWS; i += STAT_THREADS) {
    const int j = i / STAT_ROWS, r = i - j * STAT_ROWS;
    if (r >= nrows) continue;
    const int c = t.rowcnt[i];
    rows[((int64_t)d * n + j) * H + y0 + r] = c;
    if (c > 0) {
      atomicAdd(&t.cnt[j], c);
      atomicMin(&t.r0[j], y0 + r);
      atomicMax(&t.r1[j], y0 + r);
    }
  }
  __syncthreads();
  if (tid < n) {
    int* st = stats + ((int64_t)d * n + tid) * 5;
    const int c = t.cnt[tid] + (blockIdx.x == 0 ? 1 : 0);  // the pre-set left -1 in the count
    if (c) atomicAdd(st, c);
    if (t.cnt[tid] > 0) {
      atomicMin(reinterpret_cast<unsigned*>(st + 1), (unsigned)t.r0[tid]);
      atomicMax(st + 2, t.r1[tid]);
      atomicMin(reinterpret_cast<unsigned*>(st + 3), (unsigned)t.c0[tid]);
      atomicMax(st + 4, t.c1[tid]);
    }
  }
}

// Inclusive prefix sum of v over the workgroup (256 threads, 4 waves); *total = the workgroup's sum.  wsum: 4 ints of LDS, free again
// after the call's second barrier.
__device__ __forceinline__ int block_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(s, d);
    if (lane >= d) s += o;
  }
  if (lane == 63) wsum[wave] = s;
  __syncthreads();
  int before = 0, all = 0;                                  // (spelled out here and in label_pick_kernel's column scan: with one shared
#pragma unroll                                              //  function for both, label_pick_kernel's listing comes out three lines shorter)
  for (int w = 0; w < 4; ++w) {
    const int x = wsum[w];
    before += w < wave ? x : 0;
    all += x;
  }
  __syncthreads();
  *total = all;
  return s + before;
}

// blockIdx.x = object, blockIdx.y = slice
__global__ __launch_bounds__(STAT_THREADS) void label_pick_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ ids,
                                                                  const int* __restrict__ stats, const int* __restrict__ rows,
                                                                  const int* __restrict__ k, const unsigned* __restrict__ u, int H, int W,
                                                                  int n, int* __restrict__ xy) {
  __shared__ int wsum[4], found[2], res[2];
  const int tid = threadIdx.x, j = blockIdx.x, d = blockIdx.y;
  const int64_t pair = (int64_t)d * n + j;
  const int* st = stats + pair * 5;
  const int count = st[0];
  if (tid == 0) {
    found[0] = res[0] = res[1] = -1;
    found[1] = 0;
  }
  __syncthreads();
  if (count > 0) {                                          // everything below branches on values the whole workgroup shares
    long long kk = u ? (long long)(((unsigned long long)u[pair] * (unsigned long long)count) >> 32) : (long long)k[pair];
    if (kk < 0 || kk >= count) kk = count - 1;
    // the extents bound the two scans; clamped, so that tables this call was not given by msam2_label_stats cannot lead outside the volume
    const int r0 = min(max(st[1], 0), H - 1), r1 = min(max(st[2], r0), H - 1);
    const int c0 = min(max(st[3], 0), W - 1), c1 = min(max(st[4], c0), W - 1);
    const int* rc = rows + pair * H;
    long long base = 0;
    for (int yb = r0; yb <= r1; yb += STAT_THREADS) {
      const int y = yb + tid;
      const int c = y <= r1 ? max(rc[y], 0) : 0;
      int total;
      const long long incl = base + block_scan(c, wsum, &total);
      if (c > 0 && incl - c <= kk && kk < incl) {
        found[0] = y;
        found[1] = (int)(kk - (incl - c));
      }
      base += total;
      __syncthreads();
      if (found[0] >= 0) break;
    }
    const int row = found[0], kr = found[1];
    if (row >= 0) {
      const uint8_t id = ids[j];
      const uint8_t* rp = labels + ((int64_t)d * H + row) * W;
      const int lane = tid & 63, wave = tid >> 6;
      int seen = 0;                                         // voxels of the object left of this chunk
      for (int xb = c0; xb <= c1; xb += STAT_THREADS) {
        const int x = xb + tid;
        const bool hit = x <= c1 && rp[x] == id;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;                            // (block_scan's four-wave sums: see there)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int s = wsum[w];
          before += w < wave ? s : 0;
          all += s;
        }
        const int rank = seen + before + lanes_below(m, lane);
        if (hit && rank == kr) {
          res[0] = x;
          res[1] = row;
        }
        seen += all;
        __syncthreads();
        if (seen > kr) break;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    xy[pair * 2] = res[0];
    xy[pair * 2 + 1] = res[1];
  }
}

}  // namespace

extern "C" int msam2_label_stats(const uint8_t* labels, const uint8_t* ids, int64_t D, int64_t H, int64_t W, int64_t n, int* stats, int* rows,
                                 void* stream) {
  MSAM2_REQUIRE(labels && ids && stats && rows, "label_stats: null labels / ids / stats / rows");
  LABEL_REQUIRE_OBJECTS("label_stats", n);
  LABEL_REQUIRE_SIZES("label_stats", D, H, W, 1, LABEL_NO_VOXEL_CAP, "");
  hipStream_t s = (hipStream_t)stream;
  fill_on(s, stats, D * n * 5, -1);                         // (common.h: why a kernel)
  int64_t band = cdiv(STAT_BAND_BYTES, W);
  band = band < STAT_ROWS ? band : STAT_ROWS;
  band = band < H ? band : H;
  hipLaunchKernelGGL(label_stats_kernel, dim3(cdiv(H, band), (unsigned)D), dim3(STAT_THREADS), 0, s, labels, ids, (int)n,
                     (int)H, (int)W, (int)band, stats, rows);
  return msam2_check_launch("label_stats");
}

// k outside [0, count) on a present object is clamped to count - 1; an absent object (count 0) gives (-1, -1).
extern "C" int msam2_label_pick(const uint8_t* labels, const uint8_t* ids, const int* stats, const int* rows, const int* k, const uint32_t* u,
                                int64_t D, int64_t H, int64_t W, int64_t n, int* xy, void* stream) {
  MSAM2_REQUIRE(labels && ids && stats && rows && xy, "label_pick: null labels / ids / stats / rows / xy");
  MSAM2_REQUIRE((k != nullptr) != (u != nullptr), "label_pick: exactly one of k (indices) and u (uniform words) is needed");
  LABEL_REQUIRE_OBJECTS("label_pick", n);
  LABEL_REQUIRE_SIZES("label_pick", D, H, W, 1, LABEL_NO_VOXEL_CAP, "");
  hipLaunchKernelGGL(label_pick_kernel, dim3((unsigned)n, (unsigned)D), dim3(STAT_THREADS), 0, (hipStream_t)stream, labels, ids, stats, rows, k,
                     reinterpret_cast<const unsigned*>(u), (int)H, (int)W, (int)n, xy);
  return msam2_check_launch("label_pick");
}
