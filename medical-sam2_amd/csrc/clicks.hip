// Closing the interactive loop: one corrective click per (slice, object) from the error regions of a predicted uint8 label volume [D, H, W]
// against the ground truth (msam2_label_error_clicks), gfx950.
//
// Definitions.  Per slice and object j with value v = ids[j]: FN_j = {gt == v and pred != v}, FP_j = {pred == v and gt != v}.
// For q in a region R, d2(q) = min |q - z|^2 over the pixels z of the slice that are not in R, the one-pixel frame around the image (rows -1 and
// H, columns -1 and W) included: SAM 2's sample_one_point_from_error_center (zero padding, L2 distance transform), squared.  Integers >= 1.
//   mode 0 (centre): per region the voxel of largest d2, ties to the smallest raster index y W + x; the click is positive at FN's voxel iff
//     max d2(FN_j) > max d2(FP_j) (an empty region counts 0), else negative at FP's voxel; both empty: label -1 at (-1, -1).
//   mode 1 (uniform): the k-th voxel of FN_j | FP_j in raster order, k from the caller or (u * count) >> 32; label 1 iff it is in FN.
// clicks int32 [D, n, 8] = (x, y, label, |FN|, |FP|, max d2(FN), max d2(FP), 0); the two d2 fields are -1 in mode 1.
//
// A voxel with pred != gt is in at most one region of each kind: FN of gt's value, FP of pred's.  So each kind is ONE class map per slice --
// kind 0: class = gt where gt != pred, else 0; kind 1 with the volumes exchanged -- and d2 is the distance to the nearest voxel of another
// class.  The cost does not depend on n:
//   * rows (centre): one wave per row and kind, 64 columns at a time.  A ballot of the run heads (class != left neighbour's) and one
//     count-leading-zeros give every lane the distance to the first voxel of another class on its left, the head of the run that reaches into
//     the chunk is carried (wave-uniform); a second sweep from the right end (a head is where the left distance is 1) takes the smaller one.
//     The row ends count as columns -1 and W.  uint16 per voxel and kind, 1 .. 8192.
//   * columns (centre): one lane per voxel, lanes along x.  Candidate rows in order of increasing |dy|; a row outside the image or a voxel of
//     another class gives dy^2, a voxel of the same region dy^2 + (its row distance)^2; the scan stops once dy^2 is not below the best so
//     far.  int32: at most 8192^2 + 8192^2.  Then, per region present in the wave, a wave reduction and ONE 64-bit atomicMax of
//     (d2 << 32) | (0xFFFFFFFF - raster index), and one integer add of the wave's voxel count.  A maximum and a sum of integers do not depend
//     on scheduling; key 0 = empty region.
//   * counts (uniform): one wave per row, per-wave LDS counters; rows int32 [D, n, H] = |FN_j| + |FP_j| per row, every element written.
//   * table: one wave per (slice, object); in mode 1 a prefix scan over the row counts finds the row of voxel k, a ballot scan of that row of
//     the two volumes the column (msam2_label_pick's two steps).
// clicks and the keys are cleared by fill_kernel (common.h) on the caller's stream.  No thread waits for another beyond workgroup barriers: no spin, no grid
// barrier, no cooperative launch.
#include "common.h"

namespace {

constexpr int CLK_THREADS = 256;
constexpr int CLK_WAVES = CLK_THREADS / 64;
constexpr int CLK_FIELDS = 8;
enum { CLK_CENTER = 0, CLK_UNIFORM = 1 };

// workspace: mode 0: keys uint64 [D, n, 2], then the row distances uint16 [2, D, H, W]; mode 1: rows int32 [D, n, H]
size_t clk_key_bytes(int64_t D, int64_t n) { return (size_t)(D * n * 2) * sizeof(unsigned long long); }

// blockIdx.x: CLK_WAVES rows of the volume (row = d * H + y), blockIdx.y: kind.  Kind 0 (FN): a = gt, b = pred; kind 1 (FP): exchanged.
__global__ __launch_bounds__(CLK_THREADS) void clk_row_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t rows, int W,
                                                              uint16_t* __restrict__ g) {
  const int kind = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * CLK_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;                                  // wave-uniform
  const uint8_t* __restrict__ a = (kind ? pred : gt) + row * W;
  const uint8_t* __restrict__ b = (kind ? gt : pred) + row * W;
  uint16_t* out = g + ((int64_t)kind * rows + row) * W;
  const int chunks = (W + 63) >> 6;
  int start = 0;                                            // wave-uniform: the head of the run that reaches into the chunk
  int prev = -1;                                            // the class left of the chunk (-1: column -1 of the frame, no voxel's class)
#pragma unroll 1
  for (int c = 0; c < chunks; ++c) {
    const int xb = c * 64 + lane;
    const bool live = xb < W;
    int cls = -2;
    if (live) {
      const int v = a[xb];
      cls = v != b[xb] ? v : 0;
    }
    int left = __shfl_up(cls, 1);
    if (lane == 0) left = prev;
    const unsigned long long m = __ballot(live && cls != left);
    const unsigned long long below = m & (~0ull >> (63 - lane));
    const int dl = below ? lane - (63 - __clzll((long long)below)) + 1 : xb - start + 1;
    if (live) out[xb] = (uint16_t)dl;
    if (m) start = c * 64 + 63 - __clzll((long long)m);
    prev = __shfl(cls, 63);
  }
  int next = W;                                             // the first head right of the chunk (column W of the frame)
#pragma unroll 1
  for (int c = chunks - 1; c >= 0; --c) {
    const int xb = c * 64 + lane;
    const bool live = xb < W;
    const int dl = live ? (int)out[xb] : 0;                 // this lane's own store of the first sweep
    const unsigned long long m = __ballot(live && dl == 1);
    const unsigned long long above = lane == 63 ? 0ull : m >> (lane + 1);
    const int dr = above ? __ffsll((long long)above) : next - xb;
    if (live && dr < dl) out[xb] = (uint16_t)dr;
    if (m) next = c * 64 + __ffsll((long long)m) - 1;
  }
}

// d2 of voxel (y, x) of one slice, which is in the region {a == v and b != v}; g: that kind's row distances of the slice
__device__ __forceinline__ int clk_scan(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const uint16_t* __restrict__ g, int H, int W,
                                        int y, int x, int v) {
  const int g0 = g[y * W + x];
  int best = g0 * g0;
#pragma unroll 1
  for (int k = 1;; ++k) {
    const int k2 = k * k;
    if (k2 >= best) break;                                  // (ends at the frame at the latest: k <= max(y + 1, H - y))
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int yy = side ? y + k : y - k;
      if (yy < 0 || yy >= H) {
        best = k2;
        break;
      }
      const int i = yy * W + x;                             // H * W <= 2^26
      if (!(a[i] == v && b[i] != v)) {
        best = k2;
        break;
      }
      const int gx = g[i];
      best = min(best, k2 + gx * gx);
    }
  }
  return best;
}

// Every lane of the wave comes here.  slot < 0: nothing; else key joins the maximum of keys[slot] and the lane is counted into
// clicks[(slot >> 1) * 8 + 3 + (slot & 1)]: per slot present in the wave one reduction, one atomicMax and one add by one lane.
__device__ __forceinline__ void clk_wave_max(int slot, unsigned long long key, int lane, unsigned long long* __restrict__ keys,
                                             int* __restrict__ clicks) {
  unsigned long long pending = __ballot(slot >= 0);
  while (pending) {                                         // wave-uniform
    const int leader = __ffsll((long long)pending) - 1;
    const int s = __shfl(slot, leader);
    const bool mine = slot == s;
    const unsigned long long voters = __ballot(mine);
    unsigned long long v = mine ? key : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long w = __shfl_xor(v, o);
      v = w > v ? w : v;
    }
    if (lane == leader) {
      atomicMax(keys + s, v);
      atomicAdd(clicks + (int64_t)(s >> 1) * CLK_FIELDS + 3 + (s & 1), (int)__popcll(voters));
    }
    pending &= ~voters;
  }
}

__global__ __launch_bounds__(CLK_THREADS) void clk_col_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                              const uint8_t* __restrict__ ids, int n, int H, int W, int64_t vox,
                                                              const uint16_t* __restrict__ g, unsigned long long* __restrict__ keys,
                                                              int* __restrict__ clicks) {
  __shared__ signed char lut[256];
  ids_to_object_table(lut, ids, n, threadIdx.x);
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * CLK_THREADS + threadIdx.x;
  int slot[2] = {-1, -1};
  unsigned long long key[2] = {0ull, 0ull};
  if (i < vox) {
    const int p = pred[i], t = gt[i];
    if (p != t) {
      const int HW = H * W;
      const int d = (int)(i / HW), r = (int)(i - (int64_t)d * HW);
      const int y = r / W, x = r - y * W;
      const int64_t base = (int64_t)d * HW;
      const int jf = lut[t], jp = lut[p];
      if (jf >= 0) {
        const int d2 = clk_scan(gt + base, pred + base, g + base, H, W, y, x, t);
        slot[0] = (d * n + jf) * 2;
        key[0] = ((unsigned long long)d2 << 32) | (0xFFFFFFFFu - (unsigned)r);
      }
      if (jp >= 0) {
        const int d2 = clk_scan(pred + base, gt + base, g + vox + base, H, W, y, x, p);
        slot[1] = (d * n + jp) * 2 + 1;
        key[1] = ((unsigned long long)d2 << 32) | (0xFFFFFFFFu - (unsigned)r);
      }
    }
  }
  clk_wave_max(slot[0], key[0], lane, keys, clicks);
  clk_wave_max(slot[1], key[1], lane, keys, clicks);
}

// blockIdx.x: CLK_WAVES rows of the volume, one wave each
__global__ __launch_bounds__(CLK_THREADS) void clk_count_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                const uint8_t* __restrict__ ids, int n, int H, int W, int64_t nrows,
                                                                int* __restrict__ rows, int* __restrict__ clicks) {
  __shared__ signed char lut[256];
  __shared__ int cnt[CLK_WAVES][2][LABEL_MAX_OBJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  (&cnt[0][0][0])[tid] = 0;                                 // CLK_WAVES * 2 * LABEL_MAX_OBJ == CLK_THREADS
  ids_to_object_table(lut, ids, n, tid);
  const int64_t row = (int64_t)blockIdx.x * CLK_WAVES + wave;
  if (row < nrows) {
    const uint8_t* __restrict__ pr = pred + row * W;
    const uint8_t* __restrict__ gr = gt + row * W;
    for (int x = lane; x < W; x += 64) {
      const int p = pr[x], t = gr[x];
      if (p != t) {
        const int jf = lut[t], jp = lut[p];
        if (jf >= 0) atomicAdd(&cnt[wave][0][jf], 1);
        if (jp >= 0) atomicAdd(&cnt[wave][1][jp], 1);
      }
    }
  }
  __syncthreads();
  if (row < nrows && lane < n) {
    const int d = (int)(row / H), y = (int)(row - (int64_t)d * H);
    const int cf = cnt[wave][0][lane], cp = cnt[wave][1][lane];
    const int64_t pair = (int64_t)d * n + lane;
    rows[pair * H + y] = cf + cp;
    if (cf) atomicAdd(clicks + pair * CLK_FIELDS + 3, cf);
    if (cp) atomicAdd(clicks + pair * CLK_FIELDS + 4, cp);
  }
}
static_assert(CLK_WAVES * 2 * LABEL_MAX_OBJ == CLK_THREADS, "clk_count_kernel clears one counter per thread");

// one wave; blockIdx.x = object, blockIdx.y = slice
__global__ __launch_bounds__(64) void clk_table_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                       const uint8_t* __restrict__ ids, const unsigned long long* __restrict__ keys,
                                                       const int* __restrict__ rows, const int* __restrict__ k, const unsigned* __restrict__ u,
                                                       int H, int W, int n, int mode, int* __restrict__ clicks) {
  const int lane = threadIdx.x, j = blockIdx.x, d = blockIdx.y;
  const int64_t pair = (int64_t)d * n + j;
  int* c = clicks + pair * CLK_FIELDS;
  int x = -1, y = -1, label = -1, mf = -1, mp = -1;
  if (mode == CLK_CENTER) {
    const unsigned long long kf = keys[pair * 2], kp = keys[pair * 2 + 1];
    mf = (int)(kf >> 32), mp = (int)(kp >> 32);
    if (kf | kp) {
      label = mf > mp ? 1 : 0;
      const unsigned r = 0xFFFFFFFFu - (unsigned)(label ? kf : kp);
      y = (int)(r / (unsigned)W), x = (int)(r - (unsigned)y * (unsigned)W);
    }
  } else {
    const int count = c[3] + c[4];                          // H * W <= 2^26 voxels, each in at most one of the two
    if (count > 0) {                                        // everything below branches on values the whole wave shares
      long long kk = u ? (long long)(((unsigned long long)u[pair] * (unsigned long long)count) >> 32) : (long long)k[pair];
      if (kk < 0 || kk >= count) kk = count - 1;
      const int* rc = rows + pair * H;
      int row = -1, kr = 0;
      long long base = 0;
      for (int yb = 0; yb < H && row < 0; yb += 64) {
        const int yy = yb + lane;
        const int cc = yy < H ? max(rc[yy], 0) : 0;
        int s = cc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(s, o);
          if (lane >= o) s += t;
        }
        const unsigned long long m = __ballot(cc > 0 && base + s - cc <= kk && kk < base + s);
        if (m) {
          const int src = __ffsll((long long)m) - 1;
          row = yb + src;
          kr = (int)(kk - (base + __shfl(s, src) - __shfl(cc, src)));
        }
        base += __shfl(s, 63);
      }
      if (row >= 0) {
        const int id = ids[j];
        const uint8_t* __restrict__ pr = pred + ((int64_t)d * H + row) * W;
        const uint8_t* __restrict__ gr = gt + ((int64_t)d * H + row) * W;
        int seen = 0;                                       // voxels of the union left of this chunk
        for (int xb = 0; xb < W; xb += 64) {
          const int xx = xb + lane;
          bool fn = false, fp = false;
          if (xx < W) {
            const int p = pr[xx], t = gr[xx];
            fn = t == id && p != id;
            fp = p == id && t != id;
          }
          const unsigned long long m = __ballot(fn || fp);
          const unsigned long long hit = __ballot((fn || fp) && seen + lanes_below(m, lane) == kr);
          if (hit) {
            const int src = __ffsll((long long)hit) - 1;
            x = xb + src, y = row;
            label = __shfl((int)fn, src);
            break;
          }
          seen += (int)__popcll(m);
        }
      }
    }
  }
  if (lane == 0) {
    c[0] = x, c[1] = y, c[2] = label;
    c[5] = mf, c[6] = mp, c[7] = 0;
  }
}

}  // namespace

extern "C" size_t msam2_label_error_clicks_workspace_bytes(int64_t D, int64_t H, int64_t W, int64_t n, int mode) {
  if (!label_sizes_ok(D, H, W, 1, LABEL_MAX_VOXELS) || n < 1 || n > LABEL_MAX_OBJ) return 0;
  if (mode == CLK_CENTER) return clk_key_bytes(D, n) + (size_t)(D * H * W) * 2 * sizeof(uint16_t);
  if (mode == CLK_UNIFORM) return (size_t)(D * n * H) * sizeof(int);
  return 0;
}

extern "C" int msam2_label_error_clicks(const uint8_t* pred, const uint8_t* gt, const uint8_t* ids, const int* k, const uint32_t* u, int64_t D,
                                        int64_t H, int64_t W, int64_t n, int mode, int* clicks, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  MSAM2_REQUIRE(pred && gt && ids && clicks && workspace, "label_error_clicks: null pred / gt / ids / clicks / workspace");
  MSAM2_REQUIRE(mode == CLK_CENTER || mode == CLK_UNIFORM, "label_error_clicks: mode %d (0: centre of the largest error, 1: uniform over the error)",
                mode);
  MSAM2_REQUIRE(mode == CLK_CENTER ? !k && !u : (k != nullptr) != (u != nullptr),
                "label_error_clicks: mode 1 needs exactly one of k (indices) and u (uniform words), mode 0 neither");
  LABEL_REQUIRE_OBJECTS("label_error_clicks", n);
  LABEL_REQUIRE_SIZES("label_error_clicks", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  const size_t need = msam2_label_error_clicks_workspace_bytes(D, H, W, n, mode);
  MSAM2_REQUIRE(workspace_bytes >= need, "label_error_clicks: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
  MSAM2_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)clicks & 3) == 0,
                "label_error_clicks: the workspace must be 8-byte aligned, clicks 4-byte");
  hipStream_t s = (hipStream_t)stream;
  fill_on(s, clicks, D * n * CLK_FIELDS, 0);
  const int64_t rows = D * H, vox = D * H * W;
  unsigned long long* keys = mode == CLK_CENTER ? (unsigned long long*)workspace : nullptr;
  int* row_counts = mode == CLK_UNIFORM ? (int*)workspace : nullptr;
  if (mode == CLK_CENTER) {
    uint16_t* g = (uint16_t*)((char*)workspace + clk_key_bytes(D, n));
    fill_on(s, (int*)keys, D * n * 2 * 2, 0);                // 64-bit words, 8-byte aligned: two ints each
    hipLaunchKernelGGL(clk_row_kernel, dim3(cdiv(rows, CLK_WAVES), 2), dim3(CLK_THREADS), 0, s, pred, gt, rows, (int)W, g);
    hipLaunchKernelGGL(clk_col_kernel, dim3(cdiv(vox, CLK_THREADS)), dim3(CLK_THREADS), 0, s, pred, gt, ids, (int)n, (int)H, (int)W, vox, g, keys,
                       clicks);
  } else {
    hipLaunchKernelGGL(clk_count_kernel, dim3(cdiv(rows, CLK_WAVES)), dim3(CLK_THREADS), 0, s, pred, gt, ids, (int)n, (int)H, (int)W, rows,
                       row_counts, clicks);
  }
  hipLaunchKernelGGL(clk_table_kernel, dim3((unsigned)n, (unsigned)D), dim3(64), 0, s, pred, gt, ids, keys, row_counts, k,
                     reinterpret_cast<const unsigned*>(u), (int)H, (int)W, (int)n, mode, clicks);
  return msam2_check_launch("label_error_clicks");
}
