// Mask post-processing of automatic mask generation ("segment everything", automatic_mask_generator.py + utils/amg.py) on
// low-resolution logits [M, lh, lw] fp32, gfx950.
//
// The reference up-samples every batch of low-res logits to the crop size (64 x 3 x 1024^2 fp32 = 805 MB per batch), then reads the
// high-res logits again for the stability score, the boxes and an RLE built with nonzero() and a per-mask host loop.  Here every kernel
// re-evaluates the bilinear up-sampling (align_corners = False) per pixel on the fly, with the per-pixel expression of bilinear_kernel /
// bilinear4_kernel (elementwise.hip), so each result equals bit for bit the same quantity computed from msam2_bilinear_upsample's output
// -- and no high-res logits exist.  Counters are integers (ballot / popcount per wave, LDS, one atomic per workgroup): exact and
// independent of order.
#include "common.h"

namespace {

// value of output pixel (Y, X) of the (H, W) bilinear resize of plane p [h, w]; sy = (float)h / H, sx = (float)w / W.
// The expression is the one of bilinear_kernel, term for term (the two must round identically).
__device__ __forceinline__ float bilerp_at(const float* __restrict__ p, int h, int w, float sy, float sx, int Y, int X) {
  float fy = fmaxf((Y + 0.5f) * sy - 0.5f, 0.f), fx = fmaxf((X + 0.5f) * sx - 0.5f, 0.f);
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  const float ly = fy - y0, lx = fx - x0;
  const float v = (1.f - ly) * ((1.f - lx) * p[y0 * w + x0] + lx * p[y0 * w + x1]) +
                  ly * ((1.f - lx) * p[y1 * w + x0] + lx * p[y1 * w + x1]);
  return v;
}

constexpr int STATS_THREADS = 256, STATS_PPT = 8;           // 2048 crop pixels per workgroup

// Per mask: count(v > thr_hi), count(v > thr_lo), count(v > thr) and the inclusive box of v > thr over the (h, w) crop frame.
// ws [M, 4]: box accumulators as maxima of (w - x_min, h - y_min, x_max + 1, y_max + 1), zeroed by the host entry.
__global__ __launch_bounds__(STATS_THREADS) void mask_stats_kernel(const float* __restrict__ logits, int lh, int lw, int h, int w,
                                                                   float thr, float thr_hi, float thr_lo, int* __restrict__ counts,
                                                                   int* __restrict__ ws) {
  const int m = blockIdx.y;
  const float* p = logits + (int64_t)m * lh * lw;
  const float sy = (float)lh / h, sx = (float)lw / w;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t total = (int64_t)h * w;
  const int64_t base = (int64_t)blockIdx.x * STATS_THREADS * STATS_PPT;
  int c_hi = 0, c_lo = 0, c_a = 0;                               // wave-uniform (popcounts of ballots)
  int xmin = w, ymin = h, xmax = -1, ymax = -1;                  // per lane
#pragma unroll
  for (int k = 0; k < STATS_PPT; ++k) {
    const int64_t i = base + k * STATS_THREADS + threadIdx.x;
    bool hi = false, lo = false, a = false;
    int X = 0, Y = 0;
    if (i < total) {
      Y = (int)(i / w);
      X = (int)(i - (int64_t)Y * w);
      const float v = bilerp_at(p, lh, lw, sy, sx, Y, X);
      hi = v > thr_hi;
      lo = v > thr_lo;
      a = v > thr;
    }
    c_hi += __popcll(__ballot(hi));
    c_lo += __popcll(__ballot(lo));
    c_a += __popcll(__ballot(a));
    if (a) {
      xmin = min(xmin, X);
      xmax = max(xmax, X);
      ymin = min(ymin, Y);
      ymax = max(ymax, Y);
    }
  }
  xmin = wave_min(xmin);
  ymin = wave_min(ymin);
  xmax = wave_max(xmax);
  ymax = wave_max(ymax);
  __shared__ int red[STATS_THREADS / 64][7];
  if (lane == 0) {
    red[wv][0] = c_hi;
    red[wv][1] = c_lo;
    red[wv][2] = c_a;
    red[wv][3] = xmin;
    red[wv][4] = ymin;
    red[wv][5] = xmax;
    red[wv][6] = ymax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s0 = 0, s1 = 0, s2 = 0, x0 = w, y0 = h, x1 = -1, y1 = -1;
    for (int k = 0; k < STATS_THREADS / 64; ++k) {
      s0 += red[k][0];
      s1 += red[k][1];
      s2 += red[k][2];
      x0 = min(x0, red[k][3]);
      y0 = min(y0, red[k][4]);
      x1 = max(x1, red[k][5]);
      y1 = max(y1, red[k][6]);
    }
    if (s0) atomicAdd(counts + 3 * m + 0, s0);
    if (s1) atomicAdd(counts + 3 * m + 1, s1);
    if (s2) {
      atomicAdd(counts + 3 * m + 2, s2);
      atomicMax(ws + 4 * m + 0, w - x0);
      atomicMax(ws + 4 * m + 1, h - y0);
      atomicMax(ws + 4 * m + 2, x1 + 1);
      atomicMax(ws + 4 * m + 3, y1 + 1);
    }
  }
}

// box [M, 4] = (x_min, y_min, x_max, y_max), [0, 0, 0, 0] for an empty mask (batched_mask_to_box, amg.py)
__global__ void mask_box_finalize_kernel(const int* __restrict__ counts, const int* __restrict__ ws, int* __restrict__ box, int M, int h,
                                         int w) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int4 b = make_int4(0, 0, 0, 0);
  if (counts[3 * m + 2] > 0) b = make_int4(w - ws[4 * m], h - ws[4 * m + 1], ws[4 * m + 2] - 1, ws[4 * m + 3] - 1);
  *reinterpret_cast<int4*>(box + 4 * m) = b;
}

// Pixel i of the original-image frame [H, W] in column-major order (i = x * H + y), the crop (x0, y0, w, h) pasted in, 0 outside it
// (uncrop_masks).
struct RleFrame {
  const float* p;
  int lh, lw, h, w, x0, y0, H;
  float sy, sx, thr;
  __device__ __forceinline__ bool bit(int64_t i) const {
    const int x = (int)(i / H), y = (int)(i - (int64_t)x * H);
    const int X = x - x0, Y = y - y0;
    if (X < 0 || X >= w || Y < 0 || Y >= h) return false;
    return bilerp_at(p, lh, lw, sy, sx, Y, X) > thr;
  }
};

__device__ __forceinline__ RleFrame rle_frame(const float* logits, int m, int lh, int lw, int h, int w, int x0, int y0, int H, float thr) {
  RleFrame f;
  f.p = logits + (int64_t)m * lh * lw;
  f.lh = lh;
  f.lw = lw;
  f.h = h;
  f.w = w;
  f.x0 = x0;
  f.y0 = y0;
  f.H = H;
  f.sy = (float)lh / h;
  f.sx = (float)lw / w;
  f.thr = thr;
  return f;
}

constexpr int RUNS_THREADS = 256, RUNS_PPT = 8;

// Pass 1: number of entries of each mask's RLE counts list = transitions + 1 (the last run) + 1 if the first pixel is set (the list then
// starts with a 0-length run).  runs [M] zeroed by the host entry.
__global__ __launch_bounds__(RUNS_THREADS) void rle_runs_kernel(const float* __restrict__ logits, int lh, int lw, int h, int w, int x0, int y0,
                                                                int H, int64_t total, float thr, int* __restrict__ runs) {
  const int m = blockIdx.y;
  const RleFrame f = rle_frame(logits, m, lh, lw, h, w, x0, y0, H, thr);
  const int64_t base = (int64_t)blockIdx.x * RUNS_THREADS * RUNS_PPT;
  int c = 0;
#pragma unroll
  for (int k = 0; k < RUNS_PPT; ++k) {
    const int64_t i = base + k * RUNS_THREADS + threadIdx.x;
    const bool t = i > 0 && i < total && f.bit(i) != f.bit(i - 1);
    c += __popcll(__ballot(t));
  }
  __shared__ int red[RUNS_THREADS / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < RUNS_THREADS / 64; ++k) s += red[k];
    if (blockIdx.x == 0) s += 1 + (f.bit(0) ? 1 : 0);
    if (s) atomicAdd(runs + m, s);
  }
}

constexpr int RLE_THREADS = 1024, RLE_WAVES = RLE_THREADS / 64;

// Pass 2: one workgroup per mask writes its run lengths in order at counts[offsets[m] ..].  Transition positions p (pixel p differs from
// pixel p - 1, plus the closing position `total`) are compacted in ballot order; each writes p minus the previous transition position.
__global__ __launch_bounds__(RLE_THREADS) void rle_write_kernel(const float* __restrict__ logits, int lh, int lw, int h, int w, int x0,
                                                                int y0, int H, int64_t total, float thr, const int64_t* __restrict__ offsets,
                                                                int* __restrict__ counts) {
  const int m = blockIdx.x;
  const RleFrame f = rle_frame(logits, m, lh, lw, h, w, x0, y0, H, thr);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t off = offsets[m], cap = offsets[m + 1] - offsets[m];
  __shared__ int w_cnt[RLE_WAVES];
  __shared__ int64_t w_last[RLE_WAVES];
  __shared__ int64_t s_last;
  __shared__ int64_t s_written;
  const bool lead = f.bit(0);
  if (threadIdx.x == 0) {
    s_last = 0;
    s_written = lead ? 1 : 0;
    if (lead && cap > 0) counts[off] = 0;
  }
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int64_t base = 0; base <= total; base += RLE_THREADS) {
    const int64_t i = base + threadIdx.x;
    const bool t = (i == total) || (i > 0 && i < total && f.bit(i) != f.bit(i - 1));
    const unsigned long long bm = __ballot(t);
    if (lane == 0) {
      w_cnt[wv] = __popcll(bm);
      w_last[wv] = bm ? base + wv * 64 + (63 - __clzll(bm)) : -1;
    }
    __syncthreads();
    const int64_t last_before = s_last, written = s_written;
    if (t) {
      int64_t k = written + __popcll(bm & lt);
      for (int q = 0; q < wv; ++q) k += w_cnt[q];
      int64_t prev = -1;
      const unsigned long long lower = bm & lt;
      if (lower) {
        prev = base + wv * 64 + (63 - __clzll(lower));
      } else {
        for (int q = wv - 1; q >= 0 && prev < 0; --q) prev = w_last[q];
        if (prev < 0) prev = last_before;
      }
      if (k < cap) counts[off + k] = (int)(i - prev);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t s = 0, l = -1;
      for (int q = 0; q < RLE_WAVES; ++q) {
        s += w_cnt[q];
        if (w_last[q] >= 0) l = w_last[q];
      }
      s_written = written + s;
      if (l >= 0) s_last = l;
    }
    __syncthreads();
  }
}

// ---- greedy box NMS with torchvision.ops.nms semantics -------------------------------------------------------------------------------
// Total order of the scores: descending, NaN first (torch.sort), ties to the lower input index (a stable sort).
__device__ __forceinline__ bool ranks_before(float sj, int j, float si, int i) {
  const bool nj = sj != sj, ni = si != si;
  if (nj || ni) return nj && (!ni || j < i);
  return sj > si || (sj == si && j < i);
}

__global__ void nms_rank_kernel(const float* __restrict__ scores, int K, int* __restrict__ order) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  const float si = scores[i];
  int r = 0;
  for (int j = 0; j < K; ++j) r += ranks_before(scores[j], j, si, i) ? 1 : 0;
  order[r] = i;
}

// IoU of two xyxy boxes as torchvision's CPU kernel computes it, operation by operation (no contraction into FMAs)
__device__ __forceinline__ float box_iou(const float4 a, const float4 b) {
#pragma clang fp contract(off)
  const float area_a = (a.z - a.x) * (a.w - a.y);
  const float area_b = (b.z - b.x) * (b.w - b.y);
  const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y), xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
  const float iw = fmaxf(0.f, xx2 - xx1), ih = fmaxf(0.f, yy2 - yy1);
  const float inter = iw * ih;
  return inter / (area_a + area_b - inter);
}

// mask[a][j] bit t: the box of rank a suppresses the box of rank b = 64 j + t (b > a, IoU > thr)
__global__ void nms_mask_kernel(const float* __restrict__ boxes, const int* __restrict__ order, int K, int nw, float thr,
                                unsigned long long* __restrict__ mask) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)K * nw) return;
  const int a = (int)(g / nw), j = (int)(g - (int64_t)a * nw);
  unsigned long long bits = 0;
  if (j >= a / 64) {
    const float4 ba = reinterpret_cast<const float4*>(boxes)[order[a]];
    for (int t = 0; t < 64; ++t) {
      const int b = j * 64 + t;
      if (b <= a || b >= K) continue;
      const float4 bb = reinterpret_cast<const float4*>(boxes)[order[b]];
      if (box_iou(ba, bb) > thr) bits |= 1ull << t;
    }
  }
  mask[g] = bits;
}

// One workgroup sweeps the bitmask 64 ranks at a time: wave 0 resolves a chunk against itself (lane l holds row 64 c + l's word c),
// then every thread ORs the kept rows into the removed words of the later chunks.  keep: input indices in rank order.
__global__ __launch_bounds__(256) void nms_sweep_kernel(const unsigned long long* __restrict__ mask, const int* __restrict__ order, int K, int nw,
                                                        int64_t* __restrict__ keep, int* __restrict__ n_keep) {
  extern __shared__ unsigned long long removed[];
  __shared__ unsigned long long kept_s;
  for (int j = threadIdx.x; j < nw; j += blockDim.x) removed[j] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int nk = 0;                                                        // wave 0 only
  for (int c = 0; c < nw; ++c) {
    if (threadIdx.x < 64) {
      const int a = c * 64 + lane;
      const unsigned long long row = a < K ? mask[(int64_t)a * nw + c] : 0ull;
      const int n = min(64, K - c * 64);
      unsigned long long cur = removed[c];
      for (int t = 0; t < n; ++t) {
        if (!((cur >> t) & 1ull)) {
          const unsigned lo = __shfl((unsigned)(row & 0xffffffffull), t, 64), hi = __shfl((unsigned)(row >> 32), t, 64);
          cur |= ((unsigned long long)hi << 32) | lo;
        }
      }
      const unsigned long long valid = n == 64 ? ~0ull : ((1ull << n) - 1ull);
      const unsigned long long kept = ~cur & valid;
      // (lanes_below spelled out: with the call this kernel's listing gains a line)
      if ((kept >> lane) & 1ull) keep[nk + __popcll(kept & ((1ull << lane) - 1ull))] = order[a];
      nk += __popcll(kept);
      if (lane == 0) kept_s = kept;
    }
    __syncthreads();
    const unsigned long long kept = kept_s;
    for (int j = c + 1 + threadIdx.x; j < nw; j += blockDim.x) {
      unsigned long long acc = removed[j];
      unsigned long long kb = kept;
      while (kb) {
        const int t = __ffsll((long long)kb) - 1;
        kb &= kb - 1ull;
        acc |= mask[(int64_t)(c * 64 + t) * nw + j];
      }
      removed[j] = acc;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) n_keep[0] = nk;
}

// K <= 65536: the IoU bitmask workspace is then 512 MiB and the sweep's removed bits take 8 KiB of LDS (the pipeline's largest call, the
// cross-crop NMS of crop_n_layers = 2 with nothing filtered, is 21 x 3072 = 64512 boxes)
constexpr int64_t NMS_MAX_K = 65536;
constexpr int NMS_MAX_WORDS = (int)(NMS_MAX_K / 64);

size_t nms_ws_order_bytes(int64_t K) { return (size_t)((K * 4 + 255) / 256 * 256); }

}  // namespace

extern "C" size_t msam2_mask_stats_workspace_bytes(int64_t M) { return M > 0 ? (size_t)M * 4 * sizeof(int) : 0; }

extern "C" int msam2_mask_stats(const float* logits, int64_t M, int64_t lh, int64_t lw, int64_t h, int64_t w, float thr, float thr_hi,
                                float thr_lo, int* counts, int* boxes, void* workspace, size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(M >= 0 && lh > 0 && lw > 0 && h > 0 && w > 0 && h * w < (1ll << 31) && lh * lw < (1ll << 31),
                "mask_stats: bad sizes (M %lld, low-res %lldx%lld, crop %lldx%lld)", (long long)M, (long long)lh, (long long)lw, (long long)h, (long long)w);
  MSAM2_REQUIRE(M <= 65535, "mask_stats: at most 65535 masks per call");
  if (M == 0) return MSAM2_OK;
  MSAM2_REQUIRE(logits && counts && boxes && workspace, "mask_stats: null tensor");
  MSAM2_REQUIRE(((uintptr_t)boxes & 15) == 0, "mask_stats: boxes must be 16-byte aligned");
  MSAM2_REQUIRE(workspace_bytes >= msam2_mask_stats_workspace_bytes(M), "mask_stats: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  fill_on(s, counts, M * 3, 0);
  fill_on(s, (int*)workspace, M * 4, 0);
  const int64_t per = STATS_THREADS * STATS_PPT;
  hipLaunchKernelGGL(mask_stats_kernel, dim3(cdiv(h * w, per), (unsigned)M), dim3(STATS_THREADS), 0, s, logits, (int)lh,
                     (int)lw, (int)h, (int)w, thr, thr_hi, thr_lo, counts, (int*)workspace);
  hipLaunchKernelGGL(mask_box_finalize_kernel, dim3(cdiv(M, 256)), dim3(256), 0, s, (const int*)counts, (const int*)workspace, boxes, (int)M,
                     (int)h, (int)w);
  return msam2_check_launch("mask_stats");
}

static int rle_check(const char* what, int64_t M, int64_t lh, int64_t lw, int64_t h, int64_t w, int64_t x0, int64_t y0, int64_t H,
                     int64_t W) {
  MSAM2_REQUIRE(M >= 0 && M <= 65535 && lh > 0 && lw > 0 && h > 0 && w > 0 && lh * lw < (1ll << 31),
                "%s: bad sizes (M %lld, low-res %lldx%lld, crop %lldx%lld)", what, (long long)M, (long long)lh, (long long)lw, (long long)h, (long long)w);
  MSAM2_REQUIRE(x0 >= 0 && y0 >= 0 && x0 + w <= W && y0 + h <= H && H * W < (1ll << 31),
                "%s: crop (%lld, %lld, %lld x %lld) outside the %lld x %lld image", what, (long long)x0, (long long)y0, (long long)w, (long long)h,
                (long long)W, (long long)H);
  return MSAM2_OK;
}

extern "C" int msam2_mask_rle_runs(const float* logits, int64_t M, int64_t lh, int64_t lw, int64_t h, int64_t w, int64_t x0, int64_t y0,
                                   int64_t H, int64_t W, float thr, int* runs, void* stream) {
  const int rc = rle_check("mask_rle_runs", M, lh, lw, h, w, x0, y0, H, W);
  if (rc) return rc;
  if (M == 0) return MSAM2_OK;
  MSAM2_REQUIRE(logits && runs, "mask_rle_runs: null tensor");
  hipStream_t s = (hipStream_t)stream;
  fill_on(s, runs, M, 0);
  const int64_t total = H * W, per = RUNS_THREADS * RUNS_PPT;
  hipLaunchKernelGGL(rle_runs_kernel, dim3(cdiv(total, per), (unsigned)M), dim3(RUNS_THREADS), 0, s, logits, (int)lh, (int)lw,
                     (int)h, (int)w, (int)x0, (int)y0, (int)H, total, thr, runs);
  return msam2_check_launch("mask_rle_runs");
}

extern "C" int msam2_mask_rle(const float* logits, int64_t M, int64_t lh, int64_t lw, int64_t h, int64_t w, int64_t x0, int64_t y0, int64_t H,
                              int64_t W, float thr, const int64_t* offsets, int* counts, void* stream) {
  const int rc = rle_check("mask_rle", M, lh, lw, h, w, x0, y0, H, W);
  if (rc) return rc;
  if (M == 0) return MSAM2_OK;
  MSAM2_REQUIRE(logits && offsets && counts, "mask_rle: null tensor");
  hipLaunchKernelGGL(rle_write_kernel, dim3((unsigned)M), dim3(RLE_THREADS), 0, (hipStream_t)stream, logits, (int)lh, (int)lw, (int)h, (int)w,
                     (int)x0, (int)y0, (int)H, H * W, thr, offsets, counts);
  return msam2_check_launch("mask_rle");
}

extern "C" size_t msam2_box_nms_workspace_bytes(int64_t K) {
  if (K <= 0) return 0;
  const int64_t nw = (K + 63) / 64;                         // (64-bit: this entry takes any K)
  return nms_ws_order_bytes(K) + (size_t)(K * nw) * sizeof(unsigned long long);
}

extern "C" int msam2_box_nms(const float* boxes, const float* scores, int64_t K, float iou_thr, int64_t* keep, int* n_keep, void* workspace,
                             size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(K >= 0 && K <= NMS_MAX_K, "box_nms: K = %lld boxes (at most %lld)", (long long)K, (long long)NMS_MAX_K);
  static_assert(NMS_MAX_WORDS * sizeof(unsigned long long) + sizeof(unsigned long long) <= 64 * 1024, "box_nms: sweep LDS");
  MSAM2_REQUIRE(n_keep, "box_nms: null n_keep");
  hipStream_t s = (hipStream_t)stream;
  if (K == 0) {
    fill_on(s, n_keep, 1, 0);
    return msam2_check_launch("box_nms");
  }
  MSAM2_REQUIRE(boxes && scores && keep && workspace, "box_nms: null tensor");
  MSAM2_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "box_nms: boxes and workspace must be 16-byte aligned");
  MSAM2_REQUIRE(workspace_bytes >= msam2_box_nms_workspace_bytes(K), "box_nms: workspace too small");
  const int nw = cdiv(K, 64);
  int* order = (int*)workspace;
  unsigned long long* mask = (unsigned long long*)((char*)workspace + nms_ws_order_bytes(K));
  hipLaunchKernelGGL(nms_rank_kernel, dim3(cdiv(K, 256)), dim3(256), 0, s, scores, (int)K, order);
  hipLaunchKernelGGL(nms_mask_kernel, dim3(cdiv(K * nw, 256)), dim3(256), 0, s, boxes, (const int*)order, (int)K, nw, iou_thr, mask);
  hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(256), (size_t)nw * sizeof(unsigned long long), s, (const unsigned long long*)mask,
                     (const int*)order, (int)K, nw, keep, n_keep);
  return msam2_check_launch("box_nms");
}
