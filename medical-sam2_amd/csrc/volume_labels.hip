// End of the 3-D path: label volumes and per-organ counts straight from the low-resolution logits [T, n, lh, lw] fp32 that
// volume.segment_volume returns, gfx950.
//
// The composition this replaces up-samples every slice to video resolution (n x H x W fp32 written and read back: 54.5 MB per slice for 13
// organs at 1024^2), takes the per-pixel arg-max with torch reductions and scores every (slice, object) with a call and a host copy of
// its own.  Here one kernel re-evaluates the bilinear resize (align_corners = False) per output voxel, as mask_stats_kernel (amg.hip)
// does, with the ROUNDINGS of the kernel msam2_bilinear_upsample would run for the same output size (resize_taps / resize_value below),
// so every label and every count equals, integer for integer, the one taken from msam2_bilinear_upsample's output, and no high-res
// logits exist: a slice reads n x lh x lw floats (L2-resident) and writes one byte per voxel.  Counters are integers (ballot / popcount
// per wave, LDS, one global atomic per workgroup and counter): exact and independent of order.
#include "common.h"

namespace {

// ---- the per-pixel value of msam2_bilinear_upsample, rounding for rounding ------------------------------------------------------------
// Siblings: bilinear_kernel / bilinear4_kernel (elementwise.hip) and bilerp_at (amg.hip) all spell the same expression,
//   (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d),      a b = row y0, c d = row y1,
// and leave its contraction into fused multiply-adds to the compiler (hipcc's default -ffp-contract=fast).  Which products get fused is
// then decided per kernel by the vectoriser, and the listings (tools/isa_diff.py keeps them) show that the siblings do NOT agree in the
// last bit:
//   * bilinear4_kernel (W % 4 == 0, what msam2_bilinear_upsample runs for every size of the 3-D path), pixel X:
//       B = fma(1 - lx, c, lx * d)  in both cases;
//       X even:  A = fma(1 - lx, a, lx * b),  v = fma(ly, B, (1 - ly) * A);
//       X odd:   A = fma(lx, b, (1 - lx) * a),  v = fma(1 - ly, A, ly * B);
//   * bilinear_kernel when every thread has one pixel (W % 4 != 0 and planes * H * W <= 2^22; bilerp_at in mask_stats_kernel compiles to
//     the same):  A = fma(lx, b, (1 - lx) * a),  B as above,  v = (1 - ly) * A + ly * B  with both products rounded;
//   * bilinear_kernel beyond 2^22 output elements runs a two-pixel body with a third pattern for the threads that have two pixels and
//     the one above for the rest: the bits of a pixel then depend on the launch, and no per-pixel function can follow them.
// A label or a count differs between two such forms only where a value lies within an ulp of a threshold or of another object's value,
// which a test meets once in ~10^8 comparisons; "equal, integer for integer" has to hold by construction, so this file does not share the
// spelled-out expression: it states the fused multiply-adds explicitly, contraction off, in the form of the kernel that
// msam2_bilinear_upsample runs for the same W (first form for W % 4 == 0, second otherwise).  tests/test_volume_labels_gpu.py compares
// against msam2_bilinear_upsample's output for both.  If elementwise.hip or the compiler changes those kernels' contraction, that test
// is what notices.
struct ResizeTaps {            // what a pixel's value needs besides the plane: independent of the object, hoisted out of its loop
  int o00, o01, o10, o11;      // element offsets of a, b, c, d in a plane
  float lx, mx, ly, my;        // mx = 1 - lx, my = 1 - ly
};

__device__ __forceinline__ ResizeTaps resize_taps(int h, int w, float sy, float sx, int Y, int X) {
#pragma clang fp contract(off)
  const float fy = fmaxf(__builtin_fmaf(Y + 0.5f, sy, -0.5f), 0.f), fx = fmaxf(__builtin_fmaf(X + 0.5f, sx, -0.5f), 0.f);
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  ResizeTaps t;
  t.o00 = y0 * w + x0;
  t.o01 = y0 * w + x1;
  t.o10 = y1 * w + x0;
  t.o11 = y1 * w + x1;
  t.ly = fy - y0;
  t.lx = fx - x0;
  t.my = 1.f - t.ly;
  t.mx = 1.f - t.lx;
  return t;
}

// vec4_form: the roundings of bilinear4_kernel (W % 4 == 0), else those of the one-pixel path of bilinear_kernel; odd = X & 1
__device__ __forceinline__ float resize_value(const float* __restrict__ p, const ResizeTaps& t, bool vec4_form, bool odd) {
#pragma clang fp contract(off)
  const float a = p[t.o00], b = p[t.o01], c = p[t.o10], d = p[t.o11];
  const float B = __builtin_fmaf(t.mx, c, t.lx * d);
  const float A_first = __builtin_fmaf(t.mx, a, t.lx * b), A_second = __builtin_fmaf(t.lx, b, t.mx * a);
  const float even4 = __builtin_fmaf(t.ly, B, t.my * A_first), odd4 = __builtin_fmaf(t.my, A_second, t.ly * B);
  const float one = t.my * A_second + t.ly * B;
  return vec4_form ? (odd ? odd4 : even4) : one;
}

constexpr int LBL_THREADS = 256, LBL_ITER = 4;          // voxel groups per thread: a workgroup owns 1024 groups of VPT voxels of one slice
constexpr int LBL_MAX_THR = 8;

// Host side of both entries.  The refusal of their sizes (entry: a string literal):
#define LBL_REQUIRE_SIZES(entry, T, lh, lw, H, W)                                                                                        \
  MSAM2_REQUIRE((T) >= 1 && (T) <= LABEL_MAX_SLICES && (lh) > 0 && (lw) > 0 && (H) > 0 && (W) > 0 && (lh) * (lw) < (1ll << 31) &&       \
                    (H) * (W) < (1ll << 31),                                                                                             \
                entry ": bad sizes (T %lld, low-res %lldx%lld, output %lldx%lld)", (long long)(T), (long long)(lh), (long long)(lw),   \
                (long long)(H), (long long)(W))
// The VPT x COUNT ladder and the grid: launch(VPT and COUNT as std::integral_constant values, grid) for the instance that applies
template <typename F>
static inline void lbl_dispatch(bool vec4, bool count, int64_t T, int64_t H, int64_t W, F&& launch) {
  auto go = [&](auto vpt, auto cnt) { launch(vpt, cnt, dim3(cdiv(H * (W / decltype(vpt)::value), (int64_t)LBL_THREADS * LBL_ITER), (unsigned)T)); };
  const std::integral_constant<int, 4> four;
  const std::integral_constant<int, 1> one;
  if (vec4) count ? go(four, std::true_type{}) : go(four, std::false_type{});
  else count ? go(one, std::true_type{}) : go(one, std::false_type{});
}

// Counts of one object over the VPT voxels of each lane of this wave, added to the workgroup's LDS counters c[k * kstride + (0, 1, 2)] =
// (|P & G|, |P|, |G|) of threshold k.  P = in && v > th[k]; the ballots are wave-uniform, so are the branches around the LDS atomics.
template <int VPT>
__device__ __forceinline__ void tally_object(int* c, int kstride, const float (&v)[VPT], const bool (&in)[VPT], const bool (&g)[VPT],
                                             const float (&th)[LBL_MAX_THR], int K, bool lane0) {
  unsigned long long mg[VPT];
  int cg = 0;
#pragma unroll
  for (int e = 0; e < VPT; ++e) {
    mg[e] = __ballot(g[e]);
    cg += __popcll(mg[e]);
  }
#pragma unroll
  for (int k = 0; k < LBL_MAX_THR; ++k) {
    if (k >= K) break;
    int cp = 0, ci = 0;
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
      const unsigned long long mp = __ballot(in[e] && v[e] > th[k]);
      cp += __popcll(mp);
      ci += __popcll(mp & mg[e]);
    }
    if (lane0) LABEL_OVERLAP_ADD(c + k * kstride, ci, cp, cg);
  }
}

// The group of VPT voxels a thread has in iteration `it` of its workgroup: g of `groups` (Wg per row), first voxel (Y, X0).  Dead lanes
// recompute the last group (no divergent loads) and are masked by `live`.
template <int VPT>
struct VoxelGroup {
  bool live;
  int g, Y, X0;
  __device__ __forceinline__ VoxelGroup(int it, int groups, int Wg) {
    const int64_t gi = ((int64_t)blockIdx.x * LBL_ITER + it) * LBL_THREADS + threadIdx.x;
    live = gi < groups;
    g = live ? (int)gi : groups - 1;
    Y = g / Wg, X0 = (g - Y * Wg) * VPT;
  }
};
// a group's output bytes, packed one per voxel from bit 0: one 4-byte store (VPT = 4, `at` a multiple of 4 in an aligned volume) or one byte
template <int VPT>
__device__ __forceinline__ void store_group(uint8_t* __restrict__ vol, int64_t at, unsigned bytes) {
  if (VPT == 4) *reinterpret_cast<unsigned*>(vol + at) = bytes;
  else vol[at] = (uint8_t)bytes;
}

// One thread: VPT consecutive X of one row (VPT = 4 needs W % 4 == 0 and 4-byte aligned labels / gt: one 4-byte load and store), the
// object loop innermost, so a voxel's n values never leave the registers; the taps and weights do not depend on the object.
// VPT = 4: the form of a pixel's value is known at compile time (W % 4 == 0, parity of e); VPT = 1 also serves W % 4 == 0 with unaligned
// labels / gt, so it selects per lane.  blockIdx.y = slice.  labels / gt / counts may each be null (the host entry checks which).
template <int VPT, bool COUNT>
__global__ __launch_bounds__(LBL_THREADS) void label_slices_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ ids, int n,
                                                                   int lh, int lw, int H, int W, float label_thr,
                                                                   const float* __restrict__ thr, int K, const uint8_t* __restrict__ gt,
                                                                   int exclusive, uint8_t* __restrict__ labels, int* __restrict__ counts,
                                                                   int T) {
  const int t = blockIdx.y;
  const int plane = lh * lw;
  const float* base = logits + (int64_t)t * n * plane;
  const float sy = (float)lh / H, sx = (float)lw / W;
  const int Wg = W / VPT, groups = H * Wg;                  // H * W < 2^31 (host)
  const int64_t slice = (int64_t)t * H * W;
  const bool lane0 = (threadIdx.x & 63) == 0;
  __shared__ int cnt[COUNT ? LBL_MAX_THR * LABEL_MAX_OBJ * 3 : 1];
  float th[LBL_MAX_THR];
  if (COUNT) {
#pragma unroll
    for (int k = 0; k < LBL_MAX_THR; ++k) th[k] = k < K ? thr[k] : INFINITY;
    for (int i = threadIdx.x; i < K * n * 3; i += LBL_THREADS) cnt[i] = 0;
    __syncthreads();
  }
#pragma unroll 1
  for (int it = 0; it < LBL_ITER; ++it) {
    const VoxelGroup<VPT> vg(it, groups, Wg);
    const bool live = vg.live;
    const int g = vg.g, Y = vg.Y, X0 = vg.X0;
    uint8_t gb[VPT];
#pragma unroll
    for (int e = 0; e < VPT; ++e) gb[e] = 0;
    const bool has_gt = COUNT && gt != nullptr;
    if (has_gt) {
      if (VPT == 4) {
        const unsigned u = *reinterpret_cast<const unsigned*>(gt + slice + (int64_t)g * 4);
#pragma unroll
        for (int e = 0; e < VPT; ++e) gb[e] = (uint8_t)(u >> (8 * e));
      } else {
        gb[0] = gt[slice + g];
      }
    }
    float bv[VPT];
    int bo[VPT];
    bool in[VPT], gbit[VPT];
    ResizeTaps taps[VPT];
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
      bv[e] = label_thr;
      bo[e] = -1;
      in[e] = live;
      taps[e] = resize_taps(lh, lw, sy, sx, Y, X0 + e);
    }
    const bool vec4_form = VPT == 4 || (W & 3) == 0;
    for (int o = 0; o < n; ++o) {
      const float* p = base + (int64_t)o * plane;
      float v[VPT];
#pragma unroll
      for (int e = 0; e < VPT; ++e) {
        v[e] = resize_value(p, taps[e], vec4_form, VPT == 4 ? (e & 1) != 0 : (X0 & 1) != 0);
        if (v[e] > bv[e]) {                                   // strict: ties to the lower index, background at exactly label_thr, NaN never wins
          bv[e] = v[e];
          bo[e] = o;
        }
      }
      if (COUNT && !exclusive) {
        const uint8_t id = ids[o];
#pragma unroll
        for (int e = 0; e < VPT; ++e) gbit[e] = live && has_gt && gb[e] == id;
        tally_object<VPT>(cnt + o * 3, n * 3, v, in, gbit, th, K, lane0);
      }
    }
    if (COUNT && exclusive) {
      for (int o = 0; o < n; ++o) {
        const uint8_t id = ids[o];
#pragma unroll
        for (int e = 0; e < VPT; ++e) {
          gbit[e] = live && has_gt && gb[e] == id;
          in[e] = live && bo[e] == o;
        }
        tally_object<VPT>(cnt + o * 3, n * 3, bv, in, gbit, th, K, lane0);
      }
    }
    if (labels != nullptr && live) {
      unsigned u = 0;
#pragma unroll
      for (int e = 0; e < VPT; ++e) u |= (unsigned)(bo[e] >= 0 ? ids[bo[e]] : (uint8_t)0) << (8 * e);
      store_group<VPT>(labels, slice + (int64_t)g * VPT, u);
    }
  }
  if (COUNT) {
    __syncthreads();
    const int per_k = n * 3;
    for (int i = threadIdx.x; i < K * per_k; i += LBL_THREADS) {
      const int c = cnt[i];
      const int k = i / per_k;
      if (c) atomicAdd(counts + ((int64_t)k * T + t) * per_k + (i - k * per_k), c);
    }
  }
}

}  // namespace

extern "C" int msam2_label_slices(const float* logits, const uint8_t* ids, int64_t T, int64_t n, int64_t lh, int64_t lw, int64_t H, int64_t W,
                                  float label_thr, const float* thresholds, int64_t K, const uint8_t* gt, int exclusive, uint8_t* labels,
                                  int* counts, void* stream) {
  MSAM2_REQUIRE(logits && ids, "label_slices: null logits / ids");
  LABEL_REQUIRE_OBJECTS("label_slices", n);
  MSAM2_REQUIRE(K >= 0 && K <= LBL_MAX_THR, "label_slices: K = %lld thresholds (at most %d per call)", (long long)K, LBL_MAX_THR);
  LBL_REQUIRE_SIZES("label_slices", T, lh, lw, H, W);
  MSAM2_REQUIRE(labels || counts, "label_slices: neither labels nor counts requested");
  MSAM2_REQUIRE(!counts || (K >= 1 && thresholds), "label_slices: counts need 1 .. %d thresholds", LBL_MAX_THR);
  hipStream_t s = (hipStream_t)stream;
  if (counts) fill_on(s, counts, K * T * n * 3, 0);         // (common.h: why a kernel)
  const uint8_t* g = counts ? gt : nullptr;
  const bool vec4 = W % 4 == 0 && (((uintptr_t)labels | (uintptr_t)g) & 3) == 0;
  lbl_dispatch(vec4, counts != nullptr, T, H, W, [&](auto vpt, auto cnt, dim3 grid) {
    hipLaunchKernelGGL((label_slices_kernel<decltype(vpt)::value, decltype(cnt)::value>), grid, dim3(LBL_THREADS), 0, s, logits, ids, (int)n, (int)lh, (int)lw, (int)H,
                       (int)W, label_thr, thresholds, (int)K, g, exclusive, labels, counts, (int)T);
  });
  return msam2_check_launch("label_slices");
}

// ---- how far every decision was from going the other way: msam2_label_confidence ---------------------------------------------------------
// label_slices_kernel evaluates v_o for every object at every voxel, keeps the arg-max and drops the rest.  This kernel keeps, in the
// same single pass over the objects, the top value tv with its object to and the second value sv (strict comparisons: ties to the lower
// index, a tied value becomes sv, NaN never enters), and from them
//   labelled (tv > label_thr):            m = m_in  = tv - fmaxf(label_thr, sv)      how far the label is from changing
//   background with a finite tv:          m = m_out = label_thr - tv                 how far the nearest object `to` is from claiming it
// (one fp32 subtraction each, >= 0).  margins[0 .. K) ascending cut m into bands; `select` picks the band of the core / envelope volumes.
// Same shape as label_slices_kernel: blockIdx.y = slice, object loop innermost with the voxel's values in registers, VPT = 4 with one
// 4-byte store per requested volume, dead lanes recompute the last group, integer counters in LDS and one global atomicAdd per workgroup
// and non-zero counter.
//
// Counters, per (slice, object): col 0 voxels labelled o; col 1 voxels with v_o > label_thr that another object took (the workgroup
// accumulates #{v_o > label_thr} there, one ballot per object and voxel of a lane inside the object loop, and subtracts col 0 when it
// flushes); cols 2 .. 2 + K labelled o with m_in < margins[k]; cols 2 + K .. 2 + 2K background nearest o with m_out < margins[k].
// CHOSEN for cols 0 and 2 ..: a voxel belongs to ONE object there (to), so the wave walks the distinct `to` values it holds -- first pending
// lane's object broadcast, that object's lanes retired, (1 + 2K) ballots per voxel of a lane for it, lane 0 adds the non-zero popcounts to
// LDS.  A wave of 64 x VPT neighbouring voxels holds a handful of objects on an organ map, so this costs (distinct objects) x (1 + 2K) x VPT
// ballots where tally_object's form (every object asks every lane) would cost n x (1 + 2K) x VPT.  The alternative has not been built;
// tools/confidence_bench.py times the entry with and without counts, which bounds what the walk costs.
namespace {

constexpr int CONF_MAX_BANDS = 8;
constexpr int CONF_MAX_COLS = 2 + 2 * CONF_MAX_BANDS;
struct ConfMargins {           // by value in the kernel arguments: the launch reads no host memory later, so it can be captured
  float m[CONF_MAX_BANDS];     // [K ..) = +inf, never looked at
};

template <int VPT, bool COUNT>
__global__ __launch_bounds__(LBL_THREADS) void label_confidence_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ ids, int n,
                                                                       int lh, int lw, int H, int W, float label_thr, ConfMargins mg, int K,
                                                                       int select, uint8_t* __restrict__ labels, uint8_t* __restrict__ core,
                                                                       uint8_t* __restrict__ envelope, uint8_t* __restrict__ conf,
                                                                       int* __restrict__ counts) {
  const int t = blockIdx.y;
  const int plane = lh * lw;
  const float* base = logits + (int64_t)t * n * plane;
  const float sy = (float)lh / H, sx = (float)lw / W;
  const int Wg = W / VPT, groups = H * Wg;                  // H * W < 2^31 (host)
  const int64_t slice = (int64_t)t * H * W;
  const bool lane0 = (threadIdx.x & 63) == 0;
  const int cols = 2 + 2 * K;
  __shared__ int cnt[COUNT ? LABEL_MAX_OBJ * CONF_MAX_COLS : 1];
  if (COUNT) {
    for (int i = threadIdx.x; i < n * cols; i += LBL_THREADS) cnt[i] = 0;
    __syncthreads();
  }
  const float m_sel = mg.m[select];
#pragma unroll 1
  for (int it = 0; it < LBL_ITER; ++it) {
    const VoxelGroup<VPT> vg(it, groups, Wg);
    const bool live = vg.live;
    const int g = vg.g, Y = vg.Y, X0 = vg.X0;
    float tv[VPT], sv[VPT];
    int to[VPT];
    ResizeTaps taps[VPT];
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
      tv[e] = sv[e] = -INFINITY;
      to[e] = -1;
      taps[e] = resize_taps(lh, lw, sy, sx, Y, X0 + e);
    }
    const bool vec4_form = VPT == 4 || (W & 3) == 0;
    for (int o = 0; o < n; ++o) {
      const float* p = base + (int64_t)o * plane;
      int above = 0;
#pragma unroll
      for (int e = 0; e < VPT; ++e) {
        const float v = resize_value(p, taps[e], vec4_form, VPT == 4 ? (e & 1) != 0 : (X0 & 1) != 0);
        if (v > tv[e]) {                                      // strict: ties to the lower index, the tied value becomes sv; NaN never enters
          sv[e] = tv[e];
          tv[e] = v;
          to[e] = o;
        } else if (v > sv[e]) {
          sv[e] = v;
        }
        if (COUNT) above += __popcll(__ballot(live && v > label_thr));
      }
      if (COUNT && lane0 && above) atomicAdd(cnt + o * cols + 1, above);
    }
    bool lab[VPT];
    unsigned below[VPT];                                      // bit k: m < margins[k]
    unsigned lb = 0, cb = 0, eb = 0, fb = 0;                   // the four output bytes of each voxel, packed
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
      lab[e] = tv[e] > label_thr;
      const bool near = !lab[e] && tv[e] > -INFINITY && tv[e] < INFINITY;   // background with a finite top value: `to` is its nearest object
      const float m = lab[e] ? tv[e] - fmaxf(label_thr, sv[e]) : label_thr - tv[e];
      unsigned lt = 0, ge = 0;
#pragma unroll
      for (int k = 0; k < CONF_MAX_BANDS; ++k) {
        if (k >= K) break;
        lt |= (unsigned)(m < mg.m[k]) << k;
        ge += m >= mg.m[k];
      }
      const bool owned = lab[e] || near;
      below[e] = owned ? lt : 0u;
      if (!(live && owned)) to[e] = -1;                       // from here on: the object whose band columns this voxel counts in, or none
      const unsigned id = owned ? ids[to[e] < 0 ? 0 : to[e]] : 0u;
      const unsigned idl = lab[e] ? id : 0u;
      lb |= idl << (8 * e);
      cb |= (lab[e] && m >= m_sel ? id : 0u) << (8 * e);
      eb |= (lab[e] || (near && m < m_sel) ? id : 0u) << (8 * e);
      fb |= (owned ? ge : (unsigned)K) << (8 * e);
    }
    if (live) {
      const int64_t at = slice + (int64_t)g * VPT;
      if (labels) store_group<VPT>(labels, at, lb);
      if (core) store_group<VPT>(core, at, cb);
      if (envelope) store_group<VPT>(envelope, at, eb);
      if (conf) store_group<VPT>(conf, at, fb);
    }
    if (COUNT) {
      for (;;) {                                              // the distinct objects this wave holds, one per turn (wave-uniform trip count)
        int cand = -1;
#pragma unroll
        for (int e = 0; e < VPT; ++e) cand = to[e] >= 0 ? to[e] : cand;
        const unsigned long long any = __ballot(cand >= 0);
        if (!any) break;
        const int o = __shfl(cand, __ffsll((long long)any) - 1);
        bool in[VPT], out[VPT];
        int c0 = 0;
#pragma unroll
        for (int e = 0; e < VPT; ++e) {
          const bool mine = to[e] == o;
          in[e] = mine && lab[e];
          out[e] = mine && !lab[e];
          if (mine) to[e] = -1;                               // retired
          c0 += __popcll(__ballot(in[e]));
        }
        int* c = cnt + o * cols;
        if (lane0 && c0) atomicAdd(c, c0);
#pragma unroll
        for (int k = 0; k < CONF_MAX_BANDS; ++k) {
          if (k >= K) break;
          int ci = 0, co = 0;
#pragma unroll
          for (int e = 0; e < VPT; ++e) {
            const bool b = (below[e] >> k) & 1u;
            ci += __popcll(__ballot(in[e] && b));
            co += __popcll(__ballot(out[e] && b));
          }
          if (lane0 && ci) atomicAdd(c + 2 + k, ci);
          if (lane0 && co) atomicAdd(c + 2 + K + k, co);
        }
      }
    }
  }
  if (COUNT) {
    __syncthreads();
    for (int i = threadIdx.x; i < n * cols; i += LBL_THREADS) {
      const int col = i % cols;
      const int c = col == 1 ? cnt[i] - cnt[i - 1] : cnt[i];   // #{v_o > label_thr} minus the voxels o labelled: what another object took
      if (c) atomicAdd(counts + (int64_t)t * n * cols + i, c);
    }
  }
}

}  // namespace

extern "C" int msam2_label_confidence(const float* logits, const uint8_t* ids, int64_t T, int64_t n, int64_t lh, int64_t lw, int64_t H, int64_t W,
                                      float label_thr, const float* margins, int64_t K, int64_t select, uint8_t* labels, uint8_t* core,
                                      uint8_t* envelope, uint8_t* conf, int* counts, void* stream) {
  MSAM2_REQUIRE(logits && ids && margins, "label_confidence: null logits / ids / margins");
  LABEL_REQUIRE_OBJECTS("label_confidence", n);
  MSAM2_REQUIRE(K >= 1 && K <= CONF_MAX_BANDS, "label_confidence: K = %lld margins (1 .. %d per call)", (long long)K, CONF_MAX_BANDS);
  LBL_REQUIRE_SIZES("label_confidence", T, lh, lw, H, W);
  ConfMargins mg;
  for (int k = 0; k < CONF_MAX_BANDS; ++k) {
    mg.m[k] = INFINITY;
    if (k >= K) continue;
    const float m = margins[k];                              // a HOST pointer: read here, passed on by value
    MSAM2_REQUIRE(std::isfinite(m) && m > 0.f && (k == 0 || m > mg.m[k - 1]),
                  "label_confidence: margins[%d] = %g (finite, positive and strictly ascending)", k, (double)m);
    mg.m[k] = m;
  }
  MSAM2_REQUIRE(select >= 0 && select < K, "label_confidence: select = %lld (0 .. %lld)", (long long)select, (long long)(K - 1));
  MSAM2_REQUIRE(labels || core || envelope || conf || counts, "label_confidence: no output requested (labels, core, envelope, conf, counts)");
  hipStream_t s = (hipStream_t)stream;
  if (counts) fill_on(s, counts, T * n * (2 + 2 * K), 0);
  const bool vec4 = W % 4 == 0 && (((uintptr_t)labels | (uintptr_t)core | (uintptr_t)envelope | (uintptr_t)conf) & 3) == 0;
  lbl_dispatch(vec4, counts != nullptr, T, H, W, [&](auto vpt, auto cnt, dim3 grid) {
    hipLaunchKernelGGL((label_confidence_kernel<decltype(vpt)::value, decltype(cnt)::value>), grid, dim3(LBL_THREADS), 0, s, logits, ids, (int)n,
                       (int)lh, (int)lw, (int)H, (int)W, label_thr, mg, (int)K, (int)select, labels, core, envelope, conf, counts);
  });
  return msam2_check_launch("label_confidence");
}
