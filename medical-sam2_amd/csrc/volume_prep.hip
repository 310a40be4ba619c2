// Start of the 3-D path, first step: volume intake.  A raw slice stack [T, Cin, H0, W0] (uint8 / int16 / float32) becomes 8-bit greys at
// S x S and / or the normalised fp32 [T, 3, S, S] model input; a raw label map [T, H0, W0] becomes the uint8 [T, S, S] label volume.  gfx950.
//
// The contract is Pillow's, byte for byte: what `Image.fromarray(x).convert("RGB").resize((S, S))` (8-bit bicubic, a = -0.5) gives for the
// greys and `Image.fromarray(mask).resize((S, S))` (nearest) for the labels, the loop the reference's dataset runs per slice and per
// (slice, object) on the host (func_3d/dataset/btcv.py:60-104), then `(x / 255 - mean) / std` in fp32 (utils/misc.py:205-244).  Pillow
// resamples 8-bit images in fixed point: coefficients rounded to 22 fractional bits, the horizontal pass first, then the vertical one, each
// pass `clip8((1 << 21) + sum(pixel * coefficient) >> 22)` with an int32 accumulator, a pass skipped when its dimension already fits.  The
// integer coefficient tables [S, ksize] and bounds [S, 2] = (first source index, tap count) per axis come from the caller (computed in
// float64 on the host: volume_prep.resample_tables); no kernel here evaluates the cubic.  Every table entry is clamped before use, so a
// table that is not what the host computes gives other bytes, never an access outside the source, the workspace or the LDS tiles.
//
// Output channel c reads source plane c % Cin with window c.  Channels that share plane and window (the default: one CT window replicated
// to RGB, as convert("RGB") does for a grey image) form one GROUP: resampled once, stored once per channel.
//
// Window rule (source value -> g in 0 .. 255), once per source pixel:
//   uint8    g = the byte
//   int16    h = clamp(v, lo, hi); g = (510 (h - lo) + (hi - lo)) / (2 (hi - lo)) in int32: round-half-up of 255 (h - lo) / (hi - lo), exact
//   float32  NaN -> 0; t = clamp((double)v, lo, hi); g = floor(((t - lo) * 255.0) / (hi - lo) + 0.5), every operation a correctly rounded
//            float64 one (no fused multiply-add): numpy float64 gives the same bits
//
// Fused form (volume_prep_fused_kernel): a workgroup owns a PREP_TW x PREP_TH output tile of one (slice, group).  It windows the source
// span the tile needs into an LDS byte tile (once per source pixel, not once per tap), runs the horizontal pass into a second LDS byte
// tile (the source rows the tile's output rows need x PREP_TW), then the vertical pass with four pixels per lane: one ds_read_b32 per tap
// and lane, one 16-byte fp32 store (and one 4-byte grey store) per lane and channel.  The tile's coefficient rows sit in LDS too, and so
// does the [3][256] table of normalised values (IEEE fp32 divisions, computed once per workgroup instead of twice per output element).
// The span grows with H0 / S and W0 / S; when tiles plus tables exceed PREP_LDS_BUDGET the entry runs the two passes as two launches
// (volume_prep_hpass_kernel -> uint8 workspace [T, 3, H0, S] -> volume_prep_vpass_kernel).  Same integers either way, so the same bytes.
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int PREP_THREADS = 256;
constexpr int PREP_TW = 64, PREP_TH = 32;        // output tile of the fused form: 16 lanes x 4 pixels wide, two rounds of 16 rows
constexpr int PREP_LDS_BUDGET = 64 * 1024;       // no opt-in attribute needed; two workgroups per CU at the limit, ~8 KiB at 512 -> 1024
constexpr int PREP_LUT_BYTES = 3 * 256 * 4;
constexpr int PREP_BITS = 22;                    // Pillow's PRECISION_BITS = 32 - 8 - 2
enum { SRC_U8 = 0, SRC_I16 = 1, SRC_F32 = 2 };

}  // namespace

struct PrepParams {
  const void* src;
  int T, Cin, H0, W0, S;
  int ilo[3], ihi[3];                            // int16 windows
  double lo[3], hi[3];                           // float32 windows
  const int *kx, *bx, *ky, *by;                  // coefficient rows and (first, count) bounds; ksx / ksy == 0: that pass is skipped
  int ksx, ksy;
  uint8_t* grey;
  float* out;
  float mean[3], sd[3];
  int ngroups, rep[3];                           // group g is computed from channel rep[g] ..
  unsigned mask[3];                              // .. and stored to the channels of mask[g]
  int vec;                                       // S % 4 == 0 and both outputs aligned: 4-pixel stores
  int src_rows, src_pitch;                       // LDS tiles of the fused form
  uint8_t* ws;                                   // two-launch form: [T, 3, H0, S]
};

namespace {

template <typename T> __device__ __forceinline__ int window(T v, int c, const PrepParams& P);
template <> __device__ __forceinline__ int window<uint8_t>(uint8_t v, int, const PrepParams&) { return v; }
template <> __device__ __forceinline__ int window<int16_t>(int16_t v, int c, const PrepParams& P) {
  const int lo = P.ilo[c], hi = P.ihi[c], h = min(max((int)v, lo), hi), w = hi - lo;
  return (510 * (h - lo) + w) / (2 * w);
}
template <> __device__ __forceinline__ int window<float>(float v, int c, const PrepParams& P) {
  if (v != v) return 0;
  const double lo = P.lo[c], hi = P.hi[c], t = fmin(fmax((double)v, lo), hi);
  return (int)floor(__dadd_rn(__ddiv_rn(__dmul_rn(__dsub_rn(t, lo), 255.0), __dsub_rn(hi, lo)), 0.5));
}

__device__ __forceinline__ int clip8(int ss) { return min(max(ss >> PREP_BITS, 0), 255); }

// a division, then a division: the arithmetic of load_video_frames_from_data (x / 255, then (x - mean) / std), see image_prep_kernel
__device__ __forceinline__ float normalised(int g, float mean, float sd) { return ((float)g / 255.0f - mean) / sd; }

// g[0 .. cnt) = the greys of output pixels (y, x .. x + cnt) of slice t, for every channel of `mask`.  lut: [3][256] or nullptr.
__device__ __forceinline__ void store_pixels(const PrepParams& P, const float* lut, int t, unsigned mask, int y, int x, const int (&g)[4], int cnt) {
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) {
    if (!((mask >> cc) & 1u)) continue;
    const int64_t idx = (((int64_t)t * 3 + cc) * P.S + y) * P.S + x;
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = lut ? lut[cc * 256 + g[j]] : normalised(g[j], P.mean[cc], P.sd[cc]);
    if (P.vec && cnt == 4) {
      if (P.grey) *reinterpret_cast<uint32_t*>(P.grey + idx) = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[2] << 16) | ((uint32_t)g[3] << 24);
      if (P.out) *reinterpret_cast<float4*>(P.out + idx) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
      for (int j = 0; j < cnt; ++j) {
        if (P.grey) P.grey[idx + j] = (uint8_t)g[j];
        if (P.out) P.out[idx + j] = f[j];
      }
    }
  }
}

// (first source index, tap count) of output o, clamped so that first + k < n_src for every k < count <= ks
__device__ __forceinline__ void taps(const int* __restrict__ b, int o, int ks, int n_src, int& first, int& count) {
  first = min(max(b[2 * o], 0), n_src - 1);
  count = min(max(b[2 * o + 1], 0), min(ks, n_src - first));
}

}  // namespace

// (the kernels are at global scope: the tests name them by what the profiler reports)
// blockIdx.x = tile (row-major over the S x S output), blockIdx.y = group, blockIdx.z = slice
template <typename T>
__global__ __launch_bounds__(PREP_THREADS) void volume_prep_fused_kernel(PrepParams P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, t = blockIdx.z, c = P.rep[blockIdx.y];
  const unsigned mask = P.mask[blockIdx.y];
  const int S = P.S, H0 = P.H0, W0 = P.W0, ksx = P.ksx, ksy = P.ksy;
  const int tiles_x = (S + PREP_TW - 1) / PREP_TW;
  const int x0 = (blockIdx.x % tiles_x) * PREP_TW, y0 = (blockIdx.x / tiles_x) * PREP_TH;
  const int nx = min(PREP_TW, S - x0), ny = min(PREP_TH, S - y0);

  float* lut = reinterpret_cast<float*>(smem);                         // [3][256]
  int* ckx = reinterpret_cast<int*>(smem + PREP_LUT_BYTES);            // [PREP_TW][ksx]
  int* cky = ckx + PREP_TW * ksx;                                      // [PREP_TH][ksy]
  int* bxs = cky + PREP_TH * ksy;                                      // [PREP_TW][2]: (first column inside the source tile, tap count)
  int* bys = bxs + 2 * PREP_TW;                                        // [PREP_TH][2]
  uint8_t* sv = reinterpret_cast<uint8_t*>(bys + 2 * PREP_TH);         // [src_rows][src_pitch]: the windowed source span
  uint8_t* hv = ksx ? sv + P.src_rows * P.src_pitch : sv;              // [src_rows][PREP_TW]: after the horizontal pass

  // the source span of the tile: bounds are monotone in the output index, so the first and the last output delimit it
  int xlo = x0, ncols = nx, ylo = y0, nrows = ny;
  if (ksx) {
    int f0, n0, f1, n1;
    taps(P.bx, x0, ksx, W0, f0, n0);
    taps(P.bx, x0 + nx - 1, ksx, W0, f1, n1);
    xlo = f0;
    ncols = min(max(f1 + n1 - f0, 1), P.src_pitch);
  }
  if (ksy) {
    int f0, n0, f1, n1;
    taps(P.by, y0, ksy, H0, f0, n0);
    taps(P.by, y0 + ny - 1, ksy, H0, f1, n1);
    ylo = f0;
    nrows = min(max(f1 + n1 - f0, 1), P.src_rows);
  }

  for (int i = tid; i < 3 * 256; i += PREP_THREADS) lut[i] = normalised(i & 255, P.mean[i >> 8], P.sd[i >> 8]);
  for (int i = tid; i < nx * ksx; i += PREP_THREADS) ckx[i] = P.kx[(int64_t)x0 * ksx + i];
  for (int i = tid; i < ny * ksy; i += PREP_THREADS) cky[i] = P.ky[(int64_t)y0 * ksy + i];
  if (ksx)
    for (int i = tid; i < nx; i += PREP_THREADS) {
      int f, n;
      taps(P.bx, x0 + i, ksx, W0, f, n);
      f = min(max(f - xlo, 0), ncols - 1);                             // inside the tile whatever the table holds
      bxs[2 * i] = f;
      bxs[2 * i + 1] = min(n, ncols - f);
    }
  if (ksy)
    for (int i = tid; i < ny; i += PREP_THREADS) {
      int f, n;
      taps(P.by, y0 + i, ksy, H0, f, n);
      f = min(max(f - ylo, 0), nrows - 1);
      bys[2 * i] = f;
      bys[2 * i + 1] = min(n, nrows - f);
    }

  // window: once per source pixel.  ylo + r < H0 and xlo + q < W0: taps() keeps first + count <= n_src, and nrows / ncols come from it
  const T* plane = static_cast<const T*>(P.src) + ((int64_t)t * P.Cin + c % P.Cin) * H0 * W0;
  for (int i = tid; i < nrows * ncols; i += PREP_THREADS) {
    const int r = i / ncols, q = i - r * ncols;
    sv[r * P.src_pitch + q] = (uint8_t)window<T>(plane[(int64_t)(ylo + r) * W0 + xlo + q], c, P);
  }
  __syncthreads();

  if (ksx) {
    for (int i = tid; i < nrows * PREP_TW; i += PREP_THREADS) {
      const int r = i / PREP_TW, x = i % PREP_TW;
      if (x >= nx) continue;
      const int f = bxs[2 * x], n = bxs[2 * x + 1];
      const uint8_t* s = sv + r * P.src_pitch + f;
      const int* k = ckx + x * ksx;
      int ss = 1 << (PREP_BITS - 1);
      for (int j = 0; j < n; ++j) ss += (int)s[j] * k[j];
      hv[r * PREP_TW + x] = (uint8_t)clip8(ss);
    }
    __syncthreads();
  }
  const int pitch = ksx ? PREP_TW : P.src_pitch;                       // (src_pitch is a multiple of 4 and so is the tile base)

  for (int i = tid; i < PREP_TH * (PREP_TW / 4); i += PREP_THREADS) {
    const int y = i / (PREP_TW / 4), x = (i % (PREP_TW / 4)) * 4;
    if (y >= ny || x >= nx) continue;
    int g[4];
    if (ksy) {
      const int f = bys[2 * y], n = bys[2 * y + 1];
      const int* k = cky + y * ksy;
      int ss[4] = {1 << (PREP_BITS - 1), 1 << (PREP_BITS - 1), 1 << (PREP_BITS - 1), 1 << (PREP_BITS - 1)};
      for (int j = 0; j < n; ++j) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(hv + (f + j) * pitch + x);
        const int w = k[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) ss[e] += (int)((v >> (8 * e)) & 0xffu) * w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = clip8(ss[e]);
    } else {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(hv + y * pitch + x);
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = (int)((v >> (8 * e)) & 0xffu);
    }
    store_pixels(P, lut, t, mask, y0 + y, x0 + x, g, min(4, nx - x));
  }
}

// Two-launch form, pass 1: ws[t][c][r][x] = the horizontal pass of source row r at output column x (the windowed byte when it is skipped).
// blockIdx.x: 256 elements of the [H0, S] plane, blockIdx.y = group, blockIdx.z = slice
template <typename T>
__global__ __launch_bounds__(PREP_THREADS) void volume_prep_hpass_kernel(PrepParams P) {
  const int i = blockIdx.x * PREP_THREADS + threadIdx.x, t = blockIdx.z, c = P.rep[blockIdx.y];
  if (i >= P.H0 * P.S) return;
  const int r = i / P.S, x = i - r * P.S;
  const T* row = static_cast<const T*>(P.src) + (((int64_t)t * P.Cin + c % P.Cin) * P.H0 + r) * P.W0;
  int v;
  if (P.ksx) {
    int f, n;
    taps(P.bx, x, P.ksx, P.W0, f, n);
    const int* k = P.kx + (int64_t)x * P.ksx;
    int ss = 1 << (PREP_BITS - 1);
    for (int j = 0; j < n; ++j) ss += window<T>(row[f + j], c, P) * k[j];
    v = clip8(ss);
  } else {
    v = window<T>(row[x], c, P);
  }
  P.ws[(((int64_t)t * 3 + c) * P.H0 + r) * P.S + x] = (uint8_t)v;
}

// pass 2: the vertical pass over the workspace and the stores.  blockIdx.x: 256 groups of four pixels of the S x S plane
__global__ __launch_bounds__(PREP_THREADS) void volume_prep_vpass_kernel(PrepParams P) {
  const int S = P.S, q = (S + 3) / 4;
  const int i = blockIdx.x * PREP_THREADS + threadIdx.x, t = blockIdx.z, c = P.rep[blockIdx.y];
  if (i >= S * q) return;
  const int y = i / q, x = (i - y * q) * 4, cnt = min(4, S - x);
  const uint8_t* col = P.ws + ((int64_t)t * 3 + c) * P.H0 * S + x;
  int g[4] = {0, 0, 0, 0};
  if (P.ksy) {
    int f, n;
    taps(P.by, y, P.ksy, P.H0, f, n);
    const int* k = P.ky + (int64_t)y * P.ksy;
    int ss[4] = {1 << (PREP_BITS - 1), 1 << (PREP_BITS - 1), 1 << (PREP_BITS - 1), 1 << (PREP_BITS - 1)};
    for (int j = 0; j < n; ++j) {
      const uint8_t* p = col + (int64_t)(f + j) * S;
      const int w = k[j];
      for (int e = 0; e < cnt; ++e) ss[e] += (int)p[e] * w;
    }
    for (int e = 0; e < cnt; ++e) g[e] = clip8(ss[e]);
  } else {
    const uint8_t* p = col + (int64_t)y * S;
    for (int e = 0; e < cnt; ++e) g[e] = p[e];
  }
  store_pixels(P, nullptr, t, P.mask[blockIdx.y], y, x, g, cnt);
}

namespace {

// Pillow's ksize for a resize of n_src to n_out samples (precompute_coeffs, support 2): 0 when the pass is skipped
int prep_ksize(int64_t n_src, int64_t n_out) {
  if (n_src == n_out) return 0;
  const double scale = (double)n_src / (double)n_out, support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;
}
// most source samples that `n` consecutive outputs read: first = (int)(centre - support + 0.5), end = (int)(centre + support + 0.5)
int prep_span(int64_t n_src, int64_t n_out, int n) {
  if (n_src == n_out) return n;
  const double scale = (double)n_src / (double)n_out, support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  const double span = ceil((n - 1) * scale + 2.0 * support) + 2.0;
  return span < (double)n_src ? (int)span : (int)n_src;
}

struct FusedShape {
  int rows, pitch;
  size_t lds;
};
FusedShape fused_shape(int64_t H0, int64_t W0, int64_t S) {
  FusedShape f;
  f.rows = prep_span(H0, S, PREP_TH);
  f.pitch = (prep_span(W0, S, PREP_TW) + 3) & ~3;
  const size_t ksx = prep_ksize(W0, S), ksy = prep_ksize(H0, S);
  f.lds = PREP_LUT_BYTES + 4 * (PREP_TW * ksx + PREP_TH * ksy) + 8 * (PREP_TW + PREP_TH) + (size_t)f.rows * f.pitch +
          (ksx ? (size_t)f.rows * PREP_TW : 0);
  return f;
}

bool prep_sizes_ok(int64_t T, int64_t H0, int64_t W0, int64_t S) {
  return label_sizes_ok(T, H0, W0, 1, LABEL_NO_VOXEL_CAP) && S >= 1 && S <= LABEL_MAX_SIDE;   // the source stack, and the output side
}

// MSAM2_VOLUME_PREP_FUSED, read per call: 0 = the two-launch form, 1 = the fused form (an error where it does not fit), unset = by size
int fused_switch() {
  const char* e = getenv("MSAM2_VOLUME_PREP_FUSED");
  return (e && (e[0] == '0' || e[0] == '1') && !e[1]) ? e[0] - '0' : -1;
}

template <typename T>
void launch_prep(const PrepParams& P, bool fused, size_t lds, hipStream_t s) {
  const unsigned groups = (unsigned)P.ngroups, T_ = (unsigned)P.T;
  if (fused) {
    const unsigned tiles = (unsigned)(cdiv(P.S, PREP_TW) * cdiv(P.S, PREP_TH));
    hipLaunchKernelGGL(volume_prep_fused_kernel<T>, dim3(tiles, groups, T_), dim3(PREP_THREADS), lds, s, P);
  } else {
    hipLaunchKernelGGL(volume_prep_hpass_kernel<T>, dim3((unsigned)cdiv((int64_t)P.H0 * P.S, PREP_THREADS), groups, T_), dim3(PREP_THREADS), 0, s, P);
    hipLaunchKernelGGL(volume_prep_vpass_kernel, dim3((unsigned)cdiv((int64_t)P.S * cdiv(P.S, 4), PREP_THREADS), groups, T_), dim3(PREP_THREADS),
                       0, s, P);
  }
}

// ---- label maps: nearest gather through two index maps ----
enum { LAB_U8 = 0, LAB_I16 = 1, LAB_I32 = 2, LAB_I64 = 3 };

}  // namespace

struct LabelResizeParams {
  const void* src;
  int T, H0, W0, S;
  const int *ymap, *xmap;
  uint32_t keep[8];
  uint8_t* out;
  int vec;                                        // S % 16 == 0 and out 16-byte aligned
};

// blockIdx.x: 256 chunks of 16 output voxels of one slice's [S, ceil(S / 16)] chunk grid, blockIdx.y = slice
template <typename T>
__global__ __launch_bounds__(PREP_THREADS) void label_resize_kernel(LabelResizeParams P) {
  const int S = P.S, q = (S + 15) / 16;
  const int i = blockIdx.x * PREP_THREADS + threadIdx.x, t = blockIdx.y;
  if (i >= S * q) return;
  const int y = i / q, x = (i - y * q) * 16, cnt = min(16, S - x);
  const int ys = min(max(P.ymap[y], 0), P.H0 - 1);
  const T* row = static_cast<const T*>(P.src) + ((int64_t)t * P.H0 + ys) * P.W0;
  uint32_t w[4] = {0, 0, 0, 0};
  for (int e = 0; e < cnt; ++e) {
    const int xs = min(max(P.xmap[x + e], 0), P.W0 - 1);
    const long long v = (long long)row[xs];
    uint32_t b = 0;
    if (v >= 1 && v <= 255) {
      const uint32_t u = (uint32_t)v;
      if ((P.keep[u >> 5] >> (u & 31u)) & 1u) b = u;
    }
    w[e >> 2] |= b << (8 * (e & 3));
  }
  uint8_t* o = P.out + ((int64_t)t * S + y) * S + x;
  if (P.vec) {
    *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (int e = 0; e < cnt; ++e) o[e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
  }
}

// Bytes of the uint8 workspace msam2_volume_prep needs for these sizes under the current MSAM2_VOLUME_PREP_FUSED setting: 0 when the call
// takes the fused form (and for sizes the entry refuses), else T * 3 * H0 * S.
extern "C" size_t msam2_volume_prep_workspace_bytes(int64_t T, int64_t H0, int64_t W0, int64_t S) {
  if (!prep_sizes_ok(T, H0, W0, S)) return 0;
  const int sw = fused_switch();
  if (sw != 0 && (sw == 1 || fused_shape(H0, W0, S).lds <= (size_t)PREP_LDS_BUDGET)) return 0;
  return (size_t)T * 3 * (size_t)H0 * (size_t)S;
}

extern "C" int msam2_volume_prep(const void* src, int src_type, int64_t T, int64_t Cin, int64_t H0, int64_t W0, int64_t S, const double* windows,
                                 const int* kx, const int* bx, int64_t ksize_x, const int* ky, const int* by, int64_t ksize_y, const float* mean3,
                                 const float* std3, uint8_t* grey_out, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(src && mean3 && std3, "volume_prep: null src / mean3 / std3 (mean3 / std3 are HOST pointers)");
  MSAM2_REQUIRE(grey_out || out, "volume_prep: at least one of grey_out and out is needed");
  MSAM2_REQUIRE(src_type == SRC_U8 || src_type == SRC_I16 || src_type == SRC_F32, "volume_prep: src_type %d (0 uint8, 1 int16, 2 float32)", src_type);
  MSAM2_REQUIRE(Cin == 1 || Cin == 3, "volume_prep: Cin = %lld (1 or 3)", (long long)Cin);
  MSAM2_REQUIRE(prep_sizes_ok(T, H0, W0, S), "volume_prep: bad sizes (T %lld of 1 .. %d, H0 x W0 %lldx%lld and S %lld of 1 .. %d)", (long long)T,
                LABEL_MAX_SLICES, (long long)H0, (long long)W0, (long long)S, LABEL_MAX_SIDE);
  MSAM2_REQUIRE(src_type == SRC_U8 || windows, "volume_prep: int16 / float32 sources need windows (HOST pointer to three (lo, hi) pairs)");
  MSAM2_REQUIRE(ksize_x == prep_ksize(W0, S) && ksize_y == prep_ksize(H0, S),
                "volume_prep: table sizes ksize_x %lld, ksize_y %lld; %lld -> %lld needs %d and %lld -> %lld needs %d (0: pass skipped)", (long long)ksize_x,
                (long long)ksize_y, (long long)W0, (long long)S, prep_ksize(W0, S), (long long)H0, (long long)S, prep_ksize(H0, S));
  MSAM2_REQUIRE((ksize_x == 0 || (kx && bx)) && (ksize_y == 0 || (ky && by)), "volume_prep: null coefficient / bounds table of a pass that runs");
  PrepParams P = {};
  P.src = src, P.T = (int)T, P.Cin = (int)Cin, P.H0 = (int)H0, P.W0 = (int)W0, P.S = (int)S;
  for (int c = 0; c < 3; ++c) {
    P.mean[c] = mean3[c], P.sd[c] = std3[c];
    P.ilo[c] = 0, P.ihi[c] = 1, P.lo[c] = 0.0, P.hi[c] = 1.0;
    if (src_type == SRC_U8) continue;
    const double lo = windows[2 * c], hi = windows[2 * c + 1];
    MSAM2_REQUIRE(lo < hi && isfinite(hi - lo), "volume_prep: window %d is (%g, %g): lo < hi and a finite width are needed", c, lo, hi);
    if (src_type == SRC_I16) {
      MSAM2_REQUIRE(lo >= -32768.0 && hi <= 32767.0 && lo == floor(lo) && hi == floor(hi),
                    "volume_prep: int16 window %d is (%g, %g): integers with -32768 <= lo < hi <= 32767 are needed", c, lo, hi);
      P.ilo[c] = (int)lo, P.ihi[c] = (int)hi;
    }
    P.lo[c] = lo, P.hi[c] = hi;
  }
  // groups: channel c joins the first channel with its plane and window
  for (int c = 0; c < 3; ++c) {
    int g = -1;
    for (int k = 0; k < P.ngroups && g < 0; ++k) {
      const int r = P.rep[k];
      if (r % Cin == c % Cin && (src_type == SRC_U8 || (P.lo[r] == P.lo[c] && P.hi[r] == P.hi[c]))) g = k;
    }
    if (g < 0) g = P.ngroups++, P.rep[g] = c;
    P.mask[g] |= 1u << c;
  }
  const int sw = fused_switch();
  const FusedShape fs = fused_shape(H0, W0, S);
  const bool fits = fs.lds <= (size_t)PREP_LDS_BUDGET;
  MSAM2_REQUIRE(sw != 1 || fits, "volume_prep: MSAM2_VOLUME_PREP_FUSED=1, but %lldx%lld -> %lld needs %zu bytes of LDS (budget %d)", (long long)H0,
                (long long)W0, (long long)S, fs.lds, PREP_LDS_BUDGET);
  const bool fused = sw != 0 && fits;
  if (!fused) {
    const size_t need = (size_t)T * 3 * (size_t)H0 * (size_t)S;
    MSAM2_REQUIRE(workspace && workspace_bytes >= need, "volume_prep: the two-launch form needs a workspace of %zu bytes, got %zu", need,
                  workspace ? workspace_bytes : (size_t)0);
  }
  P.kx = kx, P.bx = bx, P.ky = ky, P.by = by, P.ksx = (int)ksize_x, P.ksy = (int)ksize_y;
  P.grey = grey_out, P.out = out, P.ws = static_cast<uint8_t*>(workspace);
  P.vec = S % 4 == 0 && vec_ok(4, 1, (const void*)grey_out) && vec_ok(4, 4, (const void*)out);
  P.src_rows = fs.rows, P.src_pitch = fs.pitch;
  hipStream_t s = (hipStream_t)stream;
  if (src_type == SRC_U8) launch_prep<uint8_t>(P, fused, fs.lds, s);
  else if (src_type == SRC_I16) launch_prep<int16_t>(P, fused, fs.lds, s);
  else launch_prep<float>(P, fused, fs.lds, s);
  return msam2_check_launch("volume_prep");
}

extern "C" int msam2_label_resize(const void* src, int src_type, int64_t T, int64_t H0, int64_t W0, int64_t S, const int* ymap, const int* xmap,
                                  const uint32_t* keep8, uint8_t* out, void* stream) {
  MSAM2_REQUIRE(src && ymap && xmap && out, "label_resize: null src / ymap / xmap / out");
  MSAM2_REQUIRE(src_type >= LAB_U8 && src_type <= LAB_I64, "label_resize: src_type %d (0 uint8, 1 int16, 2 int32, 3 int64)", src_type);
  MSAM2_REQUIRE(prep_sizes_ok(T, H0, W0, S), "label_resize: bad sizes (T %lld of 1 .. %d, H0 x W0 %lldx%lld and S %lld of 1 .. %d)", (long long)T,
                LABEL_MAX_SLICES, (long long)H0, (long long)W0, (long long)S, LABEL_MAX_SIDE);
  LabelResizeParams P = {};
  P.src = src, P.T = (int)T, P.H0 = (int)H0, P.W0 = (int)W0, P.S = (int)S, P.ymap = ymap, P.xmap = xmap, P.out = out;
  for (int i = 0; i < 8; ++i) P.keep[i] = keep8 ? keep8[i] : 0xffffffffu;
  P.vec = S % 16 == 0 && vec_ok(16, 1, (const void*)out);
  const dim3 grid((unsigned)cdiv(S * cdiv(S, 16), PREP_THREADS), (unsigned)T), block(PREP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (src_type == LAB_U8) hipLaunchKernelGGL(label_resize_kernel<uint8_t>, grid, block, 0, s, P);
  else if (src_type == LAB_I16) hipLaunchKernelGGL(label_resize_kernel<int16_t>, grid, block, 0, s, P);
  else if (src_type == LAB_I32) hipLaunchKernelGGL(label_resize_kernel<int32_t>, grid, block, 0, s, P);
  else hipLaunchKernelGGL(label_resize_kernel<int64_t>, grid, block, 0, s, P);
  return msam2_check_launch("label_resize");
}
