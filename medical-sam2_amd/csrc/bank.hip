// The self-sorting 2-D memory bank of Medical-SAM2 (func_2d/function.py:87-116 draw, 205-243 replacement) on the device, gfx950.
// fp32 throughout; nothing here depends on the 16-bit operand type, so both library builds hold the same code.
//
// A bank operand is a set of rows, each a [n_ch, n_px] map in the LOGICAL flat order i = ch * n_px + px, given as a base pointer and
// element strides {row, channel, pixel}: a token-major nchw_view (channel stride 1) and a contiguous row (pixel stride 1) are both
// read in place.  Device tables (capacity BANK_MAX = 32 physical slots): the raw Gram matrix of the stored memory features
// [32][32] (its diagonal holds the squared norms), the IoU of every slot [32] and `order` [32], logical position -> physical slot.
// The live slots are always 0 .. N-1: a replacement re-uses the slot of the entry it pops, only `order` shifts.
#include "common.h"

namespace {

constexpr int BANK_MAX = 32;          // physical slots the tables are laid out for (rows of Y, table stride)
constexpr int BANK_MAX_R = 8;         // rows of X (candidates / images of a step)
constexpr int DOTS_THREADS = 256;
constexpr int DOTS_MAX_WG = 512;      // K split: two 256-thread workgroups per CU on 256 CUs
constexpr int DOTS_RT = 4;            // X rows per workgroup (blockIdx.y tiles R)

struct BankOperand {
  const float* p;
  int64_t rs, os, is;                 // element strides: row, outer, inner (the inner one is 1 on the vector paths)
};

// ---- bank_dots ------------------------------------------------------------------------------------------------------------------------
// Out[r][c] = sum_i X[r][i] Y[c][i], xx[r] = sum_i X[r][i]^2, yy[c] = sum_i Y[c][i]^2 in one pass over the operands.
// The K = n_outer * n_inner elements are cut into groups of V consecutive inner elements (V = 4: one global_load_dwordx4 per row and
// group); workgroup p owns `its` consecutive blocks of 256 groups, thread t group (p * its + k) * 256 + t.  A thread loads its X
// group once (4 rows: blockIdx.y tiles R) and multiplies it against every Y row, so X is read once per workgroup and Y once per
// R-tile (once for R <= 4).  Y rows c < Ca come from Ya, the others from Yb (candidates that are not in the bank's storage yet).
// Each value is then summed over the wave (xor butterfly), over the 4 waves in wave order, and written to ws[p][value]; the
// second kernel sums the P partials.  No atomics: the order of every addition is fixed by (K, V), the result is bit-reproducible.
//
// Error bound: |computed - exact| <= gamma_n sum_i |x_i y_i| with
//   n = its * V        (the thread's sequential fma chain)
//     + 6 + 3          (wave butterfly, 4 waves)
//     + ceil(P / 64) - 1 + 6   (second kernel: a lane's sequential partials, wave butterfly)
// which msam2_bank_dots_chain returns for a given (K, V).
template <int V>
struct Vec;
template <>
struct Vec<4> {
  float4 v;
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ float dot(const Vec& o, float a) const {
    a = fmaf(v.x, o.v.x, a);
    a = fmaf(v.y, o.v.y, a);
    a = fmaf(v.z, o.v.z, a);
    return fmaf(v.w, o.v.w, a);
  }
};
template <>
struct Vec<1> {
  float v;
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ float dot(const Vec& o, float a) const { return fmaf(v, o.v, a); }
};

template <int V, int CT>
__global__ __launch_bounds__(DOTS_THREADS) void bank_dots_kernel(BankOperand X, BankOperand Ya, BankOperand Yb, int R, int Ca, int Cn, int64_t G,
                                                                 int gi, int its, float* __restrict__ ws, int NV) {
  const int r0 = blockIdx.y * DOTS_RT;
  const int nr = min(DOTS_RT, R - r0);
  const bool do_yy = blockIdx.y == 0;
  float acc[DOTS_RT][CT], xx[DOTS_RT], yy[CT];
#pragma unroll
  for (int r = 0; r < DOTS_RT; ++r) {
    xx[r] = 0.f;
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[r][c] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) yy[c] = 0.f;

  for (int k = 0; k < its; ++k) {
    const int64_t g = ((int64_t)blockIdx.x * its + k) * DOTS_THREADS + threadIdx.x;
    if (g >= G) continue;
    const int64_t o = g / gi;
    const int64_t iv = (g - o * gi) * V;
    Vec<V> xv[DOTS_RT];
#pragma unroll
    for (int r = 0; r < DOTS_RT; ++r) {
      if (r < nr) {
        xv[r].load(X.p + (r0 + r) * X.rs + o * X.os + iv * X.is);
        xx[r] = xv[r].dot(xv[r], xx[r]);
      }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      if (c < Cn) {
        Vec<V> yv;
        if (c < Ca)
          yv.load(Ya.p + c * Ya.rs + o * Ya.os + iv * Ya.is);
        else
          yv.load(Yb.p + (c - Ca) * Yb.rs + o * Yb.os + iv * Yb.is);
        if (do_yy) yy[c] = yv.dot(yv, yy[c]);
#pragma unroll
        for (int r = 0; r < DOTS_RT; ++r)
          if (r < nr) acc[r][c] = xv[r].dot(yv, acc[r][c]);
      }
    }
  }

  constexpr int SLOTS = DOTS_RT * CT + DOTS_RT + CT;
  __shared__ float red[DOTS_THREADS / 64][SLOTS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < DOTS_RT; ++r) {
    if (r < nr) {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < Cn) {
          const float s = wave_sum(acc[r][c]);
          if (lane == 0) red[wv][r * CT + c] = s;
        }
      }
      const float s = wave_sum(xx[r]);
      if (lane == 0) red[wv][DOTS_RT * CT + r] = s;
    }
  }
  if (do_yy) {
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      if (c < Cn) {
        const float s = wave_sum(yy[c]);
        if (lane == 0) red[wv][DOTS_RT * CT + DOTS_RT + c] = s;
      }
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < SLOTS) {
    int out = -1;
    if (t < DOTS_RT * CT) {
      const int r = t / CT, c = t - r * CT;
      if (r < nr && c < Cn) out = (r0 + r) * Cn + c;
    } else if (t < DOTS_RT * CT + DOTS_RT) {
      const int r = t - DOTS_RT * CT;
      if (r < nr) out = R * Cn + r0 + r;
    } else {
      const int c = t - DOTS_RT * CT - DOTS_RT;
      if (do_yy && c < Cn) out = R * Cn + R + c;
    }
    if (out >= 0) ws[(int64_t)blockIdx.x * NV + out] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  }
}

// one wave per value: lane l adds partials l, l + 64, ... in that order, then the butterfly
__global__ __launch_bounds__(64) void bank_dots_reduce_kernel(const float* __restrict__ ws, int P, int NV, int R, int Cn, float* __restrict__ dots,
                                                              float* __restrict__ xx, float* __restrict__ yy) {
  const int o = blockIdx.x;
  float s = 0.f;
  for (int p = threadIdx.x; p < P; p += 64) s += ws[(int64_t)p * NV + o];
  s = wave_sum(s);
  if (threadIdx.x != 0) return;
  if (o < R * Cn)
    dots[o] = s;
  else if (o < R * Cn + R) {
    if (xx) xx[o - R * Cn] = s;
  } else if (yy)
    yy[o - R * Cn - R] = s;
}

struct DotsPlan {
  int V, P, its;
  int64_t G;
};
DotsPlan dots_plan(int64_t K, int V) {
  DotsPlan d;
  d.V = V;
  d.G = K / V;
  const int64_t blocks = (d.G + DOTS_THREADS - 1) / DOTS_THREADS;   // (64-bit: msam2_bank_dots_chain takes any K)
  const int64_t p0 = blocks < DOTS_MAX_WG ? blocks : DOTS_MAX_WG;
  d.its = (int)((blocks + p0 - 1) / p0);
  d.P = (int)((blocks + d.its - 1) / d.its);
  return d;
}

bool aligned4(const float* p, const int64_t* st, int fast) {
  if ((uintptr_t)p & 15) return false;
  for (int k = 0; k < 3; ++k)
    if (k != fast && (st[k] & 3)) return false;
  return st[fast] == 1;
}

template <int V>
void dots_launch(int CT, dim3 grid, hipStream_t s, BankOperand X, BankOperand Ya, BankOperand Yb, int R, int Ca, int Cn, int64_t G, int gi, int its,
                 float* ws, int NV) {
  switch (CT) {
    case 8: hipLaunchKernelGGL((bank_dots_kernel<V, 8>), grid, dim3(DOTS_THREADS), 0, s, X, Ya, Yb, R, Ca, Cn, G, gi, its, ws, NV); break;
    case 16: hipLaunchKernelGGL((bank_dots_kernel<V, 16>), grid, dim3(DOTS_THREADS), 0, s, X, Ya, Yb, R, Ca, Cn, G, gi, its, ws, NV); break;
    case 24: hipLaunchKernelGGL((bank_dots_kernel<V, 24>), grid, dim3(DOTS_THREADS), 0, s, X, Ya, Yb, R, Ca, Cn, G, gi, its, ws, NV); break;
    default: hipLaunchKernelGGL((bank_dots_kernel<V, 32>), grid, dim3(DOTS_THREADS), 0, s, X, Ya, Yb, R, Ca, Cn, G, gi, its, ws, NV); break;
  }
}

// ---- bank_sample ----------------------------------------------------------------------------------------------------------------------
// cos[b][n] = dots[b][order[n]] / (max(|x_b|, eps) max(|y_order[n]|, eps)) (F.normalize's clamp), row softmax over the N live entries in
// logical order, inclusive CDF, idx[b][s] = first n with u[b][s] < cdf[b][n] (N - 1 when rounding leaves the last edge below u).
__global__ __launch_bounds__(64) void bank_sample_kernel(const float* __restrict__ dots, int ld, const float* __restrict__ xx,
                                                         const float* __restrict__ yy, const int* __restrict__ order, int N, int cap,
                                                         const float* __restrict__ u, int B, int S, int* __restrict__ indices,
                                                         float* __restrict__ probs) {
  __shared__ float cdf[BANK_MAX_R][BANK_MAX];
  const float eps = 1e-12f;
  const int t = threadIdx.x;
  if (t < B) {
    const float nx = fmaxf(sqrtf(xx[t]), eps);
    float c[BANK_MAX];
    float m = -INFINITY;
    for (int n = 0; n < N; ++n) {
      const int s = min(max(order[n], 0), cap - 1);
      c[n] = dots[t * ld + s] / (nx * fmaxf(sqrtf(yy[s]), eps));
      m = fmaxf(m, c[n]);
    }
    float sum = 0.f;
    for (int n = 0; n < N; ++n) {
      c[n] = expf(c[n] - m);
      sum += c[n];
    }
    float run = 0.f;
    for (int n = 0; n < N; ++n) {
      const float p = c[n] / sum;
      run += p;
      cdf[t][n] = run;
      if (probs) probs[t * N + n] = p;
    }
  }
  __syncthreads();
  for (int q = t; q < B * S; q += 64) {
    const int b = q / S;
    const float uu = u[q];
    int idx = N - 1;
    for (int n = N - 1; n >= 0; --n)
      if (uu < cdf[b][n]) idx = n;
    indices[q] = idx;
  }
}

// ---- bank_gather ----------------------------------------------------------------------------------------------------------------------
// memory[(s * HW + p), b, :] = feats[order[idx[b][s]]][p][:] (and the same for pos): the slots are stored token-major [HW, C], so every
// (s, p, b) moves one C-float run; a thread moves 16 bytes.
__global__ __launch_bounds__(256) void bank_gather_kernel(const float4* __restrict__ feats, const float4* __restrict__ pos, int64_t slot4,
                                                          const int* __restrict__ order, const int* __restrict__ indices, int B, int S, int HW,
                                                          int C4, int N, int cap, float4* __restrict__ memory, float4* __restrict__ memory_pos) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)S * HW * B * C4;
  if (i >= total) return;
  const int c = (int)(i % C4);
  const int64_t q = i / C4;
  const int b = (int)(q % B);
  const int64_t sp = q / B;
  const int p = (int)(sp % HW), s = (int)(sp / HW);
  const int idx = min(max(indices[b * S + s], 0), N - 1);
  const int slot = min(max(order[idx], 0), cap - 1);
  const int64_t src = slot * slot4 + (int64_t)p * C4 + c;
  memory[i] = feats[src];
  memory_pos[i] = pos[src];
}

// ---- bank_decide ----------------------------------------------------------------------------------------------------------------------
// One wave runs the sequential loop of function.py:213-243 over the B candidates of a step.  D [B, N + B]: raw dots of the candidates
// against the physical slots 0 .. N-1 as they were before the step, then against each other.  A slot replaced earlier in the same step
// is looked up through who[slot] (the candidate now stored there), so nothing is recomputed.  fill != 0: function.py:205-210, every
// candidate is appended (slot N, N + 1, ...).
__global__ __launch_bounds__(64) void bank_decide_kernel(float* __restrict__ gram, float* __restrict__ iou_bank, int* __restrict__ order, int N0,
                                                         const float* __restrict__ D, const float* __restrict__ iou_pred, int B, int M, int fill,
                                                         int* __restrict__ accept, int* __restrict__ slot_cand, float* __restrict__ iou_out) {
  __shared__ float g[BANK_MAX][BANK_MAX + 1];
  __shared__ float nrm[BANK_MAX], ious[BANK_MAX], val[BANK_MAX];
  __shared__ int ord[BANK_MAX], who[BANK_MAX];
  const float eps = 1e-12f;
  const int t = threadIdx.x;
  const int ld = N0 + B;
  for (int e = t; e < BANK_MAX * BANK_MAX; e += 64) g[e / BANK_MAX][e % BANK_MAX] = gram[e];
  if (t < BANK_MAX) {
    nrm[t] = fmaxf(sqrtf(gram[t * BANK_MAX + t]), eps);
    ious[t] = iou_bank[t];
    ord[t] = order[t];
    who[t] = -1;
  }
  // the reference's scalar: mean over the batch of the best prediction of each element (every lane computes it, in this order)
  float iou = 0.f;
  for (int b = 0; b < B; ++b) {
    float m = iou_pred[b * M];
    for (int k = 1; k < M; ++k) m = fmaxf(m, iou_pred[b * M + k]);
    iou += m;
  }
  iou = iou / (float)B;
  __syncthreads();
  int N = N0;
  for (int b = 0; b < B; ++b) {
    const float self = D[b * ld + N0 + b];
    const float cn = fmaxf(sqrtf(self), eps);
    bool acc = false;
    int slot = -1;
    if (fill) {
      acc = true;
      slot = N;
      if (t == 0) ord[N] = slot;
      ++N;
    } else if (N >= 2) {
      if (t < N) {
        const int s = ord[t];
        const float d = who[s] < 0 ? D[b * ld + s] : D[b * ld + N0 + who[s]];
        val[t] = d / (cn * nrm[s]);
      }
      __syncthreads();
      int i = 0;
      for (int n = 1; n < N; ++n)
        if (val[n] < val[i]) i = n;
      const float cmin = val[i];
      __syncthreads();
      if (t < N) val[t] = t == i ? -INFINITY : g[ord[i]][ord[t]] / (nrm[ord[i]] * nrm[ord[t]]);
      __syncthreads();
      int j = i == 0 ? 1 : 0;
      for (int n = 0; n < N; ++n)
        if (n != i && val[n] > val[j]) j = n;
      acc = cmin < val[j] && iou > ious[ord[j]] - 0.1f;
      slot = ord[j];
      int nxt = 0;
      if (acc && t >= j && t < N - 1) nxt = ord[t + 1];
      __syncthreads();
      if (acc) {
        if (t >= j && t < N - 1) ord[t] = nxt;
        if (t == 0) ord[N - 1] = slot;
      }
    }
    __syncthreads();
    if (acc) {
      if (t < N && t != slot) {
        const float d = who[t] < 0 ? D[b * ld + t] : D[b * ld + N0 + who[t]];
        g[slot][t] = d;
        g[t][slot] = d;
      }
      __syncthreads();
      if (t == 0) {
        g[slot][slot] = self;
        nrm[slot] = cn;
        ious[slot] = iou;
        who[slot] = b;
      }
    }
    if (t == 0) accept[b] = acc ? 1 : 0;
    __syncthreads();
  }
  for (int e = t; e < BANK_MAX * BANK_MAX; e += 64) gram[e] = g[e / BANK_MAX][e % BANK_MAX];
  if (t < BANK_MAX) {
    iou_bank[t] = ious[t];
    order[t] = ord[t];
    slot_cand[t] = who[t];
  }
  if (t == 0 && iou_out) iou_out[0] = iou;
}

// ---- bank_commit ----------------------------------------------------------------------------------------------------------------------
// A 32 x 32 (channel, pixel) tile through LDS so that both the strided read and the strided write run along their unit-stride side.
__device__ __forceinline__ void copy_tile(const float* __restrict__ src, int64_t scs, int64_t sps, float* __restrict__ dst, int64_t dcs,
                                          int64_t dps, int n_ch, int n_px, int tile, float (*tl)[33]) {
  const int tpx = (n_px + 31) / 32;
  const int c0 = (tile / tpx) * 32, p0 = (tile % tpx) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const bool rd_ch = scs <= sps, wr_ch = dcs <= dps;
  for (int k = ty; k < 32; k += 8) {
    const int dc = rd_ch ? tx : k, dp = rd_ch ? k : tx;
    if (c0 + dc < n_ch && p0 + dp < n_px) tl[dc][dp] = src[(c0 + dc) * scs + (p0 + dp) * sps];
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int dc = wr_ch ? tx : k, dp = wr_ch ? k : tx;
    if (c0 + dc < n_ch && p0 + dp < n_px) dst[(c0 + dc) * dcs + (p0 + dp) * dps] = tl[dc][dp];
  }
}

// blockIdx.y = physical slot; slots the step's decide pass named no candidate for exit.  Features and position encoding are stored
// token-major [HW, C] (what bank_gather copies from), the image embedding in (channel, pixel) flat order [Ce * HW].
__global__ __launch_bounds__(256) void bank_commit_kernel(const int* __restrict__ slot_cand, BankOperand F, BankOperand Pp, int C, BankOperand E,
                                                          int Ce, int HW, int B, float* __restrict__ feats, float* __restrict__ pos,
                                                          float* __restrict__ embed) {
  __shared__ float tl[32][33];
  const int slot = blockIdx.y;
  const int b = slot_cand[slot];
  if (b < 0 || b >= B) return;
  const int tpx = (HW + 31) / 32;
  const int tiles_f = ((C + 31) / 32) * tpx, tiles_e = ((Ce + 31) / 32) * tpx;
  int tile = blockIdx.x;
  if (tile < tiles_f) {
    copy_tile(F.p + b * F.rs, F.os, F.is, feats + (int64_t)slot * HW * C, 1, C, C, HW, tile, tl);
  } else if (tile < 2 * tiles_f) {
    copy_tile(Pp.p + b * Pp.rs, Pp.os, Pp.is, pos + (int64_t)slot * HW * C, 1, C, C, HW, tile - tiles_f, tl);
  } else if (tile < 2 * tiles_f + tiles_e) {
    copy_tile(E.p + b * E.rs, E.os, E.is, embed + (int64_t)slot * HW * Ce, HW, 1, Ce, HW, tile - 2 * tiles_f, tl);
  }
}

BankOperand operand(const float* p, const int64_t* st) {
  BankOperand o;
  o.p = p;
  o.rs = st[0];
  o.os = st[1];
  o.is = st[2];
  return o;
}

bool strides_ok(const int64_t* st) { return st && st[0] >= 0 && st[1] >= 0 && st[2] >= 0; }

}  // namespace

extern "C" int msam2_bank_dots_chain(int64_t K, int vec) {
  if (K <= 0 || (vec != 1 && vec != 4) || K % vec) return -1;
  const DotsPlan d = dots_plan(K, vec);
  return d.its * vec + 6 + 3 + (cdiv(d.P, 64) - 1) + 6;
}

extern "C" size_t msam2_bank_dots_workspace_bytes(int64_t R, int64_t Cn) {
  if (R <= 0 || Cn <= 0) return 0;
  return (size_t)DOTS_MAX_WG * (size_t)(R * Cn + R + Cn) * sizeof(float);
}

extern "C" int msam2_bank_dots(const float* x, const int64_t* x_strides, int64_t R, const float* ya, const int64_t* ya_strides, int64_t rows_a,
                               const float* yb, const int64_t* yb_strides, int64_t rows_b, int64_t n_ch, int64_t n_px, float* dots, float* xx,
                               float* yy, void* workspace, size_t workspace_bytes, void* stream) {
  const int64_t Cn = rows_a + rows_b;
  MSAM2_REQUIRE(R >= 1 && R <= BANK_MAX_R, "bank_dots: R = %lld rows of X (1 .. %d)", (long long)R, BANK_MAX_R);
  MSAM2_REQUIRE(rows_a >= 0 && rows_b >= 0 && Cn >= 1 && Cn <= BANK_MAX, "bank_dots: %lld + %lld rows of Y (1 .. %d in all)", (long long)rows_a,
                (long long)rows_b, BANK_MAX);
  MSAM2_REQUIRE(n_ch >= 1 && n_px >= 1 && n_ch < (1ll << 31) && n_px < (1ll << 31) && n_ch * n_px < (1ll << 31),
                "bank_dots: bad row shape (%lld channels x %lld pixels)", (long long)n_ch, (long long)n_px);
  MSAM2_REQUIRE(x && dots && workspace && (rows_a == 0 || ya) && (rows_b == 0 || yb), "bank_dots: null tensor");
  MSAM2_REQUIRE(strides_ok(x_strides) && (rows_a == 0 || strides_ok(ya_strides)) && (rows_b == 0 || strides_ok(yb_strides)),
                "bank_dots: strides {row, channel, pixel} must be given and >= 0");
  MSAM2_REQUIRE(workspace_bytes >= msam2_bank_dots_workspace_bytes(R, Cn) && ((uintptr_t)workspace & 3) == 0, "bank_dots: workspace too small");
  const int64_t* sa = rows_a ? ya_strides : yb_strides;
  const int64_t* sb = rows_b ? yb_strides : sa;
  const float* pa = rows_a ? ya : yb;
  const float* pb = rows_b ? yb : pa;
  // vector path along the pixels (fast = 2) or along the channels (fast = 1) when every operand is unit-stride and 16-byte aligned there
  int fast = 0;
  if (n_px % 4 == 0 && aligned4(x, x_strides, 2) && aligned4(pa, sa, 2) && aligned4(pb, sb, 2))
    fast = 2;
  else if (n_ch % 4 == 0 && aligned4(x, x_strides, 1) && aligned4(pa, sa, 1) && aligned4(pb, sb, 1))
    fast = 1;
  const int inner = fast == 1 ? 1 : 2, outer = fast == 1 ? 2 : 1;
  auto mk = [&](const float* p, const int64_t* st) {
    BankOperand o;
    o.p = p;
    o.rs = st[0];
    o.os = st[outer];
    o.is = st[inner];
    return o;
  };
  const int64_t K = n_ch * n_px;
  const int V = fast ? 4 : 1;
  const DotsPlan d = dots_plan(K, V);
  const int gi = (int)((fast == 1 ? n_ch : n_px) / V);
  const int NV = (int)(R * Cn + R + Cn);
  const int CT = Cn <= 8 ? 8 : Cn <= 16 ? 16 : Cn <= 24 ? 24 : 32;
  const dim3 grid((unsigned)d.P, (unsigned)cdiv(R, DOTS_RT));
  hipStream_t s = (hipStream_t)stream;
  if (V == 4)
    dots_launch<4>(CT, grid, s, mk(x, x_strides), mk(pa, sa), mk(pb, sb), (int)R, (int)rows_a, (int)Cn, d.G, gi, d.its, (float*)workspace, NV);
  else
    dots_launch<1>(CT, grid, s, mk(x, x_strides), mk(pa, sa), mk(pb, sb), (int)R, (int)rows_a, (int)Cn, d.G, gi, d.its, (float*)workspace, NV);
  hipLaunchKernelGGL(bank_dots_reduce_kernel, dim3((unsigned)NV), dim3(64), 0, s, (const float*)workspace, d.P, NV, (int)R, (int)Cn, dots, xx, yy);
  return msam2_check_launch("bank_dots");
}

extern "C" int msam2_bank_sample(const float* dots, int64_t ld, const float* xx, const float* yy, const int* order, int64_t N, int64_t cap,
                                 const float* u, int64_t B, int64_t S, int* indices, float* probs, void* stream) {
  MSAM2_REQUIRE(B >= 1 && B <= BANK_MAX_R && S >= 1 && S <= 64, "bank_sample: B = %lld images (1 .. %d), S = %lld draws (1 .. 64)", (long long)B,
                BANK_MAX_R, (long long)S);
  MSAM2_REQUIRE(N >= 1 && N <= cap && cap <= BANK_MAX && ld >= cap, "bank_sample: N = %lld live entries, capacity %lld (<= %d), row stride %lld",
                (long long)N, (long long)cap, BANK_MAX, (long long)ld);
  MSAM2_REQUIRE(dots && xx && yy && order && u && indices, "bank_sample: null tensor");
  hipLaunchKernelGGL(bank_sample_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dots, (int)ld, xx, yy, order, (int)N, (int)cap, u, (int)B, (int)S,
                     indices, probs);
  return msam2_check_launch("bank_sample");
}

extern "C" int msam2_bank_gather(const float* feats, const float* pos, const int* order, const int* indices, int64_t B, int64_t S, int64_t HW,
                                 int64_t C, int64_t N, int64_t cap, float* memory, float* memory_pos, void* stream) {
  MSAM2_REQUIRE(B >= 1 && B <= BANK_MAX_R && S >= 1 && S <= 64 && HW >= 1 && C >= 4 && C % 4 == 0 && S * HW * B * C < (1ll << 40),
                "bank_gather: bad sizes (B %lld, S %lld, HW %lld, C %lld: C must be a multiple of 4)", (long long)B, (long long)S, (long long)HW,
                (long long)C);
  MSAM2_REQUIRE(N >= 1 && N <= cap && cap <= BANK_MAX, "bank_gather: N = %lld live entries, capacity %lld (<= %d)", (long long)N, (long long)cap,
                BANK_MAX);
  MSAM2_REQUIRE(feats && pos && order && indices && memory && memory_pos, "bank_gather: null tensor");
  MSAM2_REQUIRE((((uintptr_t)feats | (uintptr_t)pos | (uintptr_t)memory | (uintptr_t)memory_pos) & 15) == 0, "bank_gather: tensors must be 16-byte aligned");
  const int64_t total = S * HW * B * (C / 4);
  hipLaunchKernelGGL(bank_gather_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)feats,
                     (const float4*)pos, HW * C / 4, order, indices, (int)B, (int)S, (int)HW, (int)(C / 4), (int)N, (int)cap, (float4*)memory,
                     (float4*)memory_pos);
  return msam2_check_launch("bank_gather");
}

extern "C" int msam2_bank_decide(float* gram, float* iou_bank, int* order, int64_t N, int64_t cap, const float* dots, const float* iou_pred, int64_t B,
                                 int64_t M, int fill, int* accept, int* slot_cand, float* iou_out, void* stream) {
  MSAM2_REQUIRE(B >= 1 && B <= BANK_MAX_R && M >= 1, "bank_decide: B = %lld candidates (1 .. %d), M = %lld predictions each", (long long)B, BANK_MAX_R,
                (long long)M);
  MSAM2_REQUIRE(N >= 0 && cap <= BANK_MAX && N + (fill ? B : 0) <= cap, "bank_decide: N = %lld live entries%s exceed the capacity %lld (<= %d)",
                (long long)N, fill ? " plus the appended batch" : "", (long long)cap, BANK_MAX);
  MSAM2_REQUIRE(gram && iou_bank && order && dots && iou_pred && accept && slot_cand, "bank_decide: null tensor");
  hipLaunchKernelGGL(bank_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gram, iou_bank, order, (int)N, dots, iou_pred, (int)B, (int)M, fill,
                     accept, slot_cand, iou_out);
  return msam2_check_launch("bank_decide");
}

extern "C" int msam2_bank_commit(const int* slot_cand, int64_t cap, const float* feats, const int64_t* feats_strides, const float* pos,
                                 const int64_t* pos_strides, int64_t C, const float* embed, const int64_t* embed_strides, int64_t Ce, int64_t HW,
                                 int64_t B, float* feats_store, float* pos_store, float* embed_store, void* stream) {
  MSAM2_REQUIRE(B >= 1 && B <= BANK_MAX_R && cap >= 1 && cap <= BANK_MAX, "bank_commit: B = %lld candidates (1 .. %d), capacity %lld (1 .. %d)",
                (long long)B, BANK_MAX_R, (long long)cap, BANK_MAX);
  MSAM2_REQUIRE(C >= 1 && Ce >= 1 && HW >= 1 && C * HW < (1ll << 31) && Ce * HW < (1ll << 31), "bank_commit: bad sizes (C %lld, Ce %lld, HW %lld)",
                (long long)C, (long long)Ce, (long long)HW);
  MSAM2_REQUIRE(slot_cand && feats && pos && embed && feats_store && pos_store && embed_store, "bank_commit: null tensor");
  MSAM2_REQUIRE(strides_ok(feats_strides) && strides_ok(pos_strides) && strides_ok(embed_strides),
                "bank_commit: strides {row, channel, pixel} must be given and >= 0");
  const int64_t tpx = (HW + 31) / 32;
  const int64_t tiles = 2 * ((C + 31) / 32) * tpx + ((Ce + 31) / 32) * tpx;
  hipLaunchKernelGGL(bank_commit_kernel, dim3((unsigned)tiles, (unsigned)cap), dim3(256), 0, (hipStream_t)stream, slot_cand, operand(feats, feats_strides),
                     operand(pos, pos_strides), (int)C, operand(embed, embed_strides), (int)Ce, (int)HW, (int)B, feats_store, pos_store, embed_store);
  return msam2_check_launch("bank_commit");
}
