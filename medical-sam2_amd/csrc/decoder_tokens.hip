// Token side of the two-way decoder (transformer.py:121-196, 74-118) as block kernels.  The B * T <= 32 token rows of width 256 went
// through 11 launches per two-way block and 3 behind the final attention (gemm_tokens, attention_small, gemm, layernorm), each at the
// launch floor of 4.4 - 7.5 us for a few KB of activations; here a block takes three launches and the tail one:
//   dec_self_kernel    q | k | v, the token self-attention, out-projection (+ residual), norm1 and the tokens -> image query projection:
//                      one workgroup per image
//   dec_mlp_kernel     tokens -> image out-projection + residual, norm2, fc1 + ReLU and fc2 for ONE 128-wide slice of the 2048 hidden units:
//                      grid (16 slices, images); every workgroup repeats the cheap out-projection + norm2 of its image and writes its fp32
//                      fc2 partial to the call's workspace -- one workgroup cannot stream the 2 MB of fc1 / fc2
//   dec_kv_kernel      sum of the 16 partials IN SLICE ORDER (no atomics: same bits on every run) + bias + residual, norm3, the image -> token
//                      k | v projection and, behind the last block, the final attention's query projection: one workgroup per image
//   dec_tail_kernel    final attention out-projection + residual + norm_final_attn
// No workgroup waits for another and nothing is shared between calls: the partials live in a caller-owned workspace.
// Rounding points are those of the launches this replaces: operands rounded to 16 bits at the load (a + addend first), q | k | v, the
// attention output and the ReLU hidden map rounded to 16 bits, out-projections, residuals and LayerNorm in fp32, the softmax as in
// attn_small_kernel (fp32, scores in the log2 domain, probabilities never rounded).  Only the order of fp32 sums differs.
#include "common.h"

constexpr int DT_C = 256;        // token width
constexpr int DT_H = 8;          // heads
constexpr int DT_CI = 128;       // internal width of the cross attentions
constexpr int DT_HID = 2048;     // hidden units of the MLP
constexpr int DT_SLICE = 128;    // hidden units per dec_mlp_kernel workgroup
constexpr int DT_NSLICE = DT_HID / DT_SLICE;
constexpr int DT_MAXT = 16;      // token rows per image (one half of a 32-row MFMA tile)
constexpr int DT_MAXR = 32;      // token rows per call
constexpr int DT_THREADS = 512, DT_WAVES = DT_THREADS / 64;
constexpr int DT_PART = 8192;    // floats of the k-split partial buffer: KP * 16 * N of every GEMM below

constexpr int lds_ld(int K) { return K + 8; }        // 16-bit operand rows in LDS: 16 bytes of padding (conflict-free ds_read_b128)

// part[kp][row < 16][n] (fp32, LDS) = A[row][k-part kp] . W[n][k-part kp] for the 16 token rows of an image: A 16-bit in LDS (row stride
// lds_ld(K); tiles of columns >= split_col read a_hi, e.g. the v third of q | k | v, which sees no position encoding), W 16-bit in global
// memory ([N, K], row stride ldw).  Unit = (32-column tile, k-part); units go round the waves.  load() issues EVERY W fragment of the wave's
// units straight from global memory (gemm_skinny_kernel's scheme) and is called a phase ahead of mma(), in front of the barrier and the
// LDS work that produce A: a kernel is a chain of five to nine such phases, and with the loads inside the phases each one paid a full
// memory latency of its own (32 us for dec_self_kernel against the 31 us of the five launches it replaces; 3.10).  Rows 16 .. 31 of the
// MFMA tile repeat rows 0 .. 15 and are dropped.  KP == 1: no partial buffer, epi(unit of the wave, row, col, value) takes the sums.
template <int N, int K, int KP>
struct TokGemm {
  static_assert(N % 32 == 0 && K % (16 * KP) == 0 && (KP == 1 || KP * 16 * N <= DT_PART), "TokGemm shape");
  static constexpr int KS = K / 16 / KP, NU = (N / 32) * KP, UPW = (NU + DT_WAVES - 1) / DT_WAVES, LDA = lds_ld(K);
  op16x8 w[UPW][KS];
  // unit j of this wave (clamped to a unit that exists: its loads are valid, its products are not used)
  __device__ __forceinline__ static int unit(int j) { return min((int)(threadIdx.x >> 6) + j * DT_WAVES, NU - 1); }
  __device__ __forceinline__ void load(const op16* __restrict__ W, int ldw) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int j = 0; j < UPW; ++j) {
      const int u = unit(j), tile = u / KP, kp = u - tile * KP;
      const op16* wp = W + (int64_t)(tile * 32 + r) * ldw + kp * KS * 16 + h * 8;
#pragma unroll
      for (int s = 0; s < KS; ++s) w[j][s] = *reinterpret_cast<const op16x8*>(wp + s * 16);
    }
  }
  template <typename Epi>
  __device__ __forceinline__ void mma(const op16* a_lo, const op16* a_hi, int split_col, float* part, Epi&& epi) const {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int j = 0; j < UPW; ++j) {
      if (wave + j * DT_WAVES >= NU) break;                    // (wave-uniform)
      const int u = wave + j * DT_WAVES, tile = u / KP, kp = u - tile * KP, n0 = tile * 32;
      const op16* ap = (n0 < split_col ? a_lo : a_hi) + (r & 15) * LDA + kp * KS * 16 + h * 8;
      // KP == 1: the reduction runs as four quarter sums added in order, in registers -- the order gemm_skinny_kernel's four waves and its
      // part[0] + part[1] + part[2] + part[3] give, so these GEMMs keep the bits of the launches they replace.  KP == 4 is that order too.
      constexpr int NQ = (KP == 1 && KS % 4 == 0) ? 4 : 1;
      f32x16 acc[NQ];
#pragma unroll
      for (int qd = 0; qd < NQ; ++qd)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[qd][e] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s)
        acc[s / (KS / NQ)] = MSAM2_MFMA_32x32x16(*reinterpret_cast<const op16x8*>(ap + s * 16), w[j][s], acc[s / (KS / NQ)], 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * h;        // < 16
        float v = acc[0][e];
#pragma unroll
        for (int qd = 1; qd < NQ; ++qd) v += acc[qd][e];
        if constexpr (KP == 1) epi(j, row, n0 + r, v);
        else part[(kp * 16 + row) * N + n0 + r] = v;
      }
    }
  }
  __device__ __forceinline__ void mma(const op16* a, float* part) const { mma(a, a, 0, part, [](int, int, int, float) {}); }
};

// Rows of one image: sum of NSLAB fp32 slabs in slab order (the k-parts of an out-projection in LDS, or the hidden slices of fc2 in the
// workspace) + bias + residual, then LayerNorm over the 256 channels -- one wave per row (rows wave and wave + 8), lane l owns channels
// 4 l .. 4 l + 3, the two-pass statistics of layernorm_kernel.  What does not depend on the slabs (bias, LayerNorm vectors, the residual
// rows, `extra` rows such as the position encoding the sink adds) is loaded by ln_preload, a phase ahead like the weights.
// sink(row, first channel, 4 values, the row's 4 extra values).
struct LnPre {
  f32x4 bias, w, b, res[2], extra[2];
};
__device__ __forceinline__ LnPre ln_preload(const float* __restrict__ bias, const float* res, const float* extra, const float* __restrict__ lnw,
                                            const float* __restrict__ lnb, int T) {
  const int wave = threadIdx.x >> 6, c = (threadIdx.x & 63) * 4;
  LnPre p;
  p.bias = *reinterpret_cast<const f32x4*>(bias + c);
  p.w = *reinterpret_cast<const f32x4*>(lnw + c);
  p.b = *reinterpret_cast<const f32x4*>(lnb + c);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = min(wave + j * DT_WAVES, T - 1);           // clamped: a valid address, the row is not used
    p.res[j] = res ? *reinterpret_cast<const f32x4*>(res + row * DT_C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    p.extra[j] = extra ? *reinterpret_cast<const f32x4*>(extra + row * DT_C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  return p;
}
template <int NSLAB, typename Sink>
__device__ __forceinline__ void sum_res_ln_rows(const float* slabs, int64_t slab_stride, const LnPre& pre, float eps, int T, Sink&& sink) {
  static_assert(DT_MAXT <= 2 * DT_WAVES, "two rows per wave");
  const int wave = threadIdx.x >> 6, c = (threadIdx.x & 63) * 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = wave + j * DT_WAVES;
    if (row >= T) break;                                       // (wave-uniform)
    f32x4 t[NSLAB];                                            // every slab's load in flight, summed in slab order
#pragma unroll
    for (int s = 0; s < NSLAB; ++s) t[s] = *reinterpret_cast<const f32x4*>(slabs + s * slab_stride + row * DT_C + c);
    f32x4 v = t[0];
#pragma unroll
    for (int s = 1; s < NSLAB; ++s) v += t[s];
    v += pre.bias;
    v += pre.res[j];
    const float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) / DT_C;
    const f32x4 d = v - mean;
    const float var = wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) / DT_C;
    const float rstd = 1.0f / sqrtf(var + eps);
    sink(row, c, d * rstd * pre.w + pre.b, pre.extra[j]);
  }
}

// The piece the three token-side places share: out-projection of the 16-bit attention output a16 [16][K] (LDS) + bias + residual rows +
// LayerNorm; the weight fragments and `pre` were loaded by the caller before the phase that produced a16.  Ends behind a barrier: `part`
// is free again and what the sink wrote to LDS is visible.
template <int K, typename Sink>
__device__ __forceinline__ void proj_res_ln(const TokGemm<DT_C, K, 1>& g, const op16* a16, const LnPre& pre, float eps, int T, float* part,
                                            Sink&& sink) {
  g.mma(a16, a16, 0, nullptr, [&](int, int row, int col, float v) { part[row * DT_C + col] = v; });
  __syncthreads();
  sum_res_ln_rows<1>(part, 0, pre, eps, T, sink);
  __syncthreads();
}

__device__ __forceinline__ op16x4 f2op4(f32x4 v) {
  op16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f2op(v[e]);
  return o;
}

// zero the rows >= T of a 16-row operand image (their products are dropped, but LDS may hold anything)
template <int K>
__device__ __forceinline__ void zero_dead_rows(op16* a, int T) {
  for (int i = threadIdx.x; i < (DT_MAXT - T) * (K / 4); i += DT_THREADS) {
    const int row = T + i / (K / 4), c = (i % (K / 4)) * 4;
    *reinterpret_cast<op16x4*>(a + row * lds_ld(K) + c) = op16x4{0, 0, 0, 0};
  }
}

// 16-bit rows [T][K] from global memory into an operand image
template <int K>
__device__ __forceinline__ void load_rows16(op16* a, const op16* __restrict__ src, int T) {
  for (int i = threadIdx.x; i < T * (K / 8); i += DT_THREADS) {
    const int row = i / (K / 8), c = (i % (K / 8)) * 8;
    *reinterpret_cast<op16x8*>(a + row * lds_ld(K) + c) = *reinterpret_cast<const op16x8*>(src + row * K + c);
  }
}

// The tokens -> image attention's output rows of image b as an operand image: the 16-bit rows o, or (part != null) the key-split partials of
// msam2_attention_fewq_keysplit -- part[((b * 8 + head) * splits + s) * T + row][18] = (max, sum, O[16]), fp32, un-normalised -- merged in
// split order with the formula of attn_fewq16_kernel's own 16-wave merge and rounded to 16 bits where that kernel rounds.  Every split's
// load is issued (index clamped, weight 0 behind the last split): no load sits behind a branch.
__device__ __forceinline__ void load_attn_rows(op16* a_o, const op16* __restrict__ o, const float* __restrict__ part, int splits, int b, int T) {
  constexpr int D = DT_CI / DT_H, MAXSPLITS = 8;
  if (!part) {                                            // (uniform over the launch)
    load_rows16<DT_CI>(a_o, o + (int64_t)b * T * DT_CI, T);
    return;
  }
  for (int i = threadIdx.x; i < T * DT_CI; i += DT_THREADS) {
    const int row = i / DT_CI, c = i % DT_CI, head = c / D, d = c % D;
    const float* base = part + (((int64_t)(b * DT_H + head) * splits) * T + row) * 18;
    float m[MAXSPLITS], l[MAXSPLITS], a[MAXSPLITS];
#pragma unroll
    for (int s = 0; s < MAXSPLITS; ++s) {
      const float* ps = base + (int64_t)min(s, splits - 1) * T * 18;
      m[s] = ps[0];
      l[s] = ps[1];
      a[s] = ps[2 + d];
    }
    float M = -INFINITY;
#pragma unroll
    for (int s = 0; s < MAXSPLITS; ++s) {
      if (s >= splits) m[s] = -INFINITY;
      M = fmaxf(M, m[s]);
    }
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int s = 0; s < MAXSPLITS; ++s) {
      const float wgt = (m[s] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m[s] - M);
      L += l[s] * wgt;
      acc += a[s] * wgt;
    }
    a_o[row * lds_ld(DT_CI) + c] = f2op(acc / L);
  }
}

// out[row][col] (16-bit, global, row stride N) = sum of the KP k-parts in part + bias for the rows < T; a thread's column is the same in
// every trip (DT_THREADS % N == 0), so its bias value `b` was loaded a phase ahead
template <int N, int KP>
__device__ __forceinline__ void store_rows16(op16* out, const float* part, float b, int T) {
  static_assert(DT_THREADS % N == 0, "one column per thread");
  for (int i = threadIdx.x; i < T * N; i += DT_THREADS) {
    const int row = i / N, col = i % N;
    float v = part[row * N + col];
#pragma unroll
    for (int kp = 1; kp < KP; ++kp) v += part[(kp * 16 + row) * N + col];
    out[row * N + col] = f2op(v + b);
  }
}

struct DecSelfParams {
  const float* x;         // queries fp32 [R, 256]
  const float* pe;        // query_pe fp32 [R, 256]
  int skip_pe;            // skip_first_layer_pe: q | k | v see no addend and the out-projection gets no residual
  const op16* wqkv; const float* bqkv;      // [768, 256]
  const op16* wo; const float* bo;          // self_attn.out_proj [256, 256]
  const float* lnw; const float* lnb; float eps;
  const op16* wcq; const float* bcq;        // cross_attn_token_to_image.q_proj [128, 256]
  float* xout;            // queries after norm1
  op16* qp;               // [R, 128]
  int T;
  float scale_log2;
};

__global__ __launch_bounds__(DT_THREADS) void dec_self_kernel(DecSelfParams p) {
  constexpr int LDA = lds_ld(DT_C), LDQ = lds_ld(3 * DT_C);
  __shared__ __attribute__((aligned(16))) op16 a_qk[DT_MAXT * LDA];        // x + pe; later the attention output
  __shared__ __attribute__((aligned(16))) op16 a_v[DT_MAXT * LDA];         // x; later norm1 + pe
  __shared__ __attribute__((aligned(16))) float part[DT_PART];             // q | k | v (16-bit) first, then the k-split partials
  op16* const qkv = reinterpret_cast<op16*>(part);
  static_assert(DT_MAXT * LDQ * 2 <= DT_PART * 4, "q | k | v fit the partial buffer");
  const int T = p.T, tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const float* x = p.x + row0 * DT_C;
  const float* pe = p.pe + row0 * DT_C;
  TokGemm<3 * DT_C, DT_C, 1> gq;
  gq.load(p.wqkv, DT_C);
  float bq[gq.UPW];
#pragma unroll
  for (int j = 0; j < gq.UPW; ++j) bq[j] = p.bqkv[gq.unit(j) * 32 + (tid & 31)];
  for (int i = tid; i < T * (DT_C / 4); i += DT_THREADS) {
    const int row = i / (DT_C / 4), c = (i % (DT_C / 4)) * 4;
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + row * DT_C + c);
    const f32x4 pv = *reinterpret_cast<const f32x4*>(pe + row * DT_C + c);
    *reinterpret_cast<op16x4*>(a_qk + row * LDA + c) = f2op4(p.skip_pe ? xv : xv + pv);
    *reinterpret_cast<op16x4*>(a_v + row * LDA + c) = f2op4(xv);
  }
  zero_dead_rows<DT_C>(a_qk, T);
  zero_dead_rows<DT_C>(a_v, T);
  __syncthreads();
  // q | k | v, 16-bit
  gq.mma(a_qk, a_v, 2 * DT_C, nullptr, [&](int j, int row, int col, float v) { qkv[row * LDQ + col] = f2op(v + bq[j]); });
  // everything the rest of the kernel reads from global memory, in flight under the attention
  TokGemm<DT_C, DT_C, 1> go;
  go.load(p.wo, DT_C);
  TokGemm<DT_CI, DT_C, 4> gc;
  gc.load(p.wcq, DT_C);
  const LnPre pre = ln_preload(p.bo, p.skip_pe ? nullptr : x, pe, p.lnw, p.lnb, T);
  const float bc = p.bcq[tid % DT_CI];
  __syncthreads();
  // self-attention: 16 lanes per (query, head).  Scores: lane = key (attn_small_kernel's dot product: q scaled into the log2 domain, fp32);
  // the group's max and sum by four shuffles each; then lane = channel pair, every key's probability broadcast from its lane.  (The first
  // form merged per-lane (max, sum, O[32]) triples by butterfly as attn_small_kernel does: 136 cross-lane moves per pair against 24.)
  {
    constexpr int D = DT_C / DT_H;
    const int l16 = tid & 15, lane = tid & 63;
    for (int pr = tid >> 4; pr < DT_H * T; pr += DT_THREADS / 16) {          // wave-uniform trip count: DT_H * T is a multiple of 4
      const int head = pr % DT_H, qi = pr / DT_H;
      const bool live = l16 < T;
      const op16* qp = qkv + qi * LDQ + head * D;
      const op16* kp = qkv + (live ? l16 : 0) * LDQ + DT_C + head * D;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < D; d += 8) {
        const op16x8 tq = *reinterpret_cast<const op16x8*>(qp + d);
        const op16x8 tk = *reinterpret_cast<const op16x8*>(kp + d);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (op2f(tq[e]) * p.scale_log2) * op2f(tk[e]);
      }
      float m = live ? s : -INFINITY;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
      const float pk = live ? __builtin_amdgcn_exp2f(s - m) : 0.f;
      float l = pk;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) l += __shfl_xor(l, off, 64);
      const op16* vp = qkv + 2 * DT_C + head * D + 2 * l16;
      float o0 = 0.f, o1 = 0.f;
      for (int key = 0; key < T; ++key) {
        const float pw = __shfl(pk, (lane & 48) | key, 64);
        const op16x2 v2 = *reinterpret_cast<const op16x2*>(vp + key * LDQ);
        o0 += pw * op2f(v2[0]);
        o1 += pw * op2f(v2[1]);
      }
      const float inv = 1.f / l;
      op16x2 o2;
      o2[0] = f2op(o0 * inv);
      o2[1] = f2op(o1 * inv);
      *reinterpret_cast<op16x2*>(a_qk + qi * LDA + head * D + 2 * l16) = o2;  // (x + pe has been consumed)
    }
  }
  __syncthreads();
  // out-projection (+ residual), norm1: the fp32 rows leave, norm1 + pe is the operand of the query projection
  float* xout = p.xout + row0 * DT_C;
  proj_res_ln<DT_C>(go, a_qk, pre, p.eps, T, part, [&](int row, int c, f32x4 y, f32x4 pv) {
    *reinterpret_cast<f32x4*>(xout + row * DT_C + c) = y;
    *reinterpret_cast<op16x4*>(a_v + row * LDA + c) = f2op4(y + pv);
  });
  gc.mma(a_v, part);
  __syncthreads();
  store_rows16<DT_CI, 4>(p.qp + row0 * DT_CI, part, bc, T);
}

struct DecMlpParams {
  const op16* o;          // tokens -> image attention output, 16-bit [R, 128], or
  const float* o_part;    // its key-split partials (load_attn_rows)
  int splits;
  const float* x;         // residual: queries after norm1
  const op16* wo; const float* bo;          // cross_attn_token_to_image.out_proj [256, 128]
  const float* lnw; const float* lnb; float eps;   // norm2
  const op16* w1; const float* b1;          // [2048, 256]
  const op16* w2;                           // [256, 2048]
  float* x2;              // queries after norm2 (fc2's residual), written by slice 0
  float* ws;              // fc2 partials fp32 [16][R][256]
  int T, R;
};

__global__ __launch_bounds__(DT_THREADS) void dec_mlp_kernel(DecMlpParams p) {
  constexpr int LDO = lds_ld(DT_CI), LDA = lds_ld(DT_C), LDH = lds_ld(DT_SLICE);
  __shared__ __attribute__((aligned(16))) op16 a_o[DT_MAXT * LDO];
  __shared__ __attribute__((aligned(16))) op16 a_y[DT_MAXT * LDA];
  __shared__ __attribute__((aligned(16))) op16 a_h[DT_MAXT * LDH];
  __shared__ __attribute__((aligned(16))) float part[DT_PART];
  const int T = p.T, tid = threadIdx.x, slice = blockIdx.x;
  const int64_t row0 = (int64_t)blockIdx.y * T;
  // every global read of the kernel is issued here: three weight slices, the LayerNorm's inputs, the attention output
  TokGemm<DT_C, DT_CI, 1> go;
  go.load(p.wo, DT_CI);
  TokGemm<DT_SLICE, DT_C, 4> g1;
  g1.load(p.w1 + (int64_t)slice * DT_SLICE * DT_C, DT_C);
  TokGemm<DT_C, DT_SLICE, 1> g2;
  g2.load(p.w2 + slice * DT_SLICE, DT_HID);
  const LnPre pre = ln_preload(p.bo, p.x + row0 * DT_C, nullptr, p.lnw, p.lnb, T);
  const float b1 = p.b1[slice * DT_SLICE + tid % DT_SLICE];
  load_attn_rows(a_o, p.o, p.o_part, p.splits, blockIdx.y, T);
  zero_dead_rows<DT_CI>(a_o, T);
  zero_dead_rows<DT_C>(a_y, T);
  zero_dead_rows<DT_SLICE>(a_h, T);
  __syncthreads();
  float* x2 = p.x2 + row0 * DT_C;
  proj_res_ln<DT_CI>(go, a_o, pre, p.eps, T, part, [&](int row, int c, f32x4 y, f32x4) {
    if (slice == 0) *reinterpret_cast<f32x4*>(x2 + row * DT_C + c) = y;
    *reinterpret_cast<op16x4*>(a_y + row * LDA + c) = f2op4(y);
  });
  // fc1 + ReLU on this slice of the hidden units, 16-bit
  g1.mma(a_y, part);
  __syncthreads();
  for (int i = tid; i < T * DT_SLICE; i += DT_THREADS) {
    const int row = i / DT_SLICE, col = i % DT_SLICE;
    float v = part[row * DT_SLICE + col];
#pragma unroll
    for (int kp = 1; kp < 4; ++kp) v += part[(kp * 16 + row) * DT_SLICE + col];
    a_h[row * LDH + col] = f2op(fmaxf(v + b1, 0.f));
  }
  __syncthreads();
  // this slice's share of fc2
  float* ws = p.ws + ((int64_t)slice * p.R + row0) * DT_C;
  g2.mma(a_h, a_h, 0, nullptr, [&](int, int row, int col, float v) {
    if (row < T) ws[row * DT_C + col] = v;
  });
}

struct DecKvParams {
  const float* ws;        // fc2 partials [16][R][256]
  const float* b2;
  const float* x2;        // residual: queries after norm2
  const float* lnw; const float* lnb; float eps;   // norm3
  const float* pe;
  const op16* wkv; const float* bkv;        // cross_attn_image_to_token k | v [256, 256]: k sees queries + pe
  const op16* wfq; const float* bfq;        // final attention's q_proj [128, 256] (last block) or null
  float* xout;            // queries after norm3
  op16* kv;               // [R, 256]
  op16* qp;               // [R, 128] (last block)
  int T, R;
};

__global__ __launch_bounds__(DT_THREADS) void dec_kv_kernel(DecKvParams p) {
  constexpr int LDA = lds_ld(DT_C);
  __shared__ __attribute__((aligned(16))) op16 a_k[DT_MAXT * LDA];
  __shared__ __attribute__((aligned(16))) op16 a_v[DT_MAXT * LDA];
  __shared__ __attribute__((aligned(16))) float part[DT_PART];
  const int T = p.T, tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const bool last = p.wfq != nullptr;                   // (uniform over the launch)
  TokGemm<DT_C, DT_C, 1> gk;
  gk.load(p.wkv, DT_C);
  TokGemm<DT_CI, DT_C, 4> gf;
  gf.load(last ? p.wfq : p.wkv, DT_C);                  // (no final projection: any valid rows, not used)
  const LnPre pre = ln_preload(p.b2, p.x2 + row0 * DT_C, p.pe + row0 * DT_C, p.lnw, p.lnb, T);
  const float bk = p.bkv[tid % DT_C], bf = last ? p.bfq[tid % DT_CI] : 0.f;
  zero_dead_rows<DT_C>(a_k, T);
  zero_dead_rows<DT_C>(a_v, T);
  float* xout = p.xout + row0 * DT_C;
  sum_res_ln_rows<DT_NSLICE>(p.ws + row0 * DT_C, (int64_t)p.R * DT_C, pre, p.eps, T, [&](int row, int c, f32x4 y, f32x4 pv) {
    *reinterpret_cast<f32x4*>(xout + row * DT_C + c) = y;
    *reinterpret_cast<op16x4*>(a_k + row * LDA + c) = f2op4(y + pv);
    *reinterpret_cast<op16x4*>(a_v + row * LDA + c) = f2op4(y);
  });
  __syncthreads();
  gk.mma(a_k, a_v, DT_CI, nullptr, [&](int, int row, int col, float v) { part[row * DT_C + col] = v; });
  __syncthreads();
  store_rows16<DT_C, 1>(p.kv + row0 * DT_C, part, bk, T);
  if (!last) return;
  __syncthreads();
  gf.mma(a_k, part);
  __syncthreads();
  store_rows16<DT_CI, 4>(p.qp + row0 * DT_CI, part, bf, T);
}

struct DecTailParams {
  const op16* o;          // final attention output, 16-bit [R, 128], or
  const float* o_part;    // its key-split partials (load_attn_rows)
  int splits;
  const float* x;         // residual
  const op16* wo; const float* bo;
  const float* lnw; const float* lnb; float eps;
  float* xout;
  int T;
};

__global__ __launch_bounds__(DT_THREADS) void dec_tail_kernel(DecTailParams p) {
  constexpr int LDO = lds_ld(DT_CI);
  __shared__ __attribute__((aligned(16))) op16 a_o[DT_MAXT * LDO];
  __shared__ __attribute__((aligned(16))) float part[DT_PART];
  const int T = p.T;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  TokGemm<DT_C, DT_CI, 1> go;
  go.load(p.wo, DT_CI);
  const LnPre pre = ln_preload(p.bo, p.x + row0 * DT_C, nullptr, p.lnw, p.lnb, T);
  load_attn_rows(a_o, p.o, p.o_part, p.splits, blockIdx.x, T);
  zero_dead_rows<DT_CI>(a_o, T);
  __syncthreads();
  float* xout = p.xout + row0 * DT_C;
  proj_res_ln<DT_CI>(go, a_o, pre, p.eps, T, part, [&](int row, int c, f32x4 y, f32x4) { *reinterpret_cast<f32x4*>(xout + row * DT_C + c) = y; });
}

static bool config_ok(int64_t C, int64_t heads, int64_t self_dim, int64_t cross_dim, int64_t mlp_hidden, int64_t mlp_layers, int mlp_act) {
  return C == DT_C && heads == DT_H && self_dim == DT_C && cross_dim == DT_CI && mlp_hidden == DT_HID && mlp_layers == 2 && mlp_act == 2;
}
static bool rows_ok(int64_t B, int64_t T) { return B >= 1 && T >= 1 && T <= DT_MAXT && B * T <= DT_MAXR; }

#define DEC_REQUIRE_ROWS(entry, B, T)                                                                                             \
  MSAM2_REQUIRE(rows_ok(B, T), entry ": B = %lld images of T = %lld tokens (T <= %d, B * T <= %d rows)", (long long)(B), (long long)(T), \
                DT_MAXT, DT_MAXR)

// the attention output comes as 16-bit rows or as key-split partials (1 .. 8 splits), never both
#define DEC_REQUIRE_ATTN(entry, o, o_partials, splits)                                                                                     \
  MSAM2_REQUIRE(((o) != nullptr) != ((o_partials) != nullptr) && (!(o_partials) || ((splits) >= 1 && (splits) <= 8)) &&                     \
                    ((uintptr_t)(o_partials) & 3) == 0,                                                                                    \
                entry ": exactly one of o and o_partials (with 1 .. 8 splits, got %lld)", (long long)(splits))

// 1 for exactly the two-way block these kernels are built for: C = 256, 8 heads, internal widths 256 (self) / 128 (cross), a 2-layer
// ReLU (act code 2) MLP of 2048 hidden units, B images of T <= 16 tokens with B * T <= 32.
extern "C" int msam2_decoder_tokens_supported(int64_t C, int64_t heads, int64_t self_dim, int64_t cross_dim, int64_t mlp_hidden,
                                              int64_t mlp_layers, int mlp_act, int64_t B, int64_t T) {
  return config_ok(C, heads, self_dim, cross_dim, mlp_hidden, mlp_layers, mlp_act) && rows_ok(B, T) ? 1 : 0;
}

extern "C" int msam2_decoder_tokens_self(const float* queries, const float* query_pe, int skip_first_layer_pe, const void* w_qkv,
                                         const float* b_qkv, const void* w_out, const float* b_out, const float* ln_w, const float* ln_b,
                                         float eps, const void* w_cq, const float* b_cq, float* queries_out, void* qp, int64_t B, int64_t T,
                                         int64_t C, int64_t heads, void* stream) {
  MSAM2_REQUIRE(queries && query_pe && w_qkv && b_qkv && w_out && b_out && ln_w && ln_b && w_cq && b_cq && queries_out && qp,
                "decoder_tokens_self: null tensor");
  MSAM2_REQUIRE(config_ok(C, heads, DT_C, DT_CI, DT_HID, 2, 2), "decoder_tokens_self: built for C = 256 and 8 heads (got %lld, %lld)",
                (long long)C, (long long)heads);
  DEC_REQUIRE_ROWS("decoder_tokens_self", B, T);
  MSAM2_REQUIRE(vec_ok(4, 4, queries, query_pe, b_qkv, b_out, ln_w, ln_b, b_cq, queries_out) && vec_ok(8, 2, w_qkv, w_out, w_cq, qp),
                "decoder_tokens_self: tensors must be 16-byte aligned");
  DecSelfParams p = {queries, query_pe, skip_first_layer_pe != 0, (const op16*)w_qkv, b_qkv, (const op16*)w_out, b_out, ln_w, ln_b, eps,
                     (const op16*)w_cq, b_cq, queries_out, (op16*)qp, (int)T, (float)(1.0 / sqrt((double)(DT_C / DT_H))) * 1.4426950408889634f};   // as msam2_attention_small_fwd gets and scales it
  hipLaunchKernelGGL(dec_self_kernel, dim3((unsigned)B), dim3(DT_THREADS), 0, (hipStream_t)stream, p);
  return msam2_check_launch("decoder_tokens_self");
}

extern "C" size_t msam2_decoder_tokens_workspace_bytes(int64_t B, int64_t T) {
  return rows_ok(B, T) ? (size_t)DT_NSLICE * B * T * DT_C * sizeof(float) : 0;
}

extern "C" int msam2_decoder_tokens_mlp(const void* o, const float* o_partials, int64_t splits, const float* queries, const void* w_out, const float* b_out, const float* ln2_w,
                                        const float* ln2_b, float eps2, const void* w1, const float* b1, const void* w2, const float* b2,
                                        const float* ln3_w, const float* ln3_b, float eps3, const float* query_pe, const void* w_kv,
                                        const float* b_kv, const void* w_fq, const float* b_fq, float* queries_mid, float* queries_out,
                                        void* kv, void* qp_final, void* workspace, size_t workspace_bytes, int64_t B, int64_t T, int64_t C,
                                        int64_t heads, int64_t mlp_hidden, void* stream) {
  MSAM2_REQUIRE(queries && w_out && b_out && ln2_w && ln2_b && w1 && b1 && w2 && b2 && ln3_w && ln3_b && query_pe && w_kv && b_kv &&
                    queries_mid && queries_out && kv && workspace,
                "decoder_tokens_mlp: null tensor");
  DEC_REQUIRE_ATTN("decoder_tokens_mlp", o, o_partials, splits);
  MSAM2_REQUIRE((w_fq != nullptr) == (b_fq != nullptr) && (w_fq != nullptr) == (qp_final != nullptr),
                "decoder_tokens_mlp: w_fq, b_fq and qp_final come together (last block) or not at all");
  MSAM2_REQUIRE(config_ok(C, heads, DT_C, DT_CI, mlp_hidden, 2, 2),
                "decoder_tokens_mlp: built for C = 256, 8 heads and 2048 hidden units (got %lld, %lld, %lld)", (long long)C, (long long)heads,
                (long long)mlp_hidden);
  DEC_REQUIRE_ROWS("decoder_tokens_mlp", B, T);
  MSAM2_REQUIRE(workspace_bytes >= msam2_decoder_tokens_workspace_bytes(B, T), "decoder_tokens_mlp: workspace of %zu bytes, %zu needed",
                workspace_bytes, msam2_decoder_tokens_workspace_bytes(B, T));
  MSAM2_REQUIRE(vec_ok(4, 4, queries, b_out, ln2_w, ln2_b, b1, b2, ln3_w, ln3_b, query_pe, b_kv, b_fq, queries_mid, queries_out, workspace) &&
                    vec_ok(8, 2, o, w_out, w1, w2, w_kv, w_fq, kv, qp_final),
                "decoder_tokens_mlp: tensors must be 16-byte aligned");
  float* ws = (float*)workspace;
  DecMlpParams pm = {(const op16*)o, o_partials, (int)splits, queries, (const op16*)w_out, b_out, ln2_w, ln2_b, eps2, (const op16*)w1, b1, (const op16*)w2,
                     queries_mid, ws, (int)T, (int)(B * T)};
  hipLaunchKernelGGL(dec_mlp_kernel, dim3(DT_NSLICE, (unsigned)B), dim3(DT_THREADS), 0, (hipStream_t)stream, pm);
  DecKvParams pk = {ws, b2, queries_mid, ln3_w, ln3_b, eps3, query_pe, (const op16*)w_kv, b_kv, (const op16*)w_fq, b_fq, queries_out,
                    (op16*)kv, (op16*)qp_final, (int)T, (int)(B * T)};
  hipLaunchKernelGGL(dec_kv_kernel, dim3((unsigned)B), dim3(DT_THREADS), 0, (hipStream_t)stream, pk);
  return msam2_check_launch("decoder_tokens_mlp");
}

extern "C" int msam2_decoder_tokens_tail(const void* o, const float* o_partials, int64_t splits, const float* queries, const void* w_out, const float* b_out, const float* ln_w,
                                         const float* ln_b, float eps, float* queries_out, int64_t B, int64_t T, int64_t C, int64_t heads,
                                         void* stream) {
  MSAM2_REQUIRE(queries && w_out && b_out && ln_w && ln_b && queries_out, "decoder_tokens_tail: null tensor");
  DEC_REQUIRE_ATTN("decoder_tokens_tail", o, o_partials, splits);
  MSAM2_REQUIRE(config_ok(C, heads, DT_C, DT_CI, DT_HID, 2, 2), "decoder_tokens_tail: built for C = 256 and 8 heads (got %lld, %lld)",
                (long long)C, (long long)heads);
  DEC_REQUIRE_ROWS("decoder_tokens_tail", B, T);
  MSAM2_REQUIRE(vec_ok(4, 4, queries, b_out, ln_w, ln_b, queries_out) && vec_ok(8, 2, o, w_out),
                "decoder_tokens_tail: tensors must be 16-byte aligned");
  DecTailParams p = {(const op16*)o, o_partials, (int)splits, queries, (const op16*)w_out, b_out, ln_w, ln_b, eps, queries_out, (int)T};
  hipLaunchKernelGGL(dec_tail_kernel, dim3((unsigned)B), dim3(DT_THREADS), 0, (hipStream_t)stream, p);
  return msam2_check_launch("decoder_tokens_tail");
}
