// MaskDownSampler stages 2 - 4 (memory_encoder.py:37-54: Conv2d(CIN, 4 CIN, k3, s2, p1) + LayerNorm2d + GELU) as ONE kernel per stage:
// an implicit GEMM whose A fragments are gathered from the NHWC input, with bias + LayerNorm2d + GELU in the epilogue
// (conv3x3s2_mfma_kernel).  It replaces im2col3x3s2_kernel -> gemm (fp32 out) -> layernorm_kernel<float, op16, .> with GELU: the patch
// matrix [pixels, 9 CIN] and the fp32 GEMM output are written once and read once by those launches and by nobody else.
//
//   Y16[B, H/2, W/2, COUT] = GELU(LayerNorm(conv(X16[B, H, W, CIN]; Wp) + bias; gamma, beta, eps))
//
// Wp is the packed weight of the GEMM path, [COUT, ldw] with columns (ky, kx, c) and zero fill up to ceil8(9 CIN).  THE OUTPUT HAS THE
// BITS OF THE THREE LAUNCHES (the training backward recomputes the forward in that form):
//   * a wave owns 32 output pixels (MFMA rows) x COUT / WC columns and runs the WHOLE reduction, k ascending in 16-wide steps of
//     MSAM2_MFMA_32x32x16 with the GEMM kernels' operand map (lane half h holds k = 16 ks + 8 h .. + 7): eight consecutive k are 8 channels
//     of one tap (CIN >= 16) or two adjacent taps x 4 channels (CIN = 4).  Taps outside the image, k >= 9 CIN and the steps up to the GEMM's
//     32-wide k-tile are zero fragments, as the im2col map and gemm_kernel's / gemm_glds_kernel's zero fill give them;
//   * SKINNY (at most 32 pixels and 9 CIN % 16 == 0): that GEMM runs in gemm_skinny_kernel, whose four waves own a quarter of the 16-wide
//     steps each and add their partial sums as ((p0 + p1) + p2) + p3 before the bias.  The instance reproduces that association (a wave
//     here runs the four quarters one after the other);
//   * acc + bias goes as fp32 into one row-major LDS tile [32 WR][COUT + 4], which is walked in layernorm_kernel's geometry (16 lanes per
//     row, lane chunks l + 16 j; 4 lanes per row at COUT = 16, where 12 of that kernel's 16 lanes hold zeros): sum, centred second pass,
//     rstd, gelu_erf_as, f2op -- its arithmetic in its order, RESTATED with every fma written out (ln_row_stats, ln_row_value in common.h, which
//     the full-row GEMM kernels share; ln_gelu_value below; layernorm_kernel is left as it is).
// Operands come straight from global memory into the fragment registers, two groups of k-steps in flight (the next group's loads are
// issued before the MFMAs of the current one): the input pixels of a wave are re-read by neighbouring taps from L1, the weight (at most
// 295 KB) from L2.  All loads are unconditional with clamped addresses and zeroed afterwards; rows past the last pixel are clamped on
// load and masked on store.
#include "common.h"

struct ConvLnParams {
  const op16* X;       // [B, H, W, CIN]
  const op16* W;       // [COUT, ldw]
  const float* bias;   // [COUT]
  const float* ln_w;
  const float* ln_b;
  op16* Y;             // [M, COUT], row stride ldy
  int64_t ldw, ldy;
  int B, H, Wd, M;     // M = B (H / 2) (Wd / 2) output pixels
  float eps;
};

// layernorm_kernel's value with act = GELU, every rounding WRITTEN OUT and contraction off, as ln_row_stats / ln_row_value (common.h)
// state the row arithmetic and for their reason: u = ln_row_value;  GELU (gelu_erf_as): d = fma(ax, 0.3275911, 1), Horner by fma,
// max(u, 0) - (|u| / 2)(poly ex) as one fma.
__device__ __forceinline__ float ln_gelu_value(float x, float mean, float rstd, float w, float b) {
#pragma clang fp contract(off)
  const float u = ln_row_value(x, mean, rstd, w, b);
  const float ab = fabsf(u);
  const float ax = ab * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(ax, 0.3275911f, 1.0f));
  float poly = __builtin_fmaf(t, 1.061405429f, -1.453152027f);
  poly = __builtin_fmaf(t, poly, 1.421413741f);
  poly = __builtin_fmaf(t, poly, -0.284496736f);
  poly = __builtin_fmaf(t, poly, 0.254829592f);
  poly = t * poly;
  const float ex = __builtin_amdgcn_exp2f((ax * ax) * (-1.44269504088896340736f));
  return __builtin_fmaf(-(ab * 0.5f), poly * ex, fmaxf(u, 0.f));
}

template <int CIN, int COUT, int WR, int WC, bool SKINNY>
__global__ __launch_bounds__(WR* WC * 64) void conv3x3s2_mfma_kernel(ConvLnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NW = WR * WC, BM = WR * 32;
  constexpr int TNW = COUT / WC;                          // columns per wave
  constexpr int FN = TNW >= 32 ? TNW / 32 : 1;            // 32-column accumulators per wave (COUT = 16: half of one)
  constexpr int KR = 9 * CIN, KP = (KR + 7) / 8 * 8;      // reduction length, and the K of the GEMM it replaces
  constexpr int KSTEPS = SKINNY ? KP / 16 : (KP + 31) / 32 * 2;
  constexpr int PER = (KSTEPS + 3) / 4;                   // SKINNY: 16-wide steps per partial sum (gemm_skinny_kernel)
  constexpr int G = CIN == 16 ? 5 : 4;                    // k-steps per group of loads
  constexpr int NG = (KSTEPS + G - 1) / G;
  constexpr int TLD = COUT + 4;                           // floats per row of the epilogue tile
  constexpr int NCH = COUT / 4;                           // 4-element chunks per row
  constexpr int LPR = NCH < 16 ? NCH : 16;                // lanes per row of the LayerNorm walk (layernorm_kernel: 16, NCH of them live)
  constexpr int CPL = NCH / LPR;                          // chunks per lane
  constexpr int RPW = 64 / LPR;                           // rows per wave and pass
  constexpr int PASSES = BM / (NW * RPW);
  static_assert(CIN == 4 || CIN % 16 == 0, "eight consecutive k: 8 channels of one tap, or two taps x 4 channels");
  static_assert(COUT % WC == 0 && (TNW % 32 == 0 || (WC == 1 && COUT == 16)) && BM % (NW * RPW) == 0 && NCH % LPR == 0 && (LPR & (LPR - 1)) == 0,
                "wave tiling");
  static_assert(!SKINNY || KP % 16 == 0, "gemm_skinny_kernel serves K % 16 == 0 only");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* tile = reinterpret_cast<float*>(lds);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wr = wave / WC, wc = wave % WC;
  const int r = lane & 31, h = lane >> 5;
  const int64_t m0 = (int64_t)xcd_tile_order(blockIdx.x, gridDim.x) * BM;
  if (m0 >= p.M) return;                                  // the whole workgroup, before the first barrier

  // this lane's output pixel (A operand row), clamped; 32-bit index arithmetic (M < 2^31 is checked on the host)
  const unsigned Ho = (unsigned)p.H >> 1, Wo = (unsigned)p.Wd >> 1;
  const unsigned m = (unsigned)min(m0 + wr * 32 + r, (int64_t)p.M - 1);
  const unsigned t1 = m / Wo, ox = m - t1 * Wo;
  const unsigned b = t1 / Ho, oy = t1 - b * Ho;
  const int y0 = 2 * (int)oy - 1, x0 = 2 * (int)ox - 1;
  const op16* xb = p.X + (int64_t)b * p.H * p.Wd * CIN;

  // eight k of pixel row `m` starting at k0 = 16 ks + 8 h: unconditional load(s) at a clamped address, zeroed when the tap is outside
  auto load_a = [&](int ks) -> op16x8 {
    op16x8 o;
    if constexpr (CIN >= 16) {
      const int tap = (16 * ks) / CIN, c = (16 * ks) % CIN + 8 * h;   // (compile-time tap: CIN % 16 == 0)
      const int ty = tap < 9 ? tap / 3 : 0, tx = tap < 9 ? tap % 3 : 0;
      const int y = y0 + ty, x = x0 + tx;
      const bool in = tap < 9 && y >= 0 && y < p.H && x >= 0 && x < p.Wd;
      const op16x8 v = *reinterpret_cast<const op16x8*>(xb + ((int64_t)min(max(y, 0), p.H - 1) * p.Wd + min(max(x, 0), p.Wd - 1)) * CIN + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = in ? v[e] : (op16)0.f;
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int tap = 4 * ks + 2 * h + q;
        const int tc = min(tap, 8), ty = tc / 3, tx = tc - 3 * ty;
        const int y = y0 + ty, x = x0 + tx;
        const bool in = tap < 9 && y >= 0 && y < p.H && x >= 0 && x < p.Wd;
        const op16x4 v = *reinterpret_cast<const op16x4*>(xb + ((int64_t)min(max(y, 0), p.H - 1) * p.Wd + min(max(x, 0), p.Wd - 1)) * CIN);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[4 * q + e] = in ? v[e] : (op16)0.f;
      }
    }
    return o;
  };
  // eight k of weight row n (B operand column), zero past the packed row's KP columns and past COUT
  const op16* wrow[FN];
  bool w_in[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = wc * TNW + j * 32 + r;
    w_in[j] = n < COUT;
    wrow[j] = p.W + (int64_t)min(n, COUT - 1) * p.ldw;
  }
  auto load_w = [&](int ks, int j) -> op16x8 {
    const int k0 = 16 * ks + 8 * h;
    const op16x8 v = *reinterpret_cast<const op16x8*>(wrow[j] + min(k0, KP - 8));
    const bool in = w_in[j] && k0 < KP;
    op16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = in ? v[e] : (op16)0.f;
    return o;
  };

  float bias_j[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) bias_j[j] = p.bias[min(wc * TNW + j * 32 + r, COUT - 1)];

  f32x16 acc[FN], tot[FN];
  zero_acc(acc);
  zero_acc(tot);
  op16x8 af[2][G], wf[2][G][FN];
  auto load_group = [&](int g, int buf) {
#pragma unroll
    for (int s = 0; s < G; ++s) {
      const int ks = min(g * G + s, KSTEPS - 1);          // (a step past the end is re-read, not multiplied)
      af[buf][s] = load_a(ks);
#pragma unroll
      for (int j = 0; j < FN; ++j) wf[buf][s][j] = load_w(ks, j);
    }
  };
  load_group(0, 0);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    if (g + 1 < NG) load_group(g + 1, (g + 1) & 1);
#pragma unroll
    for (int s = 0; s < G; ++s) {
      const int ks = g * G + s;
      if (ks < KSTEPS) {
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[j] = MSAM2_MFMA_32x32x16(af[g & 1][s], wf[g & 1][s][j], acc[j], 0, 0, 0);
        if constexpr (SKINNY) {
          if ((ks + 1) % PER == 0 || ks == KSTEPS - 1) {  // a quarter is complete: ((p0 + p1) + p2) + p3
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
              for (int e = 0; e < 16; ++e) {
                tot[j][e] = ks < PER ? acc[j][e] : tot[j][e] + acc[j][e];
                acc[j][e] = 0.f;
              }
          }
        }
      }
    }
  }
  if constexpr (SKINNY) {
    // quarters that own no step (9 steps: 3 + 3 + 3 + 0) add their zero accumulator
#pragma unroll
    for (int q = (KSTEPS + PER - 1) / PER; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[j][e] = tot[j][e] + acc[j][e];
  }

  // ---- epilogue.  Everything a lane will load, before any store
  const int ll = lane % LPR;
  f32x4 ww[CPL], bb[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    ww[j] = *reinterpret_cast<const f32x4*>(p.ln_w + (ll + LPR * j) * 4);
    bb[j] = *reinterpret_cast<const f32x4*>(p.ln_b + (ll + LPR * j) * 4);
  }
  // acc + bias -> the row-major tile: register e of lane (r, h) is row (e & 3) + 8 (e >> 2) + 4 h, column r of its 32 x 32 block
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = wc * TNW + j * 32 + r;
    if (n < COUT) {
#pragma unroll
      for (int e = 0; e < 16; ++e) tile[(wr * 32 + s_frag_key(e, h)) * TLD + n] = (SKINNY ? tot[j][e] : acc[j][e]) + bias_j[j];
    }
  }
  __syncthreads();
  // layernorm_kernel's arithmetic on the rows of the tile (act = GELU, 16-bit output): LPR lanes per row, lane l owns chunks l + LPR j
#pragma unroll
  for (int ps = 0; ps < PASSES; ++ps) {
    const int trow = (ps * NW + wave) * RPW + lane / LPR;
    const int64_t grow = m0 + trow;
    float v[CPL][4];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(tile + trow * TLD + (ll + LPR * j) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] = t[e];
    }
    float mean, rstd;
    ln_row_stats<CPL, LPR, COUT>(v, p.eps, mean, rstd);
    if (grow < p.M) {
      op16* yr = p.Y + grow * p.ldy;
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        op16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2out<op16>(ln_gelu_value(v[j][e], mean, rstd, ww[j][e], bb[j][e]));
        *reinterpret_cast<op16x4*>(yr + (ll + LPR * j) * 4) = o;
      }
    }
  }
#endif
}

template <int CIN, int COUT, int WR, int WC>
static void conv3x3s2_mfma_launch(const ConvLnParams& p, hipStream_t s) {
  constexpr int LDS = WR * 32 * (COUT + 4) * 4;
  const dim3 grid(cdiv(p.M, WR * 32)), block(WR * WC * 64);
  // the GEMM of the launches this replaces runs in gemm_skinny_kernel at M <= 32 and K % 16 == 0: another order of the k sum
  if constexpr (((9 * CIN + 7) / 8 * 8) % 16 == 0) {
    if (p.M <= 32) {
      ensure_dyn_lds<conv3x3s2_mfma_kernel<CIN, COUT, WR, WC, true>>(LDS);
      hipLaunchKernelGGL((conv3x3s2_mfma_kernel<CIN, COUT, WR, WC, true>), grid, block, LDS, s, p);
      return;
    }
  }
  ensure_dyn_lds<conv3x3s2_mfma_kernel<CIN, COUT, WR, WC, false>>(LDS);
  hipLaunchKernelGGL((conv3x3s2_mfma_kernel<CIN, COUT, WR, WC, false>), grid, block, LDS, s, p);
}

extern "C" int msam2_conv3x3s2_mfma_ln_gelu_supported(int64_t cin, int64_t cout) {
  return ((cin == 4 && cout == 16) || (cin == 16 && cout == 64) || (cin == 64 && cout == 256)) ? 1 : 0;
}

extern "C" int msam2_conv3x3s2_mfma_ln_gelu(const void* x, const void* w_packed, int64_t ldw, const float* bias, const float* ln_w, const float* ln_b,
                                            float eps, void* y, int64_t ldy, int64_t B, int64_t H, int64_t W, int64_t cin, int64_t cout, void* stream) {
  MSAM2_REQUIRE(x && w_packed && bias && ln_w && ln_b && y, "conv3x3s2_mfma_ln_gelu: null operand");
  MSAM2_REQUIRE(msam2_conv3x3s2_mfma_ln_gelu_supported(cin, cout), "conv3x3s2_mfma_ln_gelu: cin=%lld cout=%lld is not built (4->16, 16->64, 64->256)",
                (long long)cin, (long long)cout);
  MSAM2_REQUIRE(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "conv3x3s2_mfma_ln_gelu: B=%lld H=%lld W=%lld (even H, W)", (long long)B,
                (long long)H, (long long)W);
  MSAM2_REQUIRE(B * H * W * cin < (1ll << 31), "conv3x3s2_mfma_ln_gelu: more than 2^31 input elements");
  MSAM2_REQUIRE(ldw % 8 == 0 && ldw >= (9 * cin + 7) / 8 * 8 && ldy % 4 == 0 && ldy >= cout,
                "conv3x3s2_mfma_ln_gelu: ldw must be a multiple of 8, >= ceil8(9 cin); ldy a multiple of 4, >= cout");
  MSAM2_REQUIRE(vec_ok(8, 2, x, w_packed) && vec_ok(4, 4, (const void*)bias, (const void*)ln_w, (const void*)ln_b) && vec_ok(4, 2, y),
                "conv3x3s2_mfma_ln_gelu: x, w_packed, bias, ln_w, ln_b must be 16-byte aligned, y 8-byte");
  ConvLnParams p;
  p.X = (const op16*)x; p.W = (const op16*)w_packed; p.bias = bias; p.ln_w = ln_w; p.ln_b = ln_b; p.Y = (op16*)y;
  p.ldw = ldw; p.ldy = ldy; p.B = (int)B; p.H = (int)H; p.Wd = (int)W; p.M = (int)(B * (H / 2) * (W / 2)); p.eps = eps;
  hipStream_t s = (hipStream_t)stream;
  if (cin == 4) conv3x3s2_mfma_launch<4, 16, 4, 1>(p, s);
  else if (cin == 16) conv3x3s2_mfma_launch<16, 64, 4, 1>(p, s);
  else conv3x3s2_mfma_launch<64, 256, 2, 4>(p, s);
  return msam2_check_launch("conv3x3s2_mfma_ln_gelu");
}
