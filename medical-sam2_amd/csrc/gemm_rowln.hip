// Full-row GEMM with the residual add and the NEXT LayerNorm in its epilogue (gemm_rowln_kernel), for the proj and fc2 GEMMs of Hiera stage 3:
//
//   C32[M, N] = A[M, K] W[N, K]^T + bias + R32[M, N]          (fp32: the residual stream)
//   Y16[M, N] = LayerNorm(C32 rows; gamma, beta, eps)          (operand type: the A of the GEMM that follows)
//
// The two launches it replaces (gemm_glds_kernel with the fp32 + residual epilogue, layernorm_kernel<float, op16, 6>) meet in memory: the
// LayerNorm re-reads the 25 MB map the GEMM has just written to produce a 12.6 MB 16-bit copy.  A LayerNorm row is complete
// in the GEMM that produces it as soon as ONE workgroup owns all N columns of its rows, so the tile here is 64 rows x all N = 384 columns:
//
//   * cdiv(M, 64) workgroups through xcd_tile_order (256 at M = 16384: one per CU), 8 waves = 2 row slabs x 4 column quarters; a wave owns
//     32 x 96 = three 32 x 32 accumulators (48 registers);
//   * operands through a 2-stage LDS-DMA ring of BK = 64 (DmaImage<128>: 128-byte rows = whole cache lines; A 8 KB + W 48 KB = 56 KB per
//     stage, 112 KB).  A stage is 56 pieces (8 rows x 128 B each): every wave issues one A piece and 6 W pieces (rows 48 w .. 48 w + 47),
//     7 per wave and tile in all eight waves.  The next tile is issued right behind the barrier that frees its stage and waited for with
//     vmcnt(0) before the barrier of the next k-step: nothing else of this wave is in flight then (the three bias loads and the prefetch
//     pieces below are OLDER than tile 0), so there is no counted wait to get wrong.  The four-stage ring of BK = 32 the shape was first
//     built with (28 pieces per stage, 4 per tile in waves 0 - 3 and 3 in waves 4 - 7, waits 8 / 4 / 0 and 6 / 3 / 0) measured the same
//     per-k cost and a slower prologue and is not kept;
//   * W prefetch: the 32 workgroups of an XCD read the same W in step, so each of its 128-byte line columns was one Infinity Cache round
//     trip for all of them.  Before tile 0 every workgroup sends its 1 / 32 of W (rows 12 j .. 12 j + 11, j = its place in the XCD)
//     through throw-away pieces into the ring's second stage: the whole weight is on its way into the XCD's L2 at once;
//   * k order: every accumulator takes k ascending in 16-wide MFMA steps with gemm_glds_kernel's operand map (lane half h holds chunk
//     2 ks + h): the order of the kernels it replaces, so C32 has their bits;
//   * epilogue: the ring is dead after the last k-step (vmcnt(0) + barrier); every wave writes acc + bias as fp32 into one row-major LDS
//     tile [64][N + 4] (97 KB, aliasing the ring); barrier; the tile is walked in layernorm_kernel's geometry (16 lanes per row, 4 rows
//     per wave, lane chunks l16 + 16 j) in two passes of 32 rows.  A lane's 12 residual chunks, gamma and beta are loaded up front, before
//     any store (one in-order counter: a load behind a store waits for the store's round trip).  x = (acc + bias) + r is
//     gemm_epilogue_direct's fp32 + residual association; mean, centred sum of squares, rstd and the 16-bit output are layernorm_kernel's
//     expressions in its order (elementwise.hip), RESTATED here: layernorm_kernel is left as it is.
// Rows past M are clamped on load and masked on store.  Every wave runs the same number of barriers.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage): 155 VGPRs, 53 SGPRs in both builds, no scratch, one workgroup per CU by its 112 KB of LDS.
// Measured inside the benchmark step: K = 384 18.1 us against 17.9 + 9.1 for the pair, K = 1536 43.7 against 36.0 + 9.1.
#include "common.h"
#include <stdlib.h>

struct RowLnParams {
  const op16* A;
  const op16* W;
  const float* bias;     // [N] or null
  const float* R;        // [M, N] fp32 residual
  float* C;              // [M, N] fp32
  const float* ln_w;
  const float* ln_b;
  op16* Y;               // [M, N] LayerNorm(C rows)
  int64_t lda, ldw, ldr, ldc, ldy;
  int M, K;
  float eps;
};

template <int N>
__global__ __launch_bounds__(512, 1) void gemm_rowln_kernel(RowLnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Img128 Img;
  constexpr int BM = 64, BK = 64, NST = 2, KS = BK / 16;
  constexpr int A_BYTES = BM * BK * 2, STAGE_BYTES = (BM + N) * BK * 2;    // 8 KB + 48 KB
  constexpr int WPW = N / Img::PIECE_ROWS / 8;       // W pieces per wave and stage: 6
  constexpr int FN = N / 4 / 32;                     // 32-column accumulators per wave: 3
  constexpr int TLD = N + 4;                         // floats per row of the epilogue tile
  constexpr int CH = N / 64;                         // 4-element chunks per lane and row: 6
  static_assert(N % 128 == 0 && WPW * 8 * Img::PIECE_ROWS == N && BM == 8 * Img::PIECE_ROWS, "8 waves share the pieces of a stage evenly");
  static_assert(BM * TLD * 4 <= NST * STAGE_BYTES, "the epilogue tile aliases the ring");
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int ws = wave >> 2, wq = wave & 3;           // row slab of 32, column quarter of N / 4
  const int r = lane & 31, h = lane >> 5;
  const int64_t m0 = (int64_t)xcd_tile_order(blockIdx.x, gridDim.x) * BM;
  if (m0 >= p.M) return;                             // the whole workgroup, before the first barrier

  float bias_j[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) bias_j[j] = p.bias ? p.bias[wq * (N / 4) + j * 32 + r] : 0.f;

  const auto a_rsrc = raw_rsrc(p.A);
  const auto w_rsrc = raw_rsrc(p.W);
  unsigned offsA, offsW[WPW];
  {
    const int row = Img::piece_row(wave, lane);
    offsA = (unsigned)(min(m0 + row, (int64_t)p.M - 1) * p.lda * 2 + Img::src_chunk(row, lane) * 16);
  }
#pragma unroll
  for (int i = 0; i < WPW; ++i) {
    const int row = Img::piece_row(wave * WPW + i, lane);
    offsW[i] = (unsigned)((int64_t)row * p.ldw * 2 + Img::src_chunk(row, lane) * 16);
  }
  const int nk = p.K / BK;
  auto issue = [&](int kt) {
    unsigned char* base = lds + (kt % NST) * STAGE_BYTES;
    const unsigned so = (unsigned)kt * BK * 2;
    glds16(a_rsrc, base + wave * 1024, offsA, so);
#pragma unroll
    for (int i = 0; i < WPW; ++i) glds16(w_rsrc, base + A_BYTES + (wave * WPW + i) * 1024, offsW[i], so);
  };

  {
    // this workgroup's share of W (rows 12 j .. 12 j + 11, j = its place among the 32 workgroups of its XCD) into the XCD's L2, through
    // throw-away pieces into the ring's last stage: older than tile 0, so landed before the first barrier lets anybody fill that stage
    const int j = (blockIdx.x >> 3) & 31, cpr = p.K >> 3, n = (N / 32) * cpr;
    unsigned char* dst = lds + (NST - 1) * STAGE_BYTES + wave * 1024;
    for (int i = wave; i * 64 < n; i += 8) {
      const int q = min(i * 64 + lane, n - 1);
      const int row = j * (N / 32) + q / cpr, c = q - (q / cpr) * cpr;
      glds16(w_rsrc, dst, (unsigned)((int64_t)row * p.ldw * 2 + c * 16), 0);
    }
  }

  f32x16 acc[FN];
  zero_acc(acc);

  // fragment read offsets (bytes) inside a stage, without the k-substep term
  const int ra = ws * 32 + r;
  const int offA = ra * Img::ROW_BYTES, swzA = Img::swz(ra);
  int offB[FN], swzB[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int rb = wq * (N / 4) + j * 32 + r;
    offB[j] = A_BYTES + rb * Img::ROW_BYTES;
    swzB[j] = Img::swz(rb);
  }

  issue(0);
  for (int kt = 0; kt < nk; ++kt) {
    wait_vmcnt<0>();                                     // this wave's 7 pieces of tile kt (and everything older) have landed
    __builtin_amdgcn_s_barrier();                        // tile kt visible to all waves; the stage of tile kt - 1 is no longer read
    if (kt + 1 < nk) issue(kt + 1);
    const unsigned char* sb = lds + (kt % NST) * STAGE_BYTES;
    op16x8 af[KS], bfr[KS][FN];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = 2 * ks + h;
      af[ks] = *reinterpret_cast<const op16x8*>(sb + offA + ((c ^ swzA) << 4));
#pragma unroll
      for (int j = 0; j < FN; ++j) bfr[ks][j] = *reinterpret_cast<const op16x8*>(sb + offB[j] + ((c ^ swzB[j]) << 4));
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[j] = MSAM2_MFMA_32x32x16(af[ks], bfr[ks][j], acc[j], 0, 0, 0);
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();                          // every wave is past its last fragment read: the ring is dead

  // ---- epilogue.  Row side first: everything a lane will load, before any store
  const int l16 = lane & 15;
  int64_t grow[2];
  f32x4 rv[2][CH], ww[CH], bb[CH];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    grow[ps] = m0 + ps * 32 + wave * 4 + (lane >> 4);
    const float* rr = p.R + min(grow[ps], (int64_t)p.M - 1) * p.ldr;
#pragma unroll
    for (int j = 0; j < CH; ++j) rv[ps][j] = *reinterpret_cast<const f32x4*>(rr + (l16 + 16 * j) * 4);
  }
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    ww[j] = *reinterpret_cast<const f32x4*>(p.ln_w + (l16 + 16 * j) * 4);
    bb[j] = *reinterpret_cast<const f32x4*>(p.ln_b + (l16 + 16 * j) * 4);
  }
  // acc + bias -> the row-major tile: register e of lane (r, h) is row (e & 3) + 8 (e >> 2) + 4 h, column r of its 32 x 32 block
  float* tile = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e)
      tile[(ws * 32 + s_frag_key(e, h)) * TLD + wq * (N / 4) + j * 32 + r] = acc[j][e] + bias_j[j];
  __builtin_amdgcn_s_barrier();
  // x = (acc + bias) + r for both passes, and the fp32 rows
  float v[2][CH][4];
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const float* trow = tile + (ps * 32 + wave * 4 + (lane >> 4)) * TLD;
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(trow + (l16 + 16 * j) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[ps][j][e] = t[e] + rv[ps][j][e];
    }
  }
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    if (grow[ps] < p.M) {
      float* cr = p.C + grow[ps] * p.ldc;
#pragma unroll
      for (int j = 0; j < CH; ++j) *reinterpret_cast<f32x4*>(cr + (l16 + 16 * j) * 4) = f32x4{v[ps][j][0], v[ps][j][1], v[ps][j][2], v[ps][j][3]};
    }
  }
  // layernorm_kernel's arithmetic on the row (C = N, every chunk inside the row)
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += v[ps][j][e];
    group16_add(s);
    const float mean = s / N;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < CH; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[ps][j][e] - mean;
        q += d * d;
      }
    group16_add(q);
    const float rstd = 1.0f / sqrtf(q / N + p.eps);
    if (grow[ps] < p.M) {
      op16* yr = p.Y + grow[ps] * p.ldy;
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        op16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float u = (v[ps][j][e] - mean) * rstd * ww[j][e] + bb[j][e];
          o[e] = f2out<op16>(u);
        }
        *reinterpret_cast<op16x4*>(yr + (l16 + 16 * j) * 4) = o;
      }
    }
  }
#endif
}

extern "C" int msam2_gemm_residual_layernorm_supported(int64_t N, int64_t K) { return (N == 384 && K > 0 && K % 64 == 0) ? 1 : 0; }

extern "C" int msam2_gemm_residual_layernorm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* R32,
                                             int64_t ldr, float* C32, int64_t ldc, const float* ln_w, const float* ln_b, float eps, void* Y16,
                                             int64_t ldy, int64_t M, int64_t N, int64_t K, void* stream) {
  MSAM2_REQUIRE(A && W && R32 && C32 && ln_w && ln_b && Y16, "gemm_residual_layernorm: null operand");
  MSAM2_REQUIRE(msam2_gemm_residual_layernorm_supported(N, K), "gemm_residual_layernorm: N=%lld K=%lld is not built (N = 384, K %% 64 == 0)",
                (long long)N, (long long)K);
  MSAM2_REQUIRE(M > 0 && M < (1ll << 31) - 64, "gemm_residual_layernorm: M=%lld", (long long)M);
  MSAM2_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "gemm_residual_layernorm: lda, ldw must be multiples of 8 (16-byte rows), >= K");
  MSAM2_REQUIRE(ldr % 4 == 0 && ldc % 4 == 0 && ldy % 4 == 0 && ldr >= N && ldc >= N && ldy >= N,
                "gemm_residual_layernorm: ldr, ldc, ldy must be multiples of 4, >= N");
  MSAM2_REQUIRE(vec_ok(8, 2, A, W) && vec_ok(4, 4, (const void*)bias, (const void*)R32, (const void*)C32, (const void*)ln_w, (const void*)ln_b) &&
                    vec_ok(4, 2, (const void*)Y16),
                "gemm_residual_layernorm: A, W, bias, R32, C32, ln_w, ln_b must be 16-byte aligned, Y16 8-byte");
  MSAM2_REQUIRE(M * lda * 2 < (1ll << 31) && N * ldw * 2 < (1ll << 31), "gemm_residual_layernorm: A / W beyond the 2 GB of a buffer descriptor's offsets");
  RowLnParams p;
  p.A = (const op16*)A; p.W = (const op16*)W; p.bias = bias; p.R = R32; p.C = C32; p.ln_w = ln_w; p.ln_b = ln_b; p.Y = (op16*)Y16;
  p.lda = lda; p.ldw = ldw; p.ldr = ldr; p.ldc = ldc; p.ldy = ldy;
  p.M = (int)M; p.K = (int)K; p.eps = eps;
  constexpr int LDS = 2 * (64 + 384) * 64 * 2;
  ensure_dyn_lds<gemm_rowln_kernel<384>>(LDS);
  hipLaunchKernelGGL((gemm_rowln_kernel<384>), dim3(cdiv(M, 64)), dim3(512), LDS, (hipStream_t)stream, p);
  return msam2_check_launch("gemm_residual_layernorm");
}
