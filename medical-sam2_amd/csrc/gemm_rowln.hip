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
//     expressions in its order (elementwise.hip) as common.h states them, every fma written out (ln_row_stats, ln_row_value);
//     layernorm_kernel is left as it is.
// Rows past M are clamped on load and masked on store.  Every wave runs the same number of barriers.
// The tile's constants (RowTile<N>), the W prefetch, the k-step and the epilogue are rowtile.h's, which mlp_rowln.hip shares; so are the
// refusals and the params fill the C entries below have in common (rowtile_check, rowtile_fill_out).  Here: the ring, `issue`, the
// main loop, the merged-A prologue.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage): 155 VGPRs, 53 SGPRs in both builds, no scratch, one workgroup per CU by its 112 KB of LDS.
// Measured inside the benchmark step: K = 384 18.1 us against 17.9 + 9.1 for the pair, K = 1536 43.7 against 36.0 + 9.1.
//
// The figures above are those of the N = 384 instance, <384, 0>.  The memory attention's layers run the same tile at
// N = 256 -- two accumulators per wave, 4 W pieces per wave and stage, a 40 KB stage, the epilogue tile [64][260] -- in two forms:
//   * <256, 0>: A through the ring as above (K = 64, 256, 2048; nk = 1 runs: no next tile is ever issued);
//   * <256, 64>, <256, 256> ("merged"): A[M, K] is the merge of split-KV attention partials and exists in LDS only.  Before the main loop
//     every thread merges the 16-byte chunks it owns with attn_merge_kernel's arithmetic (attention.hip) and stores them into K / 64
//     RESIDENT 8 KB images in front of the ring; the ring then carries W alone (32 KB stages), so the prefetch's throw-away pieces and
//     the next W tile never touch an image.  The epilogue tile aliases images and ring behind the barrier that ends the main loop.
// The merge is restated here, compiled with contraction off and its fused multiply-adds spelled as attn_merge_kernel's listings show
// them; the LayerNorm of every instance is the written-out form of common.h (for <384, 0> it is what the compiler made of the source form
// the kernel was measured and tested with: same listing).
// Registers: <256, 0> 92, <256, 64> 91, <256, 256> 190 VGPRs (a thread's 4 x 8 partial chunks are loaded up front), 53 - 55 SGPRs, 80 / 72
// / 96 KB of LDS, no scratch in both builds.  In the step: 34.3 -> 17.0 us (K = 256) and 32.5 -> 12.2 us (K = 64) per chain of three launches.
#include "rowtile.h"
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
  // the "merged" A source (MD != 0): split-KV partials in msam2_attention_workspace_bytes' layout with H = 1, rows = M, D = K
  const op16* P;         // [splits][M][K] each split's normalised output
  const float* ML;       // [splits][M][2] its (max, sum)
  int splits;            // 2 .. 8
};

// MD = 0: A is a 16-bit matrix that goes through the ring with W.  MD = 64 / 256 (= K): A is built in LDS from split-KV partials.
template <int N, int MD>
__global__ __launch_bounds__(512, 1) void gemm_rowln_kernel(RowLnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Img128 Img;
  constexpr bool MERGED = MD != 0;
  typedef RowTile<N> T;
  constexpr int BM = T::BM, BK = T::BK, A_BYTES = T::A_BYTES, WPW = T::WPW, FN = T::FN, NST = 2;
  constexpr int RES_BYTES = MERGED ? (MD / BK) * A_BYTES : 0;              // merged: the A images of the whole K, resident in front of the ring
  constexpr int W_OFF = MERGED ? 0 : A_BYTES;                              // where W starts inside a stage
  constexpr int STAGE_BYTES = W_OFF + T::W_BYTES;                          // N = 384: 8 KB + 48 KB
  static_assert(T::TILE_BYTES <= RES_BYTES + NST * STAGE_BYTES, "the epilogue tile aliases the A images and the ring");
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  unsigned char* const ring = lds + RES_BYTES;
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
    unsigned char* base = ring + (kt % NST) * STAGE_BYTES;
    const unsigned so = (unsigned)kt * BK * 2;
    if constexpr (!MERGED) glds16(a_rsrc, base + wave * 1024, offsA, so);
#pragma unroll
    for (int i = 0; i < WPW; ++i) glds16(w_rsrc, base + W_OFF + (wave * WPW + i) * 1024, offsW[i], so);
  };

  // this workgroup's share of W (rows 12 j .. 12 j + 11 at N = 384) through the ring's last stage
  ROWTILE_PREFETCH_W(w_rsrc, p.ldw, N / 32, p.K >> 3, (blockIdx.x >> 3) & 31, ring + (NST - 1) * STAGE_BYTES + wave * 1024);

  f32x16 acc[FN];
  zero_acc(acc);

  // fragment read offsets (bytes) inside a stage, without the k-substep term
  const int ra = ws * 32 + r;
  const int offA = ra * Img::ROW_BYTES, swzA = Img::swz(ra);
  int offB[FN], swzB[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int rb = wq * (N / 4) + j * 32 + r;
    offB[j] = W_OFF + rb * Img::ROW_BYTES;
    swzB[j] = Img::swz(rb);
  }

  issue(0);
  if constexpr (MERGED) {
    // The A tile from the partials, behind the W pieces already in flight: attn_merge_kernel's `splits <= G` branch (attention.hip) for this
    // workgroup's 64 rows -- every pair and every partial chunk of a thread loaded up front (split index clamped, the upper four only
    // where there are more than four splits), then its arithmetic in its order with the contraction ITS listings show, in both builds:
    // w = l * e, L = fma(l, e, L), acc = fma(w, O, acc), o = f2op(acc * (1 / L)).  Thread (row = tid / 8, c8 = tid % 8) owns the 16-byte
    // chunk c8 of every 64-wide k image of its row.  These loads are the newest on the in-order counter: the compiler's wait for them
    // covers the DMA pieces too, and the loop's own wait_vmcnt<0> + barrier then orders the image stores for every wave.
#pragma clang fp contract(off)
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    constexpr int G = 8, KI = MD / BK;
    const int mrow = tid >> 3, c8 = tid & 7;
    const int64_t mg = min(m0 + mrow, (int64_t)p.M - 1);
    f32x2_ ml[G];
    op16x8 t[G][KI];
    auto load = [&](int u) {
      const int64_t at = (int64_t)min(u, p.splits - 1) * p.M + mg;
      ml[u] = *reinterpret_cast<const f32x2_*>(p.ML + at * 2);
#pragma unroll
      for (int i = 0; i < KI; ++i) t[u][i] = *reinterpret_cast<const op16x8*>(p.P + at * MD + i * BK + c8 * 8);
    };
#pragma unroll
    for (int u = 0; u < G / 2; ++u) load(u);
    if (p.splits > G / 2) {
#pragma unroll
      for (int u = G / 2; u < G; ++u) load(u);
    } else {
#pragma unroll
      for (int u = G / 2; u < G; ++u) {
        ml[u] = ml[0];
#pragma unroll
        for (int i = 0; i < KI; ++i) t[u][i] = t[0][i];
      }
    }
    float Mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < G; ++u)
      if (u < p.splits) Mx = fmaxf(Mx, ml[u][0]);
    float L = 0.f, macc[KI][8];
#pragma unroll
    for (int i = 0; i < KI; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) macc[i][e] = 0.f;
#pragma unroll
    for (int u = 0; u < G; ++u) {
      if (u < p.splits && ml[u][0] != -INFINITY) {
        const float ex = __builtin_amdgcn_exp2f(ml[u][0] - Mx);
        const float w = ml[u][1] * ex;
        L = __builtin_fmaf(ml[u][1], ex, L);
#pragma unroll
        for (int i = 0; i < KI; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) macc[i][e] = __builtin_fmaf(w, op2f(t[u][i][e]), macc[i][e]);
      }
    }
    const float inv = 1.f / L;
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      op16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2op(macc[i][e] * inv);
      *reinterpret_cast<op16x8*>(lds + i * A_BYTES + mrow * Img::ROW_BYTES + ((c8 ^ Img::swz(mrow)) << 4)) = o;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the image stores have left this wave before it meets the first barrier
  }
  for (int kt = 0; kt < nk; ++kt) {
    wait_vmcnt<0>();                                     // this wave's 7 pieces of tile kt (and everything older) have landed
    __builtin_amdgcn_s_barrier();                        // tile kt visible to all waves; the stage of tile kt - 1 is no longer read
    if (kt + 1 < nk) issue(kt + 1);
    const unsigned char* sb = ring + (kt % NST) * STAGE_BYTES;
    const unsigned char* sa = MERGED ? lds + kt * A_BYTES : sb;   // merged: the resident image of this k-step
    op16x8 af[T::KS], bfr[T::KS][FN];
    rowtile_read_fragments<N>(af, bfr, sa, sb, offA, swzA, offB, swzB, h);
    ROWTILE_MFMAS(N, acc, af, bfr);
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();                          // every wave is past its last fragment read: the ring is dead

  ROWTILE_EPILOGUE(N, false, p, lds, m0, acc, bias_j);
#endif
}

template <int N, int MD>
static int launch_rowln(const RowLnParams& p, void* stream, const char* what) {
  constexpr int LDS = (MD / 64) * 8192 + 2 * ((MD ? 0 : 64) + N) * 64 * 2;   // resident A images (merged) + the two stages of the ring
  ensure_dyn_lds<gemm_rowln_kernel<N, MD>>(LDS);
  hipLaunchKernelGGL((gemm_rowln_kernel<N, MD>), dim3(cdiv(p.M, 64)), dim3(512), LDS, (hipStream_t)stream, p);
  return msam2_check_launch(what);
}

// N = 384: every K % 64 == 0 (Hiera stage 3).  N = 256: the three reduction lengths of the memory attention's layers (the attention
// out-projection, the value-folded one, linear2); other K at this width are not instantiated paths of the product and stay refused.
extern "C" int msam2_gemm_residual_layernorm_supported(int64_t N, int64_t K) {
  if (N == 384) return (K > 0 && K % 64 == 0) ? 1 : 0;
  if (N == 256) return (K == 64 || K == 256 || K == 2048) ? 1 : 0;
  return 0;
}

extern "C" int msam2_gemm_residual_layernorm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* R32,
                                             int64_t ldr, float* C32, int64_t ldc, const float* ln_w, const float* ln_b, float eps, void* Y16,
                                             int64_t ldy, int64_t M, int64_t N, int64_t K, void* stream) {
  MSAM2_REQUIRE(A && W && R32 && C32 && ln_w && ln_b && Y16, "gemm_residual_layernorm: null operand");
  MSAM2_REQUIRE(msam2_gemm_residual_layernorm_supported(N, K),
                "gemm_residual_layernorm: N=%lld K=%lld is not built (N = 384 with K %% 64 == 0; N = 256 with K = 64, 256 or 2048)", (long long)N,
                (long long)K);
  const RowTileOut o = {R32, ldr, C32, ldc, ln_w, ln_b, eps, Y16, ldy, M};
  const auto own = [&] {
    MSAM2_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "gemm_residual_layernorm: lda, ldw must be multiples of 8 (16-byte rows), >= K");
    return 0;
  };
  if (const int err = rowtile_check("gemm_residual_layernorm", o, N, own, {A, W}, {bias}, "A, W, bias", {{M, lda}, {N, ldw}}, "A / W")) return err;
  RowLnParams p = {};
  p.A = (const op16*)A; p.W = (const op16*)W; p.bias = bias;
  p.lda = lda; p.ldw = ldw; p.K = (int)K;
  rowtile_fill_out(p, o);
  if (N == 384) return launch_rowln<384, 0>(p, stream, "gemm_residual_layernorm");
  return launch_rowln<256, 0>(p, stream, "gemm_residual_layernorm");
}

extern "C" size_t msam2_attention_workspace_bytes(int64_t Bz, int64_t H, int64_t Lq, int64_t D, int splits);

extern "C" int msam2_gemm_merged_residual_layernorm_supported(int64_t N, int64_t D, int splits) {
  return (N == 256 && (D == 64 || D == 256) && splits >= 2 && splits <= 8) ? 1 : 0;
}

// msam2_gemm_residual_layernorm whose A[M, D] is the merge of `splits` split-KV partials: `workspace` is what an attention call with a
// negative split count left behind for one head and M = B * Lq query rows (msam2_attention_workspace_bytes(B, 1, Lq, D, splits), splits =
// the EFFECTIVE count).  The merged rows exist in LDS only.
extern "C" int msam2_gemm_merged_residual_layernorm(const void* workspace, size_t workspace_bytes, int splits, int64_t D, const void* W,
                                                    int64_t ldw, const float* bias, const float* R32, int64_t ldr, float* C32, int64_t ldc,
                                                    const float* ln_w, const float* ln_b, float eps, void* Y16, int64_t ldy, int64_t M,
                                                    int64_t N, void* stream) {
  MSAM2_REQUIRE(workspace && W && R32 && C32 && ln_w && ln_b && Y16, "gemm_merged_residual_layernorm: null operand");
  MSAM2_REQUIRE(splits >= 2 && splits <= 8, "gemm_merged_residual_layernorm: splits=%d outside [2, 8]", splits);
  MSAM2_REQUIRE(D == 64 || D == 256, "gemm_merged_residual_layernorm: D=%lld is not built (64, 256)", (long long)D);
  MSAM2_REQUIRE(N == 256, "gemm_merged_residual_layernorm: N=%lld is not built (256)", (long long)N);
  const RowTileOut o = {R32, ldr, C32, ldc, ln_w, ln_b, eps, Y16, ldy, M};
  const auto own = [&] {
    const size_t need = msam2_attention_workspace_bytes(1, 1, M, D, splits);
    MSAM2_REQUIRE(workspace_bytes >= need, "gemm_merged_residual_layernorm: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
    MSAM2_REQUIRE(ldw % 8 == 0 && ldw >= D, "gemm_merged_residual_layernorm: ldw must be a multiple of 8 (16-byte rows), >= D");
    return 0;
  };
  if (const int err = rowtile_check("gemm_merged_residual_layernorm", o, N, own, {workspace, W}, {bias}, "workspace, W, bias", {{N, ldw}}, "W")) return err;
  RowLnParams p = {};
  p.W = (const op16*)W; p.bias = bias;
  p.ldw = ldw; p.K = (int)D;
  rowtile_fill_out(p, o);
  p.P = (const op16*)workspace;
  p.ML = reinterpret_cast<const float*>(p.P + (size_t)splits * M * D);
  p.splits = splits;
  if (D == 64) return launch_rowln<256, 64>(p, stream, "gemm_merged_residual_layernorm");
  return launch_rowln<256, 256>(p, stream, "gemm_merged_residual_layernorm");
}
