// The MLP of a Hiera stage-3 block with the residual add and the NEXT LayerNorm, as ONE kernel on gemm_rowln_kernel's tile (mlp_rowln_kernel):
//
//   C32[M, N] = GELU(A[M, N] W1[H, N]^T + b1) (rounded to the operand type) W2[N, H]^T + b2 + R32[M, N]     (fp32: the residual stream)
//   Y16[M, N] = LayerNorm(C32 rows; gamma, beta, eps)                                                      (optional: null Y = no rows)
//
// The two launches it replaces (gemm_wstat_kernel with the GELU epilogue, gemm_rowln_kernel<384, 0> at K = H) meet in memory: fc1 writes a
// 16-bit [M, H] hidden map (50 MB at M = 16384, H = 1536) that fc2 reads back through the Infinity Cache.  Here the hidden
// map exists in LDS only, 128 units at a time:
//
//   * cdiv(M, 64) workgroups through xcd_tile_order, 512 threads: 8 waves = 2 row slabs (ws) x 4 column quarters (wq), two per SIMD;
//   * LDS, 160 KB: [six resident DmaImage<128> images of the 64 x N norm2 rows, 48 KB | the hidden image of one chunk, 64 x 128 as two
//     images, 16 KB | a ring of two 48 KB weight stages].  The A rows are loaded once by LDS-DMA, 6 pieces per wave;
//   * the hidden dimension is walked in chunks of 128 units, ascending; a chunk is four ring stages of 48 pieces (6 per wave):
//       t = 0, 1  W1 rows 128 c .. 128 c + 127, k 0 - 191 and k 192 - 383, as three [128 rows][64 k] images each.  fc1 is computed
//                 TRANSPOSED: the wave's 32 W1 rows (32 wq ..) are the MFMA's A operand and its 32 token rows (32 ws ..) the B operand, so
//                 its one accumulator holds, in lane (r, h) and register e, hidden unit s_frag_key(e, h) of token r: four consecutive
//                 units per register group.  24 MFMAs, k ascending in 16-wide steps with gemm_glds_kernel's operand map (lane half h holds
//                 chunk 2 ks + h): the sums of the fc1 GEMM kernels.  Behind the last one: + b1, gelu_erf2, f2op, four 8-byte stores into
//                 the hidden image;
//       t = 2, 3  W2's 384 rows x 64 k (k = hidden 128 c + 64 (t - 2) ..): gemm_rowln_kernel's stage and its k-step, A = the hidden image.
//                 Chunks ascend, so each of the wave's three C accumulators sees the hidden index ascending in 16-wide steps: the order of
//                 gemm_rowln_kernel<384, 0> at K = H, and C32 has its bits;
//   * the ring runs across chunks without a break: stage s + 1 is issued right behind the barrier of stage s (which frees the buffer stage
//     s - 1 was read from), so chunk c + 1's first W1 stage streams under chunk c's last fc2 step.  One counter discipline, as in
//     gemm_rowln.hip: vmcnt(0) before every stage barrier.  At that point the only vector-memory operations of the wave in flight are the
//     six pieces of the stage about to be read (the next stage is issued BEHIND the barrier) and, at t = 1, the chunk's four b1 loads
//     issued one stage earlier: nothing that should stay in flight is waited for, so there is no counted wait to get wrong;
//   * the hidden image is single: it is written at the end of stage 4 c + 1 and read in stages 4 c + 2 and 4 c + 3.  The barrier of stage
//     4 c + 2 (behind a workgroup release fence) publishes it; the barriers of stages 4 c + 4 and 4 c + 5 lie between its last read and
//     the next chunk's stores;
//   * W prefetch (gemm_rowln_kernel found it decisive): before stage 0 every workgroup sends its 1 / 32 of W1 and of W2 (j = its place
//     among the 32 workgroups of its XCD) through throw-away pieces into the ring's second stage, so both weights are on their way into
//     the XCD's L2 at once.  They are older than stage 0 and land before the first barrier lets anybody fill that stage;
//   * epilogue: gemm_rowln_kernel<384, 0>'s (tile [64][N + 4] fp32 aliasing the LDS behind the last barrier; (acc + bias) + r;
//     layernorm_kernel's expressions in its order), with a null Y ending the kernel behind the fp32 rows.
// The tile's constants (RowTile<N>), the W prefetch, fc2's fragment reads and MFMAs and the epilogue are rowtile.h's, ONE text for this
// kernel and gemm_rowln_kernel; so are the refusals and the params fill of the C entry (rowtile_check, rowtile_fill_out).  Here: the
// resident A images, the hidden image, `issue`, fc1, the chunk loop.
// Rows past M are clamped on load and masked on store.  Every wave runs the same number of barriers (4 H / 128 + 2).
// H is a run-time multiple of 128; N = 384 is the template constant.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage): 166 VGPRs, 75 SGPRs in the fp16 build, 164 / 74 in the bf16 build, no scratch: two
// waves per SIMD; one workgroup per CU by its 160 KB of LDS.
// Measured at 16384 x 384 x 1536 (profiles/mlp_rowln_ladder.txt): 62 - 64 us alone against 78 - 84 us for the pair back to
// back.  The removal ladder puts the skeleton -- barriers, fragment reads, prologue, epilogue, no MFMA, no GELU, no weight stream behind
// chunk 0 -- at 49 us, the MFMAs at 3.5, the GELU at 5, the weight stream at 8: the parts ADD UP, the eight waves being in the same phase of a
// stage at the same time.  Tried and not kept: fc1's token fragments resident in 96 registers (244 VGPRs; the skeleton fell to 40 us, the
// kernel stayed at 60 - 64).
#include "rowtile.h"

struct MlpRowLnParams {
  const op16* A;         // [M, N] norm2 rows
  const op16* W1;        // [H, N]
  const op16* W2;        // [N, H]
  const float* b1;       // [H] or null
  const float* b2;       // [N] or null
  const float* R;        // [M, N] fp32 residual
  float* C;              // [M, N] fp32
  const float* ln_w;
  const float* ln_b;
  op16* Y;               // [M, N] LayerNorm(C rows), or null
  int64_t lda, ldw1, ldw2, ldr, ldc, ldy;
  int M, H;
  float eps;
};

// LAD = 0 is the product.  The other instances exist only in a build with -DMSAM2_MLP_ROWLN_LADDER (tools/mlp_rowln_bench.py): each bit REMOVES
// one part of the main loop, for timing only -- 1: the GELU, 2: fc1's MFMAs, 4: fc2's MFMAs, 8: every weight stage behind chunk 0's.
template <int N, int LAD>
__global__ __launch_bounds__(512, 1) void mlp_rowln_kernel(MlpRowLnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Img128 Img;
  typedef RowTile<N> T;
  constexpr int BM = T::BM, BK = T::BK, KS = T::KS, A_BYTES = T::A_BYTES, PPW = T::WPW, FN = T::FN, HC = 128;
  constexpr int KT = N / BK;                         // k images of the A rows: 6
  constexpr int RES_BYTES = KT * A_BYTES;            // 48 KB
  constexpr int HID_BYTES = (HC / BK) * A_BYTES;     // 16 KB
  constexpr int STAGE_BYTES = T::W_BYTES;            // 48 KB: W2's N rows x 64 k, or W1's 128 rows x N / 2 k as KT / 2 images of 16 KB
  constexpr int W1IMG_BYTES = HC * BK * 2;           // 16 KB
  static_assert(N == 384, "one instance: the stage of 48 KB holds W1's 128 rows x 192 k as well as W2's 384 rows x 64 k");
  static_assert((KT / 2) * W1IMG_BYTES == STAGE_BYTES, "a W1 stage is whole images");
  static_assert(T::TILE_BYTES <= RES_BYTES + HID_BYTES + 2 * STAGE_BYTES, "the epilogue tile aliases the images and the ring");
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  unsigned char* const hid = lds + RES_BYTES;
  unsigned char* const ring = hid + HID_BYTES;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int ws = wave >> 2, wq = wave & 3;
  const int r = lane & 31, h = lane >> 5;
  const int64_t m0 = (int64_t)xcd_tile_order(blockIdx.x, gridDim.x) * BM;
  if (m0 >= p.M) return;                             // the whole workgroup, before the first barrier

  float bias_j[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) bias_j[j] = p.b2 ? p.b2[wq * (N / 4) + j * 32 + r] : 0.f;

  const auto a_rsrc = raw_rsrc(p.A);
  const auto w1_rsrc = raw_rsrc(p.W1);
  const auto w2_rsrc = raw_rsrc(p.W2);
  unsigned offsW1[PPW], offsW2[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int q = wave * PPW + i;                    // piece of the stage
    const int row1 = Img::piece_row(q & 15, lane);   // W1: image q / 16 of the stage's three, 16 pieces of 8 rows each
    offsW1[i] = (unsigned)((int64_t)row1 * p.ldw1 * 2 + (q >> 4) * (BK * 2) + Img::src_chunk(row1, lane) * 16);
    const int row2 = Img::piece_row(q, lane);        // W2: one image of N rows
    offsW2[i] = (unsigned)((int64_t)row2 * p.ldw2 * 2 + Img::src_chunk(row2, lane) * 16);
  }
  // stage 4 c + t into ring buffer t & 1
  auto issue = [&](int c, int t) __attribute__((always_inline)) {
    unsigned char* base = ring + (t & 1) * STAGE_BYTES + wave * (PPW * 1024);
    if ((LAD & 8) && c > 0) return;
    if (t < 2) {
      const unsigned so = (unsigned)((int64_t)c * HC * p.ldw1 * 2) + (unsigned)t * (N / 2) * 2;
#pragma unroll
      for (int i = 0; i < PPW; ++i) glds16(w1_rsrc, base + i * 1024, offsW1[i], so);
    } else {
      const unsigned so = (unsigned)(c * HC + (t - 2) * BK) * 2;
#pragma unroll
      for (int i = 0; i < PPW; ++i) glds16(w2_rsrc, base + i * 1024, offsW2[i], so);
    }
  };

  {
    // the A rows: piece `wave` (rows 8 wave ..) of each of the KT resident images
    const int row = Img::piece_row(wave, lane);
    const unsigned offsA = (unsigned)(min(m0 + row, (int64_t)p.M - 1) * p.lda * 2 + Img::src_chunk(row, lane) * 16);
#pragma unroll
    for (int i = 0; i < KT; ++i) glds16(a_rsrc, lds + i * A_BYTES + wave * 1024, offsA, (unsigned)i * BK * 2);
  }
  {
    // this workgroup's share of both weights (W1 rows j H / 32 .., W2 rows j N / 32 .., j = its place among the 32 workgroups of its XCD)
    // into the XCD's L2, through throw-away pieces into the ring's second buffer: older than stage 0
    const int j = (blockIdx.x >> 3) & 31;
    unsigned char* dst = ring + STAGE_BYTES + wave * 1024;
    ROWTILE_PREFETCH_W(w1_rsrc, p.ldw1, p.H >> 5, N >> 3, j, dst);
    ROWTILE_PREFETCH_W(w2_rsrc, p.ldw2, N / 32, p.H >> 3, j, dst);
  }

  f32x16 acc[FN];
  zero_acc(acc);

  // fragment read offsets (bytes) inside an image, without the k-substep term
  const int ra = ws * 32 + r;                        // token row: fc1's B operand, fc2's A operand
  const int offA = ra * Img::ROW_BYTES, swzA = Img::swz(ra);
  const int r1 = wq * 32 + r;                        // W1 row of the chunk: fc1's A operand
  const int offW1 = r1 * Img::ROW_BYTES, swzW1 = Img::swz(r1);
  int offB[FN], swzB[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int rb = wq * (N / 4) + j * 32 + r;
    offB[j] = rb * Img::ROW_BYTES;
    swzB[j] = Img::swz(rb);
  }
  // where this lane's hidden units 32 wq + 8 g + 4 h .. + 3 of token ra go: image wq / 2, 16-byte chunk 4 (wq & 1) + g, half h
  unsigned char* const hdst = hid + (wq >> 1) * A_BYTES + offA + 8 * h;
  const int hc0 = (wq & 1) * 4;

  f32x16 acc1;
  f32x4 b1v[4];
  // fc1, half t of the chunk: k images 3 t .. 3 t + 2 from ring buffer t
  auto fc1_half = [&](int t) __attribute__((always_inline)) {
    const unsigned char* sb = ring + (t & 1) * STAGE_BYTES;
#pragma unroll
    for (int kl = 0; kl < KT / 2; ++kl) {
      const unsigned char* sw = sb + kl * W1IMG_BYTES;
      const unsigned char* sx = lds + (t * (KT / 2) + kl) * A_BYTES;
      op16x8 wf[KS], xf[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int c = 2 * ks + h;
        wf[ks] = *reinterpret_cast<const op16x8*>(sw + offW1 + ((c ^ swzW1) << 4));
        xf[ks] = *reinterpret_cast<const op16x8*>(sx + offA + ((c ^ swzA) << 4));
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (LAD & 2) acc1[ks] += op2f(wf[ks][0]) + op2f(xf[ks][0]);   // keeps the fragment reads alive
        else acc1 = MSAM2_MFMA_32x32x16(wf[ks], xf[ks], acc1, 0, 0, 0);
      }
    }
  };
  // one k-step of fc2: hidden image u against ring buffer u
  auto fc2_step = [&](int u) __attribute__((always_inline)) {
    const unsigned char* sb = ring + u * STAGE_BYTES;
    const unsigned char* sa = hid + u * A_BYTES;
    op16x8 af[KS], bfr[KS][FN];
    rowtile_read_fragments<N>(af, bfr, sa, sb, offA, swzA, offB, swzB, h);
    if constexpr (LAD & 4) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[j][ks] += op2f(af[ks][0]) + op2f(bfr[ks][j][0]);   // keeps the fragment reads alive
    } else {
      ROWTILE_MFMAS(N, acc, af, bfr);
    }
  };

  const int nc = p.H / HC;
  issue(0, 0);
  for (int c = 0; c < nc; ++c) {
    // ---- t = 0: W1, k 0 .. 191
    wait_vmcnt<0>();                                     // this wave's pieces of the stage (and everything older) have landed
    __builtin_amdgcn_s_barrier();                        // the stage is visible to all waves; the other buffer is no longer read
    issue(c, 1);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      b1v[g] = p.b1 ? *reinterpret_cast<const f32x4*>(p.b1 + c * HC + wq * 32 + 8 * g + 4 * h) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 16; ++e) acc1[e] = 0.f;
    fc1_half(0);
    // ---- t = 1: W1, k 192 .. 383; then the activation into the hidden image
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    issue(c, 2);
    fc1_half(1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x2 g0 = f32x2{acc1[4 * g] + b1v[g][0], acc1[4 * g + 1] + b1v[g][1]};
      f32x2 g1 = f32x2{acc1[4 * g + 2] + b1v[g][2], acc1[4 * g + 3] + b1v[g][3]};
      if constexpr (!(LAD & 1)) {
        g0 = gelu_erf2(g0);
        g1 = gelu_erf2(g1);
      }
      op16x4 o;
      o[0] = f2op(g0[0]);
      o[1] = f2op(g0[1]);
      o[2] = f2op(g1[0]);
      o[3] = f2op(g1[1]);
      *reinterpret_cast<op16x4*>(hdst + (((hc0 + g) ^ swzA) << 4)) = o;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the hidden stores have left this wave before it meets the next barrier
    // ---- t = 2, 3: W2, hidden k 128 c .. + 63 and + 64 .. + 127
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    issue(c, 3);
    fc2_step(0);
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (c + 1 < nc) issue(c + 1, 0);
    fc2_step(1);
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();                          // every wave is past its last fragment read: images and ring are dead

  ROWTILE_EPILOGUE(N, true, p, lds, m0, acc, bias_j);
#endif
}

template <int LAD>
static int launch_mlp_rowln(const MlpRowLnParams& p, void* stream) {
  constexpr int LDS = 160 * 1024;   // A images 48 KB + hidden image 16 KB + two stages of 48 KB: all a workgroup may have
  ensure_dyn_lds<mlp_rowln_kernel<384, LAD>>(LDS);
  hipLaunchKernelGGL((mlp_rowln_kernel<384, LAD>), dim3(cdiv(p.M, 64)), dim3(512), LDS, (hipStream_t)stream, p);
  return msam2_check_launch("mlp_residual_layernorm");
}

// N = 384 (Hiera stage 3) with any hidden width that is a whole number of 128-unit chunks
extern "C" int msam2_mlp_residual_layernorm_supported(int64_t N, int64_t H) { return (N == 384 && H > 0 && H % 128 == 0) ? 1 : 0; }

extern "C" int msam2_mlp_residual_layernorm_fwd(const void* A, int64_t lda, const void* W1, int64_t ldw1, const float* b1, const void* W2,
                                                int64_t ldw2, const float* b2, const float* R32, int64_t ldr, float* C32, int64_t ldc,
                                                const float* ln_w, const float* ln_b, float eps, void* Y16, int64_t ldy, int64_t M, int64_t N,
                                                int64_t H, void* stream) {
  MSAM2_REQUIRE(A && W1 && W2 && R32 && C32, "mlp_residual_layernorm: null operand");
  MSAM2_REQUIRE(!Y16 || (ln_w && ln_b), "mlp_residual_layernorm: LayerNorm rows asked for without ln_w, ln_b");
  MSAM2_REQUIRE(msam2_mlp_residual_layernorm_supported(N, H), "mlp_residual_layernorm: N=%lld H=%lld is not built (N = 384 with H %% 128 == 0)",
                (long long)N, (long long)H);
  const RowTileOut o = {R32, ldr, C32, ldc, ln_w, ln_b, eps, Y16, ldy, M};
  const auto own = [&] {
    MSAM2_REQUIRE(lda % 8 == 0 && ldw1 % 8 == 0 && ldw2 % 8 == 0 && lda >= N && ldw1 >= N && ldw2 >= H,
                  "mlp_residual_layernorm: lda, ldw1, ldw2 must be multiples of 8 (16-byte rows), lda, ldw1 >= N, ldw2 >= H");
    return 0;
  };
  if (const int err = rowtile_check("mlp_residual_layernorm", o, N, own, {A, W1, W2}, {b1, b2}, "A, W1, W2, b1, b2",
                                    {{M, lda}, {H, ldw1}, {N, ldw2}}, "A / W1 / W2"))
    return err;
  MlpRowLnParams p = {};
  p.A = (const op16*)A; p.W1 = (const op16*)W1; p.W2 = (const op16*)W2; p.b1 = b1; p.b2 = b2;
  p.lda = lda; p.ldw1 = ldw1; p.ldw2 = ldw2; p.H = (int)H;
  rowtile_fill_out(p, o);
  return launch_mlp_rowln<0>(p, stream);
}

#ifdef MSAM2_MLP_ROWLN_LADDER
// timing only (tools/mlp_rowln_bench.py): the product's launch with parts of the main loop removed; the results mean nothing.  Not part
// of the ABI (include/msam2_hip.h): the block form keeps tools/gen_header.py from listing it
extern "C" {
int msam2_mlp_rowln_ladder(int lad, const void* A, const void* W1, const void* W2, const float* R32, float* C32, const float* ln_w,
                                      const float* ln_b, void* Y16, int64_t M, int64_t H, void* stream) {
  MSAM2_REQUIRE(A && W1 && W2 && R32 && C32 && ln_w && ln_b && Y16 && M > 0 && H > 0 && H % 128 == 0, "mlp_rowln_ladder: operands");
  MlpRowLnParams p = {};
  p.A = (const op16*)A; p.W1 = (const op16*)W1; p.W2 = (const op16*)W2;
  p.lda = 384; p.ldw1 = 384; p.ldw2 = H; p.H = (int)H;
  rowtile_fill_out(p, RowTileOut{R32, 384, C32, 384, ln_w, ln_b, 1e-6f, Y16, 384, M});
  switch (lad) {
    case 0: return launch_mlp_rowln<0>(p, stream);
    case 1: return launch_mlp_rowln<1>(p, stream);
    case 2: return launch_mlp_rowln<3>(p, stream);
    case 3: return launch_mlp_rowln<4>(p, stream);
    case 4: return launch_mlp_rowln<7>(p, stream);
    case 5: return launch_mlp_rowln<15>(p, stream);
    case 6: return launch_mlp_rowln<8>(p, stream);
    default: MSAM2_REQUIRE(false, "mlp_rowln_ladder: variant %d", lad);
  }
}
}
#endif
