// Fused pre-LN MLP block of the Hiera trunk for gfx950:   out = x + fc2( GELU( fc1( LayerNorm(x) ) ) )      (hieradet.py:166-167,
// sam2_utils.py:108-132 with nn.GELU, LayerNorm eps 1e-6)
//
// Why one kernel.  At the two high-resolution stages (dim 96 / 192, 262144 / 65536 tokens at 4 x 1024^2) the three launches of the block --
// LayerNorm, fc1 + GELU, fc2 + residual -- are bound by what they move, not by what they compute: the 4 x dim hidden activation
// (201 MB at stage 1) is written and read back once, the LayerNorm output once more, and K = 96 / 192 GEMMs spend their life in prologue
// and epilogue.  Here the hidden activation never leaves the registers:
//
//   * everything is computed TRANSPOSED so that a lane owns one token: H^T = W1 X^T (A = W1 rows from LDS, B = the token's normalised
//     row held in registers), then Y^T += W2 H^T where the fp32 accumulator of H^T, after bias + GELU + conversion, IS the B operand
//     (the accumulator of a 32x32x16 MFMA has the token on the lane and 8 consecutive k per register group: no LDS round trip, no
//     shuffle); the k order of that operand is permuted, so W2 is given with its hidden dimension pre-permuted the same way (host);
//   * a wave carries TB blocks of 32 tokens through the whole hidden dimension, so every weight fragment read from LDS feeds TB (fc1)
//     MFMAs: LDS traffic per MFMA is well under the 1 KB of the 128 x 128 GEMM tiles;
//   * the weights stream through LDS in hidden-dimension chunks of HC (both W1 rows and W2 columns of a chunk: 72 KB), double
//     buffered by LDS-DMA (buffer_load ... lds) one chunk ahead, ONE barrier per chunk; workgroups are persistent over token passes
//     and the chunk ring runs on across passes;
//   * LayerNorm runs on the lane's half row (the other half sits 32 lanes away: one cross-half add), the residual is added in the
//     store.
// LDS images: rows of 192 B use chunk' = (c & ~3) | ((c & 3) ^ ((r >> 2) & 3)), rows of 384 B chunk' = (c & ~7) | ((c & 7) ^ ((r >> 1) & 7))
// (both conflict free for the 32-row ds_read_b128 fragment reads); applied on the DMA source address and on the reads.  Not the images of
// common.h's DmaImage: a row is 12 / 24 chunks long and the swizzle permutes inside groups of 4 / 8 of them.
#include "common.h"

// Lanes l and l + 32 trade one op16x4 each: given a (the lower half keeps it) and b (the upper half keeps it), lanes 0-31 return
// (own a, partner's a), lanes 32-63 (partner's b, own b).  v_permlane32_swap exchanges the first operand's upper-half lanes with the
// second's lower-half lanes.
__device__ __forceinline__ op16x8 half_trade(op16x4 a, op16x4 b) {
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const auto sw = __builtin_amdgcn_permlane32_swap(ua[i], ub[i], false, false);
    r[i] = sw[0];
    r[2 + i] = sw[1];
  }
  return __builtin_bit_cast(op16x8, r);
}

struct MlpFusedParams {
  const float* x;        // [T, DIM] fp32 residual stream
  float* out;            // [T, DIM]
  const float *ln_w, *ln_b, *b1, *b2;
  const op16* w1;        // [4*DIM, DIM]
  const op16* w2p;       // [DIM, 4*DIM], hidden index permuted inside every 32-block (see mlp_fused_permute)
  int64_t T;
  float eps;
  op16* out16;           // optional second output: the same rows in the 16-bit operand type (a stage's last block: the FPN's lateral GEMM operand)
  // PROJ form only (the attention's output projection in front, x = the projection's residual):
  const op16* o;         // [T, DIM] attention output
  const op16* wp;        // [DIM, DIM] proj weight (nn.Linear layout)
  const float* bp;
  const float *nln_w, *nln_b;   // optional third output: LayerNorm(out rows; nln_w, nln_b, neps) in the 16-bit operand type (the next block's norm1)
  float neps;
  op16* xn16;
};

// NWV waves per workgroup (4 or 8).  With 8 (round 4) the workgroup still owns ONE weight ring in LDS, a wave carries TB = half as many
// token blocks, and every SIMD holds two waves: one wave's GELU / LayerNorm vector work and LDS reads run under the other's MFMAs, and a
// wave's registers (<= 256) no longer spill (the 4-wave form at dim 192 spilled 21-35 registers of a 512-register budget).
//
// PROJ: the block's attention output projection runs in front, x1 = res + o Wp^T + bp never exists in memory.  The fc2
// accumulator accy is initialised with res + bp and takes Wp o^T as DB * KS1 more MFMAs (A = Wp rows, B = the token's o row, one 16-byte
// load per k-step); LayerNorm then runs on accy, whose registers, rounded, ARE fc1's B operand -- in the accumulator's channel order, so
// W1 comes with its input dimension permuted like W2's hidden one (msam2_mlp_fused_permute_w1).  The fc1 / GELU / fc2 loop is the same
// and accumulates onto x1; the store adds b2 and re-reads nothing (in place is fine).  Wp: resident form (dim 96, LDS full) -- fragments
// straight from global memory, 18 KB that stay in L1 / L2; streaming form (dim 192) -- Wp is exactly one ring slot (72 KB), one more ring
// step at the head of every pass.  Optionally the store also writes LayerNorm(out rows) for the next block's norm1.  SIDE (PROJ only):
// which 16-bit side outputs the store writes, bit 0 out16, bit 1 xn16 -- compile-time, so that the store is one straight run of
// instructions (as run-time tests every store sat in a basic block of its own).
template <int DIM, int HC, int TB, int OCC = 1, int NWV = 4, bool PROJ = false, int SIDE = 0>
__global__ __launch_bounds__(NWV * 64, OCC) void mlp_fused_kernel(MlpFusedParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int HID = 4 * DIM, NCH = HID / HC, KS1 = DIM / 16, DB = DIM / 32, HB = HC / 32;
  constexpr int RB1 = DIM * 2, RB2 = HC * 2;                 // LDS row bytes of the W1 chunk [HC][DIM] and the W2 chunk [DIM][HC]
  constexpr int CPR1 = DIM / 8, CPR2 = HC / 8;               // 16-byte chunks per row
  constexpr int W1B = HC * RB1, W2B = DIM * RB2, BUF = W1B + W2B;
  constexpr int PIECES1 = W1B / 1024, PIECES2 = W2B / 1024, PW1 = (PIECES1 + NWV - 1) / NWV, PW2 = (PIECES2 + NWV - 1) / NWV;
  static_assert((RB1 == 192 || RB1 == 384) && (RB2 == 192 || RB2 == 384), "row swizzles are built for 192 / 384-byte rows");
  static_assert(2 * BUF + (3 * DIM + HID + (PROJ ? 3 * DIM : 0)) * 4 <= 160 * 1024, "LDS budget");   // (pieces are dealt j * NWV + wave: a last, partial round is guarded)
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  float* prm = reinterpret_cast<float*>(smem + 2 * BUF);     // [gamma DIM | beta DIM | b2 DIM | b1 HID], PROJ: [| bp DIM | next gamma DIM | next beta DIM]
  constexpr int PRM_BP = 3 * DIM + HID, PRM_NG = PRM_BP + DIM, PRM_NB = PRM_NG + DIM;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  for (int i = tid; i < DIM; i += NWV * 64) {
    prm[i] = p.ln_w[i];
    prm[DIM + i] = p.ln_b[i];
    prm[2 * DIM + i] = p.b2[i];
  }
  for (int i = tid; i < HID; i += NWV * 64) prm[3 * DIM + i] = p.b1[i];
  if constexpr (PROJ)
    for (int i = tid; i < DIM; i += NWV * 64) {
      prm[PRM_BP + i] = p.bp[i];
      if constexpr (SIDE & 2) {
        prm[PRM_NG + i] = p.nln_w[i];
        prm[PRM_NB + i] = p.nln_b[i];
      }
    }

  // ---- weight stream: per-lane source offsets of this wave's DMA pieces (chunk-independent part), scalar chunk offset added per issue
  const auto w1_rsrc = raw_rsrc(p.w1, HID * DIM * 2);
  const auto w2_rsrc = raw_rsrc(p.w2p, HID * DIM * 2);
  unsigned off1[PW1], off2[PW2];
#pragma unroll
  for (int j = 0; j < PW1; ++j) {
    const int f = min(j * NWV + wave, PIECES1 - 1) * 64 + lane, row = f / CPR1, c = f % CPR1;
    off1[j] = (unsigned)(row * RB1 + mlp_swz<RB1>(c, row) * 16);                       // W1 rows are DIM * 2 bytes in memory too
  }
#pragma unroll
  for (int j = 0; j < PW2; ++j) {
    const int f = min(j * NWV + wave, PIECES2 - 1) * 64 + lane, row = f / CPR2, c = f % CPR2;
    off2[j] = (unsigned)(row * HID * 2 + mlp_swz<RB2>(c, row) * 16);
  }
  auto issue = [&](int chunk, int buf) {
    unsigned char* d1 = smem + buf * BUF;
    unsigned char* d2 = smem + buf * BUF + W1B;
    const unsigned s1 = (unsigned)chunk * HC * RB1, s2 = (unsigned)chunk * HC * 2;
#pragma unroll
    for (int j = 0; j < PW1; ++j)
      if (j * NWV + wave < PIECES1)
        glds16(w1_rsrc, d1 + (j * NWV + wave) * 1024, off1[j], s1);
#pragma unroll
    for (int j = 0; j < PW2; ++j)
      if (j * NWV + wave < PIECES2)
        glds16(w2_rsrc, d2 + (j * NWV + wave) * 1024, off2[j], s2);
  };

  const int64_t pass_tokens = NWV * 32 * TB;
  const int64_t n_pass = (p.T + pass_tokens - 1) / pass_tokens;
  int64_t g_chunk = 0;                                       // running chunk count of this workgroup (buffer = parity)
  constexpr bool RING_WP = PROJ && !((NCH == 2) && NWV == 8);   // streaming PROJ form: Wp is a ring step of its own in front of chunk 0
  // Wp [DIM][DIM] as a ring step: rows of RB1 bytes like a W1 chunk's, two W1-chunk-shaped halves of HC rows with the same lane offsets
  // (HC rows further down the row swizzle repeats), filling the slot exactly
  auto issue_wp = [&](int buf) {
    if constexpr (RING_WP) {
      static_assert(2 * HC == DIM && W1B == W2B && RB1 == 384 && (HC / 2) % 8 == 0, "Wp = one ring slot, swizzle period divides HC");
      const auto wp_rsrc = raw_rsrc(p.wp, DIM * DIM * 2);
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int j = 0; j < PW1; ++j)
          if (j * NWV + wave < PIECES1)
            glds16(wp_rsrc, smem + buf * BUF + half * W1B + (j * NWV + wave) * 1024, off1[j], (unsigned)(half * W1B));
    }
  };
  // RESIDENT (two chunks = the whole of W1 and W2 fit the two ring buffers: dim 96): both chunks are loaded ONCE and stay; the pass loop
  // then has no DMA, no wait and no barrier, so the 8 waves drift apart and one wave's LayerNorm prologue / store epilogue runs under the
  // others' MFMAs (round 4).  Otherwise the ring streams chunk c + 1 under chunk c, one barrier per chunk.
  constexpr bool RESIDENT = (NCH == 2) && NWV == 8;
  if ((int64_t)blockIdx.x < n_pass) {
    if constexpr (RING_WP) issue_wp(0);
    else issue(0, 0);
    if constexpr (RESIDENT) issue(1, 1);
  }
  if constexpr (RESIDENT) wait_vmcnt<0>();
  __syncthreads();                                           // parameters visible (streaming form: the DMA is waited for inside the loop)

  for (int64_t pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
    op16x8 xf[TB][KS1];
    int64_t tok[TB];
    f32x16 accy[TB][DB];
    if constexpr (PROJ) {
      // ---- x1 = res + bp + Wp o^T in accy: row loads first (res in the accumulator's channel order, o in the operand's)
      op16x8 of[TB][KS1];
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) {
        const int64_t t = pass * pass_tokens + (int64_t)(wave * TB + tb) * 32 + r;
        tok[tb] = t;
        const int64_t tc = t < p.T ? t : p.T - 1;
        const float* xr = p.x + tc * DIM;
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(xr + d * 32 + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) accy[tb][d][4 * g + e] = v[e];
          }
#pragma unroll
        for (int k = 0; k < KS1; ++k) of[tb][k] = *reinterpret_cast<const op16x8*>(p.o + tc * DIM + 16 * k + 8 * h);
      }
      const unsigned char* wps = smem;
      if constexpr (RING_WP) {
        const int buf = (int)(g_chunk & 1);
        wait_vmcnt<0>();     // this wave's pieces of Wp (and its rows) have landed
        __builtin_amdgcn_s_barrier();                        // ... every wave's; the other buffer is no longer read
        issue(0, buf ^ 1);
        wps = smem + buf * BUF;
        ++g_chunk;
      }
      // Wp fragments of d-block d + 1 are requested before the MFMAs of d-block d and no further ahead (all DB * KS1 at once, as the
      // compiler would have them, is 72 registers beside accy's 96 and o's 48)
      auto load_ap = [&](op16x8 (&ap)[KS1], int d) {
        const int rowp = d * 32 + r;
#pragma unroll
        for (int k = 0; k < KS1; ++k) {
          if constexpr (RING_WP) ap[k] = *reinterpret_cast<const op16x8*>(wps + rowp * RB1 + (mlp_swz<RB1>(2 * k + h, rowp) << 4));
          else ap[k] = *reinterpret_cast<const op16x8*>(p.wp + rowp * DIM + 16 * k + 8 * h);
        }
      };
      op16x8 ap[2][KS1];
      load_ap(ap[0], 0);
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        if (d + 1 < DB) load_ap(ap[(d + 1) & 1], d + 1);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(prm + PRM_BP + d * 32 + 8 * g + 4 * h);
#pragma unroll
          for (int tb = 0; tb < TB; ++tb)
#pragma unroll
            for (int e = 0; e < 4; ++e) accy[tb][d][4 * g + e] += bv[e];
        }
#pragma unroll
        for (int tb = 0; tb < TB; ++tb)
#pragma unroll
          for (int k = 0; k < KS1; ++k) accy[tb][d] = MSAM2_MFMA_32x32x16(ap[d & 1][k], of[tb][k], accy[tb][d], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // ---- LayerNorm on accy (the lane's half row + one cross-half add, two passes); registers 0-7 / 8-15 of d-block d, rounded, are
      // k-steps 2d / 2d + 1 of fc1's B operand (W1's input index is permuted to this order)
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) {
        // two independent chains (registers 0-7 / 8-15: the even / odd k-steps the rows become), then one add.  (The order is not free
        // to change: tests/test_amg_gpu.py has two cases that sit ON a discrete decision -- a prompt set with stability 3137 / 3201 =
        // 0.98001 against the threshold 0.98, and an NMS that keeps 3 of ~210 masks against a bar of 3 -- and one chain moves the first,
        // four chains the second)
        float s2[2] = {0.f, 0.f}, q2h[2] = {0.f, 0.f};
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
          for (int e = 0; e < 16; ++e) s2[e >> 3] += accy[tb][d][e];
        float s = s2[0] + s2[1];
        s += __shfl_xor(s, 32, 64);
        const float mean = s * (1.f / DIM);
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float dlt = accy[tb][d][e] - mean;
            q2h[e >> 3] += dlt * dlt;
          }
        float q2 = q2h[0] + q2h[1];
        q2 += __shfl_xor(q2, 32, 64);
        const float rstd = 1.0f / sqrtf(q2 * (1.f / DIM) + p.eps);
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 gm = *reinterpret_cast<const f32x4*>(prm + d * 32 + 8 * g + 4 * h);
            const f32x4 bt = *reinterpret_cast<const f32x4*>(prm + DIM + d * 32 + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              xf[tb][2 * d + (g >> 1)][4 * (g & 1) + e] = f2op((accy[tb][d][4 * g + e] - mean) * rstd * gm[e] + bt[e]);
          }
      }
    } else {
    // ---- this wave's TB token blocks: LayerNorm -> 16-bit B fragments
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      const int64_t t = pass * pass_tokens + (int64_t)(wave * TB + tb) * 32 + r;
      tok[tb] = t;
      const float* xr = p.x + (t < p.T ? t : p.T - 1) * DIM;
      f32x4 v[KS1][2];
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < KS1; ++k)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          v[k][q] = *reinterpret_cast<const f32x4*>(xr + 16 * k + 8 * h + 4 * q);
          s += v[k][q][0] + v[k][q][1] + v[k][q][2] + v[k][q][3];
        }
      s += __shfl_xor(s, 32, 64);
      const float mean = s * (1.f / DIM);
      float q2 = 0.f;
#pragma unroll
      for (int k = 0; k < KS1; ++k)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float dlt = v[k][q][e] - mean;
            q2 += dlt * dlt;
          }
      q2 += __shfl_xor(q2, 32, 64);
      const float rstd = 1.0f / sqrtf(q2 * (1.f / DIM) + p.eps);
#pragma unroll
      for (int k = 0; k < KS1; ++k) {
        op16x8 f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 gm = *reinterpret_cast<const f32x4*>(prm + 16 * k + 8 * h + 4 * q);
          const f32x4 bt = *reinterpret_cast<const f32x4*>(prm + DIM + 16 * k + 8 * h + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) f[4 * q + e] = f2op((v[k][q][e] - mean) * rstd * gm[e] + bt[e]);
        }
        xf[tb][k] = f;
      }
    }
#pragma unroll
    for (int tb = 0; tb < TB; ++tb)
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) accy[tb][d][e] = 0.f;

    }

    for (int chunk = 0; chunk < NCH; ++chunk, ++g_chunk) {
      const int buf = RESIDENT ? chunk : (int)(g_chunk & 1);
      if constexpr (!RESIDENT) {
        wait_vmcnt<0>();     // this wave's pieces of the chunk have landed
        __builtin_amdgcn_s_barrier();                        // ... every wave's; the other buffer is no longer read
        const bool more_here = chunk + 1 < NCH;
        const bool more = more_here || (pass + gridDim.x < n_pass);
        if (more) {
          if (RING_WP && !more_here) issue_wp(buf ^ 1);
          else issue(more_here ? chunk + 1 : 0, buf ^ 1);
        }
      }
      const unsigned char* w1s = smem + buf * BUF;
      const unsigned char* w2s = w1s + W1B;
#pragma unroll 1
      for (int hb = 0; hb < HB; ++hb) {
        // fc1 fragments of this hidden block: read once, used by all TB token blocks
        op16x8 a1[KS1];
        const int row1 = hb * 32 + r;
#pragma unroll
        for (int k = 0; k < KS1; ++k) a1[k] = *reinterpret_cast<const op16x8*>(w1s + row1 * RB1 + (mlp_swz<RB1>(2 * k + h, row1) << 4));
        // bias of the hidden rows this lane holds: (e & 3) + 8 (e >> 2) + 4 h  -> four float4 reads
        f32x4 bias1[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) bias1[g] = *reinterpret_cast<const f32x4*>(prm + 3 * DIM + chunk * HC + hb * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) {
          f32x16 acch;
#pragma unroll
          for (int e = 0; e < 16; ++e) acch[e] = bias1[e >> 2][e & 3];
#pragma unroll
          for (int k = 0; k < KS1; ++k) acch = MSAM2_MFMA_32x32x16(a1[k], xf[tb][k], acch, 0, 0, 0);
          op16x8 hf[2];
#pragma unroll
#ifdef MSAM2_MLP_NO_GELU   // timing experiment only: what the activation costs
          for (int e = 0; e < 16; ++e) hf[e >> 3][e & 7] = f2op(acch[e]);
#else
          for (int e = 0; e < 16; e += 2) {               // pairs: packed fp32 arithmetic (common.h)
            const f32x2 gp = gelu_erf2(f32x2{acch[e], acch[e + 1]});
            hf[e >> 3][e & 7] = f2op(gp[0]);
            hf[e >> 3][(e & 7) + 1] = f2op(gp[1]);
          }
#endif
          // fc2: Y^T[d][token] += W2[d][hidden] H^T[hidden][token]; operand k order = the accumulator's register order (permuted W2)
#pragma unroll
          for (int d = 0; d < DB; ++d) {
            const int row2 = d * 32 + r;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const op16x8 a2 = *reinterpret_cast<const op16x8*>(w2s + row2 * RB2 + (mlp_swz<RB2>(hb * 4 + 2 * s2 + h, row2) << 4));
              accy[tb][d] = MSAM2_MFMA_32x32x16(a2, hf[s2], accy[tb][d], 0, 0, 0);
            }
          }
        }
      }
    }
    if constexpr (PROJ) {
      // ---- epilogue: + b2, fp32 store of the lane's half row from accy (x1 is in it: nothing is re-read); optionally the rows' 16-bit
      // rounding and their LayerNorm with the next block's norm1 parameters (statistics as above, every lane takes part in the adds)
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(prm + 2 * DIM + d * 32 + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              accy[tb][d][4 * g + e] += bv[e];
              s += accy[tb][d][4 * g + e];
            }
          }
        float mean = 0.f, rstd = 0.f;
        if constexpr (SIDE & 2) {
          s += __shfl_xor(s, 32, 64);
          mean = s * (1.f / DIM);
          float q2 = 0.f;
#pragma unroll
          for (int d = 0; d < DB; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const float dlt = accy[tb][d][e] - mean;
              q2 += dlt * dlt;
            }
          q2 += __shfl_xor(q2, 32, 64);
          rstd = 1.0f / sqrtf(q2 * (1.f / DIM) + p.neps);
        }
        if (tok[tb] < p.T) {
          float* yr = p.out + tok[tb] * DIM;
#pragma unroll
          for (int d = 0; d < DB; ++d) {
            if constexpr (SIDE & 2) __builtin_amdgcn_sched_barrier(0);   // one d-block's LayerNorm parameters at a time (all DB at once spill)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int ch = d * 32 + 8 * g + 4 * h;
              f32x4 o;
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = accy[tb][d][4 * g + e];
              *reinterpret_cast<f32x4*>(yr + ch) = o;
            }
            // 16-bit side outputs: a lane's 4 channels of register group g and the other half's 4 are adjacent in the row, so the halves
            // trade (the lower keeps even g, the upper odd g) and every lane stores 8 channels = 16 bytes: half as many scattered stores
            if constexpr (SIDE != 0) {
#pragma unroll
              for (int m = 0; m < 2; ++m) {
                op16x4 lo[2], hi[2];                            // [output: 0 out16, 1 xn16], register groups 2m and 2m + 1
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                  const int g = 2 * m + q, ch = d * 32 + 8 * g + 4 * h;
                  f32x4 gm = {0.f, 0.f, 0.f, 0.f}, bt = gm;
                  if constexpr (SIDE & 2) {
                    gm = *reinterpret_cast<const f32x4*>(prm + PRM_NG + ch);
                    bt = *reinterpret_cast<const f32x4*>(prm + PRM_NB + ch);
                  }
                  op16x4 v16, n16;
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
                    const float o = accy[tb][d][4 * g + e];
                    v16[e] = f2op(o);
                    n16[e] = f2op((o - mean) * rstd * gm[e] + bt[e]);
                  }
                  (q ? hi : lo)[0] = v16;
                  (q ? hi : lo)[1] = n16;
                }
                const int64_t at = tok[tb] * DIM + d * 32 + 16 * m + 8 * h;
                if constexpr (SIDE & 1) *reinterpret_cast<op16x8*>(p.out16 + at) = half_trade(lo[0], hi[0]);
                if constexpr (SIDE & 2) *reinterpret_cast<op16x8*>(p.xn16 + at) = half_trade(lo[1], hi[1]);
              }
            }
          }
        }
      }
    } else {
    // ---- epilogue: + b2 + residual, fp32 store (a lane owns a token; 4 consecutive channels per register group)
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      if (tok[tb] < p.T) {
        const float* xr = p.x + tok[tb] * DIM;
        float* yr = p.out + tok[tb] * DIM;
        // every residual value of the token block is loaded BEFORE its first store (round 4): loads and stores share one in-order
        // counter (vmcnt), so as load / add / store triples each residual load waited for the previous store's round trip -- DB * 4
        // of them per block, one after the other
        constexpr int DG = 1;                             // d-blocks per batch (4 float4 in flight; 3 = 12 float4 spills 19-35 registers and measures no gain: 120 -> 115 us, 82.5 -> 77.9 us with 1)
        static_assert(DB % DG == 0, "d-blocks in whole batches");
#pragma unroll
        for (int d0 = 0; d0 < DB; d0 += DG) {
          f32x4 xv[DG][4];
#pragma unroll
          for (int d = 0; d < DG; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) xv[d][g] = *reinterpret_cast<const f32x4*>(xr + (d0 + d) * 32 + 8 * g + 4 * h);
#pragma unroll
          for (int d = 0; d < DG; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int ch = (d0 + d) * 32 + 8 * g + 4 * h;
              const f32x4 bv = *reinterpret_cast<const f32x4*>(prm + 2 * DIM + ch);
              f32x4 o;
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = accy[tb][d0 + d][4 * g + e] + bv[e] + xv[d][g][e];
              *reinterpret_cast<f32x4*>(yr + ch) = o;
              if (p.out16) {
                op16x4 o2;
#pragma unroll
                for (int e = 0; e < 4; ++e) o2[e] = f2op(o[e]);
                *reinterpret_cast<op16x4*>(p.out16 + tok[tb] * DIM + ch) = o2;
              }
            }
        }
      }
    }
    }
  }
#endif
}

// ------------------------------------------------------------------------------------------------------------------
// dim 384 (Hiera stage 3: 11 blocks of hiera_s, 16384 tokens at 4 x 1024^2).  OPT-IN (MSAM2_MLP_384=1), NOT the default: correct
// (tests/test_kernels_gpu.py::test_ln_mlp_residual_fused, dim 384) and, as it stands, SLOWER than the three launches it would replace
// (LayerNorm 9 + fc1 33 + fc2 32 us in the step; 90 us as an isolated sequence; this kernel 110-118 us).  Why it was built: what bounds the
// two GEMMs is what a CU can take in (~33 GB/s per CU of activations out of the Infinity Cache, ~70 GB/s of weights out of its
// XCD's L2), and the 50 MB hidden map goes out and comes back through exactly that path; fused, a CU takes in 96 KB of activations and the
// 2.36 MB of W1 | W2 from L2 (~33 us at 70 GB/s) and the hidden map never exists.  Why it does not pay yet (removal ladder, round 4,
// 16384 tokens): row loads / residual / store in the token-per-lane layout 23 us, the 36 MFMAs per wave and chunk 41 us, LDS fragment
// reads 20 us, weight DMA issue + landing 18 us, GELU 14 us -- and the parts ADD UP to the kernel's time: with ONE wave per SIMD (the
// 144 KB ring + 96 + 96 row / accumulator registers leave room for no second one) nothing overlaps them; independent MFMA chains,
// read sub-bursts and sched_group_barrier-placed GELU instructions changed the listing and not the time.  What would: a second wave per
// SIMD (needs the fc1 duplication below gone: 8 waves of this split are MFMA-bound at 44 us) and row-major I / O staged through LDS.
//
// Same transposed arithmetic as mlp_fused_kernel (a lane owns a token; the GELU'd fc1 accumulator IS fc2's B operand), other work split:
//   * one workgroup = 64 tokens (256 workgroups at 16384 tokens: one per CU), 4 waves = 2 token blocks x 2 halves of the OUTPUT channels.
//     Both waves of a token block compute the block's fc1 (duplicated: 24 MFMAs) and each accumulates its 6 of the 12 fc2 output blocks
//     (12 MFMAs): 36 MFMAs per wave and 32-unit hidden chunk, 96 accumulator registers instead of 192 -- the whole row state of a wave
//     (96 operand + 96 accumulator registers) fits one SIMD's file;
//   * the weights stream in hidden chunks of 32 units (W1 rows [32][384] = 24 KB, W2 columns [384][32] = 24 KB) through a THREE-slot
//     LDS-DMA ring, two chunks (96 KB) in flight, one barrier per chunk;
//   * W2 is given chunk-major and already in its LDS image (msam2_mlp_fused_permute_w2 at dim 384): its DMA is a linear 24 KB copy of whole
//     128-byte lines (as [384][1536] rows a chunk would be 384 pieces of 64 bytes).
// LDS images: W1 rows of 768 B, 16-byte chunk c of row r at (c & ~15) | ((c & 15) ^ (r & 15)); W2 rows of 64 B = DmaImage<64> (common.h)
// (both conflict free for the 16-lane groups of a 32-row ds_read_b128 fragment read).
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mlp_swz768(int c, int r) { return (c & ~15) | ((c & 15) ^ (r & 15)); }

__global__ __launch_bounds__(256, 1) void mlp_fused384_kernel(MlpFusedParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int DIM = 384, HID = 1536, HC = 32, NCH = HID / HC, KS1 = DIM / 16, DBW = 6, NST = 3;
  constexpr int W1B = HC * DIM * 2, W2B = DIM * HC * 2, BUF = W1B + W2B;   // 24 + 24 KB
  constexpr int PW = W1B / 1024 / 4;                                      // DMA pieces (1 KB) per wave and operand: 6
  static_assert(NST * BUF + (3 * DIM + HID) * 4 <= 160 * 1024, "LDS budget");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  float* prm = reinterpret_cast<float*>(smem + NST * BUF);   // [gamma DIM | beta DIM | b2 DIM | b1 HID]

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int tb = wave >> 1, dh = wave & 1;
  for (int i = tid; i < DIM; i += 256) {
    prm[i] = p.ln_w[i];
    prm[DIM + i] = p.ln_b[i];
    prm[2 * DIM + i] = p.b2[i];
  }
  for (int i = tid; i < HID; i += 256) prm[3 * DIM + i] = p.b1[i];

  // ---- this wave's token block: row loads first (the weight DMAs queue behind them on the in-order counter, not in front)
  const int64_t t = (int64_t)blockIdx.x * 64 + tb * 32 + r;
  const float* xr = p.x + (t < p.T ? t : p.T - 1) * DIM;
  f32x4 v[KS1][2];
#pragma unroll
  for (int k = 0; k < KS1; ++k)
#pragma unroll
    for (int q = 0; q < 2; ++q) v[k][q] = *reinterpret_cast<const f32x4*>(xr + 16 * k + 8 * h + 4 * q);

  // ---- weight stream
  const auto w1_rsrc = raw_rsrc(p.w1, HID * DIM * 2);
  const auto w2_rsrc = raw_rsrc(p.w2p, HID * DIM * 2);
  unsigned off1[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int f = (j * 4 + wave) * 64 + lane, row = f / 48, c = f % 48;
    off1[j] = (unsigned)(row * 768 + mlp_swz768(c, row) * 16);
  }
  const unsigned off2 = (unsigned)(wave * 1024 + lane * 16);
  // ring step i (0 .. NCH) holds W1 chunk i (i < NCH) and W2 chunk i - 1 (i >= 1): fc1 runs ONE chunk ahead of fc2, so the GELU of chunk
  // i - 1 (vector pipe) sits beside the fc1 MFMAs of chunk i instead of between two dependent MFMA groups
  auto issue = [&](int i) {
    unsigned char* d1 = smem + (i % NST) * BUF;
    unsigned char* d2 = d1 + W1B;
    if (i < NCH) {
      const unsigned s = (unsigned)i * W1B;
#pragma unroll
      for (int j = 0; j < PW; ++j)
        glds16(w1_rsrc, d1 + (j * 4 + wave) * 1024, off1[j], s);
    }
    if (i >= 1) {
      const unsigned s = (unsigned)(i - 1) * W2B;
#pragma unroll
      for (int j = 0; j < PW; ++j)
        glds16(w2_rsrc, d2 + (j * 4 + wave) * 1024, off2, s + j * 4096);
    }
  };
  issue(0);
  issue(1);

  // ---- LayerNorm on the lane's half row -> 16-bit B fragments
  op16x8 xf[KS1];
  {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KS1; ++k)
#pragma unroll
      for (int q = 0; q < 2; ++q) s += v[k][q][0] + v[k][q][1] + v[k][q][2] + v[k][q][3];
    s += __shfl_xor(s, 32, 64);
    const float mean = s * (1.f / DIM);
    float q2 = 0.f;
#pragma unroll
    for (int k = 0; k < KS1; ++k)
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dlt = v[k][q][e] - mean;
          q2 += dlt * dlt;
        }
    q2 += __shfl_xor(q2, 32, 64);
    const float rstd = 1.0f / sqrtf(q2 * (1.f / DIM) + p.eps);
    // parameters visible: the ds_writes have landed (lgkmcnt) + barrier; NOT __syncthreads(), whose fence would also wait for the 96 KB
    // of weight DMAs just issued
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < KS1; ++k) {
      op16x8 f;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 gm = *reinterpret_cast<const f32x4*>(prm + 16 * k + 8 * h + 4 * q);
        const f32x4 bt = *reinterpret_cast<const f32x4*>(prm + DIM + 16 * k + 8 * h + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[4 * q + e] = f2op((v[k][q][e] - mean) * rstd * gm[e] + bt[e]);
      }
      xf[k] = f;
    }
  }
  f32x16 accy[DBW];
#pragma unroll
  for (int d = 0; d < DBW; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) accy[d][e] = 0.f;

  // One ring step: fc1 of hidden chunk `chunk` (W1 image at w1s) beside the GELU of the previous chunk's accumulator `aprev` -> hf.
  //   * W1 fragments in three sub-bursts of 8 (two register sets of 32): a burst is read while the previous one's 8 MFMAs run.  (Read ->
  //     wait -> MFMA one by one the chain ran at the LDS latency; all 24 at once cost 96 registers, which the compiler parked in AGPRs:
  //     184 v_accvgpr moves per step.)
  //   * two independent accumulation chains (even / odd k), summed at the end;
  //   * the GELU's vector instructions are placed BETWEEN the MFMAs (sched_group_barrier pattern: 1 MFMA, 6 VALU): one wave per SIMD, so
  //     nothing else fills the matrix pipe's 32-cycle slots.
  auto fc1_gelu = [&](const unsigned char* w1s, int chunk, f32x16& acch, const f32x16* aprev, op16x8 (&hf)[2]) {
    op16x8 fa[8], fb[8];
    auto rd = [&](op16x8 (&f)[8], int k0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = *reinterpret_cast<const op16x8*>(w1s + r * 768 + (mlp_swz768(2 * (k0 + k) + h, r) << 4));
    };
    rd(fa, 0);
    rd(fb, 8);
    f32x4 bias1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias1[g] = *reinterpret_cast<const f32x4*>(prm + 3 * DIM + chunk * HC + 8 * g + 4 * h);
    f32x16 part[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      part[0][e] = bias1[e >> 2][e & 3];
      part[1][e] = 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 8; ++k) part[k & 1] = MSAM2_MFMA_32x32x16(fa[k], xf[k], part[k & 1], 0, 0, 0);
    if (aprev) {
#pragma unroll
      for (int e = 0; e < 6; e += 2) {
        const f32x2 gp = gelu_erf2(f32x2{(*aprev)[e], (*aprev)[e + 1]});
        hf[e >> 3][e & 7] = f2op(gp[0]);
        hf[e >> 3][(e & 7) + 1] = f2op(gp[1]);
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    rd(fa, 16);
#pragma unroll
    for (int k = 0; k < 8; ++k) part[k & 1] = MSAM2_MFMA_32x32x16(fb[k], xf[8 + k], part[k & 1], 0, 0, 0);
    if (aprev) {
#pragma unroll
      for (int e = 6; e < 12; e += 2) {
        const f32x2 gp = gelu_erf2(f32x2{(*aprev)[e], (*aprev)[e + 1]});
        hf[e >> 3][e & 7] = f2op(gp[0]);
        hf[e >> 3][(e & 7) + 1] = f2op(gp[1]);
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      __builtin_amdgcn_sched_group_barrier(0x002, 6, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 8; ++k) part[k & 1] = MSAM2_MFMA_32x32x16(fa[k], xf[16 + k], part[k & 1], 0, 0, 0);
    if (aprev) {
#pragma unroll
      for (int e = 12; e < 16; e += 2) {
        const f32x2 gp = gelu_erf2(f32x2{(*aprev)[e], (*aprev)[e + 1]});
        hf[e >> 3][e & 7] = f2op(gp[0]);
        hf[e >> 3][(e & 7) + 1] = f2op(gp[1]);
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 2);
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 2);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 16; ++e) acch[e] = part[0][e] + part[1][e];
  };
  auto gelu16 = [&](const f32x16& acch, op16x8 (&hf)[2]) {
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
      const f32x2 gp = gelu_erf2(f32x2{acch[e], acch[e + 1]});
      hf[e >> 3][e & 7] = f2op(gp[0]);
      hf[e >> 3][(e & 7) + 1] = f2op(gp[1]);
    }
  };
  auto fc2 = [&](const unsigned char* w2s, const op16x8 (&hf)[2]) {
    op16x8 a2[DBW][2];
#pragma unroll
    for (int d = 0; d < DBW; ++d) {
      const int row2 = (dh * DBW + d) * 32 + r;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) a2[d][s2] = *reinterpret_cast<const op16x8*>(w2s + row2 * Img64::ROW_BYTES + (((2 * s2 + h) ^ Img64::swz(row2)) << 4));
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)                           // s2 outer: six independent accumulators between the two MFMAs of an output block
#pragma unroll
      for (int d = 0; d < DBW; ++d) accy[d] = MSAM2_MFMA_32x32x16(a2[d][s2], hf[s2], accy[d], 0, 0, 0);
  };

  f32x16 acur;
  // step 0: W1 chunk 0 only
  wait_vmcnt<12>();          // step 1's 12 pieces may still be in flight
  __builtin_amdgcn_s_barrier();
  issue(2);
  {
    op16x8 hf0[2];
    fc1_gelu(smem, 0, acur, nullptr, hf0);
  }
#pragma unroll 1
  for (int i = 1; i < NCH; ++i) {
    // this wave's pieces of step i have landed (step i + 1's 12 -- 6 for the last step -- may still be in flight) ...
    if (i + 1 < NCH) wait_vmcnt<12>();
    else wait_vmcnt<6>();
    __builtin_amdgcn_s_barrier();                            // ... every wave's; the slot of step i - 1 is no longer read
    if (i + 2 <= NCH) issue(i + 2);
    const unsigned char* w1s = smem + (i % NST) * BUF;
    f32x16 anext;
    op16x8 hf[2];
    fc1_gelu(w1s, i, anext, &acur, hf);                      // chunk i on the matrix pipe, chunk i - 1's GELU on the vector pipe
    fc2(w1s + W1B, hf);                                      // chunk i - 1
    acur = anext;
  }
  {
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    op16x8 hf[2];
    gelu16(acur, hf);
    fc2(smem + (NCH % NST) * BUF + W1B, hf);
  }

  // ---- epilogue: + b2 + residual; every residual value of three output blocks is loaded before their first store
  if (t < p.T) {
    const float* xres = p.x + t * DIM;
    float* yr = p.out + t * DIM;
    constexpr int DG = 3;
#pragma unroll
    for (int d0 = 0; d0 < DBW; d0 += DG) {
      f32x4 xv[DG][4];
#pragma unroll
      for (int d = 0; d < DG; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) xv[d][g] = *reinterpret_cast<const f32x4*>(xres + (dh * DBW + d0 + d) * 32 + 8 * g + 4 * h);
#pragma unroll
      for (int d = 0; d < DG; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = (dh * DBW + d0 + d) * 32 + 8 * g + 4 * h;
          const f32x4 bv = *reinterpret_cast<const f32x4*>(prm + 2 * DIM + ch);
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = accy[d0 + d][4 * g + e] + bv[e] + xv[d][g][e];
          *reinterpret_cast<f32x4*>(yr + ch) = o;
          if (p.out16) {
            op16x4 o2;
#pragma unroll
            for (int e = 0; e < 4; ++e) o2[e] = f2op(o[e]);
            *reinterpret_cast<op16x4*>(p.out16 + t * DIM + ch) = o2;
          }
        }
    }
  }
#endif
}

// W2 [384, 1536] for mlp_fused384_kernel: chunk-major [48][384][32], each 64-byte row in its LDS image (16-byte chunk c at c ^ ((d >> 2) & 3)),
// hidden units of a chunk in the operand order of mlp_fused_permute_kernel
__global__ void mlp_fused384_pack_kernel(const op16* __restrict__ w2, op16* __restrict__ w2q, int dim, int hid) {
  const int64_t total = (int64_t)dim * hid;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int chunk = (int)(i / ((int64_t)dim * 32)), d = (int)((i / 32) % dim), q = (int)(i & 31);
    const int c = (q >> 3) ^ Img64::swz(d), j = q & 7, pos = c * 8 + j;
    const int s = pos >> 4, hh = (pos >> 3) & 1;
    w2q[i] = w2[(int64_t)d * hid + chunk * 32 + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)];
  }
}

// hidden-dimension permutation of W2 [DIM, HID] that matches the k order in which an H^T accumulator is consumed as the B operand:
// position 16 s + 8 h + j of every 32-block holds hidden unit 16 s + 8 (j >> 2) + 4 h + (j & 3).
__global__ void mlp_fused_permute_kernel(const op16* __restrict__ w2, op16* __restrict__ w2p, int dim, int hid) {
  const int64_t total = (int64_t)dim * hid;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i / hid), pos = (int)(i % hid);
    const int blk = pos >> 5, q = pos & 31, s = q >> 4, hh = (q >> 3) & 1, j = q & 7;
    w2p[i] = w2[(int64_t)d * hid + blk * 32 + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)];
  }
}

extern "C" int msam2_mlp_fused_permute_w2(const void* w2, void* w2p, int64_t dim, int64_t hidden, void* stream) {
  MSAM2_REQUIRE(w2 && w2p && dim > 0 && hidden % 32 == 0, "mlp_fused_permute_w2: bad arguments");
  if (dim == 384) {                                          // mlp_fused384_kernel's chunk-major LDS image
    MSAM2_REQUIRE(hidden == 1536, "mlp_fused_permute_w2: dim 384 takes hidden 1536");
    hipLaunchKernelGGL(mlp_fused384_pack_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, (const op16*)w2, (op16*)w2p, (int)dim, (int)hidden);
    return msam2_check_launch("mlp_fused_permute_w2(384)");
  }
  hipLaunchKernelGGL(mlp_fused_permute_kernel, dim3((unsigned)min((int64_t)1024, cdiv(dim * hidden, 256))), dim3(256), 0, (hipStream_t)stream,
                     (const op16*)w2, (op16*)w2p, (int)dim, (int)hidden);
  return msam2_check_launch("mlp_fused_permute_w2");
}

// 1 when the trunk should take msam2_ln_mlp_residual_fwd at this width (hidden = 4 * dim, GELU): dim 96 / 192 (Hiera stages 1 / 2; hiera_b+'s
// 112 / 224 are not built).  Dim 384 is built and callable but slower than its three launches (see mlp_fused384_kernel): MSAM2_MLP_384=1
// makes the trunk use it (A/B).
extern "C" int msam2_ln_mlp_residual_supported(int64_t dim) {
  static const bool use384 = [] { const char* e = getenv("MSAM2_MLP_384"); return e && e[0] == '1'; }();
  return dim == 96 || dim == 192 || (dim == 384 && use384);
}

static int launch_mlp_fused384(const MlpFusedParams& p, hipStream_t s) {
  constexpr int LDS = 3 * 49152 + (3 * 384 + 1536) * 4;
  ensure_dyn_lds<mlp_fused384_kernel>(LDS);
  hipLaunchKernelGGL(mlp_fused384_kernel, dim3((unsigned)((p.T + 63) / 64)), dim3(256), LDS, s, p);
  return msam2_check_launch("ln_mlp_residual_fwd(384)");
}

template <int DIM, int HC, int TB, int OCC = 1, int NWV = 4>
static int launch_mlp_fused(const MlpFusedParams& p, hipStream_t s) {
  constexpr int LDS = 2 * (2 * HC * DIM * 2) + (3 * DIM + 4 * DIM) * 4;
  ensure_dyn_lds<mlp_fused_kernel<DIM, HC, TB, OCC, NWV>>(LDS);
  const int64_t n_pass = (p.T + NWV * 32 * TB - 1) / (NWV * 32 * TB);
  hipLaunchKernelGGL((mlp_fused_kernel<DIM, HC, TB, OCC, NWV>), dim3((unsigned)min((int64_t)256 * OCC, n_pass)), dim3(NWV * 64), LDS, s, p);
  return msam2_check_launch("ln_mlp_residual_fwd");
}

// out[T, dim] (fp32) = x + fc2(GELU(fc1(LayerNorm(x)))) with x fp32 [T, dim] contiguous, w1 16-bit [4 dim, dim], w2p 16-bit [dim, 4 dim]
// permuted by msam2_mlp_fused_permute_w2, biases / LayerNorm parameters fp32.  dim in {96, 192, 384}.
static int ln_mlp_residual_launch(const float* x, int64_t T, int64_t dim, const float* ln_w, const float* ln_b, float eps, const void* w1,
                                  const float* b1, const void* w2p, const float* b2, float* out, void* out16, void* stream) {
  MSAM2_REQUIRE(x && out && ln_w && ln_b && w1 && b1 && w2p && b2 && T > 0, "ln_mlp_residual: null tensor / empty problem");
  MSAM2_REQUIRE(dim == 96 || dim == 192 || dim == 384, "ln_mlp_residual: dim %lld not built (96 / 192 / 384)", (long long)dim);
  MSAM2_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)w1 | (uintptr_t)w2p | (uintptr_t)ln_w | (uintptr_t)ln_b | (uintptr_t)b1 | (uintptr_t)b2) & 15) == 0 &&
                    ((uintptr_t)out16 & 7) == 0, "ln_mlp_residual: 16-byte aligned tensors");
  MSAM2_REQUIRE(x != out, "ln_mlp_residual: in-place not supported (a token's residual is re-read in the store)");
  MlpFusedParams p = {x, out, ln_w, ln_b, b1, b2, (const op16*)w1, (const op16*)w2p, T, eps, (op16*)out16};
  hipStream_t s = (hipStream_t)stream;
  if (dim == 384) {
    MSAM2_REQUIRE((T + 63) / 64 < (1ll << 31), "ln_mlp_residual: too many tokens");
    return launch_mlp_fused384(p, s);
  }
  static const bool four = [] { const char* e = getenv("MSAM2_MLP_WAVES4"); return e && e[0] == '1'; }();   // A/B: the 4-wave form
  if (four) {
    if (dim == 96) return launch_mlp_fused<96, 192, 4>(p, s);
    return launch_mlp_fused<192, 96, 2>(p, s);
  }
  if (dim == 96) return launch_mlp_fused<96, 192, 2, 1, 8>(p, s);
  return launch_mlp_fused<192, 96, 1, 1, 8>(p, s);
}

extern "C" int msam2_ln_mlp_residual_fwd(const float* x, int64_t T, int64_t dim, const float* ln_w, const float* ln_b, float eps, const void* w1,
                                         const float* b1, const void* w2p, const float* b2, float* out, void* stream) {
  return ln_mlp_residual_launch(x, T, dim, ln_w, ln_b, eps, w1, b1, w2p, b2, out, nullptr, stream);
}

// the same with the result also written in the 16-bit operand type (out16 [T, dim]): the last block of a Hiera stage, whose output is the
// operand of the FPN's lateral 1x1 convolution (image_encoder.py:95-110) -- no cast pass over the largest feature maps
extern "C" int msam2_ln_mlp_residual_fwd_dual(const float* x, int64_t T, int64_t dim, const float* ln_w, const float* ln_b, float eps,
                                              const void* w1, const float* b1, const void* w2p, const float* b2, float* out, void* out16,
                                              void* stream) {
  MSAM2_REQUIRE(out16, "ln_mlp_residual_dual: null 16-bit output");
  return ln_mlp_residual_launch(x, T, dim, ln_w, ln_b, eps, w1, b1, w2p, b2, out, out16, stream);
}

// ---- PROJ form: the attention's output projection in front of the MLP, the next block's norm1 behind it
// 1 when msam2_proj_ln_mlp_residual_fwd is built for this width (the proj is square: width == dim): 96 / 192.
extern "C" int msam2_proj_ln_mlp_residual_supported(int64_t dim) { return dim == 96 || dim == 192; }

// W1 [hidden, dim] with its INPUT index permuted inside every 32-block to the accumulator's register order (position 16 s + 8 h + j holds
// channel 16 s + 8 (j >> 2) + 4 h + (j & 3)): the permutation mlp_fused_permute_kernel applies to W2's hidden index, rows and columns swapped
extern "C" int msam2_mlp_fused_permute_w1(const void* w1, void* w1p, int64_t hidden, int64_t dim, void* stream) {
  MSAM2_REQUIRE(w1 && w1p && hidden > 0 && dim > 0 && dim % 32 == 0, "mlp_fused_permute_w1: bad arguments");
  hipLaunchKernelGGL(mlp_fused_permute_kernel, dim3((unsigned)min((int64_t)1024, cdiv(dim * hidden, 256))), dim3(256), 0, (hipStream_t)stream,
                     (const op16*)w1, (op16*)w1p, (int)hidden, (int)dim);
  return msam2_check_launch("mlp_fused_permute_w1");
}

template <int DIM, int HC, int TB, int SIDE>
static int launch_proj_mlp_fused_side(const MlpFusedParams& p, hipStream_t s) {
  constexpr int LDS = 2 * (2 * HC * DIM * 2) + (3 * DIM + 4 * DIM + 3 * DIM) * 4;
  ensure_dyn_lds<mlp_fused_kernel<DIM, HC, TB, 1, 8, true, SIDE>>(LDS);
  const int64_t n_pass = (p.T + 8 * 32 * TB - 1) / (8 * 32 * TB);
  hipLaunchKernelGGL((mlp_fused_kernel<DIM, HC, TB, 1, 8, true, SIDE>), dim3((unsigned)min((int64_t)256, n_pass)), dim3(512), LDS, s, p);
  return msam2_check_launch("proj_ln_mlp_residual_fwd");
}

template <int DIM, int HC, int TB>
static int launch_proj_mlp_fused(const MlpFusedParams& p, hipStream_t s) {
  switch ((p.out16 ? 1 : 0) | (p.xn16 ? 2 : 0)) {
    case 0: return launch_proj_mlp_fused_side<DIM, HC, TB, 0>(p, s);
    case 1: return launch_proj_mlp_fused_side<DIM, HC, TB, 1>(p, s);
    case 2: return launch_proj_mlp_fused_side<DIM, HC, TB, 2>(p, s);
    default: return launch_proj_mlp_fused_side<DIM, HC, TB, 3>(p, s);
  }
}

// out[T, dim] (fp32) = x1 + fc2(GELU(fc1(LayerNorm(x1; ln_w, ln_b, eps)))) with x1 = res + o wp^T + bp, which is never written.  o 16-bit [T, dim],
// wp 16-bit [dim, dim], res fp32 [T, dim] (out == res is allowed), w1p from msam2_mlp_fused_permute_w1, w2p from msam2_mlp_fused_permute_w2.
// Optional: out16 [T, dim] = out rounded to the 16-bit operand type; xn16 [T, dim] = LayerNorm(out rows; nln_w, nln_b, neps) in that type.
extern "C" int msam2_proj_ln_mlp_residual_fwd(const void* o, const void* wp, const float* bp, const float* res, int64_t T, int64_t dim,
                                              const float* ln_w, const float* ln_b, float eps, const void* w1p, const float* b1, const void* w2p,
                                              const float* b2, float* out, void* out16, const float* nln_w, const float* nln_b, float neps,
                                              void* xn16, void* stream) {
  MSAM2_REQUIRE(o && wp && bp && res && out && ln_w && ln_b && w1p && b1 && w2p && b2 && T > 0, "proj_ln_mlp_residual: null tensor / empty problem");
  MSAM2_REQUIRE(msam2_proj_ln_mlp_residual_supported(dim), "proj_ln_mlp_residual: dim %lld not built (96 / 192)", (long long)dim);
  MSAM2_REQUIRE(!xn16 || (nln_w && nln_b), "proj_ln_mlp_residual: the LayerNorm output needs its parameters");
  MSAM2_REQUIRE((((uintptr_t)o | (uintptr_t)wp | (uintptr_t)bp | (uintptr_t)res | (uintptr_t)out | (uintptr_t)w1p | (uintptr_t)w2p | (uintptr_t)ln_w |
                  (uintptr_t)ln_b | (uintptr_t)b1 | (uintptr_t)b2 | (uintptr_t)nln_w | (uintptr_t)nln_b) & 15) == 0 &&
                    (((uintptr_t)out16 | (uintptr_t)xn16) & 15) == 0, "proj_ln_mlp_residual: 16-byte aligned tensors");
  MlpFusedParams p = {res, out, ln_w, ln_b, b1, b2, (const op16*)w1p, (const op16*)w2p, T, eps, (op16*)out16,
                      (const op16*)o, (const op16*)wp, bp, nln_w, nln_b, neps, (op16*)xn16};
  if (dim == 96) return launch_proj_mlp_fused<96, 192, 2>(p, (hipStream_t)stream);
  return launch_proj_mlp_fused<192, 96, 1>(p, (hipStream_t)stream);
}
