// Hiera windowed attention with the qkv projection inside (attn_winproj_kernel): o = window_attention(xn Wqkv^T + b) for the blocks of
// stages 1-2 (head dim 96, 8 x 8 or 4 x 4 windows that tile the image exactly, optionally 2 x 2 max-pooled queries).  The two launches it
// replaces (qkv GEMM, window attention) exist to write the 16-bit q | k | v map to memory and read it back; here it never
// leaves one wave's registers.  Same transposed arithmetic as mlp_fused_kernel: a 32 x 32 accumulator, converted, IS the next MFMA's operand.
//
//   * a wave owns a UNIT of whole windows: one 8 x 8 window = NB = 2 blocks of 32 tokens, or two 4 x 4 windows = one block with the
//     block-diagonal mask of attn_tinywin_kernel.  A lane owns a token; its xn row is loaded once into the operand layout (lane (r, h):
//     elements 16 k + 8 h .. + 7 of token r), which serves as A or B alike;
//   * Q^T = Wq Xn^T, K^T = Wk Xn^T (A = weight rows from LDS, B = token rows): token on the lane, d = 32 db + s_frag_key(e, h) in register
//     e.  + bias, rounded to the operand type (the rounding point of the GEMM).  Registers 0-7 / 8-15 of d-block db are k-steps 2 db /
//     2 db + 1 of S^T[key][query] = K Q^T with A = K^T, B = Q^T fragments: both run over d in the same permuted order;
//   * V = Xn Wv^T (A = token rows, B = weight rows): d = 32 db + r on the lane, key s_frag_key(e, h) in register e -- the key order of
//     the converted P^T = softmax(S^T) registers, so O^T[d][query] += V^T P^T takes both straight from registers.  No LDS transpose;
//   * softmax over a lane's 16 NB score registers and the other lane half (half_max / half_sum, exp2 with the folded scale);
//   * q-pool: the token -> lane map puts a 2 x 2 pool group on one lane quad; the pooled query is two quad-permute max steps per Q^T
//     register, all four lanes then carry the same query and lane 0 of the quad stores it;
//   * order per head: K, then Q and scores + softmax one query block at a time (Q, K dead), then V one d-block at a time, each d-block
//     of O stored as it completes; sched_barriers keep the phases apart (interleaved, their live ranges spilled 9-34 registers).
// Weights: the packed qkv weight [3][heads][96][DIM] is 3 * heads slabs of 96 rows; LDS image of a slab = rows of 2 DIM bytes with
// mlp_swz, filled by LDS-DMA.  RESIDENT (dim 96: 1 / 2 heads = 55 / 110 KB): every slab loaded once, the persistent pass loop has no
// barrier.  STREAM (dim 192: 2 / 4 heads = 221 / 442 KB): two-slot ring, one slab ahead, ONE barrier per slab, running on across passes.
// Every wave of a workgroup runs the same number of barriers: a ragged last pass clamps its unit (loads) and masks its stores.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage): planned 2 waves per SIMD (8 waves per workgroup, <= 256 registers, no scratch);
// obtained 2 waves per SIMD, no scratch: <96,8,pool> 234 / 236, <96,8> 238 / 242, <192,4,pool> 220 / 218, <192,4> 224 / 222 (fp16 / bf16 build).
#include "common.h"
#include <stdlib.h>

struct WinProjParams {
  const op16* xn;      // [B * H * W, DIM]
  const op16* w;       // [3 * heads * 96, DIM], rows (q | k | v, head, d)
  const float* bias;   // [3 * heads * 96]
  op16* o;             // [B * Hq * Wq, heads * 96]
  int heads, H, W, nwx, nw;   // nw = windows per image
  int n_units;         // B * nw (8 x 8) or B * nw / 2 (4 x 4)
  float scale_log2;
};

__device__ __forceinline__ float quad_max(float v) {
  const int a = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
  v = fmaxf(v, __builtin_bit_cast(float, a));
  const int b = __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
  return fmaxf(v, __builtin_bit_cast(float, b));
}

// out[tb][db][s] = operand fragments of (W_slab Xn^T + bias)^T for the wave's NB token blocks: token on the lane, d in the registers
template <int DIM, int NB, bool QUADMAX>
__device__ __forceinline__ void winproj_T(const unsigned char* slab, const float* bias, const op16x8 (&xf)[NB][DIM / 16], int r, int h,
                                          op16x8 (&out)[NB][3][2]) {
  constexpr int KS = DIM / 16, RB = DIM * 2;
#pragma unroll
  for (int db = 0; db < 3; ++db) {
    const int row = db * 32 + r;
    op16x8 a[KS];
#pragma unroll
    for (int k = 0; k < KS; ++k) a[k] = *reinterpret_cast<const op16x8*>(slab + row * RB + (mlp_swz<RB>(2 * k + h, row) << 4));
    f32x4 bv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bv[g] = *reinterpret_cast<const f32x4*>(bias + db * 32 + 8 * g + 4 * h);
#pragma unroll
    for (int tb = 0; tb < NB; ++tb) {
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int k = 0; k < KS; ++k) acc = MSAM2_MFMA_32x32x16(a[k], xf[tb][k], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = acc[e];
        if constexpr (QUADMAX) v = quad_max(v);               // max commutes with + bias and with the rounding
        out[tb][db][e >> 3][e & 7] = f2op(v + bv[e >> 2][e & 3]);
      }
    }
  }
}

template <int DIM, int WS, bool POOL, bool STREAM, int NWV>
__global__ __launch_bounds__(NWV * 64, 1) void attn_winproj_kernel(WinProjParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert((DIM == 96 || DIM == 192) && (WS == 8 || WS == 4), "built forms");
  constexpr int D = 96, DB = 3, KS = DIM / 16, RB = DIM * 2, CPR = DIM / 8, NB = WS == 8 ? 2 : 1;
  constexpr int SLAB = D * RB, PIECES = SLAB / 1024, PW = (PIECES + NWV - 1) / NWV;
  static_assert(SLAB % 1024 == 0, "whole DMA pieces");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int heads = p.heads, nslab = 3 * heads;
  float* bsm = reinterpret_cast<float*>(smem + (STREAM ? 2 : nslab) * SLAB);
  for (int i = tid; i < nslab * D; i += NWV * 64) bsm[i] = p.bias[i];

  // ---- weight slabs by LDS-DMA: per-lane source offsets of this wave's pieces inside a slab, scalar slab offset per issue
  const auto w_rsrc = raw_rsrc(p.w, nslab * SLAB);
  unsigned off[PW];
#pragma unroll
  for (int j = 0; j < PW; ++j) {
    const int f = min(j * NWV + wave, PIECES - 1) * 64 + lane, row = f / CPR, c = f % CPR;
    off[j] = (unsigned)(row * RB + mlp_swz<RB>(c, row) * 16);
  }
  auto issue = [&](int slab, int slot) {
    unsigned char* d = smem + slot * SLAB;
#pragma unroll
    for (int j = 0; j < PW; ++j)
      if (j * NWV + wave < PIECES) glds16(w_rsrc, d + (j * NWV + wave) * 1024, off[j], (unsigned)slab * SLAB);
  };
  // the slabs in the order a pass consumes them: step i = head i / 3, (k, q, v)[i % 3]
  auto slab_of = [&](int i) { return ((i % 3) == 2 ? 2 : 1 - i % 3) * heads + i / 3; };

  const int n_pass = (p.n_units + NWV - 1) / NWV;
  if constexpr (STREAM) {
    if ((int)blockIdx.x < n_pass) issue(slab_of(0), 0);
  } else {
    for (int s = 0; s < nslab; ++s) issue(s, s);
    wait_vmcnt<0>();
  }
  __syncthreads();                                           // bias (and the resident slabs) visible
  int g_step = 0;                                            // STREAM: running slab count of this workgroup (slot = parity)

  for (int pass = blockIdx.x; pass < n_pass; pass += gridDim.x) {
    const bool last_pass = pass + (int)gridDim.x >= n_pass;
    // STREAM: wait for step i's slab, one barrier, start the next slab into the other slot.  RESIDENT: the slab's fixed place.
    auto slab_ptr = [&](int i) -> const unsigned char* {
      if constexpr (STREAM) {
        const int slot = g_step & 1;
        wait_vmcnt<0>();                                     // this wave's pieces of the slab have landed
        __builtin_amdgcn_s_barrier();                        // ... every wave's; the other slot is no longer read
        if (i + 1 < nslab) issue(slab_of(i + 1), slot ^ 1);
        else if (!last_pass) issue(slab_of(0), slot ^ 1);
        ++g_step;
        return smem + slot * SLAB;
      } else {
        return smem + slab_of(i) * SLAB;
      }
    };

    // ---- this wave's unit (clamped on a ragged last pass; stores masked), token -> lane map, row loads
    const int u_raw = pass * NWV + wave;
    const bool live = u_raw < p.n_units;
    const int u = live ? u_raw : p.n_units - 1;
    int64_t otok[NB];
    op16x8 xf[NB][KS];
#pragma unroll
    for (int tb = 0; tb < NB; ++tb) {
      int win, ty, tx, py = 0, px = 0;
      if constexpr (WS == 8) {
        win = u;
        if constexpr (POOL) {
          const int pq = tb * 8 + (r >> 2);
          py = pq >> 2; px = pq & 3;
          ty = 2 * py + ((r >> 1) & 1); tx = 2 * px + (r & 1);
        } else {
          const int t = tb * 32 + r;
          ty = t >> 3; tx = t & 7;
        }
      } else {
        win = 2 * u + (r >> 4);
        if constexpr (POOL) {
          const int qd = (r >> 2) & 3;
          py = qd >> 1; px = qd & 1;
          ty = 2 * py + ((r >> 1) & 1); tx = 2 * px + (r & 1);
        } else {
          const int t = r & 15;
          ty = t >> 2; tx = t & 3;
        }
      }
      const int b = win / p.nw, wi = win - b * p.nw, wy = wi / p.nwx, wx = wi - wy * p.nwx;
      const int64_t tok = ((int64_t)b * p.H + wy * WS + ty) * p.W + wx * WS + tx;
      otok[tb] = POOL ? ((int64_t)b * (p.H / 2) + wy * (WS / 2) + py) * (p.W / 2) + wx * (WS / 2) + px : tok;
      const op16* xr = p.xn + tok * DIM;
#pragma unroll
      for (int k = 0; k < KS; ++k) xf[tb][k] = __builtin_bit_cast(op16x8, *reinterpret_cast<const uint4*>(xr + 16 * k + 8 * h));
    }
    const bool do_store = live && (!POOL || (r & 3) == 0);

#pragma unroll 1
    for (int head = 0; head < heads; ++head) {
      op16x8 pf[NB][NB][2];                                  // [query block][key block][k-step]
      float inv[NB];
      {
        op16x8 kf[NB][DB][2];
        const unsigned char* sk = slab_ptr(3 * head);
        winproj_T<DIM, NB, false>(sk, bsm + (heads + head) * D, xf, r, h, kf);
        const unsigned char* sq = slab_ptr(3 * head + 1);
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
          __builtin_amdgcn_sched_barrier(0);                   // phases stay apart: interleaved, their live ranges add up to spills
          op16x8 qf[1][DB][2];                                 // one query block at a time: 24 registers instead of 48 beside K^T
          winproj_T<DIM, 1, POOL>(sq, bsm + head * D, reinterpret_cast<const op16x8(&)[1][KS]>(xf[qb]), r, h, qf);
          f32x16 s[NB];
          float mx = -INFINITY;
#pragma unroll
          for (int kb = 0; kb < NB; ++kb) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kb][e] = 0.f;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
              for (int st = 0; st < 2; ++st) s[kb] = MSAM2_MFMA_32x32x16(kf[kb][db][st], qf[0][db][st], s[kb], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              if constexpr (WS == 4) {
                if ((s_frag_key(e, h) >> 4) != (r >> 4)) s[kb][e] = -INFINITY;   // the unit's other window
              }
              mx = fmaxf(mx, s[kb][e]);
            }
          }
          mx = half_max(mx) * p.scale_log2;                  // scale > 0: max commutes with it; finite: 16 / 64 own keys
          float psum = 0.f;
#pragma unroll
          for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][e], p.scale_log2, -mx));
              psum += pe;
              pf[qb][kb][e >> 3][e & 7] = f2op_fast(pe);
            }
          inv[qb] = 1.f / half_sum(psum);
        }
      }
      // ---- V one d-block at a time: V = Xn Wv^T (d on the lane, key in the registers), O^T block = V^T P^T, stored at once
      const unsigned char* sv = slab_ptr(3 * head + 2);
      const float* bvp = bsm + (2 * heads + head) * D;
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        __builtin_amdgcn_sched_barrier(0);
        const int row = db * 32 + r;
        op16x8 a[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) a[k] = *reinterpret_cast<const op16x8*>(sv + row * RB + (mlp_swz<RB>(2 * k + h, row) << 4));
        const float bv = bvp[row];
        op16x8 vf[NB][2];
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) {
          f32x16 acc;
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
          for (int k = 0; k < KS; ++k) acc = MSAM2_MFMA_32x32x16(xf[kb][k], a[k], acc, 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 16; ++e) vf[kb][e >> 3][e & 7] = f2op(acc[e] + bv);
        }
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
          f32x16 o[1];
#pragma unroll
          for (int e = 0; e < 16; ++e) o[0][e] = 0.f;
#pragma unroll
          for (int kb = 0; kb < NB; ++kb)
#pragma unroll
            for (int st = 0; st < 2; ++st) o[0] = MSAM2_MFMA_32x32x16(vf[kb][st], pf[qb][kb][st], o[0], 0, 0, 0);
          if (do_store) ATTN_STORE_O_ROWS(1, p.o + otok[qb] * (heads * D) + head * D + db * 32, o, inv[qb], h);
        }
      }
    }
  }
#endif
}

// 1 when msam2_window_qkv_attention_fwd is built for a block: head dim 96, dim 96 / 192 with the weights' LDS plan (dim 96: resident,
// <= 2 heads), 8 x 8 or 4 x 4 windows that tile the H x W token image exactly (pooled blocks: even H, W follow), 4 x 4 windows in pairs
// inside an image.  Per-slice quantities only: never the batch.
extern "C" int msam2_window_qkv_attention_supported(int64_t dim, int64_t dim_out, int64_t heads, int64_t ws, int pool, int64_t H,
                                                    int64_t W) {
  if (heads <= 0 || dim_out != heads * 96 || H <= 0 || W <= 0) return 0;
  if (!(ws == 8 || ws == 4) || H % ws || W % ws) return 0;
  if (pool && (H % 2 || W % 2)) return 0;
  if (ws == 4 && ((H / 4) * (W / 4)) % 2) return 0;
  if (dim == 96) return ws == 8 && heads <= 2;
  if (dim == 192) return ws == 4 && heads <= 8;
  return 0;
}

template <int DIM, int WS, bool POOL, bool STREAM>
static int launch_winproj(const WinProjParams& p, hipStream_t s) {
  constexpr int NWV = 8, SLAB = 96 * DIM * 2;
  const int lds = (STREAM ? 2 : 3 * p.heads) * SLAB + 3 * p.heads * 96 * 4;
  ensure_dyn_lds<attn_winproj_kernel<DIM, WS, POOL, STREAM, NWV>>(160 * 1024);
  const int n_pass = (p.n_units + NWV - 1) / NWV;
  hipLaunchKernelGGL((attn_winproj_kernel<DIM, WS, POOL, STREAM, NWV>), dim3((unsigned)min(256, n_pass)), dim3(NWV * 64), lds, s, p);
  return msam2_check_launch("window_qkv_attention_fwd");
}

// o [B * Hq * Wq, heads * 96] (16-bit) = windowed attention of q | k | v = xn w^T + bias over the [B, H, W] token image xn [B * H * W, dim]
// (16-bit, contiguous), w the packed qkv weight [3 * heads * 96, dim] (16-bit, contiguous), bias fp32; ws x ws windows, pool = queries
// 2 x 2 max-pooled (Hq = H / 2).  The result msam2_gemm (+ msam2_gemm_qkv_pool2x2) + msam2_window_attention_fwd give, without the qkv map.
extern "C" int msam2_window_qkv_attention_fwd(const void* xn, const void* w, const float* bias, void* o, int64_t B, int64_t H, int64_t W,
                                              int64_t dim, int64_t heads, int64_t ws, int pool, float scale, void* stream) {
  MSAM2_REQUIRE(xn && w && bias && o, "window_qkv_attention: null tensor");
  MSAM2_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, "window_qkv_attention: empty problem");
  MSAM2_REQUIRE(msam2_window_qkv_attention_supported(dim, heads * 96, heads, ws, pool, H, W),
                "window_qkv_attention: dim %lld, %lld heads, window %lld, pool %d on %lld x %lld tokens is not built", (long long)dim,
                (long long)heads, (long long)ws, pool, (long long)H, (long long)W);
  MSAM2_REQUIRE((((uintptr_t)xn | (uintptr_t)w | (uintptr_t)bias) & 15) == 0 && ((uintptr_t)o & 7) == 0, "window_qkv_attention: 16-byte aligned tensors");
  MSAM2_REQUIRE(scale > 0.f, "window_qkv_attention: scale must be positive");
  const int64_t nw = (H / ws) * (W / ws), units = ws == 8 ? B * nw : B * nw / 2;
  MSAM2_REQUIRE(B * nw < (1ll << 30), "window_qkv_attention: too many windows");
  WinProjParams p = {(const op16*)xn, (const op16*)w, bias, (op16*)o, (int)heads, (int)H, (int)W, (int)(W / ws), (int)nw, (int)units,
                     scale * 1.4426950408889634f};
  hipStream_t s = (hipStream_t)stream;
  if (dim == 96) return pool ? launch_winproj<96, 8, true, false>(p, s) : launch_winproj<96, 8, false, false>(p, s);
  return pool ? launch_winproj<192, 4, true, true>(p, s) : launch_winproj<192, 4, false, true>(p, s);
}
