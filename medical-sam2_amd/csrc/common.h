// Shared device/host helpers for the gfx950 (MI355X, CDNA4) kernels of libmsam2_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// 16-bit MFMA operand type of the whole library.  Default: IEEE fp16 (11-bit significand -> 8x finer operand rounding than
// bf16 at the same MFMA rate; every activation of this network sits well inside the fp16 range because residual streams,
// softmax statistics, LayerNorm and all logits stay fp32).  -DMSAM2_OPERAND_BF16 rebuilds the library on bf16 operands.
#if defined(MSAM2_OPERAND_BF16)
typedef __bf16 op16;
#define MSAM2_OPERAND_IS_FP16 0
#define MSAM2_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#else
typedef _Float16 op16;
#define MSAM2_OPERAND_IS_FP16 1
#define MSAM2_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#endif
typedef __attribute__((ext_vector_type(8))) op16 op16x8;
typedef __attribute__((ext_vector_type(4))) op16 op16x4;
typedef __attribute__((ext_vector_type(2))) op16 op16x2;
typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((ext_vector_type(8))) short short8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define MSAM2_OK 0
#define MSAM2_ERR_ARG -1
#define MSAM2_ERR_LAUNCH -2

// error string shared by every translation unit (api.hip owns it)
void msam2_set_error(const char* fmt, ...);
int msam2_check_launch(const char* what);

#define MSAM2_REQUIRE(cond, ...)          \
  do {                                    \
    if (!(cond)) {                        \
      msam2_set_error(__VA_ARGS__);       \
      return MSAM2_ERR_ARG;               \
    }                                     \
  } while (0)

__device__ __forceinline__ float op2f(op16 x) { return (float)x; }
// fp32 -> operand.  The fp16 build SATURATES at +-65504 (one v_med3_f32): a value beyond the fp16 range -- a real checkpoint's large
// MLP / qkv activation, an un-scaled gradient -- must not become inf and travel through softmax / LayerNorm / the optimiser state.
// Reductions across the two 32-lane halves of a wave (the row halves of a 32x32 MFMA accumulator): v_permlane32_swap_b32 (gfx950)
// exchanges the halves in the VALU -- __shfl_xor(v, 32) compiles to ds_bpermute_b32, an LDS round trip plus an lgkmcnt wait in the
// middle of every softmax tile.  Both results are identical in all 64 lanes and bit-equal to the shuffle forms (max, + commute).
__device__ __forceinline__ float half_max(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}
__device__ __forceinline__ float half_sum(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}

// NaN stays NaN.  f2op_fast is the plain conversion for values known to be bounded (softmax probabilities in [0, 1]).
__device__ __forceinline__ op16 f2op_fast(float x) { return (op16)x; }
#if MSAM2_OPERAND_IS_FP16 && !defined(MSAM2_NO_SATURATE)
__device__ __forceinline__ op16 f2op(float x) { return (op16)__builtin_amdgcn_fmed3f(x, -65504.f, 65504.f); }
#else
__device__ __forceinline__ op16 f2op(float x) { return (op16)x; }
#endif

// fp32 -> the output element type of a templated kernel (saturating for the fp16 operand type, identity for fp32)
template <typename T> __device__ __forceinline__ T f2out(float x);
template <> __device__ __forceinline__ float f2out<float>(float x) { return x; }
template <> __device__ __forceinline__ op16 f2out<op16>(float x) { return f2op(x); }

// One 1-KiB LDS-DMA piece (buffer_load_dwordx4 ... offen lds: lane l's 16 bytes land at lds + 16 l), issued from INLINE ASM.
// Why not __builtin_amdgcn_raw_ptr_buffer_load_lds: hipcc tracks the builtin's LDS write on vmcnt and, before the next LDS read it cannot
// prove disjoint (every ds_read_b64_tr_b16 -- the intrinsic carries no alias information), inserts s_waitcnt vmcnt(0): the wave then
// sits out the full latency of the DMA it issued a few instructions earlier -- in every tile of a loop whose whole point is to stream
// tile t+2 under the MFMAs of tile t (found in the ISA of attn_kv64x2_kernel, round 3).  An asm statement is
// opaque to that bookkeeping; the kernels wait for their DMA themselves (s_waitcnt vmcnt(N) + s_barrier before the first read of a
// stage), which they did anyway.  M0 (the LDS base) is written in the statement that uses it and restored; s_nop 4 covers a
// just-written SGPR operand (descriptor / offsets) and the M0 write -> LDS-DMA hazard.  lds must be wave-uniform.
// -DMSAM2_DMA_BUILTIN keeps the builtin (A/B builds).
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rsrc, const unsigned char* lds, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lds), 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void glds16_asm(__amdgpu_buffer_rsrc_t rsrc, const unsigned char* lds, unsigned voff, unsigned soff) {
#ifdef MSAM2_DMA_BUILTIN
  glds16(rsrc, lds, voff, soff);
#else
  const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)(lds);
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 4\n\t"
      "buffer_load_dwordx4 %1, %2, %4 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(rsrc), "s"(dst), "s"(soff)
      : "memory");
#endif
}

// three consecutive pieces (LDS lds, lds + 1 KiB, lds + 2 KiB) in one statement: M0 saved / restored once
__device__ __forceinline__ void glds16x3_asm(__amdgpu_buffer_rsrc_t rsrc, const unsigned char* lds, unsigned v0, unsigned v1, unsigned v2,
                                             unsigned soff) {
#ifdef MSAM2_DMA_BUILTIN
  glds16(rsrc, lds, v0, soff);
  glds16(rsrc, lds + 1024, v1, soff);
  glds16(rsrc, lds + 2048, v2, soff);
#else
  const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)(lds);
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %5\n\t"
      "s_nop 4\n\t"
      "buffer_load_dwordx4 %1, %4, %6 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %2, %4, %6 offen lds\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %3, %4, %6 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(v0), "v"(v1), "v"(v2), "s"(rsrc), "s"(dst), "s"(soff)
      : "memory", "scc");
#endif
}

// ---- building blocks of the MFMA kernels (gemm.hip, attention.hip, attention_bwd.hip, backward.hip, mlp_fused.hip): one definition each ----

// XCD-aware tile order.  Workgroups are dealt round-robin over the 8 XCDs (ids congruent mod 8 share an XCD and its private L2): linear
// workgroup id `id` of a launch of `n` becomes a tile index such that every XCD walks one contiguous slice of the tile space -- the
// first n % 8 XCDs own n / 8 + 1 tiles, the others n / 8.  A bijection on [0, n) for every n; `n` must be the launch's workgroup count.
__device__ __forceinline__ int xcd_tile_order(int id, int n) {
  const int q = n / 8, rem = n % 8, xcd = id % 8;
  return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + id / 8;
}

// Which tiles of BK rows does split `split` of `splits` own, of n rows in all?  Tiles [begin, end); [begin, full_end) are whole, and
// end - 1 is the partial last tile iff the range is not empty and full_end < end (only the last live split can own it).
// Every split gets ceil(tiles / splits) tiles, so a trailing split is EMPTY whenever (splits - 1) * ceil(tiles / splits) >= tiles.  The
// hosts rule that out for a row count they know (attn_effective_splits, g96x2_applies); a key count read on the device
// (AttnParams::lk_dev) below the capacity the split count was sized for brings it back.  Then end = tiles < begin: test empty() /
// partial_tail() / count() <= 0, never full_end < end alone (min(end, n / BK) < end also holds for an empty range behind a partial
// tile, which would be taken a second time).  An empty split must report (max = -inf, sum = 0, O' = 0); the merge gives it weight 0.
struct TileRange {
  int begin, end, full_end;
  __device__ __forceinline__ int count() const { return end - begin; }   // <= 0: empty
  __device__ __forceinline__ bool empty() const { return begin >= end; }
  __device__ __forceinline__ bool partial_tail() const { return begin < end && full_end < end; }
};
__device__ __forceinline__ TileRange split_tiles(int n, int BK, int splits, int split) {
  const int tiles_total = (n + BK - 1) / BK;
  const int tiles_per = (tiles_total + splits - 1) / splits;
  const int begin = split * tiles_per;
  const int end = min(tiles_total, begin + tiles_per);
  return {begin, end, min(end, n / BK)};
}

// Transposed 16-bit fragment of a row-major LDS tile (A operand of O^T += V^T P^T and of the transposed-B GEMMs): two ds_read_b64_tr_b16,
// the second `hi_bytes` (8 rows, or 4 of a 16-row k-step image) behind the first, packed into the eight k-slots of a 32x32x16 operand.
__device__ __forceinline__ op16x8 lds_read_tr16_pair(const unsigned char* a0, int hi_bytes) {
  const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4_t __attribute__((address_space(3)))*)(a0));
  const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((short4_t __attribute__((address_space(3)))*)(a0 + hi_bytes));
  short8_t t8;
  t8[0] = lo[0]; t8[1] = lo[1]; t8[2] = lo[2]; t8[3] = lo[3];
  t8[4] = hi[0]; t8[5] = hi[1]; t8[6] = hi[2]; t8[7] = hi[3];
  return __builtin_bit_cast(op16x8, t8);
}

// Raw buffer descriptor over `bytes` bytes at p: stride 0 (raw addressing, offset = voffset + soffset), num_records = bytes -- a lane
// whose voffset is >= bytes reads 0 / drops its store (soffset is NOT range-checked on gfx9) -- and word 3 = 0x00020000 (DATA_FORMAT 32:
// the only field a raw gfx9 descriptor needs).  Default: 0x7fffffff, "no bound": the kernel clamps its rows itself.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_rsrc(const void* p, int bytes = 0x7fffffff) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// The ONLY way a kernel states a vector-memory wait: at most N of this wave's loads / LDS-DMA pieces / stores (one in-order counter) are
// still in flight afterwards.  Write N as a multiple of the kernel's pieces-per-wave constant where it is one.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int FM, int FN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[FM][FN]) {
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}
template <int FN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[FN]) {
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
}

// LDS image of a K-contiguous operand tile that LDS-DMA fills and ds_read_b128 fragment reads drain: rows of ROW_BYTES (128: 64 k per
// tile, 64: 32 k), the 16-byte chunk c of row r in slot c ^ swz(r).  swz spreads the rows that share a 256-byte bank row over distinct
// slots, so every 16-lane ds_read_b128 group of the 32x32x16 operand map (16 rows, one chunk) is conflict free.  The DMA writes LDS
// linearly (piece base + 16 * lane: lane l fills slot l % CPR of row l / CPR of its 1-KiB piece), so the swizzle is applied to the per-lane
// SOURCE address.  Both sides go through swz(): they cannot disagree.
template <int ROW_BYTES_>
struct DmaImage {
  static constexpr int ROW_BYTES = ROW_BYTES_;
  static_assert(ROW_BYTES == 128 || ROW_BYTES == 64, "two images exist: 128-byte rows, slot c ^ ((r >> 1) & 7); 64-byte rows, c ^ ((r >> 2) & 3)");
  static constexpr int CPR = ROW_BYTES / 16;            // chunks per row
  static constexpr int PIECE_ROWS = 1024 / ROW_BYTES;   // rows of one DMA piece (one instruction of a wave)
  __device__ __forceinline__ static int swz(int r) { return (r >> (ROW_BYTES == 128 ? 1 : 2)) & (CPR - 1); }
  // tile row that `lane` fills in DMA piece `piece` of the tile
  __device__ __forceinline__ static int piece_row(int piece, int lane) { return piece * PIECE_ROWS + (lane >> (ROW_BYTES == 128 ? 3 : 2)); }
  // DMA side: the chunk of its global row that `lane` must fetch for tile row r (it lands in slot lane % CPR)
  __device__ __forceinline__ static int src_chunk(int r, int lane) { return (lane & (CPR - 1)) ^ swz(r); }
  // fragment side: chunk c of row r is at byte r * ROW_BYTES + ((c ^ swz(r)) << 4) of the image
};
typedef DmaImage<128> Img128;
typedef DmaImage<64> Img64;

// Slot of 16-byte chunk c of row r in the LDS images with 192- / 384-byte rows (mlp_fused.hip's weight chunks, attention.hip's
// attn_winproj_kernel): conflict free for the 32-row ds_read_b128 fragment reads; applied where the image is filled and on the reads.
template <int RB>
__device__ __forceinline__ int mlp_swz(int c, int r) {
  if constexpr (RB == 192) return (c & ~3) | ((c & 3) ^ ((r >> 2) & 3));
  else return (c & ~7) | ((c & 7) ^ ((r >> 1) & 7));
}

// The 32x32 MFMA accumulator of lane (r = lane & 31, h = lane >> 5) holds column r, and in register e row (e & 3) + 8 * (e >> 2) + 4 * h.
// For S^T = K Q^T that row is the key of score register e (the column is the lane's query); for O^T it is the channel within a 32-block.
__device__ __forceinline__ constexpr int s_frag_key(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// Normalise-and-store of this lane's O^T column (one query row of DBLK * 32 channels) at dst: register 4 g + e of block d is channel
// 32 d + 8 g + 4 h + e (s_frag_key), so every group g is one 8-byte store.  A macro because a function changes the listing of EVERY kernel
// that calls it (after inlining the stores' address arithmetic loses its inbounds / no-wrap marks and the epilogue is scheduled
// differently); tools/isa_diff.py holds this text to the code the kernels had with the loop written out.
#define ATTN_STORE_O_ROWS(DBLK, dst, o, inv, h)                                           \
  do {                                                                                \
    op16* const dst_ = (dst);                                                         \
    _Pragma("unroll") for (int d_ = 0; d_ < DBLK; ++d_)                               \
      _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_) {                              \
        op16x4 w_;                                                                    \
        _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) w_[e_] = f2op((o)[d_][4 * g_ + e_] * (inv)); \
        *reinterpret_cast<op16x4*>(dst_ + d_ * 32 + 8 * g_ + 4 * (h)) = w_;           \
      }                                                                               \
  } while (0)

// host: raise kernel K's dynamic-LDS limit once per process (per kernel instance); the return code is ignored
template <auto K>
static inline void ensure_dyn_lds(int bytes) {
  static bool done = false;
  if (!done) {
    hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    done = true;
  }
}

// exact-erf GELU (nn.GELU default): gelu(x) = x Phi(x), Phi(x) = 0.5 (1 + erf(x / sqrt 2)).
// Phi(x) - 0.5 is odd: x Q(x^2) with Q a degree-8 polynomial in x^2 (minimax fit of the GELU's own absolute error on |x| <= 4.5, end
// value pinned so that Phi(+-4.5) = 1 / 0; outside, x is clamped: Phi(-4.5) = 3.4e-6).  |gelu_poly - gelu| <= 5e-5 absolute over all x
// (tests/test_kernels_gpu.py::test_gelu_epilogue_accuracy; a tenth of the op16 rounding of the GEMM operands that produce x).
// No transcendental: one v_med3 per element, everything else packed fp32 (v_pk_mul_f32 / v_pk_fma_f32: two elements per issue) --
// ~26 issue cycles per element against ~48 for the Abramowitz-Stegun erf (v_rcp + v_exp, 8 cycles each, + 12 ops) that it replaces;
// the activation is the whole epilogue of the fc1 GEMMs (as long as their MFMAs at K = 384) and 25-30 % of the fused MLP kernel.
// The scalar form is the same fma chain, so a value gets the same bits whichever form a kernel uses.  -DMSAM2_GELU_AS keeps the old form.
typedef __attribute__((ext_vector_type(2))) float f32x2;
#ifndef MSAM2_GELU_AS
#define MSAM2_GELU_X 4.5f
#define MSAM2_GELU_Q0 3.987085521e-01f
#define MSAM2_GELU_Q1 -6.597723812e-02f
#define MSAM2_GELU_Q2 9.580635466e-03f
#define MSAM2_GELU_Q3 -1.036248752e-03f
#define MSAM2_GELU_Q4 8.120908024e-05f
#define MSAM2_GELU_Q5 -4.431632988e-06f
#define MSAM2_GELU_Q6 1.580232549e-07f
#define MSAM2_GELU_Q7 -3.283848526e-09f
#define MSAM2_GELU_Q8 2.999938145e-11f
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 x) {
  const f32x2 xc = {__builtin_amdgcn_fmed3f(x[0], -MSAM2_GELU_X, MSAM2_GELU_X), __builtin_amdgcn_fmed3f(x[1], -MSAM2_GELU_X, MSAM2_GELU_X)};
  const f32x2 u = xc * xc;
  auto bc = [](float c) { return f32x2{c, c}; };
  f32x2 q = __builtin_elementwise_fma(u, bc(MSAM2_GELU_Q8), bc(MSAM2_GELU_Q7));
  q = __builtin_elementwise_fma(q, u, bc(MSAM2_GELU_Q6));
  q = __builtin_elementwise_fma(q, u, bc(MSAM2_GELU_Q5));
  q = __builtin_elementwise_fma(q, u, bc(MSAM2_GELU_Q4));
  q = __builtin_elementwise_fma(q, u, bc(MSAM2_GELU_Q3));
  q = __builtin_elementwise_fma(q, u, bc(MSAM2_GELU_Q2));
  q = __builtin_elementwise_fma(q, u, bc(MSAM2_GELU_Q1));
  q = __builtin_elementwise_fma(q, u, bc(MSAM2_GELU_Q0));
  const f32x2 phi = __builtin_elementwise_fma(xc, q, bc(0.5f));
  return x * phi;
}
// Phi(x) itself: the factor of the GELU and the first term of its derivative Phi(x) + x phi(x) (act_bwd_vec_kernel)
__device__ __forceinline__ float gelu_phi(float x) {
  const float xc = __builtin_amdgcn_fmed3f(x, -MSAM2_GELU_X, MSAM2_GELU_X);
  const float u = xc * xc;
  float q = __builtin_fmaf(u, MSAM2_GELU_Q8, MSAM2_GELU_Q7);
  q = __builtin_fmaf(q, u, MSAM2_GELU_Q6);
  q = __builtin_fmaf(q, u, MSAM2_GELU_Q5);
  q = __builtin_fmaf(q, u, MSAM2_GELU_Q4);
  q = __builtin_fmaf(q, u, MSAM2_GELU_Q3);
  q = __builtin_fmaf(q, u, MSAM2_GELU_Q2);
  q = __builtin_fmaf(q, u, MSAM2_GELU_Q1);
  q = __builtin_fmaf(q, u, MSAM2_GELU_Q0);
  return __builtin_fmaf(xc, q, 0.5f);
}
__device__ __forceinline__ float gelu_erf(float x) { return x * gelu_phi(x); }
#endif
// The same function with erf by Abramowitz-Stegun 7.1.26 (|abs error| <= 1.5e-7: at fp32 round-off):  erf(a) = sign(a) (1 - P(t) e^{-a^2}),
// t = 1 / (1 + p |a|);  gelu(x) = max(x, 0) - 0.5 |x| P(t) e^{-a^2}   (both signs; no 1 - (1 - ..) cancellation on the negative side).
// For kernels with fp32 outputs that are nowhere near VALU-bound (LayerNorm + GELU of the mask decoder's up-scaling).
__device__ __forceinline__ float gelu_erf_as(float x) {
  const float ab = fabsf(x);
  const float ax = ab * 0.70710678118654752440f;
  const float d = 1.0f + 0.3275911f * ax;
  const float t = __builtin_amdgcn_rcpf(d);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float arg = ax * ax * (-1.44269504088896340736f);
  const float ex = __builtin_amdgcn_exp2f(arg);
  return fmaxf(x, 0.f) - (ab * 0.5f) * (poly * ex);
}
#ifdef MSAM2_GELU_AS
__device__ __forceinline__ float gelu_erf(float x) { return gelu_erf_as(x); }
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 x) { return f32x2{gelu_erf_as(x[0]), gelu_erf_as(x[1])}; }
#endif
// erf itself (the GELU derivative of the backward pass)
__device__ __forceinline__ float fast_erf(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float e = 1.0f - poly * __expf(-ax * ax);
  return copysignf(e, x);
}
#ifdef MSAM2_GELU_AS
__device__ __forceinline__ float gelu_phi(float x) { return 0.5f * (1.f + fast_erf(x * 0.70710678118654752f)); }
#endif

// Counter-based dropout mask shared by the element-wise dropout kernel (backward.hip) and the flash attention kernels (attention.hip,
// attention_bwd.hip): element idx of stream seed is KEPT iff the upper half of splitmix64(seed + idx * golden) is >= thr = p * 2^32.
__device__ __forceinline__ bool dropout_keep(uint64_t seed, uint64_t idx, unsigned thr) {
  uint64_t z = seed + idx * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned)(z >> 32) >= thr;
}
// attention-probability dropout of a flash kernel (F.scaled_dot_product_attention(dropout_p) in train mode, transformer.py:317-318):
// probability (b, h, q, k) uses element offset + ((b * H + h) * Lq + q) * Lk + k of the stream; thr == 0 switches it off.
struct AttnDropout {
  unsigned thr;
  float inv_keep;
  uint64_t seed, offset;
  const uint64_t* seed_dev;      // optional: added to seed on the device (msam2_counter_bump)
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- building blocks of the pointwise and row kernels (elementwise.hip, conv.hip, backward.hip): one definition each ----

// sum over the 16 lanes that share a row in the 16-lanes-per-row LayerNorm kernels (lanes l ^ 1, 2, 4, 8: four shuffles), in place
// (layernorm_kernel: with the value form two of its instances are scheduled in another order) and as a value
__device__ __forceinline__ void group16_add(float& v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
}
__device__ __forceinline__ float group16_sum(float v) {
  group16_add(v);
  return v;
}

// layernorm_kernel's row arithmetic (elementwise.hip) with every rounding WRITTEN OUT, for the kernels that hold whole rows and finish
// them in their epilogue (conv_mfma.hip, and through rowtile.h gemm_rowln.hip and mlp_rowln.hip): the one statement of it outside that
// kernel.  layernorm_kernel's source leaves the choice of which multiply meets which add in one fma to the compiler
// (-ffp-contract=fast); the forms below are the ones its listings show, the same in every instance and in both builds, and contraction is
// switched off here so that no caller can be given other ones (conv3x3s2_mfma_kernel's 16-bit conversions invite the vectoriser to pair
// the multiplies first, which had split the GELU's `1 + 0.3275911 ax` into a product and a sum at C = 256: one output in 230 000 an ulp off).
//   A row of C elements lies in LPR lanes, CPL chunks of four per lane.  Sum and sum of squares: a lane adds its elements in order,
//   q = d1 d1, then fma(d0, d0, q), fma(d2, d2, q), ...; lanes meet through xor-shuffles, widest first (group16_add at LPR = 16; with
//   fewer live lanes the wider steps of that kernel add zeros and are left out);  value: fma(w, rstd (x - mean), b).
template <int CPL, int LPR, int C>
__device__ __forceinline__ void ln_row_stats(const float (&v)[CPL][4], float eps, float& mean, float& rstd) {
#pragma clang fp contract(off)
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < CPL; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) s += v[j][e];
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  mean = s / C;
  const float d0 = v[0][0] - mean, d1 = v[0][1] - mean;
  float q = d1 * d1;
  q = __builtin_fmaf(d0, d0, q);
#pragma unroll
  for (int i = 2; i < CPL * 4; ++i) {
    const float d = v[i >> 2][i & 3] - mean;
    q = __builtin_fmaf(d, d, q);
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  rstd = 1.0f / sqrtf(q / C + eps);
}
__device__ __forceinline__ float ln_row_value(float x, float mean, float rstd, float w, float b) {
#pragma clang fp contract(off)
  return __builtin_fmaf(w, rstd * (x - mean), b);
}

// the two pieces of the bicubic convolution kernel (A = -0.75 in torch): |x| <= 1 and 1 < |x| < 2 -- the position-table resize and its adjoint
__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

// element i of a [B, H/2, W/2, C] map (the output of a 2x2 / stride-2 pool over [B, H, W, C]) -> channel, output pixel, batch element
struct Pool2x2Index {
  int c, xo, yo, b;
  __device__ __forceinline__ Pool2x2Index(int64_t i, int C, int Ho, int Wo) {
    c = i % C;
    int64_t t = i / C;
    xo = t % Wo;
    t /= Wo;
    yo = t % Ho;
    b = t / Ho;
  }
};

// bilinear resize, align_corners = False: output o of a resize by scale = n_src / n_out reads sources i0 and i1 with weights 1 - l and l
struct BilinearTap {
  int i0, i1;
  float l;
  template <typename I>
  __device__ __forceinline__ BilinearTap(I o, float scale, int n_src) {
    const float f = fmaxf((o + 0.5f) * scale - 0.5f, 0.f);
    i0 = (int)f;
    i1 = min(i0 + 1, n_src - 1);
    l = f - i0;
  }
};

// pixel index of a [B, H, W] raster -> (x, y, b)
struct PixelIndex {
  int x, y;
  int64_t b;
  __device__ __forceinline__ PixelIndex(int64_t pix, int H, int W) : x((int)(pix % W)), y((int)((pix / W) % H)), b(pix / ((int64_t)W * H)) {}
};

// output pixel (b, Y, X) of a ConvTranspose2d(k2, s2) on the 2h x 2w grid -> its source token and which of the token's four outputs it is
struct ConvT2x2Index {
  int64_t tok;
  int sub;
  __device__ __forceinline__ ConvT2x2Index(int64_t b, int Y, int X, int h, int w) : tok((b * h + Y / 2) * w + X / 2), sub((Y & 1) * 2 + (X & 1)) {}
};

// Host side of those entries: the type ladder, the grid clamp and the "may I take the vector kernel" test, one statement each.
// An is_16bit flag of the ABI as a type: f(T{}) with T = op16 or float; nested for two or three flags.
template <typename F>
static inline void with_type(int is_16bit, F&& f) {
  if (is_16bit) f(op16{});
  else f(float{});
}

// workgroups of a grid-stride launch: one per `threads` elements, at most `cap` (the expression every site had: `min` takes its int overload
// here, so a total beyond 2^39 elements -- more than the device's memory holds -- would not be clamped)
static inline unsigned grid1d(int64_t total, int64_t cap, int64_t threads = 256) { return (unsigned)min(cap, (total + threads - 1) / threads); }

// The one flat pre-set of a table or workspace on the caller's stream: x[0 .. n) = value.  A kernel, never hipMemsetAsync / hipMemcpyAsync:
// issued inside a stream capture those became memset nodes that did not order reliably against the neighbouring kernel nodes (replays of a
// captured training step accumulated into stale data, NaNs from the third replay on, while eager launches were correct), so
// every in-library fill is a kernel and tests/test_fill_rule_cpu.py keeps it so.  A template in an unnamed namespace: emitted only in the
// code objects that instantiate it, with internal linkage per source.  Every table here is int32, or 64-bit words cleared to zero: <int>.
// Not flat fills, so kernels of their own: gemm_zero_kernel (strided 2-D view), gemm_tt_zero_kernel (strided, plus a column sum), zero2_kernel
// (two arrays in one launch), srf_zero_kernel (per-job tables), measure_init_kernel (five tables with three neutral elements).
namespace {
template <typename T> __global__ void fill_kernel(T* __restrict__ x, int64_t n, T value) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = value;
}
template <typename T> static inline void fill_on(hipStream_t s, T* x, int64_t n, T value) {
  if (n > 0) hipLaunchKernelGGL(fill_kernel<T>, dim3(grid1d(n, 2048)), dim3(256), 0, s, x, n, value);
}
}  // namespace

// Can every one of `a` take an access of N elements of S bytes?  A pointer: its address is a multiple of N S bytes (null passes: an
// optional tensor that is absent).  A stride in elements: every row it leads to keeps that alignment, i.e. it is a multiple of N.
static inline bool vec_ok1(const void* p, int64_t n, int64_t s) { return (uintptr_t)p % (uintptr_t)(n * s) == 0; }
static inline bool vec_ok1(int64_t ld, int64_t n, int64_t s) { return (ld * s) % (n * s) == 0; }
template <typename... A>
static inline bool vec_ok(int n, int s, A... a) { return (vec_ok1(a, n, s) && ...); }

// ---- building blocks of the label-volume and mask post-processing kernels (amg.hip, bank.hip, cc.hip, volume_labels.hip, prompts.hip,
// components.hip, holes.hip, surface.hip, morph.hip, clicks.hip, measure.hip, volume_prep.hip): one definition each.  What only the
// entries that work per organ inside a bounding box share (surface.hip, holes.hip, morph.hip) is in label_boxes.h ----

// integer siblings of wave_max: the result in all 64 lanes
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// Lock-free union-find over int parents in global memory (cc.hip, components.hip, holes.hip).  A parent only ever points to a lower index, so a
// find follows strictly decreasing indices and ends whatever other threads do; a union lowers the larger root with atomicMin and goes
// on from the value it found there when somebody lowered that parent first.  No thread waits for another.
__device__ __forceinline__ int uf_find(const int* parent, int n) {
  int p = __hip_atomic_load(parent + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != n) {                                          // p < n: strictly decreasing
    n = p;
    p = __hip_atomic_load(parent + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return n;
}
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  bool done;
  do {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a < b) {
      const int old = atomicMin(parent + b, a);
      done = (old == b);                                    // else somebody lowered parent[b] first: go on from there
      b = old;
    } else if (b < a) {
      const int old = atomicMin(parent + a, b);
      done = (old == a);
      a = old;
    } else {
      done = true;
    }
  } while (!done);
}

// number of set bits of ballot m below this lane: the lane's rank among the lanes that voted
__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// length of the run that starts at this lane, from the ballot of run heads: it ends where the next one starts, or with the wave
__device__ __forceinline__ int run_length(unsigned long long heads, int lane) {
  const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
  return rest ? __ffsll((long long)rest) : 64 - lane;
}

// The 256-entry LDS table label value -> index in ids[0 .. n), -1 = not listed, filled by a workgroup of 256 threads (tid = threadIdx.x).
// The first barrier also ends whatever the caller initialised in LDS before the call; the table may be read after the second.
// (label_stats_kernel of prompts.hip spells the same four lines out: its listing changes with the call.)
__device__ __forceinline__ void ids_to_object_table(signed char* lut, const uint8_t* ids, int n, int tid) {
  lut[tid] = -1;
  __syncthreads();
  if (tid < n) lut[ids[tid]] = (signed char)tid;
  __syncthreads();
}

// One wave's (|P & G|, |P|, |G|) added to the workgroup's LDS counters c[0 .. 3), by one lane; a zero costs no LDS access.  A macro: as a
// function it changes the register allocation of label_slices_kernel<1, true>.
// ci, cp and cg are each evaluated twice: pass values or expressions without side effects.
#define LABEL_OVERLAP_ADD(c, ci, cp, cg)  \
  do {                                    \
    if (ci) atomicAdd((c) + 0, ci);       \
    if (cp) atomicAdd((c) + 1, cp);       \
    if (cg) atomicAdd((c) + 2, cg);       \
  } while (0)

// Host side of those entries.  The limits of a label volume [D, H, W] and of the objects of one call (ops.py mirrors them by name):
constexpr int LABEL_MAX_OBJ = 32;                           // per-object tables live in LDS and in kernel arguments
constexpr int LABEL_MAX_SLICES = 65535;                     // slices ride in gridDim.y / gridDim.z
constexpr int LABEL_MAX_SIDE = 8192;                        // rows and columns (a row distance fits uint16 with 0xFFFF to spare)
constexpr int64_t LABEL_MAX_VOXELS = (1ll << 31) - 2;       // entries that hold a voxel index (+ 1) in an int32
constexpr int64_t LABEL_NO_VOXEL_CAP = INT64_MAX;           // entries that address voxels with 64-bit offsets
// Every entry states its own contract at the call site: the smallest H and W it takes (2 where a voxel needs an in-plane neighbour) and
// its voxel cap, LABEL_MAX_VOXELS or LABEL_NO_VOXEL_CAP (65535 x 8192 x 8192 < 2^63: the product cannot overflow behind the side tests).
static inline bool label_sizes_ok(int64_t D, int64_t H, int64_t W, int64_t min_side, int64_t max_voxels) {
  return D >= 1 && D <= LABEL_MAX_SLICES && H >= min_side && H <= LABEL_MAX_SIDE && W >= min_side && W <= LABEL_MAX_SIDE &&
         D * H * W <= max_voxels;
}
// The two refusals those entries share.  entry: a string literal; min_side: the literal 1 or 2 (it is printed); voxel_clause: "" or what
// the message says about the cap.
#define LABEL_REQUIRE_OBJECTS(entry, n) \
  MSAM2_REQUIRE((n) >= 1 && (n) <= LABEL_MAX_OBJ, entry ": n = %lld objects (1 .. %d per call)", (long long)(n), LABEL_MAX_OBJ)
#define LABEL_REQUIRE_SIZES(entry, D, H, W, min_side, max_voxels, voxel_clause)                                                             \
  MSAM2_REQUIRE(label_sizes_ok(D, H, W, min_side, max_voxels),                                                                              \
                entry ": bad sizes (D %lld of 1 .. %d, H x W %lldx%lld of " #min_side " .. %d" voxel_clause ")", (long long)(D), LABEL_MAX_SLICES, \
                (long long)(H), (long long)(W), LABEL_MAX_SIDE)
#define LABEL_AT_MOST_2G_VOXELS ", at most 2^31 - 2 voxels"
