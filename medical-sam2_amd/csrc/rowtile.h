// What the kernels that own whole output rows share (gemm_rowln.hip: gemm_rowln_kernel; mlp_rowln.hip: mlp_rowln_kernel): one definition
// each of the tile, its W prefetch, its k-step, its epilogue, and of what their C entries refuse and fill alike.  DESIGN.md 3.7 states
// the tile, 3.11 and 3.12 the kernels on it.
//   * The tile is 64 rows x all N columns for 512 threads: 8 waves = 2 row slabs (ws = wave >> 2) x 4 column quarters (wq = wave & 3), a
//     wave owning 32 x N / 4 as FN 32 x 32 accumulators; operands come through Img128 stages of BK = 64 (128-byte rows, 8-row pieces of
//     1 KB, N / 64 W pieces per wave and stage); the epilogue tile is [64][N + 4] fp32 and aliases whatever LDS the main loop used.
//   * tools/isa_diff.py holds these kernels to the code they were measured with.  The fragment reads of a k-step are a function.  The
//     other device parts are MACROS that are textually the code the kernels had: as functions they change the listing of the kernels
//     that call them (the epilogue's register allocation and schedule, the prefetch's scalar registers and one compare, the place of
//     zero_acc's moves in front of the MFMAs).  The macros name the kernel's thread coordinates as the kernels do: wave, lane, ws, wq,
//     r = lane & 31, h = lane >> 5.
//   * The kernels keep what differs: their main loops, `issue` lambdas, the merged-A prologue, fc1.
#pragma once
#include "common.h"
#include <initializer_list>

template <int N>
struct RowTile {
  static constexpr int BM = 64, BK = 64, KS = BK / 16;
  static constexpr int A_BYTES = BM * BK * 2;                 // a 64 x 64 image of 16-bit rows: 8 KB
  static constexpr int W_BYTES = N * BK * 2;                  // a stage of W: N rows x 64 k (N = 384: 48 KB)
  static constexpr int WPW = W_BYTES / 1024 / 8;              // its pieces per wave: 6
  static constexpr int FN = N / 4 / 32;                       // 32-column accumulators per wave: 3
  static constexpr int CH = N / 64;                           // 4-element chunks per lane and row of the epilogue walk: 6
  static constexpr int TLD = N + 4;                           // floats per row of the epilogue tile
  static constexpr int TILE_BYTES = BM * TLD * 4;             // 97 KB
  static_assert(N % 128 == 0 && WPW * 8 * Img128::PIECE_ROWS == N && BM == 8 * Img128::PIECE_ROWS, "8 waves share the pieces of a stage evenly");
};

// W prefetch.  The 32 workgroups of an XCD read the same weight in step, so each of its 128-byte line columns was one Infinity Cache round
// trip for all of them.  Workgroup j of its XCD (j = (blockIdx.x >> 3) & 31) sends its 1 / 32 of the weight -- `rows` rows from row
// j * rows on, cpr 16-byte chunks each -- through throw-away pieces to dst (this wave's KB of a ring stage nobody has filled yet): the
// whole weight is on its way into the XCD's L2 at once, and the pieces are older than the first stage, so they have landed before the
// first barrier lets anybody fill that stage.  dst is evaluated behind cpr and rows, where gemm_rowln_kernel had it (its scalar registers are named in that order).
#define ROWTILE_PREFETCH_W(w_rsrc, ldw, rows_, cpr_, j, dst)                                         \
  do {                                                                                               \
    const int j_ = (j), cpr = (cpr_), rows = (rows_), n = rows * cpr;                                \
    unsigned char* const dst_ = (dst);                                                               \
    for (int i = wave; i * 64 < n; i += 8) {                                                         \
      const int q = min(i * 64 + lane, n - 1);                                                       \
      const int row = j_ * rows + q / cpr, c = q - (q / cpr) * cpr;                                  \
      glds16(w_rsrc, dst_, (unsigned)((int64_t)row * (ldw) * 2 + c * 16), 0);                        \
    }                                                                                                \
  } while (0)

// One k-step of 64.  The fragments (a function: the listings are the same with it): A from image sa (row offset offA, swizzle swzA), W from
// stage sb (offB[j], swzB[j] of the wave's FN 32-row blocks), lane half h holding chunk 2 ks + h (gemm_glds_kernel's operand map).  Then
// KS x FN MFMAs, k ascending in every accumulator (a macro: as a function it moves zero_acc's sixteen moves in gemm_rowln_kernel<384, 0>).
template <int N>
__device__ __forceinline__ void rowtile_read_fragments(op16x8 (&af)[RowTile<N>::KS], op16x8 (&bfr)[RowTile<N>::KS][RowTile<N>::FN],
                                                       const unsigned char* sa, const unsigned char* sb, int offA, int swzA,
                                                       const int (&offB)[RowTile<N>::FN], const int (&swzB)[RowTile<N>::FN], int h) {
#pragma unroll
  for (int ks = 0; ks < RowTile<N>::KS; ++ks) {
    const int c = 2 * ks + h;
    af[ks] = *reinterpret_cast<const op16x8*>(sa + offA + ((c ^ swzA) << 4));
#pragma unroll
    for (int j = 0; j < RowTile<N>::FN; ++j) bfr[ks][j] = *reinterpret_cast<const op16x8*>(sb + offB[j] + ((c ^ swzB[j]) << 4));
  }
}
#define ROWTILE_MFMAS(N, acc, af, bfr)                                                                                         \
  _Pragma("unroll") for (int ks = 0; ks < RowTile<N>::KS; ++ks)                                                                \
    _Pragma("unroll") for (int j = 0; j < RowTile<N>::FN; ++j) acc[j] = MSAM2_MFMA_32x32x16(af[ks], bfr[ks][j], acc[j], 0, 0, 0)

// The epilogue, behind the barrier that ends the main loop (every wave past its last fragment read: the LDS is dead).  Every wave writes
// acc + bias_j as fp32 into the row-major tile at lds; barrier; the tile is walked in layernorm_kernel's geometry (16 lanes per row, 4 rows
// per wave, lane chunks l16 + 16 j) in two passes of 32 rows.  A lane's residual chunks, gamma and beta are loaded up front, before any
// store (one in-order counter: a load behind a store waits for the store's round trip).  x = (acc + bias) + r is gemm_epilogue_direct's
// fp32 + residual association; the LayerNorm is ln_row_stats / ln_row_value (common.h).  Rows past p.M are clamped on load and masked on
// store.  Y_OPTIONAL: a null p.Y ends the kernel behind the fp32 rows (uniform; no barrier follows).  p has R, C, ln_w, ln_b, Y, ldr,
// ldc, ldy, M, eps (rowtile_fill_out).
#define ROWTILE_EPILOGUE(N, Y_OPTIONAL, p, lds, m0, acc, bias_j)                                                               \
  do {                                                                                                                         \
    constexpr int FN = RowTile<N>::FN, CH = RowTile<N>::CH, TLD = RowTile<N>::TLD;                                             \
    /* row side first: everything a lane will load, before any store */                                                       \
    const int l16 = lane & 15;                                                                                                 \
    int64_t grow[2];                                                                                                           \
    f32x4 rv[2][CH], ww[CH], bb[CH];                                                                                           \
    _Pragma("unroll") for (int ps = 0; ps < 2; ++ps) {                                                                         \
      grow[ps] = m0 + ps * 32 + wave * 4 + (lane >> 4);                                                                        \
      const float* rr = p.R + min(grow[ps], (int64_t)p.M - 1) * p.ldr;                                                         \
      _Pragma("unroll") for (int j = 0; j < CH; ++j) rv[ps][j] = *reinterpret_cast<const f32x4*>(rr + (l16 + 16 * j) * 4);     \
    }                                                                                                                          \
    _Pragma("unroll") for (int j = 0; j < CH; ++j) {                                                                           \
      ww[j] = *reinterpret_cast<const f32x4*>(p.ln_w + (l16 + 16 * j) * 4);                                                    \
      bb[j] = *reinterpret_cast<const f32x4*>(p.ln_b + (l16 + 16 * j) * 4);                                                    \
    }                                                                                                                          \
    /* acc + bias -> the row-major tile: register e of lane (r, h) is row (e & 3) + 8 (e >> 2) + 4 h, column r of its block */ \
    float* tile = reinterpret_cast<float*>(lds);                                                                               \
    _Pragma("unroll") for (int j = 0; j < FN; ++j)                                                                             \
      _Pragma("unroll") for (int e = 0; e < 16; ++e)                                                                           \
        tile[(ws * 32 + s_frag_key(e, h)) * TLD + wq * (N / 4) + j * 32 + r] = acc[j][e] + bias_j[j];                          \
    __builtin_amdgcn_s_barrier();                                                                                              \
    /* x = (acc + bias) + r for both passes, and the fp32 rows */                                                             \
    float v[2][CH][4];                                                                                                         \
    _Pragma("unroll") for (int ps = 0; ps < 2; ++ps) {                                                                         \
      const float* trow = tile + (ps * 32 + wave * 4 + (lane >> 4)) * TLD;                                                     \
      _Pragma("unroll") for (int j = 0; j < CH; ++j) {                                                                         \
        const f32x4 t = *reinterpret_cast<const f32x4*>(trow + (l16 + 16 * j) * 4);                                            \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) v[ps][j][e] = t[e] + rv[ps][j][e];                                       \
      }                                                                                                                        \
    }                                                                                                                          \
    _Pragma("unroll") for (int ps = 0; ps < 2; ++ps) {                                                                         \
      if (grow[ps] < p.M) {                                                                                                    \
        float* cr = p.C + grow[ps] * p.ldc;                                                                                    \
        _Pragma("unroll") for (int j = 0; j < CH; ++j)                                                                         \
          *reinterpret_cast<f32x4*>(cr + (l16 + 16 * j) * 4) = f32x4{v[ps][j][0], v[ps][j][1], v[ps][j][2], v[ps][j][3]};      \
      }                                                                                                                        \
    }                                                                                                                          \
    if constexpr (Y_OPTIONAL) {                                                                                                \
      if (!p.Y) return;                                                                                                        \
    }                                                                                                                          \
    _Pragma("unroll") for (int ps = 0; ps < 2; ++ps) {                                                                         \
      float mean, rstd;                                                                                                        \
      ln_row_stats<CH, 16, N>(v[ps], p.eps, mean, rstd);                                                                       \
      if (grow[ps] < p.M) {                                                                                                    \
        op16* yr = p.Y + grow[ps] * p.ldy;                                                                                     \
        _Pragma("unroll") for (int j = 0; j < CH; ++j) {                                                                       \
          op16x4 o;                                                                                                            \
          _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = f2out<op16>(ln_row_value(v[ps][j][e], mean, rstd, ww[j][e], bb[j][e])); \
          *reinterpret_cast<op16x4*>(yr + (l16 + 16 * j) * 4) = o;                                                             \
        }                                                                                                                      \
      }                                                                                                                        \
    }                                                                                                                          \
  } while (0)

// ---- host: what the C entries of these kernels refuse and fill alike ----

// the output half of an entry's arguments
struct RowTileOut {
  const float* R32;      // [M, N] fp32 residual
  int64_t ldr;
  float* C32;            // [M, N] fp32
  int64_t ldc;
  const float* ln_w;
  const float* ln_b;
  float eps;
  void* Y16;             // [M, N] LayerNorm(C32 rows); null where the entry allows it
  int64_t ldy, M;
};
// a 16-bit operand that LDS-DMA reads through a buffer descriptor: rows of ld elements
struct RowTileDma {
  int64_t rows, ld;
};

// Refusals, in the order the entries have always made them, each text with the entry's name in front: the M range; the entry's `own`
// checks (the strides of its 16-bit operands, a workspace: a callable that returns 0 or has set the error); ldr / ldc / ldy; alignment
// -- 16 bytes for the 16-bit operands `op16` and the fp32 vectors `bias` (named by `aligned`, e.g. "A, W, bias") and for R32, C32, ln_w,
// ln_b, 8 bytes for Y16; null passes --; the 2 GB of a buffer descriptor's offsets for each of `dma` (named by `dma_names`, "A / W").
template <typename Own>
static int rowtile_check(const char* entry, const RowTileOut& o, int64_t N, Own own, std::initializer_list<const void*> op16,
                         std::initializer_list<const void*> bias, const char* aligned, std::initializer_list<RowTileDma> dma,
                         const char* dma_names) {
  MSAM2_REQUIRE(o.M > 0 && o.M < (1ll << 31) - 64, "%s: M=%lld", entry, (long long)o.M);
  if (const int err = own()) return err;
  MSAM2_REQUIRE(o.ldr % 4 == 0 && o.ldc % 4 == 0 && o.ldr >= N && o.ldc >= N && (!o.Y16 || (o.ldy % 4 == 0 && o.ldy >= N)),
                "%s: ldr, ldc, ldy must be multiples of 4, >= N", entry);
  bool ok = vec_ok(4, 4, (const void*)o.R32, (const void*)o.C32, (const void*)o.ln_w, (const void*)o.ln_b) && vec_ok(4, 2, (const void*)o.Y16);
  for (const void* q : op16) ok = ok && vec_ok(8, 2, q);
  for (const void* q : bias) ok = ok && vec_ok(4, 4, q);
  MSAM2_REQUIRE(ok, "%s: %s, R32, C32, ln_w, ln_b must be 16-byte aligned, Y16 8-byte", entry, aligned);
  for (const RowTileDma& d : dma) ok = ok && d.rows * d.ld * 2 < (1ll << 31);
  MSAM2_REQUIRE(ok, "%s: %s beyond the 2 GB of a buffer descriptor's offsets", entry, dma_names);
  return 0;
}

// the output half of RowLnParams / MlpRowLnParams (the members ROWTILE_EPILOGUE reads).  A null Y16 leaves ln_w, ln_b unused: the
// epilogue's up-front loads then read N valid floats of R32 that nobody uses
template <typename P>
static void rowtile_fill_out(P& p, const RowTileOut& o) {
  p.R = o.R32; p.C = o.C32; p.Y = (op16*)o.Y16;
  p.ln_w = o.Y16 ? o.ln_w : o.R32; p.ln_b = o.Y16 ? o.ln_b : o.R32;
  p.ldr = o.ldr; p.ldc = o.ldc; p.ldy = o.ldy;
  p.M = (int)o.M; p.eps = o.eps;
}
