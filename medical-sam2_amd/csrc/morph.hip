// Between the label volume and the scores: erosion, dilation, opening and closing of the organs of a uint8 label volume [D, H, W] by a ball
// of a physical radius, for up to 32 organs in one call (msam2_label_morph), gfx950.
//
// Definitions.  d2(q, f) = ((sx2 dx^2 + sy2 dy^2) + sz2 dz^2) in float64, every product and sum rounded on its own (this file
// is compiled with fp contraction off: no fused multiply-add): msam2_label_edt's.  The ball is {d2 <= r2}.  With M = {labels == v}:
//   dilate(M) = {q in the volume: min over f in M of d2(q, f) <= r2};
//   erode(M)  = {q in M: no voxel f of the volume outside M has d2(q, f) <= r2} -- beyond the volume there are no features, so an organ cut
//               by the field of view does not erode from the frame (msam2_label_edt with features 1);
//   open = dilate(erode(M)), close = erode(dilate(M)), both stages by the same two definitions.
// A ball is a threshold on the exact distance field, so every result is an integer volume with one definition.
//
// The field comes from the three passes of edt_passes.h with the scans capped just above r2: a value <= r2 is exact, every other value is
// "far", and a scan ends once the step alone leaves the ball: O(r / spacing) per voxel, not O(extent).
//
// Why a grown box suffices.  Let T hold every voxel of the organ and e_a be the largest k with s_a^2 k^2 <= r2 (the ball's extent).
//   * A voxel outside T grown by e differs from every voxel of T by more than e_a along some axis: d2 > r2 (the other terms are >= 0 and
//     rounding is monotone).  So dilate(M) lies in T grown by e, and its features, M, lie in T.
//   * For q in M the nearest voxel outside M lies in T grown by one voxel: a voxel f beyond that layer is at least two past T's end along
//     some axis a, and q moved along a to one past that end is in the volume, outside T, hence outside M, and nearer: its one term is
//     below f's term of that axis.  A volume that is all organ has no voxel outside M and does not erode.
//   * open: erode(M) and dilate(erode(M)), a subset of M, both lie in T: the box of the erosion serves both stages.
//   * close: dilate(M) lies in T grown by e, its erosion needs one voxel more: T grown by e + 1 serves both stages.
// Every grown box is clipped to the volume.  A larger box changes no result: the caller's boxes need only hold their organs.
//
// Per group of organs whose boxes fit the workspace, blockIdx.y = the organ: rows (uint16), columns and z (float64) of the first stage;
// the z kernel thresholds into a byte mask of the box; the second stage of open / close reads its features from that mask, never from the
// label bytes.  The last z kernel counts and, for erode / open, clears the organ's voxels that left the result: organs only ever touch
// their own voxels there.  dilate / close: one launch per organ in the order of ids over the organ's result set; an eligible voxel (input
// value 0; claim 1: any input value that is not in ids) is taken iff nobody took it before (out still holds its input value) or this
// organ's ORIGINAL mask is strictly nearer than the taker's: the first-stage distance, kept per box voxel, against the best so far, kept
// per voxel of the volume.  Stream order makes that "nearest wins, ties to the organ earlier in ids" without an atomic; a listed organ
// never loses a voxel.  A last launch counts every organ's voxels in out.  info meets through integer adds only.
// Before the first group out becomes a copy of labels; when out IS labels the copy goes to the workspace and every launch reads the input
// from there.  No thread waits for another: no spin, no grid barrier, no cooperative launch.
#include <cmath>

#include "edt_passes.h"
#define LABEL_BOXES_OUT
#include "label_boxes.h"

#pragma clang fp contract(off)

namespace {

constexpr int MOR_THREADS = 256;
enum { MOR_ERODE = 0, MOR_DILATE = 1, MOR_OPEN = 2, MOR_CLOSE = 3 };
// a stage: what it does, and whether its input set is the organ in the label bytes or the mask of the stage before
enum { MOR_STAGE_ERODE = 1, MOR_STAGE_FROM_MASK = 2, MOR_STAGE_KEEP_D = 4, MOR_STAGE_LAST = 8, MOR_STAGE_CLEAR = 16 };

struct MorOrgan : LabelBox {                                // the grown box
  int value, j;                                             // label value and index in ids / r2 / info
  double r2, cap;                                           // the ball, and the scans' bound: the float64 after r2
  long long ws;                                             // byte offset of the organ's tables in the workspace
};
struct MorJobs {
  int n, H, W, keep;                                        // keep: the tables hold the first-stage distance (dilate / close)
  MorOrgan o[LABEL_MAX_OBJ];
};
struct MorListed {                                          // bit v: v is one of ids
  uint32_t w[8];
};

// per box voxel: t float64, the first-stage distance float64 (keep), g uint16, the mask byte
static inline size_t mor_box_bytes(int64_t vox, bool keep) {
  return label_round16((size_t)vox * (keep ? 16 : 8) + (size_t)label_round8(vox * 2) + (size_t)label_round8(vox));
}

struct MorBufs {
  double* t;
  double* d1;
  uint16_t* g;
  uint8_t* mask;
};
__device__ __forceinline__ MorBufs mor_bufs(char* ws, const MorOrgan& o, int keep) {
  const int64_t vox = label_box_voxels(o);
  char* base = ws + o.ws;
  char* g = base + vox * (keep ? 16 : 8);
  return {(double*)base, (double*)(base + vox * 8), (uint16_t*)g, (uint8_t*)(g + label_round8(vox * 2))};
}

typedef LabelBoxVoxel<int64_t> MorVoxel;

// the features of a stage: erosion looks for the voxels outside its input set, dilation for the set itself
__global__ __launch_bounds__(MOR_THREADS) void mor_row_kernel(const uint8_t* __restrict__ src, MorJobs jobs, char* __restrict__ ws, int stage) {
  const MorOrgan& o = jobs.o[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (MOR_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= (int64_t)o.bd * o.bh) return;                  // wave-uniform
  const MorBufs bufs = mor_bufs(ws, o, jobs.keep);
  const int zb = (int)(row / o.bh), yb = (int)(row - (int64_t)zb * o.bh);
  const uint8_t* __restrict__ line = src + ((int64_t)(o.z0 + zb) * jobs.H + o.y0 + yb) * jobs.W + o.x0;
  const uint8_t* __restrict__ mline = bufs.mask + row * o.bw;
  const bool outside = stage & MOR_STAGE_ERODE, from_mask = stage & MOR_STAGE_FROM_MASK;
  const int v = o.value;
  edt_row_pass(bufs.g + row * o.bw, o.bw, lane, [&](int xb) { return (from_mask ? mline[xb] != 0 : line[xb] == v) != outside; });
}

__global__ __launch_bounds__(MOR_THREADS) void mor_col_kernel(MorJobs jobs, char* __restrict__ ws, double sx2, double sy2) {
  const MorOrgan& o = jobs.o[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * MOR_THREADS + threadIdx.x;
  if (i >= label_box_voxels(o)) return;
  const MorBufs bufs = mor_bufs(ws, o, jobs.keep);
  const int64_t r = i / o.bw;                               // (LabelBoxVoxel's position, spelled out: with it the listing changes)
  const int xb = (int)(i - r * o.bw);
  const int zb = (int)(r / o.bh), yb = (int)(r - (int64_t)zb * o.bh);
  bufs.t[i] = edt_scan_y(bufs.g + (int64_t)zb * o.bh * o.bw + xb, o.bw, yb, o.bh, sx2, sy2, o.cap);
}

// The threshold.  Every box voxel reads and writes its own mask byte only.  The last stage adds (voxels of the organ, voxels of the result)
// to info, one atomic per workgroup and counter; MOR_STAGE_CLEAR (erode / open): the result is final, the organ's other voxels become 0 and
// the result is also the organ's count afterwards.
__global__ __launch_bounds__(MOR_THREADS) void mor_z_kernel(const uint8_t* __restrict__ src, MorJobs jobs, char* __restrict__ ws, double sz2,
                                                            int stage, uint8_t* __restrict__ out, int* __restrict__ info) {
  __shared__ int cnt[2];
  const MorOrgan& o = jobs.o[blockIdx.y];
  const int64_t vox = label_box_voxels(o);
  if ((int64_t)blockIdx.x * MOR_THREADS >= vox) return;     // the whole workgroup: the grid is sized for the largest box
  const bool last = stage & MOR_STAGE_LAST;
  if (last) {
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * MOR_THREADS + threadIdx.x;
  bool organ = false, in = false;
  if (i < vox) {
    const MorBufs bufs = mor_bufs(ws, o, jobs.keep);
    const MorVoxel x(i, o, jobs.H, jobs.W);
    const double d = edt_scan_z(bufs.t + (int64_t)x.yb * o.bw + x.xb, (int64_t)o.bh * o.bw, x.zb, o.bd, sz2, o.cap);
    const bool near = d <= o.r2;
    organ = src[x.g] == o.value;
    if (stage & MOR_STAGE_ERODE) in = ((stage & MOR_STAGE_FROM_MASK) ? bufs.mask[i] != 0 : organ) && !near;
    else in = near;
    if (stage & MOR_STAGE_KEEP_D) bufs.d1[i] = d;
    bufs.mask[i] = in ? 1 : 0;
    if ((stage & MOR_STAGE_CLEAR) && organ && !in) out[x.g] = 0;
  }
  if (!last) return;
  const int n_organ = (int)__popcll(__ballot(organ)), n_in = (int)__popcll(__ballot(in));
  if ((threadIdx.x & 63) == 0) {
    if (n_organ) atomicAdd(&cnt[0], n_organ);
    if (n_in) atomicAdd(&cnt[1], n_in);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int* row = info + o.j * 4;
    if (cnt[0]) atomicAdd(row + 0, cnt[0]);
    if (cnt[1]) atomicAdd(row + 1, cnt[1]);
    if ((stage & MOR_STAGE_CLEAR) && cnt[1]) atomicAdd(row + 2, cnt[1]);
  }
}

// One organ per launch, in the order of ids.  src is the input (labels, or its snapshot when out is labels), never out; voxel g of out and
// of best is read and written by this thread alone.
__global__ __launch_bounds__(MOR_THREADS) void mor_claim_kernel(const uint8_t* __restrict__ src, MorOrgan o, int H, int W, char* __restrict__ ws,
                                                                MorListed listed, int claim_any, uint8_t* __restrict__ out,
                                                                double* __restrict__ best) {
  const int64_t i = (int64_t)blockIdx.x * MOR_THREADS + threadIdx.x;
  if (i >= label_box_voxels(o)) return;
  const MorBufs bufs = mor_bufs(ws, o, 1);
  if (!bufs.mask[i]) return;
  const MorVoxel x(i, o, H, W);
  const int in = src[x.g];
  const bool eligible = claim_any ? !((listed.w[in >> 5] >> (in & 31)) & 1u) : in == 0;
  if (!eligible) return;                                    // (the organ's own voxels are listed, or not 0)
  const double d = bufs.d1[i];
  // nobody took it: out holds the input value (a taken voxel holds an id, which an eligible input value never is)
  if (out[x.g] == in || d < best[x.g]) {
    out[x.g] = (uint8_t)o.value;
    best[x.g] = d;
  }
}

// after the last claim: (voxels of the organ in out, those of them that held another non-zero value)
__global__ __launch_bounds__(MOR_THREADS) void mor_count_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ out, MorJobs jobs,
                                                                int* __restrict__ info) {
  __shared__ int cnt[2];
  const MorOrgan& o = jobs.o[blockIdx.y];
  const int64_t vox = label_box_voxels(o);
  if ((int64_t)blockIdx.x * MOR_THREADS >= vox) return;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * MOR_THREADS + threadIdx.x;
  bool has = false, took = false;
  if (i < vox) {
    const MorVoxel x(i, o, jobs.H, jobs.W);
    const int in = src[x.g];
    has = out[x.g] == o.value;
    took = has && in != o.value && in != 0;
  }
  const int n_has = (int)__popcll(__ballot(has)), n_took = (int)__popcll(__ballot(took));
  if ((threadIdx.x & 63) == 0) {
    if (n_has) atomicAdd(&cnt[0], n_has);
    if (n_took) atomicAdd(&cnt[1], n_took);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (cnt[0]) atomicAdd(info + o.j * 4 + 2, cnt[0]);
    if (cnt[1]) atomicAdd(info + o.j * 4 + 3, cnt[1]);
  }
}

bool mor_r2_ok(double r2) { return r2 >= 0.0 && r2 < (double)INFINITY; }   // false for NaN; finite: the +inf of "no feature" is never inside

// the ball's extent along an axis of spacing s: the largest k in 0 .. lim with s^2 k^2 <= r2, in the arithmetic of the scans
int mor_reach(double s, double r2, int lim) {
  const double s2 = s * s, q = std::sqrt(r2 / s2);
  int k = q >= (double)lim ? lim : (int)q;
  while (k < lim && s2 * ((double)(k + 1) * (double)(k + 1)) <= r2) ++k;
  while (k > 0 && s2 * ((double)k * (double)k) > r2) --k;
  return k;
}

// the box the organ's stages run in: the caller's box grown per axis by what the op needs, clipped to the volume
void mor_grow(const int32_t* b, int op, double r2, double sz, double sy, double sx, int64_t D, int64_t H, int64_t W, int32_t* g) {
  const int one = op == MOR_DILATE ? 0 : 1, ball = op == MOR_DILATE || op == MOR_CLOSE;
  const int64_t dim[3] = {D, H, W};
  const double sp[3] = {sz, sy, sx};
  for (int a = 0; a < 3; ++a) {
    const int64_t by = one + (ball ? mor_reach(sp[a], r2, (int)dim[a] - 1) : 0);
    g[2 * a] = (int32_t)std::max<int64_t>(0, b[2 * a] - by);
    g[2 * a + 1] = (int32_t)std::min<int64_t>(dim[a] - 1, b[2 * a + 1] + by);
  }
}
bool mor_op_ok(int op) { return op >= MOR_ERODE && op <= MOR_CLOSE; }
bool mor_keeps(int op) { return op == MOR_DILATE || op == MOR_CLOSE; }
// the best distance per voxel of the volume (dilate / close), behind the snapshot
size_t mor_best_bytes(int64_t N, int op) { return mor_keeps(op) ? label_round16((size_t)N * 8) : 0; }

}  // namespace

// boxes: HOST int32 [n, 6], r2: HOST float64 [n].  in_place: out will be labels (the snapshot of the input rides in the workspace).
// all_at_once 0: the least the entry takes (its largest grown box alone); 1: what lets every organ go through one group.
extern "C" size_t msam2_label_morph_workspace_bytes(int64_t D, int64_t H, int64_t W, const int32_t* boxes, int64_t n, int op, const double* r2,
                                                    double sz, double sy, double sx, int in_place, int all_at_once) {
  if (!boxes || !r2 || n < 1 || n > LABEL_MAX_OBJ || !label_sizes_ok(D, H, W, 2, LABEL_MAX_VOXELS) || !mor_op_ok(op)) return 0;
  if (!label_spacing_ok(sz) || !label_spacing_ok(sy) || !label_spacing_ok(sx)) return 0;
  size_t bytes[LABEL_MAX_OBJ];
  for (int64_t j = 0; j < n; ++j) {
    if (!label_box_ok(boxes + 6 * j, D, H, W) || !mor_r2_ok(r2[j])) return 0;
    int32_t g[6];
    mor_grow(boxes + 6 * j, op, r2[j], sz, sy, sx, D, H, W, g);
    if (label_box_rows(label_box(g)) > LABEL_MAX_BOX_ROWS) return 0;
    bytes[j] = mor_box_bytes(label_box_voxels(label_box(g)), mor_keeps(op));
  }
  return label_input_bytes(D * H * W, in_place != 0) + mor_best_bytes(D * H * W, op) + label_tables_bytes(bytes, n, all_at_once != 0);
}

extern "C" int msam2_label_morph(const uint8_t* labels, int64_t D, int64_t H, int64_t W, const uint8_t* values, const int32_t* boxes, int64_t n, int op,
                                 const double* r2, double sz, double sy, double sx, int claim, uint8_t* out, int32_t* info, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(labels && values && boxes && r2 && out && info && workspace, "label_morph: null labels / values / boxes / r2 / out / info / workspace");
  LABEL_REQUIRE_OBJECTS("label_morph", n);
  LABEL_REQUIRE_SIZES("label_morph", D, H, W, 2, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(mor_op_ok(op), "label_morph: op %d (0: erode, 1: dilate, 2: open, 3: close)", op);
  MSAM2_REQUIRE(claim == 0 || claim == 1, "label_morph: claim %d (0: background voxels only, 1: any voxel whose value is not in values)", claim);
  LABEL_REQUIRE_SPACING("label_morph", sz, sy, sx);
  MorJobs all = {};                                         // every organ with its grown box, in the order of values
  all.n = (int)n, all.H = (int)H, all.W = (int)W, all.keep = mor_keeps(op) ? 1 : 0;
  MorListed listed = {};
  size_t bytes[LABEL_MAX_OBJ];
  for (int j = 0; j < (int)n; ++j) {                        // values, boxes, r2: HOST arrays
    LABEL_REQUIRE_DISTINCT_ID("label_morph", "values", values, j);
    MSAM2_REQUIRE(mor_r2_ok(r2[j]), "label_morph: r2[%d] = %g (a squared radius: >= 0 and finite)", j, r2[j]);
    LABEL_REQUIRE_BOX("label_morph", j, boxes + 6 * j, D, H, W);
    int32_t g[6];
    mor_grow(boxes + 6 * j, op, r2[j], sz, sy, sx, D, H, W, g);
    MorOrgan& o = all.o[j];
    static_cast<LabelBox&>(o) = label_box(g);
    MSAM2_REQUIRE(label_box_rows(o) <= LABEL_MAX_BOX_ROWS, "label_morph: the grown box %d has more than 2^25 rows (slices x rows: %lld)", j,
                  (long long)label_box_rows(o));
    o.value = values[j], o.j = j;
    o.r2 = r2[j], o.cap = std::nextafter(r2[j], (double)INFINITY);
    listed.w[values[j] >> 5] |= 1u << (values[j] & 31);
    bytes[j] = mor_box_bytes(label_box_voxels(o), mor_keeps(op));
  }
  const int64_t N = D * H * W;
  LABEL_REQUIRE_OUT("label_morph", labels, out, N);
  const size_t fixed = label_input_bytes(N, out == labels) + mor_best_bytes(N, op), need = fixed + label_tables_bytes(bytes, n, false);
  MSAM2_REQUIRE(workspace_bytes >= need, "label_morph: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
  MSAM2_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)info & 3) == 0, "label_morph: the workspace must be 16-byte aligned, info 4-byte");

  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const dim3 blk(MOR_THREADS);
  const uint8_t* src = label_begin_out(labels, out, N, ws, info, n, s);
  double* best = (double*)(ws + label_input_bytes(N, out == labels));   // (dilate / close; never read before it is written: see mor_claim_kernel)
  const double sx2 = sx * sx, sy2 = sy * sy, sz2 = sz * sz;
  // the stages: (first, second or -1), as flags of the row and z kernels
  const int first = (op == MOR_ERODE || op == MOR_OPEN ? MOR_STAGE_ERODE : 0) | (mor_keeps(op) ? MOR_STAGE_KEEP_D : 0) |
                    (op == MOR_ERODE ? MOR_STAGE_LAST | MOR_STAGE_CLEAR : 0) | (op == MOR_DILATE ? MOR_STAGE_LAST : 0);
  const int second = op == MOR_OPEN    ? MOR_STAGE_FROM_MASK | MOR_STAGE_LAST | MOR_STAGE_CLEAR
                     : op == MOR_CLOSE ? MOR_STAGE_FROM_MASK | MOR_STAGE_ERODE | MOR_STAGE_LAST
                                       : -1;
  int64_t all_vox = 1;
  for (int j = 0; j < (int)n;) {
    MorJobs jobs = {};
    jobs.H = (int)H, jobs.W = (int)W, jobs.keep = all.keep;
    int64_t vox = 1, rows = 1;
    j = label_next_group(bytes, (int)n, j, workspace_bytes - fixed, [&](int m, size_t at) {
      MorOrgan& o = jobs.o[jobs.n++];
      o = all.o[m];
      o.ws = (long long)(fixed + at);
      vox = std::max(vox, label_box_voxels(o)), rows = std::max(rows, label_box_rows(o));
    });
    all_vox = std::max(all_vox, vox);
    const dim3 by_row(cdiv(rows, MOR_THREADS / 64), jobs.n), by_voxel(cdiv(vox, MOR_THREADS), jobs.n);
    for (int stage : {first, second}) {
      if (stage < 0) break;
      hipLaunchKernelGGL(mor_row_kernel, by_row, blk, 0, s, src, jobs, ws, stage);
      hipLaunchKernelGGL(mor_col_kernel, by_voxel, blk, 0, s, jobs, ws, sx2, sy2);
      hipLaunchKernelGGL(mor_z_kernel, by_voxel, blk, 0, s, src, jobs, ws, sz2, stage, out, info);
    }
    if (mor_keeps(op))
      for (int k = 0; k < jobs.n; ++k) {
        const MorOrgan& o = jobs.o[k];
        hipLaunchKernelGGL(mor_claim_kernel, dim3(cdiv(label_box_voxels(o), MOR_THREADS)), blk, 0, s, src, o, (int)H, (int)W, ws, listed, claim, out,
                           best);
      }
  }
  if (mor_keeps(op))
    hipLaunchKernelGGL(mor_count_kernel, dim3(cdiv(all_vox, MOR_THREADS), (unsigned)n), blk, 0, s, src, (const uint8_t*)out, all, info);
  return msam2_check_launch("label_morph");
}
