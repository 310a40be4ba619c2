// After the overlap scores: exact anisotropic squared Euclidean distances on uint8 label volumes [D, H, W] -- the dense transform of one value
// inside one box (msam2_label_edt) and the surface distances behind HD95 / ASSD / NSD for up to 32 organs and both directions in one call
// (msam2_label_surface_distances), gfx950.
//
// Definitions.  A voxel is on the surface of value v iff it equals v and a face neighbour differs from v or lies outside the
// volume (6 neighbours; D == 1: the 4 in plane).  d2(q, F) = min over f in F of ((sx2 dx^2 + sy2 dy^2) + sz2 dz^2) in float64, every product
// and sum rounded on its own (this file is compiled with fp contraction off: no fused multiply-add), +inf for an empty F.  Float64 addition
// and multiplication by a positive constant are monotone, so the minimum is taken axis by axis and has the bits of the brute-force minimum
// (the bodies of the row pass and of the two scans are edt_passes.h's, which morph.hip shares):
//   * rows: one wave per row of the box, 64 columns at a time.  The features are marked on the fly from the label bytes; a ballot and one
//     count-leading-zeros give every lane the nearest feature at or left of it, the last feature column is carried from chunk to chunk
//     (wave-uniform); a second sweep from the right end (a feature is where the left distance is 0) takes the smaller one.  uint16 per
//     voxel, 0xFFFF = no feature in this row of the box.  A row with a feature sets its slice's flag.
//   * columns: one lane per voxel, lanes along x, so every step of the scan is one coalesced load across the wave.  Candidates y' in order of
//     increasing |dy|; the scan stops once sy2 dy^2 is not below the best so far -- exact: the other term is >= 0 and rounding is monotone,
//     so every later candidate is >= sy2 dy^2 >= best.  float64 per voxel; a slice without a flag is +inf without a scan.
//   * z: the same pruned scan along z.  The dense entry writes the field; the batch entry evaluates only at the query surface voxels and
//     appends the values to the (organ, direction)'s segment: one atomic add per workgroup of 2048 voxels, ballot ranks within it.  The
//     order inside a segment depends on scheduling, the multiset does not: the wrapper sorts.
// Boxes are host integers and travel to the kernels by value (SrfJobs).  Apart from the workgroup barrier around that one add no thread waits
// for another: no spin, no grid barrier, no cooperative launch.
#include "edt_passes.h"
#include "label_boxes.h"

#pragma clang fp contract(off)

namespace {

constexpr int SRF_THREADS = 256;
enum { SRF_SURFACE = 0, SRF_OUTSIDE = 1 };

struct SrfOrgan : LabelBox {                                // the box
  int value;
  int cap[2];                                               // per direction: elements of the segment
  int pad_;
  long long ws;                                             // byte offset of this organ's share of the workspace (both directions)
  long long seg[2];                                         // per direction: first element of the segment
};
struct SrfJobs {                                            // a kernel argument: 2 KiB
  int n, D, H, W;
  SrfOrgan o[LABEL_MAX_OBJ];
};

// one direction's share: t float64 per voxel, g uint16 per voxel, one int32 flag per slice of the box
__host__ __device__ __forceinline__ long long srf_dir_bytes(long long bd, long long vox) {
  return vox * 8 + label_round8(vox * 2) + label_round8(bd * 4);
}

struct SrfBufs {
  double* t;
  uint16_t* g;
  int* flag;
};
__device__ __forceinline__ SrfBufs srf_bufs(char* ws, const SrfOrgan& o, int dir) {
  const long long vox = label_box_voxels(o);
  char* base = ws + o.ws + dir * srf_dir_bytes(o.bd, vox);
  return {(double*)base, (uint16_t*)(base + vox * 8), (int*)(base + vox * 8 + label_round8(vox * 2))};
}

// Is voxel (z, y, x) of the volume on the surface of v?  Nothing is read outside the volume.
__device__ __forceinline__ bool srf_on_surface(const uint8_t* __restrict__ vol, int D, int H, int W, int z, int y, int x, int v) {
  const int64_t i = ((int64_t)z * H + y) * W + x;
  if (vol[i] != v) return false;
  if (x == 0 || x == W - 1 || y == 0 || y == H - 1) return true;
  if (vol[i - 1] != v || vol[i + 1] != v || vol[i - W] != v || vol[i + W] != v) return true;
  if (D == 1) return false;                                 // one slice is a 2-D image
  if (z == 0 || z == D - 1) return true;
  const int64_t HW = (int64_t)H * W;
  return vol[i - HW] != v || vol[i + HW] != v;
}

typedef LabelBoxVoxel<int64_t> SrfVoxel;                   // (the kernels here use the position in the box only)

// blockIdx.y = 2 * organ + direction.  Direction 0: queries from a, features from b; direction 1 the other way round.
__global__ __launch_bounds__(SRF_THREADS) void srf_zero_kernel(SrfJobs jobs, char* __restrict__ ws, int* __restrict__ counts) {
  const SrfOrgan& o = jobs.o[blockIdx.y >> 1];
  const int dir = blockIdx.y & 1;
  int* flag = srf_bufs(ws, o, dir).flag;
  for (int z = threadIdx.x; z < o.bd; z += SRF_THREADS) flag[z] = 0;
  if (counts && threadIdx.x == 0) counts[blockIdx.y] = 0;
}

__global__ __launch_bounds__(SRF_THREADS) void srf_row_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int mode, SrfJobs jobs,
                                                              char* __restrict__ ws) {
  const SrfOrgan& o = jobs.o[blockIdx.y >> 1];
  const int dir = blockIdx.y & 1;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (SRF_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= (int64_t)o.bd * o.bh) return;                  // wave-uniform
  const uint8_t* __restrict__ f = dir ? a : b;
  const SrfBufs bufs = srf_bufs(ws, o, dir);
  const int zb = (int)(row / o.bh), yb = (int)(row - (int64_t)zb * o.bh);
  const int z = o.z0 + zb, y = o.y0 + yb;
  const int64_t at = ((int64_t)z * jobs.H + y) * jobs.W + o.x0;
  const bool any = edt_row_pass(bufs.g + row * o.bw, o.bw, lane, [&](int xb) {
    return mode == SRF_SURFACE ? srf_on_surface(f, jobs.D, jobs.H, jobs.W, z, y, o.x0 + xb, o.value) : f[at + xb] != o.value;
  });
  if (any && lane == 0) bufs.flag[zb] = 1;                  // (every row of the slice that has a feature stores the same 1)
}

__global__ __launch_bounds__(SRF_THREADS) void srf_col_kernel(SrfJobs jobs, char* __restrict__ ws, double sx2, double sy2) {
  const SrfOrgan& o = jobs.o[blockIdx.y >> 1];
  const int dir = blockIdx.y & 1;
  const int64_t vox = label_box_voxels(o);
  const int64_t i = (int64_t)blockIdx.x * SRF_THREADS + threadIdx.x;
  if (i >= vox) return;
  const SrfBufs bufs = srf_bufs(ws, o, dir);
  const int64_t r = i / o.bw;                               // (LabelBoxVoxel's position, spelled out: with it the listing changes)
  const int xb = (int)(i - r * o.bw);
  const int zb = (int)(r / o.bh), yb = (int)(r - (int64_t)zb * o.bh);
  double best = __builtin_huge_val();
  if (bufs.flag[zb]) best = edt_scan_y(bufs.g + (int64_t)zb * o.bh * o.bw + xb, o.bw, yb, o.bh, sx2, sy2, best);
  bufs.t[i] = best;
}

// min over z' of (t[z', y, x] + sz2 dz^2) for box voxel (zb, yb, xb)
__device__ __forceinline__ double srf_scan_z(const double* __restrict__ t, const SrfOrgan& o, int zb, int yb, int xb, double sz2) {
  return edt_scan_z(t + (int64_t)yb * o.bw + xb, (int64_t)o.bh * o.bw, zb, o.bd, sz2, __builtin_huge_val());
}

__global__ __launch_bounds__(SRF_THREADS) void srf_z_dense_kernel(SrfJobs jobs, char* __restrict__ ws, double sz2, double* __restrict__ out) {
  const SrfOrgan& o = jobs.o[0];
  const int64_t i = (int64_t)blockIdx.x * SRF_THREADS + threadIdx.x;
  if (i >= label_box_voxels(o)) return;
  const SrfVoxel v(i, o, jobs.H, jobs.W);
  out[i] = srf_scan_z(srf_bufs(ws, o, 0).t, o, v.zb, v.yb, v.xb, sz2);
}

// A workgroup owns SRF_Z_ITER x 256 consecutive box voxels.  First sweep: which of them are query voxels (one bit per round and lane, one
// popcount per round and wave); then ONE atomic add per workgroup reserves its part of the segment -- a wave of a thin shell holds a
// handful of queries, and adds to the one counter of an (organ, direction) serialise in L2; second sweep: the scans and the stores.
constexpr int SRF_Z_ITER = 8;

__global__ __launch_bounds__(SRF_THREADS) void srf_z_query_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, SrfJobs jobs,
                                                                  char* __restrict__ ws, double sz2, double* __restrict__ out,
                                                                  int* __restrict__ counts) {
  __shared__ int wave_count[SRF_THREADS / 64];
  __shared__ int block_base;
  const SrfOrgan& o = jobs.o[blockIdx.y >> 1];
  const int dir = blockIdx.y & 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t vox = label_box_voxels(o);
  const int64_t first = (int64_t)blockIdx.x * (SRF_Z_ITER * SRF_THREADS);
  if (first >= vox) return;                                 // the whole workgroup: the grid is sized for the largest box
  const uint8_t* __restrict__ q = dir ? b : a;
  unsigned mine = 0;                                        // bit `it`: this lane's voxel of round `it` is a query
  int in_wave = 0;                                          // wave-uniform
#pragma unroll 1
  for (int it = 0; it < SRF_Z_ITER; ++it) {
    const int64_t i = first + it * SRF_THREADS + threadIdx.x;
    bool query = false;
    if (i < vox) {
      const SrfVoxel v(i, o, jobs.H, jobs.W);
      query = srf_on_surface(q, jobs.D, jobs.H, jobs.W, o.z0 + v.zb, o.y0 + v.yb, o.x0 + v.xb, o.value);
    }
    mine |= (query ? 1u : 0u) << it;
    in_wave += (int)__popcll(__ballot(query));
  }
  if (lane == 0) wave_count[wave] = in_wave;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < SRF_THREADS / 64; ++w) total += wave_count[w];
    block_base = total ? atomicAdd(counts + blockIdx.y, total) : 0;
  }
  __syncthreads();
  if (in_wave == 0) return;                                 // wave-uniform
  int64_t at = block_base;
  for (int w = 0; w < wave; ++w) at += wave_count[w];
  const double* __restrict__ t = srf_bufs(ws, o, dir).t;
#pragma unroll 1
  for (int it = 0; it < SRF_Z_ITER; ++it) {
    const bool query = (mine >> it) & 1u;
    const unsigned long long qm = __ballot(query);
    if (query) {
      const int64_t slot = at + lanes_below(qm, lane);
      if (slot < o.cap[dir]) {                              // past the capacity: counted, not stored
        const SrfVoxel v(first + it * SRF_THREADS + threadIdx.x, o, jobs.H, jobs.W);
        out[o.seg[dir] + slot] = srf_scan_z(t, o, v.zb, v.yb, v.xb, sz2);
      }
    }
    at += (int)__popcll(qm);
  }
}

bool srf_rows_ok(const int32_t* box) { return label_box_rows(label_box(box)) <= LABEL_MAX_BOX_ROWS; }
void srf_set_box(SrfOrgan& o, const int32_t* box) { static_cast<LabelBox&>(o) = label_box(box); }

// the three passes up to t, for jobs.n organs and `dirs` directions
void srf_launch_fields(const uint8_t* a, const uint8_t* b, int mode, const SrfJobs& jobs, int dirs, char* ws, double sy, double sx, int* counts,
                       hipStream_t s) {
  int64_t rows = 1, vox = 1;
  for (int j = 0; j < jobs.n; ++j) {
    const int64_t r = label_box_rows(jobs.o[j]), v = label_box_voxels(jobs.o[j]);
    if (r > rows) rows = r;
    if (v > vox) vox = v;
  }
  const unsigned gy = dirs == 2 ? 2 * jobs.n : 1;           // dense: organ 0, direction 0
  hipLaunchKernelGGL(srf_zero_kernel, dim3(1, gy), dim3(SRF_THREADS), 0, s, jobs, ws, counts);
  hipLaunchKernelGGL(srf_row_kernel, dim3(cdiv(rows, SRF_THREADS / 64), gy), dim3(SRF_THREADS), 0, s, a, b, mode, jobs, ws);
  hipLaunchKernelGGL(srf_col_kernel, dim3(cdiv(vox, SRF_THREADS), gy), dim3(SRF_THREADS), 0, s, jobs, ws, sx * sx, sy * sy);
}

}  // namespace

extern "C" size_t msam2_label_edt_workspace_bytes(int64_t bd, int64_t bh, int64_t bw) {
  if (!label_sizes_ok(bd, bh, bw, 1, LABEL_MAX_VOXELS) || bd * bh > LABEL_MAX_BOX_ROWS) return 0;   // a box may be one row or column thin
  return (size_t)srf_dir_bytes(bd, bd * bh * bw);
}

extern "C" int msam2_label_edt(const uint8_t* labels, int64_t D, int64_t H, int64_t W, int value, int features, const int32_t* box, double sz,
                               double sy, double sx, double* d2, void* workspace, size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(labels && d2 && workspace, "label_edt: null labels / d2 / workspace");
  LABEL_REQUIRE_SIZES("label_edt", D, H, W, 2, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(value >= 0 && value <= 255, "label_edt: value %d (0 .. 255)", value);
  MSAM2_REQUIRE(features == SRF_SURFACE || features == SRF_OUTSIDE, "label_edt: features %d (0: the surface of value, 1: the voxels != value)",
                features);
  LABEL_REQUIRE_SPACING("label_edt", sz, sy, sx);
  const int32_t whole[6] = {0, (int32_t)D - 1, 0, (int32_t)H - 1, 0, (int32_t)W - 1};
  if (!box) box = whole;                                    // host integers (z0, z1, y0, y1, x0, x1), inclusive
  MSAM2_REQUIRE(label_box_ok(box, D, H, W), "label_edt: box (%d..%d, %d..%d, %d..%d) is inverted or outside the %lld x %lld x %lld volume", box[0],
                box[1], box[2], box[3], box[4], box[5], (long long)D, (long long)H, (long long)W);
  MSAM2_REQUIRE(srf_rows_ok(box), "label_edt: the box has more than 2^25 rows (slices x rows: %lld)", (long long)label_box_rows(label_box(box)));
  SrfJobs jobs = {};
  jobs.n = 1, jobs.D = (int)D, jobs.H = (int)H, jobs.W = (int)W;
  srf_set_box(jobs.o[0], box);
  jobs.o[0].value = value;
  const size_t need = msam2_label_edt_workspace_bytes(jobs.o[0].bd, jobs.o[0].bh, jobs.o[0].bw);
  MSAM2_REQUIRE(workspace_bytes >= need, "label_edt: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
  MSAM2_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)d2 & 7) == 0, "label_edt: d2 / workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  srf_launch_fields(labels, labels, features, jobs, 1, (char*)workspace, sy, sx, nullptr, s);
  hipLaunchKernelGGL(srf_z_dense_kernel, dim3(cdiv(label_box_voxels(jobs.o[0]), SRF_THREADS)), dim3(SRF_THREADS), 0, s, jobs, (char*)workspace, sz * sz,
                     d2);
  return msam2_check_launch("label_edt");
}

// boxes: HOST int32 [n, 6]
extern "C" size_t msam2_label_surface_distances_workspace_bytes(const int32_t* boxes, int64_t n) {
  if (!boxes || n < 1 || n > LABEL_MAX_OBJ) return 0;
  size_t total = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int32_t* bx = boxes + 6 * j;
    if (!label_box_ok(bx, LABEL_MAX_SLICES, LABEL_MAX_SIDE, LABEL_MAX_SIDE)) return 0;
    const LabelBox e = label_box(bx);
    const size_t one = msam2_label_edt_workspace_bytes(e.bd, e.bh, e.bw);
    if (!one) return 0;
    total += 2 * one;
  }
  return total;
}

extern "C" int msam2_label_surface_distances(const uint8_t* pred, const uint8_t* gt, int64_t D, int64_t H, int64_t W, const uint8_t* ids,
                                             const int32_t* boxes, const int64_t* seg_offsets, const int32_t* capacity, int64_t n, double sz,
                                             double sy, double sx, double* dist, int64_t dist_len, int32_t* counts, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(pred && gt && ids && boxes && seg_offsets && capacity && dist && counts && workspace,
                "label_surface_distances: null pred / gt / ids / boxes / seg_offsets / capacity / dist / counts / workspace");
  LABEL_REQUIRE_OBJECTS("label_surface_distances", n);
  LABEL_REQUIRE_SIZES("label_surface_distances", D, H, W, 2, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  LABEL_REQUIRE_SPACING("label_surface_distances", sz, sy, sx);
  MSAM2_REQUIRE(dist_len >= 0, "label_surface_distances: dist_len %lld", (long long)dist_len);
  SrfJobs jobs = {};
  jobs.n = (int)n, jobs.D = (int)D, jobs.H = (int)H, jobs.W = (int)W;
  long long at = 0;
  for (int j = 0; j < (int)n; ++j) {
    const int32_t* bx = boxes + 6 * j;
    LABEL_REQUIRE_BOX("label_surface_distances", j, bx, D, H, W);
    MSAM2_REQUIRE(srf_rows_ok(bx), "label_surface_distances: box %d has more than 2^25 rows (slices x rows: %lld)", j,
                  (long long)label_box_rows(label_box(bx)));
    SrfOrgan& o = jobs.o[j];
    srf_set_box(o, bx);
    o.value = ids[j];                                       // ids: HOST bytes, like the boxes
    o.ws = at;
    at += 2 * srf_dir_bytes(o.bd, label_box_voxels(o));
    for (int d = 0; d < 2; ++d) {
      o.cap[d] = capacity[2 * j + d];
      o.seg[d] = seg_offsets[2 * j + d];
      MSAM2_REQUIRE(o.cap[d] >= 0 && o.seg[d] >= 0 && o.seg[d] + o.cap[d] <= dist_len,
                    "label_surface_distances: segment (%d, %d) = [%lld, %lld + %d) leaves dist (%lld elements)", j, d, o.seg[d], o.seg[d], o.cap[d],
                    (long long)dist_len);
    }
  }
  MSAM2_REQUIRE(workspace_bytes >= (size_t)at, "label_surface_distances: workspace too small (%zu of %zu bytes)", workspace_bytes, (size_t)at);
  MSAM2_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)dist & 7) == 0 && ((uintptr_t)counts & 3) == 0,
                "label_surface_distances: dist / workspace must be 8-byte aligned, counts 4-byte");
  hipStream_t s = (hipStream_t)stream;
  srf_launch_fields(pred, gt, SRF_SURFACE, jobs, 2, (char*)workspace, sy, sx, counts, s);
  int64_t vox = 1;
  for (int j = 0; j < jobs.n; ++j)
    if (label_box_voxels(jobs.o[j]) > vox) vox = label_box_voxels(jobs.o[j]);
  hipLaunchKernelGGL(srf_z_query_kernel, dim3(cdiv(vox, SRF_Z_ITER * SRF_THREADS), 2 * (unsigned)n), dim3(SRF_THREADS), 0, s, pred, gt, jobs,
                     (char*)workspace, sz * sz, dist, counts);
  return msam2_check_launch("label_surface_distances");
}
