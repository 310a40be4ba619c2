// After island removal: filling the enclosed holes of the organs of a uint8 label volume [D, H, W], 3-D or slice by slice, gfx950.
//
// A slice-propagating tracker leaves pin-holes and slice-wide gaps inside organs, lower-contrast interiors (lumen, lesions, a vessel that
// crosses the liver) do the same; the usual step after "keep the largest component" is scipy.ndimage.binary_fill_holes per organ.  This
// is its multi-organ form on the device and the dual problem of components.hip: for organ v = ids[j] the components of the COMPLEMENT
// {voxels != v} under the flood's connectivity (6 / 18 / 26 in 3-D; 4 / 8 in plane, every slice on its own) that hold no voxel of the
// frame (the six faces of the volume; in plane the four edges of the voxel's slice) are v's holes.  A hole's size counts all its voxels,
// whatever they carry; it qualifies iff max_voxels[j] == 0 or size <= max_voxels[j]; a voxel of it is eligible iff its input value is 0
// (claim 0) or always (claim 1); out[x] = ids[j*] for the smallest j* with x eligible in a qualifying hole of ids[j*], else labels[x].
// All holes are holes of the INPUT volume.  Everything is an integer; partial results meet through integer add / min atomics, everything
// else is a plain store whose order the stream fixes, so no output depends on scheduling.
//
// Why the organ's bounding box suffices.  Outside the box no voxel is v, so from a voxel outside it a straight line away from the box
// reaches the frame through the complement.  A complement voxel ON the box's boundary either lies on the frame or has such a voxel as
// its face neighbour: it is exterior.  A complement component of the volume that leaves the box does so by a step between neighbours,
// whose inside end is on the box's boundary; so the components of the complement INSIDE the box that hold no boundary voxel of the box
// are exactly v's holes.  In plane all steps stay in the slice: there the boundary is the box's four in-plane sides only, and a voxel on
// the box's first or last slice is not exterior for that.  A box with fewer than 3 rows or columns (3-D: or slices) holds no hole.
//
// msam2_label_fill_holes, per group of organs whose boxes fit the workspace (9 bytes per box voxel: an int32 union-find parent, an int32
// size at the root, an exterior byte at the root), blockIdx.y = the organ, one lane per box voxel in the box's raster order:
//   * runs: the binary class "labels != v" in place of components.hip's label byte: a ballot over "starts a run" (class differs from
//     the left lane, column 0 of the box, lane 0) gives every complement voxel its run's first voxel as its parent; size and the
//     exterior byte are zeroed in the same pass.
//   * merge: unions only between a run and the runs it touches in the BACKWARD neighbour rows of the connectivity, by the leftmost
//     witness of every (run, neighbour run) pair, with the lock-free union of common.h; rows and columns outside the box do not exist.
//   * exterior marks: the first voxel of every run on the box's boundary (and the run's last voxel on the box's last column) stores 1
//     to the exterior byte of its root -- the same value from every thread; no union with a sentinel node, which would serialise.
//   * sizes: the voxels of every component that is not exterior are added to size[root], one popcount per wave for the wave's first
//     hole, one add per run for the others; the exterior component (nearly the whole box) costs no atomic at all.
//   * apply, one launch per organ in the order of ids: a voxel of a qualifying hole is written iff it is eligible and out still holds
//     its input value (nobody claimed it: a claimed voxel holds an id its input differs from), so the smallest j wins by stream order
//     and every voxel is read and written by one thread per launch.  The four counters of info are gathered per workgroup in LDS and
//     added with one atomic per workgroup and counter.
// Before the first group out becomes a copy of labels; when out IS labels the copy goes to the workspace instead (D H W bytes) and
// every launch reads the input from there: in place gives the bytes of the out-of-place call.
// Every loop of every thread ends whatever other threads do: a find follows strictly decreasing indices, a union retries only after
// another thread lowered the parent it wanted to lower; no thread waits for another, no grid barrier, no cooperative launch.
#define LABEL_BOXES_OUT
#include "label_boxes.h"

namespace {

constexpr int HOL_THREADS = 256, HOL_ITER = 4;              // a workgroup owns HOL_ITER x 256 consecutive box voxels, a wave 64 at a time

struct HoleOrgan : LabelBox {                               // the box
  int value, j;                                             // label value and index in ids / max_voxels / info
  long long ws;                                             // byte offset of the organ's tables in the workspace
};
struct HoleJobs {
  int n, H, W, plane;                                       // plane: connectivity 4 / 8
  HoleOrgan o[LABEL_MAX_OBJ];
};

// a box that can hold a hole: the hole and the organ around it need 3 voxels along every axis the flood moves along
static inline bool hol_box_live(const LabelBox& b, bool plane) { return b.bh >= 3 && b.bw >= 3 && (plane || b.bd >= 3); }
// the tables of a box: 9 bytes per voxel; none for a box that holds no hole
static inline size_t hol_box_bytes(const int32_t* bx, bool plane) {
  const LabelBox b = label_box(bx);
  return hol_box_live(b, plane) ? label_round16((size_t)label_box_voxels(b) * 9) : 0;
}

typedef LabelBoxVoxel<int> HoleVoxel;                       // in int: a voxel of the volume is below 2^31 - 2
__device__ __forceinline__ int hol_voxels(const HoleOrgan& o) { return o.bd * o.bh * o.bw; }
__device__ __forceinline__ int* hol_parent(char* ws, const HoleOrgan& o) { return (int*)(ws + o.ws); }
__device__ __forceinline__ int* hol_size(char* ws, const HoleOrgan& o) { return (int*)(ws + o.ws) + hol_voxels(o); }
__device__ __forceinline__ uint8_t* hol_ext(char* ws, const HoleOrgan& o) { return (uint8_t*)((int*)(ws + o.ws) + 2 * (int64_t)hol_voxels(o)); }

// box voxel of this lane in round `it`: consecutive lanes hold consecutive box voxels, a wave's 64 never straddle two rounds
__device__ __forceinline__ int64_t hol_voxel(int it) { return ((int64_t)blockIdx.x * HOL_ITER + it) * HOL_THREADS + threadIdx.x; }

__global__ __launch_bounds__(HOL_THREADS) void hol_runs_kernel(const uint8_t* __restrict__ src, HoleJobs jobs, char* __restrict__ ws) {
  const HoleOrgan& o = jobs.o[blockIdx.y];
  const int V = hol_voxels(o);
  if ((int64_t)blockIdx.x * HOL_ITER * HOL_THREADS >= V) return;
  int* parent = hol_parent(ws, o);
  int* size = hol_size(ws, o);
  uint8_t* ext = hol_ext(ws, o);
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < HOL_ITER; ++it) {
    const int64_t gi = hol_voxel(it);
    const bool live = gi < V;
    const int li = live ? (int)gi : 0;
    const HoleVoxel x(li, o, jobs.H, jobs.W);
    const int cls = live && src[x.g] != o.value;
    unsigned long long heads;
    const int first = label_run_first(cls, x.xb, lane, &heads, [](int left) { return left == 0; });
    if (live) {
      if (cls) parent[li] = li - lane + first;              // nothing ever reads the parent of an organ voxel
      size[li] = 0;
      ext[li] = 0;
    }
  }
}

// The text of components.hip's cmp_merge_kernel with the class "labels != v" in place of the label byte and the box in place of the
// volume, kept as a text of its own so that neither listing moves: a fix to either belongs in the other too.
__global__ __launch_bounds__(HOL_THREADS) void hol_merge_kernel(const uint8_t* __restrict__ src, HoleJobs jobs, char* __restrict__ ws,
                                                                LabelRows rows) {
  const HoleOrgan& o = jobs.o[blockIdx.y];
  const int V = hol_voxels(o);
  if ((int64_t)blockIdx.x * HOL_ITER * HOL_THREADS >= V) return;
  int* parent = hol_parent(ws, o);
  const int lane = threadIdx.x & 63;
  const int v = o.value, bw = o.bw, bh = o.bh, W = jobs.W, HW = jobs.H * jobs.W;
#pragma unroll 1
  for (int it = 0; it < HOL_ITER; ++it) {
    const int64_t gi = hol_voxel(it);
    const bool live = gi < V;
    const int li = live ? (int)gi : 0;
    const HoleVoxel x(li, o, jobs.H, W);
    const int b = live && src[x.g] != v;
    if (__ballot(b != 0) == 0ull) continue;                 // wave-uniform: the shuffles below see whole waves
    const int col = x.xb;
    int pb = __shfl_up(b, 1);
    if (lane == 0) pb = (live && col > 0) ? src[x.g - 1] != v : 0;
    const bool left_same = col > 0 && b != 0 && pb != 0;    // the voxel to the left belongs to the same run
    if (lane == 0 && left_same) uf_union(parent, li, li - 1);    // the run was cut at this wave's first lane
    // the neighbour rows' classes first, by all lanes (wave-uniform control flow around the shuffles), the unions afterwards
    int ni[4], M[4], L[4], R[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = live && k < rows.count && x.zb + rows.dd[k] >= 0 && x.yb + rows.dr[k] >= 0 && x.yb + rows.dr[k] < bh;
      ni[k] = valid ? li + rows.dd[k] * bh * bw + rows.dr[k] * bw : -1;   // same column of the neighbour row, in the box
      const int ng = x.g + rows.dd[k] * HW + rows.dr[k] * W;              // and in the volume
      M[k] = valid ? src[ng] != v : 0;
      // left and right of it in that row: the neighbouring lanes hold them unless this lane is the wave's first / last
      L[k] = __shfl_up(M[k], 1), R[k] = __shfl_down(M[k], 1);
      if (lane == 0) L[k] = (valid && col > 0) ? src[ng - 1] != v : 0;
      if (lane == 63) R[k] = (valid && col + 1 < bw) ? src[ng + 1] != v : 0;
      if (col == 0) L[k] = 0;
      if (col + 1 >= bw) R[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (b == 0 || ni[k] < 0) continue;
      if (rows.wide[k]) {
        // M is of the neighbour run that also holds L / R when they are set; the leftmost voxel of this run that sees it joins them
        if (M[k]) {
          if (!left_same) uf_union(parent, li, ni[k]);
        } else {
          if (R[k]) uf_union(parent, li, ni[k] + 1);        // a neighbour run that starts at col + 1: nobody further left sees it
          if (L[k] && !left_same) uf_union(parent, li, ni[k] - 1);
        }
      } else if (M[k] && !(left_same && L[k])) {
        uf_union(parent, li, ni[k]);
      }
    }
  }
}

// The parents are final: nothing writes them in this launch or later, so path walking has no race.
__global__ __launch_bounds__(HOL_THREADS) void hol_mark_kernel(const uint8_t* __restrict__ src, HoleJobs jobs, char* __restrict__ ws) {
  const HoleOrgan& o = jobs.o[blockIdx.y];
  const int V = hol_voxels(o);
  if ((int64_t)blockIdx.x * HOL_ITER * HOL_THREADS >= V) return;
  const int* parent = hol_parent(ws, o);
  uint8_t* ext = hol_ext(ws, o);
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < HOL_ITER; ++it) {
    const int64_t gi = hol_voxel(it);
    const bool live = gi < V;
    const int li = live ? (int)gi : 0;
    const HoleVoxel x(li, o, jobs.H, jobs.W);
    const bool edge = x.yb == 0 || x.yb == o.bh - 1 || x.xb == 0 || x.xb == o.bw - 1 || (!jobs.plane && (x.zb == 0 || x.zb == o.bd - 1));
    const int cls = live && src[x.g] != o.value;
    const int pc = __shfl_up(cls, 1);
    const bool head = lane == 0 || x.xb == 0 || pc == 0;    // a row of the boundary marks once per run, not once per voxel
    if (cls && edge && (head || x.xb == o.bw - 1)) ext[uf_find(parent, li)] = 1;
  }
}

// A voxel that does not start a run is never a root: only the run's first lane walks the parents, the others take its result by shuffle.
__global__ __launch_bounds__(HOL_THREADS) void hol_size_kernel(const uint8_t* __restrict__ src, HoleJobs jobs, char* __restrict__ ws) {
  const HoleOrgan& o = jobs.o[blockIdx.y];
  const int V = hol_voxels(o);
  if ((int64_t)blockIdx.x * HOL_ITER * HOL_THREADS >= V) return;
  const int* parent = hol_parent(ws, o);
  int* size = hol_size(ws, o);
  const uint8_t* ext = hol_ext(ws, o);                      // final: written by the launch before this one
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < HOL_ITER; ++it) {
    const int64_t gi = hol_voxel(it);
    const bool live = gi < V;
    const int li = live ? (int)gi : 0;
    const HoleVoxel x(li, o, jobs.H, jobs.W);
    const int cls = live && src[x.g] != o.value;
    if (__ballot(cls != 0) == 0ull) continue;               // wave-uniform
    unsigned long long heads;
    const int first = label_run_first(cls, x.xb, lane, &heads, [](int left) { return left == 0; });
    const bool walks = cls && first == lane;
    const int root = walks ? uf_find(parent, li) : -1;
    const bool hole = walks && ext[root] == 0;
    const int y = __shfl(hole ? root : -1, first);          // an organ voxel is its own run: -1
    const unsigned long long holes = __ballot(hole);
    if (holes == 0ull) continue;                            // wave-uniform
    const int lead = __ffsll((long long)holes) - 1;         // the first run of a hole in the wave
    const int y0 = __shfl(y, lead);
    const int count0 = (int)__popcll(__ballot(y == y0));
    if (lane == lead) atomicAdd(size + y0, count0);
    else if (hole && y != y0) atomicAdd(size + y, run_length(heads, lane));
  }
}

// One organ per launch, in the order of ids.  src is the input (labels, or its snapshot when out is labels), never out; voxel g of out
// is read and written by this thread alone.
__global__ __launch_bounds__(HOL_THREADS) void hol_apply_kernel(const uint8_t* __restrict__ src, HoleOrgan o, int H, int W,
                                                                const char* __restrict__ ws, const int* __restrict__ max_voxels, int claim_any,
                                                                uint8_t* __restrict__ out, int* __restrict__ info) {
  __shared__ int cnt[4];
  const int V = hol_voxels(o);
  if ((int64_t)blockIdx.x * HOL_ITER * HOL_THREADS >= V) return;
  const int* parent = (const int*)(ws + o.ws);
  const int* size = parent + V;                             // final: written by the launch before this one
  const uint8_t* ext = (const uint8_t*)(parent + 2 * (int64_t)V);
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();
  const int mv = max_voxels ? max_voxels[o.j] : 0;
#pragma unroll 1
  for (int it = 0; it < HOL_ITER; ++it) {
    const int64_t gi = hol_voxel(it);
    const bool live = gi < V;
    const int li = live ? (int)gi : 0;
    const HoleVoxel x(li, o, H, W);
    const int in = live ? src[x.g] : o.value;
    const int cls = in != o.value;
    if (__ballot(cls != 0) == 0ull) continue;               // wave-uniform
    unsigned long long heads;
    const int first = label_run_first(cls, x.xb, lane, &heads, [](int left) { return left == 0; });
    const bool walks = cls && first == lane;
    const int root = walks ? uf_find(parent, li) : -1;
    const bool hole = walks && ext[root] == 0;
    const int sz = hole ? size[root] : 0;
    const bool fits = hole && (mv == 0 || sz <= mv);
    if (hole && root == li) {                               // the hole's canonical voxel reports it
      atomicAdd(&cnt[0], 1);
      atomicAdd(&cnt[1], sz);
      if (fits) atomicAdd(&cnt[2], 1);
    }
    const int run_fits = __shfl((int)fits, first);          // an organ voxel is its own run: 0
    const bool fill = cls && run_fits && (claim_any || in == 0) && out[x.g] == in;
    if (fill) out[x.g] = (uint8_t)o.value;
    const unsigned long long filled = __ballot(fill);
    if (lane == 0 && filled) atomicAdd(&cnt[3], (int)__popcll(filled));
  }
  __syncthreads();
  if (tid < 4 && cnt[tid]) atomicAdd(info + o.j * 4 + tid, cnt[tid]);
}

}  // namespace

// boxes: HOST int32 [n, 6].  in_place: out will be labels (the snapshot of the input rides in the workspace).  all_at_once 0: the least
// the entry takes (its largest box alone); 1: what lets every organ go through one group.
extern "C" size_t msam2_label_fill_holes_workspace_bytes(int64_t D, int64_t H, int64_t W, const int32_t* boxes, int64_t n, int connectivity,
                                                         int in_place, int all_at_once) {
  if (!boxes || n < 1 || n > LABEL_MAX_OBJ || !label_sizes_ok(D, H, W, 1, LABEL_MAX_VOXELS) || !label_connectivity_ok(connectivity)) return 0;
  size_t bytes[LABEL_MAX_OBJ];
  for (int64_t j = 0; j < n; ++j) {
    if (!label_box_ok(boxes + 6 * j, D, H, W)) return 0;
    bytes[j] = hol_box_bytes(boxes + 6 * j, label_connectivity_in_plane(connectivity));
  }
  return label_input_bytes(D * H * W, in_place != 0) + label_tables_bytes(bytes, n, all_at_once != 0);
}

extern "C" int msam2_label_fill_holes(const uint8_t* labels, int64_t D, int64_t H, int64_t W, const uint8_t* ids, const int32_t* boxes, int64_t n,
                                      int connectivity, const int32_t* max_voxels, int claim, uint8_t* out, int32_t* info, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(labels && ids && boxes && out && info && workspace, "label_fill_holes: null labels / ids / boxes / out / info / workspace");
  LABEL_REQUIRE_OBJECTS("label_fill_holes", n);
  LABEL_REQUIRE_SIZES("label_fill_holes", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(label_connectivity_ok(connectivity),
                "label_fill_holes: connectivity %d of the background flood (6, 18 or 26 in 3-D; 4 or 8 slice by slice)", connectivity);
  MSAM2_REQUIRE(claim == 0 || claim == 1, "label_fill_holes: claim %d (0: background voxels only, 1: any voxel of a hole)", claim);
  const bool plane = label_connectivity_in_plane(connectivity);
  size_t bytes[LABEL_MAX_OBJ];                              // 0: a box that holds no hole
  for (int j = 0; j < (int)n; ++j) {                        // ids: HOST bytes, like the boxes
    LABEL_REQUIRE_DISTINCT_ID("label_fill_holes", "ids", ids, j);
    LABEL_REQUIRE_BOX("label_fill_holes", j, boxes + 6 * j, D, H, W);
    bytes[j] = hol_box_bytes(boxes + 6 * j, plane);
  }
  const int64_t N = D * H * W;
  LABEL_REQUIRE_OUT("label_fill_holes", labels, out, N);
  const size_t fixed = label_input_bytes(N, out == labels), need = fixed + label_tables_bytes(bytes, n, false);
  MSAM2_REQUIRE(workspace_bytes >= need, "label_fill_holes: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
  MSAM2_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)info & 3) == 0 && ((uintptr_t)max_voxels & 3) == 0,
                "label_fill_holes: the workspace must be 16-byte aligned, info and max_voxels 4-byte");
  const LabelRows rows = label_rows(connectivity);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const dim3 blk(HOL_THREADS);
  const uint8_t* src = label_begin_out(labels, out, N, ws, info, n, s);
  for (int j = 0; j < (int)n;) {
    HoleJobs jobs = {};
    jobs.H = (int)H, jobs.W = (int)W, jobs.plane = plane ? 1 : 0;
    int64_t vox = 0;
    j = label_next_group(bytes, (int)n, j, workspace_bytes - fixed, [&](int m, size_t at) {
      HoleOrgan& o = jobs.o[jobs.n++];
      static_cast<LabelBox&>(o) = label_box(boxes + 6 * m);
      o.value = ids[m], o.j = m;
      o.ws = (long long)(fixed + at);
      vox = std::max(vox, label_box_voxels(o));
    });
    if (jobs.n == 0) break;                                 // no box is left that can hold a hole
    const dim3 grid(cdiv(vox, HOL_THREADS * HOL_ITER), jobs.n);
    hipLaunchKernelGGL(hol_runs_kernel, grid, blk, 0, s, src, jobs, ws);
    hipLaunchKernelGGL(hol_merge_kernel, grid, blk, 0, s, src, jobs, ws, rows);
    hipLaunchKernelGGL(hol_mark_kernel, grid, blk, 0, s, src, jobs, ws);
    hipLaunchKernelGGL(hol_size_kernel, grid, blk, 0, s, src, jobs, ws);
    for (int k = 0; k < jobs.n; ++k) {
      const HoleOrgan& o = jobs.o[k];
      hipLaunchKernelGGL(hol_apply_kernel, dim3(cdiv(label_box_voxels(o), HOL_THREADS * HOL_ITER)), blk, 0, s, src, o, (int)H, (int)W,
                         (const char*)ws, max_voxels, claim, out, info);
    }
  }
  return msam2_check_launch("label_fill_holes");
}
