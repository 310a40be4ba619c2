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
#include "common.h"

namespace {

constexpr int HOL_THREADS = 256, HOL_ITER = 4;              // a workgroup owns HOL_ITER x 256 consecutive box voxels, a wave 64 at a time
constexpr int HOL_FIXED_BYTES = 16;                         // the workspace is never empty

struct HoleOrgan {
  int z0, y0, x0, bd, bh, bw;                               // the box: first voxel and extent
  int value, j;                                             // label value and index in ids / max_voxels / info
  long long ws;                                             // byte offset of the organ's tables in the workspace
};
struct HoleJobs {
  int n, H, W, plane;                                       // plane: connectivity 4 / 8
  HoleOrgan o[LABEL_MAX_OBJ];
};

static inline int64_t hol_vox(const int32_t* b) { return (int64_t)(b[1] - b[0] + 1) * (b[3] - b[2] + 1) * (b[5] - b[4] + 1); }
static inline bool hol_box_ok(const int32_t* b, int64_t D, int64_t H, int64_t W) {
  return b[0] >= 0 && b[0] <= b[1] && b[1] < D && b[2] >= 0 && b[2] <= b[3] && b[3] < H && b[4] >= 0 && b[4] <= b[5] && b[5] < W;
}
// a box that can hold a hole: the hole and the organ around it need 3 voxels along every axis the flood moves along
static inline bool hol_box_live(const int32_t* b, bool plane) {
  return b[3] - b[2] >= 2 && b[5] - b[4] >= 2 && (plane || b[1] - b[0] >= 2);
}
static inline size_t hol_box_bytes(int64_t vox) { return ((size_t)vox * 9 + 15) & ~(size_t)15; }
static inline size_t hol_snapshot_bytes(int64_t N) { return ((size_t)N + 15) & ~(size_t)15; }

struct HoleVoxel {                                          // box voxel `li` of an organ: position in the box, index in the volume
  int dz, dr, dc, g;
  __device__ __forceinline__ HoleVoxel(const HoleOrgan& o, int li, int H, int W) {
    const int row = li / o.bw;
    dc = li - row * o.bw;
    dz = row / o.bh;
    dr = row - dz * o.bh;
    g = ((o.z0 + dz) * H + o.y0 + dr) * W + o.x0 + dc;      // a voxel of the volume: below 2^31 - 2
  }
};
__device__ __forceinline__ int hol_voxels(const HoleOrgan& o) { return o.bd * o.bh * o.bw; }
__device__ __forceinline__ int* hol_parent(char* ws, const HoleOrgan& o) { return (int*)(ws + o.ws); }
__device__ __forceinline__ int* hol_size(char* ws, const HoleOrgan& o) { return (int*)(ws + o.ws) + hol_voxels(o); }
__device__ __forceinline__ uint8_t* hol_ext(char* ws, const HoleOrgan& o) { return (uint8_t*)((int*)(ws + o.ws) + 2 * (int64_t)hol_voxels(o)); }

// box voxel of this lane in round `it`: consecutive lanes hold consecutive box voxels, a wave's 64 never straddle two rounds
__device__ __forceinline__ int64_t hol_voxel(int it) { return ((int64_t)blockIdx.x * HOL_ITER + it) * HOL_THREADS + threadIdx.x; }

// Lane of the first voxel of this lane's run among the wave's 64 box voxels: a run of complement voxels starts where the left lane is
// of the organ, at column 0 of the box and at lane 0 (organ voxels are runs of their own).  All 64 lanes call it.
__device__ __forceinline__ int hol_run_first(int cls, int col, int lane, unsigned long long* heads) {
  const int pc = __shfl_up(cls, 1);
  const bool head = lane == 0 || cls == 0 || col == 0 || pc == 0;
  *heads = __ballot(head);                                  // bit 0 is always set
  return 63 - __clzll((long long)(*heads & (~0ull >> (63 - lane))));
}

// (kernels, not hipMemcpyAsync / hipMemsetAsync: cc.hip found memset nodes of a captured graph unreliable against neighbouring kernel nodes)
__global__ void hol_copy_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t n, int vec) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {                                                // both 16-byte aligned: the tail by bytes
    const int64_t n16 = n / 16;
    for (int64_t i = t; i < n16; i += step) ((int4*)dst)[i] = ((const int4*)src)[i];
    for (int64_t i = n16 * 16 + t; i < n; i += step) dst[i] = src[i];
  } else {
    for (int64_t i = t; i < n; i += step) dst[i] = src[i];
  }
}
__global__ void hol_zero_kernel(int* __restrict__ x, int n) {
  if ((int)threadIdx.x < n) x[threadIdx.x] = 0;
}

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
    const HoleVoxel x(o, li, jobs.H, jobs.W);
    const int cls = live && src[x.g] != o.value;
    unsigned long long heads;
    const int first = hol_run_first(cls, x.dc, lane, &heads);
    if (live) {
      if (cls) parent[li] = li - lane + first;              // nothing ever reads the parent of an organ voxel
      size[li] = 0;
      ext[li] = 0;
    }
  }
}

struct HoleRows {                                           // the backward neighbour rows of a connectivity
  int count;
  int dd[4], dr[4], wide[4];                                // slice and row offset; wide: the overlap reaches one column further
};

__global__ __launch_bounds__(HOL_THREADS) void hol_merge_kernel(const uint8_t* __restrict__ src, HoleJobs jobs, char* __restrict__ ws,
                                                                HoleRows rows) {
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
    const HoleVoxel x(o, li, jobs.H, W);
    const int b = live && src[x.g] != v;
    if (__ballot(b != 0) == 0ull) continue;                 // wave-uniform: the shuffles below see whole waves
    const int col = x.dc;
    int pb = __shfl_up(b, 1);
    if (lane == 0) pb = (live && col > 0) ? src[x.g - 1] != v : 0;
    const bool left_same = col > 0 && b != 0 && pb != 0;    // the voxel to the left belongs to the same run
    if (lane == 0 && left_same) uf_union(parent, li, li - 1);    // the run was cut at this wave's first lane
    // the neighbour rows' classes first, by all lanes (wave-uniform control flow around the shuffles), the unions afterwards
    int ni[4], M[4], L[4], R[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = live && k < rows.count && x.dz + rows.dd[k] >= 0 && x.dr + rows.dr[k] >= 0 && x.dr + rows.dr[k] < bh;
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
    const HoleVoxel x(o, li, jobs.H, jobs.W);
    const bool edge = x.dr == 0 || x.dr == o.bh - 1 || x.dc == 0 || x.dc == o.bw - 1 || (!jobs.plane && (x.dz == 0 || x.dz == o.bd - 1));
    const int cls = live && src[x.g] != o.value;
    const int pc = __shfl_up(cls, 1);
    const bool head = lane == 0 || x.dc == 0 || pc == 0;    // a row of the boundary marks once per run, not once per voxel
    if (cls && edge && (head || x.dc == o.bw - 1)) ext[uf_find(parent, li)] = 1;
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
    const HoleVoxel x(o, li, jobs.H, jobs.W);
    const int cls = live && src[x.g] != o.value;
    if (__ballot(cls != 0) == 0ull) continue;               // wave-uniform
    unsigned long long heads;
    const int first = hol_run_first(cls, x.dc, lane, &heads);
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
    const HoleVoxel x(o, li, H, W);
    const int in = live ? src[x.g] : o.value;
    const int cls = in != o.value;
    if (__ballot(cls != 0) == 0ull) continue;               // wave-uniform
    unsigned long long heads;
    const int first = hol_run_first(cls, x.dc, lane, &heads);
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
  if (!boxes || n < 1 || n > LABEL_MAX_OBJ || !label_sizes_ok(D, H, W, 1, LABEL_MAX_VOXELS)) return 0;
  if (connectivity != 4 && connectivity != 8 && connectivity != 6 && connectivity != 18 && connectivity != 26) return 0;
  const bool plane = connectivity == 4 || connectivity == 8;
  size_t sum = 0, largest = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int32_t* bx = boxes + 6 * j;
    if (!hol_box_ok(bx, D, H, W)) return 0;
    if (!hol_box_live(bx, plane)) continue;
    const size_t one = hol_box_bytes(hol_vox(bx));
    sum += one;
    if (one > largest) largest = one;
  }
  return HOL_FIXED_BYTES + (in_place ? hol_snapshot_bytes(D * H * W) : 0) + (all_at_once ? sum : largest);
}

extern "C" int msam2_label_fill_holes(const uint8_t* labels, int64_t D, int64_t H, int64_t W, const uint8_t* ids, const int32_t* boxes, int64_t n,
                                      int connectivity, const int32_t* max_voxels, int claim, uint8_t* out, int32_t* info, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(labels && ids && boxes && out && info && workspace, "label_fill_holes: null labels / ids / boxes / out / info / workspace");
  LABEL_REQUIRE_OBJECTS("label_fill_holes", n);
  LABEL_REQUIRE_SIZES("label_fill_holes", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(connectivity == 4 || connectivity == 8 || connectivity == 6 || connectivity == 18 || connectivity == 26,
                "label_fill_holes: connectivity %d of the background flood (6, 18 or 26 in 3-D; 4 or 8 slice by slice)", connectivity);
  MSAM2_REQUIRE(claim == 0 || claim == 1, "label_fill_holes: claim %d (0: background voxels only, 1: any voxel of a hole)", claim);
  for (int j = 0; j < (int)n; ++j) {                        // ids: HOST bytes, like the boxes
    MSAM2_REQUIRE(ids[j] != 0, "label_fill_holes: ids[%d] is 0, the background", j);
    for (int k = 0; k < j; ++k) MSAM2_REQUIRE(ids[k] != ids[j], "label_fill_holes: ids[%d] and ids[%d] are both %d", k, j, (int)ids[j]);
    const int32_t* bx = boxes + 6 * j;
    MSAM2_REQUIRE(hol_box_ok(bx, D, H, W), "label_fill_holes: box %d (%d..%d, %d..%d, %d..%d) is inverted or outside the %lld x %lld x %lld volume", j,
                  bx[0], bx[1], bx[2], bx[3], bx[4], bx[5], (long long)D, (long long)H, (long long)W);
  }
  const int64_t N = D * H * W;
  const bool in_place = out == labels;
  MSAM2_REQUIRE(in_place || out + N <= labels || labels + N <= out, "label_fill_holes: out overlaps labels without being labels");
  const size_t need = msam2_label_fill_holes_workspace_bytes(D, H, W, boxes, n, connectivity, in_place, 0);
  MSAM2_REQUIRE(workspace_bytes >= need, "label_fill_holes: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
  MSAM2_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)info & 3) == 0 && ((uintptr_t)max_voxels & 3) == 0,
                "label_fill_holes: the workspace must be 16-byte aligned, info and max_voxels 4-byte");
  // backward neighbour rows (slice offset, row offset, widened by a column): in plane first
  HoleRows rows = {};
  const bool diag2 = connectivity == 8 || connectivity == 18 || connectivity == 26;     // offsets that differ in two coordinates
  const bool plane = connectivity == 4 || connectivity == 8;
  auto add = [&](int dd, int dr, bool wide) {
    rows.dd[rows.count] = dd, rows.dr[rows.count] = dr, rows.wide[rows.count] = wide ? 1 : 0;
    ++rows.count;
  };
  add(0, -1, diag2);
  if (!plane) {
    add(-1, 0, diag2);
    if (diag2) {
      add(-1, -1, connectivity == 26);
      add(-1, 1, connectivity == 26);
    }
  }
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const dim3 blk(HOL_THREADS);
  // the input every launch reads: labels, or its snapshot when the call is in place
  const uint8_t* src = labels;
  size_t fixed = HOL_FIXED_BYTES;
  uint8_t* copy_to = out;
  if (in_place) {
    copy_to = (uint8_t*)(ws + fixed);
    src = copy_to;
    fixed += hol_snapshot_bytes(N);
  }
  hipLaunchKernelGGL(hol_copy_kernel, dim3(grid1d(N, 4096, HOL_THREADS * 16)), blk, 0, s, labels, copy_to, N,
                     (int)((((uintptr_t)labels | (uintptr_t)copy_to) & 15) == 0));
  hipLaunchKernelGGL(hol_zero_kernel, dim3(1), dim3(LABEL_MAX_OBJ * 4), 0, s, info, (int)n * 4);
  const size_t room = workspace_bytes - fixed;
  int j = 0;
  while (j < (int)n) {
    HoleJobs jobs = {};
    jobs.H = (int)H, jobs.W = (int)W, jobs.plane = plane ? 1 : 0;
    size_t used = 0;
    int64_t vox = 0;
    for (; j < (int)n; ++j) {                               // the organs that follow, as long as their boxes fit
      const int32_t* bx = boxes + 6 * j;
      if (!hol_box_live(bx, plane)) continue;
      const size_t one = hol_box_bytes(hol_vox(bx));
      if (jobs.n > 0 && used + one > room) break;           // (one alone fits: `need` covers the largest box)
      HoleOrgan& o = jobs.o[jobs.n++];
      o.z0 = bx[0], o.y0 = bx[2], o.x0 = bx[4];
      o.bd = bx[1] - bx[0] + 1, o.bh = bx[3] - bx[2] + 1, o.bw = bx[5] - bx[4] + 1;
      o.value = ids[j], o.j = j;
      o.ws = (long long)(fixed + used);
      used += one;
      if (hol_vox(bx) > vox) vox = hol_vox(bx);
    }
    if (jobs.n == 0) break;
    const dim3 grid(cdiv(vox, HOL_THREADS * HOL_ITER), jobs.n);
    hipLaunchKernelGGL(hol_runs_kernel, grid, blk, 0, s, src, jobs, ws);
    hipLaunchKernelGGL(hol_merge_kernel, grid, blk, 0, s, src, jobs, ws, rows);
    hipLaunchKernelGGL(hol_mark_kernel, grid, blk, 0, s, src, jobs, ws);
    hipLaunchKernelGGL(hol_size_kernel, grid, blk, 0, s, src, jobs, ws);
    for (int k = 0; k < jobs.n; ++k) {
      const HoleOrgan& o = jobs.o[k];
      hipLaunchKernelGGL(hol_apply_kernel, dim3(cdiv((int64_t)o.bd * o.bh * o.bw, HOL_THREADS * HOL_ITER)), blk, 0, s, src, o, (int)H, (int)W,
                         (const char*)ws, max_voxels, claim, out, info);
    }
  }
  return msam2_check_launch("label_fill_holes");
}
