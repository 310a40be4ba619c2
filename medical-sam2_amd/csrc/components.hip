// Between the two ends of the 3-D path: connected components of a uint8 label volume [D, H, W], island removal and overlap counts, gfx950.
//
// A slice-propagating tracker leaves small blobs of an organ's label on far slices; the usual last step of an abdominal pipeline is "keep
// the largest 3-D component per organ, drop components below a voxel count".  This is the 3-D, multi-label generalisation of cc.hip (the
// reference's only native op: 8-connected, binary, one image): two voxels are adjacent iff they carry the same non-zero value and differ
// by one offset of the neighbourhood (6 / 18 / 26 in 3-D; 4 / 8 in plane, every slice on its own).  Everything is an integer with a
// canonical definition (a component's name is 1 + its smallest linear index), and partial results meet through integer add / min / max
// atomics only, so no output depends on scheduling.
//
// msam2_label_components, three launches over the voxels in raster order, one lane per voxel (the outputs are int32 per voxel, so a wave's
// 64 consecutive voxels are one 256-byte store; byte loads have no alignment to respect and nothing is read outside the volume):
//   * runs: label volumes are long runs of one value along a row.  A ballot over "this voxel starts a run" (value differs from the left
//     neighbour, column 0, or lane 0 of the wave) gives every lane its run's first voxel with one count-leading-zeros, no atomics: the
//     parent of every voxel starts at its run's first voxel.  `size` is zeroed in the same pass.
//   * merge: unions happen only between a run and the runs it touches in the BACKWARD neighbour rows -- for 26-connectivity (d, r-1),
//     (d-1, r-1), (d-1, r) and (d-1, r+1), the overlap widened by one column where the connectivity has the diagonal.  Per voxel the
//     neighbour row's bytes left / mid / right of it (two of them by shuffle from the neighbouring lanes) decide whether THIS voxel is the
//     leftmost witness of a (run, neighbour run) pair; only then it calls the lock-free union of cc.hip (atomicMin on a parent that only
//     ever points to a lower index).  The interior of an organ does no union at all; a wave of background leaves after one ballot.  Runs
//     cut at a wave's first lane are joined with their left part by one union.
//   * flatten: comp = 1 + root, read from the parents (scratch: nothing writes them in this launch, so path walking has no race) by the
//     first lane of every run and handed to the run by shuffle, and the component's voxel count into size[root]: wave-aggregated as
//     cc_count_kernel does, then gathered per workgroup in LDS, so an organ's interior costs one atomic add per 4096 voxels.
// Every loop of every thread ends whatever other threads do: a find follows strictly decreasing indices, a union retries only after
// another thread lowered the parent it wanted to lower; no thread waits for another, no grid barrier, no cooperative launch.
//
// msam2_label_clean: per listed value the number of components, their voxels and the largest one -- a 64-bit atomicMax on
// (size << 32 | 0x7fffffff - canonical index): the greatest size, ties to the smaller index -- gathered in LDS per workgroup and merged
// with one atomic per workgroup and counter; a second pass keeps or clears every voxel and counts what is kept, a last one writes info.
// msam2_label_overlap: (|P & G|, |P|, |G|) per slice and listed value from two label volumes, ballots and popcounts per wave.
#include "label_boxes.h"

namespace {

constexpr int CMP_THREADS = 256, CMP_ITER = 4;              // a workgroup owns CMP_ITER x 256 consecutive voxels, a wave 64 at a time

// voxel of this lane in round `it`: consecutive lanes hold consecutive voxels, a wave's 64 never straddle two rounds
__device__ __forceinline__ int64_t cmp_voxel(int it) { return ((int64_t)blockIdx.x * CMP_ITER + it) * CMP_THREADS + threadIdx.x; }

__global__ __launch_bounds__(CMP_THREADS) void cmp_runs_kernel(const uint8_t* __restrict__ labels, int* __restrict__ parent,
                                                               int* __restrict__ size, int W, int64_t N) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < CMP_ITER; ++it) {
    const int64_t gi = cmp_voxel(it);
    const bool live = gi < N;
    const int i = live ? (int)gi : 0;
    const int b = live ? labels[i] : 0;
    unsigned long long heads;
    const int first = label_run_first(b, i % W, lane, &heads, [&](int left) { return b != left; });
    if (live) {
      if (b != 0) parent[i] = i - lane + first;             // nothing ever reads the parent of a background voxel
      size[i] = 0;
    }
  }
}

// holes.hip's hol_merge_kernel is this text with the class "labels != v" in place of the label byte and a box in place of the volume,
// kept as a text of its own so that neither listing moves: a fix to either belongs in the other too.
__global__ __launch_bounds__(CMP_THREADS) void cmp_merge_kernel(const uint8_t* __restrict__ labels, int* __restrict__ parent, int H, int W,
                                                                int64_t N, LabelRows rows) {
  const int lane = threadIdx.x & 63;
  const int HW = H * W;
#pragma unroll 1
  for (int it = 0; it < CMP_ITER; ++it) {
    const int64_t gi = cmp_voxel(it);
    const bool live = gi < N;
    const int i = live ? (int)gi : 0;
    const int b = live ? labels[i] : 0;
    if (__ballot(b != 0) == 0ull) continue;                 // wave-uniform: the shuffles below see whole waves
    const int grow = i / W, col = i - grow * W;             // row counted through the volume
    const int d = grow / H, r = grow - d * H;
    int pb = __shfl_up(b, 1);
    if (lane == 0) pb = (live && col > 0) ? labels[i - 1] : 0;
    const bool left_same = col > 0 && b != 0 && pb == b;    // the voxel to the left belongs to the same run
    if (lane == 0 && left_same) uf_union(parent, i, i - 1);    // the run was cut at this wave's first lane
    // the neighbour rows' bytes first, by all lanes (wave-uniform control flow around the shuffles), the unions afterwards
    int ni[4], M[4], L[4], R[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = live && k < rows.count && d + rows.dd[k] >= 0 && r + rows.dr[k] >= 0 && r + rows.dr[k] < H;
      ni[k] = valid ? i + rows.dd[k] * HW + rows.dr[k] * W : -1;   // same column of the neighbour row
      M[k] = valid ? labels[ni[k]] : 0;
      // left and right of it in that row: the neighbouring lanes hold them unless this lane is the wave's first / last
      L[k] = __shfl_up(M[k], 1), R[k] = __shfl_down(M[k], 1);
      if (lane == 0) L[k] = (valid && col > 0) ? labels[ni[k] - 1] : 0;
      if (lane == 63) R[k] = (valid && col + 1 < W) ? labels[ni[k] + 1] : 0;
      if (col == 0) L[k] = 0;
      if (col + 1 >= W) R[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (b == 0 || ni[k] < 0) continue;
      if (rows.wide[k]) {
        // M is of the neighbour run that also holds L / R when they match; the leftmost voxel of this run that sees it joins them
        if (M[k] == b) {
          if (!left_same) uf_union(parent, i, ni[k]);
        } else {
          if (R[k] == b) uf_union(parent, i, ni[k] + 1);    // a neighbour run that starts at col + 1: nobody further left sees it
          if (L[k] == b && !left_same) uf_union(parent, i, ni[k] - 1);
        }
      } else if (M[k] == b && !(left_same && L[k] == b)) {
        uf_union(parent, i, ni[k]);
      }
    }
  }
}

// A voxel that does not start a run is never a root, so no union ever writes its parent: it still points to its run's first voxel, and the
// root of that voxel is the root of the whole run.  Only the run's first lane walks the parents; the others take its result by shuffle.
// Sizes: the voxels of the component of the wave's first foreground run are counted by one popcount and meet the workgroup's other waves
// and rounds in LDS (an organ's interior: one global add per workgroup -- adds to one address serialise in L2); a run of another
// component adds its length itself.
constexpr int FLAT_ITER = 16, FLAT_SLOTS = FLAT_ITER * (CMP_THREADS / 64);

__global__ __launch_bounds__(CMP_THREADS) void cmp_flatten_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ parent,
                                                                  int* __restrict__ comp, int* __restrict__ size, int W, int64_t N) {
  __shared__ int slot_name[FLAT_SLOTS], slot_count[FLAT_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < FLAT_SLOTS) slot_name[tid] = slot_count[tid] = 0;
  __syncthreads();
#pragma unroll 1
  for (int it = 0; it < FLAT_ITER; ++it) {
    const int64_t gi = ((int64_t)blockIdx.x * FLAT_ITER + it) * CMP_THREADS + tid;
    const bool live = gi < N;
    const int i = live ? (int)gi : 0;
    const int b = live ? labels[i] : 0;
    if (__ballot(b != 0) == 0ull) {                         // wave-uniform
      if (live) comp[i] = 0;
      continue;
    }
    unsigned long long heads;
    const int first = label_run_first(b, i % W, lane, &heads, [&](int left) { return b != left; });
    const bool walks = b != 0 && first == lane;
    const int root = walks ? uf_find(parent, i) + 1 : 0;
    const int y = __shfl(root, first);                      // a background voxel is its own run: 0
    if (live) comp[i] = y;
    const int lead = __ffsll((long long)__ballot(walks)) - 1;   // the first foreground run of the wave (there is one)
    const int y0 = __shfl(y, lead);
    const int count0 = (int)__popcll(__ballot(y == y0));
    if (lane == lead) {
      slot_name[it * (CMP_THREADS / 64) + wave] = y0;
      slot_count[it * (CMP_THREADS / 64) + wave] = count0;
    } else if (walks && y != y0) {
      atomicAdd(size + y - 1, run_length(heads, lane));
    }
  }
  __syncthreads();
  if (tid < FLAT_SLOTS) {
    const int name = slot_name[tid];
    int sum = 0;
    bool leader = name > 0;
    for (int s = 0; s < FLAT_SLOTS; ++s) {
      if (slot_name[s] != name) continue;
      if (s < tid) leader = false;                          // an earlier slot of the same component adds for all of them
      sum += slot_count[s];
    }
    if (leader) atomicAdd(size + name - 1, sum);
  }
}

// ---- island removal -------------------------------------------------------------------------------------------------------------------
struct CleanTables {                                        // the workspace of msam2_label_clean; LDS partials have the same form
  unsigned long long best[LABEL_MAX_OBJ];                   // size << 32 | 0x7fffffff - canonical index of the largest component
  int found[LABEL_MAX_OBJ], found_vox[LABEL_MAX_OBJ], kept[LABEL_MAX_OBJ], kept_vox[LABEL_MAX_OBJ];
};

__device__ __forceinline__ unsigned long long clean_key(int size, int index) {
  return ((unsigned long long)(unsigned)size << 32) | (unsigned)(0x7fffffff - index);
}

__global__ __launch_bounds__(CMP_THREADS) void clean_find_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ size,
                                                                 const uint8_t* __restrict__ ids, int n, CleanTables* __restrict__ t,
                                                                 int64_t N) {
  __shared__ CleanTables s;
  __shared__ signed char lut[256];
  const int tid = threadIdx.x;
  if (tid < LABEL_MAX_OBJ) {
    s.best[tid] = 0ull;
    s.found[tid] = s.found_vox[tid] = 0;
  }
  ids_to_object_table(lut, ids, n, tid);                     // CMP_THREADS == 256
#pragma unroll 1
  for (int it = 0; it < CMP_ITER; ++it) {
    const int64_t gi = cmp_voxel(it);
    if (gi >= N) break;
    const int i = (int)gi;
    const int sz = size[i];
    if (sz <= 0) continue;                                  // only a component's canonical voxel carries its size
    const int j = lut[labels[i]];
    if (j < 0) continue;
    atomicAdd(&s.found[j], 1);
    atomicAdd(&s.found_vox[j], sz);
    atomicMax(&s.best[j], clean_key(sz, i));
  }
  __syncthreads();
  if (tid < n && s.found[tid] > 0) {
    atomicAdd(&t->found[tid], s.found[tid]);
    atomicAdd(&t->found_vox[tid], s.found_vox[tid]);
    atomicMax(&t->best[tid], s.best[tid]);
  }
}

__global__ __launch_bounds__(CMP_THREADS) void clean_apply_kernel(const uint8_t* labels, const int* __restrict__ comp,
                                                                  const int* __restrict__ size, const uint8_t* __restrict__ ids, int n,
                                                                  const int* __restrict__ min_voxels, unsigned largest_mask, uint8_t* out,
                                                                  CleanTables* __restrict__ t, int64_t N) {
  __shared__ int kept[LABEL_MAX_OBJ], kept_vox[LABEL_MAX_OBJ], need[LABEL_MAX_OBJ];
  __shared__ unsigned long long best[LABEL_MAX_OBJ];
  __shared__ signed char lut[256];
  const int tid = threadIdx.x;
  if (tid < LABEL_MAX_OBJ) {
    kept[tid] = kept_vox[tid] = 0;
    need[tid] = tid < n ? max(1, min_voxels ? min_voxels[tid] : 0) : 1;
    best[tid] = tid < n ? t->best[tid] : 0ull;              // final: written by the launch before this one
  }
  ids_to_object_table(lut, ids, n, tid);                     // CMP_THREADS == 256
#pragma unroll 1
  for (int it = 0; it < CMP_ITER; ++it) {
    const int64_t gi = cmp_voxel(it);
    if (gi >= N) break;
    const int i = (int)gi;
    const uint8_t v = labels[i];                            // labels may be out: this thread alone reads and writes voxel i
    const int j = lut[v];
    uint8_t o = v;
    if (v != 0 && j >= 0) {
      const int c = comp[i] - 1;
      const int sz = c >= 0 && c < N ? size[c] : 0;         // (tables not made by msam2_label_components cannot lead outside the volume)
      const bool keep = sz >= need[j] && (!((largest_mask >> j) & 1u) || best[j] == clean_key(sz, c));
      if (!keep) o = 0;
      if (keep && c == i) {
        atomicAdd(&kept[j], 1);
        atomicAdd(&kept_vox[j], sz);
      }
    }
    out[i] = o;
  }
  __syncthreads();
  if (tid < n && kept[tid] > 0) {
    atomicAdd(&t->kept[tid], kept[tid]);
    atomicAdd(&t->kept_vox[tid], kept_vox[tid]);
  }
}

__global__ void clean_info_kernel(const CleanTables* __restrict__ t, int n, int* __restrict__ info) {
  const int j = threadIdx.x;
  if (j >= n) return;
  const unsigned long long b = t->best[j];
  int* o = info + j * 6;
  o[0] = t->found[j];
  o[1] = t->found_vox[j];
  o[2] = (int)(b >> 32);
  o[3] = b ? 0x7fffffff - (int)(unsigned)(b & 0xffffffffull) + 1 : 0;
  o[4] = t->kept[j];
  o[5] = t->kept_vox[j];
}

// ---- overlap counts -------------------------------------------------------------------------------------------------------------------
// blockIdx.y = slice; a workgroup owns CMP_ITER x 256 voxels of it
__global__ __launch_bounds__(CMP_THREADS) void overlap_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                              const uint8_t* __restrict__ ids, int n, int HW, int* __restrict__ counts) {
  __shared__ int cnt[LABEL_MAX_OBJ * 3];
  __shared__ int id[LABEL_MAX_OBJ];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < LABEL_MAX_OBJ * 3) cnt[tid] = 0;
  if (tid < n) id[tid] = ids[tid];
  __syncthreads();
  const int64_t slice = (int64_t)blockIdx.y * HW;
#pragma unroll 1
  for (int it = 0; it < CMP_ITER; ++it) {
    const int64_t gi = cmp_voxel(it);                       // within the slice
    const bool live = gi < HW;
    const int p = live ? pred[slice + gi] : 0, g = live ? gt[slice + gi] : 0;
    if (__ballot((p | g) != 0) == 0ull) continue;
    for (int j = 0; j < n; ++j) {
      const unsigned long long mp = __ballot(p == id[j]), mg = __ballot(g == id[j]);
      if (lane == 0 && (mp | mg)) LABEL_OVERLAP_ADD(cnt + j * 3, __popcll(mp & mg), __popcll(mp), __popcll(mg));
    }
  }
  __syncthreads();
  if (tid < n * 3 && cnt[tid]) atomicAdd(counts + (int64_t)blockIdx.y * n * 3 + tid, cnt[tid]);
}

}  // namespace

extern "C" size_t msam2_label_components_workspace_bytes(int64_t D, int64_t H, int64_t W) {
  if (!label_sizes_ok(D, H, W, 1, LABEL_MAX_VOXELS)) return 0;
  return (size_t)(D * H * W) * sizeof(int);
}

extern "C" int msam2_label_components(const uint8_t* labels, int64_t D, int64_t H, int64_t W, int connectivity, int32_t* comp, int32_t* size,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(labels && comp && size && workspace, "label_components: null labels / comp / size / workspace");
  MSAM2_REQUIRE(label_connectivity_ok(connectivity), "label_components: connectivity %d (6, 18 or 26 in 3-D; 4 or 8 slice by slice)", connectivity);
  LABEL_REQUIRE_SIZES("label_components", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(workspace_bytes >= msam2_label_components_workspace_bytes(D, H, W), "label_components: workspace too small (%zu of %zu bytes)",
                workspace_bytes, msam2_label_components_workspace_bytes(D, H, W));
  MSAM2_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)comp & 3) == 0 && ((uintptr_t)size & 3) == 0,
                "label_components: comp / size / workspace must be 4-byte aligned");
  const LabelRows rows = label_rows(connectivity);
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = D * H * W;
  int* parent = (int*)workspace;
  const dim3 grid(cdiv(N, CMP_THREADS * CMP_ITER)), blk(CMP_THREADS);
  hipLaunchKernelGGL(cmp_runs_kernel, grid, blk, 0, s, labels, parent, size, (int)W, N);
  hipLaunchKernelGGL(cmp_merge_kernel, grid, blk, 0, s, labels, parent, (int)H, (int)W, N, rows);
  hipLaunchKernelGGL(cmp_flatten_kernel, dim3(cdiv(N, CMP_THREADS * FLAT_ITER)), blk, 0, s, labels, parent, comp, size, (int)W, N);
  return msam2_check_launch("label_components");
}

extern "C" size_t msam2_label_clean_workspace_bytes(int64_t n) { return n >= 1 && n <= LABEL_MAX_OBJ ? sizeof(CleanTables) : 0; }

extern "C" int msam2_label_clean(const uint8_t* labels, const int32_t* comp, const int32_t* size, const uint8_t* ids, int64_t n,
                                 const int32_t* min_voxels, uint32_t largest_mask, uint8_t* out, int32_t* info, void* workspace,
                                 size_t workspace_bytes, int64_t D, int64_t H, int64_t W, void* stream) {
  MSAM2_REQUIRE(labels && comp && size && ids && out && info && workspace, "label_clean: null labels / comp / size / ids / out / info / workspace");
  LABEL_REQUIRE_OBJECTS("label_clean", n);
  LABEL_REQUIRE_SIZES("label_clean", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(workspace_bytes >= msam2_label_clean_workspace_bytes(n), "label_clean: workspace too small (%zu of %zu bytes)", workspace_bytes,
                msam2_label_clean_workspace_bytes(n));
  MSAM2_REQUIRE(((uintptr_t)workspace & 7) == 0, "label_clean: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = D * H * W;
  CleanTables* t = (CleanTables*)workspace;
  fill_on(s, (int*)workspace, (int64_t)(sizeof(CleanTables) / sizeof(int)), 0);   // (common.h: why a kernel)
  const dim3 grid(cdiv(N, CMP_THREADS * CMP_ITER)), blk(CMP_THREADS);
  hipLaunchKernelGGL(clean_find_kernel, grid, blk, 0, s, labels, size, ids, (int)n, t, N);
  hipLaunchKernelGGL(clean_apply_kernel, grid, blk, 0, s, labels, comp, size, ids, (int)n, min_voxels, (unsigned)largest_mask, out, t, N);
  hipLaunchKernelGGL(clean_info_kernel, dim3(1), dim3(LABEL_MAX_OBJ), 0, s, t, (int)n, info);
  return msam2_check_launch("label_clean");
}

extern "C" int msam2_label_overlap(const uint8_t* pred, const uint8_t* gt, const uint8_t* ids, int64_t D, int64_t H, int64_t W, int64_t n,
                                   int32_t* counts, void* stream) {
  MSAM2_REQUIRE(pred && gt && ids && counts, "label_overlap: null pred / gt / ids / counts");
  LABEL_REQUIRE_OBJECTS("label_overlap", n);
  LABEL_REQUIRE_SIZES("label_overlap", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  hipStream_t s = (hipStream_t)stream;
  fill_on(s, counts, D * n * 3, 0);
  hipLaunchKernelGGL(overlap_kernel, dim3(cdiv(H * W, CMP_THREADS * CMP_ITER), (unsigned)D), dim3(CMP_THREADS), 0, s, pred, gt, ids, (int)n, (int)(H * W), counts);
  return msam2_check_launch("label_overlap");
}
