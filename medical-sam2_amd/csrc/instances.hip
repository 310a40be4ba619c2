// Beside the per-organ scores: instance maps and the three integer tables every instance score needs, gfx950.
//
// The reference scores instances on the host (sam2_train/modeling/stats_utils.py: remap_label, get_fast_pq, get_fast_aji, get_fast_aji_plus,
// get_fast_dice_2, as called at func_2d/function.py:620-651): one boolean mask per instance and one masked np.unique per ground-truth
// instance, three times over.  All of them are functions of the non-empty entries of the pairwise-intersection matrix and the two area
// vectors; these come from ONE pass over the two maps.  Maps are contiguous int32 [D, H, W] (a 2-D map has D = 1), 0 = background.
//
//   msam2_instance_remap   arbitrary ids in 0 .. id_bound - 1 -> contiguous ids 1 .. n in ascending order of the original id (np.unique's order,
//                          remap_label(by_size=False)), with the tables original id / voxel count / largest label value per instance
//   msam2_instance_apply   out[i] = table[map[i]]: the gather behind by_size=True and the size / class filters
//   msam2_instance_pairs   rows (i, j, |a == i and b == j|) of every non-empty pair, sorted by (i, j), and the areas of both maps
//   msam2_instance_paint   N masks into one instance map in a given order, by the reference's rule (function.py:621-624)
//
// A wave owns 64 consecutive voxels in raster order through the whole volume (rows do not matter here: a run may continue across a row
// end).  A lane is a run head where its key differs from the left lane's (lane 0 always is); the ballot of heads gives every head its run
// length, and only heads touch the tables: one atomic per run, not per voxel.  Every table value is an integer sum, maximum or a store of
// a value that is the same whoever stores it, and the order of the pair rows is canonical, so no byte of any output depends on scheduling.
//
// No workgroup ever waits for another: the two scans (bitmap popcounts, pair rows per i) are split over launches (tiles of 1024, then the
// tile sums by one workgroup), the paint decision of mask k is final before the launch that uses it starts, and hash probing ends after
// `slots` steps whatever other threads do.
#include "common.h"

namespace {

constexpr int INS_THREADS = 256, INS_ITER = 4;              // a workgroup owns INS_ITER x 256 consecutive voxels, a wave 64 at a time
constexpr int INS_TILE = INS_THREADS * 4;                   // items of a scan tile: four per thread
constexpr int64_t INS_MAX_CAP = 1ll << 26;                  // pair rows (the hash table has up to 2^27 slots)
constexpr int64_t INS_MAX_MASKS = 65535;

// voxel of this lane in round `round` of the grid: consecutive lanes hold consecutive voxels, a wave's 64 never straddle two rounds
__device__ __forceinline__ int64_t ins_voxel_of(int64_t round) { return round * INS_THREADS + threadIdx.x; }
__device__ __forceinline__ int64_t ins_voxel(int it) { return ins_voxel_of((int64_t)blockIdx.x * INS_ITER + it); }
// this thread's voxel of every round, 0 beyond the volume: all loads are issued before the first is used (one load in flight per wave and
// round leaves the pass bound by latency, not by bandwidth)
__device__ __forceinline__ void ins_load(int (&v)[INS_ITER], const int* map, int64_t N, int64_t first_round) {
#pragma unroll
  for (int it = 0; it < INS_ITER; ++it) {
    const int64_t gi = ins_voxel_of(first_round + it);
    v[it] = gi < N ? map[gi] : 0;
  }
}
// lane of the head of this lane's run
__device__ __forceinline__ int ins_run_first(unsigned long long heads, int lane) { return 63 - __clzll((long long)(heads & (~0ull >> (63 - lane)))); }

// exclusive scan of one value per thread over the workgroup's 256 threads; *total: the sum of all.  All threads call it.
__device__ __forceinline__ int ins_block_scan(int v, int* total) {
  __shared__ int wave_sum[INS_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < INS_THREADS / 64; ++w) {
    if (w < wave) base += wave_sum[w];
    all += wave_sum[w];
  }
  *total = all;
  __syncthreads();                                          // wave_sum may be written again by the next call
  return base + inc - v;
}

// First level of an exclusive scan over n items: local[i] = sum of the items before i within i's tile, tile_sum[tile] = the tile's sum.
// POP: an item is the popcount of a bitmap word, else the int itself.
template <bool POP>
__global__ __launch_bounds__(INS_THREADS) void ins_scan_tiles_kernel(const unsigned* __restrict__ in, int* __restrict__ local,
                                                                     int* __restrict__ tile_sum, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * INS_TILE + threadIdx.x * 4;
  int v[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = base + k < n ? (POP ? __popc(in[base + k]) : (int)in[base + k]) : 0;
    sum += v[k];
  }
  int total;
  int run = ins_block_scan(sum, &total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (base + k < n) local[base + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// Second level, ONE workgroup: tile_sum -> the exclusive scan of the tile sums, in place, 256 tiles per trip with a carry; *total: the sum.
__device__ __forceinline__ int ins_scan_sums(int* __restrict__ tile_sum, int tiles) {
  int carry = 0;
  for (int base = 0; base < tiles; base += INS_THREADS) {
    const int t = base + threadIdx.x;
    const int v = t < tiles ? tile_sum[t] : 0;
    int total;
    const int ex = ins_block_scan(v, &total);
    if (t < tiles) tile_sum[t] = carry + ex;
    carry += total;
  }
  return carry;
}

// ---- remap ------------------------------------------------------------------------------------------------------------------------------
enum { RM_OUTSIDE = 1, RM_CTL = 4 };                        // the counters behind the bitmap

// presence bitmap of the ids 1 .. id_bound - 1, voxels with an id outside [0, id_bound) counted
__global__ __launch_bounds__(INS_THREADS) void remap_presence_kernel(const int* __restrict__ map, unsigned* __restrict__ bitmap,
                                                                     int* __restrict__ ctl, int64_t id_bound, int64_t N) {
  const int lane = threadIdx.x & 63;
  int loaded[INS_ITER];
  ins_load(loaded, map, N, (int64_t)blockIdx.x * INS_ITER);
#pragma unroll
  for (int it = 0; it < INS_ITER; ++it) {
    int v = loaded[it];
    const bool outside = v < 0 || (int64_t)v >= id_bound;
    const unsigned long long out_mask = __ballot(outside);
    if (out_mask && lane == 0) atomicAdd(ctl + RM_OUTSIDE, (int)__popcll(out_mask));
    if (outside) v = 0;
    if (__ballot(v != 0) == 0ull) continue;                 // wave-uniform
    const int left = __shfl_up(v, 1);
    if (v != 0 && (lane == 0 || v != left)) {
      const unsigned bit = 1u << (v & 31);
      unsigned* word = bitmap + (v >> 5);
      if (!(*word & bit)) atomicOr(word, bit);              // a stale read only costs the atomic
    }
  }
}

__global__ __launch_bounds__(INS_THREADS) void remap_sums_kernel(int* __restrict__ tile_sum, int tiles, const int* __restrict__ ctl, int cap,
                                                                 int* __restrict__ info) {
  const int found = ins_scan_sums(tile_sum, tiles);
  if (threadIdx.x == 0) {
    info[0] = found;
    info[1] = ctl[RM_OUTSIDE];
    info[2] = found > cap ? 1 : 0;
    info[3] = 0;
  }
}

// A workgroup of the gather owns GA_ROUNDS x 256 consecutive voxels and gathers the sizes and classes of its runs in a direct-mapped LDS
// table first, as pairs_insert_kernel does (there: why); a run whose entry is taken by another instance adds to the global tables directly.
constexpr int GA_ROUNDS = 16, GA_CACHE = 512;

__device__ __forceinline__ void remap_add(int rank, int v, int len, int lb, bool with_cls, int* __restrict__ orig, int* __restrict__ size,
                                          int* __restrict__ cls) {
  atomicAdd(size + rank - 1, len);
  if (with_cls) atomicMax(cls + rank - 1, lb);
  orig[rank - 1] = v;                                       // the same value whoever stores it
}

// rank = ids present below this one + 1: the scanned popcounts of the words before, the lower bits of its own word
__global__ __launch_bounds__(INS_THREADS) void remap_gather_kernel(const int* map, const uint8_t* __restrict__ labels,
                                                                   const unsigned* __restrict__ bitmap, const int* __restrict__ local,
                                                                   const int* __restrict__ tile_off, int* out, int* __restrict__ orig,
                                                                   int* __restrict__ size, int* __restrict__ cls, int cap, int64_t id_bound,
                                                                   int64_t N) {
  __shared__ int cache_rank[GA_CACHE], cache_orig[GA_CACHE], cache_size[GA_CACHE], cache_cls[GA_CACHE];
  const int lane = threadIdx.x & 63;
  for (int t = threadIdx.x; t < GA_CACHE; t += INS_THREADS) cache_rank[t] = cache_size[t] = cache_cls[t] = 0;
  __syncthreads();
#pragma unroll 1
  for (int part = 0; part < GA_ROUNDS / INS_ITER; ++part) {
    const int64_t first = (int64_t)blockIdx.x * GA_ROUNDS + part * INS_ITER;
    if (first * INS_THREADS >= N) break;                    // workgroup-uniform
    int loaded[INS_ITER];
    ins_load(loaded, map, N, first);                        // map may be out: this thread alone reads and writes its voxels
#pragma unroll
    for (int it = 0; it < INS_ITER; ++it) {
      const int64_t gi = ins_voxel_of(first + it);
      const bool live = gi < N;
      int v = loaded[it];
      if (v < 0 || (int64_t)v >= id_bound) v = 0;
      if (__ballot(v != 0) == 0ull) {                       // wave-uniform
        if (live) out[gi] = 0;
        continue;
      }
      const int lb = (labels && live) ? labels[gi] : 0;
      const int left_v = __shfl_up(v, 1), left_lb = __shfl_up(lb, 1);
      const bool head = lane == 0 || !live || v != left_v || lb != left_lb;
      const unsigned long long heads = __ballot(head);
      int rank = 0;
      if (head && v != 0) {
        const int w = v >> 5;
        rank = tile_off[w / INS_TILE] + local[w] + __popc(bitmap[w] & ((1u << (v & 31)) - 1u)) + 1;
        if (rank <= cap) {
          const int len = run_length(heads, lane), c = rank & (GA_CACHE - 1);
          const int prev = atomicCAS(cache_rank + c, 0, rank);
          if (prev == 0 || prev == rank) {
            atomicAdd(cache_size + c, len);
            atomicMax(cache_cls + c, lb);
            cache_orig[c] = v;                              // the same value from every run of the instance
          } else {
            remap_add(rank, v, len, lb, labels != nullptr, orig, size, cls);
          }
        }
      }
      const int r = __shfl(rank, ins_run_first(heads, lane));
      if (live) out[gi] = r;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < GA_CACHE; t += INS_THREADS)
    if (cache_rank[t]) remap_add(cache_rank[t], cache_orig[t], cache_size[t], cache_cls[t], labels != nullptr, orig, size, cls);
}

__global__ __launch_bounds__(INS_THREADS) void apply_kernel(const int* map, const int* __restrict__ table, int n, int* out, int64_t N) {
#pragma unroll
  for (int it = 0; it < INS_ITER; ++it) {
    const int64_t gi = ins_voxel(it);
    if (gi >= N) break;
    const int v = map[gi];                                  // map may be out
    out[gi] = (v >= 0 && v <= n) ? table[v] : 0;
  }
}

// ---- pairs ------------------------------------------------------------------------------------------------------------------------------
enum { PR_DISTINCT = 0, PR_OUTSIDE_A = 1, PR_OUTSIDE_B = 2, PR_CTL = 8 };

struct PairTables {                                         // the workspace of msam2_instance_pairs, cut by pair_tables()
  unsigned long long* keys;                                 // [slots] (i << 32 | j), 0 = empty
  int *counts, *rows, *cursor, *ctl;                        // [slots], [na] pairs per i, [na], [PR_CTL]: all zeroed by one fill
  int *offs, *tile, *tmp;                                   // [na] scan of rows within its tile, [tiles], [cap, 3] rows in bucket order
  int64_t slots, zeroed;                                    // zeroed: ints from keys on that the call pre-sets
  size_t bytes;
};
static inline int64_t pair_slots(int64_t cap) {
  int64_t s = 64;
  while (s < 2 * cap) s <<= 1;
  return s;
}
static inline PairTables pair_tables(void* ws, int64_t na, int64_t cap) {
  PairTables t;
  t.slots = pair_slots(cap);
  const int64_t na2 = (na + 1) & ~1ll, tiles = (na + INS_TILE - 1) / INS_TILE;
  t.keys = (unsigned long long*)ws;
  t.counts = (int*)(t.keys + t.slots);
  t.rows = t.counts + t.slots;
  t.cursor = t.rows + na2;
  t.ctl = t.cursor + na2;
  t.offs = t.ctl + PR_CTL;
  t.zeroed = t.offs - (int*)ws;
  t.tile = t.offs + na2;
  t.tmp = t.tile + ((tiles + 1) & ~1ll);
  t.bytes = (size_t)((char*)(t.tmp + cap * 3) - (char*)ws);
  t.bytes = (t.bytes + 7) & ~(size_t)7;
  return t;
}

__device__ __forceinline__ unsigned long long pair_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return k;
}

// count[key] += len in the open-addressing table: linear probing, at most `slots` steps
__device__ __forceinline__ void pair_insert(unsigned long long key, int len, unsigned long long* __restrict__ keys, int* __restrict__ counts,
                                            int64_t slots, int cap, int* __restrict__ ctl) {
  // more distinct pairs than rows already: the rows will not be written, spare the probing (a stale read only costs the probing)
  if (__hip_atomic_load(ctl + PR_DISTINCT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap) return;
  int64_t slot = (int64_t)(pair_hash(key) & (unsigned long long)(slots - 1));
  for (int64_t probe = 0; probe < slots; ++probe) {
    unsigned long long cur = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) {
      cur = atomicCAS(keys + slot, 0ull, key);
      if (cur == 0ull) {
        atomicAdd(ctl + PR_DISTINCT, 1);
        cur = key;
      }
    }
    if (cur == key) {
      atomicAdd(counts + slot, len);
      return;
    }
    slot = (slot + 1) & (slots - 1);
  }
  atomicAdd(ctl + PR_DISTINCT, 1);                          // the table is full (slots >= 2 cap distinct pairs): one more than it holds
}

// one run's (or one workgroup's) count of a key (a << 32 | b, not both 0) into the global tables
__device__ __forceinline__ void pair_add(unsigned long long key, int len, unsigned long long* __restrict__ keys, int* __restrict__ counts,
                                         int64_t slots, int cap, int* __restrict__ area_a, int* __restrict__ area_b, int* __restrict__ ctl) {
  const int av = (int)(key >> 32), bv = (int)(unsigned)(key & 0xffffffffull);
  if (av) atomicAdd(area_a + av - 1, len);
  if (bv) atomicAdd(area_b + bv - 1, len);
  if (av && bv) pair_insert(key, len, keys, counts, slots, cap, ctl);
}

// A workgroup owns PR_ROUNDS x 256 consecutive voxels (four rows of a 1024-wide map) and gathers its runs in a direct-mapped LDS table
// first: an instance crossed by several of its rows costs the global tables one add, not one per row (single-lane atomics that meet at
// the memory side are what bounds this pass).  A run whose LDS entry is taken by another key goes to the global tables directly.
constexpr int PR_ROUNDS = 16, PR_CACHE = 512;

__global__ __launch_bounds__(INS_THREADS) void pairs_insert_kernel(const int* __restrict__ a, const int* __restrict__ b, int na, int nb,
                                                                   unsigned long long* __restrict__ keys, int* __restrict__ counts,
                                                                   int64_t slots, int cap, int* __restrict__ area_a, int* __restrict__ area_b,
                                                                   int* __restrict__ ctl, int64_t N) {
  __shared__ unsigned long long cache_key[PR_CACHE];
  __shared__ int cache_count[PR_CACHE];
  const int lane = threadIdx.x & 63;
  for (int t = threadIdx.x; t < PR_CACHE; t += INS_THREADS) cache_key[t] = 0ull, cache_count[t] = 0;
  __syncthreads();
#pragma unroll 1
  for (int part = 0; part < PR_ROUNDS / INS_ITER; ++part) {
    const int64_t first = (int64_t)blockIdx.x * PR_ROUNDS + part * INS_ITER;
    if (first * INS_THREADS >= N) break;                    // workgroup-uniform
    int loaded_a[INS_ITER], loaded_b[INS_ITER];
    ins_load(loaded_a, a, N, first);
    ins_load(loaded_b, b, N, first);
#pragma unroll
    for (int it = 0; it < INS_ITER; ++it) {
      const bool live = ins_voxel_of(first + it) < N;
      int av = loaded_a[it], bv = loaded_b[it];
      const bool out_a = av < 0 || av > na, out_b = bv < 0 || bv > nb;
      const unsigned long long ma = __ballot(out_a), mb = __ballot(out_b);
      if (lane == 0) {
        if (ma) atomicAdd(ctl + PR_OUTSIDE_A, (int)__popcll(ma));
        if (mb) atomicAdd(ctl + PR_OUTSIDE_B, (int)__popcll(mb));
      }
      if (out_a) av = 0;
      if (out_b) bv = 0;
      if (__ballot((av | bv) != 0) == 0ull) continue;       // wave-uniform
      const int left_a = __shfl_up(av, 1), left_b = __shfl_up(bv, 1);
      const bool head = lane == 0 || !live || av != left_a || bv != left_b;
      const unsigned long long heads = __ballot(head);
      if (head && (av | bv) != 0) {                         // (no shuffle or ballot inside)
        const int len = run_length(heads, lane);
        const unsigned long long key = ((unsigned long long)(unsigned)av << 32) | (unsigned)bv;
        const int c = (int)(pair_hash(key) & (PR_CACHE - 1));
        const unsigned long long prev = atomicCAS(cache_key + c, 0ull, key);
        if (prev == 0ull || prev == key) atomicAdd(cache_count + c, len);
        else pair_add(key, len, keys, counts, slots, cap, area_a, area_b, ctl);
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < PR_CACHE; t += INS_THREADS)
    if (cache_key[t]) pair_add(cache_key[t], cache_count[t], keys, counts, slots, cap, area_a, area_b, ctl);
}

__global__ __launch_bounds__(INS_THREADS) void pairs_count_kernel(const unsigned long long* __restrict__ keys, int64_t slots, int na, int cap,
                                                                  const int* __restrict__ ctl, int* __restrict__ rows) {
  if (ctl[PR_DISTINCT] > cap) return;
  const int64_t s = (int64_t)blockIdx.x * INS_THREADS + threadIdx.x;
  if (s >= slots) return;
  const unsigned long long key = keys[s];
  const int i = (int)(key >> 32);
  if (key && i <= na) atomicAdd(rows + i - 1, 1);
}

__global__ __launch_bounds__(INS_THREADS) void pairs_sums_kernel(int* __restrict__ tile_sum, int tiles) { ins_scan_sums(tile_sum, tiles); }

// every pair to the bucket of its i, in the order of arrival: pairs_rank_kernel orders the bucket
__global__ __launch_bounds__(INS_THREADS) void pairs_scatter_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ counts,
                                                                    int64_t slots, int na, int cap, const int* __restrict__ ctl,
                                                                    const int* __restrict__ offs, const int* __restrict__ tile_off,
                                                                    int* __restrict__ cursor, int* __restrict__ tmp) {
  if (ctl[PR_DISTINCT] > cap) return;
  const int64_t s = (int64_t)blockIdx.x * INS_THREADS + threadIdx.x;
  if (s >= slots) return;
  const unsigned long long key = keys[s];
  const int i = (int)(key >> 32);
  if (!key || i > na) return;
  const int p = tile_off[(i - 1) / INS_TILE] + offs[i - 1] + atomicAdd(cursor + i - 1, 1);
  if (p >= cap) return;                                     // (cannot happen: the buckets hold ctl[PR_DISTINCT] <= cap rows in all)
  tmp[p * 3 + 0] = i;
  tmp[p * 3 + 1] = (int)(unsigned)(key & 0xffffffffull);
  tmp[p * 3 + 2] = counts[s];
}

// row e of the buckets goes to its bucket's start + the number of rows of the bucket with a smaller j (the j of a bucket are distinct)
__global__ __launch_bounds__(INS_THREADS) void pairs_rank_kernel(const int* __restrict__ tmp, const int* __restrict__ rows,
                                                                 const int* __restrict__ offs, const int* __restrict__ tile_off, int cap,
                                                                 const int* __restrict__ ctl, int* __restrict__ pairs, int* __restrict__ info) {
  const int distinct = ctl[PR_DISTINCT];
  const bool overflow = distinct > cap;
  const int64_t e = (int64_t)blockIdx.x * INS_THREADS + threadIdx.x;
  if (e == 0) {
    info[0] = overflow ? 0 : distinct;
    info[1] = overflow ? 1 : 0;
    info[2] = ctl[PR_OUTSIDE_A];
    info[3] = ctl[PR_OUTSIDE_B];
  }
  if (overflow || e >= distinct) return;
  const int i = tmp[e * 3], j = tmp[e * 3 + 1];
  const int start = tile_off[(i - 1) / INS_TILE] + offs[i - 1], n = rows[i - 1];
  if (start < 0 || n < 0 || (int64_t)start + n > cap) return;   // (cannot happen)
  int below = 0;
  for (int k = 0; k < n; ++k) below += tmp[(int64_t)(start + k) * 3 + 1] < j ? 1 : 0;
  int* row = pairs + (int64_t)(start + below) * 3;
  row[0] = i;
  row[1] = j;
  row[2] = tmp[e * 3 + 2];
}

// ---- paint ------------------------------------------------------------------------------------------------------------------------------
struct PaintArgs {
  const uint8_t* masks;                                     // [n, H, W]
  const int* order;                                         // [n] or null = 0 .. n - 1
  const int* boxes;                                         // [n, 4] (x0, y0, x1, y1) inclusive per MASK, or null
  int n, W;
  int64_t HW;
};

// is pixel (x, y) = p inside the mask painted at position k of the order?
__device__ __forceinline__ bool paint_covers(const PaintArgs& g, int k, int64_t p, int x, int y) {
  const int m = g.order ? g.order[k] : k;
  if (m < 0 || m >= g.n) return false;
  if (g.boxes) {
    const int* bx = g.boxes + (int64_t)m * 4;
    if (x < bx[0] || y < bx[1] || x > bx[2] || y > bx[3]) return false;
  }
  return g.masks[(int64_t)m * g.HW + p] != 0;
}

// Launch k = -1 .. n - 1: paints position k where flags[k] says so (final: written by the launches before this one), then says in
// flags[k + 1] whether position k + 1 still has a pixel on a 0 of the map -- per pixel both steps belong to one thread.
__global__ __launch_bounds__(INS_THREADS) void paint_step_kernel(PaintArgs g, int k, int* __restrict__ flags, int* __restrict__ map) {
  const int lane = threadIdx.x & 63;
  const bool paints = k >= 0 && flags[k] != 0, asks = k + 1 < g.n;
#pragma unroll 1
  for (int it = 0; it < INS_ITER; ++it) {
    const int64_t p = ins_voxel(it);
    const bool live = p < g.HW;
    bool open = false;
    if (live) {
      const int y = (int)(p / g.W), x = (int)(p - (int64_t)y * g.W);
      int cur = map[p];
      if (paints && paint_covers(g, k, p, x, y)) map[p] = cur = k + 1;
      open = asks && cur == 0 && paint_covers(g, k + 1, p, x, y);
    }
    const unsigned long long any = __ballot(open);
    if (any && lane == (int)__ffsll((long long)any) - 1) flags[k + 1] = 1;   // the same value whoever stores it
  }
}

// skip_covered == 0: a pixel takes the last position of the order that covers it
__global__ __launch_bounds__(INS_THREADS) void paint_all_kernel(PaintArgs g, int* __restrict__ map) {
#pragma unroll 1
  for (int it = 0; it < INS_ITER; ++it) {
    const int64_t p = ins_voxel(it);
    if (p >= g.HW) break;
    const int y = (int)(p / g.W), x = (int)(p - (int64_t)y * g.W);
    int id = 0;
    for (int k = g.n - 1; k >= 0 && id == 0; --k)
      if (paint_covers(g, k, p, x, y)) id = k + 1;
    map[p] = id;
  }
}

static inline bool ins_aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" size_t msam2_instance_remap_workspace_bytes(int64_t id_bound) {
  if (id_bound < 1 || id_bound > INT32_MAX) return 0;
  const int64_t words = (id_bound + 31) / 32, tiles = (words + INS_TILE - 1) / INS_TILE;
  return (size_t)(2 * words + RM_CTL + tiles) * sizeof(int);
}

extern "C" int msam2_instance_remap(const int32_t* map, const uint8_t* labels, int64_t D, int64_t H, int64_t W, int64_t id_bound, int32_t* out,
                                    int32_t* orig, int32_t* size, int32_t* cls, int64_t cap, int32_t* info, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(map && out && orig && size && cls && info && workspace, "instance_remap: null map / out / orig / size / cls / info / workspace");
  LABEL_REQUIRE_SIZES("instance_remap", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(id_bound >= 1 && id_bound <= INT32_MAX, "instance_remap: id_bound = %lld (1 .. 2^31 - 1)", (long long)id_bound);
  MSAM2_REQUIRE(cap >= 1 && cap <= INT32_MAX, "instance_remap: cap = %lld table rows (1 .. 2^31 - 1)", (long long)cap);
  MSAM2_REQUIRE(workspace_bytes >= msam2_instance_remap_workspace_bytes(id_bound), "instance_remap: workspace too small (%zu of %zu bytes)",
                workspace_bytes, msam2_instance_remap_workspace_bytes(id_bound));
  MSAM2_REQUIRE(ins_aligned4(map) && ins_aligned4(out) && ins_aligned4(orig) && ins_aligned4(size) && ins_aligned4(cls) && ins_aligned4(info) &&
                    ins_aligned4(workspace),
                "instance_remap: map / out / tables / workspace must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = D * H * W, words = (id_bound + 31) / 32;
  const int tiles = cdiv(words, INS_TILE);
  unsigned* bitmap = (unsigned*)workspace;
  int* ctl = (int*)workspace + words;
  int* local = ctl + RM_CTL;
  int* tile = local + words;
  fill_on(s, (int*)workspace, words + RM_CTL, 0);           // (common.h: why a kernel)
  fill_on(s, orig, cap, 0);
  fill_on(s, size, cap, 0);
  fill_on(s, cls, cap, 0);
  const dim3 grid(cdiv(N, INS_THREADS * INS_ITER)), blk(INS_THREADS);
  hipLaunchKernelGGL(remap_presence_kernel, grid, blk, 0, s, map, bitmap, ctl, id_bound, N);
  hipLaunchKernelGGL(ins_scan_tiles_kernel<true>, dim3(tiles), blk, 0, s, bitmap, local, tile, words);
  hipLaunchKernelGGL(remap_sums_kernel, dim3(1), blk, 0, s, tile, tiles, ctl, (int)cap, info);
  hipLaunchKernelGGL(remap_gather_kernel, dim3(cdiv(N, INS_THREADS * GA_ROUNDS)), blk, 0, s, map, labels, bitmap, local, tile, out, orig, size, cls, (int)cap, id_bound, N);
  return msam2_check_launch("instance_remap");
}

extern "C" int msam2_instance_apply(const int32_t* map, const int32_t* table, int64_t n, int64_t count, int32_t* out, void* stream) {
  MSAM2_REQUIRE(map && table && out, "instance_apply: null map / table / out");
  MSAM2_REQUIRE(n >= 0 && n < INT32_MAX, "instance_apply: n = %lld (the table holds n + 1 values, 0 .. 2^31 - 2)", (long long)n);
  MSAM2_REQUIRE(count >= 1 && count <= LABEL_MAX_VOXELS, "instance_apply: %lld voxels (1 .. 2^31 - 2)", (long long)count);
  MSAM2_REQUIRE(ins_aligned4(map) && ins_aligned4(table) && ins_aligned4(out), "instance_apply: map / table / out must be 4-byte aligned");
  hipLaunchKernelGGL(apply_kernel, dim3(cdiv(count, INS_THREADS * INS_ITER)), dim3(INS_THREADS), 0, (hipStream_t)stream, map, table, (int)n, out,
                     count);
  return msam2_check_launch("instance_apply");
}

extern "C" size_t msam2_instance_pairs_workspace_bytes(int64_t na, int64_t cap) {
  if (na < 1 || na > LABEL_MAX_VOXELS || cap < 1 || cap > INS_MAX_CAP) return 0;
  return pair_tables(nullptr, na, cap).bytes;
}

extern "C" int msam2_instance_pairs(const int32_t* a, const int32_t* b, int64_t D, int64_t H, int64_t W, int64_t na, int64_t nb, int32_t* pairs,
                                    int64_t cap, int32_t* area_a, int32_t* area_b, int32_t* info, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  MSAM2_REQUIRE(a && b && pairs && area_a && area_b && info && workspace, "instance_pairs: null a / b / pairs / area_a / area_b / info / workspace");
  LABEL_REQUIRE_SIZES("instance_pairs", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(na >= 1 && na <= LABEL_MAX_VOXELS && nb >= 1 && nb <= LABEL_MAX_VOXELS, "instance_pairs: na = %lld, nb = %lld instances (1 .. 2^31 - 2)",
                (long long)na, (long long)nb);
  MSAM2_REQUIRE(cap >= 1 && cap <= INS_MAX_CAP, "instance_pairs: cap = %lld pair rows (1 .. 2^26)", (long long)cap);
  MSAM2_REQUIRE(workspace_bytes >= msam2_instance_pairs_workspace_bytes(na, cap), "instance_pairs: workspace too small (%zu of %zu bytes)",
                workspace_bytes, msam2_instance_pairs_workspace_bytes(na, cap));
  MSAM2_REQUIRE(((uintptr_t)workspace & 7) == 0, "instance_pairs: workspace must be 8-byte aligned");
  MSAM2_REQUIRE(ins_aligned4(a) && ins_aligned4(b) && ins_aligned4(pairs) && ins_aligned4(area_a) && ins_aligned4(area_b) && ins_aligned4(info),
                "instance_pairs: maps and tables must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = D * H * W;
  const PairTables t = pair_tables(workspace, na, cap);
  const int tiles = cdiv(na, INS_TILE);
  fill_on(s, (int*)workspace, t.zeroed, 0);                 // (common.h: why a kernel)
  fill_on(s, pairs, cap * 3, 0);
  fill_on(s, area_a, na, 0);
  fill_on(s, area_b, nb, 0);
  const dim3 blk(INS_THREADS), over_slots(cdiv(t.slots, INS_THREADS));
  hipLaunchKernelGGL(pairs_insert_kernel, dim3(cdiv(N, INS_THREADS * PR_ROUNDS)), blk, 0, s, a, b, (int)na, (int)nb, t.keys, t.counts, t.slots, (int)cap,
                     area_a, area_b, t.ctl, N);
  hipLaunchKernelGGL(pairs_count_kernel, over_slots, blk, 0, s, t.keys, t.slots, (int)na, (int)cap, t.ctl, t.rows);
  hipLaunchKernelGGL(ins_scan_tiles_kernel<false>, dim3(tiles), blk, 0, s, (const unsigned*)t.rows, t.offs, t.tile, na);
  hipLaunchKernelGGL(pairs_sums_kernel, dim3(1), blk, 0, s, t.tile, tiles);
  hipLaunchKernelGGL(pairs_scatter_kernel, over_slots, blk, 0, s, t.keys, t.counts, t.slots, (int)na, (int)cap, t.ctl, t.offs, t.tile, t.cursor, t.tmp);
  hipLaunchKernelGGL(pairs_rank_kernel, dim3(cdiv(cap, INS_THREADS)), blk, 0, s, t.tmp, t.rows, t.offs, t.tile, (int)cap, t.ctl, pairs, info);
  return msam2_check_launch("instance_pairs");
}

extern "C" size_t msam2_instance_paint_workspace_bytes(int64_t n) {
  return n >= 1 && n <= INS_MAX_MASKS ? (size_t)(n + 1) * sizeof(int) : 0;
}

extern "C" int msam2_instance_paint(const uint8_t* masks, int64_t n, int64_t H, int64_t W, const int32_t* order, const int32_t* boxes,
                                    int skip_covered, int32_t* map, void* workspace, size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(masks && map && workspace, "instance_paint: null masks / map / workspace");
  MSAM2_REQUIRE(n >= 1 && n <= INS_MAX_MASKS, "instance_paint: n = %lld masks (1 .. %lld)", (long long)n, (long long)INS_MAX_MASKS);
  LABEL_REQUIRE_SIZES("instance_paint", (int64_t)1, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(workspace_bytes >= msam2_instance_paint_workspace_bytes(n), "instance_paint: workspace too small (%zu of %zu bytes)", workspace_bytes,
                msam2_instance_paint_workspace_bytes(n));
  MSAM2_REQUIRE(ins_aligned4(map) && ins_aligned4(workspace) && ins_aligned4(order) && ins_aligned4(boxes),
                "instance_paint: map / order / boxes / workspace must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const PaintArgs g = {masks, order, boxes, (int)n, (int)W, H * W};
  const dim3 grid(cdiv(H * W, INS_THREADS * INS_ITER)), blk(INS_THREADS);
  if (!skip_covered) {
    hipLaunchKernelGGL(paint_all_kernel, grid, blk, 0, s, g, map);
    return msam2_check_launch("instance_paint");
  }
  int* flags = (int*)workspace;
  fill_on(s, flags, n + 1, 0);                              // (common.h: why a kernel)
  fill_on(s, map, H * W, 0);
  for (int k = -1; k < (int)n; ++k) hipLaunchKernelGGL(paint_step_kernel, grid, blk, 0, s, g, k, flags, map);
  return msam2_check_launch("instance_paint");
}
