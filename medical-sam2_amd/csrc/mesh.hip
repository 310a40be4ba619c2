// Surface meshes of label volumes: surface nets on the device, gfx950.  DESIGN 7.22 states the definitions; in short:
//
//   lattice point p = (k, j, i), 0 <= k <= D, 0 <= j <= H, 0 <= i <= W: the common corner of the eight voxels (k-1..k, j-1..j, i-1..i), its
//   CELL; voxels outside the volume are not the organ.  p is a VERTEX of organ v iff the eight values of (labels == v) are not all equal;
//   vertices are numbered per organ in ascending lattice index.  There is one QUAD per voxel face between organ and not-organ, named by its
//   lowest lattice corner q0 and its normal axis a (z 0, y 1, x 2), ordered by 3 index(q0) + a, wound so that the normal looks out of the
//   organ.  A vertex sits at the cell's centre ("corner": the voxel-face surface) or at the mean of the cell's crossed edges' midpoints
//   ("nets"), optionally relaxed by Jacobi sweeps over the linked vertices with every vertex kept inside its cell.
//
//   msam2_label_mesh_count   one pass over the whole volume: (vertices, quads) of up to 32 organs
//   msam2_label_mesh         per organ inside its box: the vertex and quad tables in the canonical order
//
// The eight membership bits of a cell are one byte.  msam2_label_mesh reads the labels ONCE (mesh_flag_kernel) and keeps that byte per
// lattice point of the box in the workspace; vertex flag, the three quad flags, the winding, the nets position and the links of the
// relaxation are all functions of it.  A wave owns 64 consecutive lattice points of the box (a WORD): the ballot of the vertex flags is the
// word's bitmap, a vertex's number is (vertices in the words before) + popcount(the bitmap below its lane), a quad's number likewise from
// the three ballots of the quad flags.  "The words before" is an exclusive scan over the words, split over launches as in instances.hip
// (tiles of MESH_TILE_WORDS words, then the tile sums by one workgroup per organ): no workgroup ever waits for another.  Everything is an
// integer or a fixed sequence of float64 operations (contraction off), every store goes to a slot that its canonical number decides:
// no byte depends on scheduling, on the grouping or on the box's slack.
#include "label_boxes.h"

#pragma clang fp contract(off)                              // u * spacing + origin and the sweeps' sums must not fuse

namespace {

constexpr int MESH_THREADS = 256;
constexpr int MESH_WAVES = MESH_THREADS / 64;               // words per workgroup and grid-stride trip
constexpr int MESH_TILE_WORDS = 256;                        // words of a scan tile: one per thread (16384 lattice points)
constexpr int MESH_GRID_CAP = 2048;                         // workgroups per organ of the lattice kernels: 2^19 lattice points per trip
constexpr int MESH_CHUNK = 16, MESH_COUNT_GRID_CAP = 65536;     // lattice points of a lane of the count pass; its workgroups
constexpr int64_t MESH_MAX_LATTICE = 1ll << 29;             // lattice points of a box: three quads per point still fit an int32
constexpr int MESH_MAX_RELAX = 64;
enum { MESH_CORNER = 0, MESH_NETS = 1 };

struct MeshOrgan : LabelBox {
  int value, j;                                             // label value; row of counts
  int L, words, tiles;                                      // lattice points (bd + 1)(bh + 1)(bw + 1), words of 64, scan tiles
  int v_cap, q_cap;
  long long ws, v_off, q_off;                               // the organ's tables in the workspace; first row in vertices / quads
};
struct MeshJobs {
  MeshOrgan o[LABEL_MAX_OBJ];
  int n, H, W;
};

// The tables of one organ, as offsets from its place in the workspace (each 16-byte granular):
//   m8 uint8 [L] the cell bytes, vbits uint64 [words] the vertex bitmap, vpre / qpre int32 [words] vertices / quads in the tile's words
//   before, tv / tq int32 [tiles] those of the tiles before, and with relax > 0 two float64 [L, 3] position buffers.
struct MeshTables {
  long long m8, vbits, vpre, qpre, tv, tq, u0, u1, bytes;
};
__host__ __device__ __forceinline__ long long mesh_round16(long long b) { return (b + 15) & ~15ll; }
__host__ __device__ __forceinline__ MeshTables mesh_tables(long long L, bool relax) {
  const long long words = (L + 63) / 64, tiles = (words + MESH_TILE_WORDS - 1) / MESH_TILE_WORDS;
  MeshTables t;
  t.m8 = 0;
  t.vbits = mesh_round16(L);
  t.vpre = t.vbits + mesh_round16(8 * words);
  t.qpre = t.vpre + mesh_round16(4 * words);
  t.tv = t.qpre + mesh_round16(4 * words);
  t.tq = t.tv + mesh_round16(4 * tiles);
  t.u0 = t.tq + mesh_round16(4 * tiles);
  t.u1 = t.u0 + (relax ? mesh_round16(24 * L) : 0);
  t.bytes = t.u1 + (relax ? mesh_round16(24 * L) : 0);
  return t;
}
static inline int64_t mesh_box_lattice(const int32_t* b) {
  return ((int64_t)b[1] - b[0] + 2) * ((int64_t)b[3] - b[2] + 2) * ((int64_t)b[5] - b[4] + 2);
}
// (without a volume: msam2_label_mesh_workspace_bytes knows the box alone)
static inline bool mesh_box_upright(const int32_t* b) {
  return b[0] >= 0 && b[0] <= b[1] && b[1] < LABEL_MAX_SLICES && b[2] >= 0 && b[2] <= b[3] && b[3] < LABEL_MAX_SIDE && b[4] >= 0 && b[4] <= b[5] &&
         b[5] < LABEL_MAX_SIDE;
}

// ---- the cell byte ------------------------------------------------------------------------------------------------------------------------
// bit 4 dz + 2 dy + dx: voxel (k - 1 + dz, j - 1 + dy, i - 1 + dx) is the organ
__device__ __forceinline__ bool mesh_is_vertex(int m) { return m != 0 && m != 255; }
// quad with q0 = this point and normal axis a: between voxel B = (k, j, i), bit 7, and A = B - e_a, bit 3 (z), 5 (y), 6 (x)
__device__ __forceinline__ int mesh_a_bit(int m, int a) { return (m >> (a == 0 ? 3 : a == 1 ? 5 : 6)) & 1; }
__device__ __forceinline__ bool mesh_has_quad(int m, int a) { return mesh_a_bit(m, a) != ((m >> 7) & 1); }
// the four voxels with d_a = side are not all equal: the link to the neighbouring vertex on that side along a
__device__ __forceinline__ bool mesh_linked(int m, int a, int side) {
  const int all = a == 0 ? 0x0f : a == 1 ? 0x33 : 0x55, shift = side ? (a == 0 ? 4 : a == 1 ? 2 : 1) : 0;
  const int four = (m >> shift) & all;
  return four != 0 && four != all;
}

// position of a vertex in voxel units along a, c = its lattice coordinate along a
__device__ __forceinline__ double mesh_position(int m, int a, int c, int placement) {
  if (placement == MESH_CORNER) return (double)c - 0.5;
  // the crossed edges of the cell: along x at bits (dz, dy, 0), along y at (dz, 0, dx), along z at (0, dy, dx)
  const int ex = (m ^ (m >> 1)) & 0x55, ey = (m ^ (m >> 2)) & 0x33, ez = (m ^ (m >> 4)) & 0x0f;
  const int n = __popc(ex) + __popc(ey) + __popc(ez);
  int s;                                                    // crossed edges not along a: on the high side minus on the low side
  if (a == 0) s = __popc(ex & 0x50) - __popc(ex & 0x05) + __popc(ey & 0x30) - __popc(ey & 0x03);
  else if (a == 1) s = __popc(ex & 0x44) - __popc(ex & 0x11) + __popc(ez & 0x0c) - __popc(ez & 0x03);
  else s = __popc(ey & 0x22) - __popc(ey & 0x11) + __popc(ez & 0x0a) - __popc(ez & 0x05);
  return (double)((2 * c - 1) * n + s) / (double)(2 * n);   // |numerator| < 2^21: both exact
}

__device__ __forceinline__ unsigned long long mesh_lanes_below(int lane) { return (1ull << lane) - 1ull; }

// what the lattice kernels share: the organ's tables and the point of this lane in word w
struct MeshView {
  uint8_t* m8;
  unsigned long long* vbits;
  int *vpre, *qpre, *tv, *tq;
  double *u0, *u1;
  int lw, lh;                                               // lattice points per row, rows per slice
  __device__ __forceinline__ MeshView(const MeshOrgan& o, char* ws, bool relax) {
    const MeshTables t = mesh_tables(o.L, relax);
    char* base = ws + o.ws;
    m8 = (uint8_t*)(base + t.m8), vbits = (unsigned long long*)(base + t.vbits);
    vpre = (int*)(base + t.vpre), qpre = (int*)(base + t.qpre), tv = (int*)(base + t.tv), tq = (int*)(base + t.tq);
    u0 = (double*)(base + t.u0), u1 = (double*)(base + t.u1);
    lw = o.bw + 1, lh = o.bh + 1;
  }
  __device__ __forceinline__ void coords(int p, int& kb, int& jb, int& ib) const {
    const int r = p / lw;
    ib = p - r * lw, kb = r / lh, jb = r - kb * lh;
  }
  // number of the vertex at lattice point p of the box (p is a vertex)
  __device__ __forceinline__ int vertex_number(int p) const {
    const int w = p >> 6;
    return tv[w / MESH_TILE_WORDS] + vpre[w] + __popcll(vbits[w] & mesh_lanes_below(p & 63));
  }
};

// exclusive scan of one value per thread over the workgroup's 256 threads; *total: the sum of all.  All threads call it.
__device__ __forceinline__ int mesh_block_scan(int v, int* total) {
  __shared__ int wave_sum[MESH_WAVES];
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
  for (int w = 0; w < MESH_WAVES; ++w) {
    if (w < wave) base += wave_sum[w];
    all += wave_sum[w];
  }
  *total = all;
  __syncthreads();                                          // wave_sum may be written again by the next call
  return base + inc - v;
}

// the four voxels (kb - 1 + dz, jb - 1 + dy, xb) of the box, bit 2 dz + dy; beyond the box: not the organ.  0 <= xb < bw.
__device__ __forceinline__ int mesh_column(const uint8_t* __restrict__ labels, const MeshOrgan& o, int H, int W, int kb, int jb, int xb) {
  int bits = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int z = kb - 1 + (d >> 1), y = jb - 1 + (d & 1);
    if (z >= 0 && z < o.bd && y >= 0 && y < o.bh)
      bits |= (labels[((int64_t)(o.z0 + z) * H + o.y0 + y) * W + o.x0 + xb] == o.value ? 1 : 0) << d;
  }
  return bits;
}
// column bits (dz, dy) -> their places in the cell byte with dx = 0
__device__ __forceinline__ int mesh_spread(int col) { return (col & 1) | (col & 2) << 1 | (col & 4) << 2 | (col & 8) << 3; }

// ---- msam2_label_mesh ---------------------------------------------------------------------------------------------------------------------
// blockIdx.y = organ of the group.  The only launch that reads the labels: a lane loads the column of its point's own x (the cell's high
// side), the low side is the left lane's (the same row when ib > 0); lane 0 loads its own.
__global__ __launch_bounds__(MESH_THREADS) void mesh_flag_kernel(const uint8_t* __restrict__ labels, MeshJobs jobs, char* __restrict__ ws) {
  const MeshOrgan& o = jobs.o[blockIdx.y];
  const MeshView t(o, ws, false);
  const int lane = threadIdx.x & 63;
  for (int w = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6); w < o.words; w += gridDim.x * MESH_WAVES) {   // wave-uniform
    const int p = w * 64 + lane;
    const bool live = p < o.L;
    int kb = 0, jb = 0, ib = 0, high = 0;
    if (live) {
      t.coords(p, kb, jb, ib);
      if (ib < o.bw) high = mesh_column(labels, o, jobs.H, jobs.W, kb, jb, ib);
    }
    int low = __shfl_up(high, 1);
    if (ib == 0) low = 0;
    else if (lane == 0 && live) low = mesh_column(labels, o, jobs.H, jobs.W, kb, jb, ib - 1);
    const int m = live ? (mesh_spread(low) | mesh_spread(high) << 1) : 0;
    const unsigned long long bv = __ballot(mesh_is_vertex(m));
    const unsigned long long bz = __ballot(mesh_has_quad(m, 0)), by = __ballot(mesh_has_quad(m, 1)), bx = __ballot(mesh_has_quad(m, 2));
    if (live) t.m8[p] = (uint8_t)m;
    if (lane == 0) {
      t.vbits[w] = bv;
      t.qpre[w] = __popcll(bz) + __popcll(by) + __popcll(bx);
    }
  }
}

// first level of the two scans: vertices and quads in the words before, within the tile; the tile's sums
__global__ __launch_bounds__(MESH_THREADS) void mesh_scan_tiles_kernel(MeshJobs jobs, char* __restrict__ ws) {
  const MeshOrgan& o = jobs.o[blockIdx.y];
  if ((int)blockIdx.x >= o.tiles) return;                   // workgroup-uniform
  const MeshView t(o, ws, false);
  const int w = blockIdx.x * MESH_TILE_WORDS + threadIdx.x;
  const int v = w < o.words ? __popcll(t.vbits[w]) : 0, q = w < o.words ? t.qpre[w] : 0;
  int total_v, total_q;
  const int ex_v = mesh_block_scan(v, &total_v), ex_q = mesh_block_scan(q, &total_q);
  if (w < o.words) t.vpre[w] = ex_v, t.qpre[w] = ex_q;
  if (threadIdx.x == 0) t.tv[blockIdx.x] = total_v, t.tq[blockIdx.x] = total_q;
}

// second level, ONE workgroup per organ: the tile sums -> their exclusive scans, in place, 256 tiles per trip with a carry; the true counts
__global__ __launch_bounds__(MESH_THREADS) void mesh_scan_sums_kernel(MeshJobs jobs, char* __restrict__ ws, int* __restrict__ counts) {
  const MeshOrgan& o = jobs.o[blockIdx.y];
  const MeshView t(o, ws, false);
  int carry_v = 0, carry_q = 0;
  for (int base = 0; base < o.tiles; base += MESH_THREADS) {
    const int i = base + threadIdx.x;
    const int v = i < o.tiles ? t.tv[i] : 0, q = i < o.tiles ? t.tq[i] : 0;
    int total_v, total_q;
    const int ex_v = mesh_block_scan(v, &total_v), ex_q = mesh_block_scan(q, &total_q);
    if (i < o.tiles) t.tv[i] = carry_v + ex_v, t.tq[i] = carry_q + ex_q;
    carry_v += total_v, carry_q += total_q;
  }
  if (threadIdx.x == 0) counts[2 * o.j] = carry_v, counts[2 * o.j + 1] = carry_q;
}

struct MeshFrame {
  double sz, sy, sx, oz, oy, ox;
};
__device__ __forceinline__ void mesh_store_vertex(float* __restrict__ row, const double (&u)[3], const MeshFrame& f) {
  row[0] = (float)(u[0] * f.sz + f.oz);
  row[1] = (float)(u[1] * f.sy + f.oy);
  row[2] = (float)(u[2] * f.sx + f.ox);
}

// quads in the canonical order, and the vertices' start positions: to the vertex table (relax == 0) or to the first position buffer
__global__ __launch_bounds__(MESH_THREADS) void mesh_emit_kernel(MeshJobs jobs, char* __restrict__ ws, int placement, int relax, MeshFrame f,
                                                                 float* __restrict__ vertices, int* __restrict__ quads) {
  const MeshOrgan& o = jobs.o[blockIdx.y];
  const MeshView t(o, ws, relax > 0);
  const int lane = threadIdx.x & 63;
  const int stride[3] = {t.lh * t.lw, t.lw, 1};
  for (int w = blockIdx.x * MESH_WAVES + (threadIdx.x >> 6); w < o.words; w += gridDim.x * MESH_WAVES) {   // wave-uniform
    if (t.vbits[w] == 0ull) continue;                       // wave-uniform: no vertex in the word, so no quad starts in it either
    const int p = w * 64 + lane;
    const int m = p < o.L ? t.m8[p] : 0;
    const unsigned long long bz = __ballot(mesh_has_quad(m, 0)), by = __ballot(mesh_has_quad(m, 1)), bx = __ballot(mesh_has_quad(m, 2));
    if (mesh_is_vertex(m)) {
      int kb, jb, ib;
      t.coords(p, kb, jb, ib);
      const double u[3] = {mesh_position(m, 0, o.z0 + kb, placement), mesh_position(m, 1, o.y0 + jb, placement),
                           mesh_position(m, 2, o.x0 + ib, placement)};
      if (relax > 0) {
        t.u0[3ll * p] = u[0], t.u0[3ll * p + 1] = u[1], t.u0[3ll * p + 2] = u[2];
      } else {
        const int number = t.vertex_number(p);
        if (number < o.v_cap) mesh_store_vertex(vertices + (o.v_off + number) * 3, u, f);
      }
    }
    if ((bz | by | bx) == 0ull) continue;                   // wave-uniform
    const unsigned long long below = mesh_lanes_below(lane);
    int number = t.tq[w / MESH_TILE_WORDS] + t.qpre[w] + __popcll(bz & below) + __popcll(by & below) + __popcll(bx & below);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!mesh_has_quad(m, a)) continue;
      if (number < o.q_cap) {
        // (b, c): e_b x e_c = e_a in the frame (x, y, z) -- z: (x, y), y: (z, x), x: (y, z); A the organ: q0, +b, +b+c, +c, else mirrored
        const int sb = stride[a == 0 ? 2 : a == 1 ? 0 : 1], sc = stride[a == 0 ? 1 : a == 1 ? 2 : 0];
        const int first = mesh_a_bit(m, a) ? sb : sc, last = mesh_a_bit(m, a) ? sc : sb;
        int* row = quads + (o.q_off + number) * 4;
        row[0] = t.vertex_number(p);
        row[1] = t.vertex_number(p + first);
        row[2] = t.vertex_number(p + sb + sc);
        row[3] = t.vertex_number(p + last);
      }
      ++number;
    }
  }
}

// one Jacobi sweep src -> dst: the mean of the linked vertices' positions, summed in the order -z, -y, -x, +x, +y, +z, kept in the cell
__global__ __launch_bounds__(MESH_THREADS) void mesh_relax_kernel(MeshJobs jobs, char* __restrict__ ws, int flip) {
  const MeshOrgan& o = jobs.o[blockIdx.y];
  const MeshView t(o, ws, true);
  const double* __restrict__ src = flip ? t.u1 : t.u0;
  double* __restrict__ dst = flip ? t.u0 : t.u1;
  const int stride[3] = {t.lh * t.lw, t.lw, 1};
  for (int p = (blockIdx.x * MESH_WAVES + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63); p < o.L; p += gridDim.x * MESH_THREADS) {
    if (t.vbits[p >> 6] == 0ull) continue;                  // wave-uniform (a wave's 64 points are one word): nothing to move
    const int m = t.m8[p];
    if (!mesh_is_vertex(m)) continue;
    double s[3] = {0.0, 0.0, 0.0};
    int links = 0;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const int a = e < 3 ? e : 5 - e, side = e < 3 ? 0 : 1;
      if (!mesh_linked(m, a, side)) continue;
      const double* q = src + 3ll * (side ? p + stride[a] : p - stride[a]);
      s[0] += q[0], s[1] += q[1], s[2] += q[2];
      ++links;
    }
    int c[3];
    t.coords(p, c[0], c[1], c[2]);
    c[0] += o.z0, c[1] += o.y0, c[2] += o.x0;
    const double n = (double)links;                         // >= 3 at a vertex
#pragma unroll
    for (int a = 0; a < 3; ++a) dst[3ll * p + a] = fmin(fmax(s[a] / n, (double)(c[a] - 1)), (double)c[a]);
  }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_store_kernel(MeshJobs jobs, char* __restrict__ ws, int flip, MeshFrame f,
                                                                  float* __restrict__ vertices) {
  const MeshOrgan& o = jobs.o[blockIdx.y];
  const MeshView t(o, ws, true);
  const double* __restrict__ src = flip ? t.u1 : t.u0;
  for (int p = (blockIdx.x * MESH_WAVES + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63); p < o.L; p += gridDim.x * MESH_THREADS) {
    if (t.vbits[p >> 6] == 0ull || !mesh_is_vertex(t.m8[p])) continue;
    const int number = t.vertex_number(p);
    if (number >= o.v_cap) continue;
    const double u[3] = {src[3ll * p], src[3ll * p + 1], src[3ll * p + 2]};
    mesh_store_vertex(vertices + (o.v_off + number) * 3, u, f);
  }
}

// ---- msam2_label_mesh_count ---------------------------------------------------------------------------------------------------------------
struct MeshCountArgs {
  const uint8_t* labels;
  const uint8_t* ids;
  int n, D, H, W;
  unsigned long long* counts;
};

// organ (index in ids) of voxel (z, y, x), -1 for a value that is not listed and beyond the volume
__device__ __forceinline__ int mesh_count_organ(const MeshCountArgs& a, const signed char* lut, int z, int y, int x) {
  if (z < 0 || z >= a.D || y < 0 || y >= a.H || x < 0 || x >= a.W) return -1;
  return lut[a.labels[((int64_t)z * a.H + y) * a.W + x]];
}

// one lattice point whose cell may be mixed: a vertex for every organ the cell holds beside something else, a quad for both sides of the
// three faces at voxel B = (k, j, i)
__device__ __forceinline__ void mesh_count_point(const MeshCountArgs& a, const signed char* lut, int (*cnt)[2], int k, int j, int i) {
  int organ[8];                                             // cell voxel e = 4 dz + 2 dy + dx
#pragma unroll
  for (int e = 0; e < 8; ++e) organ[e] = mesh_count_organ(a, lut, k - 1 + (e >> 2), j - 1 + ((e >> 1) & 1), i - 1 + (e & 1));
  bool same = true;
#pragma unroll
  for (int e = 1; e < 8; ++e) same = same && organ[e] == organ[0];
  if (same) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bool first = organ[e] >= 0;
#pragma unroll
    for (int g = 0; g < e; ++g) first = first && organ[g] != organ[e];
    if (first) atomicAdd(&cnt[organ[e]][0], 1);
  }
  const int b = organ[7];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const int av = organ[ax == 0 ? 3 : ax == 1 ? 5 : 6];
    if (av == b) continue;
    if (av >= 0) atomicAdd(&cnt[av][1], 1);
    if (b >= 0) atomicAdd(&cnt[b][1], 1);
  }
}

__device__ __forceinline__ uint4 mesh_load16(const uint8_t* p) {   // any alignment
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// A lane owns a CHUNK of MESH_CHUNK = 16 consecutive lattice points of one lattice row (k, j), i0 .. i0 + 15: their cells are the columns
// x = i0 - 1 .. i0 + 15 of the four voxel rows (k-1..k, j-1..j).  Where all of that lies inside the volume the lane takes the four rows as
// 16-byte loads (any alignment) and the column in front as bytes; 68 equal bytes -- the inside of an organ or of the background, nearly
// every chunk -- cost nothing more.  Any other chunk, and the chunks on the frame, go point by point through bounds-checked byte loads.
__global__ __launch_bounds__(MESH_THREADS) void mesh_count_kernel(MeshCountArgs a) {
  __shared__ signed char lut[256];
  __shared__ int cnt[LABEL_MAX_OBJ][2];
  const int tid = threadIdx.x;
  if (tid < LABEL_MAX_OBJ * 2) (&cnt[0][0])[tid] = 0;
  ids_to_object_table(lut, a.ids, a.n, tid);
  const int lh = a.H + 1, per_row = (a.W + MESH_CHUNK) / MESH_CHUNK;   // chunks of a lattice row of W + 1 points
  const int64_t chunks = (int64_t)(a.D + 1) * lh * per_row;
  for (int64_t c = (int64_t)blockIdx.x * MESH_THREADS + tid; c < chunks; c += (int64_t)gridDim.x * MESH_THREADS) {
    const int64_t row = c / per_row;
    const int i0 = (int)(c - row * per_row) * MESH_CHUNK, k = (int)(row / lh), j = (int)(row - (int64_t)k * lh);
    if (k >= 1 && k < a.D && j >= 1 && j < a.H && i0 >= 1 && i0 + MESH_CHUNK <= a.W) {
      const uint8_t* p = a.labels + ((int64_t)(k - 1) * a.H + (j - 1)) * a.W + i0;
      const int64_t plane = (int64_t)a.H * a.W;
      const uint4 r0 = mesh_load16(p), r1 = mesh_load16(p + a.W), r2 = mesh_load16(p + plane), r3 = mesh_load16(p + plane + a.W);
      const unsigned v = (unsigned)p[-1] * 0x01010101u;
      const bool front = p[a.W - 1] * 0x01010101u == v && p[plane - 1] * 0x01010101u == v && p[plane + a.W - 1] * 0x01010101u == v;
      const unsigned diff = (r0.x ^ v) | (r0.y ^ v) | (r0.z ^ v) | (r0.w ^ v) | (r1.x ^ v) | (r1.y ^ v) | (r1.z ^ v) | (r1.w ^ v) | (r2.x ^ v) |
                            (r2.y ^ v) | (r2.z ^ v) | (r2.w ^ v) | (r3.x ^ v) | (r3.y ^ v) | (r3.z ^ v) | (r3.w ^ v);
      if (front && diff == 0u) continue;
    }
    const int end = min(i0 + MESH_CHUNK, a.W + 1);
    for (int i = i0; i < end; ++i) mesh_count_point(a, lut, cnt, k, j, i);
  }
  __syncthreads();
  if (tid < a.n * 2) {
    const int c = (&cnt[0][0])[tid];
    if (c) atomicAdd(a.counts + tid, (unsigned long long)c);
  }
}

static inline bool mesh_finite(double x) { return x - x == 0.0; }

}  // namespace

// ids: DEVICE uint8 [n] (distinct, 1 .. 255: the caller checks).  counts int64 [n, 2] = (vertices, quads), zeroed by the call on `stream`.
extern "C" int msam2_label_mesh_count(const uint8_t* labels, const uint8_t* ids, int64_t D, int64_t H, int64_t W, int64_t n, int64_t* counts,
                                      void* stream) {
  MSAM2_REQUIRE(labels && ids && counts, "label_mesh_count: null labels / ids / counts");
  LABEL_REQUIRE_OBJECTS("label_mesh_count", n);
  LABEL_REQUIRE_SIZES("label_mesh_count", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(((uintptr_t)counts & 7) == 0, "label_mesh_count: counts must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  MeshCountArgs a;
  a.labels = labels, a.ids = ids, a.n = (int)n, a.D = (int)D, a.H = (int)H, a.W = (int)W;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  fill_on(s, counts, n * 2, (int64_t)0);                    // (common.h: why a kernel)
  const int64_t chunks = (D + 1) * (H + 1) * ((W + MESH_CHUNK) / MESH_CHUNK), groups = (chunks + MESH_THREADS - 1) / MESH_THREADS;
  hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)std::min<int64_t>(groups, MESH_COUNT_GRID_CAP)), dim3(MESH_THREADS), 0, s, a);
  return msam2_check_launch("label_mesh_count");
}

// box: HOST int32 (z0, z1, y0, y1, x0, x1), inclusive.  What msam2_label_mesh needs for that organ alone: with L = (bd + 1)(bh + 1)(bw + 1)
// lattice points, L + 16 L / 64 + 8 L / 16384 bytes (each table rounded to 16), and 48 L more when relax > 0.  0 for a box or relax the
// entry refuses.
extern "C" size_t msam2_label_mesh_workspace_bytes(const int32_t* box, int relax) {
  if (!box || relax < 0 || relax > MESH_MAX_RELAX || !mesh_box_upright(box) || mesh_box_lattice(box) > MESH_MAX_LATTICE) return 0;
  return (size_t)mesh_tables(mesh_box_lattice(box), relax > 0).bytes;
}

// HOST arrays: ids uint8 [k], boxes int32 [k, 6], v_off / v_cap / q_off / q_cap int64 [k] (first row and rows of organ j in vertices float32
// [*, 3] and quads int32 [*, 4]); spacing, origin: 3 float64 (z, y, x).  counts int32 [k, 2] (device) = the true (vertices, quads).
extern "C" int msam2_label_mesh(const uint8_t* labels, int64_t D, int64_t H, int64_t W, const uint8_t* ids, const int32_t* boxes,
                                const int64_t* v_off, const int64_t* v_cap, const int64_t* q_off, const int64_t* q_cap, int64_t k, int placement,
                                int relax, const double* spacing, const double* origin, float* vertices, int32_t* quads, int32_t* counts,
                                void* workspace, size_t workspace_bytes, void* stream) {
  MSAM2_REQUIRE(labels && ids && boxes && v_off && v_cap && q_off && q_cap && spacing && origin && vertices && quads && counts && workspace,
                "label_mesh: null labels / ids / boxes / offsets / capacities / spacing / origin / vertices / quads / counts / workspace");
  LABEL_REQUIRE_OBJECTS("label_mesh", k);
  LABEL_REQUIRE_SIZES("label_mesh", D, H, W, 1, LABEL_MAX_VOXELS, LABEL_AT_MOST_2G_VOXELS);
  MSAM2_REQUIRE(placement == MESH_CORNER || placement == MESH_NETS, "label_mesh: placement %d (0: corner, 1: nets)", placement);
  MSAM2_REQUIRE(relax >= 0 && relax <= MESH_MAX_RELAX, "label_mesh: relax = %d sweeps (0 .. %d)", relax, MESH_MAX_RELAX);
  LABEL_REQUIRE_SPACING("label_mesh", spacing[0], spacing[1], spacing[2]);
  MSAM2_REQUIRE(mesh_finite(origin[0]) && mesh_finite(origin[1]) && mesh_finite(origin[2]), "label_mesh: origin (%g, %g, %g) must be finite",
                origin[0], origin[1], origin[2]);
  size_t bytes[LABEL_MAX_OBJ];
  for (int j = 0; j < (int)k; ++j) {                        // ids: HOST bytes, like the boxes
    LABEL_REQUIRE_DISTINCT_ID("label_mesh", "ids", ids, j);
    LABEL_REQUIRE_BOX("label_mesh", j, boxes + 6 * j, D, H, W);
    MSAM2_REQUIRE(mesh_box_lattice(boxes + 6 * j) <= MESH_MAX_LATTICE, "label_mesh: box %d has %lld lattice points (at most 2^29)", j,
                  (long long)mesh_box_lattice(boxes + 6 * j));
    MSAM2_REQUIRE(v_off[j] >= 0 && v_cap[j] >= 0 && q_off[j] >= 0 && q_cap[j] >= 0,
                  "label_mesh: organ %d: negative offset or capacity (vertices %lld + %lld, quads %lld + %lld)", j, (long long)v_off[j],
                  (long long)v_cap[j], (long long)q_off[j], (long long)q_cap[j]);
    bytes[j] = (size_t)mesh_tables(mesh_box_lattice(boxes + 6 * j), relax > 0).bytes;
  }
  const size_t need = label_tables_bytes(bytes, k, false);
  MSAM2_REQUIRE(workspace_bytes >= need, "label_mesh: workspace too small (%zu of %zu bytes)", workspace_bytes, need);
  MSAM2_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)vertices & 3) == 0 && ((uintptr_t)quads & 3) == 0 && ((uintptr_t)counts & 3) == 0,
                "label_mesh: the workspace must be 16-byte aligned, vertices, quads and counts 4-byte");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const MeshFrame f = {spacing[0], spacing[1], spacing[2], origin[0], origin[1], origin[2]};
  const dim3 blk(MESH_THREADS);
  for (int j = 0; j < (int)k;) {
    MeshJobs jobs = {};
    jobs.H = (int)H, jobs.W = (int)W;
    int words = 0, tiles = 0;
    j = label_next_group(bytes, (int)k, j, workspace_bytes, [&](int m, size_t at) {
      MeshOrgan& o = jobs.o[jobs.n++];
      static_cast<LabelBox&>(o) = label_box(boxes + 6 * m);
      o.value = ids[m], o.j = m;
      o.L = (int)mesh_box_lattice(boxes + 6 * m);
      o.words = (o.L + 63) / 64, o.tiles = (o.words + MESH_TILE_WORDS - 1) / MESH_TILE_WORDS;
      o.v_cap = (int)std::min<int64_t>(v_cap[m], INT32_MAX), o.q_cap = (int)std::min<int64_t>(q_cap[m], INT32_MAX);
      o.ws = (long long)at, o.v_off = v_off[m], o.q_off = q_off[m];
      words = std::max(words, o.words), tiles = std::max(tiles, o.tiles);
    });
    const dim3 lattice(std::min(cdiv(words, MESH_WAVES), MESH_GRID_CAP), jobs.n);
    hipLaunchKernelGGL(mesh_flag_kernel, lattice, blk, 0, s, labels, jobs, ws);
    hipLaunchKernelGGL(mesh_scan_tiles_kernel, dim3(tiles, jobs.n), blk, 0, s, jobs, ws);
    hipLaunchKernelGGL(mesh_scan_sums_kernel, dim3(1, jobs.n), blk, 0, s, jobs, ws, counts);
    hipLaunchKernelGGL(mesh_emit_kernel, lattice, blk, 0, s, jobs, ws, placement, relax, f, vertices, quads);
    for (int sweep = 0; sweep < relax; ++sweep) hipLaunchKernelGGL(mesh_relax_kernel, lattice, blk, 0, s, jobs, ws, sweep & 1);
    if (relax > 0) hipLaunchKernelGGL(mesh_store_kernel, lattice, blk, 0, s, jobs, ws, relax & 1, f, vertices);
  }
  return msam2_check_launch("label_mesh");
}
