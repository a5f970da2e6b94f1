// Connected components of label maps and the filters on top of them, 2D and 3D, for gfx950:
//
//   advchain_components      <- common.postprocess.connected_components
//   advchain_keep_largest    <- common.postprocess.keep_largest_component
//   advchain_remove_small    <- common.postprocess.remove_small_components
//   advchain_fill_holes      <- common.postprocess.fill_holes, find_holes
//   advchain_instance_match  <- common.metrics.instance_metrics (see "instance matching" below)
//   advchain_betti           <- common.metrics.betti_numbers, betti_error (see "topology" below)
//
// Two voxels of an entry are adjacent when their offsets differ by at most 1 on every axis and on at most `connectivity` axes
// (scipy's generate_binary_structure); adjacent voxels are connected when they carry the same label and that label is
// foreground: not `background` and, with a class count K, inside [0, K).  Labels are only compared.  A label-equivalence
// union-find over `parent` (int32 per voxel: an entry-local linear index, -1 on background):
//   k_cc_tile      a workgroup stages a tile of 2048 labels in LDS (each int64 label is read once), unites connected voxels
//                  inside the tile (a run of equal labels in a row by one ballot, run with run by LDS atomic minima, the first
//                  pair of two runs that touch only) and writes the tile-local root of every voxel -- the smallest linear index of
//                  its tile-local component -- and, at that root, the voxel count of the tile-local component (0 elsewhere).
//   k_cc_seam      the voxels on the low faces of a tile re-read their label and those of their neighbours in OTHER tiles (a few
//                  per cent of the voxels) and unite across the seam in global memory: faces, and with connectivity 2 / 3 the
//                  pairs that touch only across a tile edge or corner.
//   k_cc_flatten   parent[v] becomes the root; counts the roots per chunk of 2048 voxels; a tile-local root that is not the root
//                  adds its count to the root's (one integer atomic per tile a component touches, not per voxel).
//   k_cc_scan      exclusive scan of the chunk counts per entry (two levels: no workgroup waits on another), count[n].
//   k_cc_number    root -> 1 + the number of roots in front of it in C order: components are numbered by their smallest voxel.
//   k_cc_gather    labels and sizes of the root to every voxel.
//   k_cc_winner    per (entry, class) the 64-bit maximum of (size << 32) | ~root: the largest component, ties to the earlier.
//   k_cc_keep, k_cc_small   the filtered copies of the input.
//   k_hole_enclose, k_hole_fill   fill_holes: k_cc_tile, k_cc_seam and k_cc_flatten label the background instead (HOLES), then per
//                  background component the smallest and largest code of what encloses it, then the filled copy and the counts
//                  (see "hole filling" below).
// Invariant of the union-find: parent[x] <= x in every state a thread can observe (a parent is only ever lowered, by an atomic
// minimum, to the index of a voxel of the same component), so a walk towards the root moves to a strictly smaller index each
// step and ends after fewer steps than there are voxels.  No kernel waits on a value that another workgroup writes.  Integer
// atomics only: the result is a function of the input alone, the same bits on every run.  Every word that is read was written
// by a kernel of the same call: no memset, no host read-back, capturable on one stream.
#include "common.h"

namespace advchain {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kTileX = 64;                   // a wave per tile row
constexpr int kTileY2 = 32;                  // 2D tiles: 32 x 64
constexpr int kTileZ3 = 4, kTileY3 = 8;      // 3D tiles: 4 x 8 x 64 (a z-slab of four slices); ops.COMPONENTS_TILE mirrors these
constexpr int kTileVox = 2048;               // voxels of a tile, and of a chunk of the passes that run over linear indices
constexpr int kPerThread = kTileVox / kBlock;

struct Shape {
  int D, H, W;         // D == 1 for 2D
  int TZ, TY;          // tile sizes along z and y (powers of two)
  int conn;            // 1 .. ndim
};

// What the passes unite.  kHoles: they label the background instead (advchain_fill_holes): the voxels equal to `background` are the
// ones united, K is not looked at.  They all carry one label, so the equality tests that unite runs and pairs are the same.
// kComplement: they label the complement of one class (advchain_betti: the cavities of class `background`): the voxels that differ
// from `background` are united whatever they carry, so every label is first reduced to the answer to "is it not `background`"
// (canon), and the equality tests compare those.
enum { kLabels = 0, kHoles = 1, kComplement = 2 };
template <int MODE>
__device__ __forceinline__ int64_t canon(int64_t y, int64_t background) {
  return MODE == kComplement ? (int64_t)(y != background) : y;
}
// (y: a label behind canon)
template <int MODE>
__device__ __forceinline__ bool foreground(int64_t y, int64_t background, int64_t K) {
  if (MODE == kHoles) return y == background;
  if (MODE == kComplement) return y != 0;
  return y != background && (K < 0 || (y >= 0 && y < K));
}

// ---- union-find ---------------------------------------------------------------------------------------------------------------
// parent[x] <= x always, and every parent is a voxel of the same component.  SCOPE: workgroup for a tile in LDS, agent for the
// seams in global memory (a relaxed agent-scope load is served by L2; an older value is still a valid ancestor, so staleness
// costs steps, never correctness: the atomic minimum below is what decides).
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* parent, int x) {
  int y;
  while ((y = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE)) != x) x = y;       // y < x: strictly decreasing, ends at a root
  return x;
}

// Lock-free union: lower the parent of the larger root to the smaller root.  If the larger one was no root any more, the atomic
// returns its parent `old` < a, which is still to be united with b: max(a, b) strictly decreases from one turn to the next, so
// the loop ends after fewer turns than there are voxels.  It never waits for another thread.
template <int SCOPE>
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  a = uf_find<SCOPE>(parent, a);
  b = uf_find<SCOPE>(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);      // b < a: parent[a] <= a stays true
    if (old == a) break;                                                                 // a was a root and now hangs below b
    a = uf_find<SCOPE>(parent, old);                                                     // old < a
    b = uf_find<SCOPE>(parent, b);
  }
}

// ---- tile pass ----------------------------------------------------------------------------------------------------------------
// blockIdx.x = ((n tiles_z + z tile) tiles_y + y tile) tiles_x + x tile.  The local index (lz TY + ly) 64 + lx orders the voxels
// of a tile as their linear indices do, so the smallest local index of a component is its smallest linear index in the tile.
// HOLES: `winners` and `winners2` are the hole counts and voxel counts (zeroed here), and `state` gets the empty enclosure state
// (smallest code INT_MAX, largest code -1) at every tile-local root: the root of a component is the tile-local root of its tile.
template <int MODE>
__global__ void __launch_bounds__(kBlock)
k_cc_tile(const int64_t* __restrict__ labels, int* __restrict__ parent, int* __restrict__ sizes, u64* __restrict__ winners,
          u64* __restrict__ winners2, int* __restrict__ state, int64_t NK, int64_t background, int64_t K, Shape s, int tiles_z,
          int tiles_y, int tiles_x) {
  __shared__ int64_t lab[kTileVox];
  __shared__ int par[kTileVox];
  __shared__ int cnt[kTileVox];
  constexpr bool HOLES = MODE == kHoles;
  if (winners) {                                           // (keep_largest: the maxima of k_cc_winner start at 0)
    const int64_t threads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < NK; i += threads) {
      winners[i] = 0ull;
      if (HOLES) winners2[i] = 0ull;
    }
  }
  int64_t b = blockIdx.x;
  const int bx = (int)(b % tiles_x); b /= tiles_x;
  const int by = (int)(b % tiles_y); b /= tiles_y;
  const int bz = (int)(b % tiles_z);
  const int64_t n = b / tiles_z, V = (int64_t)s.D * s.H * s.W;
  const int z0 = bz * s.TZ, y0 = by * s.TY, x0 = bx * kTileX;
  const int sy = kTileX, sz = kTileX * s.TY;

#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int i = j * kBlock + threadIdx.x;
    const int lx = i & (kTileX - 1), ly = (i / kTileX) & (s.TY - 1), lz = i / sz;
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    const bool in = z < s.D && y < s.H && x < s.W;
    // (outside the image: a label that is in no component, whichever label the passes unite)
    const int64_t v = in ? canon<MODE>(labels[n * V + ((int64_t)z * s.H + y) * s.W + x], background)
                         : (MODE == kHoles ? ~background : MODE == kComplement ? 0 : background);
    lab[i] = v;
    // a wave holds one tile row: a voxel starts below the first voxel of its run of equal labels in the row (lane lx), which
    // is the union of the run without an atomic
    const int64_t left = __shfl_up(v, 1, 64);                                            // (every lane takes part: not behind ||)
    const u64 heads = __ballot(lx == 0 || left != v);
    const int start = 63 - __clzll(heads & ((2ull << lx) - 1ull));                       // (bit 0 is set: lane 0 is a head)
    par[i] = (in && foreground<MODE>(v, background, K)) ? i - lx + start : -1;
    cnt[i] = 0;
  }
  __syncthreads();

  // unite with the connected neighbours in front (in C order) that lie in this tile; the others are the seam pass's.  Offset
  // q = (dz + 1) 9 + (dy + 1) 3 + dx + 1: the 12 offsets below (0, 0, -1) (q = 12: the runs above) are the ones in front in
  // another row; 2D starts at dz = 0.  A pair whose left neighbours are the same pair of runs is left to them: the first pair
  // of two runs that touch unites them.
#pragma unroll 1
  for (int j = 0; j < kPerThread; ++j) {
    const int i = j * kBlock + threadIdx.x;
    if (par[i] < 0) continue;                              // (foreground or not never changes)
    const int lx = i & (kTileX - 1), ly = (i / kTileX) & (s.TY - 1), lz = i / sz;
    const int64_t mine = lab[i];
#pragma unroll 1
    for (int q = s.TZ > 1 ? 0 : 9; q < 12; ++q) {
      const int dz = q / 9 - 1, dy = (q / 3) % 3 - 1, dx = q % 3 - 1;
      if ((dz != 0) + (dy != 0) + (dx != 0) > s.conn) continue;
      if (lz + dz < 0 || ly + dy < 0 || ly + dy >= s.TY || lx + dx < 0 || lx + dx >= kTileX) continue;
      const int o = i + dz * sz + dy * sy + dx;
      if (lab[o] != mine) continue;                                                       // (equal to a foreground label: foreground)
      if (lx > 0 && lx + dx > 0 && lab[i - 1] == mine && lab[o - 1] == mine) continue;
      uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, o);
    }
  }
  __syncthreads();

  int root[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int i = j * kBlock + threadIdx.x;
    root[j] = par[i] < 0 ? -1 : uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i);
    if (root[j] >= 0) atomicAdd(&cnt[root[j]], 1);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int i = j * kBlock + threadIdx.x;
    const int lx = i & (kTileX - 1), ly = (i / kTileX) & (s.TY - 1), lz = i / sz;
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    if (z >= s.D || y >= s.H || x >= s.W) continue;
    const int64_t at = n * V + ((int64_t)z * s.H + y) * s.W + x;
    int r = -1;
    if (root[j] >= 0) {
      const int rx = root[j] & (kTileX - 1), ry = (root[j] / kTileX) & (s.TY - 1), rz = root[j] / sz;
      r = (int)(((int64_t)(z0 + rz) * s.H + y0 + ry) * s.W + x0 + rx);                   // (inside the image: it is foreground)
    }
    parent[at] = r;
    if (sizes) sizes[at] = cnt[i];
    if (HOLES && root[j] == i) {
      state[2 * at] = 0x7fffffff;
      state[2 * at + 1] = -1;
    }
  }
}

// ---- the passes over linear indices: blockIdx.x = n chunks + chunk, a chunk is 2048 consecutive voxels of an entry ------------
struct Chunked {
  int64_t n, base;     // entry, first voxel of the chunk
};
__device__ __forceinline__ Chunked chunk_of(int64_t chunks) {
  Chunked c;
  c.n = blockIdx.x / chunks;
  c.base = (blockIdx.x - c.n * chunks) * kTileVox;
  return c;
}

__device__ __forceinline__ bool low_face(int z, int y, int x, const Shape& s) {
  return (x > 0 && (x & (kTileX - 1)) == 0) || (y > 0 && (y & (s.TY - 1)) == 0) || (z > 0 && (z & (s.TZ - 1)) == 0);
}

// Every connected pair whose voxels lie in different tiles has a voxel on a low face of its tile (along an axis on which the
// tiles differ, the voxel with the larger coordinate).  That voxel unites the pair; when both are on a low face, the later one.
template <int MODE>
__global__ void __launch_bounds__(kBlock)
k_cc_seam(const int64_t* __restrict__ labels, int* parent, int64_t background, int64_t K, Shape s, int64_t V, int64_t chunks) {
  const Chunked c = chunk_of(chunks);
  const int64_t* L = labels + c.n * V;
  int* P = parent + c.n * V;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    if (v >= V) break;
    const int x = (int)(v % s.W), y = (int)((v / s.W) % s.H), z = (int)(v / ((int64_t)s.W * s.H));
    if (!low_face(z, y, x, s)) continue;
    const int64_t mine = canon<MODE>(L[v], background);
    if (!foreground<MODE>(mine, background, K)) continue;
#pragma unroll 1
    for (int q = s.TZ > 1 ? 0 : 9; q < (s.TZ > 1 ? 27 : 18); ++q) {                     // offsets as in k_cc_tile, all around
      const int dz = q / 9 - 1, dy = (q / 3) % 3 - 1, dx = q % 3 - 1;
      if (q == 13 || (dz != 0) + (dy != 0) + (dx != 0) > s.conn) continue;
      const int z1 = z + dz, y1 = y + dy, x1 = x + dx;
      if (z1 < 0 || z1 >= s.D || y1 < 0 || y1 >= s.H || x1 < 0 || x1 >= s.W) continue;
      if ((z1 & -s.TZ) == (z & -s.TZ) && (y1 & -s.TY) == (y & -s.TY) && (x1 & -kTileX) == (x & -kTileX)) continue;
      const int64_t u = ((int64_t)z1 * s.H + y1) * s.W + x1;
      if (u > v && low_face(z1, y1, x1, s)) continue;                                   // (that voxel takes the pair)
      if (canon<MODE>(L[u], background) != mine) continue;
      // the left neighbours are the same pair of tiles and of runs, on the same faces: the pair is theirs
      if ((x & (kTileX - 1)) != 0 && (x1 & (kTileX - 1)) != 0 && canon<MODE>(L[v - 1], background) == mine &&
          canon<MODE>(L[u - 1], background) == mine) continue;
      uf_unite<__HIP_MEMORY_SCOPE_AGENT>(P, (int)v, (int)u);
    }
  }
}

// parent[v] <- root.  Other workgroups shorten their own chains meanwhile: whatever value a walk reads is an ancestor in the
// final forest (the unions are over), parent[x] <= x still holds.  counts[chunk] = roots in the chunk.  SIZES: sizes[v] is the
// voxel count of v's tile-local component at a tile-local root and 0 elsewhere; only roots are added to, and only the words of
// voxels that are no root are read, so the adds of other workgroups cannot be seen half-way.
template <bool SIZES>
__global__ void __launch_bounds__(kBlock)
k_cc_flatten(int* parent, int* sizes, int* __restrict__ counts, int64_t V, int64_t chunks) {
  __shared__ int roots;
  const Chunked c = chunk_of(chunks);
  int* P = parent + c.n * V;
  int* S = sizes + c.n * V;
  if (threadIdx.x == 0) roots = 0;
  __syncthreads();
  int mine = 0;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    if (v >= V) break;
    const int p = P[v];
    if (p < 0) continue;
    if (p == (int)v) { ++mine; continue; }
    const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(P, p);
    if (r != p) P[v] = r;
    if (SIZES) {
      const int t = S[v];
      if (t) atomicAdd(S + r, t);
    }
  }
  if (mine) atomicAdd(&roots, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = roots;
}

// One workgroup per entry: counts[n][c] <- the sum of the counts in front of chunk c, count[n] <- their total.
__global__ void __launch_bounds__(kBlock)
k_cc_scan(int* __restrict__ counts, int64_t* __restrict__ count, int64_t chunks) {
  __shared__ int scan[2][kBlock];
  const int t = threadIdx.x;
  int* C = counts + (int64_t)blockIdx.x * chunks;
  int carry = 0;
  for (int64_t c0 = 0; c0 < chunks; c0 += kBlock) {
    const int x = c0 + t < chunks ? C[c0 + t] : 0;
    scan[0][t] = x;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < kBlock; o <<= 1) {
      scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0);
      cur ^= 1;
      __syncthreads();
    }
    if (c0 + t < chunks) C[c0 + t] = carry + scan[cur][t] - x;
    carry += scan[cur][kBlock - 1];
    __syncthreads();
  }
  if (t == 0) count[blockIdx.x] = carry;
}

// out[root] <- 1 + the number of roots of the entry in front of it
__global__ void __launch_bounds__(kBlock)
k_cc_number(const int* __restrict__ parent, const int* __restrict__ counts, int* __restrict__ out, int64_t V, int64_t chunks) {
  __shared__ int waves[kBlock / 64];
  const Chunked c = chunk_of(chunks);
  const int* P = parent + c.n * V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before = counts[blockIdx.x];
  for (int j = 0; j < kPerThread; ++j) {                                                  // (uniform: no early exit, barriers inside)
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    const bool is_root = v < V && P[v] == (int)v;
    const u64 m = __ballot(is_root);
    if (lane == 0) waves[wave] = __popcll(m);
    __syncthreads();
    int ahead = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
      ahead += w < wave ? waves[w] : 0;
      all += waves[w];
    }
    if (is_root) out[c.n * V + v] = before + ahead + __popcll(m & ((1ull << lane) - 1ull)) + 1;
    before += all;
    __syncthreads();
  }
}

// labels: the number of the root, 0 on background (the roots hold theirs already; only they are read).  sizes_out: the root's.
__global__ void __launch_bounds__(kBlock)
k_cc_gather(const int* __restrict__ parent, const int* __restrict__ sizes, int* out, int* __restrict__ sizes_out, int64_t V,
            int64_t chunks) {
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    if (v >= V) break;
    const int p = parent[e + v];
    if (p != (int)v) out[e + v] = p < 0 ? 0 : out[e + p];
    if (sizes_out) sizes_out[e + v] = p < 0 ? 0 : sizes[e + p];
  }
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// A root re-reads its label (the class index: in [0, K) since the voxel is foreground) and offers (size << 32) | ~root; the
// roots of one class in a wave are reduced first, one turn per class among them, so a map of specks does not queue one atomic
// per speck on one word.
__global__ void __launch_bounds__(kBlock)
k_cc_winner(const int64_t* __restrict__ labels, const int* __restrict__ parent, const int* __restrict__ sizes,
            u64* __restrict__ winners, int64_t K, int64_t V, int64_t chunks) {
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    const bool is_root = v < V && parent[e + v] == (int)v;
    const int k = is_root ? (int)labels[e + v] : -1;
    const u64 key = is_root ? ((u64)(u32)sizes[e + v] << 32) | (u64)(0xffffffffu - (u32)v) : 0ull;
    u64 todo = __ballot(is_root);
    while (todo) {                                                                       // one turn per class: todo loses bits
      const int k1 = __shfl(k, __builtin_ctzll(todo), 64);
      const bool same = k == k1;
      const u64 best = wave_max_u64(same ? key : 0ull);
      if (lane == 0) atomicMax(winners + c.n * K + k1, best);
      todo &= ~__ballot(same);
    }
  }
}

__global__ void __launch_bounds__(kBlock)
k_cc_keep(const int64_t* __restrict__ labels, const int* __restrict__ parent, const u64* __restrict__ winners,
          int64_t* __restrict__ out, int64_t background, int64_t K, int64_t V, int64_t chunks) {
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    if (v >= V) break;
    const int64_t y = labels[e + v];
    const int p = parent[e + v];
    bool keep = true;
    if (p >= 0) keep = 0xffffffffu - (u32)winners[c.n * K + y] == (u32)p;                 // (p >= 0: y is a class index)
    out[e + v] = keep ? y : background;
  }
}

__global__ void __launch_bounds__(kBlock)
k_cc_small(const int64_t* __restrict__ labels, const int* __restrict__ parent, const int* __restrict__ sizes,
           int64_t* __restrict__ out, int64_t background, int64_t min_size, int64_t V, int64_t chunks) {
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    if (v >= V) break;
    const int p = parent[e + v];
    const bool drop = p >= 0 && (int64_t)sizes[e + p] < min_size;
    out[e + v] = drop ? background : labels[e + v];
  }
}

// ---- hole filling -------------------------------------------------------------------------------------------------------------
// The passes above with HOLES label the background; a hole is a background component that does not touch the border of its entry
// and whose neighbours that are not background all carry one class k in [0, K).  Per root two words at state[2 root]: the
// smallest and the largest code seen, kept with atomic minimum and maximum.  The code of a class label is the label; a voxel on a
// face of the entry and a neighbouring label outside [0, K) give kPoison (above every class index: K <= 65535).  A component is
// a hole iff both words are equal and in [0, K).
constexpr int kPoison = 0x10000;

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// Every background voxel (parent >= 0: its root, after k_cc_flatten) looks all around it.  A neighbour with a parent is
// background and needs no label read; the voxels inside the outside component read 4-byte parents only.  The contributions of a
// wave are reduced per distinct root among its lanes first (the pattern of k_cc_winner): on a real map the outside is one
// component with hundreds of thousands of contributing voxels.  A lane drops out before that when a relaxed load shows its root
// as decided "no hole" (poisoned, or two different codes): every later contribution lowers the minimum or raises the maximum,
// which leaves that decision as it is.  The raw words therefore may differ from run to run; whether they are equal and in
// [0, K), and their value if so, do not, and k_hole_fill looks at nothing else.
// One voxel per thread, blockIdx.x = n rows + row of kBlock voxels, and the neighbourhood (ND axes, CONN) unrolled at compile
// time: a voxel's work is a chain of dependent accesses (its parent, its neighbours' parents, their labels, the root's state).
// Eight voxels per thread in turn, each neighbour in turn, left one wave per SIMD waiting on every access; now the parents of
// all neighbours are one batch of loads and the labels of those that are not background a second one (a background neighbour
// re-reads the voxel's own label instead, the line is there: no branch between the loads).
template <int ND, int CONN>
__global__ void __launch_bounds__(kBlock)
k_hole_enclose(const int64_t* __restrict__ labels, const int* __restrict__ parent, int* state, int64_t K, Shape s, int64_t V,
               int64_t rows) {
  constexpr int kFirst = ND == 3 ? 0 : 9, kLast = ND == 3 ? 27 : 18;                      // offsets as in k_cc_seam
  const int64_t n = blockIdx.x / rows;
  const int64_t* L = labels + n * V;
  const int* P = parent + n * V;
  int* S = state + 2 * n * V;
  const int lane = threadIdx.x & 63;
  const int64_t HW = (int64_t)s.H * s.W;
  {
    const int64_t v = (blockIdx.x - n * rows) * kBlock + threadIdx.x;                     // (no early exit: the ballots need every lane)
    const int r = v < V ? P[v] : -1;
    int lo = 0x7fffffff, hi = -1;
    if (r >= 0) {
      const u32 row = (u32)v / (u32)s.W;                                                  // (v < V < 2^31: 32-bit divisions)
      const int x = (int)((u32)v - row * (u32)s.W), y = (int)(row % (u32)s.H), z = (int)(row / (u32)s.H);
      if (x == 0 || x == s.W - 1 || y == 0 || y == s.H - 1 || (ND == 3 && (z == 0 || z == s.D - 1))) {
        lo = hi = kPoison;
      } else {                                                                            // (every neighbour is inside the entry)
        int pu[27];
        bool any = false;
#pragma unroll
        for (int q = kFirst; q < kLast; ++q) {
          const int dz = q / 9 - 1, dy = (q / 3) % 3 - 1, dx = q % 3 - 1;
          if (q == 13 || (dz != 0) + (dy != 0) + (dx != 0) > CONN) continue;
          pu[q] = P[v + dz * HW + dy * s.W + dx];
          any |= pu[q] < 0;
        }
        if (any) {
          int64_t t[27];
#pragma unroll
          for (int q = kFirst; q < kLast; ++q) {
            const int dz = q / 9 - 1, dy = (q / 3) % 3 - 1, dx = q % 3 - 1;
            if (q == 13 || (dz != 0) + (dy != 0) + (dx != 0) > CONN) continue;
            t[q] = L[pu[q] < 0 ? v + dz * HW + dy * s.W + dx : v];
          }
#pragma unroll
          for (int q = kFirst; q < kLast; ++q) {
            const int dz = q / 9 - 1, dy = (q / 3) % 3 - 1, dx = q % 3 - 1;
            if (q == 13 || (dz != 0) + (dy != 0) + (dx != 0) > CONN) continue;
            const int code = t[q] >= 0 && t[q] < K ? (int)t[q] : kPoison;
            lo = min(lo, pu[q] < 0 ? code : 0x7fffffff);
            hi = max(hi, pu[q] < 0 ? code : -1);
          }
        }
      }
    }
    if (hi >= 0) {
      // every lane looks at its root's state first, all lanes at once (inside the turns below the loads would follow one another):
      // it has nothing to offer when the root is decided, or when its codes lie between the two words -- they only move outwards
      const int seen_lo = __hip_atomic_load(S + 2 * (int64_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int seen_hi = __hip_atomic_load(S + 2 * (int64_t)r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seen_hi >= kPoison || seen_lo < seen_hi || (lo >= seen_lo && hi <= seen_hi)) hi = -1;
    }
    u64 todo = __ballot(hi >= 0);
    while (todo) {                                                                        // one turn per root: todo loses bits
      const int r1 = __shfl(r, __builtin_ctzll(todo), 64);
      const bool same = hi >= 0 && r == r1;
      const u64 group = __ballot(same);
      int mn = lo, mx = hi;
      if (group & (group - 1ull)) {                                                       // (uniform; a single lane offers its own)
        mn = wave_min_int(same ? lo : 0x7fffffff);
        mx = wave_max_int(same ? hi : -1);
      }
      if (lane == __builtin_ctzll(todo)) {
        atomicMin(S + 2 * (int64_t)r1, mn);
        atomicMax(S + 2 * (int64_t)r1 + 1, mx);
      }
      todo &= ~group;
    }
  }
}

// out: the filled copy; fill: the class a voxel is filled with, -1 elsewhere.  A root that is filled adds 1 and its size to
// count[n][k] and voxels[n][k] (zeroed by k_cc_tile): the roots of one class in a wave together, and those of the first class that
// turns up in the workgroup (on most maps the only one) summed in LDS and added once per workgroup -- a map of specks has tens of
// thousands of holes per entry, all of one class, and their adds would queue on one word.
__global__ void __launch_bounds__(kBlock)
k_hole_fill(const int64_t* __restrict__ labels, const int* __restrict__ parent, const int* __restrict__ sizes,
            const int* __restrict__ state, int64_t* __restrict__ out, int64_t* __restrict__ fill, u64* __restrict__ count,
            u64* __restrict__ voxels, int64_t K, int64_t max_size, int64_t V, int64_t chunks) {
  __shared__ int first_k;
  __shared__ u64 first_count, first_voxels;
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) {
    first_k = -1;
    first_count = first_voxels = 0ull;
  }
  __syncthreads();
  for (int j = 0; j < kPerThread; ++j) {
    if (c.base + j * kBlock >= V) break;                                                  // (uniform)
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    const int p = v < V ? parent[e + v] : -1;
    int k = -1, size = 0;
    if (p >= 0) {
      const int lo = state[2 * (e + p)], hi = state[2 * (e + p) + 1];
      size = sizes[e + p];
      if (lo == hi && lo >= 0 && lo < K && (max_size < 0 || size <= max_size)) k = lo;
    }
    if (v < V) {
      if (out) out[e + v] = k >= 0 ? (int64_t)k : labels[e + v];
      if (fill) fill[e + v] = k;
    }
    if (!count) continue;                                                                 // (uniform)
    const bool root = k >= 0 && p == (int)v;
    u64 todo = __ballot(root);
    while (todo) {                                                                        // one turn per class
      const int k1 = __shfl(k, __builtin_ctzll(todo), 64);
      const u64 same = __ballot(root && k == k1);
      u64 total = root && k == k1 ? (u64)size : 0ull;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
      if (lane == 0) {
        const int held = atomicCAS(&first_k, -1, k1);
        if (held == -1 || held == k1) {
          atomicAdd(&first_count, (u64)__popcll(same));
          atomicAdd(&first_voxels, total);
        } else {
          atomicAdd(count + c.n * K + k1, (u64)__popcll(same));
          atomicAdd(voxels + c.n * K + k1, total);
        }
      }
      todo &= ~same;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && first_k >= 0) {
    atomicAdd(count + c.n * K + first_k, first_count);
    atomicAdd(voxels + c.n * K + first_k, first_voxels);
  }
}

// ---- instance matching --------------------------------------------------------------------------------------------------------
// advchain_instance_match: k_cc_tile, k_cc_seam and k_cc_flatten<true> label pred and target, each into its own half of the
// workspace: every voxel then holds the root of its component and every root its voxel count.  On top of them:
//   k_inst_clear    the pair table (keys empty, counts 0) and the integer outputs (0).
//   k_inst_pair     every voxel with a root in both maps and the same label in both adds 1 to the key (root in pred << 32) | root
//                   in target of its entry's table; the roots of a map are counted per class and get a zero state word.
//   k_inst_match    every used slot: I, |a|, |b| and the class give the overlap marks, the match rule and iou_fixed.
//   k_inst_finish   the five quotients per (entry, class).
//   k_inst_status   the status maps, from the state word of the root.
// The table of an entry is open addressing with linear probing over `slots` = max(2 V, 64) slots: an entry has at most V
// distinct pairs (a voxel adds to one key), so at least half of the slots stay empty, a probe always ends, and nothing
// overflows.  A key is claimed by a 64-bit compare-and-swap on the empty word; a thread whose swap fails re-reads what the slot
// holds now and adds there or moves on: nobody waits.  Which slot a key lands in depends on the order of arrival; the count of a
// key, and everything k_inst_match derives from the set of (key, count), do not.
constexpr u64 kEmptyKey = ~0ull;                 // (a root is below 2^31: no key has all bits set)
constexpr int kOverlapBit = 1, kMatchBit = 2;    // the state word of a root

__device__ __forceinline__ u64 inst_hash(u64 key) {
  key ^= key >> 33;                              // (the finaliser of MurmurHash3: neighbouring roots spread over the table)
  key *= 0xff51afd7ed558ccdull;
  key ^= key >> 33;
  key *= 0xc4ceb9fe1a85ec53ull;
  key ^= key >> 33;
  return key;
}
__device__ __forceinline__ u32 inst_slot(u64 hash, u32 slots) {
  return (u32)(((hash >> 32) * (u64)slots) >> 32);                                        // < slots
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// dst[k * stride] += the number of lanes with `is` set and class k, one atomic per class among the lanes of the wave (every
// lane of the wave calls it)
__device__ __forceinline__ void wave_count_by_class(bool is, int k, u64* dst, int stride, int lane) {
  u64 todo = __ballot(is);
  while (todo) {                                                                          // one turn per class: todo loses bits
    const int k1 = __shfl(k, __builtin_ctzll(todo), 64);
    const u64 same = __ballot(is && k == k1);
    if (lane == 0) atomicAdd(dst + (int64_t)k1 * stride, (u64)__popcll(same));
    todo &= ~same;
  }
}

__global__ void __launch_bounds__(kBlock)
k_inst_clear(u64* __restrict__ keys, u32* __restrict__ counts, int64_t table, u64* __restrict__ components,
             u64* __restrict__ matched, u64* __restrict__ overlapping, u64* __restrict__ iou_fixed, int64_t NK) {
  const int64_t threads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < table; i += threads) {
    keys[i] = kEmptyKey;
    counts[i] = 0u;
  }
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < NK; i += threads) {
    components[2 * i] = components[2 * i + 1] = 0ull;
    overlapping[2 * i] = overlapping[2 * i + 1] = 0ull;
    matched[i] = 0ull;
    iou_fixed[i] = 0ull;
  }
}

// key += length in the table of an entry.  Ends: the table always has an empty slot.  A swap that fails has the slot's new key
// in hand: ours (another thread claimed it for the same pair) or another's, and then the probe moves on.
__device__ __forceinline__ void inst_add(u64* table, u32* count, u32 slots, u64 key, u32 length) {
  u32 at = inst_slot(inst_hash(key), slots);
  for (;;) {
    u64 held = __hip_atomic_load(table + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (held == kEmptyKey) held = atomicCAS(table + at, kEmptyKey, key);                  // (the old value: empty, ours or another's)
    if (held == kEmptyKey || held == key) {
      atomicAdd(count + at, length);
      return;
    }
    at = at + 1u == slots ? 0u : at + 1u;
  }
}

// The same in a table of kStageSlots slots in LDS, at most kStageProbes probes: false when they all hold other keys.
constexpr int kStageSlots = 128, kStageProbes = 8;
__device__ __forceinline__ bool inst_stage(u64* table, u32* count, u64 key, u32 length) {
  u32 at = (u32)inst_hash(key) & (kStageSlots - 1);
  for (int probe = 0; probe < kStageProbes; ++probe) {
    u64 held = __hip_atomic_load(table + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (held == kEmptyKey) held = atomicCAS(table + at, kEmptyKey, key);
    if (held == kEmptyKey || held == key) {
      atomicAdd(count + at, length);
      return true;
    }
    at = (at + 1u) & (kStageSlots - 1);
  }
  return false;
}

// Chunked as k_cc_flatten.  A wave holds 64 consecutive voxels: the lanes in a row that carry the same key are a run (found by
// one ballot, as the runs of equal labels in k_cc_tile), and the first lane of a run adds its length -- to a small table of the
// workgroup in LDS first, whose used slots go to the entry's table at the end: the 2048 voxels of a chunk seldom hold more than
// a few pairs, and the voxels that two large components share would otherwise queue an add per run on one word in global
// memory (4 x 128 x 128 x 64 blobs: 192 us for this pass without the stage, 25 us with it).  A run that finds the stage full
// goes to the entry's table itself: the stage changes how many adds a count is made of, never the count.
__global__ void __launch_bounds__(kBlock)
k_inst_pair(const int64_t* __restrict__ pred, const int64_t* __restrict__ target, const int* __restrict__ parent_p,
            const int* __restrict__ parent_t, int* __restrict__ state_p, int* __restrict__ state_t, u64* keys, u32* counts,
            u64* components, int64_t K, int64_t V, int64_t chunks, u32 slots) {
  __shared__ u64 stage_key[kStageSlots];
  __shared__ u32 stage_count[kStageSlots];
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  u64* table = keys + c.n * (int64_t)slots;
  u32* count = counts + c.n * (int64_t)slots;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < kStageSlots) {
    stage_key[threadIdx.x] = kEmptyKey;
    stage_count[threadIdx.x] = 0u;
  }
  __syncthreads();
  for (int j = 0; j < kPerThread; ++j) {
    if (c.base + j * kBlock >= V) break;                                                  // (uniform)
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    const int rp = v < V ? parent_p[e + v] : -1, rt = v < V ? parent_t[e + v] : -1;
    const bool root_p = rp >= 0 && rp == (int)v, root_t = rt >= 0 && rt == (int)v;
    // (a voxel with a root carries a class index: in [0, K))
    const int kp = rp >= 0 ? (int)pred[e + v] : -1, kt = rt >= 0 ? (int)target[e + v] : -2;
    if (root_p) state_p[e + v] = 0;
    if (root_t) state_t[e + v] = 0;
    wave_count_by_class(root_p, kp, components + 2 * c.n * K, 2, lane);
    wave_count_by_class(root_t, kt, components + 2 * c.n * K + 1, 2, lane);
    const u64 key = kp == kt ? ((u64)(u32)rp << 32) | (u64)(u32)rt : kEmptyKey;
    const u64 left = __shfl_up(key, 1, 64);                                               // (every lane takes part)
    const u64 heads = __ballot(lane == 0 || left != key);
    if (key != kEmptyKey && ((heads >> lane) & 1ull)) {
      const u64 behind = lane == 63 ? 0ull : heads >> (lane + 1);
      const u32 length = behind ? (u32)__builtin_ctzll(behind) + 1u : (u32)(64 - lane);
      if (!inst_stage(stage_key, stage_count, key, length)) inst_add(table, count, slots, key, length);
    }
  }
  __syncthreads();
  if (threadIdx.x < kStageSlots && stage_key[threadIdx.x] != kEmptyKey)
    inst_add(table, count, slots, stage_key[threadIdx.x], stage_count[threadIdx.x]);
}

// One slot per thread and turn.  The first marker of a root (the old value of the atomic OR says so) counts it as overlapping; a
// root is matched at most once (iou_threshold >= 0.5), so the match counts need no such test.  The adds of a wave are summed per
// class first.
__global__ void __launch_bounds__(kBlock)
k_inst_match(const int64_t* __restrict__ pred, const int* __restrict__ sizes_p, const int* __restrict__ sizes_t, int* state_p,
             int* state_t, const u64* __restrict__ keys, const u32* __restrict__ counts, u64* matched, u64* overlapping,
             u64* iou_fixed, double threshold, int64_t K, int64_t V, u32 slots, int64_t table) {
  const int lane = threadIdx.x & 63;
  const int64_t threads = (int64_t)gridDim.x * kBlock;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock; i0 < table; i0 += threads) {           // (uniform: ballots inside)
    const int64_t i = i0 + threadIdx.x;
    const u64 key = i < table ? keys[i] : kEmptyKey;
    const bool used = key != kEmptyKey;
    int64_t nk = -1;
    bool first_p = false, first_t = false, match = false;
    u64 fixed = 0ull;
    if (used) {
      const int64_t n = i / slots, e = n * V;
      const int64_t rp = (int64_t)(key >> 32), rt = (int64_t)(key & 0xffffffffull);
      const u64 I = counts[i];
      const u64 U = (u64)(u32)sizes_p[e + rp] + (u64)(u32)sizes_t[e + rt] - I;
      nk = n * K + pred[e + rp];                                                          // (the label at a root is a class index)
      match = (double)I > threshold * (double)U;
      const int mark = match ? kOverlapBit | kMatchBit : kOverlapBit;
      first_p = !(atomicOr(state_p + e + rp, mark) & kOverlapBit);
      first_t = !(atomicOr(state_t + e + rt, mark) & kOverlapBit);
      if (match) fixed = (I << 32) / U;
    }
    u64 todo = __ballot(used);
    while (todo) {                                                                        // one turn per (entry, class)
      const int64_t nk1 = __shfl(nk, __builtin_ctzll(todo), 64);
      const bool same = used && nk == nk1;
      const u64 np = __ballot(same && first_p), nt = __ballot(same && first_t), nm = __ballot(same && match);
      const u64 sum = nm ? wave_sum_u64(same ? fixed : 0ull) : 0ull;                      // (nm is uniform)
      if (lane == 0) {
        if (np) atomicAdd(overlapping + 2 * nk1, (u64)__popcll(np));
        if (nt) atomicAdd(overlapping + 2 * nk1 + 1, (u64)__popcll(nt));
        if (nm) {
          atomicAdd(matched + nk1, (u64)__popcll(nm));
          atomicAdd(iou_fixed + nk1, sum);
        }
      }
      todo &= ~__ballot(same);
    }
  }
}

// Every quotient in fp64 from the integers, rounded to fp32 once; 2 x and x 2^-32 are exact, so each is one division.
__global__ void __launch_bounds__(kBlock)
k_inst_finish(const int64_t* __restrict__ components, const int64_t* __restrict__ matched, const int64_t* __restrict__ iou_fixed,
              float* __restrict__ precision, float* __restrict__ recall, float* __restrict__ f1, float* __restrict__ sq,
              float* __restrict__ pq, int64_t NK) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int64_t threads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < NK; i += threads) {
    const double np = (double)components[2 * i], nt = (double)components[2 * i + 1], tp = (double)matched[i];
    const double S = (double)iou_fixed[i] * (1.0 / 4294967296.0);
    precision[i] = (float)(np == 0.0 ? nan : tp / np);
    recall[i] = (float)(nt == 0.0 ? nan : tp / nt);
    f1[i] = (float)(np + nt == 0.0 ? nan : (2.0 * tp) / (np + nt));
    sq[i] = (float)(tp == 0.0 ? nan : S / tp);
    pq[i] = (float)(np + nt == 0.0 ? nan : (2.0 * S) / (np + nt));
  }
}

// 0: in no component; 1: its component is matched; 2: unmatched, overlaps a component of its class; 3: overlaps none
__global__ void __launch_bounds__(kBlock)
k_inst_status(const int* __restrict__ parent, const int* __restrict__ state, uint8_t* __restrict__ out, int64_t V, int64_t chunks) {
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    if (v >= V) break;
    const int p = parent[e + v];
    const int s = p < 0 ? 0 : state[e + p];
    out[e + v] = (uint8_t)(p < 0 ? 0 : (s & kMatchBit) ? 1 : (s & kOverlapBit) ? 2 : 3);
  }
}

// ---- topology: Betti numbers and the Euler characteristic ---------------------------------------------------------------------
// advchain_betti, per map (pred, then target, through the same workspace) and per (entry, class k), A = {v : label == k} for
// every k in [0, K):
//   k_betti_clear    the accumulators (b0, b2 and chi live in the outputs) <- 0.
//   k_betti_euler    chi of all classes in one streaming pass over the lattice corners (see there).
//   k_cc_tile, k_cc_seam, k_cc_flatten with a background outside [0, K): every class is foreground; k_betti_roots counts the
//                    roots per class: b0.
//   3D only, per class k in turn: the same three passes in kComplement mode label {label != k} under the dual adjacency (26 for
//                    6 and the reverse); k_betti_border lowers the parent of every root whose component has a voxel on a face of
//                    the entry to kTouched, so that it is no root any more (parent[x] <= x stays true); k_betti_roots counts the
//                    roots that are left: the cavities b2.  The workspace is that of one labelling whatever K is; a call costs
//                    1 + K labellings per map in 3D and one in 2D, where b1 = b0 - chi needs no complement.
//   k_betti_finish   b1 = b0 + b2 - chi, and the error |b_i(pred) - b_i(target)|.
// Sums per class are taken in a table of the workgroup in LDS when K <= kTableClasses and reach global memory as one 64-bit
// integer add per workgroup and class that is not 0; above that every wave (roots) or window (chi) adds to global memory itself.
// chi's contributions are signed: they are added as two's complement words, so the order does not matter.
constexpr int kTableClasses = 2048;              // 8 KB of LDS
constexpr int kTouched = -2;

__global__ void __launch_bounds__(kBlock)
k_betti_clear(u64* __restrict__ betti, u64* __restrict__ euler, int64_t n_betti, int64_t n_euler) {
  const int64_t threads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_betti; i += threads) betti[i] = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_euler; i += threads) euler[i] = 0ull;
}

// The contribution of the window of a corner p to chi of one class; m: bit i of the window's voxel p - (1, 1, 1) + (i >> 2, (i >> 1)
// & 1, i & 1) is set when the voxel is in the class (bit 7 is the voxel p itself, "high" on every axis; in 2D the four voxels are
// bits 4 .. 7 and the subsets S hold x and y only).  Closed (connectivity == ndim: voxels are closed cubes): the cell at p along
// the axes of S -- vertex, edge, face, cube -- is there when some voxel that is high on every axis of S is in the class; the masks
// are those voxels.  Dual (connectivity 1): the cell is there when every voxel p - sum of e_a over a subset of S is: voxels - face
// pairs + 2 x 2 squares - 2 x 2 x 2 blocks; the masks are the closed ones of the complementary S.
template <int ND>
__device__ __forceinline__ int euler_closed(int m) {
  int c = (int)((m & 0xff) != 0) - (int)((m & 0xaa) != 0) - (int)((m & 0xcc) != 0) + (int)((m & 0x88) != 0);
  if (ND == 3) c += -(int)((m & 0xf0) != 0) + (int)((m & 0xa0) != 0) + (int)((m & 0xc0) != 0) - (int)((m & 0x80) != 0);
  return c;
}
template <int ND>
__device__ __forceinline__ int euler_dual(int m) {
  int c = (int)((m & 0x80) == 0x80) - (int)((m & 0xc0) == 0xc0) - (int)((m & 0xa0) == 0xa0) + (int)((m & 0xf0) == 0xf0);
  if (ND == 3) c += -(int)((m & 0x88) == 0x88) + (int)((m & 0xcc) == 0xcc) + (int)((m & 0xaa) == 0xaa) - (int)((m & 0xff) == 0xff);
  return c;
}

// The tiles of k_cc_tile (blockIdx.x as there), staged with a halo of one voxel on the low side of every axis as 4-byte class
// indices (-1: outside the image or outside [0, K)), so that each int64 label is read about once.  The tile owns the corners at
// the low corner of its voxels and, where it ends at the high face of the image (or the image ends inside it), the corners on that
// face: their high voxels are outside the image.  So staged voxel (lz, ly, lx) is the voxel tile + l - 1, corner (cz, cy, cx) is
// the corner tile + c, and its window is the staged voxels c + {0, 1}^ND.  Per window every distinct class among its voxels (dual:
// only that of the voxel p: every cell needs it) adds its contribution, most of which are 0 (a window inside a class) and skipped.
// E: the words of the map, entry n class k at E[(n K + k) stride].
template <int ND>
__global__ void __launch_bounds__(kBlock)
k_betti_euler(const int64_t* __restrict__ labels, u64* E, int64_t K, Shape s, int tiles_z, int tiles_y, int tiles_x, int dual,
              int stride) {
  constexpr int TZ = ND == 3 ? kTileZ3 : 1, TY = ND == 3 ? kTileY3 : kTileY2;
  constexpr int SZ = ND == 3 ? TZ + 1 : 1, SY = TY + 1, SX = kTileX + 1;                 // staged voxels, and corners, per axis
  constexpr int kStaged = SZ * SY * SX;
  __shared__ int lab[kStaged];
  __shared__ int table[kTableClasses];
  const bool lds = K <= kTableClasses;
  if (lds)
    for (int k = threadIdx.x; k < (int)K; k += kBlock) table[k] = 0;
  int64_t b = blockIdx.x;
  const int bx = (int)(b % tiles_x); b /= tiles_x;
  const int by = (int)(b % tiles_y); b /= tiles_y;
  const int bz = (int)(b % tiles_z);
  const int64_t n = b / tiles_z, V = (int64_t)s.D * s.H * s.W;
  const int z0 = bz * TZ, y0 = by * TY, x0 = bx * kTileX;
  for (int i = threadIdx.x; i < kStaged; i += kBlock) {
    const int lx = i % SX, ly = (i / SX) % SY, lz = i / (SX * SY);
    const int z = ND == 3 ? z0 + lz - 1 : 0, y = y0 + ly - 1, x = x0 + lx - 1;
    int k = -1;
    if (z >= 0 && z < s.D && y >= 0 && y < s.H && x >= 0 && x < s.W) {
      const int64_t v = labels[n * V + ((int64_t)z * s.H + y) * s.W + x];
      if (v >= 0 && v < K) k = (int)v;
    }
    lab[i] = k;
  }
  __syncthreads();
  u64* mine = E + n * K * stride;
  for (int i = threadIdx.x; i < kStaged; i += kBlock) {
    const int cx = i % SX, cy = (i / SX) % SY, cz = i / (SX * SY);
    const int pz = z0 + cz, py = y0 + cy, px = x0 + cx;
    if (px > s.W || (cx == kTileX && px != s.W) || py > s.H || (cy == TY && py != s.H)) continue;
    if (ND == 3 && (pz > s.D || (cz == TZ && pz != s.D))) continue;
    int w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int ix = cx + (q & 1), iy = cy + ((q >> 1) & 1), iz = ND == 3 ? cz + (q >> 2) : 0;
      const bool staged = ix < SX && iy < SY && (ND == 3 ? iz < SZ : (q >> 2) == 1);      // (beyond: outside the image)
      w[q] = staged ? lab[(iz * SY + iy) * SX + ix] : -1;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (dual && q != 7) continue;
      const int k = w[q];
      if (k < 0) continue;
      int m = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) m |= (int)(w[r] == k) << r;
      if (!dual && (m & ((1 << q) - 1))) continue;                                        // (an earlier voxel brought this class)
      const int c = dual ? euler_dual<ND>(m) : euler_closed<ND>(m);
      if (c == 0) continue;
      if (lds) atomicAdd(&table[k], c);
      else atomicAdd(mine + (int64_t)k * stride, (u64)(int64_t)c);
    }
  }
  if (!lds) return;                                                                       // (uniform)
  __syncthreads();
  for (int k = threadIdx.x; k < (int)K; k += kBlock) {
    const int t = table[k];
    if (t) atomicAdd(mine + (int64_t)k * stride, (u64)(int64_t)t);
  }
}

// dst[(n K + k) stride] += the roots of class k in the chunk.  CLASSES: a root re-reads its label (a class index: the voxel is
// foreground), the roots of one class in a wave are counted by one ballot; otherwise every root counts for the class `only`.
template <bool CLASSES>
__global__ void __launch_bounds__(kBlock)
k_betti_roots(const int64_t* __restrict__ labels, const int* __restrict__ parent, u64* dst, int64_t K, int64_t only, int stride,
              int64_t V, int64_t chunks) {
  __shared__ int table[CLASSES ? kTableClasses : 1];
  const Chunked c = chunk_of(chunks);
  const int64_t e = c.n * V;
  const int lane = threadIdx.x & 63;
  const bool lds = !CLASSES || K <= kTableClasses;
  const int held = !CLASSES ? 1 : lds ? (int)K : 0;
  for (int k = threadIdx.x; k < held; k += kBlock) table[k] = 0;
  __syncthreads();
  u64* mine = dst + c.n * K * stride;
  for (int j = 0; j < kPerThread; ++j) {
    if (c.base + j * kBlock >= V) break;                                                  // (uniform)
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    const bool is_root = v < V && parent[e + v] == (int)v;
    if (CLASSES) {
      const int k = is_root ? (int)labels[e + v] : -1;
      u64 todo = __ballot(is_root);
      while (todo) {                                                                      // one turn per class: todo loses bits
        const int k1 = __shfl(k, __builtin_ctzll(todo), 64);
        const u64 same = __ballot(is_root && k == k1);
        if (lane == 0) {
          if (lds) atomicAdd(&table[k1], __popcll(same));
          else atomicAdd(mine + (int64_t)k1 * stride, (u64)__popcll(same));
        }
        todo &= ~same;
      }
    } else {
      const u64 roots = __ballot(is_root);
      if (lane == 0 && roots) atomicAdd(&table[0], __popcll(roots));
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < held; k += kBlock) {
    const int t = table[k];
    if (t) atomicAdd(mine + (CLASSES ? (int64_t)k : only) * stride, (u64)t);
  }
}

// After k_cc_flatten every voxel of a component holds its root.  A voxel on a face of the entry lowers its root's parent to
// kTouched: every writer stores the same value, and a reader sees the root or kTouched, which both say what it needs.  The
// outside of a class is one component with all the faces of the entry in it, and nearly every wave holds a voxel of it (the
// two ends of a row).  So the face voxels of a wave take one turn per distinct root (the turns of k_cc_winner), the first root
// that turns up in the workgroup is kept in LDS and marked once at the end, any other root by the wave, and nobody stores to a
// root that a load shows as marked.  Measured at 2 x 64 x 128 x 128 per launch: a store per face voxel 440 us, a load and at most
// one store per wave 51 us (all on one word).
__global__ void __launch_bounds__(kBlock)
k_betti_border(int* parent, Shape s, int64_t V, int64_t chunks) {
  __shared__ int first_root;
  const Chunked c = chunk_of(chunks);
  int* P = parent + c.n * V;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) first_root = -1;
  __syncthreads();
  for (int j = 0; j < kPerThread; ++j) {
    if (c.base + j * kBlock >= V) break;                                                  // (uniform: ballots inside)
    const int64_t v = c.base + j * kBlock + threadIdx.x;
    int p = -1;
    if (v < V) {
      const u32 row = (u32)v / (u32)s.W;                                                  // (v < V < 2^31: 32-bit divisions)
      const int x = (int)((u32)v - row * (u32)s.W), y = (int)(row % (u32)s.H), z = (int)(row / (u32)s.H);
      if (x == 0 || x == s.W - 1 || y == 0 || y == s.H - 1 || z == 0 || z == s.D - 1)
        p = __hip_atomic_load(P + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // (its root, kTouched at a marked root, -1)
    }
    u64 todo = __ballot(p >= 0);
    while (todo) {                                                                        // one turn per root: todo loses bits
      const int first = __builtin_ctzll(todo);
      const int p1 = __shfl(p, first, 64);
      if (lane == first) {
        const int held = atomicCAS(&first_root, -1, p1);
        if (held != -1 && held != p1 && __hip_atomic_load(P + p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kTouched)
          __hip_atomic_store(P + p1, kTouched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      todo &= ~__ballot(p == p1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && first_root >= 0 &&
      __hip_atomic_load(P + first_root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kTouched)
    __hip_atomic_store(P + first_root, kTouched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// betti (N, K, M, 3) holds b0 and b2, euler (N, K, M) chi, M maps: b1 <- b0 + b2 - chi; error (N, K, 3) or null.
__global__ void __launch_bounds__(kBlock)
k_betti_finish(int64_t* __restrict__ betti, const int64_t* __restrict__ euler, int64_t* __restrict__ error, int64_t NK, int M) {
  const int64_t threads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < NK; i += threads) {
    for (int m = 0; m < M; ++m) {
      int64_t* b = betti + (i * M + m) * 3;
      b[1] = b[0] + b[2] - euler[i * M + m];
    }
    if (error) {
      for (int a = 0; a < 3; ++a) {
        const int64_t d = betti[i * 6 + a] - betti[i * 6 + 3 + a];                        // (error: M == 2)
        error[i * 3 + a] = d < 0 ? -d : d;
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct Plan {
  Shape s;
  int64_t V, chunks, tiles_z, tiles_y, tiles_x;
  int64_t total;                                 // 4-byte words: parent N V, sizes N V, chunk counts N chunks
};

bool components_plan(int64_t N, int ndim, const int64_t* dims, Plan* p) {
  if (N < 1 || !dims_ok(ndim, dims)) return false;
  const Dims d = make_dims(ndim, dims);
  p->V = d.voxels();
  if (p->V > 0x7fffffffLL) return false;                                  // a parent is an int32 index into its entry
  p->s.D = d.s0; p->s.H = d.s1; p->s.W = d.s2;
  p->s.TZ = ndim == 3 ? kTileZ3 : 1;
  p->s.TY = ndim == 3 ? kTileY3 : kTileY2;
  p->s.conn = 1;
  p->chunks = (p->V + kTileVox - 1) / kTileVox;
  p->tiles_z = (d.s0 + p->s.TZ - 1) / p->s.TZ;
  p->tiles_y = (d.s1 + p->s.TY - 1) / p->s.TY;
  p->tiles_x = (d.s2 + kTileX - 1) / kTileX;
  if (N > 0x7fffffffLL / p->V) return false;
  p->total = 2 * N * p->V + N * p->chunks;
  return p->total <= 0x7fffffffLL;                                        // (then every grid below fits one launch as well)
}

struct Work {
  int* parent;
  int* sizes;
  int* counts;
  int* state;          // fill_holes only: two words per voxel
};

// the passes every entry point shares: tile, seam, flatten.  kHoles: of the background; winners2 and the state words (behind the
// chunk counts in the workspace) as k_cc_tile says.  kComplement: of everything but the class `background`.
template <bool SIZES, int MODE = kLabels>
int components_label(const int64_t* labels, void* workspace, u64* winners, int64_t NK, int64_t N, const Plan& p,
                     int64_t background, int64_t K, Work* w, hipStream_t st, u64* winners2 = nullptr) {
  w->parent = (int*)workspace;
  w->sizes = w->parent + N * p.V;
  w->counts = w->sizes + N * p.V;
  w->state = MODE == kHoles ? w->counts + N * p.chunks : nullptr;
  const int64_t tiles = N * p.tiles_z * p.tiles_y * p.tiles_x;           // at most N V
  const unsigned chunked = (unsigned)(N * p.chunks);
  hipLaunchKernelGGL((k_cc_tile<MODE>), dim3((unsigned)tiles), dim3(kBlock), 0, st, labels, w->parent,
                     SIZES ? w->sizes : (int*)nullptr, winners, winners2, w->state, NK, background, K, p.s, (int)p.tiles_z,
                     (int)p.tiles_y, (int)p.tiles_x);
  ADVCHAIN_LAUNCH_CHECK();
  if (p.tiles_z * p.tiles_y * p.tiles_x > 1) {
    hipLaunchKernelGGL((k_cc_seam<MODE>), dim3(chunked), dim3(kBlock), 0, st, labels, w->parent, background, K, p.s, p.V,
                       p.chunks);
    ADVCHAIN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_cc_flatten<SIZES>, dim3(chunked), dim3(kBlock), 0, st, w->parent, w->sizes, w->counts, p.V, p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

// advchain_instance_match: the slots of an entry's pair table, and the words of the whole workspace (-1: refused): keys, counts,
// the state words of both maps, the two labelling workspaces
int64_t instance_plan(int64_t N, const Plan& p, int64_t* slots) {
  *slots = 2 * p.V < 64 ? 64 : 2 * p.V;
  if (N > 0x7fffffffLL / (3 * *slots)) return -1;
  const int64_t total = 3 * N * *slots + 2 * N * p.V + 2 * p.total;
  return total <= 0x7fffffffLL ? total : -1;
}

}  // namespace
}  // namespace advchain

using namespace advchain;

#define COMPONENTS_CHECK_SHAPE(what)                                                                                          \
  ADVCHAIN_CHECK_ARG(N >= 1, what ": bad N");                                                                                 \
  ADVCHAIN_CHECK_ARG(dims && (ndim == 2 || ndim == 3), what ": bad ndim or dims");                                            \
  for (int a = 0; a < ndim; ++a) ADVCHAIN_CHECK_ARG(dims[a] >= 1, what ": bad ndim or dims");                                 \
  ADVCHAIN_CHECK_ARG(connectivity >= 1 && connectivity <= ndim, what ": connectivity must be in 1..ndim");                    \
  Plan p;                                                                                                                     \
  if (!components_plan(N, ndim, dims, &p)) {                                                                                  \
    advchain_set_error_(what ": more than 2^31 - 1 voxels in an entry, or a workspace of more than 2^31 - 1 words");          \
    return ADVCHAIN_ERR_UNSUPPORTED;                                                                                          \
  }                                                                                                                           \
  p.s.conn = connectivity;                                                                                                    \
  hipStream_t st = (hipStream_t)stream

extern "C" {

int64_t advchain_components_workspace(int64_t N, int ndim, const int64_t* dims) {
  Plan p;
  return components_plan(N, ndim, dims, &p) ? p.total : -1;
}

int advchain_components(const int64_t* labels, int32_t* out_labels, int64_t* count, int32_t* sizes, void* workspace, int64_t N,
                        int ndim, const int64_t* dims, int connectivity, int64_t background, int64_t num_classes, void* stream) {
  ADVCHAIN_CHECK_ARG(labels && out_labels && count && workspace, "components: null pointer");
  COMPONENTS_CHECK_SHAPE("components");
  const int64_t K = num_classes < 0 ? -1 : num_classes;
  Work w;
  const int rc = sizes ? components_label<true>(labels, workspace, nullptr, 0, N, p, background, K, &w, st)
                       : components_label<false>(labels, workspace, nullptr, 0, N, p, background, K, &w, st);
  if (rc != ADVCHAIN_OK) return rc;
  const unsigned chunked = (unsigned)(N * p.chunks);
  hipLaunchKernelGGL(k_cc_scan, dim3((unsigned)N), dim3(kBlock), 0, st, w.counts, count, p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_number, dim3(chunked), dim3(kBlock), 0, st, (const int*)w.parent, (const int*)w.counts, out_labels, p.V,
                     p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_gather, dim3(chunked), dim3(kBlock), 0, st, (const int*)w.parent, (const int*)w.sizes, out_labels, sizes,
                     p.V, p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_keep_largest(const int64_t* labels, int64_t* out, void* workspace, void* winners, int64_t N, int64_t K, int ndim,
                          const int64_t* dims, int connectivity, int64_t background, void* stream) {
  ADVCHAIN_CHECK_ARG(labels && out && workspace && winners, "keep_largest: null pointer");
  ADVCHAIN_CHECK_ARG(labels != out, "keep_largest: out must not be the input");
  ADVCHAIN_CHECK_ARG(((uintptr_t)winners & 7) == 0, "keep_largest: winners must be 8-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "keep_largest: K must be in 1..65535");
  COMPONENTS_CHECK_SHAPE("keep_largest");
  ADVCHAIN_CHECK_ARG(N <= ((int64_t)1 << 39) / K, "keep_largest: bad N");
  Work w;
  const int rc = components_label<true>(labels, workspace, (u64*)winners, N * K, N, p, background, K, &w, st);
  if (rc != ADVCHAIN_OK) return rc;
  const unsigned chunked = (unsigned)(N * p.chunks);
  hipLaunchKernelGGL(k_cc_winner, dim3(chunked), dim3(kBlock), 0, st, labels, (const int*)w.parent, (const int*)w.sizes,
                     (u64*)winners, K, p.V, p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_keep, dim3(chunked), dim3(kBlock), 0, st, labels, (const int*)w.parent, (const u64*)winners, out,
                     background, K, p.V, p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_remove_small(const int64_t* labels, int64_t* out, void* workspace, int64_t N, int ndim, const int64_t* dims,
                          int connectivity, int64_t background, int64_t num_classes, int64_t min_size, void* stream) {
  ADVCHAIN_CHECK_ARG(labels && out && workspace, "remove_small: null pointer");
  ADVCHAIN_CHECK_ARG(labels != out, "remove_small: out must not be the input");
  ADVCHAIN_CHECK_ARG(min_size >= 1, "remove_small: min_size must be at least 1");
  COMPONENTS_CHECK_SHAPE("remove_small");
  const int64_t K = num_classes < 0 ? -1 : num_classes;
  Work w;
  const int rc = components_label<true>(labels, workspace, nullptr, 0, N, p, background, K, &w, st);
  if (rc != ADVCHAIN_OK) return rc;
  hipLaunchKernelGGL(k_cc_small, dim3((unsigned)(N * p.chunks)), dim3(kBlock), 0, st, labels, (const int*)w.parent,
                     (const int*)w.sizes, out, background, min_size, p.V, p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int64_t advchain_fill_holes_workspace(int64_t N, int ndim, const int64_t* dims) {
  Plan p;
  return components_plan(N, ndim, dims, &p) ? p.total + 2 * N * p.V : -1;
}

int advchain_fill_holes(const int64_t* labels, int64_t* out, int64_t* fill, int64_t* count, int64_t* voxels, void* workspace,
                        int64_t N, int64_t K, int ndim, const int64_t* dims, int connectivity, int64_t background,
                        int64_t max_size, void* stream) {
  ADVCHAIN_CHECK_ARG(labels && workspace, "fill_holes: null pointer");
  ADVCHAIN_CHECK_ARG((count == nullptr) == (voxels == nullptr), "fill_holes: count and voxels must be null together");
  ADVCHAIN_CHECK_ARG(out || fill || count, "fill_holes: no output");
  ADVCHAIN_CHECK_ARG(labels != out && labels != fill, "fill_holes: out and fill must not be the input");
  ADVCHAIN_CHECK_ARG((((uintptr_t)count | (uintptr_t)voxels) & 7) == 0, "fill_holes: count and voxels must be 8-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "fill_holes: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(max_size != 0, "fill_holes: max_size must be at least 1, or negative for none");
  COMPONENTS_CHECK_SHAPE("fill_holes");
  ADVCHAIN_CHECK_ARG(N <= ((int64_t)1 << 39) / K, "fill_holes: bad N");
  Work w;
  const int rc = components_label<true, kHoles>(labels, workspace, (u64*)count, count ? N * K : 0, N, p, background, K, &w, st,
                                              (u64*)voxels);
  if (rc != ADVCHAIN_OK) return rc;
  const unsigned chunked = (unsigned)(N * p.chunks);
  const int64_t rows = (p.V + kBlock - 1) / kBlock;                                       // (N rows <= N V: fits one launch)
  void (*enclose)(const int64_t*, const int*, int*, int64_t, Shape, int64_t, int64_t) =
      ndim == 2 ? (connectivity == 1 ? k_hole_enclose<2, 1> : k_hole_enclose<2, 2>)
                : (connectivity == 1 ? k_hole_enclose<3, 1> : connectivity == 2 ? k_hole_enclose<3, 2> : k_hole_enclose<3, 3>);
  hipLaunchKernelGGL(enclose, dim3((unsigned)(N * rows)), dim3(kBlock), 0, st, labels, (const int*)w.parent, w.state, K, p.s, p.V,
                     rows);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hole_fill, dim3(chunked), dim3(kBlock), 0, st, labels, (const int*)w.parent, (const int*)w.sizes,
                     (const int*)w.state, out, fill, (u64*)count, (u64*)voxels, K, max_size < 0 ? (int64_t)-1 : max_size, p.V,
                     p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int64_t advchain_instance_match_workspace(int64_t N, int ndim, const int64_t* dims) {
  Plan p;
  int64_t slots;
  return components_plan(N, ndim, dims, &p) ? instance_plan(N, p, &slots) : -1;
}

int advchain_instance_match(const int64_t* pred, const int64_t* target, int64_t* components, int64_t* matched, int64_t* overlapping,
                            int64_t* iou_fixed, float* precision, float* recall, float* f1, float* sq, float* pq,
                            uint8_t* pred_status, uint8_t* target_status, void* workspace, int64_t N, int64_t K, int ndim,
                            const int64_t* dims, int connectivity, int64_t background, double iou_threshold, void* stream) {
  ADVCHAIN_CHECK_ARG(pred && target && components && matched && overlapping && iou_fixed && workspace,
                     "instance_match: null pointer");
  ADVCHAIN_CHECK_ARG(precision && recall && f1 && sq && pq, "instance_match: null pointer");
  ADVCHAIN_CHECK_ARG((((uintptr_t)components | (uintptr_t)matched | (uintptr_t)overlapping | (uintptr_t)iou_fixed |
                       (uintptr_t)workspace) & 7) == 0, "instance_match: the int64 outputs and the workspace must be 8-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "instance_match: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(iou_threshold >= 0.5 && iou_threshold < 1.0, "instance_match: iou_threshold must be in [0.5, 1)");
  COMPONENTS_CHECK_SHAPE("instance_match");
  ADVCHAIN_CHECK_ARG(N <= ((int64_t)1 << 39) / K, "instance_match: bad N");
  int64_t slots;
  if (instance_plan(N, p, &slots) < 0) {
    advchain_set_error_("instance_match: a workspace of more than 2^31 - 1 words");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  const int64_t table = N * slots, NK = N * K;
  u64* keys = (u64*)workspace;
  u32* counts = (u32*)(keys + table);
  int* state_p = (int*)(counts + table);
  int* state_t = state_p + N * p.V;
  int* half_p = state_t + N * p.V;
  int* half_t = half_p + p.total;
  const unsigned chunked = (unsigned)(N * p.chunks);
  const unsigned sweep = (unsigned)((table + kBlock - 1) / kBlock < 8192 ? (table + kBlock - 1) / kBlock : 8192);
  hipLaunchKernelGGL(k_inst_clear, dim3(sweep), dim3(kBlock), 0, st, keys, counts, table, (u64*)components, (u64*)matched,
                     (u64*)overlapping, (u64*)iou_fixed, NK);
  ADVCHAIN_LAUNCH_CHECK();
  Work wp, wt;
  int rc = components_label<true>(pred, half_p, nullptr, 0, N, p, background, K, &wp, st);
  if (rc != ADVCHAIN_OK) return rc;
  rc = components_label<true>(target, half_t, nullptr, 0, N, p, background, K, &wt, st);
  if (rc != ADVCHAIN_OK) return rc;
  hipLaunchKernelGGL(k_inst_pair, dim3(chunked), dim3(kBlock), 0, st, pred, target, (const int*)wp.parent, (const int*)wt.parent,
                     state_p, state_t, keys, counts, (u64*)components, K, p.V, p.chunks, (u32)slots);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_inst_match, dim3(sweep), dim3(kBlock), 0, st, pred, (const int*)wp.sizes, (const int*)wt.sizes, state_p,
                     state_t, (const u64*)keys, (const u32*)counts, (u64*)matched, (u64*)overlapping, (u64*)iou_fixed,
                     iou_threshold, K, p.V, (u32)slots, table);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_inst_finish, dim3((unsigned)((NK + kBlock - 1) / kBlock < 8192 ? (NK + kBlock - 1) / kBlock : 8192)),
                     dim3(kBlock), 0, st,
                     (const int64_t*)components, (const int64_t*)matched, (const int64_t*)iou_fixed, precision, recall, f1, sq, pq,
                     NK);
  ADVCHAIN_LAUNCH_CHECK();
  if (pred_status) {
    hipLaunchKernelGGL(k_inst_status, dim3(chunked), dim3(kBlock), 0, st, (const int*)wp.parent, (const int*)state_p, pred_status,
                       p.V, p.chunks);
    ADVCHAIN_LAUNCH_CHECK();
  }
  if (target_status) {
    hipLaunchKernelGGL(k_inst_status, dim3(chunked), dim3(kBlock), 0, st, (const int*)wt.parent, (const int*)state_t,
                       target_status, p.V, p.chunks);
    ADVCHAIN_LAUNCH_CHECK();
  }
  return ADVCHAIN_OK;
}

int64_t advchain_betti_workspace(int64_t N, int ndim, const int64_t* dims) {
  Plan p;
  return components_plan(N, ndim, dims, &p) ? p.total : -1;
}

int advchain_betti(const int64_t* pred, const int64_t* target, int64_t* betti, int64_t* euler, int64_t* error, void* workspace,
                   int64_t N, int64_t K, int ndim, const int64_t* dims, int connectivity, void* stream) {
  ADVCHAIN_CHECK_ARG(pred && betti && euler && workspace, "betti: null pointer");
  ADVCHAIN_CHECK_ARG(!error || target, "betti: error needs a target");
  ADVCHAIN_CHECK_ARG((((uintptr_t)betti | (uintptr_t)euler | (uintptr_t)error) & 7) == 0,
                     "betti: the outputs must be 8-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "betti: K must be in 1..65535");
  COMPONENTS_CHECK_SHAPE("betti");
  ADVCHAIN_CHECK_ARG(!(ndim == 3 && connectivity == 2),
                     "betti: connectivity 2 (18-adjacency) has no dual adjacency for the complement in 3D; use 1 or 3");
  ADVCHAIN_CHECK_ARG(N <= ((int64_t)1 << 39) / K, "betti: bad N");
  const int M = target ? 2 : 1, stride = 3 * M;
  const int64_t NK = N * K;
  const unsigned chunked = (unsigned)(N * p.chunks);
  const unsigned tiles = (unsigned)(N * p.tiles_z * p.tiles_y * p.tiles_x);
  const unsigned sweep = (unsigned)((NK * stride + kBlock - 1) / kBlock < 8192 ? (NK * stride + kBlock - 1) / kBlock : 8192);
  hipLaunchKernelGGL(k_betti_clear, dim3(sweep), dim3(kBlock), 0, st, (u64*)betti, (u64*)euler, NK * stride, NK * M);
  ADVCHAIN_LAUNCH_CHECK();
  Plan dual = p;
  dual.s.conn = ndim + 1 - connectivity;                                                  // 6 <-> 26 (used in 3D only)
  const bool closed = connectivity == ndim;
  for (int m = 0; m < M; ++m) {
    const int64_t* labels = m == 0 ? pred : target;
    hipLaunchKernelGGL(ndim == 3 ? k_betti_euler<3> : k_betti_euler<2>, dim3(tiles), dim3(kBlock), 0, st, labels,
                       (u64*)euler + m, K, p.s, (int)p.tiles_z, (int)p.tiles_y, (int)p.tiles_x, closed ? 0 : 1, M);
    ADVCHAIN_LAUNCH_CHECK();
    Work w;
    int rc = components_label<false>(labels, workspace, nullptr, 0, N, p, (int64_t)-1, K, &w, st);    // (-1: no class)
    if (rc != ADVCHAIN_OK) return rc;
    hipLaunchKernelGGL(k_betti_roots<true>, dim3(chunked), dim3(kBlock), 0, st, labels, (const int*)w.parent,
                       (u64*)betti + 3 * m, K, (int64_t)0, stride, p.V, p.chunks);
    ADVCHAIN_LAUNCH_CHECK();
    if (ndim != 3) continue;
    for (int64_t k = 0; k < K; ++k) {
      rc = components_label<false, kComplement>(labels, workspace, nullptr, 0, N, dual, k, K, &w, st);
      if (rc != ADVCHAIN_OK) return rc;
      hipLaunchKernelGGL(k_betti_border, dim3(chunked), dim3(kBlock), 0, st, w.parent, p.s, p.V, p.chunks);
      ADVCHAIN_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_betti_roots<false>, dim3(chunked), dim3(kBlock), 0, st, labels, (const int*)w.parent,
                         (u64*)betti + 3 * m + 2, K, k, stride, p.V, p.chunks);
      ADVCHAIN_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(k_betti_finish, dim3((unsigned)((NK + kBlock - 1) / kBlock < 8192 ? (NK + kBlock - 1) / kBlock : 8192)),
                     dim3(kBlock), 0, st, betti, (const int64_t*)euler, error, NK, M);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
