// Surface distance metrics of a pair of label maps, every class in one call, 2D and 3D, for gfx950:
//
//   advchain_surface_metrics     <- common.metrics.surface_distance_metrics (hausdorff_distance, average_surface_distance)
//
// For entry n and class k, A = {v: pred[n,v] == k}, B = {v: target[n,v] == k}; the border of a set is its voxels with a face
// neighbour (4 in 2D, 6 in 3D) outside it, a position outside the image counting as outside.  A voxel has one label per map,
// so the borders of ALL classes of a map are one "edge label map": the label at a border voxel, -1 elsewhere.
//   k_surface_edges    one pass over pred and target.  A workgroup stages a tile of classes with a halo of one voxel in LDS
//                      (each label is read once per tile that touches it; no per-neighbour global loads), writes both edge
//                      label maps (int64: they are the SRC_LABELS source of the transform's row pass as they are) and adds the
//                      counts |dA|, |dB|, |A|, |B|, |A n B| per class: LDS counters, then one 64-bit integer atomic per
//                      non-zero counter, straight into the outputs.
//   edt_label_fields   (csrc/edt.hip) the squared distance of every voxel to the nearest border voxel of class k, for every k
//                      and both maps; int32 with unit spacing (exact), fp32 with a sampling.  Not finished: the reductions read
//                      the squares.
//   k_surface_digits   A border voxel v of class a = pred[v] contributes ONE key, the field word of (the other map, a, v),
//                      to segment (n, a, direction).  Keys are non-negative: the integer order of their 32 bits is the order
//                      of the distances.  Order statistic x_(j) by a most-significant-digit radix select: four passes of 8
//                      bits, each an LDS histogram per class merged into the segment's with 64-bit integer atomics;
//                      k_surface_select then narrows the prefix and the rank in device memory.  Pass 0 also takes the maximum
//                      key; a fifth pass takes the smallest key above x_(j), which is x_(j+1) unless enough keys tie at x_(j).
//   k_surface_sums     sum of the distances of a segment in fp64: a wave adds the lanes of one class in a fixed butterfly, one
//                      lane adds that to the wave's LDS accumulator, the four waves' are added in order into ONE partial per
//                      workgroup and segment, and the finish adds the partials in a fixed order.
//   k_surface_finish   roots in fp64 (of exact integers with unit spacing), numpy's linear percentile rule, the symmetric
//                      combinations, NaN / +inf for empty borders, Dice; one rounding to fp32.
// Integer atomics only (their order cannot change a sum, a maximum or a minimum), no memset, no host read-back: every word
// that is read was written by a kernel of the same call.  Labels are only COMPARED with class indices.
#include <math.h>

#include "common.h"
#include "edt_fields.h"

namespace advchain {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kEdgeTX = 64;                  // a wave per tile row
constexpr int kCountClasses = 256;           // classes whose five counters LDS holds at a time (k_surface_edges)
constexpr int kDigitClasses = 32;            // classes whose 256-bin histogram LDS holds at a time (32 KiB)
constexpr int kSumClasses = 256;             // classes whose four per-wave fp64 accumulators LDS holds at a time (8 KiB)
constexpr int kChunkVoxels = 4096;           // voxels of an entry per reduction workgroup ...
constexpr int kMaxChunks = 256;              // ... until there are this many workgroups per entry and direction
constexpr int kPassAbove = 4;                // the pass after the four digits: smallest key above x_(j)

__device__ __forceinline__ int class_of(int64_t y, int K) { return (y >= 0 && y < (int64_t)K) ? (int)y : -1; }

// per-call state of the segments s = (n K + k) 2 + direction, carved from the workspace
struct Segments {
  u64* hist;        // [S][256]
  u64* rank;        // [S]      rank of x_(j) among the keys that share `prefix`
  double* partial;  // [N][2][chunks][K]
  u32* prefix;      // [S]      the digits of x_(j) chosen so far; after the last digit x_(j) itself
  u32* maxkey;      // [S]
  u32* above;       // [S]      smallest key above x_(j), 0xffffffff if none
  u32* tie;         // [S]      1: x_(j+1) == x_(j)
};

// ---- clear ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_surface_clear(int64_t* __restrict__ surface_voxels, int64_t* __restrict__ overlap, Segments sg, int64_t NK) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x, S = 2 * NK;
  if (i < 2 * NK) surface_voxels[i] = 0;
  if (i < 3 * NK) overlap[i] = 0;
  if (i < S) {
    sg.maxkey[i] = 0u;
    sg.above[i] = 0xffffffffu;
  }
  if (i < S * 256) sg.hist[i] = 0ull;
}

// ---- edge label maps and counts --------------------------------------------------------------------------------------------
// blockIdx.x = ((n tz + z tile) ty + y tile) tx + x tile; the tile is TZ x TY x 64 voxels, staged with a halo of one voxel in y
// and x, and in z when the maps are 3D (hz = 1).  A staged cell holds the class, -1 for no class, -2 outside the image.
__global__ void __launch_bounds__(kBlock)
k_surface_edges(const int64_t* __restrict__ pred, const int64_t* __restrict__ target, int64_t* __restrict__ edge_p,
                int64_t* __restrict__ edge_t, int64_t* surface_voxels, int64_t* overlap, int K, int D, int H, int W, int hz,
                int TZ, int TY, int tiles_z, int tiles_y, int tiles_x) {
  extern __shared__ __align__(16) unsigned char surface_lds[];
  __shared__ u32 counts[kCountClasses * 5];
  const int LZ = TZ + 2 * hz, LY = TY + 2, LX = kEdgeTX + 2, cells = LZ * LY * LX;
  int* cp = reinterpret_cast<int*>(surface_lds);
  int* ct = cp + cells;
  int64_t b = blockIdx.x;
  const int bx = (int)(b % tiles_x); b /= tiles_x;
  const int by = (int)(b % tiles_y); b /= tiles_y;
  const int bz = (int)(b % tiles_z);
  const int64_t n = b / tiles_z, V = (int64_t)D * H * W;
  const int z0 = bz * TZ, y0 = by * TY, x0 = bx * kEdgeTX;

  for (int i = threadIdx.x; i < cells; i += kBlock) {
    const int lx = i % LX, ly = (i / LX) % LY, lz = i / (LX * LY);
    const int z = z0 + lz - hz, y = y0 + ly - 1, x = x0 + lx - 1;
    int a = -2, c = -2;
    if (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t at = n * V + ((int64_t)z * H + y) * W + x;
      a = class_of(pred[at], K);
      c = class_of(target[at], K);
    }
    cp[i] = a;
    ct[i] = c;
  }

  const int own = TZ * TY * kEdgeTX;
  for (int g0 = 0; g0 < K; g0 += kCountClasses) {
    for (int i = threadIdx.x; i < kCountClasses * 5; i += kBlock) counts[i] = 0u;
    __syncthreads();                                     // (the first time: also the barrier behind the staging)
    for (int i = threadIdx.x; i < own; i += kBlock) {
      const int tx = i % kEdgeTX, ty = (i / kEdgeTX) % TY, tz = i / (kEdgeTX * TY);
      const int z = z0 + tz, y = y0 + ty, x = x0 + tx;
      if (z >= D || y >= H || x >= W) continue;
      const int at = ((tz + hz) * LY + ty + 1) * LX + tx + 1;
      const int a = cp[at], c = ct[at];
      bool ea = cp[at - 1] != a || cp[at + 1] != a || cp[at - LX] != a || cp[at + LX] != a;
      bool ec = ct[at - 1] != c || ct[at + 1] != c || ct[at - LX] != c || ct[at + LX] != c;
      if (hz) {
        ea = ea || cp[at - LX * LY] != a || cp[at + LX * LY] != a;
        ec = ec || ct[at - LX * LY] != c || ct[at + LX * LY] != c;
      }
      ea = ea && a >= 0;
      ec = ec && c >= 0;
      if (g0 == 0) {
        const int64_t o = n * V + ((int64_t)z * H + y) * W + x;
        edge_p[o] = ea ? (int64_t)a : (int64_t)-1;
        edge_t[o] = ec ? (int64_t)c : (int64_t)-1;
      }
      if (a >= g0 && a < g0 + kCountClasses) {
        u32* q = counts + (a - g0) * 5;
        atomicAdd(q + 2, 1u);
        if (ea) atomicAdd(q + 0, 1u);
        if (a == c) atomicAdd(q + 4, 1u);
      }
      if (c >= g0 && c < g0 + kCountClasses) {
        u32* q = counts + (c - g0) * 5;
        atomicAdd(q + 3, 1u);
        if (ec) atomicAdd(q + 1, 1u);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kCountClasses * 5; i += kBlock) {
      const int kk = g0 + i / 5, f = i % 5;
      const u32 v = counts[i];
      if (kk < K && v) {
        int64_t* o = f < 2 ? surface_voxels + (n * K + kk) * 2 + f : overlap + (n * K + kk) * 3 + (f - 2);
        atomicAdd(reinterpret_cast<u64*>(o), (u64)v);
      }
    }
    __syncthreads();
  }
}

// ---- the keys of a reduction workgroup --------------------------------------------------------------------------------------
// blockIdx = (chunk, n, direction); direction 0: border voxels of pred against the field of target's borders, 1: the reverse.
// edges (2, N, V): pred's, target's; fields (2, N, K, V): squared distance to pred's borders, to target's.
struct Chunk {
  const int64_t* edge;
  const u32* field;
  int64_t begin, end, V;
};
__device__ __forceinline__ Chunk chunk_of(const int64_t* edges, const u32* fields, int64_t N, int K, int64_t V, int64_t per) {
  Chunk c;
  const int64_t n = blockIdx.y, d = blockIdx.z;
  c.edge = edges + (d * N + n) * V;
  c.field = fields + ((1 - d) * N + n) * K * V;
  c.begin = (int64_t)blockIdx.x * per;
  c.end = c.begin + per < V ? c.begin + per : V;
  c.V = V;
  return c;
}

// PASS 0..3: histogram of digit PASS (most significant first) of the keys that share the digits chosen so far; PASS 0 also the
// maximum key; kPassAbove: the smallest key above x_(j)
template <int PASS>
__global__ void __launch_bounds__(kBlock)
k_surface_digits(const int64_t* __restrict__ edges, const u32* __restrict__ fields, Segments sg, int64_t N, int K, int64_t V,
                 int64_t per) {
  __shared__ u32 bins[PASS < kPassAbove ? kDigitClasses * 256 : 1];
  __shared__ u32 extreme[kDigitClasses];
  const Chunk ch = chunk_of(edges, fields, N, K, V, per);
  const int64_t n = blockIdx.y, d = blockIdx.z;
  for (int g0 = 0; g0 < K; g0 += kDigitClasses) {
    if constexpr (PASS < kPassAbove)
      for (int i = threadIdx.x; i < kDigitClasses * 256; i += kBlock) bins[i] = 0u;
    if (threadIdx.x < kDigitClasses) extreme[threadIdx.x] = PASS == 0 ? 0u : 0xffffffffu;
    __syncthreads();
    for (int64_t v = ch.begin + threadIdx.x; v < ch.end; v += kBlock) {
      const int64_t e = ch.edge[v];
      if (e < g0 || e >= g0 + kDigitClasses) continue;          // (an edge label is a class or -1)
      const int kk = (int)e - g0;
      const u32 key = ch.field[e * V + v];
      const int64_t s = (n * K + e) * 2 + d;
      if constexpr (PASS == 0) {
        atomicAdd(&bins[kk * 256 + (key >> 24)], 1u);
        atomicMax(&extreme[kk], key);
      } else if constexpr (PASS < kPassAbove) {
        constexpr int shift = 24 - 8 * PASS;
        if ((key >> (shift + 8)) == (sg.prefix[s] >> (shift + 8))) atomicAdd(&bins[kk * 256 + ((key >> shift) & 255u)], 1u);
      } else {
        if (key > sg.prefix[s]) atomicMin(&extreme[kk], key);
      }
    }
    __syncthreads();
    if constexpr (PASS < kPassAbove)
      for (int i = threadIdx.x; i < kDigitClasses * 256; i += kBlock) {
        const int kk = g0 + (i >> 8);
        const u32 c = bins[i];
        if (kk < K && c) atomicAdd(&sg.hist[(((n * K + kk) * 2 + d) << 8) + (i & 255)], (u64)c);
      }
    if (threadIdx.x < kDigitClasses && g0 + threadIdx.x < K) {
      const int64_t s = (n * K + g0 + threadIdx.x) * 2 + d;
      if (PASS == 0 && extreme[threadIdx.x]) atomicMax(&sg.maxkey[s], extreme[threadIdx.x]);
      if (PASS == kPassAbove && extreme[threadIdx.x] != 0xffffffffu) atomicMin(&sg.above[s], extreme[threadIdx.x]);
    }
    __syncthreads();
  }
}

// rank j of the percentile among m sorted values: h = (m - 1) (q / 100), j = floor(h), g = h - j (numpy's "linear" rule)
__device__ __forceinline__ u64 percentile_rank(int64_t m, double q, double* g) {
  const double h = (double)(m - 1) * (q / 100.0), j = floor(h);
  *g = h - j;
  return (u64)j;
}

// One workgroup per segment, thread t owns bin t: the bin that holds rank r extends the prefix, r becomes the rank inside it,
// and the histogram is left cleared for the next pass.
template <int PASS>
__global__ void __launch_bounds__(256)
k_surface_select(Segments sg, const int64_t* __restrict__ surface_voxels, double q) {
  __shared__ u64 scan[2][256];
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t m = surface_voxels[s];                       // (segment s = (n K + k) 2 + direction: the layout of surface_voxels)
  const u64 c = sg.hist[(s << 8) + t];
  sg.hist[(s << 8) + t] = 0ull;
  if (m == 0) return;                                        // (uniform: no key, nothing to select)
  double g;
  const u64 r = PASS == 0 ? percentile_rank(m, q, &g) : sg.rank[s];
  scan[0][t] = c;
  __syncthreads();
  int cur = 0;
  for (int o = 1; o < 256; o <<= 1) {
    scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0ull);
    cur ^= 1;
    __syncthreads();
  }
  const u64 incl = scan[cur][t], excl = incl - c;
  if (r >= excl && r < incl) {                                // exactly one thread: 0 <= r < the sum of the bins
    constexpr int shift = 24 - 8 * PASS;
    sg.prefix[s] = (PASS == 0 ? 0u : sg.prefix[s]) | ((u32)t << shift);
    sg.rank[s] = r - excl;
    if (PASS == 3) sg.tie[s] = (r - excl + 1 < c) ? 1u : 0u;
  }
}

__device__ __forceinline__ double key_value(u32 key, int unit) { return unit ? (double)key : (double)__uint_as_float(key); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(kBlock)
k_surface_sums(const int64_t* __restrict__ edges, const u32* __restrict__ fields, Segments sg, int64_t N, int K, int64_t V,
               int64_t per, int unit) {
  __shared__ double acc[4][kSumClasses];
  const Chunk ch = chunk_of(edges, fields, N, K, V, per);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* out = sg.partial + (((int64_t)blockIdx.y * 2 + blockIdx.z) * gridDim.x + blockIdx.x) * K;
  for (int g0 = 0; g0 < K; g0 += kSumClasses) {
    acc[wave][lane] = acc[wave][lane + 64] = acc[wave][lane + 128] = acc[wave][lane + 192] = 0.0;
    __syncthreads();
    for (int64_t base = ch.begin + wave * 64; base < ch.end; base += kBlock) {           // (uniform over the wave)
      const int64_t v = base + lane;
      const int64_t e = v < ch.end ? ch.edge[v] : -1;
      const bool mine = e >= g0 && e < g0 + kSumClasses;
      const double x = mine ? sqrt(key_value(ch.field[e * V + v], unit)) : 0.0;
      const int kk = mine ? (int)e - g0 : -1;
      u64 todo = __ballot(mine);
      while (todo) {                                                                   // one turn per class among the 64 voxels
        const int k1 = __shfl(kk, __builtin_ctzll(todo), 64);
        const bool same = kk == k1;
        const double sum = wave_sum_f64(same ? x : 0.0);
        if (lane == 0) acc[wave][k1] += sum;
        todo &= ~__ballot(same);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSumClasses && g0 + i < K; i += kBlock) out[g0 + i] = ((acc[0][i] + acc[1][i]) + acc[2][i]) + acc[3][i];
    __syncthreads();
  }
}

// One wave per (n, k).  Lane l adds the partials of the workgroups l, l + 64, ... in order and a fixed butterfly adds the lanes:
// the same order on every run.  Lane 0 writes.
__global__ void __launch_bounds__(64)
k_surface_finish(Segments sg, const int64_t* __restrict__ surface_voxels, const int64_t* __restrict__ overlap, double q, int unit,
                 float* __restrict__ hausdorff, float* __restrict__ hausdorff_pct, float* __restrict__ assd,
                 float* __restrict__ directed, double* __restrict__ max_squared, float* __restrict__ dice, int64_t N, int K,
                 int chunks) {
  const int64_t i = blockIdx.x, n = i / K, k = i - n * K;
  const int lane = threadIdx.x;
  double sum[2];
  for (int d = 0; d < 2; ++d) {
    const double* p = sg.partial + (n * 2 + d) * chunks * K + k;
    double t = 0.0;
    for (int c = lane; c < chunks; c += 64) t += p[(int64_t)c * K];
    sum[d] = wave_sum_f64(t);
  }
  if (lane) return;
  const int64_t a = overlap[i * 3], b = overlap[i * 3 + 1], ab = overlap[i * 3 + 2];
  dice[i] = a + b == 0 ? (float)NAN : (float)(2.0 * (double)ab / (double)(a + b));
  const int64_t m[2] = {surface_voxels[i * 2], surface_voxels[i * 2 + 1]};
  if (m[0] == 0 || m[1] == 0) {
    const double fill = (m[0] == 0 && m[1] == 0) ? (double)NAN : (double)INFINITY;
    hausdorff[i] = hausdorff_pct[i] = assd[i] = (float)fill;
    for (int j = 0; j < 6; ++j) directed[i * 6 + j] = (float)fill;
    max_squared[i * 2] = max_squared[i * 2 + 1] = fill;
    return;
  }
  double top[2], pct[2];
  for (int d = 0; d < 2; ++d) {
    const int64_t s = i * 2 + d;
    const double sq = key_value(sg.maxkey[s], unit);
    max_squared[s] = sq;
    top[d] = sqrt(sq);
    double g;
    const u64 j = percentile_rank(m[d], q, &g);
    const double xj = sqrt(key_value(sg.prefix[s], unit));
    const bool same = sg.tie[s] || j + 1 > (u64)(m[d] - 1);
    const double xj1 = same ? xj : sqrt(key_value(sg.above[s], unit));
    pct[d] = xj + g * (xj1 - xj);
    directed[s * 3] = (float)top[d];
    directed[s * 3 + 1] = (float)pct[d];
    directed[s * 3 + 2] = (float)(sum[d] / (double)m[d]);
  }
  hausdorff[i] = (float)(top[0] > top[1] ? top[0] : top[1]);
  hausdorff_pct[i] = (float)(pct[0] > pct[1] ? pct[0] : pct[1]);
  assd[i] = (float)((sum[0] + sum[1]) / (double)(m[0] + m[1]));
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct SurfacePlan {
  int64_t V, chunks, per;
  int64_t w_fields, w_edges, w_hist, w_rank, w_partial, w_seg;     // 4-byte words of each region, in this order; w_seg x 4 at the end
  int64_t total;
};

bool surface_plan(int64_t N, int64_t K, int ndim, const int64_t* dims, SurfacePlan* p) {
  const int64_t f = edt_label_fields_words(2 * N, K, ndim, dims);
  if (f < 0) return false;
  p->V = f / (2 * N * K);
  p->chunks = (p->V + kChunkVoxels - 1) / kChunkVoxels;
  if (p->chunks > kMaxChunks) p->chunks = kMaxChunks;
  p->per = (p->V + p->chunks - 1) / p->chunks;
  const int64_t S = 2 * N * K;
  p->w_fields = f + (f & 1);
  p->w_edges = 4 * N * p->V;
  p->w_hist = 512 * S;
  p->w_rank = 2 * S;
  p->w_partial = 2 * S * p->chunks;
  p->w_seg = S;
  if (p->V > ((int64_t)1 << 58) / (4 * N)) return false;
  p->total = p->w_fields + p->w_edges + p->w_hist + p->w_rank + p->w_partial + 4 * p->w_seg;
  return p->total < ((int64_t)1 << 60);
}

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int64_t advchain_surface_metrics_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims) {
  SurfacePlan p;
  if (N < 1 || K < 1 || K > 65535 || N > ((int64_t)1 << 39) / K || !surface_plan(N, K, ndim, dims, &p)) return -1;
  return p.total;
}

int advchain_surface_metrics(const int64_t* pred, const int64_t* target, const float* sampling, double q, float* hausdorff,
                             float* hausdorff_pct, float* assd, float* directed, int64_t* surface_voxels, double* max_squared,
                             int64_t* overlap, float* dice, void* workspace, int64_t N, int64_t K, int ndim,
                             const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(pred && target && hausdorff && hausdorff_pct && assd && directed && surface_voxels && max_squared &&
                         overlap && dice && workspace, "surface_metrics: null pointer");
  ADVCHAIN_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "surface_metrics: workspace must be 16-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "surface_metrics: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(N >= 1, "surface_metrics: bad N");
  ADVCHAIN_CHECK_ARG(q >= 0.0 && q <= 100.0, "surface_metrics: the percentile must be in [0, 100]");
  ADVCHAIN_CHECK_ARG(dims && (ndim == 2 || ndim == 3), "surface_metrics: bad ndim or dims");
  for (int a = 0; a < ndim; ++a) ADVCHAIN_CHECK_ARG(dims[a] >= 1, "surface_metrics: bad ndim or dims");
  SurfacePlan p;
  if (N > ((int64_t)1 << 39) / K || !surface_plan(N, K, ndim, dims, &p)) {
    advchain_set_error_("surface_metrics: shape too large for the distance fields (an axis or the squared diagonal)");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const int D = ndim == 3 ? (int)dims[0] : 1, H = (int)dims[ndim - 2], W = (int)dims[ndim - 1];
  const int64_t S = 2 * N * K;

  u32* w = (u32*)workspace;
  u32* fields = w;                              w += p.w_fields;
  int64_t* edges = (int64_t*)w;                 w += p.w_edges;
  Segments sg;
  sg.hist = (u64*)w;                            w += p.w_hist;
  sg.rank = (u64*)w;                            w += p.w_rank;
  sg.partial = (double*)w;                      w += p.w_partial;
  sg.prefix = w;                                w += p.w_seg;
  sg.maxkey = w;                                w += p.w_seg;
  sg.above = w;                                 w += p.w_seg;
  sg.tie = w;

  const int64_t clear_blocks = (S * 256 + kBlock - 1) / kBlock;
  const int hz = ndim == 3 ? 1 : 0, TZ = hz ? 4 : 1, TY = hz ? 8 : 32;
  const int64_t tiles_z = (D + TZ - 1) / TZ, tiles_y = (H + TY - 1) / TY, tiles_x = (W + kEdgeTX - 1) / kEdgeTX;
  const int64_t edge_blocks = N * tiles_z * tiles_y * tiles_x;
  if (clear_blocks > 0x7fffffff || edge_blocks > 0x7fffffff || N > 65535) {
    advchain_set_error_("surface_metrics: too many workgroups for one launch (N above 65535, or N K or the tiles above 2^31)");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(k_surface_clear, dim3((unsigned)clear_blocks), dim3(kBlock), 0, st, surface_voxels, overlap, sg, N * K);
  ADVCHAIN_LAUNCH_CHECK();
  const size_t lds = (size_t)(TZ + 2 * hz) * (TY + 2) * (kEdgeTX + 2) * 2 * sizeof(int);
  hipLaunchKernelGGL(k_surface_edges, dim3((unsigned)edge_blocks), dim3(kBlock), lds, st, pred, target, edges, edges + N * p.V,
                     surface_voxels, overlap, (int)K, D, H, W, hz, TZ, TY, (int)tiles_z, (int)tiles_y, (int)tiles_x);
  ADVCHAIN_LAUNCH_CHECK();

  const int rc = edt_label_fields(edges, sampling, fields, 2 * N, K, ndim, dims, "surface_metrics", st);
  if (rc != ADVCHAIN_OK) return rc;

  const dim3 grid((unsigned)p.chunks, (unsigned)N, 2);
  const int unit = sampling ? 0 : 1;
#define SURFACE_DIGIT(PASS)                                                                                                   \
  hipLaunchKernelGGL(k_surface_digits<PASS>, grid, dim3(kBlock), 0, st, (const int64_t*)edges, (const u32*)fields, sg, N, (int)K, \
                     p.V, p.per);                                                                                             \
  ADVCHAIN_LAUNCH_CHECK();
#define SURFACE_SELECT(PASS)                                                                                                  \
  hipLaunchKernelGGL(k_surface_select<PASS>, dim3((unsigned)S), dim3(256), 0, st, sg, (const int64_t*)surface_voxels, q);      \
  ADVCHAIN_LAUNCH_CHECK();
  SURFACE_DIGIT(0) SURFACE_SELECT(0)
  SURFACE_DIGIT(1) SURFACE_SELECT(1)
  SURFACE_DIGIT(2) SURFACE_SELECT(2)
  SURFACE_DIGIT(3) SURFACE_SELECT(3)
  SURFACE_DIGIT(kPassAbove)
#undef SURFACE_DIGIT
#undef SURFACE_SELECT
  hipLaunchKernelGGL(k_surface_sums, grid, dim3(kBlock), 0, st, (const int64_t*)edges, (const u32*)fields, sg, N, (int)K, p.V,
                     p.per, unit);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_surface_finish, dim3((unsigned)(N * K)), dim3(64), 0, st, sg,
                     (const int64_t*)surface_voxels, (const int64_t*)overlap, q, unit, hausdorff, hausdorff_pct, assd, directed,
                     max_squared, dice, N, (int)K, (int)p.chunks);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
