// Surface distance metrics of a pair of label maps, every class in one call, 2D and 3D, for gfx950:
//
//   advchain_surface_metrics     <- common.metrics.surface_distance_metrics (hausdorff_distance, average_surface_distance)
//   advchain_surface_dice        <- common.metrics.surface_dice (further down: "surface Dice at a tolerance")
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

// ---- surface Dice at a tolerance --------------------------------------------------------------------------------------------
//   advchain_surface_dice        <- common.metrics.surface_dice
//
// within[n,k,0] = #{a in dA: d(a, dB)^2 <= thr_k}, within[n,k,1] = #{b in dB: d(b, dA)^2 <= thr_k}, next to m0 = |dA|, m1 = |dB|;
// surface_dice = (c0 + c1) / (m0 + m1).  thr_k is a device word per class: with unit spacing the integer min(floor(tau_k^2),
// 2^30 - 1), and the test is on exact integer squares; with a sampling the bits of tau_k^2 rounded to fp32 (at most 1e29), and the
// square is the fp32 value of the transform, ((s_x dx)^2 + (s_y dy)^2) + (s_z dz)^2 without contraction: the transform takes
// exact minima of these sums axis by axis and fp32 addition is monotone, so "some border voxel of the class within the
// threshold" and "field word <= threshold" are the same predicate.  Both kinds of word are non-negative: their unsigned
// integer order is their order.  Two routes with the same bits:
//   ball     k_surface_ball, one pass over the two maps, no word per class.  A workgroup stages the classes of both maps of its
//            tile and a halo of cap_a + 1 voxels per tiled axis in LDS, one 32-bit word per cell (pred's class in the low half,
//            target's in the high half, 0xffff no class, 0xfffe outside the image), evaluates the border predicate of
//            k_surface_edges for the owned cells and cap_a of the halo (the last layer only serves as their neighbours) and
//            leaves in every word the class at a border voxel and 0xffff elsewhere.  An owned border voxel of either map then
//            looks for the same class in the other half inside the ball: |dz| and |dy| outward from 0, x bounded by what is
//            left of the threshold, stopping at the first hit.  m0, m1, c0, c1: LDS counters per group of 256 classes, one
//            64-bit integer atomic per non-zero counter.  clear + ball + finish: three launches, no field, no edge map.
//            cap_a = min(the largest offset o with (s_a o)^2 <= the largest threshold, dims_a - 1): isqrt(T_max) with unit
//            spacing and floor(tau_max / s_a) with a sampling (decided by the fp32 test itself where the quotient is within
//            rounding of an integer).
//            ELIGIBLE iff K <= 65534 (the two halves of a word) and a tile of the list below -- from the widest on, the
//            first that fits is taken -- has (tz + 2 hz) (ty + 2 hy) (tx + 2 hx) cells of 5 bytes (a word and a flag byte)
//            within kBallLdsBytes, with h_a = cap_a + 1 and in 2D tz = 1, hz = 0:
//              2D  (32,64) (16,64) (8,64)            3D  (8,8,32) (4,8,32) (4,4,32) (2,4,32) (2,2,32)
//            With unit spacing that is a cap of at most 38 in 2D and 6 in 3D.  No limit on the axes beyond 2^31 - 1 tiles.
//   fields   the edge pass and edt_label_fields as for the distances, then k_surface_within: over the chunks and keys of
//            k_surface_digits, key <= thr[class] per (n, k, direction), LDS counters per group of classes merged with 64-bit
//            integer atomics.  Any tolerance; the shape limits and the workspace of the distance fields.
// Dispatch: the ball where it is eligible and no cap exceeds kBallDispatchCap2 (2D) / kBallDispatchCap3 (3D), else the fields,
// else (a shape the fields refuse) the ball where it is eligible.
constexpr int kBallLdsBytes = 61440;          // dynamic LDS of k_surface_ball: 64 KiB less the 4 KiB of its counters
constexpr int kBallClasses = 256;             // classes whose four counters LDS holds at a time
constexpr int kBallMaxK = 65534;
// Dispatch limits from profiles/r28/surface_dice/summary.md (blobs, caps 1, 2, 3 and 5 timed against the fields).  2D: the ball
// is 1.2-20x faster at every cap timed, 5 is the largest that was.  3D: 4.5x and 1.8x faster at caps 1 and 2, but 0.74x at cap 3
// and 0.38x at cap 5 (4x4x128x128x64: the halo is 5x to 22x the owned tile).
constexpr int kBallDispatchCap2 = 5;
constexpr int kBallDispatchCap3 = 2;
constexpr u32 kHalfNone = 0xffffu, kHalfOutside = 0xfffeu;
enum { DICE_ROUTE_ANY = 0, DICE_ROUTE_BALL = 1, DICE_ROUTE_FIELDS = 2 };

struct BallGeom {
  int nd, tz, ty, tx;          // owned tile (tz = 1 in 2D)
  int c[3], h[3];              // cap and halo per axis (z, y, x); 0 along z in 2D
  int lz, ly, lx;              // staged cells per axis
  int tiles_z, tiles_y, tiles_x;
  float s[3];
};

template <typename T> struct Bsq;
template <> struct Bsq<int> {
  static __device__ __forceinline__ int of(int d, float) { return d * d; }
  static __device__ __forceinline__ int word(u32 w) { return (int)w; }
};
template <> struct Bsq<float> {
  static __device__ __forceinline__ float of(int d, float s) { const float sd = s * (float)d; return sd * sd; }
  static __device__ __forceinline__ float word(u32 w) { return __uint_as_float(w); }
};

__global__ void __launch_bounds__(kBlock)
k_surface_dice_clear(int64_t* __restrict__ surface_voxels, int64_t* __restrict__ within, int64_t* __restrict__ overlap, int64_t NK) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < 2 * NK) surface_voxels[i] = within[i] = 0;
  if (overlap && i < 3 * NK) overlap[i] = 0;
}

// a border voxel of class `cls` of the other map (its half of a word at `shift`) within `thr` of cell `at`
template <typename T>
__device__ __forceinline__ bool ball_find(const u32* __restrict__ w, int at, u32 cls, int shift, T thr, const BallGeom& g) {
  const int sxy = g.lx * g.ly;
  for (int az = 0; az <= g.c[0]; ++az) {
    const T fz = Bsq<T>::of(az, g.s[0]);
    if (!(fz <= thr)) break;
    for (int sz = 0; sz < (az ? 2 : 1); ++sz) {
      const int pz = at + (sz ? -az : az) * sxy;
      for (int ay = 0; ay <= g.c[1]; ++ay) {
        const T fy = Bsq<T>::of(ay, g.s[1]);
        if (!(fy + fz <= thr)) break;
        for (int sy = 0; sy < (ay ? 2 : 1); ++sy) {
          const int py = pz + (sy ? -ay : ay) * g.lx;
          for (int ax = 0; ax <= g.c[2]; ++ax) {
            const T fx = Bsq<T>::of(ax, g.s[2]);
            if (!((fx + fy) + fz <= thr)) break;             // (the order of the transform's additions: x, then y, then z)
            if (((w[py + ax] >> shift) & 0xffffu) == cls) return true;
            if (((w[py - ax] >> shift) & 0xffffu) == cls) return true;
          }
        }
      }
    }
  }
  return false;
}

// blockIdx.x = ((n tiles_z + z tile) tiles_y + y tile) tiles_x + x tile
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_surface_ball(const int64_t* __restrict__ pred, const int64_t* __restrict__ target, const u32* __restrict__ thr,
               int64_t* surface_voxels, int64_t* within, int K, int D, int H, int W, BallGeom g) {
  extern __shared__ __align__(16) unsigned char ball_lds[];
  __shared__ u32 counts[kBallClasses * 4];
  const int LX = g.lx, LY = g.ly, cells = g.lz * LY * LX;
  u32* w = reinterpret_cast<u32*>(ball_lds);
  unsigned char* flag = ball_lds + (size_t)cells * 4;
  int64_t b = blockIdx.x;
  const int bx = (int)(b % g.tiles_x); b /= g.tiles_x;
  const int by = (int)(b % g.tiles_y); b /= g.tiles_y;
  const int bz = (int)(b % g.tiles_z);
  const int64_t n = b / g.tiles_z, V = (int64_t)D * H * W;
  const int z0 = bz * g.tz, y0 = by * g.ty, x0 = bx * g.tx;

  for (int i = threadIdx.x; i < cells; i += kBlock) {
    const int lx = i % LX, ly = (i / LX) % LY, lz = i / (LX * LY);
    const int64_t z = (int64_t)z0 + lz - g.h[0], y = (int64_t)y0 + ly - g.h[1], x = (int64_t)x0 + lx - g.h[2];
    u32 a = kHalfOutside, c = kHalfOutside;
    if (z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W) {
      const int64_t at = n * V + (z * H + y) * W + x;
      const int ka = class_of(pred[at], K), kc = class_of(target[at], K);
      a = ka < 0 ? kHalfNone : (u32)ka;
      c = kc < 0 ? kHalfNone : (u32)kc;
    }
    w[i] = a | (c << 16);
  }
  __syncthreads();

  // the border predicate for every cell but the outermost layer of the tiled axes
  const int IX = LX - 2, IY = LY - 2, IZ = g.nd == 3 ? g.lz - 2 : 1, oz = g.nd == 3 ? 1 : 0, inner = IZ * IY * IX;
  for (int i = threadIdx.x; i < inner; i += kBlock) {
    const int at = ((i / (IX * IY) + oz) * LY + (i / IX) % IY + 1) * LX + i % IX + 1;
    const u32 v = w[at], a = v & 0xffffu, c = v >> 16;
    const u32 l = w[at - 1], r = w[at + 1], u = w[at - LX], d = w[at + LX];
    bool ea = (l & 0xffffu) != a || (r & 0xffffu) != a || (u & 0xffffu) != a || (d & 0xffffu) != a;
    bool ec = (l >> 16) != c || (r >> 16) != c || (u >> 16) != c || (d >> 16) != c;
    if (g.nd == 3) {
      const u32 f = w[at - LX * LY], k = w[at + LX * LY];
      ea = ea || (f & 0xffffu) != a || (k & 0xffffu) != a;
      ec = ec || (f >> 16) != c || (k >> 16) != c;
    }
    flag[at] = (unsigned char)((ea && a < kHalfOutside ? 1 : 0) | (ec && c < kHalfOutside ? 2 : 0));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < inner; i += kBlock) {
    const int at = ((i / (IX * IY) + oz) * LY + (i / IX) % IY + 1) * LX + i % IX + 1;
    const u32 v = w[at], f = flag[at];
    w[at] = ((f & 1u) ? (v & 0xffffu) : kHalfNone) | (((f & 2u) ? (v >> 16) : kHalfNone) << 16);
  }

  const int own = g.tz * g.ty * g.tx;
  for (int g0 = 0; g0 < K; g0 += kBallClasses) {
    for (int i = threadIdx.x; i < kBallClasses * 4; i += kBlock) counts[i] = 0u;
    __syncthreads();                                     // (the first time: also the barrier behind the edge words)
    for (int i = threadIdx.x; i < own; i += kBlock) {
      const int tx = i % g.tx, ty = (i / g.tx) % g.ty, tz = i / (g.tx * g.ty);
      if (z0 + tz >= D || y0 + ty >= H || x0 + tx >= W) continue;
      const int at = ((tz + g.h[0]) * LY + ty + g.h[1]) * LX + tx + g.h[2];
      const u32 v = w[at], a = v & 0xffffu, c = v >> 16;
      if (a != kHalfNone && (int)a >= g0 && (int)a < g0 + kBallClasses) {
        u32* q = counts + ((int)a - g0) * 4;
        atomicAdd(q + 0, 1u);
        if (ball_find<T>(w, at, a, 16, Bsq<T>::word(thr[a]), g)) atomicAdd(q + 2, 1u);
      }
      if (c != kHalfNone && (int)c >= g0 && (int)c < g0 + kBallClasses) {
        u32* q = counts + ((int)c - g0) * 4;
        atomicAdd(q + 1, 1u);
        if (ball_find<T>(w, at, c, 0, Bsq<T>::word(thr[c]), g)) atomicAdd(q + 3, 1u);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBallClasses * 4; i += kBlock) {
      const int kk = g0 + i / 4, f = i % 4;
      const u32 v = counts[i];
      if (kk < K && v) {
        int64_t* o = (f < 2 ? surface_voxels : within) + (n * K + kk) * 2 + (f & 1);
        atomicAdd(reinterpret_cast<u64*>(o), (u64)v);
      }
    }
    __syncthreads();
  }
}

// the field route's count: blockIdx = (chunk, n, direction) as k_surface_digits
__global__ void __launch_bounds__(kBlock)
k_surface_within(const int64_t* __restrict__ edges, const u32* __restrict__ fields, const u32* __restrict__ thr, int64_t* within,
                 int64_t N, int K, int64_t V, int64_t per) {
  __shared__ u32 counts[kCountClasses];
  const Chunk ch = chunk_of(edges, fields, N, K, V, per);
  const int64_t n = blockIdx.y, d = blockIdx.z;
  for (int g0 = 0; g0 < K; g0 += kCountClasses) {
    for (int i = threadIdx.x; i < kCountClasses; i += kBlock) counts[i] = 0u;
    __syncthreads();
    for (int64_t v = ch.begin + threadIdx.x; v < ch.end; v += kBlock) {
      const int64_t e = ch.edge[v];
      if (e < g0 || e >= g0 + kCountClasses) continue;
      if (ch.field[e * V + v] <= thr[e]) atomicAdd(&counts[(int)e - g0], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kCountClasses; i += kBlock) {
      const u32 c = counts[i];
      if (g0 + i < K && c) atomicAdd(reinterpret_cast<u64*>(within + (n * K + g0 + i) * 2 + d), (u64)c);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlock)
k_surface_dice_finish(const int64_t* __restrict__ surface_voxels, const int64_t* __restrict__ within, float* __restrict__ out,
                      int64_t NK) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= NK) return;
  const int64_t m = surface_voxels[2 * i] + surface_voxels[2 * i + 1], c = within[2 * i] + within[2 * i + 1];
  out[i] = m == 0 ? (float)NAN : (float)((double)c / (double)m);
}

const int kBallTiles2[][3] = {{1, 32, 64}, {1, 16, 64}, {1, 8, 64}};
const int kBallTiles3[][3] = {{8, 8, 32}, {4, 8, 32}, {4, 4, 32}, {2, 4, 32}, {2, 2, 32}};

float host_sq(int d, float s) {                  // Bsq<float>::of on the host (this file is compiled without contraction)
  const float sd = s * (float)d;
  return sd * sd;
}

// The arguments every route needs: 0, or ADVCHAIN_ERR_ARG with the error set.  d = (D, H, W), s the spacing of those axes.
int dice_args(int64_t N, int64_t K, int ndim, const int64_t* dims, const float* sampling, double tolerance_max, int route,
              int64_t (&d)[3], float (&s)[3]) {
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "surface_dice: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(N >= 1, "surface_dice: bad N");
  ADVCHAIN_CHECK_ARG(dims && (ndim == 2 || ndim == 3), "surface_dice: bad ndim or dims");
  for (int a = 0; a < ndim; ++a) ADVCHAIN_CHECK_ARG(dims[a] >= 1, "surface_dice: bad ndim or dims");
  ADVCHAIN_CHECK_ARG(tolerance_max >= 0.0 && tolerance_max <= 1.79769313486231570e308,
                     "surface_dice: the tolerance must be finite and not negative");
  ADVCHAIN_CHECK_ARG(route >= DICE_ROUTE_ANY && route <= DICE_ROUTE_FIELDS, "surface_dice: route is 0 (dispatch), 1 (ball) or 2 (fields)");
  d[0] = ndim == 3 ? dims[0] : 1;
  d[1] = dims[ndim - 2];
  d[2] = dims[ndim - 1];
  s[0] = s[1] = s[2] = 1.f;
  for (int a = 0; sampling && a < ndim; ++a) {
    const float v = sampling[a];
    ADVCHAIN_CHECK_ARG(v > 0.f && v <= 3.40282347e38f && (double)v * v >= 1.0e-30,
                       "surface_dice: sampling must be positive and finite (and the physical diagonal below 1e14)");
    s[3 - ndim + a] = v;
  }
  return ADVCHAIN_OK;
}

// the ball route's tile for these caps, or false where it is not eligible
bool ball_geometry(int64_t N, int64_t K, int ndim, const int64_t (&d)[3], const float (&s)[3], bool unit, double tolerance_max,
                   BallGeom* g) {
  if (K > kBallMaxK) return false;
  const double t2 = tolerance_max * tolerance_max;
  const int64_t T = t2 >= (double)(kEdtFieldInf - 1) ? kEdtFieldInf - 1 : (int64_t)floor(t2);
  const float tf = t2 >= 1.0e29 ? 1.0e29f : (float)t2;
  g->nd = ndim;
  for (int a = 0; a < 3; ++a) {
    g->s[a] = s[a];
    int64_t c = 0;
    if (a >= 3 - ndim) {
      if (unit) {
        c = (int64_t)sqrt((double)T);
        while (c * c > T) --c;
        while ((c + 1) * (c + 1) <= T) ++c;
      } else {
        const double q = floor(tolerance_max / (double)s[a]);
        c = q >= 65536.0 ? 65536 : (int64_t)q;
        while (c < 65536 && host_sq((int)c + 1, s[a]) <= tf) ++c;
        while (c > 0 && !(host_sq((int)c, s[a]) <= tf)) --c;
      }
      if (c > d[a] - 1) c = d[a] - 1;                   // (an offset of the whole axis leaves the image)
      if (c > 4096) return false;
    }
    g->c[a] = (int)c;
    g->h[a] = a >= 3 - ndim ? (int)c + 1 : 0;
  }
  const int (*tiles)[3] = ndim == 3 ? kBallTiles3 : kBallTiles2;
  const int count = ndim == 3 ? 5 : 3;
  for (int t = 0; t < count; ++t) {
    const int64_t lz = tiles[t][0] + 2 * g->h[0], ly = tiles[t][1] + 2 * g->h[1], lx = tiles[t][2] + 2 * g->h[2];
    const int64_t cells = lz * ly * lx;
    if (cells * 4 + ((cells + 3) & ~(int64_t)3) > kBallLdsBytes) continue;
    g->tz = tiles[t][0];
    g->ty = tiles[t][1];
    g->tx = tiles[t][2];
    g->lz = (int)lz;
    g->ly = (int)ly;
    g->lx = (int)lx;
    const int64_t nz = (d[0] + g->tz - 1) / g->tz, ny = (d[1] + g->ty - 1) / g->ty, nx = (d[2] + g->tx - 1) / g->tx;
    if (d[0] > 0x7fffffff || d[1] > 0x7fffffff || d[2] > 0x7fffffff || nz * ny > 0x7fffffff || nz * ny * nx > 0x7fffffff ||
        N > 0x7fffffff / (nz * ny * nx) || N > ((int64_t)1 << 36) / K)
      return false;
    if ((double)d[0] * (double)d[1] * (double)d[2] * (double)N >= 9.0e18) return false;
    g->tiles_z = (int)nz;
    g->tiles_y = (int)ny;
    g->tiles_x = (int)nx;
    return true;
  }
  return false;
}

bool fields_plan(int64_t N, int64_t K, int ndim, const int64_t* dims, const float* sampling, SurfacePlan* p) {
  if (N > 65535 || N > ((int64_t)1 << 36) / K || !surface_plan(N, K, ndim, dims, p)) return false;
  const int64_t tz = ndim == 3 ? 4 : 1, ty = ndim == 3 ? 8 : 32, D = ndim == 3 ? dims[0] : 1;
  const int64_t tiles = ((D + tz - 1) / tz) * ((dims[ndim - 2] + ty - 1) / ty) * ((dims[ndim - 1] + kEdgeTX - 1) / kEdgeTX);
  if (N * tiles > 0x7fffffff) return false;
  int64_t d[3];
  float s[3];
  return edt_fields_check(sampling, 2 * N, K, ndim, dims, "surface_dice", d, s) == ADVCHAIN_OK;
}

// DICE_ROUTE_BALL or DICE_ROUTE_FIELDS, or ADVCHAIN_ERR_UNSUPPORTED with the error set
int dice_route(int64_t N, int64_t K, int ndim, const int64_t* dims, const float* sampling, double tolerance_max, int route,
               const int64_t (&d)[3], const float (&s)[3], BallGeom* g, SurfacePlan* p) {
  const bool ball = ball_geometry(N, K, ndim, d, s, sampling == nullptr, tolerance_max, g);
  const bool fields = fields_plan(N, K, ndim, dims, sampling, p);
  if (route == DICE_ROUTE_BALL) {
    if (ball) return DICE_ROUTE_BALL;
    advchain_set_error_("surface_dice: the ball route is not eligible (the tile with a halo of cap + 1 voxels does not fit in LDS, "
                        "K above 65534, or too many tiles)");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  if (route == DICE_ROUTE_ANY && ball) {
    const int top = g->c[0] > g->c[1] ? (g->c[0] > g->c[2] ? g->c[0] : g->c[2]) : (g->c[1] > g->c[2] ? g->c[1] : g->c[2]);
    if (top <= (ndim == 3 ? kBallDispatchCap3 : kBallDispatchCap2) || !fields) return DICE_ROUTE_BALL;
  }
  if (fields) return DICE_ROUTE_FIELDS;
  advchain_set_error_("surface_dice: shape too large for the distance fields (an axis or the squared diagonal)");
  return ADVCHAIN_ERR_UNSUPPORTED;
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

int advchain_surface_dice_route(int64_t N, int64_t K, int ndim, const int64_t* dims, const float* sampling, double tolerance_max,
                                int route) {
  int64_t d[3];
  float s[3];
  const int rc = dice_args(N, K, ndim, dims, sampling, tolerance_max, route, d, s);
  if (rc != ADVCHAIN_OK) return rc;
  BallGeom g;
  SurfacePlan p;
  return dice_route(N, K, ndim, dims, sampling, tolerance_max, route, d, s, &g, &p);
}

int64_t advchain_surface_dice_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims, const float* sampling,
                                        double tolerance_max, int route) {
  int64_t d[3];
  float s[3];
  if (dice_args(N, K, ndim, dims, sampling, tolerance_max, route, d, s) != ADVCHAIN_OK) return -1;
  BallGeom g;
  SurfacePlan p;
  const int r = dice_route(N, K, ndim, dims, sampling, tolerance_max, route, d, s, &g, &p);
  if (r < 0) return -1;
  return r == DICE_ROUTE_BALL ? 0 : p.w_fields + p.w_edges + 6 * N * K;
}

int advchain_surface_dice(const int64_t* pred, const int64_t* target, const float* sampling, const void* thresholds,
                          double tolerance_max, int route, float* surface_dice, int64_t* within, int64_t* surface_voxels,
                          void* workspace, int64_t N, int64_t K, int ndim, const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(pred && target && thresholds && surface_dice && within && surface_voxels, "surface_dice: null pointer");
  int64_t d[3];
  float s[3];
  int rc = dice_args(N, K, ndim, dims, sampling, tolerance_max, route, d, s);
  if (rc != ADVCHAIN_OK) return rc;
  BallGeom g;
  SurfacePlan p;
  const int r = dice_route(N, K, ndim, dims, sampling, tolerance_max, route, d, s, &g, &p);
  if (r < 0) return r;
  hipStream_t st = (hipStream_t)stream;
  const u32* thr = (const u32*)thresholds;
  const int64_t NK = N * K;
  const unsigned flat = (unsigned)((3 * NK + kBlock - 1) / kBlock);
  const int D = (int)d[0], H = (int)d[1], W = (int)d[2];

  if (r == DICE_ROUTE_BALL) {
    hipLaunchKernelGGL(k_surface_dice_clear, dim3(flat), dim3(kBlock), 0, st, surface_voxels, within, (int64_t*)nullptr, NK);
    ADVCHAIN_LAUNCH_CHECK();
    const int64_t cells = (int64_t)g.lz * g.ly * g.lx;
    const size_t lds = (size_t)(cells * 4 + ((cells + 3) & ~(int64_t)3));
    const unsigned blocks = (unsigned)(N * g.tiles_z * g.tiles_y * g.tiles_x);
    if (sampling)
      hipLaunchKernelGGL(k_surface_ball<float>, dim3(blocks), dim3(kBlock), lds, st, pred, target, thr, surface_voxels, within,
                         (int)K, D, H, W, g);
    else
      hipLaunchKernelGGL(k_surface_ball<int>, dim3(blocks), dim3(kBlock), lds, st, pred, target, thr, surface_voxels, within,
                         (int)K, D, H, W, g);
    ADVCHAIN_LAUNCH_CHECK();
  } else {
    ADVCHAIN_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0, "surface_dice: workspace must be 16-byte aligned and not null");
    u32* w = (u32*)workspace;
    u32* fields = w;                              w += p.w_fields;
    int64_t* edges = (int64_t*)w;                 w += p.w_edges;
    int64_t* overlap = (int64_t*)w;
    hipLaunchKernelGGL(k_surface_dice_clear, dim3(flat), dim3(kBlock), 0, st, surface_voxels, within, overlap, NK);
    ADVCHAIN_LAUNCH_CHECK();
    const int hz = ndim == 3 ? 1 : 0, TZ = hz ? 4 : 1, TY = hz ? 8 : 32;
    const int64_t tiles_z = (D + TZ - 1) / TZ, tiles_y = (H + TY - 1) / TY, tiles_x = (W + kEdgeTX - 1) / kEdgeTX;
    const size_t lds = (size_t)(TZ + 2 * hz) * (TY + 2) * (kEdgeTX + 2) * 2 * sizeof(int);
    hipLaunchKernelGGL(k_surface_edges, dim3((unsigned)(N * tiles_z * tiles_y * tiles_x)), dim3(kBlock), lds, st, pred, target, edges,
                       edges + N * p.V, surface_voxels, overlap, (int)K, D, H, W, hz, TZ, TY, (int)tiles_z, (int)tiles_y,
                       (int)tiles_x);
    ADVCHAIN_LAUNCH_CHECK();
    rc = edt_label_fields(edges, sampling, fields, 2 * N, K, ndim, dims, "surface_dice", st);
    if (rc != ADVCHAIN_OK) return rc;
    hipLaunchKernelGGL(k_surface_within, dim3((unsigned)p.chunks, (unsigned)N, 2), dim3(kBlock), 0, st, (const int64_t*)edges,
                       (const u32*)fields, thr, within, N, (int)K, p.V, p.per);
    ADVCHAIN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_surface_dice_finish, dim3((unsigned)((NK + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     (const int64_t*)surface_voxels, (const int64_t*)within, surface_dice, NK);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
