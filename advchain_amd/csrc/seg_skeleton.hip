// Soft skeletons of probability maps and the soft-clDice loss (Shit et al., CVPR 2021), 2D and 3D, for gfx950:
//
//   advchain_soft_skeleton_fwd / _bwd   <- common.loss.soft_skeletonize
//   advchain_cldice_fwd / _bwd          <- common.loss.cldice_loss
//
// With E the minimum over a voxel and its in-image face neighbours, D the maximum over the in-image 3x3(x3) box and O = D E:
//   x_0 = x,  x_{j+1} = E(x_j),  delta_j = relu(x_j - D(x_{j+1})),  skel_0 = delta_0,
//   skel_j = skel_{j-1} + relu(delta_j - skel_{j-1} delta_j)     (j = 1..iterations), every operation rounded once (the file
// is compiled without contraction, build.py): the bits of the published max_pool composition in fp32.
//
// Two forward routes with the same arithmetic and the same bits:
//   fused   k_skel_tile, iterations <= kFusedMax: a workgroup stages one tile of one plane with a halo of iterations + 2 in LDS
//           (2D 32 x 64, 3D 8 x 8 x 32 voxels; a softmax or one-hot source is evaluated as the tile is staged) and runs the whole
//           chain there, two LDS arrays swapping roles; the rim goes stale by one cell per erosion and never reaches the tile.
//   levels  on global arrays, any iteration count: k_skel_erode (x_1), then one k_skel_level per level, which also writes
//           x_{j+2} = E(x_{j+1}) for the next one (both read the neighbourhood of x_{j+1}): iterations + 2 launches, two arrays.
// The backward is in gather form, level by level, for every iteration count: the erosion chain is recomputed into the
// caller's workspace with a 1-byte selection code per voxel and level (k_skel_erode<true>), k_skel_point replays the pointwise
// recurrence (the dilations' codes, h_j = dL/d delta_j where delta_j > 0), then per level, last to first,
//   k_skel_bwd   G_j(u)      = h_j(u) + sum of ge_j(v) over the cross neighbours v whose erosion selected u
//                ge_{j-1}(u) = G_j(u) - sum of h_{j-1}(v) over the box neighbours v whose dilation selected u
// (one launch per level: 2 iterations + 4 launches in all) in a fixed order: no atomics, equal bits on every run.  Ties: the first in the order centre, axis by axis minus before plus
// (E) / centre, raster order of the box (D) wins; relu'(0) = 0.
//
// The loss: lse per voxel (k_cl_lse), S^p = skel(softmax) and S^t = skel(target), k_cl_sums (four sums per (workgroup, n, k)),
// k_cl_reduce (fixed order), k_cl_finish (value and the table A, B, C of the backward).  Backward: skeleton backward of
// m (A t + B), plus m C S^t, through the softmax (k_cl_softmax_bwd), rounded once to the logits' dtype.
#include <math.h>

#include "common.h"
#include "seg_common.h"

namespace advchain {
namespace {

constexpr int kMaxIter = 32;                 // ADVCHAIN_SKELETON_MAX_ITERATIONS
constexpr int kFusedMax = 4;                 // ADVCHAIN_SKELETON_FUSED_MAX

enum { SRC_MAP = 0, SRC_SOFTMAX_F32 = 1, SRC_SOFTMAX_BF16 = 2, SRC_ONEHOT = 3 };
enum { ROUTE_AUTO = 0, ROUTE_FUSED = 1, ROUTE_LEVELS = 2 };
enum { CLDICE_IGNORE_BACKGROUND = 1, CLDICE_BATCH = 2 };

// where the maps of a chain come from: fp32 maps (N,K,V), softmax of logits given lse (N,V), or one-hot of labels (N,V)
struct Src {
  const void* base;
  const float* lse;
  const int64_t* lab;
  int kind, K;
};

struct Geo {
  int s0, s1, s2;      // s0 == 1 for 2D
  int64_t V;
};

__device__ __forceinline__ float src_at(const Src& s, int64_t n, int k, int64_t V, int64_t v) {
  switch (s.kind) {                                                   // (uniform)
    case SRC_MAP: return ((const float*)s.base)[(n * s.K + k) * V + v];
    case SRC_SOFTMAX_F32: return __expf(ld1<float>((const float*)s.base + (n * s.K + k) * V + v) - s.lse[n * V + v]);
    case SRC_SOFTMAX_BF16:
      return __expf(ld1<unsigned short>((const unsigned short*)s.base + (n * s.K + k) * V + v) - s.lse[n * V + v]);
    default: return s.lab[n * V + v] == (int64_t)k ? 1.f : 0.f;
  }
}

__device__ __forceinline__ void coords(const Geo& g, int64_t v, int& z, int& y, int& x) {
  const int64_t r = v / g.s2;
  x = (int)(v - r * g.s2);
  z = (int)(r / g.s1);
  y = (int)(r - (int64_t)z * g.s1);
}

// offset (dz, dy, dx) of an erosion code 1..6: z-, z+, y-, y+, x-, x+
__device__ __forceinline__ void cross_offset(int c, int& dz, int& dy, int& dx) {
  dz = c == 1 ? -1 : (c == 2 ? 1 : 0);
  dy = c == 3 ? -1 : (c == 4 ? 1 : 0);
  dx = c == 5 ? -1 : (c == 6 ? 1 : 0);
}

// maximum of plane `a` over the in-image box of v; code 0: the centre, 1 + raster index of the box otherwise (first wins)
__device__ __forceinline__ float box_max(const float* __restrict__ a, const Geo& g, int z, int y, int x, int64_t v, int& code) {
  float best = a[v];
  code = 0;
  for (int dz = -1; dz <= 1; ++dz) {
    if (z + dz < 0 || z + dz >= g.s0) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      if (y + dy < 0 || y + dy >= g.s1) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (x + dx < 0 || x + dx >= g.s2) continue;
        const float val = a[v + ((int64_t)dz * g.s1 + dy) * g.s2 + dx];
        if (val > best) { best = val; code = 1 + (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }
      }
    }
  }
  return best;
}

__device__ __forceinline__ float relu(float a) { return a > 0.f ? a : 0.f; }

// ---- level-by-level route ----------------------------------------------------------------------------------------------
// out = E(src); grid (V / 256, K, N)
template <bool SEL>
__global__ void __launch_bounds__(kBlock)
k_skel_erode(Src src, float* __restrict__ out, unsigned char* __restrict__ sel, Geo g) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.V) return;
  const int k = blockIdx.y;
  const int64_t n = blockIdx.z;
  int z, y, x;
  coords(g, v, z, y, x);
  float best = src_at(src, n, k, g.V, v);
  int code = 0;
  const int64_t sy = g.s2, sz = (int64_t)g.s1 * g.s2;
#define ADVCHAIN_TRY(ok, off, c)                                      \
  if (ok) {                                                           \
    const float val = src_at(src, n, k, g.V, v + (off));              \
    if (val < best) { best = val; code = c; }                         \
  }
  ADVCHAIN_TRY(z > 0, -sz, 1)
  ADVCHAIN_TRY(z + 1 < g.s0, sz, 2)
  ADVCHAIN_TRY(y > 0, -sy, 3)
  ADVCHAIN_TRY(y + 1 < g.s1, sy, 4)
  ADVCHAIN_TRY(x > 0, -1, 5)
  ADVCHAIN_TRY(x + 1 < g.s2, 1, 6)
#undef ADVCHAIN_TRY
  const int64_t i = (n * src.K + k) * g.V + v;
  out[i] = best;
  if constexpr (SEL) sel[i] = (unsigned char)code;
}

// skel <- skel + relu(delta - skel delta), delta = relu(x_j - D(x_{j+1})); first: skel = delta.  With `next`, x_{j+2} =
// E(x_{j+1}) of the same voxel goes there: both read the neighbourhood of x_{j+1}.  `next` may be the array x_j lives in (a
// lane reads x_j at its own voxel only, before it writes), so the chain needs two arrays.
__global__ void __launch_bounds__(kBlock)
k_skel_level(Src xj, const float* xj1, float* __restrict__ skel, float* next, Geo g, int first) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.V) return;
  const int k = blockIdx.y;
  const int64_t n = blockIdx.z;
  int z, y, x, code;
  coords(g, v, z, y, x);
  const int64_t plane = (n * xj.K + k) * g.V;
  const float o = box_max(xj1 + plane, g, z, y, x, v, code);
  const float d = relu(src_at(xj, n, k, g.V, v) - o);
  if (next) {
    const float* a = xj1 + plane;
    const int64_t sy = g.s2, sz = (int64_t)g.s1 * g.s2;
    float best = a[v];
    if (z > 0) best = fminf(best, a[v - sz]);
    if (z + 1 < g.s0) best = fminf(best, a[v + sz]);
    if (y > 0) best = fminf(best, a[v - sy]);
    if (y + 1 < g.s1) best = fminf(best, a[v + sy]);
    if (x > 0) best = fminf(best, a[v - 1]);
    if (x + 1 < g.s2) best = fminf(best, a[v + 1]);
    next[plane + v] = best;
  }
  if (first) {
    skel[plane + v] = d;
  } else {
    const float s = skel[plane + v];
    const float m = s * d;
    skel[plane + v] = s + relu(d - m);
  }
}

// ---- fused route: the chain of one tile in LDS ------------------------------------------------------------------------
struct Tile {
  int tz, ty, tx;      // voxels of a tile
  int hz, h;           // halo along z (0 in 2D) and along y, x
  int ntx, nty;        // tiles along x and y
};

__global__ void __launch_bounds__(kBlock)
k_skel_tile(Src src, float* __restrict__ out, Geo g, Tile t, int iters) {
  extern __shared__ float lds[];
  const int ez = t.tz + 2 * t.hz, ey = t.ty + 2 * t.h, ex = t.tx + 2 * t.h;
  const int E = ez * ey * ex, inner = t.tz * t.ty * t.tx;
  float* A = lds;
  float* B = lds + E;
  float* S = lds + 2 * E;
  const int k = blockIdx.y;
  const int64_t n = blockIdx.z;
  const int bx = blockIdx.x % t.ntx, by = (blockIdx.x / t.ntx) % t.nty, bz = blockIdx.x / (t.ntx * t.nty);
  const int oz = bz * t.tz - t.hz, oy = by * t.ty - t.h, ox = bx * t.tx - t.h;      // image coordinates of the staged corner

  for (int i = threadIdx.x; i < E; i += kBlock) {
    const int lx = i % ex, r = i / ex, ly = r % ey, lz = r / ey;
    const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
    const bool in = gz >= 0 && gz < g.s0 && gy >= 0 && gy < g.s1 && gx >= 0 && gx < g.s2;
    A[i] = in ? src_at(src, n, k, g.V, ((int64_t)gz * g.s1 + gy) * g.s2 + gx) : 0.f;
  }
  __syncthreads();

  for (int j = 0; j <= iters; ++j) {
    for (int i = threadIdx.x; i < E; i += kBlock) {                   // B = E(A); a neighbour counts when staged and in the image
      const int lx = i % ex, r = i / ex, ly = r % ey, lz = r / ey;
      const int gz = oz + lz, gy = oy + ly, gx = ox + lx;
      float best = A[i];
      if (lz > 0 && gz > 0) best = fminf(best, A[i - ey * ex]);
      if (lz + 1 < ez && gz + 1 < g.s0) best = fminf(best, A[i + ey * ex]);
      if (ly > 0 && gy > 0) best = fminf(best, A[i - ex]);
      if (ly + 1 < ey && gy + 1 < g.s1) best = fminf(best, A[i + ex]);
      if (lx > 0 && gx > 0) best = fminf(best, A[i - 1]);
      if (lx + 1 < ex && gx + 1 < g.s2) best = fminf(best, A[i + 1]);
      B[i] = best;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < inner; c += kBlock) {               // (a cell belongs to the same lane at every level)
      const int ix = c % t.tx, r = c / t.tx, iy = r % t.ty, iz = r / t.ty;
      const int gz = oz + t.hz + iz, gy = oy + t.h + iy, gx = ox + t.h + ix;
      if (gz >= g.s0 || gy >= g.s1 || gx >= g.s2) continue;
      const int i = ((iz + t.hz) * ey + iy + t.h) * ex + ix + t.h;
      float o = B[i];
      for (int dz = -1; dz <= 1; ++dz) {
        if (gz + dz < 0 || gz + dz >= g.s0) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          if (gy + dy < 0 || gy + dy >= g.s1) continue;
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            if (gx + dx < 0 || gx + dx >= g.s2) continue;
            o = fmaxf(o, B[i + (dz * ey + dy) * ex + dx]);
          }
        }
      }
      const float d = relu(A[i] - o);
      if (j == 0) {
        S[c] = d;
      } else {
        const float s = S[c];
        const float m = s * d;
        S[c] = s + relu(d - m);
      }
    }
    __syncthreads();
    float* T = A; A = B; B = T;
  }

  const int64_t plane = (n * src.K + k) * g.V;
  for (int c = threadIdx.x; c < inner; c += kBlock) {
    const int ix = c % t.tx, r = c / t.tx, iy = r % t.ty, iz = r / t.ty;
    const int gz = oz + t.hz + iz, gy = oy + t.h + iy, gx = ox + t.h + ix;
    if (gz >= g.s0 || gy >= g.s1 || gx >= g.s2) continue;
    out[plane + ((int64_t)gz * g.s1 + gy) * g.s2 + gx] = S[c];
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// The pointwise recurrence of one voxel, replayed: writes the dilation's code and h_j = dL/d delta_j (0 where delta_j == 0) of
// every level.  chain[j] = x_{j+1}.  The cotangent is grad (N,K,V) or, for the loss, m (A_nk t + B_nk).  NI > iterations.
template <int NI>
__global__ void __launch_bounds__(kBlock)
k_skel_point(Src x0, const float* __restrict__ chain, const float* __restrict__ grad, const float* __restrict__ coef, Src tsrc,
             const int64_t* __restrict__ mask_lab, float* __restrict__ h, unsigned char* __restrict__ seld, Geo g, int iters,
             int64_t PV) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.V) return;
  const int k = blockIdx.y;
  const int64_t n = blockIdx.z;
  int z, y, x;
  coords(g, v, z, y, x);
  const int64_t plane = (n * x0.K + k) * g.V, i = plane + v;
  float d[NI], sp[NI];                                                // delta_j and skel_{j-1}
  float skel = 0.f;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    d[j] = 0.f;
    sp[j] = 0.f;
    if (j <= iters) {
      int code;
      const float o = box_max(chain + (int64_t)j * PV + plane, g, z, y, x, v, code);
      seld[(int64_t)j * PV + i] = (unsigned char)code;
      const float xj = j == 0 ? src_at(x0, n, k, g.V, v) : chain[(int64_t)(j - 1) * PV + i];
      d[j] = relu(xj - o);
      sp[j] = skel;
      skel = j == 0 ? d[0] : skel + relu(d[j] - skel * d[j]);
    }
  }
  float G;
  if (coef) {
    const bool live = !mask_lab || mask_lab[n * g.V + v] != -100;
    const float* cf = coef + (n * x0.K + k) * 3;
    G = live ? cf[0] * src_at(tsrc, n, k, g.V, v) + cf[1] : 0.f;
  } else {
    G = grad[i];
  }
#pragma unroll
  for (int j = NI - 1; j >= 1; --j) {
    if (j <= iters) {
      const float a = d[j] - sp[j] * d[j];
      const float Gr = a > 0.f ? G : 0.f;
      const float gd = Gr - Gr * sp[j];
      G = G - Gr * d[j];
      h[(int64_t)j * PV + i] = d[j] > 0.f ? gd : 0.f;
    }
  }
  h[i] = d[0] > 0.f ? G : 0.f;
}

// acc - sum of h(v) over the box neighbours v (u itself included) whose dilation selected u
__device__ __forceinline__ float gather_d(float acc, const float* __restrict__ hp, const unsigned char* __restrict__ sp,
                                          const Geo& g, int z, int y, int x, int64_t u) {
  if (sp[u] == 0) acc -= hp[u];
  for (int dz = -1; dz <= 1; ++dz) {
    if (z - dz < 0 || z - dz >= g.s0) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      if (y - dy < 0 || y - dy >= g.s1) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (x - dx < 0 || x - dx >= g.s2) continue;
        const int64_t v = u - (((int64_t)dz * g.s1 + dy) * g.s2 + dx);          // v + (dz, dy, dx) == u
        if (sp[v] == 1 + (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)) acc -= hp[v];
      }
    }
  }
  return acc;
}

// acc + sum of ge(v) over the cross neighbours v (u itself included) whose erosion selected u
__device__ __forceinline__ float gather_e(float acc, const float* __restrict__ gp, const unsigned char* __restrict__ sp,
                                          const Geo& g, int z, int y, int x, int64_t u) {
  if (sp[u] == 0) acc += gp[u];
#pragma unroll
  for (int c = 1; c <= 6; ++c) {
    int dz, dy, dx;
    cross_offset(c, dz, dy, dx);
    const int vz = z - dz, vy = y - dy, vx = x - dx;
    if (vz < 0 || vz >= g.s0 || vy < 0 || vy >= g.s1 || vx < 0 || vx >= g.s2) continue;
    const int64_t v = ((int64_t)vz * g.s1 + vy) * g.s2 + vx;
    if (sp[v] == c) acc += gp[v];
  }
  return acc;
}

// One step of the backward at voxel u: G(u) = h_e(u) + erosion gather of ge_in (level j; without ge_in: G = 0, the last level has
// nothing above it), then out(u) = G(u) - dilation gather of h_d (level j - 1; without h_d: out = G, the gradient of x_0).
__global__ void __launch_bounds__(kBlock)
k_skel_bwd(const float* __restrict__ ge_in, const float* __restrict__ h_e, const unsigned char* __restrict__ sele,
           const float* __restrict__ h_d, const unsigned char* __restrict__ seld, float* __restrict__ out, Geo g, int K) {
  const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u >= g.V) return;
  const int64_t plane = ((int64_t)blockIdx.z * K + blockIdx.y) * g.V;
  int z, y, x;
  coords(g, u, z, y, x);
  float acc = 0.f;
  if (ge_in) acc = gather_e(h_e[plane + u], ge_in + plane, sele + plane, g, z, y, x, u);
  if (h_d) acc = gather_d(acc, h_d + plane, seld + plane, g, z, y, x, u);
  out[plane + u] = acc;
}

// ---- the loss ------------------------------------------------------------------------------------------------------------
// lse(n, v) of the K logits (the online form of seg_dice.hip); grid (V / 256, N)
template <typename ST>
__global__ void __launch_bounds__(kBlock)
k_cl_lse(const ST* __restrict__ x, float* __restrict__ lse, int K, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= V) return;
  const int64_t n = blockIdx.y;
  const ST* xn = x + n * K * V + v;
  float m = -INFINITY, s = 0.f;
  for (int c = 0; c < K; ++c) {
    const float xc = ld1<ST>(xn + (int64_t)c * V);
    const float mn = fmaxf(m, xc), ms = sub_max(mn);
    s = s * __expf(m - ms) + __expf(xc - ms);
    m = mn;
  }
  lse[n * V + v] = m + logf(s);
}

// (sum m S^p t, sum m S^p, sum m S^t p, sum m S^t) of one workgroup's voxels of (n, k); grid (V / 256, K, N)
__global__ void __launch_bounds__(kBlock)
k_cl_sums(Src psrc, Src tsrc, const int64_t* __restrict__ mask_lab, const float* __restrict__ sp, const float* __restrict__ st,
          float* __restrict__ part, Geo g) {
  __shared__ float smem[16];
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int k = blockIdx.y, K = psrc.K;
  const int64_t n = blockIdx.z;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (v < g.V && (!mask_lab || mask_lab[n * g.V + v] != -100)) {
    const int64_t i = (n * K + k) * g.V + v;
    const float p = src_at(psrc, n, k, g.V, v), t = src_at(tsrc, n, k, g.V, v);
    s[0] = sp[i] * t;
    s[1] = sp[i];
    s[2] = st[i] * p;
    s[3] = st[i];
  }
  block_sum<4>(s, smem);
  if (threadIdx.x == 0) {
    float* o = part + ((n * gridDim.x + blockIdx.x) * K + k) * 4;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
  }
}

// sums[(r, k)] = the M quadruples of row r and class k, in a fixed order; grid (K, rows)
__global__ void __launch_bounds__(kBlock)
k_cl_reduce(const float* __restrict__ part, float* __restrict__ sums, int K, int64_t M) {
  __shared__ float smem[16];
  const int64_t k = blockIdx.x, r = blockIdx.y;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = threadIdx.x; i < M; i += kBlock) {
    const float* p = part + ((r * M + i) * K + k) * 4;
    s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += p[3];
  }
  block_sum<4>(s, smem);
  if (threadIdx.x == 0) {
    float* o = sums + (r * K + k) * 4;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3];
  }
}

// value = 1 - 1/R sum_rk omega_k cl_rk; coef[(n, k)] = (A, B, C): dL/dS^p = m (A t + B), dL/dp (direct) = m C S^t
__global__ void __launch_bounds__(kBlock)
k_cl_finish(const float* __restrict__ sums, const float* __restrict__ weight, float* __restrict__ coef, float* __restrict__ value,
            int64_t N, int K, int64_t R, int first_class, float smooth) {
  __shared__ float smem[4];
  const float wsum = counted_weight_sum(weight, first_class, K);
  const float cN = 1.f / (float)R;
  float acc[1] = {0.f};
  for (int64_t i = threadIdx.x; i < R * K; i += kBlock) {
    const int64_t r = i / K;
    const int k = (int)(i - r * K);
    const float omega = k < first_class ? 0.f : (weight ? weight[k] : 1.f) / wsum;
    const float na = sums[i * 4 + 0] + smooth, nb = sums[i * 4 + 1] + smooth;
    const float nc = sums[i * 4 + 2] + smooth, nd = sums[i * 4 + 3] + smooth;
    const float Tp = na / nb, Ts = nc / nd, sum = Tp + Ts;
    if (k >= first_class) acc[0] += omega * ((2.f * Tp * Ts) / sum);
    if (coef) {
      const float dTp = (2.f * Ts * Ts) / (sum * sum), dTs = (2.f * Tp * Tp) / (sum * sum);
      const float A = k < first_class ? 0.f : -cN * omega * dTp / nb;
      const float B = k < first_class ? 0.f : cN * omega * dTp * na / (nb * nb);
      const float C = k < first_class ? 0.f : -cN * omega * dTs / nd;
      for (int64_t n = (R == 1 ? 0 : r); n < (R == 1 ? N : r + 1); ++n) {       // batch: every entry reads the same row
        coef[(n * K + k) * 3 + 0] = A;
        coef[(n * K + k) * 3 + 1] = B;
        coef[(n * K + k) * 3 + 2] = C;
      }
    }
  }
  block_sum<1>(acc, smem);
  if (threadIdx.x == 0) value[0] = 1.f - acc[0] * cN;
}

// gx_k = gs p_k (g_k - sum_j g_j p_j), g_k = Gp_k + m C_nk S^t_k; grid (V / 256, N)
template <typename ST>
__global__ void __launch_bounds__(kBlock)
k_cl_softmax_bwd(const ST* __restrict__ x, const float* __restrict__ lse, const int64_t* __restrict__ mask_lab,
                 const float* __restrict__ Gp, const float* __restrict__ st, const float* __restrict__ coef,
                 const float* __restrict__ grad_scale, ST* __restrict__ gx, int K, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= V) return;
  const int64_t n = blockIdx.y;
  const int64_t base = n * K * V + v;
  const float l = lse[n * V + v];
  const bool live = !mask_lab || mask_lab[n * V + v] != -100;
  const float gs = grad_scale ? grad_scale[0] : 1.f;
  const float* cf = coef + n * K * 3;
  float s = 0.f;
  for (int c = 0; c < K; ++c) {
    const int64_t i = base + (int64_t)c * V;
    const float p = __expf(ld1<ST>(x + i) - l);
    const float gk = Gp[i] + (live ? cf[3 * c + 2] * st[i] : 0.f);
    s += gk * p;
  }
  for (int c = 0; c < K; ++c) {
    const int64_t i = base + (int64_t)c * V;
    const float p = __expf(ld1<ST>(x + i) - l);
    const float gk = Gp[i] + (live ? cf[3 * c + 2] * st[i] : 0.f);
    st1<ST>(gx + i, gs * (p * (gk - s)));
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
inline int64_t vblocks(int64_t V) { return (V + kBlock - 1) / kBlock; }

inline Geo make_geo(int ndim, const int64_t* dims) {
  Geo g;
  if (ndim == 3) { g.s0 = (int)dims[0]; g.s1 = (int)dims[1]; g.s2 = (int)dims[2]; }
  else { g.s0 = 1; g.s1 = (int)dims[0]; g.s2 = (int)dims[1]; }
  g.V = (int64_t)g.s0 * g.s1 * g.s2;
  return g;
}

// N, K, V, iterations within what the launches and the workspace arithmetic take (grid y, z <= 65535; sizes inside int64)
inline bool skel_shape_ok(int64_t N, int64_t K, int64_t V, int iters) {
  if (V < 1 || !seg_shape_ok(N, K, V) || iters < 0 || iters > kMaxIter) return false;
  return vblocks(V) <= 0x7fffffff && V <= (((int64_t)1 << 62) / 1024) / (N * K);
}

inline int64_t round4(int64_t n) { return (n + 3) / 4 * 4; }

struct BwdLayout {           // floats: chain (I+1) PV | h (I+1) PV | G PV | ge PV | erosion codes | dilation codes (bytes)
  int64_t PV, chain, h, G, ge, sele, seld, total;
  BwdLayout(int64_t N, int64_t K, int64_t V, int iters) {
    PV = round4(N * K * V);
    const int64_t L = iters + 1;
    chain = 0;
    h = chain + L * PV;
    G = h + L * PV;
    ge = G + PV;
    sele = ge + PV;
    seld = sele + L * PV / 4;
    total = seld + L * PV / 4;
  }
};

struct LossLayout {          // floats: S^p PV | two chain arrays 2 PV | quadruples per (workgroup, class) | sums per (row, class)
  int64_t PV, sp, chain, part, sums, total;
  LossLayout(int64_t N, int64_t K, int64_t V) {
    PV = round4(N * K * V);
    sp = 0;
    chain = PV;
    part = chain + 2 * PV;
    sums = part + N * vblocks(V) * K * 4;
    total = sums + N * K * 4;
  }
};

inline Tile make_tile(const Geo& g, int ndim, int iters) {
  Tile t;
  t.h = iters + 2;
  if (ndim == 3) { t.tz = 8; t.ty = 8; t.tx = 32; t.hz = t.h; }
  else { t.tz = 1; t.ty = 32; t.tx = 64; t.hz = 0; }
  t.ntx = (g.s2 + t.tx - 1) / t.tx;
  t.nty = (g.s1 + t.ty - 1) / t.ty;
  return t;
}

inline int64_t tile_count(const Geo& g, const Tile& t) { return (int64_t)t.ntx * t.nty * ((g.s0 + t.tz - 1) / t.tz); }

// The route a forward takes: -1 when `route` cannot run these sizes.  Measured (profiles/r31/cldice): in 3D the halo of a
// cubic tile costs more than the level launches save, so volumes take the levels unless the caller asks for the tiles.
inline int pick_route(int route, int ndim, const Geo& g, int iters) {
  const bool can_fuse = iters <= kFusedMax && tile_count(g, make_tile(g, ndim, iters)) <= 0x7fffffff;
  if (route == ROUTE_FUSED) return can_fuse ? ROUTE_FUSED : -1;
  if (route == ROUTE_LEVELS) return ROUTE_LEVELS;
  return (can_fuse && ndim == 2) ? ROUTE_FUSED : ROUTE_LEVELS;
}

// skel = skeleton(src), by `route` (already picked); two = 2 PV floats for the levels
int skel_forward(const Src& src, float* skel, float* two, int64_t PV, int64_t N, int K, int ndim, const Geo& g, int iters,
                 int route, hipStream_t s) {
  if (route == ROUTE_FUSED) {
    const Tile t = make_tile(g, ndim, iters);
    const int E = (t.tz + 2 * t.hz) * (t.ty + 2 * t.h) * (t.tx + 2 * t.h);
    const size_t lds = (size_t)(2 * E + t.tz * t.ty * t.tx) * sizeof(float);
    if (lds > 65536)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_skel_tile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_skel_tile, dim3((unsigned)tile_count(g, t), (unsigned)K, (unsigned)N), dim3(kBlock), lds, s, src, skel, g,
                       t, iters);
    ADVCHAIN_LAUNCH_CHECK();
    return ADVCHAIN_OK;
  }
  const dim3 grid((unsigned)vblocks(g.V), (unsigned)K, (unsigned)N);
  // x_j (j >= 1) lives in two[j & 1]: iterations + 2 launches
  hipLaunchKernelGGL(k_skel_erode<false>, grid, dim3(kBlock), 0, s, src, two + PV, (unsigned char*)nullptr, g);
  ADVCHAIN_LAUNCH_CHECK();
  Src cur = src;
  for (int j = 0; j <= iters; ++j) {
    float* xj1 = two + ((j + 1) & 1) * PV;
    float* next = j < iters ? two + (j & 1) * PV : nullptr;
    hipLaunchKernelGGL(k_skel_level, grid, dim3(kBlock), 0, s, cur, (const float*)xj1, skel, next, g, j == 0 ? 1 : 0);
    ADVCHAIN_LAUNCH_CHECK();
    cur = Src{xj1, nullptr, nullptr, SRC_MAP, K};
  }
  return ADVCHAIN_OK;
}

// gradient of the skeleton with respect to src: into `out` (N,K,V).  Cotangent: grad, or m (A t + B) from coef / tsrc / mask_lab.
int skel_backward(const Src& src, const float* grad, const float* coef, const Src& tsrc, const int64_t* mask_lab, float* out,
                  float* ws, const BwdLayout& lay, int64_t N, int K, const Geo& g, int iters, hipStream_t s) {
  const dim3 grid((unsigned)vblocks(g.V), (unsigned)K, (unsigned)N);
  const int64_t PV = lay.PV;
  float* chain = ws + lay.chain;
  float* h = ws + lay.h;
  float* G = ws + lay.G;
  float* ge = ws + lay.ge;
  unsigned char* sele = (unsigned char*)(ws + lay.sele);
  unsigned char* seld = (unsigned char*)(ws + lay.seld);
  Src cur = src;
  for (int j = 0; j <= iters; ++j) {
    hipLaunchKernelGGL(k_skel_erode<true>, grid, dim3(kBlock), 0, s, cur, chain + j * PV, sele + j * PV, g);
    ADVCHAIN_LAUNCH_CHECK();
    cur = Src{chain + j * PV, nullptr, nullptr, SRC_MAP, K};
  }
  if (iters < 4)
    hipLaunchKernelGGL(k_skel_point<4>, grid, dim3(kBlock), 0, s, src, (const float*)chain, grad, coef, tsrc, mask_lab, h, seld, g,
                       iters, PV);
  else if (iters < 11)
    hipLaunchKernelGGL(k_skel_point<11>, grid, dim3(kBlock), 0, s, src, (const float*)chain, grad, coef, tsrc, mask_lab, h, seld, g,
                       iters, PV);
  else
    hipLaunchKernelGGL(k_skel_point<kMaxIter + 1>, grid, dim3(kBlock), 0, s, src, (const float*)chain, grad, coef, tsrc, mask_lab,
                       h, seld, g, iters, PV);
  ADVCHAIN_LAUNCH_CHECK();
  // ge_I from h_I alone, then G_j and ge_{j-1} in one launch per level, last G_0: iterations + 2 launches, ge in two arrays
  float* buf[2] = {ge, G};
  hipLaunchKernelGGL(k_skel_bwd, grid, dim3(kBlock), 0, s, (const float*)nullptr, (const float*)nullptr,
                     (const unsigned char*)nullptr, (const float*)(h + iters * PV), (const unsigned char*)(seld + iters * PV),
                     buf[iters & 1], g, K);
  ADVCHAIN_LAUNCH_CHECK();
  for (int j = iters; j >= 0; --j) {
    hipLaunchKernelGGL(k_skel_bwd, grid, dim3(kBlock), 0, s, (const float*)buf[j & 1], (const float*)(h + j * PV),
                       (const unsigned char*)(sele + j * PV), j > 0 ? (const float*)(h + (j - 1) * PV) : (const float*)nullptr,
                       j > 0 ? (const unsigned char*)(seld + (j - 1) * PV) : (const unsigned char*)nullptr,
                       j > 0 ? buf[(j - 1) & 1] : out, g, K);
    ADVCHAIN_LAUNCH_CHECK();
  }
  return ADVCHAIN_OK;
}

inline bool finite_nonneg(float v) { return v >= 0.f && v <= 3.40282347e38f; }   // false for NaN

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int64_t advchain_skeleton_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims, int iterations, int what) {
  const int64_t V = seg_voxels(ndim, dims);
  if (V < 0 || !skel_shape_ok(N, K, V, iterations) || what < 0 || what > 3) return -1;
  switch (what) {
    case 0: return 2 * round4(N * K * V);
    case 2: return LossLayout(N, K, V).total;
    default: return BwdLayout(N, K, V, iterations).total;
  }
}

int advchain_soft_skeleton_fwd(const float* maps, float* skeleton, float* workspace, int64_t N, int64_t K, int ndim,
                               const int64_t* dims, int iterations, int route, void* stream) {
  ADVCHAIN_CHECK_ARG(maps && skeleton && workspace, "soft_skeleton_fwd: null pointer");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(iterations >= 0 && iterations <= kMaxIter, "soft_skeleton_fwd: iterations must be in 0..32");
  ADVCHAIN_CHECK_ARG(V > 0 && skel_shape_ok(N, K, V, iterations), "soft_skeleton_fwd: bad N, K, ndim or dims");
  ADVCHAIN_CHECK_ARG(route >= ROUTE_AUTO && route <= ROUTE_LEVELS, "soft_skeleton_fwd: unknown route");
  const Geo g = make_geo(ndim, dims);
  const int r = pick_route(route, ndim, g, iterations);
  ADVCHAIN_CHECK_ARG(r > 0, "soft_skeleton_fwd: the fused route takes at most 4 iterations");
  const Src src{maps, nullptr, nullptr, SRC_MAP, (int)K};
  return skel_forward(src, skeleton, workspace, round4(N * K * V), N, (int)K, ndim, g, iterations, r, (hipStream_t)stream);
}

int advchain_soft_skeleton_bwd(const float* maps, const float* grad_skeleton, float* grad_maps, float* workspace, int64_t N,
                               int64_t K, int ndim, const int64_t* dims, int iterations, void* stream) {
  ADVCHAIN_CHECK_ARG(maps && grad_skeleton && grad_maps && workspace, "soft_skeleton_bwd: null pointer");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(iterations >= 0 && iterations <= kMaxIter, "soft_skeleton_bwd: iterations must be in 0..32");
  ADVCHAIN_CHECK_ARG(V > 0 && skel_shape_ok(N, K, V, iterations), "soft_skeleton_bwd: bad N, K, ndim or dims");
  const Geo g = make_geo(ndim, dims);
  const Src src{maps, nullptr, nullptr, SRC_MAP, (int)K};
  return skel_backward(src, grad_skeleton, nullptr, src, nullptr, grad_maps, workspace, BwdLayout(N, K, V, iterations), N, (int)K,
                       g, iterations, (hipStream_t)stream);
}

int advchain_cldice_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                        float* lse, float* skeleton_target, float* coef, float* workspace, float* value, int64_t N, int64_t K,
                        int ndim, const int64_t* dims, int iterations, int route, int flags, float smooth, void* stream) {
  ADVCHAIN_CHECK_ARG(logits && lse && skeleton_target && workspace && value, "cldice_fwd: null pointer");
  ADVCHAIN_CHECK_ARG((labels != nullptr) != (soft != nullptr), "cldice_fwd: exactly one of labels / soft target");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "cldice_fwd: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(iterations >= 0 && iterations <= kMaxIter, "cldice_fwd: iterations must be in 0..32");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(V > 0 && skel_shape_ok(N, K, V, iterations), "cldice_fwd: bad N, ndim or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "cldice_fwd: logits are fp32 (0) or bf16 (1)");
  ADVCHAIN_CHECK_ARG((flags & ~3) == 0, "cldice_fwd: unknown flags");
  ADVCHAIN_CHECK_ARG(finite_nonneg(smooth), "cldice_fwd: smooth must be finite and >= 0");
  ADVCHAIN_CHECK_ARG(route >= ROUTE_AUTO && route <= ROUTE_LEVELS, "cldice_fwd: unknown route");
  const int first_class = (flags & CLDICE_IGNORE_BACKGROUND) ? 1 : 0;
  ADVCHAIN_CHECK_ARG(K > first_class, "cldice_fwd: no class left with ignore_background");
  const Geo g = make_geo(ndim, dims);
  const int r = pick_route(route, ndim, g, iterations);
  ADVCHAIN_CHECK_ARG(r > 0, "cldice_fwd: the fused route takes at most 4 iterations");
  const LossLayout lay(N, K, V);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nb = vblocks(V);
  if (logits_bf16)
    hipLaunchKernelGGL(k_cl_lse<unsigned short>, dim3((unsigned)nb, (unsigned)N), dim3(kBlock), 0, s,
                       (const unsigned short*)logits, lse, (int)K, V);
  else
    hipLaunchKernelGGL(k_cl_lse<float>, dim3((unsigned)nb, (unsigned)N), dim3(kBlock), 0, s, (const float*)logits, lse, (int)K, V);
  ADVCHAIN_LAUNCH_CHECK();
  const Src psrc{logits, lse, nullptr, logits_bf16 ? SRC_SOFTMAX_BF16 : SRC_SOFTMAX_F32, (int)K};
  const Src tsrc = labels ? Src{nullptr, nullptr, labels, SRC_ONEHOT, (int)K} : Src{soft, nullptr, nullptr, SRC_MAP, (int)K};
  float* sp = workspace + lay.sp;
  int rc = skel_forward(psrc, sp, workspace + lay.chain, lay.PV, N, (int)K, ndim, g, iterations, r, s);
  if (rc != ADVCHAIN_OK) return rc;
  rc = skel_forward(tsrc, skeleton_target, workspace + lay.chain, lay.PV, N, (int)K, ndim, g, iterations, r, s);
  if (rc != ADVCHAIN_OK) return rc;
  float* part = workspace + lay.part;
  float* sums = workspace + lay.sums;
  hipLaunchKernelGGL(k_cl_sums, dim3((unsigned)nb, (unsigned)K, (unsigned)N), dim3(kBlock), 0, s, psrc, tsrc, labels,
                     (const float*)sp, (const float*)skeleton_target, part, g);
  ADVCHAIN_LAUNCH_CHECK();
  const int64_t R = (flags & CLDICE_BATCH) ? 1 : N, M = (flags & CLDICE_BATCH) ? N * nb : nb;
  hipLaunchKernelGGL(k_cl_reduce, dim3((unsigned)K, (unsigned)R), dim3(kBlock), 0, s, (const float*)part, sums, (int)K, M);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cl_finish, dim3(1), dim3(kBlock), 0, s, (const float*)sums, weight, coef, value, N, (int)K, R, first_class,
                     smooth);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_cldice_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* lse,
                        const float* skeleton_target, const float* coef, const float* grad_scale, void* grad_logits,
                        float* workspace, int64_t N, int64_t K, int ndim, const int64_t* dims, int iterations, void* stream) {
  ADVCHAIN_CHECK_ARG(logits && lse && skeleton_target && coef && grad_logits && workspace, "cldice_bwd: null pointer");
  ADVCHAIN_CHECK_ARG((labels != nullptr) != (soft != nullptr), "cldice_bwd: exactly one of labels / soft target");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "cldice_bwd: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(iterations >= 0 && iterations <= kMaxIter, "cldice_bwd: iterations must be in 0..32");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(V > 0 && skel_shape_ok(N, K, V, iterations), "cldice_bwd: bad N, ndim or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "cldice_bwd: logits are fp32 (0) or bf16 (1)");
  const Geo g = make_geo(ndim, dims);
  const BwdLayout lay(N, K, V, iterations);
  hipStream_t s = (hipStream_t)stream;
  const Src psrc{logits, lse, nullptr, logits_bf16 ? SRC_SOFTMAX_BF16 : SRC_SOFTMAX_F32, (int)K};
  const Src tsrc = labels ? Src{nullptr, nullptr, labels, SRC_ONEHOT, (int)K} : Src{soft, nullptr, nullptr, SRC_MAP, (int)K};
  float* Gp = workspace + lay.G;           // (the last level writes the gradient of p where the running gradient lived)
  const int rc = skel_backward(psrc, nullptr, coef, tsrc, labels, Gp, workspace, lay, N, (int)K, g, iterations, s);
  if (rc != ADVCHAIN_OK) return rc;
  const dim3 grid((unsigned)vblocks(V), (unsigned)N);
  if (logits_bf16)
    hipLaunchKernelGGL(k_cl_softmax_bwd<unsigned short>, grid, dim3(kBlock), 0, s, (const unsigned short*)logits, lse, labels,
                       (const float*)Gp, skeleton_target, coef, grad_scale, (unsigned short*)grad_logits, (int)K, V);
  else
    hipLaunchKernelGGL(k_cl_softmax_bwd<float>, grid, dim3(kBlock), 0, s, (const float*)logits, lse, labels, (const float*)Gp,
                       skeleton_target, coef, grad_scale, (float*)grad_logits, (int)K, V);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
