// Jacobian determinant and folding statistics of deformation fields for gfx950 -- what the reference's helpers
// (adv_morph.py:57-99) refuse: 3D fields, sampling grids in normalised coordinates, and "does it fold" without a map.
//
//   advchain_image_diff3d_fwd/bwd     (dx, dy, dz) of a (N,C,S0,S1,S2) batch, the stencil of calculate_image_diff per axis
//   advchain_jacobian_det_fwd/bwd     det J of a (N,2,H,W) or (N,3,S0,S1,S2) field; mode bit 0: the field is a sampling grid
//                                     (positions, J in voxel units), bit 1: clamped to [-1, 1] as it is loaded
//   advchain_jacobian_stats           per batch entry: #(det < 0), #(!(det > 0)), min, max -- no determinant map; one partial
//                                     per wave in a workspace, folded per entry by a second launch (no atomics)
//
// Decomposition (diff_stencil.h): one wave owns 62 columns (x, the last axis) of one row strip of one plane; x neighbours come
// through DPP lane shifts, the rows y-1, y, y+1 of the wave's own plane march through registers, and the rows of the planes
// z-1 and z+1 are read directly -- they are other waves' own rows, so they come from the caches.  All lanes stay active
// through the shifts; only stores and the statistics are predicated.
//
// Arithmetic: compiled with -ffp-contract=off (build.py).  The determinant is ONE device function per dimensionality (det2,
// det3), shared by the map kernel and the statistics kernel (one kernel template, STATS on or off): the statistics are those
// of the map bit for bit.  2D displacement mode is det_of of deform_diff.hip; its map and backward ARE those kernels (the
// entries below forward to advchain_jacobian_det2d_*).
//
// Backward: grad f_i = s_i sum_j D_j^T (g cof_ij) in gather form, cofactors recomputed at the six neighbours.  cof_ij holds
// no derivative along axis j, so the neighbours along x need only their own y and z derivatives (the halo lanes have them),
// those along y only x and z derivatives of their row, those along z only x and y derivatives of their plane: the 3 x 3
// rows around the output row are enough, no value two steps away is read.  No atomics: two calls give the same bits.
#include <stdio.h>

#include "common.h"
#include "diff_stencil.h"

// mode 0 of a 2D field is the reference's own helper: those kernels (deform_diff.hip)
extern "C" int advchain_jacobian_det2d_fwd(const float* field, float* det, int64_t N, const int64_t* dims, void* stream);
extern "C" int advchain_jacobian_det2d_bwd(const float* grad_det, const float* field, float* grad_field, int64_t N,
                                           const int64_t* dims, void* stream);

namespace advchain {
namespace {

enum { MODE_POS = 1, MODE_CLAMP = 2 };

// the field value a kernel works with: clamped like torch.clamp (NaN stays NaN)
template <int MODE>
__device__ __forceinline__ float ldq(float q) {
  if (MODE & MODE_CLAMP) return q < -1.f ? -1.f : (q > 1.f ? 1.f : q);
  return q;
}

// entry (i, j) of J from d = D_j f_i: positions s_i d (s_i = (S_i - 1) / 2: normalised -> voxels), displacement delta_ij + d
template <int MODE>
__device__ __forceinline__ float jent(float d, int i, int j, float s) {
  if (MODE & MODE_POS) return s * d;
  return i == j ? 1.f + d : d;
}

template <int MODE>
__device__ __forceinline__ float det2(float dxx, float dxy, float dyx, float dyy, float sx, float sy) {
  if (MODE & MODE_POS) return (sx * dxx) * (sy * dyy) - (sx * dxy) * (sy * dyx);
  return det_of(dxx, dxy, dyx, dyy);
}

// d[i][j] = D_j f_i, i and j in (x, y, z)
template <int MODE>
__device__ __forceinline__ float det3(const float (&d)[3][3], const float (&s)[3]) {
  float J[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) J[i][j] = jent<MODE>(d[i][j], i, j, s[i]);
  return J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
         J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
}

// ---- statistics -------------------------------------------------------------------------------------------------------
// Every wave leaves ONE partial in the caller's workspace (its own slot: no atomics, nothing to clear), and one workgroup per
// batch entry folds that entry's partials -- integer sums and min / max, which do not depend on the order.  (Atomics on the
// N output words themselves serialise: 8192 waves on 4 entries took three times the map kernel's time.)
struct alignas(16) StatsPart {
  int neg, nonpos;
  float mn, mx;      // +inf / -inf when the wave saw no determinant that is a number
};

struct StatsAcc {
  int neg = 0, nonpos = 0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  __device__ __forceinline__ void add(float v) {
    neg += v < 0.f;
    nonpos += !(v > 0.f);          // zeros and NaN count
    mn = v < mn ? v : mn;          // NaN never passes a comparison: ignored
    mx = v > mx ? v : mx;
  }
  // every lane of the wave calls this; `slot`: the wave's index in the launch
  __device__ __forceinline__ void flush(StatsPart* __restrict__ parts, int64_t slot) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      neg += __shfl_xor(neg, m, 64);
      nonpos += __shfl_xor(nonpos, m, 64);
      const float a = __shfl_xor(mn, m, 64), b = __shfl_xor(mx, m, 64);
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) parts[slot] = StatsPart{neg, nonpos, mn, mx};
  }
};

__device__ __forceinline__ int64_t wave_slot() { return (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); }

// workgroup n: the `per` partials of batch entry n (consecutive waves) -> neg[n], nonpos[n], min[n], max[n]
__global__ void __launch_bounds__(kBlock) k_stats_finish(const StatsPart* __restrict__ parts, int64_t per,
                                                         int64_t* __restrict__ neg, int64_t* __restrict__ nonpos,
                                                         float* __restrict__ mn, float* __restrict__ mx) {
  __shared__ long long s_cnt[2][kWavesPerBlock];
  __shared__ float s_ext[2][kWavesPerBlock];
  const int64_t n = blockIdx.x;
  long long a = 0, b = 0;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int64_t i = threadIdx.x; i < per; i += kBlock) {
    const StatsPart p = parts[n * per + i];
    a += p.neg;
    b += p.nonpos;
    lo = p.mn < lo ? p.mn : lo;
    hi = p.mx > hi ? p.mx : hi;
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    a += __shfl_xor(a, m, 64);
    b += __shfl_xor(b, m, 64);
    const float l2 = __shfl_xor(lo, m, 64), h2 = __shfl_xor(hi, m, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_cnt[0][wave] = a; s_cnt[1][wave] = b; s_ext[0][wave] = lo; s_ext[1][wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWavesPerBlock; ++w) {
      a += s_cnt[0][w];
      b += s_cnt[1][w];
      lo = s_ext[0][w] < lo ? s_ext[0][w] : lo;
      hi = s_ext[1][w] > hi ? s_ext[1][w] : hi;
    }
    neg[n] = a;
    nonpos[n] = b;
    mn[n] = lo;
    mx[n] = hi;
  }
}

// ---- 2D ---------------------------------------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ float row2(const float* p, int r, int H, int W, int xc) {
  return ldq<MODE>(row_at(p, r, H, W, xc));
}

// k_jacobian2d_fwd with the mode; STATS: the determinants go into the statistics instead of a map
template <int MODE, bool STATS>
__global__ void __launch_bounds__(kBlock) k_jac2d_fwd(const float* __restrict__ field, float* __restrict__ det, StatsPart* __restrict__ parts,
                                                      int64_t N, int H, int W, int chunks, int strips, int R) {
  Strip s;
  if (!strip_of(N, H, W, chunks, strips, R, s)) return;
  const int64_t P = (int64_t)H * W;
  const float* u = field + s.plane * 2 * P;
  const float* v = u + P;
  const float sx = 0.5f * (float)(W - 1), sy = 0.5f * (float)(H - 1);
  float up = row2<MODE>(u, s.y0 - 1, H, W, s.xc), uc = row2<MODE>(u, s.y0, H, W, s.xc);
  float vp = row2<MODE>(v, s.y0 - 1, H, W, s.xc), vc = row2<MODE>(v, s.y0, H, W, s.xc);
  StatsAcc acc;
  for (int y = s.y0; y < s.y1; ++y) {
    const float un = row2<MODE>(u, y + 1, H, W, s.xc), vn = row2<MODE>(v, y + 1, H, W, s.xc);
    const float dxx = diff1(lane_prev_f(uc), uc, lane_next_f(uc), s.x, W);
    const float dyx = diff1(lane_prev_f(vc), vc, lane_next_f(vc), s.x, W);
    if (s.store) {
      const float d = det2<MODE>(dxx, diff1(up, uc, un, y, H), dyx, diff1(vp, vc, vn, y, H), sx, sy);
      if (STATS) acc.add(d);
      else det[s.plane * P + (int64_t)y * W + s.x] = d;
    }
    up = uc; uc = un;
    vp = vc; vc = vn;
  }
  if (STATS) acc.flush(parts, wave_slot());
}

// the products of the 2D backward at one row, from the entries of J: p1 = g Jyy, p2 = g Jyx, p3 = g Jxx, p4 = g Jxy
struct Prod2 { float p1, p2, p3, p4; };

template <int MODE>
__device__ __forceinline__ Prod2 prods_m(float um, float u0, float up, float vm, float v0, float vp, float g, int x, int r, int H,
                                        int W, float sx, float sy) {
  const float dxx = diff1(lane_prev_f(u0), u0, lane_next_f(u0), x, W);
  const float dyx = diff1(lane_prev_f(v0), v0, lane_next_f(v0), x, W);
  const float dxy = diff1(um, u0, up, r, H), dyy = diff1(vm, v0, vp, r, H);
  Prod2 q;
  q.p1 = g * jent<MODE>(dyy, 1, 1, sy);
  q.p2 = g * jent<MODE>(dyx, 1, 0, sy);
  q.p3 = g * jent<MODE>(dxx, 0, 0, sx);
  q.p4 = g * jent<MODE>(dxy, 0, 1, sx);
  return q;
}

// k_jacobian2d_bwd with the mode: grad_u = sx (Dx^T p1 - Dy^T p2), grad_v = sy (Dy^T p3 - Dx^T p4), zero where the clamp cut
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_jac2d_bwd(const float* __restrict__ gdet, const float* __restrict__ field,
                                                      float* __restrict__ gfield, int64_t N, int H, int W, int chunks,
                                                      int strips, int R) {
  Strip s;
  if (!strip_of(N, H, W, chunks, strips, R, s)) return;
  const int64_t P = (int64_t)H * W;
  const float* u = field + s.plane * 2 * P;
  const float* v = u + P;
  const float* g = gdet + s.plane * P;
  const float sx = 0.5f * (float)(W - 1), sy = 0.5f * (float)(H - 1);
  const int y0 = s.y0, x = s.x, xc = s.xc;
  float u0 = row2<MODE>(u, y0, H, W, xc), u1 = row2<MODE>(u, y0 + 1, H, W, xc);
  float v0 = row2<MODE>(v, y0, H, W, xc), v1 = row2<MODE>(v, y0 + 1, H, W, xc);
  Prod2 pm = {0.f, 0.f, 0.f, 0.f}, pc, pn;
  {
    const float um1 = row2<MODE>(u, y0 - 1, H, W, xc), vm1 = row2<MODE>(v, y0 - 1, H, W, xc);
    if (y0 >= 1) {
      const float um2 = row2<MODE>(u, y0 - 2, H, W, xc), vm2 = row2<MODE>(v, y0 - 2, H, W, xc);
      pm = prods_m<MODE>(um2, um1, u0, vm2, vm1, v0, row_at(g, y0 - 1, H, W, xc), x, y0 - 1, H, W, sx, sy);
    }
    pc = prods_m<MODE>(um1, u0, u1, vm1, v0, v1, row_at(g, y0, H, W, xc), x, y0, H, W, sx, sy);
  }
  for (int y = y0; y < s.y1; ++y) {
    // (u0, u1) are rows y, y + 1 here
    const float u2 = row2<MODE>(u, y + 2, H, W, xc), v2 = row2<MODE>(v, y + 2, H, W, xc);
    if (y + 1 < H) pn = prods_m<MODE>(u0, u1, u2, v0, v1, v2, row_at(g, y + 1, H, W, xc), x, y + 1, H, W, sx, sy);
    else pn = Prod2{0.f, 0.f, 0.f, 0.f};
    const float ax1 = diff1_adj(lane_prev_f(pc.p1), pc.p1, lane_next_f(pc.p1), x, W);
    const float ax4 = diff1_adj(lane_prev_f(pc.p4), pc.p4, lane_next_f(pc.p4), x, W);
    if (s.store) {
      const int64_t o = (int64_t)y * W + x;
      float gu = ax1 - diff1_adj(pm.p2, pc.p2, pn.p2, y, H);
      float gv = diff1_adj(pm.p3, pc.p3, pn.p3, y, H) - ax4;
      if (MODE & MODE_POS) { gu = sx * gu; gv = sy * gv; }
      if (MODE & MODE_CLAMP) {
        const float qu = u[o], qv = v[o];
        if (!(qu >= -1.f && qu <= 1.f)) gu = 0.f;
        if (!(qv >= -1.f && qv <= 1.f)) gv = 0.f;
      }
      gfield[s.plane * 2 * P + o] = gu;
      gfield[s.plane * 2 * P + o + P] = gv;
    }
    pm = pc; pc = pn;
    u0 = u1; u1 = u2;
    v0 = v1; v1 = v2;
  }
}

// ---- 3D ---------------------------------------------------------------------------------------------------------------
// wave -> (volume, plane z, column chunk, row strip): the 2D strip with `volumes * D` planes
struct Strip3 {
  Strip s;
  int64_t vol;
  int z;
};

__device__ __forceinline__ bool strip3_of(int64_t vols, int D, int H, int W, int chunks, int strips, int R, Strip3& t) {
  if (!strip_of(vols * D, H, W, chunks, strips, R, t.s)) return false;
  t.vol = t.s.plane / D;
  t.z = (int)(t.s.plane - t.vol * D);
  return true;
}

// p: one volume (D, H, W); z and r are the same in every lane
__device__ __forceinline__ float row3(const float* p, int z, int r, int D, int H, int W, int xc) {
  return (z >= 0 && z < D && r >= 0 && r < H) ? p[((int64_t)z * H + r) * W + xc] : 0.f;
}

__global__ void __launch_bounds__(kBlock) k_diff3d_fwd(const float* __restrict__ in, float* __restrict__ dx,
                                                       float* __restrict__ dy, float* __restrict__ dz, int64_t vols, int D,
                                                       int H, int W, int chunks, int strips, int R) {
  Strip3 t;
  if (!strip3_of(vols, D, H, W, chunks, strips, R, t)) return;
  const Strip& s = t.s;
  const int z = t.z;
  const int64_t base = t.vol * D * H * W;
  const float* p = in + base;
  float prev = row3(p, z, s.y0 - 1, D, H, W, s.xc), cur = row3(p, z, s.y0, D, H, W, s.xc);
  for (int y = s.y0; y < s.y1; ++y) {
    const float next = row3(p, z, y + 1, D, H, W, s.xc);
    const float zm = row3(p, z - 1, y, D, H, W, s.xc), zp = row3(p, z + 1, y, D, H, W, s.xc);
    const float l = lane_prev_f(cur), r = lane_next_f(cur);
    if (s.store) {
      const int64_t o = base + ((int64_t)z * H + y) * W + s.x;
      dx[o] = diff1(l, cur, r, s.x, W);
      dy[o] = diff1(prev, cur, next, y, H);
      dz[o] = diff1(zm, cur, zp, z, D);
    }
    prev = cur;
    cur = next;
  }
}

// grad_in = Dx^T gdx + Dy^T gdy + Dz^T gdz, each term only where its gradient is present, added in this order
__global__ void __launch_bounds__(kBlock) k_diff3d_bwd(const float* __restrict__ gdx, const float* __restrict__ gdy,
                                                       const float* __restrict__ gdz, float* __restrict__ gin, int64_t vols,
                                                       int D, int H, int W, int chunks, int strips, int R) {
  Strip3 t;
  if (!strip3_of(vols, D, H, W, chunks, strips, R, t)) return;
  const Strip& s = t.s;
  const int z = t.z;
  const int64_t base = t.vol * D * H * W;
  const float* px = gdx ? gdx + base : nullptr;
  const float* py = gdy ? gdy + base : nullptr;
  const float* pz = gdz ? gdz + base : nullptr;
  float prev = 0.f, cur = 0.f;
  if (py) { prev = row3(py, z, s.y0 - 1, D, H, W, s.xc); cur = row3(py, z, s.y0, D, H, W, s.xc); }
  for (int y = s.y0; y < s.y1; ++y) {
    float a = 0.f;
    if (px) {
      const float c = row3(px, z, y, D, H, W, s.xc);
      a = diff1_adj(lane_prev_f(c), c, lane_next_f(c), s.x, W);
    }
    float next = 0.f;
    if (py) {
      next = row3(py, z, y + 1, D, H, W, s.xc);
      a += diff1_adj(prev, cur, next, y, H);
    }
    if (pz) a += diff1_adj(row3(pz, z - 1, y, D, H, W, s.xc), row3(pz, z, y, D, H, W, s.xc), row3(pz, z + 1, y, D, H, W, s.xc), z, D);
    if (s.store) gin[base + ((int64_t)z * H + y) * W + s.x] = a;
    prev = cur;
    cur = next;
  }
}

template <int MODE>
__device__ __forceinline__ float row3q(const float* p, int z, int r, int D, int H, int W, int xc) {
  return ldq<MODE>(row3(p, z, r, D, H, W, xc));
}

template <int MODE, bool STATS>
__global__ void __launch_bounds__(kBlock) k_jac3d_fwd(const float* __restrict__ field, float* __restrict__ det, StatsPart* __restrict__ parts,
                                                      int64_t N, int D, int H, int W, int chunks, int strips, int R) {
  Strip3 t;
  if (!strip3_of(N, D, H, W, chunks, strips, R, t)) return;
  const Strip& s = t.s;
  const int z = t.z;
  const int64_t V = (int64_t)D * H * W;
  const float* f = field + t.vol * 3 * V;
  const float sc[3] = {0.5f * (float)(W - 1), 0.5f * (float)(H - 1), 0.5f * (float)(D - 1)};
  float pv[3], cv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pv[c] = row3q<MODE>(f + c * V, z, s.y0 - 1, D, H, W, s.xc);
    cv[c] = row3q<MODE>(f + c * V, z, s.y0, D, H, W, s.xc);
  }
  StatsAcc acc;
  for (int y = s.y0; y < s.y1; ++y) {
    float d[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float nv = row3q<MODE>(f + c * V, z, y + 1, D, H, W, s.xc);
      const float zm = row3q<MODE>(f + c * V, z - 1, y, D, H, W, s.xc), zp = row3q<MODE>(f + c * V, z + 1, y, D, H, W, s.xc);
      d[c][0] = diff1(lane_prev_f(cv[c]), cv[c], lane_next_f(cv[c]), s.x, W);
      d[c][1] = diff1(pv[c], cv[c], nv, y, H);
      d[c][2] = diff1(zm, cv[c], zp, z, D);
      pv[c] = cv[c];
      cv[c] = nv;
    }
    if (s.store) {
      const float v = det3<MODE>(d, sc);
      if (STATS) acc.add(v);
      else det[t.vol * V + ((int64_t)z * H + y) * W + s.x] = v;
    }
  }
  if (STATS) acc.flush(parts, wave_slot());
}

// g cof_ij, i = 0..2, for one axis j from the entries of J along the two other axes a = j + 1, b = j + 2 (cyclic):
// cof_ij = J[i+1][a] J[i+2][b] - J[i+1][b] J[i+2][a]
struct P3 { float p[3]; };

__device__ __forceinline__ P3 cof_col(const float (&Ja)[3], const float (&Jb)[3], float g) {
  P3 r;
  r.p[0] = g * (Ja[1] * Jb[2] - Jb[1] * Ja[2]);
  r.p[1] = g * (Ja[2] * Jb[0] - Jb[2] * Ja[0]);
  r.p[2] = g * (Ja[0] * Jb[1] - Jb[0] * Ja[1]);
  return r;
}

// x derivative of the three components at one row (m: the row's values), as entries of J; every lane of the wave calls this
template <int MODE>
__device__ __forceinline__ void jx_of(const float (&m)[3], int x, int W, const float (&sc)[3], float (&J)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) J[c] = jent<MODE>(diff1(lane_prev_f(m[c]), m[c], lane_next_f(m[c]), x, W), c, 0, sc[c]);
}
// derivative along y (axis = 1) or z (axis = 2) from the three values along that axis
template <int MODE>
__device__ __forceinline__ void jax_of(const float (&a)[3], const float (&b)[3], const float (&c3)[3], int i, int S, int axis,
                                       const float (&sc)[3], float (&J)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) J[c] = jent<MODE>(diff1(a[c], b[c], c3[c], i, S), c, axis, sc[c]);
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) k_jac3d_bwd(const float* __restrict__ gdet, const float* __restrict__ field,
                                                      float* __restrict__ gfield, int64_t N, int D, int H, int W, int chunks,
                                                      int strips, int R) {
  Strip3 t;
  if (!strip3_of(N, D, H, W, chunks, strips, R, t)) return;
  const Strip& s = t.s;
  const int z = t.z, x = s.x, xc = s.xc;
  const int64_t V = (int64_t)D * H * W;
  const float* f = field + t.vol * 3 * V;
  const float* g = gdet + t.vol * V;
  const float sc[3] = {0.5f * (float)(W - 1), 0.5f * (float)(H - 1), 0.5f * (float)(D - 1)};
  // v[k][r][c]: component c at plane z - 1 + k, row y - 1 + r
  float v[3][3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[k][1][c] = row3q<MODE>(f + c * V, z - 1 + k, s.y0 - 1, D, H, W, xc);
      v[k][2][c] = row3q<MODE>(f + c * V, z - 1 + k, s.y0, D, H, W, xc);
    }
  // g cof_iy of the rows y - 1, y, y + 1 of this plane: x and z derivatives of that row
  P3 pm = {{0.f, 0.f, 0.f}}, pc, pn;
  {
    float Jx[3], Jz[3];
    if (s.y0 >= 1) {
      jx_of<MODE>(v[1][1], x, W, sc, Jx);
      jax_of<MODE>(v[0][1], v[1][1], v[2][1], z, D, 2, sc, Jz);
      pm = cof_col(Jz, Jx, row3(g, z, s.y0 - 1, D, H, W, xc));
    }
    jx_of<MODE>(v[1][2], x, W, sc, Jx);
    jax_of<MODE>(v[0][2], v[1][2], v[2][2], z, D, 2, sc, Jz);
    pc = cof_col(Jz, Jx, row3(g, z, s.y0, D, H, W, xc));
  }
  for (int y = s.y0; y < s.y1; ++y) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[k][0][c] = v[k][1][c];
        v[k][1][c] = v[k][2][c];
        v[k][2][c] = row3q<MODE>(f + c * V, z - 1 + k, y + 1, D, H, W, xc);
      }
    float Jx[3], Jy[3], Jz[3];
    // along y: the row below
    if (y + 1 < H) {
      jx_of<MODE>(v[1][2], x, W, sc, Jx);
      jax_of<MODE>(v[0][2], v[1][2], v[2][2], z, D, 2, sc, Jz);
      pn = cof_col(Jz, Jx, row3(g, z, y + 1, D, H, W, xc));
    } else {
      pn = P3{{0.f, 0.f, 0.f}};
    }
    // along x: g cof_ix of this voxel (y and z derivatives), shifted across the lanes
    jax_of<MODE>(v[1][0], v[1][1], v[1][2], y, H, 1, sc, Jy);
    jax_of<MODE>(v[0][1], v[1][1], v[2][1], z, D, 2, sc, Jz);
    const P3 px = cof_col(Jy, Jz, row3(g, z, y, D, H, W, xc));
    // along z: g cof_iz of this row in the planes z - 1, z, z + 1 (x and y derivatives)
    P3 pz[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      jx_of<MODE>(v[k][1], x, W, sc, Jx);
      jax_of<MODE>(v[k][0], v[k][1], v[k][2], y, H, 1, sc, Jy);
      pz[k] = cof_col(Jx, Jy, row3(g, z - 1 + k, y, D, H, W, xc));
    }
    float out[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float ax = diff1_adj(lane_prev_f(px.p[c]), px.p[c], lane_next_f(px.p[c]), x, W);
      const float ay = diff1_adj(pm.p[c], pc.p[c], pn.p[c], y, H);
      const float az = diff1_adj(pz[0].p[c], pz[1].p[c], pz[2].p[c], z, D);
      out[c] = (ax + ay) + az;
      if (MODE & MODE_POS) out[c] = sc[c] * out[c];
    }
    if (s.store) {
      const int64_t o = ((int64_t)z * H + y) * W + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float a = out[c];
        if (MODE & MODE_CLAMP) {
          const float q = f[c * V + o];
          if (!(q >= -1.f && q <= 1.f)) a = 0.f;
        }
        gfield[t.vol * 3 * V + c * V + o] = a;
      }
    }
    pm = pc;
    pc = pn;
  }
}

// ---- host helpers -----------------------------------------------------------------------------------------------------
struct Geo {
  int D, H, W;     // D == 1 for 2D
  StripLaunch L;
};

// 0, or the message's tail
const char* geo_of(int64_t vols, int ndim, const int64_t* dims, Geo& G) {
  if (ndim != 2 && ndim != 3) return "ndim must be 2 or 3";
  if (!dims) return "null dims";
  int64_t vox = 1;
  for (int i = 0; i < ndim; ++i) {
    if (dims[i] < 2) return "every spatial size must be at least 2";
    if (dims[i] > (1 << 24)) return "spatial size too large";
    vox *= dims[i];
    if (vox >= (1ll << 31)) return "per-sample volume too large";
  }
  G.D = ndim == 3 ? (int)dims[0] : 1;
  G.H = (int)dims[ndim - 2];
  G.W = (int)dims[ndim - 1];
  if (!strip_launch(vols * G.D, G.H, G.W, G.L)) return "too large";
  return nullptr;
}

bool mode_ok(int mode) { return mode == 0 || mode == MODE_POS || mode == (MODE_POS | MODE_CLAMP); }

}  // namespace
}  // namespace advchain

using namespace advchain;

#define JAC_FAIL(entry, tail)                              \
  do {                                                     \
    static thread_local char buf_[160];                    \
    snprintf(buf_, sizeof(buf_), "%s: %s", entry, tail);   \
    advchain_set_error_(buf_);                             \
    return ADVCHAIN_ERR_ARG;                               \
  } while (0)

// launch kernel template K<MODE, ...> for the run-time mode (0, positions, positions + clamp)
#define JAC_BY_MODE(mode, LAUNCH)                         \
  do {                                                    \
    if ((mode) == 0) { LAUNCH(0); }                       \
    else if ((mode) == MODE_POS) { LAUNCH(MODE_POS); }    \
    else { LAUNCH(MODE_POS | MODE_CLAMP); }               \
  } while (0)

extern "C" {

int advchain_image_diff3d_fwd(const float* in, float* dx, float* dy, float* dz, int64_t N, int64_t C, const int64_t* dims,
                              void* stream) {
  ADVCHAIN_CHECK_ARG(in && dx && dy && dz, "image_diff3d_fwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536 && C >= 0 && C < (1 << 24), "image_diff3d_fwd: bad N or C");
  Geo G;
  if (const char* why = geo_of(N * C, 3, dims, G)) JAC_FAIL("image_diff3d_fwd", why);
  if (N == 0 || C == 0) return ADVCHAIN_OK;
  hipLaunchKernelGGL(k_diff3d_fwd, dim3(G.L.blocks), dim3(kBlock), 0, (hipStream_t)stream, in, dx, dy, dz, N * C, G.D, G.H, G.W,
                     G.L.chunks, G.L.strips, G.L.R);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_image_diff3d_bwd(const float* grad_dx, const float* grad_dy, const float* grad_dz, float* grad_in, int64_t N,
                              int64_t C, const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(grad_in && (grad_dx || grad_dy || grad_dz), "image_diff3d_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536 && C >= 0 && C < (1 << 24), "image_diff3d_bwd: bad N or C");
  Geo G;
  if (const char* why = geo_of(N * C, 3, dims, G)) JAC_FAIL("image_diff3d_bwd", why);
  if (N == 0 || C == 0) return ADVCHAIN_OK;
  hipLaunchKernelGGL(k_diff3d_bwd, dim3(G.L.blocks), dim3(kBlock), 0, (hipStream_t)stream, grad_dx, grad_dy, grad_dz, grad_in,
                     N * C, G.D, G.H, G.W, G.L.chunks, G.L.strips, G.L.R);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_jacobian_det_fwd(const float* field, float* det, int64_t N, int ndim, const int64_t* dims, int mode,
                              void* stream) {
  ADVCHAIN_CHECK_ARG(field && det, "jacobian_det_fwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536, "jacobian_det_fwd: bad N");
  ADVCHAIN_CHECK_ARG(mode_ok(mode), "jacobian_det_fwd: mode must be 0, 1 (positions) or 3 (positions, clamped)");
  Geo G;
  if (const char* why = geo_of(N, ndim, dims, G)) JAC_FAIL("jacobian_det_fwd", why);
  if (N == 0) return ADVCHAIN_OK;
  if (ndim == 2 && mode == 0) return advchain_jacobian_det2d_fwd(field, det, N, dims, stream);
  StatsPart* none = nullptr;
  const dim3 grid(G.L.blocks), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  if (ndim == 2) {
#define LAUNCH(M) hipLaunchKernelGGL((k_jac2d_fwd<M, false>), grid, block, 0, st, field, det, none, N, G.H, G.W, G.L.chunks, G.L.strips, G.L.R)
    JAC_BY_MODE(mode, LAUNCH);
#undef LAUNCH
  } else {
#define LAUNCH(M) hipLaunchKernelGGL((k_jac3d_fwd<M, false>), grid, block, 0, st, field, det, none, N, G.D, G.H, G.W, G.L.chunks, G.L.strips, G.L.R)
    JAC_BY_MODE(mode, LAUNCH);
#undef LAUNCH
  }
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int64_t advchain_jacobian_det_workspace(int64_t N, int ndim, const int64_t* dims) {
  (void)N; (void)ndim; (void)dims;
  return 0;      // the backward recomputes the cofactors at the neighbours: nothing is staged
}

int advchain_jacobian_det_bwd(const float* grad_det, const float* field, float* grad_field, float* workspace, int64_t N,
                              int ndim, const int64_t* dims, int mode, void* stream) {
  (void)workspace;
  ADVCHAIN_CHECK_ARG(grad_det && field && grad_field, "jacobian_det_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536, "jacobian_det_bwd: bad N");
  ADVCHAIN_CHECK_ARG(mode_ok(mode), "jacobian_det_bwd: mode must be 0, 1 (positions) or 3 (positions, clamped)");
  Geo G;
  if (const char* why = geo_of(N, ndim, dims, G)) JAC_FAIL("jacobian_det_bwd", why);
  if (N == 0) return ADVCHAIN_OK;
  if (ndim == 2 && mode == 0) return advchain_jacobian_det2d_bwd(grad_det, field, grad_field, N, dims, stream);
  const dim3 grid(G.L.blocks), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  if (ndim == 2) {
#define LAUNCH(M) hipLaunchKernelGGL((k_jac2d_bwd<M>), grid, block, 0, st, grad_det, field, grad_field, N, G.H, G.W, G.L.chunks, G.L.strips, G.L.R)
    JAC_BY_MODE(mode, LAUNCH);
#undef LAUNCH
  } else {
#define LAUNCH(M) hipLaunchKernelGGL((k_jac3d_bwd<M>), grid, block, 0, st, grad_det, field, grad_field, N, G.D, G.H, G.W, G.L.chunks, G.L.strips, G.L.R)
    JAC_BY_MODE(mode, LAUNCH);
#undef LAUNCH
  }
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int64_t advchain_jacobian_stats_workspace(int64_t N, int ndim, const int64_t* dims) {
  Geo G;
  if (N < 0 || N >= 65536 || geo_of(N, ndim, dims, G)) return -1;
  return (int64_t)G.D * G.L.chunks * G.L.strips * N * (int64_t)(sizeof(StatsPart) / sizeof(float));
}

int advchain_jacobian_stats(const float* field, int64_t* neg, int64_t* nonpos, float* min, float* max, float* workspace,
                            int64_t N, int ndim, const int64_t* dims, int mode, void* stream) {
  ADVCHAIN_CHECK_ARG(field && neg && nonpos && min && max && workspace, "jacobian_stats: null pointer");
  ADVCHAIN_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "jacobian_stats: the workspace must be 16-byte aligned");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536, "jacobian_stats: bad N");
  ADVCHAIN_CHECK_ARG(mode_ok(mode), "jacobian_stats: mode must be 0, 1 (positions) or 3 (positions, clamped)");
  Geo G;
  if (const char* why = geo_of(N, ndim, dims, G)) JAC_FAIL("jacobian_stats", why);
  if (N == 0) return ADVCHAIN_OK;
  StatsPart* parts = reinterpret_cast<StatsPart*>(workspace);
  const int64_t per = (int64_t)G.D * G.L.chunks * G.L.strips;      // waves of one batch entry: consecutive slots
  const dim3 grid(G.L.blocks), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  float* nomap = nullptr;
  if (ndim == 2) {
#define LAUNCH(M) hipLaunchKernelGGL((k_jac2d_fwd<M, true>), grid, block, 0, st, field, nomap, parts, N, G.H, G.W, G.L.chunks, G.L.strips, G.L.R)
    JAC_BY_MODE(mode, LAUNCH);
#undef LAUNCH
  } else {
#define LAUNCH(M) hipLaunchKernelGGL((k_jac3d_fwd<M, true>), grid, block, 0, st, field, nomap, parts, N, G.D, G.H, G.W, G.L.chunks, G.L.strips, G.L.R)
    JAC_BY_MODE(mode, LAUNCH);
#undef LAUNCH
  }
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_stats_finish, dim3((unsigned)N), block, 0, st, parts, per, neg, nonpos, min, max);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
