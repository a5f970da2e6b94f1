// Deformation helpers of advchain/augmentor/adv_morph.py for gfx950:
//
//   advchain_image_diff2d_fwd/bwd     <- calculate_image_diff           (adv_morph.py:57-77)
//   advchain_jacobian_det2d_fwd/bwd   <- calculate_jacobian_determinant (adv_morph.py:80-100)
//   advchain_expo_start               <- get_base_grid + duv / 2^n + the in-place add of vectorFieldExponentiation{2,3}D
//                                        (adv_morph.py:126-130,153-163)
//   advchain_sumsq_ordered            <- the torch.norm(duv_interval) of vectorFieldExponentiation3D (adv_morph.py:159)
//
// Stencils: one wave owns 62 consecutive columns of one plane (lanes 1..62; lanes 0 and 63 load the neighbouring columns
// and store nothing) and marches down a strip of rows, keeping the rows above and below in registers.  The x neighbours
// come from the adjacent lanes through DPP shifts, so every value is loaded once per strip by one lane; only the strip's
// halo rows and the two halo lanes are read twice (from the caches).  All lanes of a wave stay active through the shifts:
// the loads clamp the column, and only the store is predicated.
//
// Rounding: this file is compiled with -ffp-contract=off (build.py), so every +, -, * rounds once, in the reference's
// order -- the forwards equal the reference's fp32 values bit for bit.  The backwards are the adjoints of the stencils in
// gather form (each output pixel reads what it needs; no atomics), so they are bitwise reproducible.
#include "common.h"
#include "diff_stencil.h"

namespace advchain {
namespace {

__global__ void __launch_bounds__(kBlock) k_diff2d_fwd(const float* __restrict__ in, float* __restrict__ dx,
                                                       float* __restrict__ dy, int64_t planes, int H, int W, int chunks,
                                                       int strips, int R) {
  Strip s;
  if (!strip_of(planes, H, W, chunks, strips, R, s)) return;
  const int64_t base = s.plane * H * W;
  const float* p = in + base;
  float prev = row_at(p, s.y0 - 1, H, W, s.xc), cur = row_at(p, s.y0, H, W, s.xc);
  for (int y = s.y0; y < s.y1; ++y) {
    const float next = row_at(p, y + 1, H, W, s.xc);
    const float l = lane_prev_f(cur), r = lane_next_f(cur);
    if (s.store) {
      const int64_t o = base + (int64_t)y * W + s.x;
      dx[o] = diff1(l, cur, r, s.x, W);
      dy[o] = diff1(prev, cur, next, y, H);
    }
    prev = cur;
    cur = next;
  }
}

__global__ void __launch_bounds__(kBlock) k_diff2d_bwd(const float* __restrict__ gdx, const float* __restrict__ gdy,
                                                       float* __restrict__ gin, int64_t planes, int H, int W, int chunks,
                                                       int strips, int R) {
  Strip s;
  if (!strip_of(planes, H, W, chunks, strips, R, s)) return;
  const int64_t base = s.plane * H * W;
  const float* px = gdx ? gdx + base : nullptr;
  const float* py = gdy ? gdy + base : nullptr;
  float prev = 0.f, cur = 0.f;
  if (py) { prev = row_at(py, s.y0 - 1, H, W, s.xc); cur = row_at(py, s.y0, H, W, s.xc); }
  for (int y = s.y0; y < s.y1; ++y) {
    float a = 0.f;
    if (px) {
      const float c = px[(int64_t)y * W + s.xc];
      a = diff1_adj(lane_prev_f(c), c, lane_next_f(c), s.x, W);
    }
    float next = 0.f;
    if (py) {
      next = row_at(py, y + 1, H, W, s.xc);
      a += diff1_adj(prev, cur, next, y, H);
    }
    if (s.store) gin[base + (int64_t)y * W + s.x] = a;
    prev = cur;
    cur = next;
  }
}

__global__ void __launch_bounds__(kBlock) k_jacobian2d_fwd(const float* __restrict__ field, float* __restrict__ det,
                                                           int64_t N, int H, int W, int chunks, int strips, int R) {
  Strip s;
  if (!strip_of(N, H, W, chunks, strips, R, s)) return;
  const int64_t P = (int64_t)H * W;
  const float* u = field + s.plane * 2 * P;
  const float* v = u + P;
  float up = row_at(u, s.y0 - 1, H, W, s.xc), uc = row_at(u, s.y0, H, W, s.xc);
  float vp = row_at(v, s.y0 - 1, H, W, s.xc), vc = row_at(v, s.y0, H, W, s.xc);
  for (int y = s.y0; y < s.y1; ++y) {
    const float un = row_at(u, y + 1, H, W, s.xc), vn = row_at(v, y + 1, H, W, s.xc);
    const float dxx = diff1(lane_prev_f(uc), uc, lane_next_f(uc), s.x, W);
    const float dyx = diff1(lane_prev_f(vc), vc, lane_next_f(vc), s.x, W);
    if (s.store) det[s.plane * P + (int64_t)y * W + s.x] = det_of(dxx, diff1(up, uc, un, y, H), dyx, diff1(vp, vc, vn, y, H));
    up = uc; uc = un;
    vp = vc; vc = vn;
  }
}

// the four products of the backward at one row: p1 = g (1 + dyy), p2 = g dyx, p3 = g (1 + dxx), p4 = g dxy
struct Prod { float p1, p2, p3, p4; };

__device__ __forceinline__ Prod prods(float um, float u0, float up, float vm, float v0, float vp, float g, int x, int r,
                                      int H, int W) {
  const float dxx = diff1(lane_prev_f(u0), u0, lane_next_f(u0), x, W);
  const float dyx = diff1(lane_prev_f(v0), v0, lane_next_f(v0), x, W);
  const float dxy = diff1(um, u0, up, r, H), dyy = diff1(vm, v0, vp, r, H);
  Prod q;
  q.p1 = g * (1.f + dyy);
  q.p2 = g * dyx;
  q.p3 = g * (1.f + dxx);
  q.p4 = g * dxy;
  return q;
}

// grad_u = Dx^T(g (1 + dyy)) - Dy^T(g dyx),  grad_v = Dy^T(g (1 + dxx)) - Dx^T(g dxy): every output pixel gathers the
// products of its 5-point cross, which the wave recomputes from u, v (rows y-2 .. y+2) and g (rows y-1 .. y+1)
__global__ void __launch_bounds__(kBlock) k_jacobian2d_bwd(const float* __restrict__ gdet, const float* __restrict__ field,
                                                           float* __restrict__ gfield, int64_t N, int H, int W, int chunks,
                                                           int strips, int R) {
  Strip s;
  if (!strip_of(N, H, W, chunks, strips, R, s)) return;
  const int64_t P = (int64_t)H * W;
  const float* u = field + s.plane * 2 * P;
  const float* v = u + P;
  const float* g = gdet + s.plane * P;
  const int y0 = s.y0, x = s.x, xc = s.xc;
  float u0 = row_at(u, y0, H, W, xc), u1 = row_at(u, y0 + 1, H, W, xc);
  float v0 = row_at(v, y0, H, W, xc), v1 = row_at(v, y0 + 1, H, W, xc);
  Prod pm = {0.f, 0.f, 0.f, 0.f}, pc, pn;
  {
    const float um1 = row_at(u, y0 - 1, H, W, xc), vm1 = row_at(v, y0 - 1, H, W, xc);
    if (y0 >= 1) {
      const float um2 = row_at(u, y0 - 2, H, W, xc), vm2 = row_at(v, y0 - 2, H, W, xc);
      pm = prods(um2, um1, u0, vm2, vm1, v0, row_at(g, y0 - 1, H, W, xc), x, y0 - 1, H, W);
    }
    pc = prods(um1, u0, u1, vm1, v0, v1, row_at(g, y0, H, W, xc), x, y0, H, W);
  }
  for (int y = y0; y < s.y1; ++y) {
    // (u0, u1) are rows y, y + 1 here
    const float u2 = row_at(u, y + 2, H, W, xc), v2 = row_at(v, y + 2, H, W, xc);
    if (y + 1 < H) pn = prods(u0, u1, u2, v0, v1, v2, row_at(g, y + 1, H, W, xc), x, y + 1, H, W);
    else pn = Prod{0.f, 0.f, 0.f, 0.f};
    const float ax1 = diff1_adj(lane_prev_f(pc.p1), pc.p1, lane_next_f(pc.p1), x, W);
    const float ax4 = diff1_adj(lane_prev_f(pc.p4), pc.p4, lane_next_f(pc.p4), x, W);
    if (s.store) {
      const int64_t o = s.plane * 2 * P + (int64_t)y * W + x;
      gfield[o] = ax1 - diff1_adj(pm.p2, pc.p2, pn.p2, y, H);
      gfield[o + P] = diff1_adj(pm.p3, pc.p3, pn.p3, y, H) - ax4;
    }
    pm = pc; pc = pn;
    u0 = u1; u1 = u2;
    v0 = v1; v1 = v2;
  }
}

// phi0 = identity + duv * inv (inv = 2^-n: the product is the reference's exact duv / 2^n)
__global__ void __launch_bounds__(kBlock) k_expo_start(const float* __restrict__ duv, float* __restrict__ phi0, float inv,
                                                       int64_t total, int ndim, Dims d) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= total) return;
  const int64_t V = d.voxels();
  const int64_t p = i % V;
  const int c = (int)((i / V) % ndim);
  const int i2 = (int)(p % d.s2), i1 = (int)((p / d.s2) % d.s1), i0 = (int)(p / ((int64_t)d.s2 * d.s1));
  const float id = c == 0 ? lin_coord(i2, d.s2) : (c == 1 ? lin_coord(i1, d.s1) : lin_coord(i0, d.s0));
  phi0[i] = id + duv[i] * inv;
}

// sum of squares: one partial per workgroup (fixed grid-stride order, fixed tree), then one workgroup adds the partials in
// order -- the value is a deterministic function of x
__global__ void __launch_bounds__(kBlock) k_sumsq_partial(const float* __restrict__ x, int64_t n, float* __restrict__ partials) {
  __shared__ float smem[4];
  float v[1] = {0.f};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const float a = x[i];
    v[0] += a * a;
  }
  block_sum<1>(v, smem);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(kBlock) k_sum_ordered(const float* __restrict__ partials, int nb, float* __restrict__ out) {
  __shared__ float smem[4];
  float v[1] = {0.f};
  for (int i = threadIdx.x; i < nb; i += kBlock) v[0] += partials[i];
  block_sum<1>(v, smem);
  if (threadIdx.x == 0) out[0] = v[0];
}

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int advchain_image_diff2d_fwd(const float* in, float* dx, float* dy, int64_t N, int64_t C, const int64_t* dims,
                              void* stream) {
  ADVCHAIN_CHECK_ARG(in && dx && dy, "image_diff2d_fwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536 && C >= 0 && C < (1 << 24), "image_diff2d_fwd: bad N or C");
  ADVCHAIN_CHECK_ARG(hw_ok(dims), "image_diff2d_fwd: H and W must be at least 2");
  if (N == 0 || C == 0) return ADVCHAIN_OK;
  StripLaunch L;
  ADVCHAIN_CHECK_ARG(strip_launch(N * C, (int)dims[0], (int)dims[1], L), "image_diff2d_fwd: too large");
  hipLaunchKernelGGL(k_diff2d_fwd, dim3(L.blocks), dim3(kBlock), 0, (hipStream_t)stream, in, dx, dy, N * C, (int)dims[0],
                     (int)dims[1], L.chunks, L.strips, L.R);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_image_diff2d_bwd(const float* grad_dx, const float* grad_dy, float* grad_in, int64_t N, int64_t C,
                              const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(grad_in && (grad_dx || grad_dy), "image_diff2d_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536 && C >= 0 && C < (1 << 24), "image_diff2d_bwd: bad N or C");
  ADVCHAIN_CHECK_ARG(hw_ok(dims), "image_diff2d_bwd: H and W must be at least 2");
  if (N == 0 || C == 0) return ADVCHAIN_OK;
  StripLaunch L;
  ADVCHAIN_CHECK_ARG(strip_launch(N * C, (int)dims[0], (int)dims[1], L), "image_diff2d_bwd: too large");
  hipLaunchKernelGGL(k_diff2d_bwd, dim3(L.blocks), dim3(kBlock), 0, (hipStream_t)stream, grad_dx, grad_dy, grad_in, N * C,
                     (int)dims[0], (int)dims[1], L.chunks, L.strips, L.R);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_jacobian_det2d_fwd(const float* field, float* det, int64_t N, const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(field && det, "jacobian_det2d_fwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536, "jacobian_det2d_fwd: bad N");
  ADVCHAIN_CHECK_ARG(hw_ok(dims), "jacobian_det2d_fwd: H and W must be at least 2");
  if (N == 0) return ADVCHAIN_OK;
  StripLaunch L;
  ADVCHAIN_CHECK_ARG(strip_launch(N, (int)dims[0], (int)dims[1], L), "jacobian_det2d_fwd: too large");
  hipLaunchKernelGGL(k_jacobian2d_fwd, dim3(L.blocks), dim3(kBlock), 0, (hipStream_t)stream, field, det, N, (int)dims[0],
                     (int)dims[1], L.chunks, L.strips, L.R);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_jacobian_det2d_bwd(const float* grad_det, const float* field, float* grad_field, int64_t N, const int64_t* dims,
                                void* stream) {
  ADVCHAIN_CHECK_ARG(grad_det && field && grad_field, "jacobian_det2d_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536, "jacobian_det2d_bwd: bad N");
  ADVCHAIN_CHECK_ARG(hw_ok(dims), "jacobian_det2d_bwd: H and W must be at least 2");
  if (N == 0) return ADVCHAIN_OK;
  StripLaunch L;
  ADVCHAIN_CHECK_ARG(strip_launch(N, (int)dims[0], (int)dims[1], L), "jacobian_det2d_bwd: too large");
  hipLaunchKernelGGL(k_jacobian2d_bwd, dim3(L.blocks), dim3(kBlock), 0, (hipStream_t)stream, grad_det, field, grad_field, N,
                     (int)dims[0], (int)dims[1], L.chunks, L.strips, L.R);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_expo_start(const float* duv, float* phi0, float inv, int64_t N, int ndim, const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(duv && phi0, "expo_start: null pointer");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536, "expo_start: bad N");
  ADVCHAIN_CHECK_ARG(dims && (ndim == 2 || ndim == 3), "expo_start: bad ndim");
  for (int i = 0; i < ndim; ++i) ADVCHAIN_CHECK_ARG(dims[i] >= 1 && dims[i] <= (1 << 24), "expo_start: bad dims");
  Dims d;
  if (ndim == 3) { d.s0 = (int)dims[0]; d.s1 = (int)dims[1]; d.s2 = (int)dims[2]; }
  else { d.s0 = 1; d.s1 = (int)dims[0]; d.s2 = (int)dims[1]; }
  ADVCHAIN_CHECK_ARG(d.voxels() < (1ll << 31), "expo_start: per-sample volume too large");
  const int64_t total = N * ndim * d.voxels();
  if (total == 0) return ADVCHAIN_OK;
  ADVCHAIN_CHECK_ARG((total + kBlock - 1) / kBlock <= 0x7fffffffll, "expo_start: too large");
  hipLaunchKernelGGL(k_expo_start, dim3((unsigned)advchain_blocks(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, duv,
                     phi0, inv, total, ndim, d);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_sumsq_ordered(const float* x, int64_t n, float* partials, float* out, void* stream) {
  ADVCHAIN_CHECK_ARG(x && partials && out, "sumsq_ordered: null pointer");
  ADVCHAIN_CHECK_ARG(n >= 1, "sumsq_ordered: n must be at least 1");
  int64_t nb = (n + kBlock * 16 - 1) / (kBlock * 16);
  if (nb > 1024) nb = 1024;      // ADVCHAIN_SUMSQ_PARTIALS
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sumsq_partial, dim3((unsigned)nb), dim3(kBlock), 0, s, x, n, partials);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sum_ordered, dim3(1), dim3(kBlock), 0, s, partials, (int)nb, out);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
