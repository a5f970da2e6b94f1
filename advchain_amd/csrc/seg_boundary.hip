// Boundary (surface) loss of Kervadec et al. on signed distance maps, 2D and 3D, for gfx950:
//
//   advchain_boundary_fwd / advchain_boundary_bwd   <- common.loss.boundary_loss
//
// With p = softmax(logits) over the K planes and phi (N,K,dims) the signed distance maps (advchain_signed_maps, or the caller's)
//   loss = 1/(N V) sum_n sum_{v counted} sum_{k counted} omega_k p_k(v) phi_nk(v),     omega_k = w_k / sum of the counted w_j
// class 0 is not counted with ADVCHAIN_BOUNDARY_IGNORE_BACKGROUND; with labels a voxel labelled -100 is not counted (it stays
// in N V) and any other label outside [0, K) makes the value and the gradient NaN; without labels every voxel is counted.
//
// Forward, two launches (the scheme of seg_dice.hip):
//   k_boundary_fwd     grid (V / 1024, N): a lane owns 4 consecutive voxels (16-byte fp32 / 8-byte bf16 loads, or scalar loads of
//                      the same 4 voxels: no sum depends on the alignment).  ONE sweep over the K planes of logits and maps with
//                      an online max: s = sum exp(x_k - m) and a = sum omega_k phi_k exp(x_k - m) are rescaled together when the
//                      maximum moves, so t(v) = sum_k omega_k phi_k p_k = a / s.  lse and t are kept for the backward; one partial
//                      per workgroup.
//   k_seg_finish       (seg_common.h) one workgroup adds the partials in a fixed order and divides by N V.
// Backward, one launch: gx_j = gs / (N V) p_j (omega_j phi_j - t), zero at voxels that are not counted, rounded once to the
// logits' dtype.  No float atomics, no host read-back, every output written by a kernel; compiled without contraction so that the
// fp32 / bf16 and the vector / scalar instantiations round alike.
#include <math.h>

#include "common.h"
#include "seg_common.h"

namespace advchain {
namespace {

enum { BOUNDARY_IGNORE_BACKGROUND = 1 };

// what a voxel contributes: 1 (counted), 0 (not counted: -100 or past the end), NaN (a label outside [0, K))
template <bool VEC>
__device__ __forceinline__ void voxel_gates(const int64_t* __restrict__ lab, int cnt, int K, float (&gate)[kVox]) {
  int64_t y[kVox];
#pragma unroll
  for (int q = 0; q < kVox; ++q) y[q] = -100;                       // (defined without labels too; not read then)
  if (lab) ld4_labels<VEC>(lab, cnt, y);
#pragma unroll
  for (int q = 0; q < kVox; ++q) {
    if (!lab) gate[q] = q < cnt ? 1.f : 0.f;
    else gate[q] = y[q] == -100 ? 0.f : ((y[q] < 0 || y[q] >= K) ? qnan() : 1.f);
  }
}

template <typename ST, bool VEC>
__global__ void __launch_bounds__(kBlock)
k_boundary_fwd(const ST* __restrict__ x, const int64_t* __restrict__ lab, const float* __restrict__ maps,
               const float* __restrict__ weight, float* __restrict__ saved, float* __restrict__ part, int K, int64_t V, int first) {
  __shared__ float smem[4];
  const int64_t n = blockIdx.y;
  const int64_t v0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kVox;
  const int cnt = lane_count(V, v0);
  const ST* xn = x + n * K * V + v0;
  const float* fn = maps + n * K * V + v0;
  float gate[kVox];
  voxel_gates<VEC>(lab ? lab + n * V + v0 : nullptr, cnt, K, gate);
  const float wsum = counted_weight_sum(weight, first, K);

  float m[kVox], s[kVox], a[kVox];
#pragma unroll
  for (int q = 0; q < kVox; ++q) { m[q] = -INFINITY; s[q] = 0.f; a[q] = 0.f; }
  for (int c = 0; c < K; ++c) {
    float xc[kVox], fc[kVox];
    ld4<ST, VEC>(xn + (int64_t)c * V, cnt, xc);
    const bool counted = c >= first;
    if (counted) ld4<float, VEC>(fn + (int64_t)c * V, cnt, fc);
    const float om = counted ? (weight ? weight[c] : 1.f) / wsum : 0.f;
#pragma unroll
    for (int q = 0; q < kVox; ++q) {
      const float mn = fmaxf(m[q], xc[q]), ms = sub_max(mn);         // (a class masked with -inf in front: common.h)
      const float sc = __expf(m[q] - ms), e = __expf(xc[q] - ms);
      s[q] = s[q] * sc + e;
      a[q] = a[q] * sc + (counted ? (om * fc[q]) * e : 0.f);
      m[q] = mn;
    }
  }
  float l[kVox], t[kVox], sum[1] = {0.f};
#pragma unroll
  for (int q = 0; q < kVox; ++q) {
    l[q] = m[q] + logf(s[q]);
    t[q] = a[q] / s[q];
    sum[0] += gate[q] == 0.f ? 0.f : gate[q] * t[q];
  }
  if (saved) {
    st4<float, VEC>(saved + n * 2 * V + v0, cnt, l);
    st4<float, VEC>(saved + (n * 2 + 1) * V + v0, cnt, t);
  }
  block_sum<1>(sum, smem);
  if (threadIdx.x == 0) part[n * gridDim.x + blockIdx.x] = sum[0];
}

template <typename ST, bool VEC>
__global__ void __launch_bounds__(kBlock)
k_boundary_bwd(const ST* __restrict__ x, const int64_t* __restrict__ lab, const float* __restrict__ maps,
               const float* __restrict__ weight, const float* __restrict__ saved, const float* __restrict__ grad_scale,
               ST* __restrict__ gx, int K, int64_t V, int first, float inv_denom) {
  const int64_t n = blockIdx.y;
  const int64_t v0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kVox;
  const int cnt = lane_count(V, v0);
  if (cnt == 0) return;
  const int64_t base = n * K * V + v0;
  float gate[kVox], l[kVox], t[kVox];
  voxel_gates<VEC>(lab ? lab + n * V + v0 : nullptr, cnt, K, gate);
  ld4<float, VEC>(saved + n * 2 * V + v0, cnt, l);
  ld4<float, VEC>(saved + (n * 2 + 1) * V + v0, cnt, t);
  const float wsum = counted_weight_sum(weight, first, K);
  const float scale = (grad_scale ? grad_scale[0] : 1.f) * inv_denom;
  for (int c = 0; c < K; ++c) {
    float xc[kVox], fc[kVox], gc[kVox];
    ld4<ST, VEC>(x + base + (int64_t)c * V, cnt, xc);
    const bool counted = c >= first;
    if (counted) ld4<float, VEC>(maps + base + (int64_t)c * V, cnt, fc);
    const float om = counted ? (weight ? weight[c] : 1.f) / wsum : 0.f;
#pragma unroll
    for (int q = 0; q < kVox; ++q) {
      const float p = __expf(xc[q] - l[q]);
      const float g = scale * (p * ((counted ? om * fc[q] : 0.f) - t[q]));
      gc[q] = gate[q] == 0.f ? 0.f : gate[q] * g;
    }
    st4<ST, VEC>(gx + base + (int64_t)c * V, cnt, gc);
  }
}

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int64_t advchain_boundary_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims) {
  const int64_t V = seg_voxels(ndim, dims);
  if (V < 0 || !seg_shape_ok(N, K, V)) return -1;
  return N * seg_blocks(V);
}

int advchain_boundary_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* maps, const float* weight,
                          float* saved, float* workspace, float* value, int64_t N, int64_t K, int ndim, const int64_t* dims,
                          int flags, void* stream) {
  ADVCHAIN_CHECK_ARG(logits && maps && workspace && value, "boundary_fwd: null pointer");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "boundary_fwd: K must be in 1..65535");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(V > 0 && seg_shape_ok(N, K, V), "boundary_fwd: bad N, ndim or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "boundary_fwd: logits are fp32 (0) or bf16 (1)");
  ADVCHAIN_CHECK_ARG((flags & ~1) == 0, "boundary_fwd: unknown flags");
  const int first = (flags & BOUNDARY_IGNORE_BACKGROUND) ? 1 : 0;
  ADVCHAIN_CHECK_ARG(K > first, "boundary_fwd: no class left with ignore_background");
  const bool vec = V % 4 == 0 && aligned(logits, logits_bf16 ? 8 : 16) && aligned(labels, 16) && aligned(maps, 16) && aligned(saved, 16);
  const int64_t nb = seg_blocks(V);
  const dim3 grid((unsigned)nb, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  seg_dispatch(logits_bf16, false, vec, [&](auto st, auto, auto ve) {      // (no second flag)
    using ST = typename decltype(st)::type;
    hipLaunchKernelGGL((k_boundary_fwd<ST, decltype(ve)::value>), grid, dim3(kBlock), 0, s, (const ST*)logits, labels, maps, weight,
                       saved, workspace, (int)K, V, first);
  });
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seg_finish, dim3(1), dim3(kBlock), 0, s, workspace, N * nb, (float)(N * V), value);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_boundary_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* maps, const float* weight,
                          const float* saved, const float* grad_scale, void* grad_logits, int64_t N, int64_t K, int ndim,
                          const int64_t* dims, int flags, void* stream) {
  ADVCHAIN_CHECK_ARG(logits && maps && saved && grad_logits, "boundary_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "boundary_bwd: K must be in 1..65535");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(V > 0 && seg_shape_ok(N, K, V), "boundary_bwd: bad N, ndim or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "boundary_bwd: logits are fp32 (0) or bf16 (1)");
  ADVCHAIN_CHECK_ARG((flags & ~1) == 0, "boundary_bwd: unknown flags");
  const int first = (flags & BOUNDARY_IGNORE_BACKGROUND) ? 1 : 0;
  ADVCHAIN_CHECK_ARG(K > first, "boundary_bwd: no class left with ignore_background");
  const bool vec = V % 4 == 0 && aligned(logits, logits_bf16 ? 8 : 16) && aligned(labels, 16) && aligned(maps, 16) &&
                   aligned(saved, 16) && aligned(grad_logits, logits_bf16 ? 8 : 16);
  const dim3 grid((unsigned)seg_blocks(V), (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  seg_dispatch(logits_bf16, false, vec, [&](auto st, auto, auto ve) {
    using ST = typename decltype(st)::type;
    hipLaunchKernelGGL((k_boundary_bwd<ST, decltype(ve)::value>), grid, dim3(kBlock), 0, s, (const ST*)logits, labels, maps, weight,
                       saved, grad_scale, (ST*)grad_logits, (int)K, V, first, 1.f / (float)(N * V));
  });
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
