// Pieces shared by the consistency-loss translation units (loss.hip: K <= 16 in registers; loss_lp.hip: run-time K, typed
// loads; loss_ref.hip: the gradient w.r.t. the reference).
#pragma once
#include "common.h"

// exp of a softmax argument x - max <= 0: the library expf (13 VALU instructions: extended-precision argument reduction,
// ldexp, range selects) or v_exp_f32(x log2 e) (2; its argument product is rounded once: |x| 6e-8 relative, at most 2.2e-8
// absolute in a probability, against the 6e-8 of a correctly rounded exp).  A/B of tools/sessions/r06_s18.sh
#ifndef ADVCHAIN_SOFTMAX_FAST_EXP
#define ADVCHAIN_SOFTMAX_FAST_EXP 1
#endif
#if ADVCHAIN_SOFTMAX_FAST_EXP
#define ADVCHAIN_SM_EXP(x) __expf(x)
#else
#define ADVCHAIN_SM_EXP(x) expf(x)
#endif

namespace advchain {

__device__ __forceinline__ float hsm(int i) { return i == 1 ? 2.f : 1.f; }        // [1, 2, 1]
__device__ __forceinline__ float hdf(int i) { return i == 0 ? 1.f : (i == 1 ? 0.f : -1.f); }  // [1, 0, -1]

// stencil weights at tap (a0,a1,a2) in {0,1,2}^3 (a0 unused in 2D); the contour loss of seg_loss.hip takes them from here too
template <int DIM>
__device__ __forceinline__ void stencil_w(int a0, int a1, int a2, float& wa, float& wb) {
  if (DIM == 2) {
    // conv2d cross-correlation, kernel[a1][a2]: Sobel-x = h[a1]*hp[a2], Sobel-y = hp[a1]*h[a2]
    wa = hsm(a1) * hdf(a2);
    wb = hdf(a1) * hsm(a2);
  } else {
    wa = hsm(a0) * hdf(a1) * hsm(a2);
    wb = hsm(a0) * hsm(a1) * hdf(a2);
  }
}

// 'kl' (loss.py:239-248): m * p * (log p - log q).  is_gt: p = where(ref == 0, 1e-8, 1 - 1e-8) (= 1.0f in fp32), log p = log(p)
__device__ __forceinline__ float kl_prob(float t, int is_gt) { return is_gt ? (t == 0.f ? 1e-8f : 1.f) : t; }
__device__ __forceinline__ float kl_term(float t, float log_t, float log_q, float m, int is_gt) {
  const float p = kl_prob(t, is_gt);
  const float lp = is_gt ? logf(p) : log_t;
  return m * (p * lp) - m * (p * log_q);
}

// Where a forward kernel's workgroup partial of sum `row` (0 mse, 1 edge A, 2 edge B, 3 kl) goes.  The forward kernels end in
// a parameter pack: EMPTY in the default mode -- a float atomic into slot sum_slot() of the row's 64 accumulators, and the
// kernel's name, parameters and instructions are what they were before the pack -- or one SumsOrdered (the *_fwd_ord entries,
// deterministic mode): `sums` is then a [4][stride] buffer and every workgroup STORES its partial into its own cell of the
// row (zeros included, so the buffer needs no clearing), for k_consistency_finish_ord to add up in a fixed order.
struct SumsOrdered { int stride; };
__device__ __forceinline__ void sums_put(float* __restrict__ sums, int row, float v) {
  atomic_add_f32(sums + row * kSumSlots + sum_slot(), v);
}
__device__ __forceinline__ void sums_put(float* __restrict__ sums, int row, float v, const SumsOrdered& o) {
  sums[(int64_t)row * o.stride + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = v;
}
// (loss_lp.hip: the class weights of the cw entries travel in the same pack, in front)
__device__ __forceinline__ void sums_put(float* __restrict__ sums, int row, float v, const float*) { sums_put(sums, row, v); }
__device__ __forceinline__ void sums_put(float* __restrict__ sums, int row, float v, const float*, const SumsOrdered& o) {
  sums_put(sums, row, v, o);
}
// Host side of the *_fwd_ord entries: the grid of a launch fits the buffer, and the rows it writes get its workgroup count.
struct OrdCounts {
  int64_t stride;
  int32_t* counts;     // [4], host
  bool fits(dim3 g) const { return (int64_t)g.x * g.y * g.z <= stride; }
  void set(int row, dim3 g) const { counts[row] = (int32_t)((int64_t)g.x * g.y * g.z); }
};

// ---- the run-time-K kernels (loss_lp.hip, loss_ref.hip) ----

// running max / sum of exp(x - max): ONE exp per element (the other factor of the usual two is exp(0)).  sub_max (common.h):
// a second class masked with -inf in front adds exp(-inf) = 0 instead of exp(NaN).
__device__ __forceinline__ void online_step(float x, float& mx, float& s) {
  const float d = x - sub_max(mx);
  const float e = ADVCHAIN_SM_EXP(-fabsf(d));
  if (d > 0.f) { s = s * e + 1.f; mx = x; }
  else s += e;
}

// The spatial tile of a workgroup and its one-voxel halo.  256 threads: OUTS outputs and SLOTS halo voxels per thread.
template <int DIM>
struct WTile {
  static constexpr int TX = DIM == 2 ? 64 : 32, TY = 8, TZ = DIM == 2 ? 1 : 4;
  static constexpr int HX = TX + 2, HY = TY + 2, HZ = DIM == 2 ? 1 : TZ + 2;
  static constexpr int NH = HX * HY * HZ, NO = TX * TY * TZ;
  static constexpr int SLOTS = (NH + kBlock - 1) / kBlock, OUTS = NO / kBlock;
  int x0, y0, z0;
  __device__ __forceinline__ WTile(const Dims& d) {
    const int tx = (d.s2 + TX - 1) / TX, ty = (d.s1 + TY - 1) / TY;
    const int b = blockIdx.x;
    x0 = (b % tx) * TX;
    y0 = ((b / tx) % ty) * TY;
    z0 = (b / (tx * ty)) * TZ;
  }
  // volume index of halo slot e, or -1 (outside the volume or past the last slot)
  __device__ __forceinline__ int halo_voxel(int e, const Dims& d) const {
    const int hx = e % HX, hy = (e / HX) % HY, hz = e / (HX * HY);
    const int gx = x0 + hx - 1, gy = y0 + hy - 1, gz = DIM == 3 ? z0 + hz - 1 : 0;
    const bool in = e < NH && gx >= 0 && gx < d.s2 && gy >= 0 && gy < d.s1 && gz >= 0 && gz < d.s0;
    return in ? (gz * d.s1 + gy) * d.s2 + gx : -1;
  }
  // output o of the tile: its volume index (-1 outside) and the LDS index of its (-1,-1,-1) neighbour
  __device__ __forceinline__ int out_voxel(int o, const Dims& d, int& corner) const {
    const int ox = o % TX, oy = (o / TX) % TY, oz = o / (TX * TY);
    corner = (oz * HY + oy) * HX + ox;
    const int gx = x0 + ox, gy = y0 + oy, gz = z0 + oz;
    return (gx < d.s2 && gy < d.s1 && gz < d.s0) ? (gz * d.s1 + gy) * d.s2 + gx : -1;
  }
  static int64_t count(const Dims& d) {
    return (int64_t)((d.s2 + TX - 1) / TX) * ((d.s1 + TY - 1) / TY) * ((d.s0 + TZ - 1) / TZ);
  }
};

// The two 3^d stencils of one output from an LDS tile (`corner`: index of the output's (-1,-1,-1) neighbour), taps in the
// order of loss.hip's kernels.
// (3D, measured: a thread's four outputs are a column along z, and sharing the in-plane sums of its six planes -- 54 LDS
// reads per stencil instead of 4 x 27 -- costs 192 VGPRs and was slower in the forward and no faster in the backward than
// this form at 4 x 20 x 128 x 128 x 64: not kept, LESSONS 79.)
template <int DIM>
__device__ __forceinline__ void tile_stencil(const float* __restrict__ bufa, const float* __restrict__ bufb, int corner,
                                             float& ga, float& gb) {
  using T = WTile<DIM>;
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int a0 = (DIM == 3 ? 0 : 1); a0 < (DIM == 3 ? 3 : 2); ++a0)
#pragma unroll
    for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
      for (int a2 = 0; a2 < 3; ++a2) {
        float wa, wb;
        stencil_w<DIM>(a0, a1, a2, wa, wb);
        const int q = corner + ((DIM == 3 ? a0 : 0) * T::HY + a1) * T::HX + a2;
        sa += wa * bufa[q];
        sb += wb * bufb[q];
      }
  ga = sa;
  gb = sb;
}

// The adjoints of the two stencils (tap a reads the voxel at u - (a - 1)), without the taps whose weight is zero (the
// [1, 0, -1] factor: 3 of 9 taps in 2D, 9 of 27 in 3D, per stencil): a third fewer LDS reads.
template <int DIM>
__device__ __forceinline__ void adjoint_stencil(const float* __restrict__ bufa, const float* __restrict__ bufb, int corner,
                                                float& ga, float& gb) {
  using T = WTile<DIM>;
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int a0 = (DIM == 3 ? 0 : 1); a0 < (DIM == 3 ? 3 : 2); ++a0)
#pragma unroll
    for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
      for (int a2 = 0; a2 < 3; ++a2) {
        float wa, wb;
        stencil_w<DIM>(a0, a1, a2, wa, wb);
        const int q = corner + ((DIM == 3 ? 2 - a0 : 0) * T::HY + (2 - a1)) * T::HX + (2 - a2);
        if (wa != 0.f) sa += wa * bufa[q];
        if (wb != 0.f) sb += wb * bufb[q];
      }
  ga = sa;
  gb = sb;
}

// the R_k tile and its halo into one pair of LDS buffers (zero outside the volume: R is zero there)
template <int DIM>
__device__ __forceinline__ void stage_R(float (*buf)[WTile<DIM>::NH], const float* __restrict__ Ra, const float* __restrict__ Rb,
                                        const int (&hv)[WTile<DIM>::SLOTS]) {
  using T = WTile<DIM>;
#pragma unroll
  for (int j = 0; j < T::SLOTS; ++j) {
    const int e = threadIdx.x + j * kBlock;
    const int c = max(hv[j], 0);
    const float ra = Ra[c], rb = Rb[c];          // unconditional loads from a clamped index: all in flight together
    if (e < T::NH) {
      buf[0][e] = hv[j] >= 0 ? ra : 0.f;
      buf[1][e] = hv[j] >= 0 ? rb : 0.f;
    }
  }
}

}  // namespace advchain
