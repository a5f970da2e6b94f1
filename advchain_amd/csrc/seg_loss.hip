// Supervised segmentation losses of advchain/common/loss.py for gfx950:
//
//   advchain_ce2d_fwd/bwd      <- cross_entropy_2D  (loss.py:274-326): log_softmax over K + nll / soft-target sum
//   advchain_contour_fwd/bwd   <- contour_loss      (loss.py:102-220): Sobel edge energy of the class-summed map (Q14)
//   advchain_one_hot           <- One_Hot           (loss.py:252-271)
//
// Cross entropy: one streaming pass per pixel with an online max / sum-of-exp over the K planes (coalesced across pixels,
// 4 pixels per lane with 16-byte fp32 / 8-byte bf16 loads); the label's logit (or sum w t x and sum w t of a soft target) is
// picked up in the same pass, lse = max + log(sum) is saved per pixel for the backward.  A label is only ever COMPARED with the
// class index, never used as an address.  The class weights are normalised in registers (w / sum(w) * K, loss.py:290,316).
//
// Contour: the reference repeats its filter over the in- and out-channel axes (2D) or keeps one output channel (3D), so the loss
// is the edge energy of ONE field u = sum_{c in S} input_c - sum_{c in S} target_c (S = classes first_class..K-1):
//   2D: 1/2 [mean(w (Sx*u)^2) + mean(w (Sy*u)^2)],   3D: 1/3 [2 mean(w (A*u)^2) + mean(w (B*u)^2)]
// with w the mean of m^2 over the first min(|S|, mask_channels) mask channels.  u is built on the fly from the K planes into an
// LDS tile (64 x 8 outputs + halo) that marches along the slowest axis in 3D (ring of three planes).  The forward keeps
// R = (2 c_A w (A*u), 2 c_B w (B*u)) for the backward, which is the adjoint stencil over R.
//
// Reductions: one partial per workgroup into the caller's workspace, then ONE workgroup adds them in a fixed order and applies
// the normaliser -- no float atomics, the value is bitwise reproducible.  Two launches per direction at most.
#include "common.h"
#include "loss_common.h"
#include "seg_common.h"

namespace advchain {
namespace {

constexpr int kTX = 64;                 // contour tile: outputs along the fastest axis (one wave per row)
constexpr int kTY = 8;                  // rows of the tile (4 waves x 2)
constexpr int kPW = kTX + 2, kPH = kTY + 2, kPlane = kPW * kPH;
constexpr int kZChunk = 8;              // 3D: planes marched by one workgroup

// ---- cross entropy ------------------------------------------------------------------------------------------------------
// lane: VEC pixels p0..p0+VEC-1 of one image (HW % VEC == 0).  partial[block] = sum over its pixels of the per-pixel loss.
template <typename ST, bool SOFT, int VEC>
__global__ void __launch_bounds__(kBlock)
k_ce_fwd(const ST* __restrict__ x, const int64_t* __restrict__ lab, const float* __restrict__ soft,
         const float* __restrict__ weight, float* __restrict__ lse_out, float* __restrict__ partial, int K, int64_t HW,
         int64_t P) {
  __shared__ float smem[4];
  const int64_t p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
  float acc[1] = {0.f};
  if (p0 < P) {
    const int64_t n = p0 / HW, v = p0 - n * HW;
    const int64_t base = n * K * HW + v;
    const float wsum = weight ? weight_sum(weight, K) : 1.f, Kf = (float)K;
    float m[VEC], s[VEC], a[VEC], b[VEC];
    int64_t y[VEC];
    if constexpr (!SOFT) ld_labels<VEC>(lab + p0, y);
#pragma unroll
    for (int q = 0; q < VEC; ++q) { m[q] = -INFINITY; s[q] = 0.f; a[q] = SOFT ? 0.f : qnan(); b[q] = SOFT ? 0.f : qnan(); }
    for (int c = 0; c < K; ++c) {
      float xc[VEC], tc[VEC];
      ld<ST, VEC>(x + base + (int64_t)c * HW, xc);
      if constexpr (SOFT) ld<float, VEC>(soft + base + (int64_t)c * HW, tc);
      const float wc = class_weight(weight, c, wsum, Kf);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const float mn = fmaxf(m[q], xc[q]), ms = sub_max(mn);       // (a class masked with -inf in front: common.h)
        s[q] = s[q] * __expf(m[q] - ms) + __expf(xc[q] - ms);
        m[q] = mn;
        if constexpr (SOFT) {
          const float wt = wc * tc[q];
          a[q] = fmaf(wt, xc[q], a[q]);       // sum w t x
          b[q] += wt;                         // sum w t
        } else if (y[q] == c) {
          a[q] = xc[q];                       // the label's logit
          b[q] = wc;                          // its class weight
        }
      }
    }
    float l[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      l[q] = m[q] + logf(s[q]);
      if constexpr (SOFT) acc[0] += b[q] * l[q] - a[q];
      else acc[0] += (y[q] == -100) ? 0.f : b[q] * (l[q] - a[q]);   // out of [0,K) and not -100: a, b stay NaN
    }
    if (lse_out) st<float, VEC>(lse_out + p0, l);
  }
  block_sum<1>(acc, smem);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}

// grad_x_c = gs / denom * (W p_c - w_c t_c),  W = sum_c w_c t_c (label: w_y, 0 at ignore_index);
// grad_t_c = gs / denom * w_c (lse - x_c)  (soft target only)
template <typename ST, bool SOFT, int VEC>
__global__ void __launch_bounds__(kBlock)
k_ce_bwd(const ST* __restrict__ x, const int64_t* __restrict__ lab, const float* __restrict__ soft,
         const float* __restrict__ weight, const float* __restrict__ lse, const float* __restrict__ grad_scale,
         ST* __restrict__ gx, float* __restrict__ gt, int K, int64_t HW, int64_t P, float denom) {
  const int64_t p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
  if (p0 >= P) return;
  const int64_t n = p0 / HW, v = p0 - n * HW;
  const int64_t base = n * K * HW + v;
  const float wsum = weight ? weight_sum(weight, K) : 1.f, Kf = (float)K;
  const float g = (grad_scale ? grad_scale[0] : 1.f) / denom;
  float l[VEC], W[VEC];
  int64_t y[VEC];
  ld<float, VEC>(lse + p0, l);
  if constexpr (SOFT) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) W[q] = 0.f;
    for (int c = 0; c < K; ++c) {
      float tc[VEC];
      ld<float, VEC>(soft + base + (int64_t)c * HW, tc);
      const float wc = class_weight(weight, c, wsum, Kf);
#pragma unroll
      for (int q = 0; q < VEC; ++q) W[q] += wc * tc[q];
    }
  } else {
    ld_labels<VEC>(lab + p0, y);
#pragma unroll
    for (int q = 0; q < VEC; ++q) W[q] = (y[q] == -100) ? 0.f : qnan();
    for (int c = 0; c < K; ++c) {
      const float wc = class_weight(weight, c, wsum, Kf);
#pragma unroll
      for (int q = 0; q < VEC; ++q)
        if (y[q] == c) W[q] = wc;
    }
  }
  for (int c = 0; c < K; ++c) {
    float xc[VEC], tc[VEC], gc[VEC], gtc[VEC];
    ld<ST, VEC>(x + base + (int64_t)c * HW, xc);
    if constexpr (SOFT) ld<float, VEC>(soft + base + (int64_t)c * HW, tc);
    const float wc = class_weight(weight, c, wsum, Kf);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      const float p = __expf(xc[q] - l[q]);
      const float wt = SOFT ? wc * tc[q] : (y[q] == c ? wc : 0.f);
      gc[q] = g * (W[q] * p - wt);
      gtc[q] = g * (wc * (l[q] - xc[q]));
    }
    if (gx) st<ST, VEC>(gx + base + (int64_t)c * HW, gc);
    if constexpr (SOFT)
      if (gt) st<float, VEC>(gt + base + (int64_t)c * HW, gtc);
  }
}

// ---- contour ------------------------------------------------------------------------------------------------------------
// taps (a0, a1, a2) in {0,1,2}^3 of the cross-correlations (a0 unused in 2D): 2D A = Sobel-x, B = Sobel-y;
// 3D (Q14) A = h (x) hp (x) h (conv_x and conv_y alike), B = h (x) h (x) hp -- the stencils of the consistency loss (loss_common.h)
template <int DIM>
__device__ __forceinline__ float tap_a(int a0, int a1, int a2) { float wa, wb; stencil_w<DIM>(a0, a1, a2, wa, wb); return wa; }
template <int DIM>
__device__ __forceinline__ float tap_b(int a0, int a1, int a2) { float wa, wb; stencil_w<DIM>(a0, a1, a2, wa, wb); return wb; }

__device__ __forceinline__ int ring_slot(int z) { return (z + 3) % 3; }   // z >= -1

struct TileGeom {
  int n, tx0, ty0, z0, z1;
  __device__ TileGeom(const Dims& d, int tiles_x, int zc) {
    n = blockIdx.z;
    tx0 = (int)(blockIdx.x % tiles_x) * kTX;
    ty0 = (int)(blockIdx.x / tiles_x) * kTY;
    z0 = blockIdx.y * zc;
    z1 = min(z0 + zc, d.s0);
  }
};

// u (N, dims) at voxel `o` of plane-major offset: sum_{c >= c0} in_c - sum_{c >= c0} T_c
template <bool SOFT>
__device__ __forceinline__ float field_u(const float* __restrict__ in, const int64_t* __restrict__ lab,
                                         const float* __restrict__ soft, int64_t nK, int64_t V, int64_t o, int64_t nV,
                                         int K, int c0) {
  float sx = 0.f, st_ = 0.f;
  for (int c = c0; c < K; ++c) {
    sx += in[(nK + c) * V + o];
    if constexpr (SOFT) st_ += soft[(nK + c) * V + o];
  }
  if constexpr (!SOFT) {
    const int64_t y = lab[nV + o];
    st_ = (y >= c0 && y < K) ? 1.f : ((y >= 0 && y < c0) ? 0.f : qnan());
  }
  return sx - st_;
}

template <int DIM, bool SOFT>
__global__ void __launch_bounds__(kBlock)
k_contour_fwd(const float* __restrict__ in, const int64_t* __restrict__ lab, const float* __restrict__ soft,
              const float* __restrict__ mask, float* __restrict__ R, float* __restrict__ partial, int K, int c0,
              int mask_ch, int mask_used, Dims d, int tiles_x, int zc, float ca, float cb) {
  __shared__ float ring[DIM == 3 ? 3 : 1][kPlane];
  __shared__ float smem[4];
  const TileGeom t(d, tiles_x, zc);
  const int64_t V = d.voxels(), HW = (int64_t)d.s1 * d.s2;
  const int64_t nK = (int64_t)t.n * K, nV = (int64_t)t.n * V;
  auto fill = [&](int z) {
    float* dst = ring[DIM == 3 ? ring_slot(z) : 0];
    for (int i = threadIdx.x; i < kPlane; i += kBlock) {
      const int ly = i / kPW, lx = i - ly * kPW;
      const int y = t.ty0 + ly - 1, x = t.tx0 + lx - 1;
      float u = 0.f;
      if (z >= 0 && z < d.s0 && y >= 0 && y < d.s1 && x >= 0 && x < d.s2)
        u = field_u<SOFT>(in, lab, soft, nK, V, (int64_t)z * HW + (int64_t)y * d.s2 + x, nV, K, c0);
      dst[i] = u;
    }
  };
  float acc[1] = {0.f};
  const float inv_mu = 1.f / (float)(mask_used > 0 ? mask_used : 1);
  if (DIM == 3) fill(t.z0 - 1);
  fill(t.z0);
  for (int z = t.z0; z < t.z1; ++z) {
    if (DIM == 3) fill(z + 1);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) + 4 * r;
      const int x = t.tx0 + lx, y = t.ty0 + ly;
      if (x < d.s2 && y < d.s1) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int a0 = 0; a0 < (DIM == 3 ? 3 : 1); ++a0) {
          const float* pl = ring[DIM == 3 ? ring_slot(z - 1 + a0) : 0];
#pragma unroll
          for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
            for (int a2 = 0; a2 < 3; ++a2) {
              const float u = pl[(ly + a1) * kPW + lx + a2];
              const float wa = tap_a<DIM>(a0, a1, a2), wb = tap_b<DIM>(a0, a1, a2);
              if (wa != 0.f) a = fmaf(wa, u, a);
              if (wb != 0.f) b = fmaf(wb, u, b);
            }
        }
        const int64_t o = (int64_t)z * HW + (int64_t)y * d.s2 + x;
        float w = 1.f;
        if (mask) {
          float sm = 0.f;
          for (int j = 0; j < mask_used; ++j) {
            const float mv = mask[((int64_t)t.n * mask_ch + j) * V + o];
            sm = fmaf(mv, mv, sm);
          }
          w = sm * inv_mu;
        }
        acc[0] += w * (ca * (a * a) + cb * (b * b));
        if (R) {
          R[((int64_t)t.n * 2 + 0) * V + o] = 2.f * ca * (w * a);
          R[((int64_t)t.n * 2 + 1) * V + o] = 2.f * cb * (w * b);
        }
      }
    }
    __syncthreads();
  }
  block_sum<1>(acc, smem);
  if (threadIdx.x == 0)
    partial[blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z)] = acc[0];
}

// g_u(p) = gs / denom * sum_t [A(t) R_A(p - t + 1) + B(t) R_B(p - t + 1)];  grad_in_c = g_u, grad_t_c = -g_u for c >= c0, 0 else
template <int DIM>
__global__ void __launch_bounds__(kBlock)
k_contour_bwd(const float* __restrict__ R, const float* __restrict__ grad_scale, float* __restrict__ gin,
              float* __restrict__ gt, int K, int c0, Dims d, int tiles_x, int zc, float denom) {
  __shared__ float ringA[DIM == 3 ? 3 : 1][kPlane];
  __shared__ float ringB[DIM == 3 ? 3 : 1][kPlane];
  const TileGeom t(d, tiles_x, zc);
  const int64_t V = d.voxels(), HW = (int64_t)d.s1 * d.s2;
  const float* RA = R + (int64_t)t.n * 2 * V;
  const float* RB = RA + V;
  const float g = (grad_scale ? grad_scale[0] : 1.f) / denom;
  auto fill = [&](int z) {
    const int sl = DIM == 3 ? ring_slot(z) : 0;
    for (int i = threadIdx.x; i < kPlane; i += kBlock) {
      const int ly = i / kPW, lx = i - ly * kPW;
      const int y = t.ty0 + ly - 1, x = t.tx0 + lx - 1;
      float va = 0.f, vb = 0.f;
      if (z >= 0 && z < d.s0 && y >= 0 && y < d.s1 && x >= 0 && x < d.s2) {
        const int64_t o = (int64_t)z * HW + (int64_t)y * d.s2 + x;
        va = RA[o];
        vb = RB[o];
      }
      ringA[sl][i] = va;
      ringB[sl][i] = vb;
    }
  };
  if (DIM == 3) fill(t.z0 - 1);
  fill(t.z0);
  for (int z = t.z0; z < t.z1; ++z) {
    if (DIM == 3) fill(z + 1);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int lx = threadIdx.x & 63, ly = (threadIdx.x >> 6) + 4 * r;
      const int x = t.tx0 + lx, y = t.ty0 + ly;
      if (x < d.s2 && y < d.s1) {
        float s = 0.f;
#pragma unroll
        for (int a0 = 0; a0 < (DIM == 3 ? 3 : 1); ++a0) {
          const int sl = DIM == 3 ? ring_slot(z + 1 - a0) : 0;
#pragma unroll
          for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
            for (int a2 = 0; a2 < 3; ++a2) {
              const int li = (ly + 2 - a1) * kPW + lx + 2 - a2;
              const float wa = tap_a<DIM>(a0, a1, a2), wb = tap_b<DIM>(a0, a1, a2);
              if (wa != 0.f) s = fmaf(wa, ringA[sl][li], s);
              if (wb != 0.f) s = fmaf(wb, ringB[sl][li], s);
            }
        }
        const float gu = g * s;
        const int64_t o = (int64_t)z * HW + (int64_t)y * d.s2 + x;
        for (int c = 0; c < K; ++c) {
          const int64_t oc = ((int64_t)t.n * K + c) * V + o;
          if (gin) gin[oc] = c >= c0 ? gu : 0.f;
          if (gt) gt[oc] = c >= c0 ? -gu : 0.f;
        }
      }
    }
    __syncthreads();
  }
}

// ---- one-hot ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_one_hot(const int64_t* __restrict__ lab, float* __restrict__ out, int64_t D, int64_t V, int64_t NV) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= NV) return;
  const int64_t n = i / V, v = i - n * V;
  const int64_t y = lab[i];
  const bool bad = y < 0 || y >= D;
  for (int64_t c = 0; c < D; ++c) out[(n * D + c) * V + v] = bad ? qnan() : (c == y ? 1.f : 0.f);
}

// ---- host helpers -------------------------------------------------------------------------------------------------------
struct ContourGrid {
  int tiles_x, zc;
  dim3 grid;
  ContourGrid(int64_t N, int ndim, const Dims& d) {
    tiles_x = (d.s2 + kTX - 1) / kTX;
    const int tiles_y = (d.s1 + kTY - 1) / kTY;
    zc = ndim == 3 ? kZChunk : 1;
    grid = dim3((unsigned)((int64_t)tiles_x * tiles_y), (unsigned)((d.s0 + zc - 1) / zc), (unsigned)N);
  }
  int64_t blocks() const { return (int64_t)grid.x * grid.y * grid.z; }
  bool ok() const { return grid.y <= 65535u; }
};

// VEC = 4 when the rows of pixels split into 4-pixel groups and every tensor takes the vector accesses
inline int ce_vec(int64_t HW, int bf16, const void* x, const void* lab, const void* soft, const void* a, const void* b) {
  const int xs = bf16 ? 8 : 16;
  return (HW % 4 == 0 && aligned(x, xs) && aligned(lab, 16) && aligned(soft, 16) && aligned(a, 16) &&
          aligned(b, bf16 ? 8 : 16)) ? 4 : 1;
}

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int64_t advchain_seg_loss_workspace(int64_t N, int ndim, const int64_t* dims) {
  if (N < 0 || !dims_ok(ndim, dims)) return -1;
  const Dims d = make_dims(ndim, dims);
  const int64_t ce = advchain_blocks(N * d.voxels(), kBlock);           // VEC = 1 grid (the larger one)
  const int64_t cn = ContourGrid(N, ndim, d).blocks();
  return ce > cn ? ce : cn;
}

int advchain_ce2d_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      float* lse, float* workspace, float* value, int64_t N, int64_t K, const int64_t* dims, float denom,
                      void* stream) {
  ADVCHAIN_CHECK_ARG(logits && workspace && value, "ce2d_fwd: null pointer");
  ADVCHAIN_CHECK_ARG((labels != nullptr) != (soft != nullptr), "ce2d_fwd: exactly one of labels / soft target");
  ADVCHAIN_CHECK_ARG(K >= 1 && K < (1 << 24), "ce2d_fwd: K must be >= 1");
  ADVCHAIN_CHECK_ARG(N >= 1 && dims_ok(2, dims), "ce2d_fwd: bad N or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "ce2d_fwd: logits are fp32 (0) or bf16 (1)");
  const int64_t HW = dims[0] * dims[1], P = N * HW;
  const int vec = ce_vec(HW, logits_bf16, logits, labels ? (const void*)labels : nullptr, soft, lse, nullptr);
  const int64_t blocks = advchain_blocks(P, kBlock * vec);
  hipStream_t s = (hipStream_t)stream;
  seg_dispatch(logits_bf16, soft != nullptr, vec == 4, [&](auto st, auto so, auto ve) {
    using ST = typename decltype(st)::type;
    hipLaunchKernelGGL((k_ce_fwd<ST, decltype(so)::value, decltype(ve)::value ? 4 : 1>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                       (const ST*)logits, labels, soft, weight, lse, workspace, (int)K, HW, P);
  });
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seg_finish, dim3(1), dim3(kBlock), 0, s, workspace, blocks, denom, value);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_ce2d_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      const float* lse, const float* grad_scale, void* grad_logits, float* grad_soft, int64_t N, int64_t K,
                      const int64_t* dims, float denom, void* stream) {
  ADVCHAIN_CHECK_ARG(logits && lse, "ce2d_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(grad_logits || grad_soft, "ce2d_bwd: null pointer (no gradient requested)");
  ADVCHAIN_CHECK_ARG((labels != nullptr) != (soft != nullptr), "ce2d_bwd: exactly one of labels / soft target");
  ADVCHAIN_CHECK_ARG(!(labels && grad_soft), "ce2d_bwd: a label target has no gradient");
  ADVCHAIN_CHECK_ARG(K >= 1 && K < (1 << 24), "ce2d_bwd: K must be >= 1");
  ADVCHAIN_CHECK_ARG(N >= 1 && dims_ok(2, dims), "ce2d_bwd: bad N or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "ce2d_bwd: logits are fp32 (0) or bf16 (1)");
  const int64_t HW = dims[0] * dims[1], P = N * HW;
  const int vec = ce_vec(HW, logits_bf16, logits, labels ? (const void*)labels : nullptr, soft, lse, grad_logits) == 4 &&
                  aligned(grad_soft, 16) ? 4 : 1;
  const int64_t blocks = advchain_blocks(P, kBlock * vec);
  hipStream_t s = (hipStream_t)stream;
  seg_dispatch(logits_bf16, soft != nullptr, vec == 4, [&](auto st, auto so, auto ve) {
    using ST = typename decltype(st)::type;
    hipLaunchKernelGGL((k_ce_bwd<ST, decltype(so)::value, decltype(ve)::value ? 4 : 1>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                       (const ST*)logits, labels, soft, weight, lse, grad_scale, (ST*)grad_logits, grad_soft, (int)K, HW, P, denom);
  });
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_contour_fwd(const float* input, const int64_t* labels, const float* soft, const float* mask, float* R,
                         float* workspace, float* value, int64_t N, int64_t K, int ndim, const int64_t* dims, int first_class,
                         int mask_channels, void* stream) {
  ADVCHAIN_CHECK_ARG(input && workspace && value, "contour_fwd: null pointer");
  ADVCHAIN_CHECK_ARG((labels != nullptr) != (soft != nullptr), "contour_fwd: exactly one of labels / soft target");
  ADVCHAIN_CHECK_ARG(K >= 1 && K < (1 << 24), "contour_fwd: K must be >= 1");
  ADVCHAIN_CHECK_ARG(first_class == 0 || first_class == 1, "contour_fwd: first_class is 0 or 1");
  ADVCHAIN_CHECK_ARG(K > first_class, "contour_fwd: no object class left");
  ADVCHAIN_CHECK_ARG(N >= 1 && N < 65536 && dims_ok(ndim, dims), "contour_fwd: bad N or dims");
  const int oc = (int)K - first_class;
  // 2D: the conv output has |S| channels, which a mask of 2..|S|-1 channels does not broadcast against; 3D: one channel
  ADVCHAIN_CHECK_ARG(!mask || (mask_channels >= 1 && (ndim == 3 || mask_channels == 1 || mask_channels >= oc)),
                     "contour_fwd: a 2D mask needs 1 or >= K - first_class channels");
  const Dims d = make_dims(ndim, dims);
  const ContourGrid cg(N, ndim, d);
  ADVCHAIN_CHECK_ARG(cg.ok(), "contour_fwd: bad dims");
  const int mask_used = mask ? (mask_channels < oc ? mask_channels : oc) : 0;
  const float ca = ndim == 2 ? 0.5f : 2.f / 3.f, cb = ndim == 2 ? 0.5f : 1.f / 3.f;
  hipStream_t s = (hipStream_t)stream;
#define ADVCHAIN_CONTOUR_FWD(DIM, SOFT)                                                                                       \
  hipLaunchKernelGGL((k_contour_fwd<DIM, SOFT>), cg.grid, dim3(kBlock), 0, s, input, labels, soft, mask, R, workspace,     \
                     (int)K, first_class, mask_channels, mask_used, d, cg.tiles_x, cg.zc, ca, cb)
  if (ndim == 2) {
    if (soft) ADVCHAIN_CONTOUR_FWD(2, true); else ADVCHAIN_CONTOUR_FWD(2, false);
  } else {
    if (soft) ADVCHAIN_CONTOUR_FWD(3, true); else ADVCHAIN_CONTOUR_FWD(3, false);
  }
#undef ADVCHAIN_CONTOUR_FWD
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_seg_finish, dim3(1), dim3(kBlock), 0, s, workspace, cg.blocks(), (float)(N * d.voxels()), value);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_contour_bwd(const float* R, const float* grad_scale, float* grad_input, float* grad_soft, int64_t N, int64_t K,
                         int ndim, const int64_t* dims, int first_class, void* stream) {
  ADVCHAIN_CHECK_ARG(R, "contour_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(grad_input || grad_soft, "contour_bwd: null pointer (no gradient requested)");
  ADVCHAIN_CHECK_ARG(K >= 1 && K < (1 << 24), "contour_bwd: K must be >= 1");
  ADVCHAIN_CHECK_ARG(first_class == 0 || first_class == 1, "contour_bwd: first_class is 0 or 1");
  ADVCHAIN_CHECK_ARG(N >= 1 && N < 65536 && dims_ok(ndim, dims), "contour_bwd: bad N or dims");
  const Dims d = make_dims(ndim, dims);
  const ContourGrid cg(N, ndim, d);
  ADVCHAIN_CHECK_ARG(cg.ok(), "contour_bwd: bad dims");
  const float denom = (float)(N * d.voxels());
  hipStream_t s = (hipStream_t)stream;
  if (ndim == 2)
    hipLaunchKernelGGL((k_contour_bwd<2>), cg.grid, dim3(kBlock), 0, s, R, grad_scale, grad_input, grad_soft, (int)K,
                       first_class, d, cg.tiles_x, cg.zc, denom);
  else
    hipLaunchKernelGGL((k_contour_bwd<3>), cg.grid, dim3(kBlock), 0, s, R, grad_scale, grad_input, grad_soft, (int)K,
                       first_class, d, cg.tiles_x, cg.zc, denom);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_one_hot(const int64_t* labels, float* out, int64_t N, int64_t depth, int64_t V, void* stream) {
  ADVCHAIN_CHECK_ARG(labels && out, "one_hot: null pointer");
  ADVCHAIN_CHECK_ARG(depth >= 1, "one_hot: depth must be >= 1");
  ADVCHAIN_CHECK_ARG(N >= 0 && V >= 1, "one_hot: bad N or V");
  const int64_t NV = N * V;
  if (NV == 0) return ADVCHAIN_OK;
  hipLaunchKernelGGL(k_one_hot, dim3((unsigned)advchain_blocks(NV, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, labels, out,
                     depth, V, NV);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
