// Soft Dice and the fused Dice + cross entropy of a segmentation step, 2D and 3D, for gfx950:
//
//   advchain_dice_fwd / advchain_dice_bwd   <- common.loss.dice_loss, dice_ce_loss
//
// With p = softmax(logits) over the K planes, t the one-hot labels or a soft target, and the sums over the counted voxels of
// batch entry n (label -100: not counted; batch_dice: over n as well, N -> 1)
//   I_nk = sum p_k t_k,  P_nk = sum p_k,  T_nk = sum t_k,  D_nk = P_nk + T_nk + smooth,  dice_nk = (2 I_nk + smooth) / D_nk
//   loss = dice_w (1 - 1/N sum_nk omega_k dice_nk) + ce_w CE,      omega_k = w_k / sum of the counted w_j
// CE is the cross entropy of seg_loss.hip with size_average (weights w / sum(w) * K, -100 contributes 0, divided by N V).
//
// Forward, three launches:
//   k_dice_fwd     grid (V / 1024, N): a lane owns 4 consecutive voxels (16-byte fp32 / 8-byte bf16 loads, or scalar loads of the
//                  same 4 voxels: the order of every sum does not depend on the alignment).  Sweep one is the online max /
//                  sum of exp over the K planes -> lse per voxel (saved for the backward) and the CE term; sweep two forms
//                  p_k = exp(x_k - lse) (a second read of the planes) and sums (I, P, T) per class: in the wave (DPP), then across
//                  the four waves through LDS in wave order, one barrier per chunk of kChunk classes.  One triple per
//                  (workgroup, class) and one CE partial per workgroup go to the workspace.
//   k_dice_reduce  grid (K, rows): adds the triples of one (n, k) in a fixed order.
//   k_dice_finish  one workgroup: dice, the value, and the table (A_nk, B_nk) of dL/dp_k(v) = A_nk t_k(v) + B_nk.
// Backward, one launch: g_k = A_nk t_k + B_nk, gx_k = p_k (g_k - sum_j g_j p_j) (zero at ignored voxels) plus the CE gradient,
// rounded once to the logits' dtype; a soft target gets A_nk p_k + B_nk (+ CE's w_k (lse - x_k)).
//
// No float atomics and no host read-back: every output is written by a kernel, the value is bitwise reproducible.  A label is
// only ever COMPARED with class indices.  The file is compiled without contraction (build.py), so that the fp32 / bf16 and the
// vector / scalar instantiations round alike.
#include <math.h>

#include "common.h"
#include "seg_common.h"

namespace advchain {
namespace {

constexpr int kChunk = 16;                   // classes between two barriers of sweep two

enum { DICE_IGNORE_BACKGROUND = 1, DICE_BATCH = 2 };

// one-hot value of class c at a voxel labelled y: NaN for a label outside [0, K) (the caller leaves -100 out)
__device__ __forceinline__ float one_hot_at(int64_t y, int c, bool bad) { return bad ? qnan() : (y == c ? 1.f : 0.f); }

template <typename ST, bool SOFT, bool VEC>
__global__ void __launch_bounds__(kBlock)
k_dice_fwd(const ST* __restrict__ x, const int64_t* __restrict__ lab, const float* __restrict__ soft,
           const float* __restrict__ weight, float* __restrict__ lse_out, float* __restrict__ part,
           float* __restrict__ ce_part, int K, int64_t V, int want_ce) {
  __shared__ float red[2][4][kChunk * 3];
  __shared__ float smem[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = blockIdx.y;
  const int64_t slot = n * gridDim.x + blockIdx.x;                  // this workgroup's row of partials
  const int64_t v0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kVox;
  const int cnt = lane_count(V, v0);
  const ST* xn = x + n * K * V + v0;
  const float* tn = SOFT ? soft + n * K * V + v0 : nullptr;

  int64_t y[kVox];
  bool live[kVox], bad[kVox];                                       // counted in the Dice sums; label outside [0, K)
  if constexpr (!SOFT) ld4_labels<VEC>(lab + n * V + v0, cnt, y);
#pragma unroll
  for (int q = 0; q < kVox; ++q) {
    if constexpr (SOFT) { y[q] = 0; live[q] = q < cnt; bad[q] = false; }
    else { live[q] = y[q] != -100; bad[q] = live[q] && (y[q] < 0 || y[q] >= K); }
  }

  // sweep one: online max / sum of exp, and the pick-up of the cross entropy
  const float wsum = (want_ce && weight) ? weight_sum(weight, K) : 1.f, Kf = (float)K;
  float m[kVox], s[kVox], a[kVox], b[kVox];
#pragma unroll
  for (int q = 0; q < kVox; ++q) { m[q] = -INFINITY; s[q] = 0.f; a[q] = SOFT ? 0.f : qnan(); b[q] = SOFT ? 0.f : qnan(); }
  for (int c = 0; c < K; ++c) {
    float xc[kVox], tc[kVox];
    ld4<ST, VEC>(xn + (int64_t)c * V, cnt, xc);
    if constexpr (SOFT) {
      if (want_ce) ld4<float, VEC>(tn + (int64_t)c * V, cnt, tc);
    }
    const float wc = want_ce ? class_weight(weight, c, wsum, Kf) : 1.f;
#pragma unroll
    for (int q = 0; q < kVox; ++q) {
      const float mn = fmaxf(m[q], xc[q]), ms = sub_max(mn);         // (a class masked with -inf in front: common.h)
      s[q] = s[q] * __expf(m[q] - ms) + __expf(xc[q] - ms);
      m[q] = mn;
      if constexpr (SOFT) {
        if (want_ce) {
          const float wt = wc * tc[q];
          a[q] = fmaf(wt, xc[q], a[q]);       // sum w t x
          b[q] += wt;                         // sum w t
        }
      } else if (y[q] == c) {
        a[q] = xc[q];                         // the label's logit
        b[q] = wc;                            // its class weight
      }
    }
  }
  float l[kVox], ce[1] = {0.f};
#pragma unroll
  for (int q = 0; q < kVox; ++q) {
    l[q] = m[q] + logf(s[q]);
    if constexpr (SOFT) ce[0] += q < cnt ? b[q] * l[q] - a[q] : 0.f;
    else ce[0] += live[q] ? b[q] * (l[q] - a[q]) : 0.f;             // outside [0, K) and not -100: a, b stay NaN
  }
  if (lse_out) st4<float, VEC>(lse_out + n * V + v0, cnt, l);
  if (want_ce) {
    block_sum<1>(ce, smem);
    if (threadIdx.x == 0) ce_part[slot] = ce[0];
  }

  // sweep two: (I, P, T) per class
  float* out = part + slot * K * 3;
  int buf = 0;
  for (int c0 = 0; c0 < K; c0 += kChunk, buf ^= 1) {
    const int nc = min(kChunk, K - c0);
    for (int cc = 0; cc < nc; ++cc) {
      const int c = c0 + cc;
      float xc[kVox], tc[kVox];
      ld4<ST, VEC>(xn + (int64_t)c * V, cnt, xc);
      if constexpr (SOFT) ld4<float, VEC>(tn + (int64_t)c * V, cnt, tc);
      float sI = 0.f, sP = 0.f, sT = 0.f;
#pragma unroll
      for (int q = 0; q < kVox; ++q) {
        const float p = __expf(xc[q] - l[q]);
        const float t = SOFT ? tc[q] : one_hot_at(y[q], c, bad[q]);
        sI += live[q] ? p * t : 0.f;
        sP += live[q] ? p : 0.f;
        sT += live[q] ? t : 0.f;
      }
      sI = wave_sum_lane63(sI);
      sP = wave_sum_lane63(sP);
      sT = wave_sum_lane63(sT);
      if (lane == 63) {
        red[buf][wave][cc * 3 + 0] = sI;
        red[buf][wave][cc * 3 + 1] = sP;
        red[buf][wave][cc * 3 + 2] = sT;
      }
    }
    __syncthreads();                                                // (the next chunk writes the other buffer)
    if ((int)threadIdx.x < nc * 3) {
      const int i = threadIdx.x;
      out[c0 * 3 + i] = ((red[buf][0][i] + red[buf][1][i]) + red[buf][2][i]) + red[buf][3][i];
    }
  }
}

// sums[(r, k)] = the M triples of row r and class k, added in a fixed order
__global__ void __launch_bounds__(kBlock)
k_dice_reduce(const float* __restrict__ part, float* __restrict__ sums, int K, int64_t M) {
  __shared__ float smem[12];
  const int64_t k = blockIdx.x, r = blockIdx.y;
  float s[3] = {0.f, 0.f, 0.f};
  for (int64_t i = threadIdx.x; i < M; i += kBlock) {
    const float* p = part + ((r * M + i) * K + k) * 3;
    s[0] += p[0];
    s[1] += p[1];
    s[2] += p[2];
  }
  block_sum<3>(s, smem);
  if (threadIdx.x == 0) {
    float* o = sums + (r * K + k) * 3;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
  }
}

// value = dice_w (1 - 1/R sum_rk omega_k dice_rk) + ce_w (sum of the CE partials) / (N V);  coef[(n, k)] = (A_nk, B_nk)
__global__ void __launch_bounds__(kBlock)
k_dice_finish(const float* __restrict__ sums, const float* __restrict__ ce_part, const float* __restrict__ weight,
              float* __restrict__ coef, float* __restrict__ value, int64_t N, int K, int64_t R, int64_t n_ce, int first_class,
              float smooth, float dice_w, float ce_w, float ce_denom) {
  __shared__ float smem[8];
  float wsum = 0.f;                                                 // of the counted classes, in class order
  for (int c = first_class; c < K; ++c) wsum += weight ? weight[c] : 1.f;
  const float cN = 1.f / (float)R;
  float acc[2] = {0.f, 0.f};
  for (int64_t i = threadIdx.x; i < R * K; i += kBlock) {
    const int64_t r = i / K;
    const int k = (int)(i - r * K);
    const float I = sums[i * 3 + 0], P = sums[i * 3 + 1], T = sums[i * 3 + 2];
    const float omega = k < first_class ? 0.f : (weight ? weight[k] : 1.f) / wsum;
    const float D = (P + T) + smooth, num = 2.f * I + smooth;
    acc[0] += omega * (num / D);
    if (coef) {
      const float A = -2.f * cN * omega / D, B = cN * omega * num / (D * D);
      for (int64_t n = (R == 1 ? 0 : r); n < (R == 1 ? N : r + 1); ++n) {       // batch dice: every entry reads the same row
        coef[(n * K + k) * 2 + 0] = A;
        coef[(n * K + k) * 2 + 1] = B;
      }
    }
  }
  if (ce_part)
    for (int64_t i = threadIdx.x; i < n_ce; i += kBlock) acc[1] += ce_part[i];
  block_sum<2>(acc, smem);
  if (threadIdx.x == 0) {
    float v = dice_w * (1.f - acc[0] * cN);
    if (ce_part) v += ce_w * (acc[1] / ce_denom);
    value[0] = v;
  }
}

template <typename ST, bool SOFT, bool VEC>
__global__ void __launch_bounds__(kBlock)
k_dice_bwd(const ST* __restrict__ x, const int64_t* __restrict__ lab, const float* __restrict__ soft,
           const float* __restrict__ weight, const float* __restrict__ lse, const float* __restrict__ coef,
           const float* __restrict__ grad_scale, ST* __restrict__ gx, float* __restrict__ gt, int K, int64_t V, float dice_w,
           float ce_scale) {
  const int64_t n = blockIdx.y;
  const int64_t v0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kVox;
  const int cnt = lane_count(V, v0);
  if (cnt == 0) return;
  const int64_t base = n * K * V + v0;
  const float* cf = coef + n * K * 2;
  const bool want_ce = ce_scale != 0.f;
  const float gs = grad_scale ? grad_scale[0] : 1.f;
  const float wsum = (want_ce && weight) ? weight_sum(weight, K) : 1.f, Kf = (float)K;

  float l[kVox];
  int64_t y[kVox];
  bool live[kVox], bad[kVox];
  ld4<float, VEC>(lse + n * V + v0, cnt, l);
  if constexpr (!SOFT) ld4_labels<VEC>(lab + n * V + v0, cnt, y);
#pragma unroll
  for (int q = 0; q < kVox; ++q) {
    if constexpr (SOFT) { y[q] = 0; live[q] = q < cnt; bad[q] = false; }
    else { live[q] = y[q] != -100; bad[q] = live[q] && (y[q] < 0 || y[q] >= K); }
  }

  // s = sum_j g_j p_j and the CE's W = sum_j w_j t_j
  float s[kVox], W[kVox];
#pragma unroll
  for (int q = 0; q < kVox; ++q) { s[q] = 0.f; W[q] = SOFT ? 0.f : (live[q] ? qnan() : 0.f); }
  for (int c = 0; c < K; ++c) {
    float xc[kVox], tc[kVox];
    ld4<ST, VEC>(x + base + (int64_t)c * V, cnt, xc);
    if constexpr (SOFT) ld4<float, VEC>(soft + base + (int64_t)c * V, cnt, tc);
    const float A = cf[2 * c], B = cf[2 * c + 1];
    const float wc = want_ce ? class_weight(weight, c, wsum, Kf) : 1.f;
#pragma unroll
    for (int q = 0; q < kVox; ++q) {
      const float p = __expf(xc[q] - l[q]);
      const float t = SOFT ? tc[q] : one_hot_at(y[q], c, bad[q]);
      s[q] = fmaf(fmaf(A, t, B), p, s[q]);
      if constexpr (SOFT) W[q] += wc * tc[q];
      else if (y[q] == c) W[q] = wc;
    }
  }
  for (int c = 0; c < K; ++c) {
    float xc[kVox], tc[kVox], gc[kVox], gtc[kVox];
    ld4<ST, VEC>(x + base + (int64_t)c * V, cnt, xc);
    if constexpr (SOFT) ld4<float, VEC>(soft + base + (int64_t)c * V, cnt, tc);
    const float A = cf[2 * c], B = cf[2 * c + 1];
    const float wc = want_ce ? class_weight(weight, c, wsum, Kf) : 1.f;
#pragma unroll
    for (int q = 0; q < kVox; ++q) {
      const float p = __expf(xc[q] - l[q]);
      const float t = SOFT ? tc[q] : one_hot_at(y[q], c, bad[q]);
      float g = live[q] ? dice_w * (p * (fmaf(A, t, B) - s[q])) : 0.f;
      float h = dice_w * fmaf(A, p, B);
      if (want_ce) {
        const float wt = SOFT ? wc * tc[q] : (y[q] == c ? wc : 0.f);
        g += ce_scale * (W[q] * p - wt);
        h += ce_scale * (wc * (l[q] - xc[q]));
      }
      gc[q] = gs * g;
      gtc[q] = gs * h;
    }
    if (gx) st4<ST, VEC>(gx + base + (int64_t)c * V, cnt, gc);
    if constexpr (SOFT)
      if (gt) st4<float, VEC>(gt + base + (int64_t)c * V, cnt, gtc);
  }
}

// ---- host helpers -------------------------------------------------------------------------------------------------------
struct DiceLayout {          // the workspace: triples per (workgroup, class) | CE partial per workgroup | sums per (row, class)
  int64_t nb, part, ce, sums;
  DiceLayout(int64_t N, int64_t K, int64_t V) {
    nb = seg_blocks(V);
    part = N * nb * K * 3;
    ce = (N * nb + 3) / 4 * 4;             // (keeps `sums` 16-byte aligned)
    sums = N * K * 3;
  }
  int64_t total() const { return part + ce + sums; }
};

inline bool finite_nonneg(float v) { return v >= 0.f && v <= 3.40282347e38f; }   // false for NaN

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int64_t advchain_dice_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims) {
  const int64_t V = seg_voxels(ndim, dims);
  if (V < 0 || !seg_shape_ok(N, K, V)) return -1;
  return DiceLayout(N, K, V).total();
}

int advchain_dice_fwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      float* lse, float* coef, float* workspace, float* value, int64_t N, int64_t K, int ndim,
                      const int64_t* dims, int flags, float smooth, float dice_w, float ce_w, void* stream) {
  ADVCHAIN_CHECK_ARG(logits && workspace && value, "dice_fwd: null pointer");
  ADVCHAIN_CHECK_ARG((labels != nullptr) != (soft != nullptr), "dice_fwd: exactly one of labels / soft target");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "dice_fwd: K must be in 1..65535");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(V > 0 && seg_shape_ok(N, K, V), "dice_fwd: bad N, ndim or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "dice_fwd: logits are fp32 (0) or bf16 (1)");
  ADVCHAIN_CHECK_ARG((flags & ~3) == 0, "dice_fwd: unknown flags");
  ADVCHAIN_CHECK_ARG(finite_nonneg(smooth), "dice_fwd: smooth must be finite and >= 0");
  const int first_class = (flags & DICE_IGNORE_BACKGROUND) ? 1 : 0;
  ADVCHAIN_CHECK_ARG(K > first_class, "dice_fwd: no class left with ignore_background");
  const DiceLayout lay(N, K, V);
  float* part = workspace;
  float* ce_part = workspace + lay.part;
  float* sums = ce_part + lay.ce;
  const int want_ce = ce_w != 0.f;
  const bool vec = V % 4 == 0 && aligned(logits, logits_bf16 ? 8 : 16) && aligned(labels, 16) && aligned(soft, 16) &&
                   aligned(lse, 16);
  const dim3 grid((unsigned)lay.nb, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  seg_dispatch(logits_bf16, soft != nullptr, vec, [&](auto st, auto so, auto ve) {
    using ST = typename decltype(st)::type;
    hipLaunchKernelGGL((k_dice_fwd<ST, decltype(so)::value, decltype(ve)::value>), grid, dim3(kBlock), 0, s, (const ST*)logits,
                       labels, soft, weight, lse, part, ce_part, (int)K, V, want_ce);
  });
  ADVCHAIN_LAUNCH_CHECK();
  const int64_t R = (flags & DICE_BATCH) ? 1 : N, M = (flags & DICE_BATCH) ? N * lay.nb : lay.nb;
  hipLaunchKernelGGL(k_dice_reduce, dim3((unsigned)K, (unsigned)R), dim3(kBlock), 0, s, part, sums, (int)K, M);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_dice_finish, dim3(1), dim3(kBlock), 0, s, sums, want_ce ? ce_part : nullptr, weight, coef, value, N,
                     (int)K, R, N * lay.nb, first_class, smooth, dice_w, ce_w, (float)(N * V));
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_dice_bwd(const void* logits, int logits_bf16, const int64_t* labels, const float* soft, const float* weight,
                      const float* lse, const float* coef, const float* grad_scale, void* grad_logits, float* grad_soft,
                      int64_t N, int64_t K, int ndim, const int64_t* dims, float dice_w, float ce_w, void* stream) {
  ADVCHAIN_CHECK_ARG(logits && lse && coef, "dice_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(grad_logits || grad_soft, "dice_bwd: null pointer (no gradient requested)");
  ADVCHAIN_CHECK_ARG((labels != nullptr) != (soft != nullptr), "dice_bwd: exactly one of labels / soft target");
  ADVCHAIN_CHECK_ARG(!(labels && grad_soft), "dice_bwd: a label target has no gradient");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "dice_bwd: K must be in 1..65535");
  const int64_t V = seg_voxels(ndim, dims);
  ADVCHAIN_CHECK_ARG(V > 0 && seg_shape_ok(N, K, V), "dice_bwd: bad N, ndim or dims");
  ADVCHAIN_CHECK_ARG(logits_bf16 == 0 || logits_bf16 == 1, "dice_bwd: logits are fp32 (0) or bf16 (1)");
  const bool vec = V % 4 == 0 && aligned(logits, logits_bf16 ? 8 : 16) && aligned(labels, 16) && aligned(soft, 16) &&
                   aligned(lse, 16) && aligned(grad_logits, logits_bf16 ? 8 : 16) && aligned(grad_soft, 16);
  const dim3 grid((unsigned)seg_blocks(V), (unsigned)N);
  const float ce_scale = ce_w / (float)(N * V);
  hipStream_t s = (hipStream_t)stream;
  seg_dispatch(logits_bf16, soft != nullptr, vec, [&](auto st, auto so, auto ve) {
    using ST = typename decltype(st)::type;
    hipLaunchKernelGGL((k_dice_bwd<ST, decltype(so)::value, decltype(ve)::value>), grid, dim3(kBlock), 0, s, (const ST*)logits,
                       labels, soft, weight, lse, coef, grad_scale, (ST*)grad_logits, grad_soft, (int)K, V, dice_w, ce_scale);
  });
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
