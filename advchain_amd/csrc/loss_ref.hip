// Gradient of the segmentation-consistency loss ('mse' + 'contour' + 'kl') with respect to the REFERENCE, gfx950.
//
//   advchain_consistency_ref_bwd <- what autograd gives `reference` in calc_segmentation_consistency + contour_loss +
//                                   kl_divergence, advchain/common/loss.py:8-87,102-220,223-249
//
// Notation of loss.hip: P = softmax(pred), T = softmax(ref) (or ref itself when ref_is_prob), m the mask, R_A,k = 2 m^2 (A*D_k),
// R_B,k = 2 m^2 (B*D_k) the edge responses every forward family saves in one layout, gs the incoming gradient.  The
// prediction-side backward forms, in probability space,
//     g_k = gs (c_mse 2 m_k^2 (P_k - T_k) + [k >= 1] (c_a A^T R_A,k + c_b B^T R_B,k)).
// 'mse' and 'contour' depend on P - T only: their gradient w.r.t. T is -g_k.  'kl' = sum m_k T_k (log T_k - log P_k) adds
// gs c_kl m_k (log T_k + 1 - log P_k).  With h_k = -g_k + gs c_kl m_k (log T_k + 1 - log P_k):
//     logits:       grad_ref_k = T_k (h_k - sum_j T_j h_j)           (softmax Jacobian of the reference)
//     ref_is_prob:  grad_ref_k = -g_k                                (the reference's where() cuts the graph of 'kl')
// log T_k - log P_k comes from the logits and the softmax statistics, (x_r - max_r + log inv_r) - (x_p - max_p + log inv_p),
// never from the log of a probability.  With ref_is_prob the reference's softmax is never evaluated.
//
//   k_loss_ref_grad<DIM, 0>        run-time K (< 65536).  The tile scheme of k_lp_bwd (loss_lp.hip): a workgroup owns a
//                                  spatial tile, the R_k tile + one-voxel halo goes through two LDS buffers (one barrier per
//                                  class), flipped stencils read it there (zero-weight taps skipped).  Softmax statistics
//                                  of the outputs: from `stats` (saved by a run-time-K forward) or, when nothing saved them
//                                  (K <= 16), from a prologue sweep over the classes (running max / sum, one exp per
//                                  element).  First sweep: h_k goes into grad_ref, sum_j T_j h_j stays in registers.  Second
//                                  sweep: the Jacobian in place -- a thread re-reads only what it stored itself.
//   k_loss_ref_grad<DIM, 2|3|4>    the class counts of the solver's configurations: a thread keeps the logits of its 2 (2D)
//                                  or 4 (3D) outputs and their h_k in registers; every operand is read once, there is no
//                                  prologue sweep and grad_ref is written once.
//
// No atomics on grad_ref and no shared accumulator: bit-reproducible.  Streaming + 3^d stencil: memory-bound, no MFMA.
#include <atomic>

#include "loss_common.h"

namespace advchain {

template <int DIM, int KR>
__global__ void __launch_bounds__(kBlock)
k_loss_ref_grad(const float* __restrict__ pred, const float* __restrict__ ref, const float* __restrict__ stats,
                const float* __restrict__ R, const float* __restrict__ mask, const float* __restrict__ gscale, float* gref,
                float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int Krt, Dims d, int mask_ch) {
  using T = WTile<DIM>;
  __shared__ float lds[2][2][T::NH];
  const int K = KR > 0 ? KR : Krt;
  const T tile(d);
  const int n = blockIdx.y;
  const int V = (int)d.voxels();
  const float gs = gscale ? gscale[0] : 1.f;
  const bool edges = R != nullptr;
  const bool kl = c_kl != 0.f && !ref_is_prob;
  const float ckl = gs * c_kl;
  int hv[T::SLOTS];
#pragma unroll
  for (int j = 0; j < T::SLOTS; ++j) hv[j] = tile.halo_voxel(threadIdx.x + j * kBlock, d);
  int ov[T::OUTS], oc[T::OUTS];
  float om[T::OUTS], dot[T::OUTS];
#pragma unroll
  for (int j = 0; j < T::OUTS; ++j) {
    ov[j] = tile.out_voxel(threadIdx.x + j * kBlock, d, oc[j]);
    om[j] = (mask && mask_ch == 1) ? mask[(int64_t)n * V + max(ov[j], 0)] : 1.f;
    dot[j] = 0.f;
  }
  const int64_t batch = (int64_t)n * K * V;

  if constexpr (KR > 0) {
    // ---- K = KR in registers: zp = x_p - max_p, zr = x_r - max_r (ref_is_prob: the probability itself), then h ----
    float zp[T::OUTS][KR], zr[T::OUTS][KR], h[T::OUTS][KR];
    float ip[T::OUTS], ir[T::OUTS], lgd[T::OUTS];
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) {
      const int c = max(ov[j], 0);
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        zp[j][k] = pred[batch + (int64_t)k * V + c];
        zr[j][k] = ref[batch + (int64_t)k * V + c];
      }
    }
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) {
      float mp = zp[j][0], mr = zr[j][0];
#pragma unroll
      for (int k = 1; k < KR; ++k) { mp = fmaxf(mp, zp[j][k]); mr = fmaxf(mr, zr[j][k]); }
      float sp = 0.f, sr = 0.f;
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        zp[j][k] -= mp;
        sp += ADVCHAIN_SM_EXP(zp[j][k]);
        if (!ref_is_prob) {
          zr[j][k] -= mr;
          sr += ADVCHAIN_SM_EXP(zr[j][k]);
        }
      }
      ip[j] = 1.f / sp;
      ir[j] = ref_is_prob ? 1.f : 1.f / sr;
      lgd[j] = kl ? logf(sp) - logf(sr) : 0.f;     // log inv_r - log inv_p
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      float (*buf)[T::NH] = lds[k & 1];
      if (edges && k >= 1) {
        const float* Ra = R + ((int64_t)n * 2 * (KR - 1) + 2 * (k - 1)) * V;
        stage_R<DIM>(buf, Ra, Ra + V, hv);
        __syncthreads();     // (the other buffer is written next: one barrier per class)
      }
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        const int c = max(ov[j], 0);
        const float m = (mask && mask_ch > 1) ? mask[((int64_t)n * mask_ch + k) * V + c] : om[j];
        const float p = mul_nc(ADVCHAIN_SM_EXP(zp[j][k]), ip[j]);
        const float t = ref_is_prob ? zr[j][k] : mul_nc(ADVCHAIN_SM_EXP(zr[j][k]), ir[j]);
        float g = c_mse * 2.f * m * m * (p - t);
        if (edges && k >= 1) {
          float ta, tb;                 // A^T R_A, B^T R_B
          adjoint_stencil<DIM>(buf[0], buf[1], oc[j], ta, tb);
          g += c_a * ta + c_b * tb;
        }
        float hk = -(g * gs);
        if (kl) hk += ckl * m * ((zr[j][k] - zp[j][k]) + lgd[j] + 1.f);
        h[j][k] = hk;
        dot[j] += t * hk;
        zr[j][k] = t;                   // (kept for the Jacobian)
      }
    }
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) {
      if (ov[j] < 0) continue;
#pragma unroll
      for (int k = 0; k < KR; ++k)
        gref[batch + (int64_t)k * V + ov[j]] = ref_is_prob ? h[j][k] : zr[j][k] * (h[j][k] - dot[j]);
    }
  } else {
    // ---- run-time K: statistics from `stats` or from a prologue sweep, then two sweeps over the classes ----
    float omp[T::OUTS], oip[T::OUTS], omr[T::OUTS], oir[T::OUTS], lgd[T::OUTS];
    if (stats) {
      const float* sn = stats + (int64_t)n * 4 * V;
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        const int c = max(ov[j], 0);
        omp[j] = sn[c];
        oip[j] = sn[(int64_t)V + c];
        omr[j] = ref_is_prob ? 0.f : sn[2 * (int64_t)V + c];      // (the ref planes are unspecified when ref_is_prob)
        oir[j] = ref_is_prob ? 1.f : sn[3 * (int64_t)V + c];
      }
    } else {
      float sp[T::OUTS], sr[T::OUTS];
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        const int c = max(ov[j], 0);
        omp[j] = pred[batch + c];
        omr[j] = ref_is_prob ? 0.f : ref[batch + c];
        sp[j] = 1.f;
        sr[j] = 1.f;
      }
      for (int k = 1; k < K; ++k) {
        const int64_t plane = batch + (int64_t)k * V;
#pragma unroll
        for (int j = 0; j < T::OUTS; ++j) {
          const int c = max(ov[j], 0);
          online_step(pred[plane + c], omp[j], sp[j]);
          if (!ref_is_prob) online_step(ref[plane + c], omr[j], sr[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        oip[j] = 1.f / sp[j];
        oir[j] = 1.f / sr[j];
      }
    }
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) lgd[j] = kl ? logf(oir[j]) - logf(oip[j]) : 0.f;   // log inv_r - log inv_p
    for (int k = 0; k < K; ++k) {
      const int64_t plane = batch + (int64_t)k * V;
      float (*buf)[T::NH] = lds[k & 1];
      if (edges && k >= 1) {
        const float* Ra = R + ((int64_t)n * 2 * (K - 1) + 2 * (k - 1)) * V;
        stage_R<DIM>(buf, Ra, Ra + V, hv);
        __syncthreads();     // (the other buffer is written next: one barrier per class)
      }
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        const int c = max(ov[j], 0);
        const float xp = pred[plane + c], xr = ref[plane + c];
        const float m = (mask && mask_ch > 1) ? mask[((int64_t)n * mask_ch + k) * V + c] : om[j];
        const float zp = xp - omp[j], zr = xr - omr[j];
        const float p = mul_nc(ADVCHAIN_SM_EXP(zp), oip[j]);
        const float t = ref_is_prob ? xr : mul_nc(ADVCHAIN_SM_EXP(zr), oir[j]);
        float g = c_mse * 2.f * m * m * (p - t);
        if (edges && k >= 1) {
          float ta, tb;                 // A^T R_A, B^T R_B
          adjoint_stencil<DIM>(buf[0], buf[1], oc[j], ta, tb);
          g += c_a * ta + c_b * tb;
        }
        float hk = -(g * gs);
        if (kl) hk += ckl * m * ((zr - zp) + lgd[j] + 1.f);
        if (ov[j] >= 0) gref[plane + c] = hk;     // ref_is_prob: already the gradient
        dot[j] += t * hk;
      }
    }
    if (ref_is_prob) return;
    // second sweep: the softmax Jacobian of the reference, in place (every thread re-reads only its own stores)
    for (int k = 0; k < K; ++k) {
      const int64_t plane = batch + (int64_t)k * V;
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        if (ov[j] < 0) continue;
        const int c = ov[j];
        const float t = mul_nc(ADVCHAIN_SM_EXP(ref[plane + c] - omr[j]), oir[j]);
        gref[plane + c] = t * (gref[plane + c] - dot[j]);
      }
    }
  }
}

}  // namespace advchain

using namespace advchain;

// Class counts up to this one (at most 4) take the register form; 0: the run-time form for every K (tests, A/B).
static std::atomic<int> g_ref_grad_reg_max_k{4};

template <int DIM>
static void launch_ref_grad(int kr, dim3 grid, hipStream_t st, const float* pred, const float* ref, const float* stats,
                            const float* R, const float* mask, const float* gscale, float* gref, float c_mse, float c_a,
                            float c_b, float c_kl, int ref_is_prob, int K, Dims d, int mask_ch) {
#define ADVCHAIN_REF_GRAD_LAUNCH(KR)                                                                                      \
  hipLaunchKernelGGL((k_loss_ref_grad<DIM, KR>), grid, dim3(kBlock), 0, st, pred, ref, stats, R, mask, gscale, gref, c_mse, \
                     c_a, c_b, c_kl, ref_is_prob, K, d, mask_ch)
  switch (kr) {
    case 2: ADVCHAIN_REF_GRAD_LAUNCH(2); break;
    case 3: ADVCHAIN_REF_GRAD_LAUNCH(3); break;
    case 4: ADVCHAIN_REF_GRAD_LAUNCH(4); break;
    default: ADVCHAIN_REF_GRAD_LAUNCH(0); break;
  }
#undef ADVCHAIN_REF_GRAD_LAUNCH
}

extern "C" {

void advchain_set_ref_grad_reg_max_k(int k) {
  g_ref_grad_reg_max_k.store(k < 0 ? 0 : (k > 4 ? 4 : k), std::memory_order_relaxed);
}
int advchain_get_ref_grad_reg_max_k(void) { return g_ref_grad_reg_max_k.load(std::memory_order_relaxed); }

int advchain_consistency_ref_bwd(const float* pred, const float* ref, const float* stats, const float* R, const float* mask,
                                 const float* grad_scale, float* grad_ref, float c_mse, float c_a, float c_b, float c_kl,
                                 int ref_is_prob, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                                 void* stream) {
  ADVCHAIN_CHECK_ARG(pred && ref && grad_ref && dims, "consistency_ref_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(dims_ok(ndim, dims), "consistency_ref_bwd: bad dims");
  ADVCHAIN_CHECK_ARG(N >= 0 && N < 65536 && K >= 1 && K < 65536, "consistency_ref_bwd: bad N/K (N < 65536, 1 <= K < 65536)");
  ADVCHAIN_CHECK_ARG(!mask || mask_channels == 1 || mask_channels == K, "consistency_ref_bwd: mask must have 1 or K channels");
  const Dims d = make_dims(ndim, dims);
  ADVCHAIN_CHECK_ARG(d.voxels() < (1ll << 31), "consistency_ref_bwd: volume too large");
  if (N == 0) return ADVCHAIN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (K == 1) R = nullptr;        // (no object class: nothing was saved)
  const int kr = (K >= 2 && K <= advchain_get_ref_grad_reg_max_k()) ? (int)K : 0;
  if (ndim == 3)
    launch_ref_grad<3>(kr, dim3((unsigned)WTile<3>::count(d), (unsigned)N), st, pred, ref, stats, R, mask, grad_scale, grad_ref,
                       c_mse, c_a, c_b, c_kl, ref_is_prob, (int)K, d, mask_channels);
  else
    launch_ref_grad<2>(kr, dim3((unsigned)WTile<2>::count(d), (unsigned)N), st, pred, ref, stats, R, mask, grad_scale, grad_ref,
                       c_mse, c_a, c_b, c_kl, ref_is_prob, (int)K, d, mask_channels);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
