// Segmentation-consistency loss ('mse' + 'contour' + 'kl') for a RUN-TIME class count, gfx950.
//
//   advchain_consistency_wide_fwd/bwd <- calc_segmentation_consistency + contour_loss + kl_divergence,
//                                        advchain/common/loss.py:8-87,102-220,223-249 (Q13, Q14)
//
// Same mathematics as loss.hip (see its header); what differs is that nothing here is sized by K.  loss.hip keeps a softmax
// row per voxel in registers (K <= 16) or materialises P and D; here the class axis is MARCHED:
//
//   k_wide_stats   one streaming pass with a running max / sum of exp over the K planes leaves the softmax statistics of
//                  both operands, 16 bytes per voxel: stats (N, 4, V) = max_pred, 1 / sum_pred, max_ref, 1 / sum_ref.  With
//                  them every class plane is independent: P_k(v) = exp(pred_k(v) - max(v)) * inv(v), the arithmetic of
//                  loss.hip's kernels.  A second sweep over k adds up the 'mse' and 'kl' sums.
//   k_wide_edge    a workgroup owns a spatial tile (2D 64 x 8, 3D 32 x 8 x 4 outputs) and marches over the classes 1..K-1:
//                  D_k = P_k - T_k on the tile and a one-voxel halo goes into LDS (two buffers, one barrier per class), the
//                  3^d stencils read it there.  The statistics of a thread's halo voxels stay in its registers over the march.
//                  Writes R (kept for the backward) and the two edge energies.
//   k_wide_bwd     the same tile, two sweeps over the classes.  First: g_k = gs (c_mse 2 m^2 D_k + c_a A^T R_A + c_b B^T R_B)
//                  (R_k tile + halo through LDS) goes into grad_pred, and dot = sum_k g_k P_k, sum_k m_k T'_k stay in
//                  registers.  Second: grad_k = P_k (g_k - dot) + kl part, in place -- a thread re-reads only what it
//                  wrote itself.  No atomics on grad_pred: bit-reproducible.
//
// Saved per evaluation: stats 16 V N bytes and R 8 (K - 1) V N bytes; P and D (8 K V N bytes) never exist.
// Streaming + 3^d stencil: memory-bound, no MFMA.
#include <algorithm>
#include "loss_common.h"

namespace advchain {

template <int VEC>
__device__ __forceinline__ void wload(const float* __restrict__ p, float (&o)[VEC]) {
  if (VEC == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  } else {
    o[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void wstore(float* __restrict__ p, const float (&o)[VEC]) {
  if (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  else p[0] = o[0];
}

// VEC voxels per lane (4: 16-byte loads, V % 4 == 0 and 16-byte aligned tensors)
template <int VEC, class... ORD>
__global__ void __launch_bounds__(kBlock)
k_wide_stats(const float* __restrict__ pred, const float* __restrict__ ref, const float* __restrict__ mask,
             float* __restrict__ stats, float* __restrict__ sums, int K, int V, int mask_ch, int ref_is_prob, int want_kl,
             ORD... ord) {
  __shared__ float smem[8];
  const int n = blockIdx.y;
  const int v = (blockIdx.x * kBlock + threadIdx.x) * VEC;
  float acc[2] = {0.f, 0.f};
  if (v < V) {
    const float* pn = pred + (int64_t)n * K * V + v;
    const float* rn = ref + (int64_t)n * K * V + v;
    float mp[VEC], sp[VEC], mr[VEC], sr[VEC];
    wload<VEC>(pn, mp);
    wload<VEC>(rn, mr);
#pragma unroll
    for (int q = 0; q < VEC; ++q) { sp[q] = 1.f; sr[q] = 1.f; }
    for (int k = 1; k < K; ++k) {
      float a[VEC], b[VEC];
      wload<VEC>(pn + (int64_t)k * V, a);
      wload<VEC>(rn + (int64_t)k * V, b);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        online_step(a[q], mp[q], sp[q]);
        if (!ref_is_prob) online_step(b[q], mr[q], sr[q]);
      }
    }
    float isp[VEC], isr[VEC], lsp[VEC], lsr[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      isp[q] = 1.f / sp[q];                      // ONE division per voxel and side
      isr[q] = 1.f / sr[q];
      lsp[q] = want_kl ? logf(sp[q]) : 0.f;
      lsr[q] = want_kl ? logf(sr[q]) : 0.f;
    }
    float m1[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) m1[q] = 1.f;
    if (mask && mask_ch == 1) wload<VEC>(mask + (int64_t)n * V + v, m1);
    for (int k = 0; k < K; ++k) {
      float a[VEC], b[VEC], m[VEC];
      wload<VEC>(pn + (int64_t)k * V, a);
      wload<VEC>(rn + (int64_t)k * V, b);
      if (mask && mask_ch > 1) wload<VEC>(mask + ((int64_t)n * mask_ch + k) * V + v, m);
#pragma unroll
      for (int q = 0; q < VEC; ++q) {
        const float zp = a[q] - mp[q], zr = b[q] - mr[q];
        const float p = mul_nc(ADVCHAIN_SM_EXP(zp), isp[q]);
        const float t = ref_is_prob ? b[q] : mul_nc(ADVCHAIN_SM_EXP(zr), isr[q]);
        const float mm = (mask && mask_ch > 1) ? m[q] : m1[q];
        const float e = p * mm - t * mm;
        acc[0] += e * e;
        if (want_kl) acc[1] += kl_term(t, zr - lsr[q], zp - lsp[q], mm, ref_is_prob);
      }
    }
    float* sn = stats + (int64_t)n * 4 * V + v;
    wstore<VEC>(sn, mp);
    wstore<VEC>(sn + V, isp);
    wstore<VEC>(sn + 2 * (int64_t)V, mr);
    wstore<VEC>(sn + 3 * (int64_t)V, isr);
  }
  block_sum<2>(acc, smem);
  if (threadIdx.x == 0) {
    sums_put(sums, 0, acc[0], ord...);
    if (want_kl) sums_put(sums, 3, acc[1], ord...);
  }
}

template <int DIM, class... ORD>
__global__ void __launch_bounds__(kBlock)
k_wide_edge(const float* __restrict__ pred, const float* __restrict__ ref, const float* __restrict__ mask,
            const float* __restrict__ stats, float* __restrict__ R, float* __restrict__ sums, int K, Dims d, int mask_ch,
            int ref_is_prob, ORD... ord) {
  using T = WTile<DIM>;
  __shared__ float lds[2][T::NH];
  __shared__ float smem[8];
  const T tile(d);
  const int n = blockIdx.y;
  const int V = (int)d.voxels();
  const float* sn = stats + (int64_t)n * 4 * V;
  int hv[T::SLOTS];
  float hmp[T::SLOTS], hip_[T::SLOTS], hmr[T::SLOTS], hir[T::SLOTS];
#pragma unroll
  for (int j = 0; j < T::SLOTS; ++j) {
    hv[j] = tile.halo_voxel(threadIdx.x + j * kBlock, d);
    const int c = max(hv[j], 0);
    hmp[j] = sn[c];
    hip_[j] = sn[(int64_t)V + c];
    hmr[j] = sn[2 * (int64_t)V + c];
    hir[j] = sn[3 * (int64_t)V + c];
  }
  int ov[T::OUTS], oc[T::OUTS];
  float om[T::OUTS];
#pragma unroll
  for (int j = 0; j < T::OUTS; ++j) {
    ov[j] = tile.out_voxel(threadIdx.x + j * kBlock, d, oc[j]);
    om[j] = (mask && ov[j] >= 0) ? mask[(int64_t)n * mask_ch * V + ov[j]] : 1.f;   // the stencil terms read channel 0
  }
  float acc[2] = {0.f, 0.f};
  for (int k = 1; k < K; ++k) {
    const float* pk = pred + ((int64_t)n * K + k) * V;
    const float* rk = ref + ((int64_t)n * K + k) * V;
    float* buf = lds[k & 1];
#pragma unroll
    for (int j = 0; j < T::SLOTS; ++j) {
      const int e = threadIdx.x + j * kBlock;
      const int c = max(hv[j], 0);
      const float xp = pk[c], xr = rk[c];          // unconditional loads from a clamped index: all in flight together
      const float p = mul_nc(ADVCHAIN_SM_EXP(xp - hmp[j]), hip_[j]);
      const float t = ref_is_prob ? xr : mul_nc(ADVCHAIN_SM_EXP(xr - hmr[j]), hir[j]);
      if (e < T::NH) buf[e] = hv[j] >= 0 ? p - t : 0.f;      // zero padding of the convolution
    }
    __syncthreads();     // (the other buffer is written next: one barrier per class)
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) {
      float ga, gb;
      tile_stencil<DIM, false>(buf, buf, oc[j], ga, gb);
      if (ov[j] >= 0) {
        const float m = om[j];
        const float ea = ga * m, eb = gb * m;
        acc[0] += ea * ea;
        acc[1] += eb * eb;
        if (R) {
          R[((int64_t)n * 2 * (K - 1) + 2 * (k - 1)) * V + ov[j]] = 2.f * m * m * ga;
          R[((int64_t)n * 2 * (K - 1) + 2 * (k - 1) + 1) * V + ov[j]] = 2.f * m * m * gb;
        }
      }
    }
  }
  block_sum<2>(acc, smem);
  if (threadIdx.x == 0) {
    sums_put(sums, 1, acc[0], ord...);
    sums_put(sums, 2, acc[1], ord...);
  }
}

template <int DIM>
__global__ void __launch_bounds__(kBlock)
k_wide_bwd(const float* __restrict__ pred, const float* __restrict__ ref, const float* __restrict__ stats,
           const float* __restrict__ R, const float* __restrict__ mask, const float* __restrict__ gscale, float* gpred,
           float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int K, Dims d, int mask_ch) {
  using T = WTile<DIM>;
  __shared__ float lds[2][2][T::NH];
  const T tile(d);
  const int n = blockIdx.y;
  const int V = (int)d.voxels();
  const float gs = gscale ? gscale[0] : 1.f;
  const float* sn = stats + (int64_t)n * 4 * V;
  int hv[T::SLOTS];
#pragma unroll
  for (int j = 0; j < T::SLOTS; ++j) hv[j] = tile.halo_voxel(threadIdx.x + j * kBlock, d);
  int ov[T::OUTS], oc[T::OUTS];
  float omp[T::OUTS], oip[T::OUTS], omr[T::OUTS], oir[T::OUTS], om[T::OUTS], dot[T::OUTS], klS[T::OUTS];
#pragma unroll
  for (int j = 0; j < T::OUTS; ++j) {
    ov[j] = tile.out_voxel(threadIdx.x + j * kBlock, d, oc[j]);
    const int c = max(ov[j], 0);
    omp[j] = sn[c];
    oip[j] = sn[(int64_t)V + c];
    omr[j] = sn[2 * (int64_t)V + c];
    oir[j] = sn[3 * (int64_t)V + c];
    om[j] = (mask && mask_ch == 1) ? mask[(int64_t)n * V + c] : 1.f;
    dot[j] = 0.f;
    klS[j] = 0.f;
  }
  const bool edges = R != nullptr;
  for (int k = 0; k < K; ++k) {
    const int64_t plane = ((int64_t)n * K + k) * V;
    float (*buf)[T::NH] = lds[k & 1];
    if (edges && k >= 1) {
      const float* Ra = R + ((int64_t)n * 2 * (K - 1) + 2 * (k - 1)) * V;
      const float* Rb = Ra + V;
#pragma unroll
      for (int j = 0; j < T::SLOTS; ++j) {
        const int e = threadIdx.x + j * kBlock;
        const int c = max(hv[j], 0);
        const float ra = Ra[c], rb = Rb[c];
        if (e < T::NH) {
          buf[0][e] = hv[j] >= 0 ? ra : 0.f;
          buf[1][e] = hv[j] >= 0 ? rb : 0.f;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) {
      const int c = max(ov[j], 0);
      const float xp = pred[plane + c], xr = ref[plane + c];
      const float m = (mask && mask_ch > 1) ? mask[((int64_t)n * mask_ch + k) * V + c] : om[j];
      const float p = mul_nc(ADVCHAIN_SM_EXP(xp - omp[j]), oip[j]);
      const float t = ref_is_prob ? xr : mul_nc(ADVCHAIN_SM_EXP(xr - omr[j]), oir[j]);
      float g = c_mse * 2.f * m * m * (p - t);
      if (edges && k >= 1) {
        float ta, tb;                 // A^T R_A, B^T R_B (R is zero outside the volume)
        tile_stencil<DIM, true>(buf[0], buf[1], oc[j], ta, tb);
        g += c_a * ta + c_b * tb;
      }
      g *= gs;
      if (ov[j] >= 0) gpred[plane + c] = g;
      dot[j] += g * p;
      if (c_kl != 0.f) klS[j] += m * kl_prob(t, ref_is_prob);
    }
  }
  // second sweep: the softmax Jacobian, in place (every thread re-reads only its own stores)
  for (int k = 0; k < K; ++k) {
    const int64_t plane = ((int64_t)n * K + k) * V;
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) {
      if (ov[j] < 0) continue;
      const int c = ov[j];
      const float xp = pred[plane + c];
      const float p = mul_nc(ADVCHAIN_SM_EXP(xp - omp[j]), oip[j]);
      float g = p * (gpred[plane + c] - dot[j]);
      if (c_kl != 0.f) {   // 'kl': gs c_kl (P_j sum_k m_k T'_k - m_j T'_j)
        const float xr = ref[plane + c];
        const float t = ref_is_prob ? xr : mul_nc(ADVCHAIN_SM_EXP(xr - omr[j]), oir[j]);
        const float m = (mask && mask_ch > 1) ? mask[((int64_t)n * mask_ch + k) * V + c] : om[j];
        g += gs * c_kl * (p * klS[j] - m * kl_prob(t, ref_is_prob));
      }
      gpred[plane + c] = g;
    }
  }
}

}  // namespace advchain

using namespace advchain;

static inline bool wide_nk_ok(int64_t N, int64_t K) { return N >= 0 && N < 65536 && K >= 1 && K < 65536; }

// advchain_consistency_wide_fwd (ORD empty, oc == nullptr: sums = the 4 x 64 slots) and advchain_consistency_wide_fwd_ord
// (one SumsOrdered, sums = the [4][oc->stride] partials): the same choice of kernels either way.
template <class... ORD>
static int wide_fwd(const OrdCounts* oc, const float* pred, const float* ref, const float* mask, float* stats,
                    float* R, float* sums, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels, int ref_is_prob,
                    int want_edges, int want_kl, void* stream, ORD... ord) {
  ADVCHAIN_CHECK_ARG(pred && ref && stats && sums && dims, "consistency_wide_fwd: null pointer");
  ADVCHAIN_CHECK_ARG(ldims_ok(ndim, dims), "consistency_wide_fwd: bad dims");
  ADVCHAIN_CHECK_ARG(wide_nk_ok(N, K), "consistency_wide_fwd: bad N/K (N < 65536, 1 <= K < 65536)");
  ADVCHAIN_CHECK_ARG(!mask || mask_channels == 1 || mask_channels == K, "consistency_wide_fwd: mask must have 1 or K channels");
  const Dims d = lmake_dims(ndim, dims);
  ADVCHAIN_CHECK_ARG(d.voxels() < (1ll << 31), "consistency_wide_fwd: volume too large");
  if (oc)
    for (int r = 0; r < 4; ++r) oc->counts[r] = 0;
  if (N == 0) return ADVCHAIN_OK;
  const int V = (int)d.voxels();
  hipStream_t st = (hipStream_t)stream;
  const dim3 b(kBlock);
  const bool al16 = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(ref) | reinterpret_cast<uintptr_t>(mask) |
                      reinterpret_cast<uintptr_t>(stats)) & 15) == 0;
  const bool vec4 = V % 4 == 0 && al16;
  const bool edges = want_edges && K > 1;
  const dim3 gs(advchain_blocks(vec4 ? V / 4 : V, kBlock), (unsigned)N);
  const dim3 ge((unsigned)(ndim == 3 ? WTile<3>::count(d) : WTile<2>::count(d)), (unsigned)N);
  if (oc) {
    ADVCHAIN_CHECK_ARG(oc->fits(gs) && (!edges || oc->fits(ge)),
                       "consistency_wide_fwd_ord: the partial buffer is smaller than a launch (advchain_consistency_wide_fwd_partials)");
    oc->set(0, gs);
    if (want_kl) oc->set(3, gs);
    if (edges) { oc->set(1, ge); oc->set(2, ge); }
  }
  if (vec4)
    hipLaunchKernelGGL((k_wide_stats<4, ORD...>), gs, b, 0, st, pred, ref, mask, stats,
                       sums, (int)K, V, mask_channels, ref_is_prob, want_kl, ord...);
  else
    hipLaunchKernelGGL((k_wide_stats<1, ORD...>), gs, b, 0, st, pred, ref, mask, stats,
                       sums, (int)K, V, mask_channels, ref_is_prob, want_kl, ord...);
  if (edges) {
    if (ndim == 3)
      hipLaunchKernelGGL((k_wide_edge<3, ORD...>), ge, b, 0, st, pred, ref, mask, stats, R,
                         sums, (int)K, d, mask_channels, ref_is_prob, ord...);
    else
      hipLaunchKernelGGL((k_wide_edge<2, ORD...>), ge, b, 0, st, pred, ref, mask, stats, R,
                         sums, (int)K, d, mask_channels, ref_is_prob, ord...);
  }
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

extern "C" {

int advchain_consistency_wide_fwd(const float* pred, const float* ref, const float* mask, float* stats, float* R, float* sums,
                                  int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels, int ref_is_prob,
                                  int want_edges, int want_kl, void* stream) {
  return wide_fwd<>(nullptr, pred, ref, mask, stats, R, sums, N, K, ndim, dims, mask_channels, ref_is_prob,
                    want_edges, want_kl, stream);
}

// The most workgroups a launch of advchain_consistency_wide_fwd(_ord) has for these arguments (aligned16: every tensor is
// 16-byte aligned): the capacity `stride` of a row of the partial buffer.  Host-only.
int64_t advchain_consistency_wide_fwd_partials(int64_t N, int64_t K, int ndim, const int64_t* dims, int want_edges, int aligned16) {
  if (!dims || !ldims_ok(ndim, dims) || !wide_nk_ok(N, K)) return -1;
  const Dims d = lmake_dims(ndim, dims);
  if (d.voxels() >= (1ll << 31)) return -1;
  const int64_t V = d.voxels();
  int64_t w = (int64_t)advchain_blocks((V % 4 == 0 && aligned16) ? V / 4 : V, kBlock) * N;
  if (want_edges && K > 1) w = std::max(w, (ndim == 3 ? WTile<3>::count(d) : WTile<2>::count(d)) * N);
  return w;
}

// advchain_consistency_wide_fwd with the sums in a fixed order (deterministic mode): partials[r * stride + workgroup] and
// counts[4] (host) as for advchain_consistency_lp_fwd_ord.
int advchain_consistency_wide_fwd_ord(const float* pred, const float* ref, const float* mask, float* stats, float* R,
                                      float* partials, int64_t stride, int32_t* counts, int64_t N, int64_t K, int ndim,
                                      const int64_t* dims, int mask_channels, int ref_is_prob, int want_edges, int want_kl,
                                      void* stream) {
  ADVCHAIN_CHECK_ARG(counts && stride >= 1 && stride < (1ll << 31), "consistency_wide_fwd_ord: bad partial buffer (stride / counts)");
  const OrdCounts oc{stride, counts};
  return wide_fwd<SumsOrdered>(&oc, pred, ref, mask, stats, R, partials, N, K, ndim, dims, mask_channels,
                               ref_is_prob, want_edges, want_kl, stream, SumsOrdered{(int)stride});
}

int advchain_consistency_wide_bwd(const float* pred, const float* ref, const float* stats, const float* R, const float* mask,
                                  const float* grad_scale, float* grad_pred, float c_mse, float c_a, float c_b, float c_kl,
                                  int ref_is_prob, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                                  void* stream) {
  ADVCHAIN_CHECK_ARG(pred && ref && stats && grad_pred && dims, "consistency_wide_bwd: null pointer");
  ADVCHAIN_CHECK_ARG(ldims_ok(ndim, dims), "consistency_wide_bwd: bad dims");
  ADVCHAIN_CHECK_ARG(wide_nk_ok(N, K), "consistency_wide_bwd: bad N/K (N < 65536, 1 <= K < 65536)");
  ADVCHAIN_CHECK_ARG(!mask || mask_channels == 1 || mask_channels == K, "consistency_wide_bwd: mask must have 1 or K channels");
  const Dims d = lmake_dims(ndim, dims);
  ADVCHAIN_CHECK_ARG(d.voxels() < (1ll << 31), "consistency_wide_bwd: volume too large");
  if (N == 0) return ADVCHAIN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (K == 1) R = nullptr;        // (no object class: nothing was saved)
  if (ndim == 3)
    hipLaunchKernelGGL(k_wide_bwd<3>, dim3((unsigned)WTile<3>::count(d), (unsigned)N), dim3(kBlock), 0, st, pred, ref, stats, R,
                       mask, grad_scale, grad_pred, c_mse, c_a, c_b, c_kl, ref_is_prob, (int)K, d, mask_channels);
  else
    hipLaunchKernelGGL(k_wide_bwd<2>, dim3((unsigned)WTile<2>::count(d), (unsigned)N), dim3(kBlock), 0, st, pred, ref, stats, R,
                       mask, grad_scale, grad_pred, c_mse, c_a, c_b, c_kl, ref_is_prob, (int)K, d, mask_channels);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
