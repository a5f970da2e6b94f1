// Segmentation-consistency loss ('mse' + 'contour' + 'kl') for a RUN-TIME class count and logits stored in fp32 or bf16 (a model
// under autocast), gfx950.
//
//   advchain_consistency_lp_fwd / lp_bwd / lp_ref_bwd <- calc_segmentation_consistency + contour_loss + kl_divergence,
//                                                        advchain/common/loss.py:8-87,102-220,223-249 (Q13, Q14) and what
//                                                        autograd gives both operands
//
//   advchain_consistency_cw_fwd / cw_bwd / cw_ref_bwd <- the same with class weights w_k (a parameter the reference documents
//                                                        and raises on): the same kernels with a trailing weight argument
//
//   advchain_consistency_wide_fwd / wide_bwd          <- the lp entries for two fp32 operands (the fp32 loss from 17 classes on)
//
// Same mathematics as loss.hip (see its header; the reference side: loss_ref.hip); what differs is that nothing here is sized
// by K.  loss.hip keeps a softmax row per voxel in registers (K <= 16) or materialises P and D; here the class axis is MARCHED,
// and each logit operand is read as fp32 or as bf16 (raw 16-bit words), independently -- bf16 -> fp32 is exact, so the forward
// is the fp32 loss of the upcast operands -- and each gradient is written in its operand's type, computed in fp32 and rounded
// once (to nearest even) at the store.  stats, R, the slot sums and the mask stay fp32.  Every K >= 1 runs here: with a bf16
// operand or class weights the K <= 16 register kernels of loss.hip are not used.
//
//   k_lp_stats     one streaming pass with a running max / sum of exp over the K planes leaves the softmax statistics of
//                  both operands, 16 bytes per voxel: stats (N, 4, V) = max_pred, 1 / sum_pred, max_ref, 1 / sum_ref.  With
//                  them every class plane is independent: P_k(v) = exp(pred_k(v) - max(v)) * inv(v), the arithmetic of
//                  loss.hip's kernels.  A second sweep over k adds up the 'mse' and 'kl' sums.  A lane owns 4 consecutive
//                  voxels in either access form -- 16-byte fp32 / 8-byte bf16 loads when V % 4 == 0 and every pointer allows
//                  it, else scalar loads of the same 4 voxels -- so the order of every sum, and with it the value, does not
//                  depend on the alignment of a tensor.
//   k_lp_edge      a workgroup owns a spatial tile (2D 64 x 8, 3D 32 x 8 x 4 outputs) and marches over the classes 1..K-1:
//                  D_k = P_k - T_k on the tile and a one-voxel halo goes into LDS (two buffers, one barrier per class), the
//                  3^d stencils read it there.  The statistics of a thread's halo voxels stay in its registers over the march.
//                  Writes R (kept for the backward) and the two edge energies.
//   k_lp_bwd       the same tile, two sweeps over the classes.  g_k = gs (c_mse 2 m^2 D_k + c_a A^T R_A + c_b B^T R_B) (R_k
//                  tile + halo through LDS) is the probability-space gradient; the first sweep leaves dot = sum_k g_k P_k and
//                  sum_k m_k T'_k in registers, the second stores grad_k = P_k (g_k - dot) + kl part.  An fp32 grad_pred
//                  PARKS g_k between the sweeps: the first sweep stores it, the second is the Jacobian in place and a thread
//                  re-reads only what it wrote itself.  A bf16 grad_pred would round the parked g_k before p_k (g_k - dot)
//                  cancels, so there the second sweep RECOMPUTES g_k instead of re-reading it: the only store of an element
//                  is the final, rounded one and no scratch exists.  Cost of recomputing against parking, per element: one
//                  more adjoint stencil pair (12 LDS reads in 2D, 36 in 3D), one more read of R through the halo (8 bytes x
//                  halo / tile = 1.29 in 2D, 1.99 in 3D) and one more barrier per class; saved: the 4-byte store and the
//                  4-byte re-read of the parked g_k (2 + 2 in bf16, were parking possible).  An fp32 scratch from the caller
//                  would have cost 4 K V N bytes of memory, 8 bytes of traffic per element and a workspace entry in the C
//                  ABI.  Measured with an fp32 output, recomputing against parking: 434 against 418 us at 32 x 20 x 256 x 256,
//                  1704 against 1272 us at 4 x 20 x 128 x 128 x 64, where recomputing runs 178 VGPRs and 2 waves per SIMD
//                  (profiles/r18/loss_fold/summary.md); with a bf16 output recomputing takes 349 us at the 2D shape
//                  (profiles/r10/bf16_loss/summary.md).
//   k_lp_ref_grad  the run-time form of k_loss_ref_grad (statistics always from `stats`: the forward saves them for every
//                  K), with a recomputing second sweep for h_k in every storage type.  ref_is_prob: one sweep, -g_k is the
//                  gradient.  (Two fp32 operands without weights: ops takes advchain_consistency_ref_bwd, loss_ref.hip, which
//                  parks h_k in grad_ref and is faster -- 299 against 438 us, 980 against 1716 us at the shapes above.)
//
// Saved per evaluation: stats 16 V N bytes and R 8 (K - 1) V N bytes; P and D (8 K V N bytes) never exist.
// The tile kernels read one value per lane and plane (a wave reads 64 consecutive values of a tile row: 128 contiguous bytes
// in bf16) at any alignment; only k_lp_stats has a vector form.  The adjoint stencils skip the zero-weight taps.  No atomics
// on the gradients and no shared accumulator: bit-reproducible.  Streaming + 3^d stencil: memory-bound, no MFMA.
#include <stdio.h>
#include <algorithm>

#include "loss_common.h"
#include "plane_io.h"

namespace advchain {
namespace {

typedef unsigned short bf16_t;     // raw bf16 words

// Class weights.  Each kernel ends in a parameter pack W... that is EMPTY (the lp entries: the unweighted loss, the very
// kernel arguments and instructions it had without the pack) or ONE `const float*` (the cw entries: K device floats, w_k read
// with a uniform load once per class and workgroup; no per-voxel traffic).  The weights do not change while a kernel runs, so
// they are read through the constant address space: there a uniform load is a scalar one (s_load_dword) whatever the kernel
// stores between two classes -- as a plain global load the compiler keeps it on the vector unit in the loops that store R or
// a gradient.
__device__ __forceinline__ float lp_cw(int) { return 1.f; }
__device__ __forceinline__ float lp_cw(int k, const float* cw) {
  return ((const __attribute__((address_space(4))) float*)cw)[k];
}
// The two FORWARD kernels may carry one more element behind the weights: a SumsOrdered (loss_common.h; the *_fwd_ord
// entries), which sends the workgroup partials to their own cells instead of the 64 slots.  W... is then one of
// {}, {const float*}, {SumsOrdered}, {const float*, SumsOrdered}; the first two are the kernels of the default mode.
__device__ __forceinline__ float lp_cw(int, const SumsOrdered&) { return 1.f; }
__device__ __forceinline__ float lp_cw(int k, const float* cw, const SumsOrdered&) { return lp_cw(k, cw); }
// (sums_put takes the same four packs: loss_common.h)
template <typename... W> struct lp_weighted { static constexpr bool value = false; };
template <typename... T> struct lp_weighted<const float*, T...> { static constexpr bool value = true; };

// 4 consecutive values of one plane: WIDE one 16-byte (fp32) / 8-byte (bf16) access, else `cnt` (1..4) scalar ones
template <typename ST, bool WIDE>
__device__ __forceinline__ void ld4(const ST* __restrict__ p, int cnt, float (&x)[4]) {
  if constexpr (WIDE) {
    ld<ST, 4>(p, x);
  } else {
    // The select form stays: the guarded form of seg_common.h (`if (q < cnt) x[q] = ...` over zeroed registers) compiles all 16
    // k_lp_stats<..., false, ...> instantiations to other instructions, as this form does the scalar Dice and boundary kernels.
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = q < cnt ? ld1<ST>(p + q) : 0.f;
  }
}
template <bool WIDE>
__device__ __forceinline__ void st4(float* __restrict__ p, int cnt, const float (&x)[4]) {
  if constexpr (WIDE) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < cnt) p[q] = x[q];
  }
}

// A lane owns the voxels 4 i .. 4 i + 3 of a batch entry (i its index in the grid), WIDE or not.
template <typename PT, typename RT, bool WIDE, typename... W>
__global__ void __launch_bounds__(kBlock)
k_lp_stats(const PT* __restrict__ pred, const RT* __restrict__ ref, const float* __restrict__ mask, float* __restrict__ stats,
           float* __restrict__ sums, int K, int V, int mask_ch, int ref_is_prob, int want_kl, W... cw) {
  constexpr bool CW = lp_weighted<W...>::value;
  __shared__ float smem[8];
  const int n = blockIdx.y;
  const int64_t v64 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
  float acc[2] = {0.f, 0.f};
  if (v64 < V) {
    const int v = (int)v64;
    const int cnt = min(4, V - v);
    const PT* pn = pred + (int64_t)n * K * V + v;
    const RT* rn = ref + (int64_t)n * K * V + v;
    float mp[4], sp[4], mr[4], sr[4];
    ld4<PT, WIDE>(pn, cnt, mp);
    ld4<RT, WIDE>(rn, cnt, mr);
#pragma unroll
    for (int q = 0; q < 4; ++q) { sp[q] = 1.f; sr[q] = 1.f; }
    for (int k = 1; k < K; ++k) {
      float a[4], b[4];
      ld4<PT, WIDE>(pn + (int64_t)k * V, cnt, a);
      ld4<RT, WIDE>(rn + (int64_t)k * V, cnt, b);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        online_step(a[q], mp[q], sp[q]);
        if (!ref_is_prob) online_step(b[q], mr[q], sr[q]);
      }
    }
    float isp[4], isr[4], lsp[4], lsr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      isp[q] = 1.f / sp[q];                      // ONE division per voxel and side
      isr[q] = 1.f / sr[q];
      lsp[q] = want_kl ? logf(sp[q]) : 0.f;
      lsr[q] = want_kl ? logf(sr[q]) : 0.f;
    }
    float m1[4] = {1.f, 1.f, 1.f, 1.f};
    if (mask && mask_ch == 1) ld4<float, WIDE>(mask + (int64_t)n * V + v, cnt, m1);
    for (int k = 0; k < K; ++k) {
      float a[4], b[4], m[4];
      ld4<PT, WIDE>(pn + (int64_t)k * V, cnt, a);
      ld4<RT, WIDE>(rn + (int64_t)k * V, cnt, b);
      if (mask && mask_ch > 1) ld4<float, WIDE>(mask + ((int64_t)n * mask_ch + k) * V + v, cnt, m);
      const float wk = lp_cw(k, cw...);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float zp = a[q] - mp[q], zr = b[q] - mr[q];
        const float p = mul_nc(ADVCHAIN_SM_EXP(zp), isp[q]);
        const float t = ref_is_prob ? b[q] : mul_nc(ADVCHAIN_SM_EXP(zr), isr[q]);
        const float mm = (mask && mask_ch > 1) ? m[q] : m1[q];
        const float e = p * mm - t * mm;
        if (q < cnt) {
          if constexpr (CW) {
            acc[0] += wk * (e * e);
            if (want_kl) acc[1] += wk * kl_term(t, zr - lsr[q], zp - lsp[q], mm, ref_is_prob);
          } else {
            acc[0] += e * e;
            if (want_kl) acc[1] += kl_term(t, zr - lsr[q], zp - lsp[q], mm, ref_is_prob);
          }
        }
      }
    }
    float* sn = stats + (int64_t)n * 4 * V + v;
    st4<WIDE>(sn, cnt, mp);
    st4<WIDE>(sn + V, cnt, isp);
    st4<WIDE>(sn + 2 * (int64_t)V, cnt, mr);
    st4<WIDE>(sn + 3 * (int64_t)V, cnt, isr);
  }
  block_sum<2>(acc, smem);
  if (threadIdx.x == 0) {
    sums_put(sums, 0, acc[0], cw...);
    if (want_kl) sums_put(sums, 3, acc[1], cw...);
  }
}

template <typename PT, typename RT, int DIM, typename... W>
__global__ void __launch_bounds__(kBlock)
k_lp_edge(const PT* __restrict__ pred, const RT* __restrict__ ref, const float* __restrict__ mask,
          const float* __restrict__ stats, float* __restrict__ R, float* __restrict__ sums, int K, Dims d, int mask_ch,
          int ref_is_prob, W... cw) {
  constexpr bool CW = lp_weighted<W...>::value;
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
    const PT* pk = pred + ((int64_t)n * K + k) * V;
    const RT* rk = ref + ((int64_t)n * K + k) * V;
    float* buf = lds[k & 1];
    const float wk = lp_cw(k, cw...);
#pragma unroll
    for (int j = 0; j < T::SLOTS; ++j) {
      const int e = threadIdx.x + j * kBlock;
      const int c = max(hv[j], 0);
      const float xp = ld1<PT>(pk + c), xr = ld1<RT>(rk + c);     // unconditional loads from a clamped index
      const float p = mul_nc(ADVCHAIN_SM_EXP(xp - hmp[j]), hip_[j]);
      const float t = ref_is_prob ? xr : mul_nc(ADVCHAIN_SM_EXP(xr - hmr[j]), hir[j]);
      if (e < T::NH) buf[e] = hv[j] >= 0 ? p - t : 0.f;      // zero padding of the convolution
    }
    __syncthreads();     // (the other buffer is written next: one barrier per class)
#pragma unroll
    for (int j = 0; j < T::OUTS; ++j) {
      float ga, gb;
      tile_stencil<DIM>(buf, buf, oc[j], ga, gb);
      if (ov[j] >= 0) {
        const float m = om[j];
        const float ea = ga * m, eb = gb * m;
        if constexpr (CW) {
          acc[0] += wk * (ea * ea);
          acc[1] += wk * (eb * eb);
        } else {
          acc[0] += ea * ea;
          acc[1] += eb * eb;
        }
        if (R) {                // (R_k is saved unweighted: the backward scales g_k)
          R[((int64_t)n * 2 * (K - 1) + 2 * (k - 1)) * V + ov[j]] = 2.f * m * m * ga;
          R[((int64_t)n * 2 * (K - 1) + 2 * (k - 1) + 1) * V + ov[j]] = 2.f * m * m * gb;
        }
      }
    }
  }
  block_sum<2>(acc, smem);
  if (threadIdx.x == 0) {
    sums_put(sums, 1, acc[0], cw...);
    sums_put(sums, 2, acc[1], cw...);
  }
}

// grad_pred.  Sweep 0 leaves dot = sum_k g_k P_k and sum_k m_k T'_k in registers; sweep 1 stores P_k (g_k - dot) + the 'kl'
// part.  Between the two, g_k is PARKED in an fp32 grad_pred (stored by sweep 0, re-read by the thread that wrote it) and
// RECOMPUTED for a bf16 one, which would round it: sweep 0 then stores nothing and the only store of an element is the final,
// rounded one.  The barrier between the recomputing sweeps: with an even K the last class of sweep 0 and the first staged
// class of sweep 1 use the same LDS buffer.
template <typename PT, typename RT, int DIM, typename... W>
__global__ void __launch_bounds__(kBlock)
k_lp_bwd(const PT* __restrict__ pred, const RT* __restrict__ ref, const float* __restrict__ stats, const float* __restrict__ R,
         const float* __restrict__ mask, const float* __restrict__ gscale, PT* __restrict__ gpred, float c_mse, float c_a,
         float c_b, float c_kl, int ref_is_prob, int K, Dims d, int mask_ch, W... cw) {
  constexpr bool CW = sizeof...(W) != 0;
  constexpr bool PARK = sizeof(PT) == 4;
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
  for (int sweep = 0; sweep < (PARK ? 1 : 2); ++sweep) {
    if (sweep) __syncthreads();
    for (int k = 0; k < K; ++k) {
      const int64_t plane = ((int64_t)n * K + k) * V;
      const float wk = lp_cw(k, cw...);
      float (*buf)[T::NH] = lds[k & 1];
      if (edges && k >= 1) {
        const float* Ra = R + ((int64_t)n * 2 * (K - 1) + 2 * (k - 1)) * V;
        stage_R<DIM>(buf, Ra, Ra + V, hv);
        __syncthreads();     // (the other buffer is written next: one barrier per class)
      }
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        const int c = max(ov[j], 0);
        const float xp = ld1<PT>(pred + plane + c), xr = ld1<RT>(ref + plane + c);
        const float m = (mask && mask_ch > 1) ? mask[((int64_t)n * mask_ch + k) * V + c] : om[j];
        const float p = mul_nc(ADVCHAIN_SM_EXP(xp - omp[j]), oip[j]);
        const float t = ref_is_prob ? xr : mul_nc(ADVCHAIN_SM_EXP(xr - omr[j]), oir[j]);
        float g = c_mse * 2.f * m * m * (p - t);
        if (edges && k >= 1) {
          float ta, tb;                 // A^T R_A, B^T R_B (R is zero outside the volume)
          adjoint_stencil<DIM>(buf[0], buf[1], oc[j], ta, tb);
          g += c_a * ta + c_b * tb;
        }
        if constexpr (CW) g *= wk;
        g *= gs;
        const float wm = CW ? wk * m : m;     // 'kl' takes w_k m_k where the unweighted loss takes m_k
        if (sweep == 0) {
          if constexpr (PARK) {
            if (ov[j] >= 0) gpred[plane + c] = g;
          }
          dot[j] += g * p;
          if (c_kl != 0.f) klS[j] += wm * kl_prob(t, ref_is_prob);
        } else if (ov[j] >= 0) {
          float o = p * (g - dot[j]);     // the softmax Jacobian
          if (c_kl != 0.f) o += gs * c_kl * (p * klS[j] - wm * kl_prob(t, ref_is_prob));   // 'kl': gs c_kl (P_j sum_k m_k T'_k - m_j T'_j)
          st1<PT>(gpred + plane + c, o);
        }
      }
    }
  }
  if constexpr (PARK) {
    // second sweep over the parked g_k: the softmax Jacobian in place (every thread re-reads only its own stores)
    for (int k = 0; k < K; ++k) {
      const int64_t plane = ((int64_t)n * K + k) * V;
      const float wk = lp_cw(k, cw...);
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        if (ov[j] < 0) continue;
        const int c = ov[j];
        const float xp = ld1<PT>(pred + plane + c);
        const float p = mul_nc(ADVCHAIN_SM_EXP(xp - omp[j]), oip[j]);
        float o = p * (gpred[plane + c] - dot[j]);
        if (c_kl != 0.f) {   // 'kl': gs c_kl (P_j sum_k m_k T'_k - m_j T'_j)
          const float xr = ld1<RT>(ref + plane + c);
          const float t = ref_is_prob ? xr : mul_nc(ADVCHAIN_SM_EXP(xr - omr[j]), oir[j]);
          const float m = (mask && mask_ch > 1) ? mask[((int64_t)n * mask_ch + k) * V + c] : om[j];
          const float wm = CW ? wk * m : m;
          o += gs * c_kl * (p * klS[j] - wm * kl_prob(t, ref_is_prob));
        }
        gpred[plane + c] = o;
      }
    }
  }
}

// grad_ref.  h_k = -g_k + gs c_kl m_k (log T_k + 1 - log P_k); ref_is_prob: h_k is the gradient (one sweep); logits: sweep 0
// leaves sum_j T_j h_j in registers, sweep 1 recomputes h_k and stores T_k (h_k - sum), rounded once.
template <typename PT, typename RT, int DIM, typename... W>
__global__ void __launch_bounds__(kBlock)
k_lp_ref_grad(const PT* __restrict__ pred, const RT* __restrict__ ref, const float* __restrict__ stats,
              const float* __restrict__ R, const float* __restrict__ mask, const float* __restrict__ gscale,
              RT* __restrict__ gref, float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int K, Dims d,
              int mask_ch, W... cw) {
  constexpr bool CW = sizeof...(W) != 0;
  using T = WTile<DIM>;
  __shared__ float lds[2][2][T::NH];
  const T tile(d);
  const int n = blockIdx.y;
  const int V = (int)d.voxels();
  const float gs = gscale ? gscale[0] : 1.f;
  const bool edges = R != nullptr;
  const bool kl = c_kl != 0.f && !ref_is_prob;
  const float ckl = gs * c_kl;
  const float* sn = stats + (int64_t)n * 4 * V;
  int hv[T::SLOTS];
#pragma unroll
  for (int j = 0; j < T::SLOTS; ++j) hv[j] = tile.halo_voxel(threadIdx.x + j * kBlock, d);
  int ov[T::OUTS], oc[T::OUTS];
  float om[T::OUTS], dot[T::OUTS], omp[T::OUTS], oip[T::OUTS], omr[T::OUTS], oir[T::OUTS], lgd[T::OUTS];
#pragma unroll
  for (int j = 0; j < T::OUTS; ++j) {
    ov[j] = tile.out_voxel(threadIdx.x + j * kBlock, d, oc[j]);
    const int c = max(ov[j], 0);
    om[j] = (mask && mask_ch == 1) ? mask[(int64_t)n * V + c] : 1.f;
    dot[j] = 0.f;
    omp[j] = sn[c];
    oip[j] = sn[(int64_t)V + c];
    omr[j] = ref_is_prob ? 0.f : sn[2 * (int64_t)V + c];      // (the ref planes are unspecified when ref_is_prob)
    oir[j] = ref_is_prob ? 1.f : sn[3 * (int64_t)V + c];
    lgd[j] = kl ? logf(oir[j]) - logf(oip[j]) : 0.f;          // log inv_r - log inv_p
  }
  const int64_t batch = (int64_t)n * K * V;
  const int sweeps = ref_is_prob ? 1 : 2;
  for (int sweep = 0; sweep < sweeps; ++sweep) {
    if (sweep) __syncthreads();
    for (int k = 0; k < K; ++k) {
      const int64_t plane = batch + (int64_t)k * V;
      const float wk = lp_cw(k, cw...);
      float (*buf)[T::NH] = lds[k & 1];
      if (edges && k >= 1) {
        const float* Ra = R + ((int64_t)n * 2 * (K - 1) + 2 * (k - 1)) * V;
        stage_R<DIM>(buf, Ra, Ra + V, hv);
        __syncthreads();     // (the other buffer is written next: one barrier per class)
      }
#pragma unroll
      for (int j = 0; j < T::OUTS; ++j) {
        const int c = max(ov[j], 0);
        const float xp = ld1<PT>(pred + plane + c), xr = ld1<RT>(ref + plane + c);
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
        if constexpr (CW) g *= wk;
        float hk = -(g * gs);
        if (kl) hk += ckl * (CW ? wk * m : m) * ((zr - zp) + lgd[j] + 1.f);
        if (sweep == 0) {
          dot[j] += t * hk;
          if (ref_is_prob && ov[j] >= 0) st1<RT>(gref + plane + c, hk);     // already the gradient
        } else if (ov[j] >= 0) {
          st1<RT>(gref + plane + c, t * (hk - dot[j]));     // the softmax Jacobian of the reference
        }
      }
    }
  }
}

inline bool lp_nk_ok(int64_t N, int64_t K) { return N >= 0 && N < 65536 && K >= 1 && K < 65536; }
inline bool lp_flag_ok(int f) { return f == 0 || f == 1; }

// w: nothing (the lp entries) or the K class weights in device memory (the cw entries), and behind them a SumsOrdered for the
// *_fwd_ord entries; it selects the kernels' pack.  `oc` (the ord entries only): the partial buffer's capacity and the host
// array that receives the workgroup count of every row written.  false: a launch has more workgroups than the buffer holds
// (nothing was enqueued).
template <typename PT, typename RT, typename... W>
bool lp_launch_fwd(hipStream_t st, const OrdCounts* oc, const void* pred, const void* ref, const float* mask, float* stats, float* R,
                   float* sums, int N, int K, int ndim, Dims d, int mask_ch, int ref_is_prob, int want_edges, int want_kl, W... w) {
  const int V = (int)d.voxels();
  const PT* p = (const PT*)pred;
  const RT* r = (const RT*)ref;
  const dim3 b(kBlock);
  const dim3 g((unsigned)advchain_blocks(((int64_t)V + 3) / 4, kBlock), (unsigned)N);
  const bool edges = want_edges && K > 1;
  const dim3 ge((unsigned)(ndim == 3 ? WTile<3>::count(d) : WTile<2>::count(d)), (unsigned)N);
  if (oc) {
    if (!oc->fits(g) || (edges && !oc->fits(ge))) return false;
    oc->set(0, g);
    if (want_kl) oc->set(3, g);
    if (edges) { oc->set(1, ge); oc->set(2, ge); }
  }
  const bool wide = V % 4 == 0 && aligned(pred, 4 * (int)sizeof(PT)) && aligned(ref, 4 * (int)sizeof(RT)) &&
                    aligned(mask, 16) && aligned(stats, 16);
  if (wide)
    hipLaunchKernelGGL((k_lp_stats<PT, RT, true>), g, b, 0, st, p, r, mask, stats, sums, K, V, mask_ch, ref_is_prob, want_kl,
                       w...);
  else
    hipLaunchKernelGGL((k_lp_stats<PT, RT, false>), g, b, 0, st, p, r, mask, stats, sums, K, V, mask_ch, ref_is_prob, want_kl,
                       w...);
  if (edges) {
    if (ndim == 3)
      hipLaunchKernelGGL((k_lp_edge<PT, RT, 3>), ge, b, 0, st, p, r, mask, stats, R,
                         sums, K, d, mask_ch, ref_is_prob, w...);
    else
      hipLaunchKernelGGL((k_lp_edge<PT, RT, 2>), ge, b, 0, st, p, r, mask, stats, R,
                         sums, K, d, mask_ch, ref_is_prob, w...);
  }
  return true;
}

template <typename PT, typename RT, typename... W>
void lp_launch_bwd(hipStream_t st, const void* pred, const void* ref, const float* stats, const float* R, const float* mask,
                   const float* gs, void* gpred, float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int N, int K,
                   int ndim, Dims d, int mask_ch, W... w) {
  if (ndim == 3)
    hipLaunchKernelGGL((k_lp_bwd<PT, RT, 3>), dim3((unsigned)WTile<3>::count(d), (unsigned)N), dim3(kBlock), 0, st,
                       (const PT*)pred, (const RT*)ref, stats, R, mask, gs, (PT*)gpred, c_mse, c_a, c_b, c_kl, ref_is_prob, K, d,
                       mask_ch, w...);
  else
    hipLaunchKernelGGL((k_lp_bwd<PT, RT, 2>), dim3((unsigned)WTile<2>::count(d), (unsigned)N), dim3(kBlock), 0, st,
                       (const PT*)pred, (const RT*)ref, stats, R, mask, gs, (PT*)gpred, c_mse, c_a, c_b, c_kl, ref_is_prob, K, d,
                       mask_ch, w...);
}

template <typename PT, typename RT, typename... W>
void lp_launch_ref(hipStream_t st, const void* pred, const void* ref, const float* stats, const float* R, const float* mask,
                   const float* gs, void* gref, float c_mse, float c_a, float c_b, float c_kl, int ref_is_prob, int N, int K,
                   int ndim, Dims d, int mask_ch, W... w) {
  if (ndim == 3)
    hipLaunchKernelGGL((k_lp_ref_grad<PT, RT, 3>), dim3((unsigned)WTile<3>::count(d), (unsigned)N), dim3(kBlock), 0, st,
                       (const PT*)pred, (const RT*)ref, stats, R, mask, gs, (RT*)gref, c_mse, c_a, c_b, c_kl, ref_is_prob, K, d,
                       mask_ch, w...);
  else
    hipLaunchKernelGGL((k_lp_ref_grad<PT, RT, 2>), dim3((unsigned)WTile<2>::count(d), (unsigned)N), dim3(kBlock), 0, st,
                       (const PT*)pred, (const RT*)ref, stats, R, mask, gs, (RT*)gref, c_mse, c_a, c_b, c_kl, ref_is_prob, K, d,
                       mask_ch, w...);
}

// one of the four storage pairs
#define ADVCHAIN_LP_DISPATCH(fn, pb, rb, ...)                  \
  do {                                                         \
    if (pb) {                                                  \
      if (rb) fn<bf16_t, bf16_t>(__VA_ARGS__);                 \
      else fn<bf16_t, float>(__VA_ARGS__);                     \
    } else {                                                   \
      if (rb) fn<float, bf16_t>(__VA_ARGS__);                  \
      else fn<float, float>(__VA_ARGS__);                      \
    }                                                          \
  } while (0)

// an argument error of entry `who` (the lp and the cw entries share their bodies)
#define ADVCHAIN_LP_CHECK(cond, text)                          \
  do {                                                         \
    if (!(cond)) {                                             \
      char msg_[160];                                          \
      snprintf(msg_, sizeof(msg_), "%s: %s", who, text);       \
      advchain_set_error_(msg_);                               \
      return ADVCHAIN_ERR_ARG;                                 \
    }                                                          \
  } while (0)

// the checks every entry makes; `out` is the tensor it writes besides stats
#define ADVCHAIN_LP_CHECK_COMMON(out)                                                                          \
  ADVCHAIN_LP_CHECK(pred && ref && stats && out && dims, "null pointer");                                      \
  ADVCHAIN_LP_CHECK(!weighted || class_w, "null pointer (class_w)");                                           \
  ADVCHAIN_LP_CHECK(lp_flag_ok(pred_bf16) && lp_flag_ok(ref_bf16), "an operand is fp32 (0) or bf16 (1)");      \
  ADVCHAIN_LP_CHECK(dims_ok(ndim, dims), "bad dims");                                                          \
  ADVCHAIN_LP_CHECK(lp_nk_ok(N, K), "bad N/K (N < 65536, 1 <= K < 65536)");                                    \
  ADVCHAIN_LP_CHECK(!mask || mask_channels == 1 || mask_channels == K, "mask must have 1 or K channels");      \
  const Dims d = make_dims(ndim, dims);                                                                        \
  ADVCHAIN_LP_CHECK(d.voxels() < (1ll << 31), "volume too large")

// `oc` == nullptr: the lp / cw entries (sums = the 4 x 64 slots).  Otherwise the ord entries: sums = the [4][oc->stride] partials.
int lp_fwd(const char* who, bool weighted, const OrdCounts* oc, const void* pred, int pred_bf16, const void* ref, int ref_bf16,
           const float* mask, float* stats, float* R, float* sums, int64_t N, int64_t K, int ndim, const int64_t* dims,
           int mask_channels, int ref_is_prob, int want_edges, int want_kl, const float* class_w, void* stream) {
  ADVCHAIN_LP_CHECK_COMMON(sums);
  if (oc) {
    ADVCHAIN_LP_CHECK(oc->counts && oc->stride >= 1 && oc->stride < (1ll << 31), "bad partial buffer (stride / counts)");
    for (int r = 0; r < 4; ++r) oc->counts[r] = 0;
  }
  if (N == 0) return ADVCHAIN_OK;
  bool ok = true;
#define ADVCHAIN_LP_FWD_ARGS                                                                                             \
  (hipStream_t) stream, oc, pred, ref, mask, stats, R, sums, (int)N, (int)K, ndim, d, mask_channels, ref_is_prob, want_edges, \
      want_kl
  if (oc) {
    const SumsOrdered so{(int)oc->stride};
    if (weighted) ADVCHAIN_LP_DISPATCH(ok = lp_launch_fwd, pred_bf16, ref_bf16, ADVCHAIN_LP_FWD_ARGS, class_w, so);
    else ADVCHAIN_LP_DISPATCH(ok = lp_launch_fwd, pred_bf16, ref_bf16, ADVCHAIN_LP_FWD_ARGS, so);
  } else {
    if (weighted) ADVCHAIN_LP_DISPATCH(ok = lp_launch_fwd, pred_bf16, ref_bf16, ADVCHAIN_LP_FWD_ARGS, class_w);
    else ADVCHAIN_LP_DISPATCH(ok = lp_launch_fwd, pred_bf16, ref_bf16, ADVCHAIN_LP_FWD_ARGS);
  }
#undef ADVCHAIN_LP_FWD_ARGS
  ADVCHAIN_LP_CHECK(ok, "the partial buffer is smaller than a launch (size it with advchain_consistency_lp_fwd_partials)");
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int lp_bwd(const char* who, bool weighted, bool ref_side, const void* pred, int pred_bf16, const void* ref, int ref_bf16,
           const float* stats, const float* R, const float* mask, const float* grad_scale, void* grad, float c_mse, float c_a,
           float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
           const float* class_w, void* stream) {
  ADVCHAIN_LP_CHECK_COMMON(grad);
  if (N == 0) return ADVCHAIN_OK;
  if (K == 1) R = nullptr;        // (no object class: nothing was saved)
#define ADVCHAIN_LP_BWD_ARGS                                                                                              \
  (hipStream_t) stream, pred, ref, stats, R, mask, grad_scale, grad, c_mse, c_a, c_b, c_kl, ref_is_prob, (int)N, (int)K, ndim, d, \
      mask_channels
  if (ref_side) {
    if (weighted) ADVCHAIN_LP_DISPATCH(lp_launch_ref, pred_bf16, ref_bf16, ADVCHAIN_LP_BWD_ARGS, class_w);
    else ADVCHAIN_LP_DISPATCH(lp_launch_ref, pred_bf16, ref_bf16, ADVCHAIN_LP_BWD_ARGS);
  } else {
    if (weighted) ADVCHAIN_LP_DISPATCH(lp_launch_bwd, pred_bf16, ref_bf16, ADVCHAIN_LP_BWD_ARGS, class_w);
    else ADVCHAIN_LP_DISPATCH(lp_launch_bwd, pred_bf16, ref_bf16, ADVCHAIN_LP_BWD_ARGS);
  }
#undef ADVCHAIN_LP_BWD_ARGS
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int advchain_consistency_lp_fwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* mask, float* stats,
                                float* R, float* sums, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                                int ref_is_prob, int want_edges, int want_kl, void* stream) {
  return lp_fwd("consistency_lp_fwd", false, nullptr, pred, pred_bf16, ref, ref_bf16, mask, stats, R, sums, N, K, ndim, dims,
                mask_channels, ref_is_prob, want_edges, want_kl, nullptr, stream);
}

int advchain_consistency_lp_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                const float* R, const float* mask, const float* grad_scale, void* grad_pred, float c_mse,
                                float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K, int ndim,
                                const int64_t* dims, int mask_channels, void* stream) {
  return lp_bwd("consistency_lp_bwd", false, false, pred, pred_bf16, ref, ref_bf16, stats, R, mask, grad_scale, grad_pred, c_mse,
                c_a, c_b, c_kl, ref_is_prob, N, K, ndim, dims, mask_channels, nullptr, stream);
}

int advchain_consistency_lp_ref_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                    const float* R, const float* mask, const float* grad_scale, void* grad_ref, float c_mse,
                                    float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K, int ndim,
                                    const int64_t* dims, int mask_channels, void* stream) {
  return lp_bwd("consistency_lp_ref_bwd", false, true, pred, pred_bf16, ref, ref_bf16, stats, R, mask, grad_scale, grad_ref,
                c_mse, c_a, c_b, c_kl, ref_is_prob, N, K, ndim, dims, mask_channels, nullptr, stream);
}

// The most workgroups a launch of the two entries below (and of lp_fwd / cw_fwd, whose grids they share) has for these
// arguments: the capacity `stride` of a row of their partial buffer.  Host-only.
int64_t advchain_consistency_lp_fwd_partials(int64_t N, int64_t K, int ndim, const int64_t* dims, int want_edges) {
  if (!dims_ok(ndim, dims) || !lp_nk_ok(N, K)) return -1;
  const Dims d = make_dims(ndim, dims);
  if (d.voxels() >= (1ll << 31)) return -1;
  int64_t w = (int64_t)advchain_blocks((d.voxels() + 3) / 4, kBlock) * N;
  if (want_edges && K > 1) w = std::max(w, (ndim == 3 ? WTile<3>::count(d) : WTile<2>::count(d)) * N);
  return w;
}

// advchain_consistency_lp_fwd / cw_fwd with the sums in a fixed order (deterministic mode): the same kernels, but every
// workgroup stores its partial of row r at partials[r * stride + workgroup] instead of adding it into a slot, and
// counts[r] (host, 4 entries) receives the number of cells of row r that were written (0: the row is not part of this
// evaluation) -- what advchain_consistency_finish_ord adds up.  class_w == NULL: the unweighted loss.
int advchain_consistency_lp_fwd_ord(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* mask, float* stats,
                                    float* R, float* partials, int64_t stride, int32_t* counts, int64_t N, int64_t K, int ndim,
                                    const int64_t* dims, int mask_channels, int ref_is_prob, int want_edges, int want_kl,
                                    const float* class_w, void* stream) {
  const OrdCounts oc{stride, counts};
  return lp_fwd("consistency_lp_fwd_ord", class_w != nullptr, &oc, pred, pred_bf16, ref, ref_bf16, mask, stats, R, partials, N, K,
                ndim, dims, mask_channels, ref_is_prob, want_edges, want_kl, class_w, stream);
}

// the class-weighted entries: the same kernels with CW = true, for all four storage pairs (fp32-fp32 included)
int advchain_consistency_cw_fwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* mask, float* stats,
                                float* R, float* sums, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                                int ref_is_prob, int want_edges, int want_kl, const float* class_w, void* stream) {
  return lp_fwd("consistency_cw_fwd", true, nullptr, pred, pred_bf16, ref, ref_bf16, mask, stats, R, sums, N, K, ndim, dims,
                mask_channels, ref_is_prob, want_edges, want_kl, class_w, stream);
}

int advchain_consistency_cw_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                const float* R, const float* mask, const float* grad_scale, void* grad_pred, float c_mse,
                                float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K, int ndim,
                                const int64_t* dims, int mask_channels, const float* class_w, void* stream) {
  return lp_bwd("consistency_cw_bwd", true, false, pred, pred_bf16, ref, ref_bf16, stats, R, mask, grad_scale, grad_pred, c_mse,
                c_a, c_b, c_kl, ref_is_prob, N, K, ndim, dims, mask_channels, class_w, stream);
}

int advchain_consistency_cw_ref_bwd(const void* pred, int pred_bf16, const void* ref, int ref_bf16, const float* stats,
                                    const float* R, const float* mask, const float* grad_scale, void* grad_ref, float c_mse,
                                    float c_a, float c_b, float c_kl, int ref_is_prob, int64_t N, int64_t K, int ndim,
                                    const int64_t* dims, int mask_channels, const float* class_w, void* stream) {
  return lp_bwd("consistency_cw_ref_bwd", true, true, pred, pred_bf16, ref, ref_bf16, stats, R, mask, grad_scale, grad_ref,
                c_mse, c_a, c_b, c_kl, ref_is_prob, N, K, ndim, dims, mask_channels, class_w, stream);
}

// the fp32 entries of the run-time-K loss (the unweighted fp32 loss from 17 classes on): the lp entries with both operands fp32
int advchain_consistency_wide_fwd(const float* pred, const float* ref, const float* mask, float* stats, float* R, float* sums,
                                  int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels, int ref_is_prob,
                                  int want_edges, int want_kl, void* stream) {
  return lp_fwd("consistency_wide_fwd", false, nullptr, pred, 0, ref, 0, mask, stats, R, sums, N, K, ndim, dims, mask_channels,
                ref_is_prob, want_edges, want_kl, nullptr, stream);
}

int advchain_consistency_wide_bwd(const float* pred, const float* ref, const float* stats, const float* R, const float* mask,
                                  const float* grad_scale, float* grad_pred, float c_mse, float c_a, float c_b, float c_kl,
                                  int ref_is_prob, int64_t N, int64_t K, int ndim, const int64_t* dims, int mask_channels,
                                  void* stream) {
  return lp_bwd("consistency_wide_bwd", false, false, pred, 0, ref, 0, stats, R, mask, grad_scale, grad_pred, c_mse, c_a, c_b,
                c_kl, ref_is_prob, N, K, ndim, dims, mask_channels, nullptr, stream);
}

// (aligned16 is accepted and ignored: the grid does not depend on the alignment of a tensor)
int64_t advchain_consistency_wide_fwd_partials(int64_t N, int64_t K, int ndim, const int64_t* dims, int want_edges, int) {
  return advchain_consistency_lp_fwd_partials(N, K, ndim, dims, want_edges);
}

int advchain_consistency_wide_fwd_ord(const float* pred, const float* ref, const float* mask, float* stats, float* R,
                                      float* partials, int64_t stride, int32_t* counts, int64_t N, int64_t K, int ndim,
                                      const int64_t* dims, int mask_channels, int ref_is_prob, int want_edges, int want_kl,
                                      void* stream) {
  const OrdCounts oc{stride, counts};
  return lp_fwd("consistency_wide_fwd_ord", false, &oc, pred, 0, ref, 0, mask, stats, R, partials, N, K, ndim, dims,
                mask_channels, ref_is_prob, want_edges, want_kl, nullptr, stream);
}

}  // extern "C"
