// Pieces shared by the consistency-loss translation units (loss.hip: K <= 16 in registers; loss_wide.hip: run-time K).
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

// stencil weights at tap (a0,a1,a2) in {0,1,2}^3 (a0 unused in 2D)
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

static inline bool ldims_ok(int ndim, const int64_t* s) {
  if (ndim != 2 && ndim != 3) return false;
  for (int i = 0; i < ndim; ++i)
    if (s[i] < 1 || s[i] > (1 << 24)) return false;
  return true;
}
static inline Dims lmake_dims(int ndim, const int64_t* s) {
  Dims d;
  if (ndim == 3) { d.s0 = (int)s[0]; d.s1 = (int)s[1]; d.s2 = (int)s[2]; }
  else { d.s0 = 1; d.s1 = (int)s[0]; d.s2 = (int)s[1]; }
  return d;
}

}  // namespace advchain
