// Helpers shared by the supervised-loss kernels (seg_loss.hip, seg_dice.hip): 4-voxel loads and stores of fp32 / bf16 planes and
// int64 labels, and the class weights of the cross entropy.
#pragma once
#include "common.h"

namespace advchain {

__device__ __forceinline__ float qnan() { return __builtin_nanf(""); }

__device__ __forceinline__ unsigned short to_bf16(float x) {     // round to nearest even; NaN stays NaN
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// VEC consecutive values of one plane (VEC = 4: 16-byte fp32 / 8-byte bf16 accesses; the caller checks alignment)
template <typename ST, int VEC>
__device__ __forceinline__ void ld(const ST* __restrict__ p, float (&x)[VEC]) {
  if constexpr (sizeof(ST) == 4) {
    if constexpr (VEC == 4) {
      const float4 a = *reinterpret_cast<const float4*>(p);
      x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    } else {
      x[0] = p[0];
    }
  } else {
    if constexpr (VEC == 4) {
      const uint2 a = *reinterpret_cast<const uint2*>(p);
      x[0] = __uint_as_float(a.x << 16); x[1] = __uint_as_float(a.x & 0xffff0000u);
      x[2] = __uint_as_float(a.y << 16); x[3] = __uint_as_float(a.y & 0xffff0000u);
    } else {
      x[0] = __uint_as_float((unsigned)p[0] << 16);
    }
  }
}

template <typename ST, int VEC>
__device__ __forceinline__ void st(ST* __restrict__ p, const float (&x)[VEC]) {
  if constexpr (sizeof(ST) == 4) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else p[0] = x[0];
  } else {
    if constexpr (VEC == 4) {
      *reinterpret_cast<uint2*>(p) = make_uint2(to_bf16(x[0]) | ((unsigned)to_bf16(x[1]) << 16),
                                                to_bf16(x[2]) | ((unsigned)to_bf16(x[3]) << 16));
    } else {
      p[0] = to_bf16(x[0]);
    }
  }
}

template <int VEC>
__device__ __forceinline__ void ld_labels(const int64_t* __restrict__ p, int64_t (&y)[VEC]) {
  if constexpr (VEC == 4) {
    const longlong2 a = *reinterpret_cast<const longlong2*>(p);
    const longlong2 b = *reinterpret_cast<const longlong2*>(p + 2);
    y[0] = a.x; y[1] = a.y; y[2] = b.x; y[3] = b.y;
  } else {
    y[0] = p[0];
  }
}

// sum of the raw class weights, in class order (every lane the same: uniform loads)
__device__ __forceinline__ float weight_sum(const float* __restrict__ weight, int K) {
  float s = 0.f;
  for (int c = 0; c < K; ++c) s += weight[c];
  return s;
}
// w_c / sum(w) * K, rounded as the reference does (loss.py:290,316)
__device__ __forceinline__ float class_weight(const float* __restrict__ weight, int c, float wsum, float Kf) {
  return weight ? (weight[c] / wsum) * Kf : 1.f;
}

inline bool aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

}  // namespace advchain
