// Typed loads and stores of one plane of a channels-first tensor: fp32 or raw bf16 words (`ST` = float / unsigned short) come
// in and go out as fp32 registers; int64 labels stay int64.  The ONE place where bf16 is rounded and where the 16-byte accesses
// are spelled out.
//
// Included by seg_common.h (and through it by seg_loss.hip, seg_dice.hip, seg_boundary.hip) and by loss_lp.hip, which builds
// its own 4-voxel access on it and must not include seg_common.h (the ld4 / st4 there would be ambiguous with its own).
// loss.hip keeps its own bf16_rne: it maps every NaN to 0x7fc0, this one keeps the payload.
#pragma once
#include "common.h"

namespace advchain {

__device__ __forceinline__ float qnan() { return __builtin_nanf(""); }

__device__ __forceinline__ unsigned short to_bf16(float x) {     // round to nearest even; NaN stays NaN
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// one value
template <typename ST>
__device__ __forceinline__ float ld1(const ST* __restrict__ p) {
  if constexpr (sizeof(ST) == 4) return p[0];
  else return __uint_as_float((unsigned)p[0] << 16);
}
template <typename ST>
__device__ __forceinline__ void st1(ST* __restrict__ p, float x) {
  if constexpr (sizeof(ST) == 4) p[0] = x;
  else p[0] = to_bf16(x);
}

// VEC consecutive values of one plane (VEC = 4: 16-byte fp32 / 8-byte bf16 accesses; the caller checks alignment)
template <typename ST, int VEC>
__device__ __forceinline__ void ld(const ST* __restrict__ p, float (&x)[VEC]) {
  if constexpr (VEC != 4) {
    x[0] = ld1<ST>(p);
  } else if constexpr (sizeof(ST) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
  } else {
    const uint2 a = *reinterpret_cast<const uint2*>(p);
    x[0] = __uint_as_float(a.x << 16); x[1] = __uint_as_float(a.x & 0xffff0000u);
    x[2] = __uint_as_float(a.y << 16); x[3] = __uint_as_float(a.y & 0xffff0000u);
  }
}

template <typename ST, int VEC>
__device__ __forceinline__ void st(ST* __restrict__ p, const float (&x)[VEC]) {
  if constexpr (VEC != 4) {
    st1<ST>(p, x[0]);
  } else if constexpr (sizeof(ST) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
    *reinterpret_cast<uint2*>(p) = make_uint2(to_bf16(x[0]) | ((unsigned)to_bf16(x[1]) << 16),
                                              to_bf16(x[2]) | ((unsigned)to_bf16(x[3]) << 16));
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

// host: may `p` take accesses of `bytes` bytes?  (a null pointer is an absent tensor: no objection)
inline bool aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

}  // namespace advchain
