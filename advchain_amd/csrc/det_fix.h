// The passes around an int64 fixed-point image of grad_in (deterministic mode): shared by the window scatter's twin
// (scatter_window.hip) and by the twins of the general sampler backward and of the affine scatter (sampler.hip).
//   clear (advchain_zero_async) -> k_det_absmax -> the scatter kernel, 64-bit integer atomics -> k_det_convert
// The scale comes from a max |grad_out| per batch entry (a NaN / inf there turns the entry's outputs into NaN) -- per
// entry, so that a sample's result does not depend on what else is in the batch.  Resolution 2^-bits of that maximum per
// addition.  The kernels are `static`: every translation unit that includes this header gets its own copy.
#pragma once
#include "common.h"

namespace advchain {

constexpr int kDetBits = 40;   // (fix_scale)
__device__ __forceinline__ FixScale det_scale(const float* __restrict__ maxn, int n) { return fix_scale(maxn[n], kDetBits); }

// max |x| per batch entry (over `per_n` floats) -> maxn[n] (zeroed by the caller); non-finite -> +inf
static __global__ void __launch_bounds__(kBlock) k_det_absmax(const float* __restrict__ x, float* __restrict__ maxn, int64_t per_n) {
  const int n = blockIdx.y;
  const float* p = x + (int64_t)n * per_n;
  float m = 0.f;
  bool bad = false;
  const int64_t stride = (int64_t)gridDim.x * kBlock * 4;
  for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4; i < per_n; i += stride) {
    float v[4];
    if (i + 4 <= per_n && ((uintptr_t)(p + i) & 15) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(p + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = i + j < per_n ? p[i + j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { m = fmaxf(m, fabsf(v[j])); bad = bad || !(fabsf(v[j]) <= 3.0e38f); }
  }
  if (bad) m = __int_as_float(0x7f800000);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  __shared__ float wm[kBlock / 64];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) m = fmaxf(m, wm[w]);
    atomicMax(reinterpret_cast<int*>(maxn) + n, __float_as_int(m));      // (non-negative floats order as their bit patterns)
  }
}

// grad_in = int64 image * max / 2^40 (fix_out; a non-finite maximum: 0 * inf = NaN, as the owner-computes scatters do)
static __global__ void __launch_bounds__(kBlock) k_det_convert(const long long* __restrict__ acc, const float* __restrict__ maxn,
                                                               float* __restrict__ gin, int64_t per_n) {
  const int n = blockIdx.y;
  const FixScale fs = det_scale(maxn, n);
  const long long* a = acc + (int64_t)n * per_n;
  float* g = gin + (int64_t)n * per_n;
  const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
  for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; i < per_n; i += stride) {
    if (i + 2 <= per_n) {
      const longlong2 q = *reinterpret_cast<const longlong2*>(a + i);
      g[i] = fix_out((float)q.x, fs);
      g[i + 1] = fix_out((float)q.y, fs);
    } else {
      g[i] = fix_out((float)a[i], fs);
    }
  }
}
// The same with a run-time width, for images whose cells could overflow at kDetBits (more than 2^22 deposits of the maximum).
// A copy, not a shared body: k_det_convert compiles to other instructions once its loop sits in a function of its own.
static __global__ void __launch_bounds__(kBlock) k_det_convert_bits(const long long* __restrict__ acc, const float* __restrict__ maxn,
                                                                    float* __restrict__ gin, int64_t per_n, int bits) {
  const int n = blockIdx.y;
  const FixScale fs = fix_scale(maxn[n], bits);
  const long long* a = acc + (int64_t)n * per_n;
  float* g = gin + (int64_t)n * per_n;
  const int64_t stride = (int64_t)gridDim.x * kBlock * 2;
  for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2; i < per_n; i += stride) {
    if (i + 2 <= per_n) {
      const longlong2 q = *reinterpret_cast<const longlong2*>(a + i);
      g[i] = fix_out((float)q.x, fs);
      g[i + 1] = fix_out((float)q.y, fs);
    } else {
      g[i] = fix_out((float)a[i], fs);
    }
  }
}

static inline void advchain_det_absmax_launch(const float* x, float* maxn, int64_t N, int64_t per_n, hipStream_t st) {
  int64_t nb = (per_n + kBlock * 16 - 1) / (kBlock * 16);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(k_det_absmax, dim3((unsigned)nb, (unsigned)N), dim3(kBlock), 0, st, x, maxn, per_n);
}
static inline void advchain_det_convert_launch(const unsigned long long* acc, const float* maxn, float* gin, int64_t N,
                                               int64_t per_n, int bits, hipStream_t st) {
  int64_t nb = (per_n + kBlock * 8 - 1) / (kBlock * 8);
  if (nb > 2048) nb = 2048;
  const dim3 g((unsigned)nb, (unsigned)N), b(kBlock);
  if (bits == kDetBits) hipLaunchKernelGGL(k_det_convert, g, b, 0, st, reinterpret_cast<const long long*>(acc), maxn, gin, per_n);
  else hipLaunchKernelGGL(k_det_convert_bits, g, b, 0, st, reinterpret_cast<const long long*>(acc), maxn, gin, per_n, bits);
}

}  // namespace advchain
