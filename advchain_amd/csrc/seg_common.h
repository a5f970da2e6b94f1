// What the supervised-loss sources share, each written once.  Included by seg_loss.hip, seg_dice.hip and seg_boundary.hip (never
// by loss_lp.hip: its own ld4 / st4 would be ambiguous with the ones here); includes plane_io.h, the typed plane accesses.
//   seg_loss.hip      uses the class weights, k_seg_finish and seg_dispatch (its cross entropy has lanes of VEC pixels, no tail)
//   seg_dice.hip      } a lane owns kVox consecutive voxels of which `cnt` exist: ld4 / st4 / ld4_labels / lane_count, the
//   seg_boundary.hip  } shape limits seg_voxels / seg_blocks / seg_shape_ok, seg_dispatch; boundary also launches k_seg_finish
#pragma once
#include <type_traits>

#include "common.h"
#include "plane_io.h"

namespace advchain {

constexpr int kVox = 4;                      // voxels per lane
constexpr int kTile = kBlock * kVox;         // voxels per workgroup

// the lane's voxels v0..v0+3 of one plane; `cnt` of them exist (VEC: 0 or 4), the others read as 0
template <typename ST, bool VEC>
__device__ __forceinline__ void ld4(const ST* __restrict__ p, int cnt, float (&x)[kVox]) {
#pragma unroll
  for (int q = 0; q < kVox; ++q) x[q] = 0.f;
  if constexpr (VEC) {
    if (cnt > 0) ld<ST, 4>(p, x);
  } else {
#pragma unroll
    for (int q = 0; q < kVox; ++q)
      if (q < cnt) x[q] = ld1<ST>(p + q);
  }
}

template <typename ST, bool VEC>
__device__ __forceinline__ void st4(ST* __restrict__ p, int cnt, const float (&x)[kVox]) {
  if constexpr (VEC) {
    if (cnt > 0) st<ST, 4>(p, x);
  } else {
#pragma unroll
    for (int q = 0; q < kVox; ++q)
      if (q < cnt) st1<ST>(p + q, x[q]);
  }
}

// labels of the lane's voxels; a voxel that does not exist reads as -100 (not counted)
template <bool VEC>
__device__ __forceinline__ void ld4_labels(const int64_t* __restrict__ p, int cnt, int64_t (&y)[kVox]) {
#pragma unroll
  for (int q = 0; q < kVox; ++q) y[q] = -100;
  if constexpr (VEC) {
    if (cnt > 0) ld_labels<4>(p, y);
  } else {
#pragma unroll
    for (int q = 0; q < kVox; ++q)
      if (q < cnt) y[q] = p[q];
  }
}

__device__ __forceinline__ int lane_count(int64_t V, int64_t v0) {
  const int64_t left = V - v0;
  return left <= 0 ? 0 : (left >= kVox ? kVox : (int)left);
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
// sum of the counted raw weights (classes first..K-1; no weights: 1 each), in class order (uniform)
__device__ __forceinline__ float counted_weight_sum(const float* __restrict__ weight, int first, int K) {
  float s = 0.f;
  for (int c = first; c < K; ++c) s += weight ? weight[c] : 1.f;
  return s;
}

namespace {
// value[0] = (sum of the nb partials, fixed order) / denom.  One workgroup.  (Internal to every source that launches it, as
// k_zero_fill of common.h is.)
__global__ void __launch_bounds__(kBlock) k_seg_finish(const float* __restrict__ partial, int64_t nb, float denom,
                                                       float* __restrict__ value) {
  __shared__ float smem[4];
  float s[1] = {0.f};
  for (int64_t i = threadIdx.x; i < nb; i += kBlock) s[0] += partial[i];
  block_sum<1>(s, smem);
  if (threadIdx.x == 0) value[0] = s[0] / denom;
}
}  // namespace

// ---- host ---------------------------------------------------------------------------------------------------------------
// voxels per entry of an (N, K, dims) loss, or -1 for a bad shape
inline int64_t seg_voxels(int ndim, const int64_t* dims) {
  if (!dims || (ndim != 2 && ndim != 3)) return -1;
  int64_t V = 1;
  for (int i = 0; i < ndim; ++i) {
    if (dims[i] < 1 || dims[i] > (1 << 24)) return -1;
    V *= dims[i];
  }
  return V <= ((int64_t)1 << 40) ? V : -1;
}
inline int64_t seg_blocks(int64_t V) { return (V + kTile - 1) / kTile; }
// (N K V bounded so that neither the element offsets nor the workspace size, at most 3 N K (V / 1024 + 1) + N + 3 N K + 3
// floats, can leave int64)
inline bool seg_shape_ok(int64_t N, int64_t K, int64_t V) {
  if (!(N >= 1 && N <= 65535 && K >= 1 && K <= 65535 && V >= 1 && seg_blocks(V) <= 0x7fffffff)) return false;
  return V <= (((int64_t)1 << 62) / 12) / (N * K);
}

// Run-time (logits_bf16, a, b) -> template arguments: calls f(type tag, bool tag, bool tag) with the storage type of the logits
// (tag.type: unsigned short / float) and a, b as std::true_type / std::false_type.  f is a generic lambda holding ONE launch
// statement; it is instantiated for all eight combinations, so every kernel the flags can select exists.
template <typename T> struct type_tag { using type = T; };
template <typename F>
void seg_dispatch(int logits_bf16, bool a, bool b, F&& f) {
  auto flags = [&](auto st) {
    if (a) { if (b) f(st, std::true_type{}, std::true_type{}); else f(st, std::true_type{}, std::false_type{}); }
    else { if (b) f(st, std::false_type{}, std::true_type{}); else f(st, std::false_type{}, std::false_type{}); }
  };
  if (logits_bf16) flags(type_tag<unsigned short>{}); else flags(type_tag<float>{});
}

}  // namespace advchain
