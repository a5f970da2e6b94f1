// Confusion matrix and per-class overlap counts of a prediction against a label map, also straight from logits (not in the
// reference):
//   advchain_confusion        <- common.metrics.confusion_matrix   (target, pred) count matrix, rows = truth
//   advchain_overlap          <- common.metrics.overlap_metrics    |A|, |B|, |A n B| per class and the five quotients
//   advchain_overlap_scores   <- common.metrics.overlap_scores     the same quotients from a finished matrix
//
// One streaming pass, memory-bound: 16 bytes a voxel for two label maps, 4 K or 2 K + 8 bytes for logits.  A lane owns kVox
// consecutive voxels of an entry (seg_common.h: 16-byte loads where the pointers allow, the scalar form otherwise); the
// prediction is a label or the argmax over the K class planes, taken in a run-time loop with torch.argmax's rule on the CPU: the
// first maximal class wins, a NaN is larger than everything (so the first NaN wins), a row of -inf gives class 0.  bf16 words
// are widened to fp32, which is exact.  A label outside [0, K) is in no class: it maps to the extra index K of the table and is
// never used as an address.  A voxel whose TARGET equals ignore_index is left out of every count.
//
//   k_confusion_clear    the int64 counters (skipped when the call accumulates into the caller's)
//   k_confusion          a workgroup walks tiles of kTile voxels of one entry, grid-stride over at most kMaxBlocks workgroups per
//                        entry.  Per voxel slot the wave first groups equal keys -- the leader / ballot loop of seg_components.hip,
//                        at most kGroupRounds turns, whoever is left adds for itself -- so that one lane adds the group's count:
//                        in a real label map most of a wave hits the one background-background bin, which would serialise.
//                        The adds go to 32-bit counters in LDS -- matrix: (K + 1)^2 of them, key = t (K + 1) + p, up to K =
//                        kLdsMaxK (64 KB: two workgroups a CU); overlap: 3 K, up to K = kOverlapLdsMaxK -- whose nonzero words
//                        are flushed with 64-bit global adds at the end, or straight to the global counters above those limits.
//                        A workgroup sees at most kFlushTiles tiles (the grid grows beyond kMaxBlocks for entries that need it),
//                        fewer than 2^32 voxels, so no 32-bit counter can wrap.
//   k_matrix_overlap     overlap and counted from a finished matrix: column sum, row sum, diagonal; counted = the total
//   k_overlap_finish     the five quotients in fp64 from the integers, rounded to fp32 once, NaN for a zero denominator
//
// Integer atomics only, no memset, no host read-back: the same bits on every run, capturable on one stream.
#include <type_traits>

#include "advchain_hip.h"
#include "seg_common.h"

namespace advchain {
namespace {

typedef unsigned long long u64;

constexpr int kMaxBlocks = 128;                 // workgroups per entry (ops.CONFUSION_MAX_BLOCKS)
constexpr int64_t kFlushTiles = (int64_t)1 << 21;   // tiles a workgroup may see: 2^31 voxels, below the 2^32 of its counters
constexpr int kLdsMaxK = 127;                   // matrix in LDS: (K + 1)^2 words <= 64 KB (ops.CONFUSION_LDS_MAX_K)
constexpr int kMatrixMaxK = 1024;               // 8 MB of int64 per entry (ops.CONFUSION_MAX_K)
constexpr int kOverlapLdsMaxK = 2048;           // 3 K words <= 24 KB (ops.OVERLAP_LDS_MAX_K)
constexpr int kGroupRounds = 4;

enum { MODE_MATRIX = 0, MODE_OVERLAP = 1 };
enum { PRED_LABELS = 0, PRED_F32 = 1, PRED_BF16 = 2 };
enum { FLAG_REDUCE_BATCH = 1, FLAG_ACCUMULATE = 2 };

// the counters of one entry.  matrix: a (K,K), b pred_only (K), c target_only (K); overlap: a (K,3)
struct Sink {
  int64_t* a;
  int64_t* b;
  int64_t* c;
  int K;
};

// key -> its global counter; matrix keys are t (K + 1) + p with K standing for "no class" (both outside: no counter)
template <int MODE>
__device__ __forceinline__ int64_t* slot(const Sink& s, int key) {
  if constexpr (MODE == MODE_OVERLAP) {
    return s.a + key;
  } else {
    const int K1 = s.K + 1, t = key / K1, p = key - t * K1;
    if (t < s.K) return p < s.K ? s.a + (int64_t)t * s.K + p : s.c + t;
    return p < s.K ? s.b + p : nullptr;
  }
}

template <int MODE, bool LDS>
__device__ __forceinline__ void bump(unsigned* lds, const Sink& s, int key, int count) {
  if constexpr (LDS) {
    atomicAdd(lds + key, (unsigned)count);
  } else {
    int64_t* g = slot<MODE>(s, key);
    if (g) atomicAdd((u64*)g, (u64)count);
  }
}

// One add per group of equal keys of the wave (key < 0: the lane has nothing).  f(key, lanes of the group, those of them with
// `extra`) runs in the group's first lane; after kGroupRounds turns (a wave of many distinct keys) the lanes left add alone.
template <typename F>
__device__ __forceinline__ void wave_groups(int key, bool extra, int lane, F&& f) {
  u64 todo = __ballot(key >= 0);
  for (int round = 0; todo && round < kGroupRounds; ++round) {                          // one turn per key: todo loses bits
    const int first = __builtin_ctzll(todo);
    const int k1 = __shfl(key, first, 64);
    const u64 same = __ballot(key == k1), ex = __ballot(key == k1 && extra);
    if (lane == first) f(k1, __popcll(same), __popcll(ex));
    todo &= ~same;
  }
  if ((todo >> lane) & 1) f(key, 1, extra ? 1 : 0);
}

// torch.argmax on the CPU: strict first maximum, NaN above everything
__device__ __forceinline__ bool beats(float x, float best) { return x > best || (x != x && best == best); }

__global__ void __launch_bounds__(kBlock)
k_confusion_clear(int64_t* __restrict__ a, int64_t na, int64_t* __restrict__ b, int64_t nb, int64_t* __restrict__ c, int64_t nc,
                  int64_t* __restrict__ d, int64_t nd) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < na; i += stride) {
    a[i] = 0;
    if (i < nb) b[i] = 0;
    if (i < nc) c[i] = 0;
    if (i < nd) d[i] = 0;
  }
}

// PT: int64_t (a label map) or the storage type of the logits (N, K, V).  grid (workgroups per entry, N).
template <typename PT, bool VEC, int MODE, bool LDS>
__global__ void __launch_bounds__(kBlock)
k_confusion(const PT* __restrict__ pred, const int64_t* __restrict__ target, int64_t* __restrict__ labels_out, Sink sink,
            int64_t* __restrict__ counted, int64_t V, int64_t tiles, int has_ignore, int64_t ignore, int reduce_batch) {
  extern __shared__ unsigned lds[];
  const int K = sink.K, lane = threadIdx.x & 63;
  const int64_t n = blockIdx.y, e = reduce_batch ? 0 : n;
  const int words = MODE == MODE_MATRIX ? (K + 1) * (K + 1) : 3 * K;
  if constexpr (MODE == MODE_MATRIX) {
    sink.a += e * K * K; sink.b += e * K; sink.c += e * K;
  } else {
    sink.a += e * K * 3;
  }
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < words; i += kBlock) lds[i] = 0;
    __syncthreads();
  }
  unsigned seen = 0;                                                                    // counted voxels of this wave (uniform)
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t v0 = tile * kTile + (int64_t)threadIdx.x * kVox;
    const int cnt = lane_count(V, v0);
    int64_t y[kVox];
    ld4_labels<VEC>(target + n * V + v0, cnt, y);
    int p[kVox];
    if constexpr (std::is_same<PT, int64_t>::value) {
      int64_t z[kVox];
      ld4_labels<VEC>(pred + n * V + v0, cnt, z);
#pragma unroll
      for (int q = 0; q < kVox; ++q) p[q] = (z[q] >= 0 && z[q] < K) ? (int)z[q] : K;
    } else {
      const PT* plane = pred + n * K * V + v0;
      float best[kVox];
      ld4<PT, VEC>(plane, cnt, best);
#pragma unroll
      for (int q = 0; q < kVox; ++q) p[q] = 0;
#pragma unroll 4
      for (int c = 1; c < K; ++c) {
        float x[kVox];
        ld4<PT, VEC>(plane + (int64_t)c * V, cnt, x);
#pragma unroll
        for (int q = 0; q < kVox; ++q)
          if (beats(x[q], best[q])) { best[q] = x[q]; p[q] = c; }
      }
      if (labels_out) {
        int64_t* o = labels_out + n * V + v0;
        if constexpr (VEC) {
          if (cnt > 0) {
            longlong2 lo, hi;
            lo.x = p[0]; lo.y = p[1]; hi.x = p[2]; hi.y = p[3];
            *reinterpret_cast<longlong2*>(o) = lo;
            *reinterpret_cast<longlong2*>(o + 2) = hi;
          }
        } else {
#pragma unroll
          for (int q = 0; q < kVox; ++q)
            if (q < cnt) o[q] = p[q];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kVox; ++q) {
      const bool live = q < cnt && !(has_ignore && y[q] == ignore);
      const int t = (y[q] >= 0 && y[q] < K) ? (int)y[q] : K;
      seen += (unsigned)__popcll(__ballot(live));
      if constexpr (MODE == MODE_MATRIX) {
        wave_groups(live ? t * (K + 1) + p[q] : -1, false, lane,
                    [&](int key, int count, int) { bump<MODE, LDS>(lds, sink, key, count); });
      } else {                                                                          // counters of class k: 3 k + (|A|, |B|, |A n B|)
        wave_groups(live && p[q] < K ? p[q] : -1, t == p[q], lane, [&](int k, int count, int both) {
          bump<MODE, LDS>(lds, sink, 3 * k, count);
          if (both) bump<MODE, LDS>(lds, sink, 3 * k + 2, both);
        });
        wave_groups(live && t < K ? t : -1, false, lane,
                    [&](int k, int count, int) { bump<MODE, LDS>(lds, sink, 3 * k + 1, count); });
      }
    }
  }
  if (lane == 0 && seen) atomicAdd((u64*)(counted + e), (u64)seen);
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += kBlock) {
      const unsigned c = lds[i];
      if (c) {
        int64_t* g = slot<MODE>(sink, i);
        if (g) atomicAdd((u64*)g, (u64)c);
      }
    }
  }
}

// matrix (R,K,K) -> overlap (R,K,3) = column sum, row sum, diagonal; counted (R) = the total.  One workgroup per matrix.
__global__ void __launch_bounds__(kBlock)
k_matrix_overlap(const int64_t* __restrict__ matrix, int64_t* __restrict__ overlap, int64_t* __restrict__ counted, int K) {
  __shared__ u64 total;
  const int64_t r = blockIdx.x;
  const int64_t* m = matrix + r * K * K;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  u64 mine = 0;
  for (int k = threadIdx.x; k < K; k += kBlock) {
    int64_t col = 0, row = 0;
    for (int j = 0; j < K; ++j) {
      col += m[(int64_t)j * K + k];
      row += m[(int64_t)k * K + j];
    }
    int64_t* o = overlap + (r * K + k) * 3;
    o[0] = col; o[1] = row; o[2] = m[(int64_t)k * K + k];
    mine += (u64)row;
  }
  atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) counted[r] = (int64_t)total;
}

__device__ __forceinline__ float quotient(int64_t num, int64_t den) {
  return den == 0 ? (float)NAN : (float)((double)num / (double)den);
}

// TP = |A n B|, FP = |A| - TP, FN = |B| - TP, TN = counted - TP - FP - FN
__global__ void __launch_bounds__(kBlock)
k_overlap_finish(const int64_t* __restrict__ overlap, const int64_t* __restrict__ counted, float* __restrict__ dice,
                 float* __restrict__ iou, float* __restrict__ precision, float* __restrict__ recall,
                 float* __restrict__ specificity, int64_t R, int K) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= R * K) return;
  const int64_t a = overlap[i * 3], b = overlap[i * 3 + 1], tp = overlap[i * 3 + 2];
  const int64_t fp = a - tp, fn = b - tp, tn = counted[i / K] - tp - fp - fn;
  dice[i] = a + b == 0 ? (float)NAN : (float)(2.0 * (double)tp / (double)(a + b));
  iou[i] = quotient(tp, a + b - tp);
  precision[i] = quotient(tp, a);
  recall[i] = quotient(tp, b);
  specificity[i] = quotient(tn, tn + fp);
}

// (pred kind, vec, lds) -> template arguments, as seg_dispatch does: f holds ONE launch statement
template <typename F>
void confusion_dispatch(int pred_kind, bool vec, bool lds, F&& f) {
  if (pred_kind != PRED_LABELS) {
    seg_dispatch(pred_kind == PRED_BF16, vec, lds, f);
    return;
  }
  const type_tag<int64_t> st{};
  if (vec) { if (lds) f(st, std::true_type{}, std::true_type{}); else f(st, std::true_type{}, std::false_type{}); }
  else { if (lds) f(st, std::false_type{}, std::true_type{}); else f(st, std::false_type{}, std::false_type{}); }
}

int64_t confusion_grid(int64_t V) {
  const int64_t tiles = seg_blocks(V);
  const int64_t need = (tiles + kFlushTiles - 1) / kFlushTiles;
  const int64_t nb = tiles < kMaxBlocks ? tiles : kMaxBlocks;
  return nb > need ? nb : need;
}

template <int MODE>
void confusion_pass(const void* pred, int pred_kind, const int64_t* target, int64_t* labels_out, Sink sink, int64_t* counted,
                    int64_t N, int64_t V, int has_ignore, int64_t ignore, int flags, hipStream_t st) {
  const int K = sink.K;
  const bool lds = K <= (MODE == MODE_MATRIX ? kLdsMaxK : kOverlapLdsMaxK);
  const size_t bytes = lds ? sizeof(unsigned) * (MODE == MODE_MATRIX ? (size_t)(K + 1) * (K + 1) : (size_t)3 * K) : 0;
  const bool vec = V % 4 == 0 && aligned(pred, pred_kind == PRED_BF16 ? 8 : 16) && aligned(target, 16) && aligned(labels_out, 16);
  const dim3 grid((unsigned)confusion_grid(V), (unsigned)N);
  confusion_dispatch(pred_kind, vec, lds, [&](auto pt, auto ve, auto ld) {
    using PT = typename decltype(pt)::type;
    hipLaunchKernelGGL((k_confusion<PT, decltype(ve)::value, MODE, decltype(ld)::value>), grid, dim3(kBlock), bytes, st,
                       (const PT*)pred, target, labels_out, sink, counted, V, seg_blocks(V), has_ignore, ignore,
                       (flags & FLAG_REDUCE_BATCH) ? 1 : 0);
  });
}

void confusion_clear(int64_t* a, int64_t na, int64_t* b, int64_t nb, int64_t* c, int64_t nc, int64_t* d, int64_t nd,
                     hipStream_t st) {
  int64_t blocks = (na + kBlock - 1) / kBlock;                                           // (a is the longest of the four)
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_confusion_clear, dim3((unsigned)blocks), dim3(kBlock), 0, st, a, na, b, nb, c, nc, d, nd);
}

}  // namespace
}  // namespace advchain

using namespace advchain;

#define CONFUSION_COMMON_ARGS(what)                                                                                           \
  ADVCHAIN_CHECK_ARG(pred_kind >= PRED_LABELS && pred_kind <= PRED_BF16,                                                      \
                     what ": pred is a label map (0), fp32 logits (1) or bf16 logits (2)");                                   \
  ADVCHAIN_CHECK_ARG(pred_kind != PRED_LABELS || !labels_out, what ": labels_out needs logits");                              \
  ADVCHAIN_CHECK_ARG(((uintptr_t)pred & (pred_kind == PRED_BF16 ? 1 : pred_kind == PRED_F32 ? 3 : 7)) == 0 &&                 \
                         (((uintptr_t)target | (uintptr_t)labels_out) & 7) == 0,                                              \
                     what ": pred, target and labels_out must be aligned to their element size");                             \
  ADVCHAIN_CHECK_ARG((flags & ~(FLAG_REDUCE_BATCH | FLAG_ACCUMULATE)) == 0, what ": unknown flags");                          \
  ADVCHAIN_CHECK_ARG(has_ignore == 0 || has_ignore == 1, what ": has_ignore is 0 or 1");                                      \
  const int64_t V = seg_voxels(ndim, dims);                                                                                   \
  ADVCHAIN_CHECK_ARG(V > 0 && seg_shape_ok(N, K, V), what ": bad N, ndim or dims")

extern "C" {

int64_t advchain_confusion_limit(int what) {
  switch (what) {
    case 0: return kTile;
    case 1: return kMaxBlocks;
    case 2: return kLdsMaxK;
    case 3: return kMatrixMaxK;
    case 4: return kOverlapLdsMaxK;
    default: return -1;
  }
}

int advchain_confusion(const void* pred, int pred_kind, const int64_t* target, int64_t* labels_out, int64_t* matrix,
                       int64_t* pred_only, int64_t* target_only, int64_t* counted, int64_t N, int64_t K, int ndim,
                       const int64_t* dims, int has_ignore, int64_t ignore_index, int flags, void* stream) {
  ADVCHAIN_CHECK_ARG(pred && target && matrix && pred_only && target_only && counted, "confusion: null pointer");
  ADVCHAIN_CHECK_ARG((((uintptr_t)matrix | (uintptr_t)pred_only | (uintptr_t)target_only | (uintptr_t)counted) & 7) == 0,
                     "confusion: the outputs must be 8-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= kMatrixMaxK, "confusion: K must be in 1..1024 (advchain_overlap takes up to 65535)");
  CONFUSION_COMMON_ARGS("confusion");
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = (flags & FLAG_REDUCE_BATCH) ? 1 : N;
  if (!(flags & FLAG_ACCUMULATE)) {
    confusion_clear(matrix, R * K * K, pred_only, R * K, target_only, R * K, counted, R, st);
    ADVCHAIN_LAUNCH_CHECK();
  }
  const Sink sink = {matrix, pred_only, target_only, (int)K};
  confusion_pass<MODE_MATRIX>(pred, pred_kind, target, labels_out, sink, counted, N, V, has_ignore, ignore_index, flags, st);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_overlap(const void* pred, int pred_kind, const int64_t* target, int64_t* labels_out, int64_t* overlap,
                     int64_t* counted, float* dice, float* iou, float* precision, float* recall, float* specificity, int64_t N,
                     int64_t K, int ndim, const int64_t* dims, int has_ignore, int64_t ignore_index, int flags, void* stream) {
  ADVCHAIN_CHECK_ARG(pred && target && overlap && counted && dice && iou && precision && recall && specificity,
                     "overlap: null pointer");
  ADVCHAIN_CHECK_ARG((((uintptr_t)overlap | (uintptr_t)counted) & 7) == 0, "overlap: overlap and counted must be 8-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "overlap: K must be in 1..65535");
  CONFUSION_COMMON_ARGS("overlap");
  ADVCHAIN_CHECK_ARG(!(flags & FLAG_ACCUMULATE), "overlap: the counters are always cleared");
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = (flags & FLAG_REDUCE_BATCH) ? 1 : N;
  confusion_clear(overlap, R * K * 3, counted, R, nullptr, 0, nullptr, 0, st);
  ADVCHAIN_LAUNCH_CHECK();
  const Sink sink = {overlap, nullptr, nullptr, (int)K};
  confusion_pass<MODE_OVERLAP>(pred, pred_kind, target, labels_out, sink, counted, N, V, has_ignore, ignore_index, flags, st);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_overlap_finish, dim3((unsigned)((R * K + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     (const int64_t*)overlap, (const int64_t*)counted, dice, iou, precision, recall, specificity, R, (int)K);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

int advchain_overlap_scores(const int64_t* matrix, int64_t* overlap, int64_t* counted, float* dice, float* iou, float* precision,
                            float* recall, float* specificity, int64_t R, int64_t K, void* stream) {
  ADVCHAIN_CHECK_ARG(matrix && overlap && counted && dice && iou && precision && recall && specificity,
                     "overlap_scores: null pointer");
  ADVCHAIN_CHECK_ARG((((uintptr_t)matrix | (uintptr_t)overlap | (uintptr_t)counted) & 7) == 0,
                     "overlap_scores: matrix, overlap and counted must be 8-byte aligned");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "overlap_scores: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(R >= 1 && R <= 0x7fffffff && R <= ((int64_t)1 << 39) / (K * K), "overlap_scores: bad number of matrices");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_matrix_overlap, dim3((unsigned)R), dim3(kBlock), 0, st, matrix, overlap, counted, (int)K);
  ADVCHAIN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_overlap_finish, dim3((unsigned)((R * K + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     (const int64_t*)overlap, (const int64_t*)counted, dice, iou, precision, recall, specificity, R, (int)K);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // extern "C"
