// Exact Euclidean distance transform of masks and signed distance maps of label maps, 2D and 3D, for gfx950:
//
//   advchain_edt                 <- common.loss.distance_transform_edt
//   advchain_signed_maps         <- common.loss.signed_distance_maps (and boundary_loss with a label target)
//   edt_label_fields             <- csrc/seg_surface.hip, csrc/seg_morph.hip (csrc/edt_fields.h): field 0 of every class through the
//                                   passes, not finished
//   edt_mask_fields              <- csrc/seg_morph.hip: the same passes from 8-bit masks (host code only: no kernel of its own)
//
// A field holds, per voxel, the squared distance to the nearest SEED of its line so far, or the sentinel "no seed yet".  It
// is separable: one pass per axis, each in place.
//   k_edt_rows   the contiguous axis.  One workgroup per row.  Every wave takes 64 voxels at a time and turns "is a member of
//                class k" into one 64-bit ballot per class: the row is read once and serves every class from registers.  The
//                ballots stay in LDS; the nearest seed to the left and to the right of a voxel is then a count of leading /
//                trailing zeros in its own ballot, or the carry of the nearest non-empty ballot on that side (one sweep from
//                each end of the row).
//   k_edt_axis   every further axis: f'(i) = min_j f(j) + (s (i - j))^2 along the line.  A workgroup stages TX consecutive x
//                by the WHOLE line in LDS (global accesses stay rows of consecutive x; TX is halved until the tile fits in
//                64 KiB, so a long line only narrows the tile, and further down to 16 x while it is above 16 KiB: more
//                workgroups per CU), then a thread scans outward from its i, four offsets per step, and stops when (s delta)^2
//                reaches the best value so far: exact, no stack, O(line) at worst, O(distance) where seeds are near; a tile
//                without a seed is not scanned.  A wave holds 64 (or TX) x of ONE i, so its LDS reads are consecutive
//                words: no bank conflicts.
// The last pass also finishes: square root (of the exact integer, in fp64, rounded once), +inf (transform) or 0 (signed maps)
// where the sentinel survived, and for the signed maps the sign -- there a voxel scans only the field that its own membership
// selects (inside class k: the distance to the nearest non-member, negative; outside: to the nearest member, positive).
//
// With unit spacing the fields are int32 squared distances: exact, so any tiling and any run gives the same bits.  The
// sentinel is 2^30 and the squared diagonal must stay below it, so sentinel + delta^2 < 2^31 cannot overflow.  With a spacing
// they are fp32, sentinel 1e30, and f + (s delta)^2 is evaluated without contraction (build.py).  No atomics, no memset, no
// host read-back: every word that is read was written by a kernel of the same call.  Labels are only COMPARED with class
// indices.
#include <math.h>
#include <stdio.h>

#include "common.h"
#include "edt_fields.h"

namespace advchain {
namespace {

constexpr int kEdtInf = 1 << 30;
constexpr float kEdtInfF = 1.0e30f;
constexpr int kEdtMaxRow = 32767;            // longest contiguous axis (2^15 - 1: its square stays below the sentinel)
constexpr int kEdtMaxChunks = 512;           // = ceil(kEdtMaxRow / 64)
constexpr int kEdtBallots = 2048;            // (class, chunk) ballots of a row that LDS holds at a time
constexpr int kEdtTileBytes = 65536;         // LDS of one k_edt_axis workgroup
constexpr int kEdtTilePrefer = 16384;        // ... and what it is narrowed to (not below 16 x): more workgroups per CU hide the
                                             // LDS round trips of the scan (profiles/r19/boundary/summary.md)
constexpr int kScan = 4;                     // offsets of the outward scan per stop test

enum { SRC_LABELS = 0, SRC_U8 = 1, SRC_I64 = 2, SRC_F32 = 3 };
enum { AXIS_PLAIN = 0, AXIS_FINISH = 1, AXIS_FINISH_SIGNED = 2 };

template <typename T> struct Sq;
template <> struct Sq<int> {
  static __device__ __forceinline__ int inf() { return kEdtInf; }
  static __device__ __forceinline__ int of(int d, float) { return d * d; }
  static __device__ __forceinline__ float root(int v) { return (float)sqrt((double)v); }    // correctly rounded
};
template <> struct Sq<float> {
  static __device__ __forceinline__ float inf() { return kEdtInfF; }
  static __device__ __forceinline__ float of(int d, float s) { const float sd = s * (float)d; return sd * sd; }
  static __device__ __forceinline__ float root(float v) { return sqrtf(v); }
};

// the class of a voxel: a label in [0, K) or -1 (no class); of a mask: 0 where it is nonzero (foreground), -1 where it is zero
__device__ __forceinline__ int class_at(const void* __restrict__ src, int kind, int64_t i, int K) {
  if (kind == SRC_LABELS) {
    const int64_t y = ((const int64_t*)src)[i];
    return (y >= 0 && y < (int64_t)K) ? (int)y : -1;
  }
  if (kind == SRC_U8) return ((const unsigned char*)src)[i] ? 0 : -1;
  if (kind == SRC_I64) return ((const int64_t*)src)[i] ? 0 : -1;
  return ((const float*)src)[i] != 0.f ? 0 : -1;
}

// Row b = (n, r) of the source; classes k0 .. k0 + kg - 1; fields f_first .. f_first + nf - 1 of each (0: seeds are the members,
// 1: the non-members).  out[((n K + k) nf + f - f_first) V + r W + x]
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_edt_rows(const void* __restrict__ src, int kind, T* __restrict__ out, int K, int nf, int f_first, int W, int64_t R, int k0,
           int kg, int chunks, float s) {
  __shared__ unsigned long long ballots[kEdtBallots];
  __shared__ unsigned long long exist[kEdtMaxChunks];
  __shared__ int right_carry[4][kEdtMaxChunks];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x, n = b / R, r = b - n * R, V = R * W;

  for (int c = wave; c < chunks; c += 4) {
    const int x = c * 64 + lane;
    const int cls = x < W ? class_at(src, kind, b * W + x, K) : -1;
    const unsigned long long e = __ballot(x < W);
    if (lane == 0) exist[c] = e;
    for (int kk = 0; kk < kg; ++kk) {
      const unsigned long long m = __ballot(cls == k0 + kk);
      if (lane == 0) ballots[kk * chunks + c] = m;
    }
  }
  __syncthreads();

  int* rc = right_carry[wave];
  for (int p = wave; p < kg * nf; p += 4) {
    const int kk = p / nf, f = f_first + (p - kk * nf);
    const unsigned long long* bm = ballots + kk * chunks;
    int carry = -1;
    for (int c = chunks - 1; c >= 0; --c) {            // every lane writes the same word and reads back its own write
      rc[c] = carry;
      const unsigned long long m = f ? (exist[c] & ~bm[c]) : bm[c];
      if (m) carry = c * 64 + __builtin_ctzll(m);
    }
    T* o = out + (((n * K + k0 + kk) * nf + (f - f_first)) * V + r * W);
    carry = -1;
    for (int c = 0; c < chunks; ++c) {
      const unsigned long long m = f ? (exist[c] & ~bm[c]) : bm[c];
      const int x = c * 64 + lane;
      const unsigned long long ml = m & (~0ull >> (63 - lane)), mr = m & (~0ull << lane);
      const int left = ml ? c * 64 + 63 - __builtin_clzll(ml) : carry;
      const int right = mr ? c * 64 + __builtin_ctzll(mr) : rc[c];
      int d = -1;
      if (left >= 0) d = x - left;
      if (right >= 0 && (d < 0 || right - x < d)) d = right - x;
      if (x < W) o[x] = d < 0 ? Sq<T>::inf() : Sq<T>::of(d, s);
      if (m) carry = c * 64 + 63 - __builtin_clzll(m);
    }
  }
}

// Lines of length L and stride I inside blocks of L I elements; Oz blocks per entry (V = Oz L I), NF fields per entry q.
// blockIdx.x = (q Oz + oz) tiles + tile of TX consecutive i.
template <typename T, int MODE>
__global__ void __launch_bounds__(kBlock)
k_edt_axis(T* g, const int64_t* __restrict__ labels, float* out, int K, int64_t Oz, int L, int64_t I, int TX, int64_t tiles,
           float s, int squared) {                        // (`out` may be `g` itself: the tile is complete before a word is written)
  extern __shared__ __align__(16) unsigned char edt_lds[];
  T* tile = reinterpret_cast<T*>(edt_lds);
  constexpr int NF = MODE == AXIS_FINISH_SIGNED ? 2 : 1;
  const int64_t b = blockIdx.x, it = b % tiles, rest = b / tiles, oz = rest % Oz, q = rest / Oz;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX, TY = kBlock / TX;
  const int64_t i = it * TX + tx, V = Oz * L * I, off = oz * L * I + i;
  const bool ok = i < I;

  // (a tile without a seed -- a class absent from the plane, or filling it -- has nothing to scan for: every value stays the
  // sentinel.  Without this test each of its voxels would walk the whole line.)
  bool seeded[NF];
  for (int f = 0; f < NF; ++f) {
    const T* gf = g + (q * NF + f) * V + off;
    int any = 0;
    for (int j = ty; j < L; j += TY) {
      const T v = ok ? gf[j * I] : Sq<T>::inf();
      tile[((int64_t)f * L + j) * TX + tx] = v;
      any |= v < Sq<T>::inf();
    }
    seeded[f] = __syncthreads_or(any) != 0;              // (also the barrier between the loads and the scans)
  }
  if (!ok) return;

  const int64_t n = q / K;
  const int k = (int)(q - n * K);
  for (int j = ty; j < L; j += TY) {
    bool inside = false;
    if constexpr (MODE == AXIS_FINISH_SIGNED) inside = labels[n * V + off + j * I] == (int64_t)k;
    const T* col = tile + (inside ? (int64_t)L * TX : 0) + tx;
    T best = col[j * TX];
    // kScan offsets per step: their 2 kScan LDS reads are in flight together (one at a time, the loop waits a round trip per
    // offset).  The stop test runs once per step; the offsets it lets through beyond the strict bound are candidates of the
    // same minimum, so the result does not change.  An offset past the line reads the line's end and is not used.
    const int reach = j > L - 1 - j ? j : L - 1 - j;
    for (int d0 = 1; d0 <= reach && seeded[inside ? NF - 1 : 0]; d0 += kScan) {
      if (!(Sq<T>::of(d0, s) < best)) break;
      T lo[kScan], hi[kScan];
#pragma unroll
      for (int u = 0; u < kScan; ++u) {
        const int a = j - d0 - u, b = j + d0 + u;
        lo[u] = col[(a < 0 ? 0 : a) * TX];
        hi[u] = col[(b > L - 1 ? L - 1 : b) * TX];
      }
#pragma unroll
      for (int u = 0; u < kScan; ++u) {
        const T d2 = Sq<T>::of(d0 + u, s);
        const T cl = j - d0 - u >= 0 ? lo[u] + d2 : Sq<T>::inf(), ch = j + d0 + u < L ? hi[u] + d2 : Sq<T>::inf();
        const T c = cl < ch ? cl : ch;
        best = c < best ? c : best;
      }
    }
    if constexpr (MODE == AXIS_PLAIN) {
      g[q * V + off + j * I] = best;
    } else if constexpr (MODE == AXIS_FINISH) {
      out[q * V + off + j * I] = best >= Sq<T>::inf() ? INFINITY : (squared ? (float)best : Sq<T>::root(best));
    } else {
      const float d = Sq<T>::root(best);
      out[q * V + off + j * I] = best >= Sq<T>::inf() ? 0.f : (inside ? -d : d);
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct EdtShape {
  int nd;
  int64_t d[3];          // D, H, W (D = 1 in 2D)
  int64_t V;
};

// 0: fine; ADVCHAIN_ERR_ARG: not a shape; ADVCHAIN_ERR_UNSUPPORTED: a shape the fields cannot hold
int edt_shape(int ndim, const int64_t* dims, int nf, EdtShape* sh) {
  if (!dims || (ndim != 2 && ndim != 3)) return ADVCHAIN_ERR_ARG;
  for (int a = 0; a < ndim; ++a)
    if (dims[a] < 1) return ADVCHAIN_ERR_ARG;
  sh->nd = ndim;
  sh->d[0] = ndim == 3 ? dims[0] : 1;
  sh->d[1] = dims[ndim - 2];
  sh->d[2] = dims[ndim - 1];
  double diag = 0.0;
  for (int a = 0; a < 3; ++a) {
    if (sh->d[a] > kEdtMaxRow) return ADVCHAIN_ERR_UNSUPPORTED;
    diag += (double)(sh->d[a] - 1) * (double)(sh->d[a] - 1);
  }
  if (!(diag < (double)kEdtInf)) return ADVCHAIN_ERR_UNSUPPORTED;
  for (int a = 0; a < 2; ++a)                                    // one x of a whole line (of every field) must fit in LDS
    if (sh->d[a] * nf * 4 > kEdtTileBytes) return ADVCHAIN_ERR_UNSUPPORTED;
  sh->V = sh->d[0] * sh->d[1] * sh->d[2];
  return ADVCHAIN_OK;
}

// entries * fields * V words, or -1
int64_t edt_words(int64_t entries, int nf, const EdtShape& sh) {
  if (entries < 1 || entries > ((int64_t)1 << 40)) return -1;
  if (sh.V > (((int64_t)1 << 60) / nf) / entries) return -1;
  return entries * nf * sh.V;
}

// s[a] per axis (D, H, W) from `sampling` (ndim host floats) -- false for a value that is not positive and finite or a
// physical diagonal whose square reaches the sentinel
bool edt_spacing(const float* sampling, const EdtShape& sh, float (&s)[3]) {
  s[0] = s[1] = s[2] = 1.f;
  if (!sampling) return true;
  double diag = 0.0;
  for (int a = 0; a < sh.nd; ++a) {
    const float v = sampling[a];
    if (!(v > 0.f && v <= 3.40282347e38f)) return false;
    s[3 - sh.nd + a] = v;
    const double e = (double)v * (double)(sh.d[3 - sh.nd + a] - 1);
    diag += e * e;
  }
  return diag < 1.0e29 && (double)s[0] * s[0] >= 1.0e-30 && (double)s[1] * s[1] >= 1.0e-30 && (double)s[2] * s[2] >= 1.0e-30;
}

template <typename T, int MODE>
int edt_axis(T* g, const int64_t* labels, float* out, int64_t Q, int K, int64_t Oz, int64_t L, int64_t I, float s, int squared,
             hipStream_t st) {
  constexpr int NF = MODE == AXIS_FINISH_SIGNED ? 2 : 1;
  int TX = 64;
  while (TX > 1 && (TX * L * NF * 4 > kEdtTileBytes || TX / 2 >= I)) TX >>= 1;
  while (TX > 16 && TX * L * NF * 4 > kEdtTilePrefer) TX >>= 1;
  const int64_t tiles = (I + TX - 1) / TX, blocks = Q * Oz * tiles;
  if (blocks > 0x7fffffff) {
    advchain_set_error_("edt: too many tiles for one launch");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL((k_edt_axis<T, MODE>), dim3((unsigned)blocks), dim3(kBlock), (size_t)(TX * L * NF * 4), st, g, labels, out, K,
                     Oz, (int)L, I, TX, tiles, s, squared);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

// the passes of one call: src -> fields (Q = N K entries of NF fields in `g`) -> out
template <typename T, bool SIGNED>
int edt_run(const void* src, int kind, T* g, float* out, int64_t N, int K, const EdtShape& sh, const float (&s)[3], int squared,
            hipStream_t st) {
  constexpr int NF = SIGNED ? 2 : 1;
  constexpr int LAST = SIGNED ? AXIS_FINISH_SIGNED : AXIS_FINISH;
  const int64_t D = sh.d[0], H = sh.d[1], W = sh.d[2], R = D * H, Q = N * K;
  if (N * R > 0x7fffffff) {
    advchain_set_error_("edt: too many rows for one launch");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  const int chunks = (int)((W + 63) / 64);
  const int group = kEdtBallots / chunks;
  for (int k0 = 0; k0 < K; k0 += group) {
    hipLaunchKernelGGL(k_edt_rows<T>, dim3((unsigned)(N * R)), dim3(kBlock), 0, st, src, kind, g, K, NF, SIGNED ? 0 : 1, (int)W, R,
                       k0, K - k0 < group ? K - k0 : group, chunks, s[2]);
    ADVCHAIN_LAUNCH_CHECK();
  }
  const int64_t* labels = SIGNED ? (const int64_t*)src : nullptr;
  if (sh.nd == 2) return edt_axis<T, LAST>(g, labels, out, Q, K, 1, H, W, s[1], squared, st);
  const int rc = edt_axis<T, AXIS_PLAIN>(g, nullptr, nullptr, Q * NF, 1, D, H, W, s[1], 0, st);
  if (rc != ADVCHAIN_OK) return rc;
  return edt_axis<T, LAST>(g, labels, out, Q, K, 1, D, H * W, s[0], squared, st);
}

// the passes without a finish: field 0 (seeds are the members) of every class, left as squared distances with the sentinel
template <typename T>
int edt_fields_run(const void* src, int kind, T* g, int64_t N, int K, const EdtShape& sh, const float (&s)[3], hipStream_t st) {
  const int64_t D = sh.d[0], H = sh.d[1], W = sh.d[2], R = D * H, Q = N * K;
  if (N * R > 0x7fffffff) {
    advchain_set_error_("edt: too many rows for one launch");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  const int chunks = (int)((W + 63) / 64);
  const int group = kEdtBallots / chunks;
  for (int k0 = 0; k0 < K; k0 += group) {
    hipLaunchKernelGGL(k_edt_rows<T>, dim3((unsigned)(N * R)), dim3(kBlock), 0, st, src, kind, g, K, 1, 0,
                       (int)W, R, k0, K - k0 < group ? K - k0 : group, chunks, s[2]);
    ADVCHAIN_LAUNCH_CHECK();
  }
  if (sh.nd == 2) return edt_axis<T, AXIS_PLAIN>(g, nullptr, nullptr, Q, 1, 1, H, W, s[1], 0, st);
  const int rc = edt_axis<T, AXIS_PLAIN>(g, nullptr, nullptr, Q, 1, D, H, W, s[1], 0, st);
  if (rc != ADVCHAIN_OK) return rc;
  return edt_axis<T, AXIS_PLAIN>(g, nullptr, nullptr, Q, 1, 1, D, H * W, s[0], 0, st);
}

}  // namespace

// ---- csrc/edt_fields.h -------------------------------------------------------------------------------------------------------
int64_t edt_label_fields_words(int64_t entries, int64_t K, int ndim, const int64_t* dims) {
  EdtShape sh;
  if (entries < 1 || K < 1 || K > 65535 || edt_shape(ndim, dims, 2, &sh) != ADVCHAIN_OK) return -1;
  if (entries > ((int64_t)1 << 40) / K) return -1;
  return edt_words(entries * K, 1, sh);
}

int edt_fields_check(const float* sampling, int64_t entries, int64_t K, int ndim, const int64_t* dims, const char* what,
                     int64_t (&d)[3], float (&s)[3]) {
  char msg[256];
  EdtShape sh;
  const int rc = edt_shape(ndim, dims, 2, &sh);
  if (rc == ADVCHAIN_ERR_ARG || entries < 1 || K < 1 || K > 65535) {
    snprintf(msg, sizeof(msg), "%s: bad pointer, N, K, ndim or dims", what);
    advchain_set_error_(msg);
    return ADVCHAIN_ERR_ARG;
  }
  if (rc != ADVCHAIN_OK || edt_label_fields_words(entries, K, ndim, dims) < 0) {
    snprintf(msg, sizeof(msg), "%s: shape too large for the distance fields (an axis or the squared diagonal)", what);
    advchain_set_error_(msg);
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  if (!edt_spacing(sampling, sh, s)) {
    snprintf(msg, sizeof(msg), "%s: sampling must be positive and finite (and the physical diagonal below 1e14)", what);
    advchain_set_error_(msg);
    return ADVCHAIN_ERR_ARG;
  }
  for (int a = 0; a < 3; ++a) d[a] = sh.d[a];
  return ADVCHAIN_OK;
}

static int edt_fields_from(const void* src, int kind, const float* sampling, void* fields, int64_t entries, int64_t K, int ndim,
                           const int64_t* dims, const char* what, hipStream_t st) {
  if (!src || !fields) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: bad pointer, N, K, ndim or dims", what);
    advchain_set_error_(msg);
    return ADVCHAIN_ERR_ARG;
  }
  EdtShape sh;
  float s[3];
  const int rc = edt_fields_check(sampling, entries, K, ndim, dims, what, sh.d, s);
  if (rc != ADVCHAIN_OK) return rc;
  sh.nd = ndim;
  sh.V = sh.d[0] * sh.d[1] * sh.d[2];
  if (sampling) return edt_fields_run<float>(src, kind, (float*)fields, entries, (int)K, sh, s, st);
  return edt_fields_run<int>(src, kind, (int*)fields, entries, (int)K, sh, s, st);
}

int edt_label_fields(const int64_t* labels, const float* sampling, void* fields, int64_t entries, int64_t K, int ndim,
                     const int64_t* dims, const char* what, hipStream_t st) {
  return edt_fields_from(labels, SRC_LABELS, sampling, fields, entries, K, ndim, dims, what, st);
}

int edt_mask_fields(const unsigned char* mask, const float* sampling, void* fields, int64_t entries, int ndim, const int64_t* dims,
                    const char* what, hipStream_t st) {
  return edt_fields_from(mask, SRC_U8, sampling, fields, entries, 1, ndim, dims, what, st);
}

}  // namespace advchain

using namespace advchain;

extern "C" {

int advchain_edt(const void* mask, int mask_kind, const float* sampling, int squared, float* out, int64_t B, int ndim,
                 const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(mask && out, "edt: null pointer");
  ADVCHAIN_CHECK_ARG(mask_kind >= SRC_U8 && mask_kind <= SRC_F32, "edt: mask kind is 1 (8-bit), 2 (int64) or 3 (fp32)");
  ADVCHAIN_CHECK_ARG(squared == 0 || squared == 1, "edt: squared is 0 or 1");
  EdtShape sh;
  const int rc = edt_shape(ndim, dims, 1, &sh);
  ADVCHAIN_CHECK_ARG(rc != ADVCHAIN_ERR_ARG, "edt: bad ndim or dims");
  if (rc != ADVCHAIN_OK || edt_words(B, 1, sh) < 0) {
    ADVCHAIN_CHECK_ARG(B >= 1, "edt: bad B");
    advchain_set_error_("edt: shape too large for the distance fields (an axis or the squared diagonal)");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  float s[3];
  ADVCHAIN_CHECK_ARG(edt_spacing(sampling, sh, s), "edt: sampling must be positive and finite (and the physical diagonal below 1e14)");
  // the field lives in `out` itself: a word is an int32 or fp32 squared distance until the last pass rewrites it
  if (sampling) return edt_run<float, false>(mask, mask_kind, out, out, B, 1, sh, s, squared, (hipStream_t)stream);
  return edt_run<int, false>(mask, mask_kind, reinterpret_cast<int*>(out), out, B, 1, sh, s, squared, (hipStream_t)stream);
}

int64_t advchain_signed_maps_workspace(int64_t N, int64_t K, int ndim, const int64_t* dims) {
  EdtShape sh;
  if (N < 1 || K < 1 || K > 65535 || edt_shape(ndim, dims, 2, &sh) != ADVCHAIN_OK) return -1;
  if (N > ((int64_t)1 << 40) / K) return -1;
  return edt_words(N * K, 2, sh);
}

int advchain_signed_maps(const int64_t* labels, const float* sampling, float* out, float* workspace, int64_t N, int64_t K,
                         int ndim, const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(labels && out && workspace, "signed_maps: null pointer");
  ADVCHAIN_CHECK_ARG(K >= 1 && K <= 65535, "signed_maps: K must be in 1..65535");
  ADVCHAIN_CHECK_ARG(N >= 1, "signed_maps: bad N");
  EdtShape sh;
  const int rc = edt_shape(ndim, dims, 2, &sh);
  ADVCHAIN_CHECK_ARG(rc != ADVCHAIN_ERR_ARG, "signed_maps: bad ndim or dims");
  if (rc != ADVCHAIN_OK || advchain_signed_maps_workspace(N, K, ndim, dims) < 0) {
    advchain_set_error_("signed_maps: shape too large for the distance fields (an axis or the squared diagonal)");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  float s[3];
  ADVCHAIN_CHECK_ARG(edt_spacing(sampling, sh, s), "signed_maps: sampling must be positive and finite (and the physical diagonal below 1e14)");
  if (sampling) return edt_run<float, true>(labels, SRC_LABELS, workspace, out, N, (int)K, sh, s, 0, (hipStream_t)stream);
  return edt_run<int, true>(labels, SRC_LABELS, reinterpret_cast<int*>(workspace), out, N, (int)K, sh, s, 0, (hipStream_t)stream);
}

}  // extern "C"
