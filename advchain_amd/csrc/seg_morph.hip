// Erosion, dilation, opening and closing of label maps with a Euclidean ball, 2D and 3D, for gfx950:
//
//   advchain_morph               <- common.postprocess.erosion / dilation / opening / closing
//
// Morphology with a ball of radius r is a threshold at r^2 on exact squared-distance fields (csrc/edt.hip).  Two things make it
// cheaper than the transform:
//   * the ball bounds every scan at cap = ceil(r / spacing) offsets of the axis: no voxel walks a whole line;
//   * erosion and dilation of all K classes need ONE field per voxel, not K:
//       erosion    e(v) = squared distance to the nearest in-image voxel whose label differs from labels[v].  Separable with a
//                  label compare inside the scan: along a line the candidate at j' for a voxel at j of class k is
//                  g(j') + (s (j - j'))^2 with g(j') = e(j') where labels[j'] == k and 0 where it differs -- a voxel of another
//                  label is a seed whatever its own field says.  Keep iff e(v) > r^2.
//       dilation   the key (squared distance, class) of the nearest class voxel, minimised lexicographically: nearest wins, among
//                  equally near the smaller class.  A class voxel seeds (0, its class); along a line the candidate is
//                  key(j') + ((s (j - j'))^2, 0).  Two 32-bit planes.
//     k_morph_rows   the contiguous axis, one workgroup per row.  One 64-bit ballot per 64 voxels -- "differs from its left
//                    neighbour" (erosion: it serves every class) or "is a class voxel" (dilation) -- kept in LDS; the nearest set
//                    bit on either side is a count of leading / trailing zeros or the carry of the nearest non-empty ballot.
//     k_morph_axis   every further axis.  A workgroup stages TX consecutive x by the whole line, field and class key, in LDS
//                    (TX <= 32, halved until the tile fits: every multiple of 64 voxels along x is a seam of both kernels) and a
//                    thread scans outward from its voxel, at most cap offsets, stopping where (s delta)^2 passes its best value.
//                    The last pass writes the label or `background` directly: no field leaves the call.
//   * opening and closing need per-class fields in their second stage (a voxel of another class says nothing about class k
//     there); these come from edt_label_fields / edt_mask_fields (csrc/edt_fields.h), whose column passes scan whole lines:
//       opening    the erosion above writes the eroded map with the classes renumbered without `background` (-1: no class);
//                  its member fields; k_morph_open reads field[labels[v]](v) <= r^2.
//       closing    the member fields F_k of the renumbered map; k_morph_mask marks F_k > r^2; the fields G_k of those marks
//                  overwrite F_k; k_morph_claim counts the classes with G_k(v) > r^2 at a background voxel: exactly one claims it.
//     The field of k == background is never computed.
//
// With unit spacing the fields are int32 and exact; with a sampling fp32, evaluated without contraction (build.py) exactly as
// edt.hip does.  A position outside the image is nothing: no seed for either field.  No atomics, no memset, no host read-back;
// every word read was written by a kernel of the same call.  Labels are only compared.
#include <math.h>
#include <stdio.h>

#include "advchain_hip.h"
#include "common.h"
#include "edt_fields.h"

namespace advchain {
namespace {

constexpr int kMorphMaxChunks = 512;         // = ceil(32767 / 64): the longest row of the distance fields
constexpr int kMorphTileX = 32;              // widest k_morph_axis tile (ops.MORPH_TILE: both kernels have a seam every 64 x)
constexpr int kMorphTileBytes = 65536;       // LDS of one k_morph_axis workgroup
constexpr int kMorphTilePrefer = 16384;      // ... and what it is narrowed to, not below 16 x (edt.hip: more workgroups per CU)

enum { MORPH_ERODE = 0, MORPH_DILATE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3 };

template <typename T> struct Msq;
template <> struct Msq<int> {
  static __device__ __forceinline__ int inf() { return kEdtFieldInf; }
  static __device__ __forceinline__ int of(int d, float) { return d * d; }
};
template <> struct Msq<float> {
  static __device__ __forceinline__ float inf() { return kEdtFieldInfF; }
  static __device__ __forceinline__ float of(int d, float s) { const float sd = s * (float)d; return sd * sd; }
};

// What the passes need of a label.  K classes, `skip` = background where it lies in [0, K), else -1.
struct Classes {
  int K, skip;
  int64_t background;
  // a label in [0, K) or -1
  __device__ __forceinline__ int key(int64_t y) const { return (y >= 0 && y < (int64_t)K) ? (int)y : -1; }
  // key k is that of a class voxel: in [0, K) and not the background
  __device__ __forceinline__ bool is_class(int k) const { return k >= 0 && k != skip; }
  // the classes numbered without the background, and back
  __device__ __forceinline__ int compact(int k) const { return k - ((skip >= 0 && k > skip) ? 1 : 0); }
  __device__ __forceinline__ int expand(int c) const { return c + ((skip >= 0 && c >= skip) ? 1 : 0); }
};

// Row b of the map.  ERODE: f[x] = squared distance along the row to the nearest voxel whose key differs from that of x.
// DILATE: (f, cls)[x] = the key of the nearest class voxel of the row.
template <typename T, int OP>
__global__ void __launch_bounds__(kBlock)
k_morph_rows(const int64_t* __restrict__ labels, T* __restrict__ f, int* __restrict__ cls, Classes C, int W, int chunks, float s) {
  __shared__ unsigned long long bits[kMorphMaxChunks];
  __shared__ int left_carry[kMorphMaxChunks], right_carry[kMorphMaxChunks];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * W;
  const int64_t* row = labels + base;

  for (int c = wave; c < chunks; c += 4) {
    const int x = c * 64 + lane;
    bool bit = false;
    if (x < W) {
      const int k = C.key(row[x]);
      if constexpr (OP == MORPH_ERODE) bit = x > 0 && k != C.key(row[x - 1]);      // x starts a run
      else bit = C.is_class(k);
    }
    const unsigned long long m = __ballot(bit);
    if (lane == 0) bits[c] = m;
  }
  __syncthreads();
  if (wave == 0) {                                       // every lane writes the same words
    int carry = -1;
    for (int c = chunks - 1; c >= 0; --c) {
      right_carry[c] = carry;
      const unsigned long long m = bits[c];
      if (m) carry = c * 64 + __builtin_ctzll(m);
    }
    carry = -1;
    for (int c = 0; c < chunks; ++c) {
      left_carry[c] = carry;
      const unsigned long long m = bits[c];
      if (m) carry = c * 64 + 63 - __builtin_clzll(m);
    }
  }
  __syncthreads();

  for (int c = wave; c < chunks; c += 4) {
    const int x = c * 64 + lane;
    const unsigned long long m = bits[c];
    const unsigned long long le = m & (~0ull >> (63 - lane)), ge = m & (~0ull << lane);       // set bits at or below / above x
    if constexpr (OP == MORPH_ERODE) {
      const unsigned long long gt = ge & ~(1ull << lane);
      const int p = le ? c * 64 + 63 - __builtin_clzll(le) : left_carry[c];        // the start of the run of x (>= 1), or -1
      const int q = gt ? c * 64 + __builtin_ctzll(gt) : right_carry[c];            // the start of the next run, or -1
      int d = -1;
      if (p >= 0) d = x - p + 1;
      if (q >= 0 && (d < 0 || q - x < d)) d = q - x;
      if (x < W) f[base + x] = d < 0 ? Msq<T>::inf() : Msq<T>::of(d, s);
    } else {
      const int l = le ? c * 64 + 63 - __builtin_clzll(le) : left_carry[c];
      const int r = ge ? c * 64 + __builtin_ctzll(ge) : right_carry[c];
      if (x < W) {
        int d = -1, k = 0;
        if (l >= 0) {
          d = x - l;
          k = C.key(row[l]);
        }
        if (r >= 0) {
          const int dr = r - x, kr = C.key(row[r]);
          if (d < 0 || dr < d || (dr == d && kr < k)) {
            d = dr;
            k = kr;
          }
        }
        f[base + x] = d < 0 ? Msq<T>::inf() : Msq<T>::of(d, s);
        cls[base + x] = k;
      }
    }
  }
}

// Lines of length L and stride I inside blocks of L I elements; Oz blocks per entry (V = Oz L I).
// blockIdx.x = (n Oz + oz) tiles + tile of TX consecutive i.  LAST: `out` gets the result of the operation (ERODE with
// `renumber`: the eroded map with compact classes, -1 where there is no class voxel); otherwise the planes are updated in place
// (a workgroup reads and writes its own columns only, and the tile is complete before a word is written).
template <typename T, int OP, bool LAST>
__global__ void __launch_bounds__(kBlock)
k_morph_axis(T* f, int* cls, const int64_t* __restrict__ labels, int64_t* __restrict__ out, Classes C, int64_t Oz, int L, int64_t I,
             int TX, int64_t tiles, float s, int cap, T r2, int renumber) {
  extern __shared__ __align__(16) unsigned char morph_lds[];
  T* tf = reinterpret_cast<T*>(morph_lds);
  int* tk = reinterpret_cast<int*>(morph_lds) + (int64_t)L * TX;
  const int64_t b = blockIdx.x, it = b % tiles, rest = b / tiles, oz = rest % Oz, n = rest / Oz;
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX, TY = kBlock / TX;
  const int64_t i = it * TX + tx, V = Oz * L * I, base = n * V + oz * L * I + i;
  const bool ok = i < I;

  for (int j = ty; j < L; j += TY) {
    T v = Msq<T>::inf();
    int k = -1;
    if (ok) {
      v = f[base + j * I];
      if constexpr (OP == MORPH_ERODE) k = C.key(labels[base + j * I]);
      else k = cls[base + j * I];
    }
    tf[j * TX + tx] = v;
    tk[j * TX + tx] = k;
  }
  __syncthreads();
  if (!ok) return;

  const T* cf = tf + tx;
  const int* ck = tk + tx;
  for (int j = ty; j < L; j += TY) {
    const int64_t at = base + j * I;
    T best = cf[j * TX];
    int k = ck[j * TX];
    const int reach = j > L - 1 - j ? j : L - 1 - j, lim = reach < cap ? reach : cap;
    if constexpr (OP == MORPH_ERODE) {
      const bool cv = C.is_class(k);
      if (cv) {
        for (int d = 1; d <= lim; ++d) {
          const T d2 = Msq<T>::of(d, s);
          if (!(d2 < best)) break;                      // a candidate at this offset or beyond is at least d2
          const int a = j - d, e = j + d;
          if (a >= 0) {
            const T c = (ck[a * TX] == k ? cf[a * TX] : (T)0) + d2;
            best = c < best ? c : best;
          }
          if (e < L) {
            const T c = (ck[e * TX] == k ? cf[e * TX] : (T)0) + d2;
            best = c < best ? c : best;
          }
        }
      }
      if constexpr (LAST) {
        const bool keep = best > r2;
        if (renumber) out[at] = (cv && keep) ? (int64_t)C.compact(k) : (int64_t)-1;
        else out[at] = (cv && !keep) ? C.background : labels[at];
      } else {
        if (cv) f[at] = best;
      }
    } else {
      for (int d = 1; d <= lim; ++d) {
        const T d2 = Msq<T>::of(d, s);
        if (d2 > best) break;                           // (an equal distance may still bring a smaller class)
        const int a = j - d, e = j + d;
        if (a >= 0) {
          const T fa = cf[a * TX];
          const int ka = ck[a * TX];
          const T c = fa + d2;
          if (fa < Msq<T>::inf() && (c < best || (c == best && ka < k))) {
            best = c;
            k = ka;
          }
        }
        if (e < L) {
          const T fe = cf[e * TX];
          const int ke = ck[e * TX];
          const T c = fe + d2;
          if (fe < Msq<T>::inf() && (c < best || (c == best && ke < k))) {
            best = c;
            k = ke;
          }
        }
      }
      if constexpr (LAST) {
        const int64_t y = labels[at];
        out[at] = (y == C.background && best <= r2) ? (int64_t)k : y;
      } else {
        f[at] = best;
        cls[at] = k;
      }
    }
  }
}

// out = labels (renumber 0), or the map with compact classes and -1 where there is no class voxel (renumber 1)
__global__ void __launch_bounds__(kBlock)
k_morph_copy(const int64_t* __restrict__ labels, int64_t* __restrict__ out, Classes C, int64_t total, int renumber) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < total; v += stride) {
    const int64_t y = labels[v];
    const int k = C.key(y);
    out[v] = renumber ? (C.is_class(k) ? (int64_t)C.compact(k) : (int64_t)-1) : y;
  }
}

// opening: a class voxel farther than the ball from its class's eroded set becomes background.  fields (N, Kc, V)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_morph_open(const int64_t* __restrict__ labels, const T* __restrict__ fields, int64_t* __restrict__ out, Classes C, int Kc, int64_t V,
             int64_t total, T r2) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < total; v += stride) {
    const int64_t y = labels[v], n = v / V;
    const int k = C.key(y);
    int64_t o = y;
    if (C.is_class(k) && !(fields[(n * Kc + C.compact(k)) * V + (v - n * V)] <= r2)) o = C.background;
    out[v] = o;
  }
}

// closing: mask = F > r^2 (the voxels outside the dilated class: the seeds of the second stage)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_morph_mask(const T* __restrict__ fields, unsigned char* __restrict__ mask, int64_t total, T r2) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < total; v += stride) mask[v] = fields[v] > r2 ? 1 : 0;
}

// closing: a background voxel farther than the ball from every voxel outside D_k lies in C_k; exactly one such class claims it
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_morph_claim(const int64_t* __restrict__ labels, const T* __restrict__ fields, int64_t* __restrict__ out, Classes C, int Kc, int64_t V,
              int64_t total, T r2) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < total; v += stride) {
    const int64_t y = labels[v], n = v / V;
    int64_t o = y;
    if (y == C.background) {
      const T* g = fields + n * Kc * V + (v - n * V);
      int claims = 0, who = 0;
      for (int c = 0; c < Kc; ++c) {
        if (g[c * V] > r2) {
          ++claims;
          who = c;
        }
      }
      if (claims == 1) o = (int64_t)C.expand(who);
    }
    out[v] = o;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct MorphShape {
  int nd;
  int64_t N, D, H, W, V;
  float s[3];
};

int flat_blocks(int64_t total) {
  const int64_t b = (total + kBlock - 1) / kBlock;
  return (int)(b > 16384 ? 16384 : b);
}

template <typename T, int OP, bool LAST>
int morph_axis(T* f, int* cls, const int64_t* labels, int64_t* out, const Classes& C, int64_t N, int64_t Oz, int64_t L, int64_t I,
               float s, int cap, T r2, int renumber, hipStream_t st) {
  int TX = kMorphTileX;
  while (TX > 1 && (TX * L * 8 > kMorphTileBytes || TX / 2 >= I)) TX >>= 1;
  while (TX > 16 && TX * L * 8 > kMorphTilePrefer) TX >>= 1;
  const int64_t tiles = (I + TX - 1) / TX, blocks = N * Oz * tiles;
  if (blocks > 0x7fffffff) {
    advchain_set_error_("morph: too many tiles for one launch");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL((k_morph_axis<T, OP, LAST>), dim3((unsigned)blocks), dim3(kBlock), (size_t)(TX * L * 8), st, f, cls, labels, out, C,
                     Oz, (int)L, I, TX, tiles, s, cap, r2, renumber);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

// the one-field passes of erosion or dilation: labels -> out
template <typename T, int OP>
int morph_one_field(const int64_t* labels, T* f, int* cls, int64_t* out, const Classes& C, const MorphShape& sh, const int (&cap)[3],
                    T r2, int renumber, hipStream_t st) {
  const int64_t R = sh.D * sh.H;
  if (sh.N * R > 0x7fffffff) {
    advchain_set_error_("morph: too many rows for one launch");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL((k_morph_rows<T, OP>), dim3((unsigned)(sh.N * R)), dim3(kBlock), 0, st, labels, f, cls, C, (int)sh.W,
                     (int)((sh.W + 63) / 64), sh.s[2]);
  ADVCHAIN_LAUNCH_CHECK();
  if (sh.nd == 2) return morph_axis<T, OP, true>(f, cls, labels, out, C, sh.N, 1, sh.H, sh.W, sh.s[1], cap[1], r2, renumber, st);
  const int rc = morph_axis<T, OP, false>(f, cls, labels, out, C, sh.N, sh.D, sh.H, sh.W, sh.s[1], cap[1], r2, 0, st);
  if (rc != ADVCHAIN_OK) return rc;
  return morph_axis<T, OP, true>(f, cls, labels, out, C, sh.N, 1, sh.D, sh.H * sh.W, sh.s[0], cap[0], r2, renumber, st);
}

template <typename T>
int morph_run(const int64_t* labels, const float* sampling, int op, int64_t* out, void* workspace, const Classes& C, int Kc,
              const MorphShape& sh, const int (&cap)[3], T r2, int ndim, const int64_t* dims, hipStream_t st) {
  const int64_t total = sh.N * sh.V;
  T* words = reinterpret_cast<T*>(workspace);
  if (op == MORPH_ERODE) return morph_one_field<T, MORPH_ERODE>(labels, words, nullptr, out, C, sh, cap, r2, 0, st);
  if (op == MORPH_DILATE)
    return morph_one_field<T, MORPH_DILATE>(labels, words, reinterpret_cast<int*>(words + total), out, C, sh, cap, r2, 0, st);

  // [compact map: 2 N V words][fields: N Kc V][closing's marks: N Kc V bytes]
  int64_t* map = reinterpret_cast<int64_t*>(workspace);
  T* fields = words + 2 * total;
  const int64_t all = total * Kc;
  if (op == MORPH_OPEN) {
    // (the erosion field lies where the member fields go: it is dead once the eroded map is written)
    int rc = morph_one_field<T, MORPH_ERODE>(labels, fields, nullptr, map, C, sh, cap, r2, 1, st);
    if (rc != ADVCHAIN_OK) return rc;
    rc = edt_label_fields(map, sampling, fields, sh.N, Kc, ndim, dims, "morph", st);
    if (rc != ADVCHAIN_OK) return rc;
    hipLaunchKernelGGL(k_morph_open<T>, dim3(flat_blocks(total)), dim3(kBlock), 0, st, labels, (const T*)fields, out, C, Kc, sh.V, total,
                       r2);
    ADVCHAIN_LAUNCH_CHECK();
    return ADVCHAIN_OK;
  }
  unsigned char* mask = reinterpret_cast<unsigned char*>(fields + all);
  hipLaunchKernelGGL(k_morph_copy, dim3(flat_blocks(total)), dim3(kBlock), 0, st, labels, map, C, total, 1);
  ADVCHAIN_LAUNCH_CHECK();
  int rc = edt_label_fields(map, sampling, fields, sh.N, Kc, ndim, dims, "morph", st);
  if (rc != ADVCHAIN_OK) return rc;
  hipLaunchKernelGGL(k_morph_mask<T>, dim3(flat_blocks(all)), dim3(kBlock), 0, st, (const T*)fields, mask, all, r2);
  ADVCHAIN_LAUNCH_CHECK();
  rc = edt_mask_fields(mask, sampling, fields, sh.N * Kc, ndim, dims, "morph", st);
  if (rc != ADVCHAIN_OK) return rc;
  hipLaunchKernelGGL(k_morph_claim<T>, dim3(flat_blocks(total)), dim3(kBlock), 0, st, labels, (const T*)fields, out, C, Kc, sh.V, total,
                     r2);
  ADVCHAIN_LAUNCH_CHECK();
  return ADVCHAIN_OK;
}

}  // namespace
}  // namespace advchain

using namespace advchain;

extern "C" {

int64_t advchain_morph_workspace(int op, int64_t N, int64_t K, int ndim, const int64_t* dims) {
  if (op < MORPH_ERODE || op > MORPH_CLOSE) return -1;
  if (advchain_signed_maps_workspace(N, K, ndim, dims) < 0) return -1;          // the shapes and sizes of the distance fields
  int64_t V = 1;
  for (int a = 0; a < ndim; ++a) V *= dims[a];
  const int64_t total = N * V;                                                // (2 N K V fits: checked above)
  if (op == MORPH_ERODE) return total;
  if (op == MORPH_DILATE) return 2 * total;
  if (op == MORPH_OPEN) return 2 * total + total * K;
  return 2 * total + total * K + (total * K + 3) / 4;
}

int advchain_morph(const int64_t* labels, const float* sampling, double radius, int op, int64_t* out, void* workspace, int64_t N,
                   int64_t K, int64_t background, int ndim, const int64_t* dims, void* stream) {
  ADVCHAIN_CHECK_ARG(labels && out && workspace && dims, "morph: null pointer");
  ADVCHAIN_CHECK_ARG(op >= MORPH_ERODE && op <= MORPH_CLOSE, "morph: op is 0 (erosion), 1 (dilation), 2 (opening) or 3 (closing)");
  ADVCHAIN_CHECK_ARG(radius >= 0.0 && radius <= 1.79769313486231570e308, "morph: radius must be finite and not negative");
  ADVCHAIN_CHECK_ARG(out != labels, "morph: out must not be the input");
  MorphShape sh;
  int64_t d[3];
  const int rc = edt_fields_check(sampling, N, K, ndim, dims, "morph", d, sh.s);
  if (rc != ADVCHAIN_OK) return rc;
  if (advchain_morph_workspace(op, N, K, ndim, dims) < 0) {
    advchain_set_error_("morph: shape too large for the distance fields (an axis or the squared diagonal)");
    return ADVCHAIN_ERR_UNSUPPORTED;
  }
  sh.nd = ndim;
  sh.N = N;
  sh.D = d[0];
  sh.H = d[1];
  sh.W = d[2];
  sh.V = d[0] * d[1] * d[2];
  Classes C;
  C.K = (int)K;
  C.skip = (background >= 0 && background < K) ? (int)background : -1;
  C.background = background;
  const int Kc = (int)K - (C.skip >= 0 ? 1 : 0);
  hipStream_t st = (hipStream_t)stream;

  // the ball: squared radius and offsets per axis.  Unit spacing: the integer test |o|^2 <= floor(radius^2), capped below the
  // sentinel.  With a sampling: fp32 fields against radius^2 rounded to fp32 (below the sentinel: no physical diagonal reaches
  // 1e29); one offset more than radius / spacing, so that rounding cannot drop a candidate.
  const double r2d = radius * radius;
  const int R2 = r2d >= (double)(kEdtFieldInf - 1) ? kEdtFieldInf - 1 : (int)floor(r2d);
  const float r2f = r2d >= 1.0e29 ? 1.0e29f : (float)r2d;
  int cap[3];
  bool origin_only = true;
  for (int a = 0; a < 3; ++a) {
    if (sampling) {
      const double c = floor(radius / (double)sh.s[a]) + 1.0;
      cap[a] = c >= 32767.0 ? 32767 : (int)c;
      const float one = sh.s[a] * sh.s[a];
      if (d[a] > 1 && one <= r2f) origin_only = false;
    } else {
      int c = (int)sqrt((double)R2);
      while ((int64_t)c * c > R2) --c;
      while ((int64_t)(c + 1) * (c + 1) <= R2) ++c;
      cap[a] = c;
      if (d[a] > 1 && R2 >= 1) origin_only = false;
    }
  }
  if (origin_only || Kc == 0) {                        // the ball holds only the origin, or there is no class: a copy
    const int64_t total = sh.N * sh.V;
    hipLaunchKernelGGL(k_morph_copy, dim3(flat_blocks(total)), dim3(kBlock), 0, st, labels, out, C, total, 0);
    ADVCHAIN_LAUNCH_CHECK();
    return ADVCHAIN_OK;
  }
  if (sampling) return morph_run<float>(labels, sampling, op, out, workspace, C, Kc, sh, cap, r2f, ndim, dims, st);
  return morph_run<int>(labels, sampling, op, out, workspace, C, Kc, sh, cap, R2, ndim, dims, st);
}

}  // extern "C"
