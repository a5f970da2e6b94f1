// The 62-column strip scheme and the difference stencils shared by deform_diff.hip (2D helpers of the reference) and
// jacobian.hip (3D helpers, positions mode, folding statistics).  Both files are compiled with -ffp-contract=off (build.py).
#pragma once
#include "common.h"

namespace advchain {
namespace {

constexpr int kCols = 62;      // output columns per wave
constexpr int kWavesPerBlock = kBlock / 64;

// d/dx of calculate_image_diff at column x of a row of W >= 2 values (l, c, r: columns x-1, x, x+1)
__device__ __forceinline__ float diff1(float l, float c, float r, int x, int W) {
  if (x == 0) return r - c;
  if (x == W - 1) return c - l;
  return 0.5f * (r - l);
}

// adjoint of diff1 at column x: gl, g0, gr = the gradient of the difference at columns x-1, x, x+1
__device__ __forceinline__ float diff1_adj(float gl, float g0, float gr, int x, int W) {
  float a = 0.f;
  if (x == 1) a += gl;                                   // dx[0] = v[1] - v[0]
  else if (x >= 2 && x <= W - 1) a += 0.5f * gl;         // interior x-1: 0.5 (v[x] - v[x-2])
  if (x == 0) a -= g0;
  if (x == W - 1) a += g0;                               // dx[W-1] = v[W-1] - v[W-2]
  if (x == W - 2) a -= gr;
  else if (x >= 0 && x <= W - 3) a -= 0.5f * gr;         // interior x+1: 0.5 (v[x+2] - v[x])
  return a;
}

struct Strip {
  int64_t plane;   // plane (diff) or sample (Jacobian) index
  int x;           // this lane's column (may be -1 or >= W on the halo lanes)
  int xc;          // clamped column (every lane loads a valid address)
  int y0, y1;      // rows of the strip
  bool store;
};

// wave -> (plane, column chunk, row strip); false when the wave has no work (the whole wave returns together)
__device__ __forceinline__ bool strip_of(int64_t planes, int H, int W, int chunks, int strips, int R, Strip& s) {
  const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t per_plane = (int64_t)chunks * strips;
  if (w >= planes * per_plane) return false;
  const int lane = threadIdx.x & 63;
  s.plane = w / per_plane;
  const int rem = (int)(w - s.plane * per_plane);
  const int strip = rem / chunks, chunk = rem - strip * chunks;
  s.x = chunk * kCols + lane - 1;
  s.xc = s.x < 0 ? 0 : (s.x >= W ? W - 1 : s.x);
  s.y0 = strip * R;
  s.y1 = s.y0 + R < H ? s.y0 + R : H;
  s.store = lane >= 1 && lane <= kCols && s.x < W;
  return true;
}

__device__ __forceinline__ float row_at(const float* p, int r, int H, int W, int xc) {
  return (r >= 0 && r < H) ? p[(int64_t)r * W + xc] : 0.f;       // r is the same in every lane
}

// det = (1 + dxx) (1 + dyy) - dxy dyx with (dxx, dxy) = diff(u), (dyx, dyy) = diff(v)  (adv_morph.py:96-99)
__device__ __forceinline__ float det_of(float dxx, float dxy, float dyx, float dyy) {
  return (1.f + dxx) * (1.f + dyy) - dxy * dyx;
}

// ---- host helpers -------------------------------------------------------------------------------------------------------
bool hw_ok(const int64_t* dims) {
  return dims && dims[0] >= 2 && dims[1] >= 2 && dims[0] <= (1 << 24) && dims[1] <= (1 << 24) &&
         dims[0] * dims[1] < (1ll << 31);
}

struct StripLaunch {
  int chunks, strips, R;
  unsigned blocks;
};

// rows per strip: 32, halved while the launch would have fewer than 8192 waves (down to 4)
bool strip_launch(int64_t planes, int H, int W, StripLaunch& L) {
  L.chunks = (W + kCols - 1) / kCols;
  L.R = 32;
  for (;;) {
    L.strips = (H + L.R - 1) / L.R;
    if (L.R <= 4 || planes * L.chunks * L.strips >= 8192) break;
    L.R >>= 1;
  }
  const int64_t waves = planes * L.chunks * L.strips;
  if (waves > (int64_t)kWavesPerBlock * 0x7fffffffll) return false;
  L.blocks = (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
  return true;
}

}  // namespace
}  // namespace advchain
