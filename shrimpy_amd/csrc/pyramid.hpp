// What the 2x downsampling kernel (pyramid.hip) and its host twin (host_twins.hip) share: the argument checks, the
// output shape and the arithmetic of one window -- ONE definition, so that the two agree bit for bit.
//
// Output voxel (z, y, x) of a (Z, Y, X) volume is the mean over the input voxels (fz z + a, 2 y + b, 2 x + c),
// a < fz, b < 2, c < 2, that lie inside the volume: nothing is padded, nothing dropped, the output has ceil(n / f)
// voxels per axis and a window 1, 2, 4 or 8 = 2^k voxels.
//   float32: s = ((v000 + v001) + (v010 + v011)) + ((v100 + v101) + (v110 + v111))   (v[a][b][c]: x pairs, then y, then z;
//            float32 additions; a missing neighbour is left out, never added as zero), result s * 2^-k: three roundings.
//   uint16:  32-bit sum, (sum + (2^k >> 1)) >> k: round half up, exact.
#pragma once

#include "common.hpp"

namespace lsr {
namespace pyramid {

__host__ __device__ inline int64_t out_extent(int64_t n, int f) { return (n + f - 1) / f; }

inline int check_shape(int64_t Z, int64_t Y, int64_t X, int fz) {
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(fz == 1 || fz == 2, LSR_E_ARG, "z factor %d: 1 or 2", fz);
  return LSR_OK;
}

inline int check(const void* in, int64_t Z, int64_t Y, int64_t X, const void* out, int fz) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(in != out, LSR_E_ARG, "out must not alias in");
  return check_shape(Z, Y, X, fz);
}

// x pair of one input row: p[0] (+ p[1] when the neighbour exists)
__host__ __device__ inline float pair(float a, float b, bool hx) { return hx ? a + b : a; }
__host__ __device__ inline uint32_t pair(uint16_t a, uint16_t b, bool hx) {
  return hx ? static_cast<uint32_t>(a) + static_cast<uint32_t>(b) : static_cast<uint32_t>(a);
}

// The window's result from its (up to) four x pairs r[a][b]; hy / hz: the y / z neighbour rows exist; k = log2(count).
__host__ __device__ inline float finish(float r00, float r01, float r10, float r11, bool hy, bool hz, int k) {
  float s = hy ? r00 + r01 : r00;
  if (hz) s = s + (hy ? r10 + r11 : r10);
  return s * (k == 0 ? 1.0f : k == 1 ? 0.5f : k == 2 ? 0.25f : 0.125f);   // exact: a power of two
}
__host__ __device__ inline uint16_t finish(uint32_t r00, uint32_t r01, uint32_t r10, uint32_t r11, bool hy, bool hz, int k) {
  uint32_t s = hy ? r00 + r01 : r00;
  if (hz) s = s + (hy ? r10 + r11 : r10);
  return static_cast<uint16_t>((s + ((1u << k) >> 1)) >> k);
}

}  // namespace pyramid
}  // namespace lsr
