// What the rank-filter kernel (rank.hip) and its host twin (host_twins.hip) share: the rule, the entry check, the border fold,
// the selection and the fused op -- ONE definition, so that the two sides choose the same element.
//
// Rule.  A box of half-widths (rz, ry, rx), each in 0 .. kMaxHalfWidth, window 2r + 1 per axis, n elements, over a contiguous
// (Z, Y, X) float32 volume v; `rank` in 0 .. n - 1.
//   Border: scipy's `reflect` (d c b a | a b c d).  Index i on an axis of length L reads fold(i, L): m = i mod 2L, then m < L ? m
//   : 2L - 1 - m.  A half-width may exceed the axis (L = 1 included): the fold then applies more than once.  Reflected voxels
//   count as often as they fall in the window -- here the rank filter differs from the morphology's "outside does not compete".
//   m(p) is the element of rank `rank` (the rank-th smallest, from 0) of the multiset of window values.  Values are ordered by
//   label::float_key (-0.0 below +0.0, +-inf ordinary values); a NaN is the greatest code (morph::kNanCode) and comes back as
//   the canonical quiet NaN 0x7fc00000.  The result is the bit pattern of the chosen element: no order of evaluation can
//   change it.
//   op (fused into the store; t a float32 threshold, each difference ONE IEEE float32 subtraction, a comparison with a NaN
//   false):  0 value: m   1 remove_bright: (v - m > t) ? m : v   2 remove_dark: (m - v > t) ? m : v   3 remove_both: m where
//   either holds, else v.  All half-widths 0 make n = 1: every op copies v, except that a NaN becomes the canonical one under
//   op 0.
// scipy.ndimage.rank_filter / median_filter / percentile_filter with size = 2r + 1, mode = "reflect", by value on NaN-free
// volumes (on +-0.0 ties scipy may return either zero); tests/rank_ref.py restates the rule by a full sort and pins the bits.
//
// Selection.  Bitwise bisection on the 32-bit code from the most significant bit down: candidate = prefix | bit, keep the bit
// iff at least n - rank window codes are >= candidate.  After 32 steps prefix is the code of the element of rank `rank`:
// branch-free, no per-lane arrays, exact at any n.
#pragma once

#include "common.hpp"
#include "morphology.hpp"

namespace lsr {
namespace rank {

constexpr int kMaxHalfWidth = 3;            // a window of at most 7 x 7 x 7 = 343 elements
constexpr int kTileZ = 4, kTileY = 8, kTileX = 64;      // outputs per workgroup; x on the lanes of a wavefront
constexpr int kThreads = 256;
// the halo'd tile at the cap: 10 x 14 x 70 codes = 39,200 bytes of the 160 KiB of LDS (four workgroups per compute unit)
constexpr int kMaxTileCodes = (kTileZ + 2 * kMaxHalfWidth) * (kTileY + 2 * kMaxHalfWidth) * (kTileX + 2 * kMaxHalfWidth);
static_assert(kMaxTileCodes * 4 <= 64 * 1024, "the halo'd tile must fit in the LDS a launch gets without asking");
static_assert(kTileX == kWave && kTileZ * kTileY * kTileX % kThreads == 0, "a wavefront takes one row of the tile at a time");

enum Op { kValue = 0, kRemoveBright = 1, kRemoveDark = 2, kRemoveBoth = 3 };
enum Variant { kAuto = 0, kGeneric = 1 };

// scipy's `reflect`: any i, L >= 1
__host__ __device__ inline int64_t fold(int64_t i, int64_t L) {
  const int64_t p = 2 * L;
  int64_t m = i % p;
  if (m < 0) m += p;
  return m < L ? m : p - 1 - m;
}

// The code of the element of rank n - need: count_ge(c) is the number of window codes >= c.
template <typename CountGE>
__host__ __device__ inline uint32_t bisect(int need, CountGE&& count_ge) {
  uint32_t prefix = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t candidate = prefix | (1u << b);
    if (count_ge(candidate) >= need) prefix = candidate;
  }
  return prefix;
}

// the store: m the selected element, v the voxel itself
__host__ __device__ inline float fused(float m, float v, int op, float t) {
  if (op == kValue) return m;
  const bool bright = v - m > t, dark = m - v > t;
  const bool take = op == kRemoveBright ? bright : (op == kRemoveDark ? dark : (bright || dark));
  return take ? m : v;
}

inline int check_rank(const float* in, const float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int rank, int op,
                      float threshold, int variant) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(in != out, LSR_E_ARG, "out must not alias in");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(rz >= 0 && ry >= 0 && rx >= 0, LSR_E_ARG, "half-widths (%d,%d,%d) must be >= 0", rz, ry, rx);
  LSR_REQUIRE(rz <= kMaxHalfWidth && ry <= kMaxHalfWidth && rx <= kMaxHalfWidth, LSR_E_UNSUPPORTED,
              "half-widths (%d,%d,%d): at most %d per axis", rz, ry, rx, kMaxHalfWidth);
  const int n = (2 * rz + 1) * (2 * ry + 1) * (2 * rx + 1);
  LSR_REQUIRE(rank >= 0 && rank < n, LSR_E_ARG, "rank %d: 0 .. %d for a window of %d elements", rank, n - 1, n);
  LSR_REQUIRE(op >= kValue && op <= kRemoveBoth, LSR_E_ARG, "op %d: 0 value, 1 remove_bright, 2 remove_dark, 3 remove_both", op);
  LSR_REQUIRE(variant == kAuto || variant == kGeneric, LSR_E_ARG, "variant %d: 0 auto, 1 the generic path", variant);
  LSR_REQUIRE(op == kValue || threshold == threshold, LSR_E_ARG, "threshold is NaN");
  return LSR_OK;
}

// One voxel on the host: the window's codes gathered through the fold, the bisection over them, the fused op.
inline float voxel_host(const float* in, int64_t Z, int64_t Y, int64_t X, int64_t z, int64_t y, int64_t x, int rz, int ry, int rx,
                        int rank, int op, float t) {
  uint32_t codes[(2 * kMaxHalfWidth + 1) * (2 * kMaxHalfWidth + 1) * (2 * kMaxHalfWidth + 1)];
  int n = 0;
  for (int dz = -rz; dz <= rz; ++dz) {
    const int64_t pz = fold(z + dz, Z) * Y;
    for (int dy = -ry; dy <= ry; ++dy) {
      const int64_t py = (pz + fold(y + dy, Y)) * X;
      for (int dx = -rx; dx <= rx; ++dx) codes[n++] = morph::encode(in[py + fold(x + dx, X)], false);
    }
  }
  const uint32_t chosen = bisect(n - rank, [&](uint32_t c) {
    int count = 0;
    for (int i = 0; i < n; ++i) count += codes[i] >= c ? 1 : 0;
    return count;
  });
  return fused(morph::decode(chosen, false), in[(z * Y + y) * X + x], op, t);
}

}  // namespace rank
}  // namespace lsr
