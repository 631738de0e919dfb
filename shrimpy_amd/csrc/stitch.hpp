// What the stitching kernel (stitch.hip) and its host twin (host_twins.hip) share: the tile table, the split of a
// translation, the coverage test, the sample, the weight and the blend -- ONE definition, so that the two agree bit for
// bit.  biahub's stitch is not vendored: PARITY UNPINNED, the rule is this package's own (tests/stitch_ref.py restates it
// in float64).
//
// K tiles, each a dense float32 (Zk, Yk, Xk), one float64 translation t_k = (tz, ty, tx) per tile in canvas voxels: tile
// voxel i sits at canvas coordinate i + t_k.  Canvas: origin = floor(min_k t_k), shape = ceil(max_k (t_k + n_k)) - origin.
//
// Per tile and axis, split on the host in float64: ti = floor(t), tf = t - ti.  For the absolute canvas index c put
// j = c - ti.
//   tf == 0: one tap i = j, covered iff 0 <= j <= n - 1;
//   else:    two taps i0 = j - 1 (weight w0 = float32(tf)) and i1 = j (weight w1 = float32(1 - tf)), the same for every voxel
//            of the tile, covered iff 1 <= j <= n - 1.
// Indexing and coverage are integer arithmetic; a tile covers a voxel iff all three axes are covered: nothing is ever
// interpolated against the fill value.
//
// Sample s_k: the tile voxel itself without a fractional axis; otherwise w0 * v(i0) + w1 * v(i1) (two float32 products,
// one float32 sum, never fused) over the fractional axes only, x first, then y, then z.
// Weight w_k = (dy * dx)^p, p in 0 .. 4, by repeated float32 multiplication (1, then p times "* (dy * dx)"), with
// d = min(l + 1, n - l), l = c - t the position inside the tile along y or x.  In float32 that is evaluated as
//   d = min(float(j) + w1, float(n - j) + w0)            (l + 1 = j + (1 - tf), n - l = (n - j) + tf)
// so that neither branch subtracts two large numbers: each is rounded relative to its own value (the y and x extents of a tile are at most
// 2^24, so the two conversions are exact), d >= 1 on every covered voxel, and an integer placement gives the integers min(j + 1, n - j) exactly.  z only decides coverage.
// Output: no tile covers the voxel: cval; exactly one: s_k itself (no multiply, no divide: an integer placement copies the
// interior bit for bit); otherwise (sum w_k s_k) / (sum w_k) in float32, accumulated in ascending tile index.
#pragma once

#include <cmath>

#include "common.hpp"

namespace lsr {
namespace stitch {

constexpr int kMaxTiles = 1024;
constexpr int kMaxExponent = 4;
constexpr double kMaxTranslation = 1073741824.0;   // |t| < 2^30 canvas voxels
constexpr int64_t kMaxEdgeExtent = int64_t(1) << 24;   // y and x extents: float(j) and float(n - j) in edge() stay exact

// One entry of the tile table (96 bytes; the C ABI hands it around as opaque bytes, lsr_stitch_table_bytes()).
struct Tile {
  const float* data;
  int64_t n[3];      // (Z, Y, X)
  int64_t ti[3];     // floor(t)
  float w0[3];       // float32(tf): the weight of tap j - 1 (0 on an integer axis)
  float w1[3];       // float32(1 - tf): the weight of tap j (1 on an integer axis)
  int32_t frac[3];   // tf != 0
  int32_t reserved;
};
static_assert(sizeof(Tile) == 96, "the tile table's entry size is part of the ABI");

inline int check_tile(const void* data, const int64_t n[3], const double t[3], int k) {
  LSR_REQUIRE(data != nullptr, LSR_E_NULL, "tile %d is NULL", k);
  LSR_REQUIRE(n[0] > 0 && n[1] > 0 && n[2] > 0, LSR_E_SHAPE, "tile %d: shape (%lld,%lld,%lld) must be positive", k,
              (long long)n[0], (long long)n[1], (long long)n[2]);
  LSR_REQUIRE_VOLUME(n[0], n[1], n[2]);
  LSR_REQUIRE(n[1] <= kMaxEdgeExtent && n[2] <= kMaxEdgeExtent, LSR_E_UNSUPPORTED,
              "tile %d: shape (%lld,%lld,%lld): the y and x extents are at most 2^24", k, (long long)n[0], (long long)n[1],
              (long long)n[2]);
  for (int a = 0; a < 3; ++a)
    LSR_REQUIRE(std::isfinite(t[a]) && std::fabs(t[a]) < kMaxTranslation, LSR_E_ARG,
                "tile %d: translation %g on axis %d must be finite and below 2^30 in magnitude", k, t[a], a);
  return LSR_OK;
}

inline int check_count(int n_tiles) {
  LSR_REQUIRE(n_tiles > 0, LSR_E_SHAPE, "%d tiles: at least one", n_tiles);
  LSR_REQUIRE(n_tiles <= kMaxTiles, LSR_E_UNSUPPORTED, "%d tiles: the table holds at most %d", n_tiles, kMaxTiles);
  return LSR_OK;
}

inline int check_launch(const void* table, int n_tiles, const void* out, const int64_t* box_origin, const int64_t* box_shape,
                        int p) {
  LSR_REQUIRE_PTR(table);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE_PTR(box_origin);
  LSR_REQUIRE_PTR(box_shape);
  if (int rc = check_count(n_tiles)) return rc;
  LSR_REQUIRE(box_shape[0] > 0 && box_shape[1] > 0 && box_shape[2] > 0, LSR_E_SHAPE, "box shape (%lld,%lld,%lld) must be positive",
              (long long)box_shape[0], (long long)box_shape[1], (long long)box_shape[2]);
  LSR_REQUIRE_VOLUME(box_shape[0], box_shape[1], box_shape[2]);
  for (int a = 0; a < 3; ++a)
    LSR_REQUIRE(box_origin[a] > -(int64_t(1) << 31) && box_origin[a] < (int64_t(1) << 31), LSR_E_ARG,
                "box origin %lld on axis %d: below 2^31 in magnitude", (long long)box_origin[a], a);
  LSR_REQUIRE(p >= 0 && p <= kMaxExponent, LSR_E_ARG, "blending exponent %d: 0 .. %d", p, kMaxExponent);
  return LSR_OK;
}

// the float64 split of one tile's translation into the table entry
inline void fill_tile(Tile& e, const float* data, const int64_t n[3], const double t[3]) {
  e.data = data;
  for (int a = 0; a < 3; ++a) {
    const double fl = std::floor(t[a]), tf = t[a] - fl;
    e.n[a] = n[a];
    e.ti[a] = static_cast<int64_t>(fl);
    e.frac[a] = tf != 0.0 ? 1 : 0;
    e.w0[a] = static_cast<float>(tf);
    e.w1[a] = static_cast<float>(1.0 - tf);
  }
  e.reserved = 0;
}

// origin = floor(min t), shape = ceil(max (t + n)) - origin
inline void canvas(const int64_t* shapes, const double* translations, int n_tiles, int64_t origin[3], int64_t shape[3]) {
  for (int a = 0; a < 3; ++a) {
    double lo = translations[a], hi = translations[a] + static_cast<double>(shapes[a]);
    for (int k = 1; k < n_tiles; ++k) {
      lo = std::fmin(lo, translations[3 * k + a]);
      hi = std::fmax(hi, translations[3 * k + a] + static_cast<double>(shapes[3 * k + a]));
    }
    origin[a] = static_cast<int64_t>(std::floor(lo));
    shape[a] = static_cast<int64_t>(std::ceil(hi)) - origin[a];
  }
}

__host__ __device__ inline bool covered(int64_t j, int64_t n, int frac) { return j >= frac && j <= n - 1; }

// two taps of a fractional axis: (w0 * a0) + (w1 * a1), three roundings (the TUs are built with -ffp-contract=off)
__host__ __device__ inline float lerp(float a0, float a1, float w0, float w1) {
  const float p0 = w0 * a0, p1 = w1 * a1;
  return p0 + p1;
}

// one axis of the sample: both taps on a fractional axis, the tap j alone (a1) otherwise
__host__ __device__ inline float tap(float a0, float a1, bool frac, float w0, float w1) {
  return frac ? lerp(a0, a1, w0, w1) : a1;
}

// distance to the nearer tile edge along one axis, in voxels, counted from 1 (see above)
__host__ __device__ inline float edge(int64_t j, int64_t n, float w0, float w1) {
  const float a = static_cast<float>(j) + w1, b = static_cast<float>(n - j) + w0;
  return a < b ? a : b;
}

__host__ __device__ inline float weight(float dy, float dx, int p) {
  const float b = dy * dx;
  float w = 1.0f;
  for (int i = 0; i < p; ++i) w = w * b;
  return w;
}

// the blend of one canvas voxel: tiles are added in ascending index
struct Acc {
  int n;
  float first, num, den;
  __host__ __device__ inline void clear() { n = 0; first = num = den = 0.0f; }
  __host__ __device__ inline void add(float s, float w) {
    const float ws = w * s;
    if (n == 0) {
      first = s; num = ws; den = w;
    } else {
      num = num + ws; den = den + w;
    }
    ++n;
  }
  __host__ __device__ inline float finish(float cval) const { return n == 0 ? cval : n == 1 ? first : num / den; }
};

}  // namespace stitch
}  // namespace lsr
