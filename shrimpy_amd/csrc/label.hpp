// What the labelling kernels (label.hip) and their host twins (host_twins.hip) share: the entry checks, the neighbourhoods,
// the object record and the order-preserving integer image of a float -- ONE definition, so that the two sides agree on
// every integer field.  The oracle is scipy.ndimage.label (tests/label_ref.py): labels 1 .. N in raster (C-order) rank of
// each component's lowest linear index.
//
// Rule: foreground is in[v] > threshold (NaN and the threshold itself are background); connectivity 6, 18 or 26 is
// scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3): two voxels are neighbours iff they differ by at most 1 on every
// axis and on at most `level` = 1 | 2 | 3 axes.  Every set of the union-find is rooted at its SMALLEST linear index
// (parent[v] <= v always), so the roots in raster order ARE the components in label order.
#pragma once

#include <cstring>

#include "common.hpp"

namespace lsr {
namespace label {

constexpr int kTileZ = 4, kTileY = 16, kTileX = 64;      // one workgroup's tile (kTileX = the wavefront: a row per wave step)
constexpr int kTileVoxels = kTileZ * kTileY * kTileX;
constexpr int kChunk = 4096;                             // voxels per workgroup of the numbering launches
constexpr int64_t kMaxVoxels = (int64_t(1) << 31) - 1;   // linear indices and labels are int32

// One row of the object table (96 bytes; part of the ABI: shrimpy_amd/segment.py reads it as a structured array).
struct Region {
  int64_t volume;          // voxels
  int64_t sum_zyx[3];      // sum of z, of y, of x
  double sum_v;            // sum of intensity            (0 without an intensity volume)
  double sum_vzyx[3];      // sum of intensity * z, y, x
  int32_t lo[3];           // bounding box, half-open: lo <= c < hi
  int32_t hi[3];
  float v_min, v_max;      // intensity range             (0 without an intensity volume)
};
static_assert(sizeof(Region) == 96, "the object record's size is part of the ABI");

inline int level_of(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

inline int check_volume(int64_t Z, int64_t Y, int64_t X) {
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE(Z <= kMaxVoxels && Y <= kMaxVoxels && X <= kMaxVoxels && Z * Y <= kMaxVoxels && Z * Y * X <= kMaxVoxels,
              LSR_E_UNSUPPORTED, "shape (%lld,%lld,%lld): a labelled volume holds at most 2^31 - 1 voxels", (long long)Z,
              (long long)Y, (long long)X);
  return LSR_OK;
}

inline int check_label(const void* in, int64_t Z, int64_t Y, int64_t X, int connectivity, const void* labels,
                       const void* n_objects, const void* scratch) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(labels);
  LSR_REQUIRE_PTR(n_objects);
  LSR_REQUIRE_PTR(scratch);
  if (int rc = check_volume(Z, Y, X)) return rc;
  LSR_REQUIRE(level_of(connectivity) != 0, LSR_E_ARG, "connectivity %d: 6, 18 or 26", connectivity);
  return LSR_OK;
}

inline int check_regions(const void* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, const void* table) {
  LSR_REQUIRE_PTR(labels);
  if (int rc = check_volume(Z, Y, X)) return rc;
  LSR_REQUIRE(n_objects >= 0 && n_objects <= kMaxVoxels, LSR_E_ARG, "%lld objects: 0 .. 2^31 - 1", (long long)n_objects);
  if (n_objects > 0) LSR_REQUIRE_PTR(table);
  return LSR_OK;
}

inline int check_remap(const void* labels, int64_t n, const void* map, int64_t n_map) {
  LSR_REQUIRE_PTR(labels);
  LSR_REQUIRE_PTR(map);
  LSR_REQUIRE(n > 0, LSR_E_SHAPE, "%lld voxels: at least one", (long long)n);
  LSR_REQUIRE(n <= kMaxVoxels, LSR_E_UNSUPPORTED, "%lld voxels: at most 2^31 - 1", (long long)n);
  LSR_REQUIRE(n_map > 0 && n_map <= kMaxVoxels, LSR_E_ARG, "a map of %lld entries: 1 .. 2^31 - 1 (entry 0 is the background's)",
              (long long)n_map);
  return LSR_OK;
}

inline int64_t number_blocks(int64_t n) { return ceil_div(n, kChunk); }

// Is (dz, dy, dx) one of the neighbours that PRECEDE a voxel in raster order under `level`?  (13 of the 26 at level 3.)
__host__ __device__ inline bool backward_neighbour(int dz, int dy, int dx, int level) {
  const int nnz = (dz != 0) + (dy != 0) + (dx != 0);
  if (nnz == 0 || nnz > level) return false;
  return dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
}

// The order-preserving integer image of a float: a < b  <=>  key(a) < key(b) for every pair of non-NaN floats
// (-0.0 sorts just below +0.0; NaNs sort outside the infinities by their sign bit).
__host__ __device__ inline uint32_t float_key(float v) {
  uint32_t b;
  memcpy(&b, &v, sizeof(b));
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float key_float(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  memcpy(&v, &b, sizeof(v));
  return v;
}

// ---- the host twins' union-find (sequential; rooted at the smallest index, as on the device) ----

// The root of a, with path halving: a winding component stays near-linear.
inline int32_t find_host(int32_t* parent, int32_t a) {
  while (parent[a] != a) {
    parent[a] = parent[parent[a]];
    a = parent[a];
  }
  return a;
}

// From parent words (-1 on the background) to labels, in place: every chain is cut to its root, the roots are numbered in
// raster order (a numbered root holds -(label + 1), as on the device; a root precedes every other voxel of its set), and
// every voxel takes its root's label, 0 on the background.  Returns the number of roots.
inline int32_t number_roots_host(int32_t* words, int64_t n) {
  for (int64_t v = 0; v < n; ++v)
    if (words[v] >= 0) words[v] = find_host(words, static_cast<int32_t>(v));
  int32_t count = 0;
  for (int64_t v = 0; v < n; ++v)
    if (words[v] == v) words[v] = -(++count) - 1;
  for (int64_t v = 0; v < n; ++v) {
    const int32_t p = words[v];
    words[v] = p == -1 ? 0 : p < 0 ? -p - 1 : words[p];       // (p < v is a root: it has its label already)
  }
  return count;
}

}  // namespace label
}  // namespace lsr
