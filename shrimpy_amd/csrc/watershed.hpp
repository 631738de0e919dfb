// What the watershed kernels (watershed.hip) and their host twins (host_twins.hip) share: the entry checks, the direction
// codes, the `up` rule, the saddle record and its hash -- ONE definition each.  No upstream is pinned: the rule below IS the
// specification (tests/watershed_ref.py restates it in numpy), and device, twin and restatement agree element for element.
//
// Rule.  objects (int32, <= 0 is background), surface (float32), connectivity 6 | 18 | 26 (label.hpp's neighbourhoods).
//   Surface values compare by lsr::label::float_key: a total order on all bit patterns (-0.0 below +0.0, +inf ordinary; NaN
//   is unsupported, but it has a place in the order, so nothing can hang on it).
//   N(v): the neighbours of v inside the volume with objects[u] == objects[v].
//   up(v): the element of N(v) + {v} with the greatest (key(surface), then the SMALLER linear index) -- a strict total order,
//   so every ascent path ends at a summit up(v) == v and plateaus need no special case.
//   Basins: the connected components of the edges {v, up(v)}, numbered 1 .. B in raster order of their smallest linear index
//   (label.hpp's numbering); 0 on the background.  B = the number of summits.
//   Saddles: for neighbours v, u of one object in different basins a < b, pass = min(surface[v], surface[u]) (by key);
//   saddle(a, b) = the maximum of the passes.
#pragma once

#include "label.hpp"
#include "pair_table.hpp"

namespace lsr {
namespace watershed {

// One workgroup's tile of the local launch (kTileX = the wavefront: a row per wave step), staged with a one-voxel halo.
constexpr int kTileZ = 8, kTileY = 8, kTileX = 64;
constexpr int kTileVoxels = kTileZ * kTileY * kTileX;
constexpr int kHaloY = kTileY + 2, kHaloX = kTileX + 2;
constexpr int kHaloVoxels = (kTileZ + 2) * kHaloY * kHaloX;      // 6600: two words each, 52 800 B of LDS
constexpr int kSelf = 13;                                        // the code of (0, 0, 0)

// The code of a direction: (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), ascending in the linear index of the neighbour.
__host__ __device__ inline int code_of(int dz, int dy, int dx) { return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }

// up(v) as a direction code.  same(dz, dy, dx, &key) answers whether that neighbour lies in the volume and in v's object and
// if so gives the key of its surface value.  The candidates are visited in ascending linear index and one replaces the best
// so far only where its key is strictly greater: among equal keys the smallest index stays.
template <class Same>
__host__ __device__ inline int up_code(uint32_t self_key, int level, Same same) {
  long long best = -1;
  int code = kSelf;
  for (int dz = -1; dz <= 1; ++dz) {
    for (int dy = -1; dy <= 1; ++dy) {
      for (int dx = -1; dx <= 1; ++dx) {
        const int nnz = (dz != 0) + (dy != 0) + (dx != 0);
        if (nnz > level) continue;
        uint32_t key = self_key;
        if (nnz != 0 && !same(dz, dy, dx, &key)) continue;
        if (static_cast<long long>(key) > best) {
          best = static_cast<long long>(key);
          code = code_of(dz, dy, dx);
        }
      }
    }
  }
  return code;
}

// One slot of the saddle table (16 bytes; part of the ABI: shrimpy_amd/watershed.py reads it as a structured array).
struct Saddle {
  unsigned long long pair;      // a << 32 | b with 1 <= a < b; 0 = empty
  uint32_t key;                 // float_key of the greatest pass seen
  uint32_t unused;              // stays what the caller wrote (zero)
};
static_assert(sizeof(Saddle) == 16, "the saddle record's size is part of the ABI");

// Is (dz, dy, dx) one of the neighbours that FOLLOW a voxel in raster order under `level`?
__host__ __device__ inline bool forward_neighbour(int dz, int dy, int dx, int level) {
  return label::backward_neighbour(-dz, -dy, -dx, level);
}

inline int64_t scratch_bytes(int64_t n) {      // the block counts of the numbering, then one direction byte per voxel
  return label::number_blocks(n) * static_cast<int64_t>(sizeof(int)) + ceil_div(n, 4) * 4;
}

inline int check_watershed(const void* objects, const void* surface, int64_t Z, int64_t Y, int64_t X, int connectivity,
                           const void* basins, const void* n_basins, const void* scratch) {
  LSR_REQUIRE_PTR(objects);
  LSR_REQUIRE_PTR(surface);
  LSR_REQUIRE_PTR(basins);
  LSR_REQUIRE_PTR(n_basins);
  LSR_REQUIRE_PTR(scratch);
  if (int rc = label::check_volume(Z, Y, X)) return rc;
  LSR_REQUIRE(label::level_of(connectivity) != 0, LSR_E_ARG, "connectivity %d: 6, 18 or 26", connectivity);
  LSR_REQUIRE(basins != objects && basins != surface, LSR_E_ARG, "basins must not alias objects or surface");
  return LSR_OK;
}

inline int check_saddles(const void* objects, const void* basins, const void* surface, int64_t Z, int64_t Y, int64_t X,
                         int connectivity, int64_t capacity, const void* table, const void* counts) {
  LSR_REQUIRE_PTR(objects);
  LSR_REQUIRE_PTR(basins);
  LSR_REQUIRE_PTR(surface);
  LSR_REQUIRE_PTR(table);
  LSR_REQUIRE_PTR(counts);
  if (int rc = label::check_volume(Z, Y, X)) return rc;
  LSR_REQUIRE(label::level_of(connectivity) != 0, LSR_E_ARG, "connectivity %d: 6, 18 or 26", connectivity);
  return check_pair_capacity(capacity);
}

}  // namespace watershed
}  // namespace lsr
