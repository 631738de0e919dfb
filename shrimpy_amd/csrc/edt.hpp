// What the distance-transform kernels (edt.hip) and their host twins (host_twins.hip) share: the rule, the entry checks, the
// row scan's choice and the line pass itself -- ONE definition, so that the two sides take every comparison alike.
//
// Rule.  Sites are a set of voxels of a (Z, Y, X) volume; sampling (sz, sy, sx) are positive finite float64 spacings.
//   nearest[v] (int32)  the linear index of a site that minimises (sz dz)^2 + (sy dy)^2 + (sx dx)^2; among equals the
//                       SMALLEST linear index wins.
//   dist[v] (float32)   the float32 rounding of the float64 value
//                       sqrt(((sz*dz)*(sz*dz) + (sy*dy)*(sy*dy)) + (sx*dx)*(sx*dx)) measured to nearest[v], in that order
//                       (distance() below).  At a nearest site this is scipy.ndimage.distance_transform_edt(mask,
//                       sampling=...) bit for bit (tests/edt_ref.py).
//   A site has dist == 0 and nearest == v.
//   With NO site anywhere dist = +inf and nearest = -1 at every voxel.  This differs from scipy on purpose: scipy measures
//   from index -1 there and returns garbage.
// The index rule is ours (scipy's return_indices breaks ties another way) and is pinned by brute force.
//
// Scheme.  A separable min-plus over x, then y, then z, every pass breaking ties towards the SMALLER source coordinate,
// yields exactly the smallest-linear-index nearest site:
//   x     per voxel the nearest site of its row, a tie going to the left: its x, or -1 in a row without a site.
//   y, z  per line the lower envelope of the parabolas g_k + w (p - k)^2 of the line's entries (line_pass below, after
//         Meijster et al.), w = s^2 of the axis, costs in float64: exact for integer and dyadic spacings.  An entry without
//         a site (-1) contributes NO parabola.  The y pass leaves the in-plane index y' * X + x' of the winner (-1 in a
//         plane without a site), the z pass the linear index and, fused, the distance.
// Every line is independent: nothing here communicates between lines.
#pragma once

#include <cmath>
#include <cstring>

#include "common.hpp"

namespace lsr {
namespace edt {

constexpr int kChunk = 64;                               // x pass: voxels per ballot (the wavefront)
constexpr int kRowsPerBlock = 4;                         // x pass: one row per wave of a 256-thread workgroup
constexpr int kLineTile = 256;                           // y and z passes: lines per workgroup, one lane each
constexpr int64_t kMaxRowBlocks = 2048;                  // x pass: workgroups at most (they stride over the rows)
constexpr int64_t kMaxLanes = int64_t(1) << 17;          // y and z passes: lanes at most (they stride over the lines)
constexpr int kStackFields = 3;                          // an envelope entry: position, value, first position it owns
constexpr int64_t kMaxVoxels = (int64_t(1) << 31) - 1;   // linear indices are int32

inline int check_volume(int64_t Z, int64_t Y, int64_t X) {
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE(Z <= kMaxVoxels && Y <= kMaxVoxels && X <= kMaxVoxels && Z * Y <= kMaxVoxels && Z * Y * X <= kMaxVoxels,
              LSR_E_UNSUPPORTED, "shape (%lld,%lld,%lld): a distance transform holds at most 2^31 - 1 voxels", (long long)Z,
              (long long)Y, (long long)X);
  return LSR_OK;
}

inline int check_sampling(const double* sampling) {
  for (int a = 0; a < 3; ++a) {
    const double w = sampling[a] * sampling[a];       // (the envelope divides by it)
    LSR_REQUIRE(std::isfinite(sampling[a]) && sampling[a] > 0.0 && std::isfinite(w) && w > 0.0, LSR_E_ARG,
                "sampling[%d] = %g: positive and finite, and its square too", a, sampling[a]);
  }
  return LSR_OK;
}

inline int check_edt(const void* in, int64_t Z, int64_t Y, int64_t X, const double* sampling, const void* dist,
                     const void* nearest, const void* scratch) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(sampling);
  LSR_REQUIRE(dist != nullptr || nearest != nullptr, LSR_E_NULL, "dist and nearest are both NULL");
  LSR_REQUIRE_PTR(scratch);
  if (int rc = check_volume(Z, Y, X)) return rc;
  return check_sampling(sampling);
}

inline int check_expand(const void* labels, const void* nearest, int64_t Z, int64_t Y, int64_t X, const double* sampling,
                        double distance, const void* out) {
  LSR_REQUIRE_PTR(labels);
  LSR_REQUIRE_PTR(nearest);
  LSR_REQUIRE_PTR(sampling);
  LSR_REQUIRE_PTR(out);
  if (int rc = check_volume(Z, Y, X)) return rc;
  if (int rc = check_sampling(sampling)) return rc;
  LSR_REQUIRE(distance >= 0.0, LSR_E_ARG, "distance %g: not negative, not NaN", distance);
  LSR_REQUIRE(out != labels, LSR_E_ARG, "out must not alias labels");
  return LSR_OK;
}

// lanes of a line pass over `lines` lines: whole workgroups, at most kMaxLanes
inline int64_t pass_lanes(int64_t lines) {
  const int64_t whole = ceil_div(lines, kLineTile) * kLineTile;
  return whole < kMaxLanes ? whole : kMaxLanes;
}

// bytes of envelope stacks: the larger of the y pass (Z * X lines of Y entries) and the z pass (Y * X lines of Z entries)
inline int64_t scratch_bytes(int64_t Z, int64_t Y, int64_t X) {
  const int64_t y_words = pass_lanes(Z * X) * Y, z_words = pass_lanes(Y * X) * Z;
  return (y_words > z_words ? y_words : z_words) * kStackFields * static_cast<int64_t>(sizeof(int32_t));
}

struct Sampling {
  double sz, sy, sx;       // the spacings (the distance)
  double wz, wy, wx;       // their squares (the envelope costs)
};

inline Sampling make_sampling(const double* s) { return Sampling{s[0], s[1], s[2], s[0] * s[0], s[1] * s[1], s[2] * s[2]}; }

// The float64 distance of the rule, from coordinate differences.
__host__ __device__ inline double distance(const Sampling& s, int dz, int dy, int dx) {
  const double a = s.sz * static_cast<double>(dz), b = s.sy * static_cast<double>(dy), c = s.sx * static_cast<double>(dx);
  return sqrt((a * a + b * b) + c * c);
}

// ... and from a voxel (z, y, x) to the site of linear index `site`.
__host__ __device__ inline double distance_to(const Sampling& s, int z, int y, int x, int site, int Y, int X) {
  const int sx = site % X, sy = site / X % Y, sz = site / X / Y;
  return distance(s, z - sz, y - sy, x - sx);
}

// x pass: of the nearest site at or left of x (`left`) and at or right of it (`right`), -1 for none: the nearer, the left on a tie.
__host__ __device__ inline int nearer_in_row(int x, int left, int right) {
  if (left < 0) return right;
  if (right < 0) return left;
  return x - left <= right - x ? left : right;
}

// cost at position p of the parabola rooted at k with floor g
__host__ __device__ inline double cost(double g, int k, int p, double w) {
  const double d = static_cast<double>(p - k);
  return g + w * (d * d);
}

// The first position in [lo, n] at which the parabola (gu, ku) is STRICTLY below (gi, ki), ki < ku (n: nowhere on the line).
// The difference of the two falls with the position, so the quotient below is an estimate only: the comparisons of the costs
// themselves, the ones every other decision of the pass takes, settle it.
__host__ __device__ inline int first_below(double gi, int ki, double gu, int ku, double w, int lo, int n) {
  const double span = static_cast<double>(ku - ki);
  const double r = ((gu - gi) / w + span * (static_cast<double>(ku) + static_cast<double>(ki))) / (2.0 * span);
  int p = !(r < static_cast<double>(n)) ? n : !(r >= static_cast<double>(lo)) ? lo : static_cast<int>(r) + 1;
  while (p > lo && cost(gu, ku, p - 1, w) < cost(gi, ki, p - 1, w)) --p;
  while (p < n && !(cost(gu, ku, p, w) < cost(gi, ki, p, w))) ++p;
  return p;
}

// One line of a y or z pass.  `io` gives the line: n entries, load(k) -> the entry's value (-1: no parabola), floor(v) -> the
// parabola's floor g from its value, store(p, k, v) -> position p belongs to the entry (k, v), store_none(p) -> the line has
// no parabola.  `stack` holds up to n entries (position, value, first owned position): put(q, k, v, t), get(q, k, v, t).
// Ties go to the smaller position k: an entry is popped or bounded only where the later one is STRICTLY below it.
// Every load of the line precedes its first store, so the line may be rewritten in place.
template <class Io, class Stack>
__host__ __device__ inline void line_pass(int n, double w, Io& io, Stack& stack) {
  int q = -1, tk = 0, tv = 0, tt = 0;        // the top of the stack, in registers
  double tg = 0.0;
  for (int k = 0; k < n; ++k) {
    const int v = io.load(k);
    if (v < 0) continue;
    const double g = io.floor(v);
    while (q >= 0 && cost(g, k, tt, w) < cost(tg, tk, tt, w)) {
      if (--q >= 0) {
        stack.get(q, tk, tv, tt);
        tg = io.floor(tv);
      }
    }
    if (q < 0) {
      q = 0; tk = k; tv = v; tt = 0; tg = g;
      stack.put(0, k, v, 0);
    } else {
      const int t = first_below(tg, tk, g, k, w, tt + 1, n);
      if (t < n) {
        ++q; tk = k; tv = v; tt = t; tg = g;
        stack.put(q, k, v, t);
      }
    }
  }
  if (q < 0) {
    for (int p = 0; p < n; ++p) io.store_none(p);
    return;
  }
  for (int p = n - 1; p >= 0; --p) {
    io.store(p, tk, tv);
    if (p == tt && --q >= 0) stack.get(q, tk, tv, tt);
  }
}

__host__ __device__ inline int32_t float_bits(float f) {
  int32_t b;
  memcpy(&b, &f, sizeof(b));
  return b;
}

// The line of the y pass at (z, x): entries are the x pass's x' (or -1), the result y' * X + x'.
struct YLine {
  int32_t* line;           // at (z, 0, x)
  int64_t stride;          // X
  int x, X;
  double wx;
  __host__ __device__ int load(int k) const { return line[k * stride]; }
  __host__ __device__ double floor(int v) const { return cost(0.0, v, x, wx); }
  __host__ __device__ void store(int p, int k, int v) { line[p * stride] = k * X + v; }
  __host__ __device__ void store_none(int p) { line[p * stride] = -1; }
};

// The line of the z pass at (y, x): entries are the y pass's y' * X + x' (or -1), the results the linear index and the distance.
struct ZLine {
  int32_t* line;           // at (0, y, x); the entries, and `nearest` where it is asked for
  int32_t* nearest;        // at (0, y, x), or NULL
  int32_t* dist;           // at (0, y, x), or NULL: the float32's bits (may be the same words as `line`)
  int64_t stride;          // Y * X
  int y, x, X;
  Sampling s;
  __host__ __device__ int load(int k) const { return line[k * stride]; }
  __host__ __device__ double floor(int v) const {
    const double dy = static_cast<double>(y - v / X), dx = static_cast<double>(x - v % X);
    return s.wy * (dy * dy) + s.wx * (dx * dx);
  }
  __host__ __device__ void store(int p, int k, int v) {
    if (nearest != nullptr) nearest[p * stride] = static_cast<int32_t>(k * stride + v);
    if (dist != nullptr) dist[p * stride] = float_bits(static_cast<float>(distance(s, p - k, y - v / X, x - v % X)));
  }
  __host__ __device__ void store_none(int p) {
    if (nearest != nullptr) nearest[p * stride] = -1;
    if (dist != nullptr) dist[p * stride] = 0x7f800000;          // +inf
  }
};

}  // namespace edt
}  // namespace lsr
