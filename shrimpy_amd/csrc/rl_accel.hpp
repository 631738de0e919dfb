// What the kernels of rl_accel.hip and their host twins (host_twins.hip) share: the per-voxel arithmetic of the
// Biggs-Andrews extrapolation, the step length from the two inner products, the work split of the inner products and
// the argument checks.  See rl_accel.hip for the algorithm.
#pragma once

#include <cmath>

#include "common.hpp"

namespace lsr {
namespace accel {

// g_k = x_{k+1} - p_k, one float32 rounding
__host__ __device__ inline float change_of(float x1, float p) { return x1 - p; }

// a_{k+1} = clamp(<g_k, g_{k-1}> / <g_{k-1}, g_{k-1}>, 0, 1); 0 for a zero denominator (and for a quotient that is not
// a number).  Rounded to float32 once: that value is what every voxel is extrapolated with, and what is recorded.
__host__ __device__ inline float step_length(double num, double den) {
  if (den == 0.0) return 0.0f;
  const double q = num / den;
  if (!(q > 0.0)) return 0.0f;
  return static_cast<float>(q > 1.0 ? 1.0 : q);
}

// p_{k+1} = max(fma(a, x_{k+1} - x_k, x_{k+1}), 0); the comparison (not fmaxf) so that -0 and NaN give +0 on both sides
__host__ __device__ inline float predict_of(float a, float x1, float x0) {
  const float v = fmaf(a, x1 - x0, x1);
  return v > 0.0f ? v : 0.0f;
}
// the first step (a_1 = 0, nothing to extrapolate along yet): fma(0, ., x_1) = x_1, and x_0 is not read
__host__ __device__ inline float predict_first(float x1) { return x1 > 0.0f ? x1 : 0.0f; }

// Rows (z, y) are the unit of work.  The inner products are summed in `parts_of(rows)` parts -- workgroups on the device,
// row chunks on the host -- whose number depends on the shape alone, and the parts are added up in index order: the same
// bits from run to run, whatever the scheduling or the thread count.  2048 = 256 CUs x 8 workgroups of 256 threads, the
// residency a streaming kernel is sized for; beyond that the workgroups stride over the rows.
constexpr int kMaxParts = 2048;
inline int64_t parts_of(int64_t rows) { return rows < kMaxParts ? rows : kMaxParts; }

struct Vol {          // a strided (Z, Y, X) float32 volume: pitch and plane in elements
  const float* p;
  int64_t pitch, plane;
};

inline const float* end_of(const Vol& v, int64_t Z, int64_t Y, int64_t X) {
  return v.p + (Z - 1) * v.plane + (Y - 1) * v.pitch + X;
}

inline int check_shape(int64_t Z, int64_t Y, int64_t X) {
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  return LSR_OK;
}

inline int check_vol(const Vol& v, const char* name, int64_t Z, int64_t Y, int64_t X) {
  LSR_REQUIRE(v.p != nullptr, LSR_E_NULL, "%s is NULL", name);
  LSR_REQUIRE_STRIDES(v.pitch, v.plane);
  LSR_REQUIRE(v.pitch >= X, LSR_E_SHAPE, "%s: the row stride %lld is smaller than X = %lld", name, (long long)v.pitch,
              (long long)X);
  LSR_REQUIRE(Z == 1 || v.plane >= (Y - 1) * v.pitch + X, LSR_E_SHAPE, "%s: the plane stride %lld is smaller than the rows it holds",
              name, (long long)v.plane);
  return LSR_OK;
}

inline bool apart(const float* a, const float* a_end, const float* b, const float* b_end) {
  return a_end <= b || b_end <= a;
}

inline int check_dots(const Vol& x1, const Vol& p, const float* g, const double* dots2, int64_t Z, int64_t Y, int64_t X) {
  if (int rc = check_shape(Z, Y, X)) return rc;
  if (int rc = check_vol(x1, "x1", Z, Y, X)) return rc;
  if (int rc = check_vol(p, "p", Z, Y, X)) return rc;
  LSR_REQUIRE_PTR(g);
  LSR_REQUIRE_PTR(dots2);
  const float* g_end = g + Z * Y * X;
  LSR_REQUIRE(apart(g, g_end, x1.p, end_of(x1, Z, Y, X)) && apart(g, g_end, p.p, end_of(p, Z, Y, X)), LSR_E_ARG,
              "g overlaps x1 or p: it is written while they are read");
  return LSR_OK;
}

inline int check_predict(const Vol& x1, const Vol& x0, int64_t Z, int64_t Y, int64_t X) {
  if (int rc = check_shape(Z, Y, X)) return rc;
  if (int rc = check_vol(x1, "x1", Z, Y, X)) return rc;
  if (int rc = check_vol(x0, "x0", Z, Y, X)) return rc;
  LSR_REQUIRE(apart(x0.p, end_of(x0, Z, Y, X), x1.p, end_of(x1, Z, Y, X)), LSR_E_ARG,
              "x0 overlaps x1: the prediction is written over x0 while x1 is read");
  return LSR_OK;
}

}  // namespace accel
}  // namespace lsr
