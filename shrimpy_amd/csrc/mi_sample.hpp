// The per-sample rule of the mutual-information metric, ONE definition for the kernels (estimate_mi.hip) and their host
// twins (estimators_host.hip).  The joint histogram is pinned bit for bit between the two sides, so "the same arithmetic"
// is the text below: plain fp64 operators, every product, sum and quotient rounded on its own -- no fma anywhere (the
// library is built with -ffp-contract=off and the pragma below repeats it where it matters).
//
// Conventions of estimate_affine.hip: a 3x4 matrix maps a target index to a moving coordinate, in float64; the target
// grid is sampled every stride[axis] voxels; a sample counts when its moving coordinate lies in [0, n - 1) on every axis
// (all eight taps inside the moving volume); the interpolant is lerped along x, then y, then z.
//
// Binning (Mattes: zero-order on the target, a linear Parzen window on the moving intensity):
//     a  = clamp(floor((double(t) - t_lo) * bins / (t_hi - t_lo)), 0, bins - 1)
//     u  = clamp((m - m_lo) * (bins - 1) / (m_hi - m_lo), 0, bins - 1)           (both left to right)
//     b0 = min(floor(u), bins - 2),  f = u - b0
//     w1 = floor(f * 65536 + 0.5),   w0 = 65536 - w1      -> cell (a, b0) += w0, cell (a, b0 + 1) += w1
// The weights are integers in units of 2^-16 sample: sums are exact and do not depend on their order.
//
// Gradient: a sample contributes when its unclamped u lies strictly inside (0, bins - 1); a sample whose u is exactly 0
// or exactly bins - 1 counts as clamped and contributes nothing (tests/mi_ref.py states the same rule).
//
// Values that are not finite.  The lerp is IEEE arithmetic as written: a NaN tap makes m NaN, and so does an infinite
// tap, whatever its fraction (0 * inf, inf - inf).  The clamps are written as comparisons that a NaN fails:
//     target:  NaN -> bin 0,  -inf -> bin 0,  +inf -> bin bins - 1
//     moving:  u NaN -> u = 0 (b0 = 0, w1 = 0: the whole weight in column 0; no gradient term),
//              u = -inf -> 0,  u = +inf -> bins - 1 (b0 = bins - 2, w1 = 65536; no gradient term either)
// A sample with such a value is still counted: the count depends on the coordinates alone.
#pragma once

#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace lsr {
namespace mi {

constexpr int kMinBins = 4;
constexpr int kMaxBins = 64;
constexpr int kWeightOne = 65536;   // one sample in histogram units
constexpr int kGradParams = 12;

struct Geometry {
  const float* moving;
  const float* target;
  int Zi, Yi, Xi;
  int Zo, Yo, Xo;
  double m[12];
  int sz, sy, sx;        // sampling stride per axis
  int nz, ny, nx;        // sampled grid: indices 0, stride, 2 stride, ... below Zo / Yo / Xo
};

struct Binning {
  int bins;
  double t_lo, t_range;  // t_hi - t_lo
  double m_lo, m_range;  // m_hi - m_lo
};

// One sample of the strided target grid: its target value and the trilinear moving value; GRAD adds the interpolant's
// analytic gradient (z, y, x) and the target index as doubles.  false = the moving coordinate is outside [0, n - 1).
template <bool GRAD>
__host__ __device__ __forceinline__ bool sample(const Geometry& p, int64_t s, double& tv, double& mval, double* g,
                                                double* xyz) {
#pragma clang fp contract(off)
  const int ix = static_cast<int>(s % p.nx);
  const int64_t r = s / p.nx;
  const int iy = static_cast<int>(r % p.ny), iz = static_cast<int>(r / p.ny);
  const int zo = iz * p.sz, yo = iy * p.sy, xo = ix * p.sx;
  const double zd = zo, yd = yo, xd = xo;
  const double cz = p.m[0] * zd + p.m[1] * yd + p.m[2] * xd + p.m[3];
  const double cy = p.m[4] * zd + p.m[5] * yd + p.m[6] * xd + p.m[7];
  const double cx = p.m[8] * zd + p.m[9] * yd + p.m[10] * xd + p.m[11];
  if (!(cz >= 0.0 && cz < p.Zi - 1 && cy >= 0.0 && cy < p.Yi - 1 && cx >= 0.0 && cx < p.Xi - 1)) return false;
  const int jz = static_cast<int>(cz), jy = static_cast<int>(cy), jx = static_cast<int>(cx);
  const double fz = cz - jz, fy = cy - jy, fx = cx - jx;
  const int64_t plane_i = static_cast<int64_t>(p.Yi) * p.Xi;
  const float* base = p.moving + jz * plane_i + static_cast<int64_t>(jy) * p.Xi + jx;
  const double v000 = base[0], v001 = base[1], v010 = base[p.Xi], v011 = base[p.Xi + 1];
  const double v100 = base[plane_i], v101 = base[plane_i + 1], v110 = base[plane_i + p.Xi],
               v111 = base[plane_i + p.Xi + 1];
  tv = p.target[(static_cast<int64_t>(zo) * p.Yo + yo) * p.Xo + xo];
  // lerp along x, then y, then z
  const double a00 = v000 + fx * (v001 - v000), a01 = v010 + fx * (v011 - v010);
  const double a10 = v100 + fx * (v101 - v100), a11 = v110 + fx * (v111 - v110);
  const double b0 = a00 + fy * (a01 - a00), b1 = a10 + fy * (a11 - a10);
  mval = b0 + fz * (b1 - b0);
  if constexpr (GRAD) {
    g[0] = b1 - b0;
    g[1] = (a01 - a00) + fz * ((a11 - a10) - (a01 - a00));
    const double d00 = v001 - v000, d01 = v011 - v010, d10 = v101 - v100, d11 = v111 - v110;
    const double e0 = d00 + fy * (d01 - d00), e1 = d10 + fy * (d11 - d10);
    g[2] = e0 + fz * (e1 - e0);
    xyz[0] = zd; xyz[1] = yd; xyz[2] = xd;
  }
  return true;
}

__host__ __device__ __forceinline__ int target_bin(const Binning& q, double tv) {
#pragma clang fp contract(off)
  const double a = floor((tv - q.t_lo) * q.bins / q.t_range);
  // (written so that a NaN lands in bin 0 on both sides)
  return a >= q.bins - 1 ? q.bins - 1 : (a > 0.0 ? static_cast<int>(a) : 0);
}

// the unclamped position of a moving value on the bin axis
__host__ __device__ __forceinline__ double moving_position(const Binning& q, double mval) {
#pragma clang fp contract(off)
  return (mval - q.m_lo) * (q.bins - 1) / q.m_range;
}

// lower bin and the weight (units of 2^-16) of the upper bin; the lower bin's is kWeightOne - w1
__host__ __device__ __forceinline__ void parzen(const Binning& q, double u_raw, int& b0, unsigned& w1) {
#pragma clang fp contract(off)
  const double top = q.bins - 1;
  const double u = u_raw >= top ? top : (u_raw > 0.0 ? u_raw : 0.0);   // (a NaN fails both: 0)
  const int fl = static_cast<int>(floor(u));
  b0 = fl < q.bins - 2 ? fl : q.bins - 2;
  const double f = u - b0;
  w1 = static_cast<unsigned>(floor(f * 65536.0 + 0.5));
}

struct Normalise {
  double cz, cy, cx, inv_s;   // x~ = ((x - c) * inv_s, 1)
};

// One sample's term of the gradient sums: dL[a][b0] * (bins - 1) / (m_hi - m_lo) * (dM/dz, dM/dy, dM/dx) (x) x~, added
// to acc[12] (the matrix row by row).  `dl` is [bins][bins - 1]; `du` = (bins - 1) / (m_hi - m_lo).
__host__ __device__ __forceinline__ void gradient_add(const Binning& q, const Normalise& c, const double* dl, double du,
                                                      double tv, double mval, const double g[3], const double xyz[3],
                                                      double acc[kGradParams]) {
#pragma clang fp contract(off)
  const double u = moving_position(q, mval);
  if (!(u > 0.0 && u < q.bins - 1)) return;   // clamped (or exactly on an end of the range): no contribution
  const int a = target_bin(q, tv);
  const int fl = static_cast<int>(floor(u));
  const int b0 = fl < q.bins - 2 ? fl : q.bins - 2;
  const double w = dl[a * (q.bins - 1) + b0] * du;
  const double xt[4] = {(xyz[0] - c.cz) * c.inv_s, (xyz[1] - c.cy) * c.inv_s, (xyz[2] - c.cx) * c.inv_s, 1.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double wg = w * g[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[4 * i + j] += wg * xt[j];
  }
}

// the checks the four entries share (those of lsr_affine_normal_equations_f32, then the binning's)
inline int require_sampling(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target, int64_t Zo,
                            int64_t Yo, int64_t Xo, const double M[12], const int stride[3], int bins, double t_lo,
                            double t_hi, double m_lo, double m_hi) {
  LSR_REQUIRE_PTR(moving);
  LSR_REQUIRE_PTR(target);
  LSR_REQUIRE_PTR(M);
  LSR_REQUIRE(Zi >= 2 && Yi >= 2 && Xi >= 2, LSR_E_SHAPE, "moving shape (%lld,%lld,%lld): every axis needs two samples",
              (long long)Zi, (long long)Yi, (long long)Xi);
  LSR_REQUIRE(Zo > 0 && Yo > 0 && Xo > 0, LSR_E_SHAPE, "target shape (%lld,%lld,%lld) must be positive", (long long)Zo,
              (long long)Yo, (long long)Xo);
  LSR_REQUIRE_VOLUME(Zo, Yo, Xo);
  LSR_REQUIRE_VOLUME(Zi, Yi, Xi);
  LSR_REQUIRE_PTR(stride);
  LSR_REQUIRE(stride[0] >= 1 && stride[1] >= 1 && stride[2] >= 1, LSR_E_ARG, "strides must be >= 1, got (%d,%d,%d)",
              stride[0], stride[1], stride[2]);
  for (int i = 0; i < 12; ++i) LSR_REQUIRE(M[i] == M[i] && M[i] - M[i] == 0.0, LSR_E_ARG, "M[%d] is not finite", i);
  LSR_REQUIRE(bins >= kMinBins && bins <= kMaxBins, LSR_E_ARG, "bins %d outside [%d, %d]", bins, kMinBins, kMaxBins);
  LSR_REQUIRE(t_hi > t_lo && t_hi - t_lo < INFINITY, LSR_E_ARG, "target range [%g, %g] is empty or not finite", t_lo, t_hi);
  LSR_REQUIRE(m_hi > m_lo && m_hi - m_lo < INFINITY, LSR_E_ARG, "moving range [%g, %g] is empty or not finite", m_lo, m_hi);
  return LSR_OK;
}

inline void fill(Geometry& p, Binning& q, const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target,
                 int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], const int stride[3], int bins, double t_lo,
                 double t_hi, double m_lo, double m_hi) {
  p.moving = moving; p.target = target;
  p.Zi = static_cast<int>(Zi); p.Yi = static_cast<int>(Yi); p.Xi = static_cast<int>(Xi);
  p.Zo = static_cast<int>(Zo); p.Yo = static_cast<int>(Yo); p.Xo = static_cast<int>(Xo);
  for (int i = 0; i < 12; ++i) p.m[i] = M[i];
  p.sz = stride[0]; p.sy = stride[1]; p.sx = stride[2];
  p.nz = static_cast<int>(ceil_div(Zo, stride[0]));
  p.ny = static_cast<int>(ceil_div(Yo, stride[1]));
  p.nx = static_cast<int>(ceil_div(Xo, stride[2]));
  q.bins = bins;
  q.t_lo = t_lo; q.t_range = t_hi - t_lo;
  q.m_lo = m_lo; q.m_range = m_hi - m_lo;
}

}  // namespace mi
}  // namespace lsr
