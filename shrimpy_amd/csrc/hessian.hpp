// What the Hessian-eigenvalue kernel (hessian.hip) and its host twin (host_twins.hip) share: the rule, the entry check, the
// edge-aware derivative, the six Hessian entries, the eigen solver, the response switch, the NaN rule and the store -- ONE
// definition, so that the two sides give the same bits.
//
// Rule.  g is a contiguous (Z, Y, X) float32 volume, already smoothed; s = (sz, sy, sx) the sampling; `scale` a double (the
// Python layer passes sigma^2).  PINNED to numpy: np.gradient twice and np.linalg.eigvalsh, which is what
// skimage.feature.hessian_matrix(use_gaussian_derivatives=False) and hessian_matrix_eigvals compute (tests/hessian_ref.py).
//   Derivative.  D_a f along an axis of length n is np.gradient's: the central difference over 2 s_a inside, the one-sided
//   difference over s_a at i = 0 and at i = n - 1; for n = 1 it is 0 (numpy raises there: this package's rule).
//   Hessian.  H_ab = D_b (D_a g) for a <= b, in float64 from the float32 g.  At the volume's faces the one-sided forms compose
//   as numpy composes them: the form of each difference follows from the index of the voxel it is taken at, never from a
//   clamped load, and no position outside the volume is read.  The divisions by s_a and 2 s_a are multiplications by their
//   float64 reciprocals (exact under dyadic sampling, otherwise within 2^-52 of numpy's quotient, relative to each difference).
//   Eigenvalues.  l1 <= l2 <= l3 of H, with dark = 1 of -H; e_k = float32(scale * l_k).
//   Responses, bit-exact float32 functions of (e1, e2, e3); m_k = (-e_k > 0) ? -e_k : +0, so that m1 >= m2 >= m3 >= 0:
//     0, 1, 2  e1, e2, e3        3 ridge  m1        4 tube  sqrtf(m1 * m2)        5 sheet  m1 - m2        6 blob  m3
//     7 log  -((e1 + e2) + e3)
//   a NaN that this arithmetic makes (eigenvalues that overflowed float32) comes out as the canonical quiet NaN.
//   Non-finite input.  The stencil of a voxel is the set of voxels that the six entries read; if one of them is not finite,
//   every measure gives the canonical quiet NaN 0x7fc00000.  (Every value read enters a difference, so the stencil holds a
//   non-finite value exactly when one of the six entries is not finite: that is the test.)
//   Accumulation.  accumulate = 1 stores max(out, r): NaN if either is a NaN, else (out >= r) ? out : r -- np.maximum by
//   value; between -0.0 and +0.0 the stored one stays.  accumulate = 0 stores r.
//
// Solver.  Cyclic Jacobi in float64 on the six entries: rotations (0,1), (0,2), (1,2) per sweep, each from one square root and
// one division for the tangent and one of each for the cosine -- only operations that IEEE 754 rounds correctly, so host and
// device agree to the bit; no library function of an angle.  A rotation keeps ||H||_F, and by Weyl's inequality the diagonal
// is within sqrt(2 * off) of the eigenvalues, off = a01^2 + a02^2 + a12^2: the sweeps stop at off <= 2^-64 ||H||_F^2, which is
// 2^-31.5 ||H||_F, 0.0055 units of 2^-24 ||H||_F.  Convergence is quadratic: four sweeps at the most on everything
// tests/hessian_cases.py holds, kMaxSweeps is a ceiling that is never reached.  A diagonal H takes no rotation: exact.
#pragma once

#include <cmath>

#include "common.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSR_HD __host__ __device__
#else
#define LSR_HD
#endif

namespace lsr {
namespace hessian {

constexpr int kHalo = 2;                                  // the straight second derivative reaches two voxels
constexpr int kTileZ = 8, kTileY = 8, kTileX = 64;        // outputs per workgroup; x on the lanes of a wavefront
constexpr int kThreads = 256;
constexpr int kEdgeZ = kTileZ + 2 * kHalo, kEdgeY = kTileY + 2 * kHalo, kEdgeX = kTileX + 2 * kHalo;
constexpr int kTileFloats = kEdgeZ * kEdgeY * kEdgeX;     // 12 x 12 x 68 floats = 39,168 bytes: four workgroups per compute unit
static_assert(kTileFloats * 4 <= 64 * 1024, "the halo'd tile must fit in the LDS a launch gets without asking");
static_assert(kTileX == kWave && kEdgeX <= 2 * kWave, "a wavefront takes one row of the tile at a time");
constexpr int kMeasures = 8;
constexpr int kMaxSweeps = 12;
constexpr double kOffTolerance = 5.42101086242752217e-20;   // 2^-64, against ||H||_F^2

enum Measure { kE1 = 0, kE2 = 1, kE3 = 2, kRidge = 3, kTube = 4, kSheet = 5, kBlob = 6, kLog = 7 };

// One axis at a voxel: its index, the axis length, 1 / s and 1 / (2 s).
struct Axis {
  int64_t i, n;
  double inv1, inv2;
};

// The reciprocals of one launch, computed once on the host: 1 / s_a and 1 / (2 s_a) for a = z, y, x.
struct Recip {
  double inv1[3], inv2[3];
};
inline Recip recip_of(double sz, double sy, double sx) {
  return Recip{{1.0 / sz, 1.0 / sy, 1.0 / sx}, {1.0 / (2.0 * sz), 1.0 / (2.0 * sy), 1.0 / (2.0 * sx)}};
}

LSR_HD inline float canonical_nan() { return __builtin_nanf(""); }   // 0x7fc00000

// np.gradient at index j of an axis of length n > 1: the difference f[j + hi] - f[j + lo] times `weight`
LSR_HD inline void ends(int64_t j, int64_t n, int& lo, int& hi) {
  lo = j > 0 ? -1 : 0;
  hi = j < n - 1 ? 1 : 0;
}
LSR_HD inline double weight(const Axis& a, int lo, int hi) { return hi - lo == 2 ? a.inv2 : a.inv1; }

// H_AB = D_B (D_A g) at the voxel; g(dz, dy, dx) is the value at that offset from it and is only called inside the volume.
template <int A, int B, class Load>
LSR_HD inline double second(Load& g, const Axis (&ax)[3]) {
  const Axis a = ax[A], b = ax[B];
  if (a.n == 1 || b.n == 1) return 0.0;
  int blo, bhi;
  ends(b.i, b.n, blo, bhi);
  auto first = [&](int k) {                              // D_A g at the voxel moved by k along B
    int alo, ahi;
    ends(a.i + (A == B ? k : 0), a.n, alo, ahi);
    const int kz = B == 0 ? k : 0, ky = B == 1 ? k : 0, kx = B == 2 ? k : 0;
    const double up = g(kz + (A == 0 ? ahi : 0), ky + (A == 1 ? ahi : 0), kx + (A == 2 ? ahi : 0));
    const double down = g(kz + (A == 0 ? alo : 0), ky + (A == 1 ? alo : 0), kx + (A == 2 ? alo : 0));
    return (up - down) * weight(a, alo, ahi);
  };
  return (first(bhi) - first(blo)) * weight(b, blo, bhi);
}

// h = {zz, yy, xx, zy, zx, yx}
template <class Load>
LSR_HD inline void entries(Load& g, const Axis (&ax)[3], double (&h)[6]) {
  h[0] = second<0, 0>(g, ax);
  h[1] = second<1, 1>(g, ax);
  h[2] = second<2, 2>(g, ax);
  h[3] = second<0, 1>(g, ax);
  h[4] = second<0, 2>(g, ax);
  h[5] = second<1, 2>(g, ax);
}

LSR_HD inline bool finite(double v) { return v - v == 0.0; }

// One Jacobi rotation that annihilates a_pq; r is the third index.
LSR_HD inline void rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  if (apq == 0.0) return;
  const double d = aqq - app;
  const double hyp = sqrt(d * d + 4.0 * apq * apq);
  if (!(hyp > 0.0)) return;                                // (both squares underflowed: nothing to rotate by)
  const double t = (d >= 0.0 ? 2.0 * apq : -2.0 * apq) / (fabs(d) + hyp);
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double p = c * arp - s * arq, q = s * arp + c * arq;
  arp = p;
  arq = q;
}

// The eigenvalues of the symmetric matrix h, ascending.
LSR_HD inline void eigenvalues(const double (&h)[6], double& l1, double& l2, double& l3) {
  double a00 = h[0], a11 = h[1], a22 = h[2], a01 = h[3], a02 = h[4], a12 = h[5];
  const double stop = kOffTolerance * (a00 * a00 + a11 * a11 + a22 * a22 + 2.0 * (a01 * a01 + a02 * a02 + a12 * a12));
#pragma unroll 1
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    if (a01 * a01 + a02 * a02 + a12 * a12 <= stop) break;
    rotate(a00, a11, a01, a02, a12);
    rotate(a00, a22, a02, a01, a12);
    rotate(a11, a22, a12, a01, a02);
  }
  double lo = a00 < a11 ? a00 : a11, hi = a00 < a11 ? a11 : a00;
  const double mid = a22 < lo ? lo : (a22 < hi ? a22 : hi);
  l1 = a22 < lo ? a22 : lo;
  l3 = a22 < hi ? hi : a22;
  l2 = mid;
}

// The float32 response of the three float32 eigenvalue outputs.
LSR_HD inline float response(float e1, float e2, float e3, int measure) {
  const float m1 = -e1 > 0.0f ? -e1 : 0.0f, m2 = -e2 > 0.0f ? -e2 : 0.0f, m3 = -e3 > 0.0f ? -e3 : 0.0f;
  float r;
  switch (measure) {
    case kE1: r = e1; break;
    case kE2: r = e2; break;
    case kE3: r = e3; break;
    case kRidge: r = m1; break;
    case kTube: r = sqrtf(m1 * m2); break;
    case kSheet: r = m1 - m2; break;
    case kBlob: r = m3; break;
    default: r = -((e1 + e2) + e3); break;
  }
  return r == r ? r : canonical_nan();
}

// One voxel: the six entries through g, the NaN rule, the eigenvalues, the measure.
template <class Load>
LSR_HD inline float voxel(Load& g, const Axis (&ax)[3], double scale, int measure, int dark) {
  double h[6];
  entries(g, ax, h);
  if (!(finite(h[0]) && finite(h[1]) && finite(h[2]) && finite(h[3]) && finite(h[4]) && finite(h[5]))) return canonical_nan();
  if (dark)
    for (int k = 0; k < 6; ++k) h[k] = -h[k];
  double l1, l2, l3;
  eigenvalues(h, l1, l2, l3);
  return response(static_cast<float>(scale * l1), static_cast<float>(scale * l2), static_cast<float>(scale * l3), measure);
}

// The store under accumulate = 1: np.maximum(old, r) with a NaN made canonical.
LSR_HD inline float greater_of(float old, float r) {
  if (old != old || r != r) return canonical_nan();
  return old >= r ? old : r;
}

inline int check_hessian(const float* g, const float* out, int64_t Z, int64_t Y, int64_t X, double sz, double sy, double sx,
                         double scale, int measure, int dark, int accumulate) {
  LSR_REQUIRE_PTR(g);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(g != out, LSR_E_ARG, "out must not alias g");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(Z * Y * X <= int64_t(2147483647), LSR_E_UNSUPPORTED, "%lld voxels: at most 2^31 - 1", (long long)(Z * Y * X));
  LSR_REQUIRE(sz > 0.0 && sy > 0.0 && sx > 0.0 && std::isfinite(sz) && std::isfinite(sy) && std::isfinite(sx), LSR_E_ARG,
              "sampling (%g,%g,%g) must be positive and finite", sz, sy, sx);
  LSR_REQUIRE(std::isfinite(scale), LSR_E_ARG, "scale %g must be finite", scale);
  LSR_REQUIRE(measure >= 0 && measure < kMeasures, LSR_E_ARG,
              "measure %d: 0 e1, 1 e2, 2 e3, 3 ridge, 4 tube, 5 sheet, 6 blob, 7 log", measure);
  LSR_REQUIRE(dark == 0 || dark == 1, LSR_E_ARG, "dark %d: 0 or 1", dark);
  LSR_REQUIRE(accumulate == 0 || accumulate == 1, LSR_E_ARG, "accumulate %d: 0 or 1", accumulate);
  return LSR_OK;
}

// One voxel on the host: the loads go to the volume itself.
inline float voxel_host(const float* g, int64_t Z, int64_t Y, int64_t X, int64_t z, int64_t y, int64_t x, const Recip& rc,
                        double scale, int measure, int dark) {
  const float* at = g + (z * Y + y) * X + x;
  auto load = [&](int dz, int dy, int dx) { return static_cast<double>(at[(dz * Y + dy) * X + dx]); };
  const Axis ax[3] = {{z, Z, rc.inv1[0], rc.inv2[0]}, {y, Y, rc.inv1[1], rc.inv2[1]}, {x, X, rc.inv1[2], rc.inv2[2]}};
  return voxel(load, ax, scale, measure, dark);
}

}  // namespace hessian
}  // namespace lsr
