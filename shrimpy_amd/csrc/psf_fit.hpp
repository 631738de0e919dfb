// What the per-bead Gaussian fit and the Fourier-shifted PSF average (psf_fit.hip) share with their host twins
// (host_twins.hip): the argument checks, the model and its Jacobian, and the Levenberg-Marquardt steps that one lane
// (or the host) takes between the passes over the patch.  tests/psf_fit_ref.py restates all of it in NumPy / float64.
//
// Model on the patch around a centre voxel, r = the voxel offset from it:
//     m(r) = B + A exp(-1/2 (r - mu)^T W (r - mu)),     W symmetric 3 x 3
// parameters  theta = (B, A, mu_z, mu_y, mu_x, w_zz, w_yy, w_xx, w_zy, w_zx, w_yx),  unweighted least squares.
//
// Start.  B0 = the mean of the patch's six faces (bead_stats_kernel's sum), A0 = d(0) - B0.  With g = max(d - B0 - A0 / 2,
// 0) -- the part of the bead above its half maximum -- mu0 = sum(g r) / sum(g), and per axis s_i^2 = sum(g (r_i - mu0_i)^2)
// / sum(g).  For a Gaussian cut at its half maximum that second moment is kHalfMaxMoment sigma_i^2 (the radial integrals
// of (exp(-q^2 / 2) - 1/2) q^4 and q^2 over q < sqrt(2 ln 2), a third of their ratio), so W0 = diag(kHalfMaxMoment /
// max(s_i^2, kHalfMaxMoment / 4)): sigma0 is never below half a voxel, which is what a bead with one voxel above its
// half maximum gets.
//
// Iteration, all float64.  One pass over the patch gives J^T J (66 sums), J^T r and the cost at theta.  Then
//     solve  (J^T J + lambda diag(J^T J)) delta = J^T r   by Cholesky (in the scaled form D^-1 J^T J D^-1 + lambda I,
//     D = sqrt(diag)),  trial = theta + delta,  a second pass gives the trial cost;
//     trial cost <= cost: accept, lambda / 10;  otherwise reject, lambda * 10 and solve again with the same sums.
// lambda starts at 1e-3.  The fit has converged when a step moves every mu by less than 1e-9 voxel and the cost by at most
// 1e-12 of itself -- an accepted step, or a rejected one (theta is then kept: at the minimum the sign of a cost difference
// of that size is rounding).  It stops without converging after max_iter trial cost evaluations.
//
// Status: 0 converged; 1 iteration limit; 2 the damped system, or W at the end, is not positive definite; 3 some |mu_i|
// >= 1; 4 A <= 0 (at the start: A0 <= 0, nothing to fit); 5 a non-finite voxel in the patch, or the patch does not fit
// the volume.  Every status but 0 leaves NaN in the bead's twelve outputs.
#pragma once

#include <cmath>

#include "peaks.hpp"

namespace lsr {
namespace psffit {

constexpr int kParams = 11;
constexpr int kNormal = kParams * (kParams + 1) / 2;    // 66: the lower triangle of J^T J, row by row
constexpr int kSums = kNormal + kParams + 1;            // + J^T r + the cost
constexpr int kFitOut = kParams + 1;                    // per bead: theta, then the final sum of squared residuals
constexpr int kStartSums = 7;                           // sum g, sum g r (3), sum g r^2 (3)
constexpr int kShiftBatch = 64;                         // beads whose shifted patches the scratch holds at a time
constexpr double kHalfMaxMoment = 0.1888664644521538;  // see above
constexpr double kLambda0 = 1e-3, kMuTol = 1e-9, kCostTol = 1e-12;

enum Param { kB, kA, kMz, kMy, kMx, kWzz, kWyy, kWxx, kWzy, kWzx, kWyx };
enum Status { kConverged = 0, kIterLimit = 1, kNotPosDef = 2, kOffCentre = 3, kNoAmplitude = 4, kBadInput = 5 };
enum Action { kDone = 0, kNeedSums = 1, kNeedSolve = 2 };

// What the lane that steers the fit keeps (LDS on the device).
struct Lm {
  double theta[kParams];
  double trial[kParams];
  double sums[kSums];                // at theta
  double chol[kParams * kParams];    // the solver's work space
  double scale[kParams];
  double lambda, cost;
  int evals, max_iter, status;
};

// One voxel's share of the sums at parameters t: value v at offset (rz, ry, rx).  FULL: s[0..65] += J_i J_j (j <= i),
// s[66..76] += J_i res, s[77] += res^2; otherwise the cost alone.  Every index is a constant after unrolling.
template <bool FULL>
__host__ __device__ __forceinline__ void add_voxel(const double (&t)[kParams], double v, double rz, double ry, double rx,
                                                   double (&s)[kSums]) {
  const double dz = rz - t[kMz], dy = ry - t[kMy], dx = rx - t[kMx];
  const double uz = t[kWzz] * dz + t[kWzy] * dy + t[kWzx] * dx;
  const double uy = t[kWzy] * dz + t[kWyy] * dy + t[kWyx] * dx;
  const double ux = t[kWzx] * dz + t[kWyx] * dy + t[kWxx] * dx;
  const double e = exp(-0.5 * (dz * uz + dy * uy + dx * ux));
  const double res = v - (t[kB] + t[kA] * e);
  s[kSums - 1] += res * res;
  if constexpr (FULL) {
    const double ae = t[kA] * e;
    const double J[kParams] = {1.0, e, ae * uz, ae * uy, ae * ux, -0.5 * ae * dz * dz, -0.5 * ae * dy * dy,
                               -0.5 * ae * dx * dx, -ae * dz * dy, -ae * dz * dx, -ae * dy * dx};
#pragma unroll
    for (int i = 0; i < kParams; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) s[i * (i + 1) / 2 + j] += J[i] * J[j];
      s[kNormal + i] += J[i] * res;
    }
  }
}

// theta0 from the face mean, the centre voxel and the seven moment sums; false (status set) when there is nothing to fit
__host__ __device__ inline bool lm_start(Lm& lm, double bg, double centre, const double* m, int max_iter) {
  lm.lambda = kLambda0;
  lm.evals = 0;
  lm.max_iter = max_iter;
  lm.status = kConverged;
  lm.cost = 0.0;
  const double amp = centre - bg;
  if (!(amp > 0.0) || !(m[0] > 0.0)) {
    lm.status = kNoAmplitude;
    return false;
  }
  lm.theta[kB] = bg;
  lm.theta[kA] = amp;
  for (int i = 0; i < 3; ++i) {
    const double mu = m[1 + i] / m[0], var = m[4 + i] / m[0] - mu * mu;
    lm.theta[kMz + i] = mu;
    lm.theta[kWzz + i] = kHalfMaxMoment / (var > 0.25 * kHalfMaxMoment ? var : 0.25 * kHalfMaxMoment);
  }
  lm.theta[kWzy] = lm.theta[kWzx] = lm.theta[kWyx] = 0.0;
  return true;
}

// trial = theta + delta from the sums at theta and the current lambda; false (status 2) when the system is not
// positive definite
__host__ __device__ inline bool lm_solve(Lm& lm) {
  constexpr int n = kParams;
  double* a = lm.chol;
  for (int i = 0; i < n; ++i) {
    const double d = lm.sums[i * (i + 1) / 2 + i];
    if (!(d > 0.0) || !(d < 1e300)) {
      lm.status = kNotPosDef;
      return false;
    }
    lm.scale[i] = sqrt(d);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j)
      a[i * n + j] = lm.sums[i * (i + 1) / 2 + j] / (lm.scale[i] * lm.scale[j]) + (i == j ? lm.lambda : 0.0);
  for (int i = 0; i < n; ++i) {          // Cholesky, row by row, in place (lower triangle)
    for (int j = 0; j <= i; ++j) {
      double acc = a[i * n + j];
      for (int k = 0; k < j; ++k) acc -= a[i * n + k] * a[j * n + k];
      if (i == j) {
        if (!(acc > 0.0)) {
          lm.status = kNotPosDef;
          return false;
        }
        a[i * n + i] = sqrt(acc);
      } else {
        a[i * n + j] = acc / a[j * n + j];
      }
    }
  }
  double* y = lm.trial;
  for (int i = 0; i < n; ++i) {          // L y = D^-1 J^T r
    double acc = lm.sums[kNormal + i] / lm.scale[i];
    for (int k = 0; k < i; ++k) acc -= a[i * n + k] * y[k];
    y[i] = acc / a[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {     // L^T x = y
    double acc = y[i];
    for (int k = i + 1; k < n; ++k) acc -= a[k * n + i] * y[k];
    y[i] = acc / a[i * n + i];
  }
  for (int i = 0; i < n; ++i) lm.trial[i] = lm.theta[i] + y[i] / lm.scale[i];
  return true;
}

// the verdict on a trial cost: what the fit needs next
__host__ __device__ inline int lm_judge(Lm& lm, double trial_cost) {
  ++lm.evals;
  double dmu = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double d = fabs(lm.trial[kMz + i] - lm.theta[kMz + i]);
    dmu = d > dmu ? d : dmu;
  }
  const bool small = dmu < kMuTol && fabs(lm.cost - trial_cost) <= kCostTol * lm.cost;
  int next;
  if (trial_cost <= lm.cost) {
    for (int i = 0; i < kParams; ++i) lm.theta[i] = lm.trial[i];
    lm.cost = trial_cost;
    lm.lambda = lm.lambda > 1e-14 ? lm.lambda / 10.0 : lm.lambda;
    next = kNeedSums;
  } else {
    lm.lambda *= 10.0;
    next = kNeedSolve;
  }
  if (small) return kDone;
  if (lm.evals >= lm.max_iter) {
    lm.status = kIterLimit;
    return kDone;
  }
  return next;
}

// status of a fit that ended (checks of the final parameters) and the bead's twelve outputs
__host__ __device__ inline int lm_finish(Lm& lm, double* out) {
  if (lm.status == kConverged) {
    const double* t = lm.theta;
    bool finite = true;
    for (int i = 0; i < kParams; ++i) finite = finite && fabs(t[i]) < 1e300;     // (false for a NaN)
    const double m2 = t[kWzz] * t[kWyy] - t[kWzy] * t[kWzy];
    const double det = t[kWzz] * (t[kWyy] * t[kWxx] - t[kWyx] * t[kWyx]) - t[kWzy] * (t[kWzy] * t[kWxx] - t[kWyx] * t[kWzx]) +
                       t[kWzx] * (t[kWzy] * t[kWyx] - t[kWyy] * t[kWzx]);
    if (!finite || !(t[kWzz] > 0.0) || !(m2 > 0.0) || !(det > 0.0)) lm.status = kNotPosDef;      // Sylvester
    else if (!(fabs(t[kMz]) < 1.0 && fabs(t[kMy]) < 1.0 && fabs(t[kMx]) < 1.0)) lm.status = kOffCentre;
    else if (!(t[kA] > 0.0)) lm.status = kNoAmplitude;
  }
  const double nan = __builtin_nan("");
  for (int i = 0; i < kParams; ++i) out[i] = lm.status == kConverged ? lm.theta[i] : nan;
  out[kParams] = lm.status == kConverged ? lm.cost : nan;
  return lm.status;
}

inline int check_bead_fit(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n, int pz,
                          int py, int px, int max_iter, const double* fit, const int* status) {
  LSR_REQUIRE_PTR(vol);
  LSR_REQUIRE_PTR(centres);
  LSR_REQUIRE_PTR(fit);
  LSR_REQUIRE_PTR(status);
  if (int rc = lsr::peaks::check_patches(Z, Y, X, n, pz, py, px)) return rc;
  LSR_REQUIRE(max_iter >= 1, LSR_E_ARG, "max_iter %d must be positive", max_iter);
  return LSR_OK;
}

// scratch of the shifted average: the float64 accumulator, the running count and the batch's flags, then two float64
// patches per bead of a batch
inline int64_t shift_head_doubles(int64_t nvox) { return nvox + 1 + kShiftBatch; }
inline int64_t shift_scratch_bytes(int64_t n, int pz, int py, int px) {
  const int64_t nvox = int64_t(pz) * py * px, batch = n < kShiftBatch ? n : kShiftBatch;
  return (shift_head_doubles(nvox) + 2 * batch * nvox) * static_cast<int64_t>(sizeof(double));
}

inline int check_psf_shift(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n, int pz,
                           int py, int px, const double* bead_stats, const double* weights, const float* psf) {
  LSR_REQUIRE_PTR(weights);
  return lsr::peaks::check_psf_accumulate(vol, Z, Y, X, centres, n, pz, py, px, bead_stats, psf);
}

// one circulant pass along an axis of length N: out[i] = sum_j in[j] w[(i - j) mod N], j ascending, unfused
template <typename TIn>
__host__ __device__ __forceinline__ double circulant(const TIn* in, int64_t stride, double sub, const double* w, int N,
                                                     int i) {
  double acc = 0.0;
  int k = i;                                   // (i - j) mod N, walking down from i and wrapping to N - 1
  for (int j = 0; j < N; ++j) {
    acc += (static_cast<double>(in[j * stride]) - sub) * w[k];
    k = k == 0 ? N - 1 : k - 1;
  }
  return acc;
}

}  // namespace psffit
}  // namespace lsr
