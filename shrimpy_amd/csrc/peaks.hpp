// What the bead-detection / PSF-averaging kernels (peaks.hip) and their host twins (host_twins.hip) share: the
// argument checks, the peak test (the sink of the morphology's walk, morphology.hpp) and the fixed reduction tree of the
// per-bead sums.
#pragma once

#include <cmath>

#include "common.hpp"

namespace lsr {
namespace peaks {

constexpr int kMaxHalfWidth = 64;      // window half-widths per axis (as the blur's radius)
constexpr int kTreeThreads = 256;      // the per-bead sums: 256 strided partial sums, then a binary tree
constexpr int kMaxPatch = 129;         // PSF patch extent per axis (what DeconvolveSettings.psf_shape_zyx takes)

// The test at voxel `lin` of the smoothed volume s, given the maximum m of its window (a NaN where the window holds one: no
// voxel equals it): s == m, s >= threshold, and no voxel of the window with a smaller linear index reaches s.  Those voxels
// are exactly the three half-windows BELOW the voxel in C order of s along x, of A (s dilated along x) along y and of B (A
// dilated along y) along z; an axis with half-width 0 has none, and A or B may then be the volume before it.  Rarely true
// past the first line, so the division is behind it.
struct PeakTest {
  const float* s;
  const float* a;
  const float* b;
  int64_t X, plane;
  int rz, ry, rx;
  float threshold;
  // at every voxel
  __host__ __device__ bool maximum(int64_t lin, float m) const {
    const float sv = s[lin];
    return sv == m && sv >= threshold;
  }
  // the tie rule, at a voxel that passed maximum()
  __host__ __device__ bool first(int64_t lin) const {
    const float sv = s[lin];
    const int64_t z = lin / plane, rem = lin - z * plane, y = rem / X, x = rem - y * X;
    bool tie = false;
    for (int64_t d = rx < x ? rx : x; d > 0 && !tie; --d) tie = s[lin - d] >= sv;
    for (int64_t d = ry < y ? ry : y; d > 0 && !tie; --d) tie = a[lin - d * X] >= sv;
    for (int64_t d = rz < z ? rz : z; d > 0 && !tie; --d) tie = b[lin - d * plane] >= sv;
    return !tie;
  }
};

inline int check_local_max(const float* s, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, float threshold,
                           const long long* cand_index, const float* cand_value, int64_t capacity,
                           const unsigned long long* count) {
  LSR_REQUIRE_PTR(s);
  LSR_REQUIRE_PTR(cand_index);
  LSR_REQUIRE_PTR(cand_value);
  LSR_REQUIRE_PTR(count);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(rz >= 0 && ry >= 0 && rx >= 0, LSR_E_ARG, "half-widths (%d,%d,%d) must be >= 0", rz, ry, rx);
  LSR_REQUIRE(rz <= kMaxHalfWidth && ry <= kMaxHalfWidth && rx <= kMaxHalfWidth, LSR_E_UNSUPPORTED,
              "half-widths (%d,%d,%d): at most %d per axis", rz, ry, rx, kMaxHalfWidth);
  LSR_REQUIRE(threshold == threshold, LSR_E_ARG, "threshold is NaN");
  LSR_REQUIRE(capacity > 0 && capacity < (int64_t(1) << 31), LSR_E_ARG, "capacity %lld outside [1, 2^31)",
              (long long)capacity);
  return LSR_OK;
}

// a list of n odd patches of (pz, py, px) voxels in a (Z, Y, X) volume: what every per-bead entry point takes
inline int check_patches(int64_t Z, int64_t Y, int64_t X, int64_t n, int pz, int py, int px) {
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(n > 0 && n < (int64_t(1) << 24), LSR_E_ARG, "%lld beads: between 1 and 2^24", (long long)n);
  LSR_REQUIRE(pz > 0 && py > 0 && px > 0 && pz % 2 == 1 && py % 2 == 1 && px % 2 == 1, LSR_E_ARG,
              "patch (%d,%d,%d) must be odd and positive", pz, py, px);
  LSR_REQUIRE(pz <= kMaxPatch && py <= kMaxPatch && px <= kMaxPatch, LSR_E_UNSUPPORTED, "patch (%d,%d,%d): at most %d per axis",
              pz, py, px, kMaxPatch);
  LSR_REQUIRE(pz <= Z && py <= Y && px <= X, LSR_E_SHAPE, "patch (%d,%d,%d) is larger than the volume (%lld,%lld,%lld)", pz, py,
              px, (long long)Z, (long long)Y, (long long)X);
  return LSR_OK;
}

inline int check_psf_accumulate(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n,
                                int pz, int py, int px, const double* bead_stats, const float* psf) {
  LSR_REQUIRE_PTR(vol);
  LSR_REQUIRE_PTR(centres);
  LSR_REQUIRE_PTR(bead_stats);
  LSR_REQUIRE_PTR(psf);
  return check_patches(Z, Y, X, n, pz, py, px);
}

constexpr int kMaxBoxTaps = 2 * kMaxHalfWidth + 1;

// index j of a mirrored line of length L (-k -> k, L - 1 + k -> L - 1 - k; one reflection: |overhang| < L)
__host__ __device__ inline int64_t mirror(int64_t j, int64_t L) { return j < 0 ? -j : (j >= L ? 2 * (L - 1) - j : j); }

inline int check_box_smooth(const float* in, const float* out, int64_t Z, int64_t Y, int64_t X, int taps, float tap) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(in != out, LSR_E_ARG, "out must not alias in");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(taps >= 1 && taps % 2 == 1, LSR_E_ARG, "%d taps: an odd count", taps);
  LSR_REQUIRE(taps <= kMaxBoxTaps, LSR_E_UNSUPPORTED, "%d taps: at most %d", taps, kMaxBoxTaps);
  LSR_REQUIRE(taps / 2 < Z && taps / 2 < Y && taps / 2 < X, LSR_E_ARG,
              "mirrored borders need %d < every extent of (%lld,%lld,%lld)", taps / 2, (long long)Z, (long long)Y, (long long)X);
  LSR_REQUIRE(tap == tap, LSR_E_ARG, "tap is NaN");
  return LSR_OK;
}

// Corner of the patch centred on linear index `lin`, or false when the index is outside the volume or the patch
// does not fit: such a bead contributes nothing (background 0, total 0) and nothing outside the volume is read.
__host__ __device__ inline bool patch_origin(long long lin, int64_t Z, int64_t Y, int64_t X, int pz, int py, int px,
                                             int64_t& z0, int64_t& y0, int64_t& x0) {
  if (lin < 0 || lin >= Z * Y * X) return false;
  const int64_t z = lin / (Y * X), rem = lin - z * (Y * X), y = rem / X, x = rem - y * X;
  z0 = z - pz / 2; y0 = y - py / 2; x0 = x - px / 2;
  return z0 >= 0 && y0 >= 0 && x0 >= 0 && z0 + pz <= Z && y0 + py <= Y && x0 + px <= X;
}

// is patch element (iz, iy, ix) on one of the six faces?
__host__ __device__ inline bool on_shell(int iz, int iy, int ix, int pz, int py, int px) {
  return iz == 0 || iz == pz - 1 || iy == 0 || iy == py - 1 || ix == 0 || ix == px - 1;
}
__host__ __device__ inline int64_t shell_count(int pz, int py, int px) {
  const int64_t inner = (pz > 2 && py > 2 && px > 2) ? int64_t(pz - 2) * (py - 2) * (px - 2) : 0;
  return int64_t(pz) * py * px - inner;
}

// The fixed tree of the per-bead sums: every thread of a kTreeThreads workgroup brings one partial sum.
__device__ __forceinline__ double tree_sum(double* red, double a) {
  const int tid = threadIdx.x;
  red[tid] = a;
  __syncthreads();
  for (int w = kTreeThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

// bead_stats_kernel of peaks.hip on `st`: (B, S) per bead
void launch_bead_stats(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n_beads, int pz,
                       int py, int px, double* bead_stats, hipStream_t st);

}  // namespace peaks
}  // namespace lsr
