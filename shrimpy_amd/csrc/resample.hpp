// The order-1 resampling rule of scipy.ndimage.affine_transform, ONE definition each, for the kernels that apply it
// (affine.hip, affine_planar.hip, affine_box.hip, the z tap of deskew.hip) and their host twin (host_twins.hip).  Deskew and
// affine apply are pinned bit for bit against scipy and against each other: "the same arithmetic in the same order" is
// the text below, not a copy per file.  A change here is checked by comparing the compiler's listings of the four device
// units against the parent's (profiles/resample_isa.txt gives the commands and names the spellings that stay local).
#pragma once

#include <algorithm>
#include <cmath>

#include "stencil_prims.hpp"

namespace lsr {

// ---- the arithmetic: host and device --------------------------------------------------------------------------------
// Exact fp64 operations, no FMA contraction (results must match scipy's C): every product and sum is rounded on its own.
// On the host the translation unit is built with -ffp-contract=off and the plain operators are that.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
#else
inline double dmul(double a, double b) { return a * b; }
inline double dadd(double a, double b) { return a + b; }
#endif

// Coordinate of one input axis for output index (zo, yo, xo), evaluated in scipy's order:
// ((zo*m0 + yo*m1) + xo*m2) + shift, every product and sum rounded separately.
__host__ __device__ __forceinline__ double affine_coord(double zo, double yo, double xo, double m0, double m1, double m2,
                                                        double shift) {
  double c = dmul(zo, m0);
  c = dadd(c, dmul(yo, m1));
  c = dadd(c, dmul(xo, m2));
  return dadd(c, shift);
}

// scipy's weights of the two neighbours from the fractional part f = c - floor(c): w0 = 1 - f, w1 = 1 - w0 (not f: the
// two differ by up to 1 ulp).
__host__ __device__ __forceinline__ void tap_weights(double f, double& w0, double& w1) {
  w0 = 1.0 - f;
  w1 = 1.0 - w0;
}

// One corner of scipy's sum: ((v * wz) * wy) * wx added to the running total, corners taken z-major.
__host__ __device__ __forceinline__ double add_corner(double t, double v, double wz, double wy, double wx) {
  return dadd(t, dmul(dmul(dmul(v, wz), wy), wx));
}

template <typename Index>
struct AxisTap {
  Index i0, i1;     // clamped neighbour indices
  double w0, w1;    // scipy weights (tap_weights)
  double f;         // fractional part
  bool out0, out1;  // grid-constant: neighbour is outside the volume -> cval
};

// One axis of one sample.  Returns false if (mode constant) the coordinate is outside [0, n-1] -> whole sample is cval.
template <bool GRID, typename Index>
__host__ __device__ __forceinline__ bool axis_tap(double c, Index n, AxisTap<Index>& t) {
  if (!GRID && (c < 0.0 || c > static_cast<double>(n - 1))) return false;
  const double fl = floor(c);
  t.f = c - fl;
  tap_weights(t.f, t.w0, t.w1);
  if constexpr (!GRID) {
    // 0 <= c <= n-1: floor(c) is a valid index; only the upper neighbour can leave the volume
    // (c == n-1 exactly, where its weight is 0)
    t.i0 = static_cast<Index>(fl);
    t.i1 = std::min(t.i0 + 1, n - 1);
    t.out0 = t.out1 = false;
  } else {
    // indices only matter while a neighbour can be inside; clamp far-away coordinates first
    const Index start = static_cast<Index>(fmin(fmax(fl, -2.0), static_cast<double>(n) + 1.0));
    t.out0 = start < 0 || start >= n;
    t.out1 = start + 1 < 0 || start + 1 >= n;
    t.i0 = std::min(std::max(start, Index(0)), n - 1);
    t.i1 = std::min(std::max(start + 1, Index(0)), n - 1);
  }
  return true;
}

// ---- the requirements of an affine call, one function per group ------------------------------------------------------
// Each answers LSR_OK, or its code with the message in lsr_last_error().  An entry calls the groups that apply to it in
// the order it has always tested them (the status of a call that breaks two of them is part of the ABI:
// tests/golden/resample_entry_statuses.json) and multiplies extents or strides only behind the group that bounds them.
inline int require_buffers(const void* in, const void* out, const double* M) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE_PTR(M);
  return LSR_OK;
}
inline int require_positive(int64_t Zi, int64_t Yi, int64_t Xi, int64_t Zo, int64_t Yo, int64_t Xo) {
  LSR_REQUIRE(Zi > 0 && Yi > 0 && Xi > 0 && Zo > 0 && Yo > 0 && Xo > 0, LSR_E_SHAPE,
              "shapes (%lld,%lld,%lld) -> (%lld,%lld,%lld) must be positive", (long long)Zi, (long long)Yi, (long long)Xi,
              (long long)Zo, (long long)Yo, (long long)Xo);
  return LSR_OK;
}
inline int require_volumes(int64_t Zi, int64_t Yi, int64_t Xi, int64_t Zo, int64_t Yo, int64_t Xo) {
  LSR_REQUIRE_VOLUME(Zi, Yi, Xi);
  LSR_REQUIRE_VOLUME(Zo, Yo, Xo);
  return LSR_OK;
}
// strides in floats of the `side` ("source" / "output") volume: their ranges, then (behind the ranges and the volumes)
// that a (Y x X) plane fits them
inline int require_stride_range(const char* side, int64_t pitch, int64_t plane) {
  LSR_REQUIRE(strides_in_range(pitch, plane), LSR_E_UNSUPPORTED,
              "%s strides (%lld, %lld): a row stride must be in [0, 2^31), a plane stride in [0, 2^32) elements", side,
              (long long)pitch, (long long)plane);
  return LSR_OK;
}
inline int require_stride_fit(const char* side, int64_t pitch, int64_t plane, int64_t Y, int64_t X) {
  LSR_REQUIRE(pitch >= X && plane >= Y * pitch, LSR_E_SHAPE, "%s strides (%lld, %lld) are smaller than a (%lld x %lld) plane",
              side, (long long)pitch, (long long)plane, (long long)Y, (long long)X);
  return LSR_OK;
}
// The border rule of a mode word: false = neither LSR_MODE_CONSTANT nor LSR_MODE_GRID_CONSTANT under the f32 flag.
inline bool border_of(int mode, bool* grid, bool* f32 = nullptr) {
  const int border = mode & ~LSR_MODE_F32_INTERP;
  *grid = border == LSR_MODE_GRID_CONSTANT;
  if (f32 != nullptr) *f32 = (mode & LSR_MODE_F32_INTERP) != 0;
  return border == LSR_MODE_CONSTANT || *grid;
}
// ... f32 == nullptr: the entry does not take LSR_MODE_F32_INTERP (the host twin: its arithmetic is always scipy's fp64)
inline int require_border(int mode, bool* grid, bool* f32 = nullptr) {
  bool flag;
  const bool known = border_of(mode, grid, &flag);
  if (f32 != nullptr) *f32 = flag;
  LSR_REQUIRE(known && (f32 != nullptr || !flag), LSR_E_ARG,
              "mode %d: LSR_MODE_CONSTANT or LSR_MODE_GRID_CONSTANT%s", mode,
              f32 != nullptr ? ", with or without LSR_MODE_F32_INTERP" : " (the f32-interpolation flag has no host twin)");
  return LSR_OK;
}
// the most slices one output plane may average: what deskew.hip and its twin in host_twins.hip both accept
constexpr int kMaxAvgSlices = 4096;
inline int check_matrix(const double M[12]) {
  LSR_REQUIRE_PTR(M);
  for (int i = 0; i < 12; ++i) LSR_REQUIRE(M[i] == M[i] && M[i] - M[i] == 0.0, LSR_E_ARG, "M[%d] is not finite", i);
  return LSR_OK;
}

// ---- host geometry of the LDS-staged kernels ---------------------------------------------------------------------------
// Source box of a tile along one axis, from the extent |m_z| (tz - 1) + |m_y| (ty - 1) + |m_x| (tx - 1) of the coordinate
// over the tile: floor(cmax) - floor(cmin) <= floor(extent) + 1 (the extent is summed here in another order than on the
// device: 1e-6 absorbs that), + 1 for the upper neighbour, + 1 for the count.
inline int box_rows(double extent) { return static_cast<int>(extent + 1e-6) + 3; }
// ... along x, in floats: + 3 for the 16-byte alignment of the first column, rows rounded up to whole 16-byte chunks
inline int box_row_floats(double extent) { return (box_rows(extent) + 3 + 3) & ~3; }
// a box in LDS takes whole waves of 16-byte chunks: 256 floats
template <typename T>
__host__ __device__ constexpr T box_slot_floats(T floats) { return (floats + 255) & ~T(255); }
// LDS-DMA moves 16-byte chunks: rows start on 16-byte boundaries and hold whole chunks up to the last column, and the
// staging wants a box of at least two chunks and two rows
inline bool lds_dma_rows_ok(int64_t Yi, int64_t Xi, int64_t pitch) {
  return pitch % 4 == 0 && pitch >= ((Xi + 3) & ~int64_t(3)) && Xi >= 8 && Yi >= 2;
}

// affine_planar.hip: z-decoupled maps, either border rule; false = not applicable
// (pitch / plane: source strides in floats; dense = Xi, Yi * Xi)
bool launch_affine_planar(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, int64_t pitch, int64_t plane,
                          float* out, int64_t Zo, int64_t Yo, int64_t Xo, int64_t opitch, int64_t oplane,
                          const double M[12], float cval, bool f32, bool grid, hipStream_t s);
bool affine_planar_geometry(int64_t Yi, int64_t Xi, int64_t pitch, const double M[12], int* box_y, int* box_x,
                            int* slots, int64_t* lds_bytes, int* tile = nullptr, int waves = 8);
// affine_box.hip: any map whose per-block source box fits in LDS (z-coupled maps included),
// either border rule; false = not applicable
bool launch_affine_box(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, int64_t pitch, int64_t plane, float* out,
                       int64_t Zo, int64_t Yo, int64_t Xo, int64_t opitch, int64_t oplane, const double M[12], float cval,
                       bool f32, bool grid, hipStream_t s);
bool affine_box_geometry(int64_t Zi, int64_t Yi, int64_t Xi, int64_t pitch, int64_t plane, const double M[12],
                         int* box_z, int* box_y, int* box_x, int64_t* lds_bytes);
bool affine_box_shape(int64_t Zi, int64_t Yi, int64_t Xi, const double M[12], int out6[6]);

// The launch of one LDS-staged affine call: everything the host decides from the shapes, the strides, the matrix and the
// measurement switches.  launch_affine_planar / launch_affine_box launch from these and lsr_affine_plan reports them, so what
// the tests count is what runs.  (What only the call itself knows -- the alignment of `in`, in == out, a device that refuses
// the LDS budget -- is not part of a plan: each of them sends the call to the gather kernel.)
struct AffinePlanarPlan {
  int waves, tile;             // 8 or 4 waves per workgroup; index into the tile table
  int tile_y, tile_x;          // output pixels per tile
  int box_y, box_x, slots;     // staged source box of a plane (rows, floats per row), ring depth
  int64_t lds_bytes;
  int z_chunk;                 // output planes per workgroup
  int tiles_y, tiles_x;
  int patch_h, patch_w;        // exact mode: tiles per patch
  int py_n, px_n, per_xcd;
  int64_t grid;                // workgroups launched
};
bool affine_planar_plan(int64_t Yi, int64_t Xi, int64_t pitch, int64_t plane, int64_t Zo, int64_t Yo, int64_t Xo,
                        const double M[12], bool f32, AffinePlanarPlan* plan);
struct AffineBoxPlan {
  int tz, ty, tx;              // block of output voxels
  int bz, by, bx;              // staged source box (planes, rows, floats per row)
  int64_t lds_bytes;
  int tz_n, ty_n, tx_n;        // blocks per axis
  int pz_n, py_n, px_n;        // 4 x 4 x 4 patches per axis
  int per_xcd, linear;
  int64_t grid;                // workgroups launched
};
bool affine_box_plan(int64_t Zi, int64_t Yi, int64_t Xi, int64_t pitch, int64_t plane, int64_t Zo, int64_t Yo, int64_t Xo,
                     int64_t opitch, const double M[12], bool f32, AffineBoxPlan* plan);

// ---- device only -------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

using prims::f32x4;
using prims::glds_x4;   // LDS-DMA, 16 bytes per lane (the production string: no cache-policy suffix)
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));  // 8-byte load, 4-byte aligned: the two x neighbours

// Workgroups b, b + 8, ... share an XCD (round-robin dispatch): XCD k runs the contiguous items [k per_xcd, (k + 1) per_xcd).
__device__ __forceinline__ int xcd_run(int bid, int per_xcd) { return (bid & 7) * per_xcd + (bid >> 3); }

// Taps of one sample in LDS order: v[0] / v[1] = rows y0 / y1 of plane z0, v[2] / v[3] of plane z1, each the x pair.
// LSR_MODE_F32_INTERP: seven f32 FMAs with the fractional parts as weights (x, then y, then z) -- ~1e-6 relative to
// scipy, not bit-identical.
__device__ __forceinline__ float trilinear_f32(const f32x2u (&v)[4], float fx, float fy, float fz) {
  const float a0 = fmaf(fx, v[0].y - v[0].x, v[0].x), a1 = fmaf(fx, v[1].y - v[1].x, v[1].x);
  const float b0 = fmaf(fx, v[2].y - v[2].x, v[2].x), b1 = fmaf(fx, v[3].y - v[3].x, v[3].x);
  const float c0 = fmaf(fy, a1 - a0, a0), c1 = fmaf(fy, b1 - b0, b0);
  return fmaf(fz, c1 - c0, c0);
}

#endif  // __HIPCC__

}  // namespace lsr
