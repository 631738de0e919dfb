// What the grey-morphology kernels (morphology.hip) and their host twin (host_twins.hip) share: the rule, the entry check, the
// order, the plan of passes and the walk along a line -- ONE definition, so that the two sides choose the same element.
//
// Rule.  A flat box of half-widths (rz, ry, rx), window 2r + 1 per axis, over a contiguous (Z, Y, X) float32 volume v.
//   erode(v)(p)   the least    v(q) over the in-volume q of the box around p
//   dilate(v)(p)  the greatest v(q) over the same q
//   Voxels outside the volume do not compete (for centred odd boxes that is scipy.ndimage's default `reflect` border); a
//   half-width may exceed the axis.  Values compare by label::float_key (-0.0 below +0.0, +-inf ordinary values) and the
//   result is the bit pattern of the chosen element: no order of evaluation can change it.  A window that holds a NaN gives
//   the canonical quiet NaN 0x7fc00000, for erosion and dilation alike (the rule of peaks::nmax).
//   open = dilate(erode), close = erode(dilate); white top-hat = v - open(v), black top-hat = close(v) - v: one IEEE float32
//   subtraction per voxel (a NaN it produces may carry any payload).
//   An axis with half-width 0 gets no pass; with all three at 0, erode .. close copy v and the top-hats are v - v.
// scipy.ndimage.grey_erosion / grey_dilation / grey_opening / grey_closing / white_tophat / black_tophat with size = 2r + 1
// element for element on NaN-free volumes (tests/morphology_ref.py restates the rule and pins the NaNs).
//
// Scheme.  Minimum and maximum are separable and commute across axes: one pass per axis with r > 0.  Both are ONE unsigned
// maximum of a code (encode below): the float's key for a maximum, its complement for a minimum, NaN the greatest code and 0
// "does not compete".  A pass is a van Herk / Gil-Werman walk: the line is cut into blocks of w = 2r + 1; with h the suffix
// maxima of the previous block and g the running prefix maximum of the current one, out(j - r) = max(h(t + 1), g(t)) at
// offset t of the block that holds j.  About three comparisons per voxel at any w.
#pragma once

#include "common.hpp"
#include "label.hpp"

namespace lsr {
namespace morph {

constexpr int kMaxHalfWidth = 256;          // w = 513 codes per column: 131,328 bytes of the 160 KiB of LDS at kColumns = 64
constexpr int kColumns = 64;                // strided passes: columns per workgroup (one wavefront: rows of 256 bytes)
constexpr int kRowSegment = 2048;           // x pass: outputs per staged segment of a row at most (>= 4 * kMaxHalfWidth)
constexpr int kRowThreads = 256;
constexpr int kMaxPasses = 6;
static_assert(kRowSegment >= 4 * kMaxHalfWidth, "the carried halo of the x pass must not overlap its source: half a segment >= 2r");

enum Op { kErode = 0, kDilate = 1, kOpen = 2, kClose = 3, kWhiteTophat = 4, kBlackTophat = 5 };
enum Fuse { kPlain = 0, kInMinus = 1, kMinusIn = 2 };      // the last pass: m, orig - m, m - orig

constexpr uint32_t kNanCode = 0xffffffffu;   // absorbs every maximum
constexpr uint32_t kNoCode = 0u;             // outside the volume: never chosen (every window holds its own centre)
constexpr uint32_t kQuietNan = 0x7fc00000u;

__host__ __device__ inline uint32_t encode(float v, bool least) {
  if (v != v) return kNanCode;
  const uint32_t k = label::float_key(v);    // in [0x007fffff, 0xff800000] for every non-NaN float, and so is ~k
  return least ? ~k : k;
}
__host__ __device__ inline float decode(uint32_t c, bool least) {
  if (c == kNanCode) {
    float v;
    const uint32_t b = kQuietNan;
    memcpy(&v, &b, sizeof(v));
    return v;
  }
  return label::key_float(least ? ~c : c);
}
__host__ __device__ inline uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__host__ __device__ inline float fused(float m, float orig, int fuse) {
  return fuse == kInMinus ? orig - m : (fuse == kMinusIn ? m - orig : m);
}

inline int check_morph(const float* in, const float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int op,
                       const void* scratch) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE_PTR(scratch);
  LSR_REQUIRE(in != out, LSR_E_ARG, "out must not alias in");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(rz >= 0 && ry >= 0 && rx >= 0, LSR_E_ARG, "half-widths (%d,%d,%d) must be >= 0", rz, ry, rx);
  LSR_REQUIRE(rz <= kMaxHalfWidth && ry <= kMaxHalfWidth && rx <= kMaxHalfWidth, LSR_E_UNSUPPORTED,
              "half-widths (%d,%d,%d): at most %d per axis", rz, ry, rx, kMaxHalfWidth);
  LSR_REQUIRE(op >= kErode && op <= kBlackTophat, LSR_E_ARG, "op %d: 0 erode .. 5 black top-hat", op);
  return LSR_OK;
}

// One pass: axis 0 = z, 1 = y, 2 = x.
struct Pass {
  int axis, r;
  bool least;
};

// The passes of `op` in launch order: the first run x, y, z, the second z, y, x.  Returns their number (0 .. kMaxPasses).
inline int plan(int rz, int ry, int rx, int op, Pass out[kMaxPasses]) {
  const int r[3] = {rz, ry, rx};
  const bool first_least = op == kErode || op == kOpen || op == kWhiteTophat;
  const bool two = op != kErode && op != kDilate;
  int n = 0;
  for (int a = 2; a >= 0; --a)
    if (r[a] > 0) out[n++] = Pass{a, r[a], first_least};
  if (two)
    for (int a = 0; a < 3; ++a)
      if (r[a] > 0) out[n++] = Pass{a, r[a], !first_least};
  return n;
}
inline int fuse_of(int op) { return op == kWhiteTophat ? kInMinus : (op == kBlackTophat ? kMinusIn : kPlain); }

// The lines of one pass: `outer` slabs of `columns` lines each; a line has L positions `step` apart, neighbouring columns of a
// slab are `cstep` apart, slabs `ostep`.
struct Lines {
  int64_t outer, ostep, columns, cstep, L, step;
};
inline Lines lines_of(int axis, int64_t Z, int64_t Y, int64_t X) {
  if (axis == 2) return Lines{1, 0, Z * Y, X, X, 1};
  if (axis == 1) return Lines{Z, Y * X, X, 1, Y, X};
  return Lines{1, 0, Y * X, 1, Z, Y * X};
}

// Source and destination of pass k of n: the passes alternate between the two scratch volumes, the first reads `in`, the last
// writes `out` -- which is therefore written exactly once, and `in` never.
inline const float* pass_source(int k, const float* in, float* scratch, int64_t voxels) {
  return k == 0 ? in : scratch + ((k - 1) & 1) * voxels;
}
inline float* pass_target(int k, int n, float* out, float* scratch, int64_t voxels) {
  return k == n - 1 ? out : scratch + (k & 1) * voxels;
}

// The walk of `lanes` (<= kColumns) neighbouring lines at once, as a wavefront takes it: strip[t * kColumns + lane] holds the
// suffix maxima of the previous block.  The host twin runs exactly this; the kernel runs it with a lane per thread and the
// loads of a block issued ahead of their use (morphology.hip).
inline void walk_host(const float* in, float* out, const float* orig, int64_t base, int lanes, int64_t cstep, int64_t L,
                      int64_t step, int r, bool least, int fuse, uint32_t* strip) {
  const int w = 2 * r + 1;
  for (int64_t i = 0; i < int64_t(w) * kColumns; ++i) strip[i] = kNoCode;
  const int64_t blocks = (L - 1 + r) / w + 1;
  uint32_t g[kColumns];
  for (int64_t b = 0; b < blocks; ++b) {
    for (int lane = 0; lane < lanes; ++lane) g[lane] = kNoCode;
    for (int t = 0; t < w; ++t) {
      const int64_t j = b * w + t, i = j - r;
      for (int lane = 0; lane < lanes; ++lane) {
        const int64_t at = base + lane * cstep;
        const uint32_t c = j < L ? encode(in[at + j * step], least) : kNoCode;
        g[lane] = umax(g[lane], c);
        const uint32_t m = t < w - 1 ? umax(strip[(t + 1) * kColumns + lane], g[lane]) : g[lane];
        strip[t * kColumns + lane] = c;
        if (i >= 0 && i < L) out[at + i * step] = fused(decode(m, least), orig != nullptr ? orig[at + i * step] : 0.0f, fuse);
      }
    }
    for (int lane = 0; lane < lanes; ++lane) {
      uint32_t run = kNoCode;
      for (int t = w - 1; t >= 0; --t) {
        run = umax(run, strip[t * kColumns + lane]);
        strip[t * kColumns + lane] = run;
      }
    }
  }
}

}  // namespace morph
}  // namespace lsr
