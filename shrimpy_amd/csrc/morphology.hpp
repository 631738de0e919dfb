// What the grey-morphology kernels (morphology.hip) and their host twin (host_twins.hip) share: the rule, the entry check, the
// order, the plan of passes and the walk along a line -- ONE definition, so that the two sides choose the same element.  The
// bead detection (peaks.hip and its twin) runs the same passes: its box maximum is a dilation, and its test is the walk's sink.
//
// Rule.  A flat box of half-widths (rz, ry, rx), window 2r + 1 per axis, over a contiguous (Z, Y, X) float32 volume v.
//   erode(v)(p)   the least    v(q) over the in-volume q of the box around p
//   dilate(v)(p)  the greatest v(q) over the same q
//   Voxels outside the volume do not compete (for centred odd boxes that is scipy.ndimage's default `reflect` border); a
//   half-width may exceed the axis.  Values compare by label::float_key (-0.0 below +0.0, +-inf ordinary values) and the
//   result is the bit pattern of the chosen element: no order of evaluation can change it.  A window that holds a NaN gives
//   the canonical quiet NaN 0x7fc00000, for erosion and dilation alike: such a window has no least and no greatest element.
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
// offset t of the block that holds j.  About three comparisons per voxel at any w.  What is done with out(i) is the walk's
// SINK, sink(at, m) with `at` the voxel's linear index and m the decoded element: StoreSink below writes it (minus or from the
// caller's volume for the top-hats), the bead detection's (peaks.hpp) tests it against the smoothed volume and never stores it.
// A sink that answers true is handed the voxel again, sink.late(at): its rare and long path, which the kernel keeps out of its
// unrolled steps.
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
constexpr int64_t kMaxRowBlocks = 256 * 16;  // x pass: workgroups at most (they stride over the rows, reading ahead)
// The strided walk's instantiations, by the rows they read ahead: up to kNarrow registers, not LDS, limit the waves; up to
// kStaticLdsBytes of strip the launch needs no opt-in; above it the kernel is allowed dynamic LDS first (launch_strided).
constexpr int kNarrow = 12;
constexpr int kStaticLdsBytes = 64 * 1024;
constexpr int kAheadNarrow = 8, kAheadStatic = 16, kAheadDynamic = 32;
// the greatest half-width whose strip, (2r + 1) * kColumns codes, fits kStaticLdsBytes
constexpr int kMaxStaticHalfWidth = (kStaticLdsBytes / (kColumns * static_cast<int>(sizeof(uint32_t))) - 1) / 2;
static_assert(kNarrow < kMaxStaticHalfWidth && kMaxStaticHalfWidth < kMaxHalfWidth, "three instantiations, in this order");
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

struct StoreSink {
  float* out;
  const float* orig;        // read at the voxel written, unless fuse == kPlain
  int fuse;
  __host__ __device__ bool operator()(int64_t at, float m) const {
    out[at] = fused(m, fuse != kPlain ? orig[at] : 0.0f, fuse);
    return false;
  }
  __host__ __device__ void late(int64_t) const {}
};

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
// suffix maxima of the previous block.  The host twins run exactly this; morph_strided_kernel below runs it with a lane per
// thread and the loads of a block issued ahead of their use.
template <typename Sink>
inline void walk_host(const float* in, int64_t base, int lanes, int64_t cstep, int64_t L, int64_t step, int r, bool least,
                      uint32_t* strip, const Sink& sink) {
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
        if (i >= 0 && i < L && sink(at + i * step, decode(m, least))) sink.late(at + i * step);
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

// y, z (and any axis but x) on the device: one wavefront per workgroup owns kColumns neighbouring columns and walks them over
// the whole line; U rows are read ahead of the walk.  See morphology.hip.
template <int U, typename Sink>
__global__ __launch_bounds__(kColumns) void morph_strided_kernel(const float* __restrict__ in, Lines p, int r, int least_i,
                                                                  Sink sink) {
  extern __shared__ uint32_t strip[];            // [w][kColumns]
  const bool least = least_i != 0;
  const int lane = threadIdx.x, w = 2 * r + 1;
  const int64_t tiles_per_slab = (p.columns + kColumns - 1) / kColumns, tiles = p.outer * tiles_per_slab;
  const int64_t blocks = (p.L - 1 + r) / w + 1;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t slab = tile / tiles_per_slab, col = (tile - slab * tiles_per_slab) * kColumns + lane;
    if (col >= p.columns) continue;              // (no barrier anywhere below)
    const int64_t base = slab * p.ostep + col * p.cstep;
    for (int t = 0; t < w; ++t) strip[t * kColumns + lane] = kNoCode;
    // The line as one stream of positions j = 0 .. blocks * w, U at a time; the loads of the next U are issued before
    // this U is walked, so a lane has U .. 2U rows in flight whatever w is.
    const int64_t total = blocks * w;
    float ahead[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ahead[u] = u < p.L ? in[base + u * p.step] : 0.0f;
    uint32_t g = kNoCode;
    int t = 0;
    for (int64_t j0 = 0; j0 < total; j0 += U) {
      uint32_t c[U];
      unsigned late = 0;                           // bit u: the sink wants the voxel of step u again, after the U steps
#pragma unroll
      for (int u = 0; u < U; ++u) c[u] = j0 + u < p.L ? encode(ahead[u], least) : kNoCode;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + U + u;
        ahead[u] = j < p.L ? in[base + j * p.step] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + u;
        if (j < total) {
          g = umax(g, c[u]);
          const uint32_t m = t < w - 1 ? umax(strip[(t + 1) * kColumns + lane], g) : g;
          strip[t * kColumns + lane] = c[u];
          const int64_t i = j - r;
          if (i >= 0 && i < p.L && sink(base + i * p.step, decode(m, least))) late |= 1u << u;
          if (++t == w) {                          // the block is complete: its codes become its suffix maxima
            t = 0;
            g = kNoCode;
            if (j + 1 < total) {
              uint32_t run = kNoCode;
              for (int s = w - 1; s >= 0; --s) {
                run = umax(run, strip[s * kColumns + lane]);
                strip[s * kColumns + lane] = run;
              }
            }
          }
        }
      }
      for (; late != 0; late &= late - 1) sink.late(base + (j0 + __ffs(late) - 1 - r) * p.step);
    }
  }
}

// Launches the walk over `lines` on `st`, sink by sink.  Rows in flight per lane: the wider the window, the fewer wavefronts
// its LDS strip (w * kColumns codes) leaves on a compute unit, the more each has in flight; up to kNarrow registers, not LDS,
// limit the waves (kNarrow, kStaticLdsBytes and the depths: above).
constexpr int64_t kMaxBlocks = int64_t(1) << 20;
template <typename Sink>
inline int launch_strided(const float* src, const Lines& lines, int r, bool least, const Sink& sink, const char* who,
                          hipStream_t st) {
  constexpr int kMaxLds = (2 * kMaxHalfWidth + 1) * kColumns * static_cast<int>(sizeof(uint32_t));
  static std::atomic<uint64_t> lds_allowed{0};   // (one per sink: one per kernel)
  const int64_t tiles = lines.outer * ceil_div(lines.columns, kColumns);
  const size_t lds = sizeof(uint32_t) * (2 * r + 1) * kColumns;
  const dim3 grid(static_cast<unsigned>(tiles < kMaxBlocks ? tiles : kMaxBlocks));
  if (r <= kNarrow) {
    hipLaunchKernelGGL((morph_strided_kernel<kAheadNarrow, Sink>), grid, dim3(kColumns), lds, st, src, lines, r, least ? 1 : 0,
                       sink);
  } else if (lds <= static_cast<size_t>(kStaticLdsBytes)) {
    hipLaunchKernelGGL((morph_strided_kernel<kAheadStatic, Sink>), grid, dim3(kColumns), lds, st, src, lines, r, least ? 1 : 0,
                       sink);
  } else {
    if (int rc = allow_dynamic_lds(reinterpret_cast<const void*>(morph_strided_kernel<kAheadDynamic, Sink>), kMaxLds,
                                   lds_allowed, who))
      return rc;
    hipLaunchKernelGGL((morph_strided_kernel<kAheadDynamic, Sink>), grid, dim3(kColumns), lds, st, src, lines, r,
                       least ? 1 : 0, sink);
  }
  return LSR_OK;
}

// One pass of lsr_grey_morph_f32 on `st` (morphology.hip): the x pass by rows, any other through launch_strided<StoreSink>.
int launch_pass(const float* src, const StoreSink& sink, int64_t Z, int64_t Y, int64_t X, const Pass& ps, const char* who,
                hipStream_t st);

}  // namespace morph
}  // namespace lsr
