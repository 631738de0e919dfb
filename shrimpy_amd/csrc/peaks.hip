// Bead detection and PSF averaging (shrimpy_amd/psf.py; the stage scripts/measure_psf.py hands to biahub's
// _characterize_psf, which is not vendored: PARITY UNPINNED -- the rule is defined here and pinned to the NumPy / float64
// restatement tests/psf_ref.py).
//
// lsr_local_max_candidates_f32: the peaks of a smoothed volume s under a box window of half-widths (rz, ry, rx).  Voxel p
// is a peak iff  s(p) >= threshold,  s(p) >= s(q) for every in-volume q of its window  and  s(p) > s(q) for every such q
// with a smaller linear index (of tied maxima in reach of each other the first in C order wins).  A NaN compares false
// with everything: it is never a peak, and neither is a voxel with a NaN in its window.
//
// The box maximum is separable, and it is the grey dilation of morphology.hpp: the same passes, kernels and launches (about
// three comparisons per voxel at ANY window width; the (2r+1)^3 gather of the definition is 10^5..10^6 reads per voxel at the
// reference's min_distance of 20..50):
//     A = s dilated along x      morph::launch_pass: the row kernel
//     B = A dilated along y      morph::launch_pass: the strided walk with the plain store
//     M = B dilated along z      the strided walk with the test below as its sink: M is never written
// An axis with half-width 0 gets no launch (A is s, B is A); the z walk always runs -- at w = 1 it hands every voxel of B to
// the sink -- because it carries the test.  Voxels outside the volume do not compete.  The passes compare codes, not floats:
// A, B and M may hold +0.0 where a -0.0 was the first of the two in the window, and the canonical NaN for a window with any
// NaN; the test only ever COMPARES them with s, so neither shows.  A voxel with s == M and s >= threshold (rare) then checks
// the tie rule along the three half-windows BELOW it in C order (peaks::PeakTest),
//     s(z, y, x') x' in [x - rx, x)      A(z, y', x) y' in [y - ry, y)      B(z', y, x) z' in [z - rz, z)
// -- together exactly the window's voxels of smaller linear index -- and appends (linear index, value) to the caller's
// buffer through ONE integer atomic counter.  The counter keeps counting past the capacity (nothing is stored there), so
// count > capacity tells the caller that the buffer was too small.  Append order is arbitrary: callers sort.
//
// lsr_psf_accumulate_f32: the average of background-subtracted, flux-normalised patches around the given centres.  Per
// bead (one workgroup, fixed tree: 256 strided partial sums in float64, then a binary tree): B = mean of the patch's
// outer shell, S = sum(patch - B).  Then one thread per PSF voxel adds (v - B) / S over the beads with S > 0 in list
// order in float64 and stores the mean as float32: the same bits on every run, and the host twin's.

#include "morphology.hpp"
#include "peaks.hpp"

namespace {

// ---- box smoothing: one axis per launch, float64 between the passes ----
// out(i) = sum_k tap * in(mirror(i - r + k)) along one axis, accumulated in float64 in tap order (the host twin's order:
// the same bits).  The x and y passes store float64, the z pass rounds to float32: one rounding per voxel.
template <typename TIn, typename TOut>
__global__ __launch_bounds__(256) void box_pass_kernel(const TIn* __restrict__ in, TOut* __restrict__ out, int64_t n,
                                                       int64_t L, int64_t inner, int taps, double tap) {
  const int r = taps / 2;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i = (e / inner) % L;
    const TIn* line = in + (e - i * inner);
    double acc = 0.0;
    for (int k = 0; k < taps; ++k) acc += tap * static_cast<double>(line[lsr::peaks::mirror(i - r + k, L) * inner]);
    out[e] = static_cast<TOut>(acc);
  }
}

// ---- the sink of the z walk: the test, and the append ----
struct PeakSink {
  lsr::peaks::PeakTest test;
  long long* cand_index;
  float* cand_value;
  unsigned long long capacity;
  unsigned long long* count;
  __device__ bool operator()(int64_t lin, float m) const { return test.maximum(lin, m); }
  __device__ void late(int64_t lin) const {
    if (!test.first(lin)) return;
    const unsigned long long slot = atomicAdd(count, 1ull);
    if (slot < capacity) {
      cand_index[slot] = lin;
      cand_value[slot] = test.s[lin];
    }
  }
};

// ---- PSF averaging ----
constexpr int kTree = lsr::peaks::kTreeThreads;

using lsr::peaks::tree_sum;

__global__ __launch_bounds__(kTree) void bead_stats_kernel(const float* __restrict__ vol, int64_t Z, int64_t Y, int64_t X,
                                                           const long long* __restrict__ centres, int pz, int py, int px,
                                                           double* __restrict__ stats) {
  __shared__ double red[kTree];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int64_t z0 = 0, y0 = 0, x0 = 0;
  if (!lsr::peaks::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0)) {   // (the same answer in every thread)
    if (tid < 2) stats[2 * b + tid] = 0.0;
    return;
  }
  const int n = pz * py * px;
  const float* corner = vol + (z0 * Y + y0) * X + x0;
  double a = 0.0;
  for (int e = tid; e < n; e += kTree) {
    const int iz = e / (py * px), rem = e - iz * (py * px), iy = rem / px, ix = rem - iy * px;
    if (lsr::peaks::on_shell(iz, iy, ix, pz, py, px)) a += static_cast<double>(corner[(iz * Y + iy) * X + ix]);
  }
  const double bg = tree_sum(red, a) / static_cast<double>(lsr::peaks::shell_count(pz, py, px));
  a = 0.0;
  for (int e = tid; e < n; e += kTree) {
    const int iz = e / (py * px), rem = e - iz * (py * px), iy = rem / px, ix = rem - iy * px;
    a += static_cast<double>(corner[(iz * Y + iy) * X + ix]) - bg;
  }
  const double total = tree_sum(red, a);
  if (tid == 0) {
    stats[2 * b] = bg;
    stats[2 * b + 1] = total;
  }
}

__global__ __launch_bounds__(256) void psf_accumulate_kernel(const float* __restrict__ vol, int64_t Z, int64_t Y, int64_t X,
                                                             const long long* __restrict__ centres, int n_beads, int pz,
                                                             int py, int px, const double* __restrict__ stats,
                                                             float* __restrict__ psf) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= pz * py * px) return;
  const int iz = e / (py * px), rem = e - iz * (py * px), iy = rem / px, ix = rem - iy * px;
  double acc = 0.0;
  int used = 0;
  for (int b = 0; b < n_beads; ++b) {
    const double bg = stats[2 * b], total = stats[2 * b + 1];
    int64_t z0 = 0, y0 = 0, x0 = 0;
    if (!(total > 0.0) || !lsr::peaks::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0)) continue;
    acc += (static_cast<double>(vol[((z0 + iz) * Y + y0 + iy) * X + x0 + ix]) - bg) / total;
    ++used;
  }
  psf[e] = used > 0 ? static_cast<float>(acc / static_cast<double>(used)) : 0.0f;
}

}  // namespace

// the per-bead (B, S) of lsr_psf_accumulate_f32, for the shifted average of psf_fit.hip as well
void lsr::peaks::launch_bead_stats(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n_beads,
                                   int pz, int py, int px, double* bead_stats, hipStream_t st) {
  hipLaunchKernelGGL(bead_stats_kernel, dim3(static_cast<unsigned>(n_beads)), dim3(kTree), 0, st, vol, Z, Y, X, centres, pz,
                     py, px, bead_stats);
}

extern "C" int lsr_box_smooth_scratch_bytes(int64_t Z, int64_t Y, int64_t X, int64_t* bytes) {
  LSR_REQUIRE_PTR(bytes);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  *bytes = 2 * Z * Y * X * static_cast<int64_t>(sizeof(double));     // the x and the y pass's float64 results
  return LSR_OK;
}

extern "C" int lsr_box_smooth_f32(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int taps, float tap,
                                  void* scratch, lsr_stream_t stream) {
  if (int rc = lsr::peaks::check_box_smooth(in, out, Z, Y, X, taps, tap)) return rc;
  LSR_REQUIRE_PTR(scratch);
  LSR_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, LSR_E_ARG, "scratch must be 8-byte aligned");
  hipStream_t st = lsr::as_stream(stream);
  const int64_t n = Z * Y * X;
  double* a = static_cast<double*>(scratch);
  double* b = a + n;
  const int64_t want = lsr::ceil_div(n, 256);
  const dim3 grid(static_cast<unsigned>(want < 256 * 32 ? want : 256 * 32));
  const double t = static_cast<double>(tap);
  hipLaunchKernelGGL((box_pass_kernel<float, double>), grid, dim3(256), 0, st, in, a, n, X, int64_t(1), taps, t);
  hipLaunchKernelGGL((box_pass_kernel<double, double>), grid, dim3(256), 0, st, a, b, n, Y, X, taps, t);
  hipLaunchKernelGGL((box_pass_kernel<double, float>), grid, dim3(256), 0, st, b, out, n, Z, Y * X, taps, t);
  return lsr::launch_status("lsr_box_smooth_f32");
}

extern "C" int lsr_local_max_scratch_bytes(int64_t Z, int64_t Y, int64_t X, int64_t* bytes) {
  LSR_REQUIRE_PTR(bytes);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  *bytes = 2 * Z * Y * X * static_cast<int64_t>(sizeof(float));     // A and B
  return LSR_OK;
}

extern "C" int lsr_local_max_candidates_f32(const float* s, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx,
                                            float threshold, long long* cand_index, float* cand_value, int64_t capacity,
                                            unsigned long long* count, void* scratch, lsr_stream_t stream) {
  if (int rc = lsr::peaks::check_local_max(s, Z, Y, X, rz, ry, rx, threshold, cand_index, cand_value, capacity, count))
    return rc;
  LSR_REQUIRE_PTR(scratch);
  LSR_REQUIRE(X < (int64_t(1) << 30) && Y * X < (int64_t(1) << 40), LSR_E_UNSUPPORTED, "plane of %lld x %lld is too large",
              (long long)Y, (long long)X);
  hipStream_t st = lsr::as_stream(stream);
  namespace mo = lsr::morph;
  const char* who = "lsr_local_max_candidates_f32";
  float* scratch_a = static_cast<float*>(scratch);
  float* scratch_b = scratch_a + Z * Y * X;
  if (hipMemsetAsync(count, 0, sizeof(unsigned long long), st) != hipSuccess) return lsr::launch_status(who);
  const float* a = rx > 0 ? scratch_a : s;
  const float* b = ry > 0 ? scratch_b : a;
  const mo::StoreSink to_a{scratch_a, nullptr, mo::kPlain}, to_b{scratch_b, nullptr, mo::kPlain};
  if (rx > 0)
    if (int rc = mo::launch_pass(s, to_a, Z, Y, X, mo::Pass{2, rx, false}, who, st)) return rc;
  if (ry > 0)
    if (int rc = mo::launch_pass(a, to_b, Z, Y, X, mo::Pass{1, ry, false}, who, st)) return rc;
  const PeakSink sink{lsr::peaks::PeakTest{s, a, b, X, Y * X, rz, ry, rx, threshold}, cand_index, cand_value,
                      static_cast<unsigned long long>(capacity), count};
  if (int rc = mo::launch_strided(b, mo::lines_of(0, Z, Y, X), rz, false, sink, who, st)) return rc;
  return lsr::launch_status(who);
}

extern "C" int lsr_psf_accumulate_f32(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                                      int64_t n_beads, int pz, int py, int px, double* bead_stats, float* psf,
                                      lsr_stream_t stream) {
  if (int rc = lsr::peaks::check_psf_accumulate(vol, Z, Y, X, centres, n_beads, pz, py, px, bead_stats, psf)) return rc;
  hipStream_t st = lsr::as_stream(stream);
  lsr::peaks::launch_bead_stats(vol, Z, Y, X, centres, n_beads, pz, py, px, bead_stats, st);
  const int n = pz * py * px;
  hipLaunchKernelGGL(psf_accumulate_kernel, dim3(static_cast<unsigned>(lsr::ceil_div(n, 256))), dim3(256), 0, st, vol, Z, Y,
                     X, centres, static_cast<int>(n_beads), pz, py, px, bead_stats, psf);
  return lsr::launch_status("lsr_psf_accumulate_f32");
}
