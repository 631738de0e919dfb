// Bead detection and PSF averaging (shrimpy_amd/psf.py; the stage scripts/measure_psf.py hands to biahub's
// _characterize_psf, which is not vendored: PARITY UNPINNED -- the rule is defined here and pinned to the NumPy / float64
// restatement tests/psf_ref.py).
//
// lsr_local_max_candidates_f32: the peaks of a smoothed volume s under a box window of half-widths (rz, ry, rx).  Voxel p
// is a peak iff  s(p) >= threshold,  s(p) >= s(q) for every in-volume q of its window  and  s(p) > s(q) for every such q
// with a smaller linear index (of tied maxima in reach of each other the first in C order wins).  A NaN compares false
// with everything: it is never a peak, and neither is a voxel with a NaN in its window.
//
// The box maximum is separable -- three passes, one per axis, each a van Herk / Gil-Werman running maximum (about three
// comparisons per voxel at ANY window width; the (2r+1)^3 gather of the definition is 10^5..10^6 reads per voxel at the
// reference's min_distance of 20..50):
//     A = max of s over the x window      rows staged in LDS, window maxima by doubling spans (1, 2, 4, ... <= w)
//     B = max of A over the y window      one thread per (column, block of w = 2r + 1 rows): the suffix maxima h of its
//     M = max of B over the z window        block go into a private LDS strip, the prefix maxima g of the next block run
//                                           in a register, out(i) = max(h(i), g(i + w - 1)); no barrier, rows of 64
//                                           consecutive floats per wave, every input read twice (once per side)
// Voxels outside the volume do not compete (-inf).  The z pass is fused with the test: M is never written; a voxel with
// s == M and s >= threshold (rare) then checks the tie rule along the three half-windows BELOW it in C order,
//     s(z, y, x') x' in [x - rx, x)      A(z, y', x) y' in [y - ry, y)      B(z', y, x) z' in [z - rz, z)
// -- together exactly the window's voxels of smaller linear index -- and appends (linear index, value) to the caller's
// buffer through ONE integer atomic counter.  The counter keeps counting past the capacity (nothing is stored there), so
// count > capacity tells the caller that the buffer was too small.  Append order is arbitrary: callers sort.
//
// lsr_psf_accumulate_f32: the average of background-subtracted, flux-normalised patches around the given centres.  Per
// bead (one workgroup, fixed tree: 256 strided partial sums in float64, then a binary tree): B = mean of the patch's
// outer shell, S = sum(patch - B).  Then one thread per PSF voxel adds (v - B) / S over the beads with S > 0 in list
// order in float64 and stores the mean as float32: the same bits on every run, and the host twin's.

#include "peaks.hpp"

namespace {

using lsr::peaks::nmax;
constexpr float kNegInf = -__builtin_inff();
constexpr int kRowThreads = 256;
constexpr int kRowSeg = 1024;                                      // outputs per staged row segment
constexpr int kRowBuf = kRowSeg + 2 * lsr::peaks::kMaxHalfWidth;   // + the window's reach on both sides

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

// ---- x: rows in LDS, doubling spans ----
__global__ __launch_bounds__(kRowThreads) void max_rows_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               int64_t rows, int X, int r, int seg, int nsegs) {
  __shared__ float buf[2][kRowBuf];
  const int tid = threadIdx.x, w = 2 * r + 1;
  for (int64_t item = blockIdx.x; item < rows * nsegs; item += gridDim.x) {
    const int64_t row = item / nsegs;
    const int x0 = static_cast<int>(item - row * nsegs) * seg;
    const int len = min(seg, X - x0), n = len + 2 * r;
    const float* src = in + row * X;
    for (int i = tid; i < n; i += kRowThreads) {
      const int x = x0 - r + i;
      buf[0][i] = (x >= 0 && x < X) ? src[x] : kNegInf;
    }
    __syncthreads();
    int cur = 0, span = 1;                  // buf[cur][i] = max over [i, i + span)
    for (; span * 2 <= w; span *= 2) {
      for (int i = tid; i + span < n; i += kRowThreads) buf[cur ^ 1][i] = nmax(buf[cur][i], buf[cur][i + span]);
      __syncthreads();
      cur ^= 1;
    }
    float* dst = out + row * X + x0;
    for (int t = tid; t < len; t += kRowThreads) dst[t] = nmax(buf[cur][t], buf[cur][t + w - span]);
    __syncthreads();                        // the next item overwrites both buffers
  }
}

// ---- y and z: one thread per (column, block of w positions) ----
struct MaxArgs {
  const float* in;
  float* out;              // not written by the fused pass
  int64_t L, inner;        // axis length, distance between its positions (outer index: blockIdx.z)
  int r;
  // the fused pass (axis z: L = Z, inner = Y * X, in = B)
  const float* s;
  const float* a;
  int X, ry, rx;
  float threshold;
  long long* cand_index;
  float* cand_value;
  long long capacity;
  unsigned long long* count;
};

template <bool FUSED>
__global__ void max_strided_kernel(MaxArgs p) {
  extern __shared__ float strip[];          // [w][blockDim.x]: this thread's suffix maxima
  const int nt = blockDim.x, tid = threadIdx.x;
  const int64_t col = static_cast<int64_t>(blockIdx.x) * nt + tid;
  if (col >= p.inner) return;               // (no barrier below)
  const int w = 2 * p.r + 1;
  const int64_t base = static_cast<int64_t>(blockIdx.z) * p.L * p.inner + col;
  const float* in = p.in + base;
  const int64_t i0 = static_cast<int64_t>(blockIdx.y) * w;   // first output of this block; its window starts at i0 - r
  const int64_t j0 = i0 - p.r;
  float run = kNegInf;
#pragma unroll 4
  for (int t = w - 1; t >= 0; --t) {
    const int64_t j = j0 + t;
    const float v = (j >= 0 && j < p.L) ? in[j * p.inner] : kNegInf;
    run = nmax(run, v);
    strip[t * nt + tid] = run;
  }
  float g = kNegInf;
#pragma unroll 4
  for (int t = 0; t < w; ++t) {
    const int64_t i = i0 + t;
    if (i >= p.L) break;
    if (t > 0) {
      const int64_t j = j0 + w + t - 1;
      g = nmax(g, j < p.L ? in[j * p.inner] : kNegInf);
    }
    const float m = nmax(strip[t * nt + tid], g);
    if constexpr (!FUSED) {
      p.out[base + i * p.inner] = m;
    } else {
      const int64_t lin = i * p.inner + col;
      const float sv = p.s[lin];
      if (sv == m && sv >= p.threshold) {
        // the window's voxels of smaller linear index, through the three partial maxima
        const int64_t y = col / p.X, x = col - y * p.X;
        bool tie = false;
        for (int64_t d = min(static_cast<int64_t>(p.rx), x); d > 0 && !tie; --d) tie = p.s[lin - d] >= sv;
        for (int64_t d = min(static_cast<int64_t>(p.ry), y); d > 0 && !tie; --d) tie = p.a[lin - d * p.X] >= sv;
        for (int64_t d = min(static_cast<int64_t>(p.r), i); d > 0 && !tie; --d) tie = p.in[lin - d * p.inner] >= sv;
        if (!tie) {
          const unsigned long long slot = atomicAdd(p.count, 1ull);
          if (slot < static_cast<unsigned long long>(p.capacity)) {
            p.cand_index[slot] = lin;
            p.cand_value[slot] = sv;
          }
        }
      }
    }
  }
}

// threads per workgroup of the strided passes: the LDS strip is w floats per thread, kept within 33 KB
int strided_threads(int r) {
  const int w = 2 * r + 1;
  return w <= 32 ? 256 : (w <= 64 ? 128 : 64);
}

int launch_strided(bool fused, MaxArgs p, int64_t outer, hipStream_t s) {
  const int nt = strided_threads(p.r), w = 2 * p.r + 1;
  const int64_t gx = lsr::ceil_div(p.inner, nt), gy = lsr::ceil_div(p.L, w);
  LSR_REQUIRE(gx < (int64_t(1) << 31) && gy < 65536 && outer < 65536, LSR_E_SHAPE,
              "grid (%lld, %lld, %lld) is too large", (long long)gx, (long long)gy, (long long)outer);
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy), static_cast<unsigned>(outer));
  const size_t lds = sizeof(float) * w * nt;
  if (fused) hipLaunchKernelGGL(max_strided_kernel<true>, grid, dim3(nt), lds, s, p);
  else hipLaunchKernelGGL(max_strided_kernel<false>, grid, dim3(nt), lds, s, p);
  return LSR_OK;
}

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
  float* a = static_cast<float*>(scratch);
  float* b = a + Z * Y * X;
  if (hipMemsetAsync(count, 0, sizeof(unsigned long long), st) != hipSuccess)
    return lsr::launch_status("lsr_local_max_candidates_f32");
  {
    const int64_t nsegs = lsr::ceil_div(X, kRowSeg);
    const int seg = static_cast<int>(lsr::ceil_div(lsr::ceil_div(X, nsegs), 4) * 4);
    const int64_t items = Z * Y * nsegs;
    const int64_t blocks = items < 256 * 64 ? items : 256 * 64;
    hipLaunchKernelGGL(max_rows_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kRowThreads), 0, st, s, a, Z * Y,
                       static_cast<int>(X), rx, seg, static_cast<int>(lsr::ceil_div(X, seg)));
  }
  MaxArgs p{};
  p.in = a; p.out = b; p.L = Y; p.inner = X; p.r = ry;
  if (int rc = launch_strided(false, p, Z, st)) return rc;
  p.in = b; p.out = nullptr; p.L = Z; p.inner = Y * X; p.r = rz;
  p.s = s; p.a = a; p.X = static_cast<int>(X); p.ry = ry; p.rx = rx;
  p.threshold = threshold;
  p.cand_index = cand_index; p.cand_value = cand_value; p.capacity = capacity; p.count = count;
  if (int rc = launch_strided(true, p, 1, st)) return rc;
  return lsr::launch_status("lsr_local_max_candidates_f32");
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
