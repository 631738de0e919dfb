// Per-bead 3-D Gaussian fits and the Fourier-shifted PSF average (shrimpy_amd/psf.py: fit_beads, average_psf_aligned; what
// biahub's _characterize_psf / waveorder's analyze_psf do on the host, not vendored: PARITY UNPINNED -- the rule is
// defined in psf_fit.hpp and pinned to the NumPy / float64 restatement tests/psf_fit_ref.py).
//
// lsr_bead_fit_f32: one workgroup of 256 per bead runs the Levenberg-Marquardt iteration of psf_fit.hpp.  Every pass
// re-reads the patch from global memory (it stays in L2; the pass is bound by its ~250 float64 operations per voxel),
// each lane keeps the 78 sums of its voxels e = lane, lane + 256, ... in registers (no scratch memory: the indices are
// constants after unrolling), a wave adds its lanes with a fixed butterfly, the four waves meet in LDS.  Thread 0 then
// solves the damped 11 x 11 system in LDS, the trial parameters go to every lane through LDS, a second pass gives the
// trial cost.  Device and twin agree to rounding (exp, the order of the sums), not to the bit.
//
// lsr_psf_accumulate_shifted_f32: per bead c = patch - B (B, S: bead_stats_kernel of peaks.hip), shifted by three
// separable circulant passes x, y, z with the caller's Dirichlet weights -- no transcendental here -- then shifted / S is
// added to a float64 accumulator in list order.  The intermediates do not fit LDS for large patches: a batch of
// kShiftBatch = 64 beads goes through the caller's scratch (one launch, one workgroup per bead, two float64 patches
// each), one launch adds the batch in list order, the last one stores float(acc / used).  Unfused multiply-adds with j
// ascending: the twin's bits for the same weights.

#include "psf_fit.hpp"

namespace {

namespace pf = lsr::psffit;
namespace pk = lsr::peaks;
constexpr int kThreads = pk::kTreeThreads;
constexpr int kWaves = kThreads / lsr::kWave;

// s[0..N) of every lane -> dst[0..N) (LDS): butterfly within the wave, the waves in order
template <int FIRST, int N>
__device__ __forceinline__ void reduce_sums(const double (&s)[pf::kSums], double (*part)[pf::kSums], double* dst) {
  const int tid = threadIdx.x, lane = tid & (lsr::kWave - 1), wave = tid / lsr::kWave;
#pragma unroll
  for (int k = FIRST; k < FIRST + N; ++k) {
    double v = s[k];
#pragma unroll
    for (int off = lsr::kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) part[wave][k] = v;
  }
  __syncthreads();
  if (tid >= FIRST && tid < FIRST + N) {
    double v = part[0][tid];
    for (int w = 1; w < kWaves; ++w) v += part[w][tid];
    dst[tid] = v;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void bead_fit_kernel(const float* __restrict__ vol, int64_t Z, int64_t Y, int64_t X,
                                                            const long long* __restrict__ centres, int pz, int py, int px,
                                                            int max_iter, double* __restrict__ fit, int* __restrict__ status) {
  __shared__ double red[kThreads];
  __shared__ double part[kWaves][pf::kSums];
  __shared__ double sums[pf::kSums];
  __shared__ pf::Lm lm;
  __shared__ int action;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int64_t z0 = 0, y0 = 0, x0 = 0;
  if (!pk::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0)) {      // (the same answer in every thread)
    if (tid < pf::kFitOut) fit[pf::kFitOut * b + tid] = __builtin_nan("");
    if (tid == 0) status[b] = pf::kBadInput;
    return;
  }
  const int n = pz * py * px, plane = py * px, hz = pz / 2, hy = py / 2, hx = px / 2;
  const float* corner = vol + (z0 * Y + y0) * X + x0;

  // the start: face mean (bead_stats_kernel's sum), the finite test, then the moments above the half maximum
  double a = 0.0;
  int bad = 0;
  for (int e = tid; e < n; e += kThreads) {
    const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
    const float v = corner[(iz * Y + iy) * X + ix];
    bad |= !(fabsf(v) <= 3.4028234663852886e38f);
    if (pk::on_shell(iz, iy, ix, pz, py, px)) a += static_cast<double>(v);
  }
  bad = __syncthreads_or(bad);
  const double bg = pk::tree_sum(red, a) / static_cast<double>(pk::shell_count(pz, py, px));
  if (bad) {
    if (tid < pf::kFitOut) fit[pf::kFitOut * b + tid] = __builtin_nan("");
    if (tid == 0) status[b] = pf::kBadInput;
    return;
  }
  const double centre = static_cast<double>(corner[(hz * Y + hy) * X + hx]);
  double s[pf::kSums];
#pragma unroll
  for (int k = 0; k < pf::kSums; ++k) s[k] = 0.0;
  {
    const double cut = bg + 0.5 * (centre - bg);
    for (int e = tid; e < n; e += kThreads) {
      const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
      const double g = static_cast<double>(corner[(iz * Y + iy) * X + ix]) - cut;
      if (g > 0.0) {
        const double rz = iz - hz, ry = iy - hy, rx = ix - hx;
        s[0] += g;
        s[1] += g * rz; s[2] += g * ry; s[3] += g * rx;
        s[4] += g * rz * rz; s[5] += g * ry * ry; s[6] += g * rx * rx;
      }
    }
  }
  reduce_sums<0, pf::kStartSums>(s, part, sums);
  if (tid == 0) action = pf::lm_start(lm, bg, centre, sums, max_iter) ? pf::kNeedSums : pf::kDone;
  __syncthreads();

  double t[pf::kParams];
  int act = action;                        // (read between two barriers every time: thread 0 writes it after the next one)
  while (act != pf::kDone) {
    if (act == pf::kNeedSums) {
#pragma unroll
      for (int k = 0; k < pf::kParams; ++k) t[k] = lm.theta[k];
#pragma unroll
      for (int k = 0; k < pf::kSums; ++k) s[k] = 0.0;
      for (int e = tid; e < n; e += kThreads) {
        const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
        pf::add_voxel<true>(t, static_cast<double>(corner[(iz * Y + iy) * X + ix]), iz - hz, iy - hy, ix - hx, s);
      }
      reduce_sums<0, pf::kSums>(s, part, lm.sums);
      if (tid == 0) lm.cost = lm.sums[pf::kSums - 1];
    }
    __syncthreads();
    if (tid == 0) action = pf::lm_solve(lm) ? pf::kNeedSolve : pf::kDone;
    __syncthreads();
    act = action;
    if (act == pf::kDone) break;
#pragma unroll
    for (int k = 0; k < pf::kParams; ++k) t[k] = lm.trial[k];
    s[pf::kSums - 1] = 0.0;
    for (int e = tid; e < n; e += kThreads) {
      const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
      pf::add_voxel<false>(t, static_cast<double>(corner[(iz * Y + iy) * X + ix]), iz - hz, iy - hy, ix - hx, s);
    }
    reduce_sums<pf::kSums - 1, 1>(s, part, sums);
    if (tid == 0) action = pf::lm_judge(lm, sums[pf::kSums - 1]);
    __syncthreads();
    act = action;
  }
  if (tid == 0) status[b] = pf::lm_finish(lm, fit + pf::kFitOut * b);
}

// ---- the shifted average ----
// One workgroup per bead of the batch: c = patch - B through the x, y and z passes into the bead's two scratch patches
// (the result ends in the first).  A bead that does not contribute -- S <= 0, a patch that does not fit, a non-finite
// weight -- only clears its flag.
__global__ __launch_bounds__(kThreads) void shift_batch_kernel(const float* __restrict__ vol, int64_t Z, int64_t Y, int64_t X,
                                                               const long long* __restrict__ centres, int first, int pz,
                                                               int py, int px, const double* __restrict__ stats,
                                                               const double* __restrict__ weights, double* flags,
                                                               double* patches) {
  __shared__ double w[3 * pk::kMaxPatch];
  const int tid = threadIdx.x, slot = blockIdx.x;
  const int64_t b = static_cast<int64_t>(first) + slot;
  const int nw = pz + py + px, n = pz * py * px, plane = py * px;
  int bad = 0;
  for (int k = tid; k < nw; k += kThreads) {
    const double v = weights[b * nw + k];
    w[k] = v;
    bad |= !(fabs(v) <= 1.7976931348623157e308);
  }
  bad = __syncthreads_or(bad);
  int64_t z0 = 0, y0 = 0, x0 = 0;
  const double bg = stats[2 * b], total = stats[2 * b + 1];
  const bool use = !bad && total > 0.0 && pk::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0);
  if (tid == 0) flags[slot] = use ? 1.0 : 0.0;
  if (!use) return;
  const float* corner = vol + (z0 * Y + y0) * X + x0;
  double* p0 = patches + static_cast<int64_t>(slot) * 2 * n;
  double* p1 = p0 + n;
  const double *wz = w, *wy = w + pz, *wx = w + pz + py;
  for (int e = tid; e < n; e += kThreads) {
    const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
    p0[e] = pf::circulant(corner + (iz * Y + iy) * X, int64_t(1), bg, wx, px, ix);
  }
  __syncthreads();
  for (int e = tid; e < n; e += kThreads) {
    const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
    p1[e] = pf::circulant(p0 + iz * plane + ix, int64_t(px), 0.0, wy, py, iy);
  }
  __syncthreads();
  for (int e = tid; e < n; e += kThreads) {
    const int iz = e / plane, rem = e - iz * plane;
    p0[e] = pf::circulant(p1 + rem, int64_t(plane), 0.0, wz, pz, iz);
  }
}

// acc += shifted / S over the batch in list order; thread 0 of the grid keeps the count
__global__ __launch_bounds__(256) void shift_add_kernel(int first, int count, int n, const double* __restrict__ stats,
                                                        const double* __restrict__ flags,
                                                        const double* __restrict__ patches, double* __restrict__ acc,
                                                        double* __restrict__ used, int clear) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  double a = clear ? 0.0 : acc[e];
  int k = 0;
  for (int slot = 0; slot < count; ++slot) {
    if (flags[slot] == 0.0) continue;
    a += patches[static_cast<int64_t>(slot) * 2 * n + e] / stats[2 * (static_cast<int64_t>(first) + slot) + 1];
    ++k;
  }
  acc[e] = a;
  if (e == 0) *used = (clear ? 0.0 : *used) + static_cast<double>(k);
}

__global__ __launch_bounds__(256) void shift_store_kernel(int n, const double* __restrict__ acc,
                                                          const double* __restrict__ used, float* __restrict__ psf) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const double u = *used;
  psf[e] = u > 0.0 ? static_cast<float>(acc[e] / u) : 0.0f;
}

}  // namespace

extern "C" int lsr_bead_fit_f32(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n_beads,
                                int pz, int py, int px, int max_iter, double* fit, int* status, lsr_stream_t stream) {
  if (int rc = pf::check_bead_fit(vol, Z, Y, X, centres, n_beads, pz, py, px, max_iter, fit, status)) return rc;
  hipLaunchKernelGGL(bead_fit_kernel, dim3(static_cast<unsigned>(n_beads)), dim3(kThreads), 0, lsr::as_stream(stream), vol, Z,
                     Y, X, centres, pz, py, px, max_iter, fit, status);
  return lsr::launch_status("lsr_bead_fit_f32");
}

extern "C" int lsr_psf_shift_scratch_bytes(int64_t n_beads, int pz, int py, int px, int64_t* bytes) {
  LSR_REQUIRE_PTR(bytes);
  if (int rc = pk::check_patches(pz, py, px, n_beads, pz, py, px)) return rc;      // (no volume here: the patch stands in)
  *bytes = pf::shift_scratch_bytes(n_beads, pz, py, px);
  return LSR_OK;
}

extern "C" int lsr_psf_accumulate_shifted_f32(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                                              int64_t n_beads, int pz, int py, int px, double* bead_stats,
                                              const double* weights, void* scratch, float* psf, lsr_stream_t stream) {
  if (int rc = pf::check_psf_shift(vol, Z, Y, X, centres, n_beads, pz, py, px, bead_stats, weights, psf)) return rc;
  LSR_REQUIRE_PTR(scratch);
  LSR_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, LSR_E_ARG, "scratch must be 8-byte aligned");
  hipStream_t st = lsr::as_stream(stream);
  pk::launch_bead_stats(vol, Z, Y, X, centres, n_beads, pz, py, px, bead_stats, st);
  const int n = pz * py * px;
  double* acc = static_cast<double*>(scratch);
  double* used = acc + n;
  double* flags = used + 1;
  double* patches = acc + pf::shift_head_doubles(n);
  const dim3 grid(static_cast<unsigned>(lsr::ceil_div(n, 256)));
  for (int64_t first = 0; first < n_beads; first += pf::kShiftBatch) {
    const int count = static_cast<int>(n_beads - first < pf::kShiftBatch ? n_beads - first : pf::kShiftBatch);
    hipLaunchKernelGGL(shift_batch_kernel, dim3(static_cast<unsigned>(count)), dim3(kThreads), 0, st, vol, Z, Y, X, centres,
                       static_cast<int>(first), pz, py, px, bead_stats, weights, flags, patches);
    hipLaunchKernelGGL(shift_add_kernel, grid, dim3(256), 0, st, static_cast<int>(first), count, n, bead_stats, flags, patches,
                       acc, used, first == 0 ? 1 : 0);
  }
  hipLaunchKernelGGL(shift_store_kernel, grid, dim3(256), 0, st, n, acc, used, psf);
  return lsr::launch_status("lsr_psf_accumulate_shifted_f32");
}
