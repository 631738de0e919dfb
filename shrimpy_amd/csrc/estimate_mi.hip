// Mutual-information metric of the affine registration estimate (label-free <-> fluorescence: two channels whose
// intensities are related by no linear map).  Mattes-style: a joint histogram of target intensity against interpolated
// moving intensity, zero-order bins on the target and a linear Parzen window on the moving value, on the conventions of
// estimate_affine.hip (mi_sample.hpp holds the per-sample rule, shared with the host twins in estimators_host.hip).
// No reference code exists for this step.
//
//   lsr_affine_joint_histogram_f32   hist[bins][bins] (uint64, units of 2^-16 sample) and the sample count
//   lsr_affine_mi_gradient_f32       12 fp64 sums of dL[a][b0] * du/dm * grad M (x) x~, per workgroup
//
// Histogram.  Every wave keeps a private bins x bins table of 32-bit counters in LDS (4 waves x 64^2 x 4 B = 64 KB at
// the largest size) and adds it to the global 64-bit histogram with integer atomics; the entry zeroes the histogram on
// the stream first.  Integer adds are exact and commute: the result is the same on every run and equals the twin's.
// Overflow: one wave iteration adds at most 64 x 65536 = 2^22 to a cell, and a wave flushes its table every kFlushEvery
// = 1000 iterations (< 2^32 / 2^22), so a 32-bit cell cannot wrap at any size; the global cells hold 65536 n < 2^64 for
// every volume the entry accepts (n < 2^48 voxels, LSR_REQUIRE_VOLUME).
// Contention.  Real volumes are mostly background: many lanes of a wave hit ONE cell, the worst case of an LDS atomic
// (same-address adds of a wave are served one after another).  Two forms were measured (DESIGN.md 4.8,
// profiles/mi_config3.jsonl).  Kept, LSR_MI_MERGE = 0: every lane adds its two weights to its wave's table on its own
// -- the tables being private to a wave already keeps the four waves off each other, and the walk is bound by its fp64
// arithmetic and gathers, not by the adds.  Dropped, LSR_MI_MERGE = 1 (kept behind the macro so that the measurement
// can be repeated): the lanes that share the first active lane's cell are merged -- a ballot, one wave sum of their
// upper-bin weights -- into two adds by one lane; the ballot and the six shuffles cost more than the serialised adds
// they save, on a background-dominated volume too.
//
// Gradient.  The scheme of estimate_affine.hip: 12 fp64 sums per thread in registers over a grid-stride walk, a wave
// reduction, the workgroup's four waves in wave order, one row per workgroup; the host adds the rows in row order.  No
// atomics, a fixed summation order.  dL (at most 64 x 63 doubles) is staged in LDS.

#include "mi_sample.hpp"

#ifndef LSR_MI_MERGE
#define LSR_MI_MERGE 0
#endif

namespace {

using namespace lsr::mi;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kHistBlocks = 512;      // two workgroups per CU: 2 x 64 KB of LDS at 64 bins
constexpr int kGradBlocks = 512;
constexpr int kFlushEvery = 1000;     // wave iterations between two flushes of a wave's table: 1000 * 2^22 < 2^32

static_assert(static_cast<int64_t>(kFlushEvery) * 64 * kWeightOne < (int64_t(1) << 32), "a 32-bit LDS cell must not wrap");

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// a wave's table -> the global histogram; the table is the wave's own, so the wave's program order is all the ordering
// it needs (the fences keep the compiler from moving the plain accesses across the atomics)
__device__ __forceinline__ void flush(unsigned* mine, unsigned long long* hist, int cells, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (int i = lane; i < cells; i += 64) {
    const unsigned v = mine[i];
    if (v != 0u) {
      mine[i] = 0u;
      atomicAdd(&hist[i], static_cast<unsigned long long>(v));
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

template <bool MERGE>
__global__ __launch_bounds__(kThreads) void joint_histogram_kernel(Geometry p, Binning q, unsigned long long* hist,
                                                                   unsigned long long* n_out) {
  extern __shared__ unsigned s_cells[];   // [kWaves][bins * bins]
  const int cells = q.bins * q.bins;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* mine = s_cells + wave * cells;
  for (int i = lane; i < cells; i += 64) mine[i] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

  const int64_t n_samples = static_cast<int64_t>(p.nz) * p.ny * p.nx;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  unsigned long long counted = 0;
  int since_flush = 0;
  // s0 is the same for the 64 lanes: the wave walks the loop together, whatever its lanes find
  for (int64_t s0 = static_cast<int64_t>(blockIdx.x) * kThreads + wave * 64; s0 < n_samples; s0 += step) {
    const int64_t s = s0 + lane;
    bool ok = false;
    int cell = 0;
    unsigned w1 = 0u;
    if (s < n_samples) {
      double tv, mval;
      ok = sample<false>(p, s, tv, mval, nullptr, nullptr);
      if (ok) {
        int b0;
        parzen(q, moving_position(q, mval), b0, w1);
        cell = target_bin(q, tv) * q.bins + b0;
        ++counted;
      }
    }
    if constexpr (MERGE) {
      const unsigned long long pending = __ballot(ok);
      if (pending != 0ull) {
        const int lead = __ffsll(static_cast<long long>(pending)) - 1;
        const int key = __shfl(cell, lead, 64);
        const bool same = ok && cell == key;
        const unsigned long long group = __ballot(same);
        const unsigned upper = wave_sum_u32(same ? w1 : 0u);
        if (lane == lead) {
          atomicAdd(&mine[key], static_cast<unsigned>(__popcll(group)) * kWeightOne - upper);
          if (upper != 0u) atomicAdd(&mine[key + 1], upper);
        } else if (ok && !same) {
          atomicAdd(&mine[cell], kWeightOne - w1);
          if (w1 != 0u) atomicAdd(&mine[cell + 1], w1);
        }
      }
    } else {
      if (ok) {
        atomicAdd(&mine[cell], kWeightOne - w1);
        if (w1 != 0u) atomicAdd(&mine[cell + 1], w1);
      }
    }
    if (++since_flush == kFlushEvery) {
      flush(mine, hist, cells, lane);
      since_flush = 0;
    }
  }
  flush(mine, hist, cells, lane);
  // the sample count: 64-bit per lane, summed over the wave in pieces whose 64-lane sums fit a 32-bit shuffle
  const unsigned lo = wave_sum_u32(static_cast<unsigned>(counted & 0xffffu));
  const unsigned hi = wave_sum_u32(static_cast<unsigned>((counted >> 16) & 0xffffu));
  const unsigned top = wave_sum_u32(static_cast<unsigned>(counted >> 32));
  if (lane == 0) {
    const unsigned long long total = static_cast<unsigned long long>(lo) + (static_cast<unsigned long long>(hi) << 16) +
                                     (static_cast<unsigned long long>(top) << 32);
    if (total != 0ull) atomicAdd(n_out, total);
  }
}

__global__ __launch_bounds__(kThreads) void mi_gradient_kernel(Geometry p, Binning q, Normalise c, const double* dl,
                                                               double* partial) {
  extern __shared__ double s_dl[];   // [bins][bins - 1]
  __shared__ double s_part[kWaves][kGradParams];
  const int n_dl = q.bins * (q.bins - 1);
  for (int i = threadIdx.x; i < n_dl; i += kThreads) s_dl[i] = dl[i];
  __syncthreads();

  double acc[kGradParams];
#pragma unroll
  for (int i = 0; i < kGradParams; ++i) acc[i] = 0.0;
  const double du = (q.bins - 1) / q.m_range;
  const int64_t n_samples = static_cast<int64_t>(p.nz) * p.ny * p.nx;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; s < n_samples;
       s += static_cast<int64_t>(gridDim.x) * kThreads) {
    double tv, mval, g[3], xyz[3];
    if (!sample<true>(p, s, tv, mval, g, xyz)) continue;
    gradient_add(q, c, s_dl, du, tv, mval, g, xyz, acc);
  }

  // wave sums, then the workgroup's four waves in wave order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kGradParams; ++i) {
    const double v = wave_sum(acc[i]);
    if (lane == 0) s_part[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kGradParams) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += s_part[w][threadIdx.x];
    partial[static_cast<int64_t>(blockIdx.x) * kGradParams + threadIdx.x] = v;
  }
}

}  // namespace

extern "C" int lsr_affine_joint_histogram_blocks(void) { return kHistBlocks; }
extern "C" int lsr_affine_mi_gradient_size(void) { return kGradParams; }
extern "C" int lsr_affine_mi_gradient_blocks(void) { return kGradBlocks; }

extern "C" int lsr_affine_joint_histogram_f32(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target,
                                              int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], const int stride[3],
                                              int bins, double t_lo, double t_hi, double m_lo, double m_hi,
                                              unsigned long long* hist, unsigned long long* n_samples,
                                              lsr_stream_t stream) {
  if (int rc = require_sampling(moving, Zi, Yi, Xi, target, Zo, Yo, Xo, M, stride, bins, t_lo, t_hi, m_lo, m_hi)) return rc;
  LSR_REQUIRE_PTR(hist);
  LSR_REQUIRE_PTR(n_samples);
  Geometry p;
  Binning q;
  fill(p, q, moving, Zi, Yi, Xi, target, Zo, Yo, Xo, M, stride, bins, t_lo, t_hi, m_lo, m_hi);
  hipStream_t s = lsr::as_stream(stream);
  const size_t cells = static_cast<size_t>(bins) * bins;
  hipError_t e = hipMemsetAsync(hist, 0, cells * sizeof(unsigned long long), s);
  if (e == hipSuccess) e = hipMemsetAsync(n_samples, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return lsr::fail(static_cast<int>(e), "lsr_affine_joint_histogram_f32: hipMemsetAsync: %s", hipGetErrorString(e));
  const size_t lds = kWaves * cells * sizeof(unsigned);   // <= 64 KB
  hipLaunchKernelGGL(joint_histogram_kernel<LSR_MI_MERGE != 0>, dim3(kHistBlocks), dim3(kThreads), lds, s, p, q, hist,
                     n_samples);
  return lsr::launch_status("lsr_affine_joint_histogram_f32");
}

extern "C" int lsr_affine_mi_gradient_f32(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target,
                                          int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], const int stride[3],
                                          const double centre[3], double scale, int bins, double t_lo, double t_hi,
                                          double m_lo, double m_hi, const double* dL, double* partial,
                                          lsr_stream_t stream) {
  if (int rc = require_sampling(moving, Zi, Yi, Xi, target, Zo, Yo, Xo, M, stride, bins, t_lo, t_hi, m_lo, m_hi)) return rc;
  LSR_REQUIRE_PTR(centre);
  LSR_REQUIRE_PTR(dL);
  LSR_REQUIRE_PTR(partial);
  LSR_REQUIRE(scale > 0.0, LSR_E_ARG, "scale must be positive");
  Geometry p;
  Binning q;
  fill(p, q, moving, Zi, Yi, Xi, target, Zo, Yo, Xo, M, stride, bins, t_lo, t_hi, m_lo, m_hi);
  const Normalise c{centre[0], centre[1], centre[2], 1.0 / scale};
  const size_t lds = static_cast<size_t>(bins) * (bins - 1) * sizeof(double);
  hipLaunchKernelGGL(mi_gradient_kernel, dim3(kGradBlocks), dim3(kThreads), lds, lsr::as_stream(stream), p, q, c, dL,
                     partial);
  return lsr::launch_status("lsr_affine_mi_gradient_f32");
}
