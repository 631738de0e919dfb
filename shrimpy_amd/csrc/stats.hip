// Whole-volume statistics (shrimpy_amd/stats.py; the `statistics` command): one digit pass of a radix select over every voxel
// of a volume, the moment record, and the elementwise rescale.  The rule, the record, the geometry and the entry checks are
// stats.hpp's; tests/stats_ref.py restates the rule in numpy.
//
// The digit pass has the form of the other table kernels (moments.hip, intensity.hip): a contiguous span per workgroup under a
// grid cap, walked in strides of kStep; the kChunks loads of a stride (kLane voxels each: 16 bytes of float32, 8 of uint16) are
// issued before the first is used; up to kMaxRanks tables of 32-bit counters in LDS, one per prefix still alive, flushed by
// 64-bit global adds at the end of the span and every kFlushStrides strides, long before a counter could wrap.
//
//   contention   the workload's own: a deskewed volume is a quarter exact zeros and a bright-field stack is constant in its top
//                digits, so the 64 lanes of a wave step hit one bin.  kFormRuns: lanes whose slot (table and bin) equals the lane
//                before them form a run (one ballot); the run's head adds the run's length, the others add nothing.  kFormPlain:
//                one LDS add per voxel.  Both give the same tables; the bench times both.
//   moments      pass 0 with a record: every lane keeps count, nan_count, the two sums and the two codes in registers along its
//                span; a wave reduces them by shuffles once and lane 0 adds them to the record (64-bit global adds, the
//                hardware's float64 add for float32 values; atomicMax on the codes).
//   rescale      elementwise, 16-byte loads and stores, a grid-stride loop.
//
// Words shared inside a launch (the LDS tables between the barriers, the global tables, the record) are touched by atomics only
// (the zeroing of the LDS tables lies between barriers of its own), no workgroup ever waits for another, every loop is bounded.

#include <algorithm>
#include <type_traits>

#include "stats.hpp"

namespace {

namespace st = lsr::stats;

template <typename V>
using SumOf = typename std::conditional<std::is_same<V, float>::value, double, unsigned long long>::type;

__device__ __forceinline__ void add64(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
__device__ __forceinline__ void add64(unsigned long long* p, double v) { unsafeAtomicAdd(reinterpret_cast<double*>(p), v); }

template <typename V>
struct alignas(sizeof(V) * st::kLane) Quad {
  V e[st::kLane];
};

__device__ __forceinline__ void flush_tables(unsigned* lds, unsigned long long* tables) {
  for (int i = threadIdx.x; i < st::kMaxRanks * st::kBins; i += st::kThreads) {
    const unsigned c = lds[i];
    if (c == 0u) continue;                             // (a slot of a table the call does not have is never raised)
    atomicAdd(&tables[i], static_cast<unsigned long long>(c));
    lds[i] = 0u;
  }
}

template <typename V, bool kRuns, bool kMoments>
__global__ __launch_bounds__(st::kThreads) void digit_histogram_kernel(const V* __restrict__ in, int64_t n, int64_t span,
                                                                       st::Plan plan, int64_t flush_strides,
                                                                       unsigned long long* tables, unsigned long long* moments) {
  using S = SumOf<V>;
  __shared__ unsigned lds[st::kMaxRanks * st::kBins];
  for (int i = threadIdx.x; i < st::kMaxRanks * st::kBins; i += st::kThreads) lds[i] = 0u;
  __syncthreads();

  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * span, last = first + span < n ? first + span : n;
  unsigned long long count = 0ull, nans = 0ull;
  S sum = 0, sum_sq = 0;
  unsigned kmin = 0u, kmax = 0u;
  int64_t strides = 0;

  // (the loop's bounds are the workgroup's: every wave makes the same number of trips, every lane reaches the ballots, the
  // shuffles and the barriers)
  for (int64_t base = first; base < last; base += st::kStep) {
    Quad<V> q[st::kChunks];
    unsigned valid[st::kChunks];
#pragma unroll
    for (int c = 0; c < st::kChunks; ++c) {
      const int64_t v = base + ((wave * st::kChunks + c) * lsr::kWave + lane) * st::kLane;      // (a multiple of kLane: aligned)
      if (v + st::kLane <= last) {                     // (a span ends where the next begins: last <= n)
        q[c] = *reinterpret_cast<const Quad<V>*>(in + v);
        valid[c] = (1u << st::kLane) - 1u;
      } else {
        valid[c] = 0u;
#pragma unroll
        for (int e = 0; e < st::kLane; ++e) {
          const bool inside = v + e < last;
          q[c].e[e] = inside ? in[v + e] : V(0);
          valid[c] |= inside ? 1u << e : 0u;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < st::kChunks; ++c) {
#pragma unroll
      for (int e = 0; e < st::kLane; ++e) {
        const V x = q[c].e[e];
        const bool inside = (valid[c] >> e) & 1u, nan = st::is_nan(x);
        const unsigned key = st::key_of(x);
        const int slot = inside && !nan ? st::slot_of(plan, key) : -1;
        if (kMoments) {
          if (inside && nan) nans += 1ull;
          if (inside && !nan) {
            const S g = static_cast<S>(x);
            count += 1ull;
            sum += g;
            sum_sq += g * g;
            kmin = max(kmin, ~key);
            kmax = max(kmax, key);
          }
        }
        if (kRuns) {
          const int before = __shfl_up(slot, 1);
          const unsigned long long heads = __ballot(lane == 0 || slot != before);
          if (slot < 0 || !((heads >> lane) & 1ull)) continue;
          // the run ends in front of the next head above this lane (or with the wave)
          const unsigned long long above = heads & ~((2ull << lane) - 1ull);      // (lane 63: 2 << 63 == 0, nothing above)
          const int end = above != 0ull ? __ffsll(static_cast<long long>(above)) - 2 : lsr::kWave - 1;
          atomicAdd(&lds[slot], static_cast<unsigned>(end - lane + 1));
        } else {
          if (slot >= 0) atomicAdd(&lds[slot], 1u);
        }
      }
    }
    if (++strides == flush_strides && base + st::kStep < last) {       // (workgroup-uniform)
      strides = 0;
      __syncthreads();
      flush_tables(lds, tables);
      __syncthreads();
    }
  }
  __syncthreads();
  flush_tables(lds, tables);

  if (!kMoments) return;
#pragma unroll
  for (int d = lsr::kWave / 2; d > 0; d >>= 1) {
    count += __shfl_down(count, d);
    nans += __shfl_down(nans, d);
    sum += __shfl_down(sum, d);
    sum_sq += __shfl_down(sum_sq, d);
    kmin = max(kmin, __shfl_down(kmin, d));
    kmax = max(kmax, __shfl_down(kmax, d));
  }
  if (lane != 0) return;
  if (nans != 0ull) atomicAdd(&moments[1], nans);
  if (count == 0ull) return;
  atomicAdd(&moments[0], count);
  add64(&moments[2], sum);
  add64(&moments[3], sum_sq);
  unsigned* codes = reinterpret_cast<unsigned*>(moments + 4);
  atomicMax(&codes[0], kmin);
  atomicMax(&codes[1], kmax);
}

template <typename V>
__global__ __launch_bounds__(st::kThreads) void rescale_kernel(const V* in, int64_t n, float sub, float div, bool clip, float lo,
                                                               float hi, float* out) {
  constexpr int kPer = 16 / sizeof(V);
  struct alignas(16) In {
    V e[kPer];
  };
  const int64_t stride = static_cast<int64_t>(gridDim.x) * st::kThreads * kPer;
  for (int64_t v = (static_cast<int64_t>(blockIdx.x) * st::kThreads + threadIdx.x) * kPer; v < n; v += stride) {
    if (v + kPer <= n) {
      const In x = *reinterpret_cast<const In*>(in + v);
#pragma unroll
      for (int h = 0; h < kPer / 4; ++h) {
        float4 o;
        o.x = st::rescale_one(x.e[4 * h + 0], sub, div, clip, lo, hi);
        o.y = st::rescale_one(x.e[4 * h + 1], sub, div, clip, lo, hi);
        o.z = st::rescale_one(x.e[4 * h + 2], sub, div, clip, lo, hi);
        o.w = st::rescale_one(x.e[4 * h + 3], sub, div, clip, lo, hi);
        *reinterpret_cast<float4*>(out + v + 4 * h) = o;
      }
    } else {
      for (int64_t i = v; i < n; ++i) out[i] = st::rescale_one(in[i], sub, div, clip, lo, hi);
    }
  }
}

template <typename V>
int launch_histogram(const char* what, const V* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank, int k,
                     void* tables, void* moments, int grid_cap, int form, lsr_stream_t stream) {
  st::Plan plan;
  if (int rc = st::check_histogram(in, sizeof(V), n, pass, prefixes, table_of_rank, k, tables, moments, grid_cap, form, &plan)) return rc;
  const int64_t cap = std::min<int64_t>(grid_cap > 0 ? grid_cap : st::kDefaultBlocks, st::kMaxBlocks);
  const int64_t steps = lsr::ceil_div(n, st::kStep);
  const int64_t span = lsr::ceil_div(steps, std::min(steps, cap)) * st::kStep;       // voxels per workgroup, whole strides
  const dim3 grid(static_cast<unsigned>(lsr::ceil_div(n, span))), block(st::kThreads);
  const int64_t flush = (form >> 8) > 0 ? (form >> 8) : st::kFlushStrides;
  const bool runs = (form & 0xff) == st::kFormRuns;
  unsigned long long* t = static_cast<unsigned long long*>(tables);
  unsigned long long* m = static_cast<unsigned long long*>(moments);
  hipStream_t q = lsr::as_stream(stream);
  if (runs && m != nullptr)
    hipLaunchKernelGGL((digit_histogram_kernel<V, true, true>), grid, block, 0, q, in, n, span, plan, flush, t, m);
  else if (runs)
    hipLaunchKernelGGL((digit_histogram_kernel<V, true, false>), grid, block, 0, q, in, n, span, plan, flush, t, m);
  else if (m != nullptr)
    hipLaunchKernelGGL((digit_histogram_kernel<V, false, true>), grid, block, 0, q, in, n, span, plan, flush, t, m);
  else
    hipLaunchKernelGGL((digit_histogram_kernel<V, false, false>), grid, block, 0, q, in, n, span, plan, flush, t, m);
  return lsr::launch_status(what);
}

template <typename V>
int launch_rescale(const char* what, const V* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                   lsr_stream_t stream) {
  if (int rc = st::check_rescale(in, sizeof(V), n, clip, lo, hi, out)) return rc;
  constexpr int kPer = 16 / sizeof(V);
  const int64_t blocks = std::min<int64_t>(lsr::ceil_div(n, int64_t(st::kThreads) * kPer), 1 << 16);
  hipLaunchKernelGGL(rescale_kernel<V>, dim3(static_cast<unsigned>(blocks)), dim3(st::kThreads), 0, lsr::as_stream(stream), in, n, sub,
                     div, clip != 0, lo, hi, out);
  return lsr::launch_status(what);
}

}  // namespace

extern "C" int lsr_volume_stats_geometry(int64_t out[8]) {
  LSR_REQUIRE_PTR(out);
  out[0] = st::kDigitBits;
  out[1] = st::kBins;
  out[2] = st::kMaxRanks;
  out[3] = st::kThreads;
  out[4] = st::kWaveStep;
  out[5] = st::kDefaultBlocks;
  out[6] = st::kLdsBytes;
  out[7] = st::kPassesF32;                             // (a uint16 volume takes ceil(16 / out[0]) passes)
  return LSR_OK;
}

extern "C" int lsr_digit_histogram_f32(const float* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank,
                                       int k, void* tables, void* moments, int grid_cap, int form, lsr_stream_t stream) {
  return launch_histogram("lsr_digit_histogram_f32", in, n, pass, prefixes, table_of_rank, k, tables, moments, grid_cap, form, stream);
}

extern "C" int lsr_digit_histogram_u16(const uint16_t* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank,
                                       int k, void* tables, void* moments, int grid_cap, int form, lsr_stream_t stream) {
  return launch_histogram("lsr_digit_histogram_u16", in, n, pass, prefixes, table_of_rank, k, tables, moments, grid_cap, form, stream);
}

extern "C" int lsr_rescale_f32(const float* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                               lsr_stream_t stream) {
  return launch_rescale("lsr_rescale_f32", in, n, sub, div, clip, lo, hi, out, stream);
}

extern "C" int lsr_rescale_u16(const uint16_t* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                               lsr_stream_t stream) {
  return launch_rescale("lsr_rescale_u16", in, n, sub, div, clip, lo, hi, out, stream);
}
