// The intensities every object of a label volume holds in another volume (shrimpy_amd/segment.py: intensity_table; the `measure`
// command).  The rule, the two records, the codes of the extremes and the entry checks are intensity.hpp's;
// tests/intensity_ref.py restates the rule in numpy.
//
// The form is moments.hip's (read its header): a contiguous span per workgroup walked in strides of kStep, run heads from one
// __ballot, a per-workgroup open-addressing table in LDS, one flush.  What differs:
//
//   loads    two streams, labels and values, each read once: the 2 * kChunks loads of a stride are issued before the first is
//            used.  A wave step without a label in 1 .. n is left after its ballot.
//   runs     a run's sums are not closed forms: sum_v, sum_vv, sum_vx and the two codes of the extremes come from a shuffle
//            reduction restricted to the run (label.hip's absorb: lane + d takes part where it is not past the run's last lane),
//            the count is the run's length from the bit scan, and sum_vz = z * sum_v, sum_vy = y * sum_v are formed once per
//            run (z and y are constant along it: intensity.hpp's second n_k).  uint16 values take the same path in uint64.
//   LDS      per slot six 64-bit sums, two 32-bit codes and the int32 key, field-major.  atomicCAS on the key; 64-bit LDS atomic
//            adds -- for the float64 sums the hardware's ds_add_f64 through unsafeAtomicAdd, never a compare-and-swap loop;
//            atomicMax on the codes (the minimum as the maximum of the complemented code, as label.hip does).
//   flush    six global 64-bit atomic adds and two atomicMax per occupied slot; a finishing launch over the n records turns the
//            two codes back into values, as label_regions_finish_kernel does.
//
// The two hard rules of label.hip hold: words shared inside a launch (the LDS table between the barriers, the global table)
// are touched by atomics only, and no workgroup ever waits for another; every loop is bounded.

#include <algorithm>
#include <type_traits>

#include "intensity.hpp"

namespace {

namespace in = lsr::intensity;
namespace lb = lsr::label;

struct Shape {
  int Z, Y, X;
};

// float32 values are summed in float64, uint16 values in uint64
template <typename V>
using SumOf = typename std::conditional<std::is_same<V, float>::value, double, unsigned long long>::type;

__device__ __forceinline__ void add64(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
__device__ __forceinline__ void add64(unsigned long long* p, double v) { unsafeAtomicAdd(reinterpret_cast<double*>(p), v); }
__device__ __forceinline__ bool is_zero(unsigned long long v) { return v == 0ull; }
__device__ __forceinline__ bool is_zero(double v) { return __double_as_longlong(v) == 0ll; }      // (+0.0 only: adding it is a no-op)

// One run's contribution: the count, the five sums (as the 64-bit words of the record) and the two codes.
template <typename S>
struct Run {
  unsigned long long count;
  S s[in::kSums - 1];                       // sum_v, sum_vv, sum_vz, sum_vy, sum_vx
  unsigned kmin, kmax;                      // ~code and code: both under max
};

template <typename S>
__device__ __forceinline__ void global_add(unsigned long long* table, int label, const Run<S>& r) {
  unsigned long long* rec = table + static_cast<int64_t>(label - 1) * in::kWords;
  atomicAdd(&rec[0], r.count);
#pragma unroll
  for (int k = 1; k < in::kSums; ++k) add64(&rec[k], r.s[k - 1]);
  unsigned* codes = reinterpret_cast<unsigned*>(rec + in::kSums);
  atomicMax(&codes[0], r.kmin);
  atomicMax(&codes[1], r.kmax);
}

// kLds = false is the plain form (every head straight to the global record), kept for the measurement entry.
template <typename V, bool kLds>
__global__ __launch_bounds__(in::kThreads) void label_intensity_kernel(const int* __restrict__ labels, const V* __restrict__ values,
                                                                       Shape s, int n_objects, int64_t n, int64_t span, int slots,
                                                                       int probes, unsigned long long* table) {
  using S = SumOf<V>;
  extern __shared__ unsigned long long lds[];       // kSums * slots sums (field-major), 2 * slots codes (field-major), slots keys
  unsigned long long* sums = lds;
  unsigned* codes = reinterpret_cast<unsigned*>(lds + in::kSums * slots);
  int* keys = reinterpret_cast<int*>(codes + 2 * slots);
  const int slot_mask = slots - 1;
  if (kLds) {
    for (int i = threadIdx.x; i < in::kSums * slots; i += in::kThreads) sums[i] = 0ull;
    for (int i = threadIdx.x; i < 2 * slots; i += in::kThreads) codes[i] = 0u;
    for (int i = threadIdx.x; i < slots; i += in::kThreads) keys[i] = 0;
    __syncthreads();
  }

  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const unsigned X = static_cast<unsigned>(s.X), Y = static_cast<unsigned>(s.Y);
  const int64_t first = static_cast<int64_t>(blockIdx.x) * span, last = first + span < n ? first + span : n;

  // (the loop's bounds are the workgroup's: every wave makes the same number of trips, every lane of a wave reaches the ballots
  // and the shuffles)
  for (int64_t base = first; base < last; base += in::kStep) {
    int lab[in::kChunks];
    V val[in::kChunks];
#pragma unroll
    for (int c = 0; c < in::kChunks; ++c) {
      const int64_t v = base + (wave * in::kChunks + c) * lsr::kWave + lane;
      lab[c] = v < last ? labels[v] : 0;              // (a span ends where the next workgroup's begins: v < last <= n)
    }
#pragma unroll
    for (int c = 0; c < in::kChunks; ++c) {
      const int64_t v = base + (wave * in::kChunks + c) * lsr::kWave + lane;
      val[c] = v < last ? values[v] : V(0);
    }
#pragma unroll
    for (int c = 0; c < in::kChunks; ++c) {
      const int64_t v = base + (wave * in::kChunks + c) * lsr::kWave + lane;
      const int l = (lab[c] >= 1 && lab[c] <= n_objects) ? lab[c] : 0;
      if (__ballot(l != 0) == 0ull) continue;           // (wave-uniform)
      const unsigned uv = static_cast<unsigned>(v);     // (v < 2^31 + kStep)
      const unsigned row = uv / X, x = uv - row * X;
      const int before = __shfl_up(l, 1);
      const unsigned long long heads = __ballot(lane == 0 || l != before || x == 0u);
      // the run this lane lies in ends in front of the next head above the lane (or with the wave)
      const unsigned long long above = heads & ~((2ull << lane) - 1ull);       // (lane 63: 2 << 63 == 0, nothing above)
      const int end = above != 0ull ? __ffsll(static_cast<long long>(above)) - 2 : lsr::kWave - 1;      // the run's last lane
      const S g = static_cast<S>(val[c]);
      S sv = g, svv = g * g, svx = g * static_cast<S>(x);
      unsigned kmax = in::code_of(val[c]), kmin = ~kmax;
      // the segmented reduction: after the step d a lane holds the sums of lanes lane .. min(lane + 2d - 1, end)
#pragma unroll
      for (int d = 1; d < lsr::kWave; d <<= 1) {
        const S ov = __shfl_down(sv, d), ovv = __shfl_down(svv, d), ovx = __shfl_down(svx, d);
        const unsigned omin = __shfl_down(kmin, d), omax = __shfl_down(kmax, d);
        if (lane + d <= end) {
          sv += ov;
          svv += ovv;
          svx += ovx;
          kmin = max(kmin, omin);
          kmax = max(kmax, omax);
        }
      }
      if (l == 0 || !((heads >> lane) & 1ull)) continue;
      const unsigned z = row / Y, y = row - z * Y;
      Run<S> r;
      r.count = static_cast<unsigned long long>(end - lane + 1);
      r.s[0] = sv;
      r.s[1] = svv;
      r.s[2] = sv * static_cast<S>(z);
      r.s[3] = sv * static_cast<S>(y);
      r.s[4] = svx;
      r.kmin = kmin;
      r.kmax = kmax;
      bool placed = false;
      if (kLds) {
        int slot = l & slot_mask;
        for (int p = 0; p < probes; ++p, slot = (slot + 1) & slot_mask) {
          const int old = atomicCAS(&keys[slot], 0, l);
          if (old == 0 || old == l) {
            atomicAdd(&sums[slot], r.count);
#pragma unroll
            for (int k = 1; k < in::kSums; ++k) add64(&sums[k * slots + slot], r.s[k - 1]);
            atomicMax(&codes[slot], r.kmin);
            atomicMax(&codes[slots + slot], r.kmax);
            placed = true;
            break;
          }
        }
      }
      if (!placed) global_add(table, l, r);
    }
  }
  if (!kLds) return;
  __syncthreads();

  for (int i = threadIdx.x; i < in::kSums * slots; i += in::kThreads) {
    const int slot = i & slot_mask, k = i / slots;
    const int l = keys[slot];
    if (l == 0) continue;
    unsigned long long* rec = table + static_cast<int64_t>(l - 1) * in::kWords;
    if (k == 0) {
      atomicAdd(&rec[0], sums[i]);
    } else {
      S sum;
      memcpy(&sum, &sums[i], sizeof(sum));
      if (!is_zero(sum)) add64(&rec[k], sum);
    }
  }
  for (int i = threadIdx.x; i < 2 * slots; i += in::kThreads) {
    const int slot = i & slot_mask, k = i / slots;
    const int l = keys[slot];
    if (l != 0) atomicMax(reinterpret_cast<unsigned*>(table + static_cast<int64_t>(l - 1) * in::kWords + in::kSums) + k, codes[i]);
  }
}

// From the two codes back to values: v_min = decode(~word), v_max = decode(word).  A label no voxel carries keeps its zeros.
template <typename V>
__global__ __launch_bounds__(in::kThreads) void label_intensity_finish_kernel(unsigned long long* table, int n_objects) {
  const int k = blockIdx.x * in::kThreads + threadIdx.x;
  if (k >= n_objects) return;
  unsigned long long* rec = table + static_cast<int64_t>(k) * in::kWords;
  if (rec[0] == 0ull) return;
  unsigned* codes = reinterpret_cast<unsigned*>(rec + in::kSums);
  const unsigned kmin = ~codes[0], kmax = codes[1];
  if (std::is_same<V, float>::value) {
    const float lo = lb::key_float(kmin), hi = lb::key_float(kmax);
    memcpy(&codes[0], &lo, sizeof(lo));
    memcpy(&codes[1], &hi, sizeof(hi));
  } else {
    codes[0] = kmin;
    codes[1] = kmax;
  }
}

template <typename V>
int launch_intensity(const char* what, const int32_t* labels, const V* values, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                     void* table, int max_blocks, int slots, int probes, lsr_stream_t stream) {
  if (int rc = in::check_intensity(labels, values, sizeof(V), Z, Y, X, n_objects, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  const int64_t n = Z * Y * X;
  const int64_t cap = std::min<int64_t>(max_blocks > 0 ? max_blocks : in::kDefaultBlocks, in::kMaxBlocks);
  const int64_t steps = lsr::ceil_div(n, in::kStep);
  const int64_t span = lsr::ceil_div(steps, std::min(steps, cap)) * in::kStep;       // voxels per workgroup, whole strides
  const int64_t blocks = lsr::ceil_div(n, span);
  const Shape s{static_cast<int>(Z), static_cast<int>(Y), static_cast<int>(X)};
  unsigned long long* t = static_cast<unsigned long long*>(table);
  hipStream_t q = lsr::as_stream(stream);
  if (slots > 0) {
    const size_t lds = static_cast<size_t>(slots) * (in::kSums * sizeof(unsigned long long) + 2 * sizeof(unsigned) + sizeof(int));
    hipLaunchKernelGGL((label_intensity_kernel<V, true>), dim3(static_cast<unsigned>(blocks)), dim3(in::kThreads), lds, q, labels,
                       values, s, static_cast<int>(n_objects), n, span, slots, probes, t);
  } else {
    hipLaunchKernelGGL((label_intensity_kernel<V, false>), dim3(static_cast<unsigned>(blocks)), dim3(in::kThreads), 0, q, labels,
                       values, s, static_cast<int>(n_objects), n, span, 1, 0, t);
  }
  hipLaunchKernelGGL(label_intensity_finish_kernel<V>, dim3(static_cast<unsigned>(lsr::ceil_div(n_objects, in::kThreads))),
                     dim3(in::kThreads), 0, q, t, static_cast<int>(n_objects));
  return lsr::launch_status(what);
}

int check_variant(int lds_slots, int lds_probes) {
  LSR_REQUIRE(lds_slots >= 0 && lds_slots <= in::kMaxLdsSlots && (lds_slots & (lds_slots - 1)) == 0, LSR_E_ARG,
              "lds_slots %d: 0 (no LDS table) or a power of two up to %d", lds_slots, in::kMaxLdsSlots);
  LSR_REQUIRE(lds_probes >= 1 && lds_probes <= in::kMaxLdsSlots, LSR_E_ARG, "lds_probes %d: 1 .. %d", lds_probes,
              in::kMaxLdsSlots);
  return LSR_OK;
}

}  // namespace

extern "C" int lsr_label_intensity_geometry(int out[2]) {
  LSR_REQUIRE_PTR(out);
  out[0] = in::kLdsSlots;
  out[1] = in::kDefaultBlocks;
  return LSR_OK;
}

extern "C" int lsr_label_intensity_f32(const int32_t* labels, const float* values, int64_t Z, int64_t Y, int64_t X,
                                       int64_t n_objects, void* table, int max_blocks, lsr_stream_t stream) {
  return launch_intensity("lsr_label_intensity_f32", labels, values, Z, Y, X, n_objects, table, max_blocks, in::kLdsSlots,
                          in::kLdsProbes, stream);
}

extern "C" int lsr_label_intensity_u16(const int32_t* labels, const uint16_t* values, int64_t Z, int64_t Y, int64_t X,
                                       int64_t n_objects, void* table, int max_blocks, lsr_stream_t stream) {
  return launch_intensity("lsr_label_intensity_u16", labels, values, Z, Y, X, n_objects, table, max_blocks, in::kLdsSlots,
                          in::kLdsProbes, stream);
}

extern "C" int lsr_label_intensity_variant(const int32_t* labels, const void* values, int value_is_u16, int64_t Z, int64_t Y,
                                           int64_t X, int64_t n_objects, void* table, int max_blocks, int lds_slots,
                                           int lds_probes, lsr_stream_t stream) {
  if (int rc = check_variant(lds_slots, lds_probes)) return rc;
  if (value_is_u16)
    return launch_intensity("lsr_label_intensity_variant", labels, static_cast<const uint16_t*>(values), Z, Y, X, n_objects, table,
                            max_blocks, lds_slots, lds_probes, stream);
  return launch_intensity("lsr_label_intensity_variant", labels, static_cast<const float*>(values), Z, Y, X, n_objects, table,
                          max_blocks, lds_slots, lds_probes, stream);
}
