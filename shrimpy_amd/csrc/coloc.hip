// Per-object sums over two channels at once (shrimpy_amd/colocalize.py: pair_table; the `colocalize` command): everything that
// Pearson, Manders, the overlap coefficients and Costes' threshold search need, from one read of the labels and the two value
// volumes.  The rule, the two records and the entry checks are coloc.hpp's; tests/coloc_ref.py restates the rule in numpy.
//
// The form is intensity.hip's (read its header): a contiguous span per workgroup walked in strides of kStep, the 3 * kChunks
// loads of a stride issued before the first is used, run heads from one __ballot, a per-workgroup open-addressing table in LDS
// (atomicCAS on the key, 64-bit LDS atomic adds -- ds_add_f64 through unsafeAtomicAdd, never a compare-and-swap loop), one flush
// by global 64-bit atomic adds, a head without a slot straight to the global record.  What differs:
//
//   one label    a record has 16 words, and a shuffle reduction restricted to the run for each of them would cost three times
//                the ds_bpermute_b32 the intensity kernel is already bound by.  So while consecutive wave steps hold one and the
//                same label in all 64 lanes, every lane keeps the 16 quantities in registers; they are reduced over the wave and
//                placed once, when another label fills a wave step or the span ends.  That is the whole all-foreground volume
//                and the interior of every object wider than a wave step.
//   mixed steps  a wave step that holds more than one run (or a lane without a label) takes the run-restricted path.  Nothing
//                here depends on a voxel's position, so a run does not end with its row.  The four counts are population counts
//                of ballots under the run's lane mask; the twelve sums take the shuffle reduction.
//   masks        the terms "where A", "where B", "where A and B" are selects (a false mask adds a zero of the sum's type, never
//                a product with 0: a NaN or an infinity stays out of the sums it does not belong to); no branch depends on them.
//   no labels    labels == NULL is a kernel of its own without a label stream, without ballots and without the table: per-lane
//                registers, one reduction per wave, sixteen LDS words per workgroup, sixteen global adds per workgroup.
//
// The two hard rules of label.hip hold: words shared inside a launch (the LDS table between the barriers, the global table)
// are touched by atomics only, and no workgroup ever waits for another; every loop is bounded.

#include <algorithm>
#include <type_traits>

#include "coloc.hpp"

namespace {

namespace co = lsr::coloc;

// float32 values are summed in float64, uint16 values in uint64
template <typename V>
using SumOf = typename std::conditional<std::is_same<V, float>::value, double, unsigned long long>::type;

__device__ __forceinline__ void add64(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
__device__ __forceinline__ void add64(unsigned long long* p, double v) { unsafeAtomicAdd(reinterpret_cast<double*>(p), v); }
__device__ __forceinline__ bool is_zero(unsigned long long v) { return v == 0ull; }
__device__ __forceinline__ bool is_zero(double v) { return __double_as_longlong(v) == 0ll; }      // (+0.0 only: adding it is a no-op)

// What a voxel, a run or a wave's registers hold: the four counts and the twelve sums in the record's order.
template <typename S>
struct Part {
  unsigned c[co::kCounts];                  // (a lane's share of a span stays far below 2^32)
  S s[co::kSums];
};

template <typename S>
__device__ __forceinline__ void clear(Part<S>& p) {
#pragma unroll
  for (int j = 0; j < co::kCounts; ++j) p.c[j] = 0u;
#pragma unroll
  for (int i = 0; i < co::kSums; ++i) p.s[i] = S(0);
}

// The twelve terms of one voxel; a false mask gives the zero of S.
template <typename V, typename S>
__device__ __forceinline__ void terms_of(V a, V b, bool A, bool B, S t[co::kSums]) {
  const S fa = static_cast<S>(a), fb = static_cast<S>(b);
  const S aa = fa * fa, bb = fb * fb, ab = fa * fb;
  const bool both = A && B;
  t[0] = fa, t[1] = fb, t[2] = aa, t[3] = bb, t[4] = ab;
  t[5] = both ? fa : S(0), t[6] = both ? fb : S(0), t[7] = both ? aa : S(0), t[8] = both ? bb : S(0), t[9] = both ? ab : S(0);
  t[10] = B ? fa : S(0);
  t[11] = A ? fb : S(0);
}

// One voxel into a lane's registers, where `in` (the voxel belongs to the object).
template <typename V, typename S>
__device__ __forceinline__ void gain(Part<S>& p, bool in, V a, V b, float ta, float tb) {
  const bool A = in && static_cast<float>(a) > ta, B = in && static_cast<float>(b) > tb;
  S t[co::kSums];
  terms_of<V, S>(a, b, A, B, t);
  p.c[0] += in ? 1u : 0u;
  p.c[1] += (A && B) ? 1u : 0u;
  p.c[2] += A ? 1u : 0u;
  p.c[3] += B ? 1u : 0u;
#pragma unroll
  for (int i = 0; i < 5; ++i) p.s[i] += in ? t[i] : S(0);
#pragma unroll
  for (int i = 5; i < co::kSums; ++i) p.s[i] += t[i];       // (A and B already imply `in`)
}

// The sum over the wave, in every lane.
template <typename S>
__device__ __forceinline__ void wave_sum(Part<S>& p) {
#pragma unroll
  for (int d = 1; d < lsr::kWave; d <<= 1) {
#pragma unroll
    for (int j = 0; j < co::kCounts; ++j) p.c[j] += __shfl_xor(p.c[j], d);
#pragma unroll
    for (int i = 0; i < co::kSums; ++i) p.s[i] += __shfl_xor(p.s[i], d);
  }
}

// One part into sixteen words that are either a global record or, field-major, a slot of the LDS table (stride = slots).
template <typename S>
__device__ __forceinline__ void add_words(unsigned long long* words, int stride, const Part<S>& p) {
#pragma unroll
  for (int j = 0; j < co::kCounts; ++j)
    if (p.c[j] != 0u) atomicAdd(&words[co::count_word(j) * stride], static_cast<unsigned long long>(p.c[j]));
#pragma unroll
  for (int i = 0; i < co::kSums; ++i)
    if (!is_zero(p.s[i])) add64(&words[co::sum_word(i) * stride], p.s[i]);
}

// One lane places a part that belongs to label l: into the LDS table where a slot is found within `probes`, else into the
// global record.
template <typename S, bool kLds>
__device__ __forceinline__ void place(int l, const Part<S>& p, unsigned long long* sums, int* keys, int slots, int probes,
                                      unsigned long long* table) {
  if (kLds) {
    const int slot_mask = slots - 1;
    int slot = l & slot_mask;
    for (int k = 0; k < probes; ++k, slot = (slot + 1) & slot_mask) {
      const int old = atomicCAS(&keys[slot], 0, l);
      if (old == 0 || old == l) {
        add_words(sums + slot, slots, p);
        return;
      }
    }
  }
  add_words(table + static_cast<int64_t>(l - 1) * co::kWords, 1, p);
}

// kLds = false is the plain form (every part straight to the global record), kept for the measurement entry.
template <typename V, bool kLds>
__global__ __launch_bounds__(co::kThreads) void label_coloc_kernel(const int* __restrict__ labels, const V* __restrict__ va,
                                                                   const V* __restrict__ vb, int n_objects, float ta, float tb,
                                                                   int64_t n, int64_t span, int slots, int probes,
                                                                   unsigned long long* table) {
  using S = SumOf<V>;
  extern __shared__ unsigned long long lds[];       // kWords * slots words (field-major), slots keys
  unsigned long long* sums = lds;
  int* keys = reinterpret_cast<int*>(lds + co::kWords * slots);
  if (kLds) {
    for (int i = threadIdx.x; i < co::kWords * slots; i += co::kThreads) sums[i] = 0ull;
    for (int i = threadIdx.x; i < slots; i += co::kThreads) keys[i] = 0;
    __syncthreads();
  }

  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * span, last = first + span < n ? first + span : n;

  Part<S> own;                // what this lane holds of the label `held` (wave-uniform; 0: nothing)
  clear(own);
  int held = 0;

  // (the loop's bounds are the workgroup's: every wave makes the same number of trips, every lane of a wave reaches the ballots
  // and the shuffles)
  for (int64_t base = first; base < last; base += co::kStep) {
    int lab[co::kChunks];
    V a[co::kChunks], b[co::kChunks];
#pragma unroll
    for (int c = 0; c < co::kChunks; ++c) {
      const int64_t v = base + (wave * co::kChunks + c) * lsr::kWave + lane;
      lab[c] = v < last ? labels[v] : 0;              // (a span ends where the next workgroup's begins: v < last <= n)
    }
#pragma unroll
    for (int c = 0; c < co::kChunks; ++c) {
      const int64_t v = base + (wave * co::kChunks + c) * lsr::kWave + lane;
      a[c] = v < last ? va[v] : V(0);
    }
#pragma unroll
    for (int c = 0; c < co::kChunks; ++c) {
      const int64_t v = base + (wave * co::kChunks + c) * lsr::kWave + lane;
      b[c] = v < last ? vb[v] : V(0);
    }
#pragma unroll
    for (int c = 0; c < co::kChunks; ++c) {
      const int l = (lab[c] >= 1 && lab[c] <= n_objects) ? lab[c] : 0;
      const int l0 = __shfl(l, 0);
      if (__ballot(l != l0) == 0ull) {                  // (wave-uniform) one label, or none, in all 64 lanes
        if (l0 == 0) continue;
        if (l0 != held) {
          if (held != 0) {
            wave_sum(own);
            if (lane == 0) place<S, kLds>(held, own, sums, keys, slots, probes, table);
            clear(own);
          }
          held = l0;
        }
        gain<V, S>(own, true, a[c], b[c], ta, tb);
        continue;
      }
      // more than one run: heads where the label changes (a run may cross a row end: no term depends on the position)
      const int before = __shfl_up(l, 1);
      const unsigned long long heads = __ballot(lane == 0 || l != before);
      // the run this lane lies in ends in front of the next head above the lane (or with the wave)
      const unsigned long long above = heads & ~((2ull << lane) - 1ull);       // (lane 63: 2 << 63 == 0, nothing above)
      const int end = above != 0ull ? __ffsll(static_cast<long long>(above)) - 2 : lsr::kWave - 1;      // the run's last lane
      // lanes lane .. end
      const unsigned long long run = (end == lsr::kWave - 1 ? ~0ull : (2ull << end) - 1ull) & ~((1ull << lane) - 1ull);
      const bool A = static_cast<float>(a[c]) > ta, B = static_cast<float>(b[c]) > tb;
      const unsigned long long in_a = __ballot(A), in_b = __ballot(B);
      Part<S> r;
      r.c[0] = static_cast<unsigned>(end - lane + 1);
      r.c[1] = static_cast<unsigned>(__popcll(in_a & in_b & run));
      r.c[2] = static_cast<unsigned>(__popcll(in_a & run));
      r.c[3] = static_cast<unsigned>(__popcll(in_b & run));
      terms_of<V, S>(a[c], b[c], A, B, r.s);
      // the segmented reduction: after the step d a lane holds the sums of lanes lane .. min(lane + 2d - 1, end)
#pragma unroll
      for (int d = 1; d < lsr::kWave; d <<= 1) {
        const bool take = lane + d <= end;
#pragma unroll
        for (int i = 0; i < co::kSums; ++i) {
          const S o = __shfl_down(r.s[i], d);
          r.s[i] += take ? o : S(0);
        }
      }
      if (l != 0 && ((heads >> lane) & 1ull)) place<S, kLds>(l, r, sums, keys, slots, probes, table);
    }
  }
  if (held != 0) {
    wave_sum(own);
    if (lane == 0) place<S, kLds>(held, own, sums, keys, slots, probes, table);
  }
  if (!kLds) return;
  __syncthreads();

  const int slot_mask = slots - 1;
  for (int i = threadIdx.x; i < co::kWords * slots; i += co::kThreads) {
    const int slot = i & slot_mask, k = i / slots;
    const int l = keys[slot];
    if (l == 0) continue;
    unsigned long long* rec = table + static_cast<int64_t>(l - 1) * co::kWords;
    const bool counted = k == 0 || k == 6 || k == 12 || k == 13;
    if (counted || std::is_same<S, unsigned long long>::value) {
      if (sums[i] != 0ull) atomicAdd(&rec[k], sums[i]);
    } else {
      S sum;
      memcpy(&sum, &sums[i], sizeof(sum));
      if (!is_zero(sum)) add64(&rec[k], sum);
    }
  }
}

// labels == NULL: every voxel belongs to object 1.
template <typename V>
__global__ __launch_bounds__(co::kThreads) void whole_coloc_kernel(const V* __restrict__ va, const V* __restrict__ vb, float ta,
                                                                   float tb, int64_t n, int64_t span, unsigned long long* table) {
  using S = SumOf<V>;
  __shared__ unsigned long long words[co::kWords];
  if (threadIdx.x < co::kWords) words[threadIdx.x] = 0ull;
  __syncthreads();

  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * span, last = first + span < n ? first + span : n;
  Part<S> own;
  clear(own);
  for (int64_t base = first; base < last; base += co::kStep) {
    V a[co::kChunks], b[co::kChunks];
#pragma unroll
    for (int c = 0; c < co::kChunks; ++c) {
      const int64_t v = base + (wave * co::kChunks + c) * lsr::kWave + lane;
      a[c] = v < last ? va[v] : V(0);
    }
#pragma unroll
    for (int c = 0; c < co::kChunks; ++c) {
      const int64_t v = base + (wave * co::kChunks + c) * lsr::kWave + lane;
      b[c] = v < last ? vb[v] : V(0);
    }
#pragma unroll
    for (int c = 0; c < co::kChunks; ++c) {
      const int64_t v = base + (wave * co::kChunks + c) * lsr::kWave + lane;
      gain<V, S>(own, v < last, a[c], b[c], ta, tb);
    }
  }
  wave_sum(own);
  if (lane == 0) add_words(words, 1, own);
  __syncthreads();
  if (threadIdx.x >= co::kWords) return;
  const int k = threadIdx.x;
  const bool counted = k == 0 || k == 6 || k == 12 || k == 13;
  if (counted || std::is_same<S, unsigned long long>::value) {
    if (words[k] != 0ull) atomicAdd(&table[k], words[k]);
  } else {
    S sum;
    memcpy(&sum, &words[k], sizeof(sum));
    if (!is_zero(sum)) add64(&table[k], sum);
  }
}

template <typename V>
int launch_coloc(const char* what, const int32_t* labels, const V* a, const V* b, int64_t Z, int64_t Y, int64_t X,
                 int64_t n_objects, float ta, float tb, void* table, int max_blocks, int slots, int probes, lsr_stream_t stream) {
  if (int rc = co::check_coloc(labels, a, b, sizeof(V), Z, Y, X, n_objects, ta, tb, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  const int64_t n = Z * Y * X;
  const int64_t cap = std::min<int64_t>(max_blocks > 0 ? max_blocks : co::kDefaultBlocks, co::kMaxBlocks);
  const int64_t steps = lsr::ceil_div(n, co::kStep);
  const int64_t span = lsr::ceil_div(steps, std::min(steps, cap)) * co::kStep;       // voxels per workgroup, whole strides
  const int64_t blocks = lsr::ceil_div(n, span);
  unsigned long long* t = static_cast<unsigned long long*>(table);
  hipStream_t q = lsr::as_stream(stream);
  if (labels == nullptr) {
    hipLaunchKernelGGL(whole_coloc_kernel<V>, dim3(static_cast<unsigned>(blocks)), dim3(co::kThreads), 0, q, a, b, ta, tb, n, span, t);
  } else if (slots > 0) {
    const size_t lds = static_cast<size_t>(slots) * (co::kWords * sizeof(unsigned long long) + sizeof(int));
    hipLaunchKernelGGL((label_coloc_kernel<V, true>), dim3(static_cast<unsigned>(blocks)), dim3(co::kThreads), lds, q, labels, a, b,
                       static_cast<int>(n_objects), ta, tb, n, span, slots, probes, t);
  } else {
    hipLaunchKernelGGL((label_coloc_kernel<V, false>), dim3(static_cast<unsigned>(blocks)), dim3(co::kThreads), 0, q, labels, a, b,
                       static_cast<int>(n_objects), ta, tb, n, span, 1, 0, t);
  }
  return lsr::launch_status(what);
}

int check_variant(int lds_slots, int lds_probes) {
  LSR_REQUIRE(lds_slots >= 0 && lds_slots <= co::kMaxLdsSlots && (lds_slots & (lds_slots - 1)) == 0, LSR_E_ARG,
              "lds_slots %d: 0 (no LDS table) or a power of two up to %d", lds_slots, co::kMaxLdsSlots);
  LSR_REQUIRE(lds_probes >= 1 && lds_probes <= co::kMaxLdsSlots, LSR_E_ARG, "lds_probes %d: 1 .. %d", lds_probes,
              co::kMaxLdsSlots);
  return LSR_OK;
}

}  // namespace

extern "C" int lsr_label_coloc_geometry(int out[2]) {
  LSR_REQUIRE_PTR(out);
  out[0] = co::kLdsSlots;
  out[1] = co::kDefaultBlocks;
  return LSR_OK;
}

extern "C" int lsr_label_coloc_f32(const int32_t* labels, const float* a, const float* b, int64_t Z, int64_t Y, int64_t X,
                                   int64_t n_objects, float ta, float tb, void* table, int max_blocks, lsr_stream_t stream) {
  return launch_coloc("lsr_label_coloc_f32", labels, a, b, Z, Y, X, n_objects, ta, tb, table, max_blocks, co::kLdsSlots,
                      co::kLdsProbes, stream);
}

extern "C" int lsr_label_coloc_u16(const int32_t* labels, const uint16_t* a, const uint16_t* b, int64_t Z, int64_t Y, int64_t X,
                                   int64_t n_objects, float ta, float tb, void* table, int max_blocks, lsr_stream_t stream) {
  return launch_coloc("lsr_label_coloc_u16", labels, a, b, Z, Y, X, n_objects, ta, tb, table, max_blocks, co::kLdsSlots,
                      co::kLdsProbes, stream);
}

extern "C" int lsr_label_coloc_variant(const int32_t* labels, const void* a, const void* b, int value_is_u16, int64_t Z, int64_t Y,
                                       int64_t X, int64_t n_objects, float ta, float tb, void* table, int max_blocks, int lds_slots,
                                       int lds_probes, lsr_stream_t stream) {
  if (int rc = check_variant(lds_slots, lds_probes)) return rc;
  if (value_is_u16)
    return launch_coloc("lsr_label_coloc_variant", labels, static_cast<const uint16_t*>(a), static_cast<const uint16_t*>(b), Z, Y,
                        X, n_objects, ta, tb, table, max_blocks, lds_slots, lds_probes, stream);
  return launch_coloc("lsr_label_coloc_variant", labels, static_cast<const float*>(a), static_cast<const float*>(b), Z, Y, X,
                      n_objects, ta, tb, table, max_blocks, lds_slots, lds_probes, stream);
}
