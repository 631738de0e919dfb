// What the whole-volume statistics kernels (stats.hip) and their host twins (host_twins.hip) share: the rule, the record, the
// geometry and the entry checks -- ONE definition each.  tests/stats_ref.py restates the rule in numpy; shrimpy_amd/stats.py
// does the select walk and the interpolation on the host.
//
// Rule.
//   keys      a float32 value is ordered by label.hpp's float_key (so -0.0 sorts below +0.0 and the infinities are ordinary
//             values); a uint16 value is its own 16-bit key.
//   NaN       a NaN is counted (nan_count) and takes part in nothing else: no histogram, no sum, no extreme.
//   digits    a key is kPasses digits of kDigitBits bits, the most significant first.  Pass p of lsr_digit_histogram_* is given
//             k ranks, each with the prefix (the p digits above digit p, as an integer below 2^(kDigitBits p)) it has reached and
//             the table it reads; ranks with one prefix share one table.  For every non-NaN voxel whose key carries the prefix of
//             table t, word t * kBins + (digit p of the key) of `tables` gains 1.  Pass 0 has the empty prefix 0 and one table.
//             The words are 64-bit counters that the entry does NOT zero: calls on several volumes pool into one multiset.
//   moments   pass 0, when given a record, adds to it: count and nan_count 1 each, sum and sum_sq the terms v and v^2 (float64
//             for float32 values, uint64 for uint16 values), and raises the two codes of the extremes.  The record is not zeroed
//             either.  While it is accumulated (and that never ends: another volume may follow) word 4 holds ~key(min) in its low
//             and key(max) in its high 32 bits, both under an atomic maximum for which zero is neutral; a non-NaN float key is
//             never 0 or 0xffffffff, and a record with count == 0 has no extremes.
//   float32   counts, tables and extremes are exact and independent of the order of execution.  v^2 is exact in float64; a sum
//             of n terms in any order and grouping costs at most n - 1 roundings, so each sum is within n 2^-53 sum|terms| of the
//             exact one (the tests allow the intensity kernel's 2 n 2^-53).  Infinities follow IEEE addition.
//   uint16    pure integer arithmetic.  65535^2 n must stay below 2^64.
//   rescale   t = float(v) - sub; o = t / div; with a clip o = max(o, lo) then min(o, hi), each as numpy's clip takes them
//             (o < lo ? lo : o, then o > hi ? hi : o: a value equal to a bound keeps its own sign of zero, a NaN
//             stays).  One float32 rounding per step: the unit is built with -ffp-contract=off.
#pragma once

#include <cstring>

#include "label.hpp"

namespace lsr {
namespace stats {

// The digit width.  8 bits: four passes over a float32 volume and two over a uint16 one, 1 KiB of LDS per table.  (11 bits would
// save the fourth float32 pass at 8 KiB per table; DESIGN.md, "Whole-volume statistics", states what was and was not measured.)
constexpr int kDigitBits = 8;
constexpr int kBins = 1 << kDigitBits;
constexpr int kMaxRanks = 8;                        // K: ranks (and so tables) one pass serves
constexpr int kThreads = 256;                       // one workgroup
constexpr int kLane = 4;                            // voxels one lane loads at once: 16 bytes of float32, 8 of uint16
constexpr int kChunks = 4;                          // such loads a lane has in flight
constexpr int kWaveStep = 64 * kLane * kChunks;     // voxels one wave takes per stride
constexpr int kStep = kThreads / 64 * kWaveStep;    // voxels one workgroup takes per stride of its span
constexpr int kDefaultBlocks = 8192;
constexpr int kMaxBlocks = 1 << 20;
constexpr int kLdsBytes = kMaxRanks * kBins * 4;    // the workgroup's tables of 32-bit counters
// A bin gains at most kStep per stride: the LDS tables are flushed after this many strides, long before 2^32.
constexpr int64_t kFlushStrides = (int64_t(1) << 31) / kStep;
constexpr int kRecordWords = 5;                     // count, nan_count, sum, sum_sq, the two codes

constexpr int passes_of(int key_bits) { return (key_bits + kDigitBits - 1) / kDigitBits; }
constexpr int kPassesF32 = passes_of(32), kPassesU16 = passes_of(16);

constexpr int kFormRuns = 0;                        // runs of equal bins inside a wave reduced before the LDS atomic
constexpr int kFormPlain = 1;                       // one LDS atomic per voxel

template <typename V> struct KeyBits;
template <> struct KeyBits<float> { static constexpr int value = 32; };
template <> struct KeyBits<uint16_t> { static constexpr int value = 16; };

__host__ __device__ inline uint32_t key_of(float v) { return label::float_key(v); }
__host__ __device__ inline uint32_t key_of(uint16_t v) { return v; }
__host__ __device__ inline bool is_nan(float v) { return v != v; }
__host__ __device__ inline bool is_nan(uint16_t) { return false; }

// What a pass compares a key with: the distinct tables of the call and the prefix each one carries.  By value to the kernel.
struct Plan {
  int n_tables;
  int prefix_shift;                                 // key >> prefix_shift is the key's prefix (pass 0: everything matches)
  int digit_shift;
  uint32_t prefix[kMaxRanks];
  int table[kMaxRanks];                             // the table's index in `tables`
};

// The table a key counts in (its index in `tables`) or -1, and the digit.
__host__ __device__ inline int slot_of(const Plan& p, uint32_t key) {
  const uint32_t digit = (key >> p.digit_shift) & (kBins - 1);
  if (p.prefix_shift >= 32) return p.table[0] * kBins + static_cast<int>(digit);
  const uint32_t prefix = key >> p.prefix_shift;
  int t = -1;
#pragma unroll
  for (int i = 0; i < kMaxRanks; ++i)
    if (i < p.n_tables && p.prefix[i] == prefix) t = p.table[i];
  return t < 0 ? -1 : t * kBins + static_cast<int>(digit);
}

// The entry checks of lsr_digit_histogram_*: everything wrong with a call is refused here, before any launch and before
// anything is read or written.  Fills the plan.
inline int check_histogram(const void* in, int value_bytes, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank,
                           int k, const void* tables, const void* moments, int grid_cap, int form, Plan* plan) {
  const int key_bits = value_bytes == 4 ? 32 : 16, passes = passes_of(key_bits);
  LSR_REQUIRE(in != nullptr && prefixes != nullptr && table_of_rank != nullptr && tables != nullptr, LSR_E_ARG,
              "in, prefixes, table_of_rank and tables must not be NULL");
  LSR_REQUIRE(n > 0, LSR_E_ARG, "n %lld must be positive", (long long)n);
  LSR_REQUIRE_COUNT(n);
  LSR_REQUIRE(k >= 1 && k <= kMaxRanks, LSR_E_ARG, "k %d: 1 .. %d ranks", k, kMaxRanks);
  LSR_REQUIRE(pass >= 0 && pass < passes, LSR_E_ARG, "pass %d: 0 .. %d for a %d-bit key", pass, passes - 1, key_bits);
  LSR_REQUIRE(grid_cap >= 0, LSR_E_ARG, "grid_cap %d: 0 (the default) or a positive cap", grid_cap);
  LSR_REQUIRE((form & 0xff) == kFormRuns || (form & 0xff) == kFormPlain, LSR_E_ARG, "form %d: 0 (runs) or 1 (plain) in the low byte", form);
  LSR_REQUIRE(form >= 0, LSR_E_ARG, "form %d must not be negative", form);
  LSR_REQUIRE(reinterpret_cast<uintptr_t>(in) % (kLane * value_bytes) == 0, LSR_E_ARG, "in must be aligned to %d bytes",
              kLane * value_bytes);
  LSR_REQUIRE(reinterpret_cast<uintptr_t>(tables) % 8 == 0 && reinterpret_cast<uintptr_t>(moments) % 8 == 0, LSR_E_ARG,
              "tables and moments must be aligned to 8 bytes");
  LSR_REQUIRE(moments == nullptr || pass == 0, LSR_E_ARG, "the moment record is accumulated in pass 0 only");
  if (value_bytes == 2 && moments != nullptr)
    LSR_REQUIRE(static_cast<uint64_t>(n) <= ~uint64_t(0) / (65535ull * 65535ull), LSR_E_UNSUPPORTED,
                "%lld uint16 voxels: 65535^2 n must stay below 2^64 for the sums to fit", (long long)n);
  plan->n_tables = 0;
  plan->digit_shift = key_bits - kDigitBits * (pass + 1);
  if (plan->digit_shift < 0) plan->digit_shift = 0;
  plan->prefix_shift = pass == 0 ? 32 : plan->digit_shift + kDigitBits;
  const uint64_t prefix_end = uint64_t(1) << (key_bits - (pass == 0 ? key_bits : plan->prefix_shift));
  for (int i = 0; i < kMaxRanks; ++i) plan->prefix[i] = 0u, plan->table[i] = 0;
  for (int r = 0; r < k; ++r) {
    const int t = table_of_rank[r];
    LSR_REQUIRE(t >= 0 && t < k, LSR_E_ARG, "table_of_rank[%d] = %d: 0 .. k - 1", r, t);
    LSR_REQUIRE(prefixes[r] < prefix_end, LSR_E_ARG, "prefixes[%d] = %u: pass %d has prefixes below %llu", r, prefixes[r], pass,
                (unsigned long long)prefix_end);
    int at = -1;
    for (int i = 0; i < plan->n_tables; ++i) {
      const bool same_table = plan->table[i] == t, same_prefix = plan->prefix[i] == prefixes[r];
      LSR_REQUIRE(same_table == same_prefix, LSR_E_ARG, "rank %d: ranks share a table exactly where they share a prefix", r);
      if (same_table) at = i;
    }
    if (at < 0) {
      plan->prefix[plan->n_tables] = prefixes[r];
      plan->table[plan->n_tables] = t;
      plan->n_tables += 1;
    }
  }
  const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + static_cast<uintptr_t>(n) * value_bytes;
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(tables), t1 = t0 + static_cast<uintptr_t>(k) * kBins * 8;
  LSR_REQUIRE(t1 <= i0 || i1 <= t0, LSR_E_ARG, "tables must not overlap in");
  if (moments != nullptr) {
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(moments), m1 = m0 + kRecordWords * 8;
    LSR_REQUIRE((m1 <= i0 || i1 <= m0) && (m1 <= t0 || t1 <= m0), LSR_E_ARG, "moments must not overlap in or tables");
  }
  return LSR_OK;
}

// The twins' walk (host_twins.hip): voxel by voxel.
template <typename V, typename Sum>
inline void histogram_host(const V* in, int64_t n, const Plan& plan, uint64_t* tables, uint64_t* moments) {
  uint64_t count = 0, nans = 0;
  Sum sum = 0, sum_sq = 0;
  uint32_t kmin = 0, kmax = 0;
  for (int64_t i = 0; i < n; ++i) {
    const V v = in[i];
    if (is_nan(v)) {
      nans += 1;
      continue;
    }
    const uint32_t key = key_of(v);
    const int slot = slot_of(plan, key);
    if (slot >= 0) tables[slot] += 1;
    const Sum g = static_cast<Sum>(v);
    count += 1;
    sum += g;
    sum_sq += g * g;
    if (~key > kmin) kmin = ~key;
    if (key > kmax) kmax = key;
  }
  if (moments == nullptr) return;
  moments[0] += count;
  moments[1] += nans;
  Sum s[2];
  memcpy(s, &moments[2], sizeof(s));
  s[0] += sum;
  s[1] += sum_sq;
  memcpy(&moments[2], s, sizeof(s));
  if (count == 0) return;
  const uint32_t old_min = static_cast<uint32_t>(moments[4]), old_max = static_cast<uint32_t>(moments[4] >> 32);
  moments[4] = static_cast<uint64_t>(kmin > old_min ? kmin : old_min) | static_cast<uint64_t>(kmax > old_max ? kmax : old_max) << 32;
}

// lsr_rescale_*'s checks.
inline int check_rescale(const void* in, int value_bytes, int64_t n, int clip, float lo, float hi, const void* out) {
  LSR_REQUIRE(in != nullptr && out != nullptr, LSR_E_ARG, "in and out must not be NULL");
  LSR_REQUIRE(n > 0, LSR_E_ARG, "n %lld must be positive", (long long)n);
  LSR_REQUIRE_COUNT(n);
  LSR_REQUIRE(reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0, LSR_E_ARG,
              "in and out must be aligned to 16 bytes");
  LSR_REQUIRE(clip == 0 || clip == 1, LSR_E_ARG, "clip %d: 0 or 1", clip);
  LSR_REQUIRE(clip == 0 || lo <= hi, LSR_E_ARG, "clip bounds (%g, %g): lo <= hi, neither a NaN", (double)lo, (double)hi);
  const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + static_cast<uintptr_t>(n) * value_bytes;
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + static_cast<uintptr_t>(n) * 4;
  LSR_REQUIRE((value_bytes == 4 && i0 == o0) || o1 <= i0 || i1 <= o0, LSR_E_ARG,
              "out must not overlap in (a float32 volume may be rescaled in place: out == in)");
  return LSR_OK;
}

// One voxel of the rescale, as numpy evaluates np.clip((v.astype(f32) - f32(sub)) / f32(div), lo, hi).
template <typename V>
__host__ __device__ inline float rescale_one(V v, float sub, float div, bool clip, float lo, float hi) {
  const float t = static_cast<float>(v) - sub;
  float o = t / div;
  if (clip) {                                       // (a NaN compares false twice and stays)
    o = o < lo ? lo : o;
    o = o > hi ? hi : o;
  }
  return o;
}

}  // namespace stats
}  // namespace lsr
