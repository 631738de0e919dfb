// What the colocalization kernel (coloc.hip) and its host twins (host_twins.hip) share: the rule, the two records, the geometry
// and the entry checks -- ONE definition each.  PARITY UNPINNED (skimage's colocalization measures are absent): the rule below
// IS the specification, tests/coloc_ref.py restates it in numpy.
//
// Rule.  labels: an int32 (Z, Y, X) volume or NULL; a, b: two volumes of that shape and of one type, float32 or uint16; ta, tb:
//   two float32 thresholds; n objects.  With labels == NULL, n must be 1 and every voxel belongs to object 1.
//   Let A = (float(a) > ta) and B = (float(b) > tb): a uint16 converts to float32 exactly, a NaN value compares false.
//   For every voxel with 1 <= label <= n, record label - 1 gains
//       word 0        count                                       1
//       words 1..5    sum_a, sum_b, sum_aa, sum_bb, sum_ab         a, b, a^2, b^2, a b
//       word 6        count_both                                  1 where A and B
//       words 7..11   both_a, both_b, both_aa, both_bb, both_ab    the same five terms where A and B
//       words 12, 13  count_A, count_B                            1 where A; 1 where B
//       words 14, 15  a_where_B, b_where_A                        a where B; b where A
//   A record is 16 words of 8 bytes (128 bytes).  Counts are int64; sums are float64 for float32 values and uint64 for uint16
//   values.  The caller zeroes the table.  Labels outside 1 .. n are ignored; a label that no voxel carries keeps its zeros.
//
// uint16 values.  Pure integer arithmetic: device, twin and restatement are equal byte for byte.  65535^2 * 2^31 < 2^63, so no
//   sum can wrap within the 2^31 - 1 voxels the label kernels accept (the other label kernels' limit, label::check_volume).
//
// float32 values.  Counts are exact.  a b, a^2 and b^2 are exact in float64 (48 bits), so every sum is an accumulation of exact
//   terms in an order that is not fixed: it lies within m 2^-53 sum|terms| of the exact sum, m the number of terms of that sum
//   (count, count_both, count_B for a_where_B, count_A for b_where_A).  Where a mask is false the term is not added at all (a
//   select, never a product with 0), and adding to a zero accumulator is exact, so m - 1 additions round.  A non-finite voxel
//   follows IEEE arithmetic into its own object's sums and touches no other object's.
#pragma once

#include <cmath>

#include "label.hpp"

namespace lsr {
namespace coloc {

// One record of the table (part of the ABI: shrimpy_amd/colocalize.py reads both as structured arrays).
struct RecordF32 {
  int64_t count;
  double sum_a, sum_b, sum_aa, sum_bb, sum_ab;
  int64_t count_both;
  double both_a, both_b, both_aa, both_bb, both_ab;
  int64_t count_A, count_B;
  double a_where_B, b_where_A;
};
struct RecordU16 {
  int64_t count;
  uint64_t sum_a, sum_b, sum_aa, sum_bb, sum_ab;
  int64_t count_both;
  uint64_t both_a, both_b, both_aa, both_bb, both_ab;
  int64_t count_A, count_B;
  uint64_t a_where_B, b_where_A;
};
constexpr int kWords = 16;                          // a record in 64-bit words
constexpr int kCounts = 4;                          // count, count_both, count_A, count_B
constexpr int kSums = 12;                           // the other words, in the record's order
static_assert(sizeof(RecordF32) == 8 * kWords && sizeof(RecordU16) == 8 * kWords, "the records' size is part of the ABI");
// the word of the j-th count (0, 6, 12, 13) and of the i-th sum (1..5, 7..11, 14, 15)
__host__ __device__ constexpr int count_word(int j) { return j == 0 ? 0 : j == 1 ? 6 : 10 + j; }
__host__ __device__ constexpr int sum_word(int i) { return i < 5 ? 1 + i : i < 10 ? 2 + i : 4 + i; }

constexpr int kThreads = 256;                       // one workgroup
constexpr int kChunks = 4;                          // wave steps of 64 voxels a wave has in flight
constexpr int kStep = kThreads * kChunks;           // voxels one workgroup takes per stride of its span
// The per-workgroup table: per slot sixteen 64-bit words and the int32 key = 132 bytes, field-major; a label's first slot is
// label & (slots - 1), as in intensity.hpp.  256 slots are 33 KiB; 512 would pass the 64 KiB a launch gets without opting in,
// so the measurement entry stops at 256.  Slots and cap are chosen from the sweep in profiles/coloc_config2.jsonl (64 .. 256 slots,
// caps 4096 .. 262144, config-2 shape, float32; it started from the intensity kernel's 65 536 workgroups, which that run marks as
// the default).  On the all-foreground volume the table size does not matter and the cap does: 2.1 ms at 4096 and at 16 384
// workgroups, 5.4 ms at 65 536 and 19.4 ms at 262 144, where the sixteen same-record global atomics of each workgroup's flush
// queue up; the bead scene follows it (1.97 / 2.40 / 3.84 ms at 256 slots) and so does the kernel without labels (1.22 / 2.18 /
// 6.6 ms).  Labelled noise, bound by the global atomics of its 46 million records, goes the other way: 256 slots take 110.5 ms
// at 16 384 workgroups and 96.5 ms at 65 536 (64 slots: 117.5 / 113.6).  So 256 slots at 16 384 workgroups: 14 % slower on the
// noise, 18 % and 62 % faster on the other two.  The probe bound matters only on the noise (101.2 ms at 1, 96.4 at 32).
constexpr int kLdsSlots = 256;
constexpr int kMaxLdsSlots = 256;                   // (what the measurement entry accepts)
constexpr int kLdsProbes = 8;                       // a head gives up on LDS after this many slots and goes to global memory
constexpr int kDefaultBlocks = 16384;
constexpr int kMaxBlocks = 1 << 20;
static_assert((kLdsSlots & (kLdsSlots - 1)) == 0 && (kMaxLdsSlots & (kMaxLdsSlots - 1)) == 0, "the LDS table is masked");

// The entry checks (the shape of intensity::check_intensity): everything wrong with a call is refused here, before any launch
// and before anything is read or written.
inline int check_coloc(const void* labels, const void* a, const void* b, int value_bytes, int64_t Z, int64_t Y, int64_t X,
                       int64_t n_objects, float ta, float tb, const void* table, int max_blocks) {
  LSR_REQUIRE(a != nullptr && b != nullptr && table != nullptr, LSR_E_ARG, "a, b and table must not be NULL");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_ARG, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE(n_objects >= 0 && n_objects <= label::kMaxVoxels, LSR_E_ARG, "%lld objects: 0 .. 2^31 - 1", (long long)n_objects);
  LSR_REQUIRE(labels != nullptr || n_objects == 1, LSR_E_ARG, "without labels the whole volume is object 1: n_objects %lld must be 1",
              (long long)n_objects);
  LSR_REQUIRE(!std::isnan(ta) && !std::isnan(tb), LSR_E_ARG, "a threshold is NaN");
  LSR_REQUIRE(max_blocks >= 0, LSR_E_ARG, "max_blocks %d: 0 (the default) or a positive cap", max_blocks);
  if (int rc = label::check_volume(Z, Y, X)) return rc;              // (LSR_E_UNSUPPORTED above 2^31 - 1 voxels)
  const uintptr_t voxels = static_cast<uintptr_t>(Z * Y * X);
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(table), t1 = t0 + static_cast<uintptr_t>(n_objects) * sizeof(RecordF32);
  const uintptr_t l0 = reinterpret_cast<uintptr_t>(labels), l1 = l0 + voxels * sizeof(int32_t);
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + voxels * static_cast<uintptr_t>(value_bytes);
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + voxels * static_cast<uintptr_t>(value_bytes);
  LSR_REQUIRE(labels == nullptr || t1 <= l0 || l1 <= t0, LSR_E_ARG, "table must not overlap labels");
  LSR_REQUIRE(t1 <= a0 || a1 <= t0, LSR_E_ARG, "table must not overlap a");
  LSR_REQUIRE(t1 <= b0 || b1 <= t0, LSR_E_ARG, "table must not overlap b");
  return LSR_OK;
}

// The twins' walk (host_twins.hip), voxel by voxel in raster order.
template <typename V, typename Record, typename Sum>
inline void accumulate_host(const int32_t* labels, const V* a, const V* b, int64_t voxels, int64_t n_objects, float ta, float tb,
                            Record* rows) {
  for (int64_t i = 0; i < voxels; ++i) {
    const int32_t l = labels != nullptr ? labels[i] : 1;
    if (l < 1 || l > n_objects) continue;
    Record& r = rows[l - 1];
    const Sum fa = static_cast<Sum>(a[i]), fb = static_cast<Sum>(b[i]);
    const bool A = static_cast<float>(a[i]) > ta, B = static_cast<float>(b[i]) > tb;
    r.count += 1;
    r.sum_a += fa;
    r.sum_b += fb;
    r.sum_aa += fa * fa;
    r.sum_bb += fb * fb;
    r.sum_ab += fa * fb;
    if (A && B) {
      r.count_both += 1;
      r.both_a += fa;
      r.both_b += fb;
      r.both_aa += fa * fa;
      r.both_bb += fb * fb;
      r.both_ab += fa * fb;
    }
    if (A) {
      r.count_A += 1;
      r.b_where_A += fb;
    }
    if (B) {
      r.count_B += 1;
      r.a_where_B += fa;
    }
  }
}

}  // namespace coloc
}  // namespace lsr
