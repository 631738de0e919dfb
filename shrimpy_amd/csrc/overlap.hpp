// What the label-overlap kernel (overlap.hip) and its host twin (host_twins.hip) share: the rule, the record, the geometry and
// the entry checks -- ONE definition each.  No upstream is pinned: the rule below IS the specification
// (tests/track_ref.py restates it with np.unique), and device, twin and restatement agree as sets of records, exactly.
//
// Rule.  a, b: int32 (Z, Y, X) label volumes of two timepoints, shift = (sz, sy, sx) integers.
//   For every voxel v = (z, y, x), let u = v + shift.  If u lies inside the volume, a[v] > 0 and b[u] > 0, the pair
//   (a[v], b[u]) gains 1.  Labels <= 0 are background; a u outside the volume contributes nothing.
//   The table is `capacity` records of 16 bytes, capacity a power of two in 1 .. 2^30, zeroed by the caller:
//   pair = (uint32)a << 32 | (uint32)b (0 = empty: both labels are positive, so no pair is 0) and its 64-bit count.
//   A pair starts probing at pair_slot_of(pair, capacity - 1) and probes linearly over at most pair_probes(capacity)
//   slots (pair_table.hpp); a contribution that finds no slot adds its weight to counts[1] (the table then holds partial
//   counts: come back with a larger one).  counts[0] = the slots claimed.  Both are set by the entry.
//   Pure integer arithmetic: the set of records does not depend on the order of execution (which slot holds which record
//   does).
#pragma once

#include "label.hpp"
#include "pair_table.hpp"

namespace lsr {
namespace overlap {

// One record of the table (part of the ABI: shrimpy_amd/track.py reads it as a structured array).
struct Overlap {
  unsigned long long pair;      // (uint32)a << 32 | (uint32)b, 0 = empty
  unsigned long long count;     // voxels that are a at t and b at t + 1
};
static_assert(sizeof(Overlap) == 16, "the overlap record's size is part of the ABI");

constexpr int kThreads = 256;                       // one workgroup
constexpr int kChunks = 4;                          // wave steps of 64 voxels a wave has in flight
constexpr int kStep = kThreads * kChunks;           // voxels one workgroup takes per stride of its span
constexpr int kLdsSlots = 2048;                     // the per-workgroup table: 16 KiB of keys + 8 KiB of counts
constexpr int kLdsProbes = 16;                      // a head gives up on LDS after this many slots and goes to global memory
// The grid's cap, chosen from profiles/overlap_config2.jsonl: on the config-2 shape it gives spans of 12 288 voxels, short enough
// that the distinct pairs of a span of labelled NOISE (about 800) still fit the LDS table -- a span whose pairs do not fit pays
// kLdsProbes failed probes per head and then a scattered global atomic -- while beads and an all-foreground volume take what
// they take at 16 384.
constexpr int kDefaultBlocks = 65536;
constexpr int kMaxBlocks = 1 << 20;
static_assert((kLdsSlots & (kLdsSlots - 1)) == 0, "the LDS table is masked");

__host__ __device__ inline unsigned long long pack(int32_t a, int32_t b) {
  return static_cast<unsigned long long>(static_cast<uint32_t>(a)) << 32 | static_cast<uint32_t>(b);
}

// Does the shift leave no voxel with a partner inside the volume?
inline bool shift_empties(int64_t Z, int64_t Y, int64_t X, const int32_t s[3]) {
  auto beyond = [](int64_t d, int64_t n) { return d >= n || -d >= n; };
  return beyond(s[0], Z) || beyond(s[1], Y) || beyond(s[2], X);
}

// The entry checks: everything that is wrong with a call is LSR_E_ARG here, before any launch and before anything is written.
inline int check_overlap(const void* a, const void* b, int64_t Z, int64_t Y, int64_t X, const void* shift_zyx, int64_t capacity,
                         const void* table, const void* counts, int max_blocks) {
  LSR_REQUIRE(a != nullptr && b != nullptr && shift_zyx != nullptr && table != nullptr && counts != nullptr, LSR_E_ARG,
              "a, b, shift_zyx, table and counts must not be NULL");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_ARG, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  if (label::check_volume(Z, Y, X) != LSR_OK) return LSR_E_ARG;        // (its message stands: at most 2^31 - 1 voxels)
  if (int rc = check_pair_capacity(capacity)) return rc;
  LSR_REQUIRE(max_blocks >= 0, LSR_E_ARG, "max_blocks %d: 0 (the default) or a positive cap", max_blocks);
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(table), t1 = t0 + static_cast<uintptr_t>(capacity) * sizeof(Overlap);
  const uintptr_t bytes = static_cast<uintptr_t>(Z * Y * X) * sizeof(int32_t);
  auto apart = [&](const void* p) {
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(p);
    return t1 <= p0 || p0 + bytes <= t0;
  };
  LSR_REQUIRE(apart(a) && apart(b), LSR_E_ARG, "table must not alias a or b");
  return LSR_OK;
}

}  // namespace overlap
}  // namespace lsr
