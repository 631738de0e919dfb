// The open-addressing table of 64-bit pair keys that the watershed's saddles (watershed.hpp) and the label overlaps
// (overlap.hpp) are collected in, on the device and in the host twins: the hash, the capacity check, the probe bound and the
// insert -- ONE definition each.
//
// A table is `capacity` records of 16 bytes, capacity a power of two in 1 .. 2^30, zeroed by the caller; a record's first
// member is `pair` (0 = empty).  A pair starts probing at pair_slot_of(pair, capacity - 1) and probes linearly over at most
// pair_probes(capacity) slots.  counts[0] = the slots claimed (the insert adds to it); a contribution that finds no slot is
// the caller's to count in counts[1].
#pragma once

#include <algorithm>
#include <cstdint>

#include "common.hpp"

namespace lsr {

constexpr int64_t kMaxPairCapacity = int64_t(1) << 30;      // slots of a pair table: a power of two, 1 .. 2^30
constexpr int kMaxPairProbes = 256;                         // a pair gives up after min(capacity, kMaxPairProbes) slots

inline int pair_probes(int64_t capacity) { return static_cast<int>(std::min<int64_t>(capacity, kMaxPairProbes)); }

inline int check_pair_capacity(int64_t capacity) {
  LSR_REQUIRE(capacity > 0 && capacity <= kMaxPairCapacity && (capacity & (capacity - 1)) == 0, LSR_E_ARG,
              "capacity %lld: a power of two, 1 .. 2^30", (long long)capacity);
  return LSR_OK;
}

// Where a pair starts probing: the finaliser of splitmix64, masked to the table.
__host__ __device__ inline uint32_t pair_slot_of(unsigned long long pair, uint32_t mask) {
  pair ^= pair >> 30;
  pair *= 0xbf58476d1ce4e5b9ull;
  pair ^= pair >> 27;
  pair *= 0x94d049bb133111ebull;
  pair ^= pair >> 31;
  return static_cast<uint32_t>(pair) & mask;
}

// One contribution on the device: claim the pair's slot by a compare-and-swap on an empty one, or find it, within `probes`
// slots, and fold(record) the contribution in (an atomic on the record's second member).  The table's words are touched by
// atomics only, and the loop is bounded: nobody's progress is waited for.  false: no slot.  (watershed.hip's saddle kernel
// spells the same loop out: through this template hipcc more than doubles that kernel's registers.)
template <class Record, class Fold>
__device__ __forceinline__ bool pair_insert(Record* table, unsigned mask, int probes, unsigned long long pair, int* counts,
                                            Fold fold) {
  static_assert(sizeof(Record) == 16, "a pair table's record is 16 bytes");
  unsigned slot = pair_slot_of(pair, mask);
  for (int p = 0; p < probes; ++p, slot = (slot + 1) & mask) {
    const unsigned long long old = atomicCAS(&table[slot].pair, 0ull, pair);
    if (old == 0ull) atomicAdd(&counts[0], 1);
    if (old == 0ull || old == pair) {
      fold(table[slot]);
      return true;
    }
  }
  return false;
}

// ... and in a host twin: the same probe sequence, sequential.
template <class Record, class Fold>
inline bool pair_insert_host(Record* table, uint32_t mask, int probes, unsigned long long pair, int32_t* counts, Fold fold) {
  static_assert(sizeof(Record) == 16, "a pair table's record is 16 bytes");
  uint32_t slot = pair_slot_of(pair, mask);
  for (int p = 0; p < probes; ++p, slot = (slot + 1) & mask) {
    if (table[slot].pair == 0) {
      table[slot].pair = pair;
      counts[0] += 1;
    }
    if (table[slot].pair == pair) {
      fold(table[slot]);
      return true;
    }
  }
  return false;
}

}  // namespace lsr
