// Where a 64-bit pair key starts probing in an open-addressing table of a power-of-two size: ONE definition, shared by the
// watershed's saddle table (watershed.hpp) and the label-overlap table (overlap.hpp), on the device and in the host twins.
#pragma once

#include <cstdint>

#include "common.hpp"

namespace lsr {

constexpr int64_t kMaxPairCapacity = int64_t(1) << 30;      // slots of a pair table: a power of two, 1 .. 2^30

// The finaliser of splitmix64, masked to the table.
__host__ __device__ inline uint32_t pair_slot_of(unsigned long long pair, uint32_t mask) {
  pair ^= pair >> 30;
  pair *= 0xbf58476d1ce4e5b9ull;
  pair ^= pair >> 27;
  pair *= 0x94d049bb133111ebull;
  pair ^= pair >> 31;
  return static_cast<uint32_t>(pair) & mask;
}

}  // namespace lsr
