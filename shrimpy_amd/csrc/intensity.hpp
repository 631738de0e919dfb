// What the label-intensity kernel (intensity.hip) and its host twins (host_twins.hip) share: the rule, the two records, the
// geometry and the entry checks -- ONE definition each.  PARITY UNPINNED (skimage's regionprops is absent): the rule below IS
// the specification, tests/intensity_ref.py restates it in numpy.
//
// Rule.  labels: an int32 (Z, Y, X) volume, v: a float32 or uint16 volume of the same shape, n objects.  For every voxel
//   (z, y, x) with 1 <= labels[i] <= n, record labels[i] - 1 gains
//       count                                   1
//       sum_v, sum_vv, sum_vz, sum_vy, sum_vx   v, v^2, v z, v y, v x          (absolute voxel indices)
//       v_min, v_max                            the least and the greatest v
//   A record is 64 bytes: count (int64), the five sums (float64 for float32 values, uint64 for uint16 values), v_min and v_max
//   (float32, or uint32 holding the value) and 8 bytes of padding that stay zero.  The caller zeroes the table.  Labels outside
//   1 .. n are ignored; a label that no voxel carries keeps a zero record.
//
// float32 values.  count, v_min and v_max are exact and independent of the order of execution.  The extremes are compared
//   through label.hpp's float_key, which is lsr_label_regions_f32's convention: -0.0 sorts just below +0.0 (so a run of both has
//   v_min = -0.0 and v_max = +0.0) and a NaN sorts outside the infinities by its sign bit (a NaN with the sign bit clear is the
//   object's v_max, one with the sign bit set its v_min; the other extreme is that of the remaining values).
//   Every sum is within 2 n_k 2^-53 sum|terms| of the exact sum of its terms, n_k the object's voxel count, the terms the exact
//   real products: v * v is exact in float64 (48 bits) and so is v * c for a coordinate c < 2^29; an accumulation of n_k terms
//   in any order and any grouping costs at most n_k roundings; the second n_k pays for z * sum_v and y * sum_v being formed once
//   per run on the device (a run lies inside one row, so z and y are constant along it).  The twin adds voxel by voxel.  A
//   non-finite voxel follows IEEE arithmetic into its own object's sums and touches no other object's.
//
// uint16 values.  Pure integer arithmetic: device, twin and restatement are equal byte for byte.  65535 * Z*Y*X * max(Z, Y, X)
//   must stay below 2^64 (the v * coordinate sums); the squares cannot overflow within 2^31 - 1 voxels (2^32 * 2^31).
#pragma once

#include <limits>

#include "label.hpp"

namespace lsr {
namespace intensity {

// One record of the table (part of the ABI: shrimpy_amd/segment.py reads both as structured arrays).
struct RecordF32 {
  int64_t count;
  double sum_v, sum_vv, sum_vz, sum_vy, sum_vx;
  float v_min, v_max;
  uint32_t pad[2];
};
struct RecordU16 {
  int64_t count;
  uint64_t sum_v, sum_vv, sum_vz, sum_vy, sum_vx;
  uint32_t v_min, v_max;
  uint32_t pad[2];
};
constexpr int kSums = 6;                            // the 64-bit fields in front of a record: count and the five sums
constexpr int kWords = 8;                           // a record in 64-bit words
static_assert(sizeof(RecordF32) == 8 * kWords && sizeof(RecordU16) == 8 * kWords, "the records' size is part of the ABI");

constexpr int kThreads = 256;                       // one workgroup
constexpr int kChunks = 4;                          // wave steps of 64 voxels a wave has in flight
constexpr int kStep = kThreads * kChunks;           // voxels one workgroup takes per stride of its span
// The per-workgroup table: per slot six 64-bit sums, two 32-bit codes and the int32 key = 60 bytes, field-major; a label's first
// slot is label & (slots - 1), as in moments.hpp.  Slots and cap are chosen from the sweep in profiles/intensity_config2.jsonl
// (64 .. 512 slots, caps 1024 .. 262144, config-2 shape), which started from the moment kernel's 128 slots at 16 384 workgroups:
// on the bead scene every form takes the same time (the walk is bound by the label read); on the all-foreground volume every
// table size takes the same 7.1 - 7.2 ms at 16 384 and at 65 536 workgroups, and 25 ms at 262 144, where the eight same-record
// global atomics of each workgroup's flush queue up; on labelled noise, which is bound by the global atomics of its 46 million
// records, 512 slots at 65 536 workgroups take 43 ms where 128 at 16 384 take 61.  So 512 slots (30 KiB: five workgroups per
// CU, which costs the other two scenes nothing) at 65 536 workgroups.  The probe bound makes no difference on any scene (1 .. 32).
constexpr int kLdsSlots = 512;
constexpr int kMaxLdsSlots = 512;                   // (what the measurement entry accepts)
constexpr int kLdsProbes = 8;                       // a head gives up on LDS after this many slots and goes to global memory
constexpr int kDefaultBlocks = 65536;
constexpr int kMaxBlocks = 1 << 20;
static_assert((kLdsSlots & (kLdsSlots - 1)) == 0 && (kMaxLdsSlots & (kMaxLdsSlots - 1)) == 0, "the LDS table is masked");

// While it is accumulated a record holds two codes under atomicMax for which the caller's zeros are the neutral element, as in
// label.hip: v_max = code(v), v_min = ~code(v).  code is label.hpp's float_key for a float and the value itself for a uint16
// (never 0xffffffff, so ~code is never 0: an occupied record is recognised by its count alone).
__host__ __device__ inline uint32_t code_of(float v) { return label::float_key(v); }
__host__ __device__ inline uint32_t code_of(uint16_t v) { return v; }

// 65535 * Z*Y*X * max(Z, Y, X) < 2^64, evaluated without overflow (the extents are positive and the volume is below 2^31).
inline bool u16_sums_in_range(int64_t Z, int64_t Y, int64_t X) {
  const uint64_t m = static_cast<uint64_t>(Z > Y ? (Z > X ? Z : X) : (Y > X ? Y : X));       // < 2^31: 65535 m < 2^47
  return static_cast<uint64_t>(Z * Y * X) <= std::numeric_limits<uint64_t>::max() / (65535ull * m);
}

// The entry checks (the shape of moments::check_moments): everything wrong with a call is refused here, before any launch and
// before anything is read or written.
inline int check_intensity(const void* labels, const void* values, int value_bytes, int64_t Z, int64_t Y, int64_t X,
                           int64_t n_objects, const void* table, int max_blocks) {
  LSR_REQUIRE(labels != nullptr && values != nullptr && table != nullptr, LSR_E_ARG, "labels, values and table must not be NULL");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_ARG, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE(n_objects >= 0 && n_objects <= label::kMaxVoxels, LSR_E_ARG, "%lld objects: 0 .. 2^31 - 1", (long long)n_objects);
  LSR_REQUIRE(max_blocks >= 0, LSR_E_ARG, "max_blocks %d: 0 (the default) or a positive cap", max_blocks);
  if (int rc = label::check_volume(Z, Y, X)) return rc;              // (LSR_E_UNSUPPORTED above 2^31 - 1 voxels)
  if (value_bytes == 2)
    LSR_REQUIRE(u16_sums_in_range(Z, Y, X), LSR_E_UNSUPPORTED,
                "shape (%lld,%lld,%lld): 65535 * voxels * (greatest extent) must stay below 2^64 for the uint16 sums to fit",
                (long long)Z, (long long)Y, (long long)X);
  const uintptr_t voxels = static_cast<uintptr_t>(Z * Y * X);
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(table), t1 = t0 + static_cast<uintptr_t>(n_objects) * sizeof(RecordF32);
  const uintptr_t l0 = reinterpret_cast<uintptr_t>(labels), l1 = l0 + voxels * sizeof(int32_t);
  const uintptr_t v0 = reinterpret_cast<uintptr_t>(values), v1 = v0 + voxels * static_cast<uintptr_t>(value_bytes);
  LSR_REQUIRE(t1 <= l0 || l1 <= t0, LSR_E_ARG, "table must not overlap labels");
  LSR_REQUIRE(t1 <= v0 || v1 <= t0, LSR_E_ARG, "table must not overlap values");
  return LSR_OK;
}

// The twins' walk (host_twins.hip), voxel by voxel in raster order; the extremes are compared through the kernel's codes.
template <typename V, typename Record, typename Sum>
inline void accumulate_host(const int32_t* labels, const V* values, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                            Record* rows) {
  for (int64_t z = 0; z < Z; ++z) {
    for (int64_t y = 0; y < Y; ++y) {
      const int64_t row = (z * Y + y) * X;
      for (int64_t x = 0; x < X; ++x) {
        const int32_t l = labels[row + x];
        if (l < 1 || l > n_objects) continue;
        Record& r = rows[l - 1];
        const V f = values[row + x];
        const Sum g = static_cast<Sum>(f);
        const bool first = r.count == 0;
        r.count += 1;
        r.sum_v += g;
        r.sum_vv += g * g;
        r.sum_vz += g * static_cast<Sum>(z);
        r.sum_vy += g * static_cast<Sum>(y);
        r.sum_vx += g * static_cast<Sum>(x);
        const uint32_t k = code_of(f);
        if (first || k < code_of(static_cast<V>(r.v_min))) r.v_min = f;
        if (first || k > code_of(static_cast<V>(r.v_max))) r.v_max = f;
      }
    }
  }
}

}  // namespace intensity
}  // namespace lsr
