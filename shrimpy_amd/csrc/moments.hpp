// What the label-moment kernel (moments.hip) and its host twin (host_twins.hip) share: the rule, the record, the geometry, the
// run sums and the entry checks -- ONE definition each.  No upstream is pinned: the rule below IS the specification
// (tests/moments_ref.py restates it with np.add.at on int64), and device, twin and restatement are equal byte for byte.
//
// Rule.  labels: an int32 (Z, Y, X) volume, n objects.  For every voxel (z, y, x) with 1 <= labels[v] <= n, record
//   labels[v] - 1 gains
//       volume                               1
//       s_z, s_y, s_x                        z, y, x
//       m_zz, m_yy, m_xx, m_zy, m_zx, m_yx   z^2, y^2, x^2, zy, zx, yx
//   in absolute voxel indices.  A record is ten int64 in that order, 80 bytes; the caller zeroes the table.  Labels outside
//   1 .. n are ignored; a label that no voxel carries keeps a zero record.
//   Range: Z*Y*X <= 2^31 - 1 (label::check_volume) and Z*Y*X * max(Z, Y, X)^2 < 2^63, so that no sum can wrap: a sum is at most
//   voxels * (max extent - 1)^2.  (171, 2048, 2270): 2^29.6 * 2^22.3, eleven bits inside.
//   Pure integer arithmetic: the records do not depend on the order of execution.
#pragma once

#include <limits>

#include "label.hpp"

namespace lsr {
namespace moments {

// One record of the table (part of the ABI: shrimpy_amd/segment.py reads it as a structured array).
struct Moments {
  int64_t volume;
  int64_t s_z, s_y, s_x;
  int64_t m_zz, m_yy, m_xx, m_zy, m_zx, m_yx;
};
constexpr int kFields = 10;
static_assert(sizeof(Moments) == 8 * kFields, "the moment record's size is part of the ABI");

constexpr int kThreads = 256;                       // one workgroup
constexpr int kChunks = 4;                          // wave steps of 64 voxels a wave has in flight
constexpr int kStep = kThreads * kChunks;           // voxels one workgroup takes per stride of its span
// The per-workgroup table: kLdsSlots int32 keys + kFields * kLdsSlots 64-bit sums = 10.5 KiB, so that the LDS does not limit the
// workgroups of a CU.  A label's first slot is label & (kLdsSlots - 1): the labels of a span are close to consecutive (they are
// numbered in raster order), which this hash spreads without a collision.  Slots and cap are chosen from the sweep in
// profiles/moments_config2.jsonl (64 .. 512 slots, caps 1024 .. 262144, config-2 shape): 128 slots at 16 384 workgroups are the
// fastest on the bead scene and on the all-foreground volume; 512 slots cost both a half more (fewer workgroups per CU, a longer
// flush) and gain only on labelled noise, which stays bound by its 46 million records' global atomics in every form.
constexpr int kLdsSlots = 128;
constexpr int kMaxLdsSlots = 512;                   // (what the measurement entry accepts)
constexpr int kLdsProbes = 8;                       // a head gives up on LDS after this many slots and goes to global memory
// The grid's cap.  An all-foreground volume costs kFields same-record global atomics per workgroup: at 65 536 workgroups they
// take three times as long as the whole walk, at 16 384 they no longer show.
constexpr int kDefaultBlocks = 16384;
constexpr int kMaxBlocks = 1 << 20;
static_assert((kLdsSlots & (kLdsSlots - 1)) == 0 && (kMaxLdsSlots & (kMaxLdsSlots - 1)) == 0, "the LDS table is masked");

// The ten sums of a run of L voxels (z, y, x0 .. x0 + L - 1) inside one row, in closed form.  Unsigned: the arithmetic is that
// of int64 wherever the range check holds.  L is a wave's at most (64): the products of L below stay far inside 64 bits.  The
// host twin adds voxel by voxel and so checks this form.
struct RunSums {
  unsigned long long f[kFields];
};
__host__ __device__ inline RunSums run_sums(unsigned z, unsigned y, unsigned x0, unsigned L) {
  const unsigned long long l = L, uz = z, uy = y, ux = x0;
  const unsigned long long tri = l * (l - 1) / 2;                          // sum of 0 .. L-1
  const unsigned long long sq = (l - 1) * l * (2 * l - 1) / 6;             // sum of 0^2 .. (L-1)^2
  const unsigned long long sx = l * ux + tri;
  RunSums r;
  r.f[0] = l;
  r.f[1] = uz * l;
  r.f[2] = uy * l;
  r.f[3] = sx;
  r.f[4] = uz * uz * l;
  r.f[5] = uy * uy * l;
  r.f[6] = l * ux * ux + 2 * ux * tri + sq;
  r.f[7] = uz * uy * l;
  r.f[8] = uz * sx;
  r.f[9] = uy * sx;
  return r;
}

// Z*Y*X * max(Z, Y, X)^2 < 2^63, evaluated without overflow (the extents are positive and the volume is below 2^31).
inline bool sums_in_range(int64_t Z, int64_t Y, int64_t X) {
  const int64_t m = Z > Y ? (Z > X ? Z : X) : (Y > X ? Y : X);       // < 2^31: m * m < 2^62
  const int64_t limit = std::numeric_limits<int64_t>::max();        // 2^63 - 1
  return Z * Y * X <= limit / (m * m);
}

// The entry checks: everything wrong with a call is refused here, before any launch and before anything is read or written.
inline int check_moments(const void* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, const void* table,
                         int max_blocks) {
  LSR_REQUIRE(labels != nullptr && table != nullptr, LSR_E_ARG, "labels and table must not be NULL");
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_ARG, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE(n_objects >= 0 && n_objects <= label::kMaxVoxels, LSR_E_ARG, "%lld objects: 0 .. 2^31 - 1", (long long)n_objects);
  LSR_REQUIRE(max_blocks >= 0, LSR_E_ARG, "max_blocks %d: 0 (the default) or a positive cap", max_blocks);
  if (int rc = label::check_volume(Z, Y, X)) return rc;              // (LSR_E_UNSUPPORTED above 2^31 - 1 voxels)
  LSR_REQUIRE(sums_in_range(Z, Y, X), LSR_E_UNSUPPORTED,
              "shape (%lld,%lld,%lld): voxels * (greatest extent)^2 must stay below 2^63 for the second moments to fit int64",
              (long long)Z, (long long)Y, (long long)X);
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(table), t1 = t0 + static_cast<uintptr_t>(n_objects) * sizeof(Moments);
  const uintptr_t l0 = reinterpret_cast<uintptr_t>(labels), l1 = l0 + static_cast<uintptr_t>(Z * Y * X) * sizeof(int32_t);
  LSR_REQUIRE(t1 <= l0 || l1 <= t0, LSR_E_ARG, "table must not overlap labels");
  return LSR_OK;
}

}  // namespace moments
}  // namespace lsr
