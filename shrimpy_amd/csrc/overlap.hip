// The contingency table of two label volumes (shrimpy_amd/track.py): for every pair (a, b), the number of voxels that are a
// at one timepoint and b at the next.  The rule, the record and the entry checks are overlap.hpp's; tests/track_ref.py
// restates the rule with np.unique.  Integer arithmetic only: the set of records does not depend on the order of execution.
//
// Every voxel may contribute, so the reduction happens on chip and global memory is touched rarely:
//
//   span     the linear index is cut into one contiguous span per workgroup (a multiple of kStep voxels), which the workgroup
//            walks in strides of kStep: a wave takes kChunks runs of 64 consecutive indices per stride, every load of a and
//            of b (at the shifted address) issued before the first is used.  A contiguous span sees the objects of one slab of
//            the volume, not a slice of every object: fewer distinct pairs per workgroup.
//   runs     one __ballot of "this lane's pair differs from the previous lane's" gives the heads of the runs of equal pairs
//            among the 64; a run's weight is a bit count on that mask.  Only head lanes insert.
//   LDS      heads insert into a per-workgroup table of kLdsSlots records in LDS (atomicCAS on the 64-bit key, atomicAdd on a
//            32-bit count: a workgroup sees fewer than 2^31 voxels), probing at most kLdsProbes slots; a head that finds none
//            goes straight to the global table with its weight.
//   flush    the LDS table lives across the whole span and is flushed once at its end: one global atomicCAS + atomicAdd per
//            occupied slot.  An all-foreground volume costs one global atomic pair per workgroup.
//
// The two hard rules of label.hip hold: words shared inside the launch (the LDS table between the barriers, the global table,
// counts) are touched by atomics only, and no workgroup ever waits for another; every loop is bounded.

#include <algorithm>

#include "overlap.hpp"

namespace {

namespace ov = lsr::overlap;

struct Shape {
  int Z, Y, X;
};

// One contribution to the global table: claim or find the pair's slot within `probes`, add the weight; count what is lost.
__device__ __forceinline__ void global_add(ov::Overlap* table, unsigned mask, int probes, unsigned long long pair,
                                           unsigned weight, int* counts) {
  if (lsr::pair_insert(table, mask, probes, pair, counts,
                       [&](ov::Overlap& slot) { atomicAdd(&slot.count, static_cast<unsigned long long>(weight)); }))
    return;
  atomicAdd(&counts[1], static_cast<int>(weight));
}

__global__ __launch_bounds__(ov::kThreads) void label_overlap_kernel(const int* __restrict__ a, const int* __restrict__ b, Shape s,
                                                                     int sz, int sy, int sx, int64_t n, int64_t span,
                                                                     unsigned mask, int probes, ov::Overlap* table, int* counts) {
  __shared__ unsigned long long keys[ov::kLdsSlots];
  __shared__ unsigned weights[ov::kLdsSlots];
  for (int i = threadIdx.x; i < ov::kLdsSlots; i += ov::kThreads) {
    keys[i] = 0ull;
    weights[i] = 0u;
  }
  __syncthreads();

  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const unsigned plane = static_cast<unsigned>(s.Y) * static_cast<unsigned>(s.X);      // (< 2^31: the volume is)
  const bool shifted = (sz | sy | sx) != 0;
  const int64_t offset = (static_cast<int64_t>(sz) * s.Y + sy) * s.X + sx;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * span, last = first + span < n ? first + span : n;

  // (the loop's bounds are the workgroup's: every wave makes the same number of trips, every lane of a wave reaches __ballot)
  for (int64_t base = first; base < last; base += ov::kStep) {
    int av[ov::kChunks], bv[ov::kChunks];
#pragma unroll
    for (int c = 0; c < ov::kChunks; ++c) {
      const int64_t v = base + (wave * ov::kChunks + c) * lsr::kWave + lane;
      av[c] = 0;
      bv[c] = 0;
      if (v >= n) continue;
      bool in = true;
      if (shifted) {        // (|shift| < extent on every axis: the sums stay in int)
        const unsigned uv = static_cast<unsigned>(v);
        const int z = static_cast<int>(uv / plane), r = static_cast<int>(uv % plane), y = r / s.X, x = r % s.X;
        in = z + sz >= 0 && z + sz < s.Z && y + sy >= 0 && y + sy < s.Y && x + sx >= 0 && x + sx < s.X;
      }
      av[c] = a[v];
      if (in) bv[c] = b[v + offset];        // (u inside the volume: 0 <= v + offset < n)
    }
#pragma unroll
    for (int c = 0; c < ov::kChunks; ++c) {
      const unsigned long long pair = (av[c] > 0 && bv[c] > 0) ? ov::pack(av[c], bv[c]) : 0ull;
      const unsigned long long before = __shfl_up(pair, 1);
      const unsigned long long heads = __ballot(lane == 0 || pair != before);
      if (pair == 0ull || !((heads >> lane) & 1ull)) continue;
      // the run: from this lane up to the lane in front of the next head (or the wave's end)
      const unsigned long long above = heads & ~((2ull << lane) - 1ull);       // (lane 63: 2 << 63 == 0, nothing above)
      const unsigned long long next = above & (0ull - above);                  // the next head's bit, 0 without one
      const unsigned weight = __popcll((next - 1ull) & ~((1ull << lane) - 1ull));
      unsigned slot = lsr::pair_slot_of(pair, ov::kLdsSlots - 1);
      bool placed = false;
      for (int p = 0; p < ov::kLdsProbes; ++p, slot = (slot + 1) & (ov::kLdsSlots - 1)) {
        const unsigned long long old = atomicCAS(&keys[slot], 0ull, pair);
        if (old == 0ull || old == pair) {
          atomicAdd(&weights[slot], weight);
          placed = true;
          break;
        }
      }
      if (!placed) global_add(table, mask, probes, pair, weight, counts);
    }
  }
  __syncthreads();

  for (int i = threadIdx.x; i < ov::kLdsSlots; i += ov::kThreads) {
    const unsigned long long pair = keys[i];
    if (pair != 0ull) global_add(table, mask, probes, pair, weights[i], counts);
  }
}

}  // namespace

extern "C" int lsr_label_overlap_geometry(int out[2]) {
  LSR_REQUIRE_PTR(out);
  out[0] = ov::kLdsSlots;
  out[1] = ov::kDefaultBlocks;
  return LSR_OK;
}

extern "C" int lsr_label_overlap_i32(const int32_t* a, const int32_t* b, int64_t Z, int64_t Y, int64_t X,
                                     const int32_t shift_zyx[3], int64_t capacity, void* table, int32_t* counts, int max_blocks,
                                     lsr_stream_t stream) {
  if (int rc = ov::check_overlap(a, b, Z, Y, X, shift_zyx, capacity, table, counts, max_blocks)) return rc;
  const int64_t n = Z * Y * X;
  hipStream_t q = lsr::as_stream(stream);
  hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), q);
  if (e != hipSuccess) return lsr::fail(static_cast<int>(e), "lsr_label_overlap_i32: %s", hipGetErrorString(e));
  if (ov::shift_empties(Z, Y, X, shift_zyx)) return LSR_OK;        // no voxel has a partner: the table stays empty
  const int64_t cap = std::min<int64_t>(max_blocks > 0 ? max_blocks : ov::kDefaultBlocks, ov::kMaxBlocks);
  const int64_t steps = lsr::ceil_div(n, ov::kStep);
  const int64_t span = lsr::ceil_div(steps, std::min(steps, cap)) * ov::kStep;       // voxels per workgroup, whole strides
  const int64_t blocks = lsr::ceil_div(n, span);
  const Shape s{static_cast<int>(Z), static_cast<int>(Y), static_cast<int>(X)};
  hipLaunchKernelGGL(label_overlap_kernel, dim3(static_cast<unsigned>(blocks)), dim3(ov::kThreads), 0, q, a, b, s, shift_zyx[0],
                     shift_zyx[1], shift_zyx[2], n, span, static_cast<unsigned>(capacity - 1),
                     lsr::pair_probes(capacity), static_cast<ov::Overlap*>(table), counts);
  return lsr::launch_status("lsr_label_overlap_i32");
}
