// The volume, first and second moments of every object of a label volume (shrimpy_amd/segment.py: shape_table).  The rule, the
// record, the run sums and the entry checks are moments.hpp's; tests/moments_ref.py restates the rule with np.add.at.  Integer
// arithmetic only: the records do not depend on the order of execution.
//
// label_regions_kernel (label.hip) issues one set of global atomics per wave and run, which an all-foreground volume turns into
// one long queue on a single record.  This kernel takes overlap.hip's form instead:
//
//   span     the linear index is cut into one contiguous span per workgroup (a multiple of kStep voxels), which the workgroup
//            walks in strides of kStep: a wave takes kChunks runs of 64 consecutive voxels per stride, every load issued before
//            the first is used.
//   runs     a lane is a run head where its label differs from the lane before it, its voxel starts a row (x == 0) or it is
//            lane 0; one __ballot gives the heads, a bit scan to the next head the run's length L.  A run lies inside one row,
//            so its ten sums are closed forms of (z, y, x0, L) (moments.hpp run_sums): no shuffle reduction.  Only heads of
//            labels in 1 .. n contribute.
//   LDS      heads add into a per-workgroup open-addressing table in LDS (atomicCAS on the int32 key, ten 64-bit atomic adds),
//            probing at most kLdsProbes slots (a launch argument: the measurement entry varies it); a head that finds none
//            adds to the global record directly.
//   flush    the LDS table lives across the whole span and is flushed once: ten global 64-bit atomic adds per occupied slot.
//
// The two hard rules of label.hip hold: words shared inside the launch (the LDS table between the barriers, the global table)
// are touched by atomics only, and no workgroup ever waits for another; every loop is bounded.

#include <algorithm>

#include "moments.hpp"

namespace {

namespace mo = lsr::moments;

struct Shape {
  int Z, Y, X;
};

__device__ __forceinline__ void global_add(unsigned long long* table, int label, const mo::RunSums& r) {
  unsigned long long* rec = table + static_cast<int64_t>(label - 1) * mo::kFields;
#pragma unroll
  for (int k = 0; k < mo::kFields; ++k) atomicAdd(&rec[k], r.f[k]);
}

// kLds = false is the plain form (every head straight to the global record), kept for the measurement entry.
template <bool kLds>
__global__ __launch_bounds__(mo::kThreads) void label_moments_kernel(const int* __restrict__ labels, Shape s, int n_objects,
                                                                     int64_t n, int64_t span, int slots, int probes,
                                                                     unsigned long long* table) {
  extern __shared__ unsigned long long lds[];               // kFields * slots sums (field-major), then slots int32 keys
  unsigned long long* sums = lds;
  int* keys = reinterpret_cast<int*>(lds + mo::kFields * slots);
  const int slot_mask = slots - 1;
  if (kLds) {
    for (int i = threadIdx.x; i < mo::kFields * slots; i += mo::kThreads) sums[i] = 0ull;
    for (int i = threadIdx.x; i < slots; i += mo::kThreads) keys[i] = 0;
    __syncthreads();
  }

  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const unsigned X = static_cast<unsigned>(s.X), Y = static_cast<unsigned>(s.Y);
  const int64_t first = static_cast<int64_t>(blockIdx.x) * span, last = first + span < n ? first + span : n;

  // (the loop's bounds are the workgroup's: every wave makes the same number of trips, every lane of a wave reaches __ballot)
  for (int64_t base = first; base < last; base += mo::kStep) {
    int lab[mo::kChunks];
#pragma unroll
    for (int c = 0; c < mo::kChunks; ++c) {
      const int64_t v = base + (wave * mo::kChunks + c) * lsr::kWave + lane;
      lab[c] = v < last ? labels[v] : 0;              // (a span ends where the next workgroup's begins: v < last <= n)
    }
#pragma unroll
    for (int c = 0; c < mo::kChunks; ++c) {
      const int64_t v = base + (wave * mo::kChunks + c) * lsr::kWave + lane;
      const int l = (lab[c] >= 1 && lab[c] <= n_objects) ? lab[c] : 0;
      const unsigned uv = static_cast<unsigned>(v);     // (v < 2^31 + kStep)
      const unsigned row = uv / X, x = uv - row * X;
      const int before = __shfl_up(l, 1);
      const unsigned long long heads = __ballot(lane == 0 || l != before || x == 0u);
      if (l == 0 || !((heads >> lane) & 1ull)) continue;
      // the run: from this lane up to the lane in front of the next head (or the wave's end)
      const unsigned long long above = heads & ~((2ull << lane) - 1ull);       // (lane 63: 2 << 63 == 0, nothing above)
      const unsigned long long next = above & (0ull - above);                  // the next head's bit, 0 without one
      const unsigned L = __popcll((next - 1ull) & ~((1ull << lane) - 1ull));
      const unsigned z = row / Y, y = row - z * Y;
      const mo::RunSums r = mo::run_sums(z, y, x, L);
      bool placed = false;
      if (kLds) {
        int slot = l & slot_mask;
        for (int p = 0; p < probes; ++p, slot = (slot + 1) & slot_mask) {
          const int old = atomicCAS(&keys[slot], 0, l);
          if (old == 0 || old == l) {
#pragma unroll
            for (int k = 0; k < mo::kFields; ++k) atomicAdd(&sums[k * slots + slot], r.f[k]);
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

  for (int i = threadIdx.x; i < mo::kFields * slots; i += mo::kThreads) {
    const int slot = i & slot_mask, k = i / slots;
    const int l = keys[slot];
    const unsigned long long sum = sums[i];
    if (l != 0 && sum != 0ull) atomicAdd(&table[static_cast<int64_t>(l - 1) * mo::kFields + k], sum);
  }
}

int launch_moments(const char* what, const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, void* table,
                   int max_blocks, int slots, int probes, lsr_stream_t stream) {
  if (int rc = mo::check_moments(labels, Z, Y, X, n_objects, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  const int64_t n = Z * Y * X;
  const int64_t cap = std::min<int64_t>(max_blocks > 0 ? max_blocks : mo::kDefaultBlocks, mo::kMaxBlocks);
  const int64_t steps = lsr::ceil_div(n, mo::kStep);
  const int64_t span = lsr::ceil_div(steps, std::min(steps, cap)) * mo::kStep;       // voxels per workgroup, whole strides
  const int64_t blocks = lsr::ceil_div(n, span);
  const Shape s{static_cast<int>(Z), static_cast<int>(Y), static_cast<int>(X)};
  unsigned long long* t = static_cast<unsigned long long*>(table);
  hipStream_t q = lsr::as_stream(stream);
  if (slots > 0) {
    const size_t lds = static_cast<size_t>(slots) * (mo::kFields * sizeof(unsigned long long) + sizeof(int));
    hipLaunchKernelGGL(label_moments_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(mo::kThreads), lds, q, labels, s,
                       static_cast<int>(n_objects), n, span, slots, probes, t);
  } else {
    hipLaunchKernelGGL(label_moments_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(mo::kThreads), 0, q, labels, s,
                       static_cast<int>(n_objects), n, span, 1, 0, t);
  }
  return lsr::launch_status(what);
}

}  // namespace

extern "C" int lsr_label_moments_geometry(int out[2]) {
  LSR_REQUIRE_PTR(out);
  out[0] = mo::kLdsSlots;
  out[1] = mo::kDefaultBlocks;
  return LSR_OK;
}

extern "C" int lsr_label_moments_i32(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, void* table,
                                     int max_blocks, lsr_stream_t stream) {
  return launch_moments("lsr_label_moments_i32", labels, Z, Y, X, n_objects, table, max_blocks, mo::kLdsSlots, mo::kLdsProbes, stream);
}

extern "C" int lsr_label_moments_variant_i32(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                                             void* table, int max_blocks, int lds_slots, int lds_probes, lsr_stream_t stream) {
  LSR_REQUIRE(lds_slots >= 0 && lds_slots <= mo::kMaxLdsSlots && (lds_slots & (lds_slots - 1)) == 0, LSR_E_ARG,
              "lds_slots %d: 0 (no LDS table) or a power of two up to %d", lds_slots, mo::kMaxLdsSlots);
  LSR_REQUIRE(lds_probes >= 1 && lds_probes <= mo::kMaxLdsSlots, LSR_E_ARG, "lds_probes %d: 1 .. %d", lds_probes,
              mo::kMaxLdsSlots);
  return launch_moments("lsr_label_moments_variant_i32", labels, Z, Y, X, n_objects, table, max_blocks, lds_slots, lds_probes,
                        stream);
}
