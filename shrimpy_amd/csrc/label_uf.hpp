// Internal to label.hip and watershed.hip (device code: no host twin includes it): the union-find on int32 parent words that
// both keep in their output buffer, and the launches that turn its roots into labels.  parent[v] is a linear index <= v of the
// same set, -1 on the background; every set is rooted at its SMALLEST index, so the roots in raster order are the sets in
// label order and the numbering is a prefix count:
//
//   flatten  parent[v] <- root(v).  4 B read + 4 B written per voxel, plus the chain.
//   count    roots (parent[v] == v) per block of 4096 voxels -> scratch[block].  4 B read per voxel.
//   scan     one workgroup: exclusive prefix of the block counts in place, N -> *n_objects.
//   rank     parent[r] <- -(rank(r) + 2) for every root r (rank = roots before it).  4 B read per voxel, roots written.
//   final    labels[v] = rank(root(v)) + 1, 0 on the background.  4 B read + 4 B written per voxel, plus one gather.
//
// The two hard rules of label.hip hold for everything here.  Everything sits in an unnamed namespace: each of the two
// translation units compiles its own copy of the kernels into its own code object.
#pragma once

#include <algorithm>

#include "label.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / lsr::kWave;
constexpr int kPerThread = lsr::label::kChunk / kThreads;         // numbering launches: voxels per thread
constexpr int kScanThreads = 1024;
static_assert(lsr::label::kChunk % kThreads == 0, "whole steps");

// ---- union-find on LDS words (local) and on global words (merge, flatten) ------------------------------------------------

__device__ __forceinline__ int ld_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool LDS>
__device__ __forceinline__ int find(const int* P, int a) {
  for (;;) {
    const int p = LDS ? ld_lds(P + a) : ld(P + a);
    if (p == a) return a;
    a = p;                      // p < a: the walk ends
  }
}

template <bool LDS>
__device__ __forceinline__ void unite(int* P, int a, int b) {
  for (;;) {
    a = find<LDS>(P, a);
    b = find<LDS>(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }          // a > b: hang a under b
    const int old = atomicMin(P + a, b);
    if (old == a) return;       // a was still a root: linked
    a = old;                    // someone lowered parent[a] to old < a first: parent[a] = min(old, b) now, and uniting old with b
  }                             // keeps the link that lost; a strictly decreased
}

// ---- flatten --------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void label_flatten_kernel(int* parent, int64_t n) {
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; v < n; v += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int p = parent[v];                 // (this thread alone writes the word)
    if (p < 0 || p == v) continue;
    const int r = find<false>(parent, p);    // old and new values of the words on the way are both ancestors
    if (r != p) parent[v] = r;
  }
}

// ---- number: count, scan, rank, final ---------------------------------------------------------------------------------------------

// The roots of one 4096-voxel block: bit k of the result is voxel base + k * 256 + thread.
__device__ __forceinline__ unsigned root_bits(const int* __restrict__ parent, int64_t base, int64_t n) {
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t v = base + k * kThreads + threadIdx.x;
    if (v < n && parent[v] == static_cast<int>(v)) bits |= 1u << k;
  }
  return bits;
}

__global__ __launch_bounds__(kThreads) void label_count_kernel(const int* __restrict__ parent, int64_t n, int* __restrict__ counts) {
  __shared__ int part[kWaves];
  int c = __popc(root_bits(parent, static_cast<int64_t>(blockIdx.x) * lsr::label::kChunk, n));
  for (int d = lsr::kWave / 2; d > 0; d >>= 1) c += __shfl_down(c, d);
  if (threadIdx.x % lsr::kWave == 0) part[threadIdx.x / lsr::kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < kWaves; ++w) total += part[w];
    counts[blockIdx.x] = total;
  }
}

// one workgroup: counts[b] <- sum of counts[0 .. b), *n_objects <- the total
__global__ __launch_bounds__(kScanThreads) void label_scan_kernel(int* counts, int64_t blocks, int* n_objects) {
  __shared__ int sums[kScanThreads];
  const int64_t per = (blocks + kScanThreads - 1) / kScanThreads;
  const int64_t first = per * threadIdx.x, lo = first < blocks ? first : blocks, hi = lo + per < blocks ? lo + per : blocks;
  int mine = 0;
  for (int64_t b = lo; b < hi; ++b) mine += counts[b];
  sums[threadIdx.x] = mine;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {            // inclusive scan
    const int add = threadIdx.x >= static_cast<unsigned>(d) ? sums[threadIdx.x - d] : 0;
    __syncthreads();
    sums[threadIdx.x] += add;
    __syncthreads();
  }
  int run = sums[threadIdx.x] - mine;
  for (int64_t b = lo; b < hi; ++b) {
    const int c = counts[b];
    counts[b] = run;
    run += c;
  }
  if (threadIdx.x == kScanThreads - 1) *n_objects = sums[kScanThreads - 1];
}

__global__ __launch_bounds__(kThreads) void label_rank_kernel(int* __restrict__ parent, int64_t n, const int* __restrict__ offsets) {
  __shared__ unsigned long long masks[kPerThread][kWaves];
  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * lsr::label::kChunk;
  const unsigned bits = root_bits(parent, base, n);
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const unsigned long long mask = __ballot((bits >> k) & 1u);
    if (lane == 0) masks[k][wave] = mask;
  }
  __syncthreads();
  if (bits == 0) return;
  // voxel order inside the block: step k, then wave, then lane
  int run = offsets[blockIdx.x];
  for (int k = 0; k < kPerThread; ++k) {
    for (int w = 0; w < kWaves; ++w) {
      const unsigned long long mask = masks[k][w];
      if (w == wave && ((bits >> k) & 1u)) {
        const int rank = run + __popcll(mask & ((1ull << lane) - 1ull));
        parent[base + k * kThreads + threadIdx.x] = -(rank + 2);         // (a root's own word: nobody else reads it in this launch)
      }
      run += __popcll(mask);
    }
  }
}

__global__ __launch_bounds__(kThreads) void label_final_kernel(int* labels, int64_t n) {
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; v < n; v += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int p = labels[v];                 // (this thread alone writes the word)
    int out;
    if (p < 0) {
      out = -p - 1;                          // background -1 -> 0, a root -(rank + 2) -> rank + 1
    } else {
      const int r = ld(labels + p);          // the root's word: -(rank + 2) before its own thread has passed, rank + 1 after
      out = r < 0 ? -r - 1 : r;
    }
    labels[v] = out;
  }
}

constexpr int64_t kMaxBlocks = 1 << 16;      // grid-stride launches: 256 per CU
constexpr int64_t kMaxTileBlocks = 1 << 22;  // local: 2^22 * 256 threads < 2^32 (the config-2 grid has 1.9e5 labelling tiles)

inline unsigned stride_grid(int64_t n) { return static_cast<unsigned>(std::min(lsr::ceil_div(n, kThreads), kMaxBlocks)); }

// flatten, count, scan, rank, final on `stream`; `marks.mark()` is called in front of each launch (the timing entries record
// an event there).  counts: lsr::label::number_blocks(n) words.
inline void number_launches(int* parent, int64_t n, int* counts, int* n_objects, hipStream_t q, lsr::LaunchMarks& marks) {
  const int64_t blocks = lsr::label::number_blocks(n);
  marks.mark();
  hipLaunchKernelGGL(label_flatten_kernel, dim3(stride_grid(n)), dim3(kThreads), 0, q, parent, n);
  marks.mark();
  hipLaunchKernelGGL(label_count_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, q, parent, n, counts);
  marks.mark();
  hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kScanThreads), 0, q, counts, blocks, n_objects);
  marks.mark();
  hipLaunchKernelGGL(label_rank_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, q, parent, n, counts);
  marks.mark();
  hipLaunchKernelGGL(label_final_kernel, dim3(stride_grid(n)), dim3(kThreads), 0, q, parent, n);
}

}  // namespace
