// Connected-component labelling and the object table (shrimpy_amd/segment.py).  The oracle is scipy.ndimage.label
// (tests/label_ref.py): labels 1 .. N in raster rank of each component's lowest linear index, held to exact equality.
//
// A block-based union-find over one int32 word per voxel, kept in the `labels` buffer itself: parent[v] is a linear index
// <= v of the same component, -1 on the background, and every set is rooted at its SMALLEST index -- so the roots in
// raster order are the components in label order and the numbering is a prefix count.  Separate launches on the caller's
// stream; everything that one workgroup writes and another reads waits for a launch boundary, except as stated:
//
//   local    one workgroup labels one (4, 16, 64) tile in LDS.  The threshold is fused into the tile load (the mask is
//            never written).  A wave owns a tile row: the x runs come out of one ballot, then every voxel unites with the
//            foreground neighbours that precede it inside the tile (atomicMin in LDS).  Writes parent[v] = the GLOBAL index
//            of v's tile-local root, -1 for background: every voxel of the volume, 4 B read + 4 B written per voxel.
//   merge    every foreground voxel with a preceding neighbour in ANOTHER tile unites with it (atomicMin on the parent
//            words).  Reads the faces of the tiles (whole 128-B lines: ~4 B per voxel), writes only roots.
//   flatten  parent[v] <- root(v).  4 B read + 4 B written per voxel, plus the chain.
//   count    roots (parent[v] == v) per block of 4096 voxels -> scratch[block].  4 B read per voxel.
//   scan     one workgroup: exclusive prefix of the block counts in place, N -> *n_objects.
//   rank     parent[r] <- -(rank(r) + 2) for every root r (rank = roots before it).  4 B read per voxel, roots written.
//   final    labels[v] = rank(root(v)) + 1, 0 on the background.  4 B read + 4 B written per voxel, plus one gather.
//
// Two hard rules ("Labelling"):
// 1. Coherence.  The XCDs' L2s are not coherent for plain accesses inside a launch.  A word that another workgroup may
//    write during a launch is read in that launch only with an agent-scope atomic (ld() below; the writes are atomicMin),
//    or is such that its old and its new value are BOTH right: in `flatten` every value a parent word ever holds is an
//    ancestor of the voxel and the root's own word never changes; in `final` a root's word is -(rank + 2) before and
//    rank + 1 after, told apart by the sign; a word's sign never changes in `merge` (foreground stays >= 0).
// 2. No waiting.  No workgroup waits for another: no flags, no spin loops, no retry that needs someone else's progress.
//    Every loop here ends because an index strictly decreases: find() walks parent[a] < a, and unite() either installs its
//    link or continues from the strictly smaller value the atomicMin returned.

#include <climits>

#include "label_uf.hpp"

namespace {

namespace lb = lsr::label;

constexpr int kRows = lb::kTileZ * lb::kTileY;            // tile rows of kTileX = 64 voxels: one wave step each
static_assert(lb::kTileX == lsr::kWave, "a tile row is one wavefront");
static_assert(kRows % kWaves == 0, "whole steps");

// (the union-find on LDS and global words, and the launches flatten, count, scan, rank and final: label_uf.hpp)

// ---- local: one tile in LDS -------------------------------------------------------------------------------------------------

struct Shape {
  int Z, Y, X;
};

__global__ __launch_bounds__(kThreads) void label_local_kernel(const float* __restrict__ in, Shape s, float threshold, int level,
                                                               int tiles_y, int tiles_x, unsigned tiles,
                                                               int* __restrict__ parent) {
  __shared__ int L[lb::kTileVoxels];
  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  // (a grid stride over the tiles: a launch holds fewer than 2^32 threads, a volume can hold more tiles than 2^24)
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
  const int tx = static_cast<int>(tile % tiles_x), ty = static_cast<int>(tile / tiles_x % tiles_y),
            tz = static_cast<int>(tile / tiles_x / tiles_y);
  const int z0 = tz * lb::kTileZ, y0 = ty * lb::kTileY, x0 = tx * lb::kTileX;
  const int64_t plane = static_cast<int64_t>(s.Y) * s.X;

  // the x runs of every row: L[i] = the row's first voxel of i's run, -1 on the background and outside the volume
  for (int r = wave; r < kRows; r += kWaves) {
    const int gz = z0 + r / lb::kTileY, gy = y0 + r % lb::kTileY, gx = x0 + lane;
    const bool inside = gz < s.Z && gy < s.Y && gx < s.X;
    const bool fg = inside && in[gz * plane + static_cast<int64_t>(gy) * s.X + gx] > threshold;      // NaN > t is false
    const unsigned long long mask = __ballot(fg);
    const unsigned long long gaps = ~mask & ((1ull << lane) - 1ull);                 // background lanes below this one
    const int start = gaps ? 64 - __clzll(static_cast<long long>(gaps)) : 0;
    L[r * lb::kTileX + lane] = fg ? r * lb::kTileX + start : -1;
  }
  __syncthreads();

  // the other 12 preceding neighbours.  An edge is left out where two edges that ARE made imply it:
  //   dx == 0: the left neighbours of both ends are foreground -- they share the ends' runs and are joined by the same offset;
  //   dx != 0: (dz, dy, 0) is foreground -- it is a neighbour of this voxel under the same connectivity and shares the target's run.
  for (int r = wave; r < kRows; r += kWaves) {
    const int lz = r / lb::kTileY, ly = r % lb::kTileY, i = r * lb::kTileX + lane;
    if (ld_lds(L + i) < 0) continue;
    for (int dz = -1; dz <= 0; ++dz) {
      for (int dy = -1; dy <= 1; ++dy) {
        if (lz + dz < 0 || ly + dy < 0 || ly + dy >= lb::kTileY) continue;
        const int m = i + (dz * lb::kTileY + dy) * lb::kTileX;          // (dz, dy, 0)
        for (int dx = -1; dx <= 1; ++dx) {
          if (!lb::backward_neighbour(dz, dy, dx, level) || (dz == 0 && dy == 0)) continue;
          if (lane + dx < 0 || lane + dx >= lb::kTileX) continue;
          const int j = m + dx;
          if (ld_lds(L + j) < 0) continue;
          if (dx == 0 ? (lane > 0 && ld_lds(L + i - 1) >= 0 && ld_lds(L + j - 1) >= 0) : ld_lds(L + m) >= 0) continue;
          unite<true>(L, i, j);
        }
      }
    }
  }
  __syncthreads();

  for (int r = wave; r < kRows; r += kWaves) {
    const int gz = z0 + r / lb::kTileY, gy = y0 + r % lb::kTileY, gx = x0 + lane;
    if (gz >= s.Z || gy >= s.Y || gx >= s.X) continue;
    int root = -1;
    if (L[r * lb::kTileX + lane] >= 0) {
      const int a = find<true>(L, r * lb::kTileX + lane);              // (nothing writes L any more)
      const int rr = a / lb::kTileX;
      root = static_cast<int>((z0 + rr / lb::kTileY) * plane + static_cast<int64_t>(y0 + rr % lb::kTileY) * s.X + x0 + a % lb::kTileX);
    }
    parent[gz * plane + static_cast<int64_t>(gy) * s.X + gx] = root;
  }
  __syncthreads();            // (L is the next tile's)
  }
}

// ---- merge: the edges that cross a tile face ----------------------------------------------------------------------------------

// A workgroup walks (row, 256-voxel piece) units with a grid stride.  A row off the z and y faces of its tile has crossing
// edges only in its first and last tile columns: the other lanes read nothing.
__global__ __launch_bounds__(kThreads) void label_merge_kernel(int* parent, Shape s, int level, int64_t pieces, int64_t units) {
  const int64_t plane = static_cast<int64_t>(s.Y) * s.X;
  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t row = unit / pieces;
    const int z = static_cast<int>(row / s.Y), y = static_cast<int>(row % s.Y);
    const int64_t x64 = (unit % pieces) * kThreads + threadIdx.x;       // (up to X + 255: past int where X is within 255 of 2^31)
    if (x64 >= s.X) continue;
    const int x = static_cast<int>(x64);
    const int lz = z % lb::kTileZ, ly = y % lb::kTileY, lx = x % lb::kTileX;
    const bool row_face = lz == 0 || ly == 0 || ly == lb::kTileY - 1;
    if (!row_face && lx != 0 && lx != lb::kTileX - 1) continue;
    const int v = static_cast<int>(z * plane + static_cast<int64_t>(y) * s.X + x);
    if (ld(parent + v) < 0) continue;
    for (int dz = -1; dz <= 0; ++dz) {
      for (int dy = -1; dy <= 1; ++dy) {
        if (z + dz < 0 || y + dy < 0 || y + dy >= s.Y) continue;
        const int m = v + static_cast<int>(dz * plane + static_cast<int64_t>(dy) * s.X);       // (dz, dy, 0)
        for (int dx = -1; dx <= 1; ++dx) {
          if (!lb::backward_neighbour(dz, dy, dx, level)) continue;
          if (x + dx < 0 || x + dx >= s.X) continue;
          const bool crosses = (dz < 0 && lz == 0) || (dy < 0 && ly == 0) || (dy > 0 && ly == lb::kTileY - 1) ||
                               (dx < 0 && lx == 0) || (dx > 0 && lx == lb::kTileX - 1);
          if (!crosses) continue;
          const int t = m + dx;
          if (ld(parent + t) < 0) continue;
          // implied edges, as in the local launch (an x edge itself is never left out)
          if (dz != 0 || dy != 0) {
            if (dx == 0 ? (x > 0 && ld(parent + v - 1) >= 0 && ld(parent + t - 1) >= 0) : ld(parent + m) >= 0) continue;
          }
          unite<false>(parent, v, t);
        }
      }
    }
  }
}

// ---- the object table ---------------------------------------------------------------------------------------------------------------

// While it is accumulated a record holds images for which the host's zeros are the neutral element: lo[a] = INT_MAX - min,
// v_min = ~key(min), v_max = key(max) (label.hpp's order-preserving key), all under atomicMax; regions_finish decodes them.
struct Partial {
  long long count, sz, sy, sx;
  double sv, svz, svy, svx;
  int lo[3], hi[3];                          // lo as INT_MAX - c, hi as c + 1: both under max
  unsigned kmin, kmax;                       // ~key and key: both under max
};

__device__ __forceinline__ void absorb(Partial& a, int d, int id, int lane) {
  // the partial of lane + d, taken in where that lane belongs to the same run of equal labels (every lane executes the shuffles)
  const int other = __shfl_down(id, d);
  const bool same = lane + d < lsr::kWave && other == id;
  const long long count = __shfl_down(a.count, d), sz = __shfl_down(a.sz, d), sy = __shfl_down(a.sy, d), sx = __shfl_down(a.sx, d);
  const double sv = __shfl_down(a.sv, d), svz = __shfl_down(a.svz, d), svy = __shfl_down(a.svy, d), svx = __shfl_down(a.svx, d);
  int lo[3], hi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = __shfl_down(a.lo[c], d);
    hi[c] = __shfl_down(a.hi[c], d);
  }
  const unsigned kmin = __shfl_down(a.kmin, d), kmax = __shfl_down(a.kmax, d);
  if (!same) return;
  a.count += count; a.sz += sz; a.sy += sy; a.sx += sx;
  a.sv += sv; a.svz += svz; a.svy += svy; a.svx += svx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.lo[c] = max(a.lo[c], lo[c]);
    a.hi[c] = max(a.hi[c], hi[c]);
  }
  a.kmin = max(a.kmin, kmin);
  a.kmax = max(a.kmax, kmax);
}

__global__ __launch_bounds__(kThreads) void label_regions_kernel(const int* __restrict__ labels, const float* __restrict__ intensity,
                                                                 Shape s, int64_t n, int n_objects, lb::Region* table) {
  const int lane = threadIdx.x % lsr::kWave;
  const unsigned plane = static_cast<unsigned>(s.Y) * static_cast<unsigned>(s.X);      // (< 2^31: the volume is)
  for (int64_t v0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) - lane; v0 < n;
       v0 += static_cast<int64_t>(gridDim.x) * kThreads) {                               // v0: wave-uniform, 64 consecutive voxels
    const int64_t v = v0 + lane;
    int label = v < n ? labels[v] : 0;
    if (label < 0 || label > n_objects) label = 0;                                       // (never a row outside the table)
    if (__ballot(label != 0) == 0) continue;
    // runs of equal labels among consecutive lanes: id = the number of run heads up to this lane
    const int prev = __shfl_up(label, 1);
    const bool head = lane == 0 || prev != label;
    const unsigned long long heads = __ballot(head);
    const int id = __popcll(heads & ((2ull << lane) - 1ull));
    const unsigned uv = static_cast<unsigned>(v < n ? v : 0);
    const int z = static_cast<int>(uv / plane), y = static_cast<int>(uv % plane / static_cast<unsigned>(s.X)),
              x = static_cast<int>(uv % plane % static_cast<unsigned>(s.X));
    Partial a;
    a.count = 1; a.sz = z; a.sy = y; a.sx = x;
    a.lo[0] = INT_MAX - z; a.lo[1] = INT_MAX - y; a.lo[2] = INT_MAX - x;
    a.hi[0] = z + 1; a.hi[1] = y + 1; a.hi[2] = x + 1;
    a.sv = a.svz = a.svy = a.svx = 0.0;
    a.kmin = a.kmax = 0;
    if (intensity != nullptr && label != 0) {
      const float f = intensity[v];
      const double g = static_cast<double>(f);
      a.sv = g; a.svz = g * z; a.svy = g * y; a.svx = g * x;
      a.kmax = lb::float_key(f);
      a.kmin = ~a.kmax;
    }
    for (int d = 1; d < lsr::kWave; d <<= 1) absorb(a, d, id, lane);
    if (!head || label == 0) continue;
    // one set of atomics per wave and run
    lb::Region* r = table + (label - 1);
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->volume), static_cast<unsigned long long>(a.count));
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_zyx[0]), static_cast<unsigned long long>(a.sz));
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_zyx[1]), static_cast<unsigned long long>(a.sy));
    atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_zyx[2]), static_cast<unsigned long long>(a.sx));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      atomicMax(&r->lo[c], a.lo[c]);
      atomicMax(&r->hi[c], a.hi[c]);
    }
    if (intensity != nullptr) {
      unsafeAtomicAdd(&r->sum_v, a.sv);                 // (the hardware's float64 add, never a compare-and-swap loop)
      unsafeAtomicAdd(&r->sum_vzyx[0], a.svz);
      unsafeAtomicAdd(&r->sum_vzyx[1], a.svy);
      unsafeAtomicAdd(&r->sum_vzyx[2], a.svx);
      atomicMax(reinterpret_cast<unsigned*>(&r->v_min), a.kmin);
      atomicMax(reinterpret_cast<unsigned*>(&r->v_max), a.kmax);
    }
  }
}

__global__ __launch_bounds__(kThreads) void label_regions_finish_kernel(lb::Region* table, int n_objects, int has_intensity) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n_objects) return;
  lb::Region& r = table[k];
  if (r.volume == 0) return;                 // a label no voxel carries: the record stays zero
  for (int c = 0; c < 3; ++c) r.lo[c] = INT_MAX - r.lo[c];
  if (has_intensity) {
    unsigned kmin, kmax;
    memcpy(&kmin, &r.v_min, sizeof(kmin));
    memcpy(&kmax, &r.v_max, sizeof(kmax));
    r.v_min = lb::key_float(~kmin);
    r.v_max = lb::key_float(kmax);
  }
}

__global__ __launch_bounds__(kThreads) void label_remap_kernel(int* labels, int64_t n, const int* __restrict__ map, int n_map) {
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; v < n; v += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int l = labels[v];
    labels[v] = (l > 0 && l < n_map) ? map[l] : 0;      // (a label outside the map has no object: background)
  }
}

}  // namespace

extern "C" int lsr_label_tile_shape(int zyx[3]) {
  LSR_REQUIRE_PTR(zyx);
  zyx[0] = lb::kTileZ;
  zyx[1] = lb::kTileY;
  zyx[2] = lb::kTileX;
  return LSR_OK;
}

extern "C" int lsr_label_launch_geometry(int64_t out[5]) {
  LSR_REQUIRE_PTR(out);
  out[0] = kThreads;
  out[1] = lb::kChunk;
  out[2] = kScanThreads;
  out[3] = kMaxBlocks;
  out[4] = kMaxTileBlocks;
  return LSR_OK;
}

extern "C" int lsr_label_scratch_bytes(int64_t Z, int64_t Y, int64_t X) {
  if (int rc = lb::check_volume(Z, Y, X)) return rc;
  return static_cast<int>(lb::number_blocks(Z * Y * X) * sizeof(int));       // (at most 2 MiB)
}

namespace {

constexpr int kLaunches = 7;       // local, merge, flatten, count, scan, rank, final

// The seven launches; a timing entry's marks (kLaunches + 1 events) get one in front of each launch and one behind the last.
int label_launches(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int connectivity, int32_t* labels,
                   int32_t* n_objects, void* scratch, hipStream_t q, lsr::LaunchMarks marks) {
  const int level = lb::level_of(connectivity);
  const Shape s{static_cast<int>(Z), static_cast<int>(Y), static_cast<int>(X)};
  const int64_t n = Z * Y * X;
  const int64_t tz = lsr::ceil_div(Z, lb::kTileZ), ty = lsr::ceil_div(Y, lb::kTileY), tx = lsr::ceil_div(X, lb::kTileX);
  const int64_t pieces = lsr::ceil_div(X, kThreads), units = Z * Y * pieces;
  int* counts = static_cast<int*>(scratch);
  marks.mark();
  // (tz * ty * tx <= n < 2^31 tiles; at most kMaxTileBlocks workgroups walk them, one each at any shape met in practice)
  hipLaunchKernelGGL(label_local_kernel, dim3(static_cast<unsigned>(std::min(tz * ty * tx, kMaxTileBlocks))), dim3(kThreads), 0, q,
                     in, s, threshold, level, static_cast<int>(ty), static_cast<int>(tx), static_cast<unsigned>(tz * ty * tx),
                     labels);
  marks.mark();
  hipLaunchKernelGGL(label_merge_kernel, dim3(static_cast<unsigned>(std::min(units, kMaxBlocks))), dim3(kThreads), 0, q, labels, s,
                     level, pieces, units);
  number_launches(labels, n, counts, n_objects, q, marks);
  marks.mark();
  return lsr::launch_status("lsr_label_f32");
}

}  // namespace

extern "C" int lsr_label_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int connectivity,
                             int32_t* labels, int32_t* n_objects, void* scratch, lsr_stream_t stream) {
  if (int rc = lb::check_label(in, Z, Y, X, connectivity, labels, n_objects, scratch)) return rc;
  return label_launches(in, Z, Y, X, threshold, connectivity, labels, n_objects, scratch, lsr::as_stream(stream), {});
}

// Measurement only (tools/bench_kernels.py --label): lsr_label_f32 with a HIP event between its launches; waits for the
// stream and writes the seven times in milliseconds to ms7 (HOST memory).
extern "C" int lsr_label_profile_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int connectivity,
                                     int32_t* labels, int32_t* n_objects, void* scratch, float* ms7, lsr_stream_t stream) {
  if (int rc = lb::check_label(in, Z, Y, X, connectivity, labels, n_objects, scratch)) return rc;
  LSR_REQUIRE_PTR(ms7);
  hipStream_t q = lsr::as_stream(stream);
  return lsr::profile_launches<kLaunches>(ms7, q, "lsr_label_profile_f32", [&](lsr::LaunchMarks marks) {
    return label_launches(in, Z, Y, X, threshold, connectivity, labels, n_objects, scratch, q, marks);
  });
}

extern "C" int lsr_label_regions_f32(const int32_t* labels, const float* intensity, int64_t Z, int64_t Y, int64_t X,
                                     int64_t n_objects, void* table, lsr_stream_t stream) {
  if (int rc = lb::check_regions(labels, Z, Y, X, n_objects, table)) return rc;
  if (n_objects == 0) return LSR_OK;
  const Shape s{static_cast<int>(Z), static_cast<int>(Y), static_cast<int>(X)};
  const int64_t n = Z * Y * X;
  hipStream_t q = lsr::as_stream(stream);
  lb::Region* rows = static_cast<lb::Region*>(table);
  hipLaunchKernelGGL(label_regions_kernel, dim3(stride_grid(n)), dim3(kThreads), 0, q, labels, intensity, s, n,
                     static_cast<int>(n_objects), rows);
  hipLaunchKernelGGL(label_regions_finish_kernel, dim3(static_cast<unsigned>(lsr::ceil_div(n_objects, kThreads))), dim3(kThreads), 0,
                     q, rows, static_cast<int>(n_objects), intensity != nullptr ? 1 : 0);
  return lsr::launch_status("lsr_label_regions_f32");
}

extern "C" int lsr_label_remap_i32(int32_t* labels, int64_t n, const int32_t* map, int64_t n_map, lsr_stream_t stream) {
  if (int rc = lb::check_remap(labels, n, map, n_map)) return rc;
  hipLaunchKernelGGL(label_remap_kernel, dim3(stride_grid(n)), dim3(kThreads), 0, lsr::as_stream(stream), labels, n, map,
                     static_cast<int>(n_map));
  return lsr::launch_status("lsr_label_remap_i32");
}
