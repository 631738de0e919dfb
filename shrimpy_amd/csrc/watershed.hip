// Splitting touching objects: a watershed by steepest ascent (shrimpy_amd/watershed.py).  The rule is stated in watershed.hpp
// and restated in numpy in tests/watershed_ref.py; no upstream is pinned.  Basins are the connected components of the edges
// {v, up(v)}, so this is the labelling of label.hip over a selected subset of the neighbour edges: the same union-find on one
// int32 word per voxel kept in the output buffer (label_uf.hpp), the same launch structure, the same two hard rules
// (coherence: a word another workgroup may write during a launch is touched by agent-scope atomics only; no waiting: no
// workgroup ever waits for another).  No flooding queue, no loop over grey levels; the result does not depend on the order
// of execution.
//
//   local    one workgroup stages objects and the keys of surface of one (8, 8, 64) tile plus a one-voxel halo in LDS (two
//            words per halo voxel: 52 800 B, three workgroups per CU; a tile without an object voxel ends there, its words
//            written), derives up(v) of every voxel of the tile, writes it as
//            one direction byte per voxel to scratch, unites v with up(v) in LDS where both lie in the tile, and writes
//            parent[v] = the GLOBAL index of v's tile-local root, -1 on the background.  The keys' LDS words become the
//            tile's parent words once every up(v) is known.
//   merge    reads the direction bytes (four per thread and load; a word of four summits or background voxels ends there)
//            and unites v with up(v) where that lies in another tile (atomicMin on the parent words).
//   flatten, count, scan, rank, final: the labelling's (label_uf.hpp).
//
// The saddles are one more launch: every pair of forward neighbours of one object in two basins goes into an open-addressing
// table -- the pair claimed by a compare-and-swap on an empty slot, the pass folded in by atomicMax on its key -- with linear
// probing bounded by min(capacity, 256) slots; a pair that finds none is counted and the caller comes back with a larger
// table.  The table's words are touched by atomics only.

#include "label_uf.hpp"
#include "watershed.hpp"

namespace {

namespace lb = lsr::label;
namespace ws = lsr::watershed;

constexpr int kRows = ws::kTileZ * ws::kTileY;                    // tile rows of kTileX = 64 voxels: one wave step each
constexpr int kHaloRows = (ws::kTileZ + 2) * ws::kHaloY;
constexpr int kBatch = 5;                                         // halo rows a wave has in flight
static_assert(ws::kTileX == lsr::kWave, "a tile row is one wavefront");
static_assert(kRows % kWaves == 0, "whole steps");
static_assert(ws::kTileVoxels <= ws::kHaloVoxels, "the tile's parent words fit where the keys were");
static_assert(2 * ws::kHaloVoxels * sizeof(int) <= 64 * 1024, "static LDS");

struct Shape {
  int Z, Y, X;
};

// ---- local: one tile and its halo in LDS --------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void watershed_local_kernel(const int* __restrict__ objects, const float* __restrict__ surface,
                                                                   Shape s, int level, int tiles_y, int tiles_x, unsigned tiles,
                                                                   int* __restrict__ parent, unsigned char* dir) {
  __shared__ int W[2 * ws::kHaloVoxels];
  int* O = W;                              // objects, 0 on the background and outside the volume
  int* K = W + ws::kHaloVoxels;            // the keys' bits
  int* P = K;                              // ... and, once every up(v) is known, the tile's parent words
  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const int64_t plane = static_cast<int64_t>(s.Y) * s.X;
  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
  const int tx = static_cast<int>(tile % tiles_x), ty = static_cast<int>(tile / tiles_x % tiles_y),
            tz = static_cast<int>(tile / tiles_x / tiles_y);
  const int z0 = tz * ws::kTileZ, y0 = ty * ws::kTileY, x0 = tx * ws::kTileX;

  // a wave loads the tile's x range (64 aligned voxels) of kBatch halo rows at a time, every load issued before the first is
  // used; then one thread per halo row and side loads the voxel beside that range
  int any = 0;                             // does this thread see an object voxel INSIDE the tile?
  for (int r0 = wave; r0 < kHaloRows; r0 += kWaves * kBatch) {
    int o[kBatch];
    float f[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int r = r0 + b * kWaves, gz = z0 + r / ws::kHaloY - 1, gy = y0 + r % ws::kHaloY - 1, gx = x0 + lane;
      const bool in = r < kHaloRows && gz >= 0 && gz < s.Z && gy >= 0 && gy < s.Y && gx < s.X;
      const int64_t v = in ? gz * plane + static_cast<int64_t>(gy) * s.X + gx : 0;
      o[b] = in ? objects[v] : 0;
      f[b] = in ? surface[v] : 0.0f;
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {
      const int r = r0 + b * kWaves;
      if (r >= kHaloRows) continue;
      const int hz = r / ws::kHaloY, hy = r % ws::kHaloY;
      O[r * ws::kHaloX + lane + 1] = o[b] > 0 ? o[b] : 0;
      K[r * ws::kHaloX + lane + 1] = static_cast<int>(lb::float_key(f[b]));
      any |= (o[b] > 0 && hz >= 1 && hz <= ws::kTileZ && hy >= 1 && hy <= ws::kTileY) ? 1 : 0;
    }
  }
  for (int e = threadIdx.x; e < 2 * kHaloRows; e += kThreads) {
    const int r = e / 2, gz = z0 + r / ws::kHaloY - 1, gy = y0 + r % ws::kHaloY - 1;
    const int gx = e % 2 == 0 ? x0 - 1 : x0 + ws::kTileX, hx = e % 2 == 0 ? 0 : ws::kHaloX - 1;
    const bool in = gz >= 0 && gz < s.Z && gy >= 0 && gy < s.Y && gx >= 0 && gx < s.X;
    const int64_t v = in ? gz * plane + static_cast<int64_t>(gy) * s.X + gx : 0;
    const int o = in ? objects[v] : 0;
    O[r * ws::kHaloX + hx] = o > 0 ? o : 0;
    K[r * ws::kHaloX + hx] = in ? static_cast<int>(lb::float_key(surface[v])) : 0;
  }
  if (!__syncthreads_or(any)) {            // a tile of background: its words are written and that is all
    for (int r = wave; r < kRows; r += kWaves) {
      const int gz = z0 + r / ws::kTileY, gy = y0 + r % ws::kTileY, gx = x0 + lane;
      if (gz >= s.Z || gy >= s.Y || gx >= s.X) continue;
      const int64_t v = gz * plane + static_cast<int64_t>(gy) * s.X + gx;
      dir[v] = static_cast<unsigned char>(ws::kSelf);
      parent[v] = -1;
    }
    continue;                              // (everybody has read what it reads of W: the next tile may overwrite it)
  }

  // up(v): one direction byte per voxel of the volume (a summit and the background: kSelf)
  for (int r = wave; r < kRows; r += kWaves) {
    const int lz = r / ws::kTileY, ly = r % ws::kTileY;
    const int gz = z0 + lz, gy = y0 + ly, gx = x0 + lane;
    if (gz >= s.Z || gy >= s.Y || gx >= s.X) continue;
    const int h = ((lz + 1) * ws::kHaloY + ly + 1) * ws::kHaloX + lane + 1;
    const int o = O[h];
    int code = ws::kSelf;
    if (o > 0) {
      code = ws::up_code(static_cast<uint32_t>(K[h]), level, [&](int dz, int dy, int dx, uint32_t* key) {
        const int j = h + (dz * ws::kHaloY + dy) * ws::kHaloX + dx;
        if (O[j] != o) return false;
        *key = static_cast<uint32_t>(K[j]);
        return true;
      });
    }
    dir[gz * plane + static_cast<int64_t>(gy) * s.X + gx] = static_cast<unsigned char>(code);
  }
  __syncthreads();            // (nobody reads a key any more)

  for (int r = wave; r < kRows; r += kWaves) {
    const int lz = r / ws::kTileY, ly = r % ws::kTileY;
    const bool inside = z0 + lz < s.Z && y0 + ly < s.Y && x0 + lane < s.X;
    const int h = ((lz + 1) * ws::kHaloY + ly + 1) * ws::kHaloX + lane + 1;
    P[r * ws::kTileX + lane] = (inside && O[h] > 0) ? r * ws::kTileX + lane : -1;
  }
  __syncthreads();

  // v joins up(v) where that lies in this tile (the byte is this thread's own store)
  for (int r = wave; r < kRows; r += kWaves) {
    const int lz = r / ws::kTileY, ly = r % ws::kTileY, i = r * ws::kTileX + lane;
    if (ld_lds(P + i) < 0) continue;
    const int code = dir[(z0 + lz) * plane + static_cast<int64_t>(y0 + ly) * s.X + x0 + lane];
    if (code == ws::kSelf) continue;
    const int dz = code / 9 - 1, dy = code / 3 % 3 - 1, dx = code % 3 - 1;
    if (lz + dz < 0 || lz + dz >= ws::kTileZ || ly + dy < 0 || ly + dy >= ws::kTileY || lane + dx < 0 || lane + dx >= ws::kTileX)
      continue;
    unite<true>(P, i, i + (dz * ws::kTileY + dy) * ws::kTileX + dx);      // (the target is in v's object: foreground)
  }
  __syncthreads();

  for (int r = wave; r < kRows; r += kWaves) {
    const int gz = z0 + r / ws::kTileY, gy = y0 + r % ws::kTileY, gx = x0 + lane;
    if (gz >= s.Z || gy >= s.Y || gx >= s.X) continue;
    int root = -1;
    if (P[r * ws::kTileX + lane] >= 0) {
      const int a = find<true>(P, r * ws::kTileX + lane);              // (nothing writes P any more)
      const int rr = a / ws::kTileX;
      root = static_cast<int>((z0 + rr / ws::kTileY) * plane + static_cast<int64_t>(y0 + rr % ws::kTileY) * s.X + x0 + a % ws::kTileX);
    }
    parent[gz * plane + static_cast<int64_t>(gy) * s.X + gx] = root;
  }
  __syncthreads();            // (W is the next tile's)
  }
}

// ---- merge: the ascents that cross a tile face ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void watershed_merge_kernel(int* parent, const unsigned char* __restrict__ dir, Shape s, int64_t n) {
  const unsigned plane = static_cast<unsigned>(s.Y) * static_cast<unsigned>(s.X);      // (< 2^31: the volume is)
  const int64_t words = (n + 3) / 4;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; q < words; q += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int64_t v0 = q * 4;
    unsigned w;
    if (v0 + 4 <= n) {
      w = *reinterpret_cast<const unsigned*>(dir + v0);      // (dir is 4-aligned: it follows the int32 block counts)
    } else {
      w = 0;
      for (int k = 0; k < 4; ++k) w |= static_cast<unsigned>(v0 + k < n ? dir[v0 + k] : ws::kSelf) << (8 * k);
    }
    if (w == 0x0d0d0d0du) continue;
    static_assert(ws::kSelf == 0x0d, "four summits in a word");
    for (int k = 0; k < 4; ++k) {
      const int code = static_cast<int>((w >> (8 * k)) & 0xffu);
      if (code == ws::kSelf || code > 26) continue;
      const unsigned uv = static_cast<unsigned>(v0 + k);
      const int z = static_cast<int>(uv / plane), y = static_cast<int>(uv % plane / static_cast<unsigned>(s.X)),
                x = static_cast<int>(uv % plane % static_cast<unsigned>(s.X));
      const int dz = code / 9 - 1, dy = code / 3 % 3 - 1, dx = code % 3 - 1;
      const int lz = z % ws::kTileZ, ly = y % ws::kTileY, lx = x % ws::kTileX;
      const bool crosses = (dz < 0 && lz == 0) || (dz > 0 && lz == ws::kTileZ - 1) || (dy < 0 && ly == 0) ||
                           (dy > 0 && ly == ws::kTileY - 1) || (dx < 0 && lx == 0) || (dx > 0 && lx == ws::kTileX - 1);
      if (!crosses) continue;
      if (z + dz < 0 || z + dz >= s.Z || y + dy < 0 || y + dy >= s.Y || x + dx < 0 || x + dx >= s.X) continue;
      const int v = static_cast<int>(uv);
      const int t = v + dz * static_cast<int>(plane) + dy * s.X + dx;
      if (ld(parent + v) < 0 || ld(parent + t) < 0) continue;      // (a word's sign never changes in this launch)
      unite<false>(parent, v, t);
    }
  }
}

// ---- saddles --------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void watershed_saddles_kernel(const int* __restrict__ objects, const int* __restrict__ basins,
                                                                     const float* __restrict__ surface, Shape s, int64_t n, int level,
                                                                     unsigned mask, int probes, ws::Saddle* table, int* counts) {
  const unsigned plane = static_cast<unsigned>(s.Y) * static_cast<unsigned>(s.X);
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; v < n; v += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int o = objects[v], a0 = basins[v];
    if (o <= 0 || a0 <= 0) continue;
    const unsigned uv = static_cast<unsigned>(v);
    const int z = static_cast<int>(uv / plane), y = static_cast<int>(uv % plane / static_cast<unsigned>(s.X)),
              x = static_cast<int>(uv % plane % static_cast<unsigned>(s.X));
    const uint32_t kv = lb::float_key(surface[v]);
    for (int dz = 0; dz <= 1; ++dz) {
      for (int dy = -1; dy <= 1; ++dy) {
        for (int dx = -1; dx <= 1; ++dx) {
          if (!ws::forward_neighbour(dz, dy, dx, level)) continue;
          if (z + dz >= s.Z || y + dy < 0 || y + dy >= s.Y || x + dx < 0 || x + dx >= s.X) continue;
          const int64_t u = v + dz * static_cast<int64_t>(plane) + dy * s.X + dx;
          if (objects[u] != o) continue;
          const int b0 = basins[u];
          if (b0 <= 0 || b0 == a0) continue;
          const uint32_t ku = lb::float_key(surface[u]), pass = ku < kv ? ku : kv;
          const unsigned long long a = static_cast<unsigned>(a0 < b0 ? a0 : b0), b = static_cast<unsigned>(a0 < b0 ? b0 : a0);
          const unsigned long long pair = a << 32 | b;
          // lsr::pair_insert spelled out: through the template hipcc gives this kernel 65 VGPRs where this loop takes 29
          unsigned slot = lsr::pair_slot_of(pair, mask);
          bool placed = false;
          for (int p = 0; p < probes; ++p, slot = (slot + 1) & mask) {      // bounded: nobody's progress is waited for
            const unsigned long long old = atomicCAS(&table[slot].pair, 0ull, pair);
            if (old == 0ull) atomicAdd(&counts[0], 1);
            if (old == 0ull || old == pair) {
              atomicMax(&table[slot].key, pass);
              placed = true;
              break;
            }
          }
          if (!placed) atomicAdd(&counts[1], 1);
        }
      }
    }
  }
}

constexpr int kLaunches = 7;       // local, merge, flatten, count, scan, rank, final

// The seven launches; a timing entry's marks (kLaunches + 1 events) get one in front of each launch and one behind the last.
int watershed_launches(const int32_t* objects, const float* surface, int64_t Z, int64_t Y, int64_t X, int connectivity,
                       int32_t* basins, int32_t* n_basins, void* scratch, hipStream_t q, lsr::LaunchMarks marks) {
  const int level = lb::level_of(connectivity);
  const Shape s{static_cast<int>(Z), static_cast<int>(Y), static_cast<int>(X)};
  const int64_t n = Z * Y * X;
  const int64_t tz = lsr::ceil_div(Z, ws::kTileZ), ty = lsr::ceil_div(Y, ws::kTileY), tx = lsr::ceil_div(X, ws::kTileX);
  int* counts = static_cast<int*>(scratch);
  unsigned char* dir = static_cast<unsigned char*>(scratch) + lb::number_blocks(n) * sizeof(int);
  marks.mark();
  // (tz * ty * tx <= n < 2^31 tiles; at most kMaxTileBlocks workgroups walk them)
  hipLaunchKernelGGL(watershed_local_kernel, dim3(static_cast<unsigned>(std::min(tz * ty * tx, kMaxTileBlocks))), dim3(kThreads), 0, q,
                     objects, surface, s, level, static_cast<int>(ty), static_cast<int>(tx), static_cast<unsigned>(tz * ty * tx),
                     basins, dir);
  marks.mark();
  hipLaunchKernelGGL(watershed_merge_kernel, dim3(stride_grid(lsr::ceil_div(n, 4))), dim3(kThreads), 0, q, basins, dir, s, n);
  number_launches(basins, n, counts, n_basins, q, marks);
  marks.mark();
  return lsr::launch_status("lsr_watershed_f32");
}

}  // namespace

extern "C" int lsr_watershed_tile_shape(int zyx[3]) {
  LSR_REQUIRE_PTR(zyx);
  zyx[0] = ws::kTileZ;
  zyx[1] = ws::kTileY;
  zyx[2] = ws::kTileX;
  return LSR_OK;
}

extern "C" int lsr_watershed_launch_geometry(int64_t out[5]) {
  LSR_REQUIRE_PTR(out);
  out[0] = kThreads;
  out[1] = lb::kChunk;
  out[2] = kScanThreads;
  out[3] = kMaxBlocks;
  out[4] = kMaxTileBlocks;
  return LSR_OK;
}

extern "C" int64_t lsr_watershed_scratch_bytes(int64_t Z, int64_t Y, int64_t X) {
  if (int rc = lb::check_volume(Z, Y, X)) return rc;
  return ws::scratch_bytes(Z * Y * X);       // (a byte per voxel: up to 2 GiB)
}

extern "C" int lsr_watershed_f32(const int32_t* objects, const float* surface, int64_t Z, int64_t Y, int64_t X, int connectivity,
                                 int32_t* basins, int32_t* n_basins, void* scratch, lsr_stream_t stream) {
  if (int rc = ws::check_watershed(objects, surface, Z, Y, X, connectivity, basins, n_basins, scratch)) return rc;
  return watershed_launches(objects, surface, Z, Y, X, connectivity, basins, n_basins, scratch, lsr::as_stream(stream), {});
}

// Measurement only (tools/bench_kernels.py --watershed): lsr_watershed_f32 with a HIP event between its launches; waits for
// the stream and writes the seven times in milliseconds to ms7 (HOST memory).
extern "C" int lsr_watershed_profile_f32(const int32_t* objects, const float* surface, int64_t Z, int64_t Y, int64_t X,
                                         int connectivity, int32_t* basins, int32_t* n_basins, void* scratch, float* ms7,
                                         lsr_stream_t stream) {
  if (int rc = ws::check_watershed(objects, surface, Z, Y, X, connectivity, basins, n_basins, scratch)) return rc;
  LSR_REQUIRE_PTR(ms7);
  hipStream_t q = lsr::as_stream(stream);
  return lsr::profile_launches<kLaunches>(ms7, q, "lsr_watershed_profile_f32", [&](lsr::LaunchMarks marks) {
    return watershed_launches(objects, surface, Z, Y, X, connectivity, basins, n_basins, scratch, q, marks);
  });
}

extern "C" int lsr_watershed_saddles_f32(const int32_t* objects, const int32_t* basins, const float* surface, int64_t Z, int64_t Y,
                                         int64_t X, int connectivity, int64_t capacity, void* table, int32_t* counts,
                                         lsr_stream_t stream) {
  if (int rc = ws::check_saddles(objects, basins, surface, Z, Y, X, connectivity, capacity, table, counts)) return rc;
  const Shape s{static_cast<int>(Z), static_cast<int>(Y), static_cast<int>(X)};
  const int64_t n = Z * Y * X;
  hipStream_t q = lsr::as_stream(stream);
  hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), q);
  if (e != hipSuccess) return lsr::fail(static_cast<int>(e), "lsr_watershed_saddles_f32: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(watershed_saddles_kernel, dim3(stride_grid(n)), dim3(kThreads), 0, q, objects, basins, surface, s, n,
                     lb::level_of(connectivity), static_cast<unsigned>(capacity - 1),
                     lsr::pair_probes(capacity), static_cast<ws::Saddle*>(table), counts);
  return lsr::launch_status("lsr_watershed_saddles_f32");
}
