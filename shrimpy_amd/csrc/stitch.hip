// Stitching: K overlapping tiles composed into one box of their common canvas (shrimpy_amd/stitch.py; biahub's stitch is
// not vendored -- PARITY UNPINNED, the rule is defined in stitch.hpp and restated in tests/stitch_ref.py).
//
// A gather, not a scatter: every output voxel is written once, from the tile voxels under it; no accumulator canvas, no
// weight canvas, no normalisation pass, no atomics.  Algorithmic traffic: 4 * (tile voxels touched + box voxels) bytes.
//
// A workgroup owns runs of kRun consecutive voxels of one box row; runs are numbered in 64 bits and walked with a grid
// stride, so a box of any size is one launch.  Per run the workgroup walks the tile table once: whether a tile covers the
// row (z, y) and reaches into the run (x) is the same for every lane -- the table index and the run are wave-uniform and the
// table is read through the constant address space, so the entries come through scalar loads (in the listing: every read
// of an entry is an s_load from the table's base, none a vector load) -- and only tiles that do are gathered; the tiles are
// read through the global address space (global, not flat, loads).  A lane owns FOUR consecutive outputs:
// of every tile row under them it reads four (five with a fractional x translation) consecutive floats, cut out of the
// aligned 16-byte words that hold them wherever those words lie inside the tile's buffer (the phase is the same for every
// lane of a row), element by element at the tile's x edges; it stores in the widest form the address allows.  Nothing
// outside a tile's buffer is read and nothing outside the box written.

#include <algorithm>

#include "stitch.hpp"

namespace {

namespace st = lsr::stitch;

// The tile table is read-only for the whole launch and its index is wave-uniform: read through the constant address space
// its entries are scalar loads into SGPRs.  A tile's address comes out of that table, so the compiler cannot know where it
// points: naming the global address space makes the tile reads global (not flat) loads.
using TableEntry = const __attribute__((address_space(4))) st::Tile;
using gfloat = const __attribute__((address_space(1))) float;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // (a builtin vector: it can live behind an address space)
using gword = const __attribute__((address_space(1))) u32x4;

constexpr int kThreads = 256;
constexpr int kOut = 4;                       // outputs per lane along x
constexpr int kRun = kThreads * kOut;         // voxels of a row per workgroup and step
constexpr int64_t kMaxBlocks = 4096;          // 16 per CU: the rest of a large box is walked with the grid stride

// N (4 or 5) consecutive floats at p, all inside the tile's buffer [lo, hi)
template <int N>
__device__ __forceinline__ void load_run(gfloat* p, float (&v)[N], gfloat* lo, gfloat* hi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uintptr_t first = a & ~uintptr_t(15);
  const int shift = static_cast<int>(a & 15) >> 2;
  if (N == 4 && shift == 0) {
    const u32x4 w = *reinterpret_cast<gword*>(first);
    __builtin_memcpy(v, &w, sizeof(w));
  } else if (first >= reinterpret_cast<uintptr_t>(lo) && first + 32 <= reinterpret_cast<uintptr_t>(hi)) {
    u32x4 w[2];
    w[0] = reinterpret_cast<gword*>(first)[0];
    w[1] = reinterpret_cast<gword*>(first)[1];
    float wide[8];
    __builtin_memcpy(wide, w, sizeof(w));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (shift == c) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = wide[i + c];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = p[i];
  }
}

// four consecutive outputs, all inside the box row
__device__ __forceinline__ void store_piece(float* p, const float (&v)[kOut]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0) {
    uint4 w;
    __builtin_memcpy(&w, v, sizeof(w));
    *reinterpret_cast<uint4*>(p) = w;
  } else if ((a & 7) == 0) {
    uint2 w[2];
    __builtin_memcpy(w, v, sizeof(w));
    reinterpret_cast<uint2*>(p)[0] = w[0];
    reinterpret_cast<uint2*>(p)[1] = w[1];
  } else {
#pragma unroll
    for (int i = 0; i < kOut; ++i) p[i] = v[i];
  }
}

__device__ __forceinline__ int64_t div_small(int64_t a, int64_t b) {
  return ((a | b) >> 32) == 0 ? static_cast<int64_t>(static_cast<uint32_t>(a) / static_cast<uint32_t>(b)) : a / b;
}

struct Args {
  TableEntry* table;
  float* out;
  int64_t o[3];          // box origin, absolute canvas coordinates
  int64_t b[3];          // box shape
  int64_t runs;          // ceil(b[2] / kRun) per row
  int64_t units;         // b[0] * b[1] * runs
  int n_tiles, p;
  float cval;
};

// One tile under one lane's four outputs: jx0 = the first output's j along x.  FX: the x translation is fractional.
template <bool FX>
__device__ __forceinline__ void gather(gfloat* lo, gfloat* hi, gfloat* row, int64_t nx, int64_t plane,
                                       bool fz, bool fy, float wz0, float wz1, float wy0, float wy1, float wx0, float wx1,
                                       int64_t jx0, int n_out, float dy, int p, st::Acc (&acc)[kOut]) {
  constexpr int F = FX ? 1 : 0, N = kOut + F;
  if (jx0 + kOut - 1 < F || jx0 > nx - 1) return;      // none of this lane's outputs lies under the tile
  const bool whole = n_out == kOut && jx0 >= F && jx0 + kOut - 1 <= nx - 1;
  float v[2][2][N];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const bool need = (a == 1 || fz) && (b == 1 || fy);      // (tap j - 1 exists only on a fractional axis)
      gfloat* q = row + (a - 1) * plane + (b - 1) * nx + (jx0 - F);
      if (need && whole) {
        load_run<N>(q, v[a][b], lo, hi);
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const int64_t x = jx0 - F + i;
          v[a][b][i] = (need && x >= 0 && x < nx) ? q[i] : 0.0f;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kOut; ++i) {
    if (i < n_out && st::covered(jx0 + i, nx, F)) {
      float r[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) r[a][b] = FX ? st::lerp(v[a][b][i], v[a][b][i + 1], wx0, wx1) : v[a][b][i];
      }
      const float s = st::tap(st::tap(r[0][0], r[0][1], fy, wy0, wy1), st::tap(r[1][0], r[1][1], fy, wy0, wy1), fz, wz0, wz1);
      acc[i].add(s, st::weight(dy, st::edge(jx0 + i, nx, wx0, wx1), p));
    }
  }
}

__global__ __launch_bounds__(kThreads) void stitch_kernel(Args g) {
  for (int64_t unit = blockIdx.x; unit < g.units; unit += gridDim.x) {
    // wave-uniform: the row and the run
    const int64_t rowi = div_small(unit, g.runs), run = unit - rowi * g.runs;
    const int64_t zb = div_small(rowi, g.b[1]), yb = rowi - zb * g.b[1];
    const int64_t cz = g.o[0] + zb, cy = g.o[1] + yb;
    const int64_t run_x0 = run * kRun, run_x1 = min(run_x0 + kRun, g.b[2]);     // box x range [run_x0, run_x1)
    // per lane
    const int64_t x0 = run_x0 + static_cast<int64_t>(threadIdx.x) * kOut;
    const int n_out = static_cast<int>(min(static_cast<int64_t>(kOut), g.b[2] - x0));    // <= 0: an idle lane
    st::Acc acc[kOut];
#pragma unroll
    for (int i = 0; i < kOut; ++i) acc[i].clear();

    for (int k = 0; k < g.n_tiles; ++k) {
      TableEntry& e = g.table[k];                       // (k is wave-uniform: scalar loads)
      const int fz = e.frac[0], fy = e.frac[1], fx = e.frac[2];
      const int64_t nz = e.n[0], ny = e.n[1], nx = e.n[2];
      const int64_t jz = cz - e.ti[0], jy = cy - e.ti[1];
      if (!st::covered(jz, nz, fz) || !st::covered(jy, ny, fy)) continue;
      const int64_t jr0 = g.o[2] + run_x0 - e.ti[2], jr1 = g.o[2] + run_x1 - 1 - e.ti[2];   // the run's j range along x
      if (jr1 < fx || jr0 > nx - 1) continue;
      if (n_out <= 0) continue;
      gfloat* lo = (gfloat*)e.data;
      gfloat* hi = lo + nz * ny * nx;
      const int64_t plane = ny * nx;
      gfloat* row = lo + (jz * ny + jy) * nx;
      const float dy = st::edge(jy, ny, e.w0[1], e.w1[1]);
      const int64_t jx0 = g.o[2] + x0 - e.ti[2];
      if (fx) {
        gather<true>(lo, hi, row, nx, plane, fz != 0, fy != 0, e.w0[0], e.w1[0], e.w0[1], e.w1[1], e.w0[2], e.w1[2], jx0,
                     n_out, dy, g.p, acc);
      } else {
        gather<false>(lo, hi, row, nx, plane, fz != 0, fy != 0, e.w0[0], e.w1[0], e.w0[1], e.w1[1], e.w0[2], e.w1[2], jx0,
                      n_out, dy, g.p, acc);
      }
    }

    if (n_out > 0) {
      float o[kOut];
#pragma unroll
      for (int i = 0; i < kOut; ++i) o[i] = acc[i].finish(g.cval);
      float* dst = g.out + rowi * g.b[2] + x0;
      if (n_out == kOut) {
        store_piece(dst, o);
      } else {
#pragma unroll
        for (int i = 0; i < kOut; ++i)
          if (i < n_out) dst[i] = o[i];
      }
    }
  }
}

}  // namespace

extern "C" int lsr_stitch_max_tiles(void) { return st::kMaxTiles; }

extern "C" int lsr_stitch_table_bytes(int n_tiles) {
  if (n_tiles <= 0 || n_tiles > st::kMaxTiles) return 0;
  return n_tiles * static_cast<int>(sizeof(st::Tile));
}

extern "C" int lsr_stitch_canvas(const int64_t* shapes, const double* translations, int n_tiles, int64_t origin[3],
                                 int64_t shape[3]) {
  LSR_REQUIRE_PTR(shapes);
  LSR_REQUIRE_PTR(translations);
  LSR_REQUIRE_PTR(origin);
  LSR_REQUIRE_PTR(shape);
  if (int rc = st::check_count(n_tiles)) return rc;
  const int dummy = 0;       // (the geometry needs no tile data: any non-NULL address passes the pointer check)
  for (int k = 0; k < n_tiles; ++k)
    if (int rc = st::check_tile(&dummy, shapes + 3 * k, translations + 3 * k, k)) return rc;
  st::canvas(shapes, translations, n_tiles, origin, shape);
  return LSR_OK;
}

extern "C" int lsr_stitch_prepare_table(const float* const* tiles, const int64_t* shapes, const double* translations,
                                        int n_tiles, void* table) {
  LSR_REQUIRE_PTR(tiles);
  LSR_REQUIRE_PTR(shapes);
  LSR_REQUIRE_PTR(translations);
  LSR_REQUIRE_PTR(table);
  if (int rc = st::check_count(n_tiles)) return rc;
  for (int k = 0; k < n_tiles; ++k)
    if (int rc = st::check_tile(tiles[k], shapes + 3 * k, translations + 3 * k, k)) return rc;
  st::Tile* t = static_cast<st::Tile*>(table);
  for (int k = 0; k < n_tiles; ++k) st::fill_tile(t[k], tiles[k], shapes + 3 * k, translations + 3 * k);
  return LSR_OK;
}

extern "C" int lsr_stitch_f32(const void* table, int n_tiles, float* out, const int64_t box_origin[3],
                              const int64_t box_shape[3], int p, float cval, lsr_stream_t stream) {
  if (int rc = st::check_launch(table, n_tiles, out, box_origin, box_shape, p)) return rc;
  Args g{};
  g.table = (TableEntry*)table;
  g.out = out;
  for (int a = 0; a < 3; ++a) {
    g.o[a] = box_origin[a];
    g.b[a] = box_shape[a];
  }
  g.runs = lsr::ceil_div(box_shape[2], kRun);
  g.units = box_shape[0] * box_shape[1] * g.runs;       // < 2^48: a box in range has fewer voxels than that
  g.n_tiles = n_tiles;
  g.p = p;
  g.cval = cval;
  const int64_t blocks = std::min(g.units, kMaxBlocks);
  hipLaunchKernelGGL(stitch_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, lsr::as_stream(stream), g);
  return lsr::launch_status("lsr_stitch_f32");
}
