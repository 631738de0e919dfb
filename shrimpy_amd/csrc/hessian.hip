// Ridge, sheet and blob filters on the eigenvalues of the Hessian of a smoothed float32 volume (shrimpy_amd/hessian.py).  The
// rule, the derivative, the six entries, the eigen solver, the responses and the NaN rule are in hessian.hpp; PINNED to numpy's
// np.gradient and np.linalg.eigvalsh (tests/hessian_ref.py).
//
// One launch, nothing between workgroups, no atomics, no scratch.  A workgroup of 256 threads takes an (8, 8, 64) tile of
// outputs and stages the tile of g plus a halo of 2 per side in LDS -- 12 x 12 x 68 floats, 39.2 KB.  Positions outside the
// volume are neither read nor written to LDS, and no voxel reads them back: the one-sided forms of the derivative are chosen
// from the voxel's index.  A wavefront takes one x row of the tile at a time: its lanes read consecutive words of LDS.  Every
// voxel computes H in float64, its eigenvalues by cyclic Jacobi, the measure in float32, and writes one float; with
// `accumulate` it reads `out` at that voxel first.  g is never written.

#include <algorithm>

#include "hessian.hpp"

namespace {

namespace hs = lsr::hessian;

constexpr int64_t kMaxBlocks = int64_t(1) << 20;
constexpr int kAhead = 4;                                         // rows a wavefront has in flight while it stages the tile

__global__ __launch_bounds__(hs::kThreads) void hessian_kernel(const float* __restrict__ g, float* __restrict__ out, int64_t Z,
                                                               int64_t Y, int64_t X, hs::Recip rc, double scale, int measure,
                                                               int dark, int accumulate) {
  __shared__ float tile[hs::kTileFloats];        // [kEdgeZ][kEdgeY][kEdgeX]
  const int tid = threadIdx.x, lane = tid & (lsr::kWave - 1), wave = tid / lsr::kWave;
  constexpr int kWaves = hs::kThreads / lsr::kWave;
  constexpr int kRows = hs::kEdgeZ * hs::kEdgeY;
  const int64_t tiles_y = (Y + hs::kTileY - 1) / hs::kTileY, tiles_x = (X + hs::kTileX - 1) / hs::kTileX;
  const int64_t tiles = (Z + hs::kTileZ - 1) / hs::kTileZ * tiles_y * tiles_x;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t tzi = t / (tiles_y * tiles_x), rest = t - tzi * tiles_y * tiles_x, tyi = rest / tiles_x;
    const int64_t z0 = tzi * hs::kTileZ, y0 = tyi * hs::kTileY, x0 = (rest - tyi * tiles_x) * hs::kTileX;
    // kAhead rows of a wavefront at a time, every load issued before the first value is stored (a row is one full access
    // and a tail of 2 * kHalo lanes); a row or a column outside the volume is skipped
    const int64_t gx = x0 - hs::kHalo + lane, gx_tail = gx + lsr::kWave;
    const bool body_in = gx >= 0 && gx < X, tail_in = lane < 2 * hs::kHalo && gx_tail < X;
    for (int row0 = wave; row0 < kRows; row0 += kWaves * kAhead) {
      float body[kAhead], tail[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int row = row0 + u * kWaves;
        const int lz = row / hs::kEdgeY, ly = row - lz * hs::kEdgeY;
        const int64_t gz = z0 - hs::kHalo + lz, gy = y0 - hs::kHalo + ly;
        body[u] = tail[u] = 0.0f;
        if (row < kRows && gz >= 0 && gz < Z && gy >= 0 && gy < Y) {
          const float* src = g + (gz * Y + gy) * X;
          if (body_in) body[u] = src[gx];
          if (tail_in) tail[u] = src[gx_tail];
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int row = row0 + u * kWaves;
        if (row < kRows) {
          tile[row * hs::kEdgeX + lane] = body[u];
          if (lane < 2 * hs::kHalo) tile[row * hs::kEdgeX + lane + lsr::kWave] = tail[u];
        }
      }
    }
    __syncthreads();
    const int64_t x = x0 + lane;
    for (int row = wave; row < hs::kTileZ * hs::kTileY; row += kWaves) {
      const int tz = row / hs::kTileY, ty = row - tz * hs::kTileY;
      const int64_t z = z0 + tz, y = y0 + ty;
      if (z >= Z || y >= Y || x >= X) continue;                   // (no barrier inside this loop)
      const float* at = tile + ((tz + hs::kHalo) * hs::kEdgeY + ty + hs::kHalo) * hs::kEdgeX + lane + hs::kHalo;
      auto load = [&](int dz, int dy, int dx) { return static_cast<double>(at[(dz * hs::kEdgeY + dy) * hs::kEdgeX + dx]); };
      const hs::Axis ax[3] = {{z, Z, rc.inv1[0], rc.inv2[0]}, {y, Y, rc.inv1[1], rc.inv2[1]}, {x, X, rc.inv1[2], rc.inv2[2]}};
      const float r = hs::voxel(load, ax, scale, measure, dark);
      const int64_t e = (z * Y + y) * X + x;
      out[e] = accumulate ? hs::greater_of(out[e], r) : r;
    }
    __syncthreads();                             // the next tile overwrites the staged values
  }
}

}  // namespace

extern "C" int lsr_hessian_tiling(int tiling[4]) {
  LSR_REQUIRE_PTR(tiling);
  tiling[0] = hs::kHalo;
  tiling[1] = hs::kTileZ;
  tiling[2] = hs::kTileY;
  tiling[3] = hs::kTileX;
  return LSR_OK;
}

extern "C" int lsr_hessian_response_f32(const float* g, float* out, int64_t Z, int64_t Y, int64_t X, double sz, double sy, double sx,
                                        double scale, int measure, int dark, int accumulate, lsr_stream_t stream) {
  if (int rc = hs::check_hessian(g, out, Z, Y, X, sz, sy, sx, scale, measure, dark, accumulate)) return rc;
  const int64_t tiles = lsr::ceil_div(Z, hs::kTileZ) * lsr::ceil_div(Y, hs::kTileY) * lsr::ceil_div(X, hs::kTileX);
  const dim3 grid(static_cast<unsigned>(std::min(tiles, kMaxBlocks)));
  hipLaunchKernelGGL(hessian_kernel, grid, dim3(hs::kThreads), 0, lsr::as_stream(stream), g, out, Z, Y, X,
                     hs::recip_of(sz, sy, sx), scale, measure, dark, accumulate);
  return lsr::launch_status("lsr_hessian_response_f32");
}
