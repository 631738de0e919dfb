// Rank filters of a float32 volume under a box window (shrimpy_amd/rank.py): rank, median, percentile and the outlier removal
// on the median.  The rule, the fold, the selection and the fused op are in rank.hpp; PINNED to scipy.ndimage.rank_filter /
// median_filter / percentile_filter with mode = "reflect" (tests/rank_ref.py).
//
// One launch, nothing between workgroups, no atomics, no scratch.  A workgroup of 256 threads takes a (4, 8, 64) tile of
// outputs and stages the CODES (morph::encode) of the tile plus a halo of r per side in LDS -- at most 10 x 14 x 70 words,
// 39.2 KB -- with the reflect border resolved at load time through three small tables of folded indices, so the selection
// does no border logic.  A wavefront takes one x row of the tile at a time: its lanes read consecutive words of LDS.
//   register path  rank_kernel<RZ, RY, RX> for every half-width triple of {0, 1}^3 but (0, 0, 0): a lane reads its n <= 27
//                  codes from LDS once, in a fully unrolled loop, SORTS them in registers by Batcher's odd-even merge network
//                  (3, 28 and 156 compare-exchanges for n = 3, 9, 27: a minimum and a maximum each, no branch, no index that
//                  is not a constant) and takes the rank-th.  The sorted multiset is what the bisection counts in, so the
//                  code is the same; the bisection over registers it replaced costs 2 * 32 * n instructions per voxel.
//   generic path   rank_kernel<-1, -1, -1>: every other window (and every window under variant = 1); each of the 32 sweeps
//                  of the bisection reads the n codes from LDS again.
// The op's comparison is fused into the store (it reads the caller's volume at the voxel it writes).

#include <algorithm>
#include <utility>

#include "rank.hpp"

namespace {

namespace rk = lsr::rank;
namespace mo = lsr::morph;

constexpr int64_t kMaxBlocks = int64_t(1) << 20;
constexpr int kMaxEdge = rk::kTileX + 2 * rk::kMaxHalfWidth;      // the longest halo'd edge: the x one
constexpr int kAhead = 4;                                         // rows a wavefront has in flight while it stages the tile
static_assert(kMaxEdge <= 2 * lsr::kWave, "a staged row is one access of a wavefront and a tail");

// Batcher's odd-even merge sort of N keys as a list of compare-exchanges (a < b: the smaller key goes to a), built at compile
// time.  The network is the one for the next power of two with every exchange that touches an index >= N left out: keys
// thought at those indices are the greatest, sit at the top from the start and are never moved by an exchange that sends the
// greater key up.  (It sorts every 0-1 input for N = 3, 9 and 27: checked exhaustively.)
template <int N>
struct Network {
  int a[6 * N], b[6 * N], count;
  constexpr Network() : a{}, b{}, count(0) {
    int t = 1;
    while (t < N) t *= 2;
    for (int p = 1; p < t; p *= 2)
      for (int k = p; k >= 1; k /= 2)
        for (int j = k % p; j + k < t; j += 2 * k)
          for (int i = 0; i < k; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < N) {
              a[count] = i + j;
              b[count] = i + j + k;
              ++count;
            }
  }
};
template <int N>
inline constexpr Network<N> kNetwork{};
static_assert(kNetwork<3>.count == 3 && kNetwork<9>.count == 28 && kNetwork<27>.count == 156, "the exchanges of the three windows");

template <int N, size_t... I>
__device__ __forceinline__ void sort_keys(uint32_t (&c)[N], std::index_sequence<I...>) {
  auto exchange = [](uint32_t& lo, uint32_t& hi) {
    const uint32_t least = lo < hi ? lo : hi, greatest = lo < hi ? hi : lo;
    lo = least;
    hi = greatest;
  };
  (exchange(c[kNetwork<N>.a[I]], c[kNetwork<N>.b[I]]), ...);
}

template <int RZ, int RY, int RX>
__global__ __launch_bounds__(rk::kThreads) void rank_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t Z,
                                                            int64_t Y, int64_t X, int rz_, int ry_, int rx_, int rank, int op,
                                                            float threshold) {
  constexpr bool kRegisters = RZ >= 0;
  const int rz = kRegisters ? RZ : rz_, ry = kRegisters ? RY : ry_, rx = kRegisters ? RX : rx_;
  extern __shared__ uint32_t codes[];            // [ez][ey][ex]
  __shared__ int64_t at_z[rk::kTileZ + 2 * rk::kMaxHalfWidth], at_y[rk::kTileY + 2 * rk::kMaxHalfWidth], at_x[kMaxEdge];
  const int ez = rk::kTileZ + 2 * rz, ey = rk::kTileY + 2 * ry, ex = rk::kTileX + 2 * rx;
  const int wz = 2 * rz + 1, wy = 2 * ry + 1, wx = 2 * rx + 1;
  const int need = wz * wy * wx - rank;
  const int tid = threadIdx.x, lane = tid & (lsr::kWave - 1), wave = tid / lsr::kWave;
  constexpr int kWaves = rk::kThreads / lsr::kWave;
  const int64_t tiles_y = (Y + rk::kTileY - 1) / rk::kTileY, tiles_x = (X + rk::kTileX - 1) / rk::kTileX;
  const int64_t tiles = (Z + rk::kTileZ - 1) / rk::kTileZ * tiles_y * tiles_x;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t tzi = tile / (tiles_y * tiles_x), rest = tile - tzi * tiles_y * tiles_x, tyi = rest / tiles_x;
    const int64_t z0 = tzi * rk::kTileZ, y0 = tyi * rk::kTileY, x0 = (rest - tyi * tiles_x) * rk::kTileX;
    // the folded source index of every plane, row and column of the halo'd tile (element offsets for z and y)
    if (tid < ez) at_z[tid] = rk::fold(z0 - rz + tid, Z) * Y * X;
    if (tid >= lsr::kWave && tid - lsr::kWave < ey) at_y[tid - lsr::kWave] = rk::fold(y0 - ry + tid - lsr::kWave, Y) * X;
    if (tid >= 2 * lsr::kWave && tid - 2 * lsr::kWave < ex) at_x[tid - 2 * lsr::kWave] = rk::fold(x0 - rx + tid - 2 * lsr::kWave, X);
    __syncthreads();
    // kAhead rows of a wavefront at a time, every load issued before the first code is stored (ex <= 70: a row is one full
    // access and a tail of 2 * rx lanes)
    for (int row0 = wave; row0 < ez * ey; row0 += kWaves * kAhead) {
      float body[kAhead], tail[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int row = row0 + u * kWaves;
        if (row < ez * ey) {
          const int lz = row / ey, ly = row - lz * ey;
          const float* src = in + at_z[lz] + at_y[ly];
          body[u] = src[at_x[lane]];
          if (lane + lsr::kWave < ex) tail[u] = src[at_x[lane + lsr::kWave]];
        }
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int row = row0 + u * kWaves;
        if (row < ez * ey) {
          codes[row * ex + lane] = mo::encode(body[u], false);
          if (lane + lsr::kWave < ex) codes[row * ex + lane + lsr::kWave] = mo::encode(tail[u], false);
        }
      }
    }
    __syncthreads();
    const int64_t x = x0 + lane;
    for (int row = wave; row < rk::kTileZ * rk::kTileY; row += kWaves) {
      const int tz = row / rk::kTileY, ty = row - tz * rk::kTileY;
      const int64_t z = z0 + tz, y = y0 + ty;
      if (z >= Z || y >= Y || x >= X) continue;                   // (no barrier inside this loop)
      const uint32_t* win = codes + (tz * ey + ty) * ex + lane;   // the window's first code: offsets (-rz, -ry, -rx)
      uint32_t chosen;
      if constexpr (kRegisters) {
        constexpr int N = (2 * RZ + 1) * (2 * RY + 1) * (2 * RX + 1);
        uint32_t c[N];
#pragma unroll
        for (int dz = 0; dz < 2 * RZ + 1; ++dz)
#pragma unroll
          for (int dy = 0; dy < 2 * RY + 1; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2 * RX + 1; ++dx)
              c[(dz * (2 * RY + 1) + dy) * (2 * RX + 1) + dx] = win[(dz * ey + dy) * ex + dx];
        sort_keys(c, std::make_index_sequence<kNetwork<N>.count>{});
        chosen = c[0];
#pragma unroll
        for (int i = 1; i < N; ++i) chosen = rank == i ? c[i] : chosen;
      } else {
        chosen = rk::bisect(need, [&](uint32_t candidate) {
          int count = 0;
          for (int dz = 0; dz < wz; ++dz)
            for (int dy = 0; dy < wy; ++dy) {
              const uint32_t* line = win + (dz * ey + dy) * ex;
              for (int dx = 0; dx < wx; ++dx) count += line[dx] >= candidate ? 1 : 0;
            }
          return count;
        });
      }
      const int64_t e = (z * Y + y) * X + x;
      const float m = mo::decode(chosen, false);
      out[e] = rk::fused(m, op != rk::kValue ? in[e] : m, op, threshold);
    }
    __syncthreads();                             // the next tile overwrites the tables and the codes
  }
}

template <int RZ, int RY, int RX>
void launch(dim3 grid, size_t lds, hipStream_t st, const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry,
            int rx, int rank, int op, float threshold) {
  hipLaunchKernelGGL((rank_kernel<RZ, RY, RX>), grid, dim3(rk::kThreads), lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold);
}

}  // namespace

extern "C" int lsr_rank_filter_tiling(int tiling[4]) {
  LSR_REQUIRE_PTR(tiling);
  tiling[0] = rk::kMaxHalfWidth;
  tiling[1] = rk::kTileZ;
  tiling[2] = rk::kTileY;
  tiling[3] = rk::kTileX;
  return LSR_OK;
}

extern "C" int lsr_rank_filter_f32(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int rank,
                                   int op, float threshold, int variant, lsr_stream_t stream) {
  if (int rc = rk::check_rank(in, out, Z, Y, X, rz, ry, rx, rank, op, threshold, variant)) return rc;
  hipStream_t st = lsr::as_stream(stream);
  const int64_t tiles = lsr::ceil_div(Z, rk::kTileZ) * lsr::ceil_div(Y, rk::kTileY) * lsr::ceil_div(X, rk::kTileX);
  const dim3 grid(static_cast<unsigned>(std::min(tiles, kMaxBlocks)));
  const size_t lds = sizeof(uint32_t) * (rk::kTileZ + 2 * rz) * (rk::kTileY + 2 * ry) * (rk::kTileX + 2 * rx);
  const int key = variant == rk::kGeneric || std::max({rz, ry, rx}) > 1 ? 0 : rz * 4 + ry * 2 + rx;
  switch (key) {
    case 1: launch<0, 0, 1>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;
    case 2: launch<0, 1, 0>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;
    case 3: launch<0, 1, 1>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;
    case 4: launch<1, 0, 0>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;
    case 5: launch<1, 0, 1>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;
    case 6: launch<1, 1, 0>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;
    case 7: launch<1, 1, 1>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;
    default: launch<-1, -1, -1>(grid, lds, st, in, out, Z, Y, X, rz, ry, rx, rank, op, threshold); break;   // (all-zero: n = 1)
  }
  return lsr::launch_status("lsr_rank_filter_f32");
}
