// Mid-band spectral power of every z plane of a volume: the focus measure of the time-lapse stabilization
// (shrimpy_amd/focus.py; waveorder's focus_from_transverse_band, which biahub's estimate-stabilization uses for z --
// neither is vendored: PARITY UNPINNED, the rule is defined in focus.py and restated in tests/focus_ref.py).
//
//   P[z] = sum over the bins (ky, kx) of fft2(window of plane z) with  band_lo < r(ky, kx) < band_hi  of |F(ky, kx)|,
//   r = sqrt((min(ky, Yc - ky) / (Yc p))^2 + (min(kx, Xc - kx) / (Xc p))^2)
//
// on the half spectrum kx <= Xc / 2 (columns 0 < kx < Xc / 2 count twice).  The band is a thin ring: with the default
// fractions about a tenth of the bins, all of them in the first k_hi + 1 columns.  Two kernels and a reduction:
//
//   band_rows_kernel:     one row (z, y) of the window per wavefront, read straight from the uncropped volume, transformed
//                         along x in LDS (as rfft_rows.hip); only columns kx <= k_hi leave, y-contiguous: spec[z][kx][y].
//   band_columns_kernel:  one workgroup per (z, eight columns): complex transform of length Yc in LDS, then |F| on the rows
//                         inside the column's interval a <= |ky'| <= b (and their mirrors Yc - ky), times the column weight,
//                         in float64 -- one partial per workgroup.  The y-transformed spectrum is never written.
//   band_sum_kernel:      P[z] = the partials of plane z added in a fixed order (the same bits on every call; no atomics).
//
// The strict inequalities are decided ONCE, in float64 on the host (lsr_band_power_plan): the kernels and the host twin
// (host_twins.hip) take the resulting table of closed integer intervals, not float limits.
//
// The tile helpers restate those of rfft_rows.hip / phase.hip, whose kernels stay as they are.  Unnormalised, like hipFFT.
// Lengths: Xc as lsr_rfft_rows_supported; Yc 5-smooth, 2 .. 2048 (lsr_band_power_supported).

#include "fft_lds.hpp"
#include "focus.hpp"

namespace {

using namespace lsr_fft;

constexpr int kThreads = 512;
constexpr int kRows = 8;                      // x leg: y rows per workgroup (64-byte runs in the transposed layout)
constexpr int kPerRow = kThreads / kRows;     // 64 threads (one wavefront) share a sequence's butterflies
constexpr int kMaxM = 2048;                   // x leg: longest half-length
constexpr int kCols = 8;                      // y leg: columns per workgroup, one wavefront each
// y leg: longest column.  8 columns of 2049 float2 and the 2048 twiddles are 144 KB of the CU's 160 KB; the butterfly
// index arithmetic of fft_lds.hpp (stockham_pass) is exact for at most 1024 butterflies per sequence, i.e. N <= 2048.
constexpr int kMaxY = lsr::focus::kMaxY;

struct BandArgs {
  const float* in;        // the uncropped volume [Z][Y][X]
  int Z, Y, X, y0, x0;    // ... and the window's first row and column
  int Yc, Xc, M;          // window, M = Xc / 2
  int KC;                 // k_hi + 1: columns kept
  float2* spec;           // [Z][KC][Yc]
  const float2* tw_half;  // [M / 2]   exp(-2 pi i k / M)
  const float2* tw_x;     // [M + 1]   exp(-2 pi i k / Xc)
  const float2* tw_y;     // [Yc]      exp(-2 pi i k / Yc)
  const int* table;       // [KC][2]   closed interval of |ky'| per column (empty: a > b)
  Factors fx, fy;
  double* partial;        // [Z][tiles]
};

struct Tile {
  float2* buf;       // [kRows][pitch]
  float2* tw;
  int pitch;
};

__device__ __forceinline__ Tile carve(float2* smem, int n) {
  Tile t;
  t.pitch = n + 1;
  t.buf = smem;
  t.tw = smem + kRows * t.pitch;
  return t;
}

// exp(-2 pi i k / M) from the half table: w^(k + M/2) = -w^k
__device__ __forceinline__ float2 tw_m(const float2* tw, int half, int i) {
  const bool hi = i >= half;
  const float2 v = tw[hi ? i - half : i];
  return hi ? float2{-v.x, -v.y} : v;
}

// each XCD takes a contiguous run of the tile order (neighbouring y tiles share the 128-byte lines of the spectrum)
__device__ __forceinline__ int xcd_tile(int n_tiles, int block) {
  const int per = (n_tiles + 7) >> 3;
  const int t = (block & 7) * per + (block >> 3);
  return t < n_tiles ? t : -1;
}
inline unsigned xcd_grid(int64_t n_tiles) { return static_cast<unsigned>(8 * ((n_tiles + 7) / 8)); }

// x leg.  Real-to-complex post step on the columns that are kept: X[k] = E[k] + w_X^k O[k],
//   E = (Z[k] + conj(Z[M - k])) / 2,  O = -i (Z[k] - conj(Z[M - k])) / 2,  Z[M] = Z[0]
__global__ __launch_bounds__(kThreads) void band_rows_kernel(BandArgs p) {
  extern __shared__ float2 smem[];
  const int M = p.M, half = M / 2;
  const Tile t = carve(smem, M);
  const int tid = threadIdx.x;
  const int tiles_y = (p.Yc + kRows - 1) / kRows;
  const int tile = xcd_tile(p.Z * tiles_y, blockIdx.x);
  if (tile < 0) return;
  const int z = tile / tiles_y, y0 = (tile - z * tiles_y) * kRows;
  const int nrows = min(kRows, p.Yc - y0);

  for (int k = tid; k < half; k += kThreads) t.tw[k] = p.tw_half[k];
  {
    const int r = tid / kPerRow, lane = tid & (kPerRow - 1);
    float2* row = t.buf + r * t.pitch;
    if (r < nrows) {   // the window's row: 2 m + 1 < Xc, so every sample lies inside the volume
      const float* src = p.in + (static_cast<int64_t>(z) * p.Y + p.y0 + y0 + r) * p.X + p.x0;
      batched_loop<8>(lane, M, kPerRow, [src](int m) { return float2{src[2 * m], src[2 * m + 1]}; },
                      [row](int m, float2 v) { row[m] = v; });
    } else {
      for (int m = lane; m < M; m += kPerRow) row[m] = float2{0.0f, 0.0f};
    }
  }
  __syncthreads();

  const float2* twl = t.tw;
  transform<kMaxM, kPerRow>(t.buf + (tid / kPerRow) * t.pitch, M, p.fx, [twl, half](int i) { return tw_m(twl, half, i); },
                            tid & (kPerRow - 1));

  __syncthreads();            // the post step below reads rows across wavefronts
  const int r = tid & (kRows - 1), k0 = tid / kRows;
  if (r < nrows) {
    const float2* row = t.buf + r * t.pitch;
    float2* out = p.spec + static_cast<int64_t>(z) * p.KC * p.Yc + y0 + r;
    const float2* twx = p.tw_x;
    const int64_t ystride = p.Yc;
    batched_loop<8>(k0, p.KC, kThreads / kRows, [twx](int k) { return twx[k]; },
                    [row, out, M, ystride](int k, float2 w) {
                      const float2 a = row[k == M ? 0 : k], b = cconj(row[k == 0 ? 0 : M - k]);
                      const float2 e = float2{0.5f * (a.x + b.x), 0.5f * (a.y + b.y)};
                      const float2 o = mul_mi(float2{0.5f * (a.x - b.x), 0.5f * (a.y - b.y)});
                      out[static_cast<int64_t>(k) * ystride] = cadd(e, cmul(w, o));
                    });
  }
}

// y leg and the band's sum.  Wavefront c of the workgroup owns column kx0 + c: its transform needs no workgroup barrier.
__global__ __launch_bounds__(kThreads) void band_columns_kernel(BandArgs p) {
  extern __shared__ float2 smem[];
  const int N = p.Yc;
  const Tile t = carve(smem, N);
  const int tid = threadIdx.x;
  const int tiles = (p.KC + kCols - 1) / kCols;
  const int z = blockIdx.x / tiles, tile = blockIdx.x - z * tiles;
  const int kx0 = tile * kCols;
  const int c = tid / kPerRow, lane = tid & (kPerRow - 1);
  const int kx = kx0 + c;
  const bool live = kx < p.KC;
  // the column's interval, requested here: long back when the epilogue wants it; clamped so that a wrong table cannot
  // send the epilogue outside the column
  int a = 0, b = -1;
  if (live) {
    a = max(p.table[2 * kx], 0);
    b = min(p.table[2 * kx + 1], N / 2);
  }

  for (int k = tid; k < N; k += kThreads) t.tw[k] = p.tw_y[k];
  float2* col = t.buf + c * t.pitch;
  if (live) {
    const float2* src = p.spec + (static_cast<int64_t>(z) * p.KC + kx) * N;
    batched_loop<8>(lane, N, kPerRow, [src](int y) { return src[y]; }, [col](int y, float2 v) { col[y] = v; });
  }
  __syncthreads();

  double sum = 0.0;
  if (live) {   // (uniform per wavefront)
    const float2* twl = t.tw;
    transform<kMaxY, kPerRow>(col, N, p.fy, [twl](int i) { return twl[i]; }, lane);
    double acc = 0.0;
    for (int m = a + lane; m <= b; m += kPerRow) {
      const float2 v = col[m];
      acc += sqrt(static_cast<double>(v.x) * v.x + static_cast<double>(v.y) * v.y);
      if (m != 0 && 2 * m != N) {   // the mirror row ky = Yc - m
        const float2 u = col[N - m];
        acc += sqrt(static_cast<double>(u.x) * u.x + static_cast<double>(u.y) * u.y);
      }
    }
    sum = (kx == 0 || kx == p.M) ? acc : 2.0 * acc;      // M = Xc / 2: the half spectrum's two self-paired columns
  }
  // lanes of a wavefront in a fixed tree, then the eight wavefronts in order (the tile's memory is reused)
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  __syncthreads();
  double* s_sum = reinterpret_cast<double*>(smem);
  if (lane == 0) s_sum[c] = sum;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int w = 0; w < kCols; ++w) total += s_sum[w];
    p.partial[blockIdx.x] = total;
  }
}

// out[z] = the partials of plane z, in a fixed order
__global__ __launch_bounds__(64) void band_sum_kernel(const double* __restrict__ partial, int tiles, double* __restrict__ out) {
  const double* mine = partial + static_cast<int64_t>(blockIdx.x) * tiles;
  double acc = 0.0;
  for (int i = threadIdx.x; i < tiles; i += 64) acc += mine[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

size_t rows_lds_bytes(int M) { return (static_cast<size_t>(kRows) * (M + 1) + M / 2) * sizeof(float2); }
size_t columns_lds_bytes(int N) { return (static_cast<size_t>(kCols) * (N + 1) + N) * sizeof(float2); }

}  // namespace

extern "C" int lsr_band_power_supported(int64_t Yc, int64_t Xc) {
  if (!lsr::focus::lengths_ok(Yc, Xc)) return 0;
  return lsr::lds_fits(columns_lds_bytes(static_cast<int>(Yc))) && lsr::lds_fits(rows_lds_bytes(static_cast<int>(Xc / 2)));
}

extern "C" int lsr_band_power_plan(int64_t Yc, int64_t Xc, double pixel_size, double band_lo, double band_hi, int32_t* table,
                                   int64_t* k_hi, int64_t* weighted_bins) {
  LSR_REQUIRE_PTR(table);
  LSR_REQUIRE_PTR(k_hi);
  LSR_REQUIRE(Yc >= 1 && Xc >= 2 && Xc % 2 == 0 && Yc < (int64_t(1) << 20) && Xc < (int64_t(1) << 20), LSR_E_SHAPE,
              "window (%lld,%lld): Yc >= 1, Xc even and >= 2, both below 2^20", (long long)Yc, (long long)Xc);
  LSR_REQUIRE(pixel_size > 0.0 && band_lo >= 0.0 && band_hi > band_lo && std::isfinite(pixel_size) && std::isfinite(band_hi),
              LSR_E_ARG, "pixel_size must be positive and 0 <= band_lo < band_hi finite");
  lsr::focus::plan(Yc, Xc, pixel_size, band_lo, band_hi, table, k_hi, weighted_bins);
  return LSR_OK;
}

extern "C" int lsr_band_power_scratch_bytes(int64_t Z, int64_t Yc, int64_t k_hi, int64_t* spec_bytes, int64_t* partial_bytes) {
  LSR_REQUIRE_PTR(spec_bytes);
  LSR_REQUIRE_PTR(partial_bytes);
  LSR_REQUIRE(k_hi >= 0, LSR_E_ARG, "k_hi %lld must not be negative", (long long)k_hi);
  LSR_REQUIRE_VOLUME(Z, Yc, k_hi + 1);
  *spec_bytes = Z * (k_hi + 1) * Yc * static_cast<int64_t>(sizeof(float2));
  *partial_bytes = Z * lsr::ceil_div(k_hi + 1, kCols) * static_cast<int64_t>(sizeof(double));
  return LSR_OK;
}

extern "C" int lsr_band_power_f32(const float* in, int64_t Z, int64_t Y, int64_t X, int64_t y0, int64_t x0, int64_t Yc,
                                  int64_t Xc, const float* tw_half, const float* tw_x, const float* tw_y, const int32_t* table,
                                  int64_t k_hi, float* spec_scratch, double* partial, double* out_power, lsr_stream_t stream) {
  BandArgs p{};
  if (int rc = lsr::focus::check(in, Z, Y, X, y0, x0, Yc, Xc, table, k_hi, out_power)) return rc;
  LSR_REQUIRE_PTR(tw_half);
  LSR_REQUIRE_PTR(tw_x);
  LSR_REQUIRE_PTR(tw_y);
  LSR_REQUIRE_PTR(spec_scratch);
  LSR_REQUIRE_PTR(partial);
  LSR_REQUIRE(lsr_band_power_supported(Yc, Xc), LSR_E_UNSUPPORTED,
              "window (%lld,%lld): Xc a multiple of 4 whose half is 5-smooth and at most %d, Yc 5-smooth in [2, %d]",
              (long long)Yc, (long long)Xc, kMaxM, kMaxY);
  p.in = in;
  p.Z = static_cast<int>(Z); p.Y = static_cast<int>(Y); p.X = static_cast<int>(X);
  p.y0 = static_cast<int>(y0); p.x0 = static_cast<int>(x0);
  p.Yc = static_cast<int>(Yc); p.Xc = static_cast<int>(Xc); p.M = p.Xc / 2;
  p.KC = static_cast<int>(k_hi) + 1;
  p.spec = reinterpret_cast<float2*>(spec_scratch);
  p.tw_half = reinterpret_cast<const float2*>(tw_half);
  p.tw_x = reinterpret_cast<const float2*>(tw_x);
  p.tw_y = reinterpret_cast<const float2*>(tw_y);
  p.table = table;
  p.partial = partial;
  LSR_REQUIRE(factorize(p.M, &p.fx) && factorize(p.Yc, &p.fy), LSR_E_UNSUPPORTED, "window (%lld,%lld) has too many factors",
              (long long)Yc, (long long)Xc);
  const int64_t row_tiles = Z * lsr::ceil_div(Yc, kRows), col_tiles = lsr::ceil_div(k_hi + 1, kCols);
  LSR_REQUIRE(row_tiles < (int64_t(1) << 31) - 8 && Z * col_tiles < (int64_t(1) << 31), LSR_E_SHAPE,
              "grid of workgroups is too large");
  static std::atomic<uint64_t> rows_allowed{0}, cols_allowed{0};
  if (int rc = lsr::allow_dynamic_lds(reinterpret_cast<const void*>(band_rows_kernel), static_cast<int>(rows_lds_bytes(kMaxM)),
                                      rows_allowed, "lsr_band_power_f32"))
    return rc;
  if (int rc = lsr::allow_dynamic_lds(reinterpret_cast<const void*>(band_columns_kernel),
                                      static_cast<int>(columns_lds_bytes(kMaxY)), cols_allowed, "lsr_band_power_f32"))
    return rc;
  hipStream_t s = lsr::as_stream(stream);
  hipLaunchKernelGGL(band_rows_kernel, dim3(xcd_grid(row_tiles)), dim3(kThreads), rows_lds_bytes(p.M), s, p);
  hipLaunchKernelGGL(band_columns_kernel, dim3(static_cast<unsigned>(Z * col_tiles)), dim3(kThreads),
                     columns_lds_bytes(p.Yc), s, p);
  hipLaunchKernelGGL(band_sum_kernel, dim3(static_cast<unsigned>(Z)), dim3(64), 0, s, partial, static_cast<int>(col_tiles),
                     out_power);
  return lsr::launch_status("lsr_band_power_f32");
}
