// The x legs of the label-free 3-D phase reconstruction (shrimpy_amd/phase.py; reference shrimpy/preprocessing.py:419-436,
// which hands the step to waveorder): a Tikhonov inverse filter applied in the Fourier domain to the deskewed volume,
// periodically mirror-extended onto the transform grid.  The y leg is hipFFT and the z leg (transform, product with the
// filter, inverse) is lsr_spectrum_multiply_z_c64, as in the Fourier-domain Richardson-Lucy; the two kernels here are the
// row kernels of csrc/rfft_rows.hip with what this step needs around the transform:
//
//   lsr_phase_rows_forward_c64:  EVERY row (z, y) of the grid -- the padding is the mirrored volume, not zeros -- is gathered
//                                from the source through the mirror rule on z and y, extended along x by the same rule,
//                                transformed in LDS and stored transposed, spec[z][k][y]; the padded volume is never written.
//                                The rows that are the volume's own also add up to its float64 sum: one partial per
//                                workgroup, reduced in a fixed order by a second, one-workgroup launch that leaves the mean.
//   lsr_phase_rows_inverse_f32:  complex-to-real transform of the volume's rows, cropped to (Zo, Yo, Xo) and multiplied by
//                                1 / (Z Y X mean), the mean read from device memory: nothing waits for the host.
//
// The mirror rule, for an axis of n samples on a grid of g >= n points (index i): i < n is the sample itself; behind it, with
// a = i - n and b = g - 1 - i, sample n - 1 - min(a, n - 1) if a <= b, else sample min(b, n - 1) -- the volume's end mirrored
// behind it, its beginning mirrored in front of the grid's wrap-around, each clamped to the edge value where the padding is
// longer than the volume.
//
// The tile helpers (carve .. c2r_pre_step) restate those of rfft_rows.hip, whose kernels stay as they are.
// Unnormalised, like hipFFT.  Lengths: lsr_rfft_rows_supported.

#include "fft_lds.hpp"

namespace {

using namespace lsr_fft;

constexpr int kThreads = 512;
constexpr int kRows = 8;                      // y rows per workgroup: 64-byte runs in the transposed layout
constexpr int kPerRow = kThreads / kRows;     // 64 threads (one wavefront) share a row's butterflies
constexpr int kMaxM = 2048;                   // longest half-length: two workgroups per CU up to M = 1216 (78 KB each)

struct PhaseArgs {
  const float* in;        // forward: the volume [Zi][Yi][Xi]
  int Zi, Yi, Xi;         // the volume (forward: source; inverse: output)
  float2* spec;           // [Z][XC][Y] (forward: written; inverse: read)
  int Z, Y, X, M, XC;     // transform grid, M = X / 2, XC = M + 1
  const float2* tw_half;  // [M / 2]  exp(-2 pi i k / M)
  const float2* tw_x;     // [M + 1]  exp(-2 pi i k / X)
  Factors f;
  double* partial;        // forward: one sum per workgroup
  const double* mean;     // inverse: the volume's mean
  float* out;             // inverse: [Zi][Yi][Xi]
};

__device__ __forceinline__ int mirror_index(int i, int n, int g) {
  if (i < n) return i;
  const int a = i - n, b = g - 1 - i;
  return a <= b ? n - 1 - min(a, n - 1) : min(b, n - 1);
}

struct Tile {
  float2* buf;       // [kRows][pitch]
  float2* tw;        // [M / 2]
  int pitch;
};

__device__ __forceinline__ Tile carve(float2* smem, int M) {
  Tile t;
  t.pitch = M + 1;
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

// real-to-complex post step of the transformed tile, stored transposed: X[k] = E[k] + w_X^k O[k],
//   E = (Z[k] + conj(Z[M - k])) / 2,  O = -i (Z[k] - conj(Z[M - k])) / 2,  Z[M] = Z[0]
__device__ __forceinline__ void r2c_post_store(const PhaseArgs& p, const Tile& t, int z, int y0, int nrows, int tid) {
  const int M = p.M;
  const int r = tid & (kRows - 1), k0 = tid / kRows;
  if (r < nrows) {
    const float2* row = t.buf + r * t.pitch;
    float2* out = p.spec + static_cast<int64_t>(z) * p.XC * p.Y + y0 + r;
    const float2* twx = p.tw_x;
    const int64_t ystride = p.Y;
    batched_loop<8>(k0, M + 1, kThreads / kRows, [twx](int k) { return twx[k]; },
                    [row, out, M, ystride](int k, float2 w) {
                      const float2 a = row[k == M ? 0 : k], b = cconj(row[k == 0 ? 0 : M - k]);
                      const float2 e = float2{0.5f * (a.x + b.x), 0.5f * (a.y + b.y)};
                      const float2 o = mul_mi(float2{0.5f * (a.x - b.x), 0.5f * (a.y - b.y)});
                      out[static_cast<int64_t>(k) * ystride] = cadd(e, cmul(w, o));
                    });
  }
}

__global__ __launch_bounds__(kThreads) void phase_rows_forward_kernel(PhaseArgs p) {
  extern __shared__ float2 smem[];
  const int M = p.M, half = M / 2;
  const Tile t = carve(smem, M);
  const int tid = threadIdx.x;
  const int tiles_y = (p.Y + kRows - 1) / kRows;
  const int tile = xcd_tile(p.Z * tiles_y, blockIdx.x);
  if (tile < 0) return;
  const int z = tile / tiles_y, y0 = (tile - z * tiles_y) * kRows;
  const int nrows = min(kRows, p.Y - y0);

  for (int k = tid; k < half; k += kThreads) t.tw[k] = p.tw_half[k];
  // gather: row r of the tile <- source row (mirror(z), mirror(y0 + r)), columns through mirror(x); (even, odd) packed
  double sum = 0.0;
  {
    const int r = tid / kPerRow, lane = tid & (kPerRow - 1);
    float2* row = t.buf + r * t.pitch;
    if (r < nrows) {
      const int y = y0 + r;
      const float* src = p.in + (static_cast<int64_t>(mirror_index(z, p.Zi, p.Z)) * p.Yi + mirror_index(y, p.Yi, p.Y)) * p.Xi;
      const int xi = p.Xi, xg = p.X;
      const bool own = z < p.Zi && y < p.Yi;      // a row of the volume itself: its samples count towards the mean
      batched_loop<8>(lane, M, kPerRow,
                      [src, xi, xg](int m) {
                        const int x0 = 2 * m, x1 = x0 + 1;
                        return float2{src[mirror_index(x0, xi, xg)], src[mirror_index(x1, xi, xg)]};
                      },
                      [row, own, xi, &sum](int m, float2 v) {
                        row[m] = v;
                        if (own) {
                          if (2 * m < xi) sum += static_cast<double>(v.x);
                          if (2 * m + 1 < xi) sum += static_cast<double>(v.y);
                        }
                      });
    } else {
      for (int m = lane; m < M; m += kPerRow) row[m] = float2{0.0f, 0.0f};
    }
  }
  __syncthreads();

  const float2* twl = t.tw;
  transform<kMaxM, kPerRow>(t.buf + (tid / kPerRow) * t.pitch, M, p.f, [twl, half](int i) { return tw_m(twl, half, i); },
                            tid & (kPerRow - 1));

  __syncthreads();            // the post step below reads rows across wavefronts
  r2c_post_store(p, t, z, y0, nrows, tid);

  // the workgroup's share of the volume's sum: lanes of a wavefront in a fixed tree, then the eight wavefronts in order.
  // (The tile's memory is reused: static LDS beside it would cost the second workgroup of a CU.)
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  double* s_sum = reinterpret_cast<double*>(smem);
  if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) total += s_sum[w];
    p.partial[tile] = total;
  }
}

// mean[0] = (sum of the partials, in a fixed order) / count; mean[1] = the sum
__global__ __launch_bounds__(256) void phase_mean_kernel(const double* __restrict__ partial, int64_t n, double count,
                                                        double* __restrict__ mean) {
  __shared__ double s[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc += partial[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mean[0] = s[0] / count;
    mean[1] = s[0];
  }
}

// Tile of the spectrum: X[k], k = 0 .. M, of eight neighbouring y (64-byte runs); rows at or past Y are zeros.
__device__ __forceinline__ void load_spectrum_tile(const PhaseArgs& p, const Tile& t, int z, int y0, int tid) {
  const int M = p.M;
  const int r = tid & (kRows - 1), k0 = tid / kRows;
  float2* row = t.buf + r * t.pitch;
  if (y0 + r < p.Y) {
    const float2* in = p.spec + static_cast<int64_t>(z) * p.XC * p.Y + y0 + r;
    const int64_t ystride = p.Y;
    batched_loop<10>(k0, M + 1, kThreads / kRows, [in, ystride](int k) { return in[static_cast<int64_t>(k) * ystride]; },
                     [row](int k, float2 v) { row[k] = v; });
  } else {
    for (int k = k0; k <= M; k += kThreads / kRows) row[k] = float2{0.0f, 0.0f};
  }
}

// complex-to-real pre step, pairs (m, M - m) by one thread; conjugated on the way for the conj-FFT-conj inverse:
//   Zt[m] = (X[m] + conj(X[M - m])) + i conj(w_X^m) (X[m] - conj(X[M - m]))        (= 2 x the packed signal's spectrum)
__device__ __forceinline__ void c2r_pre_step(const PhaseArgs& p, const Tile& t, int tid) {
  const int M = p.M, half = M / 2;
  const int r = tid / kPerRow, lane = tid & (kPerRow - 1);
  float2* row = t.buf + r * t.pitch;
  const float2* twx = p.tw_x;
  struct Pair { float2 a, b; };
  batched_loop<5>(lane, half + 1, kPerRow, [twx, M](int m) { return Pair{twx[m], twx[M - m]}; },
                  [row, M](int m, Pair w) {
                    const int mm = M - m;                       // partner; m == 0 pairs with X[M], m == M / 2 with itself
                    const float2 xa = row[m], xb = row[mm];
                    const float2 wa = cconj(w.a), wb = cconj(w.b);
                    const float2 za = cadd(cadd(xa, cconj(xb)), mul_i(cmul(wa, csub(xa, cconj(xb)))));
                    const float2 zb = cadd(cadd(xb, cconj(xa)), mul_i(cmul(wb, csub(xb, cconj(xa)))));
                    row[m] = cconj(za);
                    if (m != 0 && mm != m) row[mm] = cconj(zb);
                  });
}

// Only the tiles that hold rows of the volume are transformed (the grid's other planes and rows are never read).
__global__ __launch_bounds__(kThreads) void phase_rows_inverse_kernel(PhaseArgs p) {
  extern __shared__ float2 smem[];
  const int M = p.M, half = M / 2;
  const Tile t = carve(smem, M);
  const int tid = threadIdx.x;
  const int ty_out = (p.Yi + kRows - 1) / kRows;
  const int tile = xcd_tile(p.Zi * ty_out, blockIdx.x);
  if (tile < 0) return;
  const int z = tile / ty_out, y0 = (tile - z * ty_out) * kRows;
  const int nrows = min(kRows, p.Yi - y0);
  // 1 / (Z Y X mean) in float64, rounded once (requested here: long back when the epilogue wants it)
  const double mean = p.mean[0];

  for (int k = tid; k < half; k += kThreads) t.tw[k] = p.tw_half[k];
  load_spectrum_tile(p, t, z, y0, tid);
  __syncthreads();
  c2r_pre_step(p, t, tid);
  __syncthreads();

  const float2* twl = t.tw;
  transform<kMaxM, kPerRow>(t.buf + (tid / kPerRow) * t.pitch, M, p.f, [twl, half](int i) { return tw_m(twl, half, i); },
                            tid & (kPerRow - 1));

  // conj(FFT(conj(Zt)))[m] = v[2m] + i v[2m + 1]: the row holds its conjugate
  const float scale = static_cast<float>(1.0 / (static_cast<double>(p.Z) * p.Y * p.X * mean));
  const int r = tid / kPerRow, lane = tid & (kPerRow - 1);
  if (r < nrows) {
    const float2* row = t.buf + r * t.pitch;
    float* out = p.out + (static_cast<int64_t>(z) * p.Yi + y0 + r) * p.Xi;
    const int xo = p.Xi;
    for (int m = lane; 2 * m < xo; m += kPerRow) {
      const float2 c = row[m];
      out[2 * m] = c.x * scale;
      if (2 * m + 1 < xo) out[2 * m + 1] = -c.y * scale;
    }
  }
}

int fill(PhaseArgs& p, int64_t Zi, int64_t Yi, int64_t Xi, int64_t Z, int64_t Y, int64_t X, const float* tw_half,
         const float* tw_x) {
  LSR_REQUIRE(Zi > 0 && Yi > 0 && Xi > 0, LSR_E_SHAPE, "volume shape (%lld,%lld,%lld) must be positive", (long long)Zi,
              (long long)Yi, (long long)Xi);
  LSR_REQUIRE_VOLUME(Zi, Yi, Xi);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(Zi <= Z && Yi <= Y && Xi <= X, LSR_E_SHAPE, "the volume (%lld,%lld,%lld) must fit the grid (%lld,%lld,%lld)",
              (long long)Zi, (long long)Yi, (long long)Xi, (long long)Z, (long long)Y, (long long)X);
  LSR_REQUIRE(lsr_rfft_rows_supported(X), LSR_E_UNSUPPORTED,
              "row length %lld: a multiple of 4 whose half is 5-smooth and at most %d", (long long)X, kMaxM);
  LSR_REQUIRE_PTR(tw_half);
  LSR_REQUIRE_PTR(tw_x);
  p.Zi = static_cast<int>(Zi); p.Yi = static_cast<int>(Yi); p.Xi = static_cast<int>(Xi);
  p.Z = static_cast<int>(Z); p.Y = static_cast<int>(Y); p.X = static_cast<int>(X);
  p.M = p.X / 2; p.XC = p.M + 1;
  p.tw_half = reinterpret_cast<const float2*>(tw_half);
  p.tw_x = reinterpret_cast<const float2*>(tw_x);
  LSR_REQUIRE(factorize(p.M, &p.f), LSR_E_UNSUPPORTED, "row length %lld has too many factors", (long long)X);
  LSR_REQUIRE(Z * lsr::ceil_div(Y, kRows) < (int64_t(1) << 31) - 8, LSR_E_SHAPE, "grid of workgroups is too large");
  return LSR_OK;
}

// the tile and the half twiddle table; at least the eight doubles the forward kernel's sum lays over it
size_t lds_bytes(int M) {
  const size_t tile = (static_cast<size_t>(kRows) * (M + 1) + M / 2) * sizeof(float2);
  const size_t reduction = (kThreads / 64) * sizeof(double);
  return tile > reduction ? tile : reduction;
}

template <typename K>
int allow_lds(K kernel, std::atomic<uint64_t>& done, const char* what) {
  return lsr::allow_dynamic_lds(reinterpret_cast<const void*>(kernel), static_cast<int>(lds_bytes(kMaxM)), done, what);
}

}  // namespace

// bytes of the `partial` buffer of lsr_phase_rows_forward_c64 on a grid of Z planes of Y rows (-1: out of range)
extern "C" int64_t lsr_phase_rows_scratch_bytes(int64_t Z, int64_t Y) {
  if (!lsr::volume_in_range(Z, Y, 1)) return -1;
  return Z * lsr::ceil_div(Y, kRows) * static_cast<int64_t>(sizeof(double));
}

extern "C" int lsr_phase_rows_forward_c64(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* spec, int64_t Z,
                                          int64_t Y, int64_t X, const float* tw_half, const float* tw_x, double* partial,
                                          double* mean, lsr_stream_t stream) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(spec);
  LSR_REQUIRE_PTR(partial);
  LSR_REQUIRE_PTR(mean);
  PhaseArgs p{};
  if (int rc = fill(p, Zi, Yi, Xi, Z, Y, X, tw_half, tw_x)) return rc;
  p.in = in;
  p.spec = reinterpret_cast<float2*>(spec);
  p.partial = partial;
  static std::atomic<uint64_t> lds_allowed{0};
  if (int rc = allow_lds(phase_rows_forward_kernel, lds_allowed, "lsr_phase_rows_forward_c64")) return rc;
  const int64_t tiles = Z * lsr::ceil_div(Y, kRows);
  hipStream_t s = lsr::as_stream(stream);
  hipLaunchKernelGGL(phase_rows_forward_kernel, dim3(xcd_grid(tiles)), dim3(kThreads), lds_bytes(p.M), s, p);
  hipLaunchKernelGGL(phase_mean_kernel, dim3(1), dim3(256), 0, s, partial, tiles,
                     static_cast<double>(Zi) * static_cast<double>(Yi) * static_cast<double>(Xi), mean);
  return lsr::launch_status("lsr_phase_rows_forward_c64");
}

extern "C" int lsr_phase_rows_inverse_f32(const float* spec, int64_t Z, int64_t Y, int64_t X, const float* tw_half,
                                          const float* tw_x, const double* mean, float* out, int64_t Zo, int64_t Yo,
                                          int64_t Xo, lsr_stream_t stream) {
  LSR_REQUIRE_PTR(spec);
  LSR_REQUIRE_PTR(mean);
  LSR_REQUIRE_PTR(out);
  PhaseArgs p{};
  if (int rc = fill(p, Zo, Yo, Xo, Z, Y, X, tw_half, tw_x)) return rc;
  p.spec = const_cast<float2*>(reinterpret_cast<const float2*>(spec));
  p.mean = mean;
  p.out = out;
  static std::atomic<uint64_t> lds_allowed{0};
  if (int rc = allow_lds(phase_rows_inverse_kernel, lds_allowed, "lsr_phase_rows_inverse_f32")) return rc;
  const unsigned blocks = xcd_grid(Zo * lsr::ceil_div(Yo, kRows));
  hipLaunchKernelGGL(phase_rows_inverse_kernel, dim3(blocks), dim3(kThreads), lds_bytes(p.M), lsr::as_stream(stream), p);
  return lsr::launch_status("lsr_phase_rows_inverse_f32");
}
