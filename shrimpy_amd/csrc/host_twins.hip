// Host twins of the hot-path entry points (no kernel in this file): the same signatures with HOST pointers,
// the same argument checks, the same arithmetic in the same order -- so the results equal the device
// kernels' bit for bit -- for the boxes where the reference itself falls back to the CPU
// (`torch.device("cuda" if torch.cuda.is_available() else "cpu")`, shrimpy/preprocessing.py:78-82; its CI has
// no GPU, shrimpy/tests/conftest.py:11-17) and for BASELINE config 1 ("deskew-only via the CPU path").
// This is product code: it does not call, link or read anything under oracle/.
//
//   lsr_deskew_f32_cpu / lsr_deskew_u16_cpu   <->  lsr_deskew_f32 / lsr_deskew_u16     (deskew.hip)
//   lsr_affine_f32_cpu                        <->  lsr_affine_f32                      (affine.hip)
//   lsr_average_slices_f32_cpu                <->  lsr_average_slices_f32              (deskew.hip)
//   lsr_correlate_sep_f32_cpu                 <->  lsr_correlate_sep_f32               (correlate.hip)
//   lsr_correlate_dense_f32_cpu               <->  lsr_correlate_dense_f32             (correlate.hip)
//   lsr_rl_dense_f32_cpu                      <->  lsr_rl_dense_f32                    (correlate.hip)
//   lsr_flatfield_pattern_f32_cpu / _u16_cpu  <->  lsr_flatfield_pattern_f32 / _u16    (flatfield.hip)
//   lsr_flatfield_apply_f32_cpu / _u16_cpu    <->  lsr_flatfield_apply_f32 / _u16      (flatfield.hip)
//   lsr_rl_accel_dots_f32_cpu / _predict_f32_cpu  <->  lsr_rl_accel_dots_f32 / _predict_f32  (rl_accel.hip)
//   lsr_box_smooth_f32_cpu, lsr_local_max_candidates_f32_cpu, lsr_psf_accumulate_f32_cpu
//                                             <->  the same names without _cpu         (peaks.hip)
//   lsr_bead_fit_f32_cpu, lsr_psf_accumulate_shifted_f32_cpu
//                                             <->  the same names without _cpu         (psf_fit.hip)
//   lsr_band_power_f32_cpu                    <->  lsr_band_power_f32                  (focus.hip)
//   lsr_downsample2_f32_cpu / _u16_cpu        <->  lsr_downsample2_f32 / _u16          (pyramid.hip)
//   lsr_stitch_f32_cpu                        <->  lsr_stitch_f32                      (stitch.hip)
//   lsr_label_f32_cpu, lsr_label_regions_f32_cpu, lsr_label_remap_i32_cpu
//                                             <->  the same names without _cpu         (label.hip)
//   lsr_edt_f32_cpu, lsr_edt_labels_i32_cpu, lsr_label_expand_i32_cpu
//                                             <->  the same names without _cpu         (edt.hip)
//   lsr_watershed_f32_cpu, lsr_watershed_saddles_f32_cpu
//                                             <->  the same names without _cpu         (watershed.hip)
//   lsr_label_overlap_i32_cpu                 <->  lsr_label_overlap_i32               (overlap.hip)
//   lsr_label_moments_i32_cpu                 <->  lsr_label_moments_i32               (moments.hip)
//   lsr_label_intensity_f32_cpu / _u16_cpu    <->  lsr_label_intensity_f32 / _u16      (intensity.hip)
//   lsr_label_coloc_f32_cpu / _u16_cpu        <->  lsr_label_coloc_f32 / _u16          (coloc.hip)
//   lsr_grey_morph_f32_cpu                    <->  lsr_grey_morph_f32                  (morphology.hip)
//   lsr_rank_filter_f32_cpu                   <->  lsr_rank_filter_f32                 (rank.hip)
//   lsr_hessian_response_f32_cpu              <->  lsr_hessian_response_f32            (hessian.hip)
//
// Arithmetic (what "the same" means):
//   resamplers -- the text the kernels compile (resample.hpp): coordinates, axis taps with their weights and the
//     8-corner sum accumulated z-major in fp64, every operation rounded on its own (the TU is built with
//     -ffp-contract=off), the result rounded to f32 once: scipy.ndimage.affine_transform(order=1);
//   averaging  -- ((d0 + d1) + ...) / n in f32, the last group edge-padded;
//   stencils   -- f32 FMA chains in tap order (separable: x, then y, then z; dense: z-major), zeros outside the
//     volume, the Richardson-Lucy epilogues of correlate.hip.
// The `stream` argument is ignored (kept so the signatures are identical).  Threads: plain std::thread over
// output planes, at most lsr_set_host_threads(n) of them (default 1) -- no OpenMP runtime enters the process
// (the reference's warning about torch plus a second OpenMP, shrimpy/tests/conftest.py:11-17).

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <type_traits>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "correlate_common.hpp"
#include "host_parallel.hpp"
#include "resample.hpp"
#include "rl_accel.hpp"

namespace {

using lsr::parallel_ranges;
std::atomic<int>& g_threads = lsr::g_host_threads;
constexpr int kMaxAvg = lsr::kMaxAvgSlices;
// the stencil kernels hold 15 taps per axis (31 along z, correlate_z.hip); larger dense PSFs run in the Fourier
// domain on the device (deconvolve_fft.py, up to 129 taps per axis) -- the twins' loops take any count
constexpr int kMaxTaps = 129;
constexpr int kMaxZTaps = 129;

// acc[x] = fma(w, v(x + shift), acc[x]) over a whole row, v = row[...] inside [0, X) and 0 outside it (row == nullptr:
// a row of zeros) -- the FMA with 0 is executed, as the kernels execute it; the middle part is a plain packed loop.
inline void row_fma(float* __restrict__ acc, float w, const float* __restrict__ row, int64_t shift, int64_t X) {
  int64_t lo = 0, hi = 0;
  if (row != nullptr) {
    lo = shift < 0 ? (-shift < X ? -shift : X) : 0;
    hi = shift > 0 ? (X - shift > lo ? X - shift : lo) : X;
    if (hi < lo) hi = lo;
  }
  for (int64_t x = 0; x < lo; ++x) acc[x] = std::fmaf(w, 0.0f, acc[x]);
  for (int64_t x = lo; x < hi; ++x) acc[x] = std::fmaf(w, row[x + shift], acc[x]);
  for (int64_t x = hi; x < X; ++x) acc[x] = std::fmaf(w, 0.0f, acc[x]);
}

using AxisTap = lsr::AxisTap<int64_t>;
using lsr::axis_tap;

inline double coord(double zo, double yo, double xo, const double* row) {
  return lsr::affine_coord(zo, yo, xo, row[0], row[1], row[2], row[3]);
}

template <typename T, bool GRID>
inline float sample(const T* in, int64_t Z, int64_t Y, int64_t X, const double M[12], double zo, double yo, double xo,
                    float cval) {
  AxisTap tz, ty, tx;
  if (!axis_tap<GRID>(coord(zo, yo, xo, M), Z, tz) || !axis_tap<GRID>(coord(zo, yo, xo, M + 4), Y, ty) ||
      !axis_tap<GRID>(coord(zo, yo, xo, M + 8), X, tx))
    return cval;
  const double cv = static_cast<double>(cval);
  double t = 0.0;
  for (int a = 0; a < 2; ++a) {
    const int64_t oz = (a ? tz.i1 : tz.i0) * Y * X;
    const double wz = a ? tz.w1 : tz.w0;
    const bool bz = a ? tz.out1 : tz.out0;
    for (int b = 0; b < 2; ++b) {
      const int64_t oy = oz + (b ? ty.i1 : ty.i0) * X;
      const double wy = b ? ty.w1 : ty.w0;
      const bool by = b ? ty.out1 : ty.out0;
      for (int c = 0; c < 2; ++c) {
        double v = static_cast<double>(in[oy + (c ? tx.i1 : tx.i0)]);
        if (GRID && (bz || by || (c ? tx.out1 : tx.out0))) v = cv;
        t = lsr::add_corner(t, v, wz, wy, c ? tx.w1 : tx.w0);
      }
    }
  }
  return static_cast<float>(t);
}

bool is_integer(double v) { return v == static_cast<double>(static_cast<int64_t>(v)); }

template <typename T>
int deskew_cpu(const T* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo, int64_t Yo, int64_t Xo,
               int64_t out_pitch, int64_t out_plane, int64_t Zd, const double M[12], int avg_n, float cval = 0.0f) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  if (int rc = lsr::check_matrix(M)) return rc;
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "raw shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(Zo > 0 && Yo > 0 && Xo > 0 && Zd > 0, LSR_E_SHAPE, "output shape (%lld,%lld,%lld) / Zd %lld must be positive",
              (long long)Zo, (long long)Yo, (long long)Xo, (long long)Zd);
  LSR_REQUIRE_VOLUME(Zo, Yo, Xo);
  LSR_REQUIRE_VOLUME(Zd, Yo, Xo);
  LSR_REQUIRE(avg_n >= 1 && avg_n <= kMaxAvg, LSR_E_ARG, "avg_n %d outside [1,%d]", avg_n, kMaxAvg);
  LSR_REQUIRE(Zo == lsr::ceil_div(Zd, avg_n), LSR_E_SHAPE, "Zo %lld != ceil(Zd %lld / avg_n %d)", (long long)Zo,
              (long long)Zd, avg_n);
  LSR_REQUIRE(out_pitch >= Xo && out_plane >= Yo * out_pitch, LSR_E_SHAPE,
              "output strides (%lld, %lld) are smaller than the output plane (%lld x %lld)", (long long)out_pitch,
              (long long)out_plane, (long long)Yo, (long long)Xo);
  const bool structured = M[1] == 0.0 && (M[4] == 1.0 || M[4] == -1.0) && M[5] == 0.0 && M[6] == 0.0 && is_integer(M[7]) &&
                          M[8] == 0.0 && (M[9] == 1.0 || M[9] == -1.0) && M[10] == 0.0 && is_integer(M[11]);
  LSR_REQUIRE(structured, LSR_E_UNSUPPORTED,
              "matrix is not a deskew shear (rows 1,2 must be signed unit axes with integer offsets, M[0][1] == 0): use "
              "lsr_affine_f32_cpu + lsr_average_slices_f32_cpu");
  // The shear's structure (deskew.hip uses the same): z_in depends on (zd, xo) only, y_in on zd only, x_in on yo only,
  // and y_in, x_in are whole numbers -- so of scipy's eight corners two carry weight (the z neighbours at (y_in, x_in))
  // and the other six add zeros.  Per deskewed plane the z taps are tabulated once along xo and reused for every yo;
  // a voxel is  float( (0.0 + double(v0) * w0) + double(v1) * w1 ), the generic resampler's own sum without its
  // zero terms (finite inputs: a zero-weight corner holding inf / NaN would poison scipy's sum and the generic twin's,
  // not the kernel's and not this one).  Then the average of avg_n planes in f32, as the kernel accumulates it.
  std::vector<int64_t> xin_v(static_cast<size_t>(Yo));
  for (int64_t yo = 0; yo < Yo; ++yo) {     // x_in(yo), or -1 where it leaves the stack
    const double c = coord(0.0, static_cast<double>(yo), 0.0, M + 8);
    xin_v[static_cast<size_t>(yo)] = (c < 0.0 || c > static_cast<double>(X - 1)) ? -1 : static_cast<int64_t>(std::floor(c));
  }
  const int64_t* const xin = xin_v.data();
  const int64_t plane = Y * X;
  std::atomic<bool> failed{false};
  parallel_ranges(Zo, [&](int64_t z_first, int64_t z_last) {
    std::vector<int64_t> o0_v(static_cast<size_t>(Xo)), o1_v(static_cast<size_t>(Xo));
    std::vector<double> w0_v(static_cast<size_t>(Xo)), w1_v(static_cast<size_t>(Xo));
    std::vector<float> d_v(static_cast<size_t>(Xo));
    int64_t* const o0 = o0_v.data();
    int64_t* const o1 = o1_v.data();
    double* const w0 = w0_v.data();
    double* const w1 = w1_v.data();
    float* const d = d_v.data();
    for (int64_t zo = z_first; zo < z_last; ++zo) {
      for (int k = 0; k < avg_n; ++k) {
        const int64_t zd = zo * avg_n + k < Zd - 1 ? zo * avg_n + k : Zd - 1;
        const double cy = coord(static_cast<double>(zd), 0.0, 0.0, M + 4);
        const bool y_ok = !(cy < 0.0 || cy > static_cast<double>(Y - 1));
        const int64_t y_in = y_ok ? static_cast<int64_t>(std::floor(cy)) : 0;
        for (int64_t xo = 0; xo < Xo; ++xo) {      // the z taps of this deskewed plane (o0 < 0: outside the stack)
          AxisTap tz;
          if (y_ok && axis_tap<false>(coord(static_cast<double>(zd), 0.0, static_cast<double>(xo), M), Z, tz)) {
            o0[xo] = tz.i0 * plane + y_in * X;
            o1[xo] = tz.i1 * plane + y_in * X;
            w0[xo] = tz.w0;
            w1[xo] = tz.w1;
          } else {
            o0[xo] = -1;
          }
        }
        for (int64_t yo = 0; yo < Yo; ++yo) {
          float* const row = out + zo * out_plane + yo * out_pitch;
          const int64_t xi = xin[yo];
          if (xi < 0) {
            for (int64_t xo = 0; xo < Xo; ++xo) d[xo] = cval;
          } else {
            const T* const col = in + xi;
            for (int64_t xo = 0; xo < Xo; ++xo) {
              if (o0[xo] < 0) {
                d[xo] = cval;
                continue;
              }
              double t = 0.0 + static_cast<double>(col[o0[xo]]) * w0[xo];
              t = t + static_cast<double>(col[o1[xo]]) * w1[xo];
              d[xo] = static_cast<float>(t);
            }
          }
          if (k == 0) {             // (avg_n == 1: the sample itself, no division)
            for (int64_t xo = 0; xo < Xo; ++xo) row[xo] = d[xo];
          } else if (k + 1 < avg_n) {
            for (int64_t xo = 0; xo < Xo; ++xo) row[xo] = row[xo] + d[xo];
          } else {
            const float n = static_cast<float>(avg_n);
            for (int64_t xo = 0; xo < Xo; ++xo) row[xo] = (row[xo] + d[xo]) / n;
          }
        }
      }
    }
  }, failed);
  if (failed.load()) return lsr::fail(LSR_E_ARG, "out of host memory for the per-thread tap tables");
  return LSR_OK;
}

int check_corr(const float* in, float* out, const float* aux, int64_t Z, int64_t Y, int64_t X, int pz, int py, int px,
               int epilogue) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(pz >= 1 && py >= 1 && px >= 1 && (pz & 1) && (py & 1) && (px & 1) && pz <= kMaxZTaps && py <= kMaxTaps &&
                  px <= kMaxTaps,
              LSR_E_UNSUPPORTED, "PSF taps (%d,%d,%d) must be odd, <= %d in plane and <= %d along z", pz, py, px, kMaxTaps,
              kMaxZTaps);
  LSR_REQUIRE(epilogue == LSR_EPI_NONE || epilogue == LSR_EPI_RATIO || epilogue == LSR_EPI_UPDATE, LSR_E_ARG,
              "unknown epilogue %d", epilogue);
  if (epilogue != LSR_EPI_NONE) LSR_REQUIRE_PTR(aux);
  LSR_REQUIRE(in != out, LSR_E_ARG, "out must not alias in");
  return LSR_OK;
}

// H^T 1 of the dense form, as correlate.hip evaluates it from the prefix-sum table
double dense_norm(const double* P, int pz, int py, int px, int64_t Z, int64_t Y, int64_t X, int64_t z, int64_t y, int64_t x) {
  const int cz = pz / 2, cy = py / 2, cx = px / 2;
  auto lo = [](int64_t v) { return static_cast<int>(v > 0 ? v : 0); };
  auto hi = [](int64_t n, int64_t v) { return static_cast<int>(v < n ? v : n); };
  const int a0 = lo(cz - z), a1 = hi(pz, Z - z + cz), b0 = lo(cy - y), b1 = hi(py, Y - y + cy), c0 = lo(cx - x),
            c1 = hi(px, X - x + cx);
  const int sb = px + 1, sa = (py + 1) * sb;
  if (a0 == 0 && a1 == pz && b0 == 0 && b1 == py && c0 == 0 && c1 == px) return P[pz * sa + py * sb + px];
  return ((P[a1 * sa + b1 * sb + c1] - P[a0 * sa + b1 * sb + c1]) - (P[a1 * sa + b0 * sb + c1] - P[a0 * sa + b0 * sb + c1])) -
         ((P[a1 * sa + b1 * sb + c0] - P[a0 * sa + b1 * sb + c0]) - (P[a1 * sa + b0 * sb + c0] - P[a0 * sa + b0 * sb + c0]));
}

}  // namespace

extern "C" int lsr_set_host_threads(int n) {
  LSR_REQUIRE(n >= 1 && n <= 1024, LSR_E_ARG, "host threads %d outside [1, 1024]", n);
  g_threads.store(n, std::memory_order_relaxed);
  return LSR_OK;
}

extern "C" int lsr_get_host_threads(void) { return g_threads.load(std::memory_order_relaxed); }

extern "C" int lsr_deskew_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo, int64_t Yo,
                                  int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd, const double M[12],
                                  int avg_n, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  return deskew_cpu(in, Z, Y, X, out, Zo, Yo, Xo, out_pitch, out_plane, Zd, M, avg_n);
}

// ... with the value outside the stack (scipy's cval; `cval` is a HOST scalar here, NULL = 0): "constant" border only
extern "C" int lsr_deskew_cval_cpu(const void* in, int in_u16, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                                   int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                                   const double M[12], int avg_n, int mode, const float* flat_pattern,
                                   const float* flat_mean, const float* cval, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  LSR_REQUIRE(mode == LSR_MODE_CONSTANT, LSR_E_UNSUPPORTED, "the host deskew twin has the \"constant\" border only");
  LSR_REQUIRE(flat_pattern == nullptr && flat_mean == nullptr, LSR_E_UNSUPPORTED, "the host deskew twin takes a corrected stack");
  const float cv = cval ? cval[0] : 0.0f;
  if (in_u16) return deskew_cpu(static_cast<const uint16_t*>(in), Z, Y, X, out, Zo, Yo, Xo, out_pitch, out_plane, Zd, M, avg_n, cv);
  return deskew_cpu(static_cast<const float*>(in), Z, Y, X, out, Zo, Yo, Xo, out_pitch, out_plane, Zd, M, avg_n, cv);
}

extern "C" int lsr_deskew_u16_cpu(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo, int64_t Yo,
                                  int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd, const double M[12],
                                  int avg_n, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  return deskew_cpu(in, Z, Y, X, out, Zo, Yo, Xo, out_pitch, out_plane, Zd, M, avg_n);
}

extern "C" int lsr_affine_f32_cpu(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* out, int64_t Zo, int64_t Yo,
                                  int64_t Xo, const double M[12], float cval, int mode, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  int rc;
  bool grid;
  if ((rc = lsr::require_buffers(in, out, M)) || (rc = lsr::check_matrix(M)) ||
      (rc = lsr::require_positive(Zi, Yi, Xi, Zo, Yo, Xo)) || (rc = lsr::require_volumes(Zi, Yi, Xi, Zo, Yo, Xo)) ||
      (rc = lsr::require_border(mode, &grid)))
    return rc;
  parallel_ranges(Zo, [&](int64_t z_first, int64_t z_last) {
    for (int64_t zo = z_first; zo < z_last; ++zo)
      for (int64_t yo = 0; yo < Yo; ++yo) {
        float* row = out + (zo * Yo + yo) * Xo;
        for (int64_t xo = 0; xo < Xo; ++xo)
          row[xo] = grid ? sample<float, true>(in, Zi, Yi, Xi, M, double(zo), double(yo), double(xo), cval)
                         : sample<float, false>(in, Zi, Yi, Xi, M, double(zo), double(yo), double(xo), cval);
      }
  });
  return LSR_OK;
}

extern "C" int lsr_average_slices_f32_cpu(const float* in, int64_t Zd, int64_t Y, int64_t X, float* out, int64_t Zo, int avg_n,
                                          lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(Zd > 0 && Y > 0 && X > 0 && Zo > 0, LSR_E_SHAPE, "shape must be positive");
  LSR_REQUIRE_VOLUME(Zd, Y, X);
  LSR_REQUIRE_VOLUME(Zo, Y, X);
  LSR_REQUIRE(avg_n >= 1 && avg_n <= kMaxAvg, LSR_E_ARG, "avg_n %d outside [1,%d]", avg_n, kMaxAvg);
  LSR_REQUIRE(Zo == lsr::ceil_div(Zd, avg_n), LSR_E_SHAPE, "Zo %lld != ceil(Zd %lld / avg_n %d)", (long long)Zo,
              (long long)Zd, avg_n);
  const int64_t plane = Y * X;
  parallel_ranges(Zo, [&](int64_t z_first, int64_t z_last) {
    for (int64_t zo = z_first; zo < z_last; ++zo)
      for (int64_t r = 0; r < plane; ++r) {
        float acc = 0.0f;
        for (int k = 0; k < avg_n; ++k) {
          const int64_t zd = zo * avg_n + k < Zd - 1 ? zo * avg_n + k : Zd - 1;
          const float d = in[zd * plane + r];
          acc = k == 0 ? d : acc + d;
        }
        out[zo * plane + r] = avg_n > 1 ? acc / static_cast<float>(avg_n) : acc;
      }
  });
  return LSR_OK;
}

// The reduction scalars of an UPDATE pass (correlate_common.hpp: flux, change, total), as the kernels add them: a
// range's rows in f64 here, one locked add per range.
namespace {
struct HostStats {
  double flux = 0.0, change = 0.0, total = 0.0;
  void add(float x_old, float xu, float x_new) {
    flux += xu;
    change += std::fabs(static_cast<double>(x_new) - static_cast<double>(x_old));
    total += x_new;
  }
  void flush(double* dst, std::mutex& m) const {
    std::lock_guard<std::mutex> g(m);
    dst[0] += flux; dst[1] += change; dst[2] += total;
  }
};
}  // namespace

extern "C" int lsr_correlate_sep_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y, int64_t X,
                                         const float* wz, int pz, const float* wy, int py, const float* wx, int px,
                                         int epilogue, float eps, const float* nz, const float* ny, const float* nx,
                                         lsr_stream_t stream) {
  return lsr_correlate_sep_stats_f32_cpu(in, out, aux, Z, Y, X, wz, pz, wy, py, wx, px, epilogue, eps, nz, ny, nx, nullptr,
                                         stream);
}

extern "C" int lsr_correlate_sep_stats_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y, int64_t X,
                                               const float* wz, int pz, const float* wy, int py, const float* wx, int px,
                                               int epilogue, float eps, const float* nz, const float* ny, const float* nx,
                                               double* stats, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  if (int rc = check_corr(in, out, aux, Z, Y, X, pz, py, px, epilogue)) return rc;
  LSR_REQUIRE_PTR(wz);
  LSR_REQUIRE_PTR(wy);
  LSR_REQUIRE_PTR(wx);
  if (epilogue == LSR_EPI_UPDATE) {
    LSR_REQUIRE_PTR(nz);
    LSR_REQUIRE_PTR(ny);
    LSR_REQUIRE_PTR(nx);
  }
  const int64_t plane = Y * X;
  const int cz = pz / 2, cy = py / 2, cx = px / 2;
  // in-plane passes of every plane first (x then y, f32 FMA chains from 0), then the z chain + epilogue.
  // Every voxel sees exactly the kernels' operations in the kernels' order -- a tap that falls outside the volume is
  // an FMA with 0, not a skipped step -- but the loops run taps outermost and x innermost over whole rows, so that
  // the compiler turns each into packed FMAs (the per-voxel tap loop was a serial dependency chain: 4x slower than
  // scipy's correlate1d on one core; this form is faster than it).
  std::atomic<bool> failed{false};
  std::vector<float> filtered;
  try {
    filtered.resize(static_cast<size_t>(Z * plane));
  } catch (const std::bad_alloc&) {
    return lsr::fail(LSR_E_ARG, "out of host memory for a %lld-voxel intermediate", (long long)(Z * plane));
  }
  parallel_ranges(Z, [&](int64_t z_first, int64_t z_last) {
    std::vector<float> rows_v(static_cast<size_t>(plane));
    float* const rows = rows_v.data();
    for (int64_t z = z_first; z < z_last; ++z) {
      const float* const src = in + z * plane;
      for (int64_t y = 0; y < Y; ++y) {
        const float* __restrict__ srow = src + y * X;
        float* __restrict__ acc = rows + y * X;
        for (int64_t x = 0; x < X; ++x) acc[x] = 0.0f;
        for (int c = 0; c < px; ++c) row_fma(acc, wx[c], srow, c - cx, X);
      }
      float* const dst = filtered.data() + z * plane;
      for (int64_t y = 0; y < Y; ++y) {
        float* __restrict__ acc = dst + y * X;
        for (int64_t x = 0; x < X; ++x) acc[x] = 0.0f;
        for (int b = 0; b < py; ++b) {
          const float w = wy[b];
          const int64_t gy = y + b - cy;
          if (gy >= 0 && gy < Y) {
            const float* __restrict__ r = rows + gy * X;
            for (int64_t x = 0; x < X; ++x) acc[x] = std::fmaf(w, r[x], acc[x]);
          } else {
            for (int64_t x = 0; x < X; ++x) acc[x] = std::fmaf(w, 0.0f, acc[x]);
          }
        }
      }
    }
  }, failed);
  if (failed.load()) return lsr::fail(LSR_E_ARG, "out of host memory for the per-thread row buffers");
  std::mutex stats_lock;
  parallel_ranges(Z * Y, [&](int64_t r_first, int64_t r_last) {
    std::vector<float> c_v(static_cast<size_t>(X));
    float* __restrict__ c = c_v.data();
    HostStats st;
    for (int64_t zy = r_first; zy < r_last; ++zy) {
      const int64_t z = zy / Y, y = zy - z * Y;
      // the march of correlate.hip: the first plane's term is a plain product, the others FMAs onto it
      for (int a = 0; a < pz; ++a) {
        const int64_t zi = z + a - cz;
        const float w = wz[a];
        const bool inside = zi >= 0 && zi < Z;
        const float* __restrict__ p = filtered.data() + (inside ? zi : 0) * plane + y * X;
        if (a == 0) {
          if (inside) for (int64_t x = 0; x < X; ++x) c[x] = w * p[x];
          else for (int64_t x = 0; x < X; ++x) c[x] = w * 0.0f;
        } else if (inside) {
          for (int64_t x = 0; x < X; ++x) c[x] = std::fmaf(w, p[x], c[x]);
        } else {
          for (int64_t x = 0; x < X; ++x) c[x] = std::fmaf(w, 0.0f, c[x]);
        }
      }
      const int64_t o = zy * X;
      float* __restrict__ dst = out + o;
      if (epilogue == LSR_EPI_RATIO) {
        const float* __restrict__ ax = aux + o;
        for (int64_t x = 0; x < X; ++x) dst[x] = ax[x] / (c[x] + eps);
      } else if (epilogue == LSR_EPI_UPDATE) {
        const float* __restrict__ ax = aux + o;
        const float nzy = nz[z] * ny[y];
        if (stats == nullptr) {
          for (int64_t x = 0; x < X; ++x) dst[x] = ax[x] * c[x] / (nzy * nx[x]);
        } else {   // (dst may be aux itself: read, then write)
          for (int64_t x = 0; x < X; ++x) {
            const float a = ax[x], ac = a * c[x], v = ac / (nzy * nx[x]);
            dst[x] = v;
            st.add(a, ac, v);
          }
        }
      } else {
        for (int64_t x = 0; x < X; ++x) dst[x] = c[x];
      }
    }
    if (stats != nullptr && epilogue == LSR_EPI_UPDATE) st.flush(stats, stats_lock);
  }, failed);
  if (failed.load()) return lsr::fail(LSR_E_ARG, "out of host memory for the per-thread row buffers");
  return LSR_OK;
}

extern "C" int lsr_correlate_dense_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y, int64_t X,
                                           const float* w, int pz, int py, int px, int epilogue, float eps,
                                           const double* norm_table, lsr_stream_t stream) {
  return lsr_correlate_dense_stats_f32_cpu(in, out, aux, Z, Y, X, w, pz, py, px, epilogue, eps, norm_table, nullptr, stream);
}

extern "C" int lsr_correlate_dense_stats_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                                                 int64_t X, const float* w, int pz, int py, int px, int epilogue, float eps,
                                                 const double* norm_table, double* stats, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  if (int rc = check_corr(in, out, aux, Z, Y, X, pz, py, px, epilogue)) return rc;
  LSR_REQUIRE_PTR(w);
  if (epilogue == LSR_EPI_UPDATE) LSR_REQUIRE_PTR(norm_table);
  const int64_t plane = Y * X;
  const int cz = pz / 2, cy = py / 2, cx = px / 2;
  // per output row: taps outermost (planes in z order, within a plane y-major, then x: the order the march accumulates
  // in), x innermost -- every voxel's chain is the same sequence of FMAs, a row at a time (packed FMAs on the host)
  std::atomic<bool> failed{false};
  std::mutex stats_lock;
  parallel_ranges(Z * Y, [&](int64_t r_first, int64_t r_last) {
    std::vector<float> c_v(static_cast<size_t>(X));
    float* __restrict__ c = c_v.data();
    HostStats st;
    for (int64_t zy = r_first; zy < r_last; ++zy) {
      const int64_t z = zy / Y, y = zy - z * Y;
      for (int64_t x = 0; x < X; ++x) c[x] = 0.0f;
      for (int a = 0; a < pz; ++a) {
        const int64_t zi = z + a - cz;
        if (zi < 0 || zi >= Z) continue;      // (a whole plane of zeros leaves the chain unchanged)
        for (int b = 0; b < py; ++b) {
          const int64_t gy = y + b - cy;
          const float* row = gy >= 0 && gy < Y ? in + zi * plane + gy * X : nullptr;
          for (int k = 0; k < px; ++k) row_fma(c, w[(a * py + b) * px + k], row, k - cx, X);
        }
      }
      const int64_t o = zy * X;
      float* __restrict__ dst = out + o;
      if (epilogue == LSR_EPI_RATIO) {
        for (int64_t x = 0; x < X; ++x) dst[x] = aux[o + x] / (c[x] + eps);
      } else if (epilogue == LSR_EPI_UPDATE) {
        for (int64_t x = 0; x < X; ++x) {
          const float a = aux[o + x], ac = a * c[x];
          const float v = ac / static_cast<float>(dense_norm(norm_table, pz, py, px, Z, Y, X, z, y, x));
          dst[x] = v;
          if (stats != nullptr) st.add(a, ac, v);
        }
      } else {
        for (int64_t x = 0; x < X; ++x) dst[x] = c[x];
      }
    }
    if (stats != nullptr && epilogue == LSR_EPI_UPDATE) st.flush(stats, stats_lock);
  }, failed);
  if (failed.load()) return lsr::fail(LSR_E_ARG, "out of host memory for the per-thread row buffers");
  return LSR_OK;
}

// The whole loop of lsr_rl_dense_f32 on host memory: `iters` x { ratio = y / (H x + eps); x <- x * H^T ratio / H^T 1 },
// x updated in place, `ratio` scratch.
extern "C" int lsr_rl_dense_f32_cpu(const float* y, float* x, float* ratio, int64_t Z, int64_t Y, int64_t X, const float* psf,
                                    const float* psf_flipped, int pz, int py, int px, const double* norm_table, int iters,
                                    float eps, lsr_stream_t stream) {
  return lsr_rl_dense_stats_f32_cpu(y, x, ratio, Z, Y, X, psf, psf_flipped, pz, py, px, norm_table, iters, eps, nullptr, stream);
}

extern "C" int lsr_rl_dense_stats_f32_cpu(const float* y, float* x, float* ratio, int64_t Z, int64_t Y, int64_t X,
                                          const float* psf, const float* psf_flipped, int pz, int py, int px,
                                          const double* norm_table, int iters, float eps, double* stats,
                                          lsr_stream_t stream) {
  LSR_REQUIRE_HOST_FMA();
  LSR_REQUIRE_PTR(y);
  LSR_REQUIRE_PTR(x);
  LSR_REQUIRE_PTR(ratio);
  LSR_REQUIRE(iters >= 0, LSR_E_ARG, "iters %d must be >= 0", iters);
  LSR_REQUIRE(ratio != x && ratio != y && x != y, LSR_E_ARG, "y, x and ratio must be distinct");
  if (stats != nullptr)
    for (int i = 0; i < lsr::kRlStats * iters; ++i) stats[i] = 0.0;
  for (int it = 0; it < iters; ++it) {
    int rc = lsr_correlate_dense_f32_cpu(x, ratio, y, Z, Y, X, psf_flipped, pz, py, px, LSR_EPI_RATIO, eps, nullptr, stream);
    if (rc) return rc;
    rc = lsr_correlate_dense_stats_f32_cpu(ratio, x, x, Z, Y, X, psf, pz, py, px, LSR_EPI_UPDATE, eps, norm_table,
                                           stats ? stats + lsr::kRlStats * it : nullptr, stream);
    if (rc) return rc;
  }
  return LSR_OK;
}

// ---- bright-field flat-field (shrimpy/preprocessing.py:385-404): pattern = volume.quantile(0.5, dim=0), its
// mean, out = in / pattern * mean.  The median as flatfield.hip forms it: the two middle order statistics a <= b under
// the order of the keys (-0.0 below +0.0), torch's lerp fma(-(b - a), 0.5, b) -- one explicit fused multiply-add -- for an
// even count, a for an odd one, the canonical NaN if the column holds one; the mean in f64.

namespace {

template <typename T>
int flat_pattern_cpu(const T* in, int64_t Z, int64_t Y, int64_t X, float* pattern, float* mean_out) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(pattern);
  LSR_REQUIRE_PTR(mean_out);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(Z < 65536, LSR_E_UNSUPPORTED, "Z = %lld: the median kernel counts in 16 bits", (long long)Z);
  const int64_t plane = Y * X;
  std::atomic<bool> failed{false};
  parallel_ranges(plane, [&](int64_t first, int64_t last) {
    // the column as keys (the order-preserving unsigned image of a float, as flatfield.hip): selecting by the keys tells
    // -0.0 from +0.0, which operator< on floats does not
    auto key_of = [](float v) {
      uint32_t u;
      std::memcpy(&u, &v, sizeof u);
      return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    };
    auto value_of = [](uint32_t k) {
      const uint32_t u = k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu);
      float v;
      std::memcpy(&v, &u, sizeof v);
      return v;
    };
    std::vector<uint32_t> col(static_cast<size_t>(Z));
    for (int64_t i = first; i < last; ++i) {
      bool nan = false;
      for (int64_t z = 0; z < Z; ++z) {
        const float v = static_cast<float>(in[z * plane + i]);
        col[static_cast<size_t>(z)] = key_of(v);
        nan |= v != v;
      }
      if (nan) {
        pattern[i] = value_of(0xffc00000u);  // the key of the canonical quiet NaN, bits 0x7fc00000, as the kernel writes it
        continue;
      }
      const int64_t hi = Z / 2;
      std::nth_element(col.begin(), col.begin() + hi, col.end());
      const float b = value_of(col[static_cast<size_t>(hi)]);
      if (Z & 1) {
        pattern[i] = b;
      } else {
        const float a = value_of(*std::max_element(col.begin(), col.begin() + hi));
        pattern[i] = std::fmaf(-(b - a), 0.5f, b);
      }
    }
  }, failed);
  if (failed.load()) return lsr::fail(LSR_E_ARG, "out of host memory for the per-thread column buffers");
  double sum = 0.0;
  for (int64_t i = 0; i < plane; ++i) sum += static_cast<double>(pattern[i]);
  mean_out[0] = static_cast<float>(sum / static_cast<double>(plane));
  return LSR_OK;
}

template <typename T>
int flat_apply_cpu(const T* in, const float* pattern, const float* mean, float* out, int64_t Z, int64_t Y, int64_t X) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(pattern);
  LSR_REQUIRE_PTR(mean);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  const int64_t plane = Y * X;
  const float m = mean[0];
  parallel_ranges(Z, [&](int64_t z_first, int64_t z_last) {
    for (int64_t z = z_first; z < z_last; ++z)
      for (int64_t i = 0; i < plane; ++i) out[z * plane + i] = static_cast<float>(in[z * plane + i]) / pattern[i] * m;
  });
  return LSR_OK;
}

}  // namespace

extern "C" int lsr_flatfield_pattern_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float* pattern, float* mean_out,
                                             void*, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  return flat_pattern_cpu(in, Z, Y, X, pattern, mean_out);
}
extern "C" int lsr_flatfield_pattern_u16_cpu(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, float* pattern,
                                             float* mean_out, void*, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  return flat_pattern_cpu(in, Z, Y, X, pattern, mean_out);
}
extern "C" int lsr_flatfield_apply_f32_cpu(const float* in, const float* pattern, const float* mean_dev, float* out, int64_t Z,
                                           int64_t Y, int64_t X, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  return flat_apply_cpu(in, pattern, mean_dev, out, Z, Y, X);
}
extern "C" int lsr_flatfield_apply_u16_cpu(const uint16_t* in, const float* pattern, const float* mean_dev, float* out,
                                           int64_t Z, int64_t Y, int64_t X, lsr_stream_t) {
  LSR_REQUIRE_HOST_FMA();
  return flat_apply_cpu(in, pattern, mean_dev, out, Z, Y, X);
}

// ---- accelerated Richardson-Lucy (rl_accel.hip): the same inline functions, so g and p are the kernels' bits.  The inner
// products are float64 from the first add, summed over fixed chunks of rows (their number depends on the shape alone,
// rl_accel.hpp: parts_of) and the chunks added in index order: the same bits at every lsr_set_host_threads value.
// `workspace` is unused (may be NULL); dots2, num, den and alpha_out are HOST memory.
extern "C" int lsr_rl_accel_dots_f32_cpu(const float* x1, int64_t x1_pitch, int64_t x1_plane, const float* p, int64_t p_pitch,
                                         int64_t p_plane, float* g, int64_t Z, int64_t Y, int64_t X, int first, double* dots2,
                                         void*) {
  namespace ac = lsr::accel;
  LSR_REQUIRE_HOST_FMA();
  if (int rc = ac::check_dots(ac::Vol{x1, x1_pitch, x1_plane}, ac::Vol{p, p_pitch, p_plane}, g, dots2, Z, Y, X)) return rc;
  const int64_t rows = Z * Y, parts = ac::parts_of(rows), per = lsr::ceil_div(rows, parts);
  double part[2 * ac::kMaxParts];
  parallel_ranges(parts, [&](int64_t c_first, int64_t c_last) {
    for (int64_t c = c_first; c < c_last; ++c) {
      double s_gh = 0.0, s_gg = 0.0;
      const int64_t r_last = (c + 1) * per < rows ? (c + 1) * per : rows;
      for (int64_t r = c * per; r < r_last; ++r) {
        const int64_t z = r / Y, y = r - z * Y;
        const float* a = x1 + z * x1_plane + y * x1_pitch;
        const float* b = p + z * p_plane + y * p_pitch;
        float* gr = g + r * X;
        for (int64_t x = 0; x < X; ++x) {
          const float gk = ac::change_of(a[x], b[x]);
          if (!first) s_gh += static_cast<double>(gk) * static_cast<double>(gr[x]);
          s_gg += static_cast<double>(gk) * static_cast<double>(gk);
          gr[x] = gk;
        }
      }
      part[2 * c] = s_gh;
      part[2 * c + 1] = s_gg;
    }
  });
  double s_gh = 0.0, s_gg = 0.0;
  for (int64_t c = 0; c < parts; ++c) {
    s_gh += part[2 * c];
    s_gg += part[2 * c + 1];
  }
  dots2[0] = s_gh;
  dots2[1] = s_gg;
  return LSR_OK;
}

extern "C" int lsr_rl_accel_predict_f32_cpu(const float* x1, int64_t x1_pitch, int64_t x1_plane, float* x0, int64_t x0_pitch,
                                            int64_t x0_plane, int64_t Z, int64_t Y, int64_t X, const double* num,
                                            const double* den, double* alpha_out) {
  namespace ac = lsr::accel;
  LSR_REQUIRE_HOST_FMA();
  if (int rc = ac::check_predict(ac::Vol{x1, x1_pitch, x1_plane}, ac::Vol{x0, x0_pitch, x0_plane}, Z, Y, X)) return rc;
  LSR_REQUIRE(den == nullptr || num != nullptr, LSR_E_NULL, "num is NULL although den is not (den == NULL: the first step)");
  const bool first = den == nullptr;
  const float alpha = first ? 0.0f : ac::step_length(*num, *den);
  if (alpha_out != nullptr) *alpha_out = static_cast<double>(alpha);
  parallel_ranges(Z * Y, [&](int64_t r_first, int64_t r_last) {
    for (int64_t r = r_first; r < r_last; ++r) {
      const int64_t z = r / Y, y = r - z * Y;
      const float* a = x1 + z * x1_plane + y * x1_pitch;
      float* b = x0 + z * x0_plane + y * x0_pitch;
      if (first) for (int64_t x = 0; x < X; ++x) b[x] = ac::predict_first(a[x]);
      else for (int64_t x = 0; x < X; ++x) b[x] = ac::predict_of(alpha, a[x], b[x]);
    }
  });
  return LSR_OK;
}

// ---- bead detection and PSF averaging (peaks.hip): the same rule, the same sums in the same order ----
#include "morphology.hpp"
#include "peaks.hpp"

namespace {

// One pass of the morphology's walk (morphology.hpp) over the workers: tiles of kColumns lines per step, a strip per worker
// range, sink_of(rank) the range's sink.  Returns the number of ranges.  The grey morphology's twin below runs its passes here
// as well.
template <typename SinkOf>
int walk_pass(const float* src, const lsr::morph::Lines& lines, int r, bool least, std::atomic<bool>& failed, SinkOf&& sink_of) {
  namespace mo = lsr::morph;
  const int64_t tiles_per_slab = lsr::ceil_div(lines.columns, mo::kColumns);
  return lsr::parallel_ranges_indexed(lines.outer * tiles_per_slab, [&](int rank, int64_t first, int64_t last) {
    std::vector<uint32_t> strip(static_cast<size_t>(2 * r + 1) * mo::kColumns);
    const auto sink = sink_of(rank);
    for (int64_t tile = first; tile < last; ++tile) {
      const int64_t slab = tile / tiles_per_slab, c0 = (tile - slab * tiles_per_slab) * mo::kColumns;
      const int lanes = static_cast<int>(std::min<int64_t>(mo::kColumns, lines.columns - c0));
      mo::walk_host(src, slab * lines.ostep + c0 * lines.cstep, lanes, lines.cstep, lines.L, lines.step, r, least, strip.data(),
                    sink);
    }
  }, failed);
}

struct Candidate {
  long long index;
  float value;
};

// the sink of the twin's z walk: the test, and the append to the worker's own list
struct PeakSink {
  const lsr::peaks::PeakTest* test;
  std::vector<Candidate>* mine;
  bool operator()(int64_t lin, float m) const { return test->maximum(lin, m); }
  void late(int64_t lin) const {
    if (test->first(lin)) mine->push_back(Candidate{static_cast<long long>(lin), test->s[lin]});
  }
};

}  // namespace

extern "C" int lsr_box_smooth_f32_cpu(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int taps, float tap,
                                      void* /* scratch: unused */, lsr_stream_t) {
  if (int rc = lsr::peaks::check_box_smooth(in, out, Z, Y, X, taps, tap)) return rc;
  const int64_t n = Z * Y * X;
  std::vector<double> a, b;
  try {
    a.resize(static_cast<size_t>(n));
    b.resize(static_cast<size_t>(n));
  } catch (const std::bad_alloc&) {
    return lsr::fail(LSR_E_ARG, "lsr_box_smooth_f32_cpu: out of memory for two float64 volumes of %lld voxels", (long long)n);
  }
  const double t = static_cast<double>(tap);
  const int r = taps / 2;
  auto pass = [&](auto* src, auto* dst, int64_t L, int64_t inner) {
    using TOut = std::remove_reference_t<decltype(*dst)>;
    parallel_ranges(n, [&](int64_t first, int64_t last) {
      for (int64_t e = first; e < last; ++e) {
        const int64_t i = (e / inner) % L;
        const auto* line = src + (e - i * inner);
        double acc = 0.0;
        for (int k = 0; k < taps; ++k) acc += t * static_cast<double>(line[lsr::peaks::mirror(i - r + k, L) * inner]);
        dst[e] = static_cast<TOut>(acc);
      }
    });
  };
  pass(in, a.data(), X, int64_t(1));
  pass(a.data(), b.data(), Y, X);
  pass(b.data(), out, Z, Y * X);
  return LSR_OK;
}

extern "C" int lsr_local_max_candidates_f32_cpu(const float* s, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx,
                                                float threshold, long long* cand_index, float* cand_value,
                                                int64_t capacity, unsigned long long* count, void* /* scratch: unused */,
                                                lsr_stream_t) {
  if (int rc = lsr::peaks::check_local_max(s, Z, Y, X, rz, ry, rx, threshold, cand_index, cand_value, capacity, count))
    return rc;
  namespace mo = lsr::morph;
  const int64_t n = Z * Y * X;
  std::atomic<bool> failed{false};
  std::vector<float> va, vb;                     // A = s dilated along x, B = A dilated along y; an axis without a window: no pass
  try {
    if (rx > 0) va.resize(static_cast<size_t>(n));
    if (ry > 0) vb.resize(static_cast<size_t>(n));
  } catch (const std::bad_alloc&) {
    return lsr::fail(LSR_E_ARG, "lsr_local_max_candidates_f32_cpu: out of memory for two volumes of %lld voxels", (long long)n);
  }
  const float* a = rx > 0 ? va.data() : s;
  const float* b = ry > 0 ? vb.data() : a;
  const mo::StoreSink to_a{va.data(), nullptr, mo::kPlain}, to_b{vb.data(), nullptr, mo::kPlain};
  if (rx > 0) walk_pass(s, mo::lines_of(2, Z, Y, X), rx, false, failed, [&](int) { return to_a; });
  if (ry > 0) walk_pass(a, mo::lines_of(1, Z, Y, X), ry, false, failed, [&](int) { return to_b; });
  // the z walk carries the test (at rz == 0 too: w = 1, every voxel of B its own maximum); M is never stored
  const lsr::peaks::PeakTest test{s, a, b, X, Y * X, rz, ry, rx, threshold};
  std::vector<std::vector<Candidate>> found(1024);
  const int used = walk_pass(b, mo::lines_of(0, Z, Y, X), rz, false, failed, [&](int rank) { return PeakSink{&test, &found[rank]}; });
  LSR_REQUIRE(!failed.load(), LSR_E_ARG, "lsr_local_max_candidates_f32_cpu: out of memory in a worker");
  unsigned long long total = 0;
  for (int k = 0; k < used; ++k)
    for (const Candidate& c : found[k]) {
      if (total < static_cast<unsigned long long>(capacity)) {
        cand_index[total] = c.index;
        cand_value[total] = c.value;
      }
      ++total;
    }
  *count = total;
  return LSR_OK;
}

extern "C" int lsr_psf_accumulate_f32_cpu(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                                          int64_t n_beads, int pz, int py, int px, double* bead_stats, float* psf,
                                          lsr_stream_t) {
  namespace pk = lsr::peaks;
  if (int rc = pk::check_psf_accumulate(vol, Z, Y, X, centres, n_beads, pz, py, px, bead_stats, psf)) return rc;
  const int n = pz * py * px;
  constexpr int kTree = pk::kTreeThreads;
  // the kernel's tree: partial sum t takes elements t, t + 256, ... in order, then red[t] += red[t + w], w = 128 .. 1
  auto tree = [](double* red) {
    for (int w = kTree / 2; w > 0; w >>= 1)
      for (int t = 0; t < w; ++t) red[t] += red[t + w];
    return red[0];
  };
  parallel_ranges(n_beads, [&](int64_t first, int64_t last) {
    double red[kTree];
    for (int64_t b = first; b < last; ++b) {
      int64_t z0 = 0, y0 = 0, x0 = 0;
      if (!pk::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0)) {
        bead_stats[2 * b] = bead_stats[2 * b + 1] = 0.0;
        continue;
      }
      const float* corner = vol + (z0 * Y + y0) * X + x0;
      auto at = [&](int e) {
        const int iz = e / (py * px), rem = e - iz * (py * px), iy = rem / px, ix = rem - iy * px;
        return corner[(iz * Y + iy) * X + ix];
      };
      for (int t = 0; t < kTree; ++t) {
        double acc = 0.0;
        for (int e = t; e < n; e += kTree) {
          const int iz = e / (py * px), rem = e - iz * (py * px), iy = rem / px, ix = rem - iy * px;
          if (pk::on_shell(iz, iy, ix, pz, py, px)) acc += static_cast<double>(at(e));
        }
        red[t] = acc;
      }
      const double bg = tree(red) / static_cast<double>(pk::shell_count(pz, py, px));
      for (int t = 0; t < kTree; ++t) {
        double acc = 0.0;
        for (int e = t; e < n; e += kTree) acc += static_cast<double>(at(e)) - bg;
        red[t] = acc;
      }
      bead_stats[2 * b] = bg;
      bead_stats[2 * b + 1] = tree(red);
    }
  });
  parallel_ranges(n, [&](int64_t first, int64_t last) {
    for (int64_t e = first; e < last; ++e) {
      const int64_t iz = e / (py * px), rem = e - iz * (py * px), iy = rem / px, ix = rem - iy * px;
      double acc = 0.0;
      int used = 0;
      for (int64_t b = 0; b < n_beads; ++b) {
        const double bg = bead_stats[2 * b], total = bead_stats[2 * b + 1];
        int64_t z0 = 0, y0 = 0, x0 = 0;
        if (!(total > 0.0) || !pk::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0)) continue;
        acc += (static_cast<double>(vol[((z0 + iz) * Y + y0 + iy) * X + x0 + ix]) - bg) / total;
        ++used;
      }
      psf[e] = used > 0 ? static_cast<float>(acc / static_cast<double>(used)) : 0.0f;
    }
  });
  return LSR_OK;
}

// ---- per-bead Gaussian fits and the Fourier-shifted average (psf_fit.hip): the steps of psf_fit.hpp ----
#include "psf_fit.hpp"

namespace {

// B of one bead as bead_stats_kernel sums it: 256 strided partial sums, then the binary tree
double face_mean(const float* corner, int64_t Y, int64_t X, int pz, int py, int px) {
  namespace pk = lsr::peaks;
  constexpr int kTree = pk::kTreeThreads;
  const int n = pz * py * px;
  double red[kTree];
  for (int t = 0; t < kTree; ++t) {
    double acc = 0.0;
    for (int e = t; e < n; e += kTree) {
      const int iz = e / (py * px), rem = e - iz * (py * px), iy = rem / px, ix = rem - iy * px;
      if (pk::on_shell(iz, iy, ix, pz, py, px)) acc += static_cast<double>(corner[(iz * Y + iy) * X + ix]);
    }
    red[t] = acc;
  }
  for (int w = kTree / 2; w > 0; w >>= 1)
    for (int t = 0; t < w; ++t) red[t] += red[t + w];
  return red[0] / static_cast<double>(pk::shell_count(pz, py, px));
}

}  // namespace

// The kernel's iteration with the sums taken voxel by voxel in C order: equal to the kernel's to rounding, not to the bit.
extern "C" int lsr_bead_fit_f32_cpu(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                                    int64_t n_beads, int pz, int py, int px, int max_iter, double* fit, int* status,
                                    lsr_stream_t) {
  namespace pf = lsr::psffit;
  namespace pk = lsr::peaks;
  if (int rc = pf::check_bead_fit(vol, Z, Y, X, centres, n_beads, pz, py, px, max_iter, fit, status)) return rc;
  const int n = pz * py * px, plane = py * px, hz = pz / 2, hy = py / 2, hx = px / 2;
  parallel_ranges(n_beads, [&](int64_t first, int64_t last) {
    pf::Lm lm;
    for (int64_t b = first; b < last; ++b) {
      double* out = fit + pf::kFitOut * b;
      int64_t z0 = 0, y0 = 0, x0 = 0;
      bool ok = pk::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0);
      const float* corner = ok ? vol + (z0 * Y + y0) * X + x0 : nullptr;
      auto at = [&](int e, int& iz, int& iy, int& ix) {
        iz = e / plane;
        const int rem = e - iz * plane;
        iy = rem / px;
        ix = rem - iy * px;
        return corner[(iz * Y + iy) * X + ix];
      };
      int iz, iy, ix;
      for (int e = 0; ok && e < n; ++e) ok = std::isfinite(at(e, iz, iy, ix));
      if (!ok) {
        for (int k = 0; k < pf::kFitOut; ++k) out[k] = std::numeric_limits<double>::quiet_NaN();
        status[b] = pf::kBadInput;
        continue;
      }
      const double bg = face_mean(corner, Y, X, pz, py, px);
      const double centre = static_cast<double>(corner[(hz * Y + hy) * X + hx]), cut = bg + 0.5 * (centre - bg);
      double s[pf::kSums] = {};
      for (int e = 0; e < n; ++e) {
        const double g = static_cast<double>(at(e, iz, iy, ix)) - cut;
        if (g > 0.0) {
          const double rz = iz - hz, ry = iy - hy, rx = ix - hx;
          s[0] += g;
          s[1] += g * rz; s[2] += g * ry; s[3] += g * rx;
          s[4] += g * rz * rz; s[5] += g * ry * ry; s[6] += g * rx * rx;
        }
      }
      int action = pf::lm_start(lm, bg, centre, s, max_iter) ? pf::kNeedSums : pf::kDone;
      double t[pf::kParams];
      while (action != pf::kDone) {
        if (action == pf::kNeedSums) {
          for (int k = 0; k < pf::kParams; ++k) t[k] = lm.theta[k];
          for (int k = 0; k < pf::kSums; ++k) s[k] = 0.0;
          for (int e = 0; e < n; ++e) {
            const double v = static_cast<double>(at(e, iz, iy, ix));
            pf::add_voxel<true>(t, v, iz - hz, iy - hy, ix - hx, s);
          }
          for (int k = 0; k < pf::kSums; ++k) lm.sums[k] = s[k];
          lm.cost = s[pf::kSums - 1];
        }
        if (!pf::lm_solve(lm)) break;
        for (int k = 0; k < pf::kParams; ++k) t[k] = lm.trial[k];
        s[pf::kSums - 1] = 0.0;
        for (int e = 0; e < n; ++e) {
          const double v = static_cast<double>(at(e, iz, iy, ix));
          pf::add_voxel<false>(t, v, iz - hz, iy - hy, ix - hx, s);
        }
        action = pf::lm_judge(lm, s[pf::kSums - 1]);
      }
      status[b] = pf::lm_finish(lm, out);
    }
  });
  return LSR_OK;
}

extern "C" int lsr_psf_accumulate_shifted_f32_cpu(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                                                  int64_t n_beads, int pz, int py, int px, double* bead_stats,
                                                  const double* weights, void* /* scratch: unused */, float* psf,
                                                  lsr_stream_t) {
  namespace pf = lsr::psffit;
  namespace pk = lsr::peaks;
  if (int rc = pf::check_psf_shift(vol, Z, Y, X, centres, n_beads, pz, py, px, bead_stats, weights, psf)) return rc;
  const int n = pz * py * px, plane = py * px, nw = pz + py + px;
  // (B, S) as lsr_psf_accumulate_f32_cpu computes them: the same tree
  constexpr int kTree = pk::kTreeThreads;
  parallel_ranges(n_beads, [&](int64_t first, int64_t last) {
    double red[kTree];
    for (int64_t b = first; b < last; ++b) {
      int64_t z0 = 0, y0 = 0, x0 = 0;
      if (!pk::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0)) {
        bead_stats[2 * b] = bead_stats[2 * b + 1] = 0.0;
        continue;
      }
      const float* corner = vol + (z0 * Y + y0) * X + x0;
      const double bg = face_mean(corner, Y, X, pz, py, px);
      for (int t = 0; t < kTree; ++t) {
        double acc = 0.0;
        for (int e = t; e < n; e += kTree) {
          const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
          acc += static_cast<double>(corner[(iz * Y + iy) * X + ix]) - bg;
        }
        red[t] = acc;
      }
      for (int w = kTree / 2; w > 0; w >>= 1)
        for (int t = 0; t < w; ++t) red[t] += red[t + w];
      bead_stats[2 * b] = bg;
      bead_stats[2 * b + 1] = red[0];
    }
  });
  // a batch of shifted patches at a time (the result does not depend on the batch: beads are added in list order)
  const int64_t batch = std::min<int64_t>(n_beads, std::max(1, lsr::g_host_threads.load()));
  std::vector<double> acc, patches;
  std::vector<char> use;
  try {
    acc.assign(static_cast<size_t>(n), 0.0);
    patches.resize(static_cast<size_t>(2 * batch * n));
    use.resize(static_cast<size_t>(batch));
  } catch (const std::bad_alloc&) {
    return lsr::fail(LSR_E_ARG, "lsr_psf_accumulate_shifted_f32_cpu: out of memory for %lld float64 patches of %d voxels",
                     (long long)(2 * batch + 1), n);
  }
  int64_t used = 0;
  for (int64_t first = 0; first < n_beads; first += batch) {
    const int64_t count = std::min(batch, n_beads - first);
    parallel_ranges(count, [&](int64_t lo, int64_t hi) {
      for (int64_t slot = lo; slot < hi; ++slot) {
        const int64_t b = first + slot;
        const double* w = weights + b * nw;
        bool ok = true;
        for (int k = 0; k < nw; ++k) ok = ok && std::isfinite(w[k]);
        int64_t z0 = 0, y0 = 0, x0 = 0;
        const double bg = bead_stats[2 * b], total = bead_stats[2 * b + 1];
        ok = ok && total > 0.0 && pk::patch_origin(centres[b], Z, Y, X, pz, py, px, z0, y0, x0);
        use[slot] = ok;
        if (!ok) continue;
        const float* corner = vol + (z0 * Y + y0) * X + x0;
        double* p0 = patches.data() + slot * 2 * n;
        double* p1 = p0 + n;
        const double *wz = w, *wy = w + pz, *wx = w + pz + py;
        for (int e = 0; e < n; ++e) {
          const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
          p0[e] = pf::circulant(corner + (iz * Y + iy) * X, int64_t(1), bg, wx, px, ix);
        }
        for (int e = 0; e < n; ++e) {
          const int iz = e / plane, rem = e - iz * plane, iy = rem / px, ix = rem - iy * px;
          p1[e] = pf::circulant(p0 + iz * plane + ix, int64_t(px), 0.0, wy, py, iy);
        }
        for (int e = 0; e < n; ++e) {
          const int iz = e / plane, rem = e - iz * plane;
          p0[e] = pf::circulant(p1 + rem, int64_t(plane), 0.0, wz, pz, iz);
        }
      }
    });
    parallel_ranges(n, [&](int64_t lo, int64_t hi) {
      for (int64_t slot = 0; slot < count; ++slot) {
        if (!use[slot]) continue;
        const double total = bead_stats[2 * (first + slot) + 1];
        const double* p0 = patches.data() + slot * 2 * n;
        for (int64_t e = lo; e < hi; ++e) acc[e] += p0[e] / total;
      }
    });
    for (int64_t slot = 0; slot < count; ++slot) used += use[slot] ? 1 : 0;
  }
  for (int e = 0; e < n; ++e) psf[e] = used > 0 ? static_cast<float>(acc[e] / static_cast<double>(used)) : 0.0f;
  return LSR_OK;
}

// ---- mid-band spectral power of every plane (focus.hip): the same table of intervals, float64 transforms ----
#include <complex>

#include "focus.hpp"

namespace {

using cplx = std::complex<double>;

struct HostFft {
  int n;
  std::vector<int> radix;
  std::vector<cplx> w;      // exp(-2 pi i k / n)
  explicit HostFft(int n_) : n(n_), w(static_cast<size_t>(n_)) {
    int m = n_;
    for (int r : {2, 3, 5})
      while (m % r == 0) { radix.push_back(r); m /= r; }
    const double step = -2.0 * 3.14159265358979323846 / n_;
    for (int k = 0; k < n_; ++k) w[static_cast<size_t>(k)] = cplx(std::cos(step * k), std::sin(step * k));
  }
  // Stockham autosort passes between x and y (each n long); returns the buffer that holds the result
  cplx* run(cplx* x, cplx* y) const {
    int len = n, s = 1;
    for (int r : radix) {
      const int m = len / r;
      for (int p = 0; p < m; ++p)
        for (int q = 0; q < s; ++q)
          for (int j = 0; j < r; ++j) {
            cplx acc(0.0, 0.0);
            for (int k = 0; k < r; ++k) acc += x[q + s * (p + m * k)] * w[static_cast<size_t>(((j * k) % r) * (n / r))];
            y[q + s * (r * p + j)] = acc * w[static_cast<size_t>(p) * s * j];
          }
      std::swap(x, y);
      len = m;
      s *= r;
    }
    return x;
  }
};

}  // namespace

// The twin of lsr_band_power_f32: host pointers; the twiddle tables and the scratch buffers are not used (may be NULL).
extern "C" int lsr_band_power_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, int64_t y0, int64_t x0, int64_t Yc,
                                      int64_t Xc, const float* /* tw_half */, const float* /* tw_x */, const float* /* tw_y */,
                                      const int32_t* table, int64_t k_hi, float* /* spec_scratch */, double* /* partial */,
                                      double* out_power, lsr_stream_t) {
  if (int rc = lsr::focus::check(in, Z, Y, X, y0, x0, Yc, Xc, table, k_hi, out_power)) return rc;
  LSR_REQUIRE(lsr::focus::lengths_ok(Yc, Xc), LSR_E_UNSUPPORTED,
              "window (%lld,%lld): Xc a multiple of 4 whose half is 5-smooth and at most 2048, Yc 5-smooth in [2, %d]",
              (long long)Yc, (long long)Xc, lsr::focus::kMaxY);
  const int ny = static_cast<int>(Yc), nx = static_cast<int>(Xc), kc = static_cast<int>(k_hi) + 1;
  std::atomic<bool> failed{false};
  parallel_ranges(Z, [&](int64_t first, int64_t last) {
    const HostFft fx(nx), fy(ny);
    const size_t longest = static_cast<size_t>(std::max(nx, ny));
    std::vector<cplx> a(longest), b(longest), spec(static_cast<size_t>(kc) * ny);
    for (int64_t z = first; z < last; ++z) {
      for (int y = 0; y < ny; ++y) {
        const float* src = in + (z * Y + y0 + y) * X + x0;
        for (int x = 0; x < nx; ++x) a[static_cast<size_t>(x)] = cplx(static_cast<double>(src[x]), 0.0);
        const cplx* f = fx.run(a.data(), b.data());
        for (int k = 0; k < kc; ++k) spec[static_cast<size_t>(k) * ny + y] = f[k];
      }
      double total = 0.0;
      for (int k = 0; k < kc; ++k) {
        const int lo = std::max(table[2 * k], 0), hi = std::min(table[2 * k + 1], ny / 2);
        if (lo > hi) continue;
        std::copy(spec.begin() + static_cast<size_t>(k) * ny, spec.begin() + static_cast<size_t>(k + 1) * ny, a.begin());
        const cplx* f = fy.run(a.data(), b.data());
        double acc = 0.0;
        for (int m = lo; m <= hi; ++m) {
          acc += std::abs(f[m]);
          if (m != 0 && 2 * m != ny) acc += std::abs(f[ny - m]);
        }
        total += (k == 0 || 2 * k == nx) ? acc : 2.0 * acc;
      }
      out_power[z] = total;
    }
  }, failed);
  LSR_REQUIRE(!failed.load(), LSR_E_ARG, "lsr_band_power_f32_cpu: out of memory for the plane buffers");
  return LSR_OK;
}

// ---- 2x mean downsampling (pyramid.hip): the window arithmetic of pyramid.hpp, voxel by voxel ----
#include "pyramid.hpp"

namespace {

template <typename T>
int downsample2_host(const T* in, int64_t Z, int64_t Y, int64_t X, T* out, int fz) {
  namespace py = lsr::pyramid;
  LSR_REQUIRE_HOST_FMA();
  if (int rc = py::check(in, Z, Y, X, out, fz)) return rc;
  const int64_t Zo = py::out_extent(Z, fz), Yo = py::out_extent(Y, 2), Xo = py::out_extent(X, 2), plane = Y * X;
  parallel_ranges(Zo * Yo, [&](int64_t first, int64_t last) {
    for (int64_t row = first; row < last; ++row) {
      const int64_t zo = row / Yo, yo = row - zo * Yo, z0 = zo * fz, y0 = 2 * yo;
      const bool hz = fz == 2 && z0 + 1 < Z, hy = y0 + 1 < Y;
      const T* r00 = in + (z0 * Y + y0) * X;
      const T* r01 = hy ? r00 + X : r00;            // (a row that does not exist is never read: finish() ignores its pair)
      const T* r10 = hz ? r00 + plane : r00;
      const T* r11 = hz ? r01 + plane : r01;
      T* dst = out + row * Xo;
      for (int64_t xo = 0; xo < Xo; ++xo) {
        const int64_t x0 = 2 * xo;
        const bool hx = x0 + 1 < X;
        const int64_t x1 = hx ? x0 + 1 : x0;
        const int k = static_cast<int>(hx) + static_cast<int>(hy) + static_cast<int>(hz);
        dst[xo] = py::finish(py::pair(r00[x0], r00[x1], hx), py::pair(r01[x0], r01[x1], hx), py::pair(r10[x0], r10[x1], hx),
                             py::pair(r11[x0], r11[x1], hx), hy, hz, k);
      }
    }
  });
  return LSR_OK;
}

}  // namespace

extern "C" int lsr_downsample2_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int fz, lsr_stream_t) {
  return downsample2_host<float>(in, Z, Y, X, out, fz);
}

extern "C" int lsr_downsample2_u16_cpu(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, uint16_t* out, int fz,
                                       lsr_stream_t) {
  return downsample2_host<uint16_t>(in, Z, Y, X, out, fz);
}

// ---- stitching (stitch.hip): the coverage, sample, weight and blend of stitch.hpp, row by row ----
#include "stitch.hpp"

extern "C" int lsr_stitch_f32_cpu(const void* table, int n_tiles, float* out, const int64_t box_origin[3],
                                  const int64_t box_shape[3], int p, float cval, lsr_stream_t) {
  namespace st = lsr::stitch;
  LSR_REQUIRE_HOST_FMA();
  if (int rc = st::check_launch(table, n_tiles, out, box_origin, box_shape, p)) return rc;
  const st::Tile* tab = static_cast<const st::Tile*>(table);
  for (int k = 0; k < n_tiles; ++k) {       // (a host table can be read here; the device entry trusts lsr_stitch_prepare_table)
    LSR_REQUIRE(tab[k].data != nullptr, LSR_E_NULL, "tile %d is NULL", k);
    LSR_REQUIRE(tab[k].n[0] > 0 && tab[k].n[1] > 0 && tab[k].n[2] > 0, LSR_E_SHAPE, "tile %d: shape (%lld,%lld,%lld) must be positive",
                k, (long long)tab[k].n[0], (long long)tab[k].n[1], (long long)tab[k].n[2]);
    LSR_REQUIRE_VOLUME(tab[k].n[0], tab[k].n[1], tab[k].n[2]);
    LSR_REQUIRE(tab[k].n[1] <= st::kMaxEdgeExtent && tab[k].n[2] <= st::kMaxEdgeExtent, LSR_E_UNSUPPORTED,
                "tile %d: the y and x extents are at most 2^24", k);
  }
  const int64_t Bz = box_shape[0], By = box_shape[1], Bx = box_shape[2];
  std::atomic<bool> failed{false};
  parallel_ranges(Bz * By, [&](int64_t first, int64_t last) {
    std::vector<st::Acc> acc(static_cast<size_t>(Bx));
    for (int64_t row = first; row < last; ++row) {
      const int64_t zb = row / By, yb = row - zb * By, cz = box_origin[0] + zb, cy = box_origin[1] + yb;
      for (st::Acc& a : acc) a.clear();
      for (int k = 0; k < n_tiles; ++k) {
        const st::Tile& e = tab[k];
        const int fz = e.frac[0], fy = e.frac[1], fx = e.frac[2];
        const int64_t ny = e.n[1], nx = e.n[2], plane = ny * nx;
        const int64_t jz = cz - e.ti[0], jy = cy - e.ti[1];
        if (!st::covered(jz, e.n[0], fz) || !st::covered(jy, ny, fy)) continue;
        // rows r[z tap][y tap], tap 0 = j - 1: it exists only on a fractional axis, otherwise the name points at tap j's row
        const float* r11 = e.data + (jz * ny + jy) * nx;
        const float* r10 = fy ? r11 - nx : r11;
        const float* r01 = fz ? r11 - plane : r11;
        const float* r00 = fz ? r10 - plane : r10;
        const float dy = st::edge(jy, ny, e.w0[1], e.w1[1]);
        const float wx0 = e.w0[2], wx1 = e.w1[2];
        const int64_t x_first = std::max<int64_t>(0, e.ti[2] + fx - box_origin[2]);
        const int64_t x_last = std::min<int64_t>(Bx - 1, e.ti[2] + nx - 1 - box_origin[2]);
        for (int64_t x = x_first; x <= x_last; ++x) {
          const int64_t j = box_origin[2] + x - e.ti[2], j0 = fx ? j - 1 : j;
          const float a00 = st::tap(r00[j0], r00[j], fx, wx0, wx1), a01 = st::tap(r01[j0], r01[j], fx, wx0, wx1);
          const float a10 = st::tap(r10[j0], r10[j], fx, wx0, wx1), a11 = st::tap(r11[j0], r11[j], fx, wx0, wx1);
          const float v = st::tap(st::tap(a00, a01, fy, e.w0[1], e.w1[1]), st::tap(a10, a11, fy, e.w0[1], e.w1[1]), fz, e.w0[0],
                                  e.w1[0]);
          acc[static_cast<size_t>(x)].add(v, st::weight(dy, st::edge(j, nx, e.w0[2], e.w1[2]), p));
        }
      }
      float* dst = out + row * Bx;
      for (int64_t x = 0; x < Bx; ++x) dst[x] = acc[static_cast<size_t>(x)].finish(cval);
    }
  }, failed);
  LSR_REQUIRE(!failed.load(), LSR_E_ARG, "lsr_stitch_f32_cpu: out of memory for the row accumulators");
  return LSR_OK;
}

// ---- labelling (label.hip): plain sequential code; scipy.ndimage.label's numbering, the kernels' integers ----
#include "label.hpp"

extern "C" int lsr_label_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int connectivity,
                                 int32_t* labels, int32_t* n_objects, void* scratch, lsr_stream_t) {
  namespace lb = lsr::label;
  if (int rc = lb::check_label(in, Z, Y, X, connectivity, labels, n_objects, scratch)) return rc;
  const int level = lb::level_of(connectivity);
  const int64_t n = Z * Y * X, plane = Y * X;
  int32_t* parent = labels;                    // a union-find rooted at the smallest index, as on the device
  for (int64_t z = 0; z < Z; ++z) {
    for (int64_t y = 0; y < Y; ++y) {
      for (int64_t x = 0; x < X; ++x) {
        const int64_t v = z * plane + y * X + x;
        if (!(in[v] > threshold)) {
          parent[v] = -1;
          continue;
        }
        int32_t root = static_cast<int32_t>(v);
        parent[v] = root;
        for (int dz = -1; dz <= 0; ++dz) {
          for (int dy = -1; dy <= 1; ++dy) {
            for (int dx = -1; dx <= 1; ++dx) {
              if (!lb::backward_neighbour(dz, dy, dx, level)) continue;
              if (z + dz < 0 || y + dy < 0 || y + dy >= Y || x + dx < 0 || x + dx >= X) continue;
              const int64_t t = v + dz * plane + dy * X + dx;
              if (parent[t] < 0) continue;
              const int32_t other = lb::find_host(parent, static_cast<int32_t>(t));
              if (other == root) continue;
              const int32_t lo = other < root ? other : root, hi = other < root ? root : other;
              parent[hi] = lo;
              root = lo;
              parent[v] = lo;                   // (keeps the walk from v short)
            }
          }
        }
      }
    }
  }
  *n_objects = lb::number_roots_host(labels, n);
  return LSR_OK;
}

extern "C" int lsr_label_regions_f32_cpu(const int32_t* labels, const float* intensity, int64_t Z, int64_t Y, int64_t X,
                                         int64_t n_objects, void* table, lsr_stream_t) {
  namespace lb = lsr::label;
  if (int rc = lb::check_regions(labels, Z, Y, X, n_objects, table)) return rc;
  if (n_objects == 0) return LSR_OK;
  lb::Region* rows = static_cast<lb::Region*>(table);
  for (int64_t z = 0; z < Z; ++z) {
    for (int64_t y = 0; y < Y; ++y) {
      for (int64_t x = 0; x < X; ++x) {
        const int64_t v = (z * Y + y) * X + x;
        const int32_t l = labels[v];
        if (l <= 0 || l > n_objects) continue;
        lb::Region& r = rows[l - 1];
        const int32_t c[3] = {static_cast<int32_t>(z), static_cast<int32_t>(y), static_cast<int32_t>(x)};
        const bool first = r.volume == 0;
        r.volume += 1;
        for (int a = 0; a < 3; ++a) {
          r.sum_zyx[a] += c[a];
          r.lo[a] = first ? c[a] : std::min(r.lo[a], c[a]);
          r.hi[a] = first ? c[a] + 1 : std::max(r.hi[a], c[a] + 1);
        }
        if (intensity == nullptr) continue;
        const float f = intensity[v];
        const double g = static_cast<double>(f);
        r.sum_v += g;
        for (int a = 0; a < 3; ++a) r.sum_vzyx[a] += g * c[a];
        // (compared through the kernels' integer image, so that -0.0, +0.0 and NaNs fall where they fall on the device)
        const uint32_t k = lb::float_key(f);
        if (first || k < lb::float_key(r.v_min)) r.v_min = f;
        if (first || k > lb::float_key(r.v_max)) r.v_max = f;
      }
    }
  }
  return LSR_OK;
}

extern "C" int lsr_label_remap_i32_cpu(int32_t* labels, int64_t n, const int32_t* map, int64_t n_map, lsr_stream_t) {
  if (int rc = lsr::label::check_remap(labels, n, map, n_map)) return rc;
  for (int64_t v = 0; v < n; ++v) {
    const int32_t l = labels[v];
    labels[v] = (l > 0 && l < n_map) ? map[l] : 0;
  }
  return LSR_OK;
}

// ---- distance transform (edt.hip): plain sequential code over edt.hpp's row rule and line pass ----
#include "edt.hpp"

namespace {

struct HostStack {           // an envelope stack in host memory
  std::vector<int32_t> words;
  void put(int q, int k, int v, int t) {
    int32_t* e = &words[static_cast<size_t>(q) * lsr::edt::kStackFields];
    e[0] = k; e[1] = v; e[2] = t;
  }
  void get(int q, int& k, int& v, int& t) const {
    const int32_t* e = &words[static_cast<size_t>(q) * lsr::edt::kStackFields];
    k = e[0]; v = e[1]; t = e[2];
  }
};

template <class Sites>
int edt_host(Sites sites, int64_t Z, int64_t Y, int64_t X, const double* sampling, float* dist, int32_t* nearest) {
  namespace ed = lsr::edt;
  const ed::Sampling s = ed::make_sampling(sampling);
  int32_t* work = nearest != nullptr ? nearest : reinterpret_cast<int32_t*>(dist);
  const int64_t plane = Y * X;
  const int iX = static_cast<int>(X);
  HostStack stack;
  try {
    stack.words.resize(static_cast<size_t>(std::max(Y, Z)) * ed::kStackFields);
  } catch (const std::bad_alloc&) {
    return lsr::fail(LSR_E_ARG, "lsr_edt_*_cpu: out of memory for the envelope stack");
  }
  for (int64_t row = 0; row < Z * Y; ++row) {             // x: left-nearest forward, the nearer of left and right backward
    int32_t* w = work + row * X;
    int carry = -1;
    for (int x = 0; x < iX; ++x) {
      if (sites(row * X + x)) carry = x;
      w[x] = carry;
    }
    carry = -1;
    for (int x = iX - 1; x >= 0; --x) {
      if (w[x] == x) carry = x;
      w[x] = ed::nearer_in_row(x, w[x], carry);
    }
  }
  for (int64_t z = 0; z < Z; ++z) {
    for (int x = 0; x < iX; ++x) {
      ed::YLine io{work + z * plane + x, X, x, iX, s.wx};
      ed::line_pass(static_cast<int>(Y), s.wy, io, stack);
    }
  }
  for (int64_t line = 0; line < plane; ++line) {
    ed::ZLine io{work + line, nearest != nullptr ? nearest + line : nullptr,
                 dist != nullptr ? reinterpret_cast<int32_t*>(dist) + line : nullptr, plane, static_cast<int>(line / X),
                 static_cast<int>(line % X), iX, s};
    ed::line_pass(static_cast<int>(Z), s.wz, io, stack);
  }
  return LSR_OK;
}

}  // namespace

extern "C" int lsr_edt_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int invert, const double* sampling,
                               float* dist, int32_t* nearest, void* scratch, lsr_stream_t) {
  if (int rc = lsr::edt::check_edt(in, Z, Y, X, sampling, dist, nearest, scratch)) return rc;
  const bool inv = invert != 0;
  return edt_host([=](int64_t v) { return !(in[v] > threshold) != inv; }, Z, Y, X, sampling, dist, nearest);
}

extern "C" int lsr_edt_labels_i32_cpu(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int invert, const double* sampling,
                                      float* dist, int32_t* nearest, void* scratch, lsr_stream_t) {
  if (int rc = lsr::edt::check_edt(labels, Z, Y, X, sampling, dist, nearest, scratch)) return rc;
  const bool inv = invert != 0;
  return edt_host([=](int64_t v) { return (labels[v] != 0) != inv; }, Z, Y, X, sampling, dist, nearest);
}

extern "C" int lsr_label_expand_i32_cpu(const int32_t* labels, const int32_t* nearest, int64_t Z, int64_t Y, int64_t X,
                                        const double* sampling, double distance, int32_t* out, lsr_stream_t) {
  namespace ed = lsr::edt;
  if (int rc = ed::check_expand(labels, nearest, Z, Y, X, sampling, distance, out)) return rc;
  const ed::Sampling s = ed::make_sampling(sampling);
  const int64_t n = Z * Y * X;
  int64_t v = 0;
  for (int z = 0; z < Z; ++z) {
    for (int y = 0; y < Y; ++y) {
      for (int x = 0; x < X; ++x, ++v) {
        const int32_t site = nearest[v];
        const bool in_reach = site >= 0 && site < n &&
                              ed::distance_to(s, z, y, x, site, static_cast<int>(Y), static_cast<int>(X)) <= distance;
        out[v] = in_reach ? labels[site] : 0;
      }
    }
  }
  return LSR_OK;
}

// ---- watershed (watershed.hip): plain sequential code over watershed.hpp's `up` rule, slot record and hash ----
#include "watershed.hpp"

extern "C" int lsr_watershed_f32_cpu(const int32_t* objects, const float* surface, int64_t Z, int64_t Y, int64_t X, int connectivity,
                                     int32_t* basins, int32_t* n_basins, void* scratch, lsr_stream_t) {
  namespace lb = lsr::label;
  namespace ws = lsr::watershed;
  if (int rc = ws::check_watershed(objects, surface, Z, Y, X, connectivity, basins, n_basins, scratch)) return rc;
  const int level = lb::level_of(connectivity);
  const int64_t n = Z * Y * X, plane = Y * X;
  int32_t* parent = basins;                    // a union-find rooted at the smallest index, as on the device
  for (int64_t v = 0; v < n; ++v) parent[v] = objects[v] > 0 ? static_cast<int32_t>(v) : -1;
  for (int64_t z = 0; z < Z; ++z) {
    for (int64_t y = 0; y < Y; ++y) {
      for (int64_t x = 0; x < X; ++x) {
        const int64_t v = z * plane + y * X + x;
        const int32_t o = objects[v];
        if (o <= 0) continue;
        const int code = ws::up_code(lb::float_key(surface[v]), level, [&](int dz, int dy, int dx, uint32_t* key) {
          if (z + dz < 0 || z + dz >= Z || y + dy < 0 || y + dy >= Y || x + dx < 0 || x + dx >= X) return false;
          const int64_t u = v + dz * plane + dy * X + dx;
          if (objects[u] != o) return false;
          *key = lb::float_key(surface[u]);
          return true;
        });
        if (code == ws::kSelf) continue;
        const int64_t t = v + (code / 9 - 1) * plane + (code / 3 % 3 - 1) * X + (code % 3 - 1);
        const int32_t a = lb::find_host(parent, static_cast<int32_t>(v)), b = lb::find_host(parent, static_cast<int32_t>(t));
        if (a != b) parent[a < b ? b : a] = a < b ? a : b;
      }
    }
  }
  *n_basins = lb::number_roots_host(basins, n);
  return LSR_OK;
}

extern "C" int lsr_watershed_saddles_f32_cpu(const int32_t* objects, const int32_t* basins, const float* surface, int64_t Z, int64_t Y,
                                             int64_t X, int connectivity, int64_t capacity, void* table, int32_t* counts,
                                             lsr_stream_t) {
  namespace lb = lsr::label;
  namespace ws = lsr::watershed;
  if (int rc = ws::check_saddles(objects, basins, surface, Z, Y, X, connectivity, capacity, table, counts)) return rc;
  const int level = lb::level_of(connectivity);
  const int64_t plane = Y * X;
  const uint32_t mask = static_cast<uint32_t>(capacity - 1);
  const int probes = lsr::pair_probes(capacity);
  ws::Saddle* slots = static_cast<ws::Saddle*>(table);
  counts[0] = counts[1] = 0;
  for (int64_t z = 0; z < Z; ++z) {
    for (int64_t y = 0; y < Y; ++y) {
      for (int64_t x = 0; x < X; ++x) {
        const int64_t v = z * plane + y * X + x;
        const int32_t o = objects[v], a0 = basins[v];
        if (o <= 0 || a0 <= 0) continue;
        const uint32_t kv = lb::float_key(surface[v]);
        for (int dz = 0; dz <= 1; ++dz) {
          for (int dy = -1; dy <= 1; ++dy) {
            for (int dx = -1; dx <= 1; ++dx) {
              if (!ws::forward_neighbour(dz, dy, dx, level)) continue;
              if (z + dz >= Z || y + dy < 0 || y + dy >= Y || x + dx < 0 || x + dx >= X) continue;
              const int64_t u = v + dz * plane + dy * X + dx;
              if (objects[u] != o) continue;
              const int32_t b0 = basins[u];
              if (b0 <= 0 || b0 == a0) continue;
              const uint32_t ku = lb::float_key(surface[u]), pass = std::min(ku, kv);
              const unsigned long long a = static_cast<uint32_t>(std::min(a0, b0)), b = static_cast<uint32_t>(std::max(a0, b0));
              const unsigned long long pair = a << 32 | b;
              const bool placed = lsr::pair_insert_host(slots, mask, probes, pair, counts,
                                                        [&](ws::Saddle& slot) { slot.key = std::max(slot.key, pass); });
              if (!placed) counts[1] += 1;
            }
          }
        }
      }
    }
  }
  return LSR_OK;
}

// ---- label overlap (overlap.hip): plain sequential code over overlap.hpp's rule, record, hash and probe bound ----
#include "overlap.hpp"

extern "C" int lsr_label_overlap_i32_cpu(const int32_t* a, const int32_t* b, int64_t Z, int64_t Y, int64_t X,
                                         const int32_t shift_zyx[3], int64_t capacity, void* table, int32_t* counts,
                                         int max_blocks, lsr_stream_t) {
  namespace ov = lsr::overlap;
  if (int rc = ov::check_overlap(a, b, Z, Y, X, shift_zyx, capacity, table, counts, max_blocks)) return rc;
  counts[0] = counts[1] = 0;
  if (ov::shift_empties(Z, Y, X, shift_zyx)) return LSR_OK;
  const int64_t sz = shift_zyx[0], sy = shift_zyx[1], sx = shift_zyx[2], plane = Y * X;
  const uint32_t mask = static_cast<uint32_t>(capacity - 1);
  const int probes = lsr::pair_probes(capacity);
  ov::Overlap* slots = static_cast<ov::Overlap*>(table);
  for (int64_t z = std::max<int64_t>(0, -sz); z < std::min(Z, Z - sz); ++z) {
    for (int64_t y = std::max<int64_t>(0, -sy); y < std::min(Y, Y - sy); ++y) {
      for (int64_t x = std::max<int64_t>(0, -sx); x < std::min(X, X - sx); ++x) {
        const int64_t v = z * plane + y * X + x;
        const int32_t a0 = a[v], b0 = b[v + sz * plane + sy * X + sx];
        if (a0 <= 0 || b0 <= 0) continue;
        const unsigned long long pair = ov::pack(a0, b0);
        if (!lsr::pair_insert_host(slots, mask, probes, pair, counts, [](ov::Overlap& slot) { slot.count += 1; })) counts[1] += 1;
      }
    }
  }
  return LSR_OK;
}

// ---- label moments (moments.hip): plain sequential code over moments.hpp's rule, record and checks, voxel by voxel (the kernel
// adds the closed-form sums of whole runs: the two must agree byte for byte) ----
#include "moments.hpp"

extern "C" int lsr_label_moments_i32_cpu(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, void* table,
                                         int max_blocks, lsr_stream_t) {
  namespace mo = lsr::moments;
  if (int rc = mo::check_moments(labels, Z, Y, X, n_objects, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  mo::Moments* rows = static_cast<mo::Moments*>(table);
  for (int64_t z = 0; z < Z; ++z) {
    for (int64_t y = 0; y < Y; ++y) {
      const int32_t* line = labels + (z * Y + y) * X;
      for (int64_t x = 0; x < X; ++x) {
        const int32_t l = line[x];
        if (l < 1 || l > n_objects) continue;
        mo::Moments& m = rows[l - 1];
        m.volume += 1;
        m.s_z += z;
        m.s_y += y;
        m.s_x += x;
        m.m_zz += z * z;
        m.m_yy += y * y;
        m.m_xx += x * x;
        m.m_zy += z * y;
        m.m_zx += z * x;
        m.m_yx += y * x;
      }
    }
  }
  return LSR_OK;
}

// ---- label intensities (intensity.hip): plain sequential code over intensity.hpp's rule, records and checks, voxel by voxel.
// uint16 values: the kernel's records byte for byte.  float32 values: count and extremes are the kernel's, the float64 sums are
// another order of the same terms (both inside intensity.hpp's bound) ----
#include "intensity.hpp"

extern "C" int lsr_label_intensity_f32_cpu(const int32_t* labels, const float* values, int64_t Z, int64_t Y, int64_t X,
                                           int64_t n_objects, void* table, int max_blocks, lsr_stream_t) {
  namespace in = lsr::intensity;
  if (int rc = in::check_intensity(labels, values, sizeof(float), Z, Y, X, n_objects, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  in::accumulate_host<float, in::RecordF32, double>(labels, values, Z, Y, X, n_objects, static_cast<in::RecordF32*>(table));
  return LSR_OK;
}

extern "C" int lsr_label_intensity_u16_cpu(const int32_t* labels, const uint16_t* values, int64_t Z, int64_t Y, int64_t X,
                                           int64_t n_objects, void* table, int max_blocks, lsr_stream_t) {
  namespace in = lsr::intensity;
  if (int rc = in::check_intensity(labels, values, sizeof(uint16_t), Z, Y, X, n_objects, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  in::accumulate_host<uint16_t, in::RecordU16, uint64_t>(labels, values, Z, Y, X, n_objects, static_cast<in::RecordU16*>(table));
  return LSR_OK;
}

// ---- per-object sums over two channels (coloc.hip): plain sequential code over coloc.hpp's rule, records and checks, voxel by
// voxel in raster order.  uint16 values: the kernel's records byte for byte.  float32 values: the counts are the kernel's, the
// float64 sums are another order of the same terms (both inside coloc.hpp's bound) ----
#include "coloc.hpp"

extern "C" int lsr_label_coloc_f32_cpu(const int32_t* labels, const float* a, const float* b, int64_t Z, int64_t Y, int64_t X,
                                       int64_t n_objects, float ta, float tb, void* table, int max_blocks, lsr_stream_t) {
  namespace co = lsr::coloc;
  if (int rc = co::check_coloc(labels, a, b, sizeof(float), Z, Y, X, n_objects, ta, tb, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  co::accumulate_host<float, co::RecordF32, double>(labels, a, b, Z * Y * X, n_objects, ta, tb, static_cast<co::RecordF32*>(table));
  return LSR_OK;
}

extern "C" int lsr_label_coloc_u16_cpu(const int32_t* labels, const uint16_t* a, const uint16_t* b, int64_t Z, int64_t Y, int64_t X,
                                       int64_t n_objects, float ta, float tb, void* table, int max_blocks, lsr_stream_t) {
  namespace co = lsr::coloc;
  if (int rc = co::check_coloc(labels, a, b, sizeof(uint16_t), Z, Y, X, n_objects, ta, tb, table, max_blocks)) return rc;
  if (n_objects == 0) return LSR_OK;
  co::accumulate_host<uint16_t, co::RecordU16, uint64_t>(labels, a, b, Z * Y * X, n_objects, ta, tb,
                                                         static_cast<co::RecordU16*>(table));
  return LSR_OK;
}

// ---- grey morphology (morphology.hip): the same plan of passes and the same walk (morphology.hpp), a tile of columns per step
// (walk_pass above) ----

extern "C" int lsr_grey_morph_f32_cpu(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int op,
                                      void* scratch, lsr_stream_t) {
  namespace mo = lsr::morph;
  if (int rc = mo::check_morph(in, out, Z, Y, X, rz, ry, rx, op, scratch)) return rc;
  const int64_t voxels = Z * Y * X;
  mo::Pass passes[mo::kMaxPasses];
  const int n = mo::plan(rz, ry, rx, op, passes);
  const int fuse = mo::fuse_of(op);
  if (n == 0) {
    for (int64_t e = 0; e < voxels; ++e) out[e] = mo::fused(in[e], in[e], fuse);
    return LSR_OK;
  }
  float* work = static_cast<float*>(scratch);
  std::atomic<bool> failed{false};
  for (int k = 0; k < n; ++k) {
    const mo::Pass ps = passes[k];
    const int f = k == n - 1 ? fuse : static_cast<int>(mo::kPlain);
    const mo::StoreSink sink{mo::pass_target(k, n, out, work, voxels), f != mo::kPlain ? in : nullptr, f};
    walk_pass(mo::pass_source(k, in, work, voxels), mo::lines_of(ps.axis, Z, Y, X), ps.r, ps.least, failed,
              [&](int) { return sink; });
    if (failed.load()) return lsr::fail(LSR_E_ARG, "lsr_grey_morph_f32_cpu: out of memory for the block strip");
  }
  return LSR_OK;
}

// ---- rank filters (rank.hip): the same fold, codes, bisection and fused op (rank.hpp), a row of voxels per step ----
#include "rank.hpp"

extern "C" int lsr_rank_filter_f32_cpu(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int rank,
                                       int op, float threshold, int variant, lsr_stream_t) {
  namespace rk = lsr::rank;
  if (int rc = rk::check_rank(in, out, Z, Y, X, rz, ry, rx, rank, op, threshold, variant)) return rc;
  lsr::parallel_ranges(Z * Y, [&](int64_t first, int64_t last) {
    for (int64_t row = first; row < last; ++row) {
      const int64_t z = row / Y, y = row - z * Y;
      for (int64_t x = 0; x < X; ++x) out[row * X + x] = rk::voxel_host(in, Z, Y, X, z, y, x, rz, ry, rx, rank, op, threshold);
    }
  });
  return LSR_OK;
}

// ---- Hessian eigenvalue responses (hessian.hip): the same derivative, entries, Jacobi sweeps, responses and store (hessian.hpp),
// a row of voxels per step; the loads go to the volume itself ----
#include "hessian.hpp"

extern "C" int lsr_hessian_response_f32_cpu(const float* g, float* out, int64_t Z, int64_t Y, int64_t X, double sz, double sy,
                                            double sx, double scale, int measure, int dark, int accumulate, lsr_stream_t) {
  namespace hs = lsr::hessian;
  if (int rc = hs::check_hessian(g, out, Z, Y, X, sz, sy, sx, scale, measure, dark, accumulate)) return rc;
  const hs::Recip recip = hs::recip_of(sz, sy, sx);
  lsr::parallel_ranges(Z * Y, [&](int64_t first, int64_t last) {
    for (int64_t row = first; row < last; ++row) {
      const int64_t z = row / Y, y = row - z * Y;
      for (int64_t x = 0; x < X; ++x) {
        const float r = hs::voxel_host(g, Z, Y, X, z, y, x, recip, scale, measure, dark);
        out[row * X + x] = accumulate ? hs::greater_of(out[row * X + x], r) : r;
      }
    }
  });
  return LSR_OK;
}

// ---- whole-volume statistics (stats.hip): plain sequential code over stats.hpp's rule, record and checks, voxel by voxel.  The
// tables, the counts and the codes of the extremes are the kernel's words; uint16 sums too; float32 sums are another order of the
// same terms (both inside stats.hpp's bound).  The rescale is the kernel's expression: the kernel's bits ----
#include "stats.hpp"

namespace {

template <typename V, typename Sum>
int digit_histogram_host(const V* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank, int k, void* tables,
                         void* moments, int grid_cap, int form) {
  namespace st = lsr::stats;
  st::Plan plan;
  if (int rc = st::check_histogram(in, sizeof(V), n, pass, prefixes, table_of_rank, k, tables, moments, grid_cap, form, &plan)) return rc;
  st::histogram_host<V, Sum>(in, n, plan, static_cast<uint64_t*>(tables), static_cast<uint64_t*>(moments));
  return LSR_OK;
}

template <typename V>
int rescale_host(const V* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out) {
  namespace st = lsr::stats;
  if (int rc = st::check_rescale(in, sizeof(V), n, clip, lo, hi, out)) return rc;
  lsr::parallel_ranges(n, [&](int64_t first, int64_t last) {
    for (int64_t i = first; i < last; ++i) out[i] = st::rescale_one(in[i], sub, div, clip != 0, lo, hi);
  });
  return LSR_OK;
}

}  // namespace

extern "C" int lsr_digit_histogram_f32_cpu(const float* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank,
                                           int k, void* tables, void* moments, int grid_cap, int form, lsr_stream_t) {
  return digit_histogram_host<float, double>(in, n, pass, prefixes, table_of_rank, k, tables, moments, grid_cap, form);
}

extern "C" int lsr_digit_histogram_u16_cpu(const uint16_t* in, int64_t n, int pass, const uint32_t* prefixes,
                                           const int32_t* table_of_rank, int k, void* tables, void* moments, int grid_cap, int form,
                                           lsr_stream_t) {
  return digit_histogram_host<uint16_t, uint64_t>(in, n, pass, prefixes, table_of_rank, k, tables, moments, grid_cap, form);
}

extern "C" int lsr_rescale_f32_cpu(const float* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                                   lsr_stream_t) {
  return rescale_host(in, n, sub, div, clip, lo, hi, out);
}

extern "C" int lsr_rescale_u16_cpu(const uint16_t* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                                   lsr_stream_t) {
  return rescale_host(in, n, sub, div, clip, lo, hi, out);
}
