// What the band-power kernels (focus.hip) and their host twin (host_twins.hip) share: the lengths they take, the
// argument checks and the float64 plan of the band -- one statement of the rule for both.
#pragma once

#include <cmath>

#include "common.hpp"

namespace lsr {
namespace focus {

constexpr int kMaxY = 2048;    // longest window column (focus.hip: LDS tile and butterfly index arithmetic)

inline bool smooth5(int64_t n) {
  if (n < 1) return false;
  for (int f : {2, 3, 5})
    while (n % f == 0) n /= f;
  return n == 1;
}

// Xc: a multiple of 4 whose half is 5-smooth, 8 .. 4096 (the rule of lsr_rfft_rows_supported); Yc: 5-smooth, 2 .. kMaxY
inline bool lengths_ok(int64_t Yc, int64_t Xc) {
  return Xc >= 8 && Xc % 4 == 0 && Xc / 2 <= 2048 && smooth5(Xc / 2) && Yc >= 2 && Yc <= kMaxY && smooth5(Yc);
}

// The band's bins, column by column of the half spectrum: table[2 kx], table[2 kx + 1] = the closed interval [a, b] of
// m = |ky'| = min(ky, Yc - ky) with band_lo < r < band_hi (a = 0, b = -1 where there is none), for kx = 0 .. Xc / 2;
// r = sqrt((m / (Yc p))^2 + (kx / (Xc p))^2) in float64, every operation rounded once (r grows with m, so the bins of a
// column are one interval).  *k_hi: the last column that holds a bin (-1: the band is empty); *weighted: the number of
// bins of the FULL spectrum inside the band (columns 0 < kx < Xc / 2 count twice).
inline void plan(int64_t Yc, int64_t Xc, double pixel_size, double band_lo, double band_hi, int32_t* table, int64_t* k_hi,
                 int64_t* weighted) {
  const double dy = static_cast<double>(Yc) * pixel_size, dx = static_cast<double>(Xc) * pixel_size;
  int64_t last = -1, count = 0;
  for (int64_t kx = 0; kx <= Xc / 2; ++kx) {
    const double fx = static_cast<double>(kx) / dx;
    int64_t a = 0, b = -1;
    bool open = false;
    for (int64_t m = 0; m <= Yc / 2; ++m) {
      const double fy = static_cast<double>(m) / dy;
      const double r = std::sqrt(fy * fy + fx * fx);
      if (band_lo < r && r < band_hi) {
        if (!open) { a = m; open = true; }
        b = m;
        count += ((m == 0 || 2 * m == Yc) ? 1 : 2) * ((kx == 0 || 2 * kx == Xc) ? 1 : 2);
      }
    }
    table[2 * kx] = static_cast<int32_t>(a);
    table[2 * kx + 1] = static_cast<int32_t>(b);
    if (open) last = kx;
  }
  *k_hi = last;
  if (weighted != nullptr) *weighted = count;
}

inline int check(const float* in, int64_t Z, int64_t Y, int64_t X, int64_t y0, int64_t x0, int64_t Yc, int64_t Xc,
                 const int32_t* table, int64_t k_hi, const double* out_power) {
  LSR_REQUIRE_PTR(in);
  LSR_REQUIRE_PTR(table);
  LSR_REQUIRE_PTR(out_power);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "volume shape (%lld,%lld,%lld) must be positive", (long long)Z,
              (long long)Y, (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE(Yc > 0 && Xc > 0 && y0 >= 0 && x0 >= 0 && y0 <= Y - Yc && x0 <= X - Xc, LSR_E_SHAPE,
              "the window (%lld,%lld) at (%lld,%lld) must lie inside the plane (%lld,%lld)", (long long)Yc, (long long)Xc,
              (long long)y0, (long long)x0, (long long)Y, (long long)X);
  LSR_REQUIRE(k_hi >= 0 && k_hi <= Xc / 2, LSR_E_ARG, "k_hi %lld must be a column of the half spectrum 0 .. %lld",
              (long long)k_hi, (long long)(Xc / 2));
  return LSR_OK;
}

}  // namespace focus
}  // namespace lsr
