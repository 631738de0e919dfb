// Total-variation factor of a regularised Richardson-Lucy iteration (RL-TV, Dey et al. 2006, multiplicative form):
//
//     out(r) = v(r) / (1 - lambda * div(r)),      div = div( grad u / |grad u| )
//
// with u = x_k (the estimate the RL launches read) and v = the plain RL update they wrote.  Forward differences for the
// gradient, backward differences for the divergence (its negative adjoint), voxel units, isotropic:
//
//     D_a u(r) = u(r + e_a) - u(r)                       0 where r + e_a is outside the volume
//     n(r)     = sqrt(D_z^2 + D_y^2 + D_x^2 + tv_eps^2)
//     p_a(r)   = D_a u(r) / n(r)
//     div(r)   = sum_a p_a(r) - p_a(r - e_a)              p_a(r - e_a) := 0 where r - e_a is outside
//
// |p_a| <= 1, so |div| <= 6 and lambda < 1/6 keeps the denominator positive.  The borders are those of (Z, Y, X): the
// kernel never reads outside the logical volume (a padded volume's zero halo is not data for this operator).  Both border
// rules fall out of ONE device: every coordinate is clamped into the volume when it is loaded.  A neighbour beyond the
// high border is then the voxel itself (D_a = an exact 0), and the "voxel" beyond the low border is a copy of the border
// voxel whose own D_a is an exact 0 (p_a(r - e_a) = 0 / n = 0): no border test anywhere in the arithmetic.
//
// Shape: a z-marching streaming stencil.  A workgroup of 256 threads owns a 16 x 64 tile (a thread: four consecutive x of
// one row) and marches along z.  Planes k and k + 1 of u sit in LDS on the tile grown by one row / column on both sides
// (a ring of three planes: plane k + 2 is fetched into registers before the arithmetic of plane k and written into the
// third slot after it, one barrier per plane); p_z(k - 1) travels in registers.  p_y(r - e_y) and p_x(r - e_x) are
// recomputed by the thread that needs them from the staged u (9 norms per 4 voxels) rather than exchanged through LDS:
// no second barrier, and the same bits as the owner's (same inputs, same operations).  Each u voxel comes from HBM once
// plus the tile-edge overlap (18 x 66 / 16 x 64) and two planes per z chunk; v and out are one 16-byte access per thread
// and plane where the rows are 16-byte aligned.  12 algorithmic bytes per voxel.
//
// Operation order (the host twin below runs the same inline functions; -ffp-contract=off, correctly rounded sqrt and
// division on both sides, so the twin's results are the kernel's):
//     inv = 1 / sqrt(((dz*dz + dy*dy) + dx*dx) + eps2);  p_a = d_a * inv
//     div = ((pz - pz_lo) + (py - py_lo)) + (px - px_lo);  out = v / (1 - lambda * div)
//
// No reference code: docs/data_structure.md:58-62 ("algorithms for deconvolution ... are being developed").

#include <cmath>

#include "common.hpp"
#include "correlate_common.hpp"
#include "host_parallel.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kTileY = 16, kTileX = 64;
constexpr int kColGroups = kTileX / 4;              // 16 threads per row
constexpr int kLdsRows = kTileY + 2;
constexpr int kLdsCol0 = 4;                         // LDS column of the tile's first x: 16-byte aligned rows
constexpr int kLdsPitch = 72;                       // [3 unused][x0 - 1][x0 .. x0 + 63][x0 + 64][3 unused]
constexpr int kLdsPlane = kLdsRows * kLdsPitch;
constexpr int kHalo = 2 * kTileX + 2 * kLdsRows;    // 164 halo elements per plane, one per thread
static_assert(kHalo <= kThreads, "one halo element per thread");

struct TvArgs {
  const float* u;
  const float* v;
  float* out;
  int64_t u_plane, v_plane, o_plane;
  int u_pitch, v_pitch, o_pitch;
  int Z, Y, X;
  float lambda, eps2;
  int z_chunk;
  double* stats;   // change, total of this launch (added to) or NULL
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline float tv_inv_norm(float dz, float dy, float dx, float eps2) {
  return 1.0f / sqrtf(((dz * dz + dy * dy) + dx * dx) + eps2);
}
__host__ __device__ inline float tv_scale(float v, float lambda, float pz, float pz_lo, float py, float py_lo, float px,
                                          float px_lo) {
  const float div = ((pz - pz_lo) + (py - py_lo)) + (px - px_lo);
  return v / (1.0f - lambda * div);
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

template <bool STATS>
__global__ __launch_bounds__(kThreads) void rl_tv_kernel(TvArgs p) {
  __shared__ __attribute__((aligned(16))) float lds[3 * kLdsPlane];
  const int tid = threadIdx.x;
  const int ly = tid / kColGroups, cg = tid % kColGroups;
  const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
  const int zb = blockIdx.z * p.z_chunk, ze = min(zb + p.z_chunk, p.Z);
  const int x = x0 + 4 * cg, y = y0 + ly;
  const int n_valid = y < p.Y ? max(0, min(4, p.X - x)) : 0;
  const int yc = min(y, p.Y - 1);                                      // (rows past Y stage a copy of the last one)

  // this thread's own four u of a plane ...
  const float* u_row = p.u + static_cast<int64_t>(yc) * p.u_pitch;
  const bool vec_u = x + 3 < p.X && ((reinterpret_cast<uintptr_t>(u_row + x) | (static_cast<uintptr_t>(p.u_plane) * 4)) & 15) == 0;
  const int xc0 = min(x, p.X - 1), xc1 = min(x + 1, p.X - 1), xc2 = min(x + 2, p.X - 1), xc3 = min(x + 3, p.X - 1);
  // ... and one element of the tile's rim: rows -1 and 16 (64 columns each), columns -1 and 64 (18 rows each)
  int hr = 0, hc = 0;
  const bool has_halo = tid < kHalo;
  if (tid < kTileX) { hr = -1; hc = tid; }
  else if (tid < 2 * kTileX) { hr = kTileY; hc = tid - kTileX; }
  else if (tid < 2 * kTileX + kLdsRows) { hr = tid - 2 * kTileX - 1; hc = -1; }
  else { hr = tid - 2 * kTileX - kLdsRows - 1; hc = kTileX; }
  const int64_t halo_off = static_cast<int64_t>(clampi(y0 + hr, p.Y - 1)) * p.u_pitch + clampi(x0 + hc, p.X - 1);
  const int halo_lds = (hr + 1) * kLdsPitch + kLdsCol0 + hc;
  const int own_lds = (ly + 1) * kLdsPitch + kLdsCol0 + 4 * cg;

  auto fetch = [&](int z, f32x4& own, float& rim) {
    const float* plane = p.u + static_cast<int64_t>(min(z, p.Z - 1)) * p.u_plane;
    const float* row = plane + static_cast<int64_t>(yc) * p.u_pitch;
    if (vec_u) own = *reinterpret_cast<const f32x4*>(row + x);
    else own = f32x4{row[xc0], row[xc1], row[xc2], row[xc3]};
    if (has_halo) rim = plane[halo_off];
  };
  auto stage = [&](int slot, const f32x4& own, float rim) {
    float* s = lds + slot * kLdsPlane;
    *reinterpret_cast<f32x4*>(s + own_lds) = own;
    if (has_halo) s[halo_lds] = rim;
  };

  // v and out: one 16-byte access where the row allows it
  const float* v_row = p.v + static_cast<int64_t>(yc) * p.v_pitch + x;
  float* o_row = p.out + static_cast<int64_t>(yc) * p.o_pitch + x;
  const bool vec_v = n_valid == 4 && ((reinterpret_cast<uintptr_t>(v_row) | (static_cast<uintptr_t>(p.v_plane) * 4)) & 15) == 0;
  const bool vec_o = n_valid == 4 && ((reinterpret_cast<uintptr_t>(o_row) | (static_cast<uintptr_t>(p.o_plane) * 4)) & 15) == 0;

  // a chunk that starts inside the volume runs plane zb - 1 first, for its p_z only
  const int ks = max(zb - 1, 0);
  f32x4 own;
  float rim = 0.0f;
  int sa = 0, sb = 1, sc = 2;             // LDS slots of planes k, k + 1, k + 2
  fetch(ks, own, rim);
  stage(sa, own, rim);
  fetch(ks + 1, own, rim);
  stage(sb, own, rim);
  __syncthreads();

  f32x4 pz_lo = {0.0f, 0.0f, 0.0f, 0.0f};   // p_z(k - 1): 0 below the volume
  float change = 0.0f, total = 0.0f;
  for (int k = ks; k < ze; ++k) {
    const bool more = k + 1 < ze;
    if (more) fetch(k + 2, own, rim);       // in flight during this plane's arithmetic
    const bool emit = k >= zb;
    f32x4 vv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (emit && n_valid > 0) {
      const float* vp = v_row + static_cast<int64_t>(k) * p.v_plane;
      if (vec_v) vv = *reinterpret_cast<const f32x4*>(vp);
      else {
        vv.x = vp[0];
        if (n_valid > 1) vv.y = vp[1];
        if (n_valid > 2) vv.z = vp[2];
        if (n_valid > 3) vv.w = vp[3];
      }
    }
    const float* a = lds + sa * kLdsPlane + own_lds;   // plane k at (y, x)
    const float* b = lds + sb * kLdsPlane + own_lds;   // plane k + 1
    const f32x4 cen4 = *reinterpret_cast<const f32x4*>(a);
    const f32x4 abv4 = *reinterpret_cast<const f32x4*>(a - kLdsPitch);
    const f32x4 blw4 = *reinterpret_cast<const f32x4*>(a + kLdsPitch);
    const f32x4 nxt4 = *reinterpret_cast<const f32x4*>(b);
    const f32x4 nab4 = *reinterpret_cast<const f32x4*>(b - kLdsPitch);
    const float cen[6] = {a[-1], cen4.x, cen4.y, cen4.z, cen4.w, a[4]};             // x - 1 .. x + 4
    const float abv[5] = {abv4.x, abv4.y, abv4.z, abv4.w, a[4 - kLdsPitch]};        // row y - 1: x .. x + 4
    const float blw[5] = {a[kLdsPitch - 1], blw4.x, blw4.y, blw4.z, blw4.w};        // row y + 1: x - 1 .. x + 3
    const float nxt[5] = {b[-1], nxt4.x, nxt4.y, nxt4.z, nxt4.w};                   // plane k + 1: x - 1 .. x + 3
    const float nab[4] = {nab4.x, nab4.y, nab4.z, nab4.w};                          // plane k + 1, row y - 1

    // p_x of the voxel to the left of the four
    float px_lo;
    {
      const float c = cen[0], dx = cen[1] - c;
      px_lo = dx * tv_inv_norm(nxt[0] - c, blw[0] - c, dx, p.eps2);
    }
    float o[4], pz[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float c = cen[i + 1];
      const float dz = nxt[i + 1] - c, dy = blw[i + 1] - c, dx = cen[i + 2] - c;
      const float inv = tv_inv_norm(dz, dy, dx, p.eps2);
      const float px = dx * inv, py = dy * inv;
      pz[i] = dz * inv;
      // p_y of the voxel above
      const float t = abv[i], ty = c - t;
      const float py_lo = ty * tv_inv_norm(nab[i] - t, ty, abv[i + 1] - t, p.eps2);
      o[i] = tv_scale(vv[i], p.lambda, pz[i], pz_lo[i], py, py_lo, px, px_lo);
      px_lo = px;
    }
    pz_lo = f32x4{pz[0], pz[1], pz[2], pz[3]};
    if (emit && n_valid > 0) {
      float* op = o_row + static_cast<int64_t>(k) * p.o_plane;
      if (vec_o) *reinterpret_cast<f32x4*>(op) = f32x4{o[0], o[1], o[2], o[3]};
      else {
        op[0] = o[0];
        if (n_valid > 1) op[1] = o[1];
        if (n_valid > 2) op[2] = o[2];
        if (n_valid > 3) op[3] = o[3];
      }
      if constexpr (STATS) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < n_valid) {
            change += __builtin_fabsf(o[i] - cen[i + 1]);
            total += o[i];
          }
      }
    }
    if (more) stage(sc, own, rim);
    __syncthreads();   // plane k + 2 is staged; every read of plane k (the slot plane k + 3 will take) is done
    const int t = sa;
    sa = sb; sb = sc; sc = t;
  }
  if constexpr (STATS) {
    // the RL epilogues' scheme (correlate_common.hpp): wave reduction -> LDS -> one f64 atomic per workgroup and sum
    const float c = lsr::wave_sum(change), t = lsr::wave_sum(total);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) {          // (behind the loop's last barrier: the planes are dead)
      lds[2 * wave] = c;
      lds[2 * wave + 1] = t;
    }
    __syncthreads();
    if (tid < 2) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < kThreads / 64; ++w) s += static_cast<double>(lds[2 * w + tid]);
      unsafeAtomicAdd(p.stats + tid, s);
    }
  }
}

// what both entries refuse; `end_*` = one past the last element a volume touches
int check_tv(const float* u, int64_t u_pitch, int64_t u_plane, const float* v, int64_t v_pitch, int64_t v_plane,
             const float* out, int64_t o_pitch, int64_t o_plane, int64_t Z, int64_t Y, int64_t X, float lambda,
             float tv_eps) {
  LSR_REQUIRE_PTR(u);
  LSR_REQUIRE_PTR(v);
  LSR_REQUIRE_PTR(out);
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  LSR_REQUIRE_STRIDES(u_pitch, u_plane);
  LSR_REQUIRE_STRIDES(v_pitch, v_plane);
  LSR_REQUIRE_STRIDES(o_pitch, o_plane);
  LSR_REQUIRE(u_pitch >= X && v_pitch >= X && o_pitch >= X, LSR_E_SHAPE, "a row stride is smaller than X");
  LSR_REQUIRE(Z == 1 || (u_plane >= (Y - 1) * u_pitch + X && v_plane >= (Y - 1) * v_pitch + X &&
                         o_plane >= (Y - 1) * o_pitch + X),
              LSR_E_SHAPE, "a plane stride is smaller than the rows it holds");
  // (!(a >= b) also catches NaN)
  LSR_REQUIRE(lambda >= 0.0f && lambda < 1.0f / 6.0f, LSR_E_ARG,
              "lambda = %g must be in [0, 1/6): |div| <= 6, the denominator 1 - lambda * div must stay positive",
              static_cast<double>(lambda));
  LSR_REQUIRE(tv_eps > 0.0f && tv_eps * tv_eps > 0.0f && std::isfinite(tv_eps * tv_eps), LSR_E_ARG,
              "tv_eps = %g must be > 0 with a square that float32 holds", static_cast<double>(tv_eps));
  const float* u_end = u + (Z - 1) * u_plane + (Y - 1) * u_pitch + X;
  const float* o_end = out + (Z - 1) * o_plane + (Y - 1) * o_pitch + X;
  LSR_REQUIRE(o_end <= u || u_end <= out, LSR_E_ARG,
              "out overlaps u: every voxel reads its neighbours' u (out may alias v, never u)");
  return LSR_OK;
}

}  // namespace

extern "C" int lsr_rl_tv_scale_f32(const float* u, int64_t u_pitch, int64_t u_plane, const float* v, int64_t v_pitch,
                                   int64_t v_plane, float* out, int64_t o_pitch, int64_t o_plane, int64_t Z, int64_t Y,
                                   int64_t X, float lambda, float tv_eps, double* stats2, lsr_stream_t stream) {
  if (int rc = check_tv(u, u_pitch, u_plane, v, v_pitch, v_plane, out, o_pitch, o_plane, Z, Y, X, lambda, tv_eps)) return rc;
  const int64_t tiles_x = lsr::ceil_div(X, kTileX), tiles_y = lsr::ceil_div(Y, kTileY);
  LSR_REQUIRE(tiles_y < 65536, LSR_E_UNSUPPORTED, "Y = %lld: this kernel's grid takes fewer than %d rows", (long long)Y,
              65536 * kTileY);
  TvArgs p{};
  p.u = u; p.v = v; p.out = out;
  p.u_plane = u_plane; p.v_plane = v_plane; p.o_plane = o_plane;
  p.u_pitch = static_cast<int>(u_pitch); p.v_pitch = static_cast<int>(v_pitch); p.o_pitch = static_cast<int>(o_pitch);
  p.Z = static_cast<int>(Z); p.Y = static_cast<int>(Y); p.X = static_cast<int>(X);
  p.lambda = lambda;
  p.eps2 = tv_eps * tv_eps;
  p.stats = stats2;
  // whole z columns where the tiles alone fill the chip several times over; otherwise z chunks (each re-reads two planes
  // and recomputes one), as few as it takes and never shorter than 24 planes
  int64_t chunks = lsr::ceil_div(int64_t(256) * 32, tiles_x * tiles_y);
  int64_t chunk = lsr::ceil_div(Z, chunks);
  if (chunk < 24) chunk = 24;
  if (chunk > Z) chunk = Z;
  p.z_chunk = static_cast<int>(chunk);
  const int64_t gz = lsr::ceil_div(Z, chunk);
  LSR_REQUIRE(gz < 65536, LSR_E_SHAPE, "grid of %lld z chunks is too large", (long long)gz);
  const dim3 grid(static_cast<unsigned>(tiles_x), static_cast<unsigned>(tiles_y), static_cast<unsigned>(gz));
  hipStream_t s = lsr::as_stream(stream);
  if (stats2 != nullptr) hipLaunchKernelGGL(rl_tv_kernel<true>, grid, dim3(kThreads), 0, s, p);
  else hipLaunchKernelGGL(rl_tv_kernel<false>, grid, dim3(kThreads), 0, s, p);
  return lsr::launch_status("lsr_rl_tv_scale_f32");
}

// The host twin: the same inline functions on the same clamped neighbourhood, one row at a time (the three norms a voxel
// needs beside its own are recomputed, as in the kernel); rows are split over the worker threads, the two sums are f64
// per row range and added in range order.
extern "C" int lsr_rl_tv_scale_f32_cpu(const float* u, int64_t u_pitch, int64_t u_plane, const float* v, int64_t v_pitch,
                                       int64_t v_plane, float* out, int64_t o_pitch, int64_t o_plane, int64_t Z,
                                       int64_t Y, int64_t X, float lambda, float tv_eps, double* stats2) {
  if (int rc = check_tv(u, u_pitch, u_plane, v, v_pitch, v_plane, out, o_pitch, o_plane, Z, Y, X, lambda, tv_eps)) return rc;
  const float eps2 = tv_eps * tv_eps;
  double part[2 * 1024];   // (parallel_ranges_indexed: at most 1024 ranges)
  const int used = lsr::parallel_ranges_indexed(Z * Y, [&](int rank, int64_t r_first, int64_t r_last) {
    double change = 0.0, total = 0.0;
    for (int64_t zy = r_first; zy < r_last; ++zy) {
      const int64_t z = zy / Y, y = zy - z * Y;
      const int64_t zl = z > 0 ? z - 1 : 0, zh = z + 1 < Z ? z + 1 : Z - 1;
      const int64_t yl = y > 0 ? y - 1 : 0, yh = y + 1 < Y ? y + 1 : Y - 1;
      auto row = [&](int64_t zz, int64_t yy) { return u + zz * u_plane + yy * u_pitch; };
      const float* c_row = row(z, y);        // the voxel's own row, the rows its differences reach ...
      const float* c_zh = row(zh, y);
      const float* c_yh = row(z, yh);
      const float* a_row = row(z, yl);       // ... the row above and what ITS differences reach ...
      const float* a_zh = row(zh, yl);
      const float* b_row = row(zl, y);       // ... and the row in the plane below (its z neighbour is c_row)
      const float* b_yh = row(zl, yh);
      const float* vr = v + z * v_plane + y * v_pitch;
      float* orow = out + z * o_plane + y * o_pitch;
      float px_lo = 0.0f;
      for (int64_t x = 0; x < X; ++x) {
        const int64_t xh = x + 1 < X ? x + 1 : X - 1;
        const float c = c_row[x];
        const float dz = c_zh[x] - c, dy = c_yh[x] - c, dx = c_row[xh] - c;
        const float inv = tv_inv_norm(dz, dy, dx, eps2);
        const float px = dx * inv, py = dy * inv, pz = dz * inv;
        const float t = a_row[x], ty = c - t;
        const float py_lo = ty * tv_inv_norm(a_zh[x] - t, ty, a_row[xh] - t, eps2);
        const float w = b_row[x], wz = c - w;
        const float pz_lo = wz * tv_inv_norm(wz, b_yh[x] - w, b_row[xh] - w, eps2);
        const float o = tv_scale(vr[x], lambda, pz, pz_lo, py, py_lo, px, px_lo);
        orow[x] = o;
        px_lo = px;
        change += std::fabs(static_cast<double>(o) - static_cast<double>(c));
        total += o;
      }
    }
    part[2 * rank] = change;
    part[2 * rank + 1] = total;
  });
  if (stats2 != nullptr)
    for (int k = 0; k < used; ++k) {
      stats2[0] += part[2 * k];
      stats2[1] += part[2 * k + 1];
    }
  return LSR_OK;
}
