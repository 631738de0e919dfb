// Accelerated Richardson-Lucy: the vector extrapolation of Biggs & Andrews (Appl. Opt. 36, 1997) around the unchanged
// RL launches.  With RL(.) one plain iteration, d the data and x_0 the start:
//
//     p_0 = x_0
//     for k = 0 .. K-1:
//         x_{k+1} = RL(p_k)                                   the plan's own launches
//         if k == K-1: stop
//         g_k     = x_{k+1} - p_k                             lsr_rl_accel_dots_f32 (float32 subtraction), which also
//         <g_k, g_{k-1}>, <g_k, g_k>                          leaves the two inner products in device memory
//         a_{k+1} = 0 for k == 0, else clamp(<g_k, g_{k-1}> / <g_{k-1}, g_{k-1}>, 0, 1), 0 for a zero denominator
//         p_{k+1} = max(fma(a_{k+1}, x_{k+1} - x_k, x_{k+1}), 0)    lsr_rl_accel_predict_f32, a_{k+1} formed on the device
//     return x_K
//
// Every step starts from a point extrapolated along the last change, with a step length taken from the last two
// changes; no tuning parameter, no host round trip.  Two streaming launches per iteration:
//
//   dots     reads x_{k+1}, p_k (strided) and g_{k-1} (dense), writes g_k over g_{k-1}: 16 bytes per voxel.  The inner
//            products are float64 sums of float64 products (exact: 24 x 24 bits) from the first add.  They feed back
//            into the result, so they must not depend on scheduling: every thread adds its voxels in a fixed order, the
//            workgroup adds its threads in a fixed tree and STORES its two partial sums; a one-workgroup kernel behind it
//            adds the partial sums in index order.  No floating-point atomics.  The number of workgroups depends on the
//            shape alone (rl_accel.hpp: parts_of).
//   predict  reads x_{k+1}, x_k (strided) and the two inner products, writes p_{k+1} over x_k: 12 bytes per voxel.  Only
//            the logical volume is touched: the zero halo of a padded working volume stays zero.
//
// Shape of both: a workgroup of 256 threads takes a row (z, y) at a time and strides over the rows.  A row's body is
// moved 16 bytes per lane; the body starts where the WRITTEN stream (g; x_k) is 16-byte aligned, the elements in front of
// it and behind the last whole vector are moved one by one.  The read streams are then aligned too whenever they share
// the written stream's alignment -- padded working volumes among each other always do; a dense g against a padded volume
// does not when X is not a multiple of 4, and those 16-byte reads start on a 4-byte boundary (the hardware takes them; a
// wave's 1 KiB then touches nine 128-byte lines instead of eight).
//
// The host twins (host_twins.hip) run the same inline functions (rl_accel.hpp): g and p are the kernels' bits.

#include "common.hpp"
#include "rl_accel.hpp"

namespace {

namespace ac = lsr::accel;

constexpr int kThreads = 256;

// 16 bytes per lane at any 4-byte boundary
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

struct RowWalk {       // how a workgroup walks the rows: start at row blockIdx.x, step gridDim.x rows
  int Y, X;
  int step_z, step_y;  // gridDim.x = step_z * Y + step_y
  int64_t rows;
};

struct DotsArgs {
  const float* x1;
  const float* p;
  float* g;
  int64_t x1_plane, p_plane;
  int x1_pitch, p_pitch;
  RowWalk w;
  double* parts;       // [gridDim.x][2]
};

struct PredictArgs {
  const float* x1;
  float* x0;
  int64_t x1_plane, x0_plane;
  int x1_pitch, x0_pitch;
  RowWalk w;
  const double* num;   // <g_k, g_{k-1}>
  const double* den;   // <g_{k-1}, g_{k-1}>
  double* alpha;       // receives a_{k+1}, or NULL
};

// a row of X elements whose written stream starts at `dst`: [0, head) one by one, nq vectors, [tail0, X) one by one
struct RowSplit {
  int head, nq, tail0;
  __device__ RowSplit(const float* dst, int X) {
    head = static_cast<int>((0u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(dst) >> 2)) & 3u);
    if (head > X) head = X;
    nq = (X - head) >> 2;
    tail0 = head + 4 * nq;
  }
  // the element thread `tid` moves on its own, or -1 (at most 3 in front and 3 behind)
  __device__ int loose(int tid, int X) const {
    if (tid < head) return tid;
    const int e = tail0 + (tid - head);
    return e < X ? e : -1;
  }
};

// the workgroup's sum of `a` and of `b`, added in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*lds)[kThreads]) {
  const int tid = threadIdx.x;
  lds[0][tid] = a;
  lds[1][tid] = b;
  __syncthreads();
#pragma unroll
  for (int o = kThreads / 2; o >= 1; o >>= 1) {
    if (tid < o) {
      lds[0][tid] += lds[0][tid + o];
      lds[1][tid] += lds[1][tid + o];
    }
    __syncthreads();
  }
  a = lds[0][0];
  b = lds[1][0];
}

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void rl_accel_dots_kernel(DotsArgs a) {
  __shared__ double lds[2][kThreads];
  const int tid = threadIdx.x;
  const int X = a.w.X, Y = a.w.Y;
  double s_gh = 0.0, s_gg = 0.0;     // <g_k, g_{k-1}>, <g_k, g_k>
  int z = static_cast<int>(blockIdx.x) / Y, y = static_cast<int>(blockIdx.x) % Y;
  for (int64_t r = blockIdx.x; r < a.w.rows; r += gridDim.x) {
    const float* __restrict__ x1 = a.x1 + z * a.x1_plane + static_cast<int64_t>(y) * a.x1_pitch;
    const float* __restrict__ p = a.p + z * a.p_plane + static_cast<int64_t>(y) * a.p_pitch;
    float* __restrict__ g = a.g + r * X;
    const RowSplit s(g, X);
    const int e = s.loose(tid, X);
    if (e >= 0) {
      const float gk = ac::change_of(x1[e], p[e]);
      if (!FIRST) s_gh += static_cast<double>(gk) * static_cast<double>(g[e]);
      s_gg += static_cast<double>(gk) * static_cast<double>(gk);
      g[e] = gk;
    }
    for (int q = tid; q < s.nq; q += kThreads) {
      const int o = s.head + 4 * q;
      const f32x4u a4 = *reinterpret_cast<const f32x4u*>(x1 + o);
      const f32x4u b4 = *reinterpret_cast<const f32x4u*>(p + o);
      f32x4u h4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!FIRST) h4 = *reinterpret_cast<const f32x4u*>(g + o);
      f32x4u g4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g4[i] = ac::change_of(a4[i], b4[i]);
        if (!FIRST) s_gh += static_cast<double>(g4[i]) * static_cast<double>(h4[i]);
        s_gg += static_cast<double>(g4[i]) * static_cast<double>(g4[i]);
      }
      *reinterpret_cast<f32x4u*>(g + o) = g4;
    }
    z += a.w.step_z;
    y += a.w.step_y;
    if (y >= Y) {
      y -= Y;
      ++z;
    }
  }
  block_sum2(s_gh, s_gg, lds);
  if (tid == 0) {
    a.parts[2 * blockIdx.x] = s_gh;
    a.parts[2 * blockIdx.x + 1] = s_gg;
  }
}

// one workgroup: thread t adds parts t, t + 256, ... in that order, the threads are added in block_sum2's tree
__global__ __launch_bounds__(kThreads) void rl_accel_finish_kernel(const double* parts, int n, double* dots2) {
  __shared__ double lds[2][kThreads];
  double s_gh = 0.0, s_gg = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    s_gh += parts[2 * i];
    s_gg += parts[2 * i + 1];
  }
  block_sum2(s_gh, s_gg, lds);
  if (threadIdx.x == 0) {
    dots2[0] = s_gh;
    dots2[1] = s_gg;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(kThreads) void rl_accel_predict_kernel(PredictArgs a) {
  const int tid = threadIdx.x;
  const int X = a.w.X, Y = a.w.Y;
  float alpha = 0.0f;
  if (!FIRST) alpha = ac::step_length(*a.num, *a.den);
  if (a.alpha != nullptr && blockIdx.x == 0 && tid == 0) *a.alpha = static_cast<double>(alpha);
  int z = static_cast<int>(blockIdx.x) / Y, y = static_cast<int>(blockIdx.x) % Y;
  for (int64_t r = blockIdx.x; r < a.w.rows; r += gridDim.x) {
    const float* __restrict__ x1 = a.x1 + z * a.x1_plane + static_cast<int64_t>(y) * a.x1_pitch;
    float* __restrict__ x0 = a.x0 + z * a.x0_plane + static_cast<int64_t>(y) * a.x0_pitch;
    const RowSplit s(x0, X);
    const int e = s.loose(tid, X);
    if (e >= 0) x0[e] = FIRST ? ac::predict_first(x1[e]) : ac::predict_of(alpha, x1[e], x0[e]);
    for (int q = tid; q < s.nq; q += kThreads) {
      const int o = s.head + 4 * q;
      const f32x4u a4 = *reinterpret_cast<const f32x4u*>(x1 + o);
      f32x4u b4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!FIRST) b4 = *reinterpret_cast<const f32x4u*>(x0 + o);
      f32x4u p4;
#pragma unroll
      for (int i = 0; i < 4; ++i) p4[i] = FIRST ? ac::predict_first(a4[i]) : ac::predict_of(alpha, a4[i], b4[i]);
      *reinterpret_cast<f32x4u*>(x0 + o) = p4;
    }
    z += a.w.step_z;
    y += a.w.step_y;
    if (y >= Y) {
      y -= Y;
      ++z;
    }
  }
}

RowWalk walk(int64_t Z, int64_t Y, int64_t X, int64_t grid) {
  RowWalk w{};
  w.Y = static_cast<int>(Y);
  w.X = static_cast<int>(X);
  w.step_z = static_cast<int>(grid / Y);
  w.step_y = static_cast<int>(grid % Y);
  w.rows = Z * Y;
  return w;
}

}  // namespace

extern "C" int lsr_rl_accel_workspace_bytes(int64_t Z, int64_t Y, int64_t X) {
  if (int rc = ac::check_shape(Z, Y, X)) return rc;
  return static_cast<int>(ac::parts_of(Z * Y) * 2 * sizeof(double));
}

extern "C" int lsr_rl_accel_dots_f32(const float* x1, int64_t x1_pitch, int64_t x1_plane, const float* p, int64_t p_pitch,
                                     int64_t p_plane, float* g, int64_t Z, int64_t Y, int64_t X, int first, double* dots2,
                                     void* workspace, lsr_stream_t stream) {
  const ac::Vol vx{x1, x1_pitch, x1_plane}, vp{p, p_pitch, p_plane};
  if (int rc = ac::check_dots(vx, vp, g, dots2, Z, Y, X)) return rc;
  LSR_REQUIRE_PTR(workspace);
  LSR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(dots2) & 7) == 0, LSR_E_ARG,
              "workspace and dots2 must be 8-byte aligned");
  const int64_t grid = ac::parts_of(Z * Y);
  DotsArgs a{};
  a.x1 = x1; a.p = p; a.g = g;
  a.x1_plane = x1_plane; a.p_plane = p_plane;
  a.x1_pitch = static_cast<int>(x1_pitch); a.p_pitch = static_cast<int>(p_pitch);
  a.w = walk(Z, Y, X, grid);
  a.parts = static_cast<double*>(workspace);
  hipStream_t s = lsr::as_stream(stream);
  if (first) hipLaunchKernelGGL(rl_accel_dots_kernel<true>, dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(rl_accel_dots_kernel<false>, dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(rl_accel_finish_kernel, dim3(1), dim3(kThreads), 0, s, a.parts, static_cast<int>(grid), dots2);
  return lsr::launch_status("lsr_rl_accel_dots_f32");
}

extern "C" int lsr_rl_accel_predict_f32(const float* x1, int64_t x1_pitch, int64_t x1_plane, float* x0, int64_t x0_pitch,
                                        int64_t x0_plane, int64_t Z, int64_t Y, int64_t X, const double* num,
                                        const double* den, double* alpha_out, lsr_stream_t stream) {
  const ac::Vol vx{x1, x1_pitch, x1_plane}, v0{x0, x0_pitch, x0_plane};
  if (int rc = ac::check_predict(vx, v0, Z, Y, X)) return rc;
  LSR_REQUIRE(den == nullptr || num != nullptr, LSR_E_NULL, "num is NULL although den is not (den == NULL: the first step)");
  LSR_REQUIRE(((reinterpret_cast<uintptr_t>(num) | reinterpret_cast<uintptr_t>(den) | reinterpret_cast<uintptr_t>(alpha_out)) & 7) == 0,
              LSR_E_ARG, "num, den and alpha_out must be 8-byte aligned");
  const int64_t grid = ac::parts_of(Z * Y);
  PredictArgs a{};
  a.x1 = x1; a.x0 = x0;
  a.x1_plane = x1_plane; a.x0_plane = x0_plane;
  a.x1_pitch = static_cast<int>(x1_pitch); a.x0_pitch = static_cast<int>(x0_pitch);
  a.w = walk(Z, Y, X, grid);
  a.num = num; a.den = den; a.alpha = alpha_out;
  hipStream_t s = lsr::as_stream(stream);
  if (den == nullptr) hipLaunchKernelGGL(rl_accel_predict_kernel<true>, dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(rl_accel_predict_kernel<false>, dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s, a);
  return lsr::launch_status("lsr_rl_accel_predict_f32");
}
