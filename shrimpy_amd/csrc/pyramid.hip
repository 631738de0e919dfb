// 2x mean downsampling of a volume: one level of a multiscale pyramid from the level above it (shrimpy_amd/pyramid.py;
// iohub's compute_pyramid is not vendored -- PARITY UNPINNED, the rule is defined in pyramid.hpp and restated in
// tests/pyramid_ref.py).  Factors (fz, 2, 2), fz in {1, 2}; partial windows at the far faces average what is there.
//
// A streaming kernel: 4 bytes read and 0.5 written per input voxel at fz = 2, no reuse, no LDS.  A lane owns FOUR
// consecutive outputs of one output row, i.e. eight consecutive inputs of each of the (up to) four input rows under it:
// 32 bytes per row and lane, consecutive lanes consecutive 32-byte pieces, so a wavefront reads 2 KB runs of each row
// and writes one 1 KB run.  A row starts wherever its pitch of X elements puts it: a piece on a 16-byte boundary is two
// 16-byte loads, any other is cut out of the three aligned 16-byte words that hold it (at the very ends of the volume,
// where such a word would reach outside: 8-, 4-byte or element loads); the stores take the widest form their address
// allows.  The choice is the same for every lane of a row.  The piece at the end of a row, when it holds fewer than
// eight inputs, goes element by element with bounds checks: nothing outside the volume is read or written.  Work items (row, piece) are numbered in 64 bits and walked with a
// grid stride, so a level of any size is one launch.

#include <algorithm>

#include "pyramid.hpp"

namespace {

namespace py = lsr::pyramid;

constexpr int kThreads = 256;
constexpr int kOut = 4;                 // outputs per lane along x
constexpr int kIn = 2 * kOut;           // inputs per lane and input row
constexpr int64_t kMaxBlocks = 4096;    // 16 per CU: the rest of a large level is walked with the grid stride

template <typename V, typename T>
__device__ __forceinline__ void load_as(const T* p, T (&v)[kIn]) {
  constexpr int n = kIn * sizeof(T) / sizeof(V);
  V t[n];
#pragma unroll
  for (int i = 0; i < n; ++i) t[i] = reinterpret_cast<const V*>(p)[i];
  __builtin_memcpy(v, t, sizeof(t));
}

// eight consecutive elements, all inside the volume [lo, hi).  A piece that starts off a 16-byte boundary is cut out of
// the aligned 16-byte words around it -- one word more than the piece has, still wide loads, and the neighbouring lanes
// want the same words -- whenever those words lie inside the volume too; the phase is the same for every lane of a row.
template <typename T>
__device__ __forceinline__ void load_piece(const T* p, T (&v)[kIn], const T* lo, const T* hi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  constexpr int kPerWord = 16 / sizeof(T), kWords = kIn / kPerWord + 1;
  const uintptr_t first = a & ~uintptr_t(15);
  if ((a & 15) == 0) {
    load_as<uint4>(p, v);
  } else if (first >= reinterpret_cast<uintptr_t>(lo) && first + 16 * kWords <= reinterpret_cast<uintptr_t>(hi)) {
    uint4 w[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = reinterpret_cast<const uint4*>(first)[i];
    T wide[kWords * kPerWord];
    __builtin_memcpy(wide, w, sizeof(w));
    const int shift = static_cast<int>(a & 15) / static_cast<int>(sizeof(T));
#pragma unroll
    for (int c = 1; c < kPerWord; ++c) {
      if (shift == c) {
#pragma unroll
        for (int i = 0; i < kIn; ++i) v[i] = wide[i + c];
      }
    }
  } else if ((a & 7) == 0) {
    load_as<uint2>(p, v);
  } else if ((a & 3) == 0) {
    load_as<uint32_t>(p, v);
  } else {
#pragma unroll
    for (int i = 0; i < kIn; ++i) v[i] = p[i];
  }
}

template <typename V, typename T>
__device__ __forceinline__ void store_as(T* p, const T (&v)[kOut]) {
  constexpr int n = kOut * sizeof(T) / sizeof(V);
  V t[n];
  __builtin_memcpy(t, v, sizeof(t));
#pragma unroll
  for (int i = 0; i < n; ++i) reinterpret_cast<V*>(p)[i] = t[i];
}

// four consecutive outputs, all inside the output row
template <typename T>
__device__ __forceinline__ void store_piece(T* p, const T (&v)[kOut]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if constexpr (kOut * sizeof(T) >= 16) {
    if ((a & 15) == 0) {
      store_as<uint4>(p, v);
      return;
    }
  }
  if ((a & 7) == 0) {
    store_as<uint2>(p, v);
  } else if (sizeof(T) < 4 && (a & 3) == 0) {
    store_as<uint32_t>(p, v);
  } else {
#pragma unroll
    for (int i = 0; i < kOut; ++i) p[i] = v[i];
  }
}

// a / b for 0 <= a, 0 < b: one 32-bit division wherever both fit (every level of a config-2 volume)
__device__ __forceinline__ int64_t div_small(int64_t a, int64_t b) {
  return ((a | b) >> 32) == 0 ? static_cast<int64_t>(static_cast<uint32_t>(a) / static_cast<uint32_t>(b)) : a / b;
}

template <typename T>
struct Args {
  const T* in;
  const T* in_end;      // in + Z * Y * X
  T* out;
  int64_t Y, X;         // input rows per plane, row length
  int64_t Z;
  int64_t Yo, Xo;       // output
  int64_t pieces;       // ceil(Xo / 4) per output row
  int64_t items;        // Zo * Yo * pieces
  int fz;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void downsample2_kernel(Args<T> p) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; item < p.items; item += stride) {
    const int64_t row = div_small(item, p.pieces), g = item - row * p.pieces;
    const int64_t zo = div_small(row, p.Yo), yo = row - zo * p.Yo;
    const int64_t z0 = zo * p.fz, y0 = 2 * yo, xb = kIn * g;
    const bool hz = p.fz == 2 && z0 + 1 < p.Z, hy = y0 + 1 < p.Y;
    const int n_in = static_cast<int>(min(static_cast<int64_t>(kIn), p.X - xb));
    const int n_out = static_cast<int>(min(static_cast<int64_t>(kOut), p.Xo - kOut * g));
    const T* src = p.in + (z0 * p.Y + y0) * p.X + xb;
    const int64_t plane = p.Y * p.X;

    T v[2][2][kIn];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const bool have = (a == 0 || hz) && (b == 0 || hy);
        const T* q = src + a * plane + b * p.X;
        if (have && n_in == kIn) {
          load_piece(q, v[a][b], p.in, p.in_end);
        } else {
#pragma unroll
          for (int i = 0; i < kIn; ++i) v[a][b][i] = (have && i < n_in) ? q[i] : T(0);
        }
      }
    }

    T o[kOut];
#pragma unroll
    for (int j = 0; j < kOut; ++j) {
      const bool hx = 2 * j + 1 < n_in;
      const int k = static_cast<int>(hx) + static_cast<int>(hy) + static_cast<int>(hz);
      o[j] = py::finish(py::pair(v[0][0][2 * j], v[0][0][2 * j + 1], hx), py::pair(v[0][1][2 * j], v[0][1][2 * j + 1], hx),
                        py::pair(v[1][0][2 * j], v[1][0][2 * j + 1], hx), py::pair(v[1][1][2 * j], v[1][1][2 * j + 1], hx),
                        hy, hz, k);
    }
    T* dst = p.out + row * p.Xo + kOut * g;
    if (n_out == kOut) {
      store_piece(dst, o);
    } else {
#pragma unroll
      for (int j = 0; j < kOut; ++j)
        if (j < n_out) dst[j] = o[j];
    }
  }
}

template <typename T>
int launch(const T* in, int64_t Z, int64_t Y, int64_t X, T* out, int fz, lsr_stream_t stream, const char* what) {
  if (int rc = py::check(in, Z, Y, X, out, fz)) return rc;
  Args<T> p{};
  p.in = in;
  p.in_end = in + Z * Y * X;
  p.out = out;
  p.Z = Z; p.Y = Y; p.X = X;
  p.Yo = py::out_extent(Y, 2);
  p.Xo = py::out_extent(X, 2);
  p.pieces = lsr::ceil_div(p.Xo, kOut);
  p.items = py::out_extent(Z, fz) * p.Yo * p.pieces;       // < 2^48: a volume in range has fewer voxels than that
  p.fz = fz;
  const int64_t blocks = std::min(lsr::ceil_div(p.items, kThreads), kMaxBlocks);
  hipLaunchKernelGGL(downsample2_kernel<T>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, lsr::as_stream(stream), p);
  return lsr::launch_status(what);
}

}  // namespace

extern "C" int lsr_downsample2_shape(int64_t Z, int64_t Y, int64_t X, int fz, int64_t out3[3]) {
  LSR_REQUIRE_PTR(out3);
  if (int rc = py::check_shape(Z, Y, X, fz)) return rc;
  out3[0] = py::out_extent(Z, fz);
  out3[1] = py::out_extent(Y, 2);
  out3[2] = py::out_extent(X, 2);
  return LSR_OK;
}

extern "C" int lsr_downsample2_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int fz, lsr_stream_t stream) {
  return launch<float>(in, Z, Y, X, out, fz, stream, "lsr_downsample2_f32");
}

extern "C" int lsr_downsample2_u16(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, uint16_t* out, int fz,
                                   lsr_stream_t stream) {
  return launch<uint16_t>(in, Z, Y, X, out, fz, stream, "lsr_downsample2_u16");
}
