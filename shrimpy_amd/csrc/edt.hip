// The exact Euclidean distance transform and the label expansion (shrimpy_amd/distance.py).  The rule is csrc/edt.hpp's; the
// distances' oracle is scipy.ndimage.distance_transform_edt, the indices' a brute-force search (tests/edt_ref.py).
//
// Three launches on the caller's stream, all working IN PLACE in one int32 word per voxel: `nearest` where it is asked for,
// else the words of `dist`.  The scratch holds nothing but the envelope stacks.
//
//   x   one wave per row, 64 voxels per step.  Forward: the site predicate is fused into the load (the mask is never
//       written), a ballot gives every lane the nearest site at or left of it, the row's last site so far is carried across
//       the steps; written to the work words.  Backward: the same words are read back (a voxel is a site iff its word is its
//       own x), a ballot and a carry give the nearest site at or right of it, and the nearer of the two is written (a tie
//       goes to the left), -1 in a row without a site.  4 B read + 4 B written per voxel, and the same again from L2.
//   y   one lane per (z, x) line, adjacent lanes on adjacent x: every plane-strided access is coalesced.  The lower envelope
//       of the line's parabolas (edt.hpp line_pass), then the line rewritten with y' * X + x' of each voxel's winner, -1 in a
//       plane without a site.  4 B read + 4 B written per voxel, plus the stack: 12 B written per entry that reaches it.
//   z   one lane per (y, x) line, the same pass along z; writes the linear index and, fused, the distance (either may be NULL).
//       4 B read + 4 B (or 8 B) written per voxel, plus the stack.
//
// A lane's stack is n entries of (position, value, first owned position), entry e's field f at word (e * 3 + f) * lanes +
// lane: adjacent lanes touch adjacent words.  Lanes beyond kMaxLanes stride over the lines and reuse their stack.
//
// No communication: every row and every line is independent, no launch reads a word another workgroup of the SAME launch
// writes, and no workgroup ever waits for another.  Both rules of label.hip hold trivially.

#include <algorithm>

#include "edt.hpp"

namespace {

namespace ed = lsr::edt;

constexpr int kThreads = 256;
static_assert(ed::kChunk == lsr::kWave, "a step of the x pass is one wavefront");
static_assert(ed::kRowsPerBlock * lsr::kWave == kThreads && ed::kLineTile == kThreads, "whole workgroups");

struct FloatSites {          // background of in > threshold (NaN is background), or with `invert` its foreground
  const float* in;
  float threshold;
  bool invert;
  __device__ __forceinline__ bool operator()(int64_t v) const { return !(in[v] > threshold) != invert; }
};

struct LabelSites {          // labels != 0, or with `invert` labels == 0
  const int32_t* labels;
  bool invert;
  __device__ __forceinline__ bool operator()(int64_t v) const { return (labels[v] != 0) != invert; }
};

// ---- x: the nearest site of the row ---------------------------------------------------------------------------------------------

template <class Sites>
__global__ __launch_bounds__(kThreads) void edt_x_kernel(Sites sites, int64_t rows, int X, int32_t* work) {
  const int lane = threadIdx.x % lsr::kWave, wave = threadIdx.x / lsr::kWave;
  const int chunks = static_cast<int>((static_cast<int64_t>(X) + ed::kChunk - 1) / ed::kChunk);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * ed::kRowsPerBlock + wave; row < rows;
       row += static_cast<int64_t>(gridDim.x) * ed::kRowsPerBlock) {           // (row: wave-uniform)
    int32_t* w = work + row * X;
    int carry = -1;                                                             // the last site of the chunks passed
    for (int c = 0; c < chunks; ++c) {
      const int64_t x = static_cast<int64_t>(c) * ed::kChunk + lane;
      const bool inside = x < X;
      const bool site = inside && sites(row * X + x);
      const unsigned long long mask = __ballot(site);
      const unsigned long long below = mask & ((2ull << lane) - 1ull);          // sites at or left of this lane (lane 63: all)
      const int left = below ? c * ed::kChunk + 63 - __clzll(static_cast<long long>(below)) : carry;
      if (inside) w[x] = left;
      if (mask) carry = c * ed::kChunk + 63 - __clzll(static_cast<long long>(mask));
    }
    carry = -1;                                                                 // the first site of the chunks passed
    for (int c = chunks - 1; c >= 0; --c) {
      const int64_t x = static_cast<int64_t>(c) * ed::kChunk + lane;
      const bool inside = x < X;
      const int left = inside ? w[x] : -1;                                      // (this thread's own store)
      const unsigned long long mask = __ballot(inside && left == static_cast<int>(x));
      const unsigned long long above = mask & (~0ull << lane);                   // sites at or right of this lane
      const int right = above ? c * ed::kChunk + __ffsll(static_cast<long long>(above)) - 1 : carry;
      if (inside) w[x] = ed::nearer_in_row(static_cast<int>(x), left, right);
      if (mask) carry = c * ed::kChunk + __ffsll(static_cast<long long>(mask)) - 1;
    }
  }
}

// ---- y and z: the lower envelope of a line ---------------------------------------------------------------------------------------

struct LaneStack {
  int32_t* base;             // this lane's word of entry 0, field 0
  int64_t lanes;
  __device__ __forceinline__ void put(int q, int k, int v, int t) {
    int32_t* e = base + static_cast<int64_t>(q) * ed::kStackFields * lanes;
    e[0] = k;
    e[lanes] = v;
    e[2 * lanes] = t;
  }
  __device__ __forceinline__ void get(int q, int& k, int& v, int& t) const {
    const int32_t* e = base + static_cast<int64_t>(q) * ed::kStackFields * lanes;
    k = e[0];
    v = e[lanes];
    t = e[2 * lanes];
  }
};

__global__ __launch_bounds__(kThreads) void edt_y_kernel(int32_t* work, int Z, int Y, int X, double wy, double wx, int32_t* stacks) {
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * kThreads, lane = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t lines = static_cast<int64_t>(Z) * X, plane = static_cast<int64_t>(Y) * X;
  LaneStack stack{stacks + lane, lanes};
  for (int64_t line = lane; line < lines; line += lanes) {
    const int z = static_cast<int>(line / X), x = static_cast<int>(line % X);
    ed::YLine io{work + z * plane + x, X, x, X, wx};
    ed::line_pass(Y, wy, io, stack);
  }
}

__global__ __launch_bounds__(kThreads) void edt_z_kernel(int32_t* work, int32_t* nearest, int32_t* dist, int Z, int Y, int X,
                                                         ed::Sampling s, int32_t* stacks) {
  const int64_t lanes = static_cast<int64_t>(gridDim.x) * kThreads, lane = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t plane = static_cast<int64_t>(Y) * X;
  LaneStack stack{stacks + lane, lanes};
  for (int64_t line = lane; line < plane; line += lanes) {
    ed::ZLine io{work + line, nearest != nullptr ? nearest + line : nullptr, dist != nullptr ? dist + line : nullptr, plane,
                 static_cast<int>(line / X), static_cast<int>(line % X), X, s};
    ed::line_pass(Z, s.wz, io, stack);
  }
}

// ---- label expansion: one gather ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void label_expand_kernel(const int32_t* __restrict__ labels, const int32_t* nearest, int Y,
                                                                int X, int64_t n, ed::Sampling s, double distance, int32_t* out) {
  const unsigned plane = static_cast<unsigned>(Y) * static_cast<unsigned>(X);      // (< 2^31: the volume is)
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; v < n; v += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int site = nearest[v];
    int label = 0;
    if (site >= 0 && site < n) {                                                    // (never a read outside the volume)
      const unsigned uv = static_cast<unsigned>(v);
      const int z = static_cast<int>(uv / plane), y = static_cast<int>(uv % plane / static_cast<unsigned>(X)),
                x = static_cast<int>(uv % plane % static_cast<unsigned>(X));
      if (ed::distance_to(s, z, y, x, site, Y, X) <= distance) label = labels[site];
    }
    out[v] = label;
  }
}

constexpr int64_t kMaxBlocks = 1 << 16;      // grid-stride launches: 256 per CU
constexpr int kLaunches = 3;                 // x, y, z

// The three launches; a timing entry's marks (kLaunches + 1 events) get one in front of each launch and one behind the last.
template <class Sites>
int edt_launches(Sites sites, int64_t Z, int64_t Y, int64_t X, const double* sampling, float* dist, int32_t* nearest, void* scratch,
                 hipStream_t q, lsr::LaunchMarks marks, const char* what) {
  const ed::Sampling s = ed::make_sampling(sampling);
  int32_t* work = nearest != nullptr ? nearest : reinterpret_cast<int32_t*>(dist);
  int32_t* stacks = static_cast<int32_t*>(scratch);
  const int iZ = static_cast<int>(Z), iY = static_cast<int>(Y), iX = static_cast<int>(X);
  marks.mark();
  hipLaunchKernelGGL(edt_x_kernel<Sites>, dim3(static_cast<unsigned>(std::min(lsr::ceil_div(Z * Y, ed::kRowsPerBlock), ed::kMaxRowBlocks))),
                     dim3(kThreads), 0, q, sites, Z * Y, iX, work);
  marks.mark();
  hipLaunchKernelGGL(edt_y_kernel, dim3(static_cast<unsigned>(ed::pass_lanes(Z * X) / kThreads)), dim3(kThreads), 0, q, work, iZ, iY,
                     iX, s.wy, s.wx, stacks);
  marks.mark();
  hipLaunchKernelGGL(edt_z_kernel, dim3(static_cast<unsigned>(ed::pass_lanes(Y * X) / kThreads)), dim3(kThreads), 0, q, work, nearest,
                     reinterpret_cast<int32_t*>(dist), iZ, iY, iX, s, stacks);
  marks.mark();
  return lsr::launch_status(what);
}

// The launches with a HIP event between them: waits for the stream and writes the three times in milliseconds to ms3.
template <class Sites>
int edt_profile(Sites sites, int64_t Z, int64_t Y, int64_t X, const double* sampling, float* dist, int32_t* nearest, void* scratch,
                float* ms3, hipStream_t q, const char* what) {
  return lsr::profile_launches<kLaunches>(ms3, q, what, [&](lsr::LaunchMarks marks) {
    return edt_launches(sites, Z, Y, X, sampling, dist, nearest, scratch, q, marks, what);
  });
}

}  // namespace

extern "C" int lsr_edt_tiling(int tiling[4]) {
  LSR_REQUIRE_PTR(tiling);
  tiling[0] = ed::kChunk;
  tiling[1] = ed::kLineTile;
  tiling[2] = static_cast<int>(ed::kMaxRowBlocks * ed::kRowsPerBlock);
  tiling[3] = static_cast<int>(ed::kMaxLanes);
  return LSR_OK;
}

extern "C" int64_t lsr_edt_scratch_bytes(int64_t Z, int64_t Y, int64_t X) {
  if (int rc = ed::check_volume(Z, Y, X)) return rc;
  return ed::scratch_bytes(Z, Y, X);
}

extern "C" int lsr_edt_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int invert, const double* sampling,
                           float* dist, int32_t* nearest, void* scratch, lsr_stream_t stream) {
  if (int rc = ed::check_edt(in, Z, Y, X, sampling, dist, nearest, scratch)) return rc;
  return edt_launches(FloatSites{in, threshold, invert != 0}, Z, Y, X, sampling, dist, nearest, scratch, lsr::as_stream(stream), {},
                      "lsr_edt_f32");
}

extern "C" int lsr_edt_labels_i32(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int invert, const double* sampling,
                                  float* dist, int32_t* nearest, void* scratch, lsr_stream_t stream) {
  if (int rc = ed::check_edt(labels, Z, Y, X, sampling, dist, nearest, scratch)) return rc;
  return edt_launches(LabelSites{labels, invert != 0}, Z, Y, X, sampling, dist, nearest, scratch, lsr::as_stream(stream), {},
                      "lsr_edt_labels_i32");
}

// Measurement only (tools/bench_kernels.py --edt): lsr_edt_f32 with a HIP event between its launches; waits for the stream and
// writes the times of x, y and z in milliseconds to ms3 (HOST memory).
extern "C" int lsr_edt_profile_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int invert,
                                   const double* sampling, float* dist, int32_t* nearest, void* scratch, float* ms3,
                                   lsr_stream_t stream) {
  if (int rc = ed::check_edt(in, Z, Y, X, sampling, dist, nearest, scratch)) return rc;
  LSR_REQUIRE_PTR(ms3);
  return edt_profile(FloatSites{in, threshold, invert != 0}, Z, Y, X, sampling, dist, nearest, scratch, ms3, lsr::as_stream(stream),
                     "lsr_edt_profile_f32");
}

extern "C" int lsr_label_expand_i32(const int32_t* labels, const int32_t* nearest, int64_t Z, int64_t Y, int64_t X,
                                    const double* sampling, double distance, int32_t* out, lsr_stream_t stream) {
  if (int rc = ed::check_expand(labels, nearest, Z, Y, X, sampling, distance, out)) return rc;
  const int64_t n = Z * Y * X;
  hipLaunchKernelGGL(label_expand_kernel, dim3(static_cast<unsigned>(std::min(lsr::ceil_div(n, kThreads), kMaxBlocks))), dim3(kThreads),
                     0, lsr::as_stream(stream), labels, nearest, static_cast<int>(Y), static_cast<int>(X), n, ed::make_sampling(sampling),
                     distance, out);
  return lsr::launch_status("lsr_label_expand_i32");
}
