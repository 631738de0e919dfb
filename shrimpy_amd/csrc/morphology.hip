// Flat grey-scale morphology (shrimpy_amd/morphology.py): erosion, dilation, opening, closing and the two top-hats of a
// float32 volume under a box window.  The rule, the order, the codes and the plan of passes are in morphology.hpp; PINNED to
// scipy.ndimage element for element (tests/morphology_ref.py).
//
// One launch per axis with a half-width > 0 (an opening: up to six), nothing between workgroups, no atomics; every launch
// reads each voxel of its source once and writes each voxel of its target once.  The bead detection (peaks.hip) runs its box
// maximum through the same launches (launch_pass, launch_strided of morphology.hpp), its z pass with a sink of its own.
//   x       morph_rows_kernel: a workgroup walks a row in equal segments of at most kRowSegment outputs.  The codes of the
//           segment and of the window's reach on both sides sit in LDS; the 2r codes the next segment shares with this one are
//           MOVED inside LDS, not read again.  Window maxima by doubling spans (1, 2, 4, ... <= w): log2 w LDS sweeps per
//           voxel.  The values of the segment to come -- of this row or of the workgroup's next one -- are read into registers
//           before the sweeps begin, so the reads of global memory run under the LDS work.
//   y, z    morph_strided_kernel (morphology.hpp, a template of the sink): one wavefront per workgroup owns kColumns = 64
//           neighbouring columns -- every row it touches is one 256-byte access -- and walks them block by block (blocks of w positions) over the whole line.  LDS holds w
//           codes per column: the suffix maxima of the previous block, overwritten in place by the current block's codes as
//           the forward sweep consumes them (slot t is free once h(t) has been used), then turned into its suffix maxima by a
//           backward sweep.  The prefix maximum runs in a register.  No barrier: a lane touches its own column only.  The
//           line is read as one stream, 8, 16 or 32 rows ahead of the walk (the wider the window, the fewer wavefronts its
//           strip leaves on a compute unit, the more each has in flight).
//           w * 256 bytes of LDS: 2.8 KB at r = 5, 25.9 KB at r = 50, 131.3 KB at the cap r = 256.
// What a pass does with a window maximum is its sink: here StoreSink, which also fuses the top-hats' subtraction into the last
// pass (it reads the caller's volume at the voxel it writes).

#include <algorithm>

#include "morphology.hpp"

namespace {

namespace mo = lsr::morph;
using mo::decode;
using mo::encode;
using mo::umax;

constexpr int kRowBuf = mo::kRowSegment + 2 * mo::kMaxHalfWidth;

constexpr int kRowRegs = (kRowBuf + mo::kRowThreads - 1) / mo::kRowThreads;   // values of one segment per thread

// One segment of one row: outputs [x0, x0 + len); raw[i] holds the code of x = x0 - r + i for i < n = len + 2r.  The first
// segment of a row brings all n of them (r positions in front of the row included: no code), a later one only those from
// index 2r on -- the 2r in front were moved down from the end of the segment before.
struct RowItem {
  int64_t row, x0;
  int len, n, lo;
};
__device__ __forceinline__ RowItem row_item(int64_t row, int sgi, int seg, int64_t X, int r) {
  RowItem it;
  it.row = row;
  it.x0 = static_cast<int64_t>(sgi) * seg;
  it.len = static_cast<int>(std::min<int64_t>(seg, X - it.x0));
  it.n = it.len + 2 * r;
  it.lo = sgi == 0 ? 0 : 2 * r;
  return it;
}

__global__ __launch_bounds__(mo::kRowThreads) void morph_rows_kernel(const float* __restrict__ in, mo::StoreSink sink,
                                                                      int64_t rows, int64_t X, int r, int least_i, int seg,
                                                                      int nsegs) {
  __shared__ uint32_t raw[kRowBuf], ping[kRowBuf], pong[kRowBuf];
  const bool least = least_i != 0;
  const int tid = threadIdx.x, w = 2 * r + 1;
  int64_t row = blockIdx.x;
  if (row >= rows) return;
  int sgi = 0;
  float pre[kRowRegs];                           // the values of the segment to come, read while this one is worked on
  auto fetch = [&](const RowItem& it) {
    const float* src = in + it.row * X;
#pragma unroll
    for (int k = 0; k < kRowRegs; ++k) {
      const int i = it.lo + tid + k * mo::kRowThreads;
      const int64_t x = it.x0 - r + i;
      pre[k] = (i < it.n && x >= 0 && x < X) ? src[x] : 0.0f;
    }
  };
  fetch(row_item(row, sgi, seg, X, r));
  while (true) {
    const RowItem it = row_item(row, sgi, seg, X, r);
#pragma unroll
    for (int k = 0; k < kRowRegs; ++k) {
      const int i = it.lo + tid + k * mo::kRowThreads;
      const int64_t x = it.x0 - r + i;
      if (i < it.n) raw[i] = (x >= 0 && x < X) ? encode(pre[k], least) : mo::kNoCode;
    }
    __syncthreads();
    int64_t next_row = row;
    int next_sgi = sgi + 1;
    if (next_sgi == nsegs) {
      next_sgi = 0;
      next_row = row + gridDim.x;
    }
    const bool more = next_row < rows;
    if (more) fetch(row_item(next_row, next_sgi, seg, X, r));
    const int n = it.n;
    const uint32_t* cur = raw;                   // cur[i] = max over [i, i + span), valid while i + span <= n
    uint32_t* nxt = ping;
    int span = 1;
    for (; span * 2 <= w; span *= 2) {
      for (int i = tid; i + 2 * span <= n; i += mo::kRowThreads) nxt[i] = umax(cur[i], cur[i + span]);
      __syncthreads();
      cur = nxt;
      nxt = nxt == ping ? pong : ping;
    }
    const int64_t at = row * X + it.x0;
    for (int t = tid; t < it.len; t += mo::kRowThreads) sink(at + t, decode(umax(cur[t], cur[t + w - span]), least));
    if (next_sgi != 0) {                         // the 2r codes the next segment starts with (len = seg >= 2r: no overlap)
      for (int i = tid; i < 2 * r; i += mo::kRowThreads) raw[i] = raw[it.len + i];
    }
    __syncthreads();
    if (!more) break;
    row = next_row;
    sgi = next_sgi;
  }
}

// no axis has a window: a copy, or v - v
__global__ __launch_bounds__(256) void morph_pointwise_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n,
                                                              int fuse) {
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float v = in[e];
    out[e] = mo::fused(v, v, fuse);
  }
}

}  // namespace

int mo::launch_pass(const float* src, const mo::StoreSink& sink, int64_t Z, int64_t Y, int64_t X, const mo::Pass& ps,
                    const char* who, hipStream_t st) {
  if (ps.axis != 2) return mo::launch_strided(src, mo::lines_of(ps.axis, Z, Y, X), ps.r, ps.least, sink, who, st);
  // segments of equal length (a multiple of the wavefront), at most kRowSegment outputs each
  const int64_t want = lsr::ceil_div(X, mo::kRowSegment);
  const int seg = static_cast<int>(lsr::ceil_div(lsr::ceil_div(X, want), lsr::kWave) * lsr::kWave);
  hipLaunchKernelGGL(morph_rows_kernel, dim3(static_cast<unsigned>(std::min(Z * Y, mo::kMaxRowBlocks))), dim3(mo::kRowThreads), 0, st,
                     src, sink, Z * Y, X, ps.r, ps.least ? 1 : 0, seg, static_cast<int>(lsr::ceil_div(X, seg)));
  return LSR_OK;
}

extern "C" int lsr_grey_morph_tiling(int tiling[4]) {
  LSR_REQUIRE_PTR(tiling);
  tiling[0] = mo::kMaxHalfWidth;
  tiling[1] = mo::kColumns;
  tiling[2] = mo::kRowSegment;
  tiling[3] = mo::kRowThreads;
  return LSR_OK;
}

extern "C" int lsr_grey_morph_dispatch(int dispatch[6]) {
  LSR_REQUIRE_PTR(dispatch);
  dispatch[0] = mo::kNarrow;
  dispatch[1] = mo::kMaxStaticHalfWidth;
  dispatch[2] = static_cast<int>(mo::kMaxRowBlocks);
  dispatch[3] = mo::kAheadNarrow;
  dispatch[4] = mo::kAheadStatic;
  dispatch[5] = mo::kAheadDynamic;
  return LSR_OK;
}

extern "C" int64_t lsr_grey_morph_scratch_bytes(int64_t Z, int64_t Y, int64_t X) {
  LSR_REQUIRE(Z > 0 && Y > 0 && X > 0, LSR_E_SHAPE, "shape (%lld,%lld,%lld) must be positive", (long long)Z, (long long)Y,
              (long long)X);
  LSR_REQUIRE_VOLUME(Z, Y, X);
  return 2 * Z * Y * X * static_cast<int64_t>(sizeof(float));
}

extern "C" int lsr_grey_morph_f32(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int op,
                                  void* scratch, lsr_stream_t stream) {
  if (int rc = mo::check_morph(in, out, Z, Y, X, rz, ry, rx, op, scratch)) return rc;
  hipStream_t st = lsr::as_stream(stream);
  const int64_t voxels = Z * Y * X;
  mo::Pass passes[mo::kMaxPasses];
  const int n = mo::plan(rz, ry, rx, op, passes);
  const int fuse = mo::fuse_of(op);
  if (n == 0) {
    const int64_t want = lsr::ceil_div(voxels, 256);
    hipLaunchKernelGGL(morph_pointwise_kernel, dim3(static_cast<unsigned>(std::min(want, mo::kMaxBlocks))), dim3(256), 0, st, in, out,
                       voxels, fuse);
    return lsr::launch_status("lsr_grey_morph_f32");
  }
  float* work = static_cast<float*>(scratch);
  for (int k = 0; k < n; ++k) {
    const int f = k == n - 1 ? fuse : static_cast<int>(mo::kPlain);
    const mo::StoreSink sink{mo::pass_target(k, n, out, work, voxels), f != mo::kPlain ? in : nullptr, f};
    if (int rc = mo::launch_pass(mo::pass_source(k, in, work, voxels), sink, Z, Y, X, passes[k], "lsr_grey_morph_f32", st)) return rc;
  }
  return lsr::launch_status("lsr_grey_morph_f32");
}
