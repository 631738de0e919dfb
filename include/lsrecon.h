/*
 * lsrecon.h -- C ABI of the MI355X (gfx950) light-sheet reconstruction hot path.
 *
 * This is the drop-in boundary: a flat, extern "C" interface with plain pointers and sizes.
 * No torch types, no allocation inside, no global scratch: every buffer is a DEVICE pointer
 * owned by the caller (in the Python host: a torch-ROCm tensor's data_ptr()), every entry
 * point takes the HIP stream to launch on and is re-entrant across streams.
 *
 * What each entry point replaces in the reference (czbiohub-sf/shrimPy, paths relative to the
 * reference root; biahub = un-vendored dependency pinned at pyproject.toml:91):
 *
 *   lsr_deskew_f32          biahub.deskew.fast_deskew_zyx, called at
 *                           shrimpy/preprocessing.py:408-413 (and the older
 *                           biahub deskew_data, scripts/measure_psf.py:238-246)
 *   lsr_affine_f32          registration apply (north-star; docs/data_structure.md:58-62) ==
 *                           scipy.ndimage.affine_transform(order=1); also the general-matrix
 *                           deskew path together with lsr_average_slices_f32
 *   lsr_average_slices_f32  biahub _average_n_slices (average_n_slices setting,
 *                           config/mda/mantis/dynatrack_demo.yaml:164)
 *   lsr_correlate_*, lsr_rl_*  Richardson-Lucy deconvolution (north-star; no reference symbol)
 *
 * Layout: all volumes are C-order (Z, Y, X) float32, X fastest, densely packed.
 * Matrices: `M` is a row-major 3x4 double, OUTPUT index -> INPUT coordinate (the
 * scipy.ndimage convention): in_c = M[c][0]*zo + M[c][1]*yo + M[c][2]*xo + M[c][3].
 *
 * Return value: 0 = ok; < 0 = argument error (LSR_E_*), nothing was launched;
 * > 0 = a hipError_t from the launch. lsr_last_error() returns a thread-local message.
 * Nothing here synchronises the stream or the device.
 *
 * Sizes: every extent in [1, 2^30), fewer than 2^48 voxels per volume, row strides below 2^31 and plane strides
 * below 2^32 elements -- anything else is LSR_E_UNSUPPORTED before the entry computes with it.  Inside those bounds
 * volumes of more than 2^32 voxels are ordinary (64-bit bases per plane / row); narrower limits are stated at the entries.
 */
#ifndef LSRECON_H
#define LSRECON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_VERSION 100 /* 0.1.0 */

#define LSR_OK 0
#define LSR_E_NULL (-1)        /* a required pointer is NULL */
#define LSR_E_SHAPE (-2)       /* a dimension is <= 0 or inconsistent */
#define LSR_E_UNSUPPORTED (-3) /* valid request this kernel does not cover (see each function) */
#define LSR_E_ARG (-4)         /* another argument is out of range */

/* Border rule of the order-1 sampler. */
#define LSR_MODE_CONSTANT 0      /* scipy mode="constant": any coordinate outside [0,n-1] -> cval */
#define LSR_MODE_GRID_CONSTANT 1 /* scipy mode="grid-constant": blend towards cval over one voxel */
/* OR-able flag for lsr_affine_f32: interpolate in f32 (coordinates and border decisions stay
 * fp64). Not bit-identical to scipy (~1e-6 relative) but HBM-bound instead of fp64-VALU-bound. */
#define LSR_MODE_F32_INTERP 256

/* Which half of a Richardson-Lucy iteration a correlation launch finishes (fused epilogue). */
#define LSR_EPI_NONE 0   /* out = corr(in)                                  (plain correlation) */
#define LSR_EPI_RATIO 1  /* out = aux / (corr(in) + eps)       aux = y      (ratio = y/(Hx+eps)) */
#define LSR_EPI_UPDATE 2 /* out = aux * corr(in) / norm        aux = x      (x <- x*H^T(ratio)/H^T1) */
#define LSR_EPI_SCALE 3  /* out = corr(in) / norm   (lsr_correlate_dense_padded_f32 only: the (z, x) half
                            of a PSF that separates along y, whose y half runs as a separable pass) */

typedef void* lsr_stream_t; /* a hipStream_t; NULL = the default stream */

int lsr_version(void);
const char* lsr_last_error(void);
/* Fingerprint of the sources this BINARY was compiled from: the first 16 hex digits of the sha256 over (name, bytes) of
 * include/lsrecon.h, csrc/Makefile and every .hip / .hpp file in csrc (csrc/Makefile computes it, api.o is rebuilt whenever
 * one of them changes).  The library is git-ignored and travels to the GPU box as a file: the Python host compares this
 * with the same hash of the checkout beside it (shrimpy_amd/_lib.py::kernel_source_sha16) and refuses a stale build. */
const char* lsr_source_sha16(void);
/* Page-locked host memory of exactly `bytes` bytes from the HIP runtime (hipHostMalloc, portable across
 * devices): the staging slots of the store-to-store path.  Returns 0 or the hipError_t (then *out = NULL). */
int lsr_pinned_alloc(int64_t bytes, void** out);
int lsr_pinned_free(void* ptr);

/*
 * Oblique-plane deskew with the slice averaging fused in.
 *
 *   in   raw stack (Z, Y, X) = (scan, tilt, coverslip)
 *   out  (Zo, Yo, Xo) with strides out_pitch (y) and out_plane (z) in floats -- dense: Xo and
 *        Yo*Xo; a padded volume (lsr_sep_padded_shape) lets the deskew write the RL input in
 *        place, on cache-line-aligned rows; Zo == ceil(Zd / avg_n), Zd = depth BEFORE averaging
 *   M    output->input map over the PRE-average grid (Zd, Yo, Xo). It must have the deskew
 *        structure: row 0 = (a, 0, b, c) (only z_in is interpolated), row 1 = (+-1, 0, 0, int),
 *        row 2 = (0, +-1, 0, int). Anything else returns LSR_E_UNSUPPORTED: use
 *        lsr_affine_f32 + lsr_average_slices_f32 for a general matrix.
 *   avg_n  >= 1; pre-average slices zd = zo*avg_n + k, k < avg_n, clamped to Zd-1 (edge pad).
 *
 * Arithmetic: coordinates and the 2-tap interpolation in fp64 exactly as
 * scipy.ndimage.affine_transform(order=1, mode="constant", cval=0) evaluates them (result
 * rounded to f32 once), then ((d0+d1)+...)/avg_n in f32: bit-identical to the CPU oracle.
 */
int lsr_deskew_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                   int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                   const double M[12], int avg_n, lsr_stream_t stream);
/* The same with the raw stack as the camera's uint16 counts: the conversion to float32 (exact)
 * happens on the way into the kernel, so neither the host nor HBM ever holds a float copy of the
 * stack -- half the PCIe upload, half the HBM read. Results equal lsr_deskew_f32 on the converted
 * stack bit for bit. */
int lsr_deskew_u16(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                   int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                   const double M[12], int avg_n, lsr_stream_t stream);

/*
 * The same kernel under an explicit border rule, all input variants behind one entry: in_u16 != 0 reads
 * uint16 counts, flat_pattern / flat_mean (both or neither NULL) fuse the flat-field correction, and
 * mode = LSR_MODE_CONSTANT | LSR_MODE_GRID_CONSTANT.  "grid-constant" continues the raw stack with zeros, so
 * a scan coordinate within one sample of either end blends its inside neighbour with 0 -- what
 * scipy mode="grid-constant" and torch grid_sample(padding_mode="zeros") do; the deskew geometry is
 * [RECALLED], this is the switch that covers the other border convention at full
 * speed.  Bit-identical to lsr_affine_f32(mode) followed by lsr_average_slices_f32.
 */
int lsr_deskew_border(const void* in, int in_u16, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                      int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                      const double M[12], int avg_n, int mode, const float* flat_pattern,
                      const float* flat_mean, lsr_stream_t stream);
/* ... with the value outside the stack (scipy's `cval`; [RECALLED] biahub's deskew_data takes one and fills with the
 * stack's minimum when it is None): `cval` is a DEVICE scalar -- a constant the caller uploaded, or out2[0] of
 * lsr_minmax_f32 / lsr_minmax_u16 over the stack, so that "min" needs no host round trip -- NULL = 0 (the entries above).
 * Under "grid-constant" the outside neighbour is cval * weight, as scipy sums it.  The _cpu twin reads a host scalar and
 * has the "constant" border only. */
int lsr_deskew_cval(const void* in, int in_u16, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo, int64_t Yo,
                    int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd, const double M[12], int avg_n, int mode,
                    const float* flat_pattern, const float* flat_mean, const float* cval, lsr_stream_t stream);
int lsr_deskew_cval_cpu(const void* in, int in_u16, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo, int64_t Yo,
                        int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd, const double M[12], int avg_n,
                        int mode, const float* flat_pattern, const float* flat_mean, const float* cval, lsr_stream_t stream);
/* The launch the deskew entries above make for this output shape and matrix -- host code, no device call; the status is
 * the one those entries return for the same shape and matrix.  out = {X' per workgroup (64 halved until the tile's scan
 * range fits the slab), Y' per workgroup, LDS slab rows, slab rows staged per pass, tiles along X', tiles along Y',
 * workgroups with work, workgroups launched (padded to a multiple of 8 unless LSR_DESKEW_SWIZZLE=0)}.  The entries launch
 * from the same function: what the tests count from it is what runs. */
int lsr_deskew_plan(int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], int64_t out[8]);
/* min / max of uint16 camera counts as two floats (exact), scratch as lsr_minmax_f32 */
int lsr_minmax_u16(const uint16_t* in, int64_t n, float* out2, void* scratch, lsr_stream_t stream);

/*
 * General order-1 (trilinear) affine resample; any 3x4 matrix.
 * mode/cval as scipy.ndimage.affine_transform. fp64 coordinates and weights, same operation
 * order as scipy: bit-identical to the CPU oracle for finite inputs.
 * Non-finite inputs: the three kernels and the host twin apply the rule of csrc/resample.hpp literally -- every corner is
 * multiplied, also by a weight of exactly 0 (inf * 0 is a NaN), so a NaN or an infinity reaches exactly the voxels one of whose
 * eight taps holds it -- and agree bit for bit (a NaN by position) at every voxel none of whose coordinates is exactly n - 1 on
 * its axis.  There the upper neighbour, of weight 0, is voxel n - 1 itself in the gather kernel and the twin and a staged
 * duplicate of in-volume data (in a padded source: the padding column) in the LDS-staged kernels: the same bits on finite data
 * only.  (tests/affine_ref.py restates the rule; tests/test_affine_edges_gpu.py holds all four to it.)
 */
int lsr_affine_f32(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* out, int64_t Zo,
                   int64_t Yo, int64_t Xo, const double M[12], float cval, int mode,
                   lsr_stream_t stream);
/*
 * The same with a source whose rows are padded: in_pitch floats from row to row, in_plane from plane to
 * plane.  The LDS-staged kernels move 16-byte chunks, so they need rows that start on 16-byte
 * boundaries: in_pitch and in_plane multiples of 4, in_pitch >= Xi rounded up to 4, `in` 16-byte aligned,
 * and FINITE values in the padding columns [Xi, in_pitch) (they only ever meet weight 0; zeros are the
 * natural choice).  A deskewed volume is Xp = ceil(Z / r - Y cos(theta)) wide -- a multiple of 4 one time
 * in four; lsr_deskew_* writes any out_pitch, so the deskew -> register chain keeps the fast kernels for
 * every width.  Other strides run the gather kernel, as lsr_affine_f32 does for Xi % 4 != 0.
 * out_pitch / out_plane (any values >= the dense ones) let the result land inside a larger allocation, e.g.
 * the padded volume the Richardson-Lucy kernels read, so no copy sits between registration and deconvolution.
 */
int lsr_affine_pitched_f32(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, int64_t in_pitch,
                           int64_t in_plane, float* out, int64_t Zo, int64_t Yo, int64_t Xo,
                           int64_t out_pitch, int64_t out_plane, const double M[12], float cval, int mode,
                           lsr_stream_t stream);
int lsr_affine_path_pitched(int64_t Zi, int64_t Yi, int64_t Xi, int64_t in_pitch, int64_t in_plane,
                            const double M[12], int mode); /* lsr_affine_path for such a source */
/* The launch lsr_affine_pitched_f32 makes for these shapes, strides, matrix and mode (lsr_affine_f32: in_pitch = Xi,
 * in_plane = Yi * Xi, out_pitch = Xo) -- host code, no device call; the status is the one that entry returns for the
 * same arguments with valid buffers.  out[0] = the path as lsr_affine_path_pitched numbers it, then
 *   1 (csrc/affine_planar.hip): out[1..13] = waves per workgroup, tile rows, tile columns, box_y, box_x (the staged box of a
 *     source plane), ring slots, LDS bytes, z_chunk (output planes per workgroup), tiles_y, tiles_x, patch h, patch w
 *     (tiles per patch, exact mode), workgroups launched;
 *   2 (csrc/affine_box.hip): out[1..13] = block tz, ty, tx, box bz, by, bx, LDS bytes, blocks along z, y, x, `linear`
 *     (1: patch-major order as numbered, 0: a contiguous run of it per XCD), 0, workgroups launched;
 *   0 (csrc/affine.hip): out[2], out[3] = rows and columns of a workgroup, out[9], out[10] = tiles_y, tiles_x, out[13] =
 *     workgroups launched; the rest 0.
 * out[14], out[15] are 0.  LSR_PLANAR_WAVES, LSR_PLANAR_PATCH and LSR_BOX_LINEAR (measurement switches, read per
 * launch) are honoured as the launchers honour them: those launch from the same functions, so what the tests count from a
 * plan is what runs.  Only what the call itself knows can still send it to the gather kernel: `in` not 16-byte aligned,
 * in == out, or a device that refuses the LDS budget. */
int lsr_affine_plan(int64_t Zi, int64_t Yi, int64_t Xi, int64_t in_pitch, int64_t in_plane, int64_t Zo, int64_t Yo,
                    int64_t Xo, int64_t out_pitch, const double M[12], int mode, int64_t out[16]);
/* Which kernel lsr_affine_f32 runs for this matrix on a (.., Yi, Xi) moving volume: 1 = the
 * LDS-staged z-marching kernel (csrc/affine_planar.hip: constant mode, z decoupled from the plane,
 * |M[0]| <= 1.5, Xi a multiple of 4, source box of a 32 x 128 tile within LDS), 0 = the general
 * gather kernel. Results are identical either way. */
int lsr_affine_kernel_choice(int64_t Yi, int64_t Xi, const double M[12], int mode);
/* The same question with all three kernels: 1 = csrc/affine_planar.hip (as above); 2 =
 * csrc/affine_box.hip (constant mode, any matrix -- maps that couple z with the plane included --
 * whose source box of an 8 x 16 x 64 output block fits in 150 KB of LDS, Xi a multiple of 4);
 * 0 = the general gather kernel. Results are identical whichever runs. */
int lsr_affine_path(int64_t Zi, int64_t Yi, int64_t Xi, const double M[12], int mode);
/* Host-side geometry of the box kernel for this matrix: out6 = {block z, y, x extents; staged source
 * box planes, rows, floats per row}; returns 1, or 0 when the box kernel does not apply.  (What the
 * CPU tests check the kernel's coverage claim against: every tap of every voxel of a block lies inside
 * the box spanned from the block's two extreme corners.) */
int lsr_affine_box_shape(int64_t Zi, int64_t Yi, int64_t Xi, const double M[12], int* out6);

/*
 * Affine registration, estimate half (no reference symbol, docs/data_structure.md:58-62).
 * Normal equations of one Gauss-Newton step of   min sum_x (gain * moving(M x) + offset - target(x))^2
 * over the target grid sampled every `stride[axis]` voxels (trilinear taps; a sample counts when all eight
 * lie inside `moving`).  Parameters: the 3x4 matrix row by row in centred, scaled target coordinates
 * ((x - centre) / scale, 1), then gain, offset (14).  `partial` receives lsr_affine_normal_blocks()
 * rows of lsr_affine_normal_size() doubles (105 upper-triangle entries of J^T J row by row, 14 of
 * J^T r, sum r^2, sample count); their sum over rows, in row order, is the result.
 */
int lsr_affine_normal_size(void);
int lsr_affine_normal_blocks(void);
int lsr_affine_normal_equations_f32(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi,
                                    const float* target, int64_t Zo, int64_t Yo, int64_t Xo,
                                    const double M[12], double gain, double offset, const int stride[3],
                                    const double centre[3], double scale, double* partial,
                                    lsr_stream_t stream);

/*
 * Affine registration, mutual-information metric (csrc/estimate_mi.hip; no reference symbol): for two channels whose
 * intensities follow no linear map.  The conventions of lsr_affine_normal_equations_f32 (matrix, float64 coordinates,
 * strided target grid, a sample counts when its moving coordinate lies in [0, n - 1) on every axis, parameters in
 * centred, scaled coordinates).  Per sample, in float64 (csrc/mi_sample.hpp is the definition):
 *     a  = clamp(floor((t - t_lo) * bins / (t_hi - t_lo)), 0, bins - 1)              target bin, zero order
 *     u  = clamp((m - m_lo) * (bins - 1) / (m_hi - m_lo), 0, bins - 1)               m = trilinear moving value
 *     b0 = min(floor(u), bins - 2), f = u - b0, w1 = floor(f * 65536 + 0.5), w0 = 65536 - w1
 *     hist[a][b0] += w0, hist[a][b0 + 1] += w1                                       (a linear Parzen window)
 * lsr_affine_joint_histogram_f32: `hist` ([bins][bins] 64-bit counters in units of 2^-16 sample) and `n_samples` (one
 * counter) are DEVICE memory, zeroed by the entry on `stream` before the launch.  The sums are integer: the same bits on
 * every run and from the host twin.  bins in [4, 64], t_hi > t_lo, m_hi > m_lo.  Size limit: the volumes every entry
 * accepts (extents below 2^30, fewer than 2^48 voxels): 65536 * n stays below 2^64, and the kernel's 32-bit LDS
 * counters are flushed before 65536 full-weight samples per lane could wrap them.  The launch has
 * lsr_affine_joint_histogram_blocks() workgroups of 256 threads; grid sample s is visited by workgroup
 * (s / 256) % blocks, in both kernels.
 * Values that are not finite (the lerp is IEEE arithmetic as written, so one NaN or infinite tap can make m NaN): a NaN
 * or -inf target value goes to target bin 0, +inf to the last; a NaN u is clamped to 0 -- all weight in column 0, w1 = 0
 * -- and adds nothing to the gradient; a u of +inf is clamped to bins - 1, of -inf to 0.
 * lsr_affine_mi_gradient_f32: for every sample whose unclamped u lies strictly inside (0, bins - 1) -- a u of exactly 0
 * or bins - 1 counts as clamped and adds nothing -- adds dL[a][b0] * (bins - 1) / (m_hi - m_lo) * (dm/dz, dm/dy, dm/dx)
 * (x) ((x - centre) / scale, 1) to 12 fp64 sums.  `dL` ([bins][bins - 1], DEVICE memory) is the caller's
 * L(a, b + 1) - L(a, b) with L = log(P(a, b) / P_m(b)) (0 where the count is 0).  `partial` receives
 * lsr_affine_mi_gradient_blocks() rows of lsr_affine_mi_gradient_size() doubles; their sum in row order is the result
 * (no atomics: the same bits on every run).
 */
int lsr_affine_joint_histogram_f32(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target,
                                   int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], const int stride[3],
                                   int bins, double t_lo, double t_hi, double m_lo, double m_hi,
                                   unsigned long long* hist, unsigned long long* n_samples, lsr_stream_t stream);
int lsr_affine_joint_histogram_blocks(void);
int lsr_affine_mi_gradient_size(void);
int lsr_affine_mi_gradient_blocks(void);
int lsr_affine_mi_gradient_f32(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target,
                               int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], const int stride[3],
                               const double centre[3], double scale, int bins, double t_lo, double t_hi, double m_lo,
                               double m_hi, const double* dL, double* partial, lsr_stream_t stream);

/*
 * Ingest, host side (no device work): the acquisition writes blosc frames (zstd, byte
 * shuffle; shrimpy/mantis/mantis_engine.py:474-481) and the reference reads them through iohub -> zarr ->
 * numcodecs.blosc.decompress.  lsr_blosc_decode_host walks one c-blosc 1.x frame, entropy-decodes every stream
 * and undoes the byte shuffle into `out` (out_bytes = the frame's nbytes; host memory, e.g. a slab of a pinned
 * staging slot).  One call per chunk, safe from many threads at once (a Python walk costs ~10 us per stream
 * under the GIL; c-blosc frames have ~1000 streams per chunk).  *typesize (may be NULL) = the frame's element
 * size.  zstd / lz4 / zlib come from the system libraries at run time (dlopen).
 * LSR_E_UNSUPPORTED: bit shuffle, blosclz / snappy, or the decoder library is missing (callers fall back to
 * another codec); LSR_E_ARG: corrupt frame; LSR_E_SHAPE: out_bytes differs from the frame's nbytes.
 */
int lsr_blosc_host_codec(int compressor); /* 1 when the decoder of blosc compressor code 1 (lz4) / 3 (zlib) / 4 (zstd) is loadable */
int lsr_blosc_decode_host(const uint8_t* frame, int64_t frame_bytes, uint8_t* out, int64_t out_bytes, int* typesize);
/*
 * The writer's side (host code): one c-blosc 1.x frame of `src` with zstd streams, one per block (not split), byte
 * shuffle (shuffle = 1, typesize > 1) or none (0) -- the format the acquisition engine writes and the CLI's default
 * output (mantis_engine.py:474-481).  Byte for byte the frames of the Python encoder (shrimpy_amd/io/codecs.py:
 * blocksize or 256 KB cut to whole elements, a block zstd does not shrink stored verbatim, a frame that does not shrink
 * in the "memcpyed" form), but callable from many threads at once.  dst: lsr_blosc_encode_bound(nbytes, typesize,
 * blocksize) bytes; *out_bytes = the frame's size.  LSR_E_UNSUPPORTED: libzstd's compressor is not loadable, or a
 * shuffle other than 0 / 1 (callers keep the Python encoder).
 */
int lsr_blosc_host_encoder(void);
int64_t lsr_blosc_encode_bound(int64_t nbytes, int typesize, int64_t blocksize);
int lsr_blosc_encode_host(const uint8_t* src, int64_t nbytes, int typesize, int clevel, int shuffle, int64_t blocksize,
                          uint8_t* dst, int64_t cap, int64_t* out_bytes);
/*
 * The writer's side ON THE DEVICE (csrc/blosc_encode.hip): the volume at `src` (src_bytes of `typesize`-byte elements,
 * 1 / 2 / 4) cut into consecutive chunks of frame_bytes -- the Zarr chunks of whole z planes -- each written as one
 * c-blosc 1.x frame (zstd, byte shuffle, blocks of `blocksize` bytes, 0 = 64 K elements; at most 64 K elements per
 * block), the last chunk zero-padded to frame_bytes as Zarr pads edge chunks.  Every shuffled byte plane of a block is
 * one zstd block: RLE, Huffman-coded literals (four streams, no sequences) or Raw -- a subset of the format that any
 * zstd decoder reads and that matches zstd level 1 (the acquisition's setting, mantis_engine.py:474-481) on shuffled
 * image data to ~1 %.  Replaces numcodecs' Blosc(cname="zstd").encode behind iohub's writer
 * (shrimpy/dynatrack/tracking.py:1337-1367) for results that are already in HBM.
 * lsr_blosc_encode_device_plan: the frame count, the scratch bytes and the capacity of `out` the call needs.
 * On return (stream order) frames[2 f] = byte offset of frame f in `out` (16-byte aligned), frames[2 f + 1] = its size.
 * scratch / out / frames: device memory, 16-byte aligned.  The _cpu twin takes host pointers and writes the same bytes.
 */
int lsr_blosc_encode_device_plan(int64_t src_bytes, int typesize, int64_t frame_bytes, int64_t blocksize,
                                 int64_t* n_frames, int64_t* scratch_bytes, int64_t* out_cap);
int lsr_blosc_encode_device(const void* src, int64_t src_bytes, int typesize, int64_t frame_bytes, int64_t blocksize,
                            void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* frames,
                            lsr_stream_t stream);
int lsr_blosc_encode_device_cpu(const void* src, int64_t src_bytes, int typesize, int64_t frame_bytes, int64_t blocksize,
                                void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_cap, int64_t* frames,
                                lsr_stream_t stream);
/*
 * The reader's side ON THE DEVICE (csrc/blosc_decode.hip, csrc/zstd_lane.hpp): `comp` holds the compressed chunks of
 * one volume as the reader threads pread() them from the shard (device memory, comp_bytes long); frames[2 f], frames[2 f + 1]
 * = byte offset and size of chunk f's c-blosc frame in it (size 0: an absent chunk, zero-filled).  Every frame must
 * decode to frame_nbytes bytes in blocks of `blocksize` with elements of `typesize` (1 / 2 / 4) -- the values of the first
 * frame's header, which the host reads before the upload -- and use the zstd compressor (byte shuffle or none); chunk f
 * lands at out + f * frame_nbytes, the last one cut at out_bytes.  One lane per blosc block runs a complete zstd decoder
 * (RFC 8878: Huffman / FSE literals, sequences, repeat offsets), a second launch undoes the shuffle.  Replaces
 * numcodecs' Blosc.decode behind iohub's reader (shrimpy/replay_camera.py:176-268) for stacks on their way into HBM.
 * *status (device, 8 bytes) is 0 afterwards, or (block + 1) << 8 | code of the first block that failed (1 corrupt,
 * 2 destination too small, 3 unsupported, 4 size mismatch) -- a damaged chunk never faults.  The _cpu twin runs the same
 * decoder from host pointers.  lsr_zstd_lane_decode_cpu: one bare zstd frame through that decoder (tests, fuzzing).
 */
int lsr_blosc_decode_device_plan(int64_t n_frames, int64_t frame_nbytes, int64_t blocksize, int typesize,
                                 int64_t* scratch_bytes);
int lsr_blosc_decode_device(const uint8_t* comp, int64_t comp_bytes, const int64_t* frames, int64_t n_frames,
                            int64_t frame_nbytes, int64_t blocksize, int typesize, uint8_t* out, int64_t out_bytes,
                            void* scratch, int64_t scratch_bytes, unsigned long long* status, lsr_stream_t stream);
int lsr_blosc_decode_device_cpu(const uint8_t* comp, int64_t comp_bytes, const int64_t* frames, int64_t n_frames,
                                int64_t frame_nbytes, int64_t blocksize, int typesize, uint8_t* out, int64_t out_bytes,
                                void* scratch, int64_t scratch_bytes, unsigned long long* status, lsr_stream_t stream);
int lsr_zstd_lane_decode_cpu(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* out_n);
/* CRC-32C (Castagnoli, the Zarr v3 `crc32c` codec: shard index, optionally every chunk) of n host bytes; seed = 0, or
 * the value of the bytes before `data` when a buffer is checked in pieces.  SSE4.2 crc32 instruction where the CPU has
 * it, slice-by-8 tables otherwise (lsr_crc32c_host_portable: always the tables -- the cross-check). */
int lsr_crc32c_host(const uint8_t* data, int64_t n, uint32_t seed, uint32_t* out);
int lsr_crc32c_host_portable(const uint8_t* data, int64_t n, uint32_t seed, uint32_t* out);

/* out[zo] = mean_k in[min(zo*avg_n + k, Zd-1)], k < avg_n, f32, ((d0+d1)+...)/avg_n. */
int lsr_average_slices_f32(const float* in, int64_t Zd, int64_t Y, int64_t X, float* out,
                           int64_t Zo, int avg_n, lsr_stream_t stream);

/*
 * Bright-field flat-field correction -- replaces _LabelfreePreprocessor._flat_field_BF
 * (shrimpy/preprocessing.py:385-404): pattern = median over Z per (y, x) pixel with
 * torch.quantile(0.5) semantics (the exact middle elements a <= b under the order-preserving integer
 * image of a float, -0.0 below +0.0 and +-inf ordinary values; fma(-(b - a), 0.5, b) -- the
 * difference rounded to float32, the rest rounded once, as torch's lerp on the host -- between the two
 * of an even count; the canonical NaN 0x7fc00000 if the column holds one; a pixel's bits depend on its
 * own column alone), out = in / pattern * mean(pattern), the division first, each rounded to float32.
 *
 * lsr_flatfield_tiling: {pixels per workgroup, z phases per pixel, loads in flight per thread, the
 *   first Z that is refused} of the median kernel.
 * lsr_flatfield_pattern_f32: `pattern` (Y*X floats) and `mean_out` (one float) are device
 *   outputs; `scratch` = lsr_flatfield_scratch_bytes() bytes of device memory. Z < 65536.
 *   Reads `in` at most four times (radix select, csrc/flatfield.hip), writes nothing else.
 * lsr_flatfield_apply_f32: out = in / pattern * mean_dev[0] (in place allowed).
 * lsr_deskew_flat_f32: lsr_deskew_f32 with the correction applied to every raw sample on its
 *   way into the kernel -- bit-identical to apply followed by deskew, without the corrected
 *   volume's round trip through HBM.
 */
int lsr_flatfield_tiling(int tiling[4]);
int lsr_flatfield_scratch_bytes(void);
int lsr_flatfield_pattern_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float* pattern,
                              float* mean_out, void* scratch, lsr_stream_t stream);
int lsr_flatfield_apply_f32(const float* in, const float* pattern, const float* mean_dev,
                            float* out, int64_t Z, int64_t Y, int64_t X, lsr_stream_t stream);
/* The same three for a raw stack of uint16 camera counts (converted exactly inside the kernels;
 * the median then always takes the two-pass select on 16-bit keys). */
int lsr_flatfield_pattern_u16(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, float* pattern,
                              float* mean_out, void* scratch, lsr_stream_t stream);
int lsr_flatfield_apply_u16(const uint16_t* in, const float* pattern, const float* mean_dev,
                            float* out, int64_t Z, int64_t Y, int64_t X, lsr_stream_t stream);
int lsr_deskew_flat_u16(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                        int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                        const double M[12], int avg_n, const float* flat_pattern,
                        const float* flat_mean, lsr_stream_t stream);
int lsr_deskew_flat_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                        int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                        const double M[12], int avg_n, const float* flat_pattern,
                        const float* flat_mean, lsr_stream_t stream);

/*
 * 3-D correlation with zero-padded borders and a fused Richardson-Lucy epilogue:
 *
 *   c[z,y,x] = sum_{a,b,c} w[a,b,c] * in[z+a-pz/2, y+b-py/2, x+c-px/2]      (0 outside)
 *   out      = epilogue(c, aux)                                  (LSR_EPI_*)
 *
 * scipy.ndimage.correlate(in, w, mode="constant") semantics; pass the flipped PSF for
 * H x = ndimage.convolve(x, psf) and the PSF itself for H^T r. pz, py, px odd, <= 15.
 *
 * Dense form: `w` = pz*py*px device floats, C-order.
 * Separable form: `wz`, `wy`, `wx` device float arrays of pz, py, px taps (w = wz x wy x wx).
 *
 * `aux` (epilogues RATIO / UPDATE) and `out` are (Z, Y, X); `out` may alias `aux`, it must
 * not alias `in`. For LSR_EPI_UPDATE the divisor norm = H^T 1 (the sum of the taps that land
 * inside the volume) comes from `nz`, `ny`, `nx`:
 *   separable: device arrays of Z, Y, X floats, norm = nz[z]*ny[y]*nx[x];
 *   dense:     `norm_table` = device doubles, the (pz+1)*(py+1)*(px+1) inclusive 3-D prefix
 *              sum of w with a leading zero plane/row/column:
 *              P[a][b][c] = sum_{a'<a, b'<b, c'<c} w[a'][b'][c'].
 */
int lsr_correlate_sep_f32(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                          int64_t X, const float* wz, int pz, const float* wy, int py,
                          const float* wx, int px, int epilogue, float eps, const float* nz,
                          const float* ny, const float* nx, lsr_stream_t stream);

int lsr_correlate_dense_f32(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                            int64_t X, const float* w, int pz, int py, int px, int epilogue,
                            float eps, const double* norm_table, lsr_stream_t stream);

/*
 * The tuned (HBM-bound) separable kernel reads its input through a ZERO HALO instead of bounds
 * checks: zero padding is real memory, every load is unconditional and 16-byte aligned.
 *
 * lsr_sep_padded_shape: for a (Y, X) plane and a pz x py x px PSF returns
 *   shape[0] = rows and shape[1] = pitch (floats, multiple of 4) of the padded plane,
 *   shape[2], shape[3] = row / column of the logical element (y=0, x=0) inside it.
 * A padded volume is Z such planes, contiguous, base 128-byte aligned; everything outside the
 * logical (Y, X) window must be zero (the kernels only ever write inside it, so zero it once).
 * The logical origin sits at column 32 so that output runs start on 128-byte lines.
 *
 * lsr_correlate_sep_strided_f32: as lsr_correlate_sep_f32, with explicit strides (floats).
 * `in`, `aux`, `out` point at the LOGICAL element (0,0,0) of their volume; `in` must live in a
 * padded volume as above; `aux` / `out` may be dense (pitch X, plane Y*X) or padded.
 */
int lsr_sep_padded_shape(int64_t Y, int64_t X, int pz, int py, int px, int64_t shape[4]);

int lsr_correlate_sep_strided_f32(const float* in, int64_t in_pitch, int64_t in_plane,
                                  const float* aux, int64_t aux_pitch, int64_t aux_plane,
                                  float* out, int64_t out_pitch, int64_t out_plane, int64_t Z,
                                  int64_t Y, int64_t X, const float* wz, int pz, const float* wy,
                                  int py, const float* wx, int px, int epilogue, float eps,
                                  const float* nz, const float* ny, const float* nx,
                                  lsr_stream_t stream);

/*
 * Whole Richardson-Lucy loop: `iters` x { ratio = y/(H x + eps); x <- x * H^T ratio / H^T 1 }.
 * Launches 2*iters kernels on `stream`; capturable in a hipGraph (no sync, no allocation).
 *
 * Separable: k* = PSF factors along z, y, x, k*_flipped the same reversed (H = correlation with
 * the flipped taps). `x_pad` and `ratio_pad` are padded volumes (lsr_sep_padded_shape) with zero
 * halos: the caller writes the initial estimate into the logical window of `x_pad` -- or sets
 * `init_from_y`, which starts from x = y without that copy (then `y` itself must live in a padded
 * volume with a zero halo, e.g. written there by lsr_deskew_f32); `ratio_pad` is scratch. The final estimate is written to the dense (Z, Y, X) `x_out`, or left
 * in `x_pad` if `x_out` is NULL. `y` points at its logical (0,0,0) with strides y_pitch / y_plane
 * (dense: X and Y*X; a padded y keeps the ratio launch's reads on cache-line boundaries).
 *
 * Dense: psf = pz*py*px floats, psf_flipped = the same reversed on all three axes; x (dense) is
 * updated in place (caller initialises it), `ratio` is dense scratch.
 */
int lsr_rl_sep_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y,
                   float* x_pad, float* ratio_pad, float* x_out, int64_t Z, int64_t Y, int64_t X,
                   const float* kz, const float* kz_flipped, int pz,
                   const float* ky, const float* ky_flipped, int py, const float* kx,
                   const float* kx_flipped, int px, const float* nz, const float* ny,
                   const float* nx, int iters, float eps, lsr_stream_t stream);

/*
 * The same iterations with ONE launch each (rl_fused_sep.hip): ratio = y / (H x + eps) is formed
 * and consumed inside the workgroup, so an iteration moves 12 bytes per voxel through HBM instead
 * of 24. Results are bit-identical to lsr_rl_sep_f32. Compiled for every odd tap count up to 15 per
 * axis except 15 z taps with 11+ in-plane taps (lsr_rl_sep_fused_supported: 1 / 0; otherwise
 * LSR_E_UNSUPPORTED: use lsr_rl_sep_f32).
 *
 * `y` points at the logical (0,0,0) of a padded volume (lsr_sep_padded_shape geometry or larger
 * strides) whose halo is ZERO: the kernel reads y on the tile grown by the PSF radius.
 * `x_a`, `x_b` are padded working volumes (allocation start, zero halos, written only inside the
 * logical window). x_a holds the initial estimate unless `init_from_y` (x0 = y, read in place).
 * Iteration i reads (i even ? x_a : x_b) and writes the other; the last one writes the dense
 * (Z, Y, X) `x_out` instead when that is not NULL. With x_out == NULL the result is in x_b for odd
 * `iters`, in x_a for even.
 */
int lsr_rl_sep_fused_supported(int pz, int py, int px);
/* `taps`: a DEVICE array of lsr_rl_sep_fused_taps_count() floats; lsr_rl_sep_fused_prepare_taps
 * fills the HOST image from the three PSF factors (host arrays of pz / py / px taps), the caller
 * uploads it once per PSF. The kernel reads it through the scalar cache. */
int lsr_rl_sep_fused_taps_count(void);
int lsr_rl_sep_fused_prepare_taps(const float* kz_host, int pz, const float* ky_host, int py,
                                  const float* kx_host, int px, float* taps_host);
int lsr_rl_sep_fused_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y,
                         float* x_a, float* x_b, float* x_out, int64_t Z, int64_t Y, int64_t X,
                         const float* taps, int pz, int py, int px, const float* nz,
                         const float* ny, const float* nx, int iters, float eps,
                         lsr_stream_t stream);

/*
 * The same one-launch iteration for PSFs that separate along y only, psf[a][b][c] = ky[b] * kzx[a][c]
 * (rl_fused_ysep.hip) -- the PSF of an oblique light sheet, tilted in (z, x) and Gaussian along y; SURVEY.md
 * section 8(d)'s secondary PSF.  Volumes as lsr_rl_sep_fused_f32 (y padded with a zero halo, x_a / x_b padded
 * working volumes, x_out dense or NULL).  `taps`: a DEVICE array of lsr_rl_ysep_fused_taps_count() floats whose
 * HOST image lsr_rl_ysep_fused_prepare_taps fills from ky (py taps) and kzx (pz x px, C order);
 * norm_table / norm_full: the full PSF's, as for lsr_correlate_dense_f32.  Compiled for pz <= 11 and
 * py, px <= 9 (lsr_rl_ysep_fused_supported; otherwise LSR_E_UNSUPPORTED: use lsr_correlate_zxy_padded_f32 twice
 * per iteration).  Results are bit-identical to that two-launch form.
 */
int lsr_rl_ysep_fused_supported(int pz, int py, int px);
int lsr_rl_ysep_fused_taps_count(void);
int lsr_rl_ysep_fused_prepare_taps(const float* ky_host, int py, const float* kzx_host, int pz, int px,
                                   float* taps_host);
int lsr_rl_ysep_fused_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y, float* x_a,
                          float* x_b, float* x_out, int64_t Z, int64_t Y, int64_t X, const float* taps,
                          int pz, int py, int px, const double* norm_table, float norm_full, int iters,
                          float eps, lsr_stream_t stream);

int lsr_rl_dense_f32(const float* y, float* x, float* ratio, int64_t Z, int64_t Y, int64_t X,
                     const float* psf, const float* psf_flipped, int pz, int py, int px,
                     const double* norm_table, int iters, float eps, lsr_stream_t stream);

/*
 * Tuned dense (non-separable) path: fp32-VALU-bound stencil on padded volumes, for PSFs with
 * pz <= 11 and py, px <= 9 (anything else: LSR_E_UNSUPPORTED, use the generic dense entries).
 *
 * The taps are prepared ONCE on the host and uploaded by the caller:
 *   n = lsr_dense_taps_count(pz, py, px)                    number of floats (or < 0)
 *   lsr_dense_prepare_taps(psf_host, pz, py, px, flip, taps_host)   HOST pointers, no GPU work;
 *       flip = 0: correlation with the PSF (H^T), flip = 1: with the reversed PSF (H = convolution)
 * and `taps` below is that array in DEVICE memory. `in` lives in a padded volume
 * (lsr_sep_padded_shape); `norm_table` as for lsr_correlate_dense_f32, `norm_full` = sum of taps.
 */
int lsr_dense_taps_count(int pz, int py, int px);
int lsr_dense_prepare_taps(const float* psf_host, int pz, int py, int px, int flip,
                           float* taps_host);

int lsr_correlate_dense_padded_f32(const float* in, int64_t in_pitch, int64_t in_plane,
                                   const float* aux, int64_t aux_pitch, int64_t aux_plane,
                                   float* out, int64_t out_pitch, int64_t out_plane, int64_t Z,
                                   int64_t Y, int64_t X, const float* taps, int pz, int py, int px,
                                   int epilogue, float eps, const double* norm_table,
                                   float norm_full, lsr_stream_t stream);

/*
 * One launch for a PSF that separates along y, psf[z][y][x] = ky[y] * kzx[z][x] (the tilted
 * light-sheet PSF): out = epilogue(correlate(in, psf), aux) with LSR_EPI_RATIO or LSR_EPI_UPDATE.
 * `taps_zx` = lsr_dense_prepare_taps of the pz x py x px array that holds kzx in its centre y row and
 * zeros elsewhere (flip = 1 for H x); `ky` = the py y taps on the device (reversed for H x);
 * norm_table / norm_full = those of the full PSF.  pz*px + py FMAs per voxel instead of pz*py*px.
 * Volumes and strides as lsr_correlate_dense_padded_f32.
 */
int lsr_correlate_zxy_padded_f32(const float* in, int64_t in_pitch, int64_t in_plane,
                                 const float* aux, int64_t aux_pitch, int64_t aux_plane, float* out,
                                 int64_t out_pitch, int64_t out_plane, int64_t Z, int64_t Y, int64_t X,
                                 const float* taps_zx, const float* ky, int pz, int py, int px,
                                 int epilogue, float eps, const double* norm_table, float norm_full,
                                 lsr_stream_t stream);
int lsr_rl_dense_padded_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y,
                            float* x_pad, float* ratio_pad, float* x_out, int64_t Z, int64_t Y, int64_t X,
                            const float* taps, const float* taps_flipped, int pz, int py, int px,
                            const double* norm_table, float norm_full, int iters, float eps,
                            lsr_stream_t stream);

/*
 * Axial PSFs beyond 15 taps: 1-D correlation along z with up to lsr_correlate_z_max_taps() (31) odd taps and the RL
 * epilogues (csrc/correlate_z.hip) -- the z half of a separable PSF whose in-plane factors run through
 * lsr_correlate_sep_strided_f32 with ONE z tap: H x = Cz(Cyx(x)), two launches per correlation, four per iteration.
 * Any strides (floats; rows may be padded), no halo needed, `in` != `out`; `out` may alias `aux`.  UPDATE divides by
 * nz[z] * ny[y] * nx[x] and adds the launch's RL scalars to stats[0..2] when that is not NULL (see below).
 */
int lsr_correlate_z_max_taps(void);
int lsr_correlate_z_f32(const float* in, int64_t in_pitch, int64_t in_plane, const float* aux, int64_t aux_pitch,
                        int64_t aux_plane, float* out, int64_t out_pitch, int64_t out_plane, int64_t Z, int64_t Y,
                        int64_t X, const float* wz, int pz, int epilogue, float eps, const float* nz, const float* ny,
                        const float* nx, double* stats, lsr_stream_t stream);

/*
 * Total-variation factor of a regularised Richardson-Lucy iteration (RL-TV, Dey et al. 2006; csrc/rl_tv.hip):
 *
 *   out(r) = v(r) / (1 - lambda * div(r)),   div(r) = sum_a p_a(r) - p_a(r - e_a),   p_a = D_a u / n,
 *   D_a u(r) = u(r + e_a) - u(r) (0 where r + e_a is outside),   n = sqrt(D_z^2 + D_y^2 + D_x^2 + tv_eps^2),
 *   p_a(r - e_a) := 0 where r - e_a is outside
 *
 * with u = x_k (what the RL launches of the iteration read) and v = the plain RL update they wrote.  The borders are
 * those of (Z, Y, X): nothing outside the logical volume is read, so u / v may be the logical origin of zero-haloed
 * padded volumes and `out` a dense tensor.  Pitches and plane strides in elements (rows may be padded).  `out` may alias
 * v (same pointer and strides) and must not overlap u.  lambda in [0, 1/6) (|div| <= 6: the denominator stays
 * positive), tv_eps > 0 with tv_eps^2 a normal float32; anything else is LSR_E_ARG.  Where u is locally constant
 * out == v bit for bit; v == 0 gives an exact 0.  stats2 (DEVICE memory, or NULL): the launch ADDS
 * change = sum |out - u| and total = sum out to stats2[0], stats2[1] -- the reduction scheme of the RL epilogues (below),
 * the caller zeroes them.  A z-marching LDS stencil, 12 algorithmic bytes per voxel.
 */
int lsr_rl_tv_scale_f32(const float* u, int64_t u_pitch, int64_t u_plane, const float* v, int64_t v_pitch,
                        int64_t v_plane, float* out, int64_t o_pitch, int64_t o_plane, int64_t Z, int64_t Y, int64_t X,
                        float lambda, float tv_eps, double* stats2, lsr_stream_t stream);

/*
 * Accelerated Richardson-Lucy: the vector extrapolation of Biggs & Andrews (Appl. Opt. 36, 1997) around the unchanged
 * RL launches (csrc/rl_accel.hip).  With RL(.) one plain iteration and p_0 = x_0, iteration k runs x_{k+1} = RL(p_k) and,
 * unless it is the last one, the two launches below on the same stream:
 *
 *   g_k     = x_{k+1} - p_k                                                     (float32)
 *   a_{k+1} = 0 for k = 0, else clamp(<g_k, g_{k-1}> / <g_{k-1}, g_{k-1}>, 0, 1); 0 for a zero denominator
 *   p_{k+1} = max(fma(a_{k+1}, x_{k+1} - x_k, x_{k+1}), 0)                      (float32; a_{k+1} rounded to float32 once)
 *
 * lsr_rl_accel_dots_f32: reads x1 = x_{k+1} and p = p_k (strided: pointer, row pitch and plane stride in elements, so the
 * logical origin of a padded working volume goes in directly), reads the dense g = g_{k-1} (Z*Y*X floats) and writes g_k
 * over it; `first` != 0 (k = 0): g is only written and <g_0, g_{-1}> := 0.  Leaves dots2[0] = <g_k, g_{k-1}> and
 * dots2[1] = <g_k, g_k> (DEVICE memory): float64 sums of float64 products, bit-reproducible from run to run -- every
 * workgroup stores its partial sums into `workspace` (lsr_rl_accel_workspace_bytes(Z, Y, X) bytes of DEVICE memory, 8-byte
 * aligned; a function of the shape alone) and a second kernel adds them in index order; no floating-point atomics.  g must
 * not overlap x1 or p.  16 algorithmic bytes per voxel.
 *
 * lsr_rl_accel_predict_f32: reads x1 = x_{k+1}, reads x0 = x_k and writes p_{k+1} over it (strided; only the logical
 * volume is touched).  a_{k+1} is formed on the device from *num = <g_k, g_{k-1}> and *den = <g_{k-1}, g_{k-1}> (DEVICE
 * memory: dots2[0] of this iteration's dots launch and dots2[1] of the one before); den == NULL is the first step:
 * a_1 = 0, p_1 = max(x_1, 0), x0 is not read.  alpha_out (DEVICE memory, or NULL) receives a_{k+1} as a double.  x0 must
 * not overlap x1.  12 algorithmic bytes per voxel.
 */
int lsr_rl_accel_workspace_bytes(int64_t Z, int64_t Y, int64_t X);
int lsr_rl_accel_dots_f32(const float* x1, int64_t x1_pitch, int64_t x1_plane, const float* p, int64_t p_pitch,
                          int64_t p_plane, float* g, int64_t Z, int64_t Y, int64_t X, int first, double* dots2,
                          void* workspace, lsr_stream_t stream);
int lsr_rl_accel_predict_f32(const float* x1, int64_t x1_pitch, int64_t x1_plane, float* x0, int64_t x0_pitch,
                             int64_t x0_plane, int64_t Z, int64_t Y, int64_t X, const double* num, const double* den,
                             double* alpha_out, lsr_stream_t stream);

/*
 * Richardson-Lucy reduction scalars (the north-star's "wavefront reductions for the ratio / normalisation").
 * Every entry that finishes an RL iteration has a `_stats` form with one more argument, `double* stats` (DEVICE memory;
 * host memory for the *_cpu twins); NULL = the plain entry, the same kernels, no cost.  Per iteration i three sums over
 * the voxels of the volume, formed in the epilogue that writes x_{i+1} (no extra pass, no extra HBM byte):
 *
 *   stats[3 i + 0]  flux    sum x_i * H^T(ratio_i)  ==  sum x_{i+1} * H^T 1   -- what the multiplicative update
 *                           conserves: equals sum_v y_v (H x_i)_v / ((H x_i)_v + eps), i.e. sum y as eps -> 0
 *   stats[3 i + 1]  change  sum |x_{i+1} - x_i|                                -- the update norm
 *   stats[3 i + 2]  total   sum x_{i+1}
 *
 * change / total is the relative change a caller can stop on (the Python host: richardson_lucy(..., tol=)).  Per thread
 * the sums run in f32 over the voxels it owns, then wavefront reduction (DPP) -> LDS -> one f64 atomic add per workgroup
 * and sum; the only run-to-run freedom is the order of those f64 adds (~1e-16 relative).
 *   lsr_rl_*_stats_f32:        stats = 3 * iters doubles, zeroed by the entry on `stream` before the first launch;
 *   lsr_correlate_*_stats_f32: stats = 3 doubles the launch ADDS to (LSR_EPI_UPDATE only; ignored for other epilogues):
 *                              the caller zeroes them -- these are the per-launch building blocks of the loops above.
 * Otherwise arguments, limits and results are exactly those of the entry without `_stats`.
 */
int lsr_rl_sep_fused_stats_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y,
                               float* x_a, float* x_b, float* x_out, int64_t Z, int64_t Y, int64_t X,
                               const float* taps, int pz, int py, int px, const float* nz,
                               const float* ny, const float* nx, int iters, float eps, double* stats,
                               lsr_stream_t stream);
int lsr_rl_sep_stats_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y,
                         float* x_pad, float* ratio_pad, float* x_out, int64_t Z, int64_t Y, int64_t X,
                         const float* kz, const float* kz_flipped, int pz,
                         const float* ky, const float* ky_flipped, int py, const float* kx,
                         const float* kx_flipped, int px, const float* nz, const float* ny,
                         const float* nx, int iters, float eps, double* stats, lsr_stream_t stream);
int lsr_rl_ysep_fused_stats_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y, float* x_a,
                                float* x_b, float* x_out, int64_t Z, int64_t Y, int64_t X, const float* taps,
                                int pz, int py, int px, const double* norm_table, float norm_full, int iters,
                                float eps, double* stats, lsr_stream_t stream);
int lsr_rl_dense_padded_stats_f32(const float* y, int64_t y_pitch, int64_t y_plane, int init_from_y,
                                  float* x_pad, float* ratio_pad, float* x_out, int64_t Z, int64_t Y, int64_t X,
                                  const float* taps, const float* taps_flipped, int pz, int py, int px,
                                  const double* norm_table, float norm_full, int iters, float eps, double* stats,
                                  lsr_stream_t stream);
int lsr_rl_dense_stats_f32(const float* y, float* x, float* ratio, int64_t Z, int64_t Y, int64_t X,
                           const float* psf, const float* psf_flipped, int pz, int py, int px,
                           const double* norm_table, int iters, float eps, double* stats, lsr_stream_t stream);
int lsr_correlate_sep_stats_f32(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                                int64_t X, const float* wz, int pz, const float* wy, int py,
                                const float* wx, int px, int epilogue, float eps, const float* nz,
                                const float* ny, const float* nx, double* stats, lsr_stream_t stream);
int lsr_correlate_dense_stats_f32(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                                  int64_t X, const float* w, int pz, int py, int px, int epilogue,
                                  float eps, const double* norm_table, double* stats, lsr_stream_t stream);
int lsr_correlate_sep_strided_stats_f32(const float* in, int64_t in_pitch, int64_t in_plane,
                                        const float* aux, int64_t aux_pitch, int64_t aux_plane,
                                        float* out, int64_t out_pitch, int64_t out_plane, int64_t Z,
                                        int64_t Y, int64_t X, const float* wz, int pz, const float* wy,
                                        int py, const float* wx, int px, int epilogue, float eps,
                                        const float* nz, const float* ny, const float* nx, double* stats,
                                        lsr_stream_t stream);
int lsr_correlate_dense_padded_stats_f32(const float* in, int64_t in_pitch, int64_t in_plane,
                                         const float* aux, int64_t aux_pitch, int64_t aux_plane,
                                         float* out, int64_t out_pitch, int64_t out_plane, int64_t Z,
                                         int64_t Y, int64_t X, const float* taps, int pz, int py, int px,
                                         int epilogue, float eps, const double* norm_table,
                                         float norm_full, double* stats, lsr_stream_t stream);
int lsr_correlate_zxy_padded_stats_f32(const float* in, int64_t in_pitch, int64_t in_plane,
                                       const float* aux, int64_t aux_pitch, int64_t aux_plane, float* out,
                                       int64_t out_pitch, int64_t out_plane, int64_t Z, int64_t Y, int64_t X,
                                       const float* taps_zx, const float* ky, int pz, int py, int px,
                                       int epilogue, float eps, const double* norm_table, float norm_full,
                                       double* stats, lsr_stream_t stream);

/*
 * Reductions and filters behind the DynaTrack shift estimators that run on the deskewed volume
 * (shrimpy/dynatrack/tracking.py). `scratch` = lsr_reduce_scratch_bytes() bytes of
 * device memory; outputs are device arrays; sums are fp64, reduced in a fixed order.
 *
 *   lsr_minmax_f32            out2 = {min, max} of n floats                         (:533-535, :583)
 *   lsr_histogram_f32         torch.histc(in, nbins, vmin, vmax) as uint32 counts   (:465, :586)
 *                             (n < 2^32 per call, LSR_E_UNSUPPORTED otherwise: add up pieces)
 *   lsr_weighted_centroid_f32 out4 = {sum w, sum w z, sum w y, sum w x}, w = max(v - background, 0)
 *                             (_intensity_center_of_mass, :596-649)
 *   lsr_mask_centroid_f32     the same with w = (v > threshold)  (_center_of_mass of a mask, :545-569)
 *   lsr_blur_reflect_f32      one axis (0 = z, 1 = y, 2 = x) of _gaussian_blur_3d (:386-422):
 *                             correlation with 2*radius+1 device taps, reflect borders
 *                             (index -k -> k; radius < axis length, radius <= 64); div != 0 maps
 *                             the input through (v - sub) / div first (the [0, 1] rescale, :533-535)
 */
int lsr_reduce_scratch_bytes(void);
int lsr_minmax_f32(const float* in, int64_t n, float* out2, void* scratch, lsr_stream_t stream);
int lsr_histogram_f32(const float* in, int64_t n, float vmin, float vmax, int nbins, unsigned* counts,
                      lsr_stream_t stream);
int lsr_weighted_centroid_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float background,
                              double* out4, void* scratch, lsr_stream_t stream);
int lsr_mask_centroid_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold,
                          double* out4, void* scratch, lsr_stream_t stream);
int lsr_blur_reflect_f32(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int axis,
                         const float* taps, int radius, float sub, float div, lsr_stream_t stream);
/* Which of its five kernels lsr_blur_reflect_f32 runs for these arguments (host only, nothing is launched; the
 * launcher itself switches on this answer): 0 contiguous (axis 2), 1 marching (radius <= 12, axis length >= 32),
 * 2 packed (two columns per lane: radius 13..28, even inner extent, axis length > 32, both arrays 8-byte aligned),
 * 3 tiled-128 (radius <= 60, axis length > 64), 4 tiled-64 (the rest); a negative status for what the launcher
 * refuses.  in_align_bytes / out_align_bytes stand in for the two addresses: any value with their low three bits --
 * the address modulo 16, or the alignment it is known to have (4, 8, 16). */
int lsr_blur_reflect_form(int64_t Z, int64_t Y, int64_t X, int axis, int radius, int in_align_bytes,
                          int out_align_bytes);
/*
 * Element-wise steps of _phase_cross_corr (:266-378); the FFTs between them are library calls.
 *   lsr_match_shape_f32       _match_shape: per axis reflect-pad (left = d / 2) or centre-crop to the FFT shape
 *   lsr_cross_power_c64       a <- a * conj(b) over n complex64 values (interleaved re, im)
 *   lsr_peak_abs_shifted_f32  argmax(fftshift(|in|)) as a flat index into the SHIFTED (Z, Y, X) array,
 *                             first maximum in that order (torch.argmax), without writing either
 */
int lsr_match_shape_f32(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* out, int64_t Zo,
                        int64_t Yo, int64_t Xo, lsr_stream_t stream);
int lsr_cross_power_c64(float* a, const float* b, int64_t n, lsr_stream_t stream);
/* dst[a][c][b] = src[a][b][c] for complex64 (8-byte) elements, out of place: the layout change between
 * the per-axis transforms of the cross-correlation's 3-D FFT (A = 1: a plain 2-D transpose). */
int lsr_transpose_last2_c64(const float* src, float* dst, int64_t A, int64_t B, int64_t C, lsr_stream_t stream);
/*
 * The z leg of the cross-correlation in one pass: g <- N * IFFT_z( f1 * conj( FFT_z(g) ) ) along the first axis of
 * g ([N][XC][Y] complex64: the moving volume's spectrum after its x and y transforms), f1 = the reference's fully
 * transformed spectrum in [XC][Y][N] (z contiguous), twiddles[k] = exp(-2 pi i k / N) (N complex64, device).  Replaces
 * transpose + forward z transform + cross power + inverse z transform + transpose (csrc/zcorr.hip).  N: 5-smooth, 2..256
 * (lsr_cross_correlate_z_supported; LSR_E_UNSUPPORTED otherwise -- callers keep the five-pass route).
 */
int lsr_cross_correlate_z_supported(int64_t n);
int lsr_cross_correlate_z_c64(const float* f1, float* g, const float* twiddles, int64_t N, int64_t Y, int64_t XC,
                              lsr_stream_t stream);
/*
 * The x leg of the same cross-correlation, each way in one kernel (csrc/rfft_rows.hip).  Row lengths X that are
 * multiples of 4 with X / 2 5-smooth and <= 2048 (lsr_rfft_rows_supported); tw_half[k] = exp(-2 pi i k / (X/2)),
 * k < X / 4, and tw_x[k] = exp(-2 pi i k / X), k <= X / 2 (complex64, device).
 * lsr_rfft_rows_t_c64: spec[z][k][y] = sum_n v(z, y, n) exp(-2 pi i k n / X), k <= X / 2, where v is `in`
 *   ((Zi, Yi, Xi) float32) reflect-padded / centre-cropped to the grid (Z, Y, X) the way _match_shape does
 *   (tracking.py:266-306: pad left = d // 2, crop start = d // 2) -- the padded volume is never written.
 *   Replaces _match_shape + the real-to-complex transform along x + the transpose to y-contiguous.
 * lsr_irfft_rows_peak: the flat index of max |corr| in fftshift order (ties: the smallest), corr = the
 *   unnormalised complex-to-real inverse along x of spec ([Z][X/2+1][Y]); corr is never written.  `scratch`:
 *   lsr_rfft_rows_scratch_bytes(Z, Y) bytes.  Replaces the transpose back, irfft along x, fftshift(abs()), argmax.
 */
int lsr_rfft_rows_supported(int64_t n);
int64_t lsr_rfft_rows_scratch_bytes(int64_t Z, int64_t Y);
int lsr_rfft_rows_t_c64(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* spec, int64_t Z, int64_t Y,
                        int64_t X, const float* tw_half, const float* tw_x, lsr_stream_t stream);
int lsr_irfft_rows_peak(const float* spec, int64_t Z, int64_t Y, int64_t X, const float* tw_half, const float* tw_x,
                        long long* out_index, void* scratch, lsr_stream_t stream);
/*
 * Richardson-Lucy in the Fourier domain (shrimpy_amd/deconvolve_fft.py): PSFs beyond the stencil kernels' extents --
 * a measured bead PSF is a dense 15 x 18 x 18 ... 30 x 36 x 18 voxel patch (/root/reference/scripts/measure_psf.py:187-190)
 * -- cost the same as any other there.  No reference code for RL itself (/root/reference/docs/data_structure.md:58-62);
 * the arithmetic is that of the stencil path: x <- x * H^T( y / (H x + eps) ) / H^T 1, zero-padded
 * borders, with H x and H^T r evaluated as products of spectra on a grid (Z, Y, X) >= volume + PSF radius per axis.
 * lsr_rfft_rows_zero_t_c64: as lsr_rfft_rows_t_c64 with the source ((Zi, Yi, Xi) <= grid) at the grid's origin and
 *   zeros behind it -- a linear convolution, not a circular one; tiles of padding rows (y >= Yi) in the source's planes
 *   store zeros without a transform, planes z >= Zi are NOT written (see z_valid below).
 * lsr_spectrum_multiply_z_c64: g <- N * IFFT_z( f1 * FFT_z(g) ) (conj_f1 = 0: H x) or N * IFFT_z( conj(f1) * FFT_z(g) )
 *   (conj_f1 = 1: H^T r); layouts and lengths as lsr_cross_correlate_z_c64, f1 = the PSF's spectrum (its centre tap at
 *   the grid's origin, wrapped).  z_valid: planes [z_valid, N) of g are the zero padding behind the volume -- taken as
 *   zeros and never read, so the forward x and y legs need not produce them; z_keep: only planes [0, z_keep) of the
 *   result are stored -- the inverse y and x legs read no others (N, N = everything).
 * lsr_irfft_rows_rl_f32: the inverse x leg with the iteration's epilogue.  v = scale * (complex-to-real inverse of
 *   spec along x) on the grid's first (Zo, Yo, Xo) points, scale = 1 / (Z Y X);
 *     LSR_EPI_RATIO:  out = aux / (max(v, 0) + eps)    aux = y
 *     LSR_EPI_UPDATE: out = aux * v / H^T 1            aux = x; H^T 1 = norm_full inside, from norm_table ((pz+1)(py+1)
 *                     (px+1) prefix sums of the PSF, float64, device) within a PSF radius of the border; stats = 3 doubles
 *                     the launch ADDS the iteration's flux / change / total to (as lsr_correlate_*_stats_f32) or NULL;
 *                     px <= 129 (LSR_E_UNSUPPORTED beyond: the border lookup covers a radius of 64 columns).
 *   out may be aux (in place).  The convolved volume is never written.
 * lsr_rl_rows_chain_f32: the same, CHAINED into the forward x leg of the iteration's next convolution: the epilogue's
 *   output row is zero-padded, transformed and stored back over its tile of `spec`, which afterwards holds what
 *   lsr_rfft_rows_zero_t_c64(out) would have produced (tiles of pure padding: zeros).  LSR_EPI_RATIO: `out` may be NULL --
 *   the ratio then never exists in memory; LSR_EPI_UPDATE stores x_new once and nobody reads it back for the transform.
 */
int lsr_rfft_rows_zero_t_c64(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* spec, int64_t Z, int64_t Y,
                             int64_t X, const float* tw_half, const float* tw_x, lsr_stream_t stream);
int lsr_spectrum_multiply_z_c64(const float* f1, float* g, const float* twiddles, int64_t N, int64_t Y, int64_t XC,
                                int conj_f1, int64_t z_valid, int64_t z_keep, lsr_stream_t stream);
int lsr_irfft_rows_rl_f32(const float* spec, int64_t Z, int64_t Y, int64_t X, const float* tw_half, const float* tw_x,
                          int epilogue, const float* aux, float* out, int64_t Zo, int64_t Yo, int64_t Xo, float scale,
                          float eps, int pz, int py, int px, const double* norm_table, float norm_full, double* stats,
                          lsr_stream_t stream);
int lsr_rl_rows_chain_f32(float* spec, int64_t Z, int64_t Y, int64_t X, const float* tw_half, const float* tw_x,
                          int epilogue, const float* aux, float* out, int64_t Zo, int64_t Yo, int64_t Xo, float scale,
                          float eps, int pz, int py, int px, const double* norm_table, float norm_full, double* stats,
                          lsr_stream_t stream);
/*
 * Label-free 3-D phase reconstruction (csrc/phase.hip, shrimpy_amd/phase.py): the x legs of a Tikhonov inverse filter
 * applied in the Fourier domain to a volume that is periodically MIRROR-extended onto the transform grid (Z, Y, X); the
 * y leg is hipFFT, the z leg lsr_spectrum_multiply_z_c64 with the filter in [XC][Y][Z] (conj_f1 = 0, z_valid = Z).
 * Mirror rule per axis (n samples, grid g, index i): i < n is sample i; otherwise, with a = i - n and b = g - 1 - i,
 * sample n - 1 - min(a, n - 1) if a <= b, else sample min(b, n - 1).  Row lengths, tw_half and tw_x as lsr_rfft_rows_t_c64.
 * lsr_phase_rows_forward_c64: spec[z][k][y] = sum_n v(z, y, n) exp(-2 pi i k n / X) for EVERY row of the grid, v = `in`
 *   ((Zi, Yi, Xi) <= grid, float32) extended by the rule on all three axes (never written).  mean[0] <- the float64 mean
 *   of `in`, mean[1] <- its sum: one partial per workgroup in `partial` (lsr_phase_rows_scratch_bytes(Z, Y) bytes, device,
 *   8-byte aligned), reduced in a fixed order by a second launch (the same bits on every call).
 * lsr_phase_rows_inverse_f32: out ((Zo, Yo, Xo) float32) = the complex-to-real inverse of spec along x on the grid's first
 *   (Zo, Yo, Xo) points, times 1 / (Z Y X mean[0]), mean read on the device (no host synchronisation in between).
 */
int64_t lsr_phase_rows_scratch_bytes(int64_t Z, int64_t Y);
int lsr_phase_rows_forward_c64(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* spec, int64_t Z, int64_t Y,
                               int64_t X, const float* tw_half, const float* tw_x, double* partial, double* mean,
                               lsr_stream_t stream);
int lsr_phase_rows_inverse_f32(const float* spec, int64_t Z, int64_t Y, int64_t X, const float* tw_half, const float* tw_x,
                               const double* mean, float* out, int64_t Zo, int64_t Yo, int64_t Xo, lsr_stream_t stream);
/*
 * Mid-band spectral power of every z plane (csrc/focus.hip, shrimpy_amd/focus.py): the focus measure of the time-lapse
 * stabilization, waveorder's focus_from_transverse_band -- not vendored, PARITY UNPINNED, the rule is defined here
 * (tests/focus_ref.py restates it).  The window (Yc, Xc) at (y0, x0) of every plane of `in` ((Z, Y, X) float32) is
 * transformed, F = fft2(window) unnormalised, and
 *   out_power[z] = sum of |F(ky, kx)| over the bins with band_lo < r < band_hi,
 *   r = sqrt((min(ky, Yc - ky) / (Yc pixel_size))^2 + (min(kx, Xc - kx) / (Xc pixel_size))^2)   (float64, both strict).
 * Lengths (lsr_band_power_supported, LSR_E_UNSUPPORTED otherwise): Xc as lsr_rfft_rows_supported, Yc 5-smooth in [2, 2048].
 * lsr_band_power_plan (host only): decides the inequalities in float64.  table (host, 2 * (Xc / 2 + 1) int32): for every
 *   column kx <= Xc / 2 of the half spectrum the closed interval [table[2 kx], table[2 kx + 1]] of min(ky, Yc - ky) inside
 *   the band (a > b: none).  *k_hi <- the last column that holds a bin (-1: the band is empty), *weighted_bins (may be
 *   NULL) <- the number of bins of the full spectrum inside the band.
 * lsr_band_power_scratch_bytes: *spec_bytes, *partial_bytes <- the sizes of spec_scratch and partial (device, 8-byte aligned).
 * lsr_band_power_f32: table = the first 2 * (k_hi + 1) entries of the plan, in device memory; tw_half, tw_x as
 *   lsr_rfft_rows_t_c64 for the length Xc; tw_y = exp(-2 pi i k / Yc), k < Yc, complex64.  Three launches: the x leg keeps
 *   only the columns kx <= k_hi (spec_scratch[z][kx][y], complex64), the y leg transforms eight columns per workgroup in LDS
 *   and adds |F| over each column's interval and its mirror rows, columns 0 < kx < Xc / 2 twice, in float64 -- one partial
 *   per workgroup; out_power (Z float64, device) <- the partials of each plane added in a fixed order: the same bits on every
 *   call, no atomics.  The cropped volume and the y-transformed spectrum are never written.
 * lsr_band_power_f32_cpu: the same arguments as host pointers (tw_*, spec_scratch and partial are unused and may be NULL),
 *   float64 transforms: a host route for machines without a GPU, close to but not bit-equal with the kernels.
 */
int lsr_band_power_supported(int64_t Yc, int64_t Xc);
int lsr_band_power_plan(int64_t Yc, int64_t Xc, double pixel_size, double band_lo, double band_hi, int32_t* table,
                        int64_t* k_hi, int64_t* weighted_bins);
int lsr_band_power_scratch_bytes(int64_t Z, int64_t Yc, int64_t k_hi, int64_t* spec_bytes, int64_t* partial_bytes);
int lsr_band_power_f32(const float* in, int64_t Z, int64_t Y, int64_t X, int64_t y0, int64_t x0, int64_t Yc, int64_t Xc,
                       const float* tw_half, const float* tw_x, const float* tw_y, const int32_t* table, int64_t k_hi,
                       float* spec_scratch, double* partial, double* out_power, lsr_stream_t stream);
int lsr_band_power_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, int64_t y0, int64_t x0, int64_t Yc, int64_t Xc,
                           const float* tw_half, const float* tw_x, const float* tw_y, const int32_t* table, int64_t k_hi,
                           float* spec_scratch, double* partial, double* out_power, lsr_stream_t stream);
/* b <- a * conj(b): the same product written over the second operand, so that `a` (the spectrum of
 * a reference volume that is compared against many timepoints) can be kept. */
int lsr_cross_power_into_c64(const float* a, float* b, int64_t n, lsr_stream_t stream);
int lsr_peak_abs_shifted_f32(const float* in, int64_t Z, int64_t Y, int64_t X, long long* out_index,
                             void* scratch, lsr_stream_t stream);

/*
 * Bead detection and PSF averaging (csrc/peaks.hip, shrimpy_amd/psf.py): what scripts/measure_psf.py hands to biahub's
 * _characterize_psf, which is not vendored -- PARITY UNPINNED, the rule is defined here (tests/psf_ref.py restates it).
 * lsr_box_smooth_f32: the smoothing in front of the detection: `taps` (odd, <= 129, taps / 2 < every extent) equal weights
 *   `tap` per axis, mirrored borders (index -k -> k: scipy.ndimage.correlate1d(mode="mirror")), one launch per axis with
 *   float64 sums in tap order and float64 results between the passes, rounded to float32 once -- within one unit of 2^-24
 *   of the float64 filter per voxel (three chained float32 passes reach 3 and can reach 4.5).  `scratch`:
 *   lsr_box_smooth_scratch_bytes(Z, Y, X, &bytes) bytes of device memory, 8-byte aligned.  out must not be in.
 * lsr_local_max_candidates_f32: the peaks of the (smoothed) volume s under a box window of half-widths (rz, ry, rx) <= 64
 *   (LSR_E_UNSUPPORTED beyond).  Voxel p is a peak iff s(p) >= threshold, s(p) >= s(q) for every in-volume q of its window
 *   and s(p) > s(q) for every such q of smaller linear index (ties: the first in C order); NaNs are never peaks and leave
 *   no peak within their reach.  Every peak is appended, in no particular order, as (linear index, value) to cand_index /
 *   cand_value (`capacity` entries each, device) through *count (one device counter, zeroed by the call); the counter
 *   keeps counting past the capacity while nothing is stored there, so *count > capacity afterwards means the buffers were
 *   too small.  `scratch`: lsr_local_max_scratch_bytes(Z, Y, X, &bytes) bytes of device memory (two volumes: s dilated
 *   along x, and that along y -- the passes of lsr_grey_morph_f32; the z pass carries the test and stores no volume).  One
 *   launch per axis with a half-width > 0 and always the z one: at most three, no host synchronisation.
 * lsr_psf_accumulate_f32: psf (pz * py * px float32, odd extents <= 129) = the mean over the contributing beads of
 *   (patch - B) / S, patches centred on the linear indices `centres` (n_beads, device), B = the float64 mean of the patch's
 *   outer shell (its six faces), S = sum(patch - B) in float64 in a fixed order; bead_stats (n_beads x {B, S}, float64,
 *   device) is written for the caller.  A bead with S <= 0 (or whose patch does not fit the volume: B = S = 0) contributes
 *   nothing; with no contributing bead the result is zeros.  Float64 accumulation in list order: reproducible bits.
 */
int lsr_box_smooth_scratch_bytes(int64_t Z, int64_t Y, int64_t X, int64_t* bytes);
int lsr_box_smooth_f32(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int taps, float tap, void* scratch,
                       lsr_stream_t stream);
int lsr_local_max_scratch_bytes(int64_t Z, int64_t Y, int64_t X, int64_t* bytes);
int lsr_local_max_candidates_f32(const float* s, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, float threshold,
                                 long long* cand_index, float* cand_value, int64_t capacity, unsigned long long* count,
                                 void* scratch, lsr_stream_t stream);
int lsr_psf_accumulate_f32(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n_beads,
                           int pz, int py, int px, double* bead_stats, float* psf, lsr_stream_t stream);

/*
 * Per-bead Gaussian fits and the sub-voxel aligned PSF average (csrc/psf_fit.hip, csrc/psf_fit.hpp; shrimpy_amd/psf.py:
 * fit_beads, average_psf_aligned).  PARITY UNPINNED as above; tests/psf_fit_ref.py restates both.
 * lsr_bead_fit_f32: for each of the n_beads patches (odd extents <= 129, centred on the linear indices `centres`, device)
 *   the unweighted least-squares fit of  m(r) = B + A exp(-1/2 (r - mu)^T W (r - mu)),  r = the voxel offset from the
 *   centre voxel, by Levenberg-Marquardt with Marquardt's diagonal scaling in float64 (lambda from 1e-3, / 10 on an
 *   accepted step, * 10 on a rejected one; at most max_iter >= 1 trial cost evaluations; start and stopping rule:
 *   csrc/psf_fit.hpp).  One workgroup per bead, one launch.  fit (n_beads x 12 float64, device): B, A, mu_z, mu_y, mu_x,
 *   w_zz, w_yy, w_xx, w_zy, w_zx, w_yx, then the final sum of squared residuals.  status (n_beads int, device): 0 converged,
 *   1 iteration limit, 2 the damped system or the final W not positive definite, 3 some |mu_i| >= 1, 4 A <= 0, 5 a
 *   non-finite voxel in the patch or a patch that does not fit the volume (nothing outside the volume is read); every
 *   status but 0 leaves NaN in the bead's twelve numbers.  Device and twin agree to rounding (exp and the order of the
 *   sums differ), not to the bit.
 * lsr_psf_accumulate_shifted_f32: lsr_psf_accumulate_f32 with every patch moved by a sub-voxel offset before it is added:
 *   c = patch - B goes through three separable circulant passes, x, then y, then z, out[i] = sum_j c[j] w[(i - j) mod N]
 *   with j ascending in unfused float64; shifted / S is added in list order, psf = float(acc / used).  `weights`
 *   (n_beads x (pz + py + px) float64, device; per bead the z, the y, then the x axis) are the CALLER's: for an offset mu
 *   along an axis of N voxels w[k] = D_N(k + mu), D_N(t) = sin(pi t) / (N sin(pi t / N)), the periodic-sinc (Fourier)
 *   shift -- an input, so that kernel and twin can be held to the same bits.  A bead with S <= 0, a patch that does not
 *   fit or a non-finite weight contributes nothing.  bead_stats as lsr_psf_accumulate_f32 writes it.  Beads go through
 *   `scratch` in batches of 64: lsr_psf_shift_scratch_bytes(n_beads, pz, py, px, &bytes) bytes of device memory, 8-byte
 *   aligned (the float64 accumulator and two float64 patches per bead of a batch).  2 launches per batch + 2.
 */
int lsr_bead_fit_f32(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n_beads, int pz,
                     int py, int px, int max_iter, double* fit, int* status, lsr_stream_t stream);
int lsr_psf_shift_scratch_bytes(int64_t n_beads, int pz, int py, int px, int64_t* bytes);
int lsr_psf_accumulate_shifted_f32(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                                   int64_t n_beads, int pz, int py, int px, double* bead_stats, const double* weights,
                                   void* scratch, float* psf, lsr_stream_t stream);

/*
 * One level of a multiscale pyramid (csrc/pyramid.hip, shrimpy_amd/pyramid.py): the 2x mean of the level above it,
 * factors (fz, 2, 2) with fz 1 or 2 (LSR_E_ARG otherwise) -- iohub's compute_pyramid is not vendored, PARITY UNPINNED,
 * the rule is defined here (tests/pyramid_ref.py restates it).  The output has ceil(n / f) voxels per axis
 * (lsr_downsample2_shape: out3 <- (Zo, Yo, Xo), host only); output voxel (z, y, x) is the mean over the input voxels
 * (fz z + a, 2 y + b, 2 x + c), a < fz, b < 2, c < 2, INSIDE the volume: nothing is padded, nothing dropped, a window
 * holds 1, 2, 4 or 8 = 2^k voxels.
 *   float32: s = ((v000 + v001) + (v010 + v011)) + ((v100 + v101) + (v110 + v111)), v[a][b][c]: x pairs, then y, then z,
 *     float32 additions, a neighbour outside the volume left out (never added as zero); out = s * 2^-k, exact.  Three
 *     roundings: |out - exact| <= 3 * 2^-24 * mean|v| over the window.  A NaN or Inf reaches its own window only.
 *   uint16: the sum in 32 bits, out = (sum + (2^k >> 1)) >> k: round half up, exact.
 * in (Z, Y, X) and out (Zo, Yo, Xo) are dense C-order device volumes that must not overlap; any X, any row alignment,
 * volumes beyond 2^31 bytes (64-bit indices).  One launch, no scratch, no LDS.
 */
int lsr_downsample2_shape(int64_t Z, int64_t Y, int64_t X, int fz, int64_t out3[3]);
int lsr_downsample2_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int fz, lsr_stream_t stream);
int lsr_downsample2_u16(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, uint16_t* out, int fz, lsr_stream_t stream);

/*
 * Stitching (csrc/stitch.hip, shrimpy_amd/stitch.py): K overlapping tiles composed into one box of their common canvas --
 * biahub's stitch is not vendored, PARITY UNPINNED, the rule is defined in csrc/stitch.hpp (tests/stitch_ref.py restates
 * it in float64).  Tile k is a dense float32 (Zk, Yk, Xk) with a float64 translation t_k (z, y, x) in canvas voxels: tile
 * voxel i sits at canvas coordinate i + t_k.  lsr_stitch_canvas (host only): origin = floor(min_k t_k),
 * shape = ceil(max_k (t_k + n_k)) - origin.
 *   Per tile and axis: ti = floor(t), tf = t - ti (float64, host); j = c - ti for the absolute canvas index c.  tf == 0:
 *   one tap i = j, covered iff 0 <= j <= n - 1; otherwise the taps j - 1 and j with the float32 weights float32(tf) and
 *   float32(1 - tf), covered iff 1 <= j <= n - 1.  A tile covers a voxel iff all three axes are covered; nothing is
 *   interpolated against cval.  The sample s_k interpolates over the fractional axes only (x, then y, then z; two products
 *   and one sum per axis, unfused); the weight is w_k = (dy dx)^p, p in 0 .. 4 by repeated multiplication,
 *   d = min(float(j) + float32(1 - tf), float(n - j) + float32(tf)): the distance to the nearer tile edge counted from 1.
 *   out = cval where no tile covers the voxel, s_k itself where exactly one does (an integer placement copies bits),
 *   (sum w_k s_k) / (sum w_k) in float32 in ascending tile index otherwise.
 * The tile table is lsr_stitch_table_bytes(n_tiles) bytes (0 for a count outside 1 .. lsr_stitch_max_tiles()), filled on
 * the HOST by lsr_stitch_prepare_table from the tiles' addresses (device addresses for lsr_stitch_f32), their shapes
 * (n_tiles x 3, int64) and translations (n_tiles x 3, float64) -- a NULL tile is LSR_E_NULL, a non-positive extent
 * LSR_E_SHAPE, a count over the cap or a y / x extent over 2^24 LSR_E_UNSUPPORTED, a translation that is not finite or reaches 2^30 LSR_E_ARG -- and
 * then copied to device memory by the caller.  lsr_stitch_f32 writes `out`, a dense box of the canvas given by its origin
 * and shape in absolute canvas coordinates (|origin| < 2^31); tiles outside the box contribute nothing, so a canvas can be
 * composed box by box with the same bits.  One launch for a box of any size, every voxel of the box written once, nothing
 * else written; no scratch, no LDS, no atomics.  `out` must not overlap a tile.
 */
int lsr_stitch_max_tiles(void);
int lsr_stitch_table_bytes(int n_tiles);
int lsr_stitch_canvas(const int64_t* shapes, const double* translations, int n_tiles, int64_t origin[3], int64_t shape[3]);
int lsr_stitch_prepare_table(const float* const* tiles, const int64_t* shapes, const double* translations, int n_tiles,
                             void* table);
int lsr_stitch_f32(const void* table, int n_tiles, float* out, const int64_t box_origin[3], const int64_t box_shape[3],
                   int p, float cval, lsr_stream_t stream);

/*
 * Connected-component labelling and the object table (csrc/label.hip, shrimpy_amd/segment.py).  The oracle is
 * scipy.ndimage.label (tests/label_ref.py), held to exact equality.
 *   Foreground is in[v] > threshold: NaN and the threshold itself are background.  connectivity is 6, 18 or 26, the
 *   neighbourhoods scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3) (LSR_E_ARG otherwise).  labels (int32, Z * Y * X)
 *   receives 0 on the background and 1 .. N on the components, numbered in raster (C-order) rank of each component's
 *   lowest linear index; *n_objects (int32, device memory for lsr_label_f32) receives N.  A volume holds at most
 *   2^31 - 1 voxels (LSR_E_UNSUPPORTED beyond); a NULL pointer is LSR_E_NULL, a non-positive extent LSR_E_SHAPE.
 * lsr_label_tile_shape: the (z, y, x) tile one workgroup labels in LDS.  lsr_label_scratch_bytes: the size of `scratch`
 * (device memory; its contents on entry do not matter), or a negative status for a shape out of range.
 * lsr_label_launch_geometry: {threads per workgroup, voxels per workgroup of the numbering launches, threads of the one
 * workgroup that scans their counts, the cap of the grid-stride launches' grids, the cap of the local launch's grid}: a
 * volume with more work than a cap is walked with a grid stride, a volume of more numbering workgroups than scan threads
 * gives every scan thread several counts.
 * lsr_label_f32 runs seven launches on `stream` -- local (one tile per workgroup, the threshold fused into the load),
 * merge (unions across tile faces, atomicMin on the parent words), flatten, count, scan, rank, final -- with the
 * union-find kept in `labels` itself; no workgroup ever waits for another (csrc/label.hip states the two rules).
 *
 * lsr_label_regions_f32: one 96-byte record per label 1 .. n_objects, in `table`, which the CALLER HAS ZEROED:
 *   int64 volume; int64 sum_z, sum_y, sum_x; float64 sum_v, sum_vz, sum_vy, sum_vx; int32 lo[3], hi[3] (the bounding box,
 *   half-open); float32 v_min, v_max.
 * The integer fields and the intensity range are exact and independent of the order of accumulation (integer atomics;
 * min / max on the order-preserving integer image of the float); the float64 sums are float64 atomic adds of per-wave
 * partial sums: within n_k * 2^-53 * sum|terms| of the exact sum, not reproducible to the bit.  `intensity` may be NULL:
 * the intensity fields then stay zero.  A label outside 1 .. n_objects is ignored; a label no voxel carries keeps a zero
 * record.  n_objects == 0 returns at once (table may be NULL).  Two launches.
 *
 * lsr_label_remap_i32: labels[v] = map[labels[v]] in place, map holding n_map int32 entries (map[0] is the background's
 * and must be 0; a label outside 0 .. n_map - 1 becomes 0).  One launch.
 */
int lsr_label_tile_shape(int zyx[3]);
int lsr_label_launch_geometry(int64_t out[5]);
int lsr_label_scratch_bytes(int64_t Z, int64_t Y, int64_t X);
int lsr_label_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int connectivity, int32_t* labels,
                  int32_t* n_objects, void* scratch, lsr_stream_t stream);
int lsr_label_regions_f32(const int32_t* labels, const float* intensity, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                          void* table, lsr_stream_t stream);
int lsr_label_remap_i32(int32_t* labels, int64_t n, const int32_t* map, int64_t n_map, lsr_stream_t stream);
/* measurement only (tools/bench_kernels.py --label): lsr_label_f32 with a HIP event between its launches; waits for the
 * stream and writes the times of local, merge, flatten, count, scan, rank and final in milliseconds to ms7 (HOST memory) */
int lsr_label_profile_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int connectivity, int32_t* labels,
                          int32_t* n_objects, void* scratch, float* ms7, lsr_stream_t stream);

/*
 * The exact Euclidean distance transform and the label expansion (csrc/edt.hip, shrimpy_amd/distance.py).  The rule is
 * stated in csrc/edt.hpp:
 *   Sites are a set of voxels; sampling[3] = (sz, sy, sx) are three HOST doubles, positive and finite (LSR_E_ARG otherwise).
 *   nearest[v] (int32) is the linear index of a site that minimises (sz dz)^2 + (sy dy)^2 + (sx dx)^2, the SMALLEST linear
 *   index among equals; dist[v] (float32) is the float32 rounding of the float64
 *   sqrt(((sz*dz)*(sz*dz) + (sy*dy)*(sy*dy)) + (sx*dx)*(sx*dx)) to nearest[v] -- scipy.ndimage.distance_transform_edt(mask,
 *   sampling) bit for bit wherever the costs are exact in float64 (integer and dyadic spacings), within one float32 ulp
 *   otherwise.  A site has dist 0 and nearest v.  With NO site anywhere dist = +inf and nearest = -1 at every voxel: a
 *   deliberate difference from scipy, which measures from index -1 there.  The index rule is this library's (scipy's
 *   return_indices breaks ties differently).
 * lsr_edt_f32: the sites are the background !(in > threshold) -- NaN is background, as in lsr_label_f32 -- so the result is
 *   scipy's distance_transform_edt(in > threshold); with invert != 0 the sites are the foreground.
 * lsr_edt_labels_i32: the sites are labels != 0, with invert != 0 labels == 0.
 * Either of dist and nearest may be NULL, not both (LSR_E_NULL).  A volume holds at most 2^31 - 1 voxels
 * (LSR_E_UNSUPPORTED beyond); a non-positive extent is LSR_E_SHAPE.  Three launches on `stream` (x: the nearest site of each
 * row from wave ballots; y, z: the lower envelope of each line's parabolas, one lane per line, float64 costs), in place in
 * the output words; no launch communicates between workgroups.  `scratch` (device memory, lsr_edt_scratch_bytes(Z, Y, X)
 * bytes or a negative status; its contents on entry do not matter) holds the envelope stacks.
 * lsr_edt_tiling: {voxels per step of the x pass, lines per workgroup of the y and z passes, rows the x pass holds at once,
 * lines a y or z pass holds at once}: beyond the last two a wave or a lane takes a further row or line.
 *
 * lsr_label_expand_i32: out[v] = labels[nearest[v]] where nearest[v] >= 0 and the float64 distance of the rule from v to
 * nearest[v] is <= distance, 0 elsewhere.  One launch.  distance must not be negative or NaN, out must not alias labels
 * (LSR_E_ARG).  With nearest from lsr_edt_labels_i32(invert = 0) this is skimage.segmentation.expand_labels(labels,
 * distance, spacing=sampling) up to the tie rule above.
 */
int lsr_edt_tiling(int tiling[4]);
int64_t lsr_edt_scratch_bytes(int64_t Z, int64_t Y, int64_t X);
int lsr_edt_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int invert, const double sampling[3],
                float* dist, int32_t* nearest, void* scratch, lsr_stream_t stream);
int lsr_edt_labels_i32(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int invert, const double sampling[3], float* dist,
                       int32_t* nearest, void* scratch, lsr_stream_t stream);
int lsr_label_expand_i32(const int32_t* labels, const int32_t* nearest, int64_t Z, int64_t Y, int64_t X, const double sampling[3],
                         double distance, int32_t* out, lsr_stream_t stream);
/* measurement only (tools/bench_kernels.py --edt): lsr_edt_f32 with a HIP event between its launches; waits for the stream
 * and writes the times of the x, y and z passes in milliseconds to ms3 (HOST memory) */
int lsr_edt_profile_f32(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int invert, const double sampling[3],
                        float* dist, int32_t* nearest, void* scratch, float* ms3, lsr_stream_t stream);

/*
 * Flat grey-scale morphology under a box (csrc/morphology.hip, shrimpy_amd/morphology.py).  The rule is stated in
 * csrc/morphology.hpp; PINNED to scipy.ndimage.grey_erosion / grey_dilation / grey_opening / grey_closing / white_tophat /
 * black_tophat with size = 2r + 1, element for element on NaN-free volumes:
 *   in, out are contiguous (Z, Y, X) float32 volumes; the window is 2r + 1 wide per axis, half-widths (rz, ry, rx).
 *   erode(v)(p) is the least and dilate(v)(p) the greatest v(q) over the in-volume q of the box around p: voxels outside the
 *   volume do not compete, and a half-width may exceed the axis.  Values compare by the order-preserving integer image of a
 *   float (-0.0 below +0.0, +-inf ordinary values); the result is the bit pattern of the chosen element.  A window that holds
 *   a NaN gives the canonical quiet NaN 0x7fc00000, for erosion and dilation alike.
 *   op: 0 erode, 1 dilate, 2 open = dilate(erode), 3 close = erode(dilate), 4 white top-hat = in - open, 5 black top-hat =
 *   close - in; the top-hats are one IEEE float32 subtraction per voxel, fused into the last pass (a NaN it produces may carry
 *   any payload).  An axis with half-width 0 gets no pass; all three at 0 make ops 0 .. 3 a copy and ops 4, 5 in - in.
 * out must not alias in (LSR_E_ARG); a negative half-width or an unknown op is LSR_E_ARG, a half-width above the cap
 * LSR_E_UNSUPPORTED, a NULL pointer LSR_E_NULL, a non-positive extent LSR_E_SHAPE; nothing is launched or written then.  One
 * launch per axis with a half-width > 0 and per erosion or dilation (an opening: up to six); every launch reads each voxel of
 * its source once and writes each voxel of its target once, no launch communicates between workgroups.  `scratch` (device
 * memory, lsr_grey_morph_scratch_bytes(Z, Y, X) bytes -- two float volumes -- or a negative status; its contents on entry do
 * not matter) holds the results between the passes; `in` is never written and `out` exactly once.
 * lsr_grey_morph_tiling: {the greatest half-width per axis, columns per workgroup of the y and z passes, outputs per staged
 * row segment of the x pass, threads per workgroup of the x pass}.
 * lsr_grey_morph_dispatch: the edges at which the launches choose their code, from the constants they branch on: {the greatest
 * half-width of the narrow instantiation of the strided walk, the greatest half-width whose strip still fits static LDS (above
 * it the widest instantiation asks for dynamic LDS), the workgroups of the x pass at most (with more rows a workgroup strides
 * over them), the rows read ahead of the walk by the narrow, the static-LDS and the dynamic-LDS instantiation}.  For tests
 * that aim at those edges; it changes nothing.
 */
int lsr_grey_morph_tiling(int tiling[4]);
int lsr_grey_morph_dispatch(int dispatch[6]);
int64_t lsr_grey_morph_scratch_bytes(int64_t Z, int64_t Y, int64_t X);
int lsr_grey_morph_f32(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int op,
                       void* scratch, lsr_stream_t stream);

/*
 * Rank filters under a box: rank, median, percentile and outlier removal (csrc/rank.hip, shrimpy_amd/rank.py).  The rule is
 * stated in csrc/rank.hpp; PINNED to scipy.ndimage.rank_filter / median_filter / percentile_filter with size = 2r + 1 and
 * mode = "reflect", by value on NaN-free volumes:
 *   in, out are contiguous (Z, Y, X) float32 volumes; half-widths (rz, ry, rx), each in 0 .. 3, window 2r + 1 per axis, n
 *   elements; `rank` in 0 .. n - 1 (the median is n / 2).  The border is scipy's `reflect` (d c b a | a b c d): index i of an
 *   axis of length L reads m = i mod 2L, then m < L ? m : 2L - 1 - m; a half-width may exceed the axis, and reflected voxels
 *   count as often as they fall in the window.  m(p) is the rank-th smallest (from 0) of the window's values under the
 *   order-preserving integer image of a float (-0.0 below +0.0, +-inf ordinary values, a NaN the greatest and returned as
 *   the canonical quiet NaN 0x7fc00000); the result is the bit pattern of the chosen element.
 *   op, fused into the store (t = threshold, v the voxel, each difference one IEEE float32 subtraction, a comparison with a
 *   NaN false): 0 value: m; 1 remove_bright: (v - m > t) ? m : v; 2 remove_dark: (m - v > t) ? m : v; 3 remove_both: m where
 *   either holds, else v.  All half-widths 0: every op copies v, except that a NaN becomes the canonical one under op 0.
 *   variant: 0 dispatches the half-width triples of {0, 1}^3 to kernels that hold the window in registers and every other
 *   window to the generic kernel, 1 forces the generic kernel; both give the same bytes.
 * out must not alias in (LSR_E_ARG); a negative half-width, a rank outside 0 .. n - 1, an unknown op or variant and a NaN
 * threshold under ops 1 .. 3 are LSR_E_ARG, a half-width above the cap LSR_E_UNSUPPORTED, a NULL pointer LSR_E_NULL, a
 * non-positive extent LSR_E_SHAPE; nothing is launched or written then.  One launch, no scratch, no atomics, nothing between
 * workgroups: a workgroup stages the codes of its tile and a halo of r per side in LDS, the border resolved at load time;
 * `in` is never written and every voxel of `out` exactly once.
 * lsr_rank_filter_tiling: {the greatest half-width per axis, the tile's z, y and x extent}.
 */
int lsr_rank_filter_tiling(int tiling[4]);
int lsr_rank_filter_f32(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int rank, int op,
                        float threshold, int variant, lsr_stream_t stream);

/*
 * Ridge, sheet and blob filters on the eigenvalues of the Hessian (csrc/hessian.hip, shrimpy_amd/hessian.py).  The rule is
 * stated in csrc/hessian.hpp; PINNED to numpy -- np.gradient twice and np.linalg.eigvalsh, what
 * skimage.feature.hessian_matrix(use_gaussian_derivatives=False) and hessian_matrix_eigvals compute (tests/hessian_ref.py):
 *   g, out are contiguous (Z, Y, X) float32 volumes, g already smoothed; (sz, sy, sx) the sampling; `scale` multiplies the
 *   eigenvalues (the Python layer passes sigma^2).  D_a f along an axis of length n is np.gradient's: the central difference
 *   over 2 s_a inside, the one-sided difference over s_a at i = 0 and i = n - 1, 0 for n = 1 (numpy raises there).  H_ab =
 *   D_b (D_a g) for a <= b in float64 from the float32 g (the divisions are multiplications by the float64 reciprocals); at
 *   the faces the one-sided forms compose as numpy composes them, chosen from the voxel's index, and no position outside the
 *   volume is read.  l1 <= l2 <= l3 are the eigenvalues of H, with dark = 1 of -H (float64, cyclic Jacobi, within 2^-31.5
 *   ||H||_F); e_k = float32(scale * l_k).  With m_k = (-e_k > 0) ? -e_k : 0, every measure is a bit-exact float32 function of
 *   (e1, e2, e3): 0, 1, 2 e1, e2, e3; 3 ridge m1; 4 tube sqrtf(m1 * m2); 5 sheet m1 - m2; 6 blob m3; 7 log -((e1 + e2) + e3).
 *   A voxel whose stencil -- the voxels its six entries read: itself, two steps along each axis, the in-plane diagonals, as
 *   the faces allow -- holds a non-finite value gives the canonical quiet NaN 0x7fc00000 under every measure.
 *   accumulate: 0 stores the response r; 1 stores max(out, r) -- NaN if either is a NaN, else (out >= r) ? out : r -- so that
 *   calls at several sigmas leave the running maximum.
 * out must not alias g (LSR_E_ARG); a sampling that is not positive and finite, a non-finite scale and an unknown measure,
 * dark or accumulate are LSR_E_ARG, a NULL pointer LSR_E_NULL, a non-positive extent LSR_E_SHAPE, more than 2^31 - 1 voxels
 * LSR_E_UNSUPPORTED; nothing is launched or written then.  One launch, no scratch, no atomics, nothing between workgroups: a
 * workgroup stages its tile of g and a halo of 2 per side in LDS; g is never written and every voxel of `out` exactly once.
 * lsr_hessian_tiling: {the halo, the tile's z, y and x extent}.
 */
int lsr_hessian_tiling(int tiling[4]);
int lsr_hessian_response_f32(const float* g, float* out, int64_t Z, int64_t Y, int64_t X, double sz, double sy, double sx,
                             double scale, int measure, int dark, int accumulate, lsr_stream_t stream);

/*
 * Splitting touching objects: a watershed by steepest ascent (csrc/watershed.hip, shrimpy_amd/watershed.py).  PARITY
 * UNPINNED: no upstream is pinned, the rule IS the specification (csrc/watershed.hpp; tests/watershed_ref.py restates it).
 *   objects (int32, Z * Y * X): values <= 0 are background.  surface (float32): its values compare by the order-preserving
 *   integer image of a float (-0.0 below +0.0, +inf an ordinary value; NaN is unsupported but cannot hang or fault anything).
 *   connectivity is 6, 18 or 26, as in lsr_label_f32.  N(v) is the set of neighbours of v inside the volume with
 *   objects[u] == objects[v]; up(v) is the element of N(v) + {v} with the greatest (surface, then the SMALLER linear index);
 *   basins are the connected components of the edges {v, up(v)}, so no basin spans two objects.  basins (int32) receives 0
 *   on the background and 1 .. B in raster order of each basin's smallest linear index; *n_basins (int32, device memory)
 *   receives B, the number of summits up(v) == v.  basins must not alias objects or surface (LSR_E_ARG).  A volume holds at
 *   most 2^31 - 1 voxels (LSR_E_UNSUPPORTED beyond); a NULL pointer is LSR_E_NULL, a non-positive extent LSR_E_SHAPE.
 * lsr_watershed_tile_shape: the (z, y, x) tile one workgroup stages in LDS with a one-voxel halo.
 * lsr_watershed_launch_geometry: lsr_label_launch_geometry's five numbers as this translation unit compiled them (it holds its
 * own copy of the numbering launches); the second cap is that of this local launch's grid.
 * lsr_watershed_scratch_bytes: the size of `scratch` (device memory; its contents on entry do not matter) -- the block counts
 * of the numbering and one direction byte per voxel -- or a negative status for a shape out of range.
 * lsr_watershed_f32 runs seven launches on `stream` -- local (up(v) of every voxel of a tile, unions inside the tile), merge
 * (unions where up(v) lies in another tile, atomicMin on the parent words), then lsr_label_f32's flatten, count, scan, rank,
 * final -- with the union-find kept in `basins` itself; no workgroup ever waits for another and the result does not depend
 * on the order of execution.
 *
 * lsr_watershed_saddles_f32: for every pair of neighbours v, u (under connectivity) of one object in different basins
 * a < b, pass = min(surface[v], surface[u]); saddle(a, b) = the maximum of the passes.  `table` (device memory, WHICH THE
 * CALLER HAS ZEROED) is an open-addressing hash table of `capacity` 16-byte slots, capacity a power of two in 1 .. 2^30
 * (LSR_E_ARG otherwise): uint64 pair = a << 32 | b (0: the slot is empty); uint32 key = the integer image of saddle(a, b)
 * (a float v with bits u maps to ~u where u's sign bit is set, to u | 0x80000000 otherwise); uint32 unused.  Probing is
 * linear over at most min(capacity, 256) slots.  counts (int32[2], device memory, set by the entry): counts[0] = the slots
 * claimed, counts[1] = the neighbour pairs that found no slot -- if it is not zero the table is incomplete: come back with a
 * larger one.  Which slot a record lands in depends on the order of arrival: the contract is the set of records.  One
 * launch (and the clearing of counts); the table's words are touched by atomics only, nothing waits for anything.
 */
int lsr_watershed_tile_shape(int zyx[3]);
int lsr_watershed_launch_geometry(int64_t out[5]);
int64_t lsr_watershed_scratch_bytes(int64_t Z, int64_t Y, int64_t X);
int lsr_watershed_f32(const int32_t* objects, const float* surface, int64_t Z, int64_t Y, int64_t X, int connectivity,
                      int32_t* basins, int32_t* n_basins, void* scratch, lsr_stream_t stream);
int lsr_watershed_saddles_f32(const int32_t* objects, const int32_t* basins, const float* surface, int64_t Z, int64_t Y, int64_t X,
                              int connectivity, int64_t capacity, void* table, int32_t* counts, lsr_stream_t stream);
/* measurement only (tools/bench_kernels.py --watershed): lsr_watershed_f32 with a HIP event between its launches; waits for
 * the stream and writes the times of local, merge, flatten, count, scan, rank and final in milliseconds to ms7 (HOST memory) */
int lsr_watershed_profile_f32(const int32_t* objects, const float* surface, int64_t Z, int64_t Y, int64_t X, int connectivity,
                              int32_t* basins, int32_t* n_basins, void* scratch, float* ms7, lsr_stream_t stream);

/*
 * The contingency table of two label volumes (csrc/overlap.hip; the rule is stated in csrc/overlap.hpp): what
 * shrimpy_amd/track.py links the objects of consecutive timepoints by.  No upstream is pinned; tests/track_ref.py restates
 * the rule with np.unique, and device, twin and restatement agree as sets of records, exactly.
 *
 * lsr_label_overlap_i32: a, b are int32 (Z, Y, X) volumes (device memory), shift_zyx three integers in HOST memory.  For
 * every voxel v = (z, y, x) with u = v + shift inside the volume, a[v] > 0 and b[u] > 0, the pair (a[v], b[u]) gains 1;
 * labels <= 0 are background.  `table` (device memory, WHICH THE CALLER HAS ZEROED) is an open-addressing hash table of
 * `capacity` 16-byte records, capacity a power of two in 1 .. 2^30: uint64 pair = (uint32)a << 32 | (uint32)b (0: the slot
 * is empty); uint64 count.  A pair starts probing where the saddle table's does (csrc/pair_table.hpp) and probes linearly
 * over at most min(capacity, 256) slots.  counts (int32[2], device memory, set by the entry): counts[0] = the slots claimed,
 * counts[1] = the contributions (voxels) that found no slot -- if it is not zero the table holds partial counts: come back
 * with a larger one.  Which slot a record lands in depends on the order of arrival: the contract is the set of records.
 * max_blocks caps the grid (0: the default of lsr_label_overlap_geometry); the result does not depend on it.
 * Everything wrong with a call is LSR_E_ARG, before any launch and with nothing written: a NULL pointer, a non-positive
 * extent or more than 2^31 - 1 voxels, a capacity that is no power of two in range, max_blocks < 0, a table that overlaps
 * a or b.  A shift at or beyond an extent leaves the table empty and counts zero.
 * One launch (and the clearing of counts): each workgroup walks one contiguous span of the volume, reduces runs of equal
 * pairs inside a wave by one ballot, accumulates in a table in LDS and flushes it once, so an all-foreground volume costs
 * one global atomic pair per workgroup; shared words are touched by atomics only, nothing waits for anything.
 * lsr_label_overlap_geometry: out[0] = the slots of one workgroup's LDS table, out[1] = the default cap of the grid.
 */
int lsr_label_overlap_geometry(int out[2]);
int lsr_label_overlap_i32(const int32_t* a, const int32_t* b, int64_t Z, int64_t Y, int64_t X, const int32_t shift_zyx[3],
                          int64_t capacity, void* table, int32_t* counts, int max_blocks, lsr_stream_t stream);

/*
 * The volume, first and second moments of every object of a label volume (csrc/moments.hip; the rule is stated in
 * csrc/moments.hpp): what shrimpy_amd/segment.py derives axis lengths and orientations from.  No upstream is pinned;
 * tests/moments_ref.py restates the rule with np.add.at on int64, and device, twin and restatement are equal byte for byte.
 *
 * lsr_label_moments_i32: labels is an int32 (Z, Y, X) volume (device memory).  For every voxel (z, y, x) with
 * 1 <= labels[v] <= n_objects, record labels[v] - 1 of `table` gains 1 (volume), z, y, x (s_z, s_y, s_x) and z^2, y^2, x^2,
 * zy, zx, yx (m_zz, m_yy, m_xx, m_zy, m_zx, m_yx), in absolute voxel indices.  `table` (device memory, WHICH THE CALLER HAS
 * ZEROED) is n_objects records of ten int64 in that order, 80 bytes each.  Labels outside 1 .. n_objects are ignored; a label
 * that no voxel carries keeps a zero record.  Pure integer arithmetic: the records do not depend on the order of execution.
 * max_blocks caps the grid (0: the default of lsr_label_moments_geometry); the result does not depend on it.
 * Refused before any launch and with nothing read or written: LSR_E_ARG for a NULL pointer, a non-positive extent,
 * n_objects < 0, max_blocks < 0 or a table that overlaps labels; LSR_E_UNSUPPORTED for more than 2^31 - 1 voxels or for
 * Z*Y*X * max(Z, Y, X)^2 >= 2^63, where a sum could wrap.  n_objects == 0 returns at once.
 * One launch: each workgroup walks one contiguous span of the volume, finds the runs of equal labels inside a row by one
 * ballot, takes a run's ten sums in closed form from (z, y, x0, length), accumulates in a table in LDS and flushes it once, so
 * an all-foreground volume costs ten global atomics per workgroup; shared words are touched by atomics only, nothing waits
 * for anything.
 * lsr_label_moments_geometry: out[0] = the slots of one workgroup's LDS table, out[1] = the default cap of the grid.
 */
int lsr_label_moments_geometry(int out[2]);
int lsr_label_moments_i32(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, void* table,
                          int max_blocks, lsr_stream_t stream);
/* measurement only (tools/bench_kernels.py --moments): the same kernel with lds_slots slots in the LDS table (a power of two
 * up to 512) probed over at most lds_probes (1 .. 512) slots, or with lds_slots == 0 the plain form in which every run head
 * adds to the global record directly */
int lsr_label_moments_variant_i32(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, void* table,
                                  int max_blocks, int lds_slots, int lds_probes, lsr_stream_t stream);

/*
 * The intensities every object of a label volume holds in another volume (csrc/intensity.hip; the rule is stated in
 * csrc/intensity.hpp): what shrimpy_amd/segment.py: intensity_table and the `measure` command read.  No upstream is pinned;
 * tests/intensity_ref.py restates the rule in numpy.
 *
 * lsr_label_intensity_f32 / _u16: labels is an int32 (Z, Y, X) volume, v a float32 / uint16 volume of the same shape (device
 * memory).  For every voxel (z, y, x) with 1 <= labels[i] <= n_objects, record labels[i] - 1 of `table` gains 1 (count), v,
 * v^2, v z, v y, v x (sum_v, sum_vv, sum_vz, sum_vy, sum_vx; absolute voxel indices) and v (v_min, v_max).  `table` (device
 * memory, WHICH THE CALLER HAS ZEROED) is n_objects records of 64 bytes: count (int64), the five sums (float64 for float32
 * values, uint64 for uint16 values), v_min and v_max (float32, or uint32 holding the value), 8 bytes of padding that stay zero.
 * Labels outside 1 .. n_objects are ignored; a label that no voxel carries keeps a zero record.
 * float32: count, v_min and v_max are exact; the extremes are ordered as lsr_label_regions_f32 orders them (-0.0 below +0.0; a
 * NaN outside the infinities on the side of its sign bit).  Every float64 sum is within 2 n_k 2^-53 sum|terms| of the exact sum
 * of its exact terms (n_k: the object's voxels), in atomic adds whose order is not fixed; a non-finite voxel follows IEEE
 * arithmetic into its own object's sums only.  uint16: pure integer arithmetic, independent of the order of execution.
 * max_blocks caps the grid (0: the default of lsr_label_intensity_geometry); only the order of the float64 adds depends on it.
 * Refused before any launch and with nothing read or written: LSR_E_ARG for a NULL pointer, a non-positive extent,
 * n_objects < 0, max_blocks < 0 or a table that overlaps labels or v; LSR_E_UNSUPPORTED for more than 2^31 - 1 voxels and, for
 * uint16 values, for 65535 * Z*Y*X * max(Z, Y, X) >= 2^64, where a sum could wrap.  n_objects == 0 returns at once.
 * Two launches: each workgroup walks one contiguous span of both volumes, finds the runs of equal labels inside a row by one
 * ballot, reduces a run's sums and extremes by shuffles restricted to the run, accumulates in a table in LDS (64-bit LDS
 * atomic adds, the hardware's float64 add among them) and flushes it once; a finishing launch over the records decodes the
 * extremes.  Shared words are touched by atomics only, nothing waits for anything.
 * lsr_label_intensity_geometry: out[0] = the slots of one workgroup's LDS table, out[1] = the default cap of the grid.
 */
int lsr_label_intensity_geometry(int out[2]);
int lsr_label_intensity_f32(const int32_t* labels, const float* v, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, void* table,
                            int max_blocks, lsr_stream_t stream);
int lsr_label_intensity_u16(const int32_t* labels, const uint16_t* v, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                            void* table, int max_blocks, lsr_stream_t stream);
/* measurement only (tools/bench_kernels.py --intensity): the same kernel (v is uint16 where value_is_u16 != 0, float32
 * otherwise) with lds_slots slots in the LDS table (a power of two up to 512) probed over at most lds_probes (1 .. 512) slots,
 * or with lds_slots == 0 the plain form in which every run head goes to the global record directly */
int lsr_label_intensity_variant(const int32_t* labels, const void* v, int value_is_u16, int64_t Z, int64_t Y, int64_t X,
                                int64_t n_objects, void* table, int max_blocks, int lds_slots, int lds_probes,
                                lsr_stream_t stream);

/*
 * Per-object sums over two channels at once (csrc/coloc.hip; the rule is stated in csrc/coloc.hpp): what
 * shrimpy_amd/colocalize.py: pair_table, coefficients, costes_thresholds and the `colocalize` command read.  No upstream is
 * pinned; tests/coloc_ref.py restates the rule in numpy.
 *
 * lsr_label_coloc_f32 / _u16: labels is an int32 (Z, Y, X) volume or NULL, a and b two float32 / uint16 volumes of that shape
 * (device memory), ta and tb two thresholds.  With labels == NULL, n_objects must be 1 and every voxel belongs to object 1.
 * Let A = (float(a) > ta), B = (float(b) > tb) (a NaN value compares false).  For every voxel with 1 <= label <= n_objects,
 * record label - 1 of `table` gains: word 0 count 1; words 1..5 sum_a, sum_b, sum_aa, sum_bb, sum_ab the terms a, b, a^2, b^2,
 * a b; word 6 count_both 1 where A and B; words 7..11 both_a .. both_ab the same five terms where A and B; words 12, 13 count_A,
 * count_B; words 14, 15 a_where_B, b_where_A.  `table` (device memory, WHICH THE CALLER HAS ZEROED) is n_objects records of 16
 * words of 8 bytes: counts int64, sums float64 for float32 values and uint64 for uint16 values.  Labels outside 1 .. n_objects
 * are ignored; a label that no voxel carries keeps a zero record.
 * uint16: pure integer arithmetic, independent of the order of execution (65535^2 * 2^31 < 2^63: no sum can wrap).  float32:
 * the counts are exact; every sum is within m 2^-53 sum|terms| of the exact sum of its exact terms (m: the number of terms of
 * that sum), in atomic adds whose order is not fixed; a non-finite voxel follows IEEE arithmetic into its own object's sums only.
 * max_blocks caps the grid (0: the default of lsr_label_coloc_geometry); only the order of the float64 adds depends on it.
 * Refused before any launch and with nothing read or written: LSR_E_ARG for a NULL a, b or table, a non-positive extent,
 * n_objects < 0, labels == NULL with n_objects != 1, a NaN threshold, max_blocks < 0 or a table that overlaps an input;
 * LSR_E_UNSUPPORTED for more than 2^31 - 1 voxels.  n_objects == 0 returns at once.
 * One launch: each workgroup walks one contiguous span of the three volumes; while whole wave steps hold one label every lane
 * keeps the sixteen quantities in registers and the wave reduces them once; wave steps with more than one run find the runs by
 * one ballot and reduce them by shuffles restricted to the run; a table in LDS (64-bit LDS atomic adds) is flushed once.  Without
 * labels there is no label stream and no table.  Shared words are touched by atomics only, nothing waits for anything.
 * lsr_label_coloc_geometry: out[0] = the slots of one workgroup's LDS table, out[1] = the default cap of the grid.
 */
int lsr_label_coloc_geometry(int out[2]);
int lsr_label_coloc_f32(const int32_t* labels, const float* a, const float* b, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                        float ta, float tb, void* table, int max_blocks, lsr_stream_t stream);
int lsr_label_coloc_u16(const int32_t* labels, const uint16_t* a, const uint16_t* b, int64_t Z, int64_t Y, int64_t X,
                        int64_t n_objects, float ta, float tb, void* table, int max_blocks, lsr_stream_t stream);
/* measurement only (tools/bench_kernels.py --coloc): the same kernel (a and b are uint16 where value_is_u16 != 0, float32
 * otherwise) with lds_slots slots in the LDS table (a power of two up to 256) probed over at most lds_probes (1 .. 256) slots,
 * or with lds_slots == 0 the plain form in which every part goes to the global record directly */
int lsr_label_coloc_variant(const int32_t* labels, const void* a, const void* b, int value_is_u16, int64_t Z, int64_t Y, int64_t X,
                            int64_t n_objects, float ta, float tb, void* table, int max_blocks, int lds_slots, int lds_probes,
                            lsr_stream_t stream);

/*
 * Whole-volume statistics (csrc/stats.hip; the rule is stated in csrc/stats.hpp): what shrimpy_amd/stats.py: order_statistics,
 * quantiles, summary and rescale read.  tests/stats_ref.py restates the rule in numpy.
 *
 * Keys: a float32 value is ordered by its order-preserving 32-bit key (the sign bit flipped for a value with the sign bit
 * clear, every bit flipped otherwise: -0.0 below +0.0, the infinities ordinary values); a uint16 value is its own 16-bit key.
 * A NaN is counted in the moment record and takes part in nothing else.  A key is `passes` digits of out[0] bits of
 * lsr_volume_stats_geometry, the most significant first.
 *
 * lsr_digit_histogram_f32 / _u16: one pass of a radix select over the n voxels of `in` (device memory, aligned to 16 / 8
 * bytes) for k ranks (1 .. K).  prefixes[r] (HOST memory) is the integer made of the `pass` digits rank r has fixed so far
 * (0 in pass 0), table_of_rank[r] (HOST memory, 0 .. k - 1) the table it reads; ranks share a table exactly where they share
 * a prefix.  For every non-NaN voxel whose key carries the prefix of table t, word t * bins + (digit `pass` of the key) of
 * `tables` (device memory, k * bins counters of 64 bits) gains 1.  THE ENTRY DOES NOT ZERO `tables`: calls on several volumes
 * pool into one multiset.  In pass 0 `moments` may be a record of 5 words of 8 bytes (device memory, not zeroed by the entry
 * either), which gains: word 0 the number of non-NaN voxels, word 1 the number of NaNs, words 2 and 3 the sums of v and v^2
 * (float64 for float32 values, uint64 for uint16 values); word 4 holds ~key(min) in its low and key(max) in its high 32 bits,
 * each raised to the maximum of what it held and the volume's (zero is neutral; with word 0 == 0 there are no extremes).
 * Otherwise `moments` is NULL.  Tables, counts and extremes are exact and independent of the order of execution; a float64
 * sum is within n 2^-53 sum|terms| of the exact sum of its exact terms, in atomic adds whose order is not fixed, and follows
 * IEEE addition where infinities are present; uint16 sums are integers.
 * grid_cap caps the grid (0: the default).  form: low byte 0 = lanes of a wave whose table and bin equal the lane before them
 * are counted by the head of their run in one LDS add, 1 = one LDS add per voxel (the same tables; kept for the bench); the
 * bits above the low byte, where not 0, are the number of strides after which a workgroup flushes its LDS tables (the default
 * is 2^31 voxels' worth: a 32-bit LDS counter cannot wrap), which the tests use to reach that flush.
 * Refused before any launch and with nothing read or written: LSR_E_ARG for n <= 0, k outside 1 .. K, a pass the key does not
 * have, a NULL or misaligned pointer, a prefix the pass cannot have, a table index outside 0 .. k - 1, ranks that share a
 * table without sharing a prefix or the reverse, moments outside pass 0, grid_cap < 0, an unknown form, or buffers that
 * overlap; LSR_E_UNSUPPORTED for n >= 2^48 and, for uint16 values with a record, for 65535^2 n >= 2^64.
 * One launch: each workgroup walks one contiguous span in strides, every load of a stride issued before the first is used,
 * counts in up to K tables of 32-bit counters in LDS and flushes them by 64-bit global adds.  Shared words are touched by
 * atomics only, nothing waits for anything.
 *
 * lsr_rescale_f32 / _u16: out[i] = (float(in[i]) - sub) / div, then with clip != 0 max(., lo) and min(., hi); a NaN stays a
 * NaN.  One float32 rounding per step: bit for bit numpy's np.clip((v.astype(f32) - f32(sub)) / f32(div), lo, hi).  in and
 * out device memory aligned to 16 bytes; a float32 volume may be rescaled in place (out == in), any other overlap is refused.
 * LSR_E_ARG for n <= 0, a NULL or misaligned pointer, clip outside {0, 1}, or with a clip lo > hi or a NaN bound;
 * LSR_E_UNSUPPORTED for n >= 2^48.
 *
 * lsr_volume_stats_geometry: out[0] = the digit's bits, out[1] = bins, out[2] = K, out[3] = threads of a workgroup, out[4] =
 * voxels one wave takes per stride (a workgroup takes out[3] / 64 times as many), out[5] = the default grid cap, out[6] = the
 * LDS bytes of a workgroup, out[7] = the passes of a float32 volume; a uint16 volume takes ceil(16 / out[0]).
 */
int lsr_volume_stats_geometry(int64_t out[8]);
int lsr_digit_histogram_f32(const float* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank, int k,
                            void* tables, void* moments, int grid_cap, int form, lsr_stream_t stream);
int lsr_digit_histogram_u16(const uint16_t* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank, int k,
                            void* tables, void* moments, int grid_cap, int form, lsr_stream_t stream);
int lsr_rescale_f32(const float* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out, lsr_stream_t stream);
int lsr_rescale_u16(const uint16_t* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                    lsr_stream_t stream);

/*
 * Host twins (csrc/host_twins.hip): the same signatures with HOST pointers, the same argument checks and the
 * same arithmetic in the same order, so the results equal the device entry points' bit for bit.  They serve
 * the boxes where the reference itself resolves to the CPU (shrimpy/preprocessing.py:78-82 -- its CI has no
 * GPU, shrimpy/tests/conftest.py:11-17) and BASELINE config 1; they are product code and never touch oracle/.
 * `stream` is ignored.  Work is split over at most lsr_set_host_threads(n) plain threads (default 1, no OpenMP).
 * lsr_affine_f32_cpu takes LSR_MODE_CONSTANT / LSR_MODE_GRID_CONSTANT only (its arithmetic is always fp64).
 */
int lsr_set_host_threads(int n);
int lsr_get_host_threads(void);
int lsr_deskew_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                       int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                       const double M[12], int avg_n, lsr_stream_t stream);
int lsr_deskew_u16_cpu(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, float* out, int64_t Zo,
                       int64_t Yo, int64_t Xo, int64_t out_pitch, int64_t out_plane, int64_t Zd,
                       const double M[12], int avg_n, lsr_stream_t stream);
int lsr_affine_f32_cpu(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* out, int64_t Zo,
                       int64_t Yo, int64_t Xo, const double M[12], float cval, int mode,
                       lsr_stream_t stream);
int lsr_average_slices_f32_cpu(const float* in, int64_t Zd, int64_t Y, int64_t X, float* out,
                               int64_t Zo, int avg_n, lsr_stream_t stream);
int lsr_correlate_sep_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                              int64_t X, const float* wz, int pz, const float* wy, int py,
                              const float* wx, int px, int epilogue, float eps, const float* nz,
                              const float* ny, const float* nx, lsr_stream_t stream);
int lsr_correlate_dense_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                                int64_t X, const float* w, int pz, int py, int px, int epilogue,
                                float eps, const double* norm_table, lsr_stream_t stream);
int lsr_rl_dense_f32_cpu(const float* y, float* x, float* ratio, int64_t Z, int64_t Y, int64_t X,
                         const float* psf, const float* psf_flipped, int pz, int py, int px,
                         const double* norm_table, int iters, float eps, lsr_stream_t stream);
/* ... with the reduction scalars (see lsr_rl_*_stats_f32; `stats` is HOST memory, sums in f64 per row range) */
int lsr_correlate_sep_stats_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                                    int64_t X, const float* wz, int pz, const float* wy, int py,
                                    const float* wx, int px, int epilogue, float eps, const float* nz,
                                    const float* ny, const float* nx, double* stats, lsr_stream_t stream);
int lsr_correlate_dense_stats_f32_cpu(const float* in, float* out, const float* aux, int64_t Z, int64_t Y,
                                      int64_t X, const float* w, int pz, int py, int px, int epilogue,
                                      float eps, const double* norm_table, double* stats, lsr_stream_t stream);
int lsr_rl_dense_stats_f32_cpu(const float* y, float* x, float* ratio, int64_t Z, int64_t Y, int64_t X,
                               const float* psf, const float* psf_flipped, int pz, int py, int px,
                               const double* norm_table, int iters, float eps, double* stats,
                               lsr_stream_t stream);
/* ... of the RL-TV factor (csrc/rl_tv.hip: the same inline arithmetic, the kernel's bits; no stream; stats2 HOST memory) */
int lsr_rl_tv_scale_f32_cpu(const float* u, int64_t u_pitch, int64_t u_plane, const float* v, int64_t v_pitch,
                            int64_t v_plane, float* out, int64_t o_pitch, int64_t o_plane, int64_t Z, int64_t Y,
                            int64_t X, float lambda, float tv_eps, double* stats2);
/* ... of the accelerated RL launches (csrc/host_twins.hip: the same inline arithmetic, g and p are the kernels' bits; the
 * inner products are summed over fixed row chunks in a fixed order, the same bits at every lsr_set_host_threads value; no
 * stream; dots2, num, den and alpha_out HOST memory) */
int lsr_rl_accel_dots_f32_cpu(const float* x1, int64_t x1_pitch, int64_t x1_plane, const float* p, int64_t p_pitch,
                              int64_t p_plane, float* g, int64_t Z, int64_t Y, int64_t X, int first, double* dots2,
                              void* workspace /* unused */);
int lsr_rl_accel_predict_f32_cpu(const float* x1, int64_t x1_pitch, int64_t x1_plane, float* x0, int64_t x0_pitch,
                                 int64_t x0_plane, int64_t Z, int64_t Y, int64_t X, const double* num, const double* den,
                                 double* alpha_out);
int lsr_flatfield_pattern_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float* pattern,
                                  float* mean_out, void* scratch /* unused */, lsr_stream_t stream);
int lsr_flatfield_pattern_u16_cpu(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, float* pattern,
                                  float* mean_out, void* scratch /* unused */, lsr_stream_t stream);
int lsr_flatfield_apply_f32_cpu(const float* in, const float* pattern, const float* mean_dev,
                                float* out, int64_t Z, int64_t Y, int64_t X, lsr_stream_t stream);
int lsr_flatfield_apply_u16_cpu(const uint16_t* in, const float* pattern, const float* mean_dev,
                                float* out, int64_t Z, int64_t Y, int64_t X, lsr_stream_t stream);
/*
 * ... and of the DynaTrack estimators (csrc/estimators_host.hip), for a tracker that runs where the reference's own
 * does without a GPU (shrimpy/dynatrack/tracking.py:1054).  Identical values for min / max, the histogram, the shape
 * map, the cross power, the peak and the blur (the kernels' FMA chain); the centroid sums are fp64 like the kernels'
 * but added in row order (equal to the last bits of a double).  `scratch` is unused.  The FFTs between the
 * cross-correlation's steps stay library calls (torch.fft on the CPU).
 */
int lsr_minmax_f32_cpu(const float* in, int64_t n, float* out2, void* scratch, lsr_stream_t stream);
int lsr_histogram_f32_cpu(const float* in, int64_t n, float vmin, float vmax, int nbins, unsigned* counts,
                          lsr_stream_t stream);
int lsr_weighted_centroid_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float background,
                                  double* out4, void* scratch, lsr_stream_t stream);
int lsr_mask_centroid_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold,
                              double* out4, void* scratch, lsr_stream_t stream);
int lsr_blur_reflect_f32_cpu(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int axis,
                             const float* taps, int radius, float sub, float div, lsr_stream_t stream);
int lsr_match_shape_f32_cpu(const float* in, int64_t Zi, int64_t Yi, int64_t Xi, float* out, int64_t Zo,
                            int64_t Yo, int64_t Xo, lsr_stream_t stream);
int lsr_cross_power_c64_cpu(float* a, const float* b, int64_t n, lsr_stream_t stream);
int lsr_cross_power_into_c64_cpu(const float* a, float* b, int64_t n, lsr_stream_t stream);
int lsr_peak_abs_shifted_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, long long* out_index,
                                 void* scratch, lsr_stream_t stream);

/* ... of the bead detection and the PSF average (csrc/peaks.hip): the same peaks (callers sort them) and the same bits of
 * bead_stats and psf; every pointer HOST memory, `scratch` unused (the twins allocate their two volumes themselves) */
int lsr_box_smooth_f32_cpu(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int taps, float tap, void* scratch,
                           lsr_stream_t stream);
int lsr_local_max_candidates_f32_cpu(const float* s, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx,
                                     float threshold, long long* cand_index, float* cand_value, int64_t capacity,
                                     unsigned long long* count, void* scratch, lsr_stream_t stream);
int lsr_psf_accumulate_f32_cpu(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                               int64_t n_beads, int pz, int py, int px, double* bead_stats, float* psf,
                               lsr_stream_t stream);

/* ... of the Gaussian fit and the shifted average (csrc/psf_fit.hip): the fit through the same steps (csrc/psf_fit.hpp)
 * with the sums in C order -- the kernel's statuses, its parameters to rounding; the shifted average to the bit for the
 * same weights.  Every pointer HOST memory, `scratch` unused. */
int lsr_bead_fit_f32_cpu(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres, int64_t n_beads,
                         int pz, int py, int px, int max_iter, double* fit, int* status, lsr_stream_t stream);
int lsr_psf_accumulate_shifted_f32_cpu(const float* vol, int64_t Z, int64_t Y, int64_t X, const long long* centres,
                                       int64_t n_beads, int pz, int py, int px, double* bead_stats, const double* weights,
                                       void* scratch, float* psf, lsr_stream_t stream);

/* ... of the pyramid level (csrc/pyramid.hip): the same window arithmetic from the same header, the same bits */
int lsr_downsample2_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float* out, int fz, lsr_stream_t stream);
int lsr_downsample2_u16_cpu(const uint16_t* in, int64_t Z, int64_t Y, int64_t X, uint16_t* out, int fz, lsr_stream_t stream);

/* ... of the stitching composite (csrc/stitch.hip): table and tiles in HOST memory (the table's entries are checked here) */
int lsr_stitch_f32_cpu(const void* table, int n_tiles, float* out, const int64_t box_origin[3], const int64_t box_shape[3],
                       int p, float cval, lsr_stream_t stream);

/* ... of the labelling (csrc/label.hip): plain sequential code, scipy.ndimage.label's labels, the kernels' integer fields and
 * intensity range; the float64 sums in raster order.  Every pointer HOST memory, `scratch` unused (but required). */
int lsr_label_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int connectivity, int32_t* labels,
                      int32_t* n_objects, void* scratch, lsr_stream_t stream);
int lsr_label_regions_f32_cpu(const int32_t* labels, const float* intensity, int64_t Z, int64_t Y, int64_t X,
                              int64_t n_objects, void* table, lsr_stream_t stream);
int lsr_label_remap_i32_cpu(int32_t* labels, int64_t n, const int32_t* map, int64_t n_map, lsr_stream_t stream);

/* ... of the distance transform and the label expansion (csrc/edt.hip): plain sequential code over the same row rule and the
 * same line pass (csrc/edt.hpp), so `nearest` and `dist` are the kernels' bits.  Every pointer HOST memory, `scratch` unused
 * (but required). */
int lsr_edt_f32_cpu(const float* in, int64_t Z, int64_t Y, int64_t X, float threshold, int invert, const double sampling[3],
                    float* dist, int32_t* nearest, void* scratch, lsr_stream_t stream);
int lsr_edt_labels_i32_cpu(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int invert, const double sampling[3],
                           float* dist, int32_t* nearest, void* scratch, lsr_stream_t stream);
int lsr_label_expand_i32_cpu(const int32_t* labels, const int32_t* nearest, int64_t Z, int64_t Y, int64_t X,
                             const double sampling[3], double distance, int32_t* out, lsr_stream_t stream);

/* ... of the watershed (csrc/watershed.hip): plain sequential code over the same `up` rule, slot record and hash
 * (csrc/watershed.hpp): the kernels' basins element for element, the kernels' set of saddle records.  Every pointer HOST
 * memory, `scratch` unused (but required). */
int lsr_watershed_f32_cpu(const int32_t* objects, const float* surface, int64_t Z, int64_t Y, int64_t X, int connectivity,
                          int32_t* basins, int32_t* n_basins, void* scratch, lsr_stream_t stream);
int lsr_watershed_saddles_f32_cpu(const int32_t* objects, const int32_t* basins, const float* surface, int64_t Z, int64_t Y,
                                  int64_t X, int connectivity, int64_t capacity, void* table, int32_t* counts,
                                  lsr_stream_t stream);

/* ... of the label-overlap table (csrc/overlap.hip): plain sequential code over the same rule, record, hash and probe bound
 * (csrc/overlap.hpp): the kernel's set of records.  Every pointer HOST memory; max_blocks is checked and otherwise unused. */
int lsr_label_overlap_i32_cpu(const int32_t* a, const int32_t* b, int64_t Z, int64_t Y, int64_t X, const int32_t shift_zyx[3],
                              int64_t capacity, void* table, int32_t* counts, int max_blocks, lsr_stream_t stream);

/* ... of the label moments (csrc/moments.hip): plain sequential code over the same rule, record and checks
 * (csrc/moments.hpp), voxel by voxel: the kernel's records byte for byte.  Every pointer HOST memory; max_blocks is checked
 * and otherwise unused. */
int lsr_label_moments_i32_cpu(const int32_t* labels, int64_t Z, int64_t Y, int64_t X, int64_t n_objects, void* table,
                              int max_blocks, lsr_stream_t stream);

/* ... of the label intensities (csrc/intensity.hip): plain sequential code over the same rule, records and checks
 * (csrc/intensity.hpp), voxel by voxel.  uint16: the kernel's records byte for byte.  float32: the kernel's count and extremes;
 * the float64 sums add the same terms in raster order, inside the same bound.  Every pointer HOST memory; max_blocks is checked
 * and otherwise unused. */
int lsr_label_intensity_f32_cpu(const int32_t* labels, const float* v, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                                void* table, int max_blocks, lsr_stream_t stream);
int lsr_label_intensity_u16_cpu(const int32_t* labels, const uint16_t* v, int64_t Z, int64_t Y, int64_t X, int64_t n_objects,
                                void* table, int max_blocks, lsr_stream_t stream);

/* ... of the two-channel sums (csrc/coloc.hip): plain sequential code over the same rule, records and checks (csrc/coloc.hpp),
 * voxel by voxel.  uint16: the kernel's records byte for byte.  float32: the kernel's counts; the float64 sums add the same
 * terms in raster order, inside the same bound.  Every pointer HOST memory; max_blocks is checked and otherwise unused. */
int lsr_label_coloc_f32_cpu(const int32_t* labels, const float* a, const float* b, int64_t Z, int64_t Y, int64_t X,
                            int64_t n_objects, float ta, float tb, void* table, int max_blocks, lsr_stream_t stream);
int lsr_label_coloc_u16_cpu(const int32_t* labels, const uint16_t* a, const uint16_t* b, int64_t Z, int64_t Y, int64_t X,
                            int64_t n_objects, float ta, float tb, void* table, int max_blocks, lsr_stream_t stream);

/* ... of the grey morphology (csrc/morphology.hip): the same plan of passes and the same walk along a line
 * (csrc/morphology.hpp), so `out` is the kernels' bits.  Every pointer HOST memory; `scratch` holds the results between the
 * passes, as on the device. */
int lsr_grey_morph_f32_cpu(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int op,
                           void* scratch, lsr_stream_t stream);

/* ... of the rank filters (csrc/rank.hip): the same fold, codes, bisection and fused op (csrc/rank.hpp), so `out` is the
 * kernel's bits.  Every pointer HOST memory; `variant` is accepted and ignored. */
int lsr_rank_filter_f32_cpu(const float* in, float* out, int64_t Z, int64_t Y, int64_t X, int rz, int ry, int rx, int rank, int op,
                            float threshold, int variant, lsr_stream_t stream);

/* ... of the Hessian eigenvalue responses (csrc/hessian.hip): the same derivative, entries, Jacobi sweeps, responses and
 * store (csrc/hessian.hpp), so `out` is the kernel's bits.  Every pointer HOST memory. */
int lsr_hessian_response_f32_cpu(const float* g, float* out, int64_t Z, int64_t Y, int64_t X, double sz, double sy, double sx,
                                 double scale, int measure, int dark, int accumulate, lsr_stream_t stream);

/* ... of the whole-volume statistics (csrc/stats.hip): plain sequential code over the same rule, record and checks
 * (csrc/stats.hpp), voxel by voxel.  Tables, counts and the codes of the extremes are the kernel's words, and so are uint16
 * sums; float32 sums add the same terms in raster order, inside the same bound.  The rescale is the kernel's expression: the
 * kernel's bits.  Every pointer HOST memory; grid_cap and form are checked and otherwise unused. */
int lsr_digit_histogram_f32_cpu(const float* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank, int k,
                                void* tables, void* moments, int grid_cap, int form, lsr_stream_t stream);
int lsr_digit_histogram_u16_cpu(const uint16_t* in, int64_t n, int pass, const uint32_t* prefixes, const int32_t* table_of_rank,
                                int k, void* tables, void* moments, int grid_cap, int form, lsr_stream_t stream);
int lsr_rescale_f32_cpu(const float* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                        lsr_stream_t stream);
int lsr_rescale_u16_cpu(const uint16_t* in, int64_t n, float sub, float div, int clip, float lo, float hi, float* out,
                        lsr_stream_t stream);

/* ... of the mutual-information metric (csrc/estimate_mi.hip): the per-sample rule of csrc/mi_sample.hpp on both sides.
 * The histogram and the count are the kernel's bits; the gradient rows are sums over lsr_affine_mi_gradient_blocks()
 * equal runs of samples (fp64, another order than the kernel's: equal to the last bits of a double, and the same at
 * every lsr_set_host_threads value).  No stream; every pointer HOST memory. */
int lsr_affine_joint_histogram_f32_cpu(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target,
                                       int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], const int stride[3],
                                       int bins, double t_lo, double t_hi, double m_lo, double m_hi,
                                       unsigned long long* hist, unsigned long long* n_samples);
int lsr_affine_mi_gradient_f32_cpu(const float* moving, int64_t Zi, int64_t Yi, int64_t Xi, const float* target,
                                   int64_t Zo, int64_t Yo, int64_t Xo, const double M[12], const int stride[3],
                                   const double centre[3], double scale, int bins, double t_lo, double t_hi,
                                   double m_lo, double m_hi, const double* dL, double* partial);

#ifdef __cplusplus
}
#endif
#endif /* LSRECON_H */
