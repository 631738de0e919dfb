// Device primitives shared by the hand-pipelined stencil kernels (correlate_sep.hip, correlate_dense.hip,
// rl_fused_sep.hip, rl_fused_ysep.hip): the inline-asm memory operations, their waits, the raw barrier, the packed-pair
// helpers and the tile walk.  ONE definition each: these helpers decide which register a load in flight lands in, and a
// fix to one copy that misses another is the class of bug correlate_common.hpp (keep_until_here) records.  A change here
// is checked by comparing the compiler's listings of all 24 per-PZ translation units against the parent's
// (profiles/stencil_prims_isa.txt gives the commands): the instruction streams must not move.
//
// Everything has internal linkage (each translation unit is compiled with its own -D switches).
#pragma once

#include "common.hpp"

// Cache policy of the hand-written stores and of the LDS-DMA, appended to the instruction text.  A translation unit
// that probes other policies (rl_fused_sep.hip: LSR_FUSED_STORE_POLICY / LSR_FUSED_GLDS_POLICY) defines these before it
// includes this header; the defaults are the production strings.
#ifndef LSR_PRIMS_STORE_SUFFIX
#define LSR_PRIMS_STORE_SUFFIX " nt"
#endif
#ifndef LSR_PRIMS_GLDS_SUFFIX
#define LSR_PRIMS_GLDS_SUFFIX ""
#endif

namespace lsr {
namespace prims {
namespace {

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

constexpr int kBand = 8;   // tile rows per band of the tile walk (band_tile below)

#if defined(__HIPCC__)

typedef float f32x4 __attribute__((ext_vector_type(4)));  // native 16-byte vector (one VGPR quad)
// Two floats in an even-aligned register pair: the operand of the packed fp32 instructions
// (v_pk_fma_f32 / v_pk_mul_f32: two lanes' worth of work per issue slot).  Each component is an
// ordinary IEEE operation, so packing never changes a result.  The pairs are chosen by hand -- the
// two column groups of a thread, which ds_read2 delivers in adjacent registers -- because hipcc's
// own pairing (rows of one column) costs two v_mov per packed instruction.
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float fast_rcp(float d) {
  float r = __builtin_amdgcn_rcpf(d);    // v_rcp_f32, 1 ulp
  return fmaf(fmaf(-d, r, 1.0f), r, r);  // + one Newton step
}
__device__ __forceinline__ f32x2 splat(float a) { return f32x2{a, a}; }
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 fast_rcp2(f32x2 d) {  // fast_rcp on both components
  const f32x2 r = f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  return pk_fma(pk_fma(-d, r, splat(1.0f)), r, r);
}

// ---- hand-managed memory operations: scalar base + unsigned 32-bit byte offset per lane -------------
// The destination is an IN/OUT operand ("+v"): a register that is loaded again before its value was read -- the
// prologue's placeholder loads, the prefetches of the planes past the last one -- must stay the same physical register
// while the older load is in flight.  As a pure output ("=v") the older value is dead to the compiler and the register
// free between the two loads: round 4 found the <13, 9, 9> instance of correlate_sep.hip computing LDS offsets in such
// a register, and the in-flight load landing on top of them (results that differed from run to run).
__device__ __forceinline__ void gload_x4(f32x4& dst, const float* sbase, int voff_bytes) {
  asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(dst) : "v"(voff_bytes), "s"(sbase) : "memory");
}
__device__ __forceinline__ void gload_x1(float& dst, const float* sbase, int voff_bytes) {
  asm volatile("global_load_dword %0, %1, %2" : "+v"(dst) : "v"(voff_bytes), "s"(sbase) : "memory");
}
// ... with a compile-time byte offset in the instruction
template <int IMM>
__device__ __forceinline__ void gload(float& dst, const float* sbase, int voff) {
  asm volatile("global_load_dword %0, %1, %2 offset:%3" : "+v"(dst) : "v"(voff), "s"(sbase), "n"(IMM) : "memory");
}
// Stores are non-temporal: x_new is not read again before the next launch, and keeping it out of
// the way leaves more of L2 / MALL to the x planes that ARE read again nine planes later
// (measured 2.56 -> 2.50 ms per launch; `nt` on the y loads instead made it slower, 2.66 ms).
template <int IMM>
__device__ __forceinline__ void gstore(float* sbase, int voff, float v) {
  asm volatile("global_store_dword %0, %1, %2 offset:%3" LSR_PRIMS_STORE_SUFFIX
               :
               : "v"(voff), "v"(v), "s"(sbase), "n"(IMM)
               : "memory");
}
// LDS-DMA: 16 bytes per lane, LDS address = m0 + 16 * lane.  One wait state between the write of
// m0 and the load (s_nop).
__device__ __forceinline__ void glds_x4(const float* sbase, int voff, unsigned lds_byte_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" LSR_PRIMS_GLDS_SUFFIX
               :
               : "v"(voff), "s"(sbase), "s"(lds_byte_addr)
               : "memory");  // (m0 is a reserved register: hipcc sets it right at each of its own uses)
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory");
}
// After a wait: pass the loaded registers through an (empty) volatile asm, so that every later use
// depends on a statement the compiler keeps behind the wait.
template <int K>
__device__ __forceinline__ void tie(float (&a)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) asm volatile("" : "+v"(a[i]));
}
__device__ __forceinline__ void tie(float& a) { asm volatile("" : "+v"(a)); }
// The workgroup barrier, raw: it waits for this wave's LDS operations only, never for the loads in flight
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes have landed
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// ---- tile walk ----------------------------------------------------------------------------------------------------
// XCD-aware order: workgroups b, b+8, ... share an XCD (round-robin dispatch), so every XCD gets a contiguous run of
// the n work items: XCD k owns per + (k < rem) of them.
__device__ __forceinline__ int xcd_contiguous(int b, int n) {
  const int per = n / 8, rem = n % 8;
  const int xcd = b % 8, idx = b / 8;
  return xcd * per + (xcd < rem ? xcd : rem) + idx;
}
// Tiles in bands of kBand tile rows, column-major inside a band, so that the workgroups an XCD keeps resident form a
// compact patch: linear tile index -> (tx, ty).
__device__ __forceinline__ void band_tile(int lin, int tiles_x, int tiles_y, int& tx, int& ty) {
  const int band = lin / (tiles_x * kBand);
  const int lb = lin - band * (tiles_x * kBand);
  const int band_h = min(kBand, tiles_y - band * kBand);
  tx = lb / band_h;
  ty = band * kBand + (lb - tx * band_h);
}
// (The fused kernels walk their work items with xcd_contiguous and the same bands, but spell the band arithmetic out
// themselves: as a call of band_tile, or of one function for the whole walk, hipcc reassociates the tile origin's
// arithmetic and commutes operands of packed multiplies further down -- their instruction streams would move.)

// H^T 1 at (z, y, x): the sum of the taps whose sample lies inside the volume, from the prefix-sum
// table P[a][b][c] = sum_{a'<a, b'<b, c'<c} w of the CALLER's pz x py x px PSF (Args: DenseArgs or YsepArgs).
// (P: the table, staged in LDS by the dense UPDATE kernel -- eight dependent global loads per border
// voxel made the UPDATE launch 22 % slower than the RATIO launch)
template <typename Args>
__device__ float dense_norm(const Args& p, const double* P, int z, int y, int x) {
  const int cz = p.pz / 2, cy = p.py / 2, cx = p.px / 2;
  const int a0 = max(0, cz - z), a1 = min(p.pz, p.Z - z + cz);
  const int b0 = max(0, cy - y), b1 = min(p.py, p.Y - y + cy);
  const int c0 = max(0, cx - x), c1 = min(p.px, p.X - x + cx);
  const int sb = p.px + 1, sa = (p.py + 1) * sb;
  return static_cast<float>(((P[a1 * sa + b1 * sb + c1] - P[a0 * sa + b1 * sb + c1]) -
                             (P[a1 * sa + b0 * sb + c1] - P[a0 * sa + b0 * sb + c1])) -
                            ((P[a1 * sa + b1 * sb + c0] - P[a0 * sa + b1 * sb + c0]) -
                             (P[a1 * sa + b0 * sb + c0] - P[a0 * sa + b0 * sb + c0])));
}

#endif  // __HIPCC__

}  // namespace
}  // namespace prims
}  // namespace lsr
