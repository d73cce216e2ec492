// mfma_tile.h -- the device primitives that the MFMA kernels share (the two GEMM cores linear_dma.hip / linear_split.hip,
// linear_group.hip, the attention in dense.hip / attention_bwd.hip, the sparse convolution in conv_body.h): vector types, the
// 32x32 accumulator layout, LDS-DMA issue, the exact three-piece bf16 split, the XCD-aware renumbering.  ONE definition each:
// the producers and consumers of bf16 pieces (weight preparation, the attention's K / V piece kernels, its sweep, the GEMM's
// V-piece epilogue) must split bit for bit alike, and so must everyone who maps an accumulator register to a row.
// Device-only; include after common.h.  Nothing with a single user belongs here.
#pragma once

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

// accumulator register e of lane half h holds row rowmap(e, h) of a 32x32 MFMA result (column = lane & 31)
__device__ __forceinline__ int rowmap(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// ---- LDS-DMA ---------------------------------------------------------------------------------------------------------------
// the (wave-uniform) LDS byte address of a pointer into a __shared__ array
__device__ __forceinline__ unsigned lds_addr(const void *p) {
  return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_void_t *)p);
}
// One LDS-DMA wave-instruction: 64 lanes x 16 B from per-lane global addresses to LDS at (wave-uniform) lds_byte_addr +
// lane*16.  Inline asm on purpose: issued through the builtin, hipcc drains it (vmcnt(0)) before the next ds_read of the
// same LDS array, which would serialise the pipeline; an asm load is not in the compiler's counters, so the kernel waits
// for it itself (s_waitcnt vmcnt(..) before the barrier that publishes the piece).  M0 is saved/restored inside the
// statement (guide section 5.7).
__device__ __forceinline__ void glds16(const void *gsrc, unsigned lds_byte_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_byte_addr) : "memory");
}
// the same with the source as (wave-uniform 64-bit base in an SGPR pair) + (per-lane 32-bit byte offset): no vector address
// arithmetic
__device__ __forceinline__ void glds16_s(unsigned voff, const void *sbase, unsigned lds_byte_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_byte_addr) : "memory");
}
// N pieces whose LDS destinations are 1 KiB apart, ONE M0 value: the destination of piece i is the instruction's offset
// field (i * 1024), which the hardware adds to the GLOBAL address as well -- the caller's source pointer of piece i is
// pre-decremented by i * 1024 bytes.  One wave pays ~45 cycles per piece for this form against ~58 for an M0 write per
// piece (tools/ubench_glds.hip; four waves issuing at once: 83 against 119).
template <int N>
__device__ __forceinline__ void glds16_group(const float *const *gsrc, unsigned lds_byte_addr) {
  static_assert(N >= 1 && N <= 4, "pieces per group");
  if constexpr (N == 1) {
    glds16(gsrc[0], lds_byte_addr);
  } else {
    unsigned keep;
    if constexpr (N == 2)
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                   "global_load_lds_dwordx4 %2, off offset:1024\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gsrc[0]), "v"(gsrc[1]), "s"(lds_byte_addr) : "memory");
    else if constexpr (N == 3)
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                   "global_load_lds_dwordx4 %2, off offset:1024\n\tglobal_load_lds_dwordx4 %3, off offset:2048\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gsrc[0]), "v"(gsrc[1]), "v"(gsrc[2]), "s"(lds_byte_addr) : "memory");
    else
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                   "global_load_lds_dwordx4 %2, off offset:1024\n\tglobal_load_lds_dwordx4 %3, off offset:2048\n\t"
                   "global_load_lds_dwordx4 %4, off offset:3072\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gsrc[0]), "v"(gsrc[1]), "v"(gsrc[2]), "v"(gsrc[3]), "s"(lds_byte_addr) : "memory");
  }
}

// ---- fp32 as the exact sum of three bf16 pieces (the scheme: linear_split.hip) ------------------------------------------------
// two floats -> two bf16 (round to nearest even: v_cvt_pk_bf16_f32), low half = a
__device__ __forceinline__ unsigned bf16_cvt2(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// (x0, x1) -> packed pieces h, m, l with x = h + m + l exactly
__device__ __forceinline__ void bf16_split2(float x0, float x1, unsigned &h, unsigned &m, unsigned &l) {
  // (the empty asm statements keep the two subtractions of a pair from being fused into one v_pk_add_f32: packed fp32 VALU beside
  //  MFMAs costs more than the two scalar instructions it replaces -- MI355X_MICROARCH.md, cycle constants)
  h = bf16_cvt2(x0, x1);
  float r0 = x0 - __uint_as_float(h << 16);
  asm volatile("" : "+v"(r0));
  float r1 = x1 - __uint_as_float(h & 0xffff0000u);
  asm volatile("" : "+v"(r1));
  m = bf16_cvt2(r0, r1);
  float s0 = r0 - __uint_as_float(m << 16);
  asm volatile("" : "+v"(s0));
  float s1 = r1 - __uint_as_float(m & 0xffff0000u);
  asm volatile("" : "+v"(s1));
  l = bf16_cvt2(s0, s1);
}
// four packed pairs as the MFMA's bf16 operand
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

// ---- XCD-aware renumbering ----------------------------------------------------------------------------------------------------
// Workgroup ids are dealt round-robin over the 8 XCDs (each with its own L2): workgroup id runs on XCD id & 7.  The first index
// of that XCD's contiguous share of n items (the shares of the first n % 8 XCDs are one longer): the workgroup works on item
// xcd_first(id, n) + (id >> 3), so the workgroups that share an L2 hold neighbouring items (a pure speed / traffic choice,
// never a correctness one).
__device__ __forceinline__ int xcd_first(int id, int n) {
  const int xq = n >> 3, xr = n & 7, xcd = id & 7;
  return xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq;
}
// a workgroup's tiles of a launch of gridDim.x (persistent) workgroups: t_lo, t_lo + t_stride, ... < t_hi -- XCD x owns a
// contiguous range of tiles and its workgroups (slot = id / 8) walk it with stride gridDim / 8
__device__ __forceinline__ void xcd_tile_range(bool remap, int tiles, int &t_lo, int &t_hi, int &t_stride) {
  const int id = blockIdx.x, nwg = gridDim.x;
  if (remap && (nwg & 7) == 0) {
    const int x_lo = xcd_first(id, tiles);
    t_lo = x_lo + (id >> 3);
    t_hi = x_lo + (tiles >> 3) + ((id & 7) < (tiles & 7) ? 1 : 0);
    t_stride = nwg >> 3;
  } else {
    t_lo = id; t_hi = tiles; t_stride = nwg;
  }
}

}  // namespace
