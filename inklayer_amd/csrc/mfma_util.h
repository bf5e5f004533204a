// Device scaffolding of the MFMA kernels (ffn_fused, proj_ln, upscale_tail, attention, attention_win, attention_glob,
// gemm): address-space typedefs, compile-time loops, the 32x32x16 MFMA wrapper, and the asm-pinned LDS reads and VALU
// ops.  One copy: a new fused kernel includes this header instead of copying the block.  Everything sits in the
// including file's anonymous namespace and is __forceinline__, so the library gains no symbol.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

// LDS-DMA (__builtin_amdgcn_global_load_lds) and ds_read_tr operands
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((address_space(3))) char* lds_char_ptr;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// the 32-bit LDS address of a __shared__ byte, as the asm reads below take it
__device__ __forceinline__ uint32_t lds_addr(char* p) { return (uint32_t)(size_t)(lds_char_ptr)p; }

// static_for<0, N>([&](auto i) { constexpr int I = decltype(i)::value; ... }): a loop whose index is a constant
// expression in the body (asm immediates, register-array indices)
template <int I> using ic = std::integral_constant<int, I>;
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(ic<I>{});
    static_for<I + 1, N>(f);
  }
}

__device__ __forceinline__ f32x16 mfma32(const f16x8& a, const f16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// transposing LDS read: four f16 of a column-major 16-B group
__device__ __forceinline__ f16x4 tr_read(const char* p) {
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(p));
  return __builtin_bit_cast(f16x4, v);
}

// ---- pinned LDS reads with counted waits -----------------------------------------------------------------------
// Fragment reads are volatile asm so that they KEEP their distance to the MFMA that consumes them (left to itself hipcc
// sinks every ds_read next to its use and waits lgkmcnt(0) in front of each MFMA: 6000 instead of 2100 cycles per chunk
// of ffn_fused.hip); the counted wait is tied to the fragment it releases, which orders the MFMA behind it.  This holds
// only while nothing else in the loop uses lgkmcnt (LDS returns in order).
// THE HAZARD: the compiler does not know that such a read completes later.  If it SPILLS the destination register, it
// stores the register before the data has arrived (round 3: NaNs from a 32-byte spill).  So every file that uses these
// reads is listed in build.py's NO_SPILL, which fails the build unless each of its kernels reports zero scratch.
template <int OFF>
__device__ __forceinline__ f16x8 lds_frag(uint32_t addr) {
  f16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int N>
__device__ __forceinline__ void wait_frag(f16x8& f) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(f) : "n"(N));
}
// four parameter vectors (2 x gamma, 2 x beta of one 8-column group pair) through the same pinned path: as plain loads
// hipcc puts all 64 of a LayerNorm in flight at once (256 registers) and spills - which is the hazard above
template <int OFF>
__device__ __forceinline__ f32x4 lds_f4(uint32_t addr) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ void wait_f4(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

// ---- pinned VALU ops (_at: stays AT its place) -------------------------------------------------------------------
// The softmax arithmetic of the one-wave-per-SIMD attention kernels (attention_win.hip, attention_glob.hip) is issued
// through VOLATILE asm statements: they keep their place between the sched_barriers of the MFMA gaps.  As plain (pure)
// operations hipcc's instruction selection hoists them - e.g. all of a tile's second-half exps into the gap that
// computes the row max - before the machine scheduler ever sees the barriers.
__device__ __forceinline__ float max3_at(float a, float b, float c) {
  float d;
  asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float fma_at(float s, float c, float add) {          // s c + add
  float t;
  asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(t) : "v"(s), "v"(c), "v"(add));
  return t;
}
__device__ __forceinline__ float exp2_at(float t) {                             // 2^t
  float d;
  asm volatile("v_exp_f32 %0, %1" : "=v"(d) : "v"(t));
  return d;
}
__device__ __forceinline__ uint32_t cvt_pk_at(float a, float b) {              // two f32 -> packed f16 (RNE)
  uint32_t d;
  asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// The generic flash kernel (attention.hip) uses max3, win4 / glob4 use max3_at, and they are not interchangeable: this
// one is plain asm - one instruction for the row max that hipcc may move and merge freely, as it must in a kernel whose
// schedule is the compiler's - while max3_at holds its MFMA gap.
__device__ __forceinline__ float max3(float a, float b, float c) {
  float d;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

}  // namespace
