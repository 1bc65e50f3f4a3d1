// Pieces shared by the two Winograd kernels (conv_wino.hip, conv_wino_wgrad.hip), which keep all 256 accumulator registers of a wave
// in AGPRs: the inline-asm MFMA and the packed-fp32 subtraction.  Kept apart from conv_common.h so that the implicit-GEMM family
// (built with -amdgpu-mfma-vgpr-form) never sees "a"-constrained asm.
#pragma once
#include "conv_common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// v_mfma_f32_16x16x4_f32 with the accumulator pinned to AGPRs ("+a"): with the builtin, hipcc's allocator moved accumulators between
// AGPRs and VGPRs inside the K loops.  MFMA0 starts an accumulator (C = 0).
#define MFMA(acc_, a_, b_) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc_) : "v"(a_), "v"(b_))
#define MFMA0(acc_, a_, b_) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=a"(acc_) : "v"(a_), "v"(b_))

// a - b on two floats at once (same rounding as two v_sub_f32).  PINNED: volatile asm, which stays where it is written between the
// (volatile asm) MFMAs -- conv_wino_wgrad.hip's step; conv_wino.hip's epilogue leaves the placement to hipcc.
template <bool PINNED>
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 d;
  if constexpr (PINNED) asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  else asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}

}  // namespace
