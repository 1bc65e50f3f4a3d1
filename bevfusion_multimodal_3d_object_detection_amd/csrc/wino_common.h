// Pieces shared by the two Winograd kernels (conv_wino.hip, conv_wino_wgrad.hip), which keep all 256 accumulator registers of a wave
// in AGPRs: the inline-asm MFMA (accumulators as "+a" operands for conv_wino_wgrad.hip, by register name for conv_wino.hip) and the
// packed-fp32 subtraction.  Kept apart from conv_common.h so that the implicit-GEMM family
// (built with -amdgpu-mfma-vgpr-form) never sees "a"-constrained asm.
#pragma once
#include "conv_common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// v_mfma_f32_16x16x4_f32 with the accumulator pinned to AGPRs ("+a"): with the builtin, hipcc's allocator moved accumulators between
// AGPRs and VGPRs inside the K loops.  MFMA0 starts an accumulator (C = 0).
#define MFMA(acc_, a_, b_) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc_) : "v"(a_), "v"(b_))
#define MFMA0(acc_, a_, b_) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=a"(acc_) : "v"(a_), "v"(b_))

// The same MFMA on accumulator registers given BY NAME: a[R : R + 3], R a compile-time constant.  hipcc then has no accumulator variable
// to allocate, copy, zero or spill (around a tile loop it did all four to "+a" operands).  Each asm names the four registers it writes
// as clobbered -- a K-loop group writes all 256, so nothing of hipcc's own can live in an AGPR across one -- and a clobber has to be a
// literal, hence one case per register quad.  ZERO starts the accumulator (C = 0).  The hazards are the caller's: hipcc sees neither
// that an MFMA is in flight nor which registers it will write.
#define WINO_MFMA_AT_(r0, r1, r2, r3)                                                                                              \
  else if constexpr (R == r0) {                                                                                                    \
    if constexpr (ZERO) asm volatile("v_mfma_f32_16x16x4_f32 a[%0:%1], %2, %3, 0" ::"n"(r0), "n"(r3), "v"(a), "v"(b) : "a" #r0, "a" #r1, "a" #r2, "a" #r3); \
    else asm volatile("v_mfma_f32_16x16x4_f32 a[%0:%1], %2, %3, a[%0:%1]" ::"n"(r0), "n"(r3), "v"(a), "v"(b) : "a" #r0, "a" #r1, "a" #r2, "a" #r3); \
  }
#define WINO_MFMA_ALL_ \
  WINO_MFMA_AT_(0, 1, 2, 3) WINO_MFMA_AT_(4, 5, 6, 7) WINO_MFMA_AT_(8, 9, 10, 11) WINO_MFMA_AT_(12, 13, 14, 15) WINO_MFMA_AT_(16, 17, 18, 19) WINO_MFMA_AT_(20, 21, 22, 23) \
  WINO_MFMA_AT_(24, 25, 26, 27) WINO_MFMA_AT_(28, 29, 30, 31) WINO_MFMA_AT_(32, 33, 34, 35) WINO_MFMA_AT_(36, 37, 38, 39) WINO_MFMA_AT_(40, 41, 42, 43) WINO_MFMA_AT_(44, 45, 46, 47) \
  WINO_MFMA_AT_(48, 49, 50, 51) WINO_MFMA_AT_(52, 53, 54, 55) WINO_MFMA_AT_(56, 57, 58, 59) WINO_MFMA_AT_(60, 61, 62, 63) WINO_MFMA_AT_(64, 65, 66, 67) WINO_MFMA_AT_(68, 69, 70, 71) \
  WINO_MFMA_AT_(72, 73, 74, 75) WINO_MFMA_AT_(76, 77, 78, 79) WINO_MFMA_AT_(80, 81, 82, 83) WINO_MFMA_AT_(84, 85, 86, 87) WINO_MFMA_AT_(88, 89, 90, 91) WINO_MFMA_AT_(92, 93, 94, 95) \
  WINO_MFMA_AT_(96, 97, 98, 99) WINO_MFMA_AT_(100, 101, 102, 103) WINO_MFMA_AT_(104, 105, 106, 107) WINO_MFMA_AT_(108, 109, 110, 111) WINO_MFMA_AT_(112, 113, 114, 115) WINO_MFMA_AT_(116, 117, 118, 119) \
  WINO_MFMA_AT_(120, 121, 122, 123) WINO_MFMA_AT_(124, 125, 126, 127) WINO_MFMA_AT_(128, 129, 130, 131) WINO_MFMA_AT_(132, 133, 134, 135) WINO_MFMA_AT_(136, 137, 138, 139) WINO_MFMA_AT_(140, 141, 142, 143) \
  WINO_MFMA_AT_(144, 145, 146, 147) WINO_MFMA_AT_(148, 149, 150, 151) WINO_MFMA_AT_(152, 153, 154, 155) WINO_MFMA_AT_(156, 157, 158, 159) WINO_MFMA_AT_(160, 161, 162, 163) WINO_MFMA_AT_(164, 165, 166, 167) \
  WINO_MFMA_AT_(168, 169, 170, 171) WINO_MFMA_AT_(172, 173, 174, 175) WINO_MFMA_AT_(176, 177, 178, 179) WINO_MFMA_AT_(180, 181, 182, 183) WINO_MFMA_AT_(184, 185, 186, 187) WINO_MFMA_AT_(188, 189, 190, 191) \
  WINO_MFMA_AT_(192, 193, 194, 195) WINO_MFMA_AT_(196, 197, 198, 199) WINO_MFMA_AT_(200, 201, 202, 203) WINO_MFMA_AT_(204, 205, 206, 207) WINO_MFMA_AT_(208, 209, 210, 211) WINO_MFMA_AT_(212, 213, 214, 215) \
  WINO_MFMA_AT_(216, 217, 218, 219) WINO_MFMA_AT_(220, 221, 222, 223) WINO_MFMA_AT_(224, 225, 226, 227) WINO_MFMA_AT_(228, 229, 230, 231) WINO_MFMA_AT_(232, 233, 234, 235) WINO_MFMA_AT_(236, 237, 238, 239) \
  WINO_MFMA_AT_(240, 241, 242, 243) WINO_MFMA_AT_(244, 245, 246, 247) WINO_MFMA_AT_(248, 249, 250, 251) WINO_MFMA_AT_(252, 253, 254, 255)
template <int R, bool ZERO>
__device__ __forceinline__ void mfma_named(float a, float b) {
  static_assert(R >= 0 && R % 4 == 0 && R + 3 < 256, "accumulator register range");
  if constexpr (false) {
  }
  WINO_MFMA_ALL_
}
// One accumulator register -> a VGPR, where the epilogue uses it.  Volatile: it stays behind the MFMAs and the wait that lets them land.
template <int R>
__device__ __forceinline__ float acc_named() {
  static_assert(R >= 0 && R < 256, "accumulator register");
  float v;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(v) : "n"(R));
  return v;
}

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
