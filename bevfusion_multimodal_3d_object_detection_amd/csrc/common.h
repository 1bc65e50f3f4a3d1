// Shared helpers for the gfx950 kernels of libbevf_hip.so (internal header).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/bevf.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void bevf_set_error(const char* fmt, ...);

#define BEVF_REQUIRE(cond, ...)              \
  do {                                       \
    if (!(cond)) {                           \
      bevf_set_error(__VA_ARGS__);           \
      return BEVF_ERR_ARG;                   \
    }                                        \
  } while (0)

static inline int bevf_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    bevf_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return BEVF_ERR_LAUNCH;
  }
  return BEVF_OK;
}

// Every launch that asks for dynamic LDS goes through bevf_launch.  Above the 64 KB default a kernel has to opt in, and
// the runtime keeps that opt-in per device: bevf_grant_lds (api.hip) remembers the bytes granted per (kernel, device),
// raises them when a launch needs more, and reports a refusal instead of leaving it to the launch.
int bevf_grant_lds(const char* entry, const void* kernel, size_t lds_bytes);

template <typename... P, typename... A>
static inline int bevf_launch(const char* entry, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
                              const A&... args) {
  if (lds_bytes > 64 * 1024) {
    const int rc = bevf_grant_lds(entry, reinterpret_cast<const void*>(kernel), lds_bytes);
    if (rc != BEVF_OK) return rc;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
  return bevf_check_launch(entry);
}

// Runtime flag -> template argument: f(std::true_type{}) or f(std::false_type{}); nest one call per flag and name only the
// combinations that should exist as kernels inside.
template <typename F>
static inline int bevf_dispatch_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

static inline bool bevf_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Blocks b and b+8 share an XCD (one L2 each): give every XCD a contiguous range of tiles so
// that neighbouring tiles -- which share input rows and the weight panel -- hit the same L2.
// Bijective for any grid size (cdna_hip_programming.md, 256^2 template, "XCD swizzle").
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// ---- division by a launch constant (implicit-GEMM convolutions: pixel -> image, row, column; CSR lift kernels) ----
// n / d for 0 <= n < 2^31 by multiply-high: q = umulhi(n, mul) >> sh with mul = ceil(2^(31+s)/d), s = ceil(log2 d), sh = s-1 (exact for
// every such n because the rounding error e < d <= 2^s); mul == 0 means d == 1.  On wave-uniform operands this stays on the scalar unit.
__device__ __forceinline__ int div_by(int n, unsigned mul, unsigned sh) {
  return mul ? (int)(__umulhi((unsigned)n, mul) >> sh) : n;
}
static inline void div_make(int d, unsigned* mul, unsigned* sh) {
  *mul = 0;
  *sh = 0;
  if (d <= 1) return;
  int s = 0;
  while ((1ll << s) < d) ++s;
  *mul = (unsigned)(((1ull << (31 + s)) + (unsigned long long)d - 1) / (unsigned long long)d);
  *sh = (unsigned)(s - 1);
}

// ---- 16-byte channel vectors of either storage type (fp32: 4 channels, bf16: 8 channels) ----------------------
template <typename T> struct vec16 { static constexpr int N = 16 / (int)sizeof(T); };
template <typename T>
__device__ __forceinline__ void load16(const T* p, float (&f)[vec16<T>::N]) {
  if constexpr (sizeof(T) == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = v[j];
  } else {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
  }
}
template <typename T>
__device__ __forceinline__ void store16(T* p, const float (&f)[vec16<T>::N]) {
  if constexpr (sizeof(T) == 4) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = f[j];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    bf16x8_t v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)f[j];
    *reinterpret_cast<bf16x8_t*>(p) = v;
  }
}

// ---- helpers of the CSR pool / lift kernels (camera_lift.hip, camera_frustum.hip) ---------------------------------
// Sum / max over the L lanes (a power of two, aligned) that hold one row: xor butterfly, widest stride first.  IEEE addition is
// commutative, so both lanes of a pair compute the same bits and every lane of the group ends with the same value.
template <bool MAX>
__device__ __forceinline__ float group_reduce(float v, int L) {
  for (int m = L >> 1; m > 0; m >>= 1) {
    const float o = __shfl_xor(v, m, 64);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  return v;
}
