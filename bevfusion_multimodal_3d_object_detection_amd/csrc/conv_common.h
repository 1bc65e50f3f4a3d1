// Pieces shared by the implicit-GEMM convolution kernels: launch arguments, buffer descriptor / load helpers, the A-operand walker
// (pixel rows under a moving filter tap) and the epilogue.  Users: conv_igemm.hip (exact fp32 / bf16) and conv_split.hip (fp32 through
// three bf16 planes) take all of it, except that conv_igemm.hip keeps the walker's text in place; conv_wgrad.hip the descriptor / load helpers; conv3x3_bf16.hip
// the vector types, kOob and the 16-byte buffer load; conv_wino.hip and conv_wino_wgrad.hip (through wino_common.h) those, the descriptor
// helper and static_for.
#pragma once
#include "common.h"

#include <type_traits>
#include <utility>

namespace {

// Element type T of activations / weights: float (v_mfma_f32_32x32x2_f32, exact fp32) or __bf16
// (v_mfma_f32_32x32x16_bf16, fp32 accumulate).  Both share the byte geometry: a K step is 8 chunks of 16 B per
// row (32 floats or 64 bf16), so staging, LDS layout, swizzle and fragment reads are identical; for bf16 the
// 16-B fragment a lane reads (k = 8h..8h+7 of a 16-deep group) is exactly the MFMA's operand layout.
struct ConvArgs {
  const void* x;
  const void* w;
  const float* scale;
  const float* shift;
  const void* res;
  void* y;
  uint32_t* colmax;
  int N, H, W, Cin, x_cs;
  int Ho, Wo, Cout, y_cs, res_cs;
  int KH, KW, stride, pad;
  int relu, rows_per_group;
  int M, K, tilesM, tilesN;
  int m_split, nbig, tilesN_big;   // hybrid launch: blocks [0,nbig) = big tiles over rows [0,m_split)
  unsigned div_hw_mul, div_hw_sh, div_w_mul, div_w_sh;   // m / (Ho*Wo) and r / Wo as multiply-high + shift
  const int* run_if;               // optional device word: every workgroup returns at once when it reads 0
  const int* group_rows;           // optional [groups] (colmax launches): a tile whose rows all lie at or past group_rows[g] of their group returns
  const float* bound_g;            // bound pass (conv_split.hip): per-channel error factor, row flags, row-tile stride of a seed launch
  int* flag;
  int tm_stride;
};

constexpr int BK = 32;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr unsigned kOob = 0x80000000u;   // >= num_records of every descriptor below: the load returns 0

// Raw buffer descriptor over `bytes` bytes at p.  A lane offset >= bytes reads as 0 and drops a store; the default covers every tensor
// here (all stay below 2 GiB), so kOob as an OFFSET is always out of range.
template <typename P>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const P* p, unsigned bytes = kOob) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<P*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
  return __builtin_bit_cast(f32x4, v);
}

// Compile-time index loop: f(ic<0>{}), ..., f(ic<N - 1>{}) in order -- for bodies whose index has to be a constant expression
// (which register array element, which MFMA gap), where `#pragma unroll` only makes it a constant after the fact.
template <int C> using ic = std::integral_constant<int, C>;
template <typename F, int... I>
__device__ __forceinline__ void static_for_seq(F&& f, std::integer_sequence<int, I...>) {
  (f(ic<I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_seq(f, std::make_integer_sequence<int, N>{});
}

// bevf_conv_desc -> ConvArgs for the implicit-GEMM entry points: the rules they share, reported as "<who>: ...", then the fill
// (tile counts and the hybrid split stay zero for the launch helpers).  x_es / w_es = bytes per activation / weight element.
// The rules that only one kernel has (y / colmax presence, y_cs, ...) stay in its entry point.
static int conv_args_from_desc(const bevf_conv_desc* d, const char* who, int x_es, int w_es, ConvArgs* out) {
  BEVF_REQUIRE(d && d->x && d->w, "%s: null x/w", who);
  BEVF_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0 && d->Cout > 0, "%s: empty shape", who);
  BEVF_REQUIRE(d->Cin > 0 && d->Cin % (128 / x_es) == 0, "%s: Cin=%d must be a positive multiple of %d", who, d->Cin, 128 / x_es);
  BEVF_REQUIRE(d->x_cs >= d->Cin && d->x_cs % (16 / x_es) == 0, "%s: x_cs=%d must be >= Cin and a multiple of %d", who, d->x_cs, 16 / x_es);
  BEVF_REQUIRE(bevf_aligned16(d->x) && bevf_aligned16(d->w), "%s: x/w must be 16-byte aligned", who);
  BEVF_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, "%s: bad kernel geometry", who);
  BEVF_REQUIRE((d->H + 2 * d->pad - d->KH) / d->stride + 1 == d->Ho && (d->W + 2 * d->pad - d->KW) / d->stride + 1 == d->Wo,
               "%s: Ho/Wo (%d,%d) inconsistent with H,W,k,stride,pad", who, d->Ho, d->Wo);
  BEVF_REQUIRE(!d->res || d->res_cs >= d->Cout, "%s: res_cs < Cout", who);
  BEVF_REQUIRE((long long)d->N * d->H * d->W * d->x_cs * x_es < (1ll << 31) &&
                   (long long)d->Cout * d->KH * d->KW * d->Cin * w_es < (1ll << 31),
               "%s: input / weight buffers must stay below 2 GiB (32-bit buffer offsets)", who);
  const long long M = (long long)d->N * d->Ho * d->Wo;
  BEVF_REQUIRE(M < (1ll << 31), "%s: pixel count overflows int32", who);
  ConvArgs& a = *out;
  a.x = d->x; a.w = d->w; a.scale = d->scale; a.shift = d->shift; a.res = d->res; a.y = d->y; a.colmax = d->colmax;
  a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.x_cs = d->x_cs;
  a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout; a.y_cs = d->y_cs; a.res_cs = d->res_cs;
  a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
  a.relu = d->relu; a.rows_per_group = d->rows_per_group;
  a.M = (int)M; a.K = d->KH * d->KW * d->Cin; a.tilesM = a.tilesN = 0;
  a.m_split = 0; a.nbig = 0; a.tilesN_big = 0;
  a.run_if = nullptr; a.group_rows = nullptr; a.bound_g = nullptr; a.flag = nullptr; a.tm_stride = 1;
  div_make(d->Ho * d->Wo, &a.div_hw_mul, &a.div_hw_sh);
  div_make(d->Wo, &a.div_w_mul, &a.div_w_sh);
  return BEVF_OK;
}

// A operand of the implicit GEMM: the thread's 16-byte chunk `chunk` of the tile rows row0 + 32*j (j < AP), walked over K = (kh, kw, c0).
// ES = bytes per activation element; a K step is 8 chunks = 128 / ES channels of ONE filter tap.  Nothing here costs vector-ALU work per
// K step: voff[j] is the byte offset of the row's pixel under tap (pad, pad), fixed for the tile; the tap moves the descriptor's scalar
// base, the channel chunk is the scalar offset, and eff[j] = voff[j] or kOob (the hardware's zero = the padding) changes only when the
// tap does.  Rows past m_hi have voff = kOob and coordinates far outside every image.  (kh, kw, c0) is the state of the NEXT load().
// conv_igemm.hip's conv_tile holds a copy of this text (why: DESIGN 3.1, "Deviation"): a fix here belongs there too.
template <int ES, int AP>
struct ConvAWalker {
  static constexpr int EPC = 16 / ES, BKE = 8 * EPC;      // elements per chunk / per K step
  unsigned voff[AP], eff[AP];
  int ih0[AP], iw0[AP];
  int kh, kw, c0;

  __device__ __forceinline__ void init(const ConvArgs& p, const int row0, const int m_hi, const int chunk) {
    const int HoWo = p.Ho * p.Wo;
#pragma unroll
    for (int j = 0; j < AP; ++j) {
      const int m = row0 + 32 * j;
      if (m < m_hi) {
        const int n = div_by(m, p.div_hw_mul, p.div_hw_sh), r = m - n * HoWo;
        const int oh = div_by(r, p.div_w_mul, p.div_w_sh), ow = r - oh * p.Wo;
        voff[j] = (unsigned)((((n * p.H + oh * p.stride) * p.W + ow * p.stride) * p.x_cs + chunk * EPC) * ES);
        ih0[j] = oh * p.stride - p.pad;
        iw0[j] = ow * p.stride - p.pad;
      } else {
        voff[j] = kOob;
        ih0[j] = -(1 << 24);
        iw0[j] = -(1 << 24);
      }
    }
    kh = kw = c0 = 0;
    set_tap(p);
  }
  __device__ __forceinline__ void set_tap(const ConvArgs& p) {     // VALU work only when the filter tap changes
#pragma unroll
    for (int j = 0; j < AP; ++j) {
      const int ih = ih0[j] + kh, iw = iw0[j] + kw;
      eff[j] = ((unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W) ? voff[j] : kOob;
    }
  }
  __device__ __forceinline__ void load(const ConvArgs& p, f32x4 (&ra)[AP]) const {
    const char* base = static_cast<const char*>(p.x) + ((long)(kh - p.pad) * p.W + (kw - p.pad)) * p.x_cs * ES;
    const __amdgpu_buffer_rsrc_t rsrcA = buf_rsrc(base);
#pragma unroll
    for (int j = 0; j < AP; ++j) ra[j] = buf_load16(rsrcA, eff[j], (unsigned)(c0 * ES));
  }
  __device__ __forceinline__ void advance(const ConvArgs& p) {     // to the next K step: chunk -> tap walk
    c0 += BKE;
    if (c0 == p.Cin) {
      c0 = 0;
      if (++kw == p.KW) { kw = 0; ++kh; }
      set_tap(p);
    }
  }
};

// The two pieces of finishing arithmetic that the three store paths of conv_epilogue share.  scale / shift of output channel n (folded
// BatchNorm or bias; null pointers = 1 and 0):
__device__ __forceinline__ void conv_scale_shift(const ConvArgs& p, const int n, float& sc, float& sh) {
  sc = p.scale ? p.scale[n] : 1.f;
  sh = p.shift ? p.shift[n] : 0.f;
}
// and one accumulator value -> output value: folded BN, then the residual, then ReLU.  The flags are compile-time constants in the
// full-tile variants and wave-uniform values elsewhere; after inlining both cost what the hand-written forms did.
__device__ __forceinline__ float conv_finish(const float acc, const float sc, const float sh, const bool has_res, const float rv,
                                             const bool relu) {
  float t = fmaf(acc, sc, sh);
  if (has_res) t += rv;
  return relu ? fmaxf(t, 0.f) : t;
}

// Epilogue of one workgroup tile.  acc[mi][ni] is the 32x32 MFMA tile (mi, ni) of this wave: C[i][j] with
// j = lane&31 (channel) and i = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel).  T = storage type of y / res.
template <typename T, int BM, int BN, int WM, int WN>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& p, f32x16 (&acc)[WM / 32][WN / 32], const int m0,
                                              const int n0, const int m_hi, const int wm, const int wn, const int lane,
                                              char* const scratch = nullptr) {
  constexpr int ES = (int)sizeof(T);
  constexpr bool kF32 = std::is_same<T, float>::value;
  constexpr int MI = WM / 32, NI = WN / 32;
  const int h = lane >> 5, l31 = lane & 31;
  // ---- epilogue: C[i][j], j = lane&31 (channel), i = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel) ----
  // Branch-free per element: residual loads of a 32x32 tile are issued as one batch (rows past
  // the end are clamped for the load and masked at the store).
  const int m_base = m0 + wm * WM, n_base = n0 + wn * WN;
  if (!p.colmax && m0 + BM <= m_hi && n0 + BN <= p.Cout) {
    // full tile: buffer stores whose row offset is the instruction's SCALAR offset (SALU arithmetic) and whose
    // lane offset is computed once; residual / ReLU chosen once -- 2-3 VALU instructions per output element
    const __amdgpu_buffer_rsrc_t ry = buf_rsrc(static_cast<const T*>(p.y) + (size_t)m_base * p.y_cs + n_base);
    const __amdgpu_buffer_rsrc_t rr = buf_rsrc(static_cast<const T*>(p.res) + (size_t)m_base * p.res_cs + n_base);
    const unsigned y_lane = (unsigned)((4 * h * p.y_cs + l31) * ES);
    const unsigned r_lane = (unsigned)((4 * h * p.res_cs + l31) * ES);
    auto run = [&](auto has_res, auto do_relu) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        float sc, sh;
        conv_scale_shift(p, n_base + ni * 32 + l31, sc, sh);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          float rv[16] = {};
          if constexpr (decltype(has_res)::value) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const unsigned so = (unsigned)(((mi * 32 + (r & 3) + 8 * (r >> 2)) * p.res_cs + ni * 32) * ES);
              if constexpr (kF32) {
                rv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, r_lane, so, 0));
              } else {
                const unsigned short u = __builtin_amdgcn_raw_buffer_load_b16(rr, r_lane, so, 0);
                rv[r] = __builtin_bit_cast(float, (unsigned)u << 16);
              }
            }
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float t = conv_finish(acc[mi][ni][r], sc, sh, decltype(has_res)::value, rv[r], decltype(do_relu)::value);
            const unsigned so = (unsigned)(((mi * 32 + (r & 3) + 8 * (r >> 2)) * p.y_cs + ni * 32) * ES);
            if constexpr (kF32)
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, t), ry, y_lane, so, 0);
            else
              __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (__bf16)t), ry, y_lane, so, 0);
          }
        }
      }
    };
    using TT = std::true_type;
    using FF = std::false_type;
    if constexpr (!kF32) {
      // bf16 output without a residual: the accumulator layout puts ONE channel of 16 pixels in a lane -- 2-byte stores, 16 per 32x32
      // tile, 64-byte runs (the access SHAPE that bounded conv3x3_bf16's short-K layers and 40 % of the bf16 stem).  Through a wave-local
      // LDS transpose (scratch: the operand tiles are dead after the K loop's last barrier) a lane stores 16 bytes = 8 channels of a pixel
      // and a wave row is WN * 2 contiguous bytes (a whole 128-byte line at WN = 64).  Same values, same rounding.
      if (scratch && !p.res && (p.y_cs * ES) % 16 == 0 && (reinterpret_cast<uintptr_t>(p.y) & 15u) == 0) {
        constexpr int PITCH = NI * 64 + 16;                           // bytes per pixel row of the wave's tile (pad: the two lane halves on different banks)
        constexpr int PPP = NI * 4;                                   // 16-byte pieces per pixel
        char* const ws = scratch + (wm * (BN / WN) + wn) * (32 * PITCH);
        float scv[NI], shv[NI];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) conv_scale_shift(p, n_base + ni * 32 + l31, scv[ni], shv[ni]);
        const bool relu = p.relu != 0;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float t = conv_finish(acc[mi][ni][r], scv[ni], shv[ni], false, 0.f, relu);
              *reinterpret_cast<__bf16*>(ws + ((r & 3) + 8 * (r >> 2) + 4 * h) * PITCH + (ni * 32 + l31) * 2) = (__bf16)t;
            }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int k = 0; k < NI * 2; ++k) {
            const int idx = k * 64 + lane, px = idx / PPP, piece = idx - px * PPP;
            const u32x4 q = *reinterpret_cast<const u32x4*>(ws + px * PITCH + piece * 16);
            __builtin_amdgcn_raw_buffer_store_b128(q, ry, (unsigned)(((mi * 32 + px) * p.y_cs) * ES + piece * 16), 0, 0);
          }
          asm volatile("" ::: "memory");
        }
        return;
      }
    }
    if (p.res) { if (p.relu) run(TT{}, TT{}); else run(TT{}, FF{}); }
    else       { if (p.relu) run(FF{}, TT{}); else run(FF{}, FF{}); }
    return;
  }
  bool cm_fast = false;
  int cm_group = 0;
  if (p.colmax) {
    cm_group = m0 / p.rows_per_group;
    cm_fast = (m0 + BM <= m_hi) && ((m0 + BM - 1) / p.rows_per_group == cm_group);
  }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int n = n_base + ni * 32 + l31;
    const bool nok = n < p.Cout;
    const int nc = nok ? n : p.Cout - 1;
    float sc, sh;
    conv_scale_shift(p, nc, sc, sh);
    float vmax = 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int mrow = m_base + mi * 32 + 4 * h;
      float rv[16];
      if (p.res) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int m = mrow + (r & 3) + 8 * (r >> 2);
          m = m < m_hi ? m : m_hi - 1;
          rv[r] = (float)static_cast<const T*>(p.res)[(size_t)m * p.res_cs + nc];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = 0.f;
      }
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = conv_finish(acc[mi][ni][r], sc, sh, true, rv[r], p.relu != 0);   // rv = +0 without a residual
      if (p.y) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mrow + (r & 3) + 8 * (r >> 2);
          if (m < m_hi && nok) static_cast<T*>(p.y)[(size_t)m * p.y_cs + n] = (T)v[r];
        }
      }
      if (p.colmax) {
        if (cm_fast) {
#pragma unroll
          for (int r = 0; r < 16; ++r) vmax = fmaxf(vmax, v[r]);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = mrow + (r & 3) + 8 * (r >> 2);
            if (m < m_hi && nok)
              atomicMax(&p.colmax[(size_t)(m / p.rows_per_group) * p.Cout + n], __float_as_uint(fmaxf(v[r], 0.f)));
          }
        }
      }
    }
    if (p.colmax && cm_fast) {
      vmax = fmaxf(vmax, __shfl_xor(vmax, 32));
      if (h == 0 && nok) atomicMax(&p.colmax[(size_t)cm_group * p.Cout + n], __float_as_uint(fmaxf(vmax, 0.f)));
    }
  }
}

}  // namespace
