// The stages shared by the two bilinear NHWC BEV resamplers -- the ego-motion warp (bev_warp.hip) and the seg head's
// grid resample (bev_seg.hip) -- each written once.  The two differ in where a sample comes from (a planar affine map
// per frame / two separable axis maps) and in how the backward finds its candidates; everything after that is here:
//   forward   resample_forward: a wave takes CELLS_PER_WAVE consecutive output cells, lane k computes cell k's fp64 sample (the file's
//             sampler), the wave walks the cells with each sample read back as scalars (read_sample), builds the four corner rows
//             (corner_rows) and the lanes walk the channels (resample_channels): one product and three fmas in the corner order
//             (i0,j0), (i0,j0+1), (i0+1,j0), (i0+1,j0+1).  That order is the contract of both kernels.
//   backward  accumulate_targets: the wave walks the contributing candidates of a ballot in ascending lane order and adds
//             w * dy[target] by fma, one channel group per lane.
// Everything is inlined into the including file's kernels; wave-uniform values stay on the scalar unit.
#pragma once
#include "common.h"

namespace {

constexpr int CELLS_PER_BLOCK = 4;  // waves per 256-thread block: one source cell each in the backward kernels ...
constexpr int CELLS_PER_WAVE = 4;   // ... and this many output cells each in the forward kernels

// Q channels at p <-> fp32: Q = 1 scalar, fp32 as quads (16 bytes), bf16 as 4 (8 bytes) or 8 (16 bytes, common.h).
template <typename T, int Q>
__device__ __forceinline__ void load_q(const T* p, float (&f)[Q]) {
  if constexpr (Q == 1) {
    f[0] = (float)p[0];
  } else if constexpr (sizeof(T) == 4 || Q == 8) {
    static_assert(Q == vec16<T>::N, "fp32 moves as channel quads, bf16 as four or eight channels");
    load16(p, f);
  } else {
    static_assert(Q == 4, "fp32 moves as channel quads, bf16 as four or eight channels");
    typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
    const bf16x4_t v = *reinterpret_cast<const bf16x4_t*>(p);
#pragma unroll
    for (int k = 0; k < Q; ++k) f[k] = (float)v[k];
  }
}

// NT: fp32 quads leave as non-temporal stores (a map larger than the 256 MiB cache); the other forms are plain.
template <typename T, int Q, bool NT = false>
__device__ __forceinline__ void store_q(T* p, const float (&f)[Q]) {
  if constexpr (Q == 1) {
    p[0] = (T)f[0];
  } else if constexpr (sizeof(T) == 4 && NT) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < Q; ++k) v[k] = f[k];
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
  } else if constexpr (sizeof(T) == 4 || Q == 8) {
    store16(p, f);
  } else {
    typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
    bf16x4_t v;
#pragma unroll
    for (int k = 0; k < Q; ++k) v[k] = (__bf16)f[k];
    *reinterpret_cast<bf16x4_t*>(p) = v;
  }
}

// A bilinear sample: the upper-left corner (i0, j0) and the four weights in the corner order, each rounded once to fp32.
// ok = false: the point is non-finite or more than one cell outside the map -- no corner contributes.
struct CornerSample {
  int i0, j0;
  float w[4];
  bool ok;
};

// The weights of the fractions fi (towards row i0 + 1) and fj (towards column j0 + 1): fp64 products, uncontracted.
__device__ __forceinline__ void corner_weights(double fi, double fj, float (&w)[4]) {
#pragma clang fp contract(off)
  w[0] = (float)((1.0 - fi) * (1.0 - fj));
  w[1] = (float)((1.0 - fi) * fj);
  w[2] = (float)(fi * (1.0 - fj));
  w[3] = (float)(fi * fj);
}

// Lane k's sample as wave-uniform scalars.
__device__ __forceinline__ CornerSample read_sample(const CornerSample& sl, int k) {
  CornerSample s;
  s.i0 = __builtin_amdgcn_readlane(sl.i0, k);
  s.j0 = __builtin_amdgcn_readlane(sl.j0, k);
  s.ok = __builtin_amdgcn_readlane((int)sl.ok, k) != 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) s.w[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sl.w[q]), k));
  return s;
}

// The four corner rows of sample s in frame b of x [.][H][W] rows at stride x_cs; corner k = (di, dj) = (k >> 1, k & 1).  A corner
// outside the map points at cell (0, 0) and is never loaded, so no address is formed outside the buffer.
template <typename T>
__device__ __forceinline__ void corner_rows(const T* __restrict__ x, const CornerSample& s, int b, int H, int W, int x_cs,
                                            int (&in)[4], const T* (&src)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ii = s.i0 + (k >> 1), jj = s.j0 + (k & 1);
    in[k] = s.ok && ii >= 0 && ii < H && jj >= 0 && jj < W;
    src[k] = x + (size_t)((b * H + (in[k] ? ii : 0)) * W + (in[k] ? jj : 0)) * (size_t)x_cs;
  }
}

// Channels [c0, c1) of one output row, Q at a time per lane: the four corner rows weighed and summed in fp32.
template <typename T, int Q, bool NT, bool SHARED>
__device__ __forceinline__ void resample_channels(const T* (&src)[4], const int (&in)[4], const float (&w)[4], T* dst, int c0,
                                                  int c1, int lane) {
  // SHARED: a second walk uses the same flags.  A boolean that lives across two loops is kept in a vector register and compared
  // again in every step; read to a scalar per walk, each loop branches on scalar masks.  (A single walk needs no help, and the
  // readfirstlane would only lengthen the cell's preamble.)
  bool use[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) use[k] = (SHARED ? __builtin_amdgcn_readfirstlane(in[k]) : in[k]) != 0;
  for (int c = c0 + lane * Q; c < c1; c += 64 * Q) {
    float v[4][Q], o[Q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (use[k]) {
        load_q<T, Q>(src[k] + c, v[k]);
      } else {
#pragma unroll
        for (int q = 0; q < Q; ++q) v[k][q] = 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      float a = w[0] * v[0][q];
      a = fmaf(w[1], v[1][q], a);
      a = fmaf(w[2], v[2][q], a);
      o[q] = fmaf(w[3], v[3][q], a);
    }
    store_q<T, Q, NT>(dst + c, o);
  }
}

// The forward of a 256-thread block: y [cells] rows at stride y_cs from x [.][H][W] rows at stride x_cs, P output cells per frame.
// sampler(r) is the CornerSample of output cell r, evaluated by lane k for cell k of the wave (the same instructions in every lane,
// so the cells of a wave share one fp64 preamble).  Q > 0: the lanes move Q channels per access -- all C of them, or C's leading
// multiple of Q with a scalar walk of the rest when TAIL; Q = 0: scalar throughout.
template <typename T, int Q, bool TAIL, bool NT, typename Sampler>
__device__ __forceinline__ void resample_forward(const T* __restrict__ x, T* __restrict__ y, int cells, int P, int H, int W, int C,
                                                 int x_cs, int y_cs, Sampler sampler) {
  static_assert(Q > 0 || TAIL, "nothing would move the channels");
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r0 = (xcd_remap((int)blockIdx.x, (int)gridDim.x) * CELLS_PER_BLOCK + wave) * CELLS_PER_WAVE;
  if (r0 >= cells) return;
  const CornerSample sl = sampler(min(r0 + (lane & (CELLS_PER_WAVE - 1)), cells - 1));
  constexpr int QV = Q > 0 ? Q : 1;
  const int cv = Q == 0 ? 0 : (TAIL ? C / QV * QV : C);   // the vector walk's end
#pragma unroll
  for (int k = 0; k < CELLS_PER_WAVE; ++k) {
    const int r = r0 + k;
    if (r >= cells) break;
    const CornerSample s = read_sample(sl, k);
    int in[4];
    const T* src[4];
    corner_rows(x, s, r / P, H, W, x_cs, in, src);
    T* dst = y + (size_t)r * (size_t)y_cs;
    if constexpr (Q > 0) resample_channels<T, Q, NT, TAIL>(src, in, s.w, dst, 0, cv, lane);
    if constexpr (TAIL) resample_channels<T, 1, false, (Q > 0)>(src, in, s.w, dst, cv, C, lane);
  }
}

// The backward's inner walk.  Lane l holds candidate l: its weight wl and its cell offset pl inside the frame's dy rows (stride
// dy_cs); mask has the contributing lanes.  They are visited in ascending order and acc += w * dy[p][c .. c + Q) by fma -- the order
// is the kernels' bit-reproducibility.  live: this lane has channels to accumulate (the whole wave walks, for the shuffles).
template <int Q>
__device__ __forceinline__ void accumulate_targets(unsigned long long mask, float wl, int pl, const float* __restrict__ dyb, int dy_cs,
                                                   int c, bool live, float (&acc)[Q]) {
  while (mask) {
    const int l = __builtin_ctzll(mask);
    mask &= mask - 1;
    const float w = __shfl(wl, l, 64);
    const int p = __shfl(pl, l, 64);
    if (live) {
      float d[Q];
      load_q<float, Q>(dyb + (size_t)p * (size_t)dy_cs + c, d);
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] = fmaf(w, d[q], acc[q]);
    }
  }
}

}  // namespace
