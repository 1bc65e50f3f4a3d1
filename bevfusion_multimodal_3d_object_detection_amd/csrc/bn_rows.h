// Shared pieces of the train-mode BatchNorm kernels (norm_train.hip) and of the kernels that evaluate relu(batchnorm(x)) on
// load (train_misc.hip): the forward affine, the row map, the row stream, the partial-sum epilogue and the max-pool gather.
// Each is defined here ONCE: the fused paths are bit-identical to the unfused chains because they run this very code.
#pragma once
#include "common.h"

// Per-channel constants of one channel quad (channels c..c+3).  Null pointers: mean 0, invstd 1, gamma 1, beta 0.
// pre() is THE forward pre-activation, y = act(pre(x) (+ res)), and pre(x) > 0 is THE recomputed ReLU mask: bn_apply, both
// backward passes, the stem max-pool and the PointNet group max all call it, so forward value and backward mask cannot drift
// apart.  Both fmaf are explicit: the bits do not depend on the contraction choices of the surrounding function.
struct BnQuad {
  float mu[4] = {0.f, 0.f, 0.f, 0.f}, is[4] = {1.f, 1.f, 1.f, 1.f}, fa[4] = {1.f, 1.f, 1.f, 1.f}, fb[4] = {0.f, 0.f, 0.f, 0.f};
  BnQuad() = default;
  __device__ __forceinline__ BnQuad(const float* __restrict__ mean, const float* __restrict__ invstd,
                                    const float* __restrict__ gamma, const float* __restrict__ beta, int c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mu[j] = mean ? mean[c + j] : 0.f;
      is[j] = invstd ? invstd[c + j] : 1.f;
      fa[j] = (gamma ? gamma[c + j] : 1.f) * is[j];
      fb[j] = fmaf(-mu[j], fa[j], beta ? beta[c + j] : 0.f);
    }
  }
  __device__ __forceinline__ float pre(float x, int j) const { return fmaf(x, fa[j], fb[j]); }
  __device__ __forceinline__ f32x4 pre(f32x4 x) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = pre(x[j], j);
    return x;
  }
  __device__ __forceinline__ f32x4 relu_pre(f32x4 x) const {     // the activation itself: max(pre, 0)
    x = pre(x);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = fmaxf(x[j], 0.f);
    return x;
  }
  __device__ __forceinline__ f32x4 mask(f32x4 x, f32x4 g) const {  // g where the forward's ReLU passed (relu'(0) = 0, as torch)
    x = pre(x);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = x[j] > 0.f ? g[j] : 0.f;
    return g;
  }
};

// dx = gamma*invstd * (dy - sum_dy/M - xhat * sum_dyx/M) for one element; gi = gamma*invstd, sd = sum_dy/M, sx = sum_dyx/M.
// (contraction switched off: every user must agree bit for bit, which contraction decisions that depend on the surrounding
//  code would not guarantee; HIP's __fmul_rn / __fsub_rn are plain operators: they do not stop contraction)
__device__ __forceinline__ float bn_dx(float gi, float g, float sd, float x, float mu, float is, float sx) {
#pragma clang fp contract(off)
  const float t = ((x - mu) * is) * sx;
  const float u = (g - sd) - t;
  return gi * u;
}

// Rows [M][C] on a grid of 256-thread workgroups.  C/4 < 256: thread (cq, rl) keeps channel quad cq = tid % (C/4) and row lane
// rl = tid / (C/4) of `lanes` = 256 / (C/4) for its whole life (threads past lanes * C/4 idle when C/4 does not divide 256).
// C/4 >= 256: one row lane, and a thread walks the quads tid, tid + 256, ...  Row lane rl of workgroup b takes the rows
// first, first + step, ... with first = b * lanes + rl and step = grid * lanes.
__host__ __device__ inline int bn_row_lanes(int C) { return C / 4 >= 256 ? 1 : 256 / (C / 4); }
struct RowMap {
  int c4, lanes, cq0, rl;
  long long first, step;
  __device__ __forceinline__ explicit RowMap(int C)
      : c4(C >> 2), lanes(bn_row_lanes(C)), cq0(c4 < 256 ? threadIdx.x % c4 : threadIdx.x), rl(c4 < 256 ? threadIdx.x / c4 : 0),
        first((long long)blockIdx.x * lanes + rl), step((long long)gridDim.x * lanes) {}
  __device__ __forceinline__ bool idle() const { return rl >= lanes; }
};
#define BN_QUADS(cq, rm) for (int cq = (rm).cq0; cq < (rm).c4; cq += 256)   // one pass unless C > 1024

// The row stream of one thread: load(m, u) for DEPTH rows (slots u = 0..DEPTH-1: that many rows of independent 16-byte loads
// in flight), then use(m, u) for the same rows; the tail goes one row at a time through slot 0.
template <int DEPTH = 4, class Load, class Use>
__device__ __forceinline__ void stream_rows(const RowMap& rm, long long M, Load load, Use use) {
  long long m = rm.first;
  for (; m + (DEPTH - 1) * rm.step < M; m += DEPTH * rm.step) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) load(m + u * rm.step, u);
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) use(m + u * rm.step, u);
  }
  if constexpr (DEPTH > 1)
    for (; m < M; m += rm.step) {
      load(m, 0);
      use(m, 0);
    }
}

// part[blockIdx.x][4cq .. 4cq+3][2] = {a1, a2} summed over the workgroup's row lanes in lane order through LDS (`red`, 256 * 8
// floats of dynamic shared memory).  Every thread of the workgroup calls it once per quad pass, idle threads with zeros.
__device__ __forceinline__ void write_partials(const RowMap& rm, int cq, const float (&a1)[4], const float (&a2)[4],
                                               float* __restrict__ part, int C) {
  extern __shared__ float red[];
  float t1[4], t2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { t1[j] = a1[j]; t2[j] = a2[j]; }
  if (rm.c4 < 256) {                                  // (one quad pass: every thread reaches the barrier exactly once)
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[threadIdx.x * 8 + j] = a1[j]; red[threadIdx.x * 8 + 4 + j] = a2[j]; }
    __syncthreads();
    if ((int)threadIdx.x >= rm.c4) return;            // thread cq < c4 (row lane 0) merges its quad
#pragma unroll
    for (int j = 0; j < 4; ++j) t1[j] = t2[j] = 0.f;
    for (int rl = 0; rl < rm.lanes; ++rl)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        t1[j] += red[(rl * rm.c4 + cq) * 8 + j];
        t2[j] += red[(rl * rm.c4 + cq) * 8 + 4 + j];
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    part[((size_t)blockIdx.x * C + cq * 4 + j) * 2] = t1[j];
    part[((size_t)blockIdx.x * C + cq * 4 + j) * 2 + 1] = t2[j];
  }
}

// Gradient of a 3x3 / stride 2 / pad 1 max-pool at pixel m of [N][H][W], channels c..c+3: the sum over the <= 4 output windows
// that contain the pixel (rows, then columns, ascending) of dpool where the saved argmax code names this pixel.
__device__ __forceinline__ f32x4 pool_gather(const float* __restrict__ dpool, const unsigned char* __restrict__ idx, long long m,
                                             int c, int H, int W, int C, int Ho, int Wo) {
  const int iw = (int)(m % W);
  const long long t = m / W;
  const int ih = (int)(t % H), n = (int)(t / H);
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  for (int oh = ih / 2; oh <= (ih + 1) / 2; ++oh) {                            // 2*oh-1 <= ih <= 2*oh+1
    if (oh >= Ho) continue;
    const int dh = ih - (2 * oh - 1);
    for (int ow = iw / 2; ow <= (iw + 1) / 2; ++ow) {
      if (ow >= Wo) continue;
      const unsigned code = (unsigned)(dh * 3 + (iw - (2 * ow - 1)));
      const size_t o = ((size_t)(n * Ho + oh) * Wo + ow) * C + c;
      const unsigned id4 = *reinterpret_cast<const unsigned*>(idx + o);
      const f32x4 d = *reinterpret_cast<const f32x4*>(dpool + o);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (((id4 >> (8 * j)) & 0xff) == code) g[j] += d[j];
    }
  }
  return g;
}

// Where a BatchNorm backward pass takes dY [M][C] from: dense rows (dy; NULL = all zero), or, with idx set, the gradient dy of a
// 3x3/s2 max-pool over the [N][H][W][C] map and its argmax codes: dY is gathered, never materialised.  The kernels are
// instantiated for either kind (POOLED): the gather's registers would cost the dense rows occupancy, and the other way round.
struct DySrc {
  const float* dy;
  const unsigned char* idx;
  int H, W, Ho, Wo;
  __device__ __forceinline__ f32x4 dense(long long m, int c, int C) const {
    return dy ? *reinterpret_cast<const f32x4*>(dy + (size_t)m * C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ f32x4 gather(long long m, int c, int C) const { return pool_gather(dy, idx, m, c, H, W, C, Ho, Wo); }
};
