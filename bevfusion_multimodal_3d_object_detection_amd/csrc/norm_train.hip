// Train-mode BatchNorm on NHWC rows ([M][C], channel stride cs): batch statistics, apply (+residual, +ReLU),
// and the backward pair (per-channel reductions, then the element-wise input gradient).
//   forward : torch.nn.BatchNorm{1,2}d in training mode, as every conv/bn pair of ref src/encoders.py and
//             src/fusion.py runs under model.train() (ref src/train_detect.py:395-434)
// Reductions are two-stage and order-fixed (deterministic): fp32 partial sums per workgroup, merged in
// double.  Variance uses sums shifted by the first row (no catastrophic cancellation when |mean| >> std).
#include "bn_rows.h"

namespace {

constexpr int kStatGrid = 1024;

// partial[g][c] = {sum(x-s), sum((x-s)^2)} ; shift s[c] = x[0][c]
__global__ __launch_bounds__(256) void stats_partials(const float* __restrict__ x, float* __restrict__ part, int M, int C,
                                                       int cs) {
  const RowMap rm(C);
  BN_QUADS(cq, rm) {
    float a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
    if (!rm.idle()) {
      const f32x4 sh = *reinterpret_cast<const f32x4*>(x + cq * 4);
      f32x4 v[4];
      stream_rows(rm, M,
                  [&](long long m, int u) { v[u] = *reinterpret_cast<const f32x4*>(x + (size_t)m * cs + cq * 4); },
                  [&](long long, int u) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float d = v[u][j] - sh[j]; a1[j] += d; a2[j] = fmaf(d, d, a2[j]); }
                  });
    }
    write_partials(rm, cq, a1, a2, part, C);
  }
}

// merge of the G partial rows of one channel by one 256-thread workgroup: thread l takes g = l, l+256, ... (fixed order), a
// fixed xor tree merges the 64 lane totals of each wave, and the four wave totals are added in wave order through LDS.
// Every thread of the workgroup must call it; the result is valid in thread 0.
__device__ __forceinline__ void merge_partials(const float* __restrict__ part, int C, int G, int c, double& s1, double& s2) {
  __shared__ double wsum[4][2];
  s1 = 0; s2 = 0;
  if (c < C)
    for (int g = threadIdx.x; g < G; g += 256) { s1 += part[((size_t)g * C + c) * 2]; s2 += part[((size_t)g * C + c) * 2 + 1]; }
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) {
    s1 += __shfl_xor(s1, sft);
    s2 += __shfl_xor(s2, sft);
  }
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = s1; wsum[threadIdx.x >> 6][1] = s2; }
  __syncthreads();
  s1 = ((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0];
  s2 = ((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1];
}

// mean, biased var, invstd from the partials (double, fixed order)
__global__ __launch_bounds__(256) void stats_finalize(const float* __restrict__ x, const float* __restrict__ part,
                                                       float* __restrict__ mean, float* __restrict__ var,
                                                       float* __restrict__ invstd, int M, int C, int G, float eps) {
  const int c = blockIdx.x;
  double s1, s2;
  merge_partials(part, C, G, c, s1, s2);
  if (c >= C || threadIdx.x != 0) return;
  const double sh = x[c], d = s1 / M;
  const double v = s2 / M - d * d;
  mean[c] = (float)(sh + d);
  var[c] = (float)(v > 0 ? v : 0);
  invstd[c] = (float)(1.0 / sqrt((v > 0 ? v : 0) + (double)eps));
}

// y = act((x - mean) * invstd * gamma + beta (+ res)).  Thread (cq, rl) keeps channel quad cq for its whole life, so
// the per-channel scale/shift live in registers and the row loop is pure 16-byte streaming with 4 rows in flight.
__global__ __launch_bounds__(256) void bn_apply(const float* __restrict__ x, const float* __restrict__ mean,
                                                 const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ res,
                                                 float* __restrict__ y, long long M, int C, int cs, int relu) {
  const RowMap rm(C);
  if (rm.idle()) return;
  BN_QUADS(cq, rm) {
    const int c = cq * 4;
    const BnQuad q(mean, invstd, gamma, beta, c);
    // (written out, not through stream_rows: the tail reads res element by element behind x, which the shared load / use pair
    //  cannot express; where a thread has about one row -- 67 200 rows x 256 channels with a residual -- that form is 6 % faster)
    const long long step = rm.step;
    long long m = rm.first;
    for (; m + 3 * step < M; m += 4 * step) {
      f32x4 v[4], r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = *reinterpret_cast<const f32x4*>(x + (size_t)(m + u * step) * cs + c);
        if (res) r[u] = *reinterpret_cast<const f32x4*>(res + (size_t)(m + u * step) * C + c);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float t = q.pre(v[u][j], j);
          if (res) t += r[u][j];
          o[j] = relu ? fmaxf(t, 0.f) : t;
        }
        *reinterpret_cast<f32x4*>(y + (size_t)(m + u * step) * C + c) = o;
      }
    }
    for (; m < M; m += step) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)m * cs + c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = q.pre(v[j], j);
        if (res) t += res[(size_t)m * C + c + j];
        o[j] = relu ? fmaxf(t, 0.f) : t;
      }
      *reinterpret_cast<f32x4*>(y + (size_t)m * C + c) = o;
    }
  }
}

// backward stage 1: partial[g][c] = {sum dy, sum dy*xhat} of dy <- dy * (y > 0) when relu.  relu == 1: y is the forward output;
// relu >= 2: y is not read, the mask is recomputed from the raw input (BnQuad::mask) -- valid for layers without a residual
// input; the masked dy is written back to dy_out (the dense source's own rows) unless relu == 3: stage 2 then masks again.
// POOLED: relu mode 3 only (fixed at compile time, so the other modes cost it no registers); the gather runs in the use phase,
// behind the four rows of x in flight.
template <bool POOLED>
__global__ __launch_bounds__(256) void bn_bwd_partials(const DySrc src, float* dy_out, const float* __restrict__ y,
                                                        const float* __restrict__ x,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ part, long long M, int C, int cs, int relu) {
  if constexpr (POOLED) relu = 3;
  const RowMap rm(C);
  BN_QUADS(cq, rm) {
    float a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
    if (!rm.idle()) {
      const int c = cq * 4;
      const BnQuad q(mean, invstd, gamma, beta, c);
      f32x4 g[4], yy[4], xv[4];
      stream_rows(rm, M,
                  [&](long long m, int u) {             // 4 rows x up to 3 streams of 16-byte loads in flight
                    if constexpr (!POOLED) g[u] = src.dense(m, c, C);
                    if (relu == 1) yy[u] = *reinterpret_cast<const f32x4*>(y + (size_t)m * C + c);
                    if (x) xv[u] = *reinterpret_cast<const f32x4*>(x + (size_t)m * cs + c);
                  },
                  [&](long long m, int u) {
                    if constexpr (POOLED) g[u] = src.gather(m, c, C);
                    if (relu) {
                      if (relu >= 2) {
                        g[u] = q.mask(xv[u], g[u]);
                      } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) g[u][j] = yy[u][j] > 0.f ? g[u][j] : 0.f;
                      }
                      if (relu != 3) *reinterpret_cast<f32x4*>(dy_out + (size_t)m * C + c) = g[u];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                      a1[j] += g[u][j];
                      if (x) a2[j] = fmaf(g[u][j], (xv[u][j] - q.mu[j]) * q.is[j], a2[j]);
                    }
                  });
    }
    write_partials(rm, cq, a1, a2, part, C);
  }
}

__global__ __launch_bounds__(256) void sums_finalize(const float* __restrict__ part, float* __restrict__ s_dy,
                                                      float* __restrict__ s_dyx, int C, int G) {
  const int c = blockIdx.x;
  double s1, s2;
  merge_partials(part, C, G, c, s1, s2);
  if (c >= C || threadIdx.x != 0) return;
  s_dy[c] = (float)s1;
  if (s_dyx) s_dyx[c] = (float)s2;
}

// backward stage 2: dx = gamma*invstd * (dy - sum_dy/M - xhat * sum_dyx/M) = k1*dy + k2*x + k3 per channel (bn_dx).
// remask: dy arrives WITHOUT the ReLU mask -- stage 1 ran in mode 3, or dY is gathered -- and is masked here (BnQuad::mask).
// frozen: the layer normalised with FIXED statistics (eval-mode BatchNorm inside a training module): mean / invstd do not depend on
// x, so the two mean-subtraction terms vanish and dx = gamma * invstd * dy
// POOLED: always remask, never frozen, x as dense as dx (fixed at compile time); one row at a time and one quad pass (the host
// requires C/4 <= 256), the loop shape of the kernel this instantiation replaces: 8 waves per SIMD hide the gather.
template <bool POOLED>
__global__ __launch_bounds__(256) void bn_bwd_apply(const DySrc src, const float* __restrict__ x, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ s_dy,
                                                     const float* __restrict__ s_dyx, float* __restrict__ dx, long long M, int C,
                                                     int cs, int remask, int frozen) {
  if constexpr (POOLED) { remask = 1; frozen = 0; cs = C; }
  const RowMap rm(C);
  if (rm.idle()) return;
  const float invM = frozen ? 0.f : 1.f / (float)M;
  auto pass = [&](int cq) {
    const int c = cq * 4;
    const BnQuad q(mean, invstd, gamma, beta, c);
    float sd[4], sx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sd[j] = s_dy[c + j] * invM;
      sx[j] = s_dyx[c + j] * invM;
    }
    constexpr int DEPTH = POOLED ? 1 : 4;
    f32x4 g[DEPTH], xv[DEPTH];
    stream_rows<DEPTH>(rm, M,
                [&](long long m, int u) {
                  if constexpr (!POOLED) g[u] = src.dense(m, c, C);
                  xv[u] = *reinterpret_cast<const f32x4*>(x + (size_t)m * cs + c);
                },
                [&](long long m, int u) {
                  if constexpr (POOLED) g[u] = src.gather(m, c, C);
                  if (remask) g[u] = q.mask(xv[u], g[u]);
                  f32x4 o;
#pragma unroll
                  for (int j = 0; j < 4; ++j) o[j] = bn_dx(q.fa[j], g[u][j], sd[j], xv[u][j], q.mu[j], q.is[j], sx[j]);
                  *reinterpret_cast<f32x4*>(dx + (size_t)m * cs + c) = o;
                });
  };
  if constexpr (POOLED) pass(rm.cq0);
  else BN_QUADS(cq, rm) pass(cq);
}

// running statistics, as torch.nn.BatchNorm updates them in training mode (one launch instead of five tiny ones)
__global__ __launch_bounds__(256) void bn_update_running(const float* __restrict__ mean, const float* __restrict__ var,
                                                          float* __restrict__ rmean, float* __restrict__ rvar,
                                                          long long* __restrict__ nbt, int C, float keep, float mom, float mom_unbiased) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  rmean[c] = fmaf(mom, mean[c], rmean[c] * keep);
  rvar[c] = fmaf(mom_unbiased, var[c], rvar[c] * keep);
}

// ---- BatchNorm backward fed by a max over rows (PointNet's last layer) ---------------------------------------------------
// The gradient of y = relu(bn(x)) arriving from g[b][c] = max_n y[b][n][c] is non-zero in ONE row per (frame, channel).
// Instead of scattering it into a dense [M][C] tensor and reducing that again, the per-channel sums are gathered from
// the B*C non-zeros, the dense part of dx is written without reading any dy, and the B*C entries are added afterwards.
__global__ __launch_bounds__(256) void gmax_bn_sums(const float* __restrict__ dg, const float* __restrict__ gmax,
                                                     const int* __restrict__ idx, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     float* __restrict__ dgm, float* __restrict__ s_dy, float* __restrict__ s_dyx,
                                                     int B, int P, int C, int cs) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float mu = mean[c], is = invstd[c];
  double a1 = 0, a2 = 0;
  for (int b = 0; b < B; ++b) {
    const float g = gmax[(size_t)b * C + c] > 0.f ? dg[(size_t)b * C + c] : 0.f;      // ReLU: relu'(0) = 0, as torch
    dgm[(size_t)b * C + c] = g;
    const float xv = x[((size_t)b * P + idx[(size_t)b * C + c]) * cs + c];
    a1 += g;
    a2 += (double)g * ((xv - mu) * is);
  }
  s_dy[c] = (float)a1;
  s_dyx[c] = (float)a2;
}

__global__ __launch_bounds__(256) void gmax_bn_scatter(const float* __restrict__ dgm, const int* __restrict__ idx,
                                                        const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                        float* __restrict__ dx, int P, int C, int cs, long long total) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= total) return;
  const long long b = i / C;
  const int c = (int)(i - b * C);
  dx[((size_t)b * P + idx[i]) * cs + c] += (gamma ? gamma[c] : 1.f) * invstd[c] * dgm[i];
}

static inline unsigned partial_grid(long long M, int C) {  // workgroups of the *_partials kernels: one row per row lane, capped
  const long long g = (M + bn_row_lanes(C) - 1) / bn_row_lanes(C);
  return (unsigned)(g > kStatGrid ? kStatGrid : g);
}
static inline unsigned row_grid(long long M, int C) {      // workgroups of the other row-streaming kernels: four rows per row lane
  const long long g = (M + bn_row_lanes(C) * 4ll - 1) / (bn_row_lanes(C) * 4ll);
  return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}
constexpr size_t kPartialLds = 256 * 8 * sizeof(float);    // write_partials' `red`

// The launches of a BatchNorm backward: partial sums, their merge into dbeta / dgamma and, with dx, the input gradient.
// relu_mode as bn_bwd_partials takes it; dy_out: where it writes the masked dY back (the dense source's rows; NULL if POOLED).
template <bool POOLED>
static void launch_bn_backward(const DySrc src, float* dy_out, const float* y, const float* x, const float* mean,
                               const float* invstd, const float* gamma, const float* beta, float* work, float* dgamma,
                               float* dbeta, float* dx, long long M, int C, int cs, int relu_mode, int frozen, hipStream_t st) {
  const unsigned G = partial_grid(M, C);
  hipLaunchKernelGGL(bn_bwd_partials<POOLED>, dim3(G), dim3(256), kPartialLds, st, src, dy_out, y, x, mean, invstd, gamma, beta,
                     work, M, C, cs, relu_mode);
  hipLaunchKernelGGL(sums_finalize, dim3(C), dim3(256), 0, st, work, dbeta, dgamma, C, (int)G);
  if (dx)
    hipLaunchKernelGGL(bn_bwd_apply<POOLED>, dim3(row_grid(M, C)), dim3(256), 0, st, src, x, mean, invstd, gamma, beta, dbeta,
                       dgamma, dx, M, C, cs, relu_mode == 3 ? 1 : 0, frozen);
}

}  // namespace

extern "C" size_t bevf_bn_work_floats(int C) { return (size_t)kStatGrid * C * 2; }

extern "C" int bevf_bn_stats_f32(const float* x, float* work, float* mean, float* var, float* invstd, int M, int C,
                                 int cs, float eps, void* stream) {
  BEVF_REQUIRE(x && work && mean && var && invstd, "bn_stats: null pointer");
  BEVF_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && cs >= C && cs % 4 == 0, "bn_stats: bad shape (M=%d C=%d cs=%d)", M, C, cs);
  BEVF_REQUIRE(bevf_aligned16(x), "bn_stats: unaligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned G = partial_grid(M, C);
  hipLaunchKernelGGL(stats_partials, dim3(G), dim3(256), kPartialLds, st, x, work, M, C, cs);
  hipLaunchKernelGGL(stats_finalize, dim3(C), dim3(256), 0, st, x, work, mean, var, invstd, M, C, (int)G, eps);
  return bevf_check_launch("bevf_bn_stats_f32");
}

// Batch statistics from partial sums a producer left behind (bevf_conv3x3_wino_f32 with `stats`): part [G][C][2] =
// {sum(x - pivot), sum((x - pivot)^2)} over disjoint row sets covering all M rows.  Same fixed-order double merge as above.
extern "C" int bevf_bn_stats_from_partials_f32(const float* part, int G, const float* pivot, float* mean, float* var,
                                               float* invstd, int M, int C, float eps, void* stream) {
  BEVF_REQUIRE(part && pivot && mean && var && invstd && G > 0 && M > 0 && C > 0, "bn_stats_from_partials: bad arguments");
  hipLaunchKernelGGL(stats_finalize, dim3(C), dim3(256), 0, static_cast<hipStream_t>(stream), pivot, part, mean, var,
                     invstd, M, C, G, eps);
  return bevf_check_launch("bevf_bn_stats_from_partials_f32");
}

extern "C" int bevf_bn_update_running_f32(const float* mean, const float* var, float* running_mean, float* running_var,
                                          int64_t* num_batches_tracked, int C, int M, float momentum, void* stream) {
  BEVF_REQUIRE(mean && var && running_mean && running_var && C > 0 && M > 0, "bn_update_running: bad arguments");
  const float unbias = M > 1 ? (float)((double)M / (double)(M - 1)) : 1.f;
  hipLaunchKernelGGL(bn_update_running, dim3((C + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), mean, var,
                     running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), C, 1.f - momentum, momentum,
                     momentum * unbias);
  return bevf_check_launch("bevf_bn_update_running_f32");
}

extern "C" int bevf_bn_apply_f32(const float* x, const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, const float* res, float* y, int M, int C, int cs, int relu,
                                 void* stream) {
  BEVF_REQUIRE(x && mean && invstd && y, "bn_apply: null pointer");
  BEVF_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && cs >= C && cs % 4 == 0, "bn_apply: bad shape");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(y) && (!res || bevf_aligned16(res)), "bn_apply: unaligned");
  hipLaunchKernelGGL(bn_apply, dim3(row_grid(M, C)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                     mean, invstd, gamma, beta, res, y, (long long)M, C, cs, relu);
  return bevf_check_launch("bevf_bn_apply_f32");
}

extern "C" int bevf_bn_backward_f32(float* dy, const float* y, const float* x, const float* mean, const float* invstd,
                                    const float* gamma, const float* beta, float* work, float* dgamma, float* dbeta,
                                    float* dx, int M, int C, int cs, int relu, void* stream) {
  BEVF_REQUIRE(dy && work && dbeta, "bn_backward: null pointer");
  BEVF_REQUIRE(!relu || y || (x && mean && invstd), "bn_backward: relu needs the forward output, or x/mean/invstd to recompute it");
  BEVF_REQUIRE(!dx || (x && mean && invstd && dgamma), "bn_backward: dx needs x, mean, invstd, dgamma");
  BEVF_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && cs >= C && cs % 4 == 0, "bn_backward: bad shape");
  // y == NULL: mask recomputed from x (no residual in the forward); relu == 2: additionally dy is left untouched (nobody reads the
  // masked gradient of a layer without a skip connection) and the second pass masks again: one write of dy less.
  // relu | 4: frozen statistics (mean / invstd are constants, e.g. the running buffers of an eval-mode layer): dx = gamma invstd dy
  const int frozen = (relu & 4) ? 1 : 0;
  relu &= 3;
  BEVF_REQUIRE(relu != 2 || (!y && x && mean && invstd), "bn_backward: relu = 2 recomputes the mask from x (y must be NULL)");
  const int relu_mode = relu ? (y ? 1 : (relu == 2 ? 3 : 2)) : 0;
  launch_bn_backward<false>(DySrc{dy}, dy, y, x, mean, invstd, gamma, beta, work, dgamma, dbeta, dx, M, C, cs, relu_mode, frozen,
                            static_cast<hipStream_t>(stream));
  return bevf_check_launch("bevf_bn_backward_f32");
}

extern "C" int bevf_bn_backward_from_partials_f32(const float* dy, const float* x, const float* mean, const float* invstd,
                                                  const float* gamma, const float* part, int G, float* dgamma, float* dbeta,
                                                  float* dx, int M, int C, int cs, void* stream) {
  BEVF_REQUIRE(dy && x && mean && invstd && part && dgamma && dbeta, "bn_backward_from_partials: null pointer");
  BEVF_REQUIRE(G > 0 && M > 0 && C > 0 && C % 4 == 0 && cs >= C && cs % 4 == 0, "bn_backward_from_partials: bad shape");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sums_finalize, dim3(C), dim3(256), 0, st, part, dbeta, dgamma, C, G);
  if (dx)
    hipLaunchKernelGGL(bn_bwd_apply<false>, dim3(row_grid(M, C)), dim3(256), 0, st, DySrc{dy}, x, mean, invstd, gamma,
                       (const float*)nullptr, dbeta, dgamma, dx, (long long)M, C, cs, 0, 0);
  return bevf_check_launch("bevf_bn_backward_from_partials_f32");
}

// BatchNorm(+ReLU) backward whose dY comes out of a 3x3/s2/p1 max-pool backward (the ResNet stem, ref src/encoders.py:154-157 in
// training): dpool [N][Ho][Wo][C] gradient of the pooled map, idx the argmax codes of bevf_maxpool3x3s2_idx_f32, x the raw conv
// output [N][H][W][C].  The dense dY is never materialised: both passes gather it with maxpool_bwd's own pool_gather and recompute
// the ReLU mask from x (relu mode 3), so sums and dx are bit-identical to bevf_maxpool3x3s2_bwd_f32 followed by
// bevf_bn_backward_f32(relu = 1, y = NULL).  Traffic at 48 images of 448x800: 9.2 GB -> 4 GB.
extern "C" int bevf_pool_bn_backward_f32(const float* dpool, const uint8_t* idx, const float* x, const float* mean,
                                         const float* invstd, const float* gamma, const float* beta, float* work, float* dgamma,
                                         float* dbeta, float* dx, int N, int H, int W, int C, void* stream) {
  BEVF_REQUIRE(dpool && idx && x && mean && invstd && work && dgamma && dbeta && dx, "pool_bn_backward: null pointer");
  BEVF_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0,
               "pool_bn_backward: C=%d must be a multiple of 4 with 256 %% (C/4) == 0", C);
  BEVF_REQUIRE(bevf_aligned16(dpool) && bevf_aligned16(x) && bevf_aligned16(dx), "pool_bn_backward: unaligned");
  const long long M = (long long)N * H * W;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  launch_bn_backward<true>(DySrc{dpool, idx, H, W, Ho, Wo}, nullptr, nullptr, x, mean, invstd, gamma, beta, work, dgamma, dbeta, dx,
                           M, C, C, 3, 0, static_cast<hipStream_t>(stream));
  return bevf_check_launch("bevf_pool_bn_backward_f32");
}

// The first stage of bevf_gmax_bn_backward_f32 alone: dgm [B][C] = dg masked by the ReLU, dbeta = sum dgm, dgamma = sum dgm * xhat
// (gathered from the B argmax rows per channel).  For callers that never build the dense dx (training.py: the low-rank form of
// PointNet's last layer).
extern "C" int bevf_gmax_bn_sums_f32(const float* dg, const float* gmax, const int32_t* idx, const float* x, const float* mean,
                                     const float* invstd, float* dgm, float* dgamma, float* dbeta, int B, int P, int C, int cs,
                                     void* stream) {
  BEVF_REQUIRE(dg && gmax && idx && x && mean && invstd && dgm && dgamma && dbeta, "gmax_bn_sums: null pointer");
  BEVF_REQUIRE(B > 0 && P > 0 && C > 0 && cs >= C, "gmax_bn_sums: bad shape");
  BEVF_REQUIRE((long long)B * P < (1ll << 31), "gmax_bn_sums: too many rows");
  hipLaunchKernelGGL(gmax_bn_sums, dim3((C + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), dg, gmax, idx, x, mean,
                     invstd, dgm, dbeta, dgamma, B, P, C, cs);
  return bevf_check_launch("bevf_gmax_bn_sums_f32");
}

// Backward of y = relu(batchnorm(x)) followed by a max over the P rows of each of B groups (ref src/encoders.py:296-299
// in training mode): dg [B][C] gradient of the max, gmax its forward value, idx its argmax row.  Writes dgamma, dbeta and
// the dense dx [B*P][cs]; dgm [B][C] is scratch.  Equivalent to group_max_bwd + bn_backward without the dense dy.
extern "C" int bevf_gmax_bn_backward_f32(const float* dg, const float* gmax, const int32_t* idx, const float* x,
                                         const float* mean, const float* invstd, const float* gamma, float* dgm,
                                         float* dgamma, float* dbeta, float* dx, int B, int P, int C, int cs, void* stream) {
  BEVF_REQUIRE(dg && gmax && idx && x && mean && invstd && dgm && dgamma && dbeta && dx, "gmax_bn_backward: null pointer");
  BEVF_REQUIRE(B > 0 && P > 0 && C > 0 && C % 4 == 0 && cs >= C && cs % 4 == 0, "gmax_bn_backward: bad shape");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long M = (long long)B * P;
  BEVF_REQUIRE(M < (1ll << 31), "gmax_bn_backward: too many rows");
  hipLaunchKernelGGL(gmax_bn_sums, dim3((C + 255) / 256), dim3(256), 0, st, dg, gmax, idx, x, mean, invstd, dgm, dbeta, dgamma,
                     B, P, C, cs);
  hipLaunchKernelGGL(bn_bwd_apply<false>, dim3(row_grid(M, C)), dim3(256), 0, st, DySrc{}, x, mean, invstd, gamma,
                     (const float*)nullptr, dbeta, dgamma, dx, M, C, cs, 0, 0);
  const long long total = (long long)B * C;
  hipLaunchKernelGGL(gmax_bn_scatter, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dgm, idx, gamma, invstd, dx, P, C,
                     cs, total);
  return bevf_check_launch("bevf_gmax_bn_backward_f32");
}
