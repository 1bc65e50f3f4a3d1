// Row kernels of the sparse-voxel LiDAR encoder: the mean VFE, BatchNorm over the active rows with the row
// count on the device, and the canvas write / its backward.  Rows are `cap` slots per frame, active while slot < count[b]; every
// grid is sized by capacity (or is a fixed reduction grid) and nothing is read back to the host.  Reductions are fp64 partials
// summed in a fixed order (like pillar_moments): no atomics, two launches give identical bits.  The BatchNorm forward value, the
// ReLU mask and dx are bn_rows.h's BnQuad::relu_pre / mask / bn_dx: the formulas the rest of the tree uses.
#include "bn_rows.h"

namespace {

constexpr int NWG = 256;                 // workgroups of the reduction kernels = partial rows
constexpr int BN_SLAB = 128;             // channels the BatchNorm reductions take at a time
constexpr int BN_MAX_C = 1024;

__device__ __forceinline__ bool slot_active(const int32_t* __restrict__ count, int cap, long long row, int& b) {
  b = (int)(row / cap);
  const int n = count[b];
  return (int)(row - (long long)b * cap) < (n < cap ? n : cap);
}

// x[row][c] = mean over the voxel's kept points of channel c (fp32 sum in point order, one division), 0 for C <= c < Cpad
__global__ __launch_bounds__(256) void sp_vfe_mean(const float* __restrict__ feats, const int32_t* __restrict__ npts,
                                                   const int32_t* __restrict__ nvox, int B, int Nv, int P, int C, int Cpad,
                                                   float* __restrict__ x) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * Nv * Cpad) return;
  const long long row = i / Cpad;
  const int c = (int)(i - row * Cpad);
  int b;
  if (!slot_active(nvox, Nv, row, b)) return;
  float v = 0.f;
  if (c < C) {
    int n = npts[row];
    n = n < 0 ? 0 : (n > P ? P : n);
    const float* f = feats + (size_t)row * P * C + c;
    float s = 0.f;
    for (int p = 0; p < n; ++p) s += f[(size_t)p * C];
    v = n > 0 ? s / (float)n : 0.f;
  }
  x[i] = v;
}

// canvas[b][y][x][z * C + c] = rows[row][c] at the row's cell (z, y, x) of (D, H, W); the caller's memset leaves the rest 0
template <typename T>
__global__ __launch_bounds__(256) void sp_canvas(const float* __restrict__ rows, const int32_t* __restrict__ cell,
                                                 const int32_t* __restrict__ count, int B, int cap, int D, int H, int W, int C,
                                                 T* __restrict__ canvas) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * cap * C) return;
  const long long row = i / C;
  const int c = (int)(i - row * C);
  int b;
  if (!slot_active(count, cap, row, b)) return;
  const int cl = cell[row];
  if (cl < 0 || cl >= D * H * W) return;
  const int z = cl / (H * W), yx = cl - z * (H * W);
  canvas[((size_t)b * H * W + yx) * ((size_t)D * C) + (size_t)z * C + c] = (T)rows[i];
}

// the gather that is sp_canvas's backward: drows[row][c] = dcanvas at the row's cell
__global__ __launch_bounds__(256) void sp_canvas_bwd(const float* __restrict__ dcanvas, const int32_t* __restrict__ cell,
                                                     const int32_t* __restrict__ count, int B, int cap, int D, int H, int W, int C,
                                                     float* __restrict__ drows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * cap * C) return;
  const long long row = i / C;
  const int c = (int)(i - row * C);
  int b;
  if (!slot_active(count, cap, row, b)) return;
  const int cl = cell[row];
  float g = 0.f;
  if (cl >= 0 && cl < D * H * W) {
    const int z = cl / (H * W), yx = cl - z * (H * W);
    g = dcanvas[((size_t)b * H * W + yx) * ((size_t)D * C) + (size_t)z * C + c];
  }
  drows[i] = g;
}

// Two fp64 sums per channel over the active rows.  Thread = (channel c = tid % C, row lane rl = tid / C of 256 / C); workgroup g
// takes slots g * lanes + rl, + NWG * lanes, ... of every frame in frame order; the row lanes are then added in lane order.
//   MODE 0  (sum y, sum y^2): the batch statistics
//   MODE 1  (sum g, sum g x_hat) with g = da through the recomputed ReLU mask: the BatchNorm backward's two sums
// One slab of Cs <= 128 channels starting at channel cb of rows that are Cr channels wide (Cs = Cr, cb = 0 up to 128 channels).
template <int MODE>
__device__ __forceinline__ void sp_bn_sums_slab(const float* __restrict__ y, const float* __restrict__ da,
                                                const int32_t* __restrict__ count, int B, int cap, int Cr, int cb, int C,
                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                double* __restrict__ part, double* red) {
  const int tid = threadIdx.x, lanes = 256 / C, c = tid % C, rl = tid / C;
  y += cb, part += (size_t)cb * 2;
  if (MODE == 1) da += cb, mean += cb, invstd += cb, gamma = gamma ? gamma + cb : gamma, beta = beta ? beta + cb : beta;
  double s1 = 0.0, s2 = 0.0;
  if (rl < lanes) {
    float mu = 0.f, is = 1.f, fa = 1.f, fb = 0.f;
    if (MODE == 1) {
      mu = mean[c];
      is = invstd[c];
      fa = (gamma ? gamma[c] : 1.f) * is;
      fb = fmaf(-mu, fa, beta ? beta[c] : 0.f);                       // BnQuad's constants for one channel
    }
    for (int b = 0; b < B; ++b) {
      const int n = count[b] < cap ? count[b] : cap;
      for (int v = blockIdx.x * lanes + rl; v < n; v += NWG * lanes) {
        const size_t o = ((size_t)b * cap + v) * Cr + c;
        const float yv = y[o];
        if (MODE == 0) {
          s1 += (double)yv;
          s2 += (double)yv * (double)yv;
        } else {
          const float g = fmaf(yv, fa, fb) > 0.f ? da[o] : 0.f;        // BnQuad::mask
          s1 += (double)g;
          s2 += (double)g * (double)((yv - mu) * is);
        }
      }
    }
  }
  red[tid * 2] = s1;
  red[tid * 2 + 1] = s2;
  __syncthreads();
  if (tid < C) {
    double t1 = 0.0, t2 = 0.0;
    for (int l = 0; l < lanes; ++l) {
      t1 += red[(l * C + tid) * 2];
      t2 += red[(l * C + tid) * 2 + 1];
    }
    part[((size_t)blockIdx.x * Cr + tid) * 2] = t1;
    part[((size_t)blockIdx.x * Cr + tid) * 2 + 1] = t2;
  }
}

// Rows wider than 128 channels (the RoI head's MLP) go slab by slab; up to 128 it is the one slab it always was.
template <int MODE>
__global__ __launch_bounds__(256) void sp_bn_sums(const float* __restrict__ y, const float* __restrict__ da,
                                                  const int32_t* __restrict__ count, int B, int cap, int C,
                                                  const float* __restrict__ mean, const float* __restrict__ invstd,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  double* __restrict__ part) {
  __shared__ double red[256 * 2];
  for (int cb = 0; cb < C; cb += BN_SLAB) {
    if (cb) __syncthreads();   // (red is reused)
    sp_bn_sums_slab<MODE>(y, da, count, B, cap, C, cb, C - cb < BN_SLAB ? C - cb : BN_SLAB, mean, invstd, gamma, beta, part, red);
  }
}

// partials -> mean, invstd (biased variance + eps); running buffers as nn.BatchNorm1d moves them (momentum, unbiased variance;
// momentum < 0 = cumulative average); num_batches_tracked + 1.  nrows_out[0] = the active rows (the host's "fewer than two rows" refusal)
__global__ __launch_bounds__(128) void sp_bn_stats_finish(const double* __restrict__ part, const int32_t* __restrict__ count, int B, int cap,
                                                          int C, float eps, float momentum, float* rmean, float* rvar, long long* nbt,
                                                          float* __restrict__ mean, float* __restrict__ invstd,
                                                          int32_t* __restrict__ nrows_out) {
  long long N = 0;
  for (int b = 0; b < B; ++b) N += count[b] < cap ? count[b] : cap;
  const long long nb_old = nbt ? *nbt : 0;
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += BN_SLAB) {
    double s1 = 0.0, s2 = 0.0;
    for (int g = 0; g < NWG; ++g) {
      s1 += part[((size_t)g * C + c) * 2];
      s2 += part[((size_t)g * C + c) * 2 + 1];
    }
    const double inv = N > 0 ? 1.0 / (double)N : 0.0;
    const double m = s1 * inv;
    double var = s2 * inv - m * m;
    var = var > 0.0 ? var : 0.0;
    mean[c] = (float)m;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rmean && rvar && N > 1) {
      const double mo = momentum >= 0.f ? (double)momentum : 1.0 / (double)(nb_old + 1);
      rmean[c] = (float)((1.0 - mo) * (double)rmean[c] + mo * m);
      rvar[c] = (float)((1.0 - mo) * (double)rvar[c] + mo * var * (double)N / (double)(N - 1));
    }
  }
  if (threadIdx.x == 0) {
    if (nbt && N > 1) *nbt = nb_old + 1;
    if (nrows_out) *nrows_out = (int32_t)(N < 0x7fffffff ? N : 0x7fffffff);
  }
}

// a = relu(batchnorm(y)) on the active rows, a channel quad per thread
__global__ __launch_bounds__(256) void sp_bn_apply(const float* __restrict__ y, const int32_t* __restrict__ count, int B, int cap, int C,
                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ a) {
  const int c4 = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * cap * c4) return;
  const long long row = i / c4;
  const int c = (int)(i - row * c4) * 4;
  int b;
  if (!slot_active(count, cap, row, b)) return;
  const BnQuad q(mean, invstd, gamma, beta, c);
  const f32x4 v = *reinterpret_cast<const f32x4*>(y + (size_t)row * C + c);
  *reinterpret_cast<f32x4*>(a + (size_t)row * C + c) = q.relu_pre(v);
}

// the backward's sums -> dgamma = sum g x_hat, dbeta = sum g, and sd = sum g / M, sx = sum g x_hat / M for the dx pass
__global__ __launch_bounds__(128) void sp_bn_bwd_finish(const double* __restrict__ part, const int32_t* __restrict__ count, int B, int cap,
                                                        int C, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                        float* __restrict__ sd, float* __restrict__ sx) {
  long long N = 0;
  for (int b = 0; b < B; ++b) N += count[b] < cap ? count[b] : cap;
  for (int c = threadIdx.x; c < C; c += BN_SLAB) {
    double s1 = 0.0, s2 = 0.0;
    for (int g = 0; g < NWG; ++g) {
      s1 += part[((size_t)g * C + c) * 2];
      s2 += part[((size_t)g * C + c) * 2 + 1];
    }
    const double inv = N > 0 ? 1.0 / (double)N : 0.0;
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
    sd[c] = (float)(s1 * inv);
    sx[c] = (float)(s2 * inv);
  }
}

// dy = gamma invstd (g - sd - x_hat sx) (bn_dx), or gamma invstd g when the statistics are frozen
__global__ __launch_bounds__(256) void sp_bn_bwd_apply(const float* __restrict__ y, const float* __restrict__ da,
                                                       const int32_t* __restrict__ count, int B, int cap, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ sd, const float* __restrict__ sx, int frozen,
                                                       float* __restrict__ dy) {
  const int c4 = C >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * cap * c4) return;
  const long long row = i / c4;
  const int c = (int)(i - row * c4) * 4;
  int b;
  if (!slot_active(count, cap, row, b)) return;
  const BnQuad q(mean, invstd, gamma, beta, c);
  const f32x4 yv = *reinterpret_cast<const f32x4*>(y + (size_t)row * C + c);
  const f32x4 g = q.mask(yv, *reinterpret_cast<const f32x4*>(da + (size_t)row * C + c));
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = frozen ? q.fa[j] * g[j] : bn_dx(q.fa[j], g[j], sd[c + j], yv[j], q.mu[j], q.is[j], sx[c + j]);
  *reinterpret_cast<f32x4*>(dy + (size_t)row * C + c) = o;
}

int rows_check(const char* who, int B, int cap, int C, int max_c = 128) {
  BEVF_REQUIRE(B > 0 && cap > 0, "%s: empty shape", who);
  BEVF_REQUIRE(C > 0 && C <= max_c && C % 32 == 0, "%s: C=%d must be a multiple of 32 up to %d", who, C, max_c);
  BEVF_REQUIRE((long long)B * cap * C < (1ll << 31), "%s: B * capacity * C does not fit int32", who);
  return BEVF_OK;
}

unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

double* aligned_part(void* work) { return reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work) + 255) & ~uintptr_t(255)); }

}  // namespace

extern "C" int bevf_sparse_vfe_mean_f32(const float* feats, const int32_t* num_points, const int32_t* num_voxels, int B, int Nv, int P,
                                        int C, int Cpad, float* rows, void* stream) {
  if (int rc = rows_check("sparse_vfe_mean", B, Nv, Cpad)) return rc;
  BEVF_REQUIRE(feats && num_points && num_voxels && rows, "sparse_vfe_mean: null pointer");
  BEVF_REQUIRE(P > 0 && C >= 3 && C <= Cpad && (long long)B * Nv * P * C < (1ll << 40), "sparse_vfe_mean: need P > 0 and 3 <= C <= Cpad");
  hipLaunchKernelGGL(sp_vfe_mean, dim3(blocks_for((long long)B * Nv * Cpad)), dim3(256), 0, static_cast<hipStream_t>(stream), feats,
                     num_points, num_voxels, B, Nv, P, C, Cpad, rows);
  return bevf_check_launch("bevf_sparse_vfe_mean_f32");
}

extern "C" int bevf_sparse_canvas_f32(const float* rows, const int32_t* cell, const int32_t* count, int B, int cap, int D, int H, int W,
                                      int C, void* canvas, int canvas_bf16, void* stream) {
  if (int rc = rows_check("sparse_canvas", B, cap, C)) return rc;
  BEVF_REQUIRE(rows && cell && count && canvas, "sparse_canvas: null pointer");
  BEVF_REQUIRE(D > 0 && H > 0 && W > 0 && (long long)B * D * H * W * C < (1ll << 31), "sparse_canvas: canvas too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(canvas, 0, (size_t)B * D * H * W * C * (canvas_bf16 ? 2 : 4), st) != hipSuccess) {     // inactive cells are exactly 0
    bevf_set_error("sparse_canvas: memset failed");
    return BEVF_ERR_LAUNCH;
  }
  const dim3 grid(blocks_for((long long)B * cap * C));
  if (canvas_bf16)
    hipLaunchKernelGGL(sp_canvas<__bf16>, grid, dim3(256), 0, st, rows, cell, count, B, cap, D, H, W, C, static_cast<__bf16*>(canvas));
  else
    hipLaunchKernelGGL(sp_canvas<float>, grid, dim3(256), 0, st, rows, cell, count, B, cap, D, H, W, C, static_cast<float*>(canvas));
  return bevf_check_launch("bevf_sparse_canvas_f32");
}

extern "C" int bevf_sparse_canvas_bwd_f32(const float* dcanvas, const int32_t* cell, const int32_t* count, int B, int cap, int D, int H,
                                          int W, int C, float* drows, void* stream) {
  if (int rc = rows_check("sparse_canvas_bwd", B, cap, C)) return rc;
  BEVF_REQUIRE(dcanvas && cell && count && drows, "sparse_canvas_bwd: null pointer");
  BEVF_REQUIRE(D > 0 && H > 0 && W > 0 && (long long)B * D * H * W * C < (1ll << 31), "sparse_canvas_bwd: canvas too large");
  hipLaunchKernelGGL(sp_canvas_bwd, dim3(blocks_for((long long)B * cap * C)), dim3(256), 0, static_cast<hipStream_t>(stream), dcanvas, cell,
                     count, B, cap, D, H, W, C, drows);
  return bevf_check_launch("bevf_sparse_canvas_bwd_f32");
}

extern "C" size_t bevf_sparse_bn_work_bytes(int C) { return (size_t)NWG * C * 2 * sizeof(double) + 256; }

extern "C" int bevf_sparse_bn_stats_f32(const float* y, const int32_t* count, int B, int cap, int C, float eps, float momentum,
                                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                                        float* invstd, int32_t* nrows, void* work, void* stream) {
  if (int rc = rows_check("sparse_bn_stats", B, cap, C, BN_MAX_C)) return rc;
  BEVF_REQUIRE(y && count && mean && invstd && work, "sparse_bn_stats: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = aligned_part(work);
  hipLaunchKernelGGL(sp_bn_sums<0>, dim3(NWG), dim3(256), 0, st, y, (const float*)nullptr, count, B, cap, C, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, part);
  hipLaunchKernelGGL(sp_bn_stats_finish, dim3(1), dim3(128), 0, st, part, count, B, cap, C, eps, momentum, running_mean, running_var,
                     reinterpret_cast<long long*>(num_batches_tracked), mean, invstd, nrows);
  return bevf_check_launch("bevf_sparse_bn_stats_f32");
}

extern "C" int bevf_sparse_bn_apply_f32(const float* y, const int32_t* count, int B, int cap, int C, const float* mean, const float* invstd,
                                        const float* gamma, const float* beta, float* a, void* stream) {
  if (int rc = rows_check("sparse_bn_apply", B, cap, C, BN_MAX_C)) return rc;
  BEVF_REQUIRE(y && count && mean && invstd && a, "sparse_bn_apply: null pointer");
  BEVF_REQUIRE(bevf_aligned16(y) && bevf_aligned16(a), "sparse_bn_apply: y / a must be 16-byte aligned");
  hipLaunchKernelGGL(sp_bn_apply, dim3(blocks_for((long long)B * cap * (C / 4))), dim3(256), 0, static_cast<hipStream_t>(stream), y, count,
                     B, cap, C, mean, invstd, gamma, beta, a);
  return bevf_check_launch("bevf_sparse_bn_apply_f32");
}

extern "C" int bevf_sparse_bn_backward_f32(const float* y, const float* da, const int32_t* count, int B, int cap, int C, const float* mean,
                                           const float* invstd, const float* gamma, const float* beta, int frozen, float* dy,
                                           float* dgamma, float* dbeta, float* sums, void* work, void* stream) {
  if (int rc = rows_check("sparse_bn_backward", B, cap, C, BN_MAX_C)) return rc;
  BEVF_REQUIRE(y && da && count && mean && invstd && dy && dgamma && dbeta && sums && work, "sparse_bn_backward: null pointer");
  BEVF_REQUIRE(bevf_aligned16(y) && bevf_aligned16(da) && bevf_aligned16(dy), "sparse_bn_backward: y / da / dy must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = aligned_part(work);
  hipLaunchKernelGGL(sp_bn_sums<1>, dim3(NWG), dim3(256), 0, st, y, da, count, B, cap, C, mean, invstd, gamma, beta, part);
  hipLaunchKernelGGL(sp_bn_bwd_finish, dim3(1), dim3(128), 0, st, part, count, B, cap, C, dgamma, dbeta, sums, sums + C);
  hipLaunchKernelGGL(sp_bn_bwd_apply, dim3(blocks_for((long long)B * cap * (C / 4))), dim3(256), 0, st, y, da, count, B, cap, C, mean,
                     invstd, gamma, beta, sums, sums + C, frozen, dy);
  return bevf_check_launch("bevf_sparse_bn_backward_f32");
}
