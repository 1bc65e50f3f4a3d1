// Ego-motion warp of an NHWC BEV map (temporal fusion): the previous frame's map resampled onto the current
// frame's grid through a per-frame planar affine map, and the transposed resample for training.  What is particular to the warp is
// here -- the affine sample (warp_sample), the backward's candidate box, the checks; the stages it shares with the seg head's grid
// resample are in bev_resample.h.
//   bevf_bev_warp_{f32,bf16}   one wave per four output cells: the sample point and its four corner rows are wave-uniform (computed in
//                              fp64 from the device-side ego matrix, so a captured graph takes the matrix as an input), lanes walk the
//                              channels four at a time (16 bytes fp32, 8 bytes bf16).  Every output row is written, zeros included.
//   bevf_bev_warp_bwd_f32      a pull, no atomics: one wave per SOURCE cell collects the targets whose sample point lies within one
//                              cell of it -- candidates from the bounding box of the inverse affine image, weights recomputed with the
//                              forward's own expression (warp_sample), accumulated in row-major target order.
// HBM-bound: no LDS, no atomics.
#include "bev_resample.h"

namespace {

constexpr int Q = 4;                // channels per lane and step

struct WarpGeom {
  double x0, y0, vx, vy;
  int H, W;
};

// The sample of target cell (row i, column j) under M = ego[b] (row-major 4 x 4; rows 0-1, columns 0, 1, 3 are read).
__device__ __forceinline__ CornerSample warp_sample(const double* __restrict__ M, const WarpGeom& g, int i, int j) {
#pragma clang fp contract(off)
  const double xc = g.x0 + ((double)j + 0.5) * g.vx, yc = g.y0 + ((double)i + 0.5) * g.vy;
  const double xp = M[0] * xc + M[1] * yc + M[3], yp = M[4] * xc + M[5] * yc + M[7];
  const double qj = (xp - g.x0) / g.vx - 0.5, qi = (yp - g.y0) / g.vy - 0.5;
  CornerSample s;
  s.ok = qj > -1.0 && qj < (double)g.W && qi > -1.0 && qi < (double)g.H;  // (false for NaN and infinities)
  s.i0 = s.j0 = 0;
  s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
  if (s.ok) {
    const double fj0 = floor(qj), fi0 = floor(qi);
    s.j0 = (int)fj0, s.i0 = (int)fi0;
    corner_weights(qi - fi0, qj - fj0, s.w);
  }
  return s;
}

// (wave-uniform) cell index of this wave -> (b, i, j); false past the end
__device__ __forceinline__ bool wave_cell(int cells, const WarpGeom& g, int& b, int& i, int& j) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = xcd_remap((int)blockIdx.x, (int)gridDim.x) * CELLS_PER_BLOCK + wave;
  if (r >= cells) return false;
  const int P = g.H * g.W;
  b = r / P;
  const int p = r - b * P;
  i = p / g.W;
  j = p - i * g.W;
  return true;
}

template <typename T>
__global__ __launch_bounds__(256) void bev_warp(const T* __restrict__ x, T* __restrict__ y, const double* __restrict__ ego,
                                                 WarpGeom g, int cells, int C, int x_cs, int y_cs) {
  const int P = g.H * g.W;
  resample_forward<T, Q, false, false>(x, y, cells, P, g.H, g.W, C, x_cs, y_cs, [&](int r) {
    const int b = r / P, i = (r - b * P) / g.W;
    return warp_sample(ego + (size_t)b * 16, g, i, r - b * P - i * g.W);
  });
}

// dx[b][u][v][:] = sum over targets (i, j), row-major, of w(i, j -> u, v) * dy[b][i][j][:].
__global__ __launch_bounds__(256) void bev_warp_bwd(const float* __restrict__ dy, float* __restrict__ dx,
                                                     const double* __restrict__ ego, WarpGeom g, int cells, int C, int dy_cs) {
  int b, u, v;
  if (!wave_cell(cells, g, b, u, v)) return;
  const int lane = (int)(threadIdx.x & 63);
  const double* M = ego + (size_t)b * 16;
  // index space: q = A p + t with p = (j, i), q = (qj, qi); the candidates are the integer points of the bounding box, widened by
  // one, of A^-1 ([v-1, v+1] x [u-1, u+1] - t), clamped to the map (so the loops are bounded whatever M holds)
  const double a00 = M[0], a01 = M[1] * g.vy / g.vx, a10 = M[4] * g.vx / g.vy, a11 = M[5];
  const double xc0 = g.x0 + 0.5 * g.vx, yc0 = g.y0 + 0.5 * g.vy;
  const double t0 = (M[0] * xc0 + M[1] * yc0 + M[3] - g.x0) / g.vx - 0.5, t1 = (M[4] * xc0 + M[5] * yc0 + M[7] - g.y0) / g.vy - 0.5;
  const double det = a00 * a11 - a01 * a10;
  double jmin = 1e300, jmax = -1e300, imin = 1e300, imax = -1e300;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double qj = (double)v + ((k & 1) ? 1.0 : -1.0) - t0, qi = (double)u + ((k >> 1) ? 1.0 : -1.0) - t1;
    const double pj = (a11 * qj - a01 * qi) / det, pi = (a00 * qi - a10 * qj) / det;
    jmin = fmin(jmin, pj), jmax = fmax(jmax, pj), imin = fmin(imin, pi), imax = fmax(imax, pi);
  }
  const int jlo = (int)fmin(fmax(floor(jmin) - 1.0, 0.0), (double)g.W), jhi = (int)fmax(fmin(ceil(jmax) + 1.0, (double)g.W - 1.0), -1.0);
  const int ilo = (int)fmin(fmax(floor(imin) - 1.0, 0.0), (double)g.H), ihi = (int)fmax(fmin(ceil(imax) + 1.0, (double)g.H - 1.0), -1.0);
  const int nj = jhi - jlo + 1, ni = ihi - ilo + 1;
  const int ncand = (nj > 0 && ni > 0) ? ni * nj : 0;
  const float* dyb = dy + (size_t)b * g.H * g.W * dy_cs;
  float* dst = dx + (size_t)((b * g.H + u) * g.W + v) * C;
  for (int c0 = 0; c0 < C; c0 += 64 * Q) {
    const int c = c0 + lane * Q;
    float acc[Q] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < ncand; k0 += 64) {
      // lane l weighs candidate k0 + l; the wave then walks the contributing ones in ascending (row-major) order
      const int k = k0 + lane;
      float wk = 0.f;
      int cell = 0;
      if (k < ncand) {
        const int i = ilo + k / nj, j = jlo + k % nj;
        const CornerSample s = warp_sample(M, g, i, j);
        const int di = u - s.i0, dj = v - s.j0;
        if (s.ok && di >= 0 && di <= 1 && dj >= 0 && dj <= 1) wk = di ? (dj ? s.w[3] : s.w[2]) : (dj ? s.w[1] : s.w[0]);
        cell = i * g.W + j;
      }
      accumulate_targets<Q>(__ballot(wk != 0.f), wk, cell, dyb, dy_cs, c, c < C, acc);
    }
    if (c < C) store_q<float, Q>(dst + c, acc);
  }
}

int warp_check(const char* what, const void* x, const void* y, const void* ego, int B, int H, int W, int C, int x_cs, int y_cs,
               float vx, float vy, size_t elem) {
  BEVF_REQUIRE(x && y && ego, "%s: null pointer", what);
  BEVF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % Q == 0, "%s: bad shape (B=%d H=%d W=%d C=%d; C a multiple of %d)", what, B, H,
               W, C, Q);
  BEVF_REQUIRE(x_cs >= C && y_cs >= C && x_cs % Q == 0 && y_cs % Q == 0, "%s: channel strides must be multiples of %d and >= C", what,
               Q);
  BEVF_REQUIRE((long long)B * H * W * (x_cs > y_cs ? x_cs : y_cs) < (1ll << 31), "%s: B * H * W * stride exceeds the 32-bit offsets",
               what);
  const uintptr_t al = Q * elem - 1;
  BEVF_REQUIRE(!((uintptr_t)x & al) && !((uintptr_t)y & al) && !((uintptr_t)ego & 7u), "%s: unaligned buffer", what);
  BEVF_REQUIRE(vx != 0.f && vy != 0.f && vx == vx && vy == vy, "%s: cell size must be non-zero", what);
  return BEVF_OK;
}

template <typename T>
int warp_entry(const void* x, void* y, const double* ego, int B, int H, int W, int C, int x_cs, int y_cs, float x0, float y0,
               float vx, float vy, void* stream) {
  const int rc = warp_check("bev_warp", x, y, ego, B, H, W, C, x_cs, y_cs, vx, vy, sizeof(T));
  if (rc != BEVF_OK) return rc;
  const WarpGeom g{(double)x0, (double)y0, (double)vx, (double)vy, H, W};
  const int cells = B * H * W;
  constexpr int per_block = CELLS_PER_BLOCK * CELLS_PER_WAVE;
  hipLaunchKernelGGL(bev_warp<T>, dim3((cells + per_block - 1) / per_block), dim3(64 * CELLS_PER_BLOCK), 0,
                     static_cast<hipStream_t>(stream), static_cast<const T*>(x), static_cast<T*>(y), ego, g, cells, C, x_cs, y_cs);
  return bevf_check_launch("bevf_bev_warp");
}

}  // namespace

extern "C" int bevf_bev_warp_f32(const float* x, float* y, const double* ego, int B, int H, int W, int C, int x_cs, int y_cs,
                                 float x0, float y0, float vx, float vy, void* stream) {
  return warp_entry<float>(x, y, ego, B, H, W, C, x_cs, y_cs, x0, y0, vx, vy, stream);
}

extern "C" int bevf_bev_warp_bf16(const void* x, void* y, const double* ego, int B, int H, int W, int C, int x_cs, int y_cs,
                                  float x0, float y0, float vx, float vy, void* stream) {
  return warp_entry<__bf16>(x, y, ego, B, H, W, C, x_cs, y_cs, x0, y0, vx, vy, stream);
}

extern "C" int bevf_bev_warp_bwd_f32(const float* dy, float* dx, const double* ego, int B, int H, int W, int C, int dy_cs, float x0,
                                     float y0, float vx, float vy, void* stream) {
  const int rc = warp_check("bev_warp_bwd", dy, dx, ego, B, H, W, C, dy_cs, C, vx, vy, sizeof(float));
  if (rc != BEVF_OK) return rc;
  const WarpGeom g{(double)x0, (double)y0, (double)vx, (double)vy, H, W};
  const int cells = B * H * W;
  hipLaunchKernelGGL(bev_warp_bwd, dim3((cells + CELLS_PER_BLOCK - 1) / CELLS_PER_BLOCK), dim3(64 * CELLS_PER_BLOCK), 0,
                     static_cast<hipStream_t>(stream), dy, dx, ego, g, cells, C, dy_cs);
  return bevf_check_launch("bevf_bev_warp_bwd_f32");
}
