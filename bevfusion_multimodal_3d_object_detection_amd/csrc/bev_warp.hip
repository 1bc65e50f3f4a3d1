// Ego-motion warp of an NHWC BEV map (temporal fusion): the previous frame's map resampled onto the current
// frame's grid through a per-frame planar affine map, and the transposed resample for training.
//   bevf_bev_warp_{f32,bf16}   one wave per four output cells: the sample point and its four corner rows are wave-uniform (computed in
//                              fp64 from the device-side ego matrix, so a captured graph takes the matrix as an input), lanes walk the
//                              channels four at a time (16 bytes fp32, 8 bytes bf16).  Every output row is written, zeros included.
//   bevf_bev_warp_bwd_f32      a pull, no atomics: one wave per SOURCE cell collects the targets whose sample point lies within one
//                              cell of it -- candidates from the bounding box of the inverse affine image, weights recomputed with the
//                              forward's own expression (warp_sample), accumulated in row-major target order.
// HBM-bound: no LDS, no atomics.
#include "common.h"

namespace {

constexpr int CELLS_PER_BLOCK = 4;  // waves per 256-thread block: one source cell each in the backward ...
constexpr int CELLS_PER_WAVE = 4;   // ... and this many output cells each in the forward
constexpr int Q = 4;                // channels per lane and step

struct WarpGeom {
  double x0, y0, vx, vy;
  int H, W;
};

// The sample of target cell (row i, column j) under M = ego[b] (row-major 4 x 4; rows 0-1, columns 0, 1, 3 are read): the upper-left
// corner (i0, j0) and the four weights in the order (i0,j0), (i0,j0+1), (i0+1,j0), (i0+1,j0+1), each rounded once to fp32.
// ok = false: the point is non-finite or more than one cell outside the map -- no corner contributes.
struct WarpSample {
  int i0, j0;
  float w[4];
  bool ok;
};

__device__ __forceinline__ WarpSample warp_sample(const double* __restrict__ M, const WarpGeom& g, int i, int j) {
#pragma clang fp contract(off)
  const double xc = g.x0 + ((double)j + 0.5) * g.vx, yc = g.y0 + ((double)i + 0.5) * g.vy;
  const double xp = M[0] * xc + M[1] * yc + M[3], yp = M[4] * xc + M[5] * yc + M[7];
  const double qj = (xp - g.x0) / g.vx - 0.5, qi = (yp - g.y0) / g.vy - 0.5;
  WarpSample s;
  s.ok = qj > -1.0 && qj < (double)g.W && qi > -1.0 && qi < (double)g.H;  // (false for NaN and infinities)
  s.i0 = s.j0 = 0;
  s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
  if (s.ok) {
    const double fj0 = floor(qj), fi0 = floor(qi);
    const double fj = qj - fj0, fi = qi - fi0;
    s.j0 = (int)fj0, s.i0 = (int)fi0;
    s.w[0] = (float)((1.0 - fi) * (1.0 - fj));
    s.w[1] = (float)((1.0 - fi) * fj);
    s.w[2] = (float)(fi * (1.0 - fj));
    s.w[3] = (float)(fi * fj);
  }
  return s;
}

template <typename T>
__device__ __forceinline__ void load_q(const T* p, float (&f)[Q]) {
  if constexpr (sizeof(T) == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < Q; ++k) f[k] = v[k];
  } else {
    typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
    const bf16x4_t v = *reinterpret_cast<const bf16x4_t*>(p);
#pragma unroll
    for (int k = 0; k < Q; ++k) f[k] = (float)v[k];
  }
}

template <typename T>
__device__ __forceinline__ void store_q(T* p, const float (&f)[Q]) {
  if constexpr (sizeof(T) == 4) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < Q; ++k) v[k] = f[k];
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
    bf16x4_t v;
#pragma unroll
    for (int k = 0; k < Q; ++k) v[k] = (__bf16)f[k];
    *reinterpret_cast<bf16x4_t*>(p) = v;
  }
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

// One output cell (b, i, j) with its sample s, all wave-uniform: the four corner rows summed into the output row.
template <typename T>
__device__ __forceinline__ void warp_row(const T* __restrict__ x, T* __restrict__ y, const WarpGeom& g, const WarpSample& s, int b,
                                         int i, int j, int lane, int C, int x_cs, int y_cs) {
  // corner k = (di, dj) = (k >> 1, k & 1): inside the map?  Offsets fit 32 bits (checked by the entry point).
  bool in[4];
  const T* src[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ii = s.i0 + (k >> 1), jj = s.j0 + (k & 1);
    in[k] = s.ok && ii >= 0 && ii < g.H && jj >= 0 && jj < g.W;
    src[k] = x + (size_t)((b * g.H + (in[k] ? ii : 0)) * g.W + (in[k] ? jj : 0)) * x_cs;
  }
  T* dst = y + (size_t)((b * g.H + i) * g.W + j) * y_cs;
  const int cq = C / Q;
  for (int c = lane; c < cq; c += 64) {
    float v[4][Q], o[Q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (in[k]) {
        load_q(src[k] + c * Q, v[k]);
      } else {
#pragma unroll
        for (int q = 0; q < Q; ++q) v[k][q] = 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      float a = s.w[0] * v[0][q];
      a = fmaf(s.w[1], v[1][q], a);
      a = fmaf(s.w[2], v[2][q], a);
      o[q] = fmaf(s.w[3], v[3][q], a);
    }
    store_q(dst + c * Q, o);
  }
}

// A wave takes CELLS_PER_WAVE consecutive cells: lane k computes the fp64 geometry of cell k (the same instructions for every lane,
// so four cells cost what one did), then the wave walks the cells with each sample read back as scalars.
template <typename T>
__global__ __launch_bounds__(256) void bev_warp(const T* __restrict__ x, T* __restrict__ y, const double* __restrict__ ego,
                                                 WarpGeom g, int cells, int C, int x_cs, int y_cs) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r0 = (xcd_remap((int)blockIdx.x, (int)gridDim.x) * CELLS_PER_BLOCK + wave) * CELLS_PER_WAVE;
  if (r0 >= cells) return;
  const int P = g.H * g.W;
  const int rl = min(r0 + (lane & (CELLS_PER_WAVE - 1)), cells - 1);
  const int bl = rl / P, il = (rl - bl * P) / g.W;
  const WarpSample sl = warp_sample(ego + (size_t)bl * 16, g, il, rl - bl * P - il * g.W);
#pragma unroll
  for (int k = 0; k < CELLS_PER_WAVE; ++k) {
    const int r = r0 + k;
    if (r >= cells) break;
    WarpSample s;
    s.i0 = __builtin_amdgcn_readlane(sl.i0, k);
    s.j0 = __builtin_amdgcn_readlane(sl.j0, k);
    s.ok = __builtin_amdgcn_readlane((int)sl.ok, k) != 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) s.w[q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sl.w[q]), k));
    const int b = r / P, i = (r - b * P) / g.W;
    warp_row(x, y, g, s, b, i, r - b * P - i * g.W, lane, C, x_cs, y_cs);
  }
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
  const int cq = C / Q;
  for (int c0 = 0; c0 < cq; c0 += 64) {
    const int c = c0 + lane;
    float acc[Q] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < ncand; k0 += 64) {
      // lane l weighs candidate k0 + l; the wave then walks the contributing ones in ascending (row-major) order
      const int k = k0 + lane;
      float wk = 0.f;
      int cell = 0;
      if (k < ncand) {
        const int i = ilo + k / nj, j = jlo + k % nj;
        const WarpSample s = warp_sample(M, g, i, j);
        const int di = u - s.i0, dj = v - s.j0;
        if (s.ok && di >= 0 && di <= 1 && dj >= 0 && dj <= 1) wk = di ? (dj ? s.w[3] : s.w[2]) : (dj ? s.w[1] : s.w[0]);
        cell = i * g.W + j;
      }
      unsigned long long mask = __ballot(wk != 0.f);
      while (mask) {
        const int l = __builtin_ctzll(mask);
        mask &= mask - 1;
        const float w = __shfl(wk, l, 64);
        const int p = __shfl(cell, l, 64);
        if (c < cq) {
          float d[Q];
          load_q(dyb + (size_t)p * dy_cs + c * Q, d);
#pragma unroll
          for (int q = 0; q < Q; ++q) acc[q] = fmaf(w, d[q], acc[q]);
        }
      }
    }
    if (c < cq) store_q(dst + c * Q, acc);
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
