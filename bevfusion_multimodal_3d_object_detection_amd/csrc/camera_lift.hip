// Learned-depth camera -> BEV lift of the opt-in `camera_view_transform: 'lift'` branch (camera_rig.build_lift_table, DESIGN.md
// 3.2d2), as a PULL over the projection-table design of camera_bev.hip: every table entry carries a depth bin next to its pixel,
//     y[b][cell][0:C] = sum_e w_e * Pd[b][pix_e][bin_e] * x[b][pix_e][0:C]          (entries in table order, fp32 accumulation)
// with Pd the per-pixel softmax over D <= 64 depth bins.  No atomics, every output element written exactly once (zeros for an
// empty row), nothing allocated: stream-ordered and graph-capturable.  fp32 only.
//
//   softmax_rows / softmax_rows_bwd   rows of D contiguous floats; a row takes the next power of two >= D lanes, so a wave holds
//                                     64 / that many rows (D = 4: 16 rows per wave)
//   csr_lift                          csr_gather's shape (one wave per cell, lanes over the channels in 16-byte vectors, entries
//                                     read with wave-uniform loads and used for GB frames at a time) plus one wave-uniform load of
//                                     Pd[b][col2] per entry and frame; col2 = pixel * D + bin
//   csr_lift_bwd                      one wave per (pixel, frame) on the transposed table: the lane keeps its channels of x[b][pix],
//                                     per entry loads dy[b][cell], accumulates dx and reduces <x, dy> over the wave with a fixed
//                                     xor butterfly into the accumulator of the entry's bin -- lane d owns bin d
#include "common.h"

namespace {

constexpr int GB = 4;              // frames per pass over a row's entries
constexpr int ROWS_PER_BLOCK = 4;  // one row per wave, 256 threads

__global__ __launch_bounds__(256) void softmax_rows(const float* __restrict__ x, int x_rs, float* __restrict__ y, int y_rs,
                                                    long long nrows, int D, int lg) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = t >> lg;                               // L = 1 << lg divides 64: a row never straddles two waves
  const int L = 1 << lg, d = (int)(t & (L - 1));
  const bool on = row < nrows && d < D;
  const float v = on ? x[row * x_rs + d] : -INFINITY;
  const float mx = group_reduce<true>(v, L);
  const float e = on ? expf(v - mx) : 0.f;
  const float s = group_reduce<false>(e, L);
  if (on) y[row * y_rs + d] = e / s;
}

// dx[row][d] = pd * (dpd - sum_d pd * dpd) for d < D, 0 for D <= d < x_cols
__global__ __launch_bounds__(256) void softmax_rows_bwd(const float* __restrict__ pd, const float* __restrict__ dpd, int p_rs,
                                                        float* __restrict__ dx, int x_rs, int x_cols, long long nrows, int D,
                                                        int lg) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = t >> lg;
  const int L = 1 << lg, d = (int)(t & (L - 1));
  const bool on = row < nrows && d < D;
  const float p = on ? pd[row * p_rs + d] : 0.f;
  const float g = on ? dpd[row * p_rs + d] : 0.f;
  const float s = group_reduce<false>(p * g, L);
  if (row < nrows && d < x_cols) dx[row * x_rs + d] = on ? p * (g - s) : 0.f;
}

template <int KV>
__global__ __launch_bounds__(256) void csr_lift(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col2,
                                                const float* __restrict__ w, int nrows, int D, unsigned dmul, unsigned dsh,
                                                const float* __restrict__ x, long long x_bs, int x_cs,
                                                const float* __restrict__ pd, long long pd_bs, float* __restrict__ y,
                                                long long y_bs, int y_cs, int B, int C) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r = xcd_remap((int)blockIdx.x, (int)gridDim.x) * ROWS_PER_BLOCK + wave;
  if (r >= nrows) return;
  const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
  const int cv = C / 4;
  for (int b0 = 0; b0 < B; b0 += GB) {
    float acc[GB][KV][4];
#pragma unroll
    for (int g = 0; g < GB; ++g)
#pragma unroll
      for (int k = 0; k < KV; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[g][k][q] = 0.f;
#pragma unroll 2
    for (int e = e0; e < e1; ++e) {
      const int c2 = col2[e];
      const long long off = (long long)div_by(c2, dmul, dsh) * x_cs;
      const float we = w[e];
#pragma unroll
      for (int g = 0; g < GB; ++g) {
        if (b0 + g < B) {
          const float s = we * pd[(long long)(b0 + g) * pd_bs + c2];
          const float* src = x + (long long)(b0 + g) * x_bs + off;
#pragma unroll
          for (int k = 0; k < KV; ++k) {
            const int j = lane + 64 * k;
            if (j < cv) {
              float v[4];
              load16(src + j * 4, v);
#pragma unroll
              for (int q = 0; q < 4; ++q) acc[g][k][q] = fmaf(s, v[q], acc[g][k][q]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      if (b0 + g < B) {
        float* dst = y + (long long)(b0 + g) * y_bs + (long long)r * y_cs;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          const int j = lane + 64 * k;
          if (j < cv) store16(dst + j * 4, acc[g][k]);
        }
      }
    }
  }
}

template <int KV>
__global__ __launch_bounds__(256) void csr_lift_bwd(const int32_t* __restrict__ t_row_ptr, const int32_t* __restrict__ t_cell,
                                                    const int32_t* __restrict__ t_bin, const float* __restrict__ t_w, int npix,
                                                    int D, const float* __restrict__ x, long long x_bs, int x_cs,
                                                    const float* __restrict__ pd, long long pd_bs, const float* __restrict__ dy,
                                                    long long dy_bs, int dy_cs, float* __restrict__ dx, long long dx_bs,
                                                    int dx_cs, float* __restrict__ dpd, long long dpd_bs, int C) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int pix = xcd_remap((int)blockIdx.x, (int)gridDim.x) * ROWS_PER_BLOCK + wave;
  if (pix >= npix) return;
  const int b = (int)blockIdx.y;
  const int e0 = t_row_ptr[pix], e1 = t_row_ptr[pix + 1];
  const int cv = C / 4;
  float xv[KV][4], acc[KV][4];
  const float* xs = x + (long long)b * x_bs + (long long)pix * x_cs;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int j = lane + 64 * k;
#pragma unroll
    for (int q = 0; q < 4; ++q) xv[k][q] = acc[k][q] = 0.f;
    if (j < cv) load16(xs + j * 4, xv[k]);
  }
  const float* pdr = pd + (long long)b * pd_bs + (long long)pix * D;
  const float* dyb = dy + (long long)b * dy_bs;
  float bin_acc = 0.f;                                          // lane d: dPd[b][pix][d]
  for (int e = e0; e < e1; ++e) {
    const int bin = t_bin[e];
    const float we = t_w[e];
    const float s = we * pdr[bin];
    const float* src = dyb + (long long)t_cell[e] * dy_cs;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int j = lane + 64 * k;
      if (j < cv) {
        float v[4];
        load16(src + j * 4, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[k][q] = fmaf(s, v[q], acc[k][q]);
          dot = fmaf(xv[k][q], v[q], dot);
        }
      }
    }
    dot = group_reduce<false>(dot, 64);
    if (lane == bin) bin_acc = fmaf(we, dot, bin_acc);
  }
  float* dst = dx + (long long)b * dx_bs + (long long)pix * dx_cs;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int j = lane + 64 * k;
    if (j < cv) store16(dst + j * 4, acc[k]);
  }
  if (lane < D) dpd[(long long)b * dpd_bs + (long long)pix * D + lane] = bin_acc;
}

int log2_lanes_per_row(int cols) {
  int lg = 0;
  while ((1 << lg) < cols) ++lg;
  return lg;
}

bool lift_shape_ok(int nrows, int D, int B, int C) { return nrows > 0 && D >= 1 && D <= 64 && B > 0 && C > 0 && C % 4 == 0 && C / 4 <= 256; }

}  // namespace

extern "C" int bevf_softmax_rows_f32(const float* x, int x_rs, float* y, int y_rs, size_t nrows, int D, void* stream) {
  BEVF_REQUIRE(x && y, "softmax_rows: null pointer");
  BEVF_REQUIRE(nrows > 0 && D >= 1 && D <= 64 && x_rs >= D && y_rs >= D, "softmax_rows: bad shape (nrows=%zu D=%d; 1 <= D <= 64 <= strides)",
               nrows, D);
  const int lg = log2_lanes_per_row(D);
  const unsigned long long blocks = (((unsigned long long)nrows << lg) + 255) / 256;
  BEVF_REQUIRE(blocks < (1ull << 31), "softmax_rows: too many rows");
  hipLaunchKernelGGL(softmax_rows, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, x_rs, y, y_rs,
                     (long long)nrows, D, lg);
  return bevf_check_launch("bevf_softmax_rows_f32");
}

extern "C" int bevf_softmax_rows_bwd_f32(const float* pd, const float* dpd, int p_rs, float* dx, int x_rs, int x_cols,
                                         size_t nrows, int D, void* stream) {
  BEVF_REQUIRE(pd && dpd && dx, "softmax_rows_bwd: null pointer");
  BEVF_REQUIRE(nrows > 0 && D >= 1 && D <= 64 && p_rs >= D && x_cols >= D && x_cols <= 64 && x_rs >= x_cols,
               "softmax_rows_bwd: bad shape (nrows=%zu D=%d x_cols=%d)", nrows, D, x_cols);
  const int lg = log2_lanes_per_row(x_cols);
  const unsigned long long blocks = (((unsigned long long)nrows << lg) + 255) / 256;
  BEVF_REQUIRE(blocks < (1ull << 31), "softmax_rows_bwd: too many rows");
  hipLaunchKernelGGL(softmax_rows_bwd, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), pd, dpd, p_rs, dx,
                     x_rs, x_cols, (long long)nrows, D, lg);
  return bevf_check_launch("bevf_softmax_rows_bwd_f32");
}

extern "C" int bevf_csr_lift_f32(const int32_t* row_ptr, const int32_t* col2, const float* w, int nrows, int D, const float* x,
                                 size_t x_bs, int x_cs, const float* pd, size_t pd_bs, float* y, size_t y_bs, int y_cs, int B,
                                 int C, void* stream) {
  BEVF_REQUIRE(row_ptr && x && pd && y, "csr_lift: null pointer");
  BEVF_REQUIRE(lift_shape_ok(nrows, D, B, C), "csr_lift: bad shape (nrows=%d D=%d B=%d C=%d; C a multiple of 4, at most 1024, D <= 64)",
               nrows, D, B, C);
  BEVF_REQUIRE(x_cs >= C && y_cs >= C && x_cs % 4 == 0 && y_cs % 4 == 0 && x_bs % 4 == 0 && y_bs % 4 == 0,
               "csr_lift: strides must be 16-byte multiples and channel strides >= C");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(y), "csr_lift: unaligned feature buffer");
  const dim3 grid((nrows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), block(64 * ROWS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned dmul, dsh;
  div_make(D, &dmul, &dsh);
  const int cv = C / 4;
#define BEVF_LIFT(KV)                                                                                                        \
  hipLaunchKernelGGL((csr_lift<KV>), grid, block, 0, s, row_ptr, col2, w, nrows, D, dmul, dsh, x, (long long)x_bs, x_cs, pd, \
                     (long long)pd_bs, y, (long long)y_bs, y_cs, B, C)
  if (cv <= 64)
    BEVF_LIFT(1);
  else if (cv <= 128)
    BEVF_LIFT(2);
  else
    BEVF_LIFT(4);
#undef BEVF_LIFT
  return bevf_check_launch("bevf_csr_lift_f32");
}

extern "C" int bevf_csr_lift_bwd_f32(const int32_t* t_row_ptr, const int32_t* t_cell, const int32_t* t_bin, const float* t_w,
                                     int npix, int D, const float* x, size_t x_bs, int x_cs, const float* pd, size_t pd_bs,
                                     const float* dy, size_t dy_bs, int dy_cs, float* dx, size_t dx_bs, int dx_cs, float* dpd,
                                     size_t dpd_bs, int B, int C, void* stream) {
  BEVF_REQUIRE(t_row_ptr && x && pd && dy && dx && dpd, "csr_lift_bwd: null pointer");
  BEVF_REQUIRE(lift_shape_ok(npix, D, B, C) && B <= 65535,
               "csr_lift_bwd: bad shape (npix=%d D=%d B=%d C=%d; C a multiple of 4, at most 1024, D <= 64, B <= 65535)", npix, D, B, C);
  BEVF_REQUIRE(x_cs >= C && dy_cs >= C && dx_cs >= C && x_cs % 4 == 0 && dy_cs % 4 == 0 && dx_cs % 4 == 0 && x_bs % 4 == 0 &&
                   dy_bs % 4 == 0 && dx_bs % 4 == 0,
               "csr_lift_bwd: strides must be 16-byte multiples and channel strides >= C");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(dy) && bevf_aligned16(dx), "csr_lift_bwd: unaligned feature buffer");
  const dim3 grid((npix + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, B), block(64 * ROWS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cv = C / 4;
#define BEVF_LIFT_BWD(KV)                                                                                                       \
  hipLaunchKernelGGL((csr_lift_bwd<KV>), grid, block, 0, s, t_row_ptr, t_cell, t_bin, t_w, npix, D, x, (long long)x_bs, x_cs,  \
                     pd, (long long)pd_bs, dy, (long long)dy_bs, dy_cs, dx, (long long)dx_bs, dx_cs, dpd, (long long)dpd_bs, C)
  if (cv <= 64)
    BEVF_LIFT_BWD(1);
  else if (cv <= 128)
    BEVF_LIFT_BWD(2);
  else
    BEVF_LIFT_BWD(4);
#undef BEVF_LIFT_BWD
  return bevf_check_launch("bevf_csr_lift_bwd_f32");
}
