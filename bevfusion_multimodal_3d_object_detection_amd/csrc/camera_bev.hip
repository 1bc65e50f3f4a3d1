// Camera -> BEV projection of the opt-in `camera_view_transform: 'project'` branch (camera_rig.py): one
// deterministic gather over a CSR table,  y[b][r][0:C] = sum_e w_e * x[b][col_e][0:C]  (entries in table order, fp32
// accumulation).  The forward runs it on the cell table (rows = BEV cells, columns = camera feature pixels), the backward on
// the exact transpose (rows = pixels): no atomics, every output row written once (zeros for an empty row).
//
// Shape: one wave per table row, lanes over the channels in 16-byte vectors (fp32: 4, bf16: 8 channels), the row's (col, w)
// entries read once with wave-uniform (scalar) loads and used for GB frames at a time, so every entry issues GB * KV
// independent 16-byte loads.  Consecutive rows -- neighbouring BEV cells, which sample neighbouring pixels -- go to the same
// XCD (xcd_remap), so the rows they share are served from that XCD's L2.
#include "common.h"

namespace {

constexpr int GB = 4;              // frames per pass over a row's entries
constexpr int ROWS_PER_BLOCK = 4;  // one row per wave, 256 threads

template <typename T, int KV>
__global__ __launch_bounds__(256) void csr_gather(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                   const float* __restrict__ w, int nrows, const T* __restrict__ x,
                                                   long long x_bs, int x_cs, T* __restrict__ y, long long y_bs, int y_cs,
                                                   int B, int C) {
  constexpr int V = vec16<T>::N;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r = xcd_remap((int)blockIdx.x, (int)gridDim.x) * ROWS_PER_BLOCK + wave;
  if (r >= nrows) return;
  const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
  const int cv = C / V;
  for (int b0 = 0; b0 < B; b0 += GB) {
    float acc[GB][KV][V];
#pragma unroll
    for (int g = 0; g < GB; ++g)
#pragma unroll
      for (int k = 0; k < KV; ++k)
#pragma unroll
        for (int q = 0; q < V; ++q) acc[g][k][q] = 0.f;
#pragma unroll 2
    for (int e = e0; e < e1; ++e) {
      const long long off = (long long)col[e] * x_cs;
      const float we = w[e];
#pragma unroll
      for (int g = 0; g < GB; ++g) {
        if (b0 + g < B) {
          const T* src = x + (long long)(b0 + g) * x_bs + off;
#pragma unroll
          for (int k = 0; k < KV; ++k) {
            const int j = lane + 64 * k;
            if (j < cv) {
              float v[V];
              load16(src + j * V, v);
#pragma unroll
              for (int q = 0; q < V; ++q) acc[g][k][q] = fmaf(we, v[q], acc[g][k][q]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      if (b0 + g < B) {
        T* dst = y + (long long)(b0 + g) * y_bs + (long long)r * y_cs;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          const int j = lane + 64 * k;
          if (j < cv) store16(dst + j * V, acc[g][k]);
        }
      }
    }
  }
}

template <typename T>
int csr_gather_entry(const int32_t* row_ptr, const int32_t* col, const float* w, int nrows, const void* x, size_t x_bs,
                     int x_cs, void* y, size_t y_bs, int y_cs, int B, int C, void* stream) {
  constexpr int V = vec16<T>::N;
  BEVF_REQUIRE(row_ptr && x && y, "csr_gather: null pointer");
  BEVF_REQUIRE(nrows > 0 && B > 0 && C > 0 && C % V == 0 && C / V <= 256,
               "csr_gather: bad shape (nrows=%d B=%d C=%d; C a multiple of %d, at most %d)", nrows, B, C, V, 256 * V);
  BEVF_REQUIRE(x_cs >= C && y_cs >= C && x_cs % V == 0 && y_cs % V == 0 && x_bs % V == 0 && y_bs % V == 0,
               "csr_gather: strides must be 16-byte multiples and channel strides >= C");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(y), "csr_gather: unaligned feature buffer");
  const dim3 grid((nrows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), block(64 * ROWS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const T* xs = static_cast<const T*>(x);
  T* ys = static_cast<T*>(y);
  const int cv = C / V;
  if (cv <= 64)
    hipLaunchKernelGGL((csr_gather<T, 1>), grid, block, 0, s, row_ptr, col, w, nrows, xs, (long long)x_bs, x_cs, ys,
                       (long long)y_bs, y_cs, B, C);
  else if (cv <= 128)
    hipLaunchKernelGGL((csr_gather<T, 2>), grid, block, 0, s, row_ptr, col, w, nrows, xs, (long long)x_bs, x_cs, ys,
                       (long long)y_bs, y_cs, B, C);
  else
    hipLaunchKernelGGL((csr_gather<T, 4>), grid, block, 0, s, row_ptr, col, w, nrows, xs, (long long)x_bs, x_cs, ys,
                       (long long)y_bs, y_cs, B, C);
  return bevf_check_launch("bevf_csr_gather");
}

}  // namespace

extern "C" int bevf_csr_gather_f32(const int32_t* row_ptr, const int32_t* col, const float* w, int nrows, const float* x,
                                   size_t x_bs, int x_cs, float* y, size_t y_bs, int y_cs, int B, int C, void* stream) {
  return csr_gather_entry<float>(row_ptr, col, w, nrows, x, x_bs, x_cs, y, y_bs, y_cs, B, C, stream);
}

extern "C" int bevf_csr_gather_bf16(const int32_t* row_ptr, const int32_t* col, const float* w, int nrows, const void* x,
                                    size_t x_bs, int x_cs, void* y, size_t y_bs, int y_cs, int B, int C, void* stream) {
  return csr_gather_entry<__bf16>(row_ptr, col, w, nrows, x, x_bs, x_cs, y, y_bs, y_cs, B, C, stream);
}
