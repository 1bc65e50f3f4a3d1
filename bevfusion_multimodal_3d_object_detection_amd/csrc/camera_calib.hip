// Per-frame camera calibration of the opt-in `camera_view_transform: 'project'` branch (camera_rig.py):
// the projection table of camera_rig.build_projection_table built ON THE DEVICE, one CSR table per frame, from a
// [B][ncam][4][4] fp64 calibration tensor -- no host synchronisation, no allocation, safe inside a graph capture.
//
//   bevf_camera_table_build_f64   cells -> fixed slots (geometry in fp64, duplicates merged, sorted by pixel)
//                                 -> per-frame scan of the row lengths -> compaction into CSR by cell
//   bevf_camera_table_transpose   histogram of the pixels (integer atomics) -> scan -> scatter through an atomic
//                                 cursor -> every pixel row rank-sorted by forward entry index: the ORDER does not
//                                 depend on the atomics, so two runs give the same bits
//   bevf_csr_gather_frames_*      bevf_csr_gather with one table per frame
//
// Frame b's entries live at [b * cap, b * cap + row_ptr[b][nrows]) of col / w, cap = the caller's per-frame capacity
// (>= P * num_heights * ncam * 4, the worst case); only the used part is touched.  Frame offsets are 64-bit.
#include "common.h"
#include "scan_counts.h"

namespace {

struct TableGeom {
  double x0, y0, vx, vy, z0, dz, min_depth;
  int bev_w, P, nh, ncam, H, W, Hc, Wc;
};

// One wave per (frame, cell).  Candidates = the in-map bilinear taps of the cell's valid (camera, height) samples, in
// the fixed order (chunk of 64 samples, tap, lane); merged by pixel key in fp64 (candidate order), exact zeros dropped,
// written to the cell's slots in ascending pixel order.  LDS: 4 * nh * ncam candidates.
__global__ __launch_bounds__(64) void table_cells(const double* __restrict__ calib, TableGeom g, int2* __restrict__ slots,
                                                  long long cap, int32_t* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int ns = g.nh * g.ncam, S = 4 * ns;
  double* cw = reinterpret_cast<double*>(sm);   // [S] tap weight wx * wy of a candidate
  double* ws = cw + S;                          // [S] merged weight (at the first candidate of a key)
  int* ck = reinterpret_cast<int*>(ws + S);     // [S] pixel key of a candidate
  int* kk = ck + S;                             // [S] the key when the candidate is the kept entry of its key, else -1
  const int lane = (int)threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)g.P), p = (int)(blockIdx.x % (unsigned)g.P);
  const int ci = p / g.bev_w, cj = p % g.bev_w;
  const double px = g.x0 + (cj + 0.5) * g.vx, py = g.y0 + (ci + 0.5) * g.vy;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n = 0, nvalid = 0;                        // wave-uniform
  for (int s0 = 0; s0 < ns; s0 += 64) {
    const int s = s0 + lane;
    bool valid = false;
    int xi = 0, yi = 0, c = 0;
    double lx = 0.0, ly = 0.0;
    if (s < ns) {
      c = s / g.nh;
      const int k = s % g.nh;
      const double pz = g.z0 + (k + 0.5) * g.dz / g.nh;
      const double* M = calib + ((long long)b * g.ncam + c) * 16;
      const double depth = M[12] * px + M[13] * py + M[14] * pz + M[15];
      if (depth > g.min_depth) {
        const double a0 = M[0] * px + M[1] * py + M[2] * pz + M[3];
        const double a1 = M[4] * px + M[5] * py + M[6] * pz + M[7];
        const double a2 = M[8] * px + M[9] * py + M[10] * pz + M[11];
        const double u = a0 / a2, v = a1 / a2;
        if (u >= 0.0 && u < (double)g.W && v >= 0.0 && v < (double)g.H) {
          valid = true;
          const double uf = (u + 0.5) * g.Wc / g.W - 0.5, vf = (v + 0.5) * g.Hc / g.H - 0.5;
          const double fx = floor(uf), fy = floor(vf);
          lx = uf - fx;
          ly = vf - fy;
          xi = (int)fx;
          yi = (int)fy;
        }
      }
    }
    nvalid += __popcll(__ballot(valid));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int dx = t & 1, dy = t >> 1;
      const int x = xi + dx, y = yi + dy;
      const bool ok = valid && x >= 0 && x < g.Wc && y >= 0 && y < g.Hc;
      const unsigned long long m = __ballot(ok);
      if (ok) {
        const int pos = n + __popcll(m & below);
        ck[pos] = (c * g.Hc + y) * g.Wc + x;
        cw[pos] = (dx ? lx : 1.0 - lx) * (dy ? ly : 1.0 - ly);
      }
      n += __popcll(m);
    }
  }
  __syncthreads();
  const double nsamp = (double)(nvalid > 0 ? nvalid : 1);
  for (int i = lane; i < n; i += 64) {
    const int key = ck[i];
    bool first = true;
    double sum = 0.0;
    for (int j = 0; j < n; ++j) {
      if (ck[j] == key) {
        first = first && j >= i;
        sum += cw[j] / nsamp;
      }
    }
    ws[i] = sum;
    kk[i] = (first && sum != 0.0) ? key : -1;
  }
  __syncthreads();
  int2* row = slots + (long long)b * cap + (long long)p * S;
  int kept = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const int key = i < n ? kk[i] : -1;
    if (key >= 0) {
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += (kk[j] >= 0 && kk[j] < key) ? 1 : 0;
      row[rank] = make_int2(key, __float_as_int((float)ws[i]));
    }
    kept += __popcll(__ballot(key >= 0));
  }
  if (lane == 0) cnt[(long long)b * g.P + p] = kept;
}

// One wave per (frame, cell): the cell's slots -> its CSR row.
__global__ __launch_bounds__(256) void compact_rows(const int2* __restrict__ slots, const int32_t* __restrict__ rp, int P,
                                                    int S, long long rows, long long cap, int32_t* __restrict__ col,
                                                    float* __restrict__ w) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = (int)(threadIdx.x & 63);
  const long long b = r / P;
  const int p = (int)(r % P);
  const int32_t* fr = rp + b * (P + 1);
  const int e0 = fr[p], n = fr[p + 1] - e0;
  const int2* src = slots + b * cap + (long long)p * S;
  for (int i = lane; i < n; i += 64) {
    const int2 v = src[i];
    col[b * cap + e0 + i] = v.x;
    w[b * cap + e0 + i] = __int_as_float(v.y);
  }
}

// One wave per (frame, cell) of the forward table.  SCATTER == false: count the entries of every pixel;
// SCATTER == true: put (forward entry index, cell) at an atomic cursor inside the pixel's row (any order).
template <bool SCATTER>
__global__ __launch_bounds__(256) void pixel_pass(const int32_t* __restrict__ rp, const int32_t* __restrict__ col, int P,
                                                  int ncols, long long rows, long long cap, int32_t* __restrict__ tcnt,
                                                  const int32_t* __restrict__ trp, int2* __restrict__ tmp) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = (int)(threadIdx.x & 63);
  const long long b = r / P;
  const int p = (int)(r % P);
  const int32_t* fr = rp + b * (P + 1);
  const int e0 = fr[p], e1 = fr[p + 1];
  for (int e = e0 + lane; e < e1; e += 64) {
    const int q = col[b * cap + e];
    if constexpr (SCATTER) {
      const int pos = trp[b * (ncols + 1) + q] + atomicSub(&tcnt[b * ncols + q], 1) - 1;
      tmp[b * cap + pos] = make_int2(e, p);
    } else {
      atomicAdd(&tcnt[b * ncols + q], 1);
    }
  }
}

// One wave per (frame, pixel): the row's scattered entries ranked by forward entry index (= ascending cell, ties in the
// forward table's order) -- whatever order the cursor gave them.
__global__ __launch_bounds__(256) void sort_pixel_rows(const int32_t* __restrict__ trp, const int2* __restrict__ tmp,
                                                       const float* __restrict__ w, int ncols, long long rows,
                                                       long long cap, int32_t* __restrict__ t_col,
                                                       float* __restrict__ t_w) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = (int)(threadIdx.x & 63);
  const long long b = r / ncols;
  const int q = (int)(r % ncols);
  const int32_t* fr = trp + b * (ncols + 1);
  const int r0 = fr[q], n = fr[q + 1] - r0;
  const int2* src = tmp + b * cap + r0;
  for (int i = lane; i < n; i += 64) {
    const int2 v = src[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += src[j].x < v.x ? 1 : 0;
    t_col[b * cap + r0 + rank] = v.y;
    t_w[b * cap + r0 + rank] = w[b * cap + v.x];
  }
}

constexpr int EU = 4;              // entries in flight per pass (the shared-table kernel has 4 frames instead)
constexpr int ROWS_PER_BLOCK = 4;  // one row per wave, 256 threads

template <typename T, int KV>
__global__ __launch_bounds__(256) void csr_gather_frames(const int32_t* __restrict__ row_ptr, long long rp_stride,
                                                          const int32_t* __restrict__ col, const float* __restrict__ w,
                                                          long long e_stride, int nrows, const T* __restrict__ x,
                                                          long long x_bs, int x_cs, T* __restrict__ y, long long y_bs,
                                                          int y_cs, int C) {
  constexpr int V = vec16<T>::N;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r = xcd_remap((int)blockIdx.x, (int)gridDim.x) * ROWS_PER_BLOCK + wave;
  if (r >= nrows) return;
  const long long b = (long long)blockIdx.y;
  const int32_t* rp = row_ptr + b * rp_stride;
  const int32_t* cl = col + b * e_stride;
  const float* wt = w + b * e_stride;
  const T* xb = x + b * x_bs;
  const int e0 = rp[r], e1 = rp[r + 1];
  const int cv = C / V;
  float acc[KV][V];
#pragma unroll
  for (int k = 0; k < KV; ++k)
#pragma unroll
    for (int q = 0; q < V; ++q) acc[k][q] = 0.f;
  for (int e = e0; e < e1; e += EU) {
    float v[EU][KV][V];
    float we[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      we[u] = 0.f;
      if (e + u < e1) {
        const T* src = xb + (long long)cl[e + u] * x_cs;
        we[u] = wt[e + u];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          const int j = lane + 64 * k;
          if (j < cv) load16(src + j * V, v[u][k]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      if (e + u < e1) {
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          if (lane + 64 * k < cv) {
#pragma unroll
            for (int q = 0; q < V; ++q) acc[k][q] = fmaf(we[u], v[u][k][q], acc[k][q]);
          }
        }
      }
    }
  }
  T* dst = y + b * y_bs + (long long)r * y_cs;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int j = lane + 64 * k;
    if (j < cv) store16(dst + j * V, acc[k]);
  }
}

template <typename T>
int csr_gather_frames_entry(const int32_t* row_ptr, size_t rp_stride, const int32_t* col, const float* w, size_t e_stride,
                            int nrows, const void* x, size_t x_bs, int x_cs, void* y, size_t y_bs, int y_cs, int B, int C,
                            void* stream) {
  constexpr int V = vec16<T>::N;
  BEVF_REQUIRE(row_ptr && col && w && x && y, "csr_gather_frames: null pointer");
  BEVF_REQUIRE(nrows > 0 && B > 0 && B <= 65535 && C > 0 && C % V == 0 && C / V <= 256,
               "csr_gather_frames: bad shape (nrows=%d B=%d C=%d; C a multiple of %d, at most %d)", nrows, B, C, V, 256 * V);
  BEVF_REQUIRE(rp_stride >= (size_t)nrows + 1, "csr_gather_frames: row_ptr stride smaller than nrows + 1");
  BEVF_REQUIRE(x_cs >= C && y_cs >= C && x_cs % V == 0 && y_cs % V == 0 && x_bs % V == 0 && y_bs % V == 0,
               "csr_gather_frames: strides must be 16-byte multiples and channel strides >= C");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(y), "csr_gather_frames: unaligned feature buffer");
  const dim3 grid((nrows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, B), block(64 * ROWS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const T* xs = static_cast<const T*>(x);
  T* ys = static_cast<T*>(y);
  const int cv = C / V;
  if (cv <= 64)
    hipLaunchKernelGGL((csr_gather_frames<T, 1>), grid, block, 0, s, row_ptr, (long long)rp_stride, col, w,
                       (long long)e_stride, nrows, xs, (long long)x_bs, x_cs, ys, (long long)y_bs, y_cs, C);
  else if (cv <= 128)
    hipLaunchKernelGGL((csr_gather_frames<T, 2>), grid, block, 0, s, row_ptr, (long long)rp_stride, col, w,
                       (long long)e_stride, nrows, xs, (long long)x_bs, x_cs, ys, (long long)y_bs, y_cs, C);
  else
    hipLaunchKernelGGL((csr_gather_frames<T, 4>), grid, block, 0, s, row_ptr, (long long)rp_stride, col, w,
                       (long long)e_stride, nrows, xs, (long long)x_bs, x_cs, ys, (long long)y_bs, y_cs, C);
  return bevf_check_launch("bevf_csr_gather_frames");
}

inline unsigned wave_blocks(long long rows) { return (unsigned)((rows + 3) / 4); }

}  // namespace

extern "C" int bevf_camera_table_build_f64(const double* calib, int B, int ncam, float x0, float y0, float vx, float vy,
                                           int bev_h, int bev_w, float z0, float z1, int num_heights, double min_depth,
                                           int img_h, int img_w, int Hc, int Wc, int32_t* row_ptr, int32_t* col, float* w,
                                           size_t cap, void* work, void* stream) {
  BEVF_REQUIRE(calib && row_ptr && col && w && work, "camera_table_build: null pointer");
  BEVF_REQUIRE(B > 0 && ncam > 0 && bev_h > 0 && bev_w > 0 && num_heights > 0 && img_h > 0 && img_w > 0 && Hc > 0 && Wc > 0,
               "camera_table_build: bad shape");
  const long long P = (long long)bev_h * bev_w, S = 4ll * num_heights * ncam, ncols = (long long)ncam * Hc * Wc;
  BEVF_REQUIRE(S * 24 <= 65536, "camera_table_build: num_heights * ncam = %d exceeds 682 (LDS of one cell)", num_heights * ncam);
  BEVF_REQUIRE(ncols < (1ll << 31) && P * S < (1ll << 31) && (long long)B * P < (1ll << 31),
               "camera_table_build: table too large for int32 indices");
  BEVF_REQUIRE((long long)cap >= P * S, "camera_table_build: capacity %zu below the worst case %lld entries per frame", cap,
               P * S);
  TableGeom g;
  g.x0 = x0, g.y0 = y0, g.vx = vx, g.vy = vy, g.z0 = z0, g.dz = (double)z1 - (double)z0, g.min_depth = min_depth;
  g.bev_w = bev_w, g.P = (int)P, g.nh = num_heights, g.ncam = ncam, g.H = img_h, g.W = img_w, g.Hc = Hc, g.Wc = Wc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int2* slots = static_cast<int2*>(work);                               // [B][cap] (key, weight bits)
  int32_t* cnt = reinterpret_cast<int32_t*>(slots + (long long)B * cap);  // [B][P]
  hipLaunchKernelGGL(table_cells, dim3((unsigned)(B * P)), dim3(64), (size_t)(S * 24), s, calib, g, slots, (long long)cap, cnt);
  hipLaunchKernelGGL(scan_counts, dim3(B), dim3(1024), 0, s, cnt, (int)P, row_ptr);
  hipLaunchKernelGGL(compact_rows, dim3(wave_blocks(B * P)), dim3(256), 0, s, slots, row_ptr, (int)P, (int)S, B * P,
                     (long long)cap, col, w);
  return bevf_check_launch("bevf_camera_table_build_f64");
}

extern "C" int bevf_camera_table_transpose(const int32_t* row_ptr, const int32_t* col, const float* w, size_t cap, int B,
                                           int P, int ncols, int32_t* t_row_ptr, int32_t* t_col, float* t_w, void* work,
                                           void* stream) {
  BEVF_REQUIRE(row_ptr && col && w && t_row_ptr && t_col && t_w && work, "camera_table_transpose: null pointer");
  BEVF_REQUIRE(B > 0 && P > 0 && ncols > 0 && cap > 0 && cap < ((size_t)1 << 31),
               "camera_table_transpose: bad shape (B=%d P=%d ncols=%d cap=%zu)", B, P, ncols, cap);
  BEVF_REQUIRE((long long)B * P < (1ll << 33) && (long long)B * ncols < (1ll << 33), "camera_table_transpose: too many rows");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int2* tmp = static_cast<int2*>(work);                                 // [B][cap] (forward entry, cell)
  int32_t* tcnt = reinterpret_cast<int32_t*>(tmp + (long long)B * cap);   // [B][ncols]
  const long long rows = (long long)B * P, trows = (long long)B * ncols;
  if (hipMemsetAsync(tcnt, 0, sizeof(int32_t) * (size_t)trows, s) != hipSuccess) {
    bevf_set_error("camera_table_transpose: memset failed");
    return BEVF_ERR_LAUNCH;
  }
  hipLaunchKernelGGL((pixel_pass<false>), dim3(wave_blocks(rows)), dim3(256), 0, s, row_ptr, col, P, ncols, rows,
                     (long long)cap, tcnt, (const int32_t*)nullptr, (int2*)nullptr);
  hipLaunchKernelGGL(scan_counts, dim3(B), dim3(1024), 0, s, tcnt, ncols, t_row_ptr);
  hipLaunchKernelGGL((pixel_pass<true>), dim3(wave_blocks(rows)), dim3(256), 0, s, row_ptr, col, P, ncols, rows,
                     (long long)cap, tcnt, t_row_ptr, tmp);
  hipLaunchKernelGGL(sort_pixel_rows, dim3(wave_blocks(trows)), dim3(256), 0, s, t_row_ptr, tmp, w, ncols, trows,
                     (long long)cap, t_col, t_w);
  return bevf_check_launch("bevf_camera_table_transpose");
}

extern "C" int bevf_csr_gather_frames_f32(const int32_t* row_ptr, size_t rp_stride, const int32_t* col, const float* w,
                                          size_t e_stride, int nrows, const float* x, size_t x_bs, int x_cs, float* y,
                                          size_t y_bs, int y_cs, int B, int C, void* stream) {
  return csr_gather_frames_entry<float>(row_ptr, rp_stride, col, w, e_stride, nrows, x, x_bs, x_cs, y, y_bs, y_cs, B, C,
                                        stream);
}

extern "C" int bevf_csr_gather_frames_bf16(const int32_t* row_ptr, size_t rp_stride, const int32_t* col, const float* w,
                                           size_t e_stride, int nrows, const void* x, size_t x_bs, int x_cs, void* y,
                                           size_t y_bs, int y_cs, int B, int C, void* stream) {
  return csr_gather_frames_entry<__bf16>(row_ptr, rp_stride, col, w, e_stride, nrows, x, x_bs, x_cs, y, y_bs, y_cs, B, C,
                                         stream);
}
