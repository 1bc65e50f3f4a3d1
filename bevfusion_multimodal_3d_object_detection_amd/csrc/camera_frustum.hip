// Lift-splat camera -> BEV view transform of the opt-in `camera_view_transform: 'frustum'` branch (camera_rig.build_frustum_table,
// DESIGN.md 3.2d3; Philion & Fidler 2020, BEVFusion's bev_pool): every (feature pixel, depth bin) is a point of the camera's
// frustum, unprojected through the frame's calibration into the BEV cell it falls in, and
//     y[b][cell][0:C] = sum over the (pix, d) of the cell of Pd[b][pix][d] * x[b][pix][0:C]      (ascending pix * D + d, fp32)
// with Pd the per-pixel softmax over D <= 64 depth bins (camera_lift.hip: softmax_rows).  A frustum is a function of the
// calibration, so the table is per frame by construction; a static rig is the same table built once with B = 1 and applied
// with stride 0.  fp32 only, stream-ordered, nothing allocated, no host synchronisation: capture-safe.
//
//   bevf_frustum_table_build_f64   frustum_inverse   A^-1 and t of every (frame, camera), fp64, one thread each
//                                  frustum_cells     one thread per (pixel, bin): cell_of, and the cell's count (integer atomic)
//                                  scan_counts       row_ptr per frame (scan_counts.h)
//                                  frustum_scatter   col2 into its row at an atomic cursor: any order
//                                  frustum_sort      every row sorted ascending from LDS: the atomics decide nothing that is kept
//   bevf_frustum_pool_f32          csr_gather_frames' shape (one wave per (cell, frame), lanes over the channels in 16-byte vectors,
//                                  EU entries in flight) plus one wave-uniform Pd[b][col2] load per entry
//   bevf_frustum_pool_bwd_f32      dense, no transposed table: one wave per (pixel, frame) walks the pixel's D bins through cell_of
//
// The calibration's third row must equal its depth row (camera_rig.calib_matrices and augment.augmented_calib keep it so: the
// last row of K and of every image map is (0, 0, 1)): the point at depth z of pixel (u, v) is then A^-1 (z (u, v, 1)^T - t).
#include "common.h"
#include "scan_counts.h"

namespace {

struct FrustumGeom {
  double x0, y0, vx, vy, z0, z1, dmin, dmax;
  int bev_w, bev_h, ncam, H, W, Hc, Wc, D;
};

constexpr int SORT_WAVE_ROWS = 512;   // rows up to this length: one wave each, from its quarter of the tile
constexpr int SORT_TILE = 2048;       // keys staged in LDS per pass of a longer row (the whole workgroup sorts it)
constexpr int SORT_KEYS = 4;          // keys a thread ranks per pass of a longer row

// inv [B * ncam][12]: A^-1 row-major, then t.  A singular A gives inf / nan, which frustum_cells reads as "no cell".
__global__ __launch_bounds__(64) void frustum_inverse(const double* __restrict__ calib, int n, double* __restrict__ inv) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= n) return;
  const double* M = calib + (long long)i * 16;
  const double a = M[0], b = M[1], c = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], k = M[10];
  const double c0 = e * k - f * h, c1 = f * g - d * k, c2 = d * h - e * g;
  const double r = 1.0 / (a * c0 + b * c1 + c * c2);
  double* o = inv + (long long)i * 12;
  o[0] = c0 * r, o[1] = (c * h - b * k) * r, o[2] = (b * f - c * e) * r;
  o[3] = c1 * r, o[4] = (a * k - c * g) * r, o[5] = (c * d - a * f) * r;
  o[6] = c2 * r, o[7] = (b * g - a * h) * r, o[8] = (a * e - b * d) * r;
  o[9] = M[3], o[10] = M[7], o[11] = M[11];
}

// One thread per (frame, pixel, bin): its cell (-1: outside the grid or the z range) and the cell's count.
__global__ __launch_bounds__(256) void frustum_cells(const double* __restrict__ inv, FrustumGeom g, long long total, int N,
                                                     int32_t* __restrict__ cell_of, int32_t* __restrict__ cnt) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int b = (int)(t / N), c2 = (int)(t % N);
  const int pix = c2 / g.D, d = c2 % g.D;
  const int hw = g.Hc * g.Wc;
  const int cam = pix / hw, rem = pix % hw;
  const int y = rem / g.Wc, x = rem % g.Wc;
  const double u = (x + 0.5) * g.W / g.Wc - 0.5, v = (y + 0.5) * g.H / g.Hc - 0.5;
  const double z = g.dmin + (d + 0.5) * (g.dmax - g.dmin) / g.D;
  const double* I = inv + ((long long)b * g.ncam + cam) * 12;
  const double r0 = z * u - I[9], r1 = z * v - I[10], r2 = z - I[11];
  const double px = I[0] * r0 + I[1] * r1 + I[2] * r2;
  const double py = I[3] * r0 + I[4] * r1 + I[5] * r2;
  const double pz = I[6] * r0 + I[7] * r1 + I[8] * r2;
  const double fj = floor((px - g.x0) / g.vx), fi = floor((py - g.y0) / g.vy);
  const bool valid = fj >= 0.0 && fj < (double)g.bev_w && fi >= 0.0 && fi < (double)g.bev_h && pz >= g.z0 && pz < g.z1;
  const int P = g.bev_h * g.bev_w;
  const int cell = valid ? (int)fi * g.bev_w + (int)fj : -1;
  cell_of[t] = cell;
  if (valid) atomicAdd(&cnt[(long long)b * P + cell], 1);
}

// One thread per (frame, pixel, bin) with a cell: col2 to an atomic cursor inside the cell's row of tmp (the cursor runs cnt
// back down to 0).
__global__ __launch_bounds__(256) void frustum_scatter(const int32_t* __restrict__ cell_of, const int32_t* __restrict__ rp,
                                                       long long total, int N, int P, int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ tmp) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int cell = cell_of[t];
  if (cell < 0) return;
  const long long b = t / N;
  const int pos = rp[b * (P + 1) + cell] + atomicSub(&cnt[b * P + cell], 1) - 1;
  tmp[b * N + pos] = (int)(t % N);
}

// Four (frame, cell) rows per 256-thread workgroup; the keys of a row are distinct, so a key's place is the count of smaller ones.
// Rows of at most SORT_WAVE_ROWS keys: one wave each, the row staged in the wave's quarter of the tile.  Longer rows: one
// after the other by the whole workgroup, the row streamed through the tile SORT_TILE keys at a time while every thread counts
// for SORT_KEYS keys of its own -- time grows with the square of the row, LDS does not grow at all.
__global__ __launch_bounds__(256) void frustum_sort(const int32_t* __restrict__ rp, const int32_t* __restrict__ tmp, int P,
                                                    long long rows, long long cap, int32_t* __restrict__ col2) {
  __shared__ int tile[SORT_TILE];
  static_assert(SORT_TILE == 4 * SORT_WAVE_ROWS, "a wave sorts a short row from its quarter of the tile");
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  {
    const long long r = (long long)blockIdx.x * 4 + wave;
    int e0 = 0, n = 0;
    long long b = 0;
    if (r < rows) {
      b = r / P;
      const int32_t* fr = rp + b * (P + 1) + (r % P);
      e0 = fr[0], n = fr[1] - e0;
    }
    const bool mine = n <= SORT_WAVE_ROWS;
    int* row = tile + wave * SORT_WAVE_ROWS;
    if (mine)
      for (int i = lane; i < n; i += 64) row[i] = tmp[b * cap + e0 + i];
    __syncthreads();
    if (mine)
      for (int i = lane; i < n; i += 64) {
        const int key = row[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += row[j] < key ? 1 : 0;
        col2[b * cap + e0 + rank] = key;
      }
  }
  for (int w = 0; w < 4; ++w) {                      // everything below is uniform over the workgroup
    const long long r = (long long)blockIdx.x * 4 + w;
    if (r >= rows) break;
    const long long b = r / P;
    const int32_t* fr = rp + b * (P + 1) + (r % P);
    const int e0 = fr[0], n = fr[1] - e0;
    if (n <= SORT_WAVE_ROWS) continue;
    const int32_t* src = tmp + b * cap + e0;
    int32_t* dst = col2 + b * cap + e0;
    for (int i0 = 0; i0 < n; i0 += 256 * SORT_KEYS) {
      int key[SORT_KEYS], rank[SORT_KEYS];
#pragma unroll
      for (int k = 0; k < SORT_KEYS; ++k) {
        const int i = i0 + k * 256 + tid;
        key[k] = i < n ? src[i] : 0;
        rank[k] = 0;
      }
      for (int t0 = 0; t0 < n; t0 += SORT_TILE) {
        const int m = n - t0 < SORT_TILE ? n - t0 : SORT_TILE;
        __syncthreads();                             // the tile's previous keys have been read by every thread
        for (int j = tid; j < m; j += 256) tile[j] = src[t0 + j];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
          const int v = tile[j];
#pragma unroll
          for (int k = 0; k < SORT_KEYS; ++k) rank[k] += v < key[k] ? 1 : 0;
        }
      }
#pragma unroll
      for (int k = 0; k < SORT_KEYS; ++k)
        if (i0 + k * 256 + tid < n) dst[rank[k]] = key[k];
    }
  }
}

constexpr int EU = 4;              // entries in flight per pass over a row
constexpr int UB = 4;              // bins in flight per pass over a pixel (backward)
constexpr int ROWS_PER_BLOCK = 4;  // one row per wave, 256 threads

template <int KV>
__global__ __launch_bounds__(256) void frustum_pool(const int32_t* __restrict__ row_ptr, long long rp_stride,
                                                    const int32_t* __restrict__ col2, long long e_stride, int nrows,
                                                    unsigned dmul, unsigned dsh, const float* __restrict__ x, long long x_bs,
                                                    int x_cs, const float* __restrict__ pd, long long pd_bs,
                                                    float* __restrict__ y, long long y_bs, int y_cs, int C) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r = xcd_remap((int)blockIdx.x, (int)gridDim.x) * ROWS_PER_BLOCK + wave;
  if (r >= nrows) return;
  const long long b = (long long)blockIdx.y;
  const int32_t* rp = row_ptr + b * rp_stride;
  const int32_t* cl = col2 + b * e_stride;
  const float* xb = x + b * x_bs;
  const float* pdb = pd + b * pd_bs;
  const int e0 = rp[r], e1 = rp[r + 1];
  const int cv = C / 4;
  float acc[KV][4];
#pragma unroll
  for (int k = 0; k < KV; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[k][q] = 0.f;
  for (int e = e0; e < e1; e += EU) {
    float v[EU][KV][4];
    float s[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      s[u] = 0.f;
      if (e + u < e1) {
        const int c2 = cl[e + u];
        s[u] = pdb[c2];
        const float* src = xb + (long long)div_by(c2, dmul, dsh) * x_cs;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          const int j = lane + 64 * k;
          if (j < cv) load16(src + j * 4, v[u][k]);
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
            for (int q = 0; q < 4; ++q) acc[k][q] = fmaf(s[u], v[u][k][q], acc[k][q]);
          }
        }
      }
    }
  }
  float* dst = y + b * y_bs + (long long)r * y_cs;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int j = lane + 64 * k;
    if (j < cv) store16(dst + j * 4, acc[k]);
  }
}

template <int KV>
__global__ __launch_bounds__(256) void frustum_pool_bwd(const int32_t* __restrict__ cell_of, long long c_stride, int npix, int D,
                                                        const float* __restrict__ x, long long x_bs, int x_cs,
                                                        const float* __restrict__ pd, long long pd_bs,
                                                        const float* __restrict__ dy, long long dy_bs, int dy_cs,
                                                        float* __restrict__ dx, long long dx_bs, int dx_cs,
                                                        float* __restrict__ dpd, long long dpd_bs, int C) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int pix = xcd_remap((int)blockIdx.x, (int)gridDim.x) * ROWS_PER_BLOCK + wave;
  if (pix >= npix) return;
  const long long b = (long long)blockIdx.y;
  const int cv = C / 4;
  float xv[KV][4], acc[KV][4];
  const float* xs = x + b * x_bs + (long long)pix * x_cs;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int j = lane + 64 * k;
#pragma unroll
    for (int q = 0; q < 4; ++q) xv[k][q] = acc[k][q] = 0.f;
    if (j < cv) load16(xs + j * 4, xv[k]);
  }
  const int32_t* co = cell_of + b * c_stride + (long long)pix * D;
  const float* pdr = pd + b * pd_bs + (long long)pix * D;
  const float* dyb = dy + b * dy_bs;
  float bin_acc = 0.f;                                          // lane d: dPd[b][pix][d]
  for (int d0 = 0; d0 < D; d0 += UB) {
    float v[UB][KV][4];
    int cell[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      cell[u] = d0 + u < D ? co[d0 + u] : -1;
      if (cell[u] >= 0) {
        const float* src = dyb + (long long)cell[u] * dy_cs;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          const int j = lane + 64 * k;
          if (j < cv) load16(src + j * 4, v[u][k]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      if (cell[u] >= 0) {
        const float s = pdr[d0 + u];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          if (lane + 64 * k < cv) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              acc[k][q] = fmaf(s, v[u][k][q], acc[k][q]);
              dot = fmaf(xv[k][q], v[u][k][q], dot);
            }
          }
        }
        dot = group_reduce<false>(dot, 64);
        if (lane == d0 + u) bin_acc = dot;
      }
    }
  }
  float* dst = dx + b * dx_bs + (long long)pix * dx_cs;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int j = lane + 64 * k;
    if (j < cv) store16(dst + j * 4, acc[k]);
  }
  if (lane < D) dpd[b * dpd_bs + (long long)pix * D + lane] = bin_acc;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

bool pool_shape_ok(int nrows, int D, int B, int C) {
  return nrows > 0 && D >= 1 && D <= 64 && B > 0 && B <= 65535 && C > 0 && C % 4 == 0 && C / 4 <= 256;
}

}  // namespace

extern "C" int bevf_frustum_table_sort_wave_rows(void) { return SORT_WAVE_ROWS; }

extern "C" size_t bevf_frustum_table_work_elems(int B, int ncam, int bev_h, int bev_w, int D, int Hc, int Wc) {
  if (B <= 0 || ncam <= 0 || bev_h <= 0 || bev_w <= 0 || D <= 0 || Hc <= 0 || Wc <= 0) return 0;
  const size_t b = (size_t)B;
  return b * (size_t)ncam * 24 + b * (size_t)ncam * (size_t)Hc * (size_t)Wc * (size_t)D + b * (size_t)bev_h * (size_t)bev_w;
}

extern "C" int bevf_frustum_table_build_f64(const double* calib, int B, int ncam, float x0, float y0, float vx, float vy,
                                            int bev_h, int bev_w, float z0, float z1, int D, double depth_min, double depth_max,
                                            int img_h, int img_w, int Hc, int Wc, int32_t* cell_of, int32_t* row_ptr,
                                            int32_t* col2, void* work, void* stream) {
  BEVF_REQUIRE(calib && cell_of && row_ptr && col2 && work, "frustum_table_build: null pointer");
  BEVF_REQUIRE(B > 0 && ncam > 0 && bev_h > 0 && bev_w > 0 && img_h > 0 && img_w > 0 && Hc > 0 && Wc > 0,
               "frustum_table_build: bad shape");
  BEVF_REQUIRE(D >= 1 && D <= 64 && depth_min > 0.0 && depth_min < depth_max, "frustum_table_build: bad depth bins (D=%d, %g..%g)", D,
               depth_min, depth_max);
  BEVF_REQUIRE(vx > 0.f && vy > 0.f && z0 < z1, "frustum_table_build: bad grid");
  BEVF_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, "frustum_table_build: work must be 8-byte aligned");
  const long long P = (long long)bev_h * bev_w, N = (long long)ncam * Hc * Wc * D, total = (long long)B * N;
  BEVF_REQUIRE(N < (1ll << 31) && P < (1ll << 31) && (long long)B * ncam < (1ll << 31) && (long long)B * P < (1ll << 33) &&
                   total < (1ll << 38),
               "frustum_table_build: table too large for int32 indices");
  FrustumGeom g;
  g.x0 = x0, g.y0 = y0, g.vx = vx, g.vy = vy, g.z0 = z0, g.z1 = z1, g.dmin = depth_min, g.dmax = depth_max;
  g.bev_w = bev_w, g.bev_h = bev_h, g.ncam = ncam, g.H = img_h, g.W = img_w, g.Hc = Hc, g.Wc = Wc, g.D = D;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* inv = static_cast<double*>(work);                                // [B][ncam][12]
  int32_t* tmp = reinterpret_cast<int32_t*>(inv + (long long)B * ncam * 12);  // [B][N] col2 in cursor order
  int32_t* cnt = tmp + total;                                               // [B][P]
  if (hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)(B * P), s) != hipSuccess) {
    bevf_set_error("frustum_table_build: memset failed");
    return BEVF_ERR_LAUNCH;
  }
  const char* name = "bevf_frustum_table_build_f64";
  int rc = bevf_launch(name, frustum_inverse, dim3(blocks_of((long long)B * ncam, 64)), dim3(64), 0, s, calib, B * ncam, inv);
  if (rc != BEVF_OK) return rc;
  rc = bevf_launch(name, frustum_cells, dim3(blocks_of(total, 256)), dim3(256), 0, s, (const double*)inv, g, total, (int)N, cell_of,
                   cnt);
  if (rc != BEVF_OK) return rc;
  rc = bevf_launch(name, scan_counts, dim3(B), dim3(1024), 0, s, (const int32_t*)cnt, (int)P, row_ptr);
  if (rc != BEVF_OK) return rc;
  rc = bevf_launch(name, frustum_scatter, dim3(blocks_of(total, 256)), dim3(256), 0, s, (const int32_t*)cell_of,
                   (const int32_t*)row_ptr, total, (int)N, (int)P, cnt, tmp);
  if (rc != BEVF_OK) return rc;
  return bevf_launch(name, frustum_sort, dim3(blocks_of((long long)B * P, 4)), dim3(256), 0, s, (const int32_t*)row_ptr,
                     (const int32_t*)tmp, (int)P, (long long)B * P, N, col2);
}

extern "C" int bevf_frustum_pool_f32(const int32_t* row_ptr, size_t rp_stride, const int32_t* col2, size_t e_stride, int nrows,
                                     int D, const float* x, size_t x_bs, int x_cs, const float* pd, size_t pd_bs, float* y,
                                     size_t y_bs, int y_cs, int B, int C, void* stream) {
  BEVF_REQUIRE(row_ptr && col2 && x && pd && y, "frustum_pool: null pointer");
  BEVF_REQUIRE(pool_shape_ok(nrows, D, B, C),
               "frustum_pool: bad shape (nrows=%d D=%d B=%d C=%d; C a multiple of 4, at most 1024, D <= 64, B <= 65535)", nrows, D, B, C);
  BEVF_REQUIRE(rp_stride == 0 || rp_stride >= (size_t)nrows + 1, "frustum_pool: row_ptr stride must be 0 (shared) or >= nrows + 1");
  BEVF_REQUIRE(x_cs >= C && y_cs >= C && x_cs % 4 == 0 && y_cs % 4 == 0 && x_bs % 4 == 0 && y_bs % 4 == 0,
               "frustum_pool: strides must be 16-byte multiples and channel strides >= C");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(y), "frustum_pool: unaligned feature buffer");
  const dim3 grid((nrows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, B), block(64 * ROWS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned dmul, dsh;
  div_make(D, &dmul, &dsh);
  const int cv = C / 4;
#define BEVF_FRUSTUM_POOL(KV)                                                                                               \
  return bevf_launch("bevf_frustum_pool_f32", frustum_pool<KV>, grid, block, 0, s, row_ptr, (long long)rp_stride, col2,     \
                     (long long)e_stride, nrows, dmul, dsh, x, (long long)x_bs, x_cs, pd, (long long)pd_bs, y, (long long)y_bs, \
                     y_cs, C)
  if (cv <= 64) BEVF_FRUSTUM_POOL(1);
  if (cv <= 128) BEVF_FRUSTUM_POOL(2);
  BEVF_FRUSTUM_POOL(4);
#undef BEVF_FRUSTUM_POOL
}

extern "C" int bevf_frustum_pool_bwd_f32(const int32_t* cell_of, size_t c_stride, int npix, int D, const float* x, size_t x_bs,
                                         int x_cs, const float* pd, size_t pd_bs, const float* dy, size_t dy_bs, int dy_cs,
                                         float* dx, size_t dx_bs, int dx_cs, float* dpd, size_t dpd_bs, int B, int C,
                                         void* stream) {
  BEVF_REQUIRE(cell_of && x && pd && dy && dx && dpd, "frustum_pool_bwd: null pointer");
  BEVF_REQUIRE(pool_shape_ok(npix, D, B, C),
               "frustum_pool_bwd: bad shape (npix=%d D=%d B=%d C=%d; C a multiple of 4, at most 1024, D <= 64, B <= 65535)", npix, D, B,
               C);
  BEVF_REQUIRE(c_stride == 0 || c_stride >= (size_t)npix * (size_t)D, "frustum_pool_bwd: cell stride must be 0 (shared) or >= npix * D");
  BEVF_REQUIRE(x_cs >= C && dy_cs >= C && dx_cs >= C && x_cs % 4 == 0 && dy_cs % 4 == 0 && dx_cs % 4 == 0 && x_bs % 4 == 0 &&
                   dy_bs % 4 == 0 && dx_bs % 4 == 0,
               "frustum_pool_bwd: strides must be 16-byte multiples and channel strides >= C");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(dy) && bevf_aligned16(dx), "frustum_pool_bwd: unaligned feature buffer");
  const dim3 grid((npix + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, B), block(64 * ROWS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cv = C / 4;
#define BEVF_FRUSTUM_BWD(KV)                                                                                                \
  return bevf_launch("bevf_frustum_pool_bwd_f32", frustum_pool_bwd<KV>, grid, block, 0, s, cell_of, (long long)c_stride, npix, D, \
                     x, (long long)x_bs, x_cs, pd, (long long)pd_bs, dy, (long long)dy_bs, dy_cs, dx, (long long)dx_bs, dx_cs, dpd, \
                     (long long)dpd_bs, C)
  if (cv <= 64) BEVF_FRUSTUM_BWD(1);
  if (cv <= 128) BEVF_FRUSTUM_BWD(2);
  BEVF_FRUSTUM_BWD(4);
#undef BEVF_FRUSTUM_BWD
}
