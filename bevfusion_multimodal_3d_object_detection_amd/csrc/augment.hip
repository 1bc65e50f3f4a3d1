// Training augmentation on the device: one world transform per frame, one image transform per camera.
//
// resample_tables_box: Pillow's bilinear coefficient tables for an integer crop window per image, the fp64 operations of
//   preprocess.resample_tables in the same order (center starts at the window's first column, scale = window / out); one thread per
//   output index, no fused multiply-add (contraction is off for this file), so the tables are bit-equal to the host restatement.
// resize_crop_u8: Pillow's two integer passes (preprocess.hip) with those per-image tables -> the resized uint8 image, plus the sum of
//   Pillow's gray value per image (integer atomics: order-independent).
// jitter_flip_normalize_u8: contrast, brightness, saturation, hue (torchvision's float formulas, this fixed order), horizontal flip as
//   a reversed store column, then ToTensor / Normalize with the operations of resize_normalize_u8.
// points_affine_filter_pad: p' = M p + t per frame, then the strict range filter, the order-preserving compaction and the zero padding
//   of lidar_filter_pad, all frames in one launch (blockIdx.y = frame).  points_affine: the transform alone, in place (radar).
//   boxes_affine: centres, sizes, headings and velocities of the ground-truth boxes.
//
// The affine map, everywhere in this file (m = one frame's 12 floats, row-major 3 x 4):
//   x' = fmaf(m[2], z, fmaf(m[1], y, fmaf(m[0], x, m[3])))     (three fused roundings per coordinate: x term, then y, then z)
//   y' = fmaf(m[6], z, fmaf(m[5], y, fmaf(m[4], x, m[7])))
//   z' = fmaf(m[10], z, fmaf(m[9], y, fmaf(m[8], x, m[11])))
// and a planar vector (velocity, heading): vx' = fmaf(m[1], vy, m[0] * vx), vy' = fmaf(m[5], vy, m[4] * vx).
// A frame whose 12 floats are exactly the identity is copied, not multiplied (block-uniform branch): its output has the input's bits.
#include "common.h"
#include "point_compact.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPrec = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
  v >>= kPrec;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- coefficient tables ------------------------------------------------------------------------------------------------------------
// win [n][4] = (x0, x1, y0, y1); axis 0: columns (in_size W, window x0..x1, out Wo), axis 1: rows.  bounds [n][out][2], coef [n][out][ks].
__global__ __launch_bounds__(256) void resample_tables_box(const int* __restrict__ win, int n, int axis, int in_size, int out_size, int ks,
                                                            int* __restrict__ bounds, int* __restrict__ coef) {
  const int xx = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  if (xx >= out_size || img >= n) return;
  const int in0 = win[4 * img + 2 * axis], in1 = win[4 * img + 2 * axis + 1];
  const double scale = (double)(in1 - in0) / (double)out_size;
  const double filterscale = scale >= 1.0 ? scale : 1.0;
  const double support = 1.0 * filterscale;
  const double ss = 1.0 / filterscale;
  const double center = (double)in0 + ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > ks) xmax = ks;                                          // never taken when ks covers the window (checked on the host)
  if (xmax < 0) xmax = 0;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double t = ((double)(x + xmin) - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    ww += t < 1.0 ? 1.0 - t : 0.0;
  }
  int* const k = coef + ((size_t)img * out_size + xx) * ks;
  for (int x = 0; x < ks; ++x) {
    int c = 0;
    if (x < xmax) {
      double t = ((double)(x + xmin) - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      const double w = t < 1.0 ? 1.0 - t : 0.0;
      const double v = ww != 0.0 ? w / ww : w;
      c = v < 0 ? (int)(-0.5 + v * (double)(1 << kPrec)) : (int)(0.5 + v * (double)(1 << kPrec));
    }
    k[x] = c;
  }
  bounds[((size_t)img * out_size + xx) * 2] = xmin;
  bounds[((size_t)img * out_size + xx) * 2 + 1] = xmax;
}

// ---- resize -------------------------------------------------------------------------------------------------------------------------
// A workgroup owns RT output rows x 64 output columns of one image (preprocess.hip's tiled form).  The input rows a tile needs depend
// on that image's window: a tile that needs more than RMAX rows (block-uniform) takes the per-pixel form instead of the LDS tile.
constexpr int RT = 16, CT_ = 64, RMAX = 48;

__global__ __launch_bounds__(256) void resize_crop_u8(const unsigned char* __restrict__ x, unsigned char* __restrict__ out,
                                                       unsigned long long* __restrict__ gray_sum, int H, int W, int Ho, int Wo,
                                                       const int* __restrict__ bh_, const int* __restrict__ kh_, int ksh,
                                                       const int* __restrict__ bv_, const int* __restrict__ kv_, int ksv, int tilesX) {
  __shared__ unsigned char hbuf[RMAX][CT_][4];
  __shared__ unsigned int gsum[4];
  const int tid = threadIdx.x, img = blockIdx.z;
  const int tx = blockIdx.x, ty = blockIdx.y;
  (void)tilesX;
  const int* const bh = bh_ + (size_t)img * Wo * 2;
  const int* const kh = kh_ + (size_t)img * Wo * ksh;
  const int* const bv = bv_ + (size_t)img * Ho * 2;
  const int* const kv = kv_ + (size_t)img * Ho * ksv;
  const int ox0 = tx * CT_, oy0 = ty * RT;
  const int oy1 = (oy0 + RT < Ho ? oy0 + RT : Ho) - 1;
  const int r0 = bv[2 * oy0], r1 = bv[2 * oy1] + bv[2 * oy1 + 1];
  const int nr = r1 - r0;
  const bool tiled = nr <= RMAX;                                     // the same in every thread of the workgroup
  const unsigned char* const base = x + (size_t)img * H * W * 3;
  if (tiled) {
    const int c = tid & (CT_ - 1), rq = tid >> 6;
    const int ox = ox0 + c;
    if (ox < Wo) {
      const int x0 = bh[2 * ox], nx = bh[2 * ox + 1];
      const int* const kx = kh + (size_t)ox * ksh;
      for (int r = rq; r < nr; r += 4) {
        const unsigned char* row = base + ((size_t)(r0 + r) * W + x0) * 3;
        int h0 = 1 << (kPrec - 1), h1 = h0, h2 = h0;
        for (int t = 0; t < nx; ++t) {
          const int k = kx[t];
          h0 += (int)row[3 * t] * k;
          h1 += (int)row[3 * t + 1] * k;
          h2 += (int)row[3 * t + 2] * k;
        }
        hbuf[r][c][0] = (unsigned char)clip8(h0);
        hbuf[r][c][1] = (unsigned char)clip8(h1);
        hbuf[r][c][2] = (unsigned char)clip8(h2);
      }
    }
  }
  __syncthreads();
  unsigned int gray = 0;
  for (int e = tid; e < RT * CT_; e += 256) {
    const int c = e & (CT_ - 1), ry = e >> 6;
    const int ox = ox0 + c, oy = oy0 + ry;
    if (ox >= Wo || oy >= Ho) continue;
    const int y0 = bv[2 * oy], ny = bv[2 * oy + 1];
    const int* const ky = kv + (size_t)oy * ksv;
    int v0 = 1 << (kPrec - 1), v1 = v0, v2 = v0;
    if (tiled) {
      for (int j = 0; j < ny; ++j) {
        const int k = ky[j];
        v0 += (int)hbuf[y0 - r0 + j][c][0] * k;
        v1 += (int)hbuf[y0 - r0 + j][c][1] * k;
        v2 += (int)hbuf[y0 - r0 + j][c][2] * k;
      }
    } else {
      const int x0 = bh[2 * ox], nx = bh[2 * ox + 1];
      const int* const kx = kh + (size_t)ox * ksh;
      for (int j = 0; j < ny; ++j) {
        const unsigned char* row = base + ((size_t)(y0 + j) * W + x0) * 3;
        int h0 = 1 << (kPrec - 1), h1 = h0, h2 = h0;
        for (int t = 0; t < nx; ++t) {
          const int k = kx[t];
          h0 += (int)row[3 * t] * k;
          h1 += (int)row[3 * t + 1] * k;
          h2 += (int)row[3 * t + 2] * k;
        }
        const int k = ky[j];
        v0 += clip8(h0) * k;
        v1 += clip8(h1) * k;
        v2 += clip8(h2) * k;
      }
    }
    const int R = clip8(v0), G = clip8(v1), B = clip8(v2);
    unsigned char* const o = out + (((size_t)img * Ho + oy) * Wo + ox) * 3;
    o[0] = (unsigned char)R;
    o[1] = (unsigned char)G;
    o[2] = (unsigned char)B;
    gray += (unsigned int)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);   // Pillow's RGB -> L
  }
  for (int o = 32; o > 0; o >>= 1) gray += __shfl_xor(gray, o);                  // <= 1024 * 255 per workgroup
  if ((tid & 63) == 0) gsum[tid >> 6] = gray;
  __syncthreads();
  if (tid == 0) atomicAdd(gray_sum + img, (unsigned long long)(gsum[0] + gsum[1] + gsum[2] + gsum[3]));
}

// ---- photometric jitter, flip, normalise -------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// jit [n][4] = (contrast, brightness, saturation, hue shift); grid (ceil(Ho*Wo / 256), n): the factors are uniform in a workgroup
__global__ __launch_bounds__(256) void jitter_flip_normalize_u8(const unsigned char* __restrict__ x, float* __restrict__ out,
                                                                 const unsigned long long* __restrict__ gray_sum,
                                                                 const float* __restrict__ jit, const int* __restrict__ flip, int Ho,
                                                                 int Wo, float m0, float m1, float m2, float s0, float s1, float s2) {
  const int img = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int plane = Ho * Wo;
  if (p >= plane) return;
  const int oy = p / Wo, ox = p - oy * Wo;
  const unsigned char* const px = x + ((size_t)img * plane + p) * 3;
  float r = __fdiv_rn((float)px[0], 255.f), g = __fdiv_rn((float)px[1], 255.f), b = __fdiv_rn((float)px[2], 255.f);
  const float fc = jit[4 * img], fb = jit[4 * img + 1], fs = jit[4 * img + 2], dh = jit[4 * img + 3];
  if (fc != 1.f) {
    const float m = (float)((double)gray_sum[img] / (double)plane / 255.0);
    const float om = (1.f - fc) * m;
    r = clamp01(fc * r + om);
    g = clamp01(fc * g + om);
    b = clamp01(fc * b + om);
  }
  if (fb != 1.f) {
    r = clamp01(fb * r);
    g = clamp01(fb * g);
    b = clamp01(fb * b);
  }
  if (fs != 1.f) {
    const float gr = 0.299f * r + 0.587f * g + 0.114f * b;
    const float og = (1.f - fs) * gr;
    r = clamp01(fs * r + og);
    g = clamp01(fs * g + og);
    b = clamp01(fs * b + og);
  }
  if (dh != 0.f) {                                                   // torchvision's _rgb2hsv / _hsv2rgb
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float crd = eqc ? 1.f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = 2.f + rc - bc;
    else h = 4.f + gc - rc;
    h = h / 6.f + 1.f;
    h = h - floorf(h);                                               // fmod(h, 1) of a positive number
    h = h + dh;
    h = h - floorf(h);                                               // Python's % 1
    const float v = maxc;
    const float h6 = h * 6.f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    int i = (int)fl % 6;
    const float pp = clamp01(v * (1.f - s));
    const float q = clamp01(v * (1.f - s * f));
    const float t = clamp01(v * (1.f - s * (1.f - f)));
    r = i == 0 ? v : i == 1 ? q : i == 2 ? pp : i == 3 ? pp : i == 4 ? t : v;
    g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? pp : pp;
    b = i == 0 ? pp : i == 1 ? pp : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
  }
  const int sx = flip[img] ? Wo - 1 - ox : ox;
  float* const o = out + (size_t)img * 3 * plane + (size_t)oy * Wo + sx;
  o[0] = __fdiv_rn(__fsub_rn(r, m0), s0);
  o[plane] = __fdiv_rn(__fsub_rn(g, m1), s1);
  o[2 * (size_t)plane] = __fdiv_rn(__fsub_rn(b, m2), s2);
}

// ---- points ---------------------------------------------------------------------------------------------------------------------------
struct Affine {
  float m[12];
  bool identity;
};
__device__ __forceinline__ Affine load_affine(const float* __restrict__ mat, int b) {
  Affine a;
  bool id = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    a.m[i] = mat[12 * b + i];
    id = id && a.m[i] == ((i == 0 || i == 5 || i == 10) ? 1.f : 0.f);
  }
  a.identity = id;
  return a;
}
__device__ __forceinline__ void affine_point(const Affine& a, float& x, float& y, float& z) {
  if (a.identity) return;
  const float nx = fmaf(a.m[2], z, fmaf(a.m[1], y, fmaf(a.m[0], x, a.m[3])));
  const float ny = fmaf(a.m[6], z, fmaf(a.m[5], y, fmaf(a.m[4], x, a.m[7])));
  const float nz = fmaf(a.m[10], z, fmaf(a.m[9], y, fmaf(a.m[8], x, a.m[11])));
  x = nx, y = ny, z = nz;
}
__device__ __forceinline__ void affine_planar(const Affine& a, float& vx, float& vy) {
  if (a.identity) return;
  const float nx = fmaf(a.m[1], vy, a.m[0] * vx);
  const float ny = fmaf(a.m[5], vy, a.m[4] * vx);
  vx = nx, vy = ny;
}

// The compaction's stages are point_compact.h's; here are the keep rule and the store.
__device__ __forceinline__ bool paf_keep(const float* __restrict__ pts, int i, int n, int C, const Affine& a, const Range6& r, float& px,
                                         float& py, float& pz) {
  if (i >= n) return false;
  px = pts[(size_t)i * C], py = pts[(size_t)i * C + 1], pz = pts[(size_t)i * C + 2];
  affine_point(a, px, py, pz);
  return in_range(r, px, py, pz);
}
// grid (tiles, B); tcount [B][tiles]
__global__ __launch_bounds__(PC_TILE) void paf_count(const float* __restrict__ pts, const int* __restrict__ n_in,
                                                     const float* __restrict__ mat, int* __restrict__ tcount, int N, int C, Range6 rg) {
  const int b = blockIdx.y;
  const Affine a = load_affine(mat, b);
  float px, py, pz;
  tile_count(paf_keep(pts + (size_t)b * N * C, blockIdx.x * PC_TILE + threadIdx.x, frame_rows(n_in, b, N), C, a, rg, px, py, pz),
             tcount + (size_t)b * gridDim.x + blockIdx.x);
}
// work [B][N][C]: the frame's survivors, transformed, in point order; count [B]
__global__ __launch_bounds__(PC_TILE) void paf_compact(const float* __restrict__ pts, const int* __restrict__ n_in,
                                                       const float* __restrict__ mat, float* __restrict__ work,
                                                       const int* __restrict__ tcount, int* __restrict__ count, int N, int C, int vc0,
                                                       int vc1, Range6 rg) {
  const int t = blockIdx.x, b = blockIdx.y, i = t * PC_TILE + threadIdx.x;
  const Affine a = load_affine(mat, b);
  const float* const fp = pts + (size_t)b * N * C;
  float px = 0.f, py = 0.f, pz = 0.f;
  const bool keep = paf_keep(fp, i, frame_rows(n_in, b, N), C, a, rg, px, py, pz);
  const int start = tiles_before(tcount + (size_t)b * gridDim.x, t);
  const TileRank r = tile_rank(keep, start);
  if (keep) {                                                        // r.row < n <= N: inside the frame's work rows
    float* dst = work + ((size_t)b * N + r.row) * C;
    dst[0] = px, dst[1] = py, dst[2] = pz;
    for (int c = 3; c < C; ++c) dst[c] = fp[(size_t)i * C + c];
    if (vc0 >= 0) {
      float vx = fp[(size_t)i * C + vc0], vy = fp[(size_t)i * C + vc1];
      affine_planar(a, vx, vy);
      dst[vc0] = vx, dst[vc1] = vy;
    }
  }
  if (threadIdx.x == 0 && t == (int)gridDim.x - 1) count[b] = start + r.total;
}

// in place: points [B][N][C]; noise [B][N][3] (or null) scaled by noise_std onto channels 0-2 after the transform
__global__ __launch_bounds__(256) void points_affine(float* __restrict__ pts, const float* __restrict__ mat, const float* __restrict__ noise,
                                                     float noise_std, int N, int C, int vc0, int vc1) {
  const int b = blockIdx.y;
  const Affine a = load_affine(mat, b);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
    float* const p = pts + ((size_t)b * N + i) * C;
    float x = p[0], y = p[1], z = p[2];
    affine_point(a, x, y, z);
    if (noise) {
      const float* const nz = noise + ((size_t)b * N + i) * 3;
      x = fmaf(noise_std, nz[0], x), y = fmaf(noise_std, nz[1], y), z = fmaf(noise_std, nz[2], z);
    }
    if (!a.identity || noise) p[0] = x, p[1] = y, p[2] = z;
    if (vc0 >= 0 && !a.identity) {
      float vx = p[vc0], vy = p[vc1];
      affine_planar(a, vx, vy);
      p[vc0] = vx, p[vc1] = vy;
    }
  }
}

// in place: boxes [B][M][ncol] (ncol 7 or 9), labels [B][M] (< 0: padding row, untouched), vel [B][M][2] or null, scale [B]
__global__ __launch_bounds__(256) void boxes_affine(float* __restrict__ boxes, const long long* __restrict__ labels, float* __restrict__ vel,
                                                    const float* __restrict__ mat, const float* __restrict__ scale, int M, int ncol) {
  const int b = blockIdx.y;
  const Affine a = load_affine(mat, b);
  if (a.identity) return;
  const float s = scale[b];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
    if (labels[(size_t)b * M + i] < 0) continue;
    float* const q = boxes + ((size_t)b * M + i) * ncol;
    float x = q[0], y = q[1], z = q[2];
    affine_point(a, x, y, z);
    q[0] = x, q[1] = y, q[2] = z;
    q[3] *= s, q[4] *= s, q[5] *= s;
    float hx, hy;
    sincosf(q[6], &hy, &hx);
    affine_planar(a, hx, hy);
    q[6] = atan2f(hy, hx);
    if (ncol == 9) {
      float vx = q[7], vy = q[8];
      affine_planar(a, vx, vy);
      q[7] = vx, q[8] = vy;
    }
    if (vel) {
      float vx = vel[((size_t)b * M + i) * 2], vy = vel[((size_t)b * M + i) * 2 + 1];
      affine_planar(a, vx, vy);
      vel[((size_t)b * M + i) * 2] = vx, vel[((size_t)b * M + i) * 2 + 1] = vy;
    }
  }
}

}  // namespace

extern "C" int bevf_resample_tables_box_f64(const int32_t* windows, int n, int H, int W, int Ho, int Wo, int ksize_h, int ksize_v,
                                            int32_t* bounds_h, int32_t* coef_h, int32_t* bounds_v, int32_t* coef_v, void* stream) {
  BEVF_REQUIRE(windows && bounds_h && coef_h && bounds_v && coef_v, "resample_tables_box: null pointer");
  BEVF_REQUIRE(n > 0 && n < 65536 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && ksize_h >= 3 && ksize_v >= 3, "resample_tables_box: bad shape");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(resample_tables_box, dim3((Wo + 255) / 256, n), dim3(256), 0, st, windows, n, 0, W, Wo, ksize_h, bounds_h, coef_h);
  hipLaunchKernelGGL(resample_tables_box, dim3((Ho + 255) / 256, n), dim3(256), 0, st, windows, n, 1, H, Ho, ksize_v, bounds_v, coef_v);
  return bevf_check_launch("bevf_resample_tables_box_f64");
}

extern "C" int bevf_resize_crop_u8(const unsigned char* x, unsigned char* out, uint64_t* gray_sum, int n, int H, int W, int Ho, int Wo,
                                   const int32_t* bounds_h, const int32_t* coef_h, int ksize_h, const int32_t* bounds_v,
                                   const int32_t* coef_v, int ksize_v, void* stream) {
  BEVF_REQUIRE(x && out && gray_sum && bounds_h && coef_h && bounds_v && coef_v, "resize_crop: null pointer");
  BEVF_REQUIRE(n > 0 && n < 65536 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && ksize_h > 0 && ksize_v > 0, "resize_crop: bad shape");
  const int tilesX = (Wo + CT_ - 1) / CT_, tilesY = (Ho + RT - 1) / RT;
  BEVF_REQUIRE(tilesY < 65536, "resize_crop: output too tall");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(gray_sum, 0, sizeof(uint64_t) * (size_t)n, st) != hipSuccess) return bevf_check_launch("bevf_resize_crop_u8");
  hipLaunchKernelGGL(resize_crop_u8, dim3(tilesX, tilesY, n), dim3(256), 0, st, x, out, reinterpret_cast<unsigned long long*>(gray_sum), H, W,
                     Ho, Wo, bounds_h, coef_h, ksize_h, bounds_v, coef_v, ksize_v, tilesX);
  return bevf_check_launch("bevf_resize_crop_u8");
}

extern "C" int bevf_jitter_flip_normalize_u8(const unsigned char* x, float* out, const uint64_t* gray_sum, const float* jitter4,
                                             const int32_t* flip, int n, int Ho, int Wo, const float* mean3, const float* std3,
                                             void* stream) {
  BEVF_REQUIRE(x && out && gray_sum && jitter4 && flip && mean3 && std3, "jitter_flip_normalize: null pointer");
  BEVF_REQUIRE(n > 0 && n < 65536 && Ho > 0 && Wo > 0 && (long long)Ho * Wo < (1ll << 30), "jitter_flip_normalize: bad shape");
  BEVF_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "jitter_flip_normalize: zero std");
  hipLaunchKernelGGL(jitter_flip_normalize_u8, dim3((Ho * Wo + 255) / 256, n), dim3(256), 0, static_cast<hipStream_t>(stream), x, out,
                     reinterpret_cast<const unsigned long long*>(gray_sum), jitter4, flip, Ho, Wo, mean3[0], mean3[1], mean3[2], std3[0],
                     std3[1], std3[2]);
  return bevf_check_launch("bevf_jitter_flip_normalize_u8");
}

extern "C" size_t bevf_points_affine_work_floats(int B, int N, int C) {
  if (B <= 0 || N < 0 || C <= 0) return 0;
  return (size_t)B * ((size_t)N * C + (size_t)point_tiles(N)) + 64;
}

extern "C" int bevf_points_affine_filter_pad_f32(const float* points, const int32_t* n_in, const float* mat12, float* out, int32_t* count,
                                                 float* work, int B, int N, int C, int max_points, int vel_c0, int vel_c1,
                                                 const float* pc_range6, void* stream) {
  BEVF_REQUIRE((points || N == 0) && mat12 && out && count && work && pc_range6, "points_affine_filter_pad: null pointer");
  BEVF_REQUIRE(B > 0 && B < 65536 && N >= 0 && C >= 3 && max_points > 0, "points_affine_filter_pad: need B > 0, N >= 0, C >= 3, max_points > 0");
  BEVF_REQUIRE((vel_c0 < 0 && vel_c1 < 0) || (vel_c0 >= 3 && vel_c1 >= 3 && vel_c0 < C && vel_c1 < C && vel_c0 != vel_c1),
               "points_affine_filter_pad: velocity channels must be two distinct channels in [3, C) or both negative");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles = point_tiles(N);
  int* const tcount = reinterpret_cast<int*>(work + (size_t)B * N * C);
  const Range6 rg = range6(pc_range6);
  if (tiles > 0) {
    hipLaunchKernelGGL(paf_count, dim3(tiles, B), dim3(PC_TILE), 0, st, points, n_in, mat12, tcount, N, C, rg);
    hipLaunchKernelGGL(paf_compact, dim3(tiles, B), dim3(PC_TILE), 0, st, points, n_in, mat12, work, tcount, count, N, C, vel_c0, vel_c1, rg);
  } else {
    (void)hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)B, st);
  }
  const long long n = (long long)max_points * C;
  hipLaunchKernelGGL(compact_output<false>, dim3((unsigned)((n + 255) / 256 < 512 ? (n + 255) / 256 : 512), B), dim3(256), 0, st,
                     (const float*)work, out, (const int*)count, (const long long*)nullptr, N, C, max_points);
  return bevf_check_launch("bevf_points_affine_filter_pad_f32");
}

extern "C" int bevf_points_affine_f32(float* points, const float* mat12, const float* noise, float noise_std, int B, int N, int C,
                                      int vel_c0, int vel_c1, void* stream) {
  BEVF_REQUIRE((points || N == 0) && mat12, "points_affine: null pointer");
  BEVF_REQUIRE(B > 0 && B < 65536 && N >= 0 && C >= 3, "points_affine: need B > 0, N >= 0, C >= 3");
  BEVF_REQUIRE((vel_c0 < 0 && vel_c1 < 0) || (vel_c0 >= 3 && vel_c1 >= 3 && vel_c0 < C && vel_c1 < C && vel_c0 != vel_c1),
               "points_affine: velocity channels must be two distinct channels in [3, C) or both negative");
  if (N == 0) return BEVF_OK;
  const int blocks = (N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024;
  hipLaunchKernelGGL(points_affine, dim3(blocks, B), dim3(256), 0, static_cast<hipStream_t>(stream), points, mat12, noise, noise_std, N, C,
                     vel_c0, vel_c1);
  return bevf_check_launch("bevf_points_affine_f32");
}

extern "C" int bevf_boxes_affine_f32(float* boxes, const int64_t* labels, float* velocities, const float* mat12, const float* scale, int B,
                                     int M, int ncol, void* stream) {
  BEVF_REQUIRE((boxes && labels) || M == 0, "boxes_affine: null pointer");
  BEVF_REQUIRE(mat12 && scale, "boxes_affine: null pointer");
  BEVF_REQUIRE(B > 0 && B < 65536 && M >= 0 && (ncol == 7 || ncol == 9), "boxes_affine: need B > 0, M >= 0, 7 or 9 columns");
  if (M == 0) return BEVF_OK;
  const int blocks = (M + 255) / 256 < 256 ? (M + 255) / 256 : 256;
  hipLaunchKernelGGL(boxes_affine, dim3(blocks, B), dim3(256), 0, static_cast<hipStream_t>(stream), boxes,
                     reinterpret_cast<const long long*>(labels), velocities, mat12, scale, M, ncol);
  return bevf_check_launch("bevf_boxes_affine_f32");
}
