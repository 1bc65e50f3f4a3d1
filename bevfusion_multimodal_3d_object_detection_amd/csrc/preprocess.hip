// Input pipeline on the device (ref src/train_detect.py:123-189).
//
// resize_normalize_u8: Pillow's antialiased bilinear resize (what torchvision's T.Resize does to a PIL image) in
//   Pillow's own 22-bit fixed-point arithmetic -- horizontal pass rounded and clamped to uint8, then the vertical
//   pass -- followed by ToTensor (/255) and Normalize ((t-mean)/std) in fp32, written planar (NCHW) for the stem.
//   The per-axis tables (first source index, count, integer weights) come from the host
//   (preprocess.resample_tables); the resized uint8 value is bit-identical to Pillow's.
// lidar_filter_pad: range filter with strict inequalities, order-preserving compaction (wave ballot + block scan),
//   zero padding / index gather to exactly max_points rows.
#include "common.h"
#include "point_compact.h"

namespace {

constexpr int kPrec = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
  v >>= kPrec;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void resize_normalize_u8(const unsigned char* __restrict__ x, float* __restrict__ out,
                                                            int n, int H, int W, int Ho, int Wo,
                                                            const int* __restrict__ bh, const int* __restrict__ kh, int ksh,
                                                            const int* __restrict__ bv, const int* __restrict__ kv, int ksv,
                                                            float m0, float m1, float m2, float s0, float s1, float s2) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  const long long total = (long long)n * Ho * Wo;
  if (i >= total) return;
  const int ox = (int)(i % Wo);
  const int oy = (int)((i / Wo) % Ho);
  const int img = (int)(i / ((long long)Wo * Ho));
  const int x0 = bh[2 * ox], nx = bh[2 * ox + 1], y0 = bv[2 * oy], ny = bv[2 * oy + 1];
  const int* const kx = kh + (size_t)ox * ksh;
  const int* const ky = kv + (size_t)oy * ksv;
  const unsigned char* const base = x + (size_t)img * H * W * 3;
  int v0 = 1 << (kPrec - 1), v1 = v0, v2 = v0;
  for (int j = 0; j < ny; ++j) {
    const unsigned char* row = base + ((size_t)(y0 + j) * W + x0) * 3;
    int h0 = 1 << (kPrec - 1), h1 = h0, h2 = h0;
    for (int t = 0; t < nx; ++t) {
      const int k = kx[t];
      h0 += (int)row[3 * t] * k;
      h1 += (int)row[3 * t + 1] * k;
      h2 += (int)row[3 * t + 2] * k;
    }
    const int k = ky[j];                              // the horizontal pass leaves a uint8 image
    v0 += clip8(h0) * k;
    v1 += clip8(h1) * k;
    v2 += clip8(h2) * k;
  }
  const size_t plane = (size_t)Ho * Wo, o = (size_t)img * 3 * plane + (size_t)oy * Wo + ox;
  out[o] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(v0), 255.f), m0), s0);
  out[o + plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(v1), 255.f), m1), s1);
  out[o + 2 * plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(v2), 255.f), m2), s2);
}

// ---- the same resize in two passes through LDS (round 3) ----------------------------------------------------------------------
// The one-thread-per-pixel form above redoes the horizontal pass for every output row that touches an input row (each input row
// feeds ~2.5 output rows at a 2x down-scale) with 3 byte loads per tap: 75 uncoalesced byte loads and 75 integer MACs per output
// pixel, 1.0 TB/s.  Here a workgroup owns RT output rows x 64 output columns: pass 1 runs Pillow's horizontal pass ONCE per
// needed input row into an LDS tile of uint8 (exactly the intermediate image Pillow itself makes), pass 2 the vertical pass and
// the normalisation from LDS.  Same integer arithmetic, same rounding, same clamp -> the same bits.
constexpr int RT = 16, CT_ = 64, RMAX = 48;                          // output rows / columns per workgroup, input rows the tile may need

__global__ __launch_bounds__(256) void resize_normalize_u8_tiled(const unsigned char* __restrict__ x, float* __restrict__ out,
                                                                  int n, int H, int W, int Ho, int Wo,
                                                                  const int* __restrict__ bh, const int* __restrict__ kh, int ksh,
                                                                  const int* __restrict__ bv, const int* __restrict__ kv, int ksv,
                                                                  float m0, float m1, float m2, float s0, float s1, float s2, int tilesX,
                                                                  int tilesY) {
  __shared__ unsigned char hbuf[RMAX][CT_][4];                       // horizontal-pass result, 3 channels (+1 pad) per pixel
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tilesX, ty = (blockIdx.x / tilesX) % tilesY, img = blockIdx.x / (tilesX * tilesY);
  const int ox0 = tx * CT_, oy0 = ty * RT;
  const int oy1 = (oy0 + RT < Ho ? oy0 + RT : Ho) - 1;
  const int r0 = bv[2 * oy0], r1 = bv[2 * oy1] + bv[2 * oy1 + 1];  // input rows [r0, r1) feed this tile (bounds are monotonic)
  const int nr = r1 - r0;                                            // <= RMAX (checked on the host)
  const unsigned char* const base = x + (size_t)img * H * W * 3;
  {                                                                  // pass 1: thread = (output column, channel-free), rows strided
    const int c = tid & (CT_ - 1), rq = tid >> 6;                    // 4 row phases
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
  const size_t plane = (size_t)Ho * Wo;
  for (int e = tid; e < RT * CT_; e += 256) {                        // pass 2: thread = output pixel
    const int c = e & (CT_ - 1), ry = e >> 6;
    const int ox = ox0 + c, oy = oy0 + ry;
    if (ox >= Wo || oy >= Ho) continue;
    const int y0 = bv[2 * oy] - r0, ny = bv[2 * oy + 1];
    const int* const ky = kv + (size_t)oy * ksv;
    int v0 = 1 << (kPrec - 1), v1 = v0, v2 = v0;
    for (int j = 0; j < ny; ++j) {
      const int k = ky[j];
      v0 += (int)hbuf[y0 + j][c][0] * k;
      v1 += (int)hbuf[y0 + j][c][1] * k;
      v2 += (int)hbuf[y0 + j][c][2] * k;
    }
    const size_t o = (size_t)img * 3 * plane + (size_t)oy * Wo + ox;
    out[o] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(v0), 255.f), m0), s0);
    out[o + plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(v1), 255.f), m1), s1);
    out[o + 2 * plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(v2), 255.f), m2), s2);
  }
}

// Three small launches over many workgroups (round 3: the one-workgroup sweep took 190 us for 120 k points): a tile of 1024 points counts its
// survivors; every tile adds the counts in front of it (<= a few hundred integers), compacts its survivors in point order into `work` and
// the last one leaves the total; the output rows (survivors then zeros, or the caller's random choice among them) are an elementwise pass.
// The stages are point_compact.h's; here are the keep rule and the store.
__device__ __forceinline__ bool lfp_keep(const float* __restrict__ pts, int i, int N, int C, const Range6& r) {
  if (i >= N) return false;
  return in_range(r, pts[(size_t)i * C], pts[(size_t)i * C + 1], pts[(size_t)i * C + 2]);
}
__global__ __launch_bounds__(PC_TILE) void lfp_count(const float* __restrict__ pts, int* __restrict__ tcount, int N, int C, Range6 rg) {
  tile_count(lfp_keep(pts, blockIdx.x * PC_TILE + threadIdx.x, N, C, rg), tcount + blockIdx.x);
}
__global__ __launch_bounds__(PC_TILE) void lfp_compact(const float* __restrict__ pts, float* __restrict__ work, const int* __restrict__ tcount,
                                                       int* __restrict__ count, int N, int C, Range6 rg) {
  const int t = blockIdx.x, i = t * PC_TILE + threadIdx.x;
  const bool keep = lfp_keep(pts, i, N, C, rg);
  const int start = tiles_before(tcount, t);
  const TileRank r = tile_rank(keep, start);
  if (keep) {
    float* dst = work + (size_t)r.row * C;
    for (int c = 0; c < C; ++c) dst[c] = pts[(size_t)i * C + c];
  }
  if (threadIdx.x == 0 && t == (int)gridDim.x - 1) *count = start + r.total;
}

}  // namespace

extern "C" int bevf_resize_normalize_u8(const unsigned char* x, float* out, int n, int H, int W, int Ho, int Wo,
                                        const int32_t* bounds_h, const int32_t* coef_h, int ksize_h,
                                        const int32_t* bounds_v, const int32_t* coef_v, int ksize_v, const float* mean3,
                                        const float* std3, void* stream) {
  BEVF_REQUIRE(x && out && bounds_h && coef_h && bounds_v && coef_v && mean3 && std3, "resize_normalize: null pointer");
  BEVF_REQUIRE(n > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && ksize_h > 0 && ksize_v > 0, "resize_normalize: bad shape");
  BEVF_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "resize_normalize: zero std");
  const long long total = (long long)n * Ho * Wo;
  BEVF_REQUIRE((total + 255) / 256 < (1ll << 31), "resize_normalize: grid too large");
  // two-pass tiled form when a tile of 16 output rows never needs more than RMAX input rows (down-scales up to ~2.7x; the row
  // support is ksize_v, consecutive windows advance by the scale): RT * scale + ksize_v <= RMAX
  const double scale_v = (double)H / Ho;
  if (scale_v >= 1.0 && (RT - 1) * scale_v + ksize_v + 2 <= RMAX) {
    const int tilesX = (Wo + CT_ - 1) / CT_, tilesY = (Ho + RT - 1) / RT;
    hipLaunchKernelGGL(resize_normalize_u8_tiled, dim3((unsigned)((long long)n * tilesX * tilesY)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, out, n, H, W, Ho, Wo, bounds_h, coef_h, ksize_h, bounds_v, coef_v, ksize_v,
                       mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], tilesX, tilesY);
    return bevf_check_launch("bevf_resize_normalize_u8");
  }
  hipLaunchKernelGGL(resize_normalize_u8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, out, n, H, W, Ho, Wo, bounds_h, coef_h, ksize_h, bounds_v,
                     coef_v, ksize_v, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  return bevf_check_launch("bevf_resize_normalize_u8");
}

extern "C" int bevf_lidar_filter_pad_f32(const float* points, float* out, int32_t* count, float* work,
                                         const int64_t* choice, int N, int C, int max_points, const float* pc_range6,
                                         void* stream) {
  BEVF_REQUIRE((points || N == 0) && out && count && work && pc_range6, "lidar_filter_pad: null pointer");
  BEVF_REQUIRE(N >= 0 && C >= 3 && max_points > 0, "lidar_filter_pad: need N >= 0, C >= 3, max_points > 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles = point_tiles(N);
  int* const tcount = reinterpret_cast<int*>(work + (size_t)N * C);   // the tile counts live behind the compacted rows
  const Range6 rg = range6(pc_range6);
  if (tiles > 0) {
    hipLaunchKernelGGL(lfp_count, dim3(tiles), dim3(PC_TILE), 0, st, points, tcount, N, C, rg);
    hipLaunchKernelGGL(lfp_compact, dim3(tiles), dim3(PC_TILE), 0, st, points, work, tcount, count, N, C, rg);
  } else {
    (void)hipMemsetAsync(count, 0, sizeof(int32_t), st);
  }
  const long long n = (long long)max_points * C;
  hipLaunchKernelGGL(compact_output<true>, dim3((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, st, (const float*)work,
                     out, (const int*)count, reinterpret_cast<const long long*>(choice), N, C, max_points);
  return bevf_check_launch("bevf_lidar_filter_pad_f32");
}
