// CenterPoint second stage, the RoI-dependent gather (roi_head.py): the NHWC BEV map sampled bilinearly at five
// points of every first-stage box -- the centre and the four face centres -- and the transposed gather for training.  What is
// particular to the RoIs is here: the box -> sample (roi_sample) and the sample table the backward scans; the forward skeleton,
// the corner rows, the channel walk and the backward's accumulation are bev_resample.h's, shared with the warp and the grid resample.
//   bevf_roi_bev_points_{f32,bf16}  resample_forward over cells = B * K * 5 output rows of C channels: row (b, k, p) is point p of RoI
//                                   k of frame b, so feat [B * K][5 * C] is the same buffer.  Lane k of a wave computes the fp64
//                                   geometry of cell k; rows of RoIs past count[b], non-finite points and points more than one cell
//                                   outside the map are written as zeros.  Optionally leaves the sample table.
//   bevf_roi_bev_points_bwd_f32     a pull, no atomics: one wave per SOURCE cell scans the frame's 5 * count[b] samples 64 at a time
//                                   from the table and adds the ones that touch the cell in ascending sample order.
// Launch-latency-bound at detection sizes (a few MB move); the backward is bound by its B * H * W table scans.
#include "bev_resample.h"

namespace {

constexpr int ROI_POINTS = 5;
constexpr int TABLE_WORDS = 6;      // i0, j0 and the four weights' bits

struct RoiGeom {
  double x0, y0, vx, vy;
  int H, W, K;
};

// clamp(count[b], 0, K)
__device__ __forceinline__ int roi_count(const int32_t* __restrict__ count, int b, int K) {
  const int n = count[b];
  return n < 0 ? 0 : (n < K ? n : K);
}

// The sample of output row r = (b * K + k) * 5 + p.  Points in order: centre, front and back (centre +- (l / 2)(cos, sin)), left and
// right (centre +- (w / 2)(-sin, cos)); fp64 from the fp32 box, column u = (px - x0) / vx - 0.5, row v = (py - y0) / vy - 0.5.
__device__ __forceinline__ CornerSample roi_sample(const float* __restrict__ boxes, const int32_t* __restrict__ count, const RoiGeom& g,
                                                   int r) {
#pragma clang fp contract(off)
  const int row = r / ROI_POINTS, p = r - row * ROI_POINTS;
  const int b = row / g.K, k = row - b * g.K;
  CornerSample s;
  s.ok = false;
  s.i0 = s.j0 = 0;
  s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
  if (k >= roi_count(count, b, g.K)) return s;       // (rows past the count are never read)
  const float* bx = boxes + (size_t)row * 7;
  double px = (double)bx[0], py = (double)bx[1];
  if (p > 0) {
    double sn, cs;
    sincos((double)bx[6], &sn, &cs);
    const double half = 0.5 * (double)(p <= 2 ? bx[4] : bx[3]);
    const double sign = (p & 1) ? 1.0 : -1.0;
    const double dx = p <= 2 ? cs : -sn, dy = p <= 2 ? sn : cs;
    px = px + sign * (half * dx);
    py = py + sign * (half * dy);
  }
  const double u = (px - g.x0) / g.vx - 0.5, v = (py - g.y0) / g.vy - 0.5;
  s.ok = u > -1.0 && u < (double)g.W && v > -1.0 && v < (double)g.H;   // (false for NaN and infinities)
  if (s.ok) {
    const double fj0 = floor(u), fi0 = floor(v);
    s.j0 = (int)fj0, s.i0 = (int)fi0;
    corner_weights(v - fi0, u - fj0, s.w);
  }
  return s;
}

template <typename T, int Q, bool TAIL>
__global__ __launch_bounds__(256) void roi_bev_points(const T* __restrict__ x, const float* __restrict__ boxes,
                                                       const int32_t* __restrict__ count, T* __restrict__ feat,
                                                       int32_t* __restrict__ table, RoiGeom g, int cells, int C, int x_cs) {
  resample_forward<T, Q, TAIL, false>(x, feat, cells, g.K * ROI_POINTS, g.H, g.W, C, x_cs, C, [&](int r) {
    const CornerSample s = roi_sample(boxes, count, g, r);
    if (table && (int)(threadIdx.x & 63) < CELLS_PER_WAVE) {    // one lane per cell (a clamped tail lane repeats the last cell's words)
      int32_t* t = table + (size_t)r * TABLE_WORDS;
      t[0] = s.i0, t[1] = s.j0;
#pragma unroll
      for (int q = 0; q < 4; ++q) t[2 + q] = __float_as_int(s.w[q]);
    }
    return s;
  });
}

// dx[b][i][j][:] = sum over the frame's samples s < 5 * count[b], ascending, of w(s -> i, j) * dfeat[b * K * 5 + s][:].
template <int Q>
__global__ __launch_bounds__(256) void roi_bev_points_bwd(const float* __restrict__ dfeat, const int32_t* __restrict__ table,
                                                           const int32_t* __restrict__ count, float* __restrict__ dx, RoiGeom g,
                                                           int cells, int C) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r = xcd_remap((int)blockIdx.x, (int)gridDim.x) * CELLS_PER_BLOCK + wave;
  if (r >= cells) return;
  const int P = g.H * g.W;
  const int b = r / P, i = (r - b * P) / g.W, j = r - b * P - i * g.W;
  const int per = g.K * ROI_POINTS;
  const int n = roi_count(count, b, g.K) * ROI_POINTS;
  const int32_t* tb = table + (size_t)b * per * TABLE_WORDS;
  const float* dyb = dfeat + (size_t)b * per * C;
  float* dst = dx + (size_t)r * C;
  for (int c0 = 0; c0 < C; c0 += 64 * Q) {
    const int c = c0 + lane * Q;
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    for (int s0 = 0; s0 < n; s0 += 64) {
      const int s = s0 + lane;
      float ws = 0.f;
      if (s < n) {
        const int32_t* t = tb + (size_t)s * TABLE_WORDS;
        const int di = i - t[0], dj = j - t[1];
        if (di >= 0 && di <= 1 && dj >= 0 && dj <= 1) ws = __int_as_float(t[2 + di * 2 + dj]);
      }
      accumulate_targets<Q>(__ballot(ws != 0.f), ws, s, dyb, C, c, c < C, acc);
    }
    if (c < C) store_q<float, Q>(dst + c, acc);
  }
}

int roi_points_check(const char* what, int B, int K, int H, int W, int C, double vx, double vy) {
  BEVF_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0 && C > 0, "%s: bad shape (B=%d K=%d H=%d W=%d C=%d)", what, B, K, H, W, C);
  BEVF_REQUIRE((long long)B * K * ROI_POINTS * TABLE_WORDS < (1ll << 31) && (long long)B * K * ROI_POINTS * C < (1ll << 31) &&
                   (long long)B * H * W < (1ll << 31),
               "%s: B * K * 5 * max(C, 6) or B * H * W exceeds the 32-bit offsets", what);
  // (a NaN cell size is served: every sample point is then non-finite and the output is zeros)
  BEVF_REQUIRE(vx != 0.0 && vy != 0.0, "%s: the map's extent must be non-empty", what);
  return BEVF_OK;
}

RoiGeom roi_geom(int K, int H, int W, double x_min, double y_min, double x_max, double y_max) {
  return RoiGeom{x_min, y_min, (x_max - x_min) / (double)W, (y_max - y_min) / (double)H, H, W, K};
}

template <typename T>
int roi_points_entry(const void* x, const float* boxes, const int32_t* count, void* feat, int32_t* table, int B, int K, int H, int W,
                     int C, int x_cs, double x_min, double y_min, double x_max, double y_max, void* stream) {
  const RoiGeom g = roi_geom(K, H, W, x_min, y_min, x_max, y_max);
  const int rc = roi_points_check("roi_bev_points", B, K, H, W, C, g.vx, g.vy);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(x && boxes && count && feat, "roi_bev_points: null pointer");
  BEVF_REQUIRE(x_cs >= C && (long long)B * H * W * x_cs < (1ll << 31), "roi_bev_points: x_cs=%d must be >= C with B * H * W * x_cs < 2^31",
               x_cs);
  BEVF_REQUIRE(!((uintptr_t)x & (sizeof(T) - 1)) && !((uintptr_t)feat & (sizeof(T) - 1)) && !((uintptr_t)boxes & 3u) &&
                   !((uintptr_t)count & 3u) && !((uintptr_t)table & 3u),
               "roi_bev_points: unaligned buffer");
  const int cells = B * K * ROI_POINTS;
  constexpr int per_block = CELLS_PER_BLOCK * CELLS_PER_WAVE, Q16 = vec16<T>::N;
  // the widest access every row of x and feat allows: 16 bytes, else (bf16) 8 bytes, else scalar
  const bool v16 = C % Q16 == 0 && x_cs % Q16 == 0 && bevf_aligned16(x) && bevf_aligned16(feat);
  const bool v8 = sizeof(T) == 2 && C % 4 == 0 && x_cs % 4 == 0 && !((uintptr_t)x & 7u) && !((uintptr_t)feat & 7u);
  const dim3 grid((cells + per_block - 1) / per_block), block(64 * CELLS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const T* xs = static_cast<const T*>(x);
  T* fs = static_cast<T*>(feat);
  const char* name = "bevf_roi_bev_points";
  if (v16) return bevf_launch(name, roi_bev_points<T, Q16, false>, grid, block, 0, s, xs, boxes, count, fs, table, g, cells, C, x_cs);
  if constexpr (sizeof(T) == 2) {
    if (v8) return bevf_launch(name, roi_bev_points<T, 4, false>, grid, block, 0, s, xs, boxes, count, fs, table, g, cells, C, x_cs);
  }
  return bevf_launch(name, roi_bev_points<T, 0, true>, grid, block, 0, s, xs, boxes, count, fs, table, g, cells, C, x_cs);
}

}  // namespace

extern "C" size_t bevf_roi_bev_points_table_words(int B, int K) {
  return (B > 0 && K > 0) ? (size_t)B * (size_t)K * ROI_POINTS * TABLE_WORDS : 0;
}

extern "C" int bevf_roi_bev_points_f32(const float* x, const float* boxes, const int32_t* count, float* feat, int32_t* table, int B,
                                       int K, int H, int W, int C, int x_cs, double x_min, double y_min, double x_max, double y_max,
                                       void* stream) {
  return roi_points_entry<float>(x, boxes, count, feat, table, B, K, H, W, C, x_cs, x_min, y_min, x_max, y_max, stream);
}

extern "C" int bevf_roi_bev_points_bf16(const void* x, const float* boxes, const int32_t* count, void* feat, int32_t* table, int B,
                                        int K, int H, int W, int C, int x_cs, double x_min, double y_min, double x_max, double y_max,
                                        void* stream) {
  return roi_points_entry<__bf16>(x, boxes, count, feat, table, B, K, H, W, C, x_cs, x_min, y_min, x_max, y_max, stream);
}

extern "C" int bevf_roi_bev_points_bwd_f32(const float* dfeat, const int32_t* table, const int32_t* count, float* dx, int B, int K,
                                           int H, int W, int C, void* stream) {
  const int rc = roi_points_check("roi_bev_points_bwd", B, K, H, W, C, 1.0, 1.0);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(dfeat && table && count && dx, "roi_bev_points_bwd: null pointer");
  BEVF_REQUIRE((long long)B * H * W * C < (1ll << 31), "roi_bev_points_bwd: B * H * W * C exceeds the 32-bit offsets");
  BEVF_REQUIRE(!((uintptr_t)dfeat & 3u) && !((uintptr_t)dx & 3u) && !((uintptr_t)table & 3u) && !((uintptr_t)count & 3u),
               "roi_bev_points_bwd: unaligned buffer");
  const RoiGeom g{0.0, 0.0, 1.0, 1.0, H, W, K};
  const int cells = B * H * W;
  const bool vec = C % 4 == 0 && bevf_aligned16(dfeat) && bevf_aligned16(dx);
  const dim3 grid((cells + CELLS_PER_BLOCK - 1) / CELLS_PER_BLOCK), block(64 * CELLS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) return bevf_launch("bevf_roi_bev_points_bwd_f32", roi_bev_points_bwd<4>, grid, block, 0, s, dfeat, table, count, dx, g, cells, C);
  return bevf_launch("bevf_roi_bev_points_bwd_f32", roi_bev_points_bwd<1>, grid, block, 0, s, dfeat, table, count, dx, g, cells, C);
}
