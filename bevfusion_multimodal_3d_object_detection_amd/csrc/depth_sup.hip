// LiDAR depth supervision of the learned-depth camera branches (`camera_view_transform: 'frustum'` / 'lift'; DESIGN.md 3.2d4;
// BEVDepth, Li et al. 2022): the sweep the model is fed anyway, projected through the frame's calibration, says which depth bin
// every feature pixel should prefer, and depth_net's logits are held to it by a cross entropy.  A target is a pure function of
// (points, calib), in fp64 with the conventions of camera_frustum.hip read backwards:
//     q = calib[b][c][0:3] . (x, y, z, 1),  zc = q_2,  u = q_0 / zc,  v = q_1 / zc            (row 2 is the depth row)
//     X = floor((u + 1/2) Wc / img_w),  Y = floor((v + 1/2) Hc / img_h),  d = min(floor((zc - dmin) D / (dmax - dmin)), D - 1)
//     target[b][c][Y][X] = the smallest d over the frame's points with dmin <= zc < dmax that land on the map (the nearest
//     return), -1 where there is none; all-zero rows and rows at or past counts[b] are padding and never count.
// fp32 logits, stream-ordered, nothing allocated, no host synchronisation: capture-safe; a second launch gives the same bits.
//
//   bevf_depth_targets_f64   memset to 0xFFFFFFFF, then depth_targets: one thread per (point, camera, frame), the 12 calibration
//                            doubles at a block-uniform address (scalar loads), an integer atomicMin on the unsigned bin -- the
//                            minimum does not depend on the order, and -1 is the largest unsigned value
//   bevf_depth_ce_f32        depth_ce: rows as softmax_rows lays them out (a row takes the next power of two >= D lanes, one lane
//                            per bin, the same xor butterfly), row loss = log(sum exp(x - max)) - (x_t - max) from the logits; a
//                            workgroup walks its chunks of rows in a fixed order and writes one (sum, count) pair in fp64;
//                            depth_ce_finish: one wave adds the pairs -- lane l takes l, l + 64, ... ascending, then the butterfly
//   bevf_depth_ce_bwd_f32    depth_ce_bwd: dlogit[r][d] += g / max(count, 1) * (pd[r][d] - [d == t]) on the rows that have a
//                            target; g and count come from device memory
#include "common.h"

namespace {

constexpr int CE_MAX_BLOCKS = 2048;  // (sum, count) pairs of bevf_depth_ce_f32: a workgroup takes every CE_MAX_BLOCKS-th chunk of rows

struct DepthGeom {
  double dmin, dmax, img_h, img_w;
  int ncam, Hc, Wc, D;
};

__global__ __launch_bounds__(256) void depth_targets(const float* __restrict__ points, long long p_bs, int p_stride, int N,
                                                     const int32_t* __restrict__ counts, const double* __restrict__ calib,
                                                     long long calib_bs, DepthGeom g, unsigned* __restrict__ target) {
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  const int cam = (int)blockIdx.y;
  const long long b = (long long)blockIdx.z;
  int n = N;
  if (counts) n = counts[b] < N ? counts[b] : N;
  if (p >= n) return;
  const float* src = points + b * p_bs + (long long)p * p_stride;
  const float xf = src[0], yf = src[1], zf = src[2];
  if (xf == 0.f && yf == 0.f && zf == 0.f) return;                 // a padding row
  const double* M = calib + b * calib_bs + (long long)cam * 16;    // the same address in every lane
  const double x = xf, y = yf, z = zf;
  const double q0 = M[0] * x + M[1] * y + M[2] * z + M[3];
  const double q1 = M[4] * x + M[5] * y + M[6] * z + M[7];
  const double zc = M[8] * x + M[9] * y + M[10] * z + M[11];
  if (!(zc >= g.dmin && zc < g.dmax)) return;                      // (a NaN fails every comparison here and below)
  const double fx = floor((q0 / zc + 0.5) * g.Wc / g.img_w), fy = floor((q1 / zc + 0.5) * g.Hc / g.img_h);
  if (!(fx >= 0.0 && fx < (double)g.Wc && fy >= 0.0 && fy < (double)g.Hc)) return;
  int d = (int)floor((zc - g.dmin) * g.D / (g.dmax - g.dmin));
  d = d < g.D - 1 ? d : g.D - 1;
  d = d > 0 ? d : 0;
  atomicMin(&target[((b * g.ncam + cam) * g.Hc + (int)fy) * g.Wc + (int)fx], (unsigned)d);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// chunk = the 256 >> lg rows one pass of the workgroup holds; workgroup w takes chunks w, w + gridDim.x, ... in that order.
__global__ __launch_bounds__(256) void depth_ce(const float* __restrict__ logits, int l_rs, const int32_t* __restrict__ target,
                                                int nrows, int D, int lg, int chunks, double* __restrict__ partials) {
  __shared__ double red[2][4];
  const int L = 1 << lg, d = (int)threadIdx.x & (L - 1), sub = (int)threadIdx.x >> lg, rows_per = 256 >> lg;
  double sum = 0.0, cnt = 0.0;
  for (int c = (int)blockIdx.x; c < chunks; c += (int)gridDim.x) {
    const int row = c * rows_per + sub;
    const int t = row < nrows ? target[row] : -1;
    const bool on = t >= 0 && d < D;
    const float v = on ? logits[(long long)row * l_rs + d] : -INFINITY;
    const float mx = group_reduce<true>(v, L);
    const float e = on ? expf(v - mx) : 0.f;
    const float s = group_reduce<false>(e, L);
    const float xt = group_reduce<false>(on && d == t ? v - mx : 0.f, L);
    if (t >= 0 && d == 0) {
      sum += (double)(logf(s) - xt);
      cnt += 1.0;
    }
  }
  sum = wave_sum(sum), cnt = wave_sum(cnt);
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[0][wave] = sum, red[1][wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    partials[2 * blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

__global__ __launch_bounds__(64) void depth_ce_finish(const double* __restrict__ partials, int n, float* __restrict__ out) {
  double sum = 0.0, cnt = 0.0;
  for (int i = (int)threadIdx.x; i < n; i += 64) sum += partials[2 * i], cnt += partials[2 * i + 1];
  sum = wave_sum(sum), cnt = wave_sum(cnt);
  if (threadIdx.x == 0) {
    out[0] = (float)(sum / (cnt > 1.0 ? cnt : 1.0));
    out[1] = (float)cnt;
  }
}

__global__ __launch_bounds__(256) void depth_ce_bwd(const float* __restrict__ pd, int p_rs, const int32_t* __restrict__ target,
                                                    const float* __restrict__ g, const float* __restrict__ out,
                                                    float* __restrict__ dlogit, int x_rs, long long nrows, int D, int lg) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = i >> lg;
  const int d = (int)(i & ((1 << lg) - 1));
  if (row >= nrows || d >= D) return;
  const int t = target[row];
  if (t < 0) return;
  const float scale = g[0] / fmaxf(out[1], 1.f);
  float* dst = dlogit + row * x_rs + d;
  *dst += scale * (pd[row * p_rs + d] - (d == t ? 1.f : 0.f));
}

int log2_lanes_per_row(int cols) {
  int lg = 0;
  while ((1 << lg) < cols) ++lg;
  return lg;
}

}  // namespace

extern "C" size_t bevf_depth_ce_work_doubles(void) { return 2 * (size_t)CE_MAX_BLOCKS; }

extern "C" int bevf_depth_targets_f64(const float* points, size_t p_bs, int p_stride, int N, const int32_t* counts,
                                      const double* calib, size_t calib_bs, int B, int ncam, int Hc, int Wc, int D, double depth_min,
                                      double depth_max, int img_h, int img_w, int32_t* target, void* stream) {
  BEVF_REQUIRE(calib && target && (points || N == 0), "depth_targets: null pointer");
  BEVF_REQUIRE(B > 0 && B <= 65535 && ncam > 0 && ncam <= 65535 && Hc > 0 && Wc > 0 && img_h > 0 && img_w > 0 && N >= 0 &&
                   N <= (1 << 30),
               "depth_targets: bad shape (B=%d ncam=%d Hc=%d Wc=%d N=%d; B, ncam <= 65535)", B, ncam, Hc, Wc, N);
  BEVF_REQUIRE(D >= 1 && D <= 64 && depth_min > 0.0 && depth_min < depth_max, "depth_targets: bad depth bins (D=%d, %g..%g)", D,
               depth_min, depth_max);
  BEVF_REQUIRE(N == 0 || (p_stride >= 3 && p_bs >= (size_t)(N - 1) * (size_t)p_stride + 3), "depth_targets: bad point strides");
  BEVF_REQUIRE(calib_bs == 0 || calib_bs >= (size_t)ncam * 16, "depth_targets: calib stride must be 0 (shared) or >= ncam * 16");
  const size_t cells = (size_t)B * (size_t)ncam * (size_t)Hc * (size_t)Wc;
  BEVF_REQUIRE(cells < ((size_t)1 << 40), "depth_targets: target too large");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(target, 0xFF, sizeof(int32_t) * cells, s) != hipSuccess) {
    bevf_set_error("depth_targets: memset failed");
    return BEVF_ERR_LAUNCH;
  }
  if (N == 0) return BEVF_OK;
  DepthGeom g;
  g.dmin = depth_min, g.dmax = depth_max, g.img_h = img_h, g.img_w = img_w;
  g.ncam = ncam, g.Hc = Hc, g.Wc = Wc, g.D = D;
  return bevf_launch("bevf_depth_targets_f64", depth_targets, dim3((unsigned)((N + 255) / 256), ncam, B), dim3(256), 0, s, points,
                     (long long)p_bs, p_stride, N, counts, calib, (long long)calib_bs, g, reinterpret_cast<unsigned*>(target));
}

extern "C" int bevf_depth_ce_f32(const float* logits, int l_rs, const int32_t* target, size_t nrows, int D, double* partials,
                                 float* out, void* stream) {
  BEVF_REQUIRE(logits && target && partials && out, "depth_ce: null pointer");
  BEVF_REQUIRE(nrows > 0 && nrows <= ((size_t)1 << 24) && D >= 1 && D <= 64 && l_rs >= D,
               "depth_ce: bad shape (nrows=%zu D=%d; at most 2^24 rows -- the count is returned as a float --, 1 <= D <= 64 <= stride)",
               nrows, D);
  BEVF_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0, "depth_ce: partials must be 8-byte aligned");
  const int lg = log2_lanes_per_row(D);
  const int rows_per = 256 >> lg;
  const int chunks = (int)((nrows + rows_per - 1) / rows_per);
  const int blocks = chunks < CE_MAX_BLOCKS ? chunks : CE_MAX_BLOCKS;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = bevf_launch("bevf_depth_ce_f32", depth_ce, dim3(blocks), dim3(256), 0, s, logits, l_rs, target, (int)nrows, D, lg,
                             chunks, partials);
  if (rc != BEVF_OK) return rc;
  return bevf_launch("bevf_depth_ce_f32", depth_ce_finish, dim3(1), dim3(64), 0, s, (const double*)partials, blocks, out);
}

extern "C" int bevf_depth_ce_bwd_f32(const float* pd, int p_rs, const int32_t* target, const float* g, const float* out,
                                     float* dlogit, int x_rs, size_t nrows, int D, void* stream) {
  BEVF_REQUIRE(pd && target && g && out && dlogit, "depth_ce_bwd: null pointer");
  BEVF_REQUIRE(nrows > 0 && nrows <= ((size_t)1 << 24) && D >= 1 && D <= 64 && p_rs >= D && x_rs >= D,
               "depth_ce_bwd: bad shape (nrows=%zu D=%d; at most 2^24 rows, 1 <= D <= 64 <= strides)", nrows, D);
  const int lg = log2_lanes_per_row(D);
  const unsigned long long blocks = (((unsigned long long)nrows << lg) + 255) / 256;
  return bevf_launch("bevf_depth_ce_bwd_f32", depth_ce_bwd, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), pd,
                     p_rs, target, g, out, dlogit, x_rs, (long long)nrows, D, lg);
}
