// BEV map-segmentation head: the kernels around the classifier's convolutions.
//   bevf_bev_grid_resample_{f32,bf16}  an NHWC map on one axis-aligned metric grid resampled bilinearly onto another.  The map is
//                                      separable: a wave takes four output cells, lane k computes the row sample and the column
//                                      sample of cell k in fp64 (the kernel's own prologue -- nothing is built on the host, so the
//                                      op sits inside a captured graph), then the wave walks the cells with each sample read back as
//                                      scalars and the lanes move the channels 16 bytes at a time; a scalar tail takes C % (16 bytes).
//                                      The axis samples and the candidate ranges are here; the stages shared with the ego-motion
//                                      warp (forward skeleton, corner rows, channel walk, backward accumulation) in bev_resample.h.
//   bevf_bev_grid_resample_bwd_f32     the transpose as a pull, no atomics: one wave per SOURCE cell; the contributing output rows and
//                                      columns are contiguous ranges found from the inverse scalar map (widened by one, every candidate
//                                      re-checked with the forward's own sample), summed in row-major target order.
//   bevf_seg_focal_loss_f32            sigmoid focal loss on logits: fixed-grid fp64 partial sums per class, then a fixed-order finish.
//   bevf_seg_focal_loss_bwd_f32        its gradient, one lane per logit column (padding columns written as zeros).
//   bevf_seg_iou_counts                TP / FP / FN per (threshold, class): wave ballots -> LDS counters -> one 64-bit integer atomic
//                                      per counter and workgroup (integer sums: the same bits in any order).
// All HBM-bound or tiny; no MFMA.
#include "bev_resample.h"

namespace {

constexpr int FOCAL_MAX_BLOCKS = 1024;
constexpr int SEG_MAX_CLASSES = 64;
constexpr int IOU_MAX_THRESHOLDS = 32;
constexpr int IOU_MAX_BLOCKS = 1024;

// ---- resample ------------------------------------------------------------------------------------------------------------------

// One axis of the map: output index o -> input coordinate q = (out0 + (o + 0.5) ovox - in0) / ivox - 0.5.
struct Axis {
  double in0, ivox, out0, ovox;
  int n_in, n_out;
};
struct ResampleGeom {
  Axis row, col;   // row i is y, column j is x (the convention of encoders.pillar_grid and bev_warp)
};

// The sample of output index o along one axis: lower neighbour i0 and the fraction f towards i0 + 1.  ok = false: the point is
// non-finite or more than one cell outside the input -- no neighbour contributes.
struct AxisSample {
  int i0;
  double f;
  bool ok;
};

__device__ __forceinline__ AxisSample axis_sample(const Axis& a, int o) {
#pragma clang fp contract(off)
  const double p = a.out0 + ((double)o + 0.5) * a.ovox;
  const double q = (p - a.in0) / a.ivox - 0.5;
  AxisSample s;
  s.ok = q > -1.0 && q < (double)a.n_in;   // (false for NaN and infinities)
  s.i0 = 0;
  s.f = 0.0;
  if (s.ok) {
    const double fl = floor(q);
    s.i0 = (int)fl;
    s.f = q - fl;
  }
  return s;
}

// The factor with which input index `src` enters the sample s: (1 - f) as the lower neighbour, f as the upper one, else 0.
__device__ __forceinline__ double axis_factor(const AxisSample& s, int src) {
#pragma clang fp contract(off)
  if (!s.ok) return 0.0;
  if (s.i0 == src) return 1.0 - s.f;
  if (s.i0 + 1 == src) return s.f;
  return 0.0;
}

// VEC: C's leading multiple of 16 bytes moves as 16-byte accesses (bases and strides allow it, checked by the entry point).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void bev_grid_resample(const T* __restrict__ x, T* __restrict__ y, ResampleGeom g, int cells, int C,
                                                          int x_cs, int y_cs) {
  const int Wo = g.col.n_out, P = g.row.n_out * Wo;
  resample_forward<T, VEC ? vec16<T>::N : 0, true, true>(x, y, cells, P, g.row.n_in, g.col.n_in, C, x_cs, y_cs, [&](int r) {
    const int p = r % P;
    const AxisSample sr = axis_sample(g.row, p / Wo), sc = axis_sample(g.col, p % Wo);
    CornerSample s;
    s.i0 = sr.i0, s.j0 = sc.i0;
    s.ok = sr.ok && sc.ok;
    s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0.f;
    if (s.ok) corner_weights(sr.f, sc.f, s.w);
    return s;
  });
}

// Candidate output indices for source index `src` along one axis: q(o) is affine in o, so the o with floor(q) in {src - 1, src} form
// a contiguous range; its ends come from the inverse map at q = src -+ 1, widened by one and clamped to the output (every candidate is
// checked again with axis_sample, so the range only has to be a superset).  lo > hi: none.
__device__ __forceinline__ void axis_candidates(const Axis& a, int src, int& lo, int& hi) {
#pragma clang fp contract(off)
  const double slope = a.ovox / a.ivox;
  const double off = (a.out0 + 0.5 * a.ovox - a.in0) / a.ivox - 0.5;   // q(o) ~= off + slope * o
  const double o1 = ((double)src - 1.0 - off) / slope, o2 = ((double)src + 1.0 - off) / slope;
  const double omin = fmin(o1, o2), omax = fmax(o1, o2);
  lo = 0, hi = -1;
  if (omin == omin && omax == omax) {   // (a NaN range or cell size: no output has a finite sample, nothing lands)
    lo = (int)fmin(fmax(floor(omin) - 1.0, 0.0), (double)a.n_out);
    hi = (int)fmax(fmin(ceil(omax) + 1.0, (double)a.n_out - 1.0), -1.0);
  }
}

// dx[b][u][v][c] = sum over the targets (i, j), row-major, of (float)(row factor * column factor) * dy[b][i][j][c]: the forward's
// weight expression, recomputed.  Q channels per lane (4 when the rows of dy and dx are 16-byte aligned, else 1).
template <int Q>
__global__ __launch_bounds__(256) void bev_grid_resample_bwd(const float* __restrict__ dy, float* __restrict__ dx, ResampleGeom g,
                                                              int cells, int C, int dy_cs) {
#pragma clang fp contract(off)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int r = xcd_remap((int)blockIdx.x, (int)gridDim.x) * CELLS_PER_BLOCK + wave;
  if (r >= cells) return;
  const int Hi = g.row.n_in, Wi = g.col.n_in, Wo = g.col.n_out;
  const int Pi = Hi * Wi;
  const int b = r / Pi, u = (r - b * Pi) / Wi, v = r - b * Pi - u * Wi;
  int ilo, ihi, jlo, jhi;
  axis_candidates(g.row, u, ilo, ihi);
  axis_candidates(g.col, v, jlo, jhi);
  const int ni = ihi - ilo + 1, nj = jhi - jlo + 1;
  // the first 64 candidate columns' factors, one per lane: all of them for every ratio above 1 / 30
  const double cf0 = lane < nj ? axis_factor(axis_sample(g.col, jlo + lane), v) : 0.0;
  const float* dyb = dy + (size_t)b * (size_t)(g.row.n_out * Wo) * (size_t)dy_cs;
  float* dst = dx + (size_t)r * (size_t)C;
  for (int c0 = 0; c0 < C; c0 += 64 * Q) {
    const int c = c0 + lane * Q;
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    for (int ib = 0; ib < ni; ib += 64) {
      const double rf = ib + lane < ni ? axis_factor(axis_sample(g.row, ilo + ib + lane), u) : 0.0;
      unsigned long long rmask = __ballot(rf != 0.0);
      while (rmask) {
        const int lr = __builtin_ctzll(rmask);
        rmask &= rmask - 1;
        const double rfv = __shfl(rf, lr, 64);
        const int rowbase = (ilo + ib + lr) * Wo + jlo;
        for (int jb = 0; jb < nj; jb += 64) {
          const double cf = jb == 0 ? cf0 : (jb + lane < nj ? axis_factor(axis_sample(g.col, jlo + jb + lane), v) : 0.0);
          accumulate_targets<Q>(__ballot(cf != 0.0), (float)(rfv * cf), rowbase + jb + lane, dyb, dy_cs, c, c < C, acc);
        }
      }
    }
    if (c < C) store_q<float, Q>(dst + c, acc);
  }
}

int resample_check(const char* what, const void* x, const void* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cs, int y_cs,
                   double vx, double vy, double ovx, double ovy) {
  BEVF_REQUIRE(x && y, "%s: null pointer", what);
  BEVF_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0, "%s: bad shape (B=%d Hi=%d Wi=%d Ho=%d Wo=%d C=%d)", what, B, Hi,
               Wi, Ho, Wo, C);
  BEVF_REQUIRE(x_cs >= C && y_cs >= C, "%s: channel strides must be >= C", what);
  BEVF_REQUIRE((long long)B * Hi * Wi < (1ll << 31) && (long long)B * Ho * Wo < (1ll << 31), "%s: more than 2^31 cells", what);
  // (a NaN cell size is served: every sample point is then non-finite and the output is zeros)
  BEVF_REQUIRE(vx != 0.0 && vy != 0.0 && ovx != 0.0 && ovy != 0.0, "%s: cell sizes must be non-zero", what);
  return BEVF_OK;
}

ResampleGeom resample_geom(int Hi, int Wi, int Ho, int Wo, double x0, double y0, double vx, double vy, double ox0, double oy0,
                           double ovx, double ovy) {
  ResampleGeom g;
  g.row = Axis{y0, vy, oy0, ovy, Hi, Ho};
  g.col = Axis{x0, vx, ox0, ovx, Wi, Wo};
  return g;
}

template <typename T>
int resample_entry(const void* x, void* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cs, int y_cs, double x0, double y0,
                   double vx, double vy, double ox0, double oy0, double ovx, double ovy, void* stream) {
  const int rc = resample_check("bev_grid_resample", x, y, B, Hi, Wi, Ho, Wo, C, x_cs, y_cs, vx, vy, ovx, ovy);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(!((uintptr_t)x & (sizeof(T) - 1)) && !((uintptr_t)y & (sizeof(T) - 1)), "bev_grid_resample: unaligned buffer");
  const ResampleGeom g = resample_geom(Hi, Wi, Ho, Wo, x0, y0, vx, vy, ox0, oy0, ovx, ovy);
  const int cells = B * Ho * Wo;
  constexpr int per_block = CELLS_PER_BLOCK * CELLS_PER_WAVE, Q = vec16<T>::N;
  const bool vec = C >= Q && x_cs % Q == 0 && y_cs % Q == 0 && bevf_aligned16(x) && bevf_aligned16(y);
  const dim3 grid((cells + per_block - 1) / per_block), block(64 * CELLS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const T* xs = static_cast<const T*>(x);
  T* ys = static_cast<T*>(y);
  return bevf_dispatch_bool(vec, [&](auto v) {
    return bevf_launch("bevf_bev_grid_resample", bev_grid_resample<T, decltype(v)::value>, grid, block, 0, s, xs, ys, g, cells, C, x_cs,
                       y_cs);
  });
}

// ---- focal loss ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// One element of the loss: p = sigmoid(x) and q = 1 - p from e = exp(-|x|) without cancellation, m = 1 - p_t, n = p_t,
// bce = max(x, 0) - x t + log1p(e).  Returns a_t m^gamma bce; *grad (when asked for) = d/dx = sign a_t m^gamma (gamma n bce + m),
// sign = -1 for t = 1 and +1 for t = 0.
__device__ __forceinline__ float focal_pow(float m, float gamma) {
  if (gamma == 2.f) return m * m;
  if (gamma == 0.f) return 1.f;
  if (gamma == 1.f) return m;
  return powf(m, gamma);
}

template <bool GRAD>
__device__ __forceinline__ float focal_term(float x, bool t, float alpha, float gamma, float* grad) {
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  const float big = inv, small = e * inv;              // sigmoid(|x|), sigmoid(-|x|)
  const float p = x >= 0.f ? big : small, q = x >= 0.f ? small : big;
  const float m = t ? q : p, n = t ? p : q;
  const float bce = fmaxf(x, 0.f) - (t ? x : 0.f) + log1pf(e);
  const float at = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  const float mg = focal_pow(m, gamma);
  if (GRAD) *grad = (t ? -1.f : 1.f) * at * mg * (gamma * n * bce + m);
  return at * mg * bce;
}

// Classes four at a time (one 16-byte load of a logit row when VEC), pixels over a fixed grid in a fixed order: thread t of block w
// takes rows w * 256 + t, + gridDim.x * 256, ...; the block's four wave sums are added in wave order.  partials [gridDim.x][K].
template <bool VEC>
__global__ __launch_bounds__(256) void seg_focal_partials(const float* __restrict__ logits, const uint8_t* __restrict__ targets,
                                                           long long rows, int P, int K, int cs, float alpha, float gamma,
                                                           double* __restrict__ partials) {
  __shared__ double red[4][4];
  const int wave = (int)threadIdx.x >> 6;
  for (int k0 = 0; k0 < K; k0 += 4) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < rows; row += (long long)gridDim.x * 256) {
      const long long b = row / P, p = row - b * P;
      const float* src = logits + row * cs + k0;
      float xv[4];
      if (VEC) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = v[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = k0 + j < K ? src[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k0 + j < K) {
          const bool t = targets[(b * K + k0 + j) * P + p] != 0;
          acc[j] += (double)focal_term<false>(xv[j], t, alpha, gamma, nullptr);
        }
      }
    }
    __syncthreads();   // (red is reused from the previous class group)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double s = wave_sum(acc[j]);
      if ((threadIdx.x & 63) == 0) red[j][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4 && k0 + (int)threadIdx.x < K) {
      const int j = (int)threadIdx.x;
      partials[(size_t)blockIdx.x * K + k0 + j] = ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
    }
  }
}

// One wave: class k's partials added lane l taking l, l + 64, ... ascending, then the butterfly; out[k] = the mean, out[K] = the
// sum of the K means in class order.
__global__ __launch_bounds__(64) void seg_focal_finish(const double* __restrict__ partials, int n, int K, double count,
                                                       float* __restrict__ out) {
  double total = 0.0;
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += 64) s += partials[(size_t)i * K + k];
    s = wave_sum(s) / count;
    total += s;
    if (threadIdx.x == 0) out[k] = (float)s;
  }
  if (threadIdx.x == 0) out[K] = (float)total;
}

// One lane per logit column of a row, padding columns included (zeros).
__global__ __launch_bounds__(256) void seg_focal_bwd(const float* __restrict__ logits, const uint8_t* __restrict__ targets,
                                                     const float* __restrict__ g, float* __restrict__ dlogit, long long rows, int P, int K,
                                                     int cs, float alpha, float gamma, float inv_count) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = i / cs;
  const int k = (int)(i - row * cs);
  if (row >= rows) return;
  float d = 0.f;
  if (k < K) {
    const long long b = row / P, p = row - b * P;
    float grad;
    focal_term<true>(logits[i], targets[(b * K + k) * P + p] != 0, alpha, gamma, &grad);
    d = g[0] * inv_count * grad;
  }
  dlogit[i] = d;
}

int focal_check(const char* what, const void* logits, const void* targets, int B, int P, int K, int cs, float gamma) {
  BEVF_REQUIRE(logits && targets, "%s: null pointer", what);
  BEVF_REQUIRE(B > 0 && P > 0 && K > 0 && K <= SEG_MAX_CLASSES && cs >= K, "%s: bad shape (B=%d P=%d K=%d stride=%d; K <= %d <= stride)",
               what, B, P, K, cs, SEG_MAX_CLASSES);
  BEVF_REQUIRE((long long)B * P * cs < (1ll << 40), "%s: logits too large", what);
  BEVF_REQUIRE(gamma >= 0.f, "%s: gamma must be >= 0, got %g", what, (double)gamma);
  return BEVF_OK;
}

// ---- IoU counts ------------------------------------------------------------------------------------------------------------------

// counts [T][K][3] = (TP, FP, FN) with the prediction logit >= thr[t]; zeroed by the entry point's memset node.
__global__ __launch_bounds__(256) void seg_iou_counts(const float* __restrict__ logits, int cs, const uint8_t* __restrict__ targets,
                                                      const float* __restrict__ thr, int T, long long rows, int P, int K,
                                                      unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned int lds_counts[];   // [T][K][3]
  const int n = T * K * 3;
  for (int i = (int)threadIdx.x; i < n; i += 256) lds_counts[i] = 0u;
  __syncthreads();
  const bool first = (threadIdx.x & 63) == 0;
  // whole waves stay in the loop (ballots): a lane past the end contributes to no count.  A block sees at most 2^32 / gridDim.x
  // rows per counter, far below the 32-bit LDS counters' range for any map the entry point admits.
  const long long span = (long long)gridDim.x * 256;
  for (long long base = (long long)blockIdx.x * 256; base < rows; base += span) {
    const long long row = base + threadIdx.x;
    const bool valid = row < rows;
    const long long b = valid ? row / P : 0, p = valid ? row - b * P : 0;
    for (int k = 0; k < K; ++k) {
      const float x = valid ? logits[row * cs + k] : 0.f;
      const bool t = valid && targets[(b * K + k) * P + p] != 0;
      for (int ti = 0; ti < T; ++ti) {
        const bool pred = valid && x >= thr[ti];
        const unsigned tp = (unsigned)__builtin_popcountll(__ballot(pred && t));
        const unsigned fp = (unsigned)__builtin_popcountll(__ballot(pred && !t));
        const unsigned fn = (unsigned)__builtin_popcountll(__ballot(valid && !pred && t));
        if (first) {
          unsigned int* c = lds_counts + (ti * K + k) * 3;
          if (tp) atomicAdd(c, tp);
          if (fp) atomicAdd(c + 1, fp);
          if (fn) atomicAdd(c + 2, fn);
        }
      }
    }
  }
  __syncthreads();
  for (int i = (int)threadIdx.x; i < n; i += 256)
    if (lds_counts[i]) atomicAdd(counts + i, (unsigned long long)lds_counts[i]);
}

}  // namespace

extern "C" int bevf_bev_grid_resample_f32(const float* x, float* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cs, int y_cs,
                                          double x0, double y0, double vx, double vy, double ox0, double oy0, double ovx, double ovy,
                                          void* stream) {
  return resample_entry<float>(x, y, B, Hi, Wi, Ho, Wo, C, x_cs, y_cs, x0, y0, vx, vy, ox0, oy0, ovx, ovy, stream);
}

extern "C" int bevf_bev_grid_resample_bf16(const void* x, void* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cs, int y_cs,
                                           double x0, double y0, double vx, double vy, double ox0, double oy0, double ovx, double ovy,
                                           void* stream) {
  return resample_entry<__bf16>(x, y, B, Hi, Wi, Ho, Wo, C, x_cs, y_cs, x0, y0, vx, vy, ox0, oy0, ovx, ovy, stream);
}

extern "C" int bevf_bev_grid_resample_bwd_f32(const float* dy, float* dx, int B, int Hi, int Wi, int Ho, int Wo, int C, int dy_cs,
                                              double x0, double y0, double vx, double vy, double ox0, double oy0, double ovx,
                                              double ovy, void* stream) {
  const int rc = resample_check("bev_grid_resample_bwd", dy, dx, B, Hi, Wi, Ho, Wo, C, C, dy_cs, vx, vy, ovx, ovy);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(!((uintptr_t)dy & 3u) && !((uintptr_t)dx & 3u), "bev_grid_resample_bwd: unaligned buffer");
  const ResampleGeom g = resample_geom(Hi, Wi, Ho, Wo, x0, y0, vx, vy, ox0, oy0, ovx, ovy);
  const int cells = B * Hi * Wi;
  const bool vec = C % 4 == 0 && dy_cs % 4 == 0 && bevf_aligned16(dy) && bevf_aligned16(dx);
  const dim3 grid((cells + CELLS_PER_BLOCK - 1) / CELLS_PER_BLOCK), block(64 * CELLS_PER_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) return bevf_launch("bevf_bev_grid_resample_bwd_f32", bev_grid_resample_bwd<4>, grid, block, 0, s, dy, dx, g, cells, C, dy_cs);
  return bevf_launch("bevf_bev_grid_resample_bwd_f32", bev_grid_resample_bwd<1>, grid, block, 0, s, dy, dx, g, cells, C, dy_cs);
}

extern "C" size_t bevf_seg_focal_work_doubles(int K) { return (size_t)FOCAL_MAX_BLOCKS * (size_t)(K > 0 ? K : 0); }

extern "C" int bevf_seg_focal_loss_f32(const float* logits, int cs, const uint8_t* targets, int B, int P, int K, float alpha,
                                       float gamma, double* partials, float* out, void* stream) {
  const int rc = focal_check("seg_focal_loss", logits, targets, B, P, K, cs, gamma);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(partials && out, "seg_focal_loss: null pointer");
  BEVF_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0, "seg_focal_loss: partials must be 8-byte aligned");
  const long long rows = (long long)B * P;
  const long long chunks = (rows + 255) / 256;
  const int blocks = (int)(chunks < FOCAL_MAX_BLOCKS ? chunks : FOCAL_MAX_BLOCKS);
  // 16-byte logit loads: every class group k0 .. k0 + 3 of every row lies inside the row and is aligned
  const bool vec = cs % 4 == 0 && (K + 3) / 4 * 4 <= cs && bevf_aligned16(logits);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc2 = bevf_dispatch_bool(vec, [&](auto v) {
    return bevf_launch("bevf_seg_focal_loss_f32", seg_focal_partials<decltype(v)::value>, dim3(blocks), dim3(256), 0, s, logits, targets,
                       rows, P, K, cs, alpha, gamma, partials);
  });
  if (rc2 != BEVF_OK) return rc2;
  return bevf_launch("bevf_seg_focal_loss_f32", seg_focal_finish, dim3(1), dim3(64), 0, s, (const double*)partials, blocks, K,
                     (double)rows, out);
}

extern "C" int bevf_seg_focal_loss_bwd_f32(const float* logits, int cs, const uint8_t* targets, const float* g, float* dlogit, int B,
                                           int P, int K, float alpha, float gamma, void* stream) {
  const int rc = focal_check("seg_focal_loss_bwd", logits, targets, B, P, K, cs, gamma);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(g && dlogit, "seg_focal_loss_bwd: null pointer");
  const long long rows = (long long)B * P;
  const long long blocks = (rows * cs + 255) / 256;
  BEVF_REQUIRE(blocks < (1ll << 31), "seg_focal_loss_bwd: logits too large");
  return bevf_launch("bevf_seg_focal_loss_bwd_f32", seg_focal_bwd, dim3((unsigned)blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), logits, targets, g, dlogit, rows, P, K, cs, alpha, gamma,
                     (float)(1.0 / (double)rows));
}

extern "C" int bevf_seg_iou_counts(const float* logits, int cs, const uint8_t* targets, const float* thr, int T, int64_t* counts,
                                   int B, int P, int K, void* stream) {
  BEVF_REQUIRE(logits && targets && thr && counts, "seg_iou_counts: null pointer");
  BEVF_REQUIRE(B > 0 && P > 0 && K > 0 && K <= SEG_MAX_CLASSES && cs >= K && T > 0 && T <= IOU_MAX_THRESHOLDS,
               "seg_iou_counts: bad shape (B=%d P=%d K=%d stride=%d T=%d; K <= %d <= stride, T <= %d)", B, P, K, cs, T, SEG_MAX_CLASSES,
               IOU_MAX_THRESHOLDS);
  BEVF_REQUIRE((long long)B * P * cs < (1ll << 40), "seg_iou_counts: logits too large");
  BEVF_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7u) == 0, "seg_iou_counts: counts must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = (size_t)T * K * 3;
  if (hipMemsetAsync(counts, 0, n * sizeof(int64_t), s) != hipSuccess) {
    bevf_set_error("seg_iou_counts: memset failed");
    return BEVF_ERR_LAUNCH;
  }
  const long long rows = (long long)B * P;
  const long long chunks = (rows + 255) / 256;
  const int blocks = (int)(chunks < IOU_MAX_BLOCKS ? chunks : IOU_MAX_BLOCKS);
  return bevf_launch("bevf_seg_iou_counts", seg_iou_counts, dim3(blocks), dim3(256), n * sizeof(unsigned int), s, logits, cs, targets,
                     thr, T, rows, P, K, reinterpret_cast<unsigned long long*>(counts));
}
