// PointPillars LiDAR front end on the BEV grid (the opt-in `model.lidar_encoder.type: PointPillars` branch).
// No reference line: the reference has no working voxel path, so the semantics are the standard
// PointPillars ones, pinned by the fp64 restatement in tests/pillar_ref.py:
//   voxelize (csrc/voxelize.hip, one pillar per BEV cell) -> decorated point f = [x, y, z, r, extra..., x-x_mean, y-y_mean,
//   z-z_mean, x-x_centre, y-y_centre] (K = C + 5 <= 16 channels; padding rows are all-zero) -> Linear -> BatchNorm -> ReLU ->
//   max over the P rows of the pillar -> the pillar's vector at its (y, x) cell of an NHWC canvas, 0 elsewhere.
// Three kernels, one wave per pillar slot (4 per workgroup; slots >= num_voxels[b] are skipped, so voxelize's outputs need no
// zero fill), the pillar's decorated rows staged once in LDS:
//   pillar_pfn      lane = output channel (two for Cout > 64): fma chain, scale / shift, ReLU, max + first-argmax over the rows
//   pillar_moments  sum f and sum f f^T over the occupied rows in fp64 (per-workgroup partials + one finishing pass): the exact batch
//                   statistics of the pre-BN activations, mean_c = w_c . mu + b_c, var_c = w_c^T Cov w_c, without ever writing
//                   the rows x Cout activation
//   pillar_bwd      canvas gradient -> the argmax row of each (pillar, channel) through the ReLU: sum dy, sum dy x_hat and
//                   A = sum dy f (sparse, one row per pillar and channel), fp64 partials; the finishing pass turns them into
//                   dW = g invstd (A - sum(dy) mu - sum(dy x_hat) invstd Cov w), db, dgamma, dbeta (no per-row pass)
// Every reduction runs in a fixed order (no atomics): two launches give identical bits.
#include "common.h"

namespace {

constexpr int KMAX = 16;                 // decorated channels per row in LDS (K = C + 5 <= 16)
constexpr int WAVES = 4;                 // pillar slots per workgroup
constexpr int NWG_MAX = 256;             // workgroups of the reduction kernels (= partial rows)

struct PillarArgs {
  const float* feats;                    // [B][Nv][P][C]
  const long long* coords;               // [B][Nv][3] (z, y, x)
  const int* npts;                       // [B][Nv]
  const int* nvox;                       // [B]
  int B, Nv, P, C, H, W;
  float x0, y0, vx, vy;
};

// Stage slot `slot`'s decorated rows (rows < n) into this wave's LDS image [P][KMAX]; returns n, the pillar's cell in cy / cx.
template <int C>
__device__ int stage_pillar(const PillarArgs& a, long long slot, float* rows, int lane, int& cy, int& cx) {
  const int nr = a.npts[slot];
  const int n = nr < 0 ? 0 : (nr > a.P ? a.P : nr);
  cy = (int)a.coords[slot * 3 + 1];
  cx = (int)a.coords[slot * 3 + 2];
  const float* src = a.feats + (size_t)slot * a.P * C;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int p = lane; p < n; p += 64) {
#pragma unroll
    for (int c = 0; c < C; ++c) rows[p * KMAX + c] = src[(size_t)p * C + c];
    sx += rows[p * KMAX + 0];
    sy += rows[p * KMAX + 1];
    sz += rows[p * KMAX + 2];
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {                         // fixed butterfly: every lane holds the same sums
    sx += __shfl_xor(sx, s);
    sy += __shfl_xor(sy, s);
    sz += __shfl_xor(sz, s);
  }
  const float mx = n > 0 ? (float)(sx / n) : 0.f, my = n > 0 ? (float)(sy / n) : 0.f, mz = n > 0 ? (float)(sz / n) : 0.f;
  const float xc = a.x0 + ((float)cx + 0.5f) * a.vx, yc = a.y0 + ((float)cy + 0.5f) * a.vy;
  for (int p = lane; p < n; p += 64) {                       // the lane that wrote row p decorates it
    float* r = rows + p * KMAX;
    const float x = r[0], y = r[1], z = r[2];
    r[C + 0] = x - mx;
    r[C + 1] = y - my;
    r[C + 2] = z - mz;
    r[C + 3] = x - xc;
    r[C + 4] = y - yc;
  }
  return n;
}

// w_c . f in one fixed fma order (forward and backward evaluate the same chain: the same ReLU decision)
template <int K>
__device__ __forceinline__ float row_dot(const float* r, const float (&w)[K]) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) acc = fmaf(r[k], w[k], acc);
  return acc;
}

// slot -> (b, v, active) for the wave; all waves of a workgroup walk the same number of slot groups (barriers stay uniform)
__device__ __forceinline__ bool slot_active(const PillarArgs& a, long long slot, long long total, int& b) {
  if (slot >= total) return false;
  b = (int)(slot / a.Nv);
  const int v = (int)(slot - (long long)b * a.Nv);
  return v < a.nvox[b];
}

template <int C>
__global__ __launch_bounds__(256) void pillar_pfn(const PillarArgs a, const float* __restrict__ w, const float* __restrict__ scale,
                                                   const float* __restrict__ shift, int Cout, float* __restrict__ yf,
                                                   __bf16* __restrict__ yb, unsigned char* __restrict__ amax) {
  constexpr int K = C + 5;
  extern __shared__ double lds_d[];
  float* lds = reinterpret_cast<float*>(lds_d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* rows = lds + wave * a.P * KMAX;
  float wv[2][K], sc[2], sh[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = lane + 64 * j;
    const bool live = c < Cout;
#pragma unroll
    for (int k = 0; k < K; ++k) wv[j][k] = live ? w[c * K + k] : 0.f;
    sc[j] = live ? scale[c] : 0.f;
    sh[j] = live ? shift[c] : 0.f;
  }
  const long long total = (long long)a.B * a.Nv;
  for (long long base = (long long)blockIdx.x * WAVES; base < total; base += (long long)gridDim.x * WAVES) {
    const long long slot = base + wave;
    int b = 0, n = 0, cy = 0, cx = 0;
    bool active = slot_active(a, slot, total, b);
    if (active) n = stage_pillar<C>(a, slot, rows, lane, cy, cx);
    __syncthreads();
    if (active && cy >= 0 && cy < a.H && cx >= 0 && cx < a.W) {
      float m[2] = {0.f, 0.f};
      int arg[2] = {0, 0};
      for (int p = 0; p < n; ++p) {
        float f[K];
#pragma unroll
        for (int k = 0; k < K; ++k) f[k] = rows[p * KMAX + k];            // broadcast reads
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float v = fmaf(row_dot<K>(f, wv[j]), sc[j], sh[j]);
          v = !(v > 0.f) ? 0.f : v;
          if (p == 0 || v > m[j]) { m[j] = v; arg[j] = p; }
        }
      }
      if (n < a.P) {                                                        // the padding rows: all identical, f = 0
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float v = fmaf(0.f, sc[j], sh[j]);
          v = !(v > 0.f) ? 0.f : v;
          if (n == 0 || v > m[j]) { m[j] = v; arg[j] = n; }
        }
      }
      const size_t cell = ((size_t)b * a.H + cy) * a.W + cx;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c < Cout) {
          if (yb) yb[cell * Cout + c] = (__bf16)m[j];
          else yf[cell * Cout + c] = m[j];
          if (amax) amax[(size_t)slot * Cout + c] = (unsigned char)arg[j];
        }
      }
    }
    __syncthreads();                                                        // the LDS rows are restaged next round
  }
}

template <int C>
__global__ __launch_bounds__(256) void pillar_moments(const PillarArgs a, double* __restrict__ part) {
  constexpr int K = C + 5, NE = K + K * K, NQ = (NE + 63) / 64;
  extern __shared__ double lds_d[];
  float* lds = reinterpret_cast<float*>(lds_d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* rows = lds + wave * a.P * KMAX;
  int ei[NQ], ej[NQ];                                     // entry e < K: sum f_e (ej = -1); else (f f^T)[i][j]
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = lane + 64 * q;
    ei[q] = e < K ? e : (e < NE ? (e - K) / K : -1);
    ej[q] = e < K ? -1 : (e < NE ? (e - K) % K : -1);
  }
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  const long long total = (long long)a.B * a.Nv;
  for (long long base = (long long)blockIdx.x * WAVES; base < total; base += (long long)gridDim.x * WAVES) {
    const long long slot = base + wave;
    int b = 0, n = 0, cy = 0, cx = 0;
    const bool active = slot_active(a, slot, total, b);
    if (active) n = stage_pillar<C>(a, slot, rows, lane, cy, cx);
    __syncthreads();
    for (int p = 0; p < n; ++p) {
      const float* r = rows + p * KMAX;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (ei[q] < 0) continue;
        const double fi = (double)r[ei[q]];
        acc[q] += ej[q] < 0 ? fi : fi * (double)r[ej[q]];
      }
    }
    __syncthreads();
  }
  double* red = lds_d;                                    // waves added in order: reproducible
  for (int wv = 0; wv < WAVES; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int e = lane + 64 * q;
        if (e < NE) red[e] = (wv == 0 ? 0.0 : red[e]) + acc[q];
      }
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < NE; e += 256) part[(size_t)blockIdx.x * NE + e] = red[e];
}

// one workgroup: partials -> mu, Cov (fp64, kept for the backward) -> per-channel batch statistics, scale / shift of the forward,
// running buffers (torch's rule: momentum, unbiased variance; momentum < 0 = cumulative average) and num_batches_tracked
__global__ __launch_bounds__(256) void pillar_moments_finish(const double* __restrict__ part, int nwg, int K, const int* __restrict__ nvox,
                                                             int B, int P, const float* __restrict__ w, const float* __restrict__ bias,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, int Cout,
                                                             float eps, float momentum, float* rmean, float* rvar, long long* nbt,
                                                             double* __restrict__ mom, float* __restrict__ mean, float* __restrict__ invstd,
                                                             float* __restrict__ scale, float* __restrict__ shift) {
  __shared__ double S[KMAX + KMAX * KMAX];
  __shared__ double mu[KMAX], cov[KMAX * KMAX];
  __shared__ double Nrows;
  const int tid = threadIdx.x, NE = K + K * K;
  for (int e = tid; e < NE; e += 256) {
    double s = 0.0;
    for (int g = 0; g < nwg; ++g) s += part[(size_t)g * NE + e];
    S[e] = s;
  }
  if (tid == 0) {
    long long cnt = 0;
    for (int b = 0; b < B; ++b) cnt += nvox[b];
    Nrows = (double)cnt * P;
  }
  __syncthreads();
  const double N = Nrows, inv = N > 0.0 ? 1.0 / N : 0.0;
  if (tid < KMAX) mu[tid] = tid < K ? S[tid] * inv : 0.0;
  __syncthreads();
  {
    const int i = tid >> 4, j = tid & 15;
    cov[tid] = (i < K && j < K) ? S[K + i * K + j] * inv - mu[i] * mu[j] : 0.0;
  }
  const long long nb_old = nbt ? *nbt : 0;
  __syncthreads();
  if (tid < KMAX) mom[tid] = mu[tid];
  mom[KMAX + tid] = cov[tid];
  for (int c = tid; c < Cout; c += 256) {
    const float* wc = w + c * K;
    const double bc = bias ? (double)bias[c] : 0.0;
    double m = bc, var = 0.0;
    for (int i = 0; i < K; ++i) {
      m += (double)wc[i] * mu[i];
      double t = 0.0;
      for (int j = 0; j < K; ++j) t += cov[i * KMAX + j] * (double)wc[j];
      var += (double)wc[i] * t;
    }
    var = var > 0.0 ? var : 0.0;
    const double is = 1.0 / sqrt(var + (double)eps);
    const double g = gamma ? (double)gamma[c] : 1.0, be = beta ? (double)beta[c] : 0.0;
    mean[c] = (float)m;
    invstd[c] = (float)is;
    scale[c] = (float)(g * is);
    shift[c] = (float)(be + (bc - m) * g * is);
    if (rmean && rvar) {
      const double mo = momentum >= 0.f ? (double)momentum : 1.0 / (double)(nb_old + 1);
      const double unb = N > 1.0 ? var * N / (N - 1.0) : var;
      rmean[c] = (float)((1.0 - mo) * (double)rmean[c] + mo * m);
      rvar[c] = (float)((1.0 - mo) * (double)rvar[c] + mo * unb);
    }
  }
  if (tid == 0 && nbt) *nbt = nb_old + 1;
}

template <int C>
__global__ __launch_bounds__(256) void pillar_bwd(const PillarArgs a, const float* __restrict__ dcanvas, const unsigned char* __restrict__ amax,
                                                   const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ scale,
                                                   const float* __restrict__ shift, const float* __restrict__ mean,
                                                   const float* __restrict__ invstd, int Cout, double* __restrict__ part) {
  constexpr int K = C + 5, NA = K + 2;                     // per channel: A[K], sum dy, sum dy x_hat
  extern __shared__ double lds_d[];
  float* lds = reinterpret_cast<float*>(lds_d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* rows = lds + wave * a.P * KMAX;
  float wv[2][K], sc[2], sh[2];
  double bb[2], mn[2], is[2];
  double A[2][K], sdy[2], sdx[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = lane + 64 * j;
    const bool live = c < Cout;
#pragma unroll
    for (int k = 0; k < K; ++k) { wv[j][k] = live ? w[c * K + k] : 0.f; A[j][k] = 0.0; }
    sc[j] = live ? scale[c] : 0.f;
    sh[j] = live ? shift[c] : 0.f;
    bb[j] = (live && bias) ? (double)bias[c] : 0.0;
    mn[j] = live ? (double)mean[c] : 0.0;
    is[j] = live ? (double)invstd[c] : 0.0;
    sdy[j] = sdx[j] = 0.0;
  }
  const long long total = (long long)a.B * a.Nv;
  for (long long base = (long long)blockIdx.x * WAVES; base < total; base += (long long)gridDim.x * WAVES) {
    const long long slot = base + wave;
    int b = 0, n = 0, cy = 0, cx = 0;
    const bool active = slot_active(a, slot, total, b);
    if (active) n = stage_pillar<C>(a, slot, rows, lane, cy, cx);
    __syncthreads();
    if (active && cy >= 0 && cy < a.H && cx >= 0 && cx < a.W) {
      const size_t cell = ((size_t)b * a.H + cy) * a.W + cx;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c >= Cout) continue;
        const int r = amax[(size_t)slot * Cout + c];
        float f[K];
#pragma unroll
        for (int k = 0; k < K; ++k) f[k] = r < n ? rows[r * KMAX + k] : 0.f;
        const float acc = r < n ? row_dot<K>(f, wv[j]) : 0.f;
        const float v = fmaf(acc, sc[j], sh[j]);
        const float g = v > 0.f ? dcanvas[cell * Cout + c] : 0.f;       // through the ReLU
        if (g != 0.f) {
          const double gd = (double)g, xh = ((double)acc + bb[j] - mn[j]) * is[j];
#pragma unroll
          for (int k = 0; k < K; ++k) A[j][k] += gd * (double)f[k];
          sdy[j] += gd;
          sdx[j] += gd * xh;
        }
      }
    }
    __syncthreads();
  }
  double* red = lds_d;                                   // [Cout][NA], waves added in order
  for (int wq = 0; wq < WAVES; ++wq) {
    if (wave == wq) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c >= Cout) continue;
        double* d = red + c * NA;
#pragma unroll
        for (int k = 0; k < K; ++k) d[k] = (wq == 0 ? 0.0 : d[k]) + A[j][k];
        d[K] = (wq == 0 ? 0.0 : d[K]) + sdy[j];
        d[K + 1] = (wq == 0 ? 0.0 : d[K + 1]) + sdx[j];
      }
    }
    __syncthreads();
  }
  const int tot = Cout * NA;
  for (int e = threadIdx.x; e < tot; e += 256) part[(size_t)blockIdx.x * tot + e] = red[e];
}

// thread = (channel c, entry k < K + 2): the partials summed in workgroup order, then the closed forms of the header
__global__ __launch_bounds__(256) void pillar_bwd_finish(const double* __restrict__ part, int nwg, int K, int Cout, const double* __restrict__ mom,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         const float* __restrict__ gamma, int frozen, float* __restrict__ dw,
                                                         float* __restrict__ db, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int NA = K + 2, tot = Cout * NA;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= tot) return;
  const int c = e / NA, k = e - c * NA;
  double s = 0.0, sdy = 0.0, sdx = 0.0;
  for (int g = 0; g < nwg; ++g) {
    const double* p = part + (size_t)g * tot + c * NA;
    s += p[k];
    sdy += p[K];
    sdx += p[K + 1];
  }
  const double is = (double)invstd[c], gi = (gamma ? (double)gamma[c] : 1.0) * is;
  const float* wc = w + c * K;
  if (k < K) {
    double v = s;
    if (!frozen) {
      double covw = 0.0;
      for (int j = 0; j < K; ++j) covw += mom[KMAX + k * KMAX + j] * (double)wc[j];
      v = s - sdy * mom[k] - sdx * is * covw;
    }
    dw[c * K + k] = (float)(gi * v);
  } else if (k == K) {
    double v = sdy;
    if (!frozen) {                                      // sum_i dx_i: zero analytically (sum x_hat = 0); the computed value
      double xs = (bias ? (double)bias[c] : 0.0) - (double)mean[c];
      for (int j = 0; j < K; ++j) xs += (double)wc[j] * mom[j];
      v = sdy - sdy - sdx * is * xs;
    }
    db[c] = (float)(gi * v);
  } else {
    dgamma[c] = (float)sdx;
    dbeta[c] = (float)sdy;
  }
}

int pillar_check(const bevf_pillar_geom* g, int Cout) {
  BEVF_REQUIRE(g && g->voxel_features && g->voxel_coords && g->num_points && g->num_voxels, "pillars: null pointer");
  BEVF_REQUIRE(g->B > 0 && g->Nv > 0 && g->H > 0 && g->W > 0, "pillars: empty shape");
  BEVF_REQUIRE(g->C >= 3 && g->C + 5 <= KMAX, "pillars: need 3 <= C <= 11 point channels (C=%d)", g->C);
  BEVF_REQUIRE(g->P > 0 && g->P <= 255, "pillars: need 0 < max_points <= 255 (P=%d)", g->P);
  BEVF_REQUIRE(Cout > 0 && Cout <= 128 && Cout % 32 == 0, "pillars: Cout must be a multiple of 32 up to 128 (Cout=%d)", Cout);
  BEVF_REQUIRE((long long)g->B * g->H * g->W * Cout < (1ll << 31) && (long long)g->B * g->Nv * g->P * g->C < (1ll << 40),
               "pillars: canvas too large");
  BEVF_REQUIRE(g->vx > 0.f && g->vy > 0.f, "pillars: pillar sizes must be positive");
  return BEVF_OK;
}

PillarArgs pillar_args(const bevf_pillar_geom* g) {
  PillarArgs a;
  a.feats = g->voxel_features; a.coords = reinterpret_cast<const long long*>(g->voxel_coords);
  a.npts = g->num_points; a.nvox = g->num_voxels;
  a.B = g->B; a.Nv = g->Nv; a.P = g->P; a.C = g->C; a.H = g->H; a.W = g->W;
  a.x0 = g->x0; a.y0 = g->y0; a.vx = g->vx; a.vy = g->vy;
  return a;
}

size_t stage_bytes(int P) { return (size_t)WAVES * P * KMAX * sizeof(float); }

int reduce_grid(const PillarArgs& a) {
  const long long groups = ((long long)a.B * a.Nv + WAVES - 1) / WAVES;
  return (int)(groups < NWG_MAX ? groups : NWG_MAX);
}

#define BEVF_PILLAR_SWITCH(C_, CALL) \
  switch (C_) { case 3: CALL(3) case 4: CALL(4) case 5: CALL(5) case 6: CALL(6) case 7: CALL(7) case 8: CALL(8) \
                case 9: CALL(9) case 10: CALL(10) case 11: CALL(11) default: break; }

}  // namespace

extern "C" size_t bevf_pillar_work_bytes(int Cout) {
  const int per = Cout * (KMAX + 2) > KMAX + KMAX * KMAX ? Cout * (KMAX + 2) : KMAX + KMAX * KMAX;
  return (size_t)NWG_MAX * per * sizeof(double) + 256;
}

extern "C" int bevf_pillar_pfn_f32(const bevf_pillar_geom* g, const float* w, const float* scale, const float* shift, int Cout,
                                   void* canvas, int canvas_bf16, uint8_t* argmax, void* stream) {
  if (int rc = pillar_check(g, Cout)) return rc;
  BEVF_REQUIRE(w && scale && shift && canvas, "pillar_pfn: null pointer");
  const PillarArgs a = pillar_args(g);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t es = canvas_bf16 ? 2 : 4;
  if (hipMemsetAsync(canvas, 0, (size_t)a.B * a.H * a.W * Cout * es, st) != hipSuccess) {     // empty cells are exactly 0
    bevf_set_error("pillar_pfn: memset failed");
    return BEVF_ERR_LAUNCH;
  }
  const long long groups = ((long long)a.B * a.Nv + WAVES - 1) / WAVES;
  const dim3 grid((unsigned)(groups < 4096 ? groups : 4096));
  float* yf = canvas_bf16 ? nullptr : static_cast<float*>(canvas);
  __bf16* yb = canvas_bf16 ? static_cast<__bf16*>(canvas) : nullptr;
#define BEVF_PFN(Cv) hipLaunchKernelGGL(pillar_pfn<Cv>, grid, dim3(256), stage_bytes(a.P), st, a, w, scale, shift, Cout, yf, yb, argmax); break;
  BEVF_PILLAR_SWITCH(a.C, BEVF_PFN)
#undef BEVF_PFN
  return bevf_check_launch("bevf_pillar_pfn_f32");
}

extern "C" int bevf_pillar_moments_f32(const bevf_pillar_geom* g, const float* w, const float* bias, const float* gamma, const float* beta,
                                       int Cout, float eps, float momentum, float* running_mean, float* running_var,
                                       int64_t* num_batches_tracked, double* moments, float* mean, float* invstd, float* scale,
                                       float* shift, void* work, void* stream) {
  if (int rc = pillar_check(g, Cout)) return rc;
  BEVF_REQUIRE(w && moments && mean && invstd && scale && shift && work, "pillar_moments: null pointer");
  const PillarArgs a = pillar_args(g);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work) + 255) & ~uintptr_t(255));
  const int nwg = reduce_grid(a);
  const int K = a.C + 5;
  const size_t lds = stage_bytes(a.P) > (size_t)(K + K * K) * 8 ? stage_bytes(a.P) : (size_t)(K + K * K) * 8;
#define BEVF_MOM(Cv) hipLaunchKernelGGL(pillar_moments<Cv>, dim3(nwg), dim3(256), lds, st, a, part); break;
  BEVF_PILLAR_SWITCH(a.C, BEVF_MOM)
#undef BEVF_MOM
  hipLaunchKernelGGL(pillar_moments_finish, dim3(1), dim3(256), 0, st, part, nwg, K, a.nvox, a.B, a.P, w, bias, gamma, beta, Cout,
                     eps, momentum, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), moments, mean,
                     invstd, scale, shift);
  return bevf_check_launch("bevf_pillar_moments_f32");
}

extern "C" int bevf_pillar_pfn_backward_f32(const bevf_pillar_geom* g, const float* dcanvas, const uint8_t* argmax, const float* w,
                                            const float* bias, const float* scale, const float* shift, const float* mean,
                                            const float* invstd, const float* gamma, const double* moments, int Cout, int frozen,
                                            float* dw, float* db, float* dgamma, float* dbeta, void* work, void* stream) {
  if (int rc = pillar_check(g, Cout)) return rc;
  BEVF_REQUIRE(dcanvas && argmax && w && scale && shift && mean && invstd && (frozen || moments) && dw && db && dgamma && dbeta && work,
               "pillar_backward: null pointer");
  const PillarArgs a = pillar_args(g);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(work) + 255) & ~uintptr_t(255));
  const int nwg = reduce_grid(a);
  const int K = a.C + 5;
  const size_t red = (size_t)Cout * (K + 2) * 8;
  const size_t lds = stage_bytes(a.P) > red ? stage_bytes(a.P) : red;
#define BEVF_BWD(Cv) hipLaunchKernelGGL(pillar_bwd<Cv>, dim3(nwg), dim3(256), lds, st, a, dcanvas, argmax, w, bias, scale, shift, mean, invstd, \
                                        Cout, part); break;
  BEVF_PILLAR_SWITCH(a.C, BEVF_BWD)
#undef BEVF_BWD
  const int tot = Cout * (K + 2);
  hipLaunchKernelGGL(pillar_bwd_finish, dim3((tot + 255) / 256), dim3(256), 0, st, part, nwg, K, Cout, moments, w, bias, mean, invstd,
                     gamma, frozen, dw, db, dgamma, dbeta);
  return bevf_check_launch("bevf_pillar_pfn_backward_f32");
}
