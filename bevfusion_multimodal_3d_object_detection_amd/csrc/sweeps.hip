// Multi-sweep LiDAR accumulation on the device: the key sweep and the preceding sweeps of every frame, each moved into
// the key sweep's sensor frame, merged into one padded cloud whose last channel is the sweep's time lag.
//
// sweep_pose_chain: T[b][s] = inv(L_k) . inv(E_k) . E_s . L_s from the four calibration tensors, fp64, one thread per (frame, sweep).
// msw_count:  keep = inside the sweep's count, not close to the sensor, in range after the transform; one int per tile of 1024 rows.
// scan_counts (scan_counts.h): the frame's exclusive scan over its S * tiles tile counts, sweep-major: a row's position in the output.
// msw_write:  the survivors straight into out, sweep 0 first, each sweep in point order; rows from max_points on are not stored.
// msw_pad:    zero rows from the last survivor to max_points.
// No atomics, no buffer proportional to the points, every grid a function of (B, S, N): the sequence can be captured and replayed.
//
// The point transform, everywhere in this file (m = the top 3 x 4 of the sweep's fp64 4 x 4, row-major):
//   x' = (float)(((m[0] * (double)x + m[1] * (double)y) + m[2] * (double)z) + m[3])        (rows 1 and 2 alike)
// in exactly this order with contraction off for the file: the numpy restatement (tests/sweeps_ref.py) reproduces it bit for bit.
#include "common.h"
#include "point_compact.h"
#include "scan_counts.h"

#pragma clang fp contract(off)

namespace {

struct Rigid {
  double m[12];
};
__device__ __forceinline__ Rigid load_rigid(const double* __restrict__ mat, size_t sweep) {
  Rigid t;
#pragma unroll
  for (int i = 0; i < 12; ++i) t.m[i] = mat[16 * sweep + i];
  return t;
}
// pts: the sweep's rows.  close_r <= 0 (or NaN) switches the close-point test off; a NaN coordinate fails the range test.
// V4: C == 4 and 16-byte aligned rows (chosen on the host): the row is one 16-byte load and w is its channel 3.
template <bool V4>
__device__ __forceinline__ bool msw_keep(const float* __restrict__ pts, int i, int n, int C, const Rigid& t, float close_r, const Range6& r,
                                         float& px, float& py, float& pz, float& w) {
  if (i >= n) return false;
  float x, y, z;
  if constexpr (V4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(pts + (size_t)i * 4);
    x = v[0], y = v[1], z = v[2], w = v[3];
  } else {
    x = pts[(size_t)i * C], y = pts[(size_t)i * C + 1], z = pts[(size_t)i * C + 2];
  }
  if (close_r > 0.f && fabsf(x) < close_r && fabsf(y) < close_r) return false;
  const double dx = (double)x, dy = (double)y, dz = (double)z;
  px = (float)(((t.m[0] * dx + t.m[1] * dy) + t.m[2] * dz) + t.m[3]);
  py = (float)(((t.m[4] * dx + t.m[5] * dy) + t.m[6] * dz) + t.m[7]);
  pz = (float)(((t.m[8] * dx + t.m[9] * dy) + t.m[10] * dz) + t.m[11]);
  return in_range(r, px, py, pz);
}

// grid (tiles, S, B); tcount [B][S * tiles]
template <bool V4>
__global__ __launch_bounds__(PC_TILE) void msw_count(const float* __restrict__ pts, const int* __restrict__ counts,
                                                     const double* __restrict__ mat, int* __restrict__ tcount, int N, int C, float close_r,
                                                     Range6 rg) {
  const size_t sweep = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  const Rigid t = load_rigid(mat, sweep);
  float px, py, pz, w;
  tile_count(msw_keep<V4>(pts + sweep * N * C, blockIdx.x * PC_TILE + threadIdx.x, frame_rows(counts, sweep, N), C, t, close_r, rg, px, py,
                          pz, w),
             tcount + sweep * gridDim.x + blockIdx.x);
}

// grid (tiles, S, B); rp [B][S * tiles + 1] from scan_counts; out [B][max_points][C + 1]; count [B]; sweep_count [B][S]
template <bool V4>
__global__ __launch_bounds__(PC_TILE) void msw_write(const float* __restrict__ pts, const int* __restrict__ counts,
                                                     const double* __restrict__ mat, const float* __restrict__ lag,
                                                     const int* __restrict__ rp, float* __restrict__ out, int* __restrict__ count,
                                                     int* __restrict__ sweep_count, int N, int C, int max_points, float close_r, Range6 rg) {
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, tiles = gridDim.x, s = blockIdx.y, S = gridDim.y, b = blockIdx.z;
  const size_t sweep = (size_t)b * S + s;
  const int* const frp = rp + (size_t)b * ((size_t)S * tiles + 1);
  if (tile == 0 && tid == 0) {
    sweep_count[sweep] = frp[(size_t)(s + 1) * tiles] - frp[(size_t)s * tiles];
    if (s == 0) count[b] = frp[(size_t)S * tiles];
  }
  const int start = frp[(size_t)s * tiles + tile];
  if (start >= max_points) return;                                   // the same in every thread: a truncated tile reads no point
  const Rigid t = load_rigid(mat, sweep);
  const float* const sp = pts + sweep * N * C;
  const int i = tile * PC_TILE + tid;
  float px = 0.f, py = 0.f, pz = 0.f, w = 0.f;
  const bool keep = msw_keep<V4>(sp, i, frame_rows(counts, sweep, N), C, t, close_r, rg, px, py, pz, w);
  const int row = tile_rank(keep, start).row;
  if (keep && row < max_points) {                                    // row < max_points: inside the frame's rows of out
    float* const dst = out + ((size_t)b * max_points + row) * (C + 1);
    dst[0] = px, dst[1] = py, dst[2] = pz;
    if constexpr (V4) {
      dst[3] = w;
    } else {
      for (int c = 3; c < C; ++c) dst[c] = sp[(size_t)i * C + c];
    }
    dst[C] = lag[sweep];
  }
}

// grid (blocks, B): zero rows min(count[b], max_points) .. max_points of out [B][max_points][row]
__global__ __launch_bounds__(256) void msw_pad(float* __restrict__ out, const int* __restrict__ count, int row, int max_points) {
  const int b = blockIdx.y;
  const int total = count[b];
  const long long lo = (long long)(total < 0 ? 0 : (total > max_points ? max_points : total)) * row, hi = (long long)max_points * row;
  float* const o = out + (size_t)b * hi;
  for (long long e = lo + blockIdx.x * 256ll + threadIdx.x; e < hi; e += (long long)gridDim.x * 256) o[e] = 0.f;
}

// ---- pose chain ---------------------------------------------------------------------------------------------------------------------
// A 4 x 4 whose bottom row is taken as 0 0 0 1 (the inputs' own bottom rows are not read).
struct Mat4 {
  double a[16];
};
__device__ __forceinline__ Mat4 load_pose(const double* __restrict__ p) {
  Mat4 m;
#pragma unroll
  for (int i = 0; i < 12; ++i) m.a[i] = p[i];
  m.a[12] = 0.0, m.a[13] = 0.0, m.a[14] = 0.0, m.a[15] = 1.0;
  return m;
}
// the rigid inverse (R^T, -(R^T t)), each element of R^T t = ((r0 t0 + r1 t1) + r2 t2)
__device__ __forceinline__ Mat4 rigid_inverse(const Mat4& m) {
  Mat4 o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.a[4 * i + j] = m.a[4 * j + i];
    o.a[4 * i + 3] = -((m.a[i] * m.a[3] + m.a[4 + i] * m.a[7]) + m.a[8 + i] * m.a[11]);
  }
  o.a[12] = 0.0, o.a[13] = 0.0, o.a[14] = 0.0, o.a[15] = 1.0;
  return o;
}
// rows 0-2 of x . y, element = (((a0 b0 + a1 b1) + a2 b2) + a3 b3); bottom row 0 0 0 1
__device__ __forceinline__ Mat4 mul_pose(const Mat4& x, const Mat4& y) {
  Mat4 o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o.a[4 * i + j] = ((x.a[4 * i] * y.a[j] + x.a[4 * i + 1] * y.a[4 + j]) + x.a[4 * i + 2] * y.a[8 + j]) + x.a[4 * i + 3] * y.a[12 + j];
  o.a[12] = 0.0, o.a[13] = 0.0, o.a[14] = 0.0, o.a[15] = 1.0;
  return o;
}
__device__ __forceinline__ bool same_pose(const Mat4& x, const Mat4& y) {
  bool same = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) same = same && x.a[i] == y.a[i];
  return same;
}

// kl / ke [B][4][4], sl / se [B][S][4][4] -> out [B][S][4][4]; n = B * S
__global__ __launch_bounds__(256) void sweep_pose_chain(const double* __restrict__ kl, const double* __restrict__ ke, const double* __restrict__ sl,
                                                        const double* __restrict__ se, double* __restrict__ out, int S, int n) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int b = e / S;
  const Mat4 Lk = load_pose(kl + 16 * (size_t)b), Ek = load_pose(ke + 16 * (size_t)b);
  const Mat4 Ls = load_pose(sl + 16 * (size_t)e), Es = load_pose(se + 16 * (size_t)e);
  Mat4 t;
  if (same_pose(Ls, Lk) && same_pose(Es, Ek)) {                      // the key sweep itself: the exact identity, its points keep their bits
#pragma unroll
    for (int i = 0; i < 16; ++i) t.a[i] = (i % 5 == 0) ? 1.0 : 0.0;
  } else {
    t = mul_pose(rigid_inverse(Lk), mul_pose(rigid_inverse(Ek), mul_pose(Es, Ls)));
  }
  double* const o = out + 16 * (size_t)e;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = t.a[i];
}

}  // namespace

extern "C" size_t bevf_sweeps_merge_work_bytes(int B, int S, int N) {
  if (B <= 0 || S <= 0 || N < 0) return 0;
  const size_t per_frame = (size_t)S * point_tiles(N);
  return sizeof(int32_t) * (size_t)B * (2 * per_frame + 1);         // tcount [B][S * tiles], then rp [B][S * tiles + 1]
}

extern "C" int bevf_sweeps_merge_f32(const float* points, const int32_t* counts, const double* sweep_to_key, const float* time_lag, float* out,
                                     int32_t* count, int32_t* sweep_count, void* work, int B, int S, int N, int C, int max_points,
                                     float close_radius, const float* pc_range6, void* stream) {
  BEVF_REQUIRE((points || N == 0) && counts && sweep_to_key && time_lag && out && count && sweep_count && work && pc_range6,
               "sweeps_merge: null pointer");
  BEVF_REQUIRE(B > 0 && B < 65536 && S > 0 && S < 65536 && N >= 0 && C >= 3 && C <= 8 && max_points > 0,
               "sweeps_merge: need 0 < B, S < 65536, N >= 0, 3 <= C <= 8, max_points > 0");
  BEVF_REQUIRE((long long)S * N < (1ll << 31) && (long long)B * S < (1ll << 31), "sweeps_merge: S * N and B * S must stay below 2^31");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles = point_tiles(N);
  int* const tcount = static_cast<int*>(work);
  int* const rp = tcount + (size_t)B * S * tiles;
  const Range6 rg = range6(pc_range6);
  if (tiles > 0) {
    bevf_dispatch_bool(C == 4 && bevf_aligned16(points), [&](auto v4) {   // a sweep's rows start at a multiple of N * 16 bytes
      constexpr bool V4 = decltype(v4)::value;
      hipLaunchKernelGGL(msw_count<V4>, dim3(tiles, S, B), dim3(PC_TILE), 0, st, points, counts, sweep_to_key, tcount, N, C, close_radius, rg);
      hipLaunchKernelGGL(scan_counts, dim3(B), dim3(1024), 0, st, (const int32_t*)tcount, S * tiles, rp);
      hipLaunchKernelGGL(msw_write<V4>, dim3(tiles, S, B), dim3(PC_TILE), 0, st, points, counts, sweep_to_key, time_lag, (const int*)rp, out,
                         count, sweep_count, N, C, max_points, close_radius, rg);
      return 0;
    });
  } else {
    (void)hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)B, st);
    (void)hipMemsetAsync(sweep_count, 0, sizeof(int32_t) * (size_t)B * S, st);
  }
  const long long n = (long long)max_points * (C + 1);
  hipLaunchKernelGGL(msw_pad, dim3((unsigned)((n + 255) / 256 < 512 ? (n + 255) / 256 : 512), B), dim3(256), 0, st, out, (const int*)count,
                     C + 1, max_points);
  return bevf_check_launch("bevf_sweeps_merge_f32");
}

extern "C" int bevf_sweep_pose_chain_f64(const double* key_lidar2ego, const double* key_ego2global, const double* sweep_lidar2ego,
                                         const double* sweep_ego2global, double* sweep_to_key, int B, int S, void* stream) {
  BEVF_REQUIRE(key_lidar2ego && key_ego2global && sweep_lidar2ego && sweep_ego2global && sweep_to_key, "sweep_pose_chain: null pointer");
  BEVF_REQUIRE(B > 0 && B < 65536 && S > 0 && S < 65536 && (long long)B * S < (1ll << 31), "sweep_pose_chain: need 0 < B, S < 65536, B * S < 2^31");
  const int n = B * S;
  hipLaunchKernelGGL(sweep_pose_chain, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), key_lidar2ego, key_ego2global,
                     sweep_lidar2ego, sweep_ego2global, sweep_to_key, S, n);
  return bevf_check_launch("bevf_sweep_pose_chain_f64");
}
