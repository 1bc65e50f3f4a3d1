// Points-in-boxes and GT-paste (object-sample) augmentation on the device.
//
// Box convention, as everywhere: [x, y, z, w, l, h, yaw(, vx, vy)] -- l along the heading (cos yaw, sin yaw), w across it, z-extent
// [z - h/2, z + h/2].  Fused multiply-add contraction is off for this file; every fma is written out.
//
// A box is staged once as (cx, cy, cz, c, s, hl, hw, hh):  sincosf(yaw, &s, &c), hl = 0.5f * l, hw = 0.5f * w, hh = 0.5f * h.
//
// The 3-D containment test (points_in_boxes, and the remove step of the paste):
//   dx = px - cx, dy = py - cy, dz = pz - cz                         (one fp32 subtraction each)
//   lx = fmaf(dy, s, dx * c)                                          (d rotated by -yaw: along the heading)
//   ly = fmaf(dy, c, -(dx * s))                                       (across it)
//   inside = |lx| <= hl && |ly| <= hw && |dz| <= hh && w > 0 && l > 0 && h > 0
//   Every comparison is false for a NaN, so a NaN in the point or in the box gives "not inside".
//
// The BEV collision test of two rectangles a, b (paste_accept), the separating-axis test on the four edge directions, z ignored:
//   dx = bx - ax, dy = by - ay
//   cc = |fmaf(sa, sb, ca * cb)|, ss = |fmaf(ca, sb, -(sa * cb))|     (|cos|, |sin| of the angle between the headings)
//   separated = |fmaf(dy, sa, dx * ca)|    > hla + fmaf(hwb, ss, hlb * cc)
//            || |fmaf(dy, ca, -(dx * sa))| > hwa + fmaf(hwb, cc, hlb * ss)
//            || |fmaf(dy, sb, dx * cb)|    > hlb + fmaf(hwa, ss, hla * cc)
//            || |fmaf(dy, cb, -(dx * sb))| > hwb + fmaf(hwa, cc, hla * ss)
//   collide = !separated, so touching counts as a collision.  A rectangle with w <= 0, l <= 0, or a NaN or an infinity among
//   (x, y, w, l, yaw) collides with nothing.
//
// points_in_boxes: grid (point tiles of 256, frame); the frame's boxes go through LDS in chunks of 64, one thread per point, the
//   lowest box index wins.
// paste_accept: one workgroup per frame.  All (candidate, GT row) pairs in parallel, then wave 0 walks the candidates in order: an
//   accepted candidate k is broadcast and the lanes of the later candidates test themselves against it.  Also the exclusive prefix of the
//   accepted objects' point counts, and the output GT rows.
// paste_count / paste_compact: the order-preserving compaction of point_compact.h with "inside an accepted pasted box" as the drop
//   rule, written straight into the output.  paste_append: the accepted objects' points (bank row + centre, one
//   fp32 addition per coordinate) behind the survivors, zeros behind those, and the count.
#include "common.h"
#include "point_compact.h"

#pragma clang fp contract(off)

namespace {

constexpr int PIB_T = 256;    // points per workgroup of points_in_boxes
constexpr int PIB_CHUNK = 64; // boxes staged per round
constexpr int KC_MAX = 64;    // candidates per frame (one wave)

struct Box8 {
  float cx, cy, cz, c, s, hl, hw, hh;
};

// box: >= 7 floats.  A box that can hold nothing (size <= 0 or NaN) gets negative half extents.
__device__ __forceinline__ Box8 stage_box(const float* __restrict__ box, bool live) {
  Box8 q;
  q.cx = box[0], q.cy = box[1], q.cz = box[2];
  const float w = box[3], l = box[4], h = box[5];
  sincosf(box[6], &q.s, &q.c);
  const bool ok = live && w > 0.f && l > 0.f && h > 0.f;
  q.hl = ok ? 0.5f * l : -1.f;
  q.hw = ok ? 0.5f * w : -1.f;
  q.hh = ok ? 0.5f * h : -1.f;
  return q;
}
__device__ __forceinline__ bool inside_box(const Box8& q, float px, float py, float pz) {
  const float dx = px - q.cx, dy = py - q.cy, dz = pz - q.cz;
  const float lx = fmaf(dy, q.s, dx * q.c);
  const float ly = fmaf(dy, q.c, -(dx * q.s));
  return fabsf(lx) <= q.hl && fabsf(ly) <= q.hw && fabsf(dz) <= q.hh;
}

// grid (ceil(N / 256), B).  mask [B][M] (or null): rows < 0 are ignored.  idx [B][N].
__global__ __launch_bounds__(PIB_T) void points_in_boxes(const float* __restrict__ pts, const int* __restrict__ n_in,
                                                         const float* __restrict__ boxes, const int* __restrict__ mask,
                                                         int* __restrict__ idx, int N, int C, int M, int ncol) {
  __shared__ Box8 sb[PIB_CHUNK];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int i = blockIdx.x * PIB_T + tid;
  const bool live = i < frame_rows(n_in, b, N);
  float px = 0.f, py = 0.f, pz = 0.f;
  if (live) {
    const float* const p = pts + ((size_t)b * N + i) * C;
    px = p[0], py = p[1], pz = p[2];
  }
  int res = -1;
  for (int j0 = 0; j0 < M; j0 += PIB_CHUNK) {
    const int nj = M - j0 < PIB_CHUNK ? M - j0 : PIB_CHUNK;
    __syncthreads();                                                 // the previous chunk has been read
    if (tid < nj) {
      const size_t row = (size_t)b * M + j0 + tid;
      sb[tid] = stage_box(boxes + row * ncol, mask ? mask[row] >= 0 : true);
    }
    __syncthreads();
    if (live && res < 0) {
      for (int j = 0; j < nj; ++j) {
        if (inside_box(sb[j], px, py, pz)) {
          res = j0 + j;
          break;
        }
      }
    }
  }
  if (i < N) idx[(size_t)b * N + i] = res;
}

// ---- accept --------------------------------------------------------------------------------------------------------------------------
struct Rect {
  float x, y, c, s, hl, hw;
  bool ok;
};
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }   // false for NaN
__device__ __forceinline__ Rect load_rect(const float* __restrict__ box, bool live) {
  Rect r;
  r.x = box[0], r.y = box[1];
  const float w = box[3], l = box[4], yaw = box[6];
  sincosf(yaw, &r.s, &r.c);
  r.hl = 0.5f * l, r.hw = 0.5f * w;
  r.ok = live && w > 0.f && l > 0.f && finite_f(r.x) && finite_f(r.y) && finite_f(w) && finite_f(l) && finite_f(yaw);
  return r;
}
__device__ __forceinline__ bool collide(const Rect& a, const Rect& b) {
  if (!a.ok || !b.ok) return false;
  const float dx = b.x - a.x, dy = b.y - a.y;
  const float cc = fabsf(fmaf(a.s, b.s, a.c * b.c)), ss = fabsf(fmaf(a.c, b.s, -(a.s * b.c)));
  const bool separated = fabsf(fmaf(dy, a.s, dx * a.c)) > a.hl + fmaf(b.hw, ss, b.hl * cc) ||
                         fabsf(fmaf(dy, a.c, -(dx * a.s))) > a.hw + fmaf(b.hw, cc, b.hl * ss) ||
                         fabsf(fmaf(dy, b.s, dx * b.c)) > b.hl + fmaf(a.hw, ss, a.hl * cc) ||
                         fabsf(fmaf(dy, b.c, -(dx * b.s))) > b.hw + fmaf(a.hw, cc, a.hl * ss);
  return !separated;
}

// grid (B), 256 threads.  gt_* [B][M]..., bank_boxes [K][bcol], bank_labels [K], obj_ptr [K + 1], cand [B][Kc] (< 0 or >= K: none).
// accepted [B][Kc]; pre [B][Kc + 1] = exclusive prefix of the accepted objects' point counts, pre[Kc] = their total;
// out_boxes [B][M + Kc][ncol], out_labels [B][M + Kc], out_vel [B][M + Kc][2] (null with gt_vel null).
__global__ __launch_bounds__(256) void paste_accept(const float* __restrict__ gt_boxes, const long long* __restrict__ gt_labels,
                                                    const float* __restrict__ gt_vel, const float* __restrict__ bank_boxes,
                                                    const long long* __restrict__ bank_labels, const int* __restrict__ obj_ptr,
                                                    const int* __restrict__ cand, int* __restrict__ accepted, int* __restrict__ pre,
                                                    float* __restrict__ out_boxes, long long* __restrict__ out_labels,
                                                    float* __restrict__ out_vel, int M, int ncol, int K, int bcol, int Kc) {
  __shared__ int hit[KC_MAX], acc[KC_MAX], obj[KC_MAX];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float* const gb = gt_boxes + (size_t)b * M * ncol;
  const long long* const gl = gt_labels + (size_t)b * M;
  if (tid < KC_MAX) {
    int c = tid < Kc ? cand[(size_t)b * Kc + tid] : -1;
    if (c >= K) c = -1;
    obj[tid] = c;
    hit[tid] = 0;
  }
  __syncthreads();
  for (int e = tid; e < Kc * M; e += 256) {                          // every (candidate, GT row) pair
    const int k = e / M, j = e - k * M;
    if (obj[k] < 0 || gl[j] < 0) continue;
    if (collide(load_rect(bank_boxes + (size_t)obj[k] * bcol, true), load_rect(gb + (size_t)j * ncol, true))) hit[k] = 1;
  }
  __syncthreads();
  if (tid < KC_MAX) {                                                // wave 0: lane k owns candidate k
    const int k = tid, c = obj[k];
    Rect me = load_rect(bank_boxes + (size_t)(c < 0 ? 0 : c) * bcol, c >= 0);
    bool ok = c >= 0 && !hit[k];
    for (int a = 0; a < Kc; ++a) {
      if (!((__ballot(ok) >> a) & 1ull)) continue;                   // wave-uniform: a rejected candidate blocks nothing
      Rect o;
      o.x = __shfl(me.x, a), o.y = __shfl(me.y, a), o.c = __shfl(me.c, a), o.s = __shfl(me.s, a);
      o.hl = __shfl(me.hl, a), o.hw = __shfl(me.hw, a);
      o.ok = __shfl((int)me.ok, a) != 0;
      if (k > a && ok && collide(o, me)) ok = false;
    }
    const int cnt = ok ? obj_ptr[c + 1] - obj_ptr[c] : 0;
    int inc = cnt;
    for (int d = 1; d < KC_MAX; d <<= 1) {
      const int v = __shfl_up(inc, d);
      if (k >= d) inc += v;
    }
    acc[k] = ok ? 1 : 0;
    if (k < Kc) {
      accepted[(size_t)b * Kc + k] = ok ? 1 : 0;
      pre[(size_t)b * (Kc + 1) + k] = inc - cnt;
    }
    if (k == Kc - 1) pre[(size_t)b * (Kc + 1) + Kc] = inc;
  }
  __syncthreads();
  const int R = M + Kc;
  for (int e = tid; e < R * ncol; e += 256) {
    const int r = e / ncol, col = e - r * ncol;
    float v = 0.f;
    if (r < M) {
      v = gb[e];
    } else if (acc[r - M]) {
      v = col < bcol ? bank_boxes[(size_t)obj[r - M] * bcol + col] : 0.f;
    }
    out_boxes[(size_t)b * R * ncol + e] = v;
  }
  for (int r = tid; r < R; r += 256) {
    out_labels[(size_t)b * R + r] = r < M ? gl[r] : (acc[r - M] ? bank_labels[obj[r - M]] : -1ll);
    if (out_vel) {
      float vx = 0.f, vy = 0.f;
      if (r < M) {
        vx = gt_vel[((size_t)b * M + r) * 2], vy = gt_vel[((size_t)b * M + r) * 2 + 1];
      } else if (acc[r - M] && bcol == 9) {
        vx = bank_boxes[(size_t)obj[r - M] * 9 + 7], vy = bank_boxes[(size_t)obj[r - M] * 9 + 8];
      }
      out_vel[((size_t)b * R + r) * 2] = vx, out_vel[((size_t)b * R + r) * 2 + 1] = vy;
    }
  }
}

// ---- remove and append ---------------------------------------------------------------------------------------------------------------
// The accepted candidates' boxes of frame b, compacted in candidate order into sb[0 .. return value); wave 0 does it, all threads call.
__device__ __forceinline__ int stage_accepted(Box8* sb, int* nb_lds, const float* __restrict__ bank_boxes, const int* __restrict__ cand,
                                              const int* __restrict__ accepted, int b, int K, int bcol, int Kc) {
  const int tid = threadIdx.x;
  if (tid < KC_MAX) {
    int c = tid < Kc ? cand[(size_t)b * Kc + tid] : -1;
    const bool a = c >= 0 && c < K && accepted[(size_t)b * Kc + (tid < Kc ? tid : 0)] != 0;
    const unsigned long long bal = __ballot(a);
    if (a) sb[__popcll(bal & ((1ull << tid) - 1ull))] = stage_box(bank_boxes + (size_t)c * bcol, true);
    if (tid == 0) *nb_lds = __popcll(bal);
  }
  __syncthreads();
  return *nb_lds;
}
__device__ __forceinline__ bool paste_keep(const float* __restrict__ fp, int i, int n, int C, const Box8* sb, int nb) {
  if (i >= n) return false;
  const float px = fp[(size_t)i * C], py = fp[(size_t)i * C + 1], pz = fp[(size_t)i * C + 2];
  for (int j = 0; j < nb; ++j)
    if (inside_box(sb[j], px, py, pz)) return false;
  return true;
}
// grid (tiles, B); tcount [B][tiles]
__global__ __launch_bounds__(PC_TILE) void paste_count(const float* __restrict__ pts, const int* __restrict__ n_in,
                                                       const float* __restrict__ bank_boxes, const int* __restrict__ cand,
                                                       const int* __restrict__ accepted, int* __restrict__ tcount, int N, int C, int K,
                                                       int bcol, int Kc) {
  __shared__ Box8 sb[KC_MAX];
  __shared__ int nb_lds;
  const int b = blockIdx.y;
  const int nb = stage_accepted(sb, &nb_lds, bank_boxes, cand, accepted, b, K, bcol, Kc);
  tile_count(paste_keep(pts + (size_t)b * N * C, blockIdx.x * PC_TILE + threadIdx.x, frame_rows(n_in, b, N), C, sb, nb),
             tcount + (size_t)b * gridDim.x + blockIdx.x);
}
// out [B][capacity][C]: survivor number r goes to row r when r < capacity; kept [B] = all survivors
__global__ __launch_bounds__(PC_TILE) void paste_compact(const float* __restrict__ pts, const int* __restrict__ n_in,
                                                         const float* __restrict__ bank_boxes, const int* __restrict__ cand,
                                                         const int* __restrict__ accepted, const int* __restrict__ tcount,
                                                         float* __restrict__ out, int* __restrict__ kept, int N, int C, int K, int bcol,
                                                         int Kc, int capacity) {
  __shared__ Box8 sb[KC_MAX];
  __shared__ int nb_lds;
  const int t = blockIdx.x, b = blockIdx.y, i = t * PC_TILE + threadIdx.x;
  const int nb = stage_accepted(sb, &nb_lds, bank_boxes, cand, accepted, b, K, bcol, Kc);
  const float* const fp = pts + (size_t)b * N * C;
  const bool keep = paste_keep(fp, i, frame_rows(n_in, b, N), C, sb, nb);
  const int start = tiles_before(tcount + (size_t)b * gridDim.x, t);
  const TileRank r = tile_rank(keep, start);
  if (keep && r.row < capacity) {                                    // i < N and r.row < capacity: inside both frames' rows
    float* const dst = out + ((size_t)b * capacity + r.row) * C;
    for (int c = 0; c < C; ++c) dst[c] = fp[(size_t)i * C + c];
  }
  if (threadIdx.x == 0 && t == (int)gridDim.x - 1) kept[b] = start + r.total;
}
// grid (blocks, B): rows [kept, kept + total) of out = the accepted objects' points, rows behind them zeros; count [B]
__global__ __launch_bounds__(256) void paste_append(const float* __restrict__ bank_points, const int* __restrict__ obj_ptr,
                                                    const float* __restrict__ bank_boxes, const int* __restrict__ cand,
                                                    const int* __restrict__ accepted, const int* __restrict__ pre,
                                                    const int* __restrict__ kept, float* __restrict__ out, int* __restrict__ count, int C,
                                                    int K, int bcol, int Kc, int capacity) {
  __shared__ int spre[KC_MAX + 1], sobj[KC_MAX];
  const int tid = threadIdx.x, b = blockIdx.y;
  if (tid <= Kc) spre[tid] = pre[(size_t)b * (Kc + 1) + tid];
  if (tid < Kc) {
    const int c = cand[(size_t)b * Kc + tid];
    sobj[tid] = (c >= 0 && c < K && accepted[(size_t)b * Kc + tid] != 0) ? c : -1;
  }
  __syncthreads();
  const int nk = kept[b], total = spre[Kc];
  const long long rows = (long long)nk + total;
  if (blockIdx.x == 0 && tid == 0) count[b] = (int)(rows < capacity ? rows : capacity);
  const long long n = (long long)capacity * C;
  float* const o = out + (size_t)b * n;
  for (long long e = (long long)nk * C + blockIdx.x * 256ll + tid; e < n; e += (long long)gridDim.x * 256) {
    const int r = (int)(e / C), ch = (int)(e - (long long)r * C);
    float v = 0.f;
    if (r < rows) {
      const int a = r - nk;                                          // 0 <= a < total
      int k = 0;
      while (k + 1 < Kc && (sobj[k] < 0 || a >= spre[k + 1])) ++k;   // the accepted candidate whose [pre[k], pre[k + 1]) holds a
      const int c = sobj[k];                                         // >= 0 when prefix and accepted come from paste_accept
      if (c >= 0) {
        v = bank_points[((size_t)obj_ptr[c] + (a - spre[k])) * C + ch];
        if (ch < 3) v = v + bank_boxes[(size_t)c * bcol + ch];
      }
    }
    o[e] = v;
  }
}

}  // namespace

extern "C" int bevf_points_in_boxes_f32(const float* points, const int32_t* n_in, const float* boxes, const int32_t* box_mask,
                                        int32_t* idx, int B, int N, int C, int M, int ncol, void* stream) {
  BEVF_REQUIRE((points && idx) || N == 0, "points_in_boxes: null pointer");
  BEVF_REQUIRE(boxes || M == 0, "points_in_boxes: null pointer");
  BEVF_REQUIRE(B > 0 && B < 65536 && N >= 0 && C >= 3 && M >= 0 && (ncol == 7 || ncol == 9),
               "points_in_boxes: need B > 0, N >= 0, C >= 3, M >= 0, 7 or 9 columns");
  if (N == 0) return BEVF_OK;
  hipLaunchKernelGGL(points_in_boxes, dim3((N + PIB_T - 1) / PIB_T, B), dim3(PIB_T), 0, static_cast<hipStream_t>(stream), points, n_in,
                     boxes, box_mask, idx, N, C, M, ncol);
  return bevf_check_launch("bevf_points_in_boxes_f32");
}

extern "C" int bevf_paste_accept_f32(const float* gt_boxes, const int64_t* gt_labels, const float* gt_velocities, const float* bank_boxes,
                                     const int64_t* bank_labels, const int32_t* obj_ptr, const int32_t* cand, int32_t* accepted,
                                     int32_t* prefix, float* out_boxes, int64_t* out_labels, float* out_velocities, int B, int M, int ncol,
                                     int K, int bank_ncol, int Kc, void* stream) {
  BEVF_REQUIRE((gt_boxes && gt_labels) || M == 0, "paste_accept: null pointer");
  BEVF_REQUIRE(bank_boxes && bank_labels && obj_ptr && cand && accepted && prefix && out_boxes && out_labels, "paste_accept: null pointer");
  BEVF_REQUIRE((gt_velocities != nullptr) == (out_velocities != nullptr) || M == 0,
               "paste_accept: velocities go in and come out together");
  BEVF_REQUIRE(B > 0 && B < 65536 && M >= 0 && M < (1 << 20) && K > 0 && Kc > 0 && Kc <= KC_MAX && (ncol == 7 || ncol == 9) &&
                   (bank_ncol == 7 || bank_ncol == 9),
               "paste_accept: need B > 0, M >= 0, K > 0, 0 < Kc <= 64, 7 or 9 columns");
  hipLaunchKernelGGL(paste_accept, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), gt_boxes,
                     reinterpret_cast<const long long*>(gt_labels), gt_velocities, bank_boxes, reinterpret_cast<const long long*>(bank_labels),
                     obj_ptr, cand, accepted, prefix, out_boxes, reinterpret_cast<long long*>(out_labels), out_velocities, M, ncol, K,
                     bank_ncol, Kc);
  return bevf_check_launch("bevf_paste_accept_f32");
}

extern "C" size_t bevf_paste_points_work_ints(int B, int N) {
  if (B <= 0 || N < 0) return 0;
  return (size_t)B * ((size_t)point_tiles(N) + 1);
}

extern "C" int bevf_paste_points_f32(const float* points, const int32_t* n_in, const float* bank_points, const int32_t* obj_ptr,
                                     const float* bank_boxes, const int32_t* cand, const int32_t* accepted, const int32_t* prefix,
                                     float* out, int32_t* count, int32_t* work, int B, int N, int C, int K, int bank_ncol, int Kc,
                                     int capacity, void* stream) {
  BEVF_REQUIRE((points || N == 0) && bank_points && obj_ptr && bank_boxes && cand && accepted && prefix && out && count && work,
               "paste_points: null pointer");
  BEVF_REQUIRE(B > 0 && B < 65536 && N >= 0 && C >= 3 && K > 0 && Kc > 0 && Kc <= KC_MAX && capacity > 0 && (bank_ncol == 7 || bank_ncol == 9),
               "paste_points: need B > 0, N >= 0, C >= 3, K > 0, 0 < Kc <= 64, capacity > 0, 7 or 9 bank columns");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles = point_tiles(N);
  int* const tcount = work;
  int* const kept = work + (size_t)B * tiles;
  if (tiles > 0) {
    hipLaunchKernelGGL(paste_count, dim3(tiles, B), dim3(PC_TILE), 0, st, points, n_in, bank_boxes, cand, accepted, tcount, N, C, K, bank_ncol, Kc);
    hipLaunchKernelGGL(paste_compact, dim3(tiles, B), dim3(PC_TILE), 0, st, points, n_in, bank_boxes, cand, accepted, tcount, out, kept, N, C, K,
                       bank_ncol, Kc, capacity);
  } else {
    (void)hipMemsetAsync(kept, 0, sizeof(int32_t) * (size_t)B, st);
  }
  const long long n = (long long)capacity * C;
  hipLaunchKernelGGL(paste_append, dim3((unsigned)((n + 255) / 256 < 512 ? (n + 255) / 256 : 512), B), dim3(256), 0, st, bank_points, obj_ptr,
                     bank_boxes, cand, accepted, prefix, kept, out, count, C, K, bank_ncol, Kc, capacity);
  return bevf_check_launch("bevf_paste_points_f32");
}
