// Greedy centre-distance multi-object tracker on the decode path: CenterPoint's published tracker, one wave per stream
// (a stream = one batch row, the B rows of a batch are B independent sequences), the state overwritten in place.
//
// State of a stream, capacity T: track_box [T][7], track_vel [T][2], track_score [T], track_label [T] i64, track_id [T] i64, track_age [T]
// (frames since the last match), track_hits [T], track_count, next_id.  Rows past track_count are zeros with id -1; the state is in the
// sensor frame of the step that wrote it.  One step, with M = ego_motion[b] (fp64, current frame -> previous frame, rigid: M = [R t],
// only the top 3 x 4 is read), n = count[b] clamped to [0, N] and tc = track_count[b] clamped to [0, T]:
//
// 1. Association, detections i = 0 .. n-1 in order.  A detection is *valid* when x, y, z, vx, vy and its score are all finite.
//      px = (double)x - (double)vx * (double)dt,  py alike                       (back to the previous time)
//      qx = (float)(((m00 px + m01 py) + m02 (double)z) + m03),  qy with row 1   (into the previous frame; fp64, rounded once)
//    Candidates are the tracks s < tc not taken yet, with track_label == label_i when class_aware, whose fp32 squared distance
//      d2 = (qx - tx) * (qx - tx) + (qy - ty) * (qy - ty)     to the stored centre satisfies     d2 <= max_dist[l] * max_dist[l],
//    l = label_i inside [0, C), else 0.  The candidate with the smallest d2 is matched and taken, a tie goes to the lower slot.  Every
//    comparison is written so that NaN is "no": an invalid detection, a NaN q or a NaN / negative max_dist matches nothing, and
//    max_dist^2 saturates at FLT_MAX, so a d2 that overflowed to +inf matches nothing either.
// 2. A matched track takes the detection's box, velocity and score; label and id stay, age = 0, hits += 1.
// 3. An unmatched track: age += 1, dropped when age > max_age, else coasted into the current frame (p, v its centre and velocity):
//      u = p - t (fp64);  v'x = r00 vx + r10 vy,  v'y = r01 vx + r11 vy                         (v' = R^T v, planar)
//      x' = (float)(((r00 ux + r10 uy) + r20 uz) + v'x dt),  y' = (float)(((r01 ux + r11 uy) + r21 uz) + v'y dt),
//      z' = (float)((r02 ux + r12 uy) + r22 uz),  velocity = ((float)v'x, (float)v'y),  yaw' = (float)((double)yaw - atan2(m10, m00));
//    size, score, label, id and hits unchanged.  The yaw is not wrapped.
// 4. Birth: a valid unmatched detection with score >= birth_score starts a track, in detection order: id = next_id++, hits = 1, age = 0.
//    With the state full the detection gets no track, consumes no id and is counted in overflow[b].
// 5. The new state = the surviving old tracks in their previous slot order, then the births in detection order.
//
// Per detection: det_track_id (-1 = none: rows >= n, unmatched and not born, overflow), det_hits (0 = none), det_slot (slot in the new
// state, -1 = none).  All mul / add chains above run with contraction off for the file, so tests/track_ref.py reproduces every column
// but the coasted yaw (atan2) bit for bit.
//
// Shape: lane l of the wave holds tracks l, 64 + l, ... (centre, label, taken / live bits) in registers; detections
// are projected 512 at a time in parallel into LDS and then walked serially, the next detection's LDS reads issued before this one's
// work: each lane forms the key (d2 bits << 32 | slot) of its best candidate, a ballot skips the reduction when nobody has one, a single candidate is read with v_readlane, otherwise a 6-step xor
// butterfly takes the 64-bit minimum (non-negative floats order like their bits; the slot in the low word breaks ties downwards).
// Compaction is ballot / popcount prefixes in slot and detection order.  No atomics, no allocation, nothing read back: one launch.
#include <float.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TRK_CHUNK = 512;                                       // detections projected per LDS stage
constexpr int TRK_MAX_N = 4096, TRK_MAX_T = 1024;

struct TrackArgs {
  const float* boxes; const float* vels; const float* scores; const long long* labels; const int32_t* count;
  const double* ego; const float* dt; const float* max_dist;
  float* t_box; float* t_vel; float* t_score; long long* t_label; long long* t_id; int32_t* t_age; int32_t* t_hits;
  int32_t* t_count; long long* next_id;
  long long* d_id; int32_t* d_hits; int32_t* d_slot; int32_t* overflow;
  int N, T, C, max_age, class_aware;
  float birth_score;
};

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < INFINITY; }                     // false for NaN

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}

// TS = track slots per lane: slot = 64 * k + lane, k < TS
template <int TS>
__global__ __launch_bounds__(64) void track_step(const TrackArgs a) {
  __shared__ f32x4 s_q[TRK_CHUNK];                                                                   // qx, qy, max_dist^2 (< 0: matches nothing), -
  __shared__ long long s_lab[TRK_CHUNK];
  __shared__ int s_match[TRK_MAX_N];                                                                 // old slot, -1 unmatched, -2 invalid
  __shared__ int s_mdet[TRK_MAX_T];                                                                  // a taken slot's detection
  const int b = blockIdx.x, lane = threadIdx.x, N = a.N, T = a.T;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int n = a.count[b];
  n = n < 0 ? 0 : (n > N ? N : n);
  int tc = a.t_count[b];
  tc = tc < 0 ? 0 : (tc > T ? T : tc);
  const double dt = (double)a.dt[b];
  const size_t dn = (size_t)b * N, tn = (size_t)b * T;                                               // the stream's first detection / track row

  // ---- the lane's tracks ----
  float tx[TS], ty[TS];
  long long tl[TS];
  unsigned avail = 0u, taken = 0u;                                                                   // bit k: slot 64 k + lane
#pragma unroll
  for (int k = 0; k < TS; ++k) {
    const int s = 64 * k + lane;
    tx[k] = 0.f, ty[k] = 0.f, tl[k] = 0;
    if (s < tc) {
      tx[k] = a.t_box[(tn + s) * 7], ty[k] = a.t_box[(tn + s) * 7 + 1];
      tl[k] = a.class_aware ? a.t_label[tn + s] : 0;
      avail |= 1u << k;
    }
  }

  // ---- 1. association ----
  for (int c0 = 0; c0 < n; c0 += TRK_CHUNK) {
    const int cn = n - c0 < TRK_CHUNK ? n - c0 : TRK_CHUNK;
    __syncthreads();
    double m[8];                                                                                     // rows 0 and 1 of M; loaded per phase, not held
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = a.ego[16 * (size_t)b + i];
    for (int j = lane; j < cn; j += 64) {
      const int i = c0 + j;
      const float x = a.boxes[(dn + i) * 7], y = a.boxes[(dn + i) * 7 + 1], z = a.boxes[(dn + i) * 7 + 2];
      const float vx = a.vels[(dn + i) * 2], vy = a.vels[(dn + i) * 2 + 1];
      const long long lab = a.labels[dn + i];
      const bool valid = finitef(x) && finitef(y) && finitef(z) && finitef(vx) && finitef(vy) && finitef(a.scores[dn + i]);
      const double px = (double)x - (double)vx * dt, py = (double)y - (double)vy * dt;
      const float qx = (float)(((m[0] * px + m[1] * py) + m[2] * (double)z) + m[3]);
      const float qy = (float)(((m[4] * px + m[5] * py) + m[6] * (double)z) + m[7]);
      const float md = a.max_dist[(lab >= 0 && lab < a.C) ? (int)lab : 0];
      f32x4 rec;
      rec[0] = qx, rec[1] = qy, rec[2] = (valid && md >= 0.f) ? fminf(md * md, FLT_MAX) : -1.f, rec[3] = 0.f;   // NaN md: -1
      s_q[j] = rec;
      s_lab[j] = a.class_aware ? lab : 0;
      s_match[i] = valid ? -1 : -2;
    }
    __syncthreads();
    f32x4 nq = s_q[0];                                                                               // LDS broadcasts: wave-uniform
    long long nlab = s_lab[0];
    for (int j = 0; j < cn; ++j) {
      const f32x4 q = nq;
      const long long lab = nlab;
      const int jn = j + 1 < cn ? j + 1 : j;                                                         // the next detection's reads fly under this one's walk
      nq = s_q[jn], nlab = s_lab[jn];
      if (!(q[2] >= 0.f)) continue;
      float bestd = INFINITY;                                                                        // max_dist^2 <= FLT_MAX: a candidate's d2 is finite
      int bests = 0;
#pragma unroll
      for (int k = 0; k < TS; ++k) {
        const float dx = q[0] - tx[k], dy = q[1] - ty[k];
        const float d2 = dx * dx + dy * dy;
        const bool ok = ((avail >> k) & 1u) && tl[k] == lab && d2 <= q[2];                           // NaN d2: no
        if (ok && d2 < bestd) bestd = d2, bests = 64 * k + lane;                                     // ascending k: the lower slot stays on a tie
      }
      const unsigned long long key = bestd < INFINITY ? ((unsigned long long)__float_as_uint(bestd) << 32) | (unsigned)bests : ~0ull;
      const unsigned long long has = __ballot(bestd < INFINITY);
      if (has == 0ull) continue;
      unsigned long long best;
      if ((has & (has - 1ull)) == 0ull) {                                                            // one lane has a candidate: read it
        const int src = __builtin_ctzll(has);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, src);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), src);
        best = ((unsigned long long)hi << 32) | lo;
      } else {
        best = wave_min_u64(key);
      }
      const int slot = (int)(unsigned)best;
      if ((slot & 63) == lane) {
#pragma unroll
        for (int k = 0; k < TS; ++k)
          if (k == (slot >> 6)) avail &= ~(1u << k), taken |= 1u << k;
      }
      if (lane == 0) s_match[c0 + j] = slot, s_mdet[slot] = c0 + j;
    }
  }
  __syncthreads();

  // ---- 2. / 3. / 5. old tracks: update or coast, compact in slot order (in place: a chunk of 64 slots is read, then written at or below) ----
  double m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = a.ego[16 * (size_t)b + i];
  const double yaw_step = atan2(m[4], m[0]);
  int base = 0;
#pragma unroll 1
  for (int k = 0; 64 * k < tc; ++k) {                                                                // wave-uniform bound, k < TS
    const int s = 64 * k + lane;
    const bool live = s < tc, hit = (taken >> k) & 1u;
    float r[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                                // box 7, velocity 2, score
    long long lab = 0, id = -1;
    int age = 0, hits = 0;
    if (live) {
      lab = a.t_label[tn + s], id = a.t_id[tn + s], age = a.t_age[tn + s], hits = a.t_hits[tn + s];
      if (hit) {
        const int i = s_mdet[s];
#pragma unroll
        for (int q = 0; q < 7; ++q) r[q] = a.boxes[(dn + i) * 7 + q];
        r[7] = a.vels[(dn + i) * 2], r[8] = a.vels[(dn + i) * 2 + 1], r[9] = a.scores[dn + i];
        age = 0, hits += 1;
      } else {
#pragma unroll
        for (int q = 0; q < 7; ++q) r[q] = a.t_box[(tn + s) * 7 + q];
        r[7] = a.t_vel[(tn + s) * 2], r[8] = a.t_vel[(tn + s) * 2 + 1], r[9] = a.t_score[tn + s];
        age += 1;
        const double ux = (double)r[0] - m[3], uy = (double)r[1] - m[7], uz = (double)r[2] - m[11];
        const double wx = m[0] * (double)r[7] + m[4] * (double)r[8], wy = m[1] * (double)r[7] + m[5] * (double)r[8];
        r[0] = (float)(((m[0] * ux + m[4] * uy) + m[8] * uz) + wx * dt);
        r[1] = (float)(((m[1] * ux + m[5] * uy) + m[9] * uz) + wy * dt);
        r[2] = (float)((m[2] * ux + m[6] * uy) + m[10] * uz);
        r[6] = (float)((double)r[6] - yaw_step);
        r[7] = (float)wx, r[8] = (float)wy;
      }
    }
    const bool keep = live && (hit || age <= a.max_age);
    const unsigned long long bal = __ballot(keep);
    const int pos = base + __popcll(bal & lt);
    base += __popcll(bal);
    __syncthreads();                                                                                 // every read of this chunk has landed
    if (keep) {
#pragma unroll
      for (int q = 0; q < 7; ++q) a.t_box[(tn + pos) * 7 + q] = r[q];
      a.t_vel[(tn + pos) * 2] = r[7], a.t_vel[(tn + pos) * 2 + 1] = r[8], a.t_score[tn + pos] = r[9];
      a.t_label[tn + pos] = lab, a.t_id[tn + pos] = id, a.t_age[tn + pos] = age, a.t_hits[tn + pos] = hits;
      if (hit) {
        const int i = s_mdet[s];
        a.d_id[dn + i] = id, a.d_hits[dn + i] = hits, a.d_slot[dn + i] = pos;
      }
    }
  }
  const int survivors = base;                                                                        // <= tc <= T

  // ---- 4. births and the detections without a track ----
  const long long id0 = a.next_id[b];
  int nbirth = 0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    int mt = -2;
    float sc = 0.f;
    if (i < n) mt = s_match[i], sc = a.scores[dn + i];
    const bool cand = mt == -1 && sc >= a.birth_score;
    const unsigned long long bal = __ballot(cand);
    const int rank = nbirth + __popcll(bal & lt);
    nbirth += __popcll(bal);
    const int pos = survivors + rank;
    if (i < N && mt < 0) {
      const bool born = cand && pos < T;
      if (born) {
#pragma unroll
        for (int q = 0; q < 7; ++q) a.t_box[(tn + pos) * 7 + q] = a.boxes[(dn + i) * 7 + q];
        a.t_vel[(tn + pos) * 2] = a.vels[(dn + i) * 2], a.t_vel[(tn + pos) * 2 + 1] = a.vels[(dn + i) * 2 + 1], a.t_score[tn + pos] = sc;
        a.t_label[tn + pos] = a.labels[dn + i], a.t_id[tn + pos] = id0 + rank, a.t_age[tn + pos] = 0, a.t_hits[tn + pos] = 1;
      }
      a.d_id[dn + i] = born ? id0 + rank : -1, a.d_hits[dn + i] = born ? 1 : 0, a.d_slot[dn + i] = born ? pos : -1;
    }
  }
  const int total = survivors + nbirth < T ? survivors + nbirth : T;
  for (int s = total + lane; s < T; s += 64) {                                                       // padding, so two runs are bit-equal
#pragma unroll
    for (int q = 0; q < 7; ++q) a.t_box[(tn + s) * 7 + q] = 0.f;
    a.t_vel[(tn + s) * 2] = 0.f, a.t_vel[(tn + s) * 2 + 1] = 0.f, a.t_score[tn + s] = 0.f;
    a.t_label[tn + s] = 0, a.t_id[tn + s] = -1, a.t_age[tn + s] = 0, a.t_hits[tn + s] = 0;
  }
  if (lane == 0) {
    a.t_count[b] = total;
    a.next_id[b] = id0 + (total - survivors);
    a.overflow[b] = survivors + nbirth - total;
  }
}

}  // namespace

extern "C" int bevf_track_step_f32(const float* boxes, const float* velocities, const float* scores, const int64_t* labels,
                                   const int32_t* count, const double* ego_motion, const float* dt, const float* max_dist,
                                   float* track_box, float* track_vel, float* track_score, int64_t* track_label, int64_t* track_id,
                                   int32_t* track_age, int32_t* track_hits, int32_t* track_count, int64_t* next_id,
                                   int64_t* det_track_id, int32_t* det_hits, int32_t* det_slot, int32_t* overflow, int B, int N, int T,
                                   int C, int max_age, float birth_score, int class_aware, void* stream) {
  BEVF_REQUIRE(B > 0 && N >= 0 && T > 0 && C > 0, "track_step: need B > 0, N >= 0, T > 0, C > 0");
  BEVF_REQUIRE(N <= TRK_MAX_N, "track_step: N=%d exceeds 4096 detections per stream (the decode's own limit)", N);
  BEVF_REQUIRE(T <= TRK_MAX_T, "track_step: T=%d exceeds 1024 tracks per stream (16 slots per lane)", T);
  BEVF_REQUIRE(max_age >= 0, "track_step: max_age must be >= 0");
  BEVF_REQUIRE(N == 0 || (boxes && velocities && scores && labels && det_track_id && det_hits && det_slot),
               "track_step: null detection pointer");
  BEVF_REQUIRE(count && ego_motion && dt && max_dist && overflow, "track_step: null pointer");
  BEVF_REQUIRE(track_box && track_vel && track_score && track_label && track_id && track_age && track_hits && track_count && next_id,
               "track_step: null state pointer");
  TrackArgs a;
  a.boxes = boxes; a.vels = velocities; a.scores = scores; a.labels = (const long long*)labels; a.count = count;
  a.ego = ego_motion; a.dt = dt; a.max_dist = max_dist;
  a.t_box = track_box; a.t_vel = track_vel; a.t_score = track_score; a.t_label = (long long*)track_label; a.t_id = (long long*)track_id;
  a.t_age = track_age; a.t_hits = track_hits; a.t_count = track_count; a.next_id = (long long*)next_id;
  a.d_id = (long long*)det_track_id; a.d_hits = det_hits; a.d_slot = det_slot; a.overflow = overflow;
  a.N = N; a.T = T; a.C = C; a.max_age = max_age; a.class_aware = class_aware ? 1 : 0; a.birth_score = birth_score;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (T <= 256) hipLaunchKernelGGL(track_step<4>, dim3(B), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(track_step<16>, dim3(B), dim3(64), 0, st, a);
  return bevf_check_launch("bevf_track_step_f32");
}
