// Compaction step of the pruned PointNet max (engine.PointNetEngine): the rows that the bound pass of conv_split.hip
// flagged are copied, frame by frame, into a fixed-size candidate buffer on which the exact convolution then runs.
//   flag [B][N] (0 / 1)  ->  rp [B][N + 1] exclusive prefix (scan_counts.h)  ->  cand [B][cap][C]
// Slot s < count of a frame holds its s-th flagged row; the slots from there to the next multiple of 128 hold the frame's row 0, which
// is a legitimate contributor to the frame's max, and the rest is left alone: rows[b] = min(count, cap) tells the exact launch which
// tiles to skip (group_rows of bevf_conv2d_nhwc_f32_if).  A frame with more than `cap` flagged rows sets *overflow (the caller then runs the
// full launch, run_if of bevf_conv2d_nhwc_f32_if).
#include "scan_counts.h"

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

// one wave per work item of a frame: items [0, N) are the frame's rows, items [N, N + cap) the candidate slots that may need padding
__global__ __launch_bounds__(256) void prune_gather(const float* __restrict__ x, const int32_t* __restrict__ flag,
                                                    const int32_t* __restrict__ rp, float* __restrict__ cand, int32_t* __restrict__ rows,
                                                    int32_t* __restrict__ overflow, int B, int N, int C4, int cap) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int per = N + cap;
  if (w >= (long long)B * per) return;
  const int b = (int)(w / per), i = (int)(w - (long long)b * per);
  const int count = rp[(long long)b * (N + 1) + N];
  int src, slot;
  if (i < N) {
    if (!flag[(long long)b * N + i]) return;
    src = i;
    slot = rp[(long long)b * (N + 1) + i];
    if (slot >= cap) return;
  } else {
    slot = i - N;
    if (slot == 0 && lane == 0) {
      rows[b] = count < cap ? count : cap;
      if (count > cap) *overflow = 1;
    }
    if (slot < count || slot >= ((count + 127) & ~127)) return;           // (cap % 128 == 0: the padding ends inside the frame's slots)
    src = 0;
  }
  const f32x4v* s = reinterpret_cast<const f32x4v*>(x) + ((long long)b * N + src) * C4;
  f32x4v* d = reinterpret_cast<f32x4v*>(cand) + ((long long)b * cap + slot) * C4;
  for (int c = lane; c < C4; c += 64) d[c] = s[c];
}

}  // namespace

extern "C" int bevf_prune_compact_f32(const float* x, const int32_t* flag, int32_t* rp, float* cand, int32_t* rows, int32_t* overflow,
                                      int B, int N, int C, int cap, void* stream) {
  BEVF_REQUIRE(x && flag && rp && cand && rows && overflow, "prune_compact: null argument");
  BEVF_REQUIRE(B > 0 && N > 0 && cap > 0 && cap % 128 == 0 && C > 0 && C % 4 == 0,
               "prune_compact: B, N must be positive, cap a positive multiple of 128 and C a positive multiple of 4");
  BEVF_REQUIRE(bevf_aligned16(x) && bevf_aligned16(cand), "prune_compact: x / cand must be 16-byte aligned");
  BEVF_REQUIRE((long long)B * ((long long)N + cap) < (1ll << 31), "prune_compact: B * (N + cap) overflows int32");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(scan_counts, dim3(B), dim3(1024), 0, st, flag, N, rp);
  if (const int rc = bevf_check_launch("bevf_prune_compact_f32")) return rc;
  const long long waves = (long long)B * ((long long)N + cap);
  hipLaunchKernelGGL(prune_gather, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, x, flag, rp, cand, rows, overflow, B, N, C / 4, cap);
  return bevf_check_launch("bevf_prune_compact_f32");
}
