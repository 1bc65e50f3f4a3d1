// The stable compaction of a point cloud (keep a subset of rows, preserve point order, pad to a fixed row count), the stages shared by
// preprocess.hip (lfp_*), augment.hip (paf_*), gt_paste.hip (paste_*) and sweeps.hip (msw_*); DESIGN.md 3.2k2 says who owns what.
// A file keeps its keep predicate, its stores and its entry point; a tile of PC_TILE rows is one workgroup of PC_TILE threads.
//
// Integer and comparison code only: nothing in here rounds, so it does not matter that some of the including files switch
// floating-point contraction off with a pragma placed in front of their own code and others do not.
#pragma once
#include "common.h"

namespace {

constexpr int PC_TILE = 1024;                                        // rows per tile = threads per workgroup (16 waves)

struct Range6 {
  float x0, y0, z0, x1, y1, z1;
};
inline Range6 range6(const float* pc_range6) {
  return {pc_range6[0], pc_range6[1], pc_range6[2], pc_range6[3], pc_range6[4], pc_range6[5]};
}
// strict inequalities; NaN fails every test, like numpy
__device__ __forceinline__ bool in_range(const Range6& r, float x, float y, float z) {
  return x > r.x0 && x < r.x1 && y > r.y0 && y < r.y1 && z > r.z0 && z < r.z1;
}

// rows of frame (or sweep) b that hold points: counts[b], or N without counts, never past the frame's N rows
__device__ __forceinline__ int frame_rows(const int* __restrict__ counts, size_t b, int N) {
  const int n = counts ? counts[b] : N;
  return n < 0 ? 0 : (n > N ? N : n);
}
inline int point_tiles(int N) { return (N + PC_TILE - 1) / PC_TILE; }

// All threads of the workgroup call.  row: start + the kept rows of this tile in front of the thread (its output row when it keeps);
// total: the tile's survivors.
struct TileRank {
  int row, total;
};
__device__ __forceinline__ TileRank tile_rank(bool keep, int start) {
  __shared__ int wsum[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  int woff = 0, tot = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  for (int w = 0; w < 16; ++w) tot += wsum[w];
  return {start + woff + before, tot};
}
// the count kernels: the tile's survivors into the caller's slot
__device__ __forceinline__ void tile_count(bool keep, int* __restrict__ slot) {
  const int tot = tile_rank(keep, 0).total;
  if (threadIdx.x == 0) *slot = tot;
}
// All threads call: the survivors in the t tiles in front of this one, tcount[0 .. t).  A strided trip per PC_TILE tiles.
__device__ __forceinline__ int tiles_before(const int* __restrict__ tcount, int t) {
  __shared__ int wpre[16];
  int part = 0;
  for (int j = threadIdx.x; j < t; j += PC_TILE) part += tcount[j];
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if ((threadIdx.x & 63) == 0) wpre[threadIdx.x >> 6] = part;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < 16; ++w) off += wpre[w];
  return off;
}

// grid (blocks, B): out [B][max_points][C] = the first max_points rows of work [B][N][C] below count[b], then zeros.  CHOICE (B = 1):
// with a choice [max_points] and at least max_points survivors, row r = survivor choice[r] (zeros where that is none).
template <bool CHOICE>
__global__ __launch_bounds__(256) void compact_output(const float* __restrict__ work, float* __restrict__ out, const int* __restrict__ count,
                                                      const long long* __restrict__ choice, int N, int C, int max_points) {
  const int b = blockIdx.y;
  const int total = count[b];
  const bool gather = CHOICE && choice != nullptr && total >= max_points;
  const long long n = (long long)max_points * C;
  const float* const w = work + (size_t)b * N * C;
  float* const o = out + (size_t)b * n;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int r = (int)(e / C);
    float v = 0.f;
    if (gather) {
      const long long s = choice[r];
      if (s >= 0 && s < total) v = w[(size_t)s * C + (int)(e - (long long)r * C)];
    } else if (r < total) {                                          // r < total <= N: inside the frame's work rows
      v = w[e];
    }
    o[e] = v;
  }
}

}  // namespace
