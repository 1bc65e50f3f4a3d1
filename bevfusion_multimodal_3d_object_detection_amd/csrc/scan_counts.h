// Per-frame exclusive scan of row lengths, shared by the device table builds (camera_calib.hip, camera_frustum.hip).
#pragma once
#include "common.h"

namespace {

// cnt [B][n] -> rp [B][n + 1], the exclusive prefix sums of each frame; one 1024-thread block per frame.
__global__ __launch_bounds__(1024) void scan_counts(const int32_t* __restrict__ cnt, int n, int32_t* __restrict__ rp) {
  __shared__ int part[1024];
  const int t = (int)threadIdx.x;
  const int32_t* c = cnt + (long long)blockIdx.x * n;
  int32_t* r = rp + (long long)blockIdx.x * (n + 1);
  const int chunk = (n + 1023) / 1024;
  const long long lo64 = (long long)t * chunk;
  const int lo = lo64 < n ? (int)lo64 : n, hi = lo + chunk < n ? lo + chunk : n;
  int s = 0;
  for (int k = lo; k < hi; ++k) s += c[k];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int k = lo; k < hi; ++k) {
    r[k] = run;
    run += c[k];
  }
  if (t == 1023) r[n] = part[t];
}

}  // namespace
