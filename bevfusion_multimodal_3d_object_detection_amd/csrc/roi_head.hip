// CenterPoint second stage around the RoI head's GEMMs (roi_head.py / roi_refine.py): the RoI targets, the loss
// with its gradient, and the refine step that turns the head's output into the final padded records.
//
// RoIs are the decode's padded records: boxes [B][K][7] = (x, y, z, w, l, h, yaw), l along the heading (box_geom.h::load_box), with
// count int32 [B] clamped to [0, K]; rows past the count are never read.  The head's output is pred [B * K][8]: the logit, then the
// residual t[7].  The box encoding (OpenPCDet's, in the RoI's frame), d = gt - roi, c = cos yaw, s = sin yaw of the RoI:
//   t = ((c dx + s dy) / diag, (-s dx + c dy) / diag, dz / h, log(w_g / w), log(l_g / l), log(h_g / h), dyaw),  diag = sqrt(l^2 + w^2),
//   dyaw = yaw_g - yaw wrapped into [-pi, pi) and folded into [-pi / 2, pi / 2] by -+ pi (opposite headings are the same box).
//   bevf_roi_targets_f32    one wave per RoI: the lanes take the frame's ground-truth boxes 64 at a time, the best IoU (lowest index
//                           among equals) wins by a butterfly; lane 0 encodes.  No atomics.
//   bevf_roi_loss_f32       one workgroup: thread partials in row order (fp64), butterfly, four wave sums in order.
//   bevf_roi_loss_bwd_f32   one thread per row; the two normalisers are integer counts, recounted by every workgroup.
//   bevf_roi_refine_f32     one workgroup per frame: final scores into LDS, each kept row's rank by counting, records written at
//                           their rank -- compacted, descending score, ties by ascending RoI index.
// All tiny; bound by launch latency.
#include "box_geom.h"

namespace {

constexpr int REFINE_MAX_K = 4096;   // scores of one frame staged in LDS; the tracker's own limit on its detections
constexpr float PI_F = 3.14159265358979323846f;

__device__ __forceinline__ int roi_count(const int32_t* __restrict__ count, int b, int K) {
  const int n = count[b];
  return n < 0 ? 0 : (n < K ? n : K);
}

// ---- targets ---------------------------------------------------------------------------------------------------------------------

struct TargetArgs {
  const float* rois; const int32_t* count; const long long* roi_labels; const float* gt; const int32_t* gt_labels;
  float* iou; int32_t* gt_index; float* cls_target; unsigned char* reg_mask; float* reg_target;
  int B, K, M, use_bev, match_labels;
  float reg_fg_thresh;
};

__device__ __forceinline__ float fold_heading(float d) {
  d = d - 2.f * PI_F * floorf((d + PI_F) / (2.f * PI_F));     // [-pi, pi)
  if (d > 0.5f * PI_F) d -= PI_F;
  else if (d < -0.5f * PI_F) d += PI_F;
  return d;
}

__global__ __launch_bounds__(256) void roi_targets_k(const TargetArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int row = (int)blockIdx.x * 4 + wave;
  if (row >= a.B * a.K) return;
  const int b = row / a.K, k = row - b * a.K;
  const bool valid = k < roi_count(a.count, b, a.K);
  float best = -1.f;
  int arg = -1;
  if (valid) {
    const RBox rb = load_box(a.rois + (size_t)row * 7);
    const long long lab = a.match_labels ? a.roi_labels[row] : 0;
    for (int m = lane; m < a.M; m += 64) {                     // ascending m per lane: a strict > keeps the lowest index
      const int gl = a.gt_labels[b * a.M + m];
      if (gl < 0 || (a.match_labels && (long long)gl != lab)) continue;
      const RBox gb = load_box(a.gt + ((size_t)b * a.M + m) * 7);
      const float v = a.use_bev ? iou_bev(rb, gb) : iou_3d(rb, gb);
      if (v > best) best = v, arg = m;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const float ov = __shfl_xor(best, s, 64);
      const int oa = __shfl_xor(arg, s, 64);
      if (oa >= 0 && (arg < 0 || ov > best || (ov == best && oa < arg))) best = ov, arg = oa;
    }
  }
  if (lane != 0) return;
  float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float iou = arg >= 0 ? best : 0.f;
  bool fg = false;
  if (arg >= 0) {
    const float* r = a.rois + (size_t)row * 7;
    const float* g = a.gt + ((size_t)b * a.M + arg) * 7;
    fg = iou >= a.reg_fg_thresh && r[3] > 0.f && r[4] > 0.f && r[5] > 0.f && g[3] > 0.f && g[4] > 0.f && g[5] > 0.f;
    if (fg) {
      float s, c;
      sincosf(r[6], &s, &c);
      const float dx = g[0] - r[0], dy = g[1] - r[1];
      const float diag = sqrtf(r[4] * r[4] + r[3] * r[3]);
      t[0] = (c * dx + s * dy) / diag;
      t[1] = (c * dy - s * dx) / diag;
      t[2] = (g[2] - r[2]) / r[5];
      t[3] = logf(g[3] / r[3]);
      t[4] = logf(g[4] / r[4]);
      t[5] = logf(g[5] / r[5]);
      t[6] = fold_heading(g[6] - r[6]);
    }
  }
  a.iou[row] = iou;
  a.gt_index[row] = arg;
  a.cls_target[row] = valid ? clampf(2.f * iou - 0.5f, 0.f, 1.f) : 0.f;
  a.reg_mask[row] = fg ? 1 : 0;
#pragma unroll
  for (int q = 0; q < 7; ++q) a.reg_target[(size_t)row * 7 + q] = t[q];
}

// ---- loss ------------------------------------------------------------------------------------------------------------------------

struct LossArgs {
  const float* pred; const int32_t* count; const float* cls_target; const unsigned char* reg_mask; const float* reg_target;
  int B, K;
  float w_cls, w_reg;
};

// the sum of v over the 256 threads in a fixed order; every thread gets it.  red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// (valid rows, foreground rows) of the batch: integers, exact in any order
__device__ __forceinline__ void batch_counts(const LossArgs& a, int* red, int& n_valid, int& n_fg) {
  int nv = 0, nf = 0;
  for (int r = threadIdx.x; r < a.B * a.K; r += 256) {
    const int b = r / a.K;
    if (r - b * a.K < roi_count(a.count, b, a.K)) {
      nv += 1;
      nf += a.reg_mask[r] ? 1 : 0;
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) nv += __shfl_xor(nv, s, 64), nf += __shfl_xor(nf, s, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nv, red[4 + (threadIdx.x >> 6)] = nf;
  __syncthreads();
  n_valid = red[0] + red[1] + red[2] + red[3];
  n_fg = red[4] + red[5] + red[6] + red[7];
}

// out[3] = total, cls_loss, reg_loss
__global__ __launch_bounds__(256) void roi_loss_k(const LossArgs a, float* __restrict__ out) {
  __shared__ double red[4];
  __shared__ int cnt[8];
  int n_valid, n_fg;
  batch_counts(a, cnt, n_valid, n_fg);
  double sc = 0.0, sr = 0.0;
  for (int r = threadIdx.x; r < a.B * a.K; r += 256) {
    const int b = r / a.K;
    if (r - b * a.K >= roi_count(a.count, b, a.K)) continue;
    const float* p = a.pred + (size_t)r * 8;
    const float x = p[0], t = a.cls_target[r];
    sc += (double)(fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))));
    if (a.reg_mask[r]) {
      float l1 = 0.f;
#pragma unroll
      for (int q = 0; q < 7; ++q) l1 += fabsf(p[1 + q] - a.reg_target[(size_t)r * 7 + q]);
      sr += (double)l1;
    }
  }
  sc = block_sum(sc, red);
  sr = block_sum(sr, red);
  if (threadIdx.x != 0) return;
  const float lc = (float)(sc / ((double)n_valid + 1e-4)), lr = (float)(sr / ((double)n_fg + 1e-4));
  out[0] = a.w_cls * lc + a.w_reg * lr;
  out[1] = lc;
  out[2] = lr;
}

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// dpred [B * K][8] = d total / d pred; exact zeros on invalid rows
__global__ __launch_bounds__(256) void roi_loss_bwd_k(const LossArgs a, float* __restrict__ dpred) {
  __shared__ int cnt[8];
  int n_valid, n_fg;
  batch_counts(a, cnt, n_valid, n_fg);
  const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (r >= a.B * a.K) return;
  const int b = r / a.K;
  float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (r - b * a.K < roi_count(a.count, b, a.K)) {
    const float* p = a.pred + (size_t)r * 8;
    const float x = p[0];
    const float e = expf(-fabsf(x)), inv = 1.f / (1.f + e);
    const float sig = x >= 0.f ? inv : e * inv;
    d[0] = a.w_cls * (sig - a.cls_target[r]) * (float)(1.0 / ((double)n_valid + 1e-4));
    if (a.reg_mask[r]) {
      const float wr = a.w_reg * (float)(1.0 / ((double)n_fg + 1e-4));
#pragma unroll
      for (int q = 0; q < 7; ++q) d[1 + q] = wr * sgn(p[1 + q] - a.reg_target[(size_t)r * 7 + q]);
    }
  }
  float* o = dpred + (size_t)r * 8;
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = d[q];
}

int loss_args(LossArgs* a, const char* what, const float* pred, const int32_t* count, const float* cls_target, const uint8_t* reg_mask,
              const float* reg_target, int B, int K, float w_cls, float w_reg) {
  BEVF_REQUIRE(pred && count && cls_target && reg_mask && reg_target, "%s: null pointer", what);
  BEVF_REQUIRE(B > 0 && K > 0 && (long long)B * K < (1ll << 27), "%s: bad shape (B=%d K=%d)", what, B, K);
  *a = LossArgs{pred, count, cls_target, reg_mask, reg_target, B, K, w_cls, w_reg};
  return BEVF_OK;
}

// ---- refine ----------------------------------------------------------------------------------------------------------------------

struct RefineArgs {
  const float* rois; const float* scores; const long long* labels; const float* vel; const int32_t* count; const float* pred;
  float* out_boxes; float* out_scores; long long* out_labels; float* out_vel; int32_t* out_count;
  int B, K;
  float score_thresh;
};

// final score of row (b, k): sqrt(s1 * sigmoid(logit)); -1 = dropped (past the count, non-finite, below the threshold)
__device__ __forceinline__ float refine_score(const RefineArgs& a, int b, int k, int n) {
  if (k >= n) return -1.f;
  const int row = b * a.K + k;
  const float x = a.pred[(size_t)row * 8];
  const float e = expf(-fabsf(x)), inv = 1.f / (1.f + e);
  const float s = sqrtf(a.scores[row] * (x >= 0.f ? inv : e * inv));
  return (s - s == 0.f && s >= a.score_thresh) ? s : -1.f;      // (s - s is NaN for NaN and infinities)
}

__global__ __launch_bounds__(256) void roi_refine_k(const RefineArgs a) {
  extern __shared__ float key[];       // [K]
  __shared__ int red[4];
  const int b = (int)blockIdx.x, K = a.K;
  const int n = roi_count(a.count, b, K);
  int kept = 0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float s = refine_score(a, b, k, n);
    key[k] = s;
    kept += s >= 0.f ? 1 : 0;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) kept += __shfl_xor(kept, s, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = kept;
  __syncthreads();                     // (also: key is complete)
  kept = red[0] + red[1] + red[2] + red[3];
  if (threadIdx.x == 0) a.out_count[b] = kept;
  for (int k = threadIdx.x; k < K; k += 256) {
    // the padding behind the kept rows: slot `k` when k >= kept
    if (k >= kept) {
      const size_t o = (size_t)b * K + k;
#pragma unroll
      for (int q = 0; q < 7; ++q) a.out_boxes[o * 7 + q] = 0.f;
      a.out_scores[o] = 0.f;
      a.out_labels[o] = 0;
      if (a.out_vel) a.out_vel[o * 2] = 0.f, a.out_vel[o * 2 + 1] = 0.f;
    }
    const float s = key[k];
    if (!(s >= 0.f)) continue;
    int rank = 0;                      // rows ahead of k: a higher score, or the same score at a lower index
#pragma unroll 8
    for (int j = 0; j < n; ++j) {
      const float sj = key[j];
      rank += (sj > s || (sj == s && j < k)) ? 1 : 0;
    }
    const size_t row = (size_t)b * K + k, o = (size_t)b * K + rank;
    const float* r = a.rois + row * 7;
    const float* t = a.pred + row * 8 + 1;
    float sn, cs;
    sincosf(r[6], &sn, &cs);
    const float diag = sqrtf(r[4] * r[4] + r[3] * r[3]);
    const float lx = t[0] * diag, ly = t[1] * diag;
    float* ob = a.out_boxes + o * 7;
    ob[0] = r[0] + (cs * lx - sn * ly);
    ob[1] = r[1] + (sn * lx + cs * ly);
    ob[2] = r[2] + t[2] * r[5];
    ob[3] = r[3] * expf(t[3]);
    ob[4] = r[4] * expf(t[4]);
    ob[5] = r[5] * expf(t[5]);
    ob[6] = r[6] + t[6];
    a.out_scores[o] = s;
    a.out_labels[o] = a.labels[row];
    if (a.out_vel) a.out_vel[o * 2] = a.vel[row * 2], a.out_vel[o * 2 + 1] = a.vel[row * 2 + 1];
  }
}

}  // namespace

extern "C" int bevf_roi_targets_f32(const float* rois, const int32_t* count, const int64_t* roi_labels, const float* gt,
                                    const int32_t* gt_labels, float* iou, int32_t* gt_index, float* cls_target, uint8_t* reg_mask,
                                    float* reg_target, int B, int K, int M, int use_bev, int match_labels, float reg_fg_thresh,
                                    void* stream) {
  BEVF_REQUIRE(rois && count && iou && gt_index && cls_target && reg_mask && reg_target, "roi_targets: null pointer");
  BEVF_REQUIRE(B > 0 && K > 0 && M >= 0 && (long long)B * K < (1ll << 27) && (long long)B * M < (1ll << 27),
               "roi_targets: bad shape (B=%d K=%d M=%d)", B, K, M);
  BEVF_REQUIRE(M == 0 || (gt && gt_labels), "roi_targets: null ground truth with M=%d", M);
  BEVF_REQUIRE(!match_labels || roi_labels, "roi_targets: match_labels needs the RoI labels");
  const TargetArgs a{rois, count, reinterpret_cast<const long long*>(roi_labels), gt, gt_labels, iou, gt_index, cls_target, reg_mask,
                     reg_target, B, K, M, use_bev, match_labels, reg_fg_thresh};
  return bevf_launch("bevf_roi_targets_f32", roi_targets_k, dim3((B * K + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), a);
}

extern "C" int bevf_roi_loss_f32(const float* pred, const int32_t* count, const float* cls_target, const uint8_t* reg_mask,
                                 const float* reg_target, float* out, int B, int K, float w_cls, float w_reg, void* stream) {
  LossArgs a;
  const int rc = loss_args(&a, "roi_loss", pred, count, cls_target, reg_mask, reg_target, B, K, w_cls, w_reg);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(out, "roi_loss: null output");
  return bevf_launch("bevf_roi_loss_f32", roi_loss_k, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a, out);
}

extern "C" int bevf_roi_loss_bwd_f32(const float* pred, const int32_t* count, const float* cls_target, const uint8_t* reg_mask,
                                     const float* reg_target, float* dpred, int B, int K, float w_cls, float w_reg, void* stream) {
  LossArgs a;
  const int rc = loss_args(&a, "roi_loss_bwd", pred, count, cls_target, reg_mask, reg_target, B, K, w_cls, w_reg);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(dpred, "roi_loss_bwd: null output");
  return bevf_launch("bevf_roi_loss_bwd_f32", roi_loss_bwd_k, dim3((B * K + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     dpred);
}

extern "C" int bevf_roi_refine_f32(const float* rois, const float* scores, const int64_t* labels, const float* velocities,
                                   const int32_t* count, const float* pred, float* out_boxes, float* out_scores, int64_t* out_labels,
                                   float* out_velocities, int32_t* out_count, int B, int K, float score_thresh, void* stream) {
  BEVF_REQUIRE(rois && scores && labels && count && pred && out_boxes && out_scores && out_labels && out_count,
               "roi_refine: null pointer");
  BEVF_REQUIRE(!velocities == !out_velocities, "roi_refine: velocities and out_velocities go together");
  BEVF_REQUIRE(B > 0 && B <= 65535 && K > 0 && K <= REFINE_MAX_K, "roi_refine: bad shape (B=%d K=%d; K <= %d)", B, K, REFINE_MAX_K);
  BEVF_REQUIRE(rois != out_boxes && scores != out_scores && (const void*)labels != (const void*)out_labels &&
                   count != out_count,
               "roi_refine: the outputs must not alias the inputs");
  const RefineArgs a{rois, scores, reinterpret_cast<const long long*>(labels), velocities, count, pred, out_boxes, out_scores,
                     reinterpret_cast<long long*>(out_labels), out_velocities, out_count, B, K, score_thresh};
  return bevf_launch("bevf_roi_refine_f32", roi_refine_k, dim3(B), dim3(256), (size_t)K * sizeof(float),
                     static_cast<hipStream_t>(stream), a);
}
