// IoU-aware head, training side (iou_aware.py): the IoU regression target of every ground-truth object, the L1
// loss of the iou map against it, and an aligned distance-IoU loss on the regressed box -- forward and backward.
//
// For an object (b, k) with reg_mask set, at the cell ind = cy * W + cx:
//   predicted box  x = (cx + offset[0]) * vx + x_min, y likewise, w = size[0], l = size[1], yaw = atan2f(rot[0], rot[1]) -- what
//                  decode_frame assembles, on the targets' cell size vx = (x_max - x_min) / W;
//   GT box         the same from target_offset / target_size / target_rot;
//   t            = 2 * IoU_bev(pred, gt) - 1   (box_geom.h: the rotated IoU of the NMS, 0 for w <= 0 or l <= 0), a constant;
//   iou term     = |iou_map[cell] - t|;
//   diou term    = 1 - (inter / (union + 1e-6) - rho^2 / (c^2 + 1e-6)) of the two rectangles in the GT box's frame, the predicted
//                  one taken parallel to it (OpenPCDet's aligned DIoU): sizes clamped below at 1e-3, gradients to offset and
//                  size[0:2].
// Both sums are divided by (sum of reg_mask over the batch + 1e-4).
//
// Determinism: no float atomics.  The forward reduces each frame in one workgroup (thread partials in k order, xor butterfly,
// four wave sums in order) and the frames in order; the backward stages every object's gradient in LDS and the lowest-k object of
// a cell sums the cell's objects in ascending k and stores once.  Objects whose ind lies outside the map are skipped.
#include "box_geom.h"

namespace {

constexpr float SIZE_MIN = 1e-3f;
constexpr int MAX_K = 2048;          // objects per frame the backward stages in LDS (6 words each)

struct IouArgs {
  const float* iou; const float* offset; const float* size; const float* rot;
  const float* toff; const float* tsize; const float* trot;
  const long long* ind; const unsigned char* mask;
  int B, K, H, W;
  float x_min, y_min, vx, vy;
};

struct ObjTerms {
  float t;                           // IoU target in [-1, 1]
  float diou;                        // 1 - d
  float g_ox, g_oy, g_w, g_l;        // d diou / d offset[0], offset[1], size[0], size[1]
};

__device__ __forceinline__ bool obj_valid(const IouArgs& a, int bk, int* cell) {
  if (!a.mask[bk]) return false;
  const long long i = a.ind[bk];
  if (i < 0 || i >= (long long)a.H * a.W) return false;
  *cell = (int)i;
  return true;
}

__device__ __forceinline__ ObjTerms obj_terms(const IouArgs& a, int b, int bk, int cell) {
  const int n = a.H * a.W;
  const int cy = cell / a.W, cx = cell - cy * a.W;
  const float* off = a.offset + (size_t)b * 2 * n;
  const float* sz = a.size + (size_t)b * 3 * n;
  const float* rt = a.rot + (size_t)b * 2 * n;
  const float ox = off[cell], oy = off[n + cell], wp = sz[cell], lp = sz[n + cell];
  const float gox = a.toff[bk * 2], goy = a.toff[bk * 2 + 1], wg = a.tsize[bk * 3], lg = a.tsize[bk * 3 + 1];
  const float s = a.trot[bk * 2], c = a.trot[bk * 2 + 1];
  ObjTerms o;
  {
    const float pb[7] = {((float)cx + ox) * a.vx + a.x_min, ((float)cy + oy) * a.vy + a.y_min, 0.f, wp, lp, 0.f,
                         atan2f(rt[cell], rt[n + cell])};
    const float gb[7] = {((float)cx + gox) * a.vx + a.x_min, ((float)cy + goy) * a.vy + a.y_min, 0.f, wg, lg, 0.f, atan2f(s, c)};
    o.t = 2.f * iou_bev(load_box(pb), load_box(gb)) - 1.f;
  }
  // aligned DIoU in the GT box's frame; the cell's origin cancels in the centre distance
  const float dx = (ox - gox) * a.vx, dy = (oy - goy) * a.vy;
  const float ex = c * dx + s * dy, ey = c * dy - s * dx;
  const float L = fmaxf(lp, SIZE_MIN), Wd = fmaxf(wp, SIZE_MIN);
  const float hl = 0.5f * lg, hw = 0.5f * wg;
  const float xh = ex + 0.5f * L, xl = ex - 0.5f * L, yh = ey + 0.5f * Wd, yl = ey - 0.5f * Wd;
  // which operand each min / max takes: 1 where it is the predicted rectangle's edge
  const float ih_x = xh < hl ? 1.f : 0.f, il_x = xl > -hl ? 1.f : 0.f, ih_y = yh < hw ? 1.f : 0.f, il_y = yl > -hw ? 1.f : 0.f;
  const float ovx = fminf(xh, hl) - fmaxf(xl, -hl), ovy = fminf(yh, hw) - fmaxf(yl, -hw);
  const bool hit = ovx > 0.f && ovy > 0.f;
  const float inter = hit ? ovx * ovy : 0.f;
  const float U = L * Wd + lg * wg - inter + 1e-6f;
  const float ch_x = 1.f - ih_x, cl_x = 1.f - il_x, ch_y = 1.f - ih_y, cl_y = 1.f - il_y;     // the enclosing rectangle's choices
  const float ex_len = fmaxf(xh, hl) - fminf(xl, -hl), ey_len = fmaxf(yh, hw) - fminf(yl, -hw);
  const float C2 = ex_len * ex_len + ey_len * ey_len + 1e-6f;
  const float rho2 = ex * ex + ey * ey;
  o.diou = 1.f - (inter / U - rho2 / C2);
  // d inter / d (ex, ey, L, Wd)
  const float di_ex = hit ? (ih_x - il_x) * ovy : 0.f, di_ey = hit ? (ih_y - il_y) * ovx : 0.f;
  const float di_L = hit ? 0.5f * (ih_x + il_x) * ovy : 0.f, di_W = hit ? 0.5f * (ih_y + il_y) * ovx : 0.f;
  const float iU2 = 1.f / (U * U), iC2 = 1.f / (C2 * C2);
  // d (inter / U): dU = -di for the centre, (other extent - di) for a size
  const float q_ex = (di_ex * U + inter * di_ex) * iU2, q_ey = (di_ey * U + inter * di_ey) * iU2;
  const float q_L = (di_L * U - inter * (Wd - di_L)) * iU2, q_W = (di_W * U - inter * (L - di_W)) * iU2;
  // d C2
  const float dc_ex = 2.f * ex_len * (ch_x - cl_x), dc_ey = 2.f * ey_len * (ch_y - cl_y);
  const float dc_L = ex_len * (ch_x + cl_x), dc_W = ey_len * (ch_y + cl_y);
  const float r_ex = (2.f * ex * C2 - rho2 * dc_ex) * iC2, r_ey = (2.f * ey * C2 - rho2 * dc_ey) * iC2;
  const float r_L = -rho2 * dc_L * iC2, r_W = -rho2 * dc_W * iC2;
  const float g_ex = -(q_ex - r_ex), g_ey = -(q_ey - r_ey);                                   // of 1 - d
  o.g_ox = (c * g_ex - s * g_ey) * a.vx;
  o.g_oy = (s * g_ex + c * g_ey) * a.vy;
  o.g_l = lp > SIZE_MIN ? -(q_L - r_L) : 0.f;
  o.g_w = wp > SIZE_MIN ? -(q_W - r_W) : 0.f;
  return o;
}

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// sum of v over the 256 threads, in a fixed order; every thread gets it.  red: 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// number of set reg_mask entries of the whole batch (an integer: exact in any order), as the loss's denominator
__device__ __forceinline__ float batch_denominator(const unsigned char* mask, int BK, int* red) {
  int m = 0;
  for (int i = threadIdx.x; i < BK; i += 256) m += mask[i] ? 1 : 0;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) m += __shfl_xor(m, s);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return (float)(red[0] + red[1] + red[2] + red[3]) + 1e-4f;
}

__global__ __launch_bounds__(256) void iou_targets_k(const IouArgs a, float* __restrict__ out) {
  const int total = a.B * a.K;
  for (int bk = blockIdx.x * 256 + threadIdx.x; bk < total; bk += gridDim.x * 256) {
    int cell;
    out[bk] = obj_valid(a, bk, &cell) ? obj_terms(a, bk / a.K, bk, cell).t : 0.f;
  }
}

// one workgroup per frame: part[b] = (sum |iou - t|, sum (1 - d))
__global__ __launch_bounds__(256) void iou_loss_frame(const IouArgs a, float* __restrict__ part) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  float si = 0.f, sd = 0.f;
  for (int k = threadIdx.x; k < a.K; k += 256) {
    const int bk = b * a.K + k;
    int cell;
    if (!obj_valid(a, bk, &cell)) continue;
    const ObjTerms o = obj_terms(a, b, bk, cell);
    si += fabsf(a.iou[(size_t)b * a.H * a.W + cell] - o.t);
    sd += o.diou;
  }
  si = block_sum(si, red);
  sd = block_sum(sd, red);
  if (threadIdx.x == 0) { part[2 * b] = si; part[2 * b + 1] = sd; }
}

// out[3] = total, iou_loss, diou_loss: the frames' sums in frame order over the batch's denominator
__global__ __launch_bounds__(256) void iou_loss_final(const IouArgs a, const float* __restrict__ part, float* __restrict__ out,
                                                      float w_iou, float w_diou) {
  __shared__ int red[4];
  const float denom = batch_denominator(a.mask, a.B * a.K, red);
  if (threadIdx.x != 0) return;
  float si = 0.f, sd = 0.f;
  for (int b = 0; b < a.B; ++b) { si += part[2 * b]; sd += part[2 * b + 1]; }
  const float li = si / denom, ld = sd / denom;
  out[0] = w_iou * li + w_diou * ld;
  out[1] = li;
  out[2] = ld;
}

// one workgroup per frame; d total / d (iou map, offset, size) stored at the objects' cells (the caller zero-fills the maps)
__global__ __launch_bounds__(256) void iou_loss_bwd_frame(const IouArgs a, float* __restrict__ d_iou, float* __restrict__ d_offset,
                                                          float* __restrict__ d_size, float w_iou, float w_diou) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* cells = reinterpret_cast<int*>(smem);                       // [K], -1 = no object
  float* g = reinterpret_cast<float*>(smem) + a.K;                 // [5][K]: iou, offset x, offset y, w, l
  __shared__ int red[4];
  const int b = blockIdx.x, K = a.K, n = a.H * a.W;
  const float inv = 1.f / batch_denominator(a.mask, a.B * K, red);
  for (int k = threadIdx.x; k < K; k += 256) {
    const int bk = b * K + k;
    int cell;
    if (!obj_valid(a, bk, &cell)) { cells[k] = -1; continue; }
    const ObjTerms o = obj_terms(a, b, bk, cell);
    cells[k] = cell;
    g[k] = w_iou * sgn(a.iou[(size_t)b * n + cell] - o.t) * inv;
    g[K + k] = w_diou * o.g_ox * inv;
    g[2 * K + k] = w_diou * o.g_oy * inv;
    g[3 * K + k] = w_diou * o.g_w * inv;
    g[4 * K + k] = w_diou * o.g_l * inv;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) {
    const int cell = cells[k];
    if (cell < 0) continue;
    // one pass over the frame's cells (LDS broadcasts, no early exit, so the reads pipeline): an earlier object of the cell owns
    // it; otherwise the later ones are added in ascending j
    bool first = true;
    float s[5] = {g[k], g[K + k], g[2 * K + k], g[3 * K + k], g[4 * K + k]};
#pragma unroll 8
    for (int j = 0; j < K; ++j) {
      if (cells[j] != cell || j == k) continue;
      if (j < k) first = false;
      else {
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] += g[q * K + j];
      }
    }
    if (!first) continue;
    d_iou[(size_t)b * n + cell] = s[0];
    d_offset[((size_t)b * 2) * n + cell] = s[1];
    d_offset[((size_t)b * 2 + 1) * n + cell] = s[2];
    d_size[((size_t)b * 3) * n + cell] = s[3];
    d_size[((size_t)b * 3 + 1) * n + cell] = s[4];
  }
}

static int make_args(IouArgs* a, const char* what, const float* iou, bool need_iou, const float* offset, const float* size,
                     const float* rot, const float* toff, const float* tsize, const float* trot, const int64_t* ind,
                     const uint8_t* mask, int B, int K, int H, int W, float x_min, float y_min, float x_max, float y_max) {
  BEVF_REQUIRE((iou || !need_iou) && offset && size && rot && toff && tsize && trot && ind && mask, "%s: null pointer", what);
  BEVF_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, "%s: empty shape", what);
  BEVF_REQUIRE((long long)H * W < (1ll << 30) && (long long)B * K < (1ll << 28), "%s: shape too large", what);
  BEVF_REQUIRE(x_max > x_min && y_max > y_min, "%s: empty point-cloud range", what);
  a->iou = iou; a->offset = offset; a->size = size; a->rot = rot; a->toff = toff; a->tsize = tsize; a->trot = trot;
  a->ind = reinterpret_cast<const long long*>(ind); a->mask = mask;
  a->B = B; a->K = K; a->H = H; a->W = W;
  a->x_min = x_min; a->y_min = y_min; a->vx = (x_max - x_min) / (float)W; a->vy = (y_max - y_min) / (float)H;
  return BEVF_OK;
}

}  // namespace

extern "C" int bevf_iou_targets_f32(const float* offset, const float* size, const float* rot, const float* target_offset,
                                    const float* target_size, const float* target_rot, const int64_t* ind,
                                    const uint8_t* reg_mask, float* out, int B, int K, int H, int W, float x_min, float y_min,
                                    float x_max, float y_max, void* stream) {
  IouArgs a;
  const int rc = make_args(&a, "iou_targets", nullptr, false, offset, size, rot, target_offset, target_size, target_rot, ind,
                           reg_mask, B, K, H, W, x_min, y_min, x_max, y_max);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(out, "iou_targets: null output");
  const int grid = (B * K + 255) / 256;
  hipLaunchKernelGGL(iou_targets_k, dim3(grid < 1024 ? grid : 1024), dim3(256), 0, static_cast<hipStream_t>(stream), a, out);
  return bevf_check_launch("bevf_iou_targets_f32");
}

extern "C" size_t bevf_iou_aware_loss_work_floats(int B) { return (size_t)2 * (B > 0 ? B : 0); }

extern "C" int bevf_iou_aware_loss_f32(const float* iou, const float* offset, const float* size, const float* rot,
                                       const float* target_offset, const float* target_size, const float* target_rot,
                                       const int64_t* ind, const uint8_t* reg_mask, float* work, float* out, int B, int K, int H,
                                       int W, float x_min, float y_min, float x_max, float y_max, float w_iou, float w_diou,
                                       void* stream) {
  IouArgs a;
  const int rc = make_args(&a, "iou_aware_loss", iou, true, offset, size, rot, target_offset, target_size, target_rot, ind,
                           reg_mask, B, K, H, W, x_min, y_min, x_max, y_max);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(work && out, "iou_aware_loss: null work / output");
  BEVF_REQUIRE(B <= 65535, "iou_aware_loss: B=%d too large for one grid", B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(iou_loss_frame, dim3(B), dim3(256), 0, st, a, work);
  hipLaunchKernelGGL(iou_loss_final, dim3(1), dim3(256), 0, st, a, work, out, w_iou, w_diou);
  return bevf_check_launch("bevf_iou_aware_loss_f32");
}

extern "C" int bevf_iou_aware_loss_bwd_f32(const float* iou, const float* offset, const float* size, const float* rot,
                                           const float* target_offset, const float* target_size, const float* target_rot,
                                           const int64_t* ind, const uint8_t* reg_mask, float* d_iou, float* d_offset,
                                           float* d_size, int B, int K, int H, int W, float x_min, float y_min, float x_max,
                                           float y_max, float w_iou, float w_diou, void* stream) {
  IouArgs a;
  const int rc = make_args(&a, "iou_aware_loss_bwd", iou, true, offset, size, rot, target_offset, target_size, target_rot, ind,
                           reg_mask, B, K, H, W, x_min, y_min, x_max, y_max);
  if (rc != BEVF_OK) return rc;
  BEVF_REQUIRE(d_iou && d_offset && d_size, "iou_aware_loss_bwd: null gradient pointer");
  BEVF_REQUIRE(B <= 65535, "iou_aware_loss_bwd: B=%d too large for one grid", B);
  BEVF_REQUIRE(K <= MAX_K, "iou_aware_loss_bwd: max_objects=%d exceeds %d (one frame's objects are staged in LDS)", K, MAX_K);
  hipLaunchKernelGGL(iou_loss_bwd_frame, dim3(B), dim3(256), (size_t)6 * K * sizeof(float), static_cast<hipStream_t>(stream), a,
                     d_iou, d_offset, d_size, w_iou, w_diou);
  return bevf_check_launch("bevf_iou_aware_loss_bwd_f32");
}
