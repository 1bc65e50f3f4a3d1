// Box-to-box geometry of the decode path: rotated BEV / 3-D IoU and greedy box NMS (rotated-IoU or circle), on device.
//
// Box convention (include/bevf.h): [x, y, z, w, l, h, yaw] is the rectangle centred at (x, y) with extent l along the
// heading (cos yaw, sin yaw) and w across it, z-extent [z - h/2, z + h/2].
//
// Intersection area.  Box b is translated by -centre(a) and rotated by -yaw(a) first, so a becomes the axis-aligned
// rectangle R = [-la/2, la/2] x [-wa/2, wa/2] and every later quantity is relative to it (fp32 error does not grow with the
// distance from the origin).  Each of b's four edges is then clipped against R in closed form: with b counter-clockwise,
//     area(b & R) = - sum over edges  dx * integral_{t0}^{t1} clamp(y(t), -wa/2, wa/2) dt,
// where [t0, t1] is the part of the edge inside the strip |x| <= la/2 and y(t) is linear, so the integral is one constant
// piece, one trapezoid and one constant piece.  This is Sutherland-Hodgman's per-edge clipping with the shoelace sum taken
// edge by edge: no vertex list, no sort by angle, nothing indexed at run time (all in registers), and every term is bounded
// by la * wa whatever the angle between the edges -- near-parallel edges only make a division saturate into a clamp.
#include "box_geom.h"

namespace {

__device__ __forceinline__ int frame_count(const int32_t* count, int b, int n) {
  if (!count) return n;
  const int c = count[b];
  return c < 0 ? 0 : (c > n ? n : c);
}

// ---- pairwise IoU: one workgroup (4 waves) per 64 x 64 tile of out[b]; both box tiles staged once in LDS ---------------
__global__ __launch_bounds__(256) void boxes_iou_tile(const float* A, const int32_t* cntA, const float* Bx, const int32_t* cntB,
                                                      float* out, int N, int M, int mode) {
  __shared__ RBox rows[64], cols[64];
  const int b = blockIdx.z, r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, tid = threadIdx.x;
  const int na = frame_count(cntA, b, N), nb = frame_count(cntB, b, M);
  if (tid < 64) {
    if (r0 + tid < na) rows[tid] = load_box(A + ((size_t)b * N + r0 + tid) * 7);
  } else if (tid < 128) {
    const int j = tid - 64;
    if (c0 + j < nb) cols[j] = load_box(Bx + ((size_t)b * M + c0 + j) * 7);
  }
  __syncthreads();
  const int j = tid & 63, col = c0 + j;
  if (col >= M) return;
  const RBox cb = cols[j];                                                 // unused where col >= nb
  for (int r = tid >> 6; r < 64; r += 4) {
    const int row = r0 + r;
    if (row >= N) break;
    float v = 0.f;
    if (row < na && col < nb) v = mode ? iou_3d(rows[r], cb) : iou_bev(rows[r], cb);
    out[((size_t)b * N + row) * M + col] = v;
  }
}

// ---- NMS stage (a): one wave per 64 x 64 tile of the upper triangle.  Lane = row box i; bit jj of the lane's word says that
// box i suppresses box j = 64 * cb + jj (j > i).  The 64 column boxes are staged once in LDS and read as broadcasts. --------
struct ColBox { RBox g; long long label; };

__global__ __launch_bounds__(64) void nms_mask_tile(const float* boxes, const long long* labels, const int32_t* count,
                                                    unsigned long long* mask, int N, int nblk, int circle, float thresh,
                                                    int class_aware) {
  __shared__ ColBox cols[64];
  const int b = blockIdx.z, rb = blockIdx.y, cb = blockIdx.x, lane = threadIdx.x;
  if (cb < rb) return;
  const int n = frame_count(count, b, N);
  if (rb * 64 >= n || cb * 64 >= n) return;                                // the scan never reads these tiles
  const int j0 = cb * 64, i = rb * 64 + lane;
  if (j0 + lane < n) {
    cols[lane].g = load_box(boxes + ((size_t)b * N + j0 + lane) * 7);
    cols[lane].label = class_aware ? labels[(size_t)b * N + j0 + lane] : 0;
  }
  __syncthreads();
  unsigned long long word = 0ull;
  if (i < n) {
    RBox a;
    long long la;
    if (cb == rb) { a = cols[lane].g; la = cols[lane].label; }
    else {
      a = load_box(boxes + ((size_t)b * N + i) * 7);
      la = class_aware ? labels[(size_t)b * N + i] : 0;
    }
    const float ra = sqrtf(a.hl * a.hl + a.hw * a.hw), r2 = thresh * thresh;
    const int jn = (n - j0 < 64) ? n - j0 : 64;
    for (int jj = 0; jj < jn; ++jj) {
      const ColBox& c = cols[jj];
      const float dx = c.g.x - a.x, dy = c.g.y - a.y, d2 = dx * dx + dy * dy;
      bool hit;
      if (circle) {
        hit = d2 < r2;
      } else {
        // rectangles whose circumscribed circles are more than a rounding margin apart cannot touch: IoU is exactly 0
        const float reach = (ra + sqrtf(c.g.hl * c.g.hl + c.g.hw * c.g.hw)) * 1.0001f;
        hit = (d2 <= reach * reach) && (iou_bev(a, c.g) > thresh);
      }
      if (hit && j0 + jj > i && c.label == la) word |= 1ull << jj;
    }
  }
  if (i < n) mask[((size_t)b * N + i) * nblk + cb] = word;                 // rows past n are never read (and may lie past N)
}

// ---- NMS stage (b): one wave per frame.  Lane w holds the "removed" bits of boxes 64w .. 64w+63; the mask rows of one 64-row
// block are staged in LDS, the serial walk visits only rows that are still alive and reads LDS, never global memory. ----------
struct ScanArgs {
  const float* boxes; const float* scores; const long long* labels; const float* vels; const int32_t* count;
  const unsigned long long* mask;
  int32_t* keep_idx; int32_t* keep_count;
  float* o_boxes; float* o_scores; long long* o_labels; float* o_vels;
  int N, nblk, post_max;
};

__global__ __launch_bounds__(64) void nms_scan_frame(const ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* rowsm = reinterpret_cast<unsigned long long*>(smem);       // [64][nw]
  const int b = blockIdx.x, lane = threadIdx.x, N = a.N;
  const int n = frame_count(a.count, b, N);
  const int nb = (n + 63) >> 6;
  unsigned long long removed = 0ull;
  int nkept = 0;
  for (int rb = 0; rb < nb && nkept < a.post_max; ++rb) {
    const int left = n - rb * 64;
    const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    unsigned long long cur = __shfl(removed, rb);                          // removed bits of this block, wave-uniform
    if ((~cur & valid) == 0ull) continue;                                  // the whole block is already suppressed
    const int nw = nb - rb;
    __syncthreads();
    for (int e = lane; e < 64 * nw; e += 64) {
      const int r = e / nw, w = e - r * nw;
      rowsm[e] = (rb * 64 + r < n) ? a.mask[((size_t)b * N + (size_t)rb * 64 + r) * a.nblk + rb + w] : 0ull;
    }
    __syncthreads();
    unsigned long long kept = 0ull, acc = 0ull;
    const bool mine = lane >= rb && lane < nb;
    int room = a.post_max - nkept;
    unsigned long long alive = ~cur & valid;
    while (alive != 0ull && room > 0) {
      const int r = __builtin_ctzll(alive);
      kept |= 1ull << r;
      --room;
      if (mine) acc |= rowsm[r * nw + lane - rb];
      cur |= rowsm[r * nw];                                                // the diagonal word: one broadcast LDS read
      alive = ~cur & valid & ~((2ull << r) - 1ull);
    }
    removed |= acc;
    if ((kept >> lane) & 1ull) {
      const int pos = nkept + __builtin_popcountll(kept & ((1ull << lane) - 1ull));
      const size_t src = (size_t)b * N + rb * 64 + lane, dst = (size_t)b * N + pos;
      a.keep_idx[dst] = rb * 64 + lane;
      if (a.o_boxes) for (int q = 0; q < 7; ++q) a.o_boxes[dst * 7 + q] = a.boxes[src * 7 + q];
      if (a.o_scores) a.o_scores[dst] = a.scores[src];
      if (a.o_labels) a.o_labels[dst] = a.labels[src];
      if (a.o_vels) { a.o_vels[dst * 2] = a.vels[src * 2]; a.o_vels[dst * 2 + 1] = a.vels[src * 2 + 1]; }
    }
    nkept += __builtin_popcountll(kept);
  }
  for (int p = nkept + lane; p < N; p += 64) {                             // padding: -1 / zeros, so two runs are bit-equal
    const size_t dst = (size_t)b * N + p;
    a.keep_idx[dst] = -1;
    if (a.o_boxes) for (int q = 0; q < 7; ++q) a.o_boxes[dst * 7 + q] = 0.f;
    if (a.o_scores) a.o_scores[dst] = 0.f;
    if (a.o_labels) a.o_labels[dst] = 0;
    if (a.o_vels) { a.o_vels[dst * 2] = 0.f; a.o_vels[dst * 2 + 1] = 0.f; }
  }
  if (lane == 0) a.keep_count[b] = nkept;
}

}  // namespace

extern "C" int bevf_boxes_iou_f32(const float* a, const int32_t* count_a, const float* b, const int32_t* count_b, float* out,
                                  int B, int N, int M, int mode, void* stream) {
  BEVF_REQUIRE(a && b && out, "boxes_iou: null pointer");
  BEVF_REQUIRE(B > 0 && N > 0 && M > 0, "boxes_iou: empty shape");
  BEVF_REQUIRE(mode == BEVF_IOU_BEV || mode == BEVF_IOU_3D, "boxes_iou: mode %d is neither bev (0) nor 3d (1)", mode);
  BEVF_REQUIRE(B <= 65535 && (N + 63) / 64 <= 65535, "boxes_iou: B=%d / N=%d too large for one grid", B, N);
  hipLaunchKernelGGL(boxes_iou_tile, dim3((M + 63) / 64, (N + 63) / 64, B), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     count_a, b, count_b, out, N, M, mode);
  return bevf_check_launch("bevf_boxes_iou_f32");
}

extern "C" size_t bevf_nms_boxes_work_bytes(int B, int N) {
  return (size_t)B * N * ((N + 63) / 64) * sizeof(unsigned long long);
}

extern "C" int bevf_nms_boxes_f32(const float* boxes, const float* scores, const int64_t* labels, const float* velocities,
                                  const int32_t* count, int B, int N, int mode, float thresh, int class_aware, int post_max,
                                  void* work, int32_t* keep_idx, int32_t* keep_count, float* out_boxes, float* out_scores,
                                  int64_t* out_labels, float* out_velocities, void* stream) {
  BEVF_REQUIRE(boxes && work && keep_idx && keep_count, "nms_boxes: null pointer");
  BEVF_REQUIRE(B > 0 && N > 0, "nms_boxes: empty shape");
  BEVF_REQUIRE(N <= 4096, "nms_boxes: N=%d exceeds 4096 (one removed word per lane)", N);
  BEVF_REQUIRE(B <= 65535, "nms_boxes: B=%d too large for one grid", B);
  BEVF_REQUIRE(mode == BEVF_NMS_ROTATE || mode == BEVF_NMS_CIRCLE, "nms_boxes: mode %d is neither rotate (0) nor circle (1)", mode);
  BEVF_REQUIRE(thresh >= 0.f, "nms_boxes: threshold / radius must be >= 0");
  BEVF_REQUIRE(!class_aware || labels, "nms_boxes: class_aware needs labels");
  BEVF_REQUIRE(post_max > 0, "nms_boxes: post_max must be positive");
  BEVF_REQUIRE((!out_scores || scores) && (!out_labels || labels) && (!out_velocities || velocities),
               "nms_boxes: a gathered output without its input");
  BEVF_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, "nms_boxes: work must be 8-byte aligned");
  const int nblk = (N + 63) / 64;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* mask = static_cast<unsigned long long*>(work);
  hipLaunchKernelGGL(nms_mask_tile, dim3(nblk, nblk, B), dim3(64), 0, st, boxes, (const long long*)labels, count, mask, N, nblk,
                     mode == BEVF_NMS_CIRCLE, thresh, class_aware);
  ScanArgs a;
  a.boxes = boxes; a.scores = scores; a.labels = (const long long*)labels; a.vels = velocities; a.count = count; a.mask = mask;
  a.keep_idx = keep_idx; a.keep_count = keep_count;
  a.o_boxes = out_boxes; a.o_scores = out_scores; a.o_labels = (long long*)out_labels; a.o_vels = out_velocities;
  a.N = N; a.nblk = nblk; a.post_max = post_max;
  hipLaunchKernelGGL(nms_scan_frame, dim3(B), dim3(64), (size_t)64 * nblk * 8, st, a);
  return bevf_check_launch("bevf_nms_boxes_f32");
}
