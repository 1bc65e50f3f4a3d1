/*
 * bevf.h -- C-ABI of libbevf_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * BEV-fusion detector hot path of meg89/bevfusion_multimodal_3d_object_detection.
 *
 * The reference has no FFI of its own: its boundary is the Python module API
 * of src/encoders.py, src/fusion.py, src/fusion_detection.py and src/centernet_target.py.  Each
 * entry point below names the reference lines whose arithmetic it replaces; the Python host
 * in bevfusion_multimodal_3d_object_detection_amd/ binds them with ctypes and keeps the
 * reference's class names, constructor signatures and state-dict keys.
 *
 * Conventions: plain device pointers and sizes, no torch types; every call is asynchronous on
 * `stream` (a hipStream_t passed as void*), never allocates, never synchronises, is re-entrant
 * and graph-capturable; returns 0 or a negative bevf_status, message via bevf_last_error().
 * Activations are fp32 NHWC ("pixel-major": [image][row][col][channel]) with an explicit
 * per-pixel channel stride so producers write straight into channel slices of a concat buffer.
 */
#ifndef BEVF_H
#define BEVF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  BEVF_OK = 0,
  BEVF_ERR_ARG = -1,      /* shape / alignment / null-pointer contract violated */
  BEVF_ERR_LAUNCH = -2,   /* hipLaunchKernel reported an error */
  BEVF_ERR_UNSUPPORTED = -3
} bevf_status;

int bevf_version(void);
const char* bevf_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM 2-D convolution on v_mfma_f32_32x32x2_f32 (exact fp32), fused epilogue
 *     y = act( conv(x, w) * scale + shift (+ res) )
 * Replaces every nn.Conv2d(+BatchNorm2d eval)(+ReLU)(+residual add) on the path:
 *   ResNet-18 layer1..3 + channel_proj   ref src/encoders.py:159-165 (torchvision BasicBlock)
 *   camera_proj / lidar_upsample / radar_refine / bev_fusion   ref src/fusion.py:126-207,239-295
 *   CenterNet 3x3 branches (5 fused into one Cout=320 conv)    ref src/fusion.py:822-854
 * and, with KH=KW=1, the shared per-point MLP layers (nn.Conv1d k=1 + BatchNorm1d + ReLU)
 *   PointNetLiDAREncoder conv2..conv5   ref src/encoders.py:290-295
 * With `colmax` set the output is not stored; instead the per-group column maximum
 * (torch.max(x, 2)[0], ref src/encoders.py:298) is accumulated with integer atomics on the
 * non-negative post-ReLU bit patterns (order-independent, hence deterministic).
 * Requires Cin % 32 == 0, x_cs % 4 == 0, 16-byte aligned x / w, and x / w below 2 GiB each (32-bit buffer
 * offsets; callers chunk larger batches over images).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* x;      /* [N][H][W][x_cs], first Cin channels of each pixel are read        */
  const float* w;      /* [Cout][KH][KW][Cin]  (OHWI)                                        */
  const float* scale;  /* [Cout] or NULL (1)   folded BN: gamma / sqrt(var + eps)            */
  const float* shift;  /* [Cout] or NULL (0)   beta - mean*scale + conv_bias*scale           */
  const float* res;    /* optional residual [N*Ho*Wo][res_cs], added before the activation   */
  float* y;            /* [N*Ho*Wo][y_cs] (may be NULL when colmax is set)                   */
  uint32_t* colmax;    /* optional [ceil(M/rows_per_group)][Cout], caller zeroes it          */
  int32_t N, H, W, Cin, x_cs;
  int32_t Ho, Wo, Cout, y_cs, res_cs;
  int32_t KH, KW, stride, pad;
  int32_t relu;            /* 0: none, 1: ReLU                                               */
  int32_t rows_per_group;  /* colmax grouping (points per batch element)                     */
  int32_t tile;            /* 0: auto (cost model); 1 128x128, 2 256x64, 3 128x64, 4 64x64, 5-7 hybrid
                              big + 64x64 tail of 1 / 2 / 3 -- forced variants for bench / tests     */
  /* bevf_conv3x3_wino_f32 only (training forward, ref train-mode nn.BatchNorm2d after the conv): when `stats` is set the
   * epilogue also leaves per-tile-block partial sums of the stored outputs, {sum(y - pivot), sum((y - pivot)^2)}
   * per channel, as rows [bevf_wino_stat_rows(N,H,W)][Cout][2] for bevf_bn_stats_from_partials_f32 -- the BatchNorm
   * batch statistics without re-reading the activation.  Needs relu = 0 and res = NULL. */
  float* stats;
  const float* stats_pivot; /* [Cout] any value near the channel mean (e.g. the running mean); NULL = 0 */
  /* bevf_conv3x3_wino_f32 only (training backward): when `bnb_x` is set, this convolution's output (+ res) is the gradient
   * dY reaching a train-mode BatchNorm(+ReLU) layer, and the epilogue does that layer's first backward pass on the way out
   * (what bevf_bn_backward_f32 would start with): dY is stored with the layer's ReLU mask applied -- mask from its output
   * `bnb_y`, or, if NULL (the layer had no residual input), recomputed from its raw input `bnb_x` exactly as the forward did --
   * and `stats` receives {sum dY, sum dY * xhat} per (tile block, channel) for bevf_bn_backward_from_partials_f32.
   * bnb_x / bnb_y: [N*H*W][Cout]; bnb_mean, bnb_invstd (required), bnb_gamma, bnb_beta (NULL = 1 / 0): [Cout].
   * Needs relu = 0, stats_pivot = NULL, y_cs == Cout. */
  const float* bnb_x;
  const float* bnb_y;
  const float* bnb_mean;
  const float* bnb_invstd;
  const float* bnb_gamma;
  const float* bnb_beta;
} bevf_conv_desc;
int bevf_conv2d_nhwc_f32(const bevf_conv_desc* d, void* stream);
/* The same launch, decided on the device by results computed earlier on the stream, with no host round trip (both optional):
 * run_if: device word; when it reads 0 every workgroup of the launch returns at once and nothing is written.
 * group_rows: device array [groups], with colmax and no y only: rows at or past group_rows[g] inside group g are not wanted, and a
 * tile that holds only such rows is skipped.  Every row of a tile that does run is read, so the caller fills the group's slots up to
 * the next multiple of 128 with rows that may take part in the max.  rows_per_group % 128 == 0; not with the 256-row tile variants
 * (tile = 2, 6).  (Arguments, not descriptor fields: the descriptor's layout is pinned by recorded launch traces.) */
int bevf_conv2d_nhwc_f32_if(const bevf_conv_desc* d, const int32_t* run_if, const int32_t* group_rows, void* stream);

/* The same convolution for the 3x3 / stride 1 / pad 1 layers (ResNet blocks, camera_proj, lidar_upsample, radar_refine,
 * bev_fusion, the fused CenterNet 3x3: ~90 % of the path's FLOPs) as fp32 Winograd F(2x2,3x3), fully fused, on
 * v_mfma_f32_16x16x4_f32: 16 multiplies per 2x2 outputs instead of 36.  fp32 products and fp32 accumulation as in the
 * direct kernel, a different summation structure: agrees with it to a few 1e-7 relative, not bit for bit.
 * `d->w` is the transformed-filter image made by bevf_wino_filter_transform_f32 from the OHWI filter
 * (bevf_wino_filter_floats(Cout, Cin) floats); everything else in the descriptor means what it means above
 * (colmax unsupported, `tile` ignored).  Requires KH = KW = 3, stride 1, pad 1, Cin % 32 == 0. */
size_t bevf_wino_filter_floats(int Cout, int Cin);
int bevf_wino_filter_transform_f32(const float* w_ohwi, float* u, int Cout, int Cin, void* stream);
int bevf_conv3x3_wino_f32(const bevf_conv_desc* d, void* stream);
int bevf_wino_stat_rows(int N, int H, int W);   /* rows of the `stats` partial buffer */

/* ResNet stem: 7x7 stride-2 pad-3 conv on a planar 3-channel image + BN (+ ReLU when relu != 0),
 * ref src/encoders.py:154-156 (torchvision conv1/bn1/relu).  x: [N][3][H][W] (NCHW, as the
 * reference's callers hand it over), w: the filter bank packed k-major [148][64] with
 * k = c*49 + kh*7 + kw and a zero row k = 147 (packed once per weight update by the host),
 * y: [N][Ho][Wo][64] NHWC.                                                                  */
int bevf_stem_conv7x7_f32(const float* x, const float* w, const float* scale, const float* shift,
                          float* y, int N, int H, int W, int relu, void* stream);
/* conv1 + bn1 + relu + maxpool(3, stride 2, pad 1) of ref src/encoders.py:154-157 in ONE kernel (inference): y is the pooled
 * NHWC map [N][Hp][Wp][64]; the stem map itself (the largest activation of the path) never reaches HBM.  Bit-identical to
 * bevf_stem_conv7x7_f32(relu = 1) followed by bevf_maxpool3x3s2_nhwc_f32. */
int bevf_stem_pool_f32(const float* x, const float* w_packed, const float* scale, const float* shift, float* y, int N,
                       int H, int W, void* stream);

/* 3x3 stride-2 pad-1 max-pool, NHWC, ref src/encoders.py:157.                               */
int bevf_maxpool3x3s2_nhwc_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* Small-K pointwise layer y[m][n] = act((sum_k x[m][k] w[n][k]) * scale[n] + shift[n]), K <= 16:
 * PointNet conv1 (K = 4|5), ref src/encoders.py:289.                                         */
int bevf_pointwise_smallk_f32(const float* x, const float* w, const float* scale, const float* shift,
                              float* y, int M, int K, int Cout, int relu, void* stream);

/* PointNet conv1 -> conv2 -> conv3 (K -> 64 -> 128 -> 256, each with folded BatchNorm + ReLU; ref src/encoders.py:289-291:
 * `x = F.relu(self.bn1(self.conv1(x)))` ... `bn3(conv3(x))`) as ONE launch whose 64- and 128-wide activations stay in
 * registers.  x: [M][K] points (K <= 8), w1: [64][K], w2f / w3f: the [128][64] and [256][128] filters in MFMA fragment
 * order (bevf_pointnet_front_pack_f32), s* / b*: per-channel scale / shift, y: [M][256].                              */
int bevf_pointnet_front_f32(const float* x, int M, int K, const float* w1, const float* s1, const float* b1,
                            const float* w2f, const float* s2, const float* b2, const float* w3f, const float* s3,
                            const float* b3, float* y, void* stream);
/* w: [Cout][Cin] row-major (Conv1d k=1 weight) -> wf: [Cout/32][Cin/32][4][64][4] fragments for the kernel above.     */
int bevf_pointnet_front_pack_f32(const float* w, float* wf, int Cout, int Cin, void* stream);

/* y[g][c] = max over the P rows of group g: the per-voxel max of VFELayer ("pillar reduction"),
 * ref src/encoders.py:451-452.  x: [G][P][C] post-ReLU point features -> y: [G][C].           */
int bevf_group_max_f32(const float* x, float* y, int G, int P, int C, void* stream);
/* The whole VFELayer for K <= 16 input channels in one pass (ref src/encoders.py:431-455): y[g][n] = max over the P rows of
 * group g of relu((x[g][p][:] . w[n][:]) * scale[n] + shift[n]); bit-identical to bevf_pointwise_smallk_f32 followed by
 * bevf_group_max_f32, without the [G][P][Cout] intermediate.  x: [G][P][K], w: [Cout][K], y: [G][Cout].               */
int bevf_vfe_smallk_max_f32(const float* x, const float* w, const float* scale, const float* shift, float* y, int G, int P,
                            int K, int Cout, void* stream);

/* One radar sweep -> 256-d feature: 4 x (Conv1d k=1 + BN + ReLU) + max over points, all in
 * LDS, one workgroup per (radar, batch element, 32-point chunk); `out` must be ZERO-FILLED (the chunk maxima
 * are merged with integer atomicMax).  ref src/encoders.py:549-555, loop :642-644.
 * x: [R][B][P][Cin]; w_i packed k-major [c_{i-1}][c_i]; out: [B][R][c4] (== torch.stack(dim=1)). */
typedef struct {
  const float* x;
  const float* w[4];
  const float* scale[4];
  const float* shift[4];
  float* out;
  int32_t R, B, P, Cin;
  int32_t c[4];
} bevf_radar_desc;
int bevf_radar_mlp_max_f32(const bevf_radar_desc* d, void* stream);

/* Dense layer for small batch (weight-streaming GEMV): y[b][perm(o)] = act(W[o].x[b] + bias[o]).
 * lidar_init (ref src/fusion.py:144-148,258), radar_proj (:183-186,274), fusion_fc
 * (ref src/encoders.py:624,653).  perm(o) = (o % perm_inner) * perm_outer + o / perm_inner when
 * perm_inner > 0 (writes the (B,128,25,25) view of ref :259 directly as NHWC), else o.        */
int bevf_linear_f32(const float* x, const float* w, const float* bias, float* y, int B, int K, int O,
                    int relu, int perm_inner, int perm_outer, void* stream);

/* Camera "BEV pooling" part 1: mean over the cameras, ref src/fusion.py:233-234.
 * x: [B][ncam][P][C] -> y: [B][P][C]; sum in camera order, then true division by ncam.       */
int bevf_cam_mean_f32(const float* x, float* y, int B, int ncam, int P, int C, void* stream);

/* Camera "BEV pooling" part 2 / nn.Upsample: bilinear resample, align_corners=False,
 * ref src/fusion.py:242-247 and :156.  NHWC in (stride x_cs) -> NHWC out slice (stride y_cs). */
int bevf_bilinear_nhwc_f32(const float* x, float* y, int B, int Hi, int Wi, int C, int x_cs,
                           int Ho, int Wo, int y_cs, void* stream);

/* radar broadcast, ref src/fusion.py:277-278: y[b][p][0:C] = v[b][0:C] for p < P.            */
int bevf_broadcast_nhwc_f32(const float* v, float* y, int B, int P, int C, int y_cs, void* stream);

/* Radar branch shortcut (exact): a 3x3/pad-1 conv stack on a spatially constant image yields at most 5x5
 * distinct pixels after two layers (a pixel's value depends only on its border class per axis), so
 * radar_refine (ref src/fusion.py:189-196,281) runs on a 5x5 image and this expands the classes:
 * y[b][i][j][0:C] = small[b][cls(i)][cls(j)][0:C], cls(i) = i<2 ? i : (i>=S-2 ? 4-(S-1-i) : 2).        */
int bevf_expand_border_classes_f32(const float* small, float* y, int B, int Sh, int Sw, int C, int y_cs,
                                   void* stream);

/* CenterNet head tail: block-diagonal 1x1 convs of the five branches + sigmoid on the heatmap,
 * ref src/fusion.py:825,832,839,846,853,869-884.  hid: [B*P][5*hc] post-ReLU hidden maps;
 * w: concatenated [sum(c_k)][hc]; bias: [sum(c_k)]; outputs NCHW (B,c_k,H,W) as the reference
 * returns them.  n_sigmoid = number of leading output channels passed through sigmoid.       */
typedef struct {
  const float* hid;
  const float* w;
  const float* bias;
  float* out[5];
  int32_t B, P, hc;
  int32_t c[5];
  int32_t n_sigmoid;
} bevf_head_desc;
int bevf_head_tail_f32(const bevf_head_desc* d, void* stream);

/* Layout changes at the module-API boundary (the reference's tensors are NCHW).              */
int bevf_nchw_to_nhwc_f32(const float* x, float* y, int N, int C, int P, int y_cs, void* stream);
int bevf_nhwc_to_nchw_f32(const float* x, float* y, int N, int C, int P, int x_cs, void* stream);

/* (N,P,Cin) point rows -> NHWC rows of a padded width (zero fill), for Cin not a multiple of 4 */
int bevf_fill_f32(float* y, float v, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Post-processing, ref src/centernet_target.py:326-452 / src/fusion_detection.py:695-820:
 * 3x3 keep-mask (_nms), per-class top-K then top-K of the C*K pool (_topk), gather + box
 * assembly.  One workgroup per batch element; outputs are fixed-size [B][K] records plus a
 * per-frame count of entries with score > thresh (they are a prefix: scores are sorted).
 * Ties are broken by the lower flattened index, like a stable descending sort.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* heat;   /* (B,C,H,W) post-sigmoid */
  const float* offset; /* (B,2,H,W) */
  const float* size;   /* (B,3,H,W) */
  const float* rot;    /* (B,2,H,W) */
  const float* vel;    /* (B,2,H,W) */
  float* boxes;        /* [B][K][7]  x,y,z,w,l,h,yaw */
  float* scores;       /* [B][K]     descending */
  int64_t* labels;     /* [B][K]     */
  float* velocities;   /* [B][K][2]  */
  int32_t* count;      /* [B]        entries with score > thresh (a prefix) */
  void* work;          /* scratch of bevf_centernet_decode_work_bytes(B,C,H,W,K) bytes */
  int64_t* pool_ind;   /* [B][K] or NULL: position of each winner in the flattened (C,K) pool of per-class
                          winners -- the second return value of the reference's _topk (ref centernet_target.py:441) */
  int32_t B, C, H, W, K;
  int32_t true_labels; /* 0: reference behaviour (label is always 0, ref centernet_target.py:434);
                          1: opt-in fix, label = class of the winning heatmap plane */
  int32_t raw_scores;  /* 0: apply the 3x3 keep mask first (decode_centernet_predictions calls _nms, ref :352);
                          1: rank `heat` as given (the reference's bare _topk, ref :424-452) */
  float thresh, voxel, x_min, y_min;
} bevf_decode_desc;
size_t bevf_centernet_decode_work_bytes(int B, int C, int H, int W, int K);
int bevf_centernet_decode_f32(const bevf_decode_desc* d, void* stream);
/* The same decode with IoU-aware score rectification (same descriptor, launches and work buffer; raw_scores must be 0): a cell
 * of class c that survives the 3x3 keep mask is scored s^(1 - alpha[c]) * q^alpha[c], q = clamp((iou + 1) / 2, 0, 1) with
 * NaN -> 0, before any top-K; alpha[c] == 0 leaves s bit for bit.  iou: (B,1,H,W) device map, alpha: [C] device floats in
 * [0, 1] (the caller checks the range).  scores / count / order are those of the rectified score.                          */
int bevf_centernet_decode_rectify_f32(const bevf_decode_desc* d, const float* iou, const float* alpha, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training targets, ref src/centernet_target.py:170-324 (+ gaussian_radius :128-150, gaussian_2d :118-125,
 * draw_gaussian :152-168): one workgroup per frame.  boxes are float32 [B][nmax][9] (x,y,z,w,l,h,yaw,vx,vy;
 * the last two ignored unless has_vel[b]), labels int32 (-1 or >= C skips the object, like the padding of
 * ref src/train_detect.py).  Grid index / radius arithmetic is fp32 in the reference's own operation order
 * (bit-exact ind / mask / reg_mask); the gaussian is float64 rounded to fp32; dense maps keep the LAST object
 * of a cell, as the reference's sequential writes do.  All outputs must be zero-filled by the caller.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* boxes;
  const int32_t* labels;
  const int32_t* has_vel;        /* [B] */
  float* heatmap;                /* (B,C,H,W) */
  float* offset; float* size; float* rot; float* vel;      /* (B,2|3|2|2,H,W) */
  uint8_t* mask; int64_t* ind; uint8_t* reg_mask;          /* [B][max_objects] */
  float* target_offset; float* target_size; float* target_rot; float* target_vel;   /* [B][max_objects][2|3|2|2] */
  int32_t* owner_scratch;        /* [B][H*W] int32, zero-filled */
  int32_t B, nmax, H, W, C, max_objects, min_radius;
  float pc_range[6];
  float gaussian_overlap;
} bevf_targets_desc;
int bevf_centernet_targets_f32(const bevf_targets_desc* d, void* stream);

/* _nms of ref src/centernet_target.py:416-421: out = heat * (maxpool3x3(heat) == heat), planes = B*C.  */
int bevf_nms_keep_f32(const float* heat, float* out, int planes, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Box-to-box geometry of the decode path (no counterpart in the reference: its YAML's nms_threshold is unread and
 * its only IoU, inference.py _compute_iou_3d, is axis-aligned).
 *
 * Box convention, the one the decode and the reference's drawing code imply: a box [x, y, z, w, l, h, yaw] is the
 * rectangle centred at (x, y) with extent l ALONG the heading (cos yaw, sin yaw) and w ACROSS it; its z-extent is
 * [z - h/2, z + h/2].  The reference's axis-aligned formula (w along x, l along y) therefore coincides with the rotated
 * one at yaw = pi/2, not at yaw = 0.
 *
 * All entry points take padded per-frame sets [B][N][7] and int32 count[B] (NULL = every frame holds N boxes; values
 * are clamped to [0, N]).  Deterministic (two runs are bit-equal), no atomics, no allocation, no host synchronisation.
 *
 * bevf_boxes_iou_f32: out[B][N][M] = IoU of a[b][i] with b[b][j].  mode BEVF_IOU_BEV: area of the intersection of the two
 * rotated rectangles / (area_a + area_b - inter); BEVF_IOU_3D: that intersection times the z-overlap / (vol_a + vol_b -
 * inter_vol).  Box b is moved into box a's frame before any other arithmetic.  A box with w <= 0 or l <= 0 (for 3D also
 * h <= 0) has IoU 0 with everything; every value is finite and in [0, 1] (NaN / inf inputs give 0); entries with
 * i >= count_a[b] or j >= count_b[b] are 0.
 *
 * bevf_nms_boxes_f32: greedy NMS per frame over boxes already in descending score order: box i is kept iff no kept box
 * j < i suppresses it.  BEVF_NMS_ROTATE: suppress when IoU_bev(i, j) > thresh; BEVF_NMS_CIRCLE: when the squared centre
 * distance < thresh^2 (thresh = the radius in metres).  class_aware: only a box with the same label suppresses.  N <= 4096.
 * Outputs, compacted in input order and truncated to post_max: keep_idx [B][N] (indices into the frame, -1 padded),
 * keep_count [B], and -- each optional, NULL to skip -- the gathered boxes [B][N][7], scores [B][N], labels [B][N],
 * velocities [B][N][2], zero padded.  scores / velocities are only gathered; labels are also read when class_aware.
 * work: bevf_nms_boxes_work_bytes(B, N) bytes, 8-byte aligned (the [B][N][ceil(N/64)] suppression mask).
 * ------------------------------------------------------------------------------------------ */
#define BEVF_IOU_BEV 0
#define BEVF_IOU_3D 1
#define BEVF_NMS_ROTATE 0
#define BEVF_NMS_CIRCLE 1
int bevf_boxes_iou_f32(const float* a, const int32_t* count_a, const float* b, const int32_t* count_b, float* out,
                       int B, int N, int M, int mode, void* stream);
size_t bevf_nms_boxes_work_bytes(int B, int N);
int bevf_nms_boxes_f32(const float* boxes, const float* scores, const int64_t* labels, const float* velocities,
                       const int32_t* count, int B, int N, int mode, float thresh, int class_aware, int post_max,
                       void* work, int32_t* keep_idx, int32_t* keep_count, float* out_boxes, float* out_scores,
                       int64_t* out_labels, float* out_velocities, void* stream);

/* CenterNetLoss.forward, ref src/centernet_target.py:476-622: penalty-reduced focal loss on
 * clamp(sigmoid(pred)) -- the reference applies sigmoid to the already-sigmoided head output and so does
 * this -- and mask-weighted gather-L1 for offset/size/rot/vel.  out[6] = total, heatmap, offset, size, rot,
 * vel.  Two launches (fixed-grid partial sums, then a fixed-order final sum): deterministic.            */
typedef struct {
  const float* pred_heatmap;     /* (B,C,H,W) */
  const float* tgt_heatmap;
  const float* pred_reg[4];      /* offset,size,rot,vel (B,c,H,W) */
  const float* tgt_reg[4];       /* target_offset,... [B][K][c] */
  const int64_t* ind;            /* [B][K] */
  const uint8_t* reg_mask;       /* [B][K] */
  float* work;                   /* bevf_centernet_loss_work_floats() floats */
  float* out;                    /* [6] */
  int32_t B, C, H, W, K;
  float weights[5];              /* heatmap, offset, size, rot, vel */
} bevf_loss_desc;
size_t bevf_centernet_loss_work_floats(void);
int bevf_centernet_loss_f32(const bevf_loss_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * IoU-aware head, training side (no counterpart in the reference; CenterPoint's IoU-aware variant).  For every object
 * (b, k) with reg_mask set, at the cell ind = cy * W + cx, on cells of vx = (x_max - x_min) / W by vy = (y_max - y_min) / H:
 *   predicted box: x = (cx + offset[0]) * vx + x_min, y likewise, w = size[0], l = size[1], yaw = atan2f(rot[0], rot[1]);
 *   GT box: the same from target_offset / target_size / target_rot;
 *   t = 2 * IoU_bev(pred, gt) - 1 (the rotated IoU of bevf_boxes_iou_f32 on the raw sizes: w <= 0 or l <= 0 gives IoU 0).
 * bevf_iou_targets_f32: out[B][K] = t where reg_mask is set, else 0.
 * bevf_iou_aware_loss_f32: out[3] = (w_iou * iou_loss + w_diou * diou_loss, iou_loss, diou_loss) with
 *   iou_loss  = sum |iou_map[b][cell] - t| / (sum reg_mask + 1e-4)            (t is a constant),
 *   diou_loss = sum (1 - d) / (sum reg_mask + 1e-4), d = inter / (union + 1e-6) - rho^2 / (c^2 + 1e-6) of the GT rectangle
 *   and the predicted one taken parallel to it, both in the GT box's frame ((sin, cos) = target_rot), the predicted sizes
 *   clamped below at 1e-3; rho = centre distance, c = diagonal of the smallest enclosing rectangle.
 *   work: bevf_iou_aware_loss_work_floats(B) floats.
 * bevf_iou_aware_loss_bwd_f32: d out[0] / d (iou map, offset, size) stored at the objects' cells of the zero-filled maps
 *   d_iou (B,1,H,W), d_offset (B,2,H,W), d_size (B,3,H,W; channel 2 stays 0); nothing flows to rot.  K <= 2048.
 * No float atomics: objects that share a cell are summed in ascending k, the loss sums in a fixed order -- two runs are
 * bit-equal.  Objects whose ind lies outside [0, H*W) are skipped.  Nothing is read back; graph-capturable.
 * ------------------------------------------------------------------------------------------ */
int bevf_iou_targets_f32(const float* offset, const float* size, const float* rot, const float* target_offset,
                         const float* target_size, const float* target_rot, const int64_t* ind, const uint8_t* reg_mask,
                         float* out, int B, int K, int H, int W, float x_min, float y_min, float x_max, float y_max,
                         void* stream);
size_t bevf_iou_aware_loss_work_floats(int B);
int bevf_iou_aware_loss_f32(const float* iou, const float* offset, const float* size, const float* rot,
                            const float* target_offset, const float* target_size, const float* target_rot,
                            const int64_t* ind, const uint8_t* reg_mask, float* work, float* out, int B, int K, int H, int W,
                            float x_min, float y_min, float x_max, float y_max, float w_iou, float w_diou, void* stream);
int bevf_iou_aware_loss_bwd_f32(const float* iou, const float* offset, const float* size, const float* rot,
                                const float* target_offset, const float* target_size, const float* target_rot,
                                const int64_t* ind, const uint8_t* reg_mask, float* d_iou, float* d_offset, float* d_size,
                                int B, int K, int H, int W, float x_min, float y_min, float x_max, float y_max, float w_iou,
                                float w_diou, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hard voxelisation: points -> the (voxel_features, voxel_coords) layout of
 * VFELayer / VoxelNetLiDAREncoder (ref src/encoders.py:313-321, :385-387).  The reference contains no voxel
 * assignment, so the semantics are the usual deterministic ones: cell = floor((p - range_min) / voxel_size)
 * in fp32, out-of-grid points dropped, voxels numbered by first point, first max_points points per voxel in
 * input order, zero padding.  Outputs must be zero-filled by the caller.  voxel_coords are (z, y, x) = the
 * (D, H, W) index order of ref :399-410.  Grid dims = round((max - min) / voxel_size), and the grid must be a whole
 * number of voxels: an axis whose fp32 ratio (max - min) / voxel_size lies further than 0.01 from an integer is refused
 * (BEVF_ERR_ARG, the message names the axis) -- there is no agreed rounding for half a voxel, and a voxel size derived
 * as range / cells in fp32 is an integer ratio to a few ulps.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* points;       /* [B][N][C], x y z first */
  float* voxel_features;     /* [B][max_voxels][max_points][C] */
  int64_t* voxel_coords;     /* [B][max_voxels][3] */
  int32_t* num_points;       /* [B][max_voxels] */
  int32_t* num_voxels;       /* [B] */
  void* work;                /* bevf_voxelize_work_bytes(B, N) bytes */
  int32_t B, N, C, max_points, max_voxels;
  float pc_range[6];
  float voxel_size[3];
} bevf_voxelize_desc;
size_t bevf_voxelize_work_bytes(int B, int N);
int bevf_voxelize_f32(const bevf_voxelize_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * PointPillars front end (csrc/pillars.hip): the opt-in LiDAR branch `model.lidar_encoder.type: PointPillars`.  The
 * reference has no line for it (its voxel path never runs): the semantics are the standard PointPillars
 * ones, held against the fp64 restatement of tests/pillar_ref.py.  Input = bevf_voxelize_f32's outputs on a grid of ONE
 * pillar per BEV cell; only rows < num_points of pillars < num_voxels are read (those outputs need no zero fill).
 * Decorated point (K = C + 5 <= 16 channels): [x, y, z, r, extra..., x - x_mean, y - y_mean, z - z_mean, x - x_c, y - y_c],
 * means over the pillar's kept points, (x_c, y_c) = (x0, y0) + (index + 0.5) * (vx, vy); padding rows are all-zero.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* voxel_features;   /* [B][Nv][P][C] */
  const int64_t* voxel_coords;   /* [B][Nv][3] (z, y, x): y = canvas row, x = canvas column */
  const int32_t* num_points;     /* [B][Nv] */
  const int32_t* num_voxels;     /* [B] */
  int32_t B, Nv, P, C, H, W;     /* 3 <= C <= 11, 0 < P <= 255 */
  float x0, y0, vx, vy;          /* grid origin and pillar size */
} bevf_pillar_geom;
/* fp64 partials of the two reduction kernels below: bytes for a work buffer (Cout <= 128).                           */
size_t bevf_pillar_work_bytes(int Cout);
/* canvas[b][y][x][c] = max over the P rows of pillar (b, v) of relu((f . w[c]) * scale[c] + shift[c]) at the pillar's
 * cell, exactly 0 at every other cell (stream-ordered memset inside).  w: [Cout][C + 5], Cout % 32 == 0, <= 128.
 * canvas fp32, or bf16 (round to nearest even) when canvas_bf16.  argmax (optional): [B][Nv][Cout] uint8, the first
 * row reaching the maximum (padding rows count as one row at index num_points).  No atomics: bit-reproducible.       */
int bevf_pillar_pfn_f32(const bevf_pillar_geom* g, const float* w, const float* scale, const float* shift, int Cout,
                        void* canvas, int canvas_bf16, uint8_t* argmax, void* stream);
/* Train-mode BatchNorm statistics of the pre-BN activations x = f . w[c] + bias[c] over all P rows of every occupied
 * pillar (P * sum(num_voxels) rows; the empty slots up to Nv stay out): sum f and sum f f^T in fp64 (per-workgroup
 * partials, one finishing pass), mean_c = w_c . mu + b_c, var_c = w_c^T Cov w_c.  Writes moments [16 + 256] doubles
 * (mu, then Cov as [16][16]), mean / invstd (biased variance + eps) and the forward's scale = gamma * invstd,
 * shift = beta + (bias - mean) * scale.  running_mean / running_var (optional) move as torch's do: momentum, unbiased
 * variance; momentum < 0 = cumulative average over num_batches_tracked, which is incremented.  gamma / beta / bias may
 * be null (1 / 0 / 0).                                                                                               */
int bevf_pillar_moments_f32(const bevf_pillar_geom* g, const float* w, const float* bias, const float* gamma, const float* beta,
                            int Cout, float eps, float momentum, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, double* moments, float* mean, float* invstd, float* scale,
                            float* shift, void* work, void* stream);
/* Parameter gradients of the PFN from the canvas gradient dcanvas [B][H][W][Cout] (fp32): each (pillar, channel) passes
 * its cell's gradient to its argmax row through the ReLU, giving sum dy, sum dy x_hat and A = sum dy f; then
 *   dw[c] = gamma invstd (A - sum(dy) mu - sum(dy x_hat) invstd Cov w[c]),  db = sum of the BatchNorm data gradient,
 *   dgamma = sum dy x_hat,  dbeta = sum dy
 * (frozen != 0: mean / invstd are the running statistics, dw = gamma invstd A, db = gamma invstd sum dy, moments unused).
 * scale / shift / mean / invstd as the forward used them.  Two-stage fp64 partials, no atomics.                       */
int bevf_pillar_pfn_backward_f32(const bevf_pillar_geom* g, const float* dcanvas, const uint8_t* argmax, const float* w,
                                 const float* bias, const float* scale, const float* shift, const float* mean,
                                 const float* invstd, const float* gamma, const double* moments, int Cout, int frozen,
                                 float* dw, float* db, float* dgamma, float* dbeta, void* work, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sparse-voxel LiDAR encoder (csrc/sparse_index.hip, sparse_conv.hip, sparse_rows.hip): the opt-in LiDAR branch
 * `model.lidar_encoder.type: SparseVoxel`.  The reference has no line for it: spconv's semantics, held
 * against the fp64 restatement of tests/sparse_ref.py.  A level is `cap` row slots per frame: row r = b * cap + v is active
 * iff v < count[b].  The counts stay on the device: grids are sized by capacity, threads past the count return, inactive
 * slots are neither read nor written.  No atomics anywhere: every entry point is bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
/* Level 0 from bevf_voxelize_f32's voxel_coords [B][cap][3] (z, y, x) / num_voxels: index [B][D][H][W] = the row of each cell
 * or -1 (memset inside), cell [B][cap] = (z * H + y) * W + x of each active row.  B * D * H * W must fit int32.          */
int bevf_sparse_fill_index(const int64_t* coords, const int32_t* count, int B, int cap, int D, int H, int W, int32_t* index,
                           int32_t* cell, void* stream);
/* The active set of a 3x3x3 / stride 2 / pad 1 layer: output cell o of (D/2, H/2, W/2) is active iff some active input i has
 * 2o-1 <= i <= 2o+1 on every axis.  Rows in raster (z, y, x) order within a frame (mark, fixed-order scan, emit); writes
 * index_out [B][D/2][H/2][W/2], cell_out [B][cap_out], count_out [B] (clamped to cap_out; cap_out >= min(8 cap_in, cells)
 * never truncates).  work: bevf_sparse_down_work_bytes(B, D, H, W) bytes.                                               */
size_t bevf_sparse_down_work_bytes(int B, int D, int H, int W);
int bevf_sparse_down(const int32_t* index_in, int B, int D, int H, int W, int cap_out, int32_t* index_out, int32_t* cell_out,
                     int32_t* count_out, void* work, void* stream);
/* Neighbour table [B * cap][27] (tap k = (kz * 3 + ky) * 3 + kx; -1 = absent) of the rows whose cells (in the grid Dr, Hr, Wr)
 * are `cell`, looking into `index` [B][Di][Hi][Wi]: forward, in = out * stride - 1 + k; transposed (the data gradient of a
 * strided layer: the rows are the layer's inputs, index its output volume), out = (in + 1 - k) / stride when that divides. */
int bevf_sparse_table(const int32_t* index, const int32_t* cell, const int32_t* count, int B, int cap, int Di, int Hi, int Wi,
                      int Dr, int Hr, int Wr, int stride, int transposed, int32_t* table, void* stream);
/* Mean VFE: rows[b * Nv + v][c] = mean over the voxel's kept points (fp32 sum in point order, one division) for c < C, 0 for
 * C <= c < Cpad (the conv kernel's 32-channel K granule).  Inputs are bevf_voxelize_f32's outputs.                       */
int bevf_sparse_vfe_mean_f32(const float* feats, const int32_t* num_points, const int32_t* num_voxels, int B, int Nv, int P,
                             int C, int Cpad, float* rows, void* stream);
/* y[r] = sum over taps k of x[table[r][k]] . w[k] on v_mfma_f32_32x32x2_f32 (exact fp32), then y * scale + shift (either may
 * be NULL = 1 / 0) and ReLU when relu.  x [rows_in][Cin], w [27][Cin][Cout], y [B * cap][Cout]; Cin, Cout multiples of 32
 * up to 128.  The data gradient is this entry point on dy, the input-side table and weights packed [27][Cout][Cin].
 * bevf_sparse_conv_row_tile(): output rows per workgroup.                                                               */
int bevf_sparse_conv_f32(const float* x, const int32_t* table, const int32_t* count, const float* w, const float* scale,
                         const float* shift, int B, int cap, int rows_in, int Cin, int Cout, int relu, float* y, void* stream);
int bevf_sparse_conv_row_tile(void);
/* dw [Cout][cin_real][3][3][3] (torch's Conv3d layout; channels >= cin_real of x are padding) = sum over the active rows of
 * x[table[r][k]]^T dy[r]: per-chunk fp32 partials, one fixed-order sum.  work: bevf_sparse_wgrad_work_floats(Cin, Cout).  */
size_t bevf_sparse_wgrad_work_floats(int Cin, int Cout);
int bevf_sparse_conv_wgrad_f32(const float* x, const float* dy, const int32_t* table, const int32_t* count, int B, int cap,
                               int rows_in, int Cin, int Cout, int cin_real, float* dw, float* work, void* stream);
/* canvas[b][y][x][z * C + c] = rows[r][c] at the row's cell (z, y, x) of (D, H, W), exactly 0 elsewhere (memset inside);
 * fp32, or bf16 when canvas_bf16.  The backward gathers dcanvas (fp32) into drows.                                      */
int bevf_sparse_canvas_f32(const float* rows, const int32_t* cell, const int32_t* count, int B, int cap, int D, int H, int W,
                           int C, void* canvas, int canvas_bf16, void* stream);
int bevf_sparse_canvas_bwd_f32(const float* dcanvas, const int32_t* cell, const int32_t* count, int B, int cap, int D, int H,
                               int W, int C, float* drows, void* stream);
/* BatchNorm over the active rows of y [B * cap][C].  stats: fp64 fixed-order partials -> mean, invstd (biased variance +
 * eps), the running buffers as nn.BatchNorm1d moves them (momentum < 0 = cumulative average; untouched below two rows),
 * nrows[0] = the active rows (optional).  apply: a = relu(batchnorm(y)).  backward: g = da through the recomputed ReLU mask,
 * dgamma = sum g x_hat, dbeta = sum g, dy = gamma invstd (g - mean(g) - x_hat mean(g x_hat)), or gamma invstd g when frozen
 * (mean / invstd then are the running statistics).  sums: 2 C floats of scratch.  work: bevf_sparse_bn_work_bytes(C).
 * These three take C up to 1024 (a multiple of 32; the reductions go in slabs of 128 channels, so up to 128 nothing differs from
 * a single slab): the RoI head's MLP rows run through them with cap = K.                                   */
size_t bevf_sparse_bn_work_bytes(int C);
int bevf_sparse_bn_stats_f32(const float* y, const int32_t* count, int B, int cap, int C, float eps, float momentum,
                             float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean,
                             float* invstd, int32_t* nrows, void* work, void* stream);
int bevf_sparse_bn_apply_f32(const float* y, const int32_t* count, int B, int cap, int C, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, float* a, void* stream);
int bevf_sparse_bn_backward_f32(const float* y, const float* da, const int32_t* count, int B, int cap, int C, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, int frozen, float* dy,
                                float* dgamma, float* dbeta, float* sums, void* work, void* stream);

/* Dense scatter of per-voxel features [B][Nv][C] into out [B][C][D][H][W] at voxel_coords (z,y,x) -- the pillar -> BEV
 * canvas step, ref src/encoders.py:399-410 (`feature_grid[b, :, c0, c1, c2] = features.T`, rows in order: when several
 * rows name one cell the LAST one wins; cells no row names are zero).  num_voxels [B] or NULL: with it only rows
 * v < num_voxels[b] take part (the padding rows of bevf_voxelize_f32 stay out); NULL = every row, exactly like the
 * reference.  owner: scratch of B*D*H*W int32.  Rows with coordinates outside the grid are ignored. */
int bevf_scatter_voxels_f32(const float* features, const int64_t* coords, const int32_t* num_voxels, int32_t* owner,
                            float* out, int B, int Nv, int C, int D, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Camera -> BEV projection (csrc/camera_bev.hip): the opt-in camera branch `model.bev_fusion.camera_view_transform:
 * project`.  Not in the reference (it averages the cameras and stretches the map): the lift is a fixed sparse matrix built
 * on the host from the camera rig (camera_rig.py), applied here as a CSR gather
 *     y[b][r][0:C] = sum over e in [row_ptr[r], row_ptr[r+1]) of w[e] * x[b][col[e]][0:C]
 * x: [b] at x + b * x_bs, row i at x_cs elements; y likewise (x_bs / y_bs in elements): the output may be a channel slice.
 * Entries are summed in table order in fp32 (bf16 entry: bf16 x / y, fp32 accumulation, round to nearest even on the
 * store).  A row without entries is written as zeros; every output row r < nrows is written exactly once.  No atomics:
 * bit-reproducible.  The forward runs the cell table (rows = BEV cells, col = cam*Hc*Wc + y*Wc + x), the backward the
 * transposed table (rows = camera pixels, col = cell) on the output gradient.  Needs C % (16 / element size) == 0,
 * C <= 1024 fp32 / 2048 bf16, 16-byte aligned x / y, 16-byte multiples for all strides, col[e] < the caller's column
 * count, x and y not overlapping.  col / w may be NULL when the table has no entries.
 * ------------------------------------------------------------------------------------------ */
int bevf_csr_gather_f32(const int32_t* row_ptr, const int32_t* col, const float* w, int nrows, const float* x,
                        size_t x_bs, int x_cs, float* y, size_t y_bs, int y_cs, int B, int C, void* stream);
int bevf_csr_gather_bf16(const int32_t* row_ptr, const int32_t* col, const float* w, int nrows, const void* x,
                         size_t x_bs, int x_cs, void* y, size_t y_bs, int y_cs, int B, int C, void* stream);

/* Per-frame camera calibration (csrc/camera_calib.hip; DESIGN.md 3.2d "Per-frame calibration"): the table of
 * camera_rig.build_projection_table built on the device, one CSR table per frame, with no host synchronisation and no
 * allocation (capture-safe).
 *
 * bevf_camera_table_build_f64.  calib [B][ncam][4][4] fp64 (camera_rig.calib_matrices): rows 0-2 = K . E[0:3], row 3 = E[2]
 * with E = cam_to_bev^-1.  Grid: x0, y0, vx, vy = encoders.pillar_grid's fp32 values, bev_h x bev_w cells, num_heights
 * centres over the fp32 z range [z0, z1]; the images are img_h x img_w, the feature maps Hc x Wc.  Sample (cell, height k,
 * camera c) is valid when its depth > min_depth and its pixel lies in [0, img_w) x [0, img_h); taps, weights and the mean
 * over the valid samples exactly as build_projection_table's docstring states.  The geometry runs in fp64; the duplicate
 * (cell, pixel) entries of a cell are merged in fp64, exact zeros dropped, and the weight rounded to fp32 once.
 * Output, per frame b: row_ptr [B][P + 1] (P = bev_h * bev_w; offsets within the frame), and the frame's entries at
 * col / w [b * cap ...], sorted by pixel inside a row (the host table's order); cap >= P * num_heights * ncam * 4 entries
 * (the worst case), only the used part is written.  work: B * cap * 8 bytes + B * P int32.  Needs num_heights * ncam <= 682.
 * Deterministic: two builds give the same bits.
 *
 * bevf_camera_table_transpose.  The same (cell, pixel, w) entries as CSR by pixel, per frame: t_row_ptr [B][ncols + 1],
 * t_col (= cell) / t_w at [b * cap ...], every row in ascending cell order (ties in the forward table's order), weights
 * bit-equal.  Integer atomics count the rows and hand out cursor positions; each row is then rank-sorted by forward entry
 * index, so the order does not depend on them.  work: B * cap * 8 bytes + B * ncols int32 (may be the build's).
 *
 * bevf_csr_gather_frames_{f32,bf16}.  bevf_csr_gather with a table per frame: frame b reads row_ptr + b * rp_stride
 * (rp_stride >= nrows + 1) and col / w + b * e_stride.  Same strides, slice output, zero rows, fp32 accumulation in table
 * order, no atomics, every output row written once; B <= 65535. */
int bevf_camera_table_build_f64(const double* calib, int B, int ncam, float x0, float y0, float vx, float vy, int bev_h,
                                int bev_w, float z0, float z1, int num_heights, double min_depth, int img_h, int img_w,
                                int Hc, int Wc, int32_t* row_ptr, int32_t* col, float* w, size_t cap, void* work,
                                void* stream);
int bevf_camera_table_transpose(const int32_t* row_ptr, const int32_t* col, const float* w, size_t cap, int B, int P,
                                int ncols, int32_t* t_row_ptr, int32_t* t_col, float* t_w, void* work, void* stream);
int bevf_csr_gather_frames_f32(const int32_t* row_ptr, size_t rp_stride, const int32_t* col, const float* w,
                               size_t e_stride, int nrows, const float* x, size_t x_bs, int x_cs, float* y, size_t y_bs,
                               int y_cs, int B, int C, void* stream);
int bevf_csr_gather_frames_bf16(const int32_t* row_ptr, size_t rp_stride, const int32_t* col, const float* w,
                                size_t e_stride, int nrows, const void* x, size_t x_bs, int x_cs, void* y, size_t y_bs,
                                int y_cs, int B, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Learned-depth camera -> BEV lift (csrc/camera_lift.hip): the opt-in camera branch `model.bev_fusion.camera_view_transform:
 * lift`.  None of these has a counterpart in the reference (it has no view transform at all).  fp32 only,
 * stream-ordered, capture-safe (nothing allocated), no atomics, every output element written exactly once, two launches
 * give the same bits.  D = depth bins, 1 <= D <= 64.
 *
 * bevf_softmax_rows_f32.  y[r][0:D] (row stride y_rs) = softmax of x[r][0:D] (row stride x_rs) for r < nrows: row maximum
 * subtracted, expf, the sum by a fixed butterfly over the row's lanes, one division per element.  No reference counterpart.
 *
 * bevf_softmax_rows_bwd_f32.  dx[r][d] (row stride x_rs) = pd[r][d] * (dpd[r][d] - sum_d pd[r][d] * dpd[r][d]) for d < D and
 * 0 for D <= d < x_cols (x_cols <= 64: the padding columns of a logit buffer wider than D); pd / dpd rows at stride p_rs.
 * No reference counterpart.
 *
 * bevf_csr_lift_f32.  y[b][r][0:C] = sum over e in [row_ptr[r], row_ptr[r+1]) of w[e] * pd[b][col2[e]] * x[b][col2[e] / D][0:C]
 * -- bevf_csr_gather_f32 with a per-frame scalar per entry: col2 = pixel * D + bin (camera_rig.build_lift_table), pd [b] at
 * pd + b * pd_bs holds the depth distribution [pixel][D] densely.  Same strides, slice output, zero rows, fp32 accumulation in
 * table order as bevf_csr_gather_f32; with D = 1 and pd == 1 the same bits.  Needs C % 4 == 0, C <= 1024, 16-byte aligned
 * x / y and 16-byte multiples for their strides, col2[e] < pixels * D.  No reference counterpart.
 *
 * bevf_csr_lift_bwd_f32.  The transposed table, CSR by pixel with (t_cell, t_bin, t_w) per entry, one wave per (pixel, frame):
 *     dx [b][pix][0:C] = sum_e t_w[e] * pd[b][pix][t_bin[e]] * dy[b][t_cell[e]][0:C]
 *     dpd[b][pix][d]   = sum over e with t_bin[e] == d of t_w[e] * <x[b][pix][0:C], dy[b][t_cell[e]][0:C]>
 * in table order; the dot product is reduced over the wave by a fixed butterfly.  Bins and pixels without an entry get
 * zeros.  dpd [b] at dpd + b * dpd_bs, dense [pixel][D] like pd.  B <= 65535; t_cell / t_bin / t_w may be NULL when the table
 * has no entries.  No reference counterpart.
 * ------------------------------------------------------------------------------------------ */
int bevf_softmax_rows_f32(const float* x, int x_rs, float* y, int y_rs, size_t nrows, int D, void* stream);
int bevf_softmax_rows_bwd_f32(const float* pd, const float* dpd, int p_rs, float* dx, int x_rs, int x_cols, size_t nrows,
                              int D, void* stream);
int bevf_csr_lift_f32(const int32_t* row_ptr, const int32_t* col2, const float* w, int nrows, int D, const float* x,
                      size_t x_bs, int x_cs, const float* pd, size_t pd_bs, float* y, size_t y_bs, int y_cs, int B, int C,
                      void* stream);
int bevf_csr_lift_bwd_f32(const int32_t* t_row_ptr, const int32_t* t_cell, const int32_t* t_bin, const float* t_w, int npix,
                          int D, const float* x, size_t x_bs, int x_cs, const float* pd, size_t pd_bs, const float* dy,
                          size_t dy_bs, int dy_cs, float* dx, size_t dx_bs, int dx_cs, float* dpd, size_t dpd_bs, int B,
                          int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Lift-splat camera -> BEV view transform (csrc/camera_frustum.hip): the opt-in camera branch
 * `model.bev_fusion.camera_view_transform: frustum` (Philion & Fidler 2020, BEVFusion's bev_pool).  None of
 * these has a counterpart in the reference (it has no view transform at all).  fp32 features, fp64 geometry, stream-ordered,
 * capture-safe (nothing allocated, no host synchronisation), every output element written exactly once, two launches give
 * the same bits.  D = depth bins, 1 <= D <= 64; ncols = ncam * Hc * Wc feature pixels, pix = cam * Hc * Wc + y * Wc + x,
 * col2 = pix * D + d; P = bev_h * bev_w cells, cell = i * bev_w + j.
 *
 * bevf_frustum_table_build_f64.  calib [B][ncam][4][4] fp64 as camera_rig.calib_matrices / augment.augmented_calib make it:
 * rows 0-2 = [A | t], row 3 the depth row.  THE THIRD ROW MUST EQUAL THE DEPTH ROW (both producers keep it so: the last row
 * of K and of every image map is (0, 0, 1)); the entry point relies on it and does not read row 3.  Feature pixel (x, y)
 * sits at the image point u = (x + 1/2) img_w / Wc - 1/2, v = (y + 1/2) img_h / Hc - 1/2; bin d has the centre depth
 * z_d = depth_min + (d + 1/2) (depth_max - depth_min) / D; the frustum point is p = A^-1 (z_d (u, v, 1)^T - t), with A^-1
 * taken once per (frame, camera); j = floor((p_x - x0) / vx), i = floor((p_y - y0) / vy) with x0, y0, vx, vy =
 * encoders.pillar_grid's fp32 values; the point is valid when 0 <= j < bev_w, 0 <= i < bev_h and z0 <= p_z < z1.  Output, per
 * frame b: cell_of [B][ncols * D] (the cell of col2, -1 when invalid); row_ptr [B][P + 1] (offsets within the frame) and the
 * frame's entries at col2 [b * ncols * D ...], EVERY ROW IN ASCENDING col2; the capacity per frame is exactly ncols * D and
 * there are no weights (each is 1).  Integer atomics count the rows and hand out cursor positions; every row is then sorted
 * from LDS -- one wave per row up to bevf_frustum_table_sort_wave_rows() entries, the whole workgroup streaming the row
 * through LDS beyond (time grows with the square of the row length) -- so the order does not depend on them.  work:
 * bevf_frustum_table_work_elems(...) int32 elements, 8-byte aligned.  No reference counterpart.
 *
 * bevf_frustum_pool_f32.  y[b][r][0:C] = sum over e in [row_ptr[b][r], row_ptr[b][r+1]) of pd[b][col2[b][e]] *
 * x[b][col2[b][e] / D][0:C]: one wave per (cell, frame), fp32 accumulation in table order, several entries in flight.
 * Frame b reads row_ptr + b * rp_stride and col2 + b * e_stride; BOTH STRIDES MAY BE 0: one table shared by all frames (the
 * static rig).  pd [b] at pd + b * pd_bs holds [pixel][D] densely.  Same strides, slice output and zero rows as
 * bevf_csr_gather_f32.  Needs C % 4 == 0, C <= 1024, B <= 65535, 16-byte aligned x / y and 16-byte multiples for their strides,
 * col2 < pixels * D.  No reference counterpart.
 *
 * bevf_frustum_pool_bwd_f32.  Dense, no transposed table: one wave per (pixel, frame) keeps x[b][pix] and walks the pixel's D
 * bins through cell_of (frame b at cell_of + b * c_stride, c_stride may be 0):
 *     dpd[b][pix][d]  = <x[b][pix][0:C], dy[b][cell][0:C]> for a valid bin (reduced over the wave by bevf_csr_lift_bwd_f32's
 *                       fixed butterfly), exactly 0 for an invalid one
 *     dx[b][pix][0:C] = sum over the valid d, ascending, of pd[b][pix][d] * dy[b][cell][0:C]
 * Both written once for every pixel.  cell_of < the rows of dy.  No reference counterpart.
 * ------------------------------------------------------------------------------------------ */
int bevf_frustum_table_sort_wave_rows(void);
size_t bevf_frustum_table_work_elems(int B, int ncam, int bev_h, int bev_w, int D, int Hc, int Wc);
int bevf_frustum_table_build_f64(const double* calib, int B, int ncam, float x0, float y0, float vx, float vy, int bev_h,
                                 int bev_w, float z0, float z1, int D, double depth_min, double depth_max, int img_h,
                                 int img_w, int Hc, int Wc, int32_t* cell_of, int32_t* row_ptr, int32_t* col2, void* work,
                                 void* stream);
int bevf_frustum_pool_f32(const int32_t* row_ptr, size_t rp_stride, const int32_t* col2, size_t e_stride, int nrows, int D,
                          const float* x, size_t x_bs, int x_cs, const float* pd, size_t pd_bs, float* y, size_t y_bs,
                          int y_cs, int B, int C, void* stream);
int bevf_frustum_pool_bwd_f32(const int32_t* cell_of, size_t c_stride, int npix, int D, const float* x, size_t x_bs, int x_cs,
                              const float* pd, size_t pd_bs, const float* dy, size_t dy_bs, int dy_cs, float* dx,
                              size_t dx_bs, int dx_cs, float* dpd, size_t dpd_bs, int B, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * LiDAR depth supervision of the 'frustum' and 'lift' camera branches (csrc/depth_sup.hip; BEVDepth, Li et al.
 * 2022): opt-in through the detector's `depth_points=` argument and depth_supervision.py.  None of these has a counterpart in
 * the reference.  fp64 geometry, fp32 logits, stream-ordered, capture-safe (nothing allocated, no host synchronisation), no
 * floating-point atomics, two launches give the same bits.  D = depth bins, 1 <= D <= 64.
 *
 * bevf_depth_targets_f64.  points: B frames of N rows, frame b at points + b * p_bs, row p at + p * p_stride floats, columns
 * 0-2 = (x, y, z) in the frame the calibration maps from; counts [B] = valid rows per frame or NULL (= N).  calib as
 * bevf_frustum_table_build_f64 takes it, frame b at calib + b * calib_bs doubles; calib_bs == 0: one calibration for all frames
 * (the static rig).  Rows 0-2 only are read; ROW 2 MUST EQUAL THE DEPTH ROW.  For frame b, camera c and point p = (x, y, z, 1):
 *     q = calib[b][c][0:3] . p,   zc = q_2,   u = q_0 / zc,   v = q_1 / zc
 *     X = floor((u + 1/2) Wc / img_w),   Y = floor((v + 1/2) Hc / img_h)      (the inverse of u = (x + 1/2) img_w / Wc - 1/2)
 *     d = min(floor((zc - depth_min) D / (depth_max - depth_min)), D - 1)     (camera_rig.depth_bin_of)
 * The point counts for camera c when depth_min <= zc < depth_max, 0 <= X < Wc and 0 <= Y < Hc.  A row whose x, y, z are all
 * exactly 0 is padding, and so is a row at or past counts[b]: padding never counts.  target [B][ncam][Hc][Wc] int32 = the
 * smallest d among the pixel's points (the nearest return), -1 for a pixel with none: filled with 0xFFFFFFFF in the stream,
 * then one thread per (point, camera, frame) and an integer atomicMin on the unsigned bin, which no order can change.
 * B <= 65535, ncam <= 65535.  No reference counterpart.
 *
 * bevf_depth_ce_f32.  logits: nrows rows of D floats at row stride l_rs (columns >= D are never read); target [nrows] as above
 * (< 0: not supervised, else < D).  Row r with target t >= 0 contributes logsumexp(logits[r][0:D]) - logits[r][t], computed
 * from the logits with the row maximum subtracted (one lane per bin, bevf_softmax_rows_f32's butterfly).  Workgroups write
 * (sum, count) pairs in fp64 to partials (bevf_depth_ce_work_doubles() doubles, 8-byte aligned) in a fixed order and a second,
 * single-wave launch adds them in fp64: out[0] = sum / max(count, 1), out[1] = count (exact as a float: nrows <= 2^24 is
 * required).  With no supervised row out = (0, 0) exactly.  No reference counterpart.
 *
 * bevf_depth_ce_bwd_f32.  pd: the softmax of the logits, rows at stride p_rs; g: the gradient arriving at out[0], ONE FLOAT ON
 * THE DEVICE; out: what bevf_depth_ce_f32 wrote.  For a row with a target
 *     dlogit[r][d] += g[0] / max(out[1], 1) * (pd[r][d] - [d == target[r]])     for d < D     (rows at stride x_rs)
 * Rows without a target and columns >= D are not touched; every touched element is read and written once.  No reference
 * counterpart.
 * ------------------------------------------------------------------------------------------ */
size_t bevf_depth_ce_work_doubles(void);
int bevf_depth_targets_f64(const float* points, size_t p_bs, int p_stride, int N, const int32_t* counts, const double* calib,
                           size_t calib_bs, int B, int ncam, int Hc, int Wc, int D, double depth_min, double depth_max,
                           int img_h, int img_w, int32_t* target, void* stream);
int bevf_depth_ce_f32(const float* logits, int l_rs, const int32_t* target, size_t nrows, int D, double* partials, float* out,
                      void* stream);
int bevf_depth_ce_bwd_f32(const float* pd, int p_rs, const int32_t* target, const float* g, const float* out, float* dlogit,
                          int x_rs, size_t nrows, int D, void* stream);

/* ==========================================================================================
 * bf16 storage, fp32 accumulate (BASELINE configs 3 and 5).  Same layouts and geometry as the fp32 entry
 * points, element type bfloat16 wherever a pointer is typed void*: the convolution runs on
 * v_mfma_f32_32x32x16_bf16 (a K step is 64 bf16 = the same 128-byte rows; needs Cin % 64 == 0), BN
 * scale/shift, biases, the small per-frame vectors (PointNet / radar features) and the head outputs stay
 * fp32.  bevf_conv2d_nhwc_bf16 takes the same descriptor with x / w / res / y pointing at bf16 data.
 * ========================================================================================== */
int bevf_conv2d_nhwc_bf16(const bevf_conv_desc* d, void* stream);

/* The 3x3 / stride 1 / pad 1 layers of the bf16 path (ResNet blocks ref src/encoders.py:158-160 via torchvision's BasicBlock,
 * camera_proj / lidar_upsample / bev_fusion ref src/fusion.py:141-207, the CenterNet 3x3 convs ref src/fusion.py:822-854) as a
 * direct convolution on v_mfma_f32_16x16x32_bf16 that stages each 18x18-pixel input patch ONCE per 32-channel chunk (LDS-DMA)
 * and reads all nine taps from it; same descriptor as bevf_conv2d_nhwc_bf16 (colmax / stats unsupported, `tile` ignored).
 * `d->w` = the filter image made by bevf_conv3x3_pack_bf16 from the OHWI bf16 filter (bevf_conv3x3_pack_elems(Cout, Cin)
 * bf16 elements).  Requires KH = KW = 3, stride 1, pad 1, Cin % 32 == 0, Cout % 64 == 0, x_cs % 8 == 0, y_cs % 4 == 0. */
size_t bevf_conv3x3_pack_elems(int Cout, int Cin);
int bevf_conv3x3_bf16_ct(int Cout);   /* output-channel tile (64 | 128) the kernel uses for this layer */
int bevf_conv3x3_pack_bf16(const void* w_ohwi, void* packed, int Cout, int Cin, void* stream);
int bevf_conv3x3_bf16(const bevf_conv_desc* d, void* stream);
/* Diagnostic only (in-kernel s_memtime stamps of the kernel above: start / operands landed / K loop done / stores acknowledged per
 * workgroup, 4 x uint64 each, into `buf` for every following launch; NULL switches it off).  Never set by the product path. */
int bevf_debug_conv3x3_stamps(void* buf);
/* The same for bevf_conv3x3_wino_f32 (plain ReLU launches): start / first patch DMA issued / first operands transformed / K loop done /
 * epilogue issued / stores acknowledged, 6 x uint64 per workgroup. */
int bevf_debug_wino_stamps(void* buf);
/* Diagnostic / tests: the plain launches of bevf_conv3x3_wino_f32 with Cin >= 64 run `n` workgroups that each walk tiles b, b + n,
 * b + 2n, ... (0 = automatic: one per compute unit); a count at or above a launch's tile count gives one tile per workgroup.  Results
 * do not depend on it.  Never set by the product path. */
int bevf_debug_wino_workgroups(int n);

/* Opt-in "f32x3" convolution: same contract as bevf_conv2d_nhwc_f32 (fp32 activations in and out, no colmax), but
 * the products run on the bf16 MFMA over an exact three-way bf16 split of both operands (six partial products,
 * fp32 accumulate): fp32-level error, not bit-identical to the fp32 FMA chain.  `w` = planes written by
 * bevf_split_weights_f32x3: [3][Cout][KH][KW][Cin] bf16 (hi, mid, lo).  tile: 0 auto, 1 / 3 / 4 as above.      */
int bevf_split_weights_f32x3(const float* w, void* planes, size_t n, void* stream);
int bevf_conv2d_nhwc_f32x3(const bevf_conv_desc* d, void* stream);
/* Bound pass of the pruned column max: the f32x3 kernel on two planes and three products (hi*hi + hi*mid + mid*hi;
 * `w` = the planes of bevf_split_weights_f32x3), which stores no y.  For row p and channel c it brackets what bevf_conv2d_nhwc_f32
 * would compute: val = fma(acc, scale[c], shift[c]), eps = |x_p| * bound_g[c] + 2^-21 |val| with |x_p| the row's Euclidean norm
 * (summed while the row is staged, inflated by 2^-10), and bound_g[c] >= rel(K) * |w_c| * |scale[c]| from the caller.  It raises
 * thr = d->colmax [ceil(M/rows_per_group)][Cout] (zeroed by the caller) to max(val - eps, 0) by atomicMax on the bit patterns.
 * seed_stride = k > 0: only row tiles 0, k, 2k, ... run and only thresholds are written (flag = NULL).  seed_stride = 0: all rows;
 * flag[p] [M] (zeroed by the caller) is set to 1 when !(val + eps < thr) and !(val + eps <= 0) for some channel, so a NaN or
 * infinite bound flags the row.  Needs relu = 1, y = res = NULL.  tile: 0 auto, 1 128x128, 4 64x64.                          */
int bevf_conv2d_bound_f32x2(const bevf_conv_desc* d, const float* bound_g, int32_t* flag, int seed_stride, void* stream);
/* Compaction for the same: flag [B][N] -> cand [B][cap][C], the flagged rows of x [B][N][C] in order, the remaining slots filled
 * with the frame's row 0 up to the next multiple of 128 (the rest of the slots is left as it is: group_rows of bevf_conv2d_nhwc_f32_if);
 * rows[b] = min(flagged rows of frame b, cap); *overflow (zeroed by the caller) is set to 1 when a frame has more than cap
 * flagged rows.  rp: work, [B][N + 1] int32.  C % 4 == 0, cap % 128 == 0.                                                    */
int bevf_prune_compact_f32(const float* x, const int32_t* flag, int32_t* rp, float* cand, int32_t* rows, int32_t* overflow, int B,
                           int N, int C, int cap, void* stream);
int bevf_stem_conv7x7_bf16out(const float* x, const float* w, const float* scale, const float* shift, void* y, int N,
                              int H, int W, int relu, void* stream);
/* bf16 stem on the bf16 MFMA (bf16-storage models): x fp32 NCHW (rounded to bf16 while it is staged), filter bank
 * bf16 [64][176] from bevf_stem_pack_bf16 (k = (c*7+kh)*8 + kw, zero columns for kw = 7 and k >= 168), fp32
 * accumulate, folded BN + ReLU, bf16 NHWC out.                                                                   */
int bevf_stem_pack_bf16(const float* w_oihw, void* packed, void* stream);
int bevf_stem_conv7x7_bf16mma(const float* x, const void* w_packed, const float* scale, const float* shift, void* y,
                              int N, int H, int W, int relu, void* stream); /* The bf16 stem and the 3x3/s2 max-pool in one kernel (bf16-storage inference): fp32 image in, pooled bf16 NHWC
 * [N][Hp][Wp][64] out, bit-identical to bevf_stem_conv7x7_bf16mma (relu = 1) followed by bevf_maxpool3x3s2_nhwc_bf16;
 * the 64-channel stem map never reaches HBM (ref src/encoders.py:154-157).                                          */
int bevf_stem_pool_bf16mma(const float* x, const void* w_packed, const float* scale, const float* shift, void* y, int N,
                           int H, int W, void* stream);
    /* fp32 image + fp32 MFMA, bf16 NHWC out */
int bevf_maxpool3x3s2_nhwc_bf16(const void* x, void* y, int N, int H, int W, int C, void* stream);
int bevf_pointwise_smallk_bf16out(const float* x, const float* w, const float* scale, const float* shift, void* y,
                                  int M, int K, int Cout, int relu, void* stream);
int bevf_linear_bf16w(const float* x, const void* w, const float* bias, void* y, int y_bf16, int B, int K, int O,
                      int relu, int perm_inner, int perm_outer, void* stream);
int bevf_cam_mean_bf16(const void* x, void* y, int B, int ncam, int P, int C, void* stream);
int bevf_bilinear_nhwc_bf16(const void* x, void* y, int B, int Hi, int Wi, int C, int x_cs, int Ho, int Wo, int y_cs,
                            void* stream);
int bevf_broadcast_nhwc_bf16(const float* v, void* y, int B, int P, int C, int y_cs, void* stream);
int bevf_expand_border_classes_bf16(const void* small, void* y, int B, int Sh, int Sw, int C, int y_cs, void* stream);
int bevf_head_tail_bf16(const bevf_head_desc* d, void* stream);          /* hid bf16, outputs fp32 NCHW */

/* ==========================================================================================
 * Training step (ref src/train_detect.py:401-434): the backward of every layer on
 * the path, train-mode BatchNorm, gradient clipping and AdamW.  Gradients accumulated with fp32 atomics
 * (conv weight gradient, bilinear / gather-L1 scatter) are not bitwise reproducible run to run.
 * ========================================================================================== */

/* Tap table for the weight gradient: tab[m][t] = byte offset of x[n][ih][iw][0] under filter tap t of output pixel
 * m (0x80000000 for padding taps and for the rows that pad M up to a multiple of 32); depends on the shape and on
 * x_cs only, so callers cache it.  bevf_conv_pixtab_bytes = size of the table.                                   */
size_t bevf_conv_pixtab_bytes(int N, int H, int W, int KH, int KW, int stride, int pad);
int bevf_conv_pixtab(int32_t* tab, int N, int H, int W, int KH, int KW, int stride, int pad, int x_cs, void* stream);

/* dW[co][kh][kw][ci] += sum_m dy[m][co] * x[pixel(m)+tap][ci]   (dw zero-filled by the caller; OHWI like the
 * forward weights; the host permutes back to the parameter's OIHW).  MFMA fp32, pixel range split over WGs. */
typedef struct {
  const float* x;          /* [N][H][W][x_cs] forward input */
  const float* dy;         /* [N*Ho*Wo][dy_cs] gradient of the raw conv output */
  float* dw;               /* [Cout][KH][KW][Cin] */
  const int32_t* pixtab;   /* bevf_conv_pixtab for this shape and x_cs */
  int32_t N, H, W, Cin, x_cs, Cout, dy_cs, KH, KW, stride, pad;
} bevf_wgrad_desc;
int bevf_conv2d_wgrad_f32(const bevf_wgrad_desc* d, void* stream);
/* The same gradient for 3x3 / stride 1 / pad 1 layers with Cin, Cout multiples of 64, in the Winograd F(2x2,3x3) domain
 * (csrc/conv_wino_wgrad.hip): 2.25x fewer MFMA FLOPs, deterministic (fixed-order sum of per-workgroup partial blocks, no
 * atomics).  `workspace`: bevf_wino_wgrad_workspace_floats() floats (0 = shape not supported: use bevf_conv2d_wgrad_f32);
 * `pixtab` of the descriptor = the per-shape tile table written by bevf_wino_wgrad_table (bevf_wino_wgrad_table_bytes()
 * bytes; depends on N, H, W and the two channel strides only, reusable across layers and steps); accumulate != 0 adds to
 * dw instead of overwriting it.  dw: [Cout][3][3][Cin]. */
size_t bevf_wino_wgrad_workspace_floats(int N, int H, int W, int Cin, int Cout);
size_t bevf_wino_wgrad_table_bytes(int N, int H, int W);
int bevf_wino_wgrad_table(int32_t* tab, int N, int H, int W, int x_cs, int dy_cs, void* stream);
int bevf_conv3x3_wgrad_wino_f32(const bevf_wgrad_desc* d, float* workspace, int accumulate, void* stream);

/* Data gradient: the forward kernel (bevf_conv2d_nhwc_f32) run on dy with the spatially flipped, channel-
 * transposed filter; strided convs first spread dy onto the input grid with zeros in between:            */
int bevf_zero_stuff_nhwc_f32(const float* dy, float* out, int N, int Ho, int Wo, int C, int H, int W, int s, void* stream);
/* Stride-2 data gradients without the zeros: the four input-parity classes are each a small stride-1 conv over dy
 * (1x1, 1x2, 2x1, 2x2 taps for a 3x3 filter); this writes dx[n][ih][iw] = cls[(ih&1)*2+(iw&1)][n][ih>>1][iw>>1]
 * (class q stored hq[q] x wq[q]; a null class is zeros, e.g. three of the four for a 1x1 stride-2 conv).          */
int bevf_interleave2x2_nhwc_f32(const float* const* cls4, const int32_t* hq4, const int32_t* wq4, float* dx, int N, int H,
                                int W, int C, void* stream);

/* Train-mode BatchNorm{1,2}d over rows [M][C] (channel stride cs): batch mean / biased variance / invstd
 * (two-stage, fixed order, shifted sums), apply (+residual)(+ReLU), and backward:
 *   dy <- dy * (y > 0) if relu;  dbeta = sum dy;  dgamma = sum dy*xhat;
 *   dx = gamma*invstd*(dy - dbeta/M - xhat*dgamma/M)   (dx == NULL: only the sums -> conv bias gradients) */
size_t bevf_bn_work_floats(int C);
/* running_mean/var <- (1-momentum)*running + momentum*batch (variance unbiased by M/(M-1)), num_batches_tracked += 1
 * (may be NULL): torch.nn.BatchNorm's training-mode buffer update in one launch.                                  */
int bevf_bn_update_running_f32(const float* mean, const float* var, float* running_mean, float* running_var,
                               int64_t* num_batches_tracked, int C, int M, float momentum, void* stream);
int bevf_bn_stats_f32(const float* x, float* work, float* mean, float* var, float* invstd, int M, int C, int cs,
                      float eps, void* stream);
/* The same statistics from partial sums a producer left behind (bevf_conv3x3_wino_f32 with `stats`): part [G][C][2] =
 * {sum(x - pivot), sum((x - pivot)^2)} over disjoint row sets covering all M rows; fixed-order merge in double. */
int bevf_bn_stats_from_partials_f32(const float* part, int G, const float* pivot, float* mean, float* var, float* invstd,
                                    int M, int C, float eps, void* stream);
int bevf_bn_apply_f32(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      const float* res, float* y, int M, int C, int cs, int relu, void* stream);
/* relu with y == NULL: the mask is recomputed from x exactly as bn_apply computed it (gamma, beta as in the forward;
 * only valid when the forward had no residual input) -- saves reading the forward output.  relu == 2: the same, and
 * dy is left untouched (relu == 1 writes the masked gradient back in place): both passes mask on the fly.
 * relu | 4: the layer normalised with FIXED statistics (an eval-mode BatchNorm inside a module that trains, mean / invstd =
 * its running buffers): dgamma / dbeta as always, dx = gamma * invstd * dy (the two mean terms vanish).               */
int bevf_bn_backward_f32(float* dy, const float* y, const float* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, float* work, float* dgamma, float* dbeta, float* dx,
                         int M, int C, int cs, int relu, void* stream);
/* The same backward when the producer of dy has already applied the ReLU mask and left the per-channel partial sums
 * (bevf_conv3x3_wino_f32 with bnb_x): part [G][C][2] = {sum dy, sum dy * xhat}.  Merges them (fixed order, double) into
 * dbeta / dgamma and writes dx = gamma * invstd * (dy - sum_dy / M - xhat * sum_dyx / M). */
int bevf_bn_backward_from_partials_f32(const float* dy, const float* x, const float* mean, const float* invstd,
                                       const float* gamma, const float* part, int G, float* dgamma, float* dbeta, float* dx,
                                       int M, int C, int cs, void* stream);
/* BatchNorm(+ReLU) backward whose dY is the backward of a 3x3/s2/p1 max-pool (the ResNet stem in training, ref
 * src/encoders.py:154-157): dpool [N][Ho][Wo][C], idx from bevf_maxpool3x3s2_idx_f32, x the raw conv output [N][H][W][C].
 * Bit-identical to bevf_maxpool3x3s2_bwd_f32 + bevf_bn_backward_f32(relu = 1, y = NULL); the dense dY never exists.       */
int bevf_pool_bn_backward_f32(const float* dpool, const uint8_t* idx, const float* x, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, float* work, float* dgamma, float* dbeta, float* dx,
                              int N, int H, int W, int C, void* stream);
/* Forward twin: y = maxpool3x3s2(relu(batchnorm(x))) with the argmax codes of bevf_maxpool3x3s2_idx_f32, the normalised map never
 * written (bit-identical to bevf_bn_apply_f32(relu = 1) followed by bevf_maxpool3x3s2_idx_f32).                                */
int bevf_bn_relu_maxpool3x3s2_idx_f32(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                      float* y, uint8_t* idx, int N, int H, int W, int C, void* stream);

/* Elementwise over n floats; both require n % 4 == 0 and 16-byte aligned buffers (callers round n up and size both
 * buffers for the rounded count).                                                                                    */
int bevf_add_inplace_f32(float* y, const float* x, size_t n, void* stream);            /* y += x            */
int bevf_relu_mask_f32(float* dy, const float* y, size_t n, void* stream);             /* dy *= (y > 0)     */
int bevf_maxpool3x3s2_idx_f32(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int bevf_maxpool3x3s2_bwd_f32(const float* dy, const uint8_t* idx, float* dx, int N, int H, int W, int C, void* stream);
int bevf_bilinear_bwd_nhwc_f32(const float* dy, float* dx, int B, int Hi, int Wi, int C, int x_cs, int Ho, int Wo,
                               int y_cs, void* stream);                                 /* dx zero-filled    */
int bevf_cam_mean_bwd_f32(const float* dy, float* dx, int B, int ncam, int P, int C, void* stream);
size_t bevf_group_max_idx_work_bytes(int G, int P, int C);
int bevf_group_max_idx_f32(const float* x, float* y, int32_t* idx, void* work, int G, int P, int C, void* stream);
int bevf_group_max_bwd_f32(const float* dy, const int32_t* idx, float* dx, int G, int P, int C, void* stream); /* dx zero-filled */
/* The sparse rows of the low-rank backward of conv -> BatchNorm -> ReLU -> max over points (ref src/encoders.py:296-299): S [G][C] = one entry
 * per (frame, channel), living at row g*P + idx[g][c] of the [G*P][K] layer input A.  out[c][k] = sum_g S[g][c] A[row(g,c)][k];
 * dA[row(g,c)][k] += S[g][c] W[c][k].  Fixed summation order, no atomics: bit-identical run to run. */
int bevf_sparse_rows_wgrad_f32(const float* S, const int32_t* idx, const float* A, float* out, int G, int P, int C, int K, void* stream);
int bevf_sparse_rows_scatter_add_f32(const float* S, const int32_t* idx, const float* W, float* dA, int G, int P, int C, int K, void* stream);
/* Same max / argmax (work: bevf_group_max_idx_work_bytes) over relu(batchnorm(x)) evaluated on the fly from the raw
 * rows x with bn_apply's own fma: the training forward of PointNet's last layer writes no activation.            */
int bevf_bn_relu_group_max_idx_f32(const float* x, const float* mean, const float* invstd, const float* gamma,
                                   const float* beta, float* y, int32_t* idx, void* work, int G, int P, int C, void* stream);
/* Backward of max-over-rows( relu( batchnorm(x) ) ) without the dense intermediate gradient (PointNet's last layer,
 * ref src/encoders.py:296-299): dg / gmax / idx [B][C] = gradient, value and argmax row of the max; writes dgamma,
 * dbeta, dx [B*P][cs]; dgm [B][C] scratch.                                                                        */
int bevf_gmax_bn_backward_f32(const float* dg, const float* gmax, const int32_t* idx, const float* x, const float* mean,
                              const float* invstd, const float* gamma, float* dgm, float* dgamma, float* dbeta, float* dx,
                              int B, int P, int C, int cs, void* stream);
/* Its first stage alone (masked dg, dgamma, dbeta), for callers that never build the dense dx (the low-rank backward of
 * PointNet's last layer in training.py).                                                                             */
int bevf_gmax_bn_sums_f32(const float* dg, const float* gmax, const int32_t* idx, const float* x, const float* mean,
                          const float* invstd, float* dgm, float* dgamma, float* dbeta, int B, int P, int C, int cs, void* stream);
size_t bevf_linear_bwd_work_floats(int B, int K, int O);
/* Backward of bevf_linear_f32: dy [B][O] in the forward's stored order, i.e. read at perm(o).  perm_inner == 0: no permutation;
 * otherwise perm_outer > 0 and perm_inner * perm_outer == O are required (only then is perm a permutation of [0, O)).
 * dx and db may be NULL; B <= 64, K % 4 == 0.  Fixed summation order: bit-identical run to run.                                 */
int bevf_linear_bwd_f32(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, float* work,
                        int B, int K, int O, int perm_inner, int perm_outer, void* stream);
typedef struct {
  const float* hid; const float* w; const float* out0;   /* out0: post-sigmoid heatmap (B,c0,H,W) */
  const float* dout[5];
  float* dhid; float* dw; float* db;                     /* dw, db zero-filled by the caller */
  int32_t B, P, hc;
  int32_t c[5];
  int32_t n_sigmoid;                                     /* leading heatmap channels behind a sigmoid: 0 <= n_sigmoid <= c[0] */
} bevf_head_bwd_desc;
int bevf_head_tail_bwd_f32(const bevf_head_bwd_desc* d, void* stream);
/* d total_loss / d predictions for CenterNetLoss (ref src/centernet_target.py:544-622); dpred[5] zero-filled;
 * scratch2: 2 floats.                                                                                        */
int bevf_centernet_loss_bwd_f32(const bevf_loss_desc* d, float* const dpred[5], float* scratch2, void* stream);
int bevf_stem_im2col_f32(const float* x, float* col, int N, int H, int W, void* stream);   /* [M][160], k=c*49+kh*7+kw */
/* Stem weight gradient without the column matrix: dw [64][160] (k = c*49+kh*7+kw, columns >= 147 unused, zero-filled
 * by the caller) += sum over pixels dy[pixel][co] * x under tap k; x planar NCHW fp32, dy [N][Ho][Wo][64].       */
int bevf_stem_wgrad_f32(const float* x, const float* dy, float* dw, int N, int H, int W, void* stream);
int bevf_smallk_wgrad_f32(const float* dy, const float* x, float* dw, int M, int K, int Cout, void* stream);
/* clip_grad_norm_: out2 = {total L2 norm, min(1, max_norm/(norm+1e-6))}; work512: 512 doubles.                */
int bevf_grad_norm_f32(const float* g, size_t n, double* work512, float max_norm, float* out2, void* stream);
/* torch.optim.AdamW single step on a flat parameter range; gradients are scaled by clip2[1] when given.  The
 * hyper-parameters are doubles, as torch's Python floats: 1 - beta, 1 - lr * weight_decay and lr / (1 - beta1^step)
 * are formed in double and rounded once (1 - 0.999f formed in float would be 1.3e-5 off).                      */
int bevf_adamw_step_f32(float* p, const float* g, float* m, float* v, const float* clip2, size_t n, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int step, void* stream);

/* ==========================================================================================
 * Input pipeline (ref src/train_detect.py:123-189, the dataset's per-sample host work)
 * ========================================================================================== */

/* uint8 HWC frames -> Pillow-identical antialiased bilinear resize (T.Resize on a PIL image: 22-bit fixed point,
 * uint8 after the horizontal pass) -> /255 -> (t-mean)/std -> planar fp32 [n][3][Ho][Wo].  bounds_* [out][2] =
 * (first source index, count), coef_* [out][ksize] = Pillow's integer weights for that axis (host:
 * preprocess.resample_tables).  Replaces ref src/train_detect.py:127-143.                                        */
int bevf_resize_normalize_u8(const unsigned char* x, float* out, int n, int H, int W, int Ho, int Wo,
                             const int32_t* bounds_h, const int32_t* coef_h, int ksize_h, const int32_t* bounds_v,
                             const int32_t* coef_v, int ksize_v, const float* mean3, const float* std3, void* stream);

/* One LiDAR sweep [N][C]: keep points strictly inside pc_range6 = (x0,y0,z0,x1,y1,z1), in input order; out
 * [max_points][C] = the survivors then zero rows, or survivors[choice[i]] when `choice` (max_points int64 indices,
 * the reference's np.random.choice) is given and at least max_points survive.  count = number of survivors.
 * work: N*C + ceil(N / 1024) floats (the compacted rows, then one counter per tile of 1024 points).  Replaces ref
 * src/train_detect.py:150-159, 181-189.                                                                          */
int bevf_lidar_filter_pad_f32(const float* points, float* out, int32_t* count, float* work, const int64_t* choice,
                              int N, int C, int max_points, const float* pc_range6, void* stream);

/* ==========================================================================================
 * Training augmentation (the `dataset.augmentation` section of the reference's YAML, ref configs/base.yaml:85-114,
 * which the reference's drivers never read).  One world transform per frame, one image transform per (frame, camera).
 * ========================================================================================== */

/* Pillow's bilinear coefficient tables for an integer crop window per image: windows [n][4] = (x0, x1, y0, y1) in source pixels;
 * bounds_h [n][Wo][2], coef_h [n][Wo][ksize_h], bounds_v [n][Ho][2], coef_v [n][Ho][ksize_v]; ksize_* = the table stride, at least
 * 2 * ceil(max(1, window / out)) + 1 of the largest window.  Same fp64 operations in the same order as augment.resample_tables_box
 * (no fused multiply-add): bit-equal to the host restatement; unused weights are 0.                                            */
int bevf_resample_tables_box_f64(const int32_t* windows, int n, int H, int W, int Ho, int Wo, int ksize_h, int ksize_v,
                                 int32_t* bounds_h, int32_t* coef_h, int32_t* bounds_v, int32_t* coef_v, void* stream);
/* bevf_resize_normalize_u8's two integer passes with the per-image tables above: x [n][H][W][3] -> out [n][Ho][Wo][3] uint8
 * (= PIL Image.resize((Wo, Ho), BILINEAR, box=window)), gray_sum [n] = sum over the output pixels of Pillow's
 * L = (19595 R + 38470 G + 7471 B + 32768) >> 16 (zeroed here, integer atomics).                                          */
int bevf_resize_crop_u8(const unsigned char* x, unsigned char* out, uint64_t* gray_sum, int n, int H, int W, int Ho, int Wo,
                        const int32_t* bounds_h, const int32_t* coef_h, int ksize_h, const int32_t* bounds_v,
                        const int32_t* coef_v, int ksize_v, void* stream);
/* x [n][Ho][Wo][3] uint8 -> out planar fp32 [n][3][Ho][Wo]: u8 / 255, then per image jitter4 [n][4] = (contrast f_c, brightness f_b,
 * saturation f_s, hue shift) in this order -- clamp(f_c x + (1 - f_c) m) with m = gray_sum / (Ho Wo) / 255, clamp(f_b x), the blend
 * with 0.299 r + 0.587 g + 0.114 b, RGB -> HSV -> (h + shift) mod 1 -> RGB (torchvision's float formulas); a factor of 1 / a shift
 * of 0 skips its step.  flip [n] != 0 stores column Wo - 1 - x.  Last (x - mean) / std as bevf_resize_normalize_u8 does it.     */
int bevf_jitter_flip_normalize_u8(const unsigned char* x, float* out, const uint64_t* gray_sum, const float* jitter4,
                                  const int32_t* flip, int n, int Ho, int Wo, const float* mean3, const float* std3, void* stream);
/* B frames of points [B][N][C] (n_in [B] valid rows each, NULL = N): p' = M p + t with mat12 [B][12] (row-major 3 x 4; x' =
 * fmaf(m2, z, fmaf(m1, y, fmaf(m0, x, m3))), rows 1 and 2 alike), channels (vel_c0, vel_c1) -- both < 0 for none -- multiplied by
 * the upper-left 2 x 2; then bevf_lidar_filter_pad_f32's strict range filter, order-preserving compaction and zero padding: out
 * [B][max_points][C] = the first max_points survivors, count [B] = all survivors.  An exactly-identity frame is copied bit for bit.
 * work: bevf_points_affine_work_floats(B, N, C) floats.                                                                       */
size_t bevf_points_affine_work_floats(int B, int N, int C);
int bevf_points_affine_filter_pad_f32(const float* points, const int32_t* n_in, const float* mat12, float* out, int32_t* count,
                                      float* work, int B, int N, int C, int max_points, int vel_c0, int vel_c1,
                                      const float* pc_range6, void* stream);
/* The same transform in place without the filter (radar): noise [B][N][3] or NULL is added to channels 0-2 times noise_std. */
int bevf_points_affine_f32(float* points, const float* mat12, const float* noise, float noise_std, int B, int N, int C,
                           int vel_c0, int vel_c1, void* stream);
/* Ground-truth boxes in place: boxes [B][M][ncol] (7, or 9 with velocity in columns 7-8), labels [B][M] (< 0: padding row, left
 * untouched), velocities [B][M][2] or NULL, scale [B] = the transform's isotropic scale.  Centre through the affine map, w l h
 * times scale, yaw' = atan2 of the transformed heading (cos yaw, sin yaw), velocities times the upper-left 2 x 2.            */
int bevf_boxes_affine_f32(float* boxes, const int64_t* labels, float* velocities, const float* mat12, const float* scale, int B,
                          int M, int ncol, void* stream);

/* ==========================================================================================
 * Points in boxes and GT-paste (object-sample) augmentation (csrc/gt_paste.hip).
 * Boxes are [x, y, z, w, l, h, yaw(, vx, vy)]: l along the heading (cos yaw, sin yaw), w across it, z-extent [z - h/2, z + h/2].
 * ========================================================================================== */

/* idx [B][N] = the lowest j such that box j of frame b contains point i, or -1.  points [B][N][C] (C >= 3; n_in [B] valid rows each,
 * NULL = N; rows at or past n_in give -1), boxes [B][M][ncol] (ncol 7 or 9), box_mask [B][M] or NULL: rows < 0 are ignored.
 * Inside iff, with d = p - centre, lx = fmaf(dy, sin, dx * cos), ly = fmaf(dy, cos, -(dx * sin)) (sincosf of yaw):
 * |lx| <= l/2, |ly| <= w/2, |dz| <= h/2 and w, l, h > 0; a NaN anywhere gives not inside.  Any M: the boxes pass through LDS in
 * chunks of 64.                                                                                                                  */
int bevf_points_in_boxes_f32(const float* points, const int32_t* n_in, const float* boxes, const int32_t* box_mask, int32_t* idx,
                             int B, int N, int C, int M, int ncol, void* stream);
/* The accept step of the paste, one workgroup per frame.  cand [B][Kc] (Kc <= 64) indexes the bank (bank_boxes [K][bank_ncol],
 * bank_labels [K], obj_ptr [K + 1] = the objects' point ranges); an entry < 0 or >= K is no candidate.  Candidates are taken in order
 * k = 0 .. Kc - 1; candidate k is accepted iff it is one, its BEV rectangle collides with no GT row of label >= 0 (gt_boxes
 * [B][M][ncol], gt_labels [B][M]) and with no ACCEPTED candidate k' < k (a rejected candidate blocks nothing).  Collision = the
 * separating-axis test on the four edge directions, touching counts, z ignored; a rectangle with w <= 0, l <= 0 or a NaN / infinity
 * among (x, y, w, l, yaw) collides with nothing.  Writes accepted [B][Kc] (0 / 1), prefix [B][Kc + 1] = the exclusive prefix of the
 * accepted objects' point counts with their total last, and the new GT rows: out_boxes [B][M + Kc][ncol], out_labels [B][M + Kc],
 * out_velocities [B][M + Kc][2] (NULL together with gt_velocities): rows < M are copies, row M + k is candidate k's box (columns 7-8
 * zeros when the bank has none), label and velocity (the bank's columns 7-8, else zeros) if accepted, else label -1 and zeros.      */
int bevf_paste_accept_f32(const float* gt_boxes, const int64_t* gt_labels, const float* gt_velocities, const float* bank_boxes,
                          const int64_t* bank_labels, const int32_t* obj_ptr, const int32_t* cand, int32_t* accepted, int32_t* prefix,
                          float* out_boxes, int64_t* out_labels, float* out_velocities, int B, int M, int ncol, int K, int bank_ncol,
                          int Kc, void* stream);
/* The remove and append steps.  Points of points [B][N][C] (n_in as above) inside the 3-D extent of an accepted candidate's box (the
 * test of bevf_points_in_boxes_f32) are dropped, the survivors keep their order and their bits; behind them come the accepted objects'
 * points in candidate order and bank order (bank_points [P][C]: xyz relative to the box centre, xyz = relative + centre with one fp32
 * addition per coordinate, other channels copied); then zeros.  out [B][capacity][C] = the first `capacity` rows of that stream,
 * count [B] = min(survivors + appended, capacity).  accepted / prefix: from bevf_paste_accept_f32.  work:
 * bevf_paste_points_work_ints(B, N) int32.  No float atomics; every element of out and count is written.                         */
size_t bevf_paste_points_work_ints(int B, int N);
int bevf_paste_points_f32(const float* points, const int32_t* n_in, const float* bank_points, const int32_t* obj_ptr,
                          const float* bank_boxes, const int32_t* cand, const int32_t* accepted, const int32_t* prefix, float* out,
                          int32_t* count, int32_t* work, int B, int N, int C, int K, int bank_ncol, int Kc, int capacity, void* stream);

/* ==========================================================================================
 * Ego-motion BEV warp (temporal fusion; csrc/bev_warp.hip).
 * ========================================================================================== */

/* y[b][i][j][0:C] (row stride y_cs) = the previous frame's map x [B][H][W] rows of C channels (row stride x_cs) sampled bilinearly
 * at the point current cell (row i = y, column j = x) had in the previous frame.  ego: DEVICE fp64 [B][4][4], M = ego[b] maps a point
 * of the current frame to the previous one, in metres; only M[0:2, 0:2] and M[0:2, 3] are read.  All in fp64:
 *   xc = x0 + (j + 0.5) vx, yc = y0 + (i + 0.5) vy;  (xp, yp) = M[0:2,0:2] (xc, yc) + M[0:2,3]
 *   qj = (xp - x0) / vx - 0.5, qi = (yp - y0) / vy - 0.5;  j0 = floor(qj), fj = qj - j0, i0 = floor(qi), fi = qi - i0
 * weights (1-fi)(1-fj), (1-fi)fj, fi(1-fj), fi fj, each rounded once to fp32; a corner outside [0,H) x [0,W) contributes zero
 * (grid_sample, padding_mode='zeros', align_corners=False), a non-finite q gives a zero row; the sum is fp32 in the corner order
 * (i0,j0), (i0,j0+1), (i0+1,j0), (i0+1,j0+1).  bf16 storage computes in fp32.  Every output row is written.  C, x_cs, y_cs
 * multiples of 4; B * H * W * max(x_cs, y_cs) < 2^31.                                                                           */
int bevf_bev_warp_f32(const float* x, float* y, const double* ego, int B, int H, int W, int C, int x_cs, int y_cs, float x0,
                      float y0, float vx, float vy, void* stream);
int bevf_bev_warp_bf16(const void* x, void* y, const double* ego, int B, int H, int W, int C, int x_cs, int y_cs, float x0,
                       float y0, float vx, float vy, void* stream);
/* The transpose: dx [B][H][W][C] (dense) from dy (row stride dy_cs).  A pull without atomics: source cell (u, v) sums w * dy over the
 * targets whose sample point lies within one cell of it, in row-major target order, the weight recomputed by the forward's own
 * expression; the candidates are the integer bounding box, widened by one cell, of the inverse affine image of
 * [v-1, v+1] x [u-1, u+1].  Every element of dx is written.  The caller keeps the index-space map away from singular (the Python
 * wrapper refuses singular values outside [1/4, 4]).                                                                              */
int bevf_bev_warp_bwd_f32(const float* dy, float* dx, const double* ego, int B, int H, int W, int C, int dy_cs, float x0, float y0,
                          float vx, float vy, void* stream);

/* ==========================================================================================
 * BEV map-segmentation head (csrc/bev_seg.hip).
 * ========================================================================================== */

/* y[b][i][j][0:C] (row stride y_cs), a map [B][Ho][Wo] on the grid (ox0, oy0, ovx, ovy), = x [B][Hi][Wi] rows of C channels (row
 * stride x_cs) on the grid (x0, y0, vx, vy), sampled bilinearly at the output cell's centre; row i is y, column j is x.  All in fp64:
 *   xo = ox0 + (j + 0.5) ovx, qj = (xo - x0) / vx - 0.5, j0 = floor(qj), fj = qj - j0;  the same along y for qi, i0, fi
 * weights (1-fi)(1-fj), (1-fi)fj, fi(1-fj), fi fj, each rounded once to fp32; a corner outside [0,Hi) x [0,Wi) contributes zero
 * (grid_sample, padding_mode='zeros', align_corners=False), a non-finite q gives a zero row; the sum is fp32 in the corner order
 * (i0,j0), (i0,j0+1), (i0+1,j0), (i0+1,j0+1).  bf16 storage computes in fp32.  Every element of the B * Ho * Wo output rows' C
 * channels is written and nothing else.  Any C and strides >= C: 16-byte accesses where bases and strides are multiples of 16
 * bytes, a scalar tail for the rest.  B * Hi * Wi and B * Ho * Wo below 2^31.                                                     */
int bevf_bev_grid_resample_f32(const float* x, float* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cs, int y_cs, double x0,
                               double y0, double vx, double vy, double ox0, double oy0, double ovx, double ovy, void* stream);
int bevf_bev_grid_resample_bf16(const void* x, void* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int x_cs, int y_cs, double x0,
                                double y0, double vx, double vy, double ox0, double oy0, double ovx, double ovy, void* stream);
/* The transpose: dx [B][Hi][Wi][C] (dense) from dy [B][Ho][Wo] rows at stride dy_cs.  A pull without atomics: source cell (r, c)
 * sums w * dy over the output rows and columns whose sample has it as a neighbour -- contiguous index ranges, from the inverse of
 * the scalar map -- in row-major target order, the weight recomputed by the forward's own expression.  Every element of dx is
 * written; bit-reproducible.                                                                                                      */
int bevf_bev_grid_resample_bwd_f32(const float* dy, float* dx, int B, int Hi, int Wi, int Ho, int Wo, int C, int dy_cs, double x0,
                                   double y0, double vx, double vy, double ox0, double oy0, double ovx, double ovy, void* stream);

/* Sigmoid focal loss on logits.  logits: B * P rows of K classes at row stride cs (NHWC); targets uint8 [B][K][P], non-zero = 1.
 * With p = sigmoid(x), p_t = t p + (1 - t)(1 - p), BCE = max(x, 0) - x t + log1p(exp(-|x|)), a_t = alpha t + (1 - alpha)(1 - t) for
 * alpha >= 0 and 1 for alpha < 0:  out[k] = (1 / (B P)) sum a_t (1 - p_t)^gamma BCE over class k, out[K] = sum_k out[k].
 * Elements in fp32, sums in fp64: `partials` (bevf_seg_focal_work_doubles(K) doubles) takes fixed-grid partial sums, a second
 * launch adds them in a fixed order.  K <= 64, gamma >= 0.                                                                       */
size_t bevf_seg_focal_work_doubles(int K);
int bevf_seg_focal_loss_f32(const float* logits, int cs, const uint8_t* targets, int B, int P, int K, float alpha, float gamma,
                            double* partials, float* out, void* stream);
/* dlogit[r][k] (row stride cs) = g[0] * d out[K] / d logits[r][k] for k < K, 0 for K <= k < cs; g: one fp32 on the DEVICE.       */
int bevf_seg_focal_loss_bwd_f32(const float* logits, int cs, const uint8_t* targets, const float* g, float* dlogit, int B, int P,
                                int K, float alpha, float gamma, void* stream);
/* counts int64 [T][K][3] = (TP, FP, FN) over the B * P pixels with the prediction logits[r][k] >= thr[t] (thr: T fp32 on the
 * device, T <= 32) against targets as above.  Integer sums: deterministic.                                                      */
int bevf_seg_iou_counts(const float* logits, int cs, const uint8_t* targets, const float* thr, int T, int64_t* counts, int B, int P,
                        int K, void* stream);

/* ==========================================================================================
 * Map polygons and polylines rasterised into segmentation targets (csrc/map_raster.hip).
 * ========================================================================================== */

/* out uint8 [B][K][Ho][Wo] = 1 where a shape of frame b with class k contains (polygon) or hits (polyline) the centre of cell
 * (row i = y, column j = x), px = x0 + (j + 0.5) vx, py = y0 + (i + 0.5) vy, else 0: the union over the frame's shapes.  The shapes of
 * the whole batch are one CSR set on the DEVICE: vertices fp32 [V][2] in metres, ring_offsets [R + 1] into vertices, shape_offsets
 * [S + 1] into rings, shape_class [S] in 0 .. K-1, shape_kind [S] (0 = polygon: ring 0 the exterior, further rings holes; 1 =
 * polyline: exactly one open ring), shape_width fp32 [S] (a polyline's full width in metres), frame_offsets [B + 1] into shapes.
 * mat: fp32 [B][12], rows 0-2 of the frame's world transform, or NULL = identity; scale: fp32 [B], or NULL = 1.  All in fp64, no
 * contraction, transformed vertices never rounded to fp32:
 *   vertex   x' = (m00 x + m01 y) + m03, y' = (m10 x + m11 y) + m13;  half width hw = 0.5 width scale[b]
 *   polygon  inside = odd number of crossed edges over ALL rings (even-odd).  An edge with equal endpoint y is skipped; otherwise a =
 *            the endpoint with the smaller y, and the edge is crossed when a.y <= py < b.y and
 *            (b.x - a.x) (py - a.y) - (px - a.x) (b.y - a.y) > 0
 *   polyline segment a -> b: e = b - a, u = p - a, w = p - b, t = u.e, l2 = e.e, c = e.x u.y - e.y u.x (dot products x x' + y y');
 *            t <= 0: hit when u.u <= hw^2;  else t >= l2: hit when w.w <= hw^2;  else hit when c c <= hw^2 l2
 * A shape with a non-finite transformed vertex, a ring below 3 vertices (polygon) or 2 (polyline), or an offset or class outside its
 * array contributes nothing (checked on the device; nothing is read out of bounds).  Every byte of out is written; no atomics; two
 * launches on `stream`.  1 <= K <= 64; S = 0 (then the shape arrays may be NULL) writes zeros.  work:
 * bevf_map_raster_work_bytes(S, V) bytes, 16-byte aligned (one 64-byte record per shape, one 32-byte fp64 edge per vertex).      */
size_t bevf_map_raster_work_bytes(int S, int V);
int bevf_map_raster_u8(const float* vertices, int V, const int32_t* ring_offsets, int R, const int32_t* shape_offsets,
                       const int32_t* shape_class, const int32_t* shape_kind, const float* shape_width, int S,
                       const int32_t* frame_offsets, int B, const float* mat, const float* scale, int K, int Ho, int Wo, double x0,
                       double y0, double vx, double vy, void* work, uint8_t* out, void* stream);

/* ==========================================================================================
 * Multi-sweep LiDAR accumulation (csrc/sweeps.hip).
 * ========================================================================================== */

/* The key sweep and the preceding sweeps of B frames merged into one padded cloud per frame.  points [B][S][N][C] (3 <= C <= 8),
 * counts [B][S] valid rows per sweep (clamped to [0, N]; 0 = an absent sweep), sweep 0 the key sweep, later indices older.  A row is
 * dropped when fabsf(x) < close_radius && fabsf(y) < close_radius on the sweep's own fp32 coordinates (close_radius <= 0: no such
 * test).  The others go through sweep_to_key (DEVICE fp64 [B][S][4][4], only the top 3 x 4 is read) in fp64, rounded once to fp32:
 *   x' = (float)(((m00 (double)x + m01 (double)y) + m02 (double)z) + m03), y' and z' alike, in this order, no fused multiply-add,
 * then bevf_lidar_filter_pad_f32's strict range filter on the rounded coordinates (a NaN fails it).  out [B][max_points][C + 1]: a
 * surviving row = x' y' z', channels 3 .. C-1 copied bit for bit, then time_lag[b][s] (fp32 [B][S]); sweep 0's survivors in point
 * order, then sweep 1's, ...; the first max_points of that order are kept, the rows behind the last survivor are zeros.  count [B] =
 * all survivors and sweep_count [B][S] = each sweep's, both untruncated.  No atomics (bit-reproducible), no allocation, four launches
 * on `stream` whose grids depend on (B, S, N) only.  work: bevf_sweeps_merge_work_bytes(B, S, N) bytes, 4-byte aligned (two ints
 * per tile of 1024 rows).  B, S < 65536; S * N < 2^31.                                                                          */
size_t bevf_sweeps_merge_work_bytes(int B, int S, int N);
int bevf_sweeps_merge_f32(const float* points, const int32_t* counts, const double* sweep_to_key, const float* time_lag, float* out,
                          int32_t* count, int32_t* sweep_count, void* work, int B, int S, int N, int C, int max_points,
                          float close_radius, const float* pc_range6, void* stream);
/* sweep_to_key [B][S][4][4] = inv(L_k) . inv(E_k) . E_s . L_s, all DEVICE fp64: key_lidar2ego L_k and key_ego2global E_k [B][4][4],
 * sweep_lidar2ego L_s and sweep_ego2global E_s [B][S][4][4]; only the top 3 x 4 of each is read, the bottom rows count as 0 0 0 1.
 * inv = the rigid inverse (R^T, -(R^T t)) with each element of R^T t = ((r0 t0 + r1 t1) + r2 t2); a product element =
 * (((a0 b0 + a1 b1) + a2 b2) + a3 b3); products right to left (E_s . L_s first); no fused multiply-add; the bottom row is written as
 * 0 0 0 1.  A sweep whose L_s and E_s equal L_k and E_k element for element (the key sweep itself) gets the exact identity.      */
int bevf_sweep_pose_chain_f64(const double* key_lidar2ego, const double* key_ego2global, const double* sweep_lidar2ego,
                              const double* sweep_ego2global, double* sweep_to_key, int B, int S, void* stream);

/* ==========================================================================================
 * Multi-object tracking on the decode path (csrc/track.hip).
 * ========================================================================================== */

/* One step of CenterPoint's greedy centre-distance tracker for B independent streams (a stream = one batch row), one wave per stream.
 * Detections, as bevf_centernet_decode_f32 / bevf_nms_boxes_f32 leave them (descending score): boxes [B][N][7], velocities [B][N][2],
 * scores [B][N], labels int64 [B][N], count [B] (clamped to [0, N]; rows past it are never read).  ego_motion: DEVICE fp64 [B][4][4],
 * current frame -> previous frame, rigid M = [R t] (the tensor bevf_bev_warp_* takes; only the top 3 x 4 is read); dt fp32 [B] seconds;
 * max_dist fp32 [C] metres per label.  The state (capacity T per stream, overwritten in place, owned by the caller): track_box
 * [B][T][7], track_vel [B][T][2], track_score [B][T], track_label / track_id int64 [B][T], track_age (steps since the last match) /
 * track_hits int32 [B][T], track_count [B] (clamped to [0, T]), next_id int64 [B]; rows past track_count are zeros with id -1 and the
 * state is in the sensor frame of the step that wrote it.  A fresh state is all zeros with track_id -1.  The step, per stream:
 *  1. detections i < count in order; a detection is valid when x, y, z, vx, vy and score are finite.  In fp64, rounded once:
 *       px = x - vx dt, py = y - vy dt;  qx = (float)(((m00 px + m01 py) + m02 z) + m03), qy = (float)(((m10 px + m11 py) + m12 z) + m13)
 *     Among the tracks not taken yet (with track_label == label_i when class_aware) whose fp32 squared distance
 *     d2 = (qx - tx)(qx - tx) + (qy - ty)(qy - ty) to the stored centre is <= max_dist[l]^2 (l = label_i inside [0, C), else 0), the
 *     one with the smallest d2 is matched and taken; a tie goes to the lower slot.  NaN anywhere (q, max_dist) compares as no match;
 *     max_dist^2 saturates at FLT_MAX, so a d2 that overflowed to +inf matches nothing.
 *  2. a matched track takes the detection's box, velocity and score; label and id stay; age = 0, hits += 1.
 *  3. an unmatched track: age += 1; dropped when age > max_age; else coasted into the current frame, fp64 mul / add, rounded once:
 *       u = p - t;  v'x = r00 vx + r10 vy, v'y = r01 vx + r11 vy;  x' = (float)(((r00 ux + r10 uy) + r20 uz) + v'x dt),
 *       y' = (float)(((r01 ux + r11 uy) + r21 uz) + v'y dt), z' = (float)((r02 ux + r12 uy) + r22 uz), velocity = (float)v',
 *       yaw' = (float)((double)yaw - atan2(m10, m00)) (not wrapped); size, score, label, id, hits unchanged.
 *  4. a valid unmatched detection with score >= birth_score starts a track in detection order: id = next_id++, hits = 1, age = 0;
 *     with the state full it gets no track, consumes no id and is counted in overflow[b].
 *  5. new state = surviving old tracks in their previous slot order, then the births in detection order; the rest is padding.
 * Per detection: det_track_id int64 [B][N] (-1: rows >= count, neither matched nor born, overflow), det_hits int32 [B][N] (0 where
 * there is no track), det_slot int32 [B][N] (slot in the new state or -1); overflow int32 [B].  No fused multiply-add: every column
 * but the coasted yaw is reproducible bit for bit.  One launch on `stream`, no workspace, no atomics, no allocation, nothing read
 * back (graph-capturable).  0 <= N <= 4096 (N = 0: the detection pointers may be NULL), 1 <= T <= 1024, C >= 1, max_age >= 0.   */
int bevf_track_step_f32(const float* boxes, const float* velocities, const float* scores, const int64_t* labels,
                        const int32_t* count, const double* ego_motion, const float* dt, const float* max_dist, float* track_box,
                        float* track_vel, float* track_score, int64_t* track_label, int64_t* track_id, int32_t* track_age,
                        int32_t* track_hits, int32_t* track_count, int64_t* next_id, int64_t* det_track_id, int32_t* det_hits,
                        int32_t* det_slot, int32_t* overflow, int B, int N, int T, int C, int max_age, float birth_score,
                        int class_aware, void* stream);

/* ==========================================================================================
 * BEV backbone + FPN neck: transposed convolution with kernel = stride (csrc/deconv.hip).
 * ========================================================================================== */

/* nn.ConvTranspose2d(Cin, Cout, kernel_size = s, stride = s, bias = False) (+ folded BatchNorm)(+ ReLU) on NHWC maps:
 *     y[n][s*h + i][s*w + j][co] = act( (sum_ci x[n][h][w][ci] * W[ci][co][i][j]) * scale[co] + shift[co] )
 * One launch: a GEMM over the N*H*W input pixels whose epilogue scatters each pixel's s*s channel runs to its s*s output pixels (no
 * intermediate, no shuffle pass).  fp32: v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulate.  bf16: x / y / packed weights
 * in bf16, v_mfma_f32_32x32x16_bf16, fp32 accumulate, one rounding at the store; scale / shift stay fp32.  `y` may point into a
 * channel slice of a wider map (y_cs = that map's channel count): only the Cout channels of the slice are written.
 * `w`: the packed filter made by bevf_deconv_pack_f32 / _bf16 from the module's fp32 (Cin, Cout, s, s) tensor, once per weight
 * version (bevf_deconv_pack_elems(Cin, Cout, s, bf16) elements of the storage type).
 * Supported (anything else: BEVF_ERR_UNSUPPORTED with a message, nothing launched): s in {2, 4}; Cin % 32 == 0; Cout % 32 == 0;
 * x_cs >= Cin, y_cs >= Cout, both multiples of 4 (fp32) / 8 (bf16); x, w, y 16-byte aligned; N*H*W*x_cs and N*sH*sW*y_cs below
 * 2^31 elements and below 2 GiB (32-bit byte offsets).  s = 1 is a 1x1 convolution: bevf_conv2d_nhwc_* with the transposed weight.
 * Stream-ordered, no allocation, no atomics, bit-equal run to run, graph-capturable.
 * (A tagged struct, unlike the descriptors above: it is passed as an opaque pointer by the bindings.) */
typedef struct bevf_deconv_desc {
  const void* x;       /* [N][H][W][x_cs], first Cin channels of each pixel are read */
  const void* w;       /* packed filter */
  const float* scale;  /* [Cout] or NULL (1) */
  const float* shift;  /* [Cout] or NULL (0) */
  void* y;             /* [N][s*H][s*W][y_cs], Cout channels of each pixel are written */
  int32_t N, H, W, Cin, x_cs, Cout, y_cs, s;
  int32_t relu;        /* 0: none, 1: ReLU */
} bevf_deconv_desc;
size_t bevf_deconv_pack_elems(int Cin, int Cout, int s, int bf16);
int bevf_deconv_pack_f32(const float* w, float* out, int Cin, int Cout, int s, void* stream);
int bevf_deconv_pack_bf16(const float* w, void* out, int Cin, int Cout, int s, void* stream);
int bevf_deconv_nhwc_f32(const bevf_deconv_desc* d, void* stream);
int bevf_deconv_nhwc_bf16(const bevf_deconv_desc* d, void* stream);

/* ==========================================================================================
 * CenterPoint second stage: RoI BEV-point head (csrc/roi_points.hip, csrc/roi_head.hip).
 * ========================================================================================== */

/* Conventions of all entry points below.  RoIs are the decode's padded records: boxes [B][K][7] = (x, y, z, w, l, h, yaw) with l along
 * the heading, count int32 [B] clamped to [0, K]; rows past the count are never read.  The map is flat NHWC [B][H][W] rows of C
 * channels at channel stride x_cs, covering [x_min, x_max) x [y_min, y_max): cells of vx = (x_max - x_min) / W by
 * vy = (y_max - y_min) / H, a cell's feature at the cell centre, so a world point (px, py) samples at column
 * u = (px - x_min) / vx - 0.5, row v = (py - y_min) / vy - 0.5.  Everything is stream-ordered, allocates nothing, uses no atomics, is
 * bit-equal run to run, reads nothing back and is graph-capturable.
 *
 * bevf_roi_bev_points_*: feat [B * K][5 * C] in the map's storage type, row (b, k); point p occupies channels [p C, (p + 1) C).  The
 * points, in order: the centre, centre +- (l / 2)(cos yaw, sin yaw) (front, back), centre +- (w / 2)(-sin yaw, cos yaw) (left, right),
 * in fp64 from the fp32 box.  A sample = the corner (i0, j0) = (floor v, floor u) and the four weights (1 - fi)(1 - fj), (1 - fi) fj,
 * fi (1 - fj), fi fj (fp64 products, each rounded once to fp32) of the corners (i0, j0), (i0, j0 + 1), (i0 + 1, j0), (i0 + 1, j0 + 1);
 * a channel = w0 v0, then fma with corners 1, 2, 3 in fp32 (bevf_bev_warp_* / bevf_bev_grid_resample_*'s order), rounded once to the
 * storage type.  A corner outside the map contributes zero; a row with k >= count[b], a non-finite point and a point with u or v
 * outside (-1, W) / (-1, H) are written as zeros.  table (optional, for the backward): int32 [B * K * 5][6] = i0, j0 and the bits
 * of the four weights (all zero for a zero row); bevf_roi_bev_points_table_words(B, K) words.  fp32 moves channel quads when
 * C % 4 == 0 (x_cs % 4 == 0, 16-byte aligned buffers), bf16 eight or four channels when C % 8 == 0 / C % 4 == 0; anything else scalar.
 * B * K * 5 * max(C, 6), B * H * W * x_cs below 2^31.                                                                               */
size_t bevf_roi_bev_points_table_words(int B, int K);
int bevf_roi_bev_points_f32(const float* x, const float* boxes, const int32_t* count, float* feat, int32_t* table, int B, int K,
                            int H, int W, int C, int x_cs, double x_min, double y_min, double x_max, double y_max, void* stream);
int bevf_roi_bev_points_bf16(const void* x, const float* boxes, const int32_t* count, void* feat, int32_t* table, int B, int K,
                             int H, int W, int C, int x_cs, double x_min, double y_min, double x_max, double y_max, void* stream);
/* The gradient of the map: dx [B][H][W][C] (dense) = sum over the frame's samples s = k * 5 + p < 5 count[b], in ascending s, of
 * w(s -> cell) * dfeat[b * K * 5 + s][:] (dfeat [B * K][5 * C] dense), by fma from 0.  A pull: one wave per map cell scans the frame's
 * table rows 64 at a time.  Cells no sample touches are exact zeros; every cell is written.                                      */
int bevf_roi_bev_points_bwd_f32(const float* dfeat, const int32_t* table, const int32_t* count, float* dx, int B, int K, int H,
                                int W, int C, void* stream);
/* RoI targets against the padded ground truth gt [B][M][7], gt_labels int32 [B][M] (< 0 = padding; M = 0: both may be NULL).  A GT is
 * a candidate of RoI (b, k) when its label is >= 0 and, with match_labels, equals roi_labels[b][k] (int64 [B][K], else may be NULL).
 * Per RoI with k < count[b]:  iou = the best IoU(roi, gt) over the candidates (box_geom.h's rotated 3-D IoU, or the BEV IoU when
 * use_bev), gt_index = the lowest index among equal best values; no candidate: gt_index = -1, iou = 0.
 *   cls_target = clamp(2 iou - 0.5, 0, 1);  reg_mask = iou >= reg_fg_thresh and all six sizes > 0;
 *   reg_target[7] (zeros where reg_mask is 0), with d = gt - roi, c = cos yaw, s = sin yaw, diag = sqrt(l^2 + w^2) of the RoI:
 *     ((c dx + s dy) / diag, (c dy - s dx) / diag, dz / h, log(w_g / w), log(l_g / l), log(h_g / h), dyaw),
 *     dyaw = yaw_g - yaw wrapped into [-pi, pi), then folded into [-pi / 2, pi / 2] by -+ pi (opposite headings are the same box).
 * Rows past the count: zeros with gt_index -1.  iou, cls_target [B][K]; gt_index int32 [B][K]; reg_mask uint8 [B][K]; reg_target
 * [B][K][7].  One wave per RoI.                                                                                                  */
int bevf_roi_targets_f32(const float* rois, const int32_t* count, const int64_t* roi_labels, const float* gt, const int32_t* gt_labels,
                         float* iou, int32_t* gt_index, float* cls_target, uint8_t* reg_mask, float* reg_target, int B, int K, int M,
                         int use_bev, int match_labels, float reg_fg_thresh, void* stream);
/* The head's output pred [B * K][8] = the logit, then seven residuals.  Over the rows with k < count[b] (n_valid of them, n_fg with
 * reg_mask set):  cls_loss = sum (max(x, 0) - x t + log1p(exp(-|x|))) / (n_valid + 1e-4), reg_loss = sum over reg_mask of
 * sum_7 |res - reg_target| / (n_fg + 1e-4);  out[3] = w_cls cls_loss + w_reg reg_loss, cls_loss, reg_loss.  One workgroup, sums in
 * fp64 in a fixed order.  bwd: dpred [B * K][8] = d out[0] / d pred, exact zeros on rows past the count.                          */
int bevf_roi_loss_f32(const float* pred, const int32_t* count, const float* cls_target, const uint8_t* reg_mask,
                      const float* reg_target, float* out, int B, int K, float w_cls, float w_reg, void* stream);
int bevf_roi_loss_bwd_f32(const float* pred, const int32_t* count, const float* cls_target, const uint8_t* reg_mask,
                          const float* reg_target, float* dpred, int B, int K, float w_cls, float w_reg, void* stream);
/* The refine step: the inverse of the encoding above applied to every RoI with the residual t = pred[1 .. 7],
 *   x' = x + (c t0 - s t1) diag, y' = y + (s t0 + c t1) diag, z' = z + t2 h, (w', l', h') = (w exp t3, l exp t4, h exp t5),
 *   yaw' = yaw + t6 (not wrapped);  score' = sqrt(score * sigmoid(pred[0]));  labels (int64) and velocities ([B][K][2], optional:
 *   both pointers NULL) carried through.
 * A row is dropped when k >= count[b], when score' is not finite or when score' < score_thresh.  The frame's kept rows are written
 * compacted and in descending score', ties by ascending RoI index -- what bevf_nms_boxes_f32 and bevf_track_step_f32 expect of their
 * input -- out_count[b] = their number, the rows behind them zeros.  One workgroup per frame, ranks by counting over the scores in
 * LDS.  K <= 4096, B <= 65535; the outputs must not alias the inputs.                                                             */
int bevf_roi_refine_f32(const float* rois, const float* scores, const int64_t* labels, const float* velocities, const int32_t* count,
                        const float* pred, float* out_boxes, float* out_scores, int64_t* out_labels, float* out_velocities,
                        int32_t* out_count, int B, int K, float score_thresh, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVF_H */
