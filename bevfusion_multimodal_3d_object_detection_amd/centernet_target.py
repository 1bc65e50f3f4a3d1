"""Drop-in for the reference's `centernet_target` module (ref src/centernet_target.py), on device.

* `prepare_centernet_targets` -- one kernel launch for the whole batch (the reference loops over
  objects on the host and round-trips the heatmap device->numpy->device per object, ref :278-280).
* `CenterNetLoss` -- focal + gather-L1 reductions on device, including the reference's second
  sigmoid on the already-sigmoided heatmap (ref :563).
* `decode_padded` -- the same decode left on the device as padded records and a count (for `tracking.Tracker`).
* `decode_centernet_predictions` -- keep mask, two-level top-K, gather and box assembly on device;
  voxel size 2.048 m (ref :389).  `labels` are always 0 exactly like the reference (ref :434);
  pass `true_labels=True` for the class of the winning heatmap plane.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import box_ops
from . import engine as E
from .box_ops import decode_settings  # noqa: F401

PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def _decode_device(predictions: Dict[str, torch.Tensor], score_thresh: float, max_detections: int, voxel_size: float,
                   true_labels: bool = False, nms_type: Optional[str] = None, nms_iou_thresh: float = 0.5,
                   nms_radius: Optional[float] = None, nms_pre_max: int = 512, class_aware: bool = False, iou_rectify=None):
    """The decode's device half: padded (boxes, scores, labels, velocities) records and count, nothing read back."""
    box_ops.check_nms_args(nms_type, nms_iou_thresh, nms_radius, nms_pre_max, class_aware, true_labels)
    heat = predictions["heatmap"]
    E.require_cuda(heat)
    pred = {k: predictions[k].float().contiguous() for k in ("heatmap", "offset", "size", "rot", "vel")}
    K = max_detections if nms_type is None else int(nms_pre_max)
    if iou_rectify is None:
        boxes, scores, labels, vels, count = L.centernet_decode(pred, K, float(score_thresh),
                                                                float(voxel_size), PC_RANGE[0], PC_RANGE[1], true_labels)
    else:
        # IoU-aware score rectification: fused into the decode's first kernel, no extra launch or map
        from .iou_aware import rectify_alpha
        alpha = rectify_alpha(iou_rectify, heat.shape[1])
        if "iou" not in predictions:
            raise L.BevfError("iou_rectify needs predictions['iou'] (build the detector with iou_head=True)")
        E.require_cuda(predictions["iou"])
        boxes, scores, labels, vels, count = L.centernet_decode(
            pred, K, float(score_thresh), float(voxel_size), PC_RANGE[0], PC_RANGE[1], true_labels,
            iou=predictions["iou"].float().contiguous(), alpha=torch.tensor(alpha, dtype=torch.float32, device=heat.device))
    if nms_type is not None:
        # box NMS over the count[b] candidates above score_thresh (already in descending score order); the survivors come back
        # compacted and cut to max_detections, and their number replaces `count` (the one value `_decode` reads back)
        thresh = float(nms_radius) if nms_type == "circle" else float(nms_iou_thresh)
        _, count, boxes, scores, labels, vels = L.nms_boxes(boxes, count, nms_type, thresh, int(max_detections), scores=scores,
                                                            labels=labels, velocities=vels, class_aware=class_aware, gather=True)
    return boxes, scores, labels, vels, count


def _decode(predictions: Dict[str, torch.Tensor], score_thresh: float, max_detections: int, voxel_size: float,
            true_labels: bool = False, nms_type: Optional[str] = None, nms_iou_thresh: float = 0.5,
            nms_radius: Optional[float] = None, nms_pre_max: int = 512, class_aware: bool = False,
            iou_rectify=None) -> List[Dict[str, torch.Tensor]]:
    boxes, scores, labels, vels, count = _decode_device(predictions, score_thresh, max_detections, voxel_size, true_labels, nms_type,
                                                        nms_iou_thresh, nms_radius, nms_pre_max, class_aware, iou_rectify)
    counts = count.cpu().tolist()                     # the reference syncs here too (mask.sum() == 0, ref :362)
    out = []
    for b, n in enumerate(counts):
        if n == 0:                                    # ref :363-368 returns CPU zeros for an empty frame
            out.append({"boxes": torch.zeros(0, 7), "scores": torch.zeros(0),
                        "labels": torch.zeros(0, dtype=torch.long), "velocities": torch.zeros(0, 2)})
        else:
            out.append({"boxes": boxes[b, :n], "scores": scores[b, :n], "labels": labels[b, :n],
                        "velocities": vels[b, :n]})
    return out


def decode_padded(predictions: Dict[str, torch.Tensor], score_thresh: float = 0.3, max_detections: int = 100,
                  true_labels: bool = False, *, nms_type: Optional[str] = None, nms_iou_thresh: float = 0.5,
                  nms_radius: Optional[float] = None, nms_pre_max: int = 512, class_aware: bool = False,
                  voxel_size: float = 2.048, iou_rectify=None) -> Dict[str, torch.Tensor]:
    """`decode_centernet_predictions` without its host read: the padded device records the decode (and the box NMS) compute, as
    {"boxes" (B,K,7), "velocities" (B,K,2), "scores" (B,K), "labels" int64 (B,K), "count" int32 (B,)} with K = max_detections
    (nms_pre_max with an NMS), rows past count[b] not meaningful.  Same keywords and the same launches; nothing is synchronised, so
    decode -> NMS -> `tracking.Tracker.step` runs without a round trip to the host."""
    boxes, scores, labels, vels, count = _decode_device(predictions, score_thresh, max_detections, voxel_size, true_labels, nms_type,
                                                        nms_iou_thresh, nms_radius, nms_pre_max, class_aware, iou_rectify)
    return {"boxes": boxes, "velocities": vels, "scores": scores, "labels": labels, "count": count}


def decode_centernet_predictions(predictions: Dict[str, torch.Tensor], score_thresh: float = 0.3,
                                 max_detections: int = 100, true_labels: bool = False, *, nms_type: Optional[str] = None,
                                 nms_iou_thresh: float = 0.5, nms_radius: Optional[float] = None, nms_pre_max: int = 512,
                                 class_aware: bool = False, iou_rectify=None) -> List[Dict[str, torch.Tensor]]:
    """ref src/centernet_target.py:326-413 (2.048 m cells).  nms_type 'rotate' | 'circle' (opt-in, not in the reference): decode the
    nms_pre_max best peaks, run box NMS over those above score_thresh (box_ops; rotated IoU > nms_iou_thresh, or centres closer
    than nms_radius metres; class_aware: within a label only, needs true_labels) and return the first max_detections survivors.
    iou_rectify (opt-in): alpha in [0, 1], or one per class -- a peak of class c that survives the 3x3 keep mask
    is scored s^(1 - alpha_c) * q^alpha_c, q = clamp((predictions['iou'] + 1) / 2, 0, 1), before the top-K; the threshold, the NMS
    order and the returned scores are the rectified ones.  None: the unrectified decode, launch for launch and bit for bit."""
    return _decode(predictions, score_thresh, max_detections, 2.048, true_labels, nms_type, nms_iou_thresh, nms_radius,
                   nms_pre_max, class_aware, iou_rectify)


def _nms(heat: torch.Tensor, kernel: int = 3) -> torch.Tensor:
    """ref :416-421 -- heat * (maxpool3x3(heat) == heat).  Device tensor in, device tensor out."""
    if kernel != 3:
        raise NotImplementedError("only the 3x3 keep mask of the reference is built")
    E.require_cuda(heat)
    out = torch.empty_like(heat, dtype=torch.float32)
    B, C, H, W = heat.shape
    L.nms_keep(heat.float().contiguous(), out, B * C, H, W)
    return out


def gaussian_2d(shape: Tuple[int, int], sigma: float = 1.0):
    """ref :118-125 -- (m,n) gaussian window exp(-(x^2+y^2)/(2 sigma^2)) centred on the middle element, values below
    eps*max flushed to 0.  Host numpy helper kept for API parity (`prepare_centernet_targets` evaluates the same
    window inside its kernel)."""
    import numpy as np
    half_m, half_n = (shape[0] - 1.) / 2., (shape[1] - 1.) / 2.
    y, x = np.ogrid[-half_m:half_m + 1, -half_n:half_n + 1]
    g = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    g[g < np.finfo(g.dtype).eps * g.max()] = 0
    return g


def draw_gaussian(heatmap, center: Tuple[int, int], radius: float, k: float = 1.0):
    """ref :152-168 -- element-wise max of `heatmap` (H,W numpy array, modified in place) with a (2r+1)^2 gaussian of
    sigma (2r+1)/6 centred on `center` = (x, y), clipped at the borders.  Host helper for API parity."""
    import numpy as np
    diameter = 2 * radius + 1
    g = gaussian_2d((diameter, diameter), sigma=diameter / 6)
    x, y = int(center[0]), int(center[1])
    H, W = heatmap.shape[0:2]
    left, right = min(x, radius), min(W - x, radius + 1)
    top, bottom = min(y, radius), min(H - y, radius + 1)
    dst = heatmap[y - top:y + bottom, x - left:x + right]
    src = g[radius - top:radius + bottom, radius - left:radius + right]
    if min(src.shape) > 0 and min(dst.shape) > 0:
        np.maximum(dst, src * k, out=dst)


def gaussian_radius(det_size: Tuple[float, float], min_overlap: float = 0.7) -> float:
    """ref :128-150 (host helper kept for API parity; the device kernel evaluates the same expression)."""
    import numpy as np
    height, width = det_size
    b1 = height + width
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * (width * height * (1 - min_overlap) / (1 + min_overlap)))) / 2
    b2 = 2 * (height + width)
    r2 = (b2 + np.sqrt(b2 ** 2 - 16 * ((1 - min_overlap) * width * height))) / 2
    a3, b3 = 4 * min_overlap, -2 * min_overlap * (height + width)
    r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * ((min_overlap - 1) * width * height))) / 2
    return min(r1, r2, r3)


def prepare_centernet_targets(batch: Dict, device: torch.device, pc_range: Optional[List[float]] = None,
                              bev_size: Tuple[int, int] = (50, 50), num_classes: int = 10, max_objects: int = 500,
                              gaussian_overlap: float = 0.7, min_radius: int = 2) -> Dict[str, torch.Tensor]:
    """ref :170-324.  batch['gt_boxes'] / ['gt_labels']: per-frame (M,7|9) boxes and (M,) labels (-1 = padding),
    lists or stacked tensors.  Returns the reference's 12 target tensors, computed by one kernel launch."""
    if pc_range is None:
        pc_range = PC_RANGE
    device = torch.device(device)
    if device.type != "cuda":
        raise L.BevfError("prepare_centernet_targets runs on the GPU: pass device='cuda' (no CPU fallback)")
    boxes_l, labels_l = batch["gt_boxes"], batch["gt_labels"]
    B = len(boxes_l)
    H, W = bev_size
    nmax = max([min(len(b), max_objects) for b in boxes_l] + [1])
    bc = max([b.shape[1] if hasattr(b, "shape") and len(b.shape) == 2 and len(b) else 7 for b in boxes_l] + [7])
    bc = 9 if bc > 7 else 7
    boxes = torch.zeros(B, nmax, 9, dtype=torch.float32)
    labels = torch.full((B, nmax), -1, dtype=torch.int32)
    has_vel = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        bb = torch.as_tensor(boxes_l[b]).detach().float().cpu()
        ll = torch.as_tensor(labels_l[b]).detach().cpu()
        n = min(len(bb), max_objects)
        if n:
            boxes[b, :n, :min(bb.shape[1], 9)] = bb[:n, :9]
            labels[b, :n] = ll[:n].to(torch.int32)
            has_vel[b] = 1 if bb.shape[1] > 7 else 0
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
    out = dict(heatmap=f(B, num_classes, H, W), offset=f(B, 2, H, W), size=f(B, 3, H, W), rot=f(B, 2, H, W),
               vel=f(B, 2, H, W), mask=torch.zeros(B, max_objects, dtype=torch.uint8, device=device),
               ind=torch.zeros(B, max_objects, dtype=torch.long, device=device),
               reg_mask=torch.zeros(B, max_objects, dtype=torch.uint8, device=device),
               target_offset=f(B, max_objects, 2), target_size=f(B, max_objects, 3),
               target_rot=f(B, max_objects, 2), target_vel=f(B, max_objects, 2))
    L.centernet_targets(boxes.to(device), labels.to(device), has_vel.to(device), out, B, nmax, H, W, num_classes,
                        max_objects, pc_range, float(gaussian_overlap), int(min_radius))
    return out


class CenterNetLoss(nn.Module):
    """ref :455-622.  weights 1,1,1,1,0.1 (the YAML's loss_weights are unread in the reference, ref :460-467)."""

    def __init__(self, heatmap_weight: float = 1.0, offset_weight: float = 1.0, size_weight: float = 1.0,
                 rot_weight: float = 1.0, vel_weight: float = 0.1):
        super().__init__()
        self.heatmap_weight, self.offset_weight = heatmap_weight, offset_weight
        self.size_weight, self.rot_weight, self.vel_weight = size_weight, rot_weight, vel_weight

    def forward(self, predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        E.require_cuda(predictions["heatmap"], targets["heatmap"])
        w = (self.heatmap_weight, self.offset_weight, self.size_weight, self.rot_weight, self.vel_weight)
        if torch.is_grad_enabled() and any(t.requires_grad for t in predictions.values()):
            from . import training
            return training.loss_with_grad(predictions, targets, w)
        with torch.no_grad():
            vals = L.centernet_loss(predictions, targets, w)        # (6,) device tensor
        names = ("total_loss", "heatmap_loss", "offset_loss", "size_loss", "rot_loss", "vel_loss")
        return {n: vals[i] for i, n in enumerate(names)}


def _topk(scores: torch.Tensor, K: int = 100):
    """ref :424-452 (see fusion_detection._topk)."""
    from .fusion_detection import _topk as impl
    return impl(scores, K)


class DetectionLoss(nn.Module):
    """ref :13-116 -- the loss of the MLP-head path (`cls`/`box` predictions), imported by src/train_detect.py:24-29
    but never used by the bev + centernet path (out of scope as compute).  Importable name that
    raises on construction."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError("DetectionLoss (ref src/centernet_target.py:13-116) belongs to the MLP detection "
                                  "head, which is outside the MI355X bev+centernet hot path; use CenterNetLoss")


def example_usage(seed: int = 0) -> Dict[str, torch.Tensor]:
    """ref :626-679 -- the reference's own walk-through of this module: targets for its two hand-written frames (2 + 3 boxes) on
    a 200 x 200 BEV grid, then CenterNetLoss on random predictions; prints the target shapes and the five loss terms and returns
    the loss dict.  Runs on the GPU only (the predictions come from torch's generator, seeded here)."""
    if not torch.cuda.is_available():
        raise L.BevfError("example_usage runs the target / loss kernels on the GPU: no 'cuda' device is visible")
    device = torch.device("cuda")
    batch = {
        "gt_boxes": [torch.tensor([[10.5, 20.3, -0.5, 1.8, 4.5, 1.6, 0.5], [-5.2, -15.7, -0.8, 2.0, 4.8, 1.7, -1.2]]),
                     torch.tensor([[8.1, 12.4, -0.6, 1.9, 4.6, 1.65, 0.8], [15.3, -8.9, -0.7, 1.85, 4.55, 1.62, -0.5],
                                   [-12.7, 25.6, -0.55, 1.95, 4.7, 1.68, 1.1]])],
        "gt_labels": [torch.tensor([0, 0]), torch.tensor([0, 1, 0])],
    }
    targets = prepare_centernet_targets(batch=batch, device=device, pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0],
                                        bev_size=(200, 200), num_classes=10)
    print("Target shapes:")
    for key, value in targets.items():
        print(f"  {key}: {value.shape}")
    gen = torch.Generator(device="cpu").manual_seed(seed)
    predictions = {k: torch.randn(2, c, 200, 200, generator=gen).to(device)
                   for k, c in (("heatmap", 10), ("offset", 2), ("size", 3), ("rot", 2), ("vel", 2))}
    losses = CenterNetLoss()(predictions, targets)
    print("\nLosses:")
    for key, value in losses.items():
        print(f"  {key}: {value.item():.4f}")
    return losses
