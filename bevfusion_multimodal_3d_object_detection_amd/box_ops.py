"""Box-to-box geometry on device: rotated BEV / 3-D IoU and box NMS (csrc/box_nms.hip).

Box convention, the one `decode_centernet_predictions` writes: `[x, y, z, w, l, h, yaw]` is the rectangle centred at (x, y)
with extent l along the heading (cos yaw, sin yaw) and w across it; its z-extent is [z - h/2, z + h/2].

* `boxes_iou_bev(a, b)` / `boxes_iou3d(a, b)` -- pairwise IoU, (N,7) x (M,7) -> (N,M), or batched (B,N,7) x (B,M,7) -> (B,N,M)
  with optional per-frame counts (entries past a count are 0).
* `points_in_boxes(points, boxes, point_counts, box_mask)` -- per point the lowest index of a box that contains it, or -1
  (csrc/gt_paste.hip; the crop of `gt_paste.ObjectBank.from_frames`).
* `nms_rotated(boxes, scores, iou_thresh, ...)` / `nms_circle(boxes, scores, radius, ...)` -- greedy NMS of one frame, kept
  indices in descending score order (ties: the lower index first).
* `decode_settings(config, section)` -- the reference YAML's `<section>.post_processing` keys as keyword arguments of
  `decode_centernet_predictions` (the reference never reads `nms_threshold`; here it switches the rotated NMS on).

Everything runs on the GPU; CPU tensors raise `BevfError` (no CPU fallback).
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from . import _lib as L
from . import engine as E

NMS_TYPES = (None, "rotate", "circle")


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def _counts(c, B: int, dev) -> Optional[torch.Tensor]:
    if c is None:
        return None
    c = torch.as_tensor(c, device=dev).to(torch.int32).contiguous()
    if c.numel() != B:
        raise ValueError(f"counts must hold one entry per frame ({B}), got {c.numel()}")
    return c


def _iou(a: torch.Tensor, b: torch.Tensor, mode: str, count_a, count_b) -> torch.Tensor:
    E.require_cuda(a, b)
    if a.dim() != b.dim() or a.dim() not in (2, 3) or a.shape[-1] != 7 or b.shape[-1] != 7:
        raise ValueError(f"boxes must be (N,7) and (M,7), or (B,N,7) and (B,M,7); got {tuple(a.shape)} and {tuple(b.shape)}")
    single = a.dim() == 2
    if single:
        if count_a is not None or count_b is not None:
            raise ValueError("counts belong to batched (B,N,7) inputs")
        a, b = a[None], b[None]
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"batch sizes differ: {a.shape[0]} and {b.shape[0]}")
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    if B == 0 or N == 0 or M == 0:
        out = torch.zeros(B, N, M, device=a.device)
    else:
        out = L.boxes_iou(_f32(a), _f32(b), mode, _counts(count_a, B, a.device), _counts(count_b, B, a.device))
    return out[0] if single else out


def boxes_iou_bev(a: torch.Tensor, b: torch.Tensor, count_a=None, count_b=None) -> torch.Tensor:
    """IoU of the rotated BEV rectangles: intersection area / (area_a + area_b - intersection).  A box with w <= 0 or l <= 0 has
    IoU 0 with everything; every value is finite and in [0, 1], whatever the input."""
    return _iou(a, b, "bev", count_a, count_b)


def boxes_iou3d(a: torch.Tensor, b: torch.Tensor, count_a=None, count_b=None) -> torch.Tensor:
    """3-D IoU: BEV intersection area times the z-overlap / (vol_a + vol_b - intersection volume); h <= 0 gives 0 as well."""
    return _iou(a, b, "3d", count_a, count_b)


def points_in_boxes(points: torch.Tensor, boxes: torch.Tensor, point_counts=None, box_mask=None) -> torch.Tensor:
    """points (B,N,C>=3) fp32, boxes (B,M,7|9) fp32 -> int32 (B,N): the lowest index j of a box of the same frame that contains the
    point, or -1 for none (csrc/gt_paste.hip).  Rows at or past `point_counts[b]` give -1.  `box_mask` (B,M): integer labels (rows < 0
    are ignored) or bool (false rows are ignored).  With d = p - centre rotated by -yaw into (lx, ly), a point is inside iff
    |lx| <= l/2, |ly| <= w/2, |dz| <= h/2 and w, l, h > 0; a NaN anywhere gives not inside.  Unbatched (N,C) / (M,7|9) inputs give
    (N,)."""
    E.require_cuda(points, boxes, box_mask)
    if points.dim() != boxes.dim() or points.dim() not in (2, 3) or points.shape[-1] < 3 or boxes.shape[-1] not in (7, 9):
        raise ValueError(f"points must be (N,C>=3) and boxes (M,7|9), or (B,N,C) and (B,M,7|9); got {tuple(points.shape)} and "
                         f"{tuple(boxes.shape)}")
    if points.dtype != torch.float32 or boxes.dtype != torch.float32:
        raise ValueError(f"points and boxes must be fp32, got {points.dtype} and {boxes.dtype}")
    single = points.dim() == 2
    if single:
        points, boxes = points[None], boxes[None]
        box_mask = None if box_mask is None else box_mask[None]
        point_counts = None if point_counts is None else torch.as_tensor(point_counts).reshape(1)
    if points.shape[0] != boxes.shape[0]:
        raise ValueError(f"batch sizes differ: {points.shape[0]} and {boxes.shape[0]}")
    B, N, Cc = points.shape
    M, ncol = boxes.shape[1], boxes.shape[2]
    mask = None
    if box_mask is not None:
        if tuple(box_mask.shape) != (B, M) or box_mask.dtype.is_floating_point:
            raise ValueError(f"box_mask must be (B,M) = {(B, M)} integer labels or bool, got {tuple(box_mask.shape)} {box_mask.dtype}")
        mask = (box_mask.to(torch.int32) - 1 if box_mask.dtype == torch.bool else box_mask.clamp(min=-1).to(torch.int32)).contiguous()
    out = torch.full((B, N), -1, dtype=torch.int32, device=points.device)
    if B > 0 and N > 0 and M > 0:
        L.points_in_boxes(points.contiguous(), _counts(point_counts, B, points.device), boxes.contiguous(), mask, out, B, N, Cc, M, ncol)
    return out[0] if single else out


def _nms(boxes: torch.Tensor, scores: torch.Tensor, mode: str, thresh: float, labels, pre_max, post_max) -> torch.Tensor:
    E.require_cuda(boxes, scores, labels)
    if boxes.dim() != 2 or boxes.shape[1] != 7 or scores.shape != boxes.shape[:1]:
        raise ValueError(f"boxes must be (N,7) and scores (N,); got {tuple(boxes.shape)} and {tuple(scores.shape)}")
    if labels is not None and labels.shape != scores.shape:
        raise ValueError(f"labels must be (N,) like scores, got {tuple(labels.shape)}")
    if not float(thresh) >= 0.0:
        raise ValueError(f"the NMS threshold / radius must be >= 0, got {thresh}")
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    scores = scores.detach().float()
    order = None
    if n > 1 and not bool((scores[1:] <= scores[:-1]).all()):
        order = torch.sort(scores, descending=True, stable=True).indices        # ties: the lower index first
    if pre_max is not None:
        if int(pre_max) <= 0:
            raise ValueError("pre_max must be positive")
        if int(pre_max) < n:
            order = (torch.arange(n, device=boxes.device) if order is None else order)[:int(pre_max)]
    b = _f32(boxes if order is None else boxes[order])
    lab = None
    if labels is not None:
        lab = (labels if order is None else labels[order]).to(torch.int64).contiguous()[None]
    m = b.shape[0]
    post = m if post_max is None else int(post_max)
    if post <= 0:
        raise ValueError("post_max must be positive")
    keep_idx, keep_count = L.nms_boxes(b[None], None, mode, float(thresh), min(post, m), labels=lab, class_aware=lab is not None)
    keep = keep_idx[0, :int(keep_count[0])].long()
    return keep if order is None else order[keep]


def nms_rotated(boxes: torch.Tensor, scores: torch.Tensor, iou_thresh: float, labels: Optional[torch.Tensor] = None,
                pre_max: Optional[int] = None, post_max: Optional[int] = None) -> torch.Tensor:
    """Greedy rotated-IoU NMS of one frame: a box is dropped when a kept box of higher score has IoU_bev > iou_thresh with it (and,
    with `labels`, the same label).  Only the pre_max best boxes take part; at most post_max indices come back.  Returns int64
    indices into `boxes`, in descending score order.  At most 4096 boxes take part."""
    return _nms(boxes, scores, "rotate", iou_thresh, labels, pre_max, post_max)


def nms_circle(boxes: torch.Tensor, scores: torch.Tensor, radius: float, labels: Optional[torch.Tensor] = None,
               pre_max: Optional[int] = None, post_max: Optional[int] = None) -> torch.Tensor:
    """CenterPoint's circle NMS: as nms_rotated, but a box is dropped when its centre lies closer than `radius` metres to a kept
    box's centre."""
    return _nms(boxes, scores, "circle", radius, labels, pre_max, post_max)


def check_nms_args(nms_type, nms_iou_thresh, nms_radius, nms_pre_max, class_aware: bool, true_labels: bool) -> None:
    """Argument validation of the decode's NMS keywords (raises ValueError)."""
    if nms_type not in NMS_TYPES:
        raise ValueError(f"nms_type must be None, 'rotate' or 'circle', got {nms_type!r}")
    if class_aware and not true_labels:
        raise ValueError("class_aware=True needs true_labels=True: the reference's labels are all 0, so a class-aware NMS over "
                         "them would be the class-agnostic one")
    if nms_type is None:
        return
    if int(nms_pre_max) <= 0:
        raise ValueError(f"nms_pre_max must be positive, got {nms_pre_max}")
    if nms_type == "circle":
        if nms_radius is None or not float(nms_radius) > 0.0:
            raise ValueError("nms_type='circle' needs nms_radius (metres, > 0)")
    elif not 0.0 <= float(nms_iou_thresh) <= 1.0:
        raise ValueError(f"nms_iou_thresh must lie in [0, 1], got {nms_iou_thresh}")


def decode_settings(config: Dict[str, Any], section: str = "inference") -> Dict[str, Any]:
    """Keyword arguments for `decode_centernet_predictions` from `<section>.post_processing` of a reference-style YAML (as a
    dict): score_threshold -> score_thresh, max_detections -> max_detections, nms_threshold -> nms_iou_thresh with
    nms_type='rotate', iou_rectify -> iou_rectify (a float or a list of floats).  Missing keys keep the decode's defaults."""
    try:
        pp = config[section]["post_processing"]
    except (KeyError, TypeError):
        raise KeyError(f"the config has no '{section}.post_processing' section") from None
    out: Dict[str, Any] = {"nms_type": "rotate"}
    for key, name, cast in (("score_threshold", "score_thresh", float), ("max_detections", "max_detections", int),
                            ("nms_threshold", "nms_iou_thresh", float)):
        if key in pp:
            out[name] = cast(pp[key])
    if pp.get("iou_rectify") is not None:             # IoU-aware score rectification: one exponent, or one per class
        r = pp["iou_rectify"]
        out["iou_rectify"] = float(r) if isinstance(r, (int, float)) else [float(a) for a in r]
    return out
