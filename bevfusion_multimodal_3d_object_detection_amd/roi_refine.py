"""CenterPoint's second stage, training and decode side (csrc/roi_head.hip): the RoI targets, the loss of
`roi_head.RoIHead` and the refine step that turns its output into the detector's final padded records.

RoIs are the dict of `centernet_target.decode_padded`: 'boxes' (B, K, 7) = (x, y, z, w, l, h, yaw), 'velocities', 'scores', 'labels'
and 'count' int32 (B,); rows past count[b] are never read.  For a RoI and its best ground-truth box (the highest rotated 3-D IoU, the
lowest index among equals), with `d = gt - roi`, `c, s = cos, sin` of the RoI's yaw and `diag = sqrt(l^2 + w^2)` of the RoI:

* `cls_target = clamp(2 * iou - 0.5, 0, 1)`; `reg_mask = iou >= reg_fg_thresh` (0.55) and all six sizes > 0;
* `reg_target = ((c dx + s dy) / diag, (c dy - s dx) / diag, dz / h, log(w_g / w), log(l_g / l), log(h_g / h), dyaw)` where reg_mask
  is set (zeros elsewhere), `dyaw = yaw_g - yaw` wrapped into [-pi, pi) and folded into [-pi / 2, pi / 2] by -+ pi: opposite
  headings count as the same box (OpenPCDet's rule);
* `cls_loss = sum BCEWithLogits(logit, cls_target) / (n_valid + 1e-4)`, `reg_loss = sum_{reg_mask} sum_7 |residual - reg_target| /
  (n_fg + 1e-4)` over the rows below count (every one of them trains: no RoI sampling);
* refine: the inverse encoding, `score' = sqrt(score * sigmoid(logit))`, rows compacted in descending `score'` (ties by RoI index).

Everything runs on the GPU, reads nothing back and is graph-capturable; two runs give the same bits (no float atomics).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E
from .roi_head import check_rois

REG_FG_THRESH = 0.55


def pad_gt(batch, device, max_objects: int = 500) -> tuple:
    """batch['gt_boxes'] / ['gt_labels'] -- per-frame (M, >= 7) boxes and (M,) labels (-1 = padding), lists or stacked tensors --
    padded on the host the way prepare_centernet_targets pads them -> (gt (B, M, 7) fp32, gt_labels int32 (B, M)) on `device`."""
    boxes_l, labels_l = batch["gt_boxes"], batch["gt_labels"]
    B = len(boxes_l)
    nmax = max([min(len(b), max_objects) for b in boxes_l] + [1])
    boxes = torch.zeros(B, nmax, 7, dtype=torch.float32)
    labels = torch.full((B, nmax), -1, dtype=torch.int32)
    for b in range(B):
        bb = torch.as_tensor(boxes_l[b]).detach().float().cpu()
        ll = torch.as_tensor(labels_l[b]).detach().cpu()
        n = min(len(bb), max_objects)
        if n:
            boxes[b, :n] = bb[:n, :7]
            labels[b, :n] = ll[:n].to(torch.int32)
    return boxes.to(device), labels.to(device)


def roi_targets(rois: Dict[str, torch.Tensor], gt, *, iou: str = "3d", match_labels: bool = False,
                reg_fg_thresh: float = REG_FG_THRESH, max_objects: int = 500) -> Dict[str, torch.Tensor]:
    """The targets of every RoI (module docstring) -> {'iou', 'cls_target' (B, K), 'gt_index' int32 (B, K), 'reg_mask' uint8 (B, K),
    'reg_target' (B, K, 7), 'count'}; rows past the count are zeros with gt_index -1.  `gt`: a batch dict with 'gt_boxes' /
    'gt_labels' lists (padded on the host as prepare_centernet_targets does), or ready device tensors (gt (B, M, 7) fp32, gt_labels
    int32 (B, M), -1 = padding).  iou: '3d' (default) or 'bev'.  match_labels: only a ground-truth box with the RoI's label
    (rois['labels']) is a candidate."""
    if iou not in ("3d", "bev"):
        raise ValueError(f"roi_targets: iou must be '3d' or 'bev', got {iou!r}")
    boxes, count = check_rois("roi_targets", rois)
    if isinstance(gt, dict):
        g, gl = pad_gt(gt, boxes.device, max_objects)
    else:
        try:
            g, gl = gt
        except (TypeError, ValueError):
            raise L.BevfError("roi_targets: gt must be a batch dict with 'gt_boxes' / 'gt_labels' or a (gt, gt_labels) pair") from None
        E.require_cuda(g, gl)
    labels = None
    if match_labels:
        if "labels" not in rois:
            raise L.BevfError("roi_targets: match_labels needs rois['labels']")
        labels = rois["labels"].contiguous()
    with torch.no_grad():
        return L.roi_targets(boxes, count, labels, g.contiguous(), gl.contiguous(), iou == "bev", match_labels, reg_fg_thresh)


def as_pred(head_out) -> torch.Tensor:
    """RoIHead's output -> the (B, K, 8) tensor the kernels read: the logit, then the residual (differentiable)."""
    if isinstance(head_out, torch.Tensor):
        pred = head_out
    else:
        missing = [k for k in ("logit", "residual") if k not in head_out]
        if missing:
            raise L.BevfError(f"the RoI head's output lacks {missing}")
        pred = torch.cat([head_out["logit"].unsqueeze(-1), head_out["residual"]], -1)
    if pred.dim() != 3 or pred.shape[2] != 8:
        raise L.BevfError(f"the RoI head's output must be (B, K) logits with (B, K, 7) residuals, got {tuple(pred.shape)} together")
    E.require_cuda(pred)
    return pred


class _RoILossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, tgt, pred):
        pred = pred.detach().float().contiguous()
        vals = L.roi_loss(pred, tgt, *weights)
        ctx.pred, ctx.tgt, ctx.weights = pred, tgt, weights
        ctx.set_materialize_grads(False)                   # unused terms arrive as None: the check below reads nothing back
        return tuple(vals[i].clone() for i in range(3))

    @staticmethod
    def backward(ctx, g_total, *g_rest):
        for g in g_rest:
            if g is not None and bool((g != 0).any()):
                raise NotImplementedError("backward through the individual loss terms is not built; use total_loss")
        dpred = torch.empty_like(ctx.pred)
        L.roi_loss_bwd(ctx.pred, ctx.tgt, *ctx.weights, dpred)
        gt = g_total if g_total is not None else torch.zeros((), device=dpred.device)
        return None, None, dpred * gt


class RoIHeadLoss(nn.Module):
    """`RoIHeadLoss()(head_out, targets)` -> {'total_loss', 'cls_loss', 'reg_loss'} with
    `total_loss = cls_weight * cls_loss + reg_weight * reg_loss` (module docstring).  `head_out` is RoIHead's output, `targets` that
    of `roi_targets` for the same RoIs.  The backward runs through total_loss only."""

    def __init__(self, cls_weight: float = 1.0, reg_weight: float = 1.0):
        super().__init__()
        self.cls_weight, self.reg_weight = float(cls_weight), float(reg_weight)

    def forward(self, head_out, targets: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        pred = as_pred(head_out)
        w = (self.cls_weight, self.reg_weight)
        names = ("total_loss", "cls_loss", "reg_loss")
        if torch.is_grad_enabled() and pred.requires_grad:
            return dict(zip(names, _RoILossFn.apply(w, targets, pred)))
        with torch.no_grad():
            vals = L.roi_loss(pred.detach().float().contiguous(), targets, *w)
        return {n: vals[i] for i, n in enumerate(names)}


def refine_padded(rois: Dict[str, torch.Tensor], head_out, score_thresh: float = 0.0) -> Dict[str, torch.Tensor]:
    """The refine step (module docstring) -> a dict of decode_padded's form: {'boxes', 'velocities', 'scores', 'labels', 'count'},
    each frame's kept rows first, in descending final score (what `tracking.Tracker.step` and the box NMS expect), zeros behind
    them.  Rows whose final score is not finite or below score_thresh are dropped."""
    boxes, count = check_rois("refine_padded", rois)
    missing = [k for k in ("scores", "labels") if k not in rois]
    if missing:
        raise L.BevfError(f"refine_padded: rois lack {missing}")
    with torch.no_grad():
        pred = as_pred(head_out).detach().float().contiguous()
        vel: Optional[torch.Tensor] = rois.get("velocities")
        return L.roi_refine(boxes, rois["scores"].contiguous(), rois["labels"].contiguous(),
                            vel.contiguous() if vel is not None else None, count, pred, float(score_thresh))
