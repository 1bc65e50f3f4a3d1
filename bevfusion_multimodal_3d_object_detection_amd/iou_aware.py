"""IoU-aware detection head, training and decode side (csrc/iou_loss.hip, csrc/decode.hip).

The heatmap score says how sure the head is of a class at a cell, not how well the regressed box fits.  CenterPoint's IoU-aware
variant (also PillarNet, VoxelNeXt) adds three parts, all opt-in here:

* `iou_head.IoUHead` regresses `2 * IoU - 1` of the cell's box with its ground truth (the detector's 'iou' output);
* `IoUAwareLoss` trains it -- L1 against `iou_targets` -- and adds an aligned distance-IoU term to the box regression;
* `decode_centernet_predictions(..., iou_rectify=alpha)` scores a peak `s^(1 - alpha) * q^alpha`, `q = clamp((iou + 1) / 2, 0, 1)`.

For every object (b, k) with `reg_mask[b, k]` set, at the cell `ind = cy * W + cx` and with cells of
`vx = (pc_range[3] - pc_range[0]) / W` by `vy = (pc_range[4] - pc_range[1]) / H` (the targets' convention):

* predicted box: `x = (cx + offset[b, 0, cell]) * vx + x_min`, y likewise, `w = size[b, 0, cell]`, `l = size[b, 1, cell]`,
  `yaw = atan2(rot[b, 0, cell], rot[b, 1, cell])` -- the decode's assembly; GT box: the same from `target_offset`, `target_size`,
  `target_rot`;
* `t = 2 * IoU_bev(pred, gt) - 1`, the rotated BEV IoU of `box_ops` on the raw sizes (a size <= 0 gives IoU 0, as the NMS sees it);
* `iou_loss = sum |iou[b, 0, cell] - t| / (sum reg_mask + 1e-4)`; t is a constant, so no gradient reaches the boxes through it;
* `diou_loss = sum (1 - d) / (sum reg_mask + 1e-4)`, `d = inter / (union + 1e-6) - rho^2 / (c^2 + 1e-6)` of the GT rectangle and the
  predicted one taken parallel to it in the GT box's frame, predicted sizes clamped below at 1e-3 (OpenPCDet's aligned DIoU; it
  does not change under a common rotation of both boxes).  Gradients reach `offset` and `size[:, 0:2]` only.

Everything runs on the GPU, reads nothing back and is graph-capturable; two runs give the same bits (no float atomics).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E

PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)

_PRED_KEYS = ("offset", "size", "rot")
_TGT_KEYS = ("target_offset", "target_size", "target_rot", "ind", "reg_mask")


def _check(what: str, predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor], need_iou: bool) -> None:
    """Key, device and rank checks; the wrappers in _lib check the shapes against each other."""
    for name, d, keys in (("predictions", predictions, (("iou",) if need_iou else ()) + _PRED_KEYS), ("targets", targets, _TGT_KEYS)):
        missing = [k for k in keys if k not in d]
        if missing:
            hint = " (build the detector with iou_head=True)" if "iou" in missing else ""
            raise L.BevfError(f"{what}: {name} lack {missing}{hint}")
    if predictions["offset"].dim() != 4 or targets["ind"].dim() != 2:
        raise ValueError(f"{what}: offset must be (B,2,H,W) and ind (B,max_objects), got {tuple(predictions['offset'].shape)} and "
                         f"{tuple(targets['ind'].shape)}")
    if predictions["offset"].shape[0] != targets["ind"].shape[0]:
        raise ValueError(f"{what}: predictions hold {predictions['offset'].shape[0]} frames, targets {targets['ind'].shape[0]}")
    E.require_cuda(*[predictions[k] for k in (("iou",) if need_iou else ()) + _PRED_KEYS], *[targets[k] for k in _TGT_KEYS])


def _range(pc_range: Sequence[float]) -> tuple:
    r = tuple(float(v) for v in pc_range)
    if len(r) != 6 or not (r[3] > r[0] and r[4] > r[1]):
        raise ValueError(f"pc_range must be [xmin, ymin, zmin, xmax, ymax, zmax] with a non-empty x / y extent, got {list(pc_range)}")
    return r


def iou_targets(predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor],
                pc_range: Sequence[float] = PC_RANGE) -> torch.Tensor:
    """(B, max_objects) fp32: `2 * IoU_bev(predicted box, GT box) - 1` where reg_mask is set and 0 elsewhere -- what the 'iou'
    output regresses at the object's cell.  The loss kernels share this device code."""
    _check("iou_targets", predictions, targets, False)
    with torch.no_grad():
        return L.iou_targets(predictions, targets, _range(pc_range))


class _IoULossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pc_range, weights, tgt_keys, iou, offset, size, rot, *tgt):
        preds = dict(iou=iou, offset=offset, size=size, rot=rot)
        tgts = dict(zip(tgt_keys, tgt))
        vals = L.iou_aware_loss(preds, tgts, pc_range, *weights)
        ctx.preds, ctx.tgts, ctx.pc_range, ctx.weights = preds, tgts, pc_range, weights
        ctx.set_materialize_grads(False)                   # unused terms arrive as None: the check below reads nothing back
        return tuple(vals[i].clone() for i in range(3))

    @staticmethod
    def backward(ctx, g_total, *g_rest):
        for g in g_rest:
            if g is not None and bool((g != 0).any()):
                raise NotImplementedError("backward through the individual loss terms is not built; use total_loss")
        p = ctx.preds
        d_iou, d_off, d_size = (torch.zeros_like(p[n], dtype=torch.float32) for n in ("iou", "offset", "size"))
        L.iou_aware_loss_bwd(p, ctx.tgts, ctx.pc_range, *ctx.weights, d_iou, d_off, d_size)
        gt = g_total if g_total is not None else torch.zeros((), device=d_iou.device)
        return (None, None, None, d_iou * gt, d_off * gt, d_size * gt, None, *([None] * len(ctx.tgts)))


class IoUAwareLoss(nn.Module):
    """`IoUAwareLoss()(predictions, targets)` -> {'total_loss', 'iou_loss', 'diou_loss'} with
    `total_loss = iou_weight * iou_loss + diou_weight * diou_loss` (module docstring).  `predictions` is the output of a detector
    built with `iou_head=True` ('iou', 'offset', 'size', 'rot' are read), `targets` that of `prepare_centernet_targets` with the
    same `pc_range`.  Sum `total_loss` with CenterNetLoss's: the two gradients on offset / size add in autograd.  The backward runs
    through total_loss only."""

    def __init__(self, iou_weight: float = 1.0, diou_weight: float = 1.0, pc_range: Sequence[float] = PC_RANGE):
        super().__init__()
        self.iou_weight, self.diou_weight = float(iou_weight), float(diou_weight)
        self.pc_range = _range(pc_range)

    def forward(self, predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        _check("IoUAwareLoss", predictions, targets, True)
        w = (self.iou_weight, self.diou_weight)
        names = ("total_loss", "iou_loss", "diou_loss")
        if torch.is_grad_enabled() and any(predictions[k].requires_grad for k in ("iou",) + _PRED_KEYS):
            vals = _IoULossFn.apply(self.pc_range, w, _TGT_KEYS, *[predictions[k] for k in ("iou",) + _PRED_KEYS],
                                    *[targets[k] for k in _TGT_KEYS])
            return dict(zip(names, vals))
        with torch.no_grad():
            vals = L.iou_aware_loss(predictions, targets, self.pc_range, *w)
        return {n: vals[i] for i, n in enumerate(names)}


def rectify_alpha(iou_rectify: Union[None, float, Sequence[float]], num_classes: int) -> Optional[list]:
    """The decode's `iou_rectify=` keyword -> None (off) or the per-class exponents as a list of num_classes floats in [0, 1]; raises
    ValueError for anything else."""
    if iou_rectify is None:
        return None
    if isinstance(iou_rectify, bool):
        raise ValueError("iou_rectify must be None, a float in [0, 1] or one float per class, got a bool")
    if isinstance(iou_rectify, (int, float)):
        alpha = [float(iou_rectify)] * int(num_classes)
    else:
        try:
            alpha = [float(a) for a in (iou_rectify.tolist() if isinstance(iou_rectify, torch.Tensor) else iou_rectify)]
        except TypeError:
            raise ValueError(f"iou_rectify must be None, a float or a sequence of floats, got {type(iou_rectify).__name__}") from None
        if len(alpha) != int(num_classes):
            raise ValueError(f"iou_rectify names {len(alpha)} exponents, the heatmap has {num_classes} classes")
    if not all(0.0 <= a <= 1.0 for a in alpha):                        # (NaN fails the comparison too)
        raise ValueError(f"iou_rectify must lie in [0, 1], got {alpha}")
    return alpha
