"""CenterPoint's second stage (opt-in): for every first-stage box the BEV feature map is sampled at the box centre
and at its four face centres, and a small MLP turns the five feature vectors into a class-agnostic confidence and a box refinement.

`RoIHead` is `shared_fc = (Linear(no bias) + BatchNorm1d + ReLU) x 2`, `cls_out = Linear(fc, 1)`, `reg_out = Linear(fc, 7)`.
`roi_refine.RoIHeadLoss` trains it against `roi_refine.roi_targets`, `roi_refine.refine_padded` applies it.  The detector owns a head
when built with `roi_head=` (fusion.py); it then returns 'feat', the map its heads read, and `model.refine(out)` runs
decode -> RoI head -> refine on the device.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E
from .encoders import _cfg

PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)

_KNOWN = ("fc",)


def roi_head_settings(roi_head, config) -> Optional[dict]:
    """The detector's `roi_head=` keyword (True / False / dict / None) and the config's model.roi_head -> the keyword arguments of
    RoIHead the two spell out (the keyword's entries win), or None when the head is off.  None = the config decides
    (model.roi_head.enable), False = off whatever the config says."""
    sc = ((config or {}).get("model", {}) or {}).get("roi_head", {}) or {}
    if isinstance(sc, bool):
        sc = dict(enable=sc)
    if roi_head is None:
        if not sc.get("enable", False):
            return None
        roi_head = {}
    elif roi_head is False:
        return None
    elif roi_head is True:
        roi_head = {}
    elif not isinstance(roi_head, dict):
        raise L.BevfError(f"roi_head must be True, False, None or a dict of RoIHead settings, got {type(roi_head).__name__}")
    unknown = sorted(set(roi_head) - set(_KNOWN) - {"enable"})
    if unknown:
        raise L.BevfError(f"roi_head: unknown settings {unknown} (known: {list(_KNOWN)})")
    merged = {k: sc[k] for k in _KNOWN if k in sc}
    merged.update({k: v for k, v in roi_head.items() if k in _KNOWN})
    if roi_head.get("enable", True) is False:
        return None
    return merged


def check_rois(what: str, rois) -> tuple:
    """The padded records of `decode_padded` -> (boxes (B,K,7) fp32, count int32 (B,)), checked."""
    if not isinstance(rois, dict) or "boxes" not in rois or "count" not in rois:
        raise L.BevfError(f"{what}: rois must be the dict of centernet_target.decode_padded ('boxes' (B,K,7) and 'count' (B,) at least)")
    boxes, count = rois["boxes"], rois["count"]
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.shape[2] != 7 or boxes.dtype != torch.float32:
        got = f"{boxes.dtype} {tuple(boxes.shape)}" if isinstance(boxes, torch.Tensor) else type(boxes).__name__
        raise L.BevfError(f"{what}: rois['boxes'] must be a float32 (B,K,7) tensor, got {got}")
    if not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or tuple(count.shape) != (boxes.shape[0],):
        got = f"{count.dtype} {tuple(count.shape)}" if isinstance(count, torch.Tensor) else type(count).__name__
        raise L.BevfError(f"{what}: rois['count'] must be an int32 ({boxes.shape[0]},) tensor, got {got}")
    E.require_cuda(boxes, count)
    return boxes.contiguous(), count.contiguous()


class RoIHead(nn.Module):
    """`shared_fc` = Linear(5 * in_channels, fc, bias=False) + BatchNorm1d + ReLU, twice; `cls_out` = Linear(fc, 1), `reg_out` =
    Linear(fc, 7); no dropout.  Init: Linear weights xavier-normal, reg_out N(0, 0.001), biases 0 (OpenPCDet's RoI heads).
    forward(feat_map (B, in_channels, H, W), rois) -> {'logit' (B, K), 'residual' (B, K, 7)} fp32; rows past rois['count'] carry no
    meaning.  `pc_range` says which metres the map covers (x / y extent; cells as the targets count them).
    Eval mode runs the gather and the packed 1x1 convolution kernels (engine.RoIHeadEngine; fp32 or bf16 storage), train mode the
    tape (training.RoIHeadTape; fp32) with gradients for the parameters and, when it requires one, for the map."""

    def __init__(self, in_channels: Optional[int] = None, fc: Optional[int] = None, pc_range: Optional[Sequence[float]] = None,
                 config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        mc = (config or {}).get("model", {}) or {}
        sc, hc, bc = (mc.get("roi_head", {}) or {}), (mc.get("centernet_head", {}) or {}), (mc.get("bev_fusion", {}) or {})
        if isinstance(sc, bool):
            sc = {}
        if in_channels is None:
            in_channels = sc.get("in_channels", hc.get("in_channels", bc.get("bev_channels", 256)))
        if fc is None:
            fc = sc.get("fc", 256)
        self.in_channels, self.fc = int(in_channels), int(fc)
        if self.in_channels <= 0 or self.fc <= 0 or self.fc % 4:
            raise L.BevfError(f"RoIHead: in_channels must be positive and fc a positive multiple of 4, got {in_channels} and {fc}")
        if self.fc > 1024:
            raise L.BevfError(f"RoIHead: fc={fc} exceeds the row BatchNorm kernels' 1024 channels")
        r = tuple(float(v) for v in (PC_RANGE if pc_range is None else pc_range))
        if len(r) != 6 or not (r[3] > r[0] and r[4] > r[1]):
            raise L.BevfError(f"RoIHead: pc_range must be [xmin, ymin, zmin, xmax, ymax, zmax] with a non-empty x / y extent, got {list(r)}")
        self.pc_range = r
        self.shared_fc = nn.Sequential(nn.Linear(5 * self.in_channels, self.fc, bias=False), nn.BatchNorm1d(self.fc), nn.ReLU(inplace=True),
                                       nn.Linear(self.fc, self.fc, bias=False), nn.BatchNorm1d(self.fc), nn.ReLU(inplace=True))
        self.cls_out = nn.Linear(self.fc, 1)
        self.reg_out = nn.Linear(self.fc, 7)
        for m in (self.shared_fc[0], self.shared_fc[3], self.cls_out):
            nn.init.xavier_normal_(m.weight)
        nn.init.normal_(self.reg_out.weight, std=0.001)
        nn.init.constant_(self.cls_out.bias, 0)
        nn.init.constant_(self.reg_out.bias, 0)
        self._engine = None

    @property
    def bev_range(self) -> tuple:
        """(x_min, y_min, x_max, y_max) of the map."""
        r = self.pc_range
        return (r[0], r[1], r[3], r[4])

    def _eng(self) -> "E.RoIHeadEngine":
        if self._engine is None:
            self._engine = E.RoIHeadEngine(self)
        return self._engine

    def forward_nhwc(self, bev_nhwc: torch.Tensor, B: int, H: int, W: int, rois) -> torch.Tensor:
        """Eval-mode fast path on the flat NHWC map in the storage dtype -> pred (B, K, 8) fp32: the logit, then the residual."""
        boxes, count = check_rois("RoIHead", rois)
        if boxes.shape[0] != B or boxes.shape[1] == 0:
            raise L.BevfError(f"RoIHead: the map holds {B} frames, the RoIs are {tuple(boxes.shape)}")
        return self._eng().run(bev_nhwc, boxes, count, B, boxes.shape[1], H, W, self.bev_range)

    def predict(self, feat_map: torch.Tensor, rois) -> torch.Tensor:
        """forward as one (B, K, 8) tensor: the logit, then the seven residuals."""
        if not isinstance(feat_map, torch.Tensor) or feat_map.dim() != 4 or feat_map.shape[1] != self.in_channels:
            got = tuple(feat_map.shape) if isinstance(feat_map, torch.Tensor) else type(feat_map).__name__
            raise L.BevfError(f"RoIHead: expected a (B, {self.in_channels}, H, W) BEV map, got {got}")
        E.require_cuda(feat_map)
        boxes, count = check_rois("RoIHead", rois)
        B, _, H, W = feat_map.shape
        if boxes.shape[0] != B or boxes.shape[1] == 0:
            raise L.BevfError(f"RoIHead: the map holds {B} frames, the RoIs are {tuple(boxes.shape)}")
        from . import training
        if self.training and (torch.is_grad_enabled() or training.any_bn_training(self)):
            if self._eng().dtype != torch.float32:
                raise L.BevfError(f"RoIHead: {self._eng().dtype} storage in train mode is not supported (the training tape is fp32); "
                                  "call .eval() for bf16 inference")
            return training.roi_head_train_forward(self, feat_map, boxes, count, self.bev_range)
        with torch.no_grad():
            dt = self._eng().dtype
            rows = feat_map.permute(0, 2, 3, 1)
            if feat_map.dtype == dt and rows.is_contiguous():      # channels-last already (the detector's 'feat'): no copy
                flat = rows.reshape(-1)
            else:
                flat = E.to_nhwc(feat_map.float()).to(dt)
            return self._eng().run(flat, boxes, count, B, boxes.shape[1], H, W, self.bev_range)

    def forward(self, feat_map: torch.Tensor, rois) -> Dict[str, torch.Tensor]:
        pred = self.predict(feat_map, rois)
        return {"logit": pred[..., 0], "residual": pred[..., 1:]}
