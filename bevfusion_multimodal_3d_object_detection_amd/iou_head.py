"""IoU-aware head (opt-in): one more CenterNetHead-shaped branch on the fused BEV map that regresses, per cell, how
well the box regressed there fits its ground truth.

`IoUHead` is `branch = conv3x3(+bias) + ReLU + conv1x1(+bias)` -> (B, 1, H, W) fp32 with no activation; the value means
`2 * IoU - 1`.  `iou_aware.IoUAwareLoss` trains it, the decode's `iou_rectify=` uses it.  The detector owns a head when built with
`iou_head=` (fusion.py) and then returns 'iou' beside the detection tensors.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E
from .encoders import _cfg


def iou_head_settings(iou_head, config) -> Optional[dict]:
    """The detector's `iou_head=` keyword (True / False / dict / None) and the config's model.iou_head -> the keyword arguments of
    IoUHead the two spell out (the keyword's entries win), or None when the head is off.  None = the config decides
    (model.iou_head.enable), False = off whatever the config says."""
    sc = ((config or {}).get("model", {}) or {}).get("iou_head", {}) or {}
    if isinstance(sc, bool):
        sc = dict(enable=sc)
    if iou_head is None:
        if not sc.get("enable", False):
            return None
        iou_head = {}
    elif iou_head is False:
        return None
    elif iou_head is True:
        iou_head = {}
    elif not isinstance(iou_head, dict):
        raise L.BevfError(f"iou_head must be True, False, None or a dict of IoUHead settings, got {type(iou_head).__name__}")
    known = ("head_conv",)
    unknown = sorted(set(iou_head) - set(known) - {"enable"})
    if unknown:
        raise L.BevfError(f"iou_head: unknown settings {unknown} (known: {list(known)})")
    merged = {k: sc[k] for k in known if k in sc}
    merged.update({k: v for k, v in iou_head.items() if k in known})
    if iou_head.get("enable", True) is False:
        return None
    return merged


class IoUHead(nn.Module):
    """`branch` = Conv2d(in_channels, head_conv, 3, padding=1) + ReLU + Conv2d(head_conv, 1, 1): the shape and the init (weights
    N(0, 0.001), biases 0) of one CenterNetHead branch.  forward: (B, in_channels, H, W) -> (B, 1, H, W) fp32, read as 2 * IoU - 1.
    Eval mode runs the packed convolution kernels (engine.IoUHeadEngine; fp32 or bf16 storage), train mode the tape
    (training.IoUHeadTape; fp32) with gradients for the parameters and the input map."""

    def __init__(self, in_channels: Optional[int] = None, head_conv: Optional[int] = None, config: Optional[Dict] = None,
                 config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        mc = (config or {}).get("model", {}) or {}
        sc, hc, bc = (mc.get("iou_head", {}) or {}), (mc.get("centernet_head", {}) or {}), (mc.get("bev_fusion", {}) or {})
        if isinstance(sc, bool):
            sc = {}
        if in_channels is None:
            in_channels = sc.get("in_channels", hc.get("in_channels", bc.get("bev_channels", 256)))
        if head_conv is None:
            head_conv = sc.get("head_conv", hc.get("head_conv", 64))
        self.in_channels, self.head_conv = int(in_channels), int(head_conv)
        if self.in_channels <= 0 or self.head_conv <= 0:
            raise L.BevfError(f"IoUHead: in_channels and head_conv must be positive, got {in_channels} and {head_conv}")
        self.branch = nn.Sequential(nn.Conv2d(self.in_channels, self.head_conv, 3, padding=1, bias=True), nn.ReLU(inplace=True),
                                    nn.Conv2d(self.head_conv, 1, 1, bias=True))
        for m in self.branch:
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.001)
                nn.init.constant_(m.bias, 0)
        self._engine = None

    def _eng(self) -> "E.IoUHeadEngine":
        if self._engine is None:
            self._engine = E.IoUHeadEngine(self)
        return self._engine

    def forward_nhwc(self, bev_nhwc: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        """Eval-mode fast path on the flat NHWC fused map in the storage dtype -> (B, 1, H, W) fp32."""
        return self._eng().run(bev_nhwc, B, H, W)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.in_channels:
            got = tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__
            raise L.BevfError(f"IoUHead: expected a (B, {self.in_channels}, H, W) BEV map, got {got}")
        E.require_cuda(x)
        if self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if self._eng().dtype != torch.float32:
                raise L.BevfError(f"IoUHead: {self._eng().dtype} storage in train mode is not supported (the training tape is fp32); "
                                  "call .eval() for bf16 inference")
            from . import training                      # no BatchNorm in the head: same values as eval mode, plus a gradient path
            return training.iou_head_train_forward(self, x)
        with torch.no_grad():
            B, _, H, W = x.shape
            return self.forward_nhwc(E.to_nhwc(x.float()).to(self._eng().dtype), B, H, W)
