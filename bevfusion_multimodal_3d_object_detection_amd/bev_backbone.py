"""BEV backbone + FPN neck (opt-in): the decoder between the BEV fuser and the heads.

`BEVBackbone` is the SECOND multi-scale backbone (per level one strided 3x3 convolution and n plain ones, each with BatchNorm and
ReLU) followed by the SECONDFPN neck (per level one kernel = stride transposed convolution back to the input grid, BatchNorm, ReLU,
then the channel concat).  The convolutions run on the package's convolution kernels, the transposed convolutions on
csrc/deconv.hip, whose store goes straight into the level's channel slice of the concat.  The detector owns one when built with
`bev_backbone=` (fusion.py); every head then reads its output instead of the fused map.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E

KNOWN = ("layer_nums", "layer_strides", "out_channels", "upsample_strides", "upsample_channels", "bn_eps", "bn_momentum")


def bev_backbone_settings(bev_backbone, config) -> Optional[dict]:
    """The detector's `bev_backbone=` keyword (True / False / dict / None) and the config's model.bev_backbone -> the keyword
    arguments of BEVBackbone the two spell out (the keyword's entries win), or None when it is off.  None = the config decides
    (model.bev_backbone.enable), False = off whatever the config says."""
    bc = ((config or {}).get("model", {}) or {}).get("bev_backbone", {}) or {}
    if isinstance(bc, bool):
        bc = dict(enable=bc)
    if bev_backbone is None:
        if not bc.get("enable", False):
            return None
        bev_backbone = {}
    elif bev_backbone is False:
        return None
    elif bev_backbone is True:
        bev_backbone = {}
    elif not isinstance(bev_backbone, dict):
        raise L.BevfError(f"bev_backbone must be True, False, None or a dict of BEVBackbone settings, got {type(bev_backbone).__name__}")
    unknown = sorted(set(bev_backbone) - set(KNOWN) - {"enable"})
    if unknown:
        raise L.BevfError(f"bev_backbone: unknown settings {unknown} (known: {list(KNOWN)})")
    if bev_backbone.get("enable", True) is False:
        return None
    merged = {k: bc[k] for k in KNOWN if k in bc}
    merged.update({k: v for k, v in bev_backbone.items() if k in KNOWN})
    return merged


def _ints(name: str, v) -> tuple:
    try:
        return tuple(int(a) for a in v)
    except (TypeError, ValueError):
        raise L.BevfError(f"BEVBackbone: {name} must be a sequence of integers, got {v!r}") from None


class BEVBackbone(nn.Module):
    """(B, in_channels, H, W) -> (B, sum(upsample_channels), H, W).

    backbone.blocks[i] = Sequential(Conv2d(3x3, stride layer_strides[i], pad 1, no bias), BN, ReLU, layer_nums[i] x (Conv2d 3x3 +
    BN + ReLU)); neck.deblocks[i] = Sequential(ConvTranspose2d(out_channels[i], upsample_channels[i], kernel = stride =
    upsample_strides[i], no bias), BN, ReLU).  The attribute names are those of the SECOND / SECONDFPN pair of published BEV
    detectors: their tensors map onto this module by a prefix rename.  Every level returns to the input grid:
    upsample_strides[i] == prod(layer_strides[:i+1]), each 1, 2 or 4; H and W are multiples of the largest; channel counts are
    multiples of 32.  Eval mode runs engine.BackboneEngine (folded BatchNorm, fp32 or bf16 storage), train mode the tape
    (training.BackboneTape, fp32): batch statistics and gradients for the parameters and the input map."""

    def __init__(self, in_channels: int, layer_nums: Sequence[int] = (5, 5), layer_strides: Sequence[int] = (1, 2),
                 out_channels: Sequence[int] = (128, 256), upsample_strides: Sequence[int] = (1, 2),
                 upsample_channels: Sequence[int] = (256, 256), bn_eps: float = 1e-3, bn_momentum: float = 0.01):
        super().__init__()
        nums, strides, outs = _ints("layer_nums", layer_nums), _ints("layer_strides", layer_strides), _ints("out_channels", out_channels)
        ups, upc = _ints("upsample_strides", upsample_strides), _ints("upsample_channels", upsample_channels)
        n = len(nums)
        for name, t in (("layer_strides", strides), ("out_channels", outs), ("upsample_strides", ups), ("upsample_channels", upc)):
            if len(t) != n:
                raise L.BevfError(f"BEVBackbone: {name} has {len(t)} entries but layer_nums has {n}: one per level")
        if n == 0:
            raise L.BevfError("BEVBackbone: layer_nums is empty: at least one level")
        for name, t in (("in_channels", (int(in_channels),)), ("out_channels", outs), ("upsample_channels", upc)):
            for c in t:
                if c <= 0 or c % 32:
                    raise L.BevfError(f"BEVBackbone: {name} = {c} must be a positive multiple of 32 (the convolution kernels' channel step)")
        if any(k < 0 for k in nums):
            raise L.BevfError(f"BEVBackbone: layer_nums = {nums} must not be negative")
        total = 1
        for i in range(n):
            if strides[i] not in (1, 2):
                raise L.BevfError(f"BEVBackbone: layer_strides[{i}] = {strides[i]} must be 1 or 2 (the 3x3 convolution kernels' strides)")
            total *= strides[i]
            if ups[i] != total:
                raise L.BevfError(f"BEVBackbone: upsample_strides[{i}] = {ups[i]} but level {i} sits at stride {total} "
                                  f"(prod(layer_strides[:{i + 1}])): every level must return to the input grid")
            if ups[i] not in (1, 2, 4):
                raise L.BevfError(f"BEVBackbone: upsample_strides[{i}] = {ups[i]} must be 1, 2 or 4 (the transposed-convolution kernel's strides)")
        self.in_channels = int(in_channels)
        self.layer_nums, self.layer_strides, self.level_channels = nums, strides, outs
        self.upsample_strides, self.upsample_channels = ups, upc
        self.out_channels = sum(upc)
        self.max_stride = max(ups)
        bn = lambda c: nn.BatchNorm2d(c, eps=float(bn_eps), momentum=float(bn_momentum))
        self.backbone, self.neck = nn.Module(), nn.Module()
        blocks, deblocks, cin = [], [], self.in_channels
        for i in range(n):
            layers = [nn.Conv2d(cin, outs[i], 3, stride=strides[i], padding=1, bias=False), bn(outs[i]), nn.ReLU(inplace=True)]
            for _ in range(nums[i]):
                layers += [nn.Conv2d(outs[i], outs[i], 3, padding=1, bias=False), bn(outs[i]), nn.ReLU(inplace=True)]
            blocks.append(nn.Sequential(*layers))
            deblocks.append(nn.Sequential(nn.ConvTranspose2d(outs[i], upc[i], ups[i], stride=ups[i], bias=False), bn(upc[i]),
                                          nn.ReLU(inplace=True)))
            cin = outs[i]
        self.backbone.blocks = nn.ModuleList(blocks)
        self.neck.deblocks = nn.ModuleList(deblocks)
        self._engine = None

    def check_grid(self, bev_h: int, bev_w: int) -> None:
        if bev_h <= 0 or bev_w <= 0 or bev_h % self.max_stride or bev_w % self.max_stride:
            raise L.BevfError(f"BEVBackbone: the BEV grid (bev_h, bev_w) = ({bev_h}, {bev_w}) must be divisible by the largest "
                              f"upsample stride {self.max_stride}")

    def _eng(self) -> "E.BackboneEngine":
        if self._engine is None:
            self._engine = E.BackboneEngine(self)
        return self._engine

    def forward_nhwc(self, bev_nhwc: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        """Eval-mode fast path: the flat NHWC map [B][H][W][in_channels] in the storage dtype -> the flat NHWC concat
        [B][H][W][out_channels] (the engine's buffer: the next call overwrites it)."""
        self.check_grid(H, W)
        return self._eng().run(bev_nhwc, B, H, W)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.in_channels:
            got = tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__
            raise L.BevfError(f"BEVBackbone: expected a (B, {self.in_channels}, H, W) BEV map, got {got}")
        B, _, H, W = x.shape
        self.check_grid(H, W)
        E.require_cuda(x)
        if self.training:
            from . import training
            if training.wants_train_path(self):
                if self._eng().dtype != torch.float32:
                    raise L.BevfError(f"BEVBackbone: {self._eng().dtype} storage in train mode is not supported (the training tape "
                                      "is fp32); call .eval() for bf16 inference")
                return training.bev_backbone_train_forward(self, x)
        with torch.no_grad():
            dt = self._eng().dtype
            y = self.forward_nhwc(E.to_nhwc(x.float()).to(dt), B, H, W)
            return E.to_nchw(y, B, self.out_channels, H, W)
