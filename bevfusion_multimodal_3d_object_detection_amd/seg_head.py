"""BEV map segmentation (opt-in): a second consumer of the fused BEV map beside the CenterNet head.

`bev_grid_resample` puts a BEV map given on one metric range onto another range and size (csrc/bev_seg.hip), `BEVSegmentationHead`
resamples the fused map onto the map grid and classifies every cell (logits, one channel per map class), `SegFocalLoss` is the
sigmoid focal loss on those logits with its gradient on the device, and `seg_iou_counts` / `seg_iou` give the thresholded IoU the
task is scored with.  The detector owns a head when built with `seg_head=` (fusion.py) and then returns 'seg' beside the detection
tensors.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E
from .encoders import _cfg

DEFAULT_CLASSES = ("drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "divider")
DEFAULT_OUTPUT_RANGE = (-50.0, -50.0, 50.0, 50.0)
DEFAULT_OUTPUT_SIZE = (200, 200)
DEFAULT_THRESHOLDS = (0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65)


# ---- grids -----------------------------------------------------------------------------------------------------------------

def range_grid(rng: Sequence[float], H: int, W: int, what: str = "range") -> Tuple[float, float, float, float]:
    """[xmin, ymin, xmax, ymax] over H rows (y) and W columns (x) -> (x0, y0, vx, vy) in fp64.  A NaN component passes (the
    resample then writes zeros); an empty or reversed range, or a non-positive size, raises."""
    r = [float(v) for v in rng]
    if len(r) != 4:
        raise L.BevfError(f"{what} must be [xmin, ymin, xmax, ymax], got {list(rng)}")
    if int(H) != H or int(W) != W or H <= 0 or W <= 0:
        raise L.BevfError(f"{what}: the size must be positive integers (rows, columns), got ({H}, {W})")
    if r[2] <= r[0] or r[3] <= r[1] or any(math.isinf(v) for v in r):
        raise L.BevfError(f"{what} is degenerate: need finite xmin < xmax and ymin < ymax, got {r}")
    return r[0], r[1], (r[2] - r[0]) / int(W), (r[3] - r[1]) / int(H)


def _size(out_size) -> Tuple[int, int]:
    try:
        Ho, Wo = out_size
    except (TypeError, ValueError):
        raise L.BevfError(f"out_size must be (rows, columns), got {out_size!r}") from None
    return Ho, Wo


class _GridResample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, in_grid, out_grid, Ho, Wo):
        B, Cc, H, W = x.shape
        xr = x.detach().permute(0, 2, 3, 1).contiguous()              # (a view of channels-last memory)
        y = torch.empty(B, Ho, Wo, Cc, dtype=x.dtype, device=x.device)
        L.bev_grid_resample(xr, y, B, H, W, Ho, Wo, Cc, Cc, Cc, in_grid, out_grid)
        ctx.geom = (B, H, W, Ho, Wo, Cc, in_grid, out_grid)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        B, H, W, Ho, Wo, Cc, in_grid, out_grid = ctx.geom
        if dy.dtype != torch.float32:
            raise L.BevfError(f"bev_grid_resample: the backward is fp32 only, got a {dy.dtype} gradient")
        dyr = dy.permute(0, 2, 3, 1).contiguous()
        dx = torch.empty(B, H, W, Cc, device=dy.device)
        L.bev_grid_resample_bwd(dyr, dx, B, H, W, Ho, Wo, Cc, Cc, in_grid, out_grid)
        return dx.permute(0, 3, 1, 2), None, None, None, None


def bev_grid_resample(x: torch.Tensor, in_range, out_range, out_size) -> torch.Tensor:
    """The (B, C, H, W) BEV map x, which covers in_range = [xmin, ymin, xmax, ymax] (row i is y, column j is x, as everywhere in
    this package), resampled bilinearly onto out_size = (rows, columns) cells covering out_range: the output cell whose centre is p
    holds x sampled at p, with zeros outside the map -- grid_sample(align_corners=False, padding_mode='zeros') on an axis-aligned
    grid.  fp32 or bf16; channels-last memory is taken without a copy and the result is channels-last.  Differentiable in x (fp32;
    a deterministic pull kernel)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise L.BevfError("bev_grid_resample: x must be a (B, C, H, W) tensor")
    B, _, H, W = x.shape
    Ho, Wo = _size(out_size)
    in_grid = range_grid(in_range, H, W, "bev_grid_resample: in_range")
    out_grid = range_grid(out_range, Ho, Wo, "bev_grid_resample: out_range")
    if not x.is_cuda:
        raise L.BevfError("bev_grid_resample: x is a CPU tensor (no CPU fallback in this package)")
    return _GridResample.apply(x, in_grid, out_grid, int(Ho), int(Wo))


# ---- the head ----------------------------------------------------------------------------------------------------------------

def seg_head_settings(seg_head, config) -> Optional[dict]:
    """The detector's `seg_head=` keyword (True / False / dict / None) and the config's model.seg_head -> the keyword arguments of
    BEVSegmentationHead the two spell out (the keyword's entries win), or None when the head is off.  None = the config decides
    (model.seg_head.enable), False = off whatever the config says."""
    sc = ((config or {}).get("model", {}) or {}).get("seg_head", {}) or {}
    if isinstance(sc, bool):
        sc = dict(enable=sc)
    if seg_head is None:
        if not sc.get("enable", False):
            return None
        seg_head = {}
    elif seg_head is False:
        return None
    elif seg_head is True:
        seg_head = {}
    elif not isinstance(seg_head, dict):
        raise L.BevfError(f"seg_head must be True, False, None or a dict of BEVSegmentationHead settings, got {type(seg_head).__name__}")
    known = ("num_classes", "classes", "output_range", "output_size", "hidden_channels")
    unknown = sorted(set(seg_head) - set(known) - {"enable"})
    if unknown:
        raise L.BevfError(f"seg_head: unknown settings {unknown} (known: {list(known)})")
    merged = {k: sc[k] for k in known if k in sc}
    merged.update({k: v for k, v in seg_head.items() if k in known})
    if seg_head.get("enable", True) is False:
        return None
    classes = merged.pop("classes", None)
    if classes is not None:
        if "num_classes" in merged and int(merged["num_classes"]) != len(classes):
            raise L.BevfError(f"seg_head: num_classes = {merged['num_classes']} but {len(classes)} classes are named")
        merged["num_classes"] = len(classes)
        merged["classes"] = tuple(str(c) for c in classes)
    return merged


class BEVSegmentationHead(nn.Module):
    """BEV map segmentation on a fused BEV map (the second task of multi-task BEV fusion): the (B, in_channels, bev_h, bev_w) map
    on pc_range is resampled onto output_size cells covering output_range (bev_grid_resample), then
    classifier = conv3x3 + BN + ReLU, conv3x3 + BN + ReLU, conv1x1 (+ bias) -> num_classes.  forward returns LOGITS
    (B, num_classes, Ho, Wo) in fp32; a class is present where sigmoid(logit) passes a threshold (seg_iou_counts).
    Eval mode runs the folded-BatchNorm convolution kernels (engine.SegHeadEngine; fp32 or bf16 storage), train mode the tape
    (training.SegHeadTape; fp32): batch statistics and gradients for the parameters and the input map."""

    def __init__(self, in_channels: Optional[int] = None, num_classes: Optional[int] = None, hidden_channels: Optional[int] = None,
                 pc_range: Optional[Sequence[float]] = None, bev_h: Optional[int] = None, bev_w: Optional[int] = None,
                 output_range: Optional[Sequence[float]] = None, output_size: Optional[Sequence[int]] = None,
                 config: Optional[Dict] = None, config_path: Optional[str] = None, classes: Optional[Sequence[str]] = None):
        super().__init__()
        config = _cfg(config, config_path)
        mc, dc = ((config or {}).get("model", {}) or {}), ((config or {}).get("dataset", {}) or {})
        sc, bc = (mc.get("seg_head", {}) or {}), (mc.get("bev_fusion", {}) or {})
        if isinstance(sc, bool):
            sc = {}
        if in_channels is None:
            in_channels = sc.get("in_channels", bc.get("bev_channels", 256))
        if classes is None and "classes" in sc:
            classes = sc["classes"]
        if num_classes is None:
            num_classes = len(classes) if classes is not None else sc.get("num_classes", len(DEFAULT_CLASSES))
        if classes is not None and len(classes) != int(num_classes):
            raise L.BevfError(f"BEVSegmentationHead: num_classes = {num_classes} but {len(classes)} classes are named")
        if hidden_channels is None:
            hidden_channels = sc.get("hidden_channels", None) or in_channels
        self.in_channels, self.num_classes, self.hidden_channels = int(in_channels), int(num_classes), int(hidden_channels)
        if not 1 <= self.num_classes <= 64:
            raise L.BevfError(f"BEVSegmentationHead: num_classes must be 1 .. 64, got {num_classes}")
        self.classes = tuple(classes) if classes is not None else (
            DEFAULT_CLASSES if self.num_classes == len(DEFAULT_CLASSES) else tuple(f"class_{k}" for k in range(self.num_classes)))
        self.pc_range = list(dc.get("point_cloud_range", [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]) if pc_range is None else pc_range)
        if len(self.pc_range) != 6:
            raise L.BevfError(f"BEVSegmentationHead: pc_range must be [xmin, ymin, zmin, xmax, ymax, zmax], got {self.pc_range}")
        self.bev_h = int(bc.get("bev_h", dc.get("bev_h", 200)) if bev_h is None else bev_h)
        self.bev_w = int(bc.get("bev_w", dc.get("bev_w", 200)) if bev_w is None else bev_w)
        self.output_range = [float(v) for v in (sc.get("output_range", DEFAULT_OUTPUT_RANGE) if output_range is None else output_range)]
        Ho, Wo = _size(sc.get("output_size", DEFAULT_OUTPUT_SIZE) if output_size is None else output_size)
        self.in_grid = range_grid([self.pc_range[0], self.pc_range[1], self.pc_range[3], self.pc_range[4]], self.bev_h, self.bev_w,
                                  "BEVSegmentationHead: pc_range")
        self.out_grid = range_grid(self.output_range, Ho, Wo, "BEVSegmentationHead: output_range")
        self.output_size = (int(Ho), int(Wo))
        c, h = self.in_channels, self.hidden_channels
        self.classifier = nn.Sequential(nn.Conv2d(c, h, 3, padding=1), nn.BatchNorm2d(h), nn.ReLU(inplace=True),
                                        nn.Conv2d(h, h, 3, padding=1), nn.BatchNorm2d(h), nn.ReLU(inplace=True),
                                        nn.Conv2d(h, self.num_classes, 1, bias=True))
        self._engine = None

    def _eng(self) -> "E.SegHeadEngine":
        if self._engine is None:
            self._engine = E.SegHeadEngine(self)
        return self._engine

    def _check_input(self, shape) -> None:
        want = (self.in_channels, self.bev_h, self.bev_w)
        if len(shape) != 4 or tuple(shape[1:]) != want:
            raise L.BevfError(f"BEVSegmentationHead: expected a (B, {want[0]}, {want[1]}, {want[2]}) BEV map, got {tuple(shape)}")

    def forward_nhwc(self, bev_nhwc: torch.Tensor, B: int) -> torch.Tensor:
        """Eval-mode fast path on the flat NHWC fused map in the storage dtype -> logits (B, K, Ho, Wo) fp32."""
        return self._eng().run(bev_nhwc, B)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            raise L.BevfError("BEVSegmentationHead: x must be a (B, C, H, W) tensor")
        self._check_input(x.shape)
        E.require_cuda(x)
        if self.training:
            from . import training
            if training.wants_train_path(self):
                if self._eng().dtype != torch.float32:
                    raise L.BevfError(f"BEVSegmentationHead: {self._eng().dtype} storage in train mode is not supported (the training "
                                      "tape is fp32); call .eval() for bf16 inference")
                return training.seg_head_train_forward(self, x)
        with torch.no_grad():
            return self.forward_nhwc(E.to_nhwc(x.float()).to(self._eng().dtype), x.shape[0])


# ---- loss and metric -----------------------------------------------------------------------------------------------------------

def seg_targets_u8(targets: torch.Tensor, shape, what: str) -> torch.Tensor:
    """`targets` (B, K, Ho, Wo) in bool, uint8 or a float dtype, values in {0, 1} by contract -> a contiguous uint8 tensor on the
    logits' device.  Any other dtype or shape raises."""
    if not isinstance(targets, torch.Tensor) or tuple(targets.shape) != tuple(shape):
        got = tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets).__name__
        raise L.BevfError(f"{what}: targets must be a (B, K, Ho, Wo) = {tuple(shape)} mask tensor, got {got}")
    if targets.dtype == torch.bool or targets.dtype.is_floating_point:
        targets = targets.to(torch.uint8)
    elif targets.dtype != torch.uint8:
        raise L.BevfError(f"{what}: targets must be bool, uint8 or float with values in {{0, 1}}, got {targets.dtype}")
    return targets.contiguous()


def _check_logits(logits, what: str) -> None:
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
        raise L.BevfError(f"{what}: logits must be a (B, K, Ho, Wo) tensor")
    if not logits.is_cuda:
        raise L.BevfError(f"{what}: logits is a CPU tensor (no CPU fallback in this package)")
    if logits.dtype != torch.float32:
        raise L.BevfError(f"{what}: logits must be float32 (BEVSegmentationHead returns fp32 logits), got {logits.dtype}")


def _logit_rows(logits: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """(B, K, Ho, Wo) fp32 logits -> (NHWC rows [B * P][K], row stride K): a view of channels-last memory, a copy otherwise."""
    return logits.detach().permute(0, 2, 3, 1).contiguous(), logits.shape[1]


class _SegFocal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, alpha, gamma):
        B, K, Ho, Wo = logits.shape
        rows, cs = _logit_rows(logits)
        out = torch.empty(K + 1, device=logits.device)
        work = torch.empty(L.seg_focal_work_doubles(K), dtype=torch.float64, device=logits.device)
        L.seg_focal_loss(rows, cs, targets, B, Ho * Wo, K, alpha, gamma, work, out)
        ctx.saved = (rows, cs, targets, alpha, gamma, (B, K, Ho, Wo))
        per_class = out[:K].clone()
        ctx.mark_non_differentiable(per_class)
        return out[K].clone(), per_class

    @staticmethod
    def backward(ctx, g, _g_per_class):
        rows, cs, targets, alpha, gamma, (B, K, Ho, Wo) = ctx.saved
        dl = torch.empty(B, Ho, Wo, cs, device=rows.device)
        L.seg_focal_loss_bwd(rows, cs, targets, g.reshape(1).float().contiguous(), dl, B, Ho * Wo, K, alpha, gamma)
        return dl.permute(0, 3, 1, 2), None, None, None


class SegFocalLoss(nn.Module):
    """Sigmoid focal loss on segmentation logits (Lin et al. 2017), one mean per class over the B * Ho * Wo cells:
    loss[k] = mean a_t (1 - p_t)^gamma BCE(x, t), p = sigmoid(x), p_t = t p + (1 - t)(1 - p), a_t = alpha t + (1 - alpha)(1 - t);
    alpha < 0 (the default) switches the alpha weighting off.  __call__(logits (B, K, Ho, Wo) fp32, targets (B, K, Ho, Wo) bool /
    uint8 / float in {0, 1}) -> {'loss': the sum of the K class means (differentiable in the logits; the gradient arrives as a device
    scalar, no host sync), 'per_class': the K means (for logging, not differentiable)}.  Sums are fp64 in a fixed order: the same
    bits every run."""

    def __init__(self, alpha: float = -1.0, gamma: float = 2.0):
        super().__init__()
        if not gamma >= 0.0 or not alpha <= 1.0:
            raise L.BevfError(f"SegFocalLoss: need gamma >= 0 and alpha <= 1 (alpha < 0: no alpha weighting), got alpha = {alpha}, "
                              f"gamma = {gamma}")
        self.alpha, self.gamma = float(alpha), float(gamma)

    def forward(self, logits: torch.Tensor, targets: torch.Tensor) -> Dict[str, torch.Tensor]:
        _check_logits(logits, "SegFocalLoss")
        t = seg_targets_u8(targets, logits.shape, "SegFocalLoss").to(logits.device)
        loss, per_class = _SegFocal.apply(logits, t, self.alpha, self.gamma)
        return {"loss": loss, "per_class": per_class}


def threshold_logits(thresholds: Sequence[float]) -> torch.Tensor:
    """Probability thresholds in (0, 1) -> the logits log(p / (1 - p)), computed in fp64 on the host and rounded to fp32."""
    th = [float(v) for v in thresholds]
    if not th or len(th) > 32 or any(not 0.0 < v < 1.0 for v in th):
        raise L.BevfError(f"seg_iou_counts: 1 .. 32 probability thresholds inside (0, 1), got {th}")
    return torch.tensor([math.log(v / (1.0 - v)) for v in th], dtype=torch.float64).to(torch.float32)


def seg_iou_counts(logits: torch.Tensor, targets: torch.Tensor, thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> torch.Tensor:
    """int64 (T, K, 3) on the device: true positives, false positives and false negatives of sigmoid(logit) >= threshold against
    the masks, per threshold and class -- evaluated as logit >= log(t / (1 - t)).  Counts of several batches add."""
    _check_logits(logits, "seg_iou_counts")
    rows, cs = _logit_rows(logits)
    B, K, Ho, Wo = logits.shape
    t = seg_targets_u8(targets, logits.shape, "seg_iou_counts").to(logits.device)
    thr = threshold_logits(thresholds).to(logits.device)
    counts = torch.empty(thr.numel(), K, 3, dtype=torch.int64, device=logits.device)
    L.seg_iou_counts(rows, cs, t, thr, counts, B, Ho * Wo, K)
    return counts


def seg_iou(counts: torch.Tensor) -> Dict[str, torch.Tensor]:
    """(T, K, 3) counts -> {'iou': (T, K) TP / (TP + FP + FN) in fp64 (0 where a class has no positive at all), 'max_iou': (K,)
    the best threshold's IoU per class, 'mean_iou': their mean}."""
    if counts.dim() != 3 or counts.shape[-1] != 3:
        raise L.BevfError(f"seg_iou: counts must be (T, K, 3), got {tuple(counts.shape)}")
    c = counts.to(torch.float64)
    union = c.sum(-1)
    iou = torch.where(union > 0, c[..., 0] / union.clamp(min=1.0), torch.zeros_like(union))
    best = iou.max(0).values
    return {"iou": iou, "max_iou": best, "mean_iou": best.mean()}
