"""LiDAR depth supervision of the learned-depth camera branches (camera_view_transform 'frustum' / 'lift'; BEVDepth,
Li et al. 2022).  depth_net otherwise learns only from what the detection loss sends back through the BEV pool; the LiDAR sweep the
model is fed anyway says where along its ray a pixel's feature belongs.

    depth_targets(points, calib, image_size, Hc, Wc, depth)   the nearest depth bin a LiDAR return puts on every feature pixel (-1:
                                                              none) -- a pure function of (points, calib), so it follows
                                                              augment.augment_batch's points and camera_calib without further work
    depth_cross_entropy(logits, targets)                      (mean cross entropy over the pixels with a target, their count), on
                                                              its own kernels and differentiable in the logits

The detector runs both inside its training step when `forward` gets `depth_points=` and returns 'depth_loss' / 'depth_pixels'
(training.DepthLossTape); the caller adds w * out['depth_loss'] to its loss.  Hard one-hot targets on the uniform bins of
model.bev_fusion.camera_bev.depth only.  No reference counterpart (the reference has no view transform)."""
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import camera_rig as CR


def calib_tensor(calib, dev) -> torch.Tensor:
    """What `camera_calib=` accepts -> contiguous fp64 (B or 1, ncam, 4, 4) on dev: a CameraRig (every frame), a sequence of rigs,
    or a float64 tensor on the host or the device."""
    if isinstance(calib, CR.CameraRig):
        calib = [calib]
    if isinstance(calib, torch.Tensor):
        if calib.dtype != torch.float64:
            raise L.BevfError(f"depth supervision: calib must be float64 (camera_rig.calib_matrices), got {calib.dtype}")
        t = calib
    else:
        t = torch.from_numpy(CR.calib_matrices(list(calib)))
    if t.dim() != 4 or tuple(t.shape[2:]) != (4, 4):
        raise ValueError(f"depth supervision: calib holds {tuple(t.shape)}, expected (B, ncam, 4, 4)")
    return t.to(dev).contiguous()


def check_points(points, counts) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] < 3:
        raise ValueError(f"depth supervision: points must be a (B, N, >= 3) tensor, got "
                         f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    if not points.is_cuda:
        raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    if points.dtype != torch.float32:
        raise L.BevfError(f"depth supervision: points must be float32, got {points.dtype}")
    if points.stride(2) != 1 or (points.shape[1] > 1 and points.stride(1) < 3) or points.stride(0) < points.shape[1] * points.stride(1):
        points = points.contiguous()
    if counts is not None:
        if not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (points.shape[0],):
            raise ValueError(f"depth supervision: counts must hold one entry per frame ({points.shape[0]},)")
        if not counts.is_cuda:
            raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
        if counts.dtype not in (torch.int32, torch.int64):
            raise L.BevfError(f"depth supervision: counts must be int32 or int64, got {counts.dtype}")
        counts = counts.to(torch.int32).contiguous()
    return points, counts


def build_targets(points, counts, calib: torch.Tensor, image_size, Hc: int, Wc: int, depth: Sequence[float], target=None) -> torch.Tensor:
    """depth_targets on checked inputs: calib a contiguous fp64 device tensor (B or 1, ncam, 4, 4); writes `target` when given."""
    B, N = points.shape[:2]
    ncam = calib.shape[1]
    if calib.shape[0] not in (1, B):
        raise L.BevfError(f"depth supervision: calib holds {calib.shape[0]} frames, the points {B} (1 = shared, or one per frame)")
    D, dmin, dmax = depth
    if target is None:
        target = torch.empty(B, ncam, Hc, Wc, dtype=torch.int32, device=points.device)
    L.depth_targets(points, N, counts, calib, calib.shape[0] == 1, B, ncam, Hc, Wc, int(D), dmin, dmax, image_size, target)
    return target


def depth_targets(points: torch.Tensor, calib, image_size: Sequence[int], Hc: int, Wc: int, depth: Sequence[float],
                  counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 (B, ncam, Hc, Wc): the depth bin of the nearest LiDAR return on every pixel of the Hc x Wc feature maps, -1 where no
    point lands.  points fp32 (B, N, >= 3) on the device, columns 0-2 = (x, y, z) in the frame of point_cloud_range; all-zero rows
    (filter_pad_lidar's padding) and rows at or past counts[b] are ignored.  calib: what `camera_calib=` accepts -- a sequence of B
    camera_rig.CameraRig or the fp64 (B, ncam, 4, 4) tensor of camera_rig.calib_matrices / augment.augmented_calib, host or device;
    (1, ncam, 4, 4) or one CameraRig serves every frame.  image_size = (H, W) the calibration refers to; depth = (D, depth_min,
    depth_max), the uniform bins of camera_rig.depth_bin_of.  A point counts for a camera when depth_min <= zc < depth_max and its
    pixel floor((u + 1/2) Wc / W), floor((v + 1/2) Hc / H) is on the map."""
    D, dmin, dmax = CR.check_depth_settings(depth[0], depth[1], depth[2], min(CR.DEFAULT_MIN_DEPTH, float(depth[1])))
    points, counts = check_points(points, counts)
    return build_targets(points, counts, calib_tensor(calib, points.device), image_size, int(Hc), int(Wc), (D, dmin, dmax))


class _DepthCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, D):
        rows, width = logits.shape
        dev = logits.device
        out = torch.empty(2, device=dev)
        L.depth_ce(logits, width, target, rows, D, torch.empty(L.depth_ce_work_doubles(), dtype=torch.float64, device=dev), out)
        ctx.save_for_backward(logits, target, out)
        ctx.D = D
        loss, count = out[0], out[1]
        ctx.mark_non_differentiable(count)
        return loss, count

    @staticmethod
    def backward(ctx, g, _):
        logits, target, out = ctx.saved_tensors
        rows, width = logits.shape
        pd = torch.empty(rows, ctx.D, device=logits.device)
        L.softmax_rows(logits, width, pd, ctx.D, rows, ctx.D)
        dlogit = torch.zeros_like(logits)
        L.depth_ce_bwd(pd, ctx.D, target, g.reshape(1).float().contiguous(), out, dlogit, width, rows, ctx.D)
        return dlogit, None, None


def depth_cross_entropy(logits: torch.Tensor, targets: torch.Tensor, depth_bins: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, count): the mean over the supervised pixels of cross_entropy(logits, target) and their number, both 0-dim fp32 on
    the device; the loss is exactly 0 when no pixel has a target.  logits: fp32 (rows, >= D) -- columns past depth_bins (default:
    all of them) are padding, never read and given no gradient -- or NCHW (B * ncam, D, Hc, Wc) as depth_net returns them;
    targets: int32 with one entry per row / pixel in the same order (depth_targets' output), < 0 = not supervised.  Differentiable
    in the logits; usable on its own, e.g. for a validation depth loss."""
    if not logits.is_cuda or not targets.is_cuda:
        raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    if logits.dtype != torch.float32:
        raise L.BevfError(f"depth_cross_entropy: logits must be float32, got {logits.dtype} (bf16 storage is not supported)")
    if logits.dim() == 4:
        if depth_bins not in (None, logits.shape[1]):
            raise ValueError(f"depth_cross_entropy: NCHW logits have {logits.shape[1]} bins, depth_bins = {depth_bins}")
        logits = logits.permute(0, 2, 3, 1).reshape(-1, logits.shape[1])
    elif logits.dim() != 2:
        raise ValueError(f"depth_cross_entropy: logits must be (rows, >= D) or (N, D, H, W), got {tuple(logits.shape)}")
    D = logits.shape[1] if depth_bins is None else int(depth_bins)
    if not 1 <= D <= logits.shape[1]:
        raise ValueError(f"depth_cross_entropy: depth_bins = {D} for rows of {logits.shape[1]} columns")
    if targets.numel() != logits.shape[0]:
        raise ValueError(f"depth_cross_entropy: {targets.numel()} targets for {logits.shape[0]} rows")
    if targets.dtype != torch.int32:
        raise L.BevfError(f"depth_cross_entropy: targets must be int32 (depth_targets), got {targets.dtype}")
    return _DepthCE.apply(logits.contiguous(), targets.reshape(-1).contiguous(), D)
