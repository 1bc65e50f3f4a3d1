"""Temporal BEV fusion (opt-in): the previous frame's fused BEV map, aligned to the current frame by ego-motion,
is a fourth slot of FlexibleBEVFusion's concatenated map (model.bev_fusion.temporal.enable / temporal=True).

ego_motion(pose_prev, pose_cur) gives the matrix the warp takes -- current frame -> previous frame, in metres, in the frame of
point_cloud_range --, augmented_ego_motion carries it through the BEV augmentation of the two steps, and bev_warp is the resample
itself (csrc/bev_warp.hip) as an autograd function.  The model-side checks of `prev_bev=` / `ego_motion=` live here too.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .encoders import pillar_grid


def temporal_enabled(temporal: Optional[bool], config) -> bool:
    """The keyword if given, else model.bev_fusion.temporal.enable of the config, else off."""
    if temporal is not None:
        return bool(temporal)
    t = ((config or {}).get("model", {}).get("bev_fusion", {}) or {}).get("temporal", {}) or {}
    return bool(t.get("enable", False)) if isinstance(t, dict) else bool(t)


def ego_motion(pose_prev, pose_cur) -> np.ndarray:
    """inv(pose_prev) @ pose_cur for 4 x 4 fp64 ego -> global poses ((4, 4) or batched (B, 4, 4)): the map from a point of the
    current ego frame to the same world point in the previous ego frame.  numpy, on the host."""
    a, b = np.asarray(pose_prev, dtype=np.float64), np.asarray(pose_cur, dtype=np.float64)
    if a.shape != b.shape or a.shape[-2:] != (4, 4):
        raise L.BevfError(f"ego_motion: expected two (..., 4, 4) pose arrays of one shape, got {a.shape} and {b.shape}")
    return np.linalg.inv(a) @ b


def augmented_ego_motion(M, aug_cur, aug_prev=None) -> np.ndarray:
    """T_prev . M . T_cur^-1 with T the AugmentParams.bev_aug matrices of the two steps (aug_prev None: the same as aug_cur): the
    ego-motion between two frames that were each augmented with their own world transform.  aug_*: an AugmentParams or its
    (B, 4, 4) bev_aug array.  Flips and scales make the result a general planar affine map, which the warp handles."""
    M = np.asarray(M, dtype=np.float64)
    Tc = np.asarray(getattr(aug_cur, "bev_aug", aug_cur), dtype=np.float64)
    Tp = Tc if aug_prev is None else np.asarray(getattr(aug_prev, "bev_aug", aug_prev), dtype=np.float64)
    return Tp @ M @ np.linalg.inv(Tc)


def check_ego(ego_motion, B: int, dev) -> Tuple[torch.Tensor, Optional[np.ndarray]]:
    """`ego_motion=` -> (fp64 (B, 4, 4) contiguous tensor on dev, its host copy when the caller passed one on the host)."""
    if isinstance(ego_motion, np.ndarray):
        ego_motion = torch.from_numpy(np.ascontiguousarray(ego_motion))
    if not isinstance(ego_motion, torch.Tensor) or ego_motion.dtype != torch.float64 or tuple(ego_motion.shape) != (B, 4, 4):
        got = (f"{ego_motion.dtype} {tuple(ego_motion.shape)}" if isinstance(ego_motion, torch.Tensor) else type(ego_motion).__name__)
        raise L.BevfError(f"ego_motion must be a float64 ({B}, 4, 4) tensor (temporal.ego_motion: current frame -> previous frame), got {got}")
    host = None if ego_motion.is_cuda else ego_motion.detach().numpy()
    return ego_motion.detach().to(dev).contiguous(), host


def check_history(fus, prev_bev, ego_motion, B: int, dev, dtype):
    """The `prev_bev=` / `ego_motion=` arguments of a forward of FlexibleBEVFusion `fus` for B frames on dev, storage dtype
    `dtype` -> None for a module without temporal fusion, else (prev_bev or None for a first frame, ego tensor or None, host ego or
    None).  Raises BevfError, saying what is expected, for every combination that is not served."""
    if not getattr(fus, "temporal", False):
        if prev_bev is not None or ego_motion is not None:
            raise L.BevfError("prev_bev / ego_motion need a model built with temporal fusion: pass temporal=True (or set "
                              "model.bev_fusion.temporal.enable) when constructing it")
        return None
    if prev_bev is None:
        return None, None, None                                   # first frame of a sequence: a zero history slot
    if ego_motion is None:
        raise L.BevfError("prev_bev without ego_motion: pass ego_motion=, the float64 (B, 4, 4) current -> previous frame map of "
                          "temporal.ego_motion (the identity for a standing vehicle)")
    want = (B, fus.bev_channels, fus.bev_h, fus.bev_w)
    if not isinstance(prev_bev, torch.Tensor) or tuple(prev_bev.shape) != want:
        got = tuple(prev_bev.shape) if isinstance(prev_bev, torch.Tensor) else type(prev_bev).__name__
        raise L.BevfError(f"prev_bev must be (B, bev_channels, bev_h, bev_w) = {want}, the 'bev' output of the previous frame, got {got}")
    if prev_bev.dtype != dtype:
        raise L.BevfError(f"prev_bev must be {dtype}, the model's storage dtype, got {prev_bev.dtype}")
    ego, host = check_ego(ego_motion, B, dev)
    return prev_bev, ego, host


def nhwc_rows(x: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) -> a contiguous (B, H, W, C) tensor of the same values: a view of channels-last memory, a copy otherwise."""
    return x.permute(0, 2, 3, 1).contiguous()


def own_bev(fused: torch.Tensor, B: int, H: int, W: int, Cc: int) -> torch.Tensor:
    """The flat NHWC fused map -> an owned (B, C, H, W) tensor in channels-last memory: the detector's 'bev' output."""
    return fused[:B * H * W * Cc].detach().clone().view(B, H, W, Cc).permute(0, 3, 1, 2)


class _BevWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ego, ego_host, grid):
        B, Cc, H, W = x.shape
        xr = nhwc_rows(x.detach())
        y = torch.empty_like(xr)
        L.bev_warp(xr, y, ego, B, H, W, Cc, Cc, Cc, grid)
        ctx.ego, ctx.ego_host, ctx.grid = ego, ego_host, grid
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        B, Cc, H, W = dy.shape
        if dy.dtype != torch.float32:
            raise L.BevfError(f"bev_warp: the backward is fp32 only, got a {dy.dtype} gradient")
        dyr = nhwc_rows(dy)
        dx = torch.empty_like(dyr)
        L.bev_warp_bwd(dyr, dx, ctx.ego, B, H, W, Cc, Cc, ctx.grid, ctx.ego_host)
        return dx.permute(0, 3, 1, 2), None, None, None


def bev_warp(x: torch.Tensor, ego_motion, pc_range) -> torch.Tensor:
    """The (B, C, H, W) BEV map x of the previous frame resampled onto the current frame's grid: the output cell whose centre is p
    holds x sampled bilinearly at ego_motion[b] p (zeros outside the map).  ego_motion: float64 (B, 4, 4), host or device
    (temporal.ego_motion); pc_range: the point_cloud_range both grids share.  fp32 or bf16; channels-last memory is taken without a
    copy and the result is channels-last.  Differentiable in x (fp32; a deterministic pull kernel), not in ego_motion."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise L.BevfError("bev_warp: x must be a (B, C, H, W) tensor")
    if not x.is_cuda:
        raise L.BevfError("bev_warp: x is a CPU tensor (no CPU fallback in this package)")
    B, _, H, W = x.shape
    ego, host = check_ego(ego_motion, B, x.device)
    return _BevWarp.apply(x, ego, host, pillar_grid(pc_range, H, W)[:4])
