"""Multi-sweep LiDAR accumulation on the device (csrc/sweeps.hip): the standard nuScenes-style LiDAR input.

The key sweep and the preceding sweeps of every frame are moved into the key sweep's sensor frame through the ego poses and merged into
one padded cloud whose extra last channel is the sweep's time lag (the channel a velocity head learns from):

    points, counts = pack_sweeps(frames, "cuda")                      # (B, S, N, C), (B, S); sweep 0 = the key sweep
    T = sweep_transforms(key_l2e, key_e2g, sweep_l2e, sweep_e2g)      # (B, S, 4, 4) fp64 on the device
    lag = time_lags(key_us, sweep_us).cuda()                          # (B, S) fp32 seconds
    o = merge_sweeps(points, counts, T, lag, max_points=262144)
    augment_batch(frames, o["lidar_points"], o["lidar_count"].clamp(max=262144), ...)   # or straight into the detector

The merged cloud is an ordinary (B, max_points, C + 1) input with counts; `sweep_count[:, 0]` says how many leading rows are the key's.

The rules (close-point removal before the transform, the fp64 transform rounded once, the strict range filter after it, sweep order,
truncation from the oldest sweep) are stated in include/bevf.h.  Nothing here synchronises with the host; `SweepMerger.merge` does not
allocate either, so it can be captured in a graph and replayed on new data in the same buffers.  There is no CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
MAX_POINTS = 262144

__all__ = ["pack_sweeps", "time_lags", "sweep_transforms", "SweepMerger", "merge_sweeps"]

_NO_CPU = "HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)"


# ---- host helpers --------------------------------------------------------------------------------------------------------------------

def pack_sweeps(frames: Sequence[Sequence], device, n: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """frames[b][s] = the (n_i, C) points (array or tensor) of sweep s of frame b, sweep 0 the key sweep; None or an empty array is an
    absent sweep.  -> (points (B, S, N, C) fp32 zero-padded, counts (B, S) int32) on `device`; N = n, or the longest sweep."""
    B = len(frames)
    S = len(frames[0]) if B else 0
    if B == 0 or S == 0 or any(len(f) != S for f in frames):
        raise L.BevfError("pack_sweeps: needs at least one frame, and the same number of sweeps (at least one) in every frame")
    arrs, Cc = [], None
    for f in frames:
        for a in f:
            a = np.zeros((0, 0), dtype=np.float32) if a is None else (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a))
            if a.size:
                if a.ndim != 2 or a.shape[1] < 3:
                    raise L.BevfError(f"pack_sweeps: a sweep is (n, C >= 3), got {a.shape}")
                if Cc is not None and a.shape[1] != Cc:
                    raise L.BevfError(f"pack_sweeps: ragged channel counts ({Cc} and {a.shape[1]})")
                Cc = a.shape[1]
            arrs.append(a)
    if Cc is None:
        raise L.BevfError("pack_sweeps: every sweep is empty, the channel count is unknown")
    longest = max(a.shape[0] if a.size else 0 for a in arrs)
    N = longest if n is None else int(n)
    if N < longest:
        raise L.BevfError(f"pack_sweeps: n = {N} but a sweep holds {longest} points")
    pts = np.zeros((B * S, N, Cc), dtype=np.float32)
    cnt = np.zeros(B * S, dtype=np.int32)
    for i, a in enumerate(arrs):
        if a.size:
            pts[i, :a.shape[0]] = a
            cnt[i] = a.shape[0]
    return torch.from_numpy(pts.reshape(B, S, N, Cc)).to(device), torch.from_numpy(cnt.reshape(B, S)).to(device)


def time_lags(key_us, sweep_us) -> torch.Tensor:
    """key_us (B,) and sweep_us (B, S) integer microsecond stamps -> (B, S) fp32 seconds on the host: (key - sweep) * 1e-6 in float64
    (the difference itself in int64, exact), rounded once to fp32."""
    k = np.asarray(key_us.cpu() if isinstance(key_us, torch.Tensor) else key_us)
    s = np.asarray(sweep_us.cpu() if isinstance(sweep_us, torch.Tensor) else sweep_us)
    if k.dtype.kind not in "iu" or s.dtype.kind not in "iu":
        raise L.BevfError("time_lags: stamps are integer microseconds")
    k, s = k.astype(np.int64).reshape(-1), s.astype(np.int64)
    if s.ndim != 2 or s.shape[0] != k.shape[0]:
        raise L.BevfError(f"time_lags: key stamps (B,) and sweep stamps (B, S), got {k.shape} and {s.shape}")
    return torch.from_numpy(((k[:, None] - s).astype(np.float64) * 1e-6).astype(np.float32))


# ---- device ----------------------------------------------------------------------------------------------------------------------------

def _dev(what: str, **specs) -> None:
    """Each keyword = (tensor, shape, dtype): all shapes and dtypes first, then that every tensor is on the device and contiguous.
    Nothing is converted, so nothing is allocated."""
    for name, (t, shape, dtype) in specs.items():
        if not isinstance(t, torch.Tensor):
            raise L.BevfError(f"{what}: {name}: expected a tensor, got {type(t).__name__}")
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            raise L.BevfError(f"{what}: {name}: expected {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    for name, (t, _, _) in specs.items():
        if not t.is_cuda:
            raise L.BevfError(_NO_CPU)
        if not t.is_contiguous():
            raise L.BevfError(f"{what}: {name} must be contiguous")


def sweep_transforms(key_lidar2ego: torch.Tensor, key_ego2global: torch.Tensor, sweep_lidar2ego: torch.Tensor,
                     sweep_ego2global: torch.Tensor) -> torch.Tensor:
    """(B, 4, 4), (B, 4, 4), (B, S, 4, 4), (B, S, 4, 4) float64 cuda -> (B, S, 4, 4) float64 cuda, sweep sensor frame -> key sensor
    frame: inv(L_k) . inv(E_k) . E_s . L_s in fp64 on the device (global poses carry translations of order 1e3 m)."""
    if not isinstance(sweep_lidar2ego, torch.Tensor) or sweep_lidar2ego.dim() != 4:
        raise L.BevfError("sweep_transforms: sweep_lidar2ego is a (B, S, 4, 4) tensor")
    B, S = sweep_lidar2ego.shape[:2]
    f64 = torch.float64
    _dev("sweep_transforms", key_lidar2ego=(key_lidar2ego, (B, 4, 4), f64), key_ego2global=(key_ego2global, (B, 4, 4), f64),
         sweep_lidar2ego=(sweep_lidar2ego, (B, S, 4, 4), f64), sweep_ego2global=(sweep_ego2global, (B, S, 4, 4), f64))
    out = torch.empty(B, S, 4, 4, dtype=f64, device=sweep_lidar2ego.device)
    L.sweep_pose_chain(key_lidar2ego, key_ego2global, sweep_lidar2ego, sweep_ego2global, out, B, S)
    return out


class SweepMerger:
    """Owns the output and work buffers of one merge shape.  `merge` launches a fixed sequence into them and returns views of them, so a
    captured `merge` can be replayed after the inputs were overwritten in place."""

    def __init__(self, B: int, S: int, N: int, C: int, max_points: int = MAX_POINTS, pc_range: Sequence[float] = PC_RANGE,
                 close_radius: float = 1.0, device="cuda"):
        if not (B > 0 and S > 0 and N >= 0 and 3 <= C <= 8 and max_points > 0):
            raise L.BevfError(f"SweepMerger: bad shape B = {B}, S = {S}, N = {N}, C = {C}, max_points = {max_points} (3 <= C <= 8)")
        if len(pc_range) != 6:
            raise L.BevfError(f"SweepMerger: pc_range is (x0, y0, z0, x1, y1, z1), got {tuple(pc_range)}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise L.BevfError(_NO_CPU)
        self.B, self.S, self.N, self.C, self.max_points = B, S, N, C, int(max_points)
        self.pc_range, self.close_radius = tuple(float(v) for v in pc_range), float(close_radius)
        self.out = torch.empty(B, self.max_points, C + 1, device=dev)
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.sweep_count = torch.zeros(B, S, dtype=torch.int32, device=dev)
        self.work = torch.empty(-(-L.sweeps_merge_work_bytes(B, S, N) // 4), dtype=torch.int32, device=dev)

    def merge(self, points: torch.Tensor, counts: torch.Tensor, sweep_to_key: torch.Tensor, time_lag: torch.Tensor) -> Dict[str, torch.Tensor]:
        """points (B, S, N, C) fp32, counts (B, S) int32, sweep_to_key (B, S, 4, 4) float64, time_lag (B, S) fp32, all cuda ->
        dict(lidar_points (B, max_points, C + 1), lidar_count (B,) int32 = all survivors, untruncated, sweep_count (B, S) int32)."""
        B, S, N, C = self.B, self.S, self.N, self.C
        _dev("merge", points=(points, (B, S, N, C), torch.float32), counts=(counts, (B, S), torch.int32),
             sweep_to_key=(sweep_to_key, (B, S, 4, 4), torch.float64), time_lag=(time_lag, (B, S), torch.float32))
        L.sweeps_merge(points, counts, sweep_to_key, time_lag, self.out, self.count, self.sweep_count, self.work, B, S, N, C, self.max_points, self.close_radius,
                       self.pc_range)
        return dict(lidar_points=self.out, lidar_count=self.count, sweep_count=self.sweep_count)


def merge_sweeps(points: torch.Tensor, counts: torch.Tensor, sweep_to_key: torch.Tensor, time_lag: torch.Tensor,
                 max_points: int = MAX_POINTS, pc_range: Sequence[float] = PC_RANGE, close_radius: float = 1.0) -> Dict[str, torch.Tensor]:
    """The one-shot form of SweepMerger.merge, with fresh buffers."""
    if not isinstance(points, torch.Tensor) or points.dim() != 4:
        raise L.BevfError("merge_sweeps: points is a (B, S, N, C) tensor")
    if not points.is_cuda:
        raise L.BevfError(_NO_CPU)
    B, S, N, C = points.shape
    return SweepMerger(B, S, N, C, max_points, pc_range, close_radius, points.device).merge(points, counts, sweep_to_key, time_lag)
