"""Training augmentation on the device, with the calibration kept consistent.

The reference's YAML lists augmentation under `dataset.augmentation` (ref configs/base.yaml:85-114) and its drivers never read it.
This module reads that section and applies the BEVFusion-style pair -- one world transform per frame, one image transform per
(frame, camera) -- as HIP kernels (csrc/augment.hip), so no per-sample host work comes back:

* world: T = Trans . Scale(s) . Rz(theta) . Flip, one 4x4 per frame, applied to the LiDAR points, the radar points, the boxes, the
  velocities and the calibration.  Flip is two independent p = 0.5 flips, x -> -x and y -> -y (BEVFusion's RandomFlip3D): what
  `lidar.random_flip: true` means here.  `radar.random_flip` adds nothing of its own: a radar flip that differs from the frame's flip
  would put the radar returns in another world than the LiDAR points and the boxes, so radar always follows the frame's T; from
  the radar section only `enable` and `noise_std` are used.
* image: an integer crop window [x0, x1) x [y0, y1) in source pixels, resized to the network's input size exactly as Pillow's
  `Image.resize(size, BILINEAR, box=window)` does it, and a horizontal flip bit.  Window edges are integers on purpose: Pillow keeps
  `box` in single precision, an integer box is exact in both.  Camera rotation is out of scope.
* photometric: contrast, brightness, saturation, hue with torchvision's float formulas, applied in THIS FIXED ORDER (a deviation:
  torchvision's ColorJitter draws a random order per call).  A neutral factor (1, 1, 1, 0) skips its operation, so an all-neutral
  image is bit-equal to `preprocess.preprocess_camera_images`.

Random numbers are drawn on the host from a `numpy.random.Generator` (a few dozen scalars per step); the radar noise is `torch.randn`
on the device.  `augment_batch(..., paste=, bank=)` runs the GT-paste of `gt_paste.py` in front of the world
transform; `augment_batch(..., map_shapes=, map_grid=)` rasterises the map's polygons and polylines into the segmentation head's
target masks after the world transform (`map_targets.py`).  `augmented_calib` returns the matching `camera_calib=` tensor of the 'project' and 'frustum' camera branches.  No
CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import camera_rig as CR
from .preprocess import IMAGENET_MEAN, IMAGENET_STD, PRECISION_BITS

PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)


# ---- settings ------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class AugmentSettings:
    """`dataset.augmentation`, with the neutral value for everything absent or disabled."""
    brightness: float = 0.0
    contrast: float = 0.0
    saturation: float = 0.0
    hue: float = 0.0
    mean: Tuple[float, float, float] = IMAGENET_MEAN
    std: Tuple[float, float, float] = IMAGENET_STD
    camera_flip: bool = False
    camera_scale: Optional[Tuple[float, float]] = None
    flip: bool = False
    scale: Optional[Tuple[float, float]] = None
    rotation: Optional[Tuple[float, float]] = None                 # degrees
    translation: Optional[Tuple[float, float, float]] = None       # sigma of a normal per axis, metres
    radar_noise_std: float = 0.0


def _pair(v, what: str) -> Optional[Tuple[float, float]]:
    if v is None or v is False:
        return None
    lo, hi = (float(x) for x in v)
    if not lo <= hi:
        raise ValueError(f"augmentation: {what} must be [lo, hi] with lo <= hi, got {v}")
    return lo, hi


def settings(config: Optional[Dict]) -> AugmentSettings:
    """AugmentSettings from a loaded YAML (`dataset.augmentation`).  Honoured: camera.enable, camera.color_jitter.{brightness,
    contrast, saturation, hue}, camera.normalize.{mean, std}, the opt-in camera.random_flip and camera.random_scale [lo, hi];
    lidar.enable, lidar.random_flip, lidar.random_scale, the opt-in lidar.random_rotation [deg_lo, deg_hi] and
    lidar.random_translation [sx, sy, sz]; radar.enable, radar.noise_std.  The lidar section defines the frame's world transform;
    radar.random_flip is not read (module docstring).  A missing section or `enable: false` gives that part's neutral value."""
    aug = ((config or {}).get("dataset", {}) or {}).get("augmentation", {}) or {}
    kw: Dict = {}
    cam = aug.get("camera") or {}
    norm = cam.get("normalize") or {}
    if norm.get("mean") is not None:
        kw["mean"] = tuple(float(v) for v in norm["mean"])
    if norm.get("std") is not None:
        kw["std"] = tuple(float(v) for v in norm["std"])
    if cam.get("enable", False):
        cj = cam.get("color_jitter") or {}
        for k in ("brightness", "contrast", "saturation", "hue"):
            kw[k] = float(cj.get(k, 0.0) or 0.0)
        if not 0.0 <= kw["hue"] <= 0.5 or min(kw["brightness"], kw["contrast"], kw["saturation"]) < 0.0:
            raise ValueError("augmentation: color_jitter needs hue in [0, 0.5] and non-negative brightness / contrast / saturation")
        kw["camera_flip"] = bool(cam.get("random_flip", False))
        kw["camera_scale"] = _pair(cam.get("random_scale"), "camera.random_scale")
        if kw["camera_scale"] is not None and kw["camera_scale"][0] <= 0.0:
            raise ValueError("augmentation: camera.random_scale must be positive")
    lid = aug.get("lidar") or {}
    if lid.get("enable", False):
        kw["flip"] = bool(lid.get("random_flip", False))
        kw["scale"] = _pair(lid.get("random_scale"), "lidar.random_scale")
        if kw["scale"] is not None and kw["scale"][0] <= 0.0:
            raise ValueError("augmentation: lidar.random_scale must be positive")
        kw["rotation"] = _pair(lid.get("random_rotation"), "lidar.random_rotation")
        tr = lid.get("random_translation")
        if tr is not None and tr is not False:
            kw["translation"] = tuple(float(v) for v in tr)
            if len(kw["translation"]) != 3 or min(kw["translation"]) < 0.0:
                raise ValueError("augmentation: lidar.random_translation must be three non-negative sigmas")
    rad = aug.get("radar") or {}
    if rad.get("enable", False):
        kw["radar_noise_std"] = float(rad.get("noise_std", 0.0) or 0.0)
    return AugmentSettings(**kw)


# ---- parameters ----------------------------------------------------------------------------------------------------------------------

@dataclass
class AugmentParams:
    """One step's parameters (host, fp64 / integers).  bev_aug [B][4][4] = T; scale [B] = s; windows [B][ncam][4] = (x0, x1, y0, y1)
    in source pixels; flip [B][ncam] (0 / 1); jitter [B][ncam][4] = (contrast f_c, brightness f_b, saturation f_s, hue shift)."""
    bev_aug: np.ndarray
    scale: np.ndarray
    windows: np.ndarray
    flip: np.ndarray
    jitter: np.ndarray
    src_size: Tuple[int, int]
    out_size: Tuple[int, int]

    @property
    def B(self) -> int:
        return int(self.bev_aug.shape[0])

    @property
    def ncam(self) -> int:
        return int(self.windows.shape[1])

    def mat12(self) -> np.ndarray:
        """fp32 [B][12]: the first three rows of T, rounded once."""
        return np.ascontiguousarray(self.bev_aug[:, :3, :].reshape(self.B, 12).astype(np.float32))


def neutral_params(B: int, ncam: int, src_size: Tuple[int, int], out_size: Tuple[int, int]) -> AugmentParams:
    Hs, Ws = (int(v) for v in src_size)
    win = np.tile(np.array([0, Ws, 0, Hs], dtype=np.int32), (B, ncam, 1))
    jit = np.tile(np.array([1.0, 1.0, 1.0, 0.0]), (B, ncam, 1))
    return AugmentParams(np.tile(np.eye(4), (B, 1, 1)), np.ones(B), win, np.zeros((B, ncam), dtype=np.int32), jit,
                         (Hs, Ws), (int(out_size[0]), int(out_size[1])))


def world_transform(flip_x: bool, flip_y: bool, theta: float, s: float, t: Sequence[float]) -> np.ndarray:
    """T = Trans(t) . Scale(s) . Rz(theta) . Flip as a 4x4 fp64 matrix (theta in radians)."""
    c, sn = math.cos(theta), math.sin(theta)
    R = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]])
    F = np.diag([-1.0 if flip_x else 1.0, -1.0 if flip_y else 1.0, 1.0])
    T = np.eye(4)
    T[:3, :3] = s * (R @ F)
    T[:3, 3] = np.asarray(t, dtype=np.float64)
    return T


def sample(st: AugmentSettings, B: int, ncam: int, src_size: Tuple[int, int], out_size: Tuple[int, int],
           rng: np.random.Generator) -> AugmentParams:
    """Draw one step's parameters; the same generator state gives the same parameters.  Per frame, in this order: flip x, flip y
    (p = 0.5 each), s ~ U(random_scale), theta ~ U(random_rotation) degrees, translation ~ N(0, sigma) per axis; then per (frame,
    camera): zoom z ~ U[lo, hi] of camera.random_scale -- the window is round(Ws lo / z) x round(Hs lo / z) (z = lo shows the whole
    frame) with its origin uniform over the integer offsets that keep it inside the frame --, the flip bit, and f_c, f_b, f_s ~
    U[1 - v, 1 + v] (at least 0), hue shift ~ U[-hue, hue].  Every draw is made whether or not its setting is enabled."""
    p = neutral_params(B, ncam, src_size, out_size)
    Hs, Ws = p.src_size
    for b in range(B):
        fx, fy = rng.random() < 0.5, rng.random() < 0.5
        us, ur = rng.random(), rng.random()
        tn = rng.standard_normal(3)
        s = st.scale[0] + us * (st.scale[1] - st.scale[0]) if st.scale else 1.0
        th = math.radians(st.rotation[0] + ur * (st.rotation[1] - st.rotation[0])) if st.rotation else 0.0
        t = tn * np.asarray(st.translation) if st.translation else np.zeros(3)
        p.bev_aug[b] = world_transform(st.flip and fx, st.flip and fy, th, s, t)
        p.scale[b] = s
        for c in range(ncam):
            u = rng.random(8)
            if st.camera_scale:
                lo, hi = st.camera_scale
                z = lo + u[0] * (hi - lo)
                ww = min(max(int(round(Ws * lo / z)), 1), Ws)
                wh = min(max(int(round(Hs * lo / z)), 1), Hs)
                x0 = min(int(u[1] * (Ws - ww + 1)), Ws - ww)
                y0 = min(int(u[2] * (Hs - wh + 1)), Hs - wh)
                p.windows[b, c] = (x0, x0 + ww, y0, y0 + wh)
            p.flip[b, c] = 1 if (st.camera_flip and u[3] < 0.5) else 0
            for j, v in enumerate((st.contrast, st.brightness, st.saturation)):
                p.jitter[b, c, j] = max(0.0, 1.0 + (2.0 * u[4 + j] - 1.0) * v) if v else 1.0
            p.jitter[b, c, 3] = (2.0 * u[7] - 1.0) * st.hue if st.hue else 0.0
    return p


# ---- Pillow's coefficients for a box -------------------------------------------------------------------------------------------------

def box_ksize(window: int, out_size: int) -> int:
    scale = float(window) / out_size
    return int(math.ceil(scale if scale >= 1.0 else 1.0)) * 2 + 1


def resample_tables_box(in_size: int, in0: int, in1: int, out_size: int, stride: Optional[int] = None):
    """preprocess.resample_tables for `Image.resize(..., box=)` along one axis: the source interval [in0, in1) of an axis of in_size
    pixels.  Pillow's precompute_coeffs with center starting at in0 and scale = (in1 - in0) / out; the taps are clipped to the
    image, not to the box (Pillow reads past a box edge).  (bounds (out, 2), coef (out, stride) zero-padded, ksize)."""
    scale = float(in1 - in0) / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    stride = ksize if stride is None else int(stride)
    if stride < ksize:
        raise ValueError(f"resample_tables_box: stride {stride} below ksize {ksize}")
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, stride), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = float(in0) + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _check_windows(windows: np.ndarray, src_size: Tuple[int, int]) -> np.ndarray:
    w = np.ascontiguousarray(np.asarray(windows).reshape(-1, 4))
    if not np.issubdtype(w.dtype, np.integer):
        raise L.BevfError("augment: crop windows must be integers (x0, x1, y0, y1)")
    Hs, Ws = src_size
    if (w[:, 0] < 0).any() or (w[:, 1] > Ws).any() or (w[:, 0] >= w[:, 1]).any() or (w[:, 2] < 0).any() or (w[:, 3] > Hs).any() \
            or (w[:, 2] >= w[:, 3]).any():
        raise L.BevfError(f"augment: a crop window is empty or leaves the {Hs} x {Ws} frame")
    return w.astype(np.int32)


# ---- the image leg -------------------------------------------------------------------------------------------------------------------

def device_tables(windows, src_size: Tuple[int, int], out_size: Tuple[int, int], device):
    """The per-image Pillow tables for integer windows [n][4] = (x0, x1, y0, y1), built on the device:
    (bounds_h [n][Wo][2], coef_h [n][Wo][ksh], ksh, bounds_v [n][Ho][2], coef_v [n][Ho][ksv], ksv), int32; the strides ksh / ksv
    are the largest ksize among the windows."""
    device = torch.device(device)
    if device.type != "cuda":
        raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    Hs, Ws = (int(v) for v in src_size)
    Ho, Wo = (int(v) for v in out_size)
    w = _check_windows(windows, (Hs, Ws))
    n = w.shape[0]
    ksh = box_ksize(int((w[:, 1] - w[:, 0]).max()), Wo)
    ksv = box_ksize(int((w[:, 3] - w[:, 2]).max()), Ho)
    wd = torch.from_numpy(w).to(device)
    i32 = dict(dtype=torch.int32, device=device)
    bh, kh = torch.empty(n, Wo, 2, **i32), torch.empty(n, Wo, ksh, **i32)
    bv, kv = torch.empty(n, Ho, 2, **i32), torch.empty(n, Ho, ksv, **i32)
    L.resample_tables_box(wd, n, Hs, Ws, Ho, Wo, ksh, ksv, bh, kh, bv, kv)
    return bh, kh, ksh, bv, kv, ksv


def _frames(imgs: torch.Tensor, what: str):
    if imgs.dtype != torch.uint8 or imgs.dim() < 3 or imgs.shape[-1] != 3:
        raise L.BevfError(f"{what}: expected uint8 (..., H, W, 3)")
    if not imgs.is_cuda:
        raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    lead = tuple(imgs.shape[:-3])
    H, W = int(imgs.shape[-3]), int(imgs.shape[-2])
    return imgs.reshape(-1, H, W, 3).contiguous(), lead, H, W


def resize_crop(imgs: torch.Tensor, windows, out_size: Tuple[int, int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 (..., H, W, 3) cuda frames and one integer window (x0, x1, y0, y1) per frame -> (uint8 (..., Ho, Wo, 3) equal to PIL's
    `Image.resize((Wo, Ho), BILINEAR, box=(x0, y0, x1, y1))`, int64 (...,) sums of Pillow's gray value over each output image)."""
    x, lead, H, W = _frames(imgs, "resize_crop")
    n = x.shape[0]
    Ho, Wo = (int(v) for v in out_size)
    if np.asarray(windows).reshape(-1, 4).shape[0] != n:
        raise L.BevfError(f"resize_crop: {n} frames but {np.asarray(windows).reshape(-1, 4).shape[0]} windows")
    bh, kh, ksh, bv, kv, ksv = device_tables(windows, (H, W), (Ho, Wo), x.device)
    out = torch.empty(n, Ho, Wo, 3, dtype=torch.uint8, device=x.device)
    gray = torch.empty(n, dtype=torch.int64, device=x.device)
    L.resize_crop_u8(x, out, gray, n, H, W, Ho, Wo, bh, kh, ksh, bv, kv, ksv)
    return out.reshape(*lead, Ho, Wo, 3), gray.reshape(lead)


def jitter_flip_normalize(imgs_u8: torch.Tensor, gray_sum: torch.Tensor, jitter, flip, mean: Sequence[float] = IMAGENET_MEAN,
                          std: Sequence[float] = IMAGENET_STD) -> torch.Tensor:
    """uint8 (..., Ho, Wo, 3) -> fp32 (..., 3, Ho, Wo): per image jitter (contrast, brightness, saturation, hue shift) in that order,
    horizontal flip where flip != 0, then (x - mean) / std.  gray_sum: resize_crop's second output."""
    x, lead, Ho, Wo = _frames(imgs_u8, "jitter_flip_normalize")
    n = x.shape[0]
    j = torch.from_numpy(np.ascontiguousarray(np.asarray(jitter, dtype=np.float64).reshape(-1, 4).astype(np.float32))).to(x.device)
    f = torch.from_numpy(np.ascontiguousarray(np.asarray(flip).reshape(-1).astype(np.int32))).to(x.device)
    if j.shape[0] != n or f.shape[0] != n:
        raise L.BevfError(f"jitter_flip_normalize: {n} images, {j.shape[0]} jitter rows, {f.shape[0]} flip bits")
    out = torch.empty(n, 3, Ho, Wo, device=x.device)
    L.jitter_flip_normalize_u8(x, out, gray_sum.reshape(-1).contiguous(), j, f, n, Ho, Wo, mean, std)
    return out.reshape(*lead, 3, Ho, Wo)


def augment_images(frames_u8: torch.Tensor, params: AugmentParams, st: AugmentSettings) -> torch.Tensor:
    """uint8 (B, ncam, Hs, Ws, 3) -> fp32 (B, ncam, 3, Ho, Wo): crop + resize, jitter, flip, normalise with st.mean / st.std."""
    if tuple(frames_u8.shape[-3:-1]) != tuple(params.src_size):
        raise L.BevfError(f"augment_images: frames are {tuple(frames_u8.shape[-3:-1])}, the parameters were drawn for {params.src_size}")
    u8, gray = resize_crop(frames_u8, params.windows, params.out_size)
    return jitter_flip_normalize(u8, gray, params.jitter, params.flip, st.mean, st.std)


# ---- the world leg -------------------------------------------------------------------------------------------------------------------

def _mat(mat, B: int, device) -> torch.Tensor:
    """(B, 12) fp32 on the device from AugmentParams, a (B, 4, 4) / (B, 3, 4) / (B, 12) array or tensor."""
    if isinstance(mat, AugmentParams):
        mat = mat.mat12()
    if isinstance(mat, torch.Tensor):
        m = mat.detach().cpu().double().numpy()
    else:
        m = np.asarray(mat, dtype=np.float64)
    m = m.reshape(B, -1)
    if m.shape[1] == 16:
        m = m[:, :12]
    if m.shape[1] != 12:
        raise L.BevfError(f"augment: the world transform must be (B, 4, 4), (B, 3, 4) or (B, 12), got {tuple(np.shape(mat))}")
    return torch.from_numpy(np.ascontiguousarray(m.astype(np.float32))).to(device)


def _points(points: torch.Tensor, what: str) -> torch.Tensor:
    if points.dim() != 3 or points.shape[2] < 3 or points.dtype != torch.float32:
        raise L.BevfError(f"{what}: expected fp32 (B, N, C>=3)")
    if not points.is_cuda:
        raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    return points.contiguous()


def transform_filter_pad_lidar(points: torch.Tensor, counts: Optional[torch.Tensor], mat, max_points: int = 35000,
                               pc_range: Sequence[float] = PC_RANGE, vel_ch: Optional[Sequence[int]] = None
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(B, N, C) fp32 cuda sweeps (frame b holds counts[b] points, None = N) -> p' = T p per frame, then what
    `preprocess.filter_pad_lidar` does without `choice`: strict range filter, input order kept, zero padding to max_points, the first
    max_points survivors when more survive.  One launch sequence for the whole batch.  -> ((B, max_points, C), int32 (B,) counts)."""
    pts = _points(points, "transform_filter_pad_lidar")
    B, N, Cc = pts.shape
    dev = pts.device
    n_in = None
    if counts is not None:
        n_in = torch.as_tensor(counts).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if n_in.numel() != B:
            raise L.BevfError(f"transform_filter_pad_lidar: {B} frames but {n_in.numel()} counts")
    out = torch.empty(B, max_points, Cc, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    work = torch.empty(L.points_affine_work_floats(B, N, Cc), device=dev)
    L.points_affine_filter_pad(pts, n_in, _mat(mat, B, dev), out, count, work, B, N, Cc, max_points, vel_ch, pc_range)
    return out, count


def transform_points_(points: torch.Tensor, mat, noise_std: float = 0.0, vel_ch: Optional[Sequence[int]] = None,
                      generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(B, N, C) fp32 cuda points through T IN PLACE (radar): no filter; noise_std > 0 adds noise_std * torch.randn (device
    generator) to channels 0-2.  The radar channel layout is not defined by the reference (it fills radar with randn), so the
    velocity channels are a parameter and default to none."""
    if not points.is_contiguous():
        raise L.BevfError("transform_points_: in place, needs a contiguous tensor")
    pts = _points(points, "transform_points_")
    B, N, Cc = pts.shape
    noise = torch.randn(B, N, 3, device=pts.device, generator=generator) if noise_std > 0.0 else None
    L.points_affine(pts, _mat(mat, B, pts.device), noise, noise_std, B, N, Cc, vel_ch)
    return points


def transform_boxes(gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_velocities: Optional[torch.Tensor], mat, scale
                    ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """gt_boxes (B, M, 7|9) fp32, gt_labels (B, M) integers (< 0 = padding row, left untouched), gt_velocities (B, M, 2) or None ->
    new tensors: centre through T, (w, l, h) times s, yaw' = atan2 of the transformed heading, velocities (and columns 7-8 of a
    9-column box) through the 2x2 linear part."""
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] not in (7, 9) or gt_boxes.dtype != torch.float32:
        raise L.BevfError("transform_boxes: expected fp32 (B, M, 7 or 9) boxes")
    if not gt_boxes.is_cuda or not gt_labels.is_cuda or (gt_velocities is not None and not gt_velocities.is_cuda):
        raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    B, M, ncol = gt_boxes.shape
    if tuple(gt_labels.shape) != (B, M) or (gt_velocities is not None and tuple(gt_velocities.shape) != (B, M, 2)):
        raise L.BevfError("transform_boxes: labels must be (B, M) and velocities (B, M, 2)")
    boxes = gt_boxes.clone(memory_format=torch.contiguous_format)
    vel = None if gt_velocities is None else gt_velocities.float().clone(memory_format=torch.contiguous_format)
    s = torch.from_numpy(np.asarray(scale, dtype=np.float64).reshape(-1).astype(np.float32)).to(boxes.device)
    L.boxes_affine(boxes, gt_labels.to(torch.int64).contiguous(), vel, _mat(mat, B, boxes.device), s, B, M, ncol)
    return boxes, vel


# ---- calibration ---------------------------------------------------------------------------------------------------------------------

def image_maps(params: AugmentParams, image_size: Tuple[int, int]) -> np.ndarray:
    """A [B][ncam][3][3] fp64: the pixel map of each image transform in the coordinates of a rig whose intrinsics refer to
    image_size (H, W).  With u~ = (u + 1/2) / W: crop u~' = (u~ Ws - x0) / (x1 - x0), flip u~'' = 1 - u~', and u' = W u~' - 1/2
    (v alike with H, Hs, y0, y1; no vertical flip)."""
    H, W = (float(v) for v in image_size)
    Hs, Ws = params.src_size
    A = np.zeros((params.B, params.ncam, 3, 3))
    for b in range(params.B):
        for c in range(params.ncam):
            x0, x1, y0, y1 = (float(v) for v in params.windows[b, c])
            ax = Ws / (x1 - x0)
            cx = (0.5 * Ws - W * x0) / (x1 - x0) - 0.5
            ay = Hs / (y1 - y0)
            cy = (0.5 * Hs - H * y0) / (y1 - y0) - 0.5
            if params.flip[b, c]:
                ax, cx = -ax, W - 1.0 - cx
            A[b, c] = [[ax, 0.0, cx], [0.0, ay, cy], [0.0, 0.0, 1.0]]
    return A


def augmented_calib(base, params: AugmentParams, image_size: Optional[Tuple[int, int]] = None):
    """The fp64 (B, ncam, 4, 4) `camera_calib=` tensor of the augmented batch: rows 0-2 = A . (K . E[0:3]) . T^-1, row 3 =
    E[2] . T^-1 -- `camera_rig.calib_matrices` of the rig with K' = A . K and cam_to_bev' = T . cam_to_bev.  base: a CameraRig (every
    frame), a sequence of B rigs, or a calib_matrices array / tensor (then image_size = the (H, W) its intrinsics refer to is
    needed; default the default rig's).  Returns a torch tensor (on base's device when base is a tensor).  The last row of every
    image map A is (0, 0, 1), so row 2 of the result equals its depth row 3 -- what the 'frustum' branch relies on: its frustum
    points are then bev_aug[b] applied to the base rig's."""
    dev = None
    if isinstance(base, CR.CameraRig):
        base = [base] * params.B
    if isinstance(base, torch.Tensor):
        dev = base.device
        P = base.detach().cpu().double().numpy()
    elif isinstance(base, np.ndarray):
        P = np.asarray(base, dtype=np.float64)
    else:
        rigs = list(base)
        P = CR.calib_matrices(rigs)
        image_size = rigs[0].image_size
    if image_size is None:
        image_size = CR.default_rig().image_size
    if P.shape != (params.B, params.ncam, 4, 4):
        raise ValueError(f"augmented_calib: base calibration holds {P.shape}, the parameters ({params.B}, {params.ncam}, 4, 4)")
    A = image_maps(params, image_size)
    out = np.empty_like(P)
    for b in range(params.B):
        Tinv = np.linalg.inv(params.bev_aug[b])
        for c in range(params.ncam):
            out[b, c, :3] = A[b, c] @ P[b, c, :3] @ Tinv
            out[b, c, 3] = P[b, c, 3] @ Tinv
    t = torch.from_numpy(out)
    return t if dev is None else t.to(dev)


# ---- the batch -----------------------------------------------------------------------------------------------------------------------

def augment_batch(frames_u8: Optional[torch.Tensor], lidar: Optional[torch.Tensor], lidar_counts: Optional[torch.Tensor],
                  radar: Optional[Sequence[torch.Tensor]], gt_boxes: Optional[torch.Tensor], gt_labels: Optional[torch.Tensor],
                  gt_velocities: Optional[torch.Tensor], params: AugmentParams, settings: AugmentSettings, base_calib=None,
                  max_points: int = 35000, pc_range: Sequence[float] = PC_RANGE, lidar_vel_ch: Optional[Sequence[int]] = None,
                  radar_vel_ch: Optional[Sequence[int]] = None, generator: Optional[torch.Generator] = None,
                  image_size: Optional[Tuple[int, int]] = None, *, paste=None, bank=None, map_shapes=None, map_grid=None) -> Dict:
    """One augmented training batch, everything on the device:

    frames_u8 (B, ncam, Hs, Ws, 3) uint8; lidar (B, N, C) fp32 with lidar_counts (B,) valid points per frame (None = N); radar: a
    sequence of (B, P, C) fp32 tensors (transformed in place on copies); gt_boxes (B, M, 7|9), gt_labels (B, M) with -1 padding,
    gt_velocities (B, M, 2) or None.  Any input may be None.  Returns camera_imgs (B, ncam, 3, Ho, Wo), lidar_points (B, max_points,
    C), lidar_count, radar_points, gt_boxes, gt_labels, gt_velocities, camera_calib (None without base_calib): the inputs of
    `model(...)` and `prepare_centernet_targets`.

    paste= (a `gt_paste.PasteParams` with at least one candidate per frame) and bank= (a `gt_paste.ObjectBank`), given together, run
    the GT-paste of `gt_paste.paste` first, before the world transform (ObjectSample, then GlobalRotScaleTrans): lidar, gt_boxes and
    gt_labels are then required, the paste's outputs take their place (Kc more GT rows per frame), and the result gains
    paste_accepted int32 (B, Kc).  With a camera branch the pasted objects are NOT drawn into the images, as in BEVFusion's own
    recipe.  Without the two arguments the function takes exactly the path it takes without them.

    map_shapes= (a `map_targets.MapShapes`) and map_grid= (a `BEVSegmentationHead`, or (output_range, output_size)), given together,
    add seg_targets uint8 (B, K, Ho, Wo): the map's polygons and polylines moved through the step's T and rasterised after it
    (`map_targets.rasterize`), the masks `SegFocalLoss` takes.  Without the two arguments the result has no such key."""
    accepted = None
    if (paste is None) != (bank is None):
        raise L.BevfError("augment_batch: paste= and bank= go together")
    if (map_shapes is None) != (map_grid is None):
        raise L.BevfError("augment_batch: map_shapes= and map_grid= go together")
    if paste is not None and paste.Kc > 0:
        if lidar is None or gt_boxes is None or gt_labels is None:
            raise L.BevfError("augment_batch: paste= needs lidar, gt_boxes and gt_labels")
        from . import gt_paste
        pasted = gt_paste.paste(lidar, lidar_counts, gt_boxes, gt_labels, gt_velocities, bank, paste)
        lidar, lidar_counts = pasted["lidar_points"], pasted["lidar_count"]
        gt_boxes, gt_labels, gt_velocities, accepted = pasted["gt_boxes"], pasted["gt_labels"], pasted["gt_velocities"], pasted["accepted"]
    out: Dict = dict(camera_imgs=None, lidar_points=None, lidar_count=None, radar_points=None, gt_boxes=None, gt_labels=gt_labels,
                     gt_velocities=None, camera_calib=None)
    if frames_u8 is not None:
        out["camera_imgs"] = augment_images(frames_u8, params, settings)
    if lidar is not None:
        out["lidar_points"], out["lidar_count"] = transform_filter_pad_lidar(lidar, lidar_counts, params, max_points, pc_range,
                                                                              lidar_vel_ch)
    if radar is not None:
        if any(not r.is_cuda for r in radar):
            raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
        out["radar_points"] = [transform_points_(r.clone(memory_format=torch.contiguous_format), params, settings.radar_noise_std,
                                                 radar_vel_ch, generator) for r in radar]
    if gt_boxes is not None:
        out["gt_boxes"], out["gt_velocities"] = transform_boxes(gt_boxes, gt_labels, gt_velocities, params, params.scale)
    if base_calib is not None:
        out["camera_calib"] = augmented_calib(base_calib, params, image_size)
    if accepted is not None:
        out["paste_accepted"] = accepted
    if map_shapes is not None:
        from . import map_targets
        if isinstance(map_grid, torch.nn.Module):
            out["seg_targets"] = map_targets.rasterize_for(map_grid, map_shapes, params)
        else:
            try:
                rng, size = map_grid
            except (TypeError, ValueError):
                raise L.BevfError("augment_batch: map_grid= is a BEVSegmentationHead or (output_range, output_size)") from None
            out["seg_targets"] = map_targets.rasterize(map_shapes, rng, size, params)
    return out
