"""GT-paste (object-sample) LiDAR augmentation on the device (csrc/gt_paste.hip).

The step of the BEVFusion / CenterPoint recipes that makes rare classes trainable: objects cropped from other frames (an `ObjectBank`)
are pasted into the sweep where they collide with nothing, the sweep's points inside a pasted box are removed, and the ground truth
gains the pasted boxes.  It runs before the world transform of `augment.py` (ObjectSample, then GlobalRotScaleTrans):
`augment.augment_batch(..., paste=params, bank=bank)`.

* `ObjectBank` -- the objects on the device: `points [Ptot][C]` (xyz relative to the object's box centre, other channels verbatim),
  `obj_ptr [K + 1]`, `boxes [K][7|9]`, `labels [K]`, with host copies of the labels and the object sizes so that sampling and the
  output capacity need no device synchronisation.  `ObjectBank.from_frames` crops a bank out of frames with `box_ops.points_in_boxes`;
  an object keeps its position, GT-paste pastes at the source location.
* `settings(config)` reads the opt-in `dataset.augmentation.lidar.object_sample: {enable, per_frame: {label: n}, min_points}` (the
  reference YAML has no such key: absent or `enable: false` means no paste).  `per_frame` is the number of CANDIDATES per frame and
  class, whatever the frame already holds, so no label count comes back from the device; the candidates that collide are dropped.
* `sample(settings, bank, B, rng)` draws the candidates on the host; `paste(...)` does the rest on the device, all frames in one launch
  sequence on torch's current stream, no host synchronisation, no float atomics.

Box convention as everywhere: `[x, y, z, w, l, h, yaw(, vx, vy)]`, l along the heading (cos yaw, sin yaw), w across it, z-extent
[z - h/2, z + h/2].  With a camera branch the pasted objects are NOT drawn into the images, as in BEVFusion's own recipe.  Not built:
per-object random yaw / position jitter, class-balanced counts that depend on the frame, ground-plane alignment.  No CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import box_ops

KC_MAX = 64
_NO_CPU = "HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)"


# ---- the bank ------------------------------------------------------------------------------------------------------------------------

class ObjectBank:
    """K objects: points (Ptot, C>=3) fp32 with xyz relative to the object's box centre, obj_ptr (K + 1,) (object k owns rows
    obj_ptr[k] .. obj_ptr[k + 1]), boxes (K, 7|9) fp32, labels (K,) integers >= 0.  The tensors stay on the device they come on
    (`paste` needs them on the GPU: `bank.to('cuda')`); `host_labels` / `host_sizes` are numpy copies."""

    def __init__(self, points: torch.Tensor, obj_ptr: torch.Tensor, boxes: torch.Tensor, labels: torch.Tensor):
        for name, t in (("points", points), ("obj_ptr", obj_ptr), ("boxes", boxes), ("labels", labels)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"ObjectBank: {name} must be a torch tensor, got {type(t).__name__}")
        if points.dim() != 2 or points.shape[1] < 3 or points.dtype != torch.float32:
            raise ValueError(f"ObjectBank: points must be fp32 (Ptot, C>=3), got {points.dtype} {tuple(points.shape)}")
        if boxes.dim() != 2 or boxes.shape[1] not in (7, 9) or boxes.dtype != torch.float32:
            raise ValueError(f"ObjectBank: boxes must be fp32 (K, 7 or 9), got {boxes.dtype} {tuple(boxes.shape)}")
        K = int(boxes.shape[0])
        if labels.dim() != 1 or labels.shape[0] != K or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise ValueError(f"ObjectBank: labels must be {K} integers, got {labels.dtype} {tuple(labels.shape)}")
        if obj_ptr.dim() != 1 or obj_ptr.shape[0] != K + 1 or obj_ptr.dtype.is_floating_point or obj_ptr.dtype == torch.bool:
            raise ValueError(f"ObjectBank: obj_ptr must be {K + 1} integers, got {obj_ptr.dtype} {tuple(obj_ptr.shape)}")
        if len({t.device for t in (points, obj_ptr, boxes, labels)}) != 1:
            raise ValueError("ObjectBank: the four tensors must live on one device")
        ptr = obj_ptr.detach().cpu().numpy().astype(np.int64)
        lab = labels.detach().cpu().numpy().astype(np.int64)
        if ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != points.shape[0]:
            raise ValueError(f"ObjectBank: obj_ptr must rise from 0 to the {points.shape[0]} point rows")
        if points.shape[0] >= 2 ** 31:
            raise ValueError("ObjectBank: more than 2^31 - 1 point rows")
        if (lab < 0).any():
            raise ValueError("ObjectBank: labels must be >= 0")
        self.points = points.detach().contiguous()
        self.obj_ptr = obj_ptr.detach().to(torch.int32).contiguous()
        self.boxes = boxes.detach().contiguous()
        self.labels = labels.detach().to(torch.int64).contiguous()
        self.host_labels = lab
        self.host_sizes = np.diff(ptr)

    def __len__(self) -> int:
        return int(self.boxes.shape[0])

    @property
    def channels(self) -> int:
        return int(self.points.shape[1])

    @property
    def device(self) -> torch.device:
        return self.points.device

    def to(self, device) -> "ObjectBank":
        return ObjectBank(self.points.to(device), self.obj_ptr.to(device), self.boxes.to(device), self.labels.to(device))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"points": self.points.cpu(), "obj_ptr": self.obj_ptr.cpu(), "boxes": self.boxes.cpu(), "labels": self.labels.cpu()}

    @classmethod
    def from_state_dict(cls, state: Dict[str, torch.Tensor], device=None) -> "ObjectBank":
        missing = [k for k in ("points", "obj_ptr", "boxes", "labels") if k not in state]
        if missing:
            raise ValueError(f"ObjectBank: the state lacks {missing}")
        bank = cls(state["points"], state["obj_ptr"], state["boxes"], state["labels"])
        return bank if device is None else bank.to(device)

    @classmethod
    def from_frames(cls, lidar: torch.Tensor, lidar_counts, gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                    min_points: int = 5) -> "ObjectBank":
        """Crop the objects of lidar (B, N, C) / gt_boxes (B, M, 7|9) / gt_labels (B, M) (rows < 0 are padding) with
        `box_ops.points_in_boxes` (a point in two boxes goes to the lower row); objects with fewer than min_points points are left
        out.  Objects are ordered by (frame, row), an object's points keep the sweep's order, xyz = point - centre (one fp32
        subtraction).  Offline ETL: torch indexing around the kernel, with host synchronisation."""
        if lidar.dim() != 3 or gt_boxes.dim() != 3 or tuple(gt_labels.shape) != tuple(gt_boxes.shape[:2]):
            raise ValueError("ObjectBank.from_frames: expected lidar (B, N, C), gt_boxes (B, M, 7|9), gt_labels (B, M)")
        idx = box_ops.points_in_boxes(lidar, gt_boxes, lidar_counts, gt_labels).long()
        B, N, Cc = lidar.shape
        M = gt_boxes.shape[1]
        key = (idx + torch.arange(B, device=idx.device)[:, None] * M).reshape(-1)
        sel = torch.nonzero(idx.reshape(-1) >= 0).reshape(-1)
        order = sel[torch.sort(key[sel], stable=True).indices]
        sizes = torch.bincount(key[sel], minlength=B * M)
        keep_obj = sizes >= max(int(min_points), 1)
        obj_of_point = key[order]
        order = order[keep_obj[obj_of_point]]
        obj_of_point = key[order]
        flat_boxes = gt_boxes.reshape(B * M, -1)
        pts = lidar.reshape(B * N, Cc)[order].clone()
        pts[:, :3] = pts[:, :3] - flat_boxes[obj_of_point, :3]
        kept = torch.nonzero(keep_obj).reshape(-1)
        ptr = torch.zeros(kept.numel() + 1, dtype=torch.int64, device=idx.device)
        ptr[1:] = torch.cumsum(sizes[kept], 0)
        return cls(pts, ptr, flat_boxes[kept].clone(), gt_labels.reshape(-1)[kept].clone())


# ---- settings and sampling (host) ----------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class PasteSettings:
    """`dataset.augmentation.lidar.object_sample`: per_frame = ((label, candidates), ...) in ascending label order (empty = no paste);
    bank objects with fewer than min_points points are never drawn."""
    per_frame: Tuple[Tuple[int, int], ...] = ()
    min_points: int = 5

    @property
    def Kc(self) -> int:
        return sum(n for _, n in self.per_frame)


def _int(v, what: str) -> int:
    if isinstance(v, bool) or (isinstance(v, float) and v != int(v)):
        raise ValueError(f"object_sample: {what} must be an integer, got {v!r}")
    try:
        return int(v)
    except (TypeError, ValueError):
        raise ValueError(f"object_sample: {what} must be an integer, got {v!r}") from None


def settings(config: Optional[Dict]) -> PasteSettings:
    """PasteSettings from a loaded YAML.  Keys of `dataset.augmentation.lidar.object_sample`: enable, per_frame {label: n} (labels
    integers >= 0, n >= 0, the sum over the classes Kc <= 64) and min_points (>= 1, default 5).  Absent or `enable: false`: no paste."""
    aug = ((config or {}).get("dataset", {}) or {}).get("augmentation", {}) or {}
    sec = (aug.get("lidar") or {}).get("object_sample") or {}
    if not sec.get("enable", False):
        return PasteSettings()
    per = sec.get("per_frame") or {}
    if not isinstance(per, dict):
        raise ValueError(f"object_sample: per_frame must map labels to counts, got {per!r}")
    rows = {}
    for k, v in per.items():
        lab, n = _int(k, "a label"), _int(v, f"the count of label {k!r}")
        if lab < 0:
            raise ValueError(f"object_sample: labels must be >= 0, got {lab}")
        if n < 0:
            raise ValueError(f"object_sample: the count of label {lab} is negative ({n})")
        if lab in rows:
            raise ValueError(f"object_sample: label {lab} is listed twice")
        rows[lab] = n
    st = PasteSettings(tuple((lab, rows[lab]) for lab in sorted(rows) if rows[lab] > 0), _int(sec.get("min_points", 5), "min_points"))
    if st.min_points < 1:
        raise ValueError(f"object_sample: min_points must be >= 1, got {st.min_points}")
    if st.Kc > KC_MAX:
        raise ValueError(f"object_sample: {st.Kc} candidates per frame, at most {KC_MAX}")
    return st


@dataclass
class PasteParams:
    """One step's candidates (host): cand int32 [B][Kc], indices into the bank, -1 = none."""
    cand: np.ndarray

    @property
    def B(self) -> int:
        return int(self.cand.shape[0])

    @property
    def Kc(self) -> int:
        return int(self.cand.shape[1])


def sample(st: PasteSettings, bank: ObjectBank, B: int, rng: np.random.Generator) -> PasteParams:
    """Draw one step's candidates; the same generator state gives the same candidates.  Per frame, the classes in ascending order; per
    class n uniforms u_0 .. u_{n-1} (always n of them, whatever the bank holds), and the partial Fisher-Yates shuffle over the m
    eligible bank objects of the class (ascending bank index, at least min_points points): pick i swaps positions i and
    i + floor(u_i (m - i)).  The first min(n, m) picks are the candidates -- distinct, uniform --, -1 fills the rest."""
    cand = np.full((int(B), st.Kc), -1, dtype=np.int32)
    pools = [np.nonzero((bank.host_labels == lab) & (bank.host_sizes >= st.min_points))[0] for lab, _ in st.per_frame]
    for b in range(int(B)):
        at = 0
        for (lab, n), pool in zip(st.per_frame, pools):
            u = rng.random(n)
            p = pool.copy()
            m = p.shape[0]
            for i in range(min(n, m)):
                j = min(i + int(u[i] * (m - i)), m - 1)
                p[i], p[j] = p[j], p[i]
                cand[b, at + i] = p[i]
            at += n
    return PasteParams(cand)


# ---- the paste (device) --------------------------------------------------------------------------------------------------------------

def default_capacity(bank: ObjectBank, params: PasteParams, N: int) -> int:
    """N plus the largest per-frame point total of the candidates (from the bank's host copy): nothing can be cut off."""
    c = params.cand
    sizes = np.where(c >= 0, bank.host_sizes[np.clip(c, 0, max(len(bank) - 1, 0))], 0) if len(bank) else np.zeros_like(c)
    return max(int(N) + (int(sizes.sum(1).max()) if c.size else 0), 1)


def _buffer(out: Optional[Dict], key: str, shape, dtype, dev) -> torch.Tensor:
    if out is None or out.get(key) is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    t = out[key]
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise L.BevfError(f"paste: out['{key}'] must be a contiguous {dtype} {tuple(shape)} tensor on {dev}")
    return t


def paste(lidar: torch.Tensor, lidar_counts, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_velocities: Optional[torch.Tensor],
          bank: ObjectBank, params: PasteParams, capacity: Optional[int] = None, out: Optional[Dict] = None) -> Dict:
    """lidar (B, N, C) fp32 with lidar_counts (B,) valid points per frame (None = N), gt_boxes (B, M, 7|9), gt_labels (B, M) with -1
    padding, gt_velocities (B, M, 2) or None, all on the GPU.

    Accept: per frame the candidates k = 0 .. Kc - 1 in order; candidate k is accepted iff cand >= 0, its BEV rectangle collides with
    no GT row of label >= 0, and with no ACCEPTED candidate k' < k (a rejected candidate blocks nothing).  Collision is the
    separating-axis test; touching counts, z is ignored, a box with w <= 0, l <= 0 or a NaN collides with nothing.
    Remove / append: the sweep's points inside the 3-D extent of an accepted box (`box_ops.points_in_boxes`' test) are removed, the
    survivors keep their order and bits, the accepted objects' points follow in candidate order and bank order (xyz = relative +
    centre, one fp32 addition), zeros pad to `capacity` rows (default: N + the largest per-frame candidate point total); a smaller
    capacity keeps the first `capacity` rows of that stream, the rule `filter_pad_lidar` has for max_points.

    Returns lidar_points (B, capacity, C), lidar_count int32 (B,) = min(kept + appended, capacity), gt_boxes / gt_labels /
    gt_velocities with Kc extra rows -- row M + k is candidate k's box, label and velocity (the bank's columns 7-8, zeros without) if
    accepted, else label -1 with a zero box and velocity; the original rows are copies, padding included; gt_velocities stays None
    when None comes in -- and accepted int32 (B, Kc).  `out`: optional preallocated tensors under the same keys (gt_labels int64)."""
    if lidar.dim() != 3 or lidar.shape[2] < 3 or lidar.dtype != torch.float32:
        raise L.BevfError("paste: expected fp32 (B, N, C>=3) lidar")
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] not in (7, 9) or gt_boxes.dtype != torch.float32:
        raise L.BevfError("paste: expected fp32 (B, M, 7 or 9) boxes")
    tensors = [lidar, gt_boxes, gt_labels, gt_velocities, bank.points]
    if any(t is not None and not t.is_cuda for t in tensors):
        raise L.BevfError(_NO_CPU)
    B, N, Cc = lidar.shape
    M, ncol = int(gt_boxes.shape[1]), int(gt_boxes.shape[2])
    dev = lidar.device
    if gt_boxes.shape[0] != B or tuple(gt_labels.shape) != (B, M) or gt_labels.dtype.is_floating_point or \
            (gt_velocities is not None and tuple(gt_velocities.shape) != (B, M, 2)):
        raise L.BevfError("paste: boxes must be (B, M, 7|9), labels (B, M) integers and velocities (B, M, 2)")
    if bank.device != dev or len(bank) == 0 or bank.channels != Cc:
        raise L.BevfError(f"paste: the bank must hold objects of {Cc}-channel points on {dev}; it holds {len(bank)} of "
                          f"{bank.channels} channels on {bank.device}")
    cand = np.ascontiguousarray(params.cand, dtype=np.int32)
    if cand.ndim != 2 or cand.shape[0] != B or not 0 < cand.shape[1] <= KC_MAX:
        raise L.BevfError(f"paste: candidates must be ({B}, 1..{KC_MAX}), got {cand.shape}")
    if cand.max() >= len(bank):
        raise L.BevfError(f"paste: candidate {int(cand.max())} is past the bank's {len(bank)} objects")
    Kc, K = int(cand.shape[1]), len(bank)
    capacity = default_capacity(bank, PasteParams(cand), N) if capacity is None else int(capacity)
    if capacity <= 0:
        raise L.BevfError(f"paste: capacity must be positive, got {capacity}")
    n_in = None
    if lidar_counts is not None:
        n_in = torch.as_tensor(lidar_counts).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if n_in.numel() != B:
            raise L.BevfError(f"paste: {B} frames but {n_in.numel()} counts")
    i32 = dict(dtype=torch.int32, device=dev)
    cand_d = torch.from_numpy(cand).to(dev)
    accepted = _buffer(out, "accepted", (B, Kc), torch.int32, dev)
    prefix = torch.empty(B, Kc + 1, **i32)
    o_boxes = _buffer(out, "gt_boxes", (B, M + Kc, ncol), torch.float32, dev)
    o_labels = _buffer(out, "gt_labels", (B, M + Kc), torch.int64, dev)
    vel = None if gt_velocities is None else gt_velocities.float().contiguous()
    o_vel = None if vel is None else _buffer(out, "gt_velocities", (B, M + Kc, 2), torch.float32, dev)
    L.paste_accept(gt_boxes.contiguous(), gt_labels.to(torch.int64).contiguous(), vel, bank.boxes, bank.labels, bank.obj_ptr, cand_d,
                   accepted, prefix, o_boxes, o_labels, o_vel, B, M, ncol, K, int(bank.boxes.shape[1]), Kc)
    o_pts = _buffer(out, "lidar_points", (B, capacity, Cc), torch.float32, dev)
    o_cnt = _buffer(out, "lidar_count", (B,), torch.int32, dev)
    work = torch.empty(L.paste_points_work_ints(B, N), **i32)
    L.paste_points(lidar.contiguous(), n_in, bank.points, bank.obj_ptr, bank.boxes, cand_d, accepted, prefix, o_pts, o_cnt, work, B, N,
                   Cc, K, int(bank.boxes.shape[1]), Kc, capacity)
    if gt_labels.dtype != torch.int64:
        o_labels = o_labels.to(gt_labels.dtype)
    return dict(lidar_points=o_pts, lidar_count=o_cnt, gt_boxes=o_boxes, gt_labels=o_labels, gt_velocities=o_vel, accepted=accepted)
