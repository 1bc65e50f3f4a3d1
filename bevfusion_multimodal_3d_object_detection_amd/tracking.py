"""Multi-object tracking on the decode path (csrc/track.hip): CenterPoint's greedy centre-distance tracker, on device.

`Tracker` owns the state of B independent streams (a stream = one batch row of the detector) and advances it by one kernel launch
per `step`: every detection is projected back by its own velocity and the ego motion, matched greedily in score order to the
nearest free track inside its class's distance limit, unmatched tracks coast for up to `max_age` steps, unmatched detections start
tracks.  The exact rules are in include/bevf.h (bevf_track_step_f32).  `ego_motion` is the tensor `temporal.ego_motion` produces and
the BEV warp consumes: current frame -> previous frame, rigid.  Not in the reference (it stops at boxes).
"""
from __future__ import annotations

from typing import Any, Dict, List, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L

# CenterPoint's published nuScenes limits (metres a centre may lie from its projected track), by class name
CENTERPOINT_MAX_DIST = {"car": 4.0, "truck": 4.0, "bus": 5.5, "trailer": 3.0, "pedestrian": 1.0, "motorcycle": 13.0, "bicycle": 3.0}
DEFAULT_MAX_DIST = 4.0                                   # for a class the table does not name


def class_max_dist(class_names: Sequence[str], limits: Union[float, Mapping[str, float], None] = None,
                   default: float = DEFAULT_MAX_DIST) -> List[float]:
    """Per-class limits in the order of class_names: a scalar for all, or a name -> metres mapping (None: CENTERPOINT_MAX_DIST) whose
    missing names take `default`."""
    if limits is None:
        limits = CENTERPOINT_MAX_DIST
    if isinstance(limits, Mapping):
        unknown = sorted(set(limits) - set(class_names))
        if unknown and limits is not CENTERPOINT_MAX_DIST:
            raise L.BevfError(f"max_dist names classes the model does not have: {unknown} (classes: {list(class_names)})")
        return [float(limits.get(name, default)) for name in class_names]
    return [float(limits)] * len(class_names)


def tracking_settings(config: Dict[str, Any], class_names: Sequence[str]) -> Dict[str, Any]:
    """Keyword arguments for `Tracker` from the `tracking:` section of a reference-style YAML (as a dict): max_age, birth_score,
    class_aware, max_tracks, and max_dist as a scalar or a class-name -> metres mapping (classes it does not name take
    DEFAULT_MAX_DIST; no max_dist at all: CENTERPOINT_MAX_DIST).  Other missing keys keep the Tracker's defaults."""
    try:
        tr = config["tracking"]
    except (KeyError, TypeError):
        raise KeyError("the config has no 'tracking' section") from None
    tr = tr or {}
    out: Dict[str, Any] = {"num_classes": len(class_names)}
    for key, cast in (("max_age", int), ("birth_score", float), ("max_tracks", int)):
        if key in tr:
            out[key] = cast(tr[key])
    if "class_aware" in tr:
        if not isinstance(tr["class_aware"], bool):                  # bool("false") is True
            raise L.BevfError(f"tracking.class_aware must be true or false, got {tr['class_aware']!r}")
        out["class_aware"] = tr["class_aware"]
    out["max_dist"] = class_max_dist(class_names, tr.get("max_dist"))
    return out


_KEYS = ("boxes", "velocities", "scores", "labels", "count")


class Tracker:
    """The tracks of B streams on one device.  max_dist: metres, a scalar or one per class label; max_age: a track unmatched for
    more than max_age steps is dropped; birth_score: an unmatched detection below it starts no track; class_aware: a detection
    only matches a track of its own label.  At most max_tracks (<= 1024) tracks per stream; what does not fit is counted in
    `overflow`."""

    def __init__(self, B: int, num_classes: int, max_tracks: int = 256, max_dist: Union[float, Sequence[float]] = DEFAULT_MAX_DIST,
                 max_age: int = 3, birth_score: float = 0.0, class_aware: bool = True, device="cuda"):
        if int(B) <= 0 or int(num_classes) <= 0:
            raise L.BevfError(f"Tracker: B and num_classes must be positive, got {B} and {num_classes}")
        if not 0 < int(max_tracks) <= L.TRACK_MAX_T:
            raise L.BevfError(f"Tracker: max_tracks must be in 1 .. {L.TRACK_MAX_T}, got {max_tracks}")
        if int(max_age) < 0:
            raise L.BevfError(f"Tracker: max_age must be >= 0, got {max_age}")
        limits = [float(max_dist)] * int(num_classes) if np.isscalar(max_dist) else [float(v) for v in max_dist]
        if len(limits) != int(num_classes):
            raise L.BevfError(f"Tracker: max_dist holds {len(limits)} limits for {num_classes} classes")
        if not all(v >= 0.0 for v in limits):
            raise L.BevfError(f"Tracker: max_dist must be >= 0 metres, got {limits}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.BevfError("Tracker runs on MI355X only: pass a 'cuda' device (there is no CPU fallback)")
        self.B, self.num_classes, self.max_tracks = int(B), int(num_classes), int(max_tracks)
        self.max_age, self.birth_score, self.class_aware = int(max_age), float(birth_score), bool(class_aware)
        self.max_dist = torch.tensor(limits, dtype=torch.float32, device=self.device)
        self._identity = torch.eye(4, dtype=torch.float64, device=self.device).repeat(self.B, 1, 1)
        self.state: Dict[str, torch.Tensor] = {
            name: torch.zeros((self.B, self.max_tracks) + tail, dtype=dtype, device=self.device) for name, dtype, tail in L.TRACK_STATE}
        self.state["track_count"] = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.state["next_id"] = torch.zeros(self.B, dtype=torch.int64, device=self.device)
        self.state["track_id"].fill_(-1)

    # ---- inputs ----
    def _pack(self, frames: Sequence[Mapping[str, torch.Tensor]]):
        """The decode's list of per-frame dicts -> padded tensors (one host-side loop; the padded form avoids it)."""
        if len(frames) != self.B:
            raise L.BevfError(f"Tracker.step: {len(frames)} frames for {self.B} streams")
        counts = [int(f["boxes"].shape[0]) for f in frames]
        N = max(counts)
        dev = self.device
        boxes, vels = torch.zeros(self.B, N, 7, device=dev), torch.zeros(self.B, N, 2, device=dev)
        scores, labels = torch.zeros(self.B, N, device=dev), torch.zeros(self.B, N, dtype=torch.int64, device=dev)
        for b, (f, n) in enumerate(zip(frames, counts)):
            if n:
                boxes[b, :n], vels[b, :n] = f["boxes"].to(dev), f["velocities"].to(dev)
                scores[b, :n], labels[b, :n] = f["scores"].to(dev), f["labels"].to(dev)
        return boxes, vels, scores, labels, torch.tensor(counts, dtype=torch.int32, device=dev)

    def _per_stream(self, v, dtype, tail) -> torch.Tensor:
        """A tensor as it is (track_step checks it); a number -> filled on the device (no copy from the host, so the default dt can be
        captured); an array -> a (B,) + tail device tensor, broadcast over the streams (one host-to-device copy)."""
        if isinstance(v, torch.Tensor):
            return v
        if np.isscalar(v) and not tail:
            return torch.full((self.B,), float(v), dtype=dtype, device=self.device)
        t = torch.as_tensor(np.asarray(v, dtype=np.float64), dtype=dtype)
        if t.dim() == len(tail):
            t = t.expand((self.B,) + tail)
        return t.contiguous().to(self.device)

    def step(self, detections, ego_motion=None, dt=0.5) -> Dict[str, torch.Tensor]:
        """Advance every stream by one frame.  detections: (boxes, velocities, scores, labels, count) padded device tensors, a dict of
        them (as `decode_padded` returns), or the decode's list of per-frame dicts (packed on the host).  ego_motion: float64 (B,4,4)
        current -> previous frame (`temporal.ego_motion`; numpy or tensor), None = the vehicle stood still; dt: seconds since the
        previous step, a number or a (B,) float32 tensor.  Returns det_track_id int64 (B,N), det_hits / det_slot int32 (B,N) and
        overflow int32 (B,) on the device.  With padded tensors and device ego_motion / dt nothing is synchronised."""
        if isinstance(detections, Mapping):
            missing = [k for k in _KEYS if k not in detections]
            if missing:
                raise L.BevfError(f"Tracker.step: the detections dict lacks {missing}")
            detections = tuple(detections[k] for k in _KEYS)
        elif isinstance(detections, (list, tuple)) and (len(detections) == 0 or isinstance(detections[0], Mapping)):
            detections = self._pack(detections)
        if not isinstance(detections, (list, tuple)) or len(detections) != 5:
            raise L.BevfError("Tracker.step: detections are (boxes, velocities, scores, labels, count), a dict of them, or the "
                              "decode's list of per-frame dicts")
        boxes, vels, scores, labels, count = detections
        if isinstance(boxes, torch.Tensor) and boxes.dim() == 3 and boxes.shape[0] != self.B:
            raise L.BevfError(f"Tracker.step: detections of {boxes.shape[0]} frames for {self.B} streams")
        ego = self._identity if ego_motion is None else self._per_stream(ego_motion, torch.float64, (4, 4))
        dtt = self._per_stream(dt, torch.float32, ())
        shape = tuple(boxes.shape[:2]) if isinstance(boxes, torch.Tensor) and boxes.dim() == 3 else (self.B, 0)
        out = {name: torch.empty(shape, dtype=dtype, device=self.device) for name, dtype in L.TRACK_OUT}
        out["overflow"] = torch.empty(self.B, dtype=torch.int32, device=self.device)
        L.track_step(boxes, vels, scores, labels, count, ego, dtt, self.max_dist, self.state, out, self.max_age, self.birth_score,
                     self.class_aware)
        return out

    # ---- state ----
    def tracks(self) -> List[Dict[str, torch.Tensor]]:
        """Per stream, the live tracks as views of the state: box (n,7), velocity (n,2), score, label, id, age, hits (n,), in the
        sensor frame of the last step.  Reads track_count back (one synchronisation)."""
        counts = self.state["track_count"].cpu().tolist()
        return [{name[len("track_"):]: self.state[name][b, :n] for name, _, _ in L.TRACK_STATE} for b, n in enumerate(counts)]

    def reset(self, streams: Optional[Sequence[int]] = None, ids: bool = False) -> None:
        """Forget the tracks of `streams` (None: all).  next_id keeps counting, so ids stay unique over a reset, unless ids=True."""
        rows = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.int64, device=self.device)
        for name, _, _ in L.TRACK_STATE:
            self.state[name][rows] = -1 if name == "track_id" else 0
        self.state["track_count"][rows] = 0
        if ids:
            self.state["next_id"][rows] = 0
