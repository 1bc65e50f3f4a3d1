"""Segmentation targets rasterised from map polygons and polylines on the device (csrc/map_raster.hip).

The BEV map-segmentation head (seg_head.py) trains on (B, K, Ho, Wo) uint8 masks.  The map stays vector geometry here: `pack_shapes`
packs one batch's polygons (with holes) and polylines (with a width) into one CSR set of device tensors, once per dataset sample;
`rasterize` moves the vertices through the step's world transform -- the `T` of `augment.augment_batch`, so the masks live in the
same augmented world as the points and the boxes -- and fills the masks, all in fp64 by rules that a numpy restatement reproduces bit
for bit (include/bevf.h).  `rasterize_for` does it on a `BEVSegmentationHead`'s grid and classes, and
`augment.augment_batch(..., map_shapes=, map_grid=)` returns the masks as `seg_targets` beside the rest of the batch.  No CPU fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from . import augment as A
from .seg_head import _size, range_grid

MAX_CLASSES = 64
POLYGON, POLYLINE = 0, 1


@dataclass(frozen=True)
class MapShapes:
    """One batch's map shapes, packed (the tensors of bevf_map_raster_u8, on one device): vertices fp32 (V, 2) in metres in the
    frame's ego / LiDAR BEV frame, ring_offsets int32 (R + 1) into vertices, shape_offsets int32 (S + 1) into rings, shape_class
    int32 (S), shape_kind int32 (S) (0 = polygon, 1 = polyline), shape_width fp32 (S), frame_offsets int32 (B + 1) into shapes.
    num_classes is None, and shape_class holds -1, while the shapes carry class NAMES that no class list has resolved yet
    (`class_names`, one per shape; `with_classes` resolves them)."""
    vertices: torch.Tensor
    ring_offsets: torch.Tensor
    shape_offsets: torch.Tensor
    shape_class: torch.Tensor
    shape_kind: torch.Tensor
    shape_width: torch.Tensor
    frame_offsets: torch.Tensor
    B: int
    num_classes: Optional[int]
    class_names: Optional[Tuple[str, ...]] = None

    @property
    def num_shapes(self) -> int:
        return int(self.shape_class.numel())

    def with_classes(self, classes: Sequence[str]) -> "MapShapes":
        """The same shapes with their class names resolved through `classes` (index = position); an unknown name raises."""
        if self.class_names is None:
            raise L.BevfError("MapShapes.with_classes: the shapes were packed with class indices, there is no name to resolve")
        idx = _resolve(self.class_names, tuple(classes), "MapShapes.with_classes")
        cls = torch.from_numpy(np.asarray(idx, dtype=np.int32).reshape(-1)).to(self.shape_class.device)
        return replace(self, shape_class=cls, num_classes=len(classes), class_names=None)


def _resolve(names: Sequence[str], classes: Tuple[str, ...], what: str):
    lut = {str(c): k for k, c in enumerate(classes)}
    if not 1 <= len(classes) <= MAX_CLASSES or len(lut) != len(classes):
        raise L.BevfError(f"{what}: need 1 .. {MAX_CLASSES} distinct class names, got {list(classes)}")
    unknown = sorted({n for n in names if n not in lut})
    if unknown:
        raise L.BevfError(f"{what}: unknown class {unknown} (known: {list(classes)})")
    return [lut[n] for n in names]


def _ring(pts, least: int, what: str) -> np.ndarray:
    try:
        a = np.asarray(pts, dtype=np.float32)
    except (TypeError, ValueError):
        raise L.BevfError(f"{what}: expected an (n, 2) array of x, y in metres") from None
    if a.ndim != 2 or a.shape[1] != 2:
        raise L.BevfError(f"{what}: expected an (n, 2) array of x, y in metres, got shape {a.shape}")
    if a.shape[0] < least:
        raise L.BevfError(f"{what}: {a.shape[0]} vertices, needs at least {least}")
    return a                                                      # (non-finite vertices pass: the device drops such a shape)


def pack_shapes(frames, classes: Optional[Sequence[str]] = None, num_classes: Optional[int] = None,
                device: Union[str, torch.device] = "cuda") -> MapShapes:
    """frames: one list of shape dicts per frame (a frame may be empty).  A polygon is {"cls": name or index, "polygon": exterior
    (n, 2), "holes": [(m, 2), ...]} (holes optional; rings are closed implicitly, do not repeat the first vertex), a polyline
    {"cls": ..., "line": (n, 2), "width": metres}.  `classes` maps names to indices and sets K = len(classes); with class indices
    alone give `num_classes`.  With names and no `classes` the names are kept for `rasterize_for` to resolve through the head's.
    Packed on the host (it is data loading: once per dataset sample), then one copy per tensor.  Raises BevfError for an unknown
    class, an index outside 0 .. K-1, a polygon ring under 3 vertices, a line under 2, a negative or non-finite width and wrong
    array shapes."""
    what = "pack_shapes"
    if classes is not None:
        classes = tuple(str(c) for c in classes)
        if num_classes is not None and int(num_classes) != len(classes):
            raise L.BevfError(f"{what}: num_classes = {num_classes} but {len(classes)} classes are named")
        num_classes = len(classes)
        _resolve((), classes, what)
    if num_classes is not None and not 1 <= int(num_classes) <= MAX_CLASSES:
        raise L.BevfError(f"{what}: num_classes must be 1 .. {MAX_CLASSES}, got {num_classes}")
    rings, ring_off, shape_off, cls, kinds, widths, frame_off = [], [0], [0], [], [], [], [0]
    for b, shapes in enumerate(frames):
        for n, sh in enumerate(shapes):
            at = f"{what}: frame {b}, shape {n}"
            if not isinstance(sh, dict) or "cls" not in sh or ("polygon" in sh) == ("line" in sh):
                raise L.BevfError(f"{at}: a shape is a dict with 'cls' and either 'polygon' (+ 'holes') or 'line' + 'width'")
            if "polygon" in sh:
                mine = [_ring(sh["polygon"], 3, f"{at}: polygon")]
                mine += [_ring(h, 3, f"{at}: hole {k}") for k, h in enumerate(sh.get("holes") or ())]
                kinds.append(POLYGON)
                widths.append(0.0)
            else:
                mine = [_ring(sh["line"], 2, f"{at}: line")]
                try:
                    w = float(sh["width"])
                except (KeyError, TypeError, ValueError):
                    raise L.BevfError(f"{at}: a line needs 'width' in metres") from None
                if not (math.isfinite(w) and w >= 0.0):
                    raise L.BevfError(f"{at}: the width must be finite and >= 0, got {w}")
                kinds.append(POLYLINE)
                widths.append(w)
            cls.append(sh["cls"])
            for r in mine:
                rings.append(r)
                ring_off.append(ring_off[-1] + r.shape[0])
            shape_off.append(len(rings))
        frame_off.append(len(cls))
    by_name = [isinstance(c, str) for c in cls]
    names = None
    if any(by_name) and classes is None:
        if not all(by_name):
            raise L.BevfError(f"{what}: class names and class indices are mixed and no `classes` list resolves the names")
        if num_classes is not None:
            raise L.BevfError(f"{what}: class names need `classes`, not num_classes alone")
        names, idx = tuple(cls), [-1] * len(cls)
    else:
        if num_classes is None:
            raise L.BevfError(f"{what}: class indices need num_classes= or classes=")
        resolved = iter(_resolve([c for c in cls if isinstance(c, str)], classes or (), what) if any(by_name) else ())
        idx = []
        for c in cls:
            if isinstance(c, str):
                idx.append(next(resolved))
                continue
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < int(num_classes):
                raise L.BevfError(f"{what}: class index {c!r} outside 0 .. {int(num_classes) - 1}")
            idx.append(int(c))
    if ring_off[-1] >= 2 ** 31:
        raise L.BevfError(f"{what}: more than 2^31 vertices")
    device = torch.device(device)
    verts = np.concatenate(rings, 0) if rings else np.zeros((0, 2), dtype=np.float32)

    def dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(device)

    return MapShapes(dev(verts, np.float32), dev(ring_off, np.int32), dev(shape_off, np.int32), dev(idx, np.int32).reshape(-1),
                     dev(kinds, np.int32).reshape(-1), dev(widths, np.float32).reshape(-1), dev(frame_off, np.int32),
                     len(frame_off) - 1, None if num_classes is None else int(num_classes), names)


def rasterize(shapes: MapShapes, output_range, output_size, mat=None, scale=None) -> torch.Tensor:
    """uint8 (B, K, Ho, Wo): mask k of frame b is 1 where a shape of class k contains (polygon, even-odd over its rings) or hits
    (polyline, within half its width) the cell's centre, on output_size = (rows, columns) cells covering output_range = [xmin, ymin,
    xmax, ymax] (row i is y, column j is x: seg_head.range_grid).  mat: the frames' world transform, whatever `augment._mat` takes --
    an AugmentParams, a (B, 4, 4) / (B, 3, 4) / (B, 12) array or tensor --, None = identity; the vertices are transformed, then
    rasterised.  scale: the frames' scale (B,), by which a polyline's width grows; None = the AugmentParams' scale, else 1.
    Stream-ordered on the current stream, no host synchronisation."""
    if not isinstance(shapes, MapShapes):
        raise L.BevfError(f"rasterize: shapes must be a MapShapes (pack_shapes), got {type(shapes).__name__}")
    if shapes.num_classes is None:
        raise L.BevfError("rasterize: the shapes carry unresolved class names; pack with classes= or call with_classes / rasterize_for")
    Ho, Wo = _size(output_size)
    grid = range_grid(output_range, Ho, Wo, "rasterize: output_range")
    dev = shapes.vertices.device
    if dev.type != "cuda":
        raise L.BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    B, K = shapes.B, shapes.num_classes
    if isinstance(mat, A.AugmentParams) and scale is None:
        scale = mat.scale
    m = None if mat is None else A._mat(mat, B, dev)
    s = None
    if scale is not None:
        sc = scale.detach().cpu().double().numpy() if isinstance(scale, torch.Tensor) else np.asarray(scale, dtype=np.float64)
        if sc.size != B:
            raise L.BevfError(f"rasterize: {B} frames but {sc.size} scales")
        s = torch.from_numpy(np.ascontiguousarray(sc.reshape(-1).astype(np.float32))).to(dev)
    work = torch.empty(L.map_raster_work_bytes(shapes.num_shapes, shapes.vertices.shape[0]), dtype=torch.uint8, device=dev)
    out = torch.empty(B, K, int(Ho), int(Wo), dtype=torch.uint8, device=dev)
    L.map_raster(shapes.vertices, shapes.ring_offsets, shapes.shape_offsets, shapes.shape_class, shapes.shape_kind,
                 shapes.shape_width, shapes.frame_offsets, m, s, work, out, B, K, int(Ho), int(Wo), grid)
    return out


def rasterize_for(head, shapes: MapShapes, params=None) -> torch.Tensor:
    """`rasterize` on a BEVSegmentationHead's output_range, output_size and classes: shapes packed by name are resolved through
    head.classes, shapes packed by index must have been packed for head.num_classes.  params: the step's AugmentParams (or anything
    `rasterize` takes as mat), None = no augmentation."""
    if not isinstance(shapes, MapShapes):
        raise L.BevfError(f"rasterize_for: shapes must be a MapShapes (pack_shapes), got {type(shapes).__name__}")
    if shapes.class_names is not None:
        shapes = shapes.with_classes(head.classes)
    if shapes.num_classes != head.num_classes:
        raise L.BevfError(f"rasterize_for: the shapes were packed for {shapes.num_classes} classes, the head has {head.num_classes}")
    return rasterize(shapes, head.output_range, head.output_size, params)
