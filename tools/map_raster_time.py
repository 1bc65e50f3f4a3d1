#!/usr/bin/env python3
"""The map rasteriser (map_targets.py, csrc/map_raster.hip), timed at the workload shape: B = 8 frames, K = 6 classes,
200 x 200 cells over +-50 m, synthetic maps of a few hundred shapes and a few thousand edges per frame, under one random world
transform per frame.
1. `bevf_map_raster_u8` (its two launches, the pre-pass map_raster_shapes and the main pass map_raster_fill, buffers allocated once)
   against `torch.zeros` of the same number of output bytes -- the floor: one write of the masks -- in alternating rounds of one process,
   device events around back-to-back calls, medians.  The split between the two kernels comes from running this tool under
   `rocprofv3 --kernel-trace --stats` (give --no-host then).
2. `map_targets.rasterize` as the training step calls it (allocations and the copies of the transform included).
3. The numpy fp64 restatement of the rules (tests/map_raster_ref.py) on the same input: the host alternative, and a check -- the
   device result must equal it byte for byte.
It also prints what the algorithm moves and computes: the output bytes, the edge tests of a plain cell x edge loop and the tests left
after the tile cull (counted on the host with the kernel's own box rule).
usage: map_raster_time.py [rounds] [--no-host]   (prints one JSON object per measurement)"""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import augment, map_targets, seg_head

B, K, HO, WO = 8, 6, 200, 200
RANGE = [-50.0, -50.0, 50.0, 50.0]
TILE = 32


def _blob(rng, n, cx, cy, r):
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
    rad = r * rng.uniform(0.6, 1.0, n)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)


def synthetic_frames(seed=3):
    """Per frame: one drivable area of 400 vertices with four holes, 200 polygons of 6 .. 24 vertices (crossings, walkways, car parks,
    stop lines) and 100 polylines of 4 .. 12 points (dividers)."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(B):
        shapes = [dict(cls=0, polygon=_blob(rng, 400, 0.0, 0.0, 55.0),
                       holes=[_blob(rng, 40, *rng.uniform(-30, 30, 2), 8.0) for _ in range(4)])]
        for n in range(200):
            shapes.append(dict(cls=1 + n % 4, polygon=_blob(rng, int(rng.integers(6, 25)), *rng.uniform(-55, 55, 2), rng.uniform(2.0, 9.0))))
        for n in range(100):
            pts = rng.uniform(-55, 55, 2) + np.cumsum(rng.normal(0.0, 4.0, (int(rng.integers(4, 13)), 2)), 0)
            shapes.append(dict(cls=5, line=pts, width=float(rng.uniform(0.2, 0.6))))
        frames.append(shapes)
    return frames


def transforms(seed=4):
    rng = np.random.default_rng(seed)
    p = augment.neutral_params(B, 1, (4, 4), (4, 4))
    for b in range(B):
        s = float(rng.uniform(0.9, 1.1))
        p.bev_aug[b] = augment.world_transform(rng.random() < 0.5, rng.random() < 0.5, float(rng.uniform(-0.4, 0.4)), s, rng.normal(0, 0.5, 3))
        p.scale[b] = s
    return p


def counts(host, params):
    """Edges, the edge tests of a plain cell x edge loop, and those left after the 32 x 32 tile cull (box of the transformed vertices,
    a polyline's grown by its half width, against the tile's span of centres)."""
    v = host.vertices.numpy().astype(np.float64)
    ro, so, fo = (t.numpy() for t in (host.ring_offsets, host.shape_offsets, host.frame_offsets))
    kind, width = host.shape_kind.numpy(), host.shape_width.numpy().astype(np.float64)
    m = params.mat12().astype(np.float64)
    x0, y0, vx, vy = seg_head.range_grid(RANGE, HO, WO)
    edges = plain = culled = 0
    for b in range(B):
        for s in range(fo[b], fo[b + 1]):
            a, e = ro[so[s]], ro[so[s + 1]]
            ne = int(e - a) - (1 if kind[s] else 0)
            xt = m[b, 0] * v[a:e, 0] + m[b, 1] * v[a:e, 1] + m[b, 3]
            yt = m[b, 4] * v[a:e, 0] + m[b, 5] * v[a:e, 1] + m[b, 7]
            hw = 0.5 * width[s] * float(params.scale[b]) if kind[s] else 0.0
            edges += ne
            plain += ne * HO * WO
            for ti in range(0, HO, TILE):
                for tj in range(0, WO, TILE):
                    cx0, cx1 = x0 + (tj + 0.5) * vx, x0 + (min(tj + TILE, WO) - 0.5) * vx
                    cy0, cy1 = y0 + (ti + 0.5) * vy, y0 + (min(ti + TILE, HO) - 0.5) * vy
                    if xt.min() - hw <= cx1 and cx0 <= xt.max() + hw and yt.min() - hw <= cy1 and cy0 <= yt.max() + hw:
                        culled += ne * TILE * TILE
    return edges, plain, culled


def timed_ab(fns, rounds=7, inner=20, warm=2):
    """Medians (us) of each callable, measured in alternating rounds of one process."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / inner)
    return [sorted(t)[len(t) // 2] * 1e3 for t in ts]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    if not torch.cuda.is_available():
        raise SystemExit("map_raster_time.py measures on the GPU: no 'cuda' device is visible")
    dev = torch.device("cuda")
    frames, params = synthetic_frames(), transforms()
    host = map_targets.pack_shapes(frames, num_classes=K, device="cpu")
    shapes = map_targets.pack_shapes(frames, num_classes=K, device=dev)
    S, V = shapes.num_shapes, shapes.vertices.shape[0]
    edges, plain, culled = counts(host, params)
    out_bytes = B * K * HO * WO
    print(json.dumps({"shape": f"B = {B}, K = {K}, {HO} x {WO}", "shapes": S, "vertices": V, "edges": int(edges), "output_bytes": out_bytes,
                      "vertex_edge_and_record_bytes": 8 * V + 32 * V + 64 * S, "edge_tests_plain": int(plain),
                      "edge_tests_after_tile_cull": int(culled)}), flush=True)
    grid = seg_head.range_grid(RANGE, HO, WO)
    mat = augment._mat(params, B, dev)
    scale = torch.from_numpy(params.scale.astype(np.float32)).to(dev)
    work = torch.empty(L.map_raster_work_bytes(S, V), dtype=torch.uint8, device=dev)
    out = torch.empty(B, K, HO, WO, dtype=torch.uint8, device=dev)

    def kernels():
        L.map_raster(shapes.vertices, shapes.ring_offsets, shapes.shape_offsets, shapes.shape_class, shapes.shape_kind, shapes.shape_width,
                     shapes.frame_offsets, mat, scale, work, out, B, K, HO, WO, grid)

    legs = [("bevf_map_raster_u8 (pre-pass + main pass)", kernels),
            ("torch.zeros of the output bytes (floor)", lambda: torch.zeros(out_bytes, dtype=torch.uint8, device=dev)),
            ("map_targets.rasterize (allocations and transform copies included)", lambda: map_targets.rasterize(shapes, RANGE, (HO, WO), params))]
    for (name, _), t in zip(legs, timed_ab([leg[1] for leg in legs], rounds)):
        print(json.dumps({"leg": name, "us": round(t, 1)}), flush=True)
    if "--no-host" in sys.argv:
        return
    from tests import map_raster_ref as R
    t0 = time.perf_counter()
    ref = R.rasterize_np(host, grid, HO, WO, R.mat12(params, B), R.scale32(params, None, B))
    t_host = time.perf_counter() - t0
    kernels()
    print(json.dumps({"leg": "numpy fp64 restatement on the host, same input", "ms": round(t_host * 1e3, 1),
                      "device_equals_it": bool(np.array_equal(out.cpu().numpy(), ref)), "cells_set": int(ref.sum())}), flush=True)


if __name__ == "__main__":
    main()
