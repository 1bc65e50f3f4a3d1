#!/usr/bin/env python
"""The IoU-aware head's kernels: the IoU targets and the IoU / DIoU loss forward and backward at B = 8, BEV 128^2,
max_objects = 500 (100 objects per frame), and the decode of inference config 2 (B = 8, C = 10, BEV 128^2, K = 100) with and
without score rectification.

usage: iou_aware_bench.py [rounds] [--plain-only]

The legs are interleaved round by round in one process and timed with device events around `iters` back-to-back calls (no host
synchronisation inside a leg); the figure of a leg is the median over rounds of its per-call time.  Each leg is timed twice: called
from Python (the figure then includes what the host needs to enqueue the launches, which is more than these short kernels take),
and as `iters` calls captured into one graph and replayed (`_graph`: the device time alone).  --plain-only times the unrectified
decode alone and runs on a tree without the IoU-aware head, for a comparison across commits."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bevfusion_multimodal_3d_object_detection_amd import _lib as L  # noqa: E402
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct  # noqa: E402
from nms_bench import B, C, heads, timed  # noqa: E402

SIDE, K_DET, MAX_OBJECTS, N_OBJ, VOXEL = 128, 100, 500, 100, 2.048
PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)


def targets(dev, seed: int = 1):
    """prepare_centernet_targets for N_OBJ boxes per frame scattered over the range."""
    g = torch.Generator().manual_seed(seed)
    boxes, labels = [], []
    for _ in range(B):
        b = torch.zeros(N_OBJ, 7)
        b[:, :2] = torch.rand(N_OBJ, 2, generator=g) * 96.0 - 48.0
        b[:, 3:6] = torch.tensor([1.9, 4.5, 1.6]) * (0.8 + 0.4 * torch.rand(N_OBJ, 3, generator=g))
        b[:, 6] = torch.rand(N_OBJ, generator=g) * 6.283 - 3.1415
        boxes.append(b)
        labels.append(torch.randint(0, C, (N_OBJ,), generator=g))
    return ct.prepare_centernet_targets({"gt_boxes": boxes, "gt_labels": labels}, dev, bev_size=(SIDE, SIDE), num_classes=C,
                                        max_objects=MAX_OBJECTS)


def main() -> None:
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plain_only = "--plain-only" in sys.argv
    rounds = int(args[0]) if args else 15
    if not torch.cuda.is_available():
        raise SystemExit("iou_aware_bench needs the GPU: no 'cuda' device is visible")
    dev = torch.device("cuda:0")
    iters = 20
    pred = heads(SIDE, dev)
    legs = {"decode": lambda: L.centernet_decode(pred, K_DET, 0.3, VOXEL, -51.2, -51.2, True)}
    if not plain_only:
        g = torch.Generator().manual_seed(2)
        pred["iou"] = (torch.rand(B, 1, SIDE, SIDE, generator=g) * 2.0 - 1.0).to(dev)
        alpha = torch.full((C,), 0.5, device=dev)
        tgt = targets(dev)
        d = {k: torch.zeros_like(pred[k]) for k in ("iou", "offset", "size")}
        legs["decode_rectified"] = lambda: L.centernet_decode(pred, K_DET, 0.3, VOXEL, -51.2, -51.2, True, iou=pred["iou"], alpha=alpha)
        legs["iou_targets"] = lambda: L.iou_targets(pred, tgt, PC_RANGE)
        legs["loss_forward"] = lambda: L.iou_aware_loss(pred, tgt, PC_RANGE, 1.0, 1.0)
        legs["loss_backward"] = lambda: L.iou_aware_loss_bwd(pred, tgt, PC_RANGE, 1.0, 1.0, d["iou"], d["offset"], d["size"])
    graphs = {}
    for name, fn in legs.items():
        timed(fn, 3)                                                   # warm every leg before it is captured
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(iters):
                fn()
        graphs[name + "_graph"] = graph
        timed(graph.replay, 1)
    times = {k: [] for k in list(legs) + list(graphs)}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
        for k, gr in graphs.items():
            times[k].append(timed(gr.replay, 1) / iters)
    result = {"B": B, "C": C, "bev": SIDE, "K": K_DET, "rounds": rounds, "iters": iters, "unit": "us per call, median over rounds",
              **{k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}}
    if not plain_only:
        result.update(max_objects=MAX_OBJECTS, objects=int(tgt["reg_mask"].sum()),
                      count_plain=legs["decode"]()[4].tolist(), count_rectified=legs["decode_rectified"]()[4].tolist())
    print(json.dumps(result))


if __name__ == "__main__":
    main()
