#!/usr/bin/env python3
"""The GT-paste augmentation (gt_paste.py), timed at the flagship LiDAR size: 8 sweeps of 35 k points x 4 channels, 20 GT
boxes per frame, Kc = 16 candidates per frame out of a bank of 256 objects of about 200 points each.
  (a) `gt_paste.paste` against `augment.transform_filter_pad_lidar` on the same batch (the yardstick: the augmentation's other LiDAR
      leg), the two alternating in one process, and paste's share of the recorded training step;
  (b) the two entry points of the paste on their own (accept; remove + append) and `box_ops.points_in_boxes` of the sweeps against the
      20 GT boxes.
Device events around `inner` back-to-back calls, median over the rounds.
usage: gt_paste_bench.py [rounds]   (prints one JSON object per measurement)"""
import json
import math
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import box_ops, synth
from bevfusion_multimodal_3d_object_detection_amd import gt_paste as G

TRAIN_STEP_MS = (41.2, 42.6)   # the recorded config-4 training step


def timed_ab(fns, rounds=7, inner=5):
    """Medians (us) of each callable, measured in alternating rounds of one process."""
    for _ in range(2):
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
            e1.record(); torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) / inner)
    return [sorted(t)[len(t) // 2] * 1e3 for t in ts]


def make_bank(K, mean_points, C, rs, dev):
    """K car-sized objects spread over the range, labels 0-9, sizes around mean_points."""
    boxes = np.zeros((K, 9), dtype=np.float32)
    boxes[:, 0:2] = rs.uniform(-48, 48, (K, 2))
    boxes[:, 2] = rs.uniform(-2, 0, K)
    boxes[:, 3:6] = rs.uniform((1.6, 3.8, 1.4), (2.2, 5.0, 2.0), (K, 3))
    boxes[:, 6] = rs.uniform(-math.pi, math.pi, K)
    sizes = rs.randint(mean_points // 2, mean_points * 3 // 2 + 1, K)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    pts = rs.uniform(-1, 1, (int(ptr[-1]), C)).astype(np.float32)
    half = np.repeat(boxes[:, [4, 3, 5]] / 2, sizes, axis=0)
    yaw = np.repeat(boxes[:, 6], sizes)
    lx, ly = pts[:, 0] * half[:, 0], pts[:, 1] * half[:, 1]
    pts[:, 0], pts[:, 1], pts[:, 2] = lx * np.cos(yaw) - ly * np.sin(yaw), lx * np.sin(yaw) + ly * np.cos(yaw), pts[:, 2] * half[:, 2]
    labels = rs.randint(0, 10, K)
    return G.ObjectBank(torch.from_numpy(pts).to(dev), torch.from_numpy(ptr).to(dev), torch.from_numpy(boxes).to(dev),
                        torch.from_numpy(labels).to(dev))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    dev = torch.device("cuda")
    B, N, C, M, K = 8, 35000, 4, 20, 256
    rs = np.random.RandomState(0)
    bank = make_bank(K, 200, C, rs, dev)
    st = G.settings({"dataset": {"augmentation": {"lidar": {"object_sample": {"enable": True, "min_points": 5,
                                                                               "per_frame": {c: 2 if c < 6 else 1 for c in range(10)}}}}}})
    params = G.sample(st, bank, B, np.random.default_rng(0))
    assert params.Kc == 16
    _, pts, _ = synth.frame_inputs(B, 0, 0, 0, N, C, 0, seed=0x5EED)
    pts = pts.to(dev)
    boxes, labels = synth.gt_boxes(B, M, seed=5)
    boxes, labels = boxes.to(dev), labels.to(dev)
    world = A.sample(A.AugmentSettings(flip=True, scale=(0.95, 1.05), rotation=(-5.0, 5.0), translation=(0.5, 0.5, 0.2)), B, 1, (8, 8), (8, 8),
                     np.random.default_rng(0))
    cap = G.default_capacity(bank, params, N)
    out = G.paste(pts, None, boxes, labels, None, bank, params)
    acc = out["accepted"].cpu().numpy()
    removed = N + (acc * bank.host_sizes[np.clip(params.cand, 0, K - 1)]).sum(1) - out["lidar_count"].cpu().numpy()
    print(json.dumps({"scene": f"{B} x {N} x {C} points, {M} GT boxes, Kc = {params.Kc}, bank of {K} objects x ~200 points", "capacity": cap,
                      "accepted_per_frame": acc.sum(1).tolist(), "removed_per_frame": removed.tolist()}), flush=True)

    a, b = timed_ab([lambda: G.paste(pts, None, boxes, labels, None, bank, params, out=out),
                     lambda: A.transform_filter_pad_lidar(pts, None, world, N)], rounds)
    print(json.dumps({"leg": "(a) paste against transform_filter_pad_lidar", "paste_us": round(a, 1), "transform_filter_pad_lidar_us": round(b, 1),
                      "ratio": round(a / b, 3), "paste_share_of_training_step": [round(a / 1e3 / t, 4) for t in TRAIN_STEP_MS]}), flush=True)

    L = G.L
    i32 = dict(dtype=torch.int32, device=dev)
    cand = torch.from_numpy(params.cand).to(dev)
    accepted, prefix = torch.empty(B, 16, **i32), torch.empty(B, 17, **i32)
    ob, ol = torch.empty(B, M + 16, 9, device=dev), torch.empty(B, M + 16, dtype=torch.int64, device=dev)
    lab64 = labels.to(torch.int64)
    work = torch.empty(L.paste_points_work_ints(B, N), **i32)
    op, oc = torch.empty(B, cap, C, device=dev), torch.empty(B, **i32)
    stages = [
        ("paste_accept (8 x 16 candidates x 20 GT rows)",
         lambda: L.paste_accept(boxes, lab64, None, bank.boxes, bank.labels, bank.obj_ptr, cand, accepted, prefix, ob, ol, None, B, M, 9, K, 9, 16)),
        ("paste_points (count, compact, append)",
         lambda: L.paste_points(pts, None, bank.points, bank.obj_ptr, bank.boxes, cand, accepted, prefix, op, oc, work, B, N, C, K, 9, 16, cap)),
        ("points_in_boxes (8 x 35k points x 20 boxes)", lambda: box_ops.points_in_boxes(pts, boxes, None, labels)),
    ]
    stages[0][1]()
    us = timed_ab([s[1] for s in stages], rounds, 10)
    for (name, _), t in zip(stages, us):
        print(json.dumps({"stage": name, "us": round(t, 1)}), flush=True)


if __name__ == "__main__":
    main()
