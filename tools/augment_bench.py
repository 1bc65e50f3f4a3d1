#!/usr/bin/env python3
"""The training augmentation (augment.py), timed at the flagship input sizes: 8 frames x 6 cameras of 900x1600 uint8
resized to 448x800, 8 sweeps of 35 k points x 4 channels, 5 radar tensors of 8 x 125 x 7, 8 x 20 boxes.
  (a) the augmented pipeline (augment_batch with every transform on) against the plain one (preprocess_camera_images + 8 x
      filter_pad_lidar) on the same inputs, the two legs alternating in one process;
  (b) each kernel stage on its own with the bytes it has to move (inputs read once, outputs written once) against the 6.29 TB/s
      measured copy rate.
Device events around `inner` back-to-back calls, median over the rounds.
usage: augment_bench.py [rounds]   (prints one JSON object per measurement)"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import preprocess, synth

COPY_GBS = 6290.0          # measured device-to-device copy rate
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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    dev = torch.device("cuda")
    B, ncam, src, out, N, C, maxp = 8, 6, (900, 1600), (448, 800), 35000, 4, 35000
    st = A.AugmentSettings(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, camera_flip=True, camera_scale=(0.9, 1.1), flip=True,
                           scale=(0.95, 1.05), rotation=(-5.0, 5.0), translation=(0.5, 0.5, 0.2), radar_noise_std=0.01)
    p = A.sample(st, B, ncam, src, out, np.random.default_rng(0))
    frames = torch.randint(0, 256, (B, ncam, *src, 3), dtype=torch.uint8, device=dev)
    _, pts, radars = synth.frame_inputs(B, 0, 0, 0, N, C, 5, 125, 7, seed=0x5EED)
    pts, radars = pts.to(dev), [r.to(dev) for r in radars]
    boxes, labels = synth.gt_boxes(B, 20, seed=5)
    boxes, labels = boxes.to(dev), labels.to(dev)
    rig = CR.default_rig()

    def plain():
        preprocess.preprocess_camera_images(frames, out)
        for b in range(B):
            preprocess.filter_pad_lidar(pts[b], maxp)

    def augmented():
        A.augment_batch(frames, pts, None, radars, boxes, labels, None, p, st, base_calib=rig, max_points=maxp)

    a, b = timed_ab([plain, augmented], rounds)
    print(json.dumps({"leg": "(a) pipeline, 8 x 6 x 900x1600 -> 448x800 + 8 x 35k points", "plain_us": round(a, 1), "augmented_us": round(b, 1),
                      "ratio": round(b / a, 3), "augmented_share_of_training_step": [round(b / 1e3 / t, 4) for t in TRAIN_STEP_MS]}),
          flush=True)

    n = B * ncam
    Ho, Wo = out
    wins = p.windows.reshape(-1, 4)
    tabs = A.device_tables(wins, src, out, dev)
    bh, kh, ksh, bv, kv, ksv = tabs
    u8 = torch.empty(n, Ho, Wo, 3, dtype=torch.uint8, device=dev)
    gray = torch.empty(n, dtype=torch.int64, device=dev)
    x = frames.view(n, *src, 3)
    f32 = torch.empty(n, 3, Ho, Wo, device=dev)
    jit = torch.from_numpy(p.jitter.reshape(-1, 4).astype(np.float32)).to(dev)
    flip = torch.from_numpy(p.flip.reshape(-1).astype(np.int32)).to(dev)
    L = A.L
    mat = torch.from_numpy(p.mat12()).to(dev)
    lout = torch.empty(B, maxp, C, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    work = torch.empty(L.points_affine_work_floats(B, N, C), device=dev)
    rad = radars[0].clone()
    bx = boxes.clone()
    sc = torch.from_numpy(p.scale.astype(np.float32)).to(dev)
    lab = labels.to(torch.int64)
    window_bytes = int(((wins[:, 1] - wins[:, 0]) * (wins[:, 3] - wins[:, 2])).sum()) * 3
    stages = [
        ("resample_tables_box (48 images)", lambda: A.device_tables(wins, src, out, dev),
         4 * n * (Wo * (2 + ksh) + Ho * (2 + ksv))),
        ("resize_crop_u8", lambda: L.resize_crop_u8(x, u8, gray, n, src[0], src[1], Ho, Wo, bh, kh, ksh, bv, kv, ksv),
         window_bytes + n * Ho * Wo * 3),
        ("jitter_flip_normalize_u8", lambda: L.jitter_flip_normalize_u8(u8, f32, gray, jit, flip, n, Ho, Wo, st.mean, st.std),
         n * Ho * Wo * (3 + 12)),
        ("points_affine_filter_pad (8 x 35k x 4)", lambda: L.points_affine_filter_pad(pts, None, mat, lout, cnt, work, B, N, C, maxp, None,
                                                                                       A.PC_RANGE), 4 * B * C * (N + maxp)),
        ("points_affine (one radar tensor, 8 x 125 x 7)", lambda: L.points_affine(rad, mat, None, 0.0, B, 125, 7, None), 2 * 4 * B * 125 * 3),
        ("boxes_affine (8 x 20 x 9)", lambda: L.boxes_affine(bx, lab, None, mat, sc, B, 20, 9), 2 * 4 * B * 20 * 9),
    ]
    us = timed_ab([s[1] for s in stages], rounds, 10)
    for (name, _, nbytes), t in zip(stages, us):
        gbs = nbytes / t / 1e3
        print(json.dumps({"stage": name, "us": round(t, 1), "algorithmic_mb": round(nbytes / 1e6, 3), "gb_per_s": round(gbs, 1),
                          "frac_of_copy_rate": round(gbs / COPY_GBS, 4)}), flush=True)
    pa, pb = timed_ab([lambda: preprocess.preprocess_camera_images(frames, out),
                       lambda: [preprocess.filter_pad_lidar(pts[i], maxp) for i in range(B)]], rounds)
    print(json.dumps({"leg": "plain stages", "preprocess_camera_images_us": round(pa, 1), "8 x filter_pad_lidar_us": round(pb, 1)}), flush=True)


if __name__ == "__main__":
    main()
