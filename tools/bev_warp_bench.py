#!/usr/bin/env python3
"""The ego-motion BEV warp (temporal.py, csrc/bev_warp.hip), timed at B = 8, 128 x 128, C = 256: the forward in fp32
and bf16 and the fp32 backward, each against its algorithmic bytes -- one read plus one write of the map -- over the HBM peak bench.py
uses; and `bevf_bilinear_nhwc` at the same shape (128 x 128 -> 128 x 128), the project's own yardstick for a kernel that moves the
same bytes.  The map is a 5 degree turn with a 3 m step, so most cells have four inside corners.
Device events around `inner` back-to-back calls, the callables alternating in one process, median over the rounds.
usage: bev_warp_bench.py [rounds]   (prints one JSON object per measurement)"""
import json
import math
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import synth
from bevfusion_multimodal_3d_object_detection_amd.encoders import DEFAULT_PC_RANGE, pillar_grid

PEAK_HBM_GBS = 8000.0          # bench.py's


def timed_ab(fns, rounds=7, inner=20):
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
    B, H, W, C = 8, 128, 128, 256
    grid = pillar_grid(DEFAULT_PC_RANGE, H, W)[:4]
    c, s = math.cos(math.radians(5.0)), math.sin(math.radians(5.0))
    M = np.eye(4)
    M[:2, :2], M[:2, 3] = [[c, -s], [s, c]], [3.0, 0.4]
    ego_host = np.tile(M, (B, 1, 1))
    ego = torch.from_numpy(ego_host).to(dev)
    n = B * H * W * C
    x32 = synth.normal((n,), 1).to(dev)
    x16 = x32.bfloat16()
    y32, y16, dx = torch.empty_like(x32), torch.empty_like(x16), torch.empty_like(x32)
    print(json.dumps({"shape": f"B = {B}, {H} x {W}, C = {C}", "map": "5 degree turn, (3.0, 0.4) m step", "peak_hbm_gbs": PEAK_HBM_GBS}),
          flush=True)
    legs = [("bev_warp_f32", 4, lambda: L.bev_warp(x32, y32, ego, B, H, W, C, C, C, grid)),
            ("bev_warp_bf16", 2, lambda: L.bev_warp(x16, y16, ego, B, H, W, C, C, C, grid)),
            ("bev_warp_bwd_f32", 4, lambda: L.bev_warp_bwd(y32, dx, ego, B, H, W, C, C, grid, ego_host)),
            ("bilinear_nhwc_f32 (yardstick)", 4, lambda: L.bilinear_nhwc(x32, y32, B, H, W, C, C, H, W, C)),
            ("bilinear_nhwc_bf16 (yardstick)", 2, lambda: L.bilinear_nhwc(x16, y16, B, H, W, C, C, H, W, C))]
    us = timed_ab([leg[2] for leg in legs], rounds)
    for (name, es, _), t in zip(legs, us):
        nbytes = 2.0 * es * n                                   # algorithmic: one read and one write of the map
        gbs = nbytes / (t * 1e-6) / 1e9
        print(json.dumps({"kernel": name, "us": round(t, 1), "algorithmic_mb": round(nbytes / 1e6, 1), "gb_per_s": round(gbs, 1),
                          "hbm_fraction": round(gbs / PEAK_HBM_GBS, 3)}), flush=True)


if __name__ == "__main__":
    main()
