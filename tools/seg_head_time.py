#!/usr/bin/env python3
"""The BEV map-segmentation head (seg_head.py, csrc/bev_seg.hip), timed.
1. The grid resample at B = 8, C = 256, 128 x 128 -> 200 x 200, fp32: forward and backward against their algorithmic bytes (one read
   of the input map plus one write of the output, and the reverse), with `bevf_bilinear_nhwc_f32` / `bevf_bilinear_bwd_nhwc_f32`
   (the atomic backward, its zero fill included) on the same shapes in the same run as the yardstick.
2. The focal loss, forward plus backward, at B = 8, K = 6, 200 x 200, and the IoU counts at seven thresholds.
3. The config-4-shaped detector (camera+LiDAR, 6 x 448 x 800 images, 35 k points, BEV 50 x 50, B = 8): the eval forward and the
   training step (forward, CenterNetLoss (+ SegFocalLoss), backward) without the seg head -- the parent's behaviour -- and with it
   (6 classes, 200 x 200 cells over +-50 m).
Device events around back-to-back calls, the legs alternating in one process, medians over the rounds.
usage: seg_head_time.py [rounds] [--no-detector]   (prints one JSON object per measurement)"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct
from bevfusion_multimodal_3d_object_detection_amd import fusion, seg_head, synth

PEAK_HBM_GBS = 8000.0          # bench.py's


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


def kernels(rounds, dev):
    B, C, Hi, Wi, Ho, Wo = 8, 256, 128, 128, 200, 200
    gi = seg_head.range_grid([-51.2, -51.2, 51.2, 51.2], Hi, Wi)
    go = seg_head.range_grid([-50.0, -50.0, 50.0, 50.0], Ho, Wo)
    nin, nout = B * Hi * Wi * C, B * Ho * Wo * C
    x, y = synth.normal((nin,), 1).to(dev), torch.empty(nout, device=dev)
    dy, dx = synth.normal((nout,), 2).to(dev), torch.empty(nin, device=dev)

    def bilinear_bwd():
        dx.zero_()                                               # the atomic backward accumulates into zeros: part of its cost
        L.bilinear_bwd_nhwc(dy, dx, B, Hi, Wi, C, C, Ho, Wo, C)

    legs = [("bev_grid_resample_f32", lambda: L.bev_grid_resample(x, y, B, Hi, Wi, Ho, Wo, C, C, C, gi, go)),
            ("bilinear_nhwc_f32 (yardstick)", lambda: L.bilinear_nhwc(x, y, B, Hi, Wi, C, C, Ho, Wo, C)),
            ("bev_grid_resample_bwd_f32", lambda: L.bev_grid_resample_bwd(dy, dx, B, Hi, Wi, Ho, Wo, C, C, gi, go)),
            ("bilinear_bwd_nhwc_f32 + zero fill (yardstick, atomic)", bilinear_bwd)]
    print(json.dumps({"shape": f"B = {B}, C = {C}, {Hi} x {Wi} -> {Ho} x {Wo}, fp32", "peak_hbm_gbs": PEAK_HBM_GBS}), flush=True)
    nbytes = 4.0 * (nin + nout)                                  # algorithmic: one read of one map, one write of the other
    for (name, _), t in zip(legs, timed_ab([leg[1] for leg in legs], rounds)):
        gbs = nbytes / (t * 1e-6) / 1e9
        print(json.dumps({"kernel": name, "us": round(t, 1), "algorithmic_mb": round(nbytes / 1e6, 1), "gb_per_s": round(gbs, 1),
                          "hbm_fraction": round(gbs / PEAK_HBM_GBS, 3)}), flush=True)
    K = 6
    logits = (4 * synth.normal((B, K, Ho, Wo), 3)).to(dev).requires_grad_(True)
    masks = (synth.uniform((B, K, Ho, Wo), 4) < 0.3).to(torch.uint8).to(dev)
    loss = seg_head.SegFocalLoss()

    def focal():
        logits.grad = None
        loss(logits, masks)["loss"].backward()

    us = timed_ab([focal, lambda: seg_head.seg_iou_counts(logits.detach(), masks)], rounds)
    print(json.dumps({"op": f"SegFocalLoss forward + backward, B = {B}, K = {K}, {Ho} x {Wo} (layout copies included)", "us": round(us[0], 1)}),
          flush=True)
    print(json.dumps({"op": "seg_iou_counts, 7 thresholds, same shape", "us": round(us[1], 1)}), flush=True)


def detector(rounds, dev):
    B, bev = 8, 50
    imgs, pts, _ = synth.frame_inputs(B, 6, 448, 800, 35000, 4, seed=11)
    imgs, pts = imgs.to(dev), pts.to(dev)
    boxes = [torch.cat([synth.uniform((20, 2), 20 + b, -45.0, 45.0), torch.zeros(20, 1), synth.uniform((20, 3), 40 + b, 1.0, 5.0),
                        synth.uniform((20, 1), 60 + b, -3.0, 3.0)], 1) for b in range(B)]
    labels = [synth.randint((20,), 80 + b, 0, 10) for b in range(B)]
    tgt = ct.prepare_centernet_targets({"gt_boxes": boxes, "gt_labels": labels}, dev, bev_size=(bev, bev))
    masks = (synth.uniform((B, 6, 200, 200), 5) < 0.3).to(torch.uint8).to(dev)
    models = {}
    for name, seg in (("without seg head", None), ("with seg head", True)):
        m = fusion.create_detector("camera+lidar", "bev", "centernet", bev_h=bev, bev_w=bev, seg_head=seg)
        synth.fill_state_dict_(m, 1)
        models[name] = m.to(dev)
    focal, det = seg_head.SegFocalLoss(), ct.CenterNetLoss()

    def fwd(m):
        def run():
            with torch.no_grad():
                m(imgs, pts, None)
        return run

    def step(m):
        def run():
            m.zero_grad(set_to_none=True)
            out = m(imgs, pts, None)
            loss = det(out, tgt)["total_loss"]
            if "seg" in out:
                loss = loss + focal(out["seg"], masks)["loss"]
            loss.backward()
        return run

    for m in models.values():
        m.eval()
    us = timed_ab([fwd(m) for m in models.values()], rounds, inner=3, warm=2)
    for name, t in zip(models, us):
        print(json.dumps({"detector": f"config-4 shape, B = {B}, eval forward, {name}", "ms": round(t / 1e3, 2)}), flush=True)
    for m in models.values():
        m.train()
    us = timed_ab([step(m) for m in models.values()], rounds, inner=2, warm=2)
    for name, t in zip(models, us):
        print(json.dumps({"detector": f"config-4 shape, B = {B}, training step (forward, loss, backward), {name}", "ms": round(t / 1e3, 2)}),
              flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    if not torch.cuda.is_available():
        raise SystemExit("seg_head_time.py measures on the GPU: no 'cuda' device is visible")
    dev = torch.device("cuda")
    kernels(rounds, dev)
    if "--no-detector" not in sys.argv:
        detector(max(3, rounds // 2), dev)


if __name__ == "__main__":
    main()
