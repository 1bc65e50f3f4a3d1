#!/usr/bin/env python3
"""The opt-in PointPillars LiDAR branch, timed:
  (a) the pillar front end at B = 8 x 35 k points, BEV 128^2 (P = 32, 12000 pillars): voxelize, the fused PFN kernel
      (bevf_pillar_pfn_f32: decoration + Linear + BN + ReLU + max + canvas), and the whole encoder; the PFN kernel's
      algorithmic bytes (occupied rows + their coords / counts read once, the canvas written once) against the 6.29 TB/s
      measured copy rate;
  (b) the inference detector forward at config-2 shapes (camera+LiDAR, 6 x 900x1600, 35 k points, BEV 128^2, B = 8, fp32, default
      conv mode): PointNet against PointPillars;
  (c) the config-4 training step (6 x 448x800, 35 k points, BEV 50^2, B = 8, 20 GT boxes, loss + backward + AdamW + clip) with the
      same two LiDAR branches.
usage: pillar_bench.py [rounds] [--skip-train]   (prints one JSON object per measurement)"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import encoders, engine, fusion, synth

COPY_GBS = 6290.0          # measured device-to-device copy rate


def timed(fn, rounds=5, inner=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / inner)
    return sorted(t)[len(t) // 2] * 1e3          # us, median


def front_end(rounds, dev):
    out = []
    B, N, S = 8, 35000, 128
    _, pts, _ = synth.frame_inputs(B, 0, 0, 0, N, 4, seed=77)
    pts = pts.to(dev)
    enc = encoders.PillarLiDAREncoder(input_channels=4, bev_h=S, bev_w=S)
    synth.fill_state_dict_(enc, 3)
    enc = enc.to(dev).eval()
    eng = enc._eng()
    enc.forward_nhwc(pts)                                         # packs, sizes the workspaces
    alloc = lambda name, n, dt: eng.buf(name, n, dt)            # noqa: E731
    us_vox = timed(lambda: engine.pillar_voxelize(enc, pts, alloc), rounds)
    g, _, _ = engine.pillar_voxelize(enc, pts, alloc)
    canvas = eng.buf("canvas", B * S * S * eng.cout)
    us_pfn = timed(lambda: L.pillar_pfn(g, eng.w, eng.scale, eng.shift, eng.cout, canvas), rounds)
    us_all = timed(lambda: enc.forward_nhwc(pts), rounds)
    nvox = eng._bufs["vox_nvox"][:B].cpu()
    npts = eng._bufs["vox_npts"][:B * enc.max_pillars].view(B, -1).cpu()
    occ = int(nvox.sum())
    rows = int(sum(int(npts[b, :int(nvox[b])].sum()) for b in range(B)))
    nbytes = rows * 4 * 4 + occ * (24 + 4) + B * S * S * eng.cout * 4
    gbs = nbytes / us_pfn / 1e3
    base = dict(batch=B, points=N, bev=S, occupied_pillars=occ, kept_points=rows)
    out.append(dict(base, stage="voxelize (one pillar per BEV cell, P=32, 12000 pillars)", us=round(us_vox, 1)))
    out.append(dict(base, stage="pillar_pfn (memset + fused PFN kernel)", us=round(us_pfn, 1),
                    algorithmic_mb=round(nbytes / 1e6, 2), gb_per_s=round(gbs, 1), frac_of_copy_rate=round(gbs / COPY_GBS, 4)))
    out.append(dict(base, stage="PillarLiDAREncoder.forward_nhwc (voxelize + PFN)", us=round(us_all, 1)))
    return out


def detector(kind, cfg, dev, rounds, train):
    B = 8
    model = fusion.create_detector("camera+lidar", "bev", "centernet", bev_h=cfg["bev"], bev_w=cfg["bev"], lidar_encoder_type=kind)
    synth.fill_state_dict_(model, 0)
    model = model.to(dev)
    imgs, pts, _ = synth.frame_inputs(B, 6, cfg["h"], cfg["w"], 35000, 4, 0, seed=0x5EED)
    imgs, pts = imgs.to(dev), pts.to(dev)
    if not train:
        model.eval()
        ms = timed(lambda: model(imgs, pts, None), rounds, 3) / 1e3
    else:
        from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct
        from bevfusion_multimodal_3d_object_detection_amd import training
        model.train()
        boxes, labels = synth.gt_boxes(B, 20, seed=5)
        gt = {"gt_boxes": boxes.to(dev), "gt_labels": labels.to(dev)}
        crit = ct.CenterNetLoss()
        opt = training.FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=10.0)

        def step():
            losses = crit(model(imgs, pts, None), ct.prepare_centernet_targets(gt, dev))
            opt.zero_grad()
            losses["total_loss"].backward()
            opt.step()
        ms = timed(step, rounds, 2) / 1e3
    del model, imgs, pts
    torch.cuda.empty_cache()
    return ms


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 5
    dev = torch.device("cuda")
    for r in front_end(rounds, dev):
        print(json.dumps(r), flush=True)
    legs = [("(b) inference, config-2 shapes", dict(h=900, w=1600, bev=128), False)]
    if "--skip-train" not in sys.argv:
        legs.append(("(c) training step, config-4 shapes", dict(h=448, w=800, bev=50), True))
    for name, cfg, train in legs:
        res = {kind: round(detector(kind, cfg, dev, rounds, train), 3) for kind in ("PointNet", "PointPillars")}
        print(json.dumps({"leg": name, "batch": 8, "conv_mode": engine.conv_mode(), "ms_per_step": res,
                          "pillars_minus_pointnet_ms": round(res["PointPillars"] - res["PointNet"], 3)}), flush=True)


if __name__ == "__main__":
    main()
