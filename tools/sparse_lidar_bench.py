#!/usr/bin/env python3
"""The opt-in sparse-voxel LiDAR encoder, timed at B = 8 x 35 k points, BEV 128^2 (level 0: 512 x 512 x 8,
8 points per voxel, 40000 voxels per frame), next to the PointPillars front end on the same sweeps:
  (a) four legs interleaved in one process, device events, median over the rounds: SparseLiDAREncoder.forward_nhwc (eval), its
      training forward + backward (stand-alone encoder, canvas gradient given), and the same two for PillarLiDAREncoder;
  (b) per-kernel times of one eval forward and one training forward + backward (engine.KernelTimer brackets, a pass of its own);
  (c) the gather-GEMM's FLOP rates per layer: `useful` = 2 Cin Cout per present (row, tap) pair, `executed` = what the MFMAs
      issued, 2 * (rows per tile) * Cin * Cout per (tile, tap some row of the tile uses), both over the layer's kernel time.
Sweeps: `uniform` (synth.frame_inputs, as tools/pillar_bench.py: nearly every point its own voxel) and `clustered` (half the
points in 64 clusters of sigma 2 m per frame: voxels with neighbours).
usage: sparse_lidar_bench.py [rounds]   (prints one JSON object per measurement)"""
import copy
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import encoders, engine, synth

B, N, S = 8, 35000, 128


def sweeps(dev):
    _, uni, _ = synth.frame_inputs(B, 0, 0, 0, N, 4, seed=77)
    g = torch.Generator().manual_seed(78)
    ctr = torch.rand(B, 64, 2, generator=g) * 90.0 - 45.0
    pick = torch.randint(0, 64, (B, N // 2), generator=g)
    clu = uni.clone()
    clu[:, : N // 2, :2] = torch.gather(ctr, 1, pick[..., None].expand(B, N // 2, 2)) + torch.randn(B, N // 2, 2, generator=g) * 2.0
    clu[:, : N // 2, 2] = -3.0 + torch.rand(B, N // 2, generator=g) * 3.0
    return {"uniform": uni.to(dev), "clustered": clu.to(dev)}


def interleaved(legs, rounds, inner=3):
    """legs: name -> fn.  Every round times each leg once (inner calls between two events): the legs share the machine's state."""
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) / inner * 1e3)
    return {k: dict(us_median=round(sorted(v)[len(v) // 2], 1), us_min=round(min(v), 1), us_max=round(max(v), 1)) for k, v in t.items()}


def train_leg(enc, pts, G):
    def step():
        for p in enc.parameters():
            p.grad = None
        (enc(pts) * G).sum().backward()
    return step


def kernel_times(fn):
    t = engine.KernelTimer()
    engine.set_timer(t)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        engine.set_timer(None)
    return {k: round(v["ms"] * 1e3, 1) for k, v in t.totals().items()}


def gemm_rates(enc, times):
    """Per layer, from the last eval batch's tables: present (row, tap) pairs, (tile, tap) pairs the kernel ran, FLOP rates."""
    s = enc._eng().last
    tile = L.sparse_conv_row_tile()
    out = {}
    cin = engine.SPARSE_KPAD
    for name, blk in zip(engine.SPARSE_SPEC, enc.layers()):
        lr = engine.SPARSE_SPEC[name][0]
        cap, cout = s.caps[lr], blk.conv.weight.shape[0]
        tab = s.table[name][: s.B * cap * 27].view(s.B, cap, 27)
        act = torch.arange(cap, device=tab.device)[None, :] < s.count[lr][: s.B, None].long()
        present = (tab >= 0) & act[..., None]                              # (inactive slots hold stale entries: masked)
        pairs = int(present.sum())
        tiles = int(present.view(s.B * cap // tile, tile, 27).any(1).sum()) if (s.B * cap) % tile == 0 else None
        us = times.get(f"sparse_conv_f32:{name}")
        r = dict(rows=int(act.sum()), cin=cin, cout=cout, row_tap_pairs=pairs, taps_per_row=round(pairs / max(int(act.sum()), 1), 2), us=us)
        if us:
            r["useful_tflops"] = round(2.0 * pairs * cin * cout / us / 1e6, 2)
            if tiles is not None:
                r["tile_tap_pairs"] = tiles
                r["executed_tflops"] = round(2.0 * tiles * tile * cin * cout / us / 1e6, 2)
        out[name] = r
        cin = cout
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 7
    dev = torch.device("cuda")
    sp = encoders.SparseLiDAREncoder(input_channels=4, bev_h=S, bev_w=S)
    pl = encoders.PillarLiDAREncoder(input_channels=4, bev_h=S, bev_w=S)
    synth.fill_state_dict_(sp, 3)
    synth.fill_state_dict_(pl, 3)
    sp, pl = sp.to(dev).eval(), pl.to(dev).eval()
    sp_t, pl_t = copy.deepcopy(sp).train(), copy.deepcopy(pl).train()        # own instances: a training step moves the running buffers,
                                                                             # and the eval engines would repack after every one
    gs = torch.randn(B, sp.out_channels, S, S, device=dev)
    gp = torch.randn(B, pl.pfn_channels, S, S, device=dev)
    for sweep, pts in sweeps(dev).items():
        def ev(enc):
            def run():
                with torch.no_grad():
                    enc.forward_nhwc(pts)
            return run

        legs = {"sparse eval forward": ev(sp), "sparse train forward+backward": train_leg(sp_t, pts, gs),
                "pillars eval forward": ev(pl), "pillars train forward+backward": train_leg(pl_t, pts, gp)}
        res = interleaved(legs, rounds)
        print(json.dumps(dict(sweep=sweep, batch=B, points=N, bev=S, rounds=rounds, legs=res)), flush=True)
        k_eval = kernel_times(legs["sparse eval forward"])
        print(json.dumps(dict(sweep=sweep, kernels_us="sparse eval forward", **k_eval)), flush=True)
        print(json.dumps(dict(sweep=sweep, gather_gemm=gemm_rates(sp, k_eval))), flush=True)
        print(json.dumps(dict(sweep=sweep, kernels_us="sparse train forward+backward", **kernel_times(legs["sparse train forward+backward"]))),
              flush=True)
        s = sp._eng().last
        print(json.dumps(dict(sweep=sweep, active_rows=[int(c[:B].sum()) for c in s.count], capacity_rows=[B * c for c in s.caps])), flush=True)


if __name__ == "__main__":
    main()
