"""Pruned PointNet max on the GPU, launch by launch, on the benchmark's LiDAR frames (config 2 weights and sweeps): HIP-event time
of the seed and main bound launches, the compaction, the exact launch on the candidate slots, the guarded full launch that is
skipped, and today's full launch; the flagged rows per frame and the overflow word, read back after the timing; and a bit
comparison of the pruned result with the full launch's.

usage: pointnet_prune_stats.py [--batch 8] [--points 35000] [--strides 2,4,8] [--reps 10]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from bevfusion_multimodal_3d_object_detection_amd import _lib as L  # noqa: E402
from bevfusion_multimodal_3d_object_detection_amd import engine as E  # noqa: E402
from bevfusion_multimodal_3d_object_detection_amd import replicas, synth  # noqa: E402


def timed(fn, reps):
    """min / median ms of fn() over reps launches, each between its own pair of events."""
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return ms[0], ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=35000)
    ap.add_argument("--strides", default="2,4,8")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    B, N = args.batch, args.points
    model = bench.build_model(bench.CONFIGS[2]).cuda()
    _, pts, _ = synth.frame_inputs(B, 0, 0, 0, N, 4, 0, 125, 7, seed=replicas.frame_seed(0x5EED, 2, 0))
    pts = pts.cuda()
    enc = model.lidar_encoder
    seen = {}
    run = E.PrunedColMax.run

    def spy(self, x, gmax, B_, N_, **kw):
        seen["x"] = x
        return run(self, x, gmax, B_, N_, **kw)
    E.PrunedColMax.run = spy
    E.PRUNE_POINTNET_MAX = True
    with torch.no_grad():
        on = enc(pts).clone()
    E.PrunedColMax.run = run
    E.PRUNE_POINTNET_MAX = False
    with torch.no_grad():
        off = enc(pts).clone()
    print(f"B = {B}, N = {N}: pruned result bit-equal to the full launch: {torch.equal(on.view(torch.int32), off.view(torch.int32))}")
    pm, x = enc._eng().prune, seen["x"]
    pc, M, cap = pm.pc, B * N, E.prune_cap(N)
    nthr, nb = B * pc.cout, -(-B // 4) * 4
    work = pm._bufs["work"][:4 + nb + nthr + M]
    ovf, rows, thr, flag = work[:1], work[4:4 + B], work[4 + nb:4 + nb + nthr], work[4 + nb + nthr:]
    rp, cand = pm._bufs["rp"], pm._bufs["cand"]
    geo = dict(M=M, Cin=pc.cin, Cout=pc.cout, rows_per_group=N)
    gmax = torch.zeros(B, pc.cout, dtype=torch.int32, device=x.device)
    full = timed(lambda: E._conv_call(pc, x, None, M, 1, 1, colmax=gmax, rows_per_group=N), args.reps)
    print(f"full launch ({M} rows): min {full[0]:.3f} ms, median {full[1]:.3f} ms;  cap = {cap} slots per frame ({100.0 * cap / N:.1f} %)")
    for k in (int(s) for s in args.strides.split(",")):
        work.zero_()
        seed = timed(lambda: L.conv2d_bound(x, pm.planes, pc.scale, pc.shift, pm.g, thr, None, seed_stride=k, **geo), args.reps)
        work.zero_()
        L.conv2d_bound(x, pm.planes, pc.scale, pc.shift, pm.g, thr, None, seed_stride=k, **geo)
        thr_seed = thr.clone()

        def main_launch():                                    # every repetition starts from the seed launch's thresholds
            thr.copy_(thr_seed)
            L.conv2d_bound(x, pm.planes, pc.scale, pc.shift, pm.g, thr, flag, **geo)
        copy = timed(lambda: thr.copy_(thr_seed), args.reps)
        mainl = timed(main_launch, args.reps)
        compact = timed(lambda: L.prune_compact(x, flag, rp, cand, rows, ovf, B, N, pc.cin, cap), args.reps)
        exact = timed(lambda: E._conv_call(pc, cand, None, B * cap, 1, 1, colmax=gmax, rows_per_group=cap, group_rows=rows), args.reps)
        zero = timed(lambda: work.zero_(), args.reps)
        ovf.zero_()
        skipped = timed(lambda: E._conv_call(pc, x, None, M, 1, 1, colmax=gmax, rows_per_group=N, run_if=ovf), args.reps)
        work.zero_()
        L.conv2d_bound(x, pm.planes, pc.scale, pc.shift, pm.g, thr, None, seed_stride=k, **geo)
        L.conv2d_bound(x, pm.planes, pc.scale, pc.shift, pm.g, thr, flag, **geo)
        L.prune_compact(x, flag, rp, cand, rows, ovf, B, N, pc.cin, cap)
        torch.cuda.synchronize()
        per_frame = flag.view(B, N).sum(1).tolist()
        total = seed[0] + (mainl[0] - copy[0]) + compact[0] + exact[0] + zero[0] + skipped[0]
        print(f"k = {k}: zero {zero[0]:.3f}  seed {seed[0]:.3f}  main {mainl[0] - copy[0]:.3f}  compact {compact[0]:.3f}  exact {exact[0]:.3f}  "
              f"skipped full {skipped[0]:.3f}  sum {total:.3f} ms (min of {args.reps}; full launch {full[0]:.3f})")
        print(f"        flagged rows per frame {per_frame} = {100.0 * max(per_frame) / N:.1f} % at most, overflow word {int(ovf.item())}")


if __name__ == "__main__":
    main()
