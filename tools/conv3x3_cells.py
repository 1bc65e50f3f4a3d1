#!/usr/bin/env python3
"""The layer1 row of conv3x3_bench.py with every cell's library chosen by hand: is a difference between two builds of libbevf_hip.so in
one cell the kernel's, or does the cell follow what ran before it?  Both libraries are loaded into one process; a round runs the cells in
the order given, timed as conv3x3_bench.py times them (5 launches between two events, median of the rounds).
usage: conv3x3_cells.py name=lib.so,name=lib.so name:tile,name:tile,.. [rounds]     tile = old | 0 .. 5 as in conv3x3_bench.py
e.g. the persistent kernel of build a among the other cells of build b:  a=A.so,b=B.so b:old,b:0,b:1,b:2,b:3,a:4,b:5"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L

libs = {}
for spec in sys.argv[1].split(","):
    name, path = spec.split("=")
    L._lib, L.LIB_PATH = None, os.path.abspath(path)
    libs[name] = L.lib()
cells = [tuple(c.split(":")) for c in sys.argv[2].split(",")]                 # (library, tile)
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev, BF = torch.device("cuda"), torch.bfloat16
N, H, W, Cin, Cout = 48, 225, 400, 64, 64                                     # layer1 of conv3x3_bench.py
x = torch.randn(N * H * W * Cin, device=dev).clamp_(min=0).to(BF)
w = (torch.randn(Cout * 9 * Cin, device=dev) * (1.0 / (9 * Cin)) ** 0.5).to(BF)
wp = L.conv3x3_pack_bf16(w, Cout, Cin)
sc, sh = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
res = torch.randn(N * H * W * Cout, device=dev).to(BF)
y0, y1 = torch.empty(N * H * W * Cout, device=dev, dtype=BF), torch.empty(N * H * W * Cout, device=dev, dtype=BF)
kw = dict(N=N, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=Cout, y_cs=Cout, relu=True, res=res, res_cs=Cout)


def run(name, tile):
    L._lib = libs[name]
    if tile == "old":
        L.conv2d_nhwc(x, w, sc, sh, y0, KH=3, KW=3, stride=1, pad=1, **kw)
    else:
        L.conv3x3_bf16(x, wp, sc, sh, y1, tile=int(tile), **kw)


t = [[] for _ in cells]
for _ in range(2):
    for c in cells:
        run(*c)
torch.cuda.synchronize()
for _ in range(rounds):
    for k, c in enumerate(cells):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            run(*c)
        e1.record(); torch.cuda.synchronize()
        t[k].append(e0.elapsed_time(e1) / 5 * 1e3)
for c, v in zip(cells, t):
    v = sorted(v)
    print(f"{c[0]:8s} tile {c[1]:3s}  median {v[len(v) // 2]:6.1f}us  min {v[0]:6.1f}  max {v[-1]:6.1f}", flush=True)
