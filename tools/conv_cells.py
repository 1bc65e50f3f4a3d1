#!/usr/bin/env python3
"""Cells of conv_bench.py with every cell's library chosen by hand: is a difference between two builds of libbevf_hip.so in one cell the
kernel's, or the process's (where its buffers landed, what ran before)?  Both libraries are loaded into one process and launch on the SAME
buffers; a round runs the cells in the order given (odd rounds backwards), timed as conv_bench.py times them (10 launches between two events).
usage: conv_cells.py name=lib.so,name=lib.so default|split|bf16 layer,layer,.. name:tile,name:tile,.. [rounds]
e.g. tiles 1 and 2 of two builds side by side:  a=A.so,b=B.so bf16 pn_fwd,sq1k a:1,b:1,a:2,b:2"""
import os
import re
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bevfusion_multimodal_3d_object_detection_amd import _lib as L

libs = {}
for spec in sys.argv[1].split(","):
    name, path = spec.split("=")
    L._lib, L.LIB_PATH = None, os.path.abspath(path)
    libs[name] = L.lib()
mode, layers = sys.argv[2], sys.argv[3].split(",")
cells = [(c.split(":")[0], int(c.split(":")[1])) for c in sys.argv[4].split(",")]        # (library, tile)
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 7
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_bench.py")) as f:        # the layer table of conv_bench.py
    SHAPES = eval("{" + re.search(r"^SHAPES = \{(.*?)^\}", f.read(), re.S | re.M).group(1) + "}")
dev = torch.device("cuda")
for layer in layers:
    N, H, W, Cin, Cout, k, s, p = SHAPES[layer]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(N * H * W * Cin, device=dev)
    w = torch.randn(Cout * k * k * Cin, device=dev) * 0.05
    sc, sh = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
    if mode == "split": w = L.split_weights_f32x3(w)
    y = torch.empty(N * Ho * Wo * Cout, device=dev)
    if mode == "bf16": x, w, y = x.bfloat16(), w.bfloat16(), y.bfloat16()

    def run(name, tile):
        L._lib = libs[name]
        L.conv2d_nhwc(x, w, sc, sh, y, N=N, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=Cout, y_cs=Cout, KH=k, KW=k, stride=s, pad=p, relu=True, tile=tile)

    t = {c: [] for c in cells}
    for c in cells * 2:
        run(*c)
    torch.cuda.synchronize()
    for r in range(rounds):
        for c in (cells if r % 2 == 0 else cells[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                run(*c)
            e1.record(); torch.cuda.synchronize()
            t[c].append(e0.elapsed_time(e1) / 10 * 1e3)
    for c in cells:
        v = sorted(t[c])
        print(f"{mode:7s} {layer:10s} {c[0]:8s} tile{c[1]}  median {v[len(v) // 2]:7.1f}us  min {v[0]:7.1f}  max {v[-1]:7.1f}", flush=True)
    del x, w, y
