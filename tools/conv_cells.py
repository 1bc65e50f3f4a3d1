#!/usr/bin/env python3
"""Cells of conv_bench.py / wino_bench.py / wgrad_bench.py with every cell's library chosen by hand: is a difference between two builds of
libbevf_hip.so in one cell the kernel's, or the process's (where its buffers landed, what ran before)?  Both libraries are loaded into one
process and launch on the SAME buffers; a round runs the cells in the order given (odd rounds backwards), timed as the bench tools time
them (10 launches between two events).  The same build under two names (two copies of the file) gives the noise floor of a cell.
usage: conv_cells.py name=lib.so,name=lib.so default|split|bf16|wino|wino_wgrad layer,layer,.. name:tile,name:tile,.. [rounds]
  default / split / bf16: the layers of conv_bench.py through bevf_conv2d_nhwc_*;  wino: the layers of wino_bench.py through
  bevf_conv3x3_wino_f32 (tile = its tiling);  wino_wgrad: the layers of wgrad_bench.py through bevf_conv3x3_wgrad_wino_f32 (tile unused)
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


def layer_table(tool, pattern):
    """The SHAPES literal of a neighbouring bench tool."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), tool)) as f:
        return eval(re.search(pattern, f.read(), re.S | re.M).group(1))


if mode == "wino":
    SHAPES = layer_table("wino_bench.py", r"^SHAPES = (\{.*?^\})")                      # name: (N, H, W, Cin, Cout, residual)
elif mode == "wino_wgrad":
    SHAPES = {s[0]: s[1:] for s in layer_table("wgrad_bench.py", r"^SHAPES = (\[.*?\])$")}   # name: (N, H, W, Cin, Cout)
else:
    SHAPES = layer_table("conv_bench.py", r"^SHAPES = (\{.*?^\})")                      # name: (N, H, W, Cin, Cout, k, stride, pad)
dev = torch.device("cuda")


def launcher(layer):
    """The layer's buffers (made once, shared by every cell) -> launch(tile) through whichever library L._lib is."""
    if mode == "wino":
        N, H, W, Cin, Cout, res = SHAPES[layer]
        x = torch.randn(N * H * W * Cin, device=dev)
        u = L.wino_filter_transform(torch.randn(Cout * 9 * Cin, device=dev) * 0.05, Cout, Cin)
        sc, sh = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
        r = torch.randn(N * H * W * Cout, device=dev) if res else None
        y = torch.empty(N * H * W * Cout, device=dev)
        return lambda tile: L.conv3x3_wino(x, u, sc, sh, y, N=N, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=Cout, y_cs=Cout, relu=True, res=r,
                                           res_cs=Cout if res else 0, tile=tile)
    if mode == "wino_wgrad":
        N, H, W, Cin, Cout = SHAPES[layer]
        x, dy = torch.randn(N * H * W * Cin, device=dev), torch.randn(N * H * W * Cout, device=dev)
        dw = torch.empty(Cout * 9 * Cin, device=dev)
        tab = torch.empty(L.wino_wgrad_table_bytes(N, H, W) // 4, dtype=torch.int32, device=dev)
        L.wino_wgrad_table(tab, N, H, W, Cin, Cout)
        work = torch.empty(L.wino_wgrad_workspace_floats(N, H, W, Cin, Cout), device=dev)
        return lambda tile: L.conv3x3_wgrad_wino(x, dy, dw, tab, work, N=N, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=Cout, dy_cs=Cout,
                                                 accumulate=False)
    N, H, W, Cin, Cout, k, s, p = SHAPES[layer]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(N * H * W * Cin, device=dev)
    w = torch.randn(Cout * k * k * Cin, device=dev) * 0.05
    sc, sh = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
    if mode == "split": w = L.split_weights_f32x3(w)
    y = torch.empty(N * Ho * Wo * Cout, device=dev)
    if mode == "bf16": x, w, y = x.bfloat16(), w.bfloat16(), y.bfloat16()
    return lambda tile: L.conv2d_nhwc(x, w, sc, sh, y, N=N, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=Cout, y_cs=Cout, KH=k, KW=k, stride=s, pad=p,
                                      relu=True, tile=tile)


for layer in layers:
    L._lib = libs[cells[0][0]]
    launch = launcher(layer)

    def run(name, tile):
        L._lib = libs[name]
        launch(tile)

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
    del launch
