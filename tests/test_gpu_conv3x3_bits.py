"""Bit anchor of the bf16 3x3 kernels (csrc/conv3x3_bf16.hip: conv3x3_bf16<CT, PB, BH>, conv3x3_bf16_wide64, conv3x3_bf16_persist).

The "variants agree bit for bit" assertions of test_gpu_conv3x3_bf16.py compare kernels that are built from the same helpers of
conv3x3_bf16.hip with each other.  This module is the anchor outside that code: every case builds its inputs on the CPU with
`synth.uniform` (pure arithmetic, the same bits on every host), runs L.conv3x3_bf16 ONCE with an explicit `tile` into an output
prefilled with NaN, and compares the SHA-256 of the output with tests/golden/conv3x3_kernel_bits.json, which was recorded from a
library built at the commit BEFORE the three kernels were moved onto the shared helpers.  The kernels use no atomics, so the match is
exact.  The fixture also holds a digest of each case's inputs: a changed generator shows up as such, not as a kernel difference.

Record (only when an intended change of the arithmetic replaces the anchor):
    python -m tests.test_gpu_conv3x3_bits [path of the libbevf_hip.so to record from] [output json]
"""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv3x3_kernel_bits.json")
BF = torch.bfloat16

# (N, H, W, Cin, Cout, affine, residual, relu, x_cs, y_cs, res_cs)
SHAPES = [
    (1, 1, 1, 64, 64, False, False, False, 64, 64, 0),        # all padding; null scale and shift pointers
    (1, 17, 23, 64, 64, True, True, True, 64, 64, 64),        # the second block row has 1, 2, 3 live rows: every branch of the
    (1, 18, 23, 64, 64, True, True, True, 64, 64, 64),        # dead-row switch at MT = 4 (1, 2, 3 here; 0 and 4 in the first block row
    (1, 19, 23, 64, 64, True, True, True, 64, 64, 64),        # and the 57-row maps); ragged right edge
    (2, 57, 100, 64, 64, True, True, True, 64, 64, 64),       # edge blocks both ways; tile 3: 32-row blocks, partly dead last wave
    (1, 33, 18, 32, 64, True, False, True, 32, 64, 0),        # NCH = 1: prologue, first and last chunk coincide; 3 block rows of 16, 2 of 32
    (3, 5, 40, 96, 192, True, True, False, 128, 256, 256),    # odd chunk count (patch buffer parity); channel slices; three tiles of 64
    (1, 17, 33, 64, 128, True, True, True, 64, 128, 128),     # CT = 128 (waves 2 x 2, MT = 8), Cin = 64 off wide64; 1 live row at the bottom
    (1, 22, 20, 128, 128, True, True, True, 128, 128, 128),   # CT = 128, 6 live rows in the last block
    (1, 40, 40, 256, 256, True, True, True, 256, 512, 256),   # CT = 128, 72 steps: the four-slot ring wraps many times
    (7, 57, 100, 64, 192, True, True, True, 64, 192, 192),    # 588 tiles of 64 channels > 512 persistent workgroups: one or two tiles per
]                                                             # workgroup, the channel tile changing between a workgroup's two tiles
TILES = (1, 2, 3, 4, 5)
GAP_X, GAP_RES = 77.0, -33.0                                  # what the unused channels of a sliced input / residual hold


def sha(*named):
    """SHA-256 over (name, bytes) of each tensor."""
    h = hashlib.sha256()
    for name, t in named:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _sliced(v, cs, gap):
    """[M][C] float -> flat bf16 [M][cs], the channels past C holding `gap`."""
    m, c = v.shape
    if cs > c:
        v = torch.cat([v, torch.full((m, cs - c), gap)], dim=1)
    return v.reshape(-1).to(BF)


@functools.lru_cache(maxsize=1)
def inputs(shape):
    """The CPU inputs of a shape (bf16 NHWC activations, bf16 OHWI filter, fp32 scale / shift) and their copies on the GPU with the
    filter packed.  Built once per shape, shared by its five tiles, never modified."""
    N, H, W, cin, cout, affine, res, relu, x_cs, y_cs, res_cs = shape
    M, seed = N * H * W, synth.name_seed(f"conv3x3_bits {N}x{H}x{W} {cin}->{cout}")    # a stream of its own per shape
    ins = {"x": _sliced(synth.uniform((M, cin), seed, -1.0, 2.0).clamp_(min=0), x_cs, GAP_X),
           "w": synth.uniform((cout * 9 * cin,), seed + 1, -1.0, 1.0).mul_((3.0 / (9 * cin)) ** 0.5).to(BF)}
    if affine:
        ins["scale"], ins["shift"] = synth.uniform((cout,), seed + 2, 0.5, 1.5), synth.uniform((cout,), seed + 3, -0.3, 0.3)
    if res:
        ins["res"] = _sliced(synth.uniform((M, cout), seed + 4, -2.0, 2.0), res_cs, GAP_RES)
    dev = {k: v.cuda() for k, v in ins.items()}
    dev["wp"] = L.conv3x3_pack_bf16(dev["w"], cout, cin)
    return ins, dev


def run(shape, tile):
    """One launch -> (CPU inputs, the whole output buffer)."""
    N, H, W, cin, cout, affine, res, relu, x_cs, y_cs, res_cs = shape
    ins, dev = inputs(shape)
    y = torch.full((N * H * W * y_cs,), float("nan"), dtype=BF, device="cuda")
    L.conv3x3_bf16(dev["x"], dev["wp"], dev.get("scale"), dev.get("shift"), y, N=N, H=H, W=W, Cin=cin, x_cs=x_cs, Cout=cout, y_cs=y_cs,
                   relu=relu, res=dev.get("res"), res_cs=res_cs, tile=tile)
    torch.cuda.synchronize()
    full = y.view(N * H * W, y_cs)
    assert not bool(full[:, :cout].isnan().any()), "left output elements unwritten"
    assert bool(full[:, cout:].isnan().all()), "wrote outside its channel slice"
    return ins, y


def _name(shape, tile):
    N, H, W, cin, cout = shape[:5]
    return f"tile{tile}:{N}x{H}x{W}:{cin}->{cout}"


CASES = {_name(s, t): functools.partial(run, s, t) for s in SHAPES for t in TILES}       # shape-major: inputs() is reused


def digests(case):
    ins, y = case()
    return {"in": sha(*sorted(ins.items())), "out": sha(("y", y))}


@functools.lru_cache(maxsize=1)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_these_cases(gpu):
    assert sorted(fixture()) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_recorded_kernels(gpu, name):
    want, got = fixture()[name], digests(CASES[name])
    assert got["in"] == want["in"], "the input generator changed (not a kernel difference): record again from the anchor commit"
    assert got["out"] == want["out"]


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1]:
        L.LIB_PATH = os.path.abspath(sys.argv[1])                # before the first lib() call
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    rec = {name: digests(case) for name, case in CASES.items()}
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases from {L.LIB_PATH} -> {out}")
