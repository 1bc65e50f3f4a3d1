"""Bit anchor of the Winograd convolution kernels (csrc/conv_wino.hip: wino_f32<RES, RELU, STATS, BNB, GEO, DIAG> and the filter
transform; csrc/conv_wino_wgrad.hip: wino_wgrad_table, wino_wgrad_f32, wino_wgrad_fold, wino_wgrad_final; their shared pieces in
csrc/wino_common.h and csrc/conv_common.h).

The parity tests compare these kernels with references inside a tolerance.  This module is the anchor outside that: every case builds
its inputs on the CPU with `synth.uniform` / `synth.normal` (the same bits on every host), makes ONE launch into buffers prefilled with
NaN, and compares the SHA-256 of every whole buffer the launch writes (y and the partial-sum rows; dw and the workspace of partial
blocks; the tile table) with tests/golden/wino_kernel_bits.json, which was recorded from a library built at the commit BEFORE the
kernels' shared stages were given one text each.  Neither kernel has atomics and the weight gradient is summed in a fixed order, so the
match is exact.  The fixture also holds a digest of each case's inputs: a changed generator shows up as such, not as a kernel
difference.

What the cases reach: Cin 32 / 64 / 96 (one patch chunk; first + last; a middle chunk), Cout 64 / 80 and W 32 / 21 / 13 (interior and
edge epilogues), N = 3 with H 17 / 34 (the stacked tilings cut across images with one / two dead rows), tile 1-4, RES x RELU, channel
slices on x / y / res, STATS with a pivot, BNB 1 / 2 x RES, the four DIAG instantiations (their y must equal the plain launch's); the
weight gradient with one split, two channel-block pairs, more splits than FOLD (the fold kernel), three output blocks, accumulate 0 / 1,
channel-strided x / dy, and the tile table itself.

Record (only when an intended change of the arithmetic replaces the anchor):
    python -m tests.test_gpu_wino_bits [path of the libbevf_hip.so to record from] [output json]
"""
import functools
import hashlib
import json
import os
import sys
from collections import namedtuple

import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wino_kernel_bits.json")
NAN = float("nan")
GAP_X, GAP_RES = 77.0, -33.0                                  # what the unused channels of a sliced input / residual hold
NSTAMPS = 6                                                   # kWinoStamps

# ---- wino_f32 ----------------------------------------------------------------------------------------------------------------------
Fwd = namedtuple("Fwd", "tag N H W cin cout x_gap y_gap res_gap", defaults=(0, 0, 0))
FWD = [Fwd("c32", 3, 17, 21, 32, 64),                         # one chunk; edge columns; one dead row between stacked images
       Fwd("c64", 3, 34, 32, 64, 80),                         # first + last chunk; interior columns; slab 0 interior, slab 1 edge; two dead rows
       Fwd("c96", 3, 17, 13, 96, 80),                         # a middle chunk
       Fwd("slices", 3, 34, 32, 64, 80, 32, 16, 8)]           # x_cs > Cin, y_cs > Cout, res_cs > Cout
BNB = Fwd("bnb", 1, 16, 16, 64, 64)


def sha(*named):
    """SHA-256 over (name, bytes) of each tensor."""
    h = hashlib.sha256()
    for name, t in named:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _sliced(v, gap, fill):
    """[M][C] -> flat [M][C + gap], the channels past C holding `fill`."""
    if gap:
        v = torch.cat([v, torch.full((v.shape[0], gap), fill)], dim=1)
    return v.reshape(-1).contiguous()


@functools.lru_cache(maxsize=None)
def fwd_inputs(s):
    """CPU inputs of a forward shape (flat NHWC x, OHWI filter, scale / shift / pivot, residual, the BNB operands) and their GPU copies;
    `u` = the filter through the library's own transform.  Built once per shape, never modified."""
    M, seed = s.N * s.H * s.W, synth.name_seed(f"wino_bits {s.tag}")
    ins = {"x": _sliced(synth.uniform((M, s.cin), seed, -1.0, 2.0).clamp_(min=0), s.x_gap, GAP_X),
           "w": synth.normal((s.cout * 9 * s.cin,), seed + 1, 0.0, (2.0 / (9 * s.cin)) ** 0.5),
           "scale": synth.uniform((s.cout,), seed + 2, 0.5, 1.5), "shift": synth.uniform((s.cout,), seed + 3, -0.3, 0.3),
           "res": _sliced(synth.uniform((M, s.cout), seed + 4, -2.0, 2.0), s.res_gap, GAP_RES),
           "pivot": synth.normal((s.cout,), seed + 5, 0.5, 1.0)}
    if s.tag == "bnb":
        ins.update(bnb_x=synth.normal((M * s.cout,), seed + 6), bnb_y=synth.normal((M * s.cout,), seed + 7),
                   mean=synth.normal((s.cout,), seed + 8, 0.0, 0.5), invstd=synth.uniform((s.cout,), seed + 9, 0.5, 2.0),
                   gamma=synth.normal((s.cout,), seed + 10, 1.0, 0.5), beta=synth.normal((s.cout,), seed + 11, 0.0, 0.5))
    dev = {k: v.cuda() for k, v in ins.items()}
    dev["u"] = L.wino_filter_transform(dev["w"], s.cout, s.cin)
    return ins, dev


def run_fwd(s, res=False, relu=False, tile=0, stats=False, bnb=0, diag=False):
    """One bevf_conv3x3_wino_f32 launch -> (CPU inputs, {buffer name: whole buffer})."""
    ins, dev = fwd_inputs(s)
    M, y_cs = s.N * s.H * s.W, s.cout + s.y_gap
    y = torch.full((M * y_cs,), NAN, device="cuda")
    out = {"y": y}
    kw = dict(N=s.N, H=s.H, W=s.W, Cin=s.cin, x_cs=s.cin + s.x_gap, Cout=s.cout, y_cs=y_cs, relu=relu, res=dev["res"] if res else None,
              res_cs=s.cout + s.res_gap if res else 0, tile=tile)
    if stats or bnb:
        out["part"] = kw["stats"] = torch.full((L.wino_stat_rows(s.N, s.H, s.W) * s.cout * 2,), NAN, device="cuda")
    if stats:
        kw["stats_pivot"] = dev["pivot"]
    if bnb:
        kw["bnb"] = dict(x=dev["bnb_x"], y=dev["bnb_y"] if bnb == 2 else None, mean=dev["mean"], invstd=dev["invstd"],
                         gamma=dev["gamma"], beta=dev["beta"])
    scale, shift = (None, None) if bnb else (dev["scale"], dev["shift"])
    stamps = None
    if diag:                                                     # an upper bound of the workgroups of every tiling; not hashed
        stamps = torch.zeros(s.N * (s.H // 16 + 2) * (s.W // 8 + 2) * ((s.cout + 63) // 64) * NSTAMPS, dtype=torch.int64, device="cuda")
        L.lib().bevf_debug_wino_stamps(stamps.data_ptr())
    try:
        L.conv3x3_wino(dev["x"], dev["u"], scale, shift, y, **kw)
        torch.cuda.synchronize()
    finally:
        if diag:
            L.lib().bevf_debug_wino_stamps(None)
    if diag:
        assert bool((stamps != 0).any()), "the diagnostic instantiation did not run"
    full = y.view(M, y_cs)
    assert not bool(full[:, :s.cout].isnan().any()), "left output elements unwritten"
    assert bool(full[:, s.cout:].isnan().all()), "wrote outside its channel slice"
    return ins, out


def run_filter(s):
    ins, dev = fwd_inputs(s)
    return {"w": ins["w"]}, {"u": dev["u"]}


# ---- wino_wgrad_f32 + reduction ----------------------------------------------------------------------------------------------------
Wg = namedtuple("Wg", "tag N H W cin cout x_gap dy_gap", defaults=(0, 0))
WGRAD = [Wg("1step", 1, 3, 3, 64, 64),                        # one step, one split
         Wg("pairs", 1, 8, 7, 128, 64),                       # two channel-block pairs, 2 splits
         Wg("fold", 2, 13, 21, 64, 64),                       # 39 steps -> 20 splits > FOLD: the fold kernel runs
         Wg("co192", 3, 8, 7, 64, 192)]
WGRAD_STRIDED = Wg("strided", 2, 13, 21, 64, 64, 32, 16)


@functools.lru_cache(maxsize=None)
def wgrad_inputs(s):
    M, seed = s.N * s.H * s.W, synth.name_seed(f"wino_bits wgrad {s.tag}")
    ins = {"x": _sliced(synth.normal((M, s.cin), seed), s.x_gap, GAP_X), "dy": _sliced(synth.normal((M, s.cout), seed + 1), s.dy_gap, GAP_RES),
           "dw0": synth.normal((s.cout * 9 * s.cin,), seed + 2)}
    return ins, {k: v.cuda() for k, v in ins.items()}


def _table(s):
    tab = torch.full((L.wino_wgrad_table_bytes(s.N, s.H, s.W) // 4,), -1, dtype=torch.int32, device="cuda")
    L.wino_wgrad_table(tab, s.N, s.H, s.W, s.cin + s.x_gap, s.cout + s.dy_gap)
    return tab


def run_wgrad(s, accumulate):
    """One bevf_conv3x3_wgrad_wino_f32 call (main kernel, fold where splits > FOLD, final) -> dw and the whole workspace."""
    ins, dev = wgrad_inputs(s)
    dw = dev["dw0"].clone() if accumulate else torch.full((s.cout * 9 * s.cin,), NAN, device="cuda")
    work = torch.full((L.wino_wgrad_workspace_floats(s.N, s.H, s.W, s.cin, s.cout),), NAN, device="cuda")
    L.conv3x3_wgrad_wino(dev["x"], dev["dy"], dw, _table(s), work, N=s.N, H=s.H, W=s.W, Cin=s.cin, x_cs=s.cin + s.x_gap, Cout=s.cout,
                         dy_cs=s.cout + s.dy_gap, accumulate=accumulate)
    torch.cuda.synchronize()
    assert not bool(dw.isnan().any()) and not bool(work.isnan().any()), "left elements unwritten"
    return ins, {"dw": dw, "work": work}


def run_table(s):
    geom = torch.tensor([s.N, s.H, s.W, s.cin + s.x_gap, s.cout + s.dy_gap], dtype=torch.int32)
    tab = _table(s)
    torch.cuda.synchronize()
    return {"geom": geom}, {"tab": tab}


CASES = {}
for _s in FWD:
    for _res in (0, 1):
        for _relu in (0, 1):
            for _t in (1, 2, 3, 4):
                if _s.tag != "slices" or (_res and _relu):
                    CASES[f"wino:{_s.tag}:res{_res}:relu{_relu}:tile{_t}"] = functools.partial(run_fwd, _s, bool(_res), bool(_relu), _t)
CASES["wino:c64:stats"] = functools.partial(run_fwd, FWD[1], stats=True)
CASES["wino:c96:stats"] = functools.partial(run_fwd, FWD[2], stats=True)
for _b in (1, 2):
    for _res in (0, 1):
        CASES[f"wino:bnb{_b}:res{_res}"] = functools.partial(run_fwd, BNB, bool(_res), bnb=_b)
DIAG = {f"wino:c32:res{_res}:relu1:tile{_t}:diag": f"wino:c32:res{_res}:relu1:tile{_t}" for _res in (0, 1) for _t in (1, 2)}
for _name in DIAG:
    CASES[_name] = functools.partial(run_fwd, FWD[0], "res1" in _name, True, int(_name[-6]), diag=True)
CASES["wino:filter:c96"] = functools.partial(run_filter, FWD[2])
for _s in WGRAD:
    for _acc in (0, 1):
        CASES[f"wgrad:{_s.tag}:acc{_acc}"] = functools.partial(run_wgrad, _s, bool(_acc))
CASES["wgrad:strided:acc0"] = functools.partial(run_wgrad, WGRAD_STRIDED, False)
CASES["wgrad:table:fold"] = functools.partial(run_table, WGRAD[2])
CASES["wgrad:table:strided"] = functools.partial(run_table, WGRAD_STRIDED)


def digests(case):
    ins, outs = case()
    return {"in": sha(*sorted(ins.items())), "out": {k: sha((k, v)) for k, v in sorted(outs.items())}}


@functools.lru_cache(maxsize=1)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_these_cases(gpu):
    assert sorted(fixture()) == sorted(CASES)


def test_diagnostic_launches_are_recorded_with_the_plain_launch_bits(gpu):
    """The time stamps change nothing a launch computes: the anchor of each DIAG case is the anchor of the same case without them."""
    for diag, plain in DIAG.items():
        assert fixture()[diag]["out"]["y"] == fixture()[plain]["out"]["y"], diag


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
