"""Bit anchor of the stem's forward kernels (csrc/stem.hip: stem_conv7x7, stem_pool7x7, stem_conv7x7_bf16mma, stem_pool7x7_bf16mma,
stem_pool7x7_bf16v2).

The "fused equals unfused" tests of test_gpu_stem_pool.py compare kernels that call the same helpers of stem.hip with each other.
This module is the anchor outside that code: every case runs ONE raw entry point on inputs made on the CPU with `synth.uniform`
(pure arithmetic, the same bits on every host), into an output prefilled with NaN, and compares the SHA-256 of the output with
tests/golden/stem_kernel_bits.json, which was recorded from a library built at the commit BEFORE the kernels were moved onto the
shared helpers.  The kernels use no atomics, so the match is exact (stem_wgrad does, was not edited, and is not anchored here).  The
fixture also holds a digest of each case's inputs: a changed generator shows up as such, not as a kernel difference.

bevf_stem_pool_bf16mma chooses its kernel once per process (BEVF_STEM_BF16_EXPAND): the kernel behind the switch runs in one fresh
child process that prints the digests of all shapes; the fixture holds them under "expand".

Record (only when an intended change of the arithmetic replaces the anchor):
    python -m tests.test_gpu_stem_bits [path of the libbevf_hip.so to record from] [output json]
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "stem_kernel_bits.json")
SWITCH = "BEVF_STEM_BF16_EXPAND"

# (N, H, W, float offset of the image in its buffer)
SHAPES = [(2, 1, 1, 0), (1, 7, 9, 0),       # a map smaller than one window: no interior anywhere
          (1, 37, 50, 0), (3, 33, 46, 0),   # W % 4 != 0: scalar staging, several images
          (2, 64, 96, 0),                   # vector staging, one tile
          (1, 255, 482, 0),                 # Wo = 241: two 128-pixel tiles (the second ragged), three 120-column strips (both halves
                                            # live, the last strip partly outside); Ho = 128 in several row segments, some ending mid-chunk
          (1, 129, 1027, 0),                # odd height and width, many strips
          (1, 64, 96, 1)]                   # W % 4 == 0 but the image starts 4 bytes into its buffer: the other way into the scalar path
ENTRIES = ["conv7x7_f32:relu0", "conv7x7_f32:relu1", "conv7x7_bf16out", "pool_f32", "conv7x7_bf16mma", "pool_bf16mma"]


def sha(*named):
    """SHA-256 over (name, bytes) of each tensor."""
    h = hashlib.sha256()
    for name, t in named:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=1)
def filters():
    """The fp32 bank [148][64] (k = c*49 + kh*7 + kw, row 147 zero) and the bf16 bank [64][176] (k = (c*7 + kh)*8 + kw, the rest zero)
    of one OIHW filter, scale and shift."""
    w = synth.uniform((64, 3, 7, 7), 2, -0.1, 0.1)
    w32 = torch.zeros(148, 64)
    w32[:147] = w.reshape(64, 147).t()
    w16 = torch.zeros(64, 22, 8)
    w16[:, :21, :7] = w.reshape(64, 21, 7)
    return dict(w32=w32.contiguous().view(-1), w16=w16.to(torch.bfloat16).contiguous().view(-1),
                scale=synth.uniform((64,), 3, 0.5, 1.5), shift=synth.uniform((64,), 4, -0.3, 0.3))


@functools.lru_cache(maxsize=2)
def image(N, H, W):
    return synth.uniform((N * 3 * H * W,), 1000 + 7 * H + W, -2.0, 2.0)


def run(entry, N, H, W, off):
    """One raw entry point -> (CPU inputs, output tensor)."""
    f = filters()
    bf16_bank = entry in ("conv7x7_bf16mma", "pool_bf16mma")
    ins = {"x": image(N, H, W), "w": f["w16" if bf16_bank else "w32"], "scale": f["scale"], "shift": f["shift"]}
    buf = torch.zeros(off + N * 3 * H * W, device="cuda")
    x = buf[off:]
    x.copy_(ins["x"])
    w, scale, shift = ins["w"].cuda(), ins["scale"].cuda(), ins["shift"].cuda()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pooled = entry.startswith("pool")
    if pooled:
        Ho, Wo = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    dtype = torch.float32 if entry.startswith("conv7x7_f32") or entry == "pool_f32" else torch.bfloat16
    y = torch.full((N * Ho * Wo * 64,), float("nan"), device="cuda", dtype=dtype)
    name, _, tag = entry.partition(":")
    args = [x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), N, H, W]
    if not pooled:
        args.append(0 if tag == "relu0" else 1)
    rc = getattr(L.lib(), "bevf_stem_" + name)(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (entry, L.lib().bevf_last_error().decode())
    torch.cuda.synchronize()
    return ins, y


def _name(entry, shape):
    N, H, W, off = shape
    return f"{entry}:{N}x{H}x{W}" + (":offset4" if off else "")


CASES = {_name(e, s): functools.partial(run, e, *s) for s in SHAPES for e in ENTRIES}
EXPAND_CASES = {_name("pool_bf16mma", s): functools.partial(run, "pool_bf16mma", *s) for s in SHAPES}


def digests(case):
    ins, y = case()
    return {"in": sha(*sorted(ins.items())), "out": sha(("y", y))}


def expand_digests(lib_path):
    """The digests of EXPAND_CASES from a fresh process that has the switch set."""
    env = dict(os.environ, **{SWITCH: "1"})
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_stem_bits", "--child", lib_path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@functools.lru_cache(maxsize=1)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_these_cases(gpu):
    assert sorted(fixture()["default"]) == sorted(CASES)
    assert sorted(fixture()["expand"]) == sorted(EXPAND_CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_recorded_kernels(gpu, name):
    assert SWITCH not in os.environ, "this process must run the default kernel"
    want, got = fixture()["default"][name], digests(CASES[name])
    assert got["in"] == want["in"], "the input generator changed (not a kernel difference): record again from the anchor commit"
    assert got["out"] == want["out"]


def test_bits_of_the_kernel_behind_the_switch(gpu):
    want, got = fixture()["expand"], expand_digests(L.LIB_PATH)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name]["in"] == want[name]["in"], "the input generator changed (not a kernel difference): record again from the anchor commit"
    assert [n for n in want if got[n]["out"] != want[n]["out"]] == []


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        assert SWITCH in os.environ
        L.LIB_PATH = os.path.abspath(sys.argv[2])                # before the first lib() call
        print(json.dumps({name: digests(case) for name, case in EXPAND_CASES.items()}))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1]:
        L.LIB_PATH = os.path.abspath(sys.argv[1])                # before the first lib() call
    assert SWITCH not in os.environ
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    rec = {"default": {name: digests(case) for name, case in CASES.items()}, "expand": expand_digests(L.LIB_PATH)}
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} + {len(EXPAND_CASES)} cases from {L.LIB_PATH} -> {out}")
