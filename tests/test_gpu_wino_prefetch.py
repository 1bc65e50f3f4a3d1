"""wino_f32's prologue and its idle "next chunk" DMA slots (csrc/conv_wino.hip; DESIGN.md 3.1b "The prologue, measured in two parts").
These cases were written for a first-patch prefetch -- in its last chunk a workgroup touched the chunk-0 lines of the patch of the workgroup
256 dispatch positions behind it -- which was measured and not kept; they stay because they guard what the prologue does now (each slot's
DMA issued as its offset exists, the hand-written first wait that leaves the chunk-1 loads in flight) and what the idle slots of a tile's
last chunk do (zeros into the idle buffer, the residual prefetch).  None of that can change a result, so the cases guard addressing and
synchronisation: a grid of one block, a grid that crosses a slab (z) boundary, edge blocks in every direction, dead rows of the stacked
tilings, and (Cin = 32) a tile whose last chunk is its first, so that the prologue's own chunk-1 slots are idle too; the input ends exactly
where its allocation ends, and the output sits in a wider buffer whose gaps and tail must keep their poison.  Error measure and bound are
those of tests/test_gpu_wino.py (rel_err against fp64 torch <= 2e-6); every tiling the launcher can be forced into must give the same bits."""
import functools

import pytest
import torch
import torch.nn.functional as F

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import synth
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

POISON = -5.0
TAIL = 1024                                                     # poisoned floats behind the last output pixel
HEAD = 64                                                       # floats in front of x in its allocation (keeps the 16-byte alignment)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(N, H, W, cin, cout):
    """Inputs and the fp64 reference before residual / ReLU: computed once per shape, shared by its two tests, never modified."""
    s = N * 1000 + H * 10 + cin
    x = synth.normal((N, cin, H, W), s + 1).relu() * 2.0
    w = synth.normal((cout, cin, 3, 3), s + 2, 0, (2.0 / (9 * cin)) ** 0.5)
    scale, shift = synth.uniform((cout,), s + 3, 0.5, 1.5), synth.normal((cout,), s + 4, 0, 0.3)
    rs = synth.normal((N, cout, H, W), s + 5)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return x, w, scale, shift, rs, ref


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("N,H,W,cin,cout,ycs", [
    (3, 37, 45, 96, 80, 96),      # edge blocks in every direction, a partial channel slab, 2 slabs
    (2, 17, 19, 32, 64, 72),      # one chunk: the last chunk is chunk 0, and the slots group 3 fetches are idle as well
    (1, 1, 1, 64, 64, 80),        # a one-block grid, one pixel: every other slot of the patch is out of range
    (5, 57, 100, 64, 64, 68),     # stacked rows with dead rows between the images, 32x8 blocks chosen; under 256 blocks (less than one per CU)
    (12, 57, 100, 64, 64, 68)])   # ... and more than 256
def test_wino_prefetch_shapes(gpu, N, H, W, cin, cout, ycs, res):
    x, w, scale, shift, rs, ref = _case(N, H, W, cin, cout)
    relu = cin != 32                                            # the one-chunk case also runs the epilogues without ReLU
    if res:
        ref = ref + rs.double()
    if relu:
        ref = ref.relu()
    M = N * H * W
    xall = torch.full((HEAD + M * cin,), 7.0, device=gpu)
    xall[HEAD:] = _nhwc(x).view(-1).to(gpu)
    xs = xall[HEAD:]                                            # ends exactly where its allocation ends: nothing behind it is padding
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() + xs.numel() * 4 == xall.data_ptr() + xall.numel() * 4
    rb = _nhwc(rs).view(-1).to(gpu) if res else None
    u = L.wino_filter_transform(_nhwc(w).view(-1).to(gpu), cout, cin)
    sc, sh = scale.to(gpu), shift.to(gpu)
    outs = []
    for tile in (0, 1, 2, 3, 4):                                # auto; 16x16 / 32x8-pixel blocks per image; the same over stacked rows
        y = torch.full((M * ycs + TAIL,), POISON, device=gpu)
        L.conv3x3_wino(xs, u, sc, sh, y, N=N, H=H, W=W, Cin=cin, x_cs=cin, Cout=cout, y_cs=ycs, relu=relu, res=rb,
                       res_cs=cout if res else 0, tile=tile)
        got = y.cpu()
        body = got[:M * ycs].view(M, ycs)
        err = rel_err(body[:, :cout].view(N, H, W, cout).permute(0, 3, 1, 2), ref)
        print(f"N={N} {H}x{W} {cin}->{cout} res={res} tile={tile}: rel_err {err:.3e}")
        assert err <= 2e-6
        assert bool((body[:, cout:] == POISON).all())            # the gaps of the wider pixels ...
        assert bool((got[M * ycs:] == POISON).all())             # ... and the tail behind the last pixel are intact
        outs.append(got)
    assert all(torch.equal(outs[0], o) for o in outs[1:])        # the tiling changes a tile's block, not its arithmetic
    assert bool((xall[:HEAD] == 7.0).all()) and torch.equal(xall[HEAD:].cpu(), _nhwc(x).view(-1))   # the input is untouched
