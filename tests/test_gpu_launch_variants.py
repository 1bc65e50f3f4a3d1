"""Kernel instantiations that ask for more than 64 KB of dynamic LDS and that no other test launches (csrc/common.h bevf_launch;
DESIGN.md 3, "Launching with more than 64 KB of LDS").  The opt-in is taken per instantiation at its first launch, so one that lost it
fails only when something launches it: each case here is one launch through the `_lib` wrapper with the variant forced, compared with
the reference and the bound of the neighbouring test file of that kernel.  Every instantiation above 64 KB and the test that launches it
(worked out by reading the dispatch code and the tests' shapes):

  wino_f32<RES, RELU> x GEO 0 / 1, 160 KB (8)      test_gpu_wino.py::test_conv_wino_against_fp64_and_direct: tile 1 -> GEO 0, tile 2 -> GEO 1 (any
                                                   shape); its cases (2,13,21), (1,33,18), (1,16,16), (1,2,47) are the four RES x RELU
  wino_f32<0, 0, STATS>                            test_gpu_wino.py::test_conv_wino_bn_partial_sums
  wino_f32<0, 0, 0, BNB 1>, <1, 0, 0, BNB 2>       test_gpu_training.py::test_bn_backward_fused_into_the_dgrad_epilogue_gives_the_same_gradients
                                                   (c2 -> c1 without a skip gradient, c1 -> the previous block's c2 with it)
  wino_f32<1, 0, 0, BNB 1>, <0, 0, 0, BNB 2>       HERE: test_wino_bn_backward_epilogue
  wino_f32<RES, 1, 0, 0, GEO, DIAG> (4)            HERE: test_wino_diagnostic_launch
  conv3x3_bf16<64, 2, 16>, <128, 2, 16>, 80 KB     test_gpu_conv3x3_bf16.py::test_conv3x3_bf16_against_fp64 (tile 1; Cout = 128)
  conv3x3_bf16_wide64<64>, _persist<64>, 80 KB     the same test, tile 5 at Cin = 64 and tile 4
  conv_igemm<float, 256, 64, 64, 64>, 80 KB        test_gpu_parity.py conv case "tall tile 256x64" (tile 2)
  conv_igemm_hybrid<float, 256, 64, 64, 64>        test_gpu_fullsize.py::test_full_size_conv_linearity_and_tile_invariance (tile 6)
  conv_igemm[_hybrid]<__bf16, 256, 64, 64, 64>     test_gpu_conv_fuzz.py::test_conv_fuzz_bf16 (its cases with tile 2 and tile 6)
  stem_conv7x7<float>, stem_pool7x7, 77 KB         test_gpu_parity.py::test_stem_and_maxpool, test_gpu_stem_pool.py
  stem_conv7x7<__bf16>                             HERE: test_stem_bf16_output
  stem_wgrad, 72 KB                                test_gpu_training.py::test_stem_weight_gradient_direct_kernel
  head_tail_bwd_tiled, 93 KB at the real head      test_gpu_training.py (every training step)

The other conv3x3_bf16 / conv_igemm tiles, conv_split and both bf16-MFMA stems stay at or under 64 KB and take no opt-in."""
import functools

import pytest
import torch
import torch.nn.functional as F

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import synth
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

WINO_TOL = 2e-6                # tests/test_gpu_wino.py: rel_err against fp64 torch
NSTAMPS = 6                    # kWinoStamps: 8-byte time stamps per workgroup of a diagnostic launch


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _wino_case():
    """N=1, 16x16, 32 -> 64 channels: one 16x16 block or two 32x8 blocks, one channel slab.  Computed once, never modified."""
    N, H, W, cin, cout = 1, 16, 16, 32, 64
    x = synth.normal((N, cin, H, W), 11).relu() * 2.0
    w = synth.normal((cout, cin, 3, 3), 12, 0, (2.0 / (9 * cin)) ** 0.5)
    scale, shift = synth.uniform((cout,), 13, 0.5, 1.5), synth.normal((cout,), 14, 0, 0.3)
    rs = synth.normal((N, cout, H, W), 15)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    return (N, H, W, cin, cout), x, w, scale, shift, rs, ref


@pytest.mark.parametrize("tile,blocks", [(1, 1), (2, 2)], ids=["16x16", "32x8"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
def test_wino_diagnostic_launch(gpu, res, tile, blocks):
    """bevf_debug_wino_stamps: the next ReLU launches run wino_f32<RES, true, false, 0, GEO, DIAG = true> -- same result, and every
    workgroup (and nothing else) leaves its six time stamps in launch order."""
    (N, H, W, cin, cout), x, w, scale, shift, rs, ref = _wino_case()
    ref = (ref + rs.double() if res else ref).relu()
    u = L.wino_filter_transform(_nhwc(w).view(-1).to(gpu), cout, cin)
    y = torch.full((N * H * W * cout,), -5.0, device=gpu)
    buf = torch.zeros((blocks + 2) * NSTAMPS, dtype=torch.int64, device=gpu)
    L.lib().bevf_debug_wino_stamps(buf.data_ptr())
    try:
        L.conv3x3_wino(_nhwc(x).view(-1).to(gpu), u, scale.to(gpu), shift.to(gpu), y, N=N, H=H, W=W, Cin=cin, x_cs=cin, Cout=cout,
                       y_cs=cout, relu=True, res=_nhwc(rs).view(-1).to(gpu) if res else None, res_cs=cout if res else 0, tile=tile)
        torch.cuda.synchronize()
    finally:
        L.lib().bevf_debug_wino_stamps(None)
    err = rel_err(y.view(N, H, W, cout).permute(0, 3, 1, 2).cpu(), ref)
    print(f"res={res} tile={tile}: rel_err {err:.3e}")
    assert err <= WINO_TOL
    t = buf.view(-1, NSTAMPS).cpu()
    assert bool((t[:blocks] != 0).all()) and bool((t[blocks:] == 0).all())
    assert bool((t[:blocks, 1:] >= t[:blocks, :-1]).all())


BNB_PIX = 256                  # one 16x16 block: one row of partial sums
SUM_ROUNDINGS = 32             # fp32 roundings on the way to a channel's sum: 16 per lane, 2 shuffle levels, 4 waves, the fma (< 32)


@functools.lru_cache(maxsize=None)
def _bnb_case():
    """The data-gradient use of wino_f32: N=1, 16x16, 64 -> 64 channels (one block, one row of partials).  The consumer's BatchNorm
    input, mean, invstd, gamma and beta are small dyadic numbers, so its normalised input and pre-activation are exact in fp32 and
    the ReLU mask the kernel derives from them is the float64 one, whatever the order of the arithmetic."""
    N, H, W, c = 1, 16, 16, 64
    dy = synth.normal((N, c, H, W), 21)
    w = synth.normal((c, c, 3, 3), 22, 0, (2.0 / (9 * c)) ** 0.5)
    rs = synth.normal((N, c, H, W), 23)
    bx = (synth.normal((N, c, H, W), 24) * 8).round() / 8
    by = synth.normal((N, c, H, W), 25)
    mean = (synth.normal((c,), 26) * 4).round() / 4
    invstd = torch.tensor([0.5, 1.0, 2.0]).repeat(22)[:c]
    gamma = torch.tensor([1.0, -1.0, 2.0, 0.5]).repeat(16)
    beta = (synth.normal((c,), 27) * 4).round() / 4
    conv = F.conv2d(dy.double(), w.double(), None, 1, 1)
    return (N, H, W, c), dy, w, rs, bx, by, mean, invstd, gamma, beta, conv


@pytest.mark.parametrize("mask_from_y,res", [(False, True), (True, False)], ids=["bnb1_residual", "bnb2_plain"])
def test_wino_bn_backward_epilogue(gpu, mask_from_y, res):
    """wino_f32<RES, false, false, BNB>: BNB = 1 (mask from the recomputed pre-activation) with a residual and BNB = 2 (mask from the
    stored output) without -- the training step launches the other two.  Output: the fp64 convolution (+ residual) under the exact
    mask, rel_err <= the bound of tests/test_gpu_wino.py.  Partial sums {sum o, sum o xhat} per channel: that bound allows every
    element an error E = 2e-6 max|o|, so a sum may be off by E sum|xhat| (256 E for the plain sum), plus SUM_ROUNDINGS fp32
    roundings of the sum of the terms' magnitudes."""
    (N, H, W, c), dy, w, rs, bx, by, mean, invstd, gamma, beta, conv = _bnb_case()
    v = lambda t: t.double().view(1, -1, 1, 1)
    xhat = (bx.double() - v(mean)) * v(invstd)
    mask = (by > 0) if mask_from_y else (xhat * v(gamma) + v(beta) > 0)
    ref = (conv + rs.double() if res else conv) * mask
    M = N * H * W
    assert L.wino_stat_rows(N, H, W) == 1
    part = torch.full((c * 2,), float("nan"), device=gpu)
    y = torch.full((M * c,), -5.0, device=gpu)
    u = L.wino_filter_transform(_nhwc(w).view(-1).to(gpu), c, c)
    bnb = dict(x=_nhwc(bx).view(-1).to(gpu), y=_nhwc(by).view(-1).to(gpu) if mask_from_y else None, mean=mean.to(gpu),
               invstd=invstd.to(gpu), gamma=gamma.to(gpu), beta=beta.to(gpu))
    L.conv3x3_wino(_nhwc(dy).view(-1).to(gpu), u, None, None, y, N=N, H=H, W=W, Cin=c, x_cs=c, Cout=c, y_cs=c, relu=False,
                   res=_nhwc(rs).view(-1).to(gpu) if res else None, res_cs=c if res else 0, stats=part, bnb=bnb)
    torch.cuda.synchronize()
    err = rel_err(y.view(N, H, W, c).permute(0, 3, 1, 2).cpu(), ref)
    print(f"bnb={2 if mask_from_y else 1} res={res}: rel_err {err:.3e}")
    assert err <= WINO_TOL
    got = part.view(c, 2).cpu().double()
    E, eps = WINO_TOL * float(ref.abs().max()), 2.0 ** -24
    terms = ref * xhat
    b1 = BNB_PIX * E + SUM_ROUNDINGS * eps * ref.abs().sum(dim=(0, 2, 3))
    b2 = E * xhat.abs().sum(dim=(0, 2, 3)) + SUM_ROUNDINGS * eps * terms.abs().sum(dim=(0, 2, 3))
    r1 = ((got[:, 0] - ref.sum(dim=(0, 2, 3))).abs() / b1).max()
    r2 = ((got[:, 1] - terms.sum(dim=(0, 2, 3))).abs() / b2).max()
    print(f"  sums: worst |dev - ref| / bound {float(r1):.3f} (sum o), {float(r2):.3f} (sum o xhat)")
    assert float(r1) <= 1.0 and float(r2) <= 1.0


def test_stem_bf16_output(gpu):
    """stem_conv7x7<__bf16> (bevf_stem_conv7x7_bf16out: the fp32 stem storing bf16) against torch as tests/test_gpu_parity.py's stem
    case, with the bound tests/test_gpu_bf16.py gives a kernel that rounds once, at the store."""
    N, H, W = 1, 32, 32
    x = synth.normal((N, 3, H, W), 31)
    w = synth.normal((64, 3, 7, 7), 32, 0, 0.08)
    scale, shift = synth.uniform((64,), 33, 0.5, 1.5), synth.normal((64,), 34, 0, 0.2)
    ref = F.relu(F.conv2d(x, w, None, 2, 3) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    Ho, Wo = ref.shape[-2:]
    packed = torch.zeros(148, 64)
    packed[:147] = w.reshape(64, 147).t()
    y = torch.full((N * Ho * Wo * 64,), float("nan"), dtype=torch.bfloat16, device=gpu)
    L.stem_conv7x7(x.to(gpu), packed.view(-1).to(gpu), scale.to(gpu), shift.to(gpu), y, N, H, W)
    err = rel_err(y.float().view(N, Ho, Wo, 64).permute(0, 3, 1, 2).cpu(), ref)
    print(f"stem bf16 out: rel_err {err:.3e}")
    assert err <= 4e-3
