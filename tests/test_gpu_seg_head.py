"""BEV map-segmentation head on the GPU: the resample, focal-loss and IoU kernels against tests/seg_ref.py, the
head module in eval (fp32, bf16) and train mode against the fp64 composition, and the detector with its second consumer of the
fused map -- eager, trained, combined with the other options, and as a replayed graph.

Bounds.  Forward resample: each of the four products w_k v_k carries the weight's rounding to fp32 and the product's (the first
product) or the fma's, and there are three additions: |y - ref| <= 8 * 2^-24 * max_k |v_k|, as tests/test_gpu_temporal.py derives
for the same arithmetic; a bf16 output adds its rounding, 2^-8 |ref|.
Backward resample: dx = sum_k w_k dy_k over the n contributing targets of a source cell, accumulated by n fmas in fp32.  Each
weight is the fp64 product rounded once to fp32 (relative 2^-24), each fma rounds a partial sum whose magnitude is at most
S = sum_k |w_k dy_k| (1 + O(2^-24)) (relative 2^-24), so to first order |dx - ref| <= (1 + n) 2^-24 S; one more 2^-24 S covers the
second-order terms for every n below 2^20.  Hence (n + 2) * 2^-24 * S, the bound tests/test_gpu_temporal.py holds bev_warp_bwd to.
The adjoint identity <dy, fwd(x)> = <bwd(dy), x> is held to the sum of those two elementwise bounds weighed by |dy| and |x|.
Focal loss: the yardstick is torch's fp32 CPU evaluation of seg_ref.focal (the same stable formula) against the fp64 one; the
kernel's worst relative error over all cases (per_class entries and loss) may be 4 x the yardstick's worst, the factor covering
the different summation order; the gradient likewise, elementwise relative to max |grad|, against fp32 torch autograd.
"""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct
from bevfusion_multimodal_3d_object_detection_amd import engine, fusion, seg_head, synth
from tests import seg_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SENT = 777.0
# input ranges with cells of exactly 1 x 1: whole-cell shifts give weights of exactly 0 / 1
IN_RANGE = {(6, 5): [-2.5, -3.0, 2.5, 3.0], (12, 9): [-4.5, -6.0, 4.5, 6.0], (8, 8): [-4.0, -4.0, 4.0, 4.0]}
GRIDS = [((6, 5), (6, 5)), ((6, 5), (9, 7)), ((12, 9), (5, 4)), ((8, 8), (16, 16))]
SHAPES = [(C, pad) for C in (4, 68, 260) for pad in (0, 8)]
TAIL = [(6, 1), (7, 0)]                                # C % 4 != 0, odd strides: the scalar path of every kernel


def _cells(rng, sx, sy, Ho, Wo):
    """Ho x Wo cells of the input's own size, the origin moved by (sx, sy) whole cells."""
    return [rng[0] + sx, rng[1] + sy, rng[0] + sx + Wo, rng[1] + sy + Ho]


def _exact_ranges(hw_in, hw_out):
    rng, (Ho, Wo) = IN_RANGE[hw_in], hw_out
    out = dict(shift=_cells(rng, -1.0, 2.0, Ho, Wo), disjoint=_cells(rng, 3.0 * hw_in[1], 0.0, Ho, Wo),
               nan=[rng[0], float("nan"), rng[0] + Wo, rng[1] + Ho])
    if hw_in == hw_out:
        out["same"] = list(rng)
    return out


# one general case per grid pair: partial overlap at the input's cell size, a non-integer ratio, down-sampling, 2 x up -- each
# reaching past the input on one side so that interior, border and outside cells all occur
GENERAL = {((6, 5), (6, 5)): [-2.5 + 1.3, -3.0 - 2.4, 2.5 + 1.3, 3.0 - 2.4],
           ((6, 5), (9, 7)): [-4.1, -5.3, 0.9, 3.9],
           ((12, 9), (5, 4)): [-7.5, -8.2, 7.5, 7.3],
           ((8, 8), (16, 16)): [-5.25, -5.25, 2.75, 2.75]}


def _x(B, H, W, C, x_cs, dtype, seed):
    rows = synth.normal((B * H * W, x_cs), seed).to(dtype)
    return rows, rows[:, :C].float().numpy().astype(np.float64).reshape(B, H, W, C)


def _forward(rows, hw_in, hw_out, out_range, C, x_cs, pad, dtype):
    """-> the slot [B][Ho][Wo][C] as fp64: the last third of a (3C + pad)-wide sentinel buffer, whose other columns must stay."""
    (Hi, Wi), (Ho, Wo), B = hw_in, hw_out, 2
    y = torch.full((B * Ho * Wo, 3 * C + pad), SENT, dtype=dtype, device="cuda")
    gi, go = R.grid_of(IN_RANGE[hw_in], Hi, Wi), R.grid_of(out_range, Ho, Wo)
    L.bev_grid_resample(rows.cuda().view(-1), y.view(-1)[2 * C:], B, Hi, Wi, Ho, Wo, C, x_cs, 3 * C + pad, gi, go)
    torch.cuda.synchronize()
    keep = torch.cat([y[:, :2 * C], y[:, 3 * C:]], 1)
    assert (keep == SENT).all(), "the resample wrote outside its slot"
    slot = y[:, 2 * C:3 * C]
    return slot.float().cpu().numpy().astype(np.float64).reshape(B, Ho, Wo, C), slot, gi, go


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_resample_exact_cases_are_bit_exact(gpu, dtype):
    checked = 0
    for hw_in, hw_out in GRIDS:
        for C, pad in SHAPES + TAIL[:1]:
            rows, x = _x(2, *hw_in, C, C + pad, dtype, 3)
            for name, out_range in _exact_ranges(hw_in, hw_out).items():
                got, slot, gi, go = _forward(rows, hw_in, hw_out, out_range, C, C + pad, pad, dtype)
                w = R.corners(gi, go, *hw_in, *hw_out)[2]
                assert set(np.unique(w)) <= {0.0, 1.0}, (name, hw_in, hw_out)        # the case is what it claims
                ref, _ = R.resample(x, gi, go, *hw_out)
                assert np.array_equal(got, ref), (name, hw_in, hw_out, C, pad)
                assert not (slot == SENT).any()                                       # every element of the slot is written
                if name == "same":
                    assert np.array_equal(got, x)
                elif name == "shift":
                    assert (ref == 0).all(-1).any() and (ref != 0).any()              # zero rows where it leaves the input
                else:
                    assert (got == 0).all()                                           # disjoint / NaN: all zero
                checked += 1
    assert checked == 7 * (3 * 3 + 4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_resample_general_cases_within_the_derived_bound(gpu, dtype):
    """8 * 2^-24 * max|corner| (+ 2^-8 |ref| for a bf16 output); the reference sees the inputs as stored; no element left out."""
    worst = 0.0
    for hw_in, hw_out in GRIDS:
        for C, pad in SHAPES + TAIL:
            rows, x = _x(2, *hw_in, C, C + pad, dtype, 6)
            got, _, gi, go = _forward(rows, hw_in, hw_out, GENERAL[(hw_in, hw_out)], C, C + pad, pad, dtype)
            ref, vmax = R.resample(x, gi, go, *hw_out)
            inside = R.corners(gi, go, *hw_in, *hw_out)[3]
            assert inside.all(0).any() and (~inside.any(0)).any() and (inside.any(0) & ~inside.all(0)).any()   # interior, outside, border
            bound = 8 * EPS * vmax + (2.0 ** -8 * np.abs(ref) if dtype == torch.bfloat16 else 0.0)
            err = np.abs(got - ref)
            assert err.shape == bound.shape and (err <= bound).all(), (hw_in, hw_out, C, pad, float((err / np.maximum(bound, 1e-300)).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"bev_grid_resample forward {dtype}: worst error / bound = {worst:.3f}")


def _backward(dy_rows, off, dy_cs, hw_in, hw_out, out_range, C):
    (Hi, Wi), (Ho, Wo), B = hw_in, hw_out, 2
    dx = torch.full((B * Hi * Wi * C,), SENT, device="cuda")
    gi, go = R.grid_of(IN_RANGE[hw_in], Hi, Wi), R.grid_of(out_range, Ho, Wo)
    L.bev_grid_resample_bwd(dy_rows.view(-1)[off:], dx, B, Hi, Wi, Ho, Wo, C, dy_cs, gi, go)
    torch.cuda.synchronize()
    return dx, gi, go


def test_resample_backward_bound_adjoint_full_write_and_determinism(gpu):
    worst, worst_adj, multi = 0.0, 0.0, False
    for hw_in, hw_out in GRIDS:
        ranges = dict(_exact_ranges(hw_in, hw_out), general=GENERAL[(hw_in, hw_out)])
        for C, pad in SHAPES + TAIL:
            rows = synth.normal((2 * hw_out[0] * hw_out[1], 3 * C + pad), 8)
            dy = rows[:, 2 * C:3 * C].numpy().astype(np.float64).reshape(2, *hw_out, C)
            if pad == 8:                                                       # the dense layout as well as the strided slice
                dy_rows, dy_cs, off = rows[:, 2 * C:3 * C].contiguous().cuda(), C, 0
            else:
                dy_rows, dy_cs, off = rows.cuda(), 3 * C + pad, 2 * C
            for name, out_range in ranges.items():
                dx1, gi, go = _backward(dy_rows, off, dy_cs, hw_in, hw_out, out_range, C)
                dx2, _, _ = _backward(dy_rows, off, dy_cs, hw_in, hw_out, out_range, C)
                assert torch.equal(dx1, dx2), (name, hw_in, hw_out, C, pad)
                got = dx1.cpu().numpy().astype(np.float64).reshape(2, *hw_in, C)
                ref, mag, n = R.resample_bwd(dy, gi, go, *hw_in)
                bound = (n[None, :, :, None] + 2) * EPS * mag
                err = np.abs(got - ref)
                assert (err <= bound).all(), (name, hw_in, hw_out, C, pad, float((err / np.maximum(bound, 1e-300)).max()))
                assert (got[:, n == 0] == 0).all()                             # every element is written, zeros included
                if name != "general":
                    continue
                assert (n == 0).any() and (n > 0).any()
                multi = multi or bool((n > 1).any())
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
                xr, x = _x(2, *hw_in, C, C, torch.float32, 9)
                y, _, _, _ = _forward(xr, hw_in, hw_out, out_range, C, C, 0, torch.float32)
                _, vmax = R.resample(x, gi, go, *hw_out)
                a, b = float((y * dy).sum()), float((x * got).sum())
                tol = float((np.abs(dy) * 8 * EPS * vmax).sum() + (np.abs(x) * bound).sum())
                assert abs(a - b) <= tol, (a, b, tol)
                worst_adj = max(worst_adj, abs(a - b) / tol)
    assert multi                                                               # some source cell sums several targets
    print(f"bev_grid_resample backward: worst error / bound = {worst:.3f}, worst adjoint mismatch / bound = {worst_adj:.3f}")


def test_public_resample_autograd_and_layouts(gpu):
    hw_in, hw_out, C = (12, 9), (5, 4), 68
    in_range, out_range = IN_RANGE[hw_in], GENERAL[(hw_in, hw_out)]
    gi, go = R.grid_of(in_range, *hw_in), R.grid_of(out_range, *hw_out)
    x = synth.normal((2, C, *hw_in), 10)
    g = synth.normal((2, C, *hw_out), 11)
    ref, _ = R.resample(x.permute(0, 2, 3, 1).double().numpy(), gi, go, *hw_out)
    dref = R.resample_bwd(g.permute(0, 2, 3, 1).double().numpy(), gi, go, *hw_in)[0]
    outs = []
    for xin in (x.cuda(), x.cuda().contiguous(memory_format=torch.channels_last)):
        xin.requires_grad_(True)
        y = seg_head.bev_grid_resample(xin, in_range, out_range, hw_out)
        assert y.shape == (2, C, *hw_out) and y.is_contiguous(memory_format=torch.channels_last)
        (y * g.cuda()).sum().backward()
        assert rel_err(y.detach().cpu().permute(0, 2, 3, 1), ref) <= 1e-6 and rel_err(xin.grad.cpu().permute(0, 2, 3, 1), dref) <= 1e-6
        outs.append((y.detach(), xin.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    yb = seg_head.bev_grid_resample(x.cuda().bfloat16(), in_range, out_range, hw_out)
    assert yb.dtype == torch.bfloat16 and rel_err(yb.float().cpu().permute(0, 2, 3, 1), ref) <= 2e-2


# ---- focal loss and IoU ---------------------------------------------------------------------------------------------------------------

FOCAL_CASES = [(K, P, cs) for K in (1, 6) for P in (35, 1000) for cs in ((K + 3) // 4 * 4, 32)]
PLANTED = (30.0, -30.0, 90.0, -90.0)


def _focal_inputs(K, P, seed):
    """logits (2, K, 1, P) = 4 * normal with +-30 and +-90 planted under both target values, targets ~30 % ones with (K = 6) one
    all-zero and one all-one class."""
    x = 4 * synth.normal((2, K, 1, P), seed)
    t = (synth.uniform((2, K, 1, P), seed + 1) < 0.3).float()
    x[:, :, 0, :4] = torch.tensor(PLANTED)
    t[0, :, 0, :4], t[1, :, 0, :4] = 1.0, 0.0                            # frame 0 plants them on ones, frame 1 on zeros
    if K > 1:
        t[:, 1], t[:, 4] = 0.0, 1.0
    return x, t


def _rows(x, cs, fill=5.0):
    """(B, K, 1, P) -> device rows [B * P][cs], the padding columns holding `fill` (the kernels must not read them)."""
    B, K, _, P = x.shape
    rows = torch.full((B * P, cs), fill)
    rows[:, :K] = x.permute(0, 2, 3, 1).reshape(B * P, K)
    return rows.cuda()


_FOCAL = {}


def _focal_reference(K, P, alpha, gamma):
    """fp64 reference and the fp32 torch yardstick for one case: computed once, shared, never modified."""
    key = (K, P, alpha, gamma)
    if key not in _FOCAL:
        x, t = _focal_inputs(K, P, 30 + K + P)
        pc64, l64 = R.focal(x.double(), t.double(), alpha, gamma)
        x32 = x.clone().requires_grad_(True)
        pc32, l32 = R.focal(x32, t, alpha, gamma)
        l32.backward()
        _FOCAL[key] = dict(x=x, t=t, pc64=pc64, l64=l64, g64=R.focal_grad(x, t, alpha, gamma), pc32=pc32.detach(), l32=l32.detach(),
                           g32=x32.grad)
    return _FOCAL[key]


def _relerr(a, b):
    return float(((a.double() - b.double()).abs() / b.double().abs()).max())


@pytest.mark.parametrize("alpha,gamma", [(-1.0, 2.0), (0.25, 2.0), (0.6, 1.5)])
def test_focal_loss_and_gradient_against_the_fp32_yardstick(gpu, alpha, gamma):
    """Measured on an MI355X (worst over the eight cases; DESIGN.md 3.2i holds the figures): the kernel's relative error on
    per_class / loss and its gradient error relative to max |grad|, each beside the fp32-torch yardstick's."""
    k_val = y_val = k_grad = y_grad = 0.0
    gscale = 1.7
    for K, P, cs in FOCAL_CASES:
        r = _focal_reference(K, P, alpha, gamma)
        rows, tg = _rows(r["x"], cs), r["t"].to(torch.uint8).contiguous().cuda()
        work = torch.empty(L.seg_focal_work_doubles(K), dtype=torch.float64, device="cuda")
        outs = []
        for _ in range(2):
            out = torch.full((K + 1,), SENT, device="cuda")
            L.seg_focal_loss(rows, cs, tg, 2, P, K, alpha, gamma, work, out)
            dl = torch.full((2 * P, cs), SENT, device="cuda")
            L.seg_focal_loss_bwd(rows, cs, tg, torch.tensor([gscale], device="cuda"), dl, 2, P, K, alpha, gamma)
            outs.append((out.cpu(), dl.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])          # two runs bit-equal
        out, dl = outs[0]
        assert torch.isfinite(out).all() and torch.isfinite(dl).all()                                # finite at +-90
        assert (dl[:, K:] == 0).all()                                                                # padding columns exactly 0
        k_val = max(k_val, _relerr(out[:K], r["pc64"]), _relerr(out[K:], r["l64"].reshape(1)))
        y_val = max(y_val, _relerr(r["pc32"], r["pc64"]), _relerr(r["l32"].reshape(1), r["l64"].reshape(1)))
        g64 = r["g64"].permute(0, 2, 3, 1).reshape(2 * P, K)
        gmax = float(g64.abs().max())
        k_grad = max(k_grad, float((dl[:, :K].double() / gscale - g64).abs().max()) / gmax)
        y_grad = max(y_grad, float((r["g32"].permute(0, 2, 3, 1).reshape(2 * P, K).double() - g64).abs().max()) / gmax)
    print(f"seg focal loss alpha={alpha} gamma={gamma}: value rel err kernel {k_val:.3e} / fp32 torch {y_val:.3e}; "
          f"gradient err / max|grad| kernel {k_grad:.3e} / fp32 torch autograd {y_grad:.3e}")
    assert k_val <= 4 * y_val, (k_val, y_val)
    assert k_grad <= 4 * y_grad, (k_grad, y_grad)


def test_focal_module_autograd(gpu):
    r = _focal_reference(6, 1000, -1.0, 2.0)
    x = r["x"].reshape(2, 6, 25, 40).cuda().requires_grad_(True)
    t = r["t"].reshape(2, 6, 25, 40)
    res = seg_head.SegFocalLoss()(x, t.bool().cuda())
    assert set(res) == {"loss", "per_class"} and res["per_class"].shape == (6,) and not res["per_class"].requires_grad
    (3.0 * res["loss"]).backward()
    assert rel_err(res["loss"].detach().cpu(), r["l64"]) <= 1e-6 and rel_err(res["per_class"].cpu(), r["pc64"]) <= 1e-6
    assert rel_err(x.grad.cpu() / 3.0, r["g64"].reshape(2, 6, 25, 40)) <= 1e-6
    for tt in (t.to(torch.uint8).cuda(), t.cuda(), t.double()):                               # the other target dtypes, host or device
        assert torch.equal(seg_head.SegFocalLoss()(x.detach(), tt)["loss"], res["loss"].detach())
    with pytest.raises(L.BevfError, match="bool, uint8 or float"):
        seg_head.SegFocalLoss()(x, t.long().cuda())
    with pytest.raises(L.BevfError, match="mask tensor"):
        seg_head.SegFocalLoss()(x, t[:, :5].cuda())


def test_iou_counts_equal_the_reference(gpu):
    thr = R.threshold_logits(seg_head.DEFAULT_THRESHOLDS)
    x, t = _focal_inputs(6, 1000, 77)
    x, t = x.reshape(2, 6, 25, 40).clone(), t.reshape(2, 6, 25, 40)
    for k, v in enumerate(thr[:6]):                                      # logits exactly on a threshold count as predicted
        x[0, k, 3, 5 + k], x[1, k, 7, 9] = float(v), float(v)
    x[0, 0, 4, 4] = float(np.nextafter(thr[3], np.float32(-np.inf)))     # and one float below does not
    want = R.iou_counts(x.numpy(), t.numpy(), thr)
    on = R.iou_counts(np.where(x.numpy() == thr[3], np.float32(np.nextafter(thr[3], np.float32(-np.inf))), x.numpy()), t.numpy(), thr)
    assert not np.array_equal(want, on)                                   # the planted logits do decide counts
    got = seg_head.seg_iou_counts(x.cuda(), t.bool().cuda())
    assert got.dtype == torch.int64 and got.shape == (7, 6, 3) and np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, seg_head.seg_iou_counts(x.cuda(), t.cuda()))
    iou = seg_head.seg_iou(got)
    assert iou["iou"].shape == (7, 6) and float(iou["iou"][:, 1].max()) == 0.0 and 0.0 < float(iou["mean_iou"]) < 1.0
    # a padded row stride, one class, a pixel count that is no multiple of the wave
    x1, t1 = _focal_inputs(1, 35, 78)
    counts = torch.full((2, 1, 3), -1, dtype=torch.int64, device="cuda")
    L.seg_iou_counts(_rows(x1, 32), 32, t1.to(torch.uint8).cuda(), torch.from_numpy(thr[2:4]).cuda(), counts, 2, 35, 1)
    assert np.array_equal(counts.cpu().numpy(), R.iou_counts(x1.numpy(), t1.numpy(), thr[2:4]))


# ---- the head module ------------------------------------------------------------------------------------------------------------------

PC = [-4.5, -6.0, -5.0, 4.5, 6.0, 3.0]
OUT_RANGE, OUT_SIZE = [-3.7, -5.2, 4.1, 4.4], (10, 14)


def _head_pair(seed=3):
    mod = seg_head.BEVSegmentationHead(in_channels=64, num_classes=6, pc_range=PC, bev_h=12, bev_w=9, output_range=OUT_RANGE,
                                       output_size=OUT_SIZE)
    ref = R.SegHeadRef(64, 6, 64, mod.in_grid, mod.out_grid, (12, 9), OUT_SIZE)
    synth.fill_state_dict_(ref, seed)
    mod.load_state_dict(ref.state_dict())
    return ref, mod


def _r16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def test_head_eval_fp32_and_bf16_against_the_fp64_composition(gpu):
    ref, mod = _head_pair()
    x = synth.normal((2, 64, 12, 9), 21)
    with torch.no_grad():
        want = ref.double().eval()(x.double())
    out = mod.cuda().eval()(x.cuda())
    assert out.shape == (2, 6, 10, 14) and out.dtype == torch.float32 and not out.requires_grad
    e32 = rel_err(out.cpu(), want)
    # bf16 storage: the reference on bf16-rounded weights, buffers and input, as tests/test_gpu_bf16.py does
    ref16, mod16 = _head_pair()
    with torch.no_grad():
        for t in list(ref16.parameters()) + [b for b in ref16.buffers() if b.dtype.is_floating_point]:
            t.copy_(_r16(t))
    mod16.load_state_dict(ref16.state_dict())
    with torch.no_grad():
        want16 = ref16.double().eval()(_r16(x).double())
    out16 = mod16.cuda().bfloat16().eval()(x.cuda())
    assert out16.dtype == torch.float32
    e16 = rel_err(out16.cpu(), want16)
    print(f"BEVSegmentationHead eval: rel_err fp32 {e32:.3e}, bf16 storage {e16:.3e}")
    assert e32 <= 1e-4 and e16 <= 3e-2


@pytest.fixture
def exact_convs():
    """Conv mode "f32" (the exact kernel), the remedy of tests/test_gpu_standalone_train.py: forward values within 1e-7 of the
    reference, so ReLU decisions agree and the gradient comparison can be tight."""
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    yield
    engine.set_conv_mode(old)


def _check_grads(named, ref_named, what, hard=2e-2, tight=2e-3, most=8):
    """tests/test_gpu_standalone_train._check_params restated for (name, gradient) pairs: relative L2 per tensor (plus a floor of
    5e-5 of the whole gradient norm), every tensor within `hard`, all but max(2, n / most) within `tight`."""
    gref = dict(ref_named)
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gref.values())))
    worst = []
    for name, g in named:
        assert g is not None, name
        r = gref[name].double().cpu()
        worst.append((round(float((g.cpu().double() - r).norm() / (r.norm() + 5e-5 * gn)), 6), name))
    worst.sort(reverse=True)
    print(f"{what}: worst gradients {worst[:4]}")
    assert worst and worst[0][0] <= hard, worst[:6]
    loose = sum(w > tight for w, _ in worst)
    assert loose <= max(2, len(worst) // most), (loose, worst[:6])


def test_head_alone_in_train_mode_against_fp64_autograd(gpu, exact_convs):
    ref, mod = _head_pair(seed=5)
    ref, mod = ref.double().train(), mod.cuda().train()
    x = synth.normal((2, 64, 12, 9), 22)
    w = synth.normal((2, 6, 10, 14), 23)
    xr, xg = x.double().requires_grad_(True), x.cuda().requires_grad_(True)
    want, out = ref(xr), mod(xg)
    assert out.requires_grad and rel_err(out.detach().cpu(), want.detach()) <= 1e-4
    (want * w.double()).sum().backward()
    (out * w.cuda()).sum().backward()
    _check_grads([(n, p.grad) for n, p in mod.named_parameters()], [(n, p.grad) for n, p in ref.named_parameters()], "seg head parameters")
    for (n1, b1), (n2, b2) in zip(mod.named_buffers(), ref.named_buffers()):          # BatchNorm running statistics moved alike
        assert n1 == n2 and rel_err(b1.cpu().double(), b2.double()) <= 2e-5, n1
    assert int(mod.classifier[1].num_batches_tracked) == 4
    assert xg.grad.shape == x.shape and rel_err(xg.grad.cpu(), xr.grad) <= 2e-4
    with torch.no_grad():                                                           # train mode under no_grad: batch statistics still
        again = mod(x.cuda())
    assert not again.requires_grad and rel_err(again.cpu(), want.detach()) <= 1e-4
    with pytest.raises(L.BevfError, match="train mode is not supported"):
        mod.bfloat16()(x.cuda().requires_grad_(True))


# ---- the detector ---------------------------------------------------------------------------------------------------------------------

SEG = dict(num_classes=3, output_range=[-30, -30, 30, 30], output_size=(12, 12))


def _detectors(seed=7):
    """The detector with the seg head and one without it on the same weights."""
    m = fusion.create_detector("camera+lidar", bev_h=16, bev_w=16, seg_head=SEG)
    synth.fill_state_dict_(m, seed)
    plain = fusion.create_detector("camera+lidar", bev_h=16, bev_w=16)
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("seg_head.")})
    return m.cuda(), plain.cuda()


def _frame(seed):
    imgs, pts, _ = synth.frame_inputs(2, 2, 32, 32, 200, 4, seed=seed)
    return imgs.cuda(), pts.cuda()


def test_detector_eval_seg_beside_unchanged_detection_outputs(gpu):
    m, plain = _detectors()
    m.eval(), plain.eval()
    imgs, pts = _frame(40)
    out, base = m(imgs, pts, None), plain(imgs, pts, None)
    assert set(out) == set(engine.HEAD_BRANCHES) | {"seg"} and set(base) == set(engine.HEAD_BRANCHES)
    for k in engine.HEAD_BRANCHES:
        assert torch.equal(out[k], base[k]), k                                         # bit-equal to the detector without the head
    fused = m.fusion(m.camera_encoder(imgs), m.lidar_encoder(pts), None)
    assert out["seg"].shape == (2, 3, 12, 12) and out["seg"].dtype == torch.float32
    assert torch.equal(out["seg"], m.seg_head(fused))
    assert float(out["seg"].std()) > 0


def _targets(gpu):
    boxes = [torch.tensor([[10.0, -8.0, 0.0, 4.0, 2.0, 1.5, 0.3], [-20.0, 15.0, 0.0, 5.0, 2.2, 1.6, -1.0]]),
             torch.tensor([[30.0, 30.0, 0.0, 3.0, 1.5, 1.5, 2.0]])]
    labels = [torch.tensor([1, 4]), torch.tensor([7])]
    tgt = ct.prepare_centernet_targets({"gt_boxes": boxes, "gt_labels": labels}, gpu, bev_size=(16, 16))
    masks = (synth.uniform((2, 3, 12, 12), 61) < 0.3).cuda()
    return tgt, masks


def test_detector_train_gradients_are_the_sum_of_the_two_tasks(gpu):
    """CenterNetLoss + SegFocalLoss backward through the detector = the detection loss alone (the detector WITHOUT the seg head:
    the unchanged single-consumer path) + the seg loss alone (the other head's output gradients zero), with the same batch
    statistics -- every pass starts from the same BatchNorm buffers."""
    m, plain = _detectors(seed=9)
    m.train(), plain.train()
    imgs, pts = _frame(41)
    tgt, masks = _targets(gpu)
    saved = {n: b.clone() for n, b in m.named_buffers()}

    def run(model, det, seg):
        for n, b in model.named_buffers():
            b.copy_(saved[n])
        model.zero_grad(set_to_none=True)
        out = model(imgs, pts, None)
        loss = 0.0
        if det:
            loss = loss + ct.CenterNetLoss()(out, tgt)["total_loss"]
        if seg:
            loss = loss + seg_head.SegFocalLoss()(out["seg"], masks)["loss"]
        loss.backward()
        return out, {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}

    out, both = run(m, True, True)
    assert set(out) == set(engine.HEAD_BRANCHES) | {"seg"} and out["seg"].requires_grad
    _, det_only = run(plain, True, False)
    _, seg_only = run(m, False, True)
    assert all(g is not None and torch.isfinite(g).all() for g in both.values())
    shared = [n for n in both if not n.startswith(("seg_head.", "det_head."))]
    assert len(shared) > 60 and any(n.startswith("fusion.") for n in shared) and any(n.startswith("camera_encoder.") for n in shared)
    assert all(float(seg_only[n].abs().sum()) > 0 for n in shared if n.endswith("conv1.weight"))     # the seg loss reaches the encoders
    _check_grads([(n, both[n]) for n in shared], [(n, det_only[n] + seg_only[n]) for n in shared], "detector, two consumers of fused")
    _check_grads([(n, g) for n, g in both.items() if n.startswith("seg_head.")],
                 [(n, g) for n, g in seg_only.items() if n.startswith("seg_head.")], "seg head inside the detector")
    _check_grads([(n, g) for n, g in both.items() if n.startswith("det_head.")],
                 [(n, g) for n, g in det_only.items() if n.startswith("det_head.")], "detection head inside the detector")


def test_detector_with_frustum_temporal_depth_supervision_and_seg_together(gpu):
    m = fusion.create_detector("camera+lidar", bev_h=16, bev_w=16, camera_view_transform="frustum", temporal=True, seg_head=SEG)
    m.fusion.set_camera_rig(CR.default_rig().subset(2))
    synth.fill_state_dict_(m, 11)
    m = m.cuda().train()
    imgs, pts, _ = synth.frame_inputs(2, 2, 64, 96, 300, 4, seed=42)
    imgs, pts = imgs.cuda(), pts.cuda()
    prev = synth.normal((2, m.fusion.bev_channels, 16, 16), 43).cuda()
    ego = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    ego[0, 0, 3], ego[1, 1, 3] = 3.0, -2.0
    out = m(imgs, pts, None, prev_bev=prev, ego_motion=ego, depth_points=pts)
    assert set(out) == set(engine.HEAD_BRANCHES) | {"seg", "bev", "depth_loss", "depth_pixels"}
    assert out["seg"].shape == (2, 3, 12, 12) and out["bev"].shape == prev.shape and out["depth_loss"].dim() == 0
    tgt, masks = _targets(gpu)
    loss = ct.CenterNetLoss()(out, tgt)["total_loss"] + seg_head.SegFocalLoss()(out["seg"], masks)["loss"] + 0.5 * out["depth_loss"]
    assert torch.isfinite(loss)
    loss.backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert float(m.seg_head.classifier[0].weight.grad.abs().sum()) > 0 and float(m.fusion.depth_net.weight.grad.abs().sum()) > 0


def test_graphed_detector_replays_seg_bit_equal_to_eager(gpu):
    m, _ = _detectors(seed=13)
    m.eval()
    frames = [_frame(44), _frame(45)]
    eager = [{k: v.clone() for k, v in m(i, p, None).items()} for i, p in frames]
    assert not torch.equal(eager[0]["seg"], eager[1]["seg"])
    g = m.make_graphed(frames[0][0], frames[0][1], None)
    for t, (i, p) in enumerate(frames):
        out = g(i, p, None)
        assert set(out) == set(eager[t])
        for k, v in eager[t].items():
            assert torch.equal(out[k], v), (t, k)
