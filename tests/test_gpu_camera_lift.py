"""The opt-in learned-depth camera -> BEV lift (camera_view_transform 'lift') on the MI355X against the fp64
grid_sample restatement of tests/camera_lift_ref.py (parity unpinned by the reference, which has no view transform): the lift gather
and its backward on the transposed table, the depth softmax, FlexibleBEVFusion in eval and train mode, a detector training step,
hipGraph replay, and the 'mean' / 'project' inference paths held bit for bit against their launches restated by hand.  The cases and
their margin condition (no sample near a bin edge or an image border, so nothing is excluded) are stated in camera_lift_ref.py and
checked on the CPU by tests/test_camera_lift_host.py."""
import functools

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct
from bevfusion_multimodal_3d_object_detection_amd import engine, fusion, synth, training
from oracle import ref_model
from tests import camera_lift_ref as LR
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
RANGE = LR.RANGE
MTOL = 1e-4                      # tests/test_gpu_camera_bev.py's module bound
KTOL = 2e-6                      # the bound the shared-table gather is held to there


def _table(n, Hc, Wc, h, w, D, dev):
    t = CR.build_lift_table(LR.kernel_rig(n), Hc, Wc, RANGE, h, w, LR.NUM_HEIGHTS, LR.MIN_DEPTH, D, *LR.DEPTH[D])
    d = lambda a: torch.from_numpy(a).to(dev)                              # noqa: E731
    return t, engine.CameraLiftTable(t.P, t.ncols, t.D, d(t.row_ptr), d(t.col2), d(t.w), d(t.t_row_ptr), d(t.t_cell), d(t.t_bin), d(t.t_w))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """fp64, computed once per case and shared by the forward and the backward test: inputs, output, autograd gradients."""
    n, Hc, Wc, h, w, C, D, B = case
    g = torch.Generator().manual_seed(sum(case))
    feats = torch.randn(B, n, C, Hc, Wc, generator=g, dtype=torch.float64, requires_grad=True)
    pd = torch.softmax(2 * torch.randn(B, n, D, Hc, Wc, generator=g, dtype=torch.float64), 2).requires_grad_()
    G = torch.randn(B, C, h, w, generator=g, dtype=torch.float64)
    out = LR.lift_ref(feats, pd, LR.kernel_rig(n), RANGE, h, w, LR.NUM_HEIGHTS, LR.MIN_DEPTH, (D,) + LR.DEPTH[D])
    (out * G).sum().backward()
    return feats.detach(), pd.detach(), G, out.detach(), feats.grad, pd.grad


def _nhwc(t, dev):
    """(B, n, K, Hc, Wc) fp64 -> fp32 [B][n*Hc*Wc][K] on the device."""
    B, _, K = t.shape[:3]
    return t.permute(0, 1, 3, 4, 2).reshape(B, -1, K).float().contiguous().to(dev)


def test_cases_cover_empty_cell_rows_and_empty_pixel_rows():
    cells = pixels = False
    for n, Hc, Wc, h, w, _, D, _ in LR.KERNEL_CASES:
        t = CR.build_lift_table(LR.kernel_rig(n), Hc, Wc, RANGE, h, w, LR.NUM_HEIGHTS, LR.MIN_DEPTH, D, *LR.DEPTH[D])
        cells |= bool((np.diff(t.row_ptr) == 0).any())
        pixels |= bool((np.diff(t.t_row_ptr) == 0).any())
    assert cells and pixels


@pytest.mark.parametrize("case", LR.KERNEL_CASES)
def test_lift_kernel_against_fp64(gpu, case):
    n, Hc, Wc, h, w, C, D, B = case
    t, tab = _table(n, Hc, Wc, h, w, D, gpu)
    feats, pd, _, want, _, _ = _reference(case)
    x, p = _nhwc(feats, gpu), _nhwc(pd, gpu)
    # strided slice: C columns at offset C of a 3C-wide map, the rest must stay untouched; empty rows come out as zeros
    y = torch.full((B, t.P, 3 * C), 7.0, device=gpu)
    L.csr_lift(tab.row_ptr, tab.col2, tab.w, t.P, t.ncols, D, x, t.ncols * C, C, p, t.ncols * D, y.view(-1)[C:], t.P * 3 * C, 3 * C, B, C)
    got = y[:, :, C:2 * C].cpu()
    err = rel_err(got.view(B, h, w, C).permute(0, 3, 1, 2), want)
    print(f"csr_lift {case}: nnz {t.nnz} rel err {err:.2e}")
    assert err <= KTOL
    assert (y[:, :, :C] == 7.0).all() and (y[:, :, 2 * C:] == 7.0).all()
    empty = torch.from_numpy(np.diff(t.row_ptr) == 0)
    assert (got[:, empty] == 0).all()
    y2 = torch.full_like(y, -3.0)
    L.csr_lift(tab.row_ptr, tab.col2, tab.w, t.P, t.ncols, D, x, t.ncols * C, C, p, t.ncols * D, y2.view(-1)[C:], t.P * 3 * C, 3 * C, B, C)
    assert torch.equal(y2[:, :, C:2 * C], y[:, :, C:2 * C])                 # two launches: identical bits


@pytest.mark.parametrize("n,Hc,Wc,h,w,C,B", [(2, 5, 7, 8, 10, 32, 1), (3, 6, 9, 16, 16, 40, 5)])
def test_one_bin_with_unit_probability_is_the_projection_gather_bit_for_bit(gpu, n, Hc, Wc, h, w, C, B):
    rig = LR.kernel_rig(n)
    p = CR.build_projection_table(rig, Hc, Wc, RANGE, h, w, LR.NUM_HEIGHTS, LR.MIN_DEPTH)
    t, tab = _table(n, Hc, Wc, h, w, 1, gpu)
    assert np.array_equal(t.col2, p.col) and np.array_equal(t.w.view(np.int32), p.w.view(np.int32))
    d = lambda a: torch.from_numpy(a).to(gpu)                              # noqa: E731
    x = torch.randn(B, t.ncols, C, generator=torch.Generator().manual_seed(B)).to(gpu)
    a, b = torch.full((B * t.P * C,), 5.0, device=gpu), torch.full((B * t.P * C,), -5.0, device=gpu)
    tab.lift(x, torch.ones(B * t.ncols, device=gpu), a, B, C)
    L.csr_gather(d(p.row_ptr), d(p.col), d(p.w), p.P, p.ncols, x, p.ncols * C, C, b, p.P * C, C, B, C)
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", LR.KERNEL_CASES)
def test_lift_backward_against_fp64_autograd(gpu, case):
    n, Hc, Wc, h, w, C, D, B = case
    t, tab = _table(n, Hc, Wc, h, w, D, gpu)
    feats, pd, G, _, dfeats, dpd_ref = _reference(case)
    x, p = _nhwc(feats, gpu), _nhwc(pd, gpu)
    dy = G.permute(0, 2, 3, 1).reshape(-1).float().contiguous().to(gpu)
    dx = torch.full((B * t.ncols * C,), float("nan"), device=gpu)          # every element must be written
    dpd = torch.full((B * t.ncols * D,), float("nan"), device=gpu)
    tab.lift_backward(x, p, dy, dx, dpd, B, C)
    got_dx, got_dpd = dx.view(B, t.ncols, C).cpu(), dpd.view(B, t.ncols, D).cpu()
    assert torch.isfinite(got_dx).all() and torch.isfinite(got_dpd).all()
    e1, e2 = rel_err(got_dx, _nhwc(dfeats, "cpu").double()), rel_err(got_dpd, _nhwc(dpd_ref, "cpu").double())
    print(f"csr_lift_bwd {case}: dx rel err {e1:.2e} dPd rel err {e2:.2e}")
    assert e1 <= KTOL and e2 <= KTOL
    # pixel rows without an entry, and bins without an entry, are exactly zero
    empty = torch.from_numpy(np.diff(t.t_row_ptr) == 0)
    assert (got_dx[:, empty] == 0).all() and (got_dpd[:, empty] == 0).all()
    has = torch.zeros(t.ncols, D, dtype=torch.bool)
    has[torch.from_numpy(t.col2 // D).long(), torch.from_numpy(t.col2 % D).long()] = True
    assert not has.all() and (got_dpd[:, ~has] == 0).all()
    dx2, dpd2 = torch.empty_like(dx), torch.empty_like(dpd)
    tab.lift_backward(x, p, dy, dx2, dpd2, B, C)
    assert torch.equal(dx, dx2) and torch.equal(dpd, dpd2)                  # two launches: identical bits


@pytest.mark.parametrize("D", [1, 4, 33, 64])
def test_depth_softmax_forward_and_backward_against_fp64(gpu, D):
    rows, Dp = 1031, engine.depth_net_width(D)
    g = torch.Generator().manual_seed(D)
    logits = 4 * torch.randn(rows, Dp, generator=g)
    logits[::7, :D] = 80.0 * torch.sign(torch.randn(rows, D, generator=g))[::7]          # +-80: exp overflows without the row maximum
    logits[3, :D], logits[4, :D] = 80.0, -80.0
    logits[:, D:] = float("nan")                                                        # the padding columns are never read
    G = torch.randn(rows, D, generator=g)
    ref = logits[:, :D].double().requires_grad_()
    want = torch.softmax(ref, -1)
    (want * G.double()).sum().backward()
    pd = torch.full((rows, D), float("nan"), device=gpu)
    L.softmax_rows(logits.to(gpu), Dp, pd, D, rows, D)
    assert torch.isfinite(pd).all()
    err = float((pd.cpu().double() - want.detach()).abs().max())
    dl = torch.full((rows, Dp), float("nan"), device=gpu)
    L.softmax_rows_bwd(pd, G.to(gpu), D, dl, Dp, Dp, rows, D)
    # the gradient of the kernel's own fp32 Pd differs from fp64's by Pd's rounding: compare against fp64 at the same bound
    gerr = rel_err(dl[:, :D].cpu(), ref.grad)
    print(f"softmax D={D}: Pd abs err {err:.2e}, gradient rel err {gerr:.2e}")
    assert err <= 1e-6 and gerr <= 2e-6
    assert (dl[:, D:] == 0).all()                                                       # padding columns of the logit gradient: zeros
    pd2, dl2 = torch.empty_like(pd), torch.empty_like(dl)
    L.softmax_rows(logits.to(gpu), Dp, pd2, D, rows, D)
    L.softmax_rows_bwd(pd, G.to(gpu), D, dl2, Dp, Dp, rows, D)
    assert torch.equal(pd, pd2) and torch.equal(dl, dl2)


# ---- FlexibleBEVFusion alone (the shapes of tests/test_gpu_camera_bev.py's project module tests) ---------------------------------

def _fusion_pair(modality, H, W, ncam, seed=5):
    m = modality.replace(" ", "")
    cam, lid, rad = "camera" in m, "lidar" in m, "radar" in m
    rig = CR.default_rig().subset(ncam)
    ora = LR.lifting(ref_model.BEVFusion(cam, lid, rad, bev_h=H, bev_w=W), rig, RANGE)
    synth.fill_state_dict_(ora, seed)
    fus = fusion.FlexibleBEVFusion(use_camera=cam, use_lidar=lid, use_radar=rad, bev_h=H, bev_w=W, pc_range=list(RANGE),
                                   camera_view_transform="lift")
    fus.set_camera_rig(rig)
    fus.load_state_dict(ora.state_dict())
    return ora.double(), fus.to("cuda")


def _features(B, ncam, Hc, Wc, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, ncam, 512, Hc, Wc, generator=g), torch.randn(B, 1024, generator=g)


def test_fusion_eval_against_fp64(gpu):
    ora, fus = _fusion_pair("camera+lidar", 20, 20, 3)
    ora.eval(), fus.eval()
    cam, lid = _features(2, 3, 6, 10)
    out = fus(cam.cuda(), lid.cuda())
    with torch.no_grad():
        want = ora(cam.double(), lid.double())
    err = rel_err(out.cpu(), want)
    print(f"fusion(lift) eval: rel err {err:.2e}")
    assert out.shape == (2, 256, 20, 20) and err <= MTOL
    with pytest.raises(L.BevfError, match="3 cameras"):
        fus(_features(1, 4, 6, 10)[0].cuda(), lid[:1].cuda())


def test_fusion_train_mode_returns_parameter_and_camera_gradients(gpu):
    ora, fus = _fusion_pair("camera+lidar", 20, 20, 3, seed=17)
    ora.train(), fus.train()
    cam, lid = _features(2, 3, 6, 10, seed=4)
    G = torch.randn(2, 256, 20, 20, generator=torch.Generator().manual_seed(8))
    cam_d, lid_d = cam.cuda().requires_grad_(), lid.cuda().requires_grad_()
    out = fus(cam_d, lid_d)
    (out * G.cuda()).sum().backward()
    cam_r, lid_r = cam.double().requires_grad_(), lid.double().requires_grad_()
    want = ora(cam_r, lid_r)
    (want * G.double()).sum().backward()
    assert rel_err(out.detach().cpu(), want.detach()) <= MTOL
    assert cam_d.grad is not None and cam_d.grad.shape == cam.shape
    e = rel_err(cam_d.grad.cpu(), cam_r.grad)
    print(f"fusion(lift) train: camera gradient rel err {e:.2e}")
    assert e <= 2e-3
    gref = dict(ora.named_parameters())
    gn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in ora.parameters())))
    seen = []
    for n, p in fus.named_parameters():          # (+ a floor of 2e-6 of the gradient norm, as tests/test_gpu_camera_bev.py has it)
        if not n.startswith(("camera_proj.", "depth_net.")):
            continue
        r = gref[n].grad
        d = float((p.grad.cpu().double() - r).abs().max())
        print(f"  {n}: err {d:.2e} of max {float(r.abs().max()):.2e}")
        assert d <= 2e-3 * float(r.abs().max()) + 2e-6 * gn, n
        seen.append(n)
    assert "depth_net.weight" in seen and "depth_net.bias" in seen
    assert float(fus.depth_net.weight.grad.abs().sum()) > 0
    r = gref["depth_net.weight"].grad
    assert float((fus.depth_net.weight.grad.cpu().double() - r).abs().max()) <= 2e-3 * float(r.abs().max())     # without the floor


# ---- the detector (detector_cam_s16x24's sizes: 2 frames of 2 cameras 96 x 64, BEV 16 x 24) -----------------------------------------

def _detector(kind, seed=31):
    model = fusion.create_detector("camera+lidar", "bev", "centernet", bev_h=16, bev_w=24, camera_view_transform=kind)
    if kind != "mean":
        model.fusion.set_camera_rig(CR.default_rig().subset(2))
    synth.fill_state_dict_(model, seed)
    return model.to("cuda")


def _inputs(seed=103):
    imgs, pts, _ = synth.frame_inputs(2, 2, 96, 64, 300, 4, seed=seed)
    return imgs.cuda(), pts.cuda()


def test_detector_training_step(gpu):
    from tests.golden import cases
    model = _detector("lift").train()
    imgs, pts = _inputs()
    boxes, labels = cases.target_inputs(cases.TRAIN_CASE)
    tgt = ct.prepare_centernet_targets({"gt_boxes": boxes, "gt_labels": labels}, gpu, bev_size=(16, 24))
    state = {k: v.clone() for k, v in model.state_dict().items()}

    def step():
        opt = training.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        loss = ct.CenterNetLoss()(model(imgs, pts, None), tgt)["total_loss"]
        opt.zero_grad()
        loss.backward()
        training.clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        return loss.detach().clone()

    first = step()
    assert torch.isfinite(first)
    for k in ("fusion.depth_net.weight", "fusion.depth_net.bias"):
        assert not torch.equal(model.state_dict()[k], state[k]), k
    assert float(model.fusion.depth_net.weight.grad.abs().sum()) > 0 and float(model.camera_encoder.conv1.weight.grad.abs().sum()) > 0
    model.load_state_dict(state)
    assert torch.equal(step(), first)                                      # the same step from the same state: the same loss bits


def test_graphed_lift_detector_replays_bit_identically(gpu):
    model = _detector("lift").eval()
    a, b = _inputs(41), _inputs(42)
    g = model.make_graphed(*a)
    for inp in (b, a):
        got = {k: v.clone() for k, v in g(*inp).items()}
        eager = model(*inp)
        for k in eager:
            assert torch.equal(got[k], eager[k]), k
    assert float((model(*a)["heatmap"] - model(*b)["heatmap"]).abs().max()) > 0


@pytest.mark.parametrize("kind", ["mean", "project"])
def test_mean_and_project_inference_run_their_own_launches_unchanged(gpu, kind):
    """The detector's eval forward against the branch's launches restated here by hand from the entry points the existing tests
    pin (camera mean / projection gather, exact convolutions, bilinear resize): bit for bit, and no lift state on the model."""
    model = _detector(kind).eval()
    imgs, pts = _inputs(44)
    out = {k: v.clone() for k, v in model(imgs, pts, None).items()}         # (the outputs live in the head engine's workspace)
    fus, eng = model.fusion, model.fusion._eng()
    assert not hasattr(fus, "depth_net") and not any(k.startswith("lift") for k in eng._bufs)
    assert type(eng.branches[0]) is {"mean": engine.CameraMeanBranch, "project": engine.CameraProjectBranch}[kind]
    with torch.no_grad():
        cam, (B, ncam, Hc, Wc) = model.camera_encoder.forward_nhwc(imgs)
        lid = model.lidar_encoder._forward_eval(pts)
        Sh, Sw, bc, Cc = 16, 24, fus.bev_channels, 512
        new = lambda n: torch.empty(n, device=gpu)                         # noqa: E731
        concat = new(B * Sh * Sw * 2 * bc)
        c1 = engine.pack_conv(fus.camera_proj[0], fus.camera_proj[1], True)
        c2 = engine.pack_conv(fus.camera_proj[3], fus.camera_proj[4], True)
        if kind == "mean":
            pooled = new(B * Hc * Wc * Cc)
            L.cam_mean(cam, pooled, B, ncam, Hc * Wc, Cc)
            t1, t2 = new(B * Hc * Wc * c1.cout), new(B * Hc * Wc * bc)
            engine._run_conv(c1, pooled, t1, B, Hc, Wc)
            engine._run_conv(c2, t1, t2, B, Hc, Wc)
            L.bilinear_nhwc(t2, concat, B, Hc, Wc, bc, bc, Sh, Sw, 2 * bc)
        else:
            tab = engine.camera_table(fus, ncam, Hc, Wc, cam.device)
            proj, t1 = new(B * Sh * Sw * Cc), new(B * Sh * Sw * c1.cout)
            tab.project(cam, proj, B, Cc)
            engine._run_conv(c1, proj, t1, B, Sh, Sw)
            engine._run_conv(c2, t1, concat, B, Sh, Sw, y_cs=2 * bc)
        lidar_branch = engine.LidarVectorBranch(eng)
        lidar_branch.pack(fus)
        lidar_branch.run(lid.float(), B, concat[bc:], 2 * bc)
        f1 = engine.pack_conv(fus.bev_fusion[0], fus.bev_fusion[1], True)
        f2 = engine.pack_conv(fus.bev_fusion[3], fus.bev_fusion[4], True)
        a1, fused = new(B * Sh * Sw * f1.cout), new(B * Sh * Sw * f2.cout)
        engine._run_conv(f1, concat, a1, B, Sh, Sw)
        engine._run_conv(f2, a1, fused, B, Sh, Sw)
        want = model.det_head.forward_nhwc(fused, B, Sh, Sw)
    for k in want:
        assert torch.equal(out[k], want[k]), k
