"""LiDAR depth supervision of the 'frustum' and 'lift' camera branches (depth_supervision.py, csrc/depth_sup.hip) on
the MI355X: the device targets against the point-by-point restatement of tests/depth_sup_ref.py integer for integer, the cross
entropy and its gradient against fp64, one training step of the detector with CenterNetLoss + 0.5 * depth_loss against the oracle's
fp64 autograd ('frustum' with per-frame calibration, 'lift' with the static rig), an augmented batch, and a hipGraph replay.  Parity
unpinned by the reference, which has no view transform.  The cases and their margin condition (no point within 1e-9 of a pixel, bin
or range edge, so nothing is excluded) are stated in depth_sup_ref.py and checked on the CPU by tests/test_depth_sup_host.py."""
import functools

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct
from bevfusion_multimodal_3d_object_detection_amd import depth_supervision as DS
from bevfusion_multimodal_3d_object_detection_amd import engine, fusion, synth, training
from oracle import ref_model
from tests import augment_ref
from tests import camera_frustum_ref as FR
from tests import camera_lift_ref as LR
from tests import depth_sup_ref as DR
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
RANGE = FR.RANGE
KTOL = 2e-6                      # the bound tests/test_gpu_camera_lift.py holds softmax_rows' gradient to
GTOL = 2e-3                      # tests/test_gpu_camera_frustum.py's gradient bound (+ a floor of 2e-6 of the gradient norm)
NAN = float("nan")


# ---- the targets ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    """Computed once per case: (points, counts, rigs, the restatement's targets)."""
    pts, counts, rigs = DR.case_points(name)
    _, _, Hc, Wc, depth, _, _ = DR.CASES[name]
    return pts, counts, rigs, DR.targets_ref(pts, rigs, Hc, Wc, depth, counts)


def _build(pts, counts, calib, image_size, Hc, Wc, depth, poison):
    """bevf_depth_targets_f64 into a buffer pre-filled with `poison`."""
    target = torch.full((pts.shape[0], calib.shape[1], Hc, Wc), poison, dtype=torch.int32, device="cuda")
    DS.build_targets(pts, counts, calib, image_size, Hc, Wc, depth, target=target)
    return target


def _dev(pts, counts):
    return torch.from_numpy(pts).cuda(), None if counts is None else torch.from_numpy(counts).cuda()


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_device_targets_equal_the_restatement(gpu, name):
    pts, counts, rigs, want = _case(name)
    _, _, Hc, Wc, depth, N, _ = DR.CASES[name]
    p, c = _dev(pts, counts)
    calib = torch.from_numpy(CR.calib_matrices(rigs)).cuda()
    got = _build(p, c, calib, rigs[0].image_size, Hc, Wc, depth, poison=-7)
    assert np.array_equal(got.cpu().numpy(), want)                                 # integer for integer, nothing excluded
    assert (want >= 0).mean() >= 1 / 3
    again = _build(p, c, calib, rigs[0].image_size, Hc, Wc, depth, poison=12345)   # a second build: the same bits
    assert torch.equal(got, again)
    # the public function, in each calibration form it accepts
    for form in (rigs, torch.from_numpy(CR.calib_matrices(rigs)), calib):
        assert torch.equal(DS.depth_targets(p, form, rigs[0].image_size, Hc, Wc, depth, counts=c), got)
    if c is not None:
        assert torch.equal(DS.depth_targets(p, rigs, rigs[0].image_size, Hc, Wc, depth, counts=c.long()), got)
        assert not torch.equal(DS.depth_targets(p, rigs, rigs[0].image_size, Hc, Wc, depth), got)       # the counts count
    # wider rows inside a larger buffer: the point strides
    big = torch.full((pts.shape[0], N + 9, 6), 3.0, device=gpu)
    big[:, :N, :4] = p
    assert torch.equal(DS.depth_targets(big[:, :N], rigs, rigs[0].image_size, Hc, Wc, depth, counts=c), got)


def test_no_points_and_zero_counts_give_no_targets(gpu):
    pts, _, rigs, want = _case("1")
    _, ncam, Hc, Wc, depth, N, _ = DR.CASES["1"]
    calib = torch.from_numpy(CR.calib_matrices(rigs)).cuda()
    empty = _build(torch.zeros(2, 0, 4, device=gpu), None, calib, rigs[0].image_size, Hc, Wc, depth, poison=9)
    assert empty.shape == (2, ncam, Hc, Wc) and (empty == -1).all()
    zero = torch.zeros(2, dtype=torch.int32, device=gpu)
    assert (_build(torch.from_numpy(pts).cuda(), zero, calib, rigs[0].image_size, Hc, Wc, depth, poison=9) == -1).all()
    assert (_build(torch.zeros(2, N, 4, device=gpu), None, calib, rigs[0].image_size, Hc, Wc, depth, poison=9) == -1).all()   # padding only
    assert (want >= 0).any()


def test_shared_calibration_equals_the_same_calibration_per_frame(gpu):
    pts, _, rigs, _ = _case("1")
    _, _, Hc, Wc, depth, _, _ = DR.CASES["1"]
    p = torch.from_numpy(pts).cuda()
    one = torch.from_numpy(CR.calib_matrices(rigs[:1])).cuda()
    shared = _build(p, None, one, rigs[0].image_size, Hc, Wc, depth, poison=-3)                      # stride 0
    rep = _build(p, None, one.expand(2, -1, -1, -1).contiguous(), rigs[0].image_size, Hc, Wc, depth, poison=-5)
    assert torch.equal(shared, rep)
    assert np.array_equal(shared.cpu().numpy(), DR.targets_ref(pts, [rigs[0]] * 2, Hc, Wc, depth))
    assert torch.equal(DS.depth_targets(p, rigs[0], rigs[0].image_size, Hc, Wc, depth), shared)      # one CameraRig: every frame


def test_frustum_points_get_their_own_bin_on_the_device(gpu):
    """The inverse of 3.2d3's geometry on the device: frame d holds the frustum points of bin d of a one-camera rig, rounded to
    float32 (pixel and bin centres: half a pixel / half a bin from every edge) -- every pixel of frame d gets target d."""
    Hc, Wc, depth = 5, 7, (8, 1.0, 65.0)
    rig = FR.case_rig(1, 1)
    calib = CR.calib_matrices([rig])
    fp = CR.frustum_points(calib, rig.image_size, Hc, Wc, *depth)[0].reshape(Hc * Wc, depth[0], 3)
    p = torch.from_numpy(np.ascontiguousarray(fp.transpose(1, 0, 2)).astype(np.float32)).cuda()       # (D frames, Hc * Wc, 3)
    got = DS.depth_targets(p, torch.from_numpy(calib), rig.image_size, Hc, Wc, depth)
    want = torch.arange(depth[0], dtype=torch.int32, device=gpu).view(-1, 1, 1, 1).expand(-1, 1, Hc, Wc)
    assert torch.equal(got, want)


# ---- the cross entropy ---------------------------------------------------------------------------------------------------------------

GUP = 0.7                        # the gradient arriving at the loss


@functools.lru_cache(maxsize=None)
def _ce_reference(D, supervised=True, rows=DR.CE_ROWS):
    """Computed once per case: logits 4 * randn at depth_net_width(D) with NaN in the padding columns, about half of the targets -1
    (all of them with supervised = False), the fp64 loss / count / logit gradient of depth_sup_ref.ce_ref."""
    Dp = engine.depth_net_width(D)
    g = torch.Generator().manual_seed(100 + D)
    logits = 4 * torch.randn(rows, Dp, generator=g)
    logits[:, D:] = NAN
    target = torch.randint(0, D, (rows,), generator=g).int()
    target[torch.rand(rows, generator=g) < 0.5] = -1
    if not supervised:
        target[:] = -1
    ref = logits[:, :D].double().requires_grad_()
    loss, count = DR.ce_ref(ref, target)
    (GUP * loss).backward()
    return dict(logits=logits, target=target, loss=float(loss.detach()), count=count, grad=ref.grad)


def _device_ce(ref, D, prefill):
    """depth_ce and depth_ce_bwd through the _lib wrappers: out (poisoned first) and dlogit, which starts as `prefill`."""
    rows, Dp = ref["logits"].shape
    lg, tg = ref["logits"].cuda(), ref["target"].cuda()
    out = torch.full((2,), NAN, device="cuda")
    partials = torch.full((L.depth_ce_work_doubles(),), NAN, dtype=torch.float64, device="cuda")
    L.depth_ce(lg, Dp, tg, rows, D, partials, out)
    pd = torch.empty(rows, D, device="cuda")
    L.softmax_rows(lg, Dp, pd, D, rows, D)
    dl = prefill.cuda().clone()
    L.depth_ce_bwd(pd, D, tg, torch.tensor([GUP], device="cuda"), out, dl, Dp, rows, D)
    return out, dl


def _rows_past_one_pass(D):
    """More rows than one pass of the CE forward's workgroups holds (each takes 256 / (lanes per row) rows at a time and there are
    at most depth_ce_work_doubles() / 2 of them): some workgroups walk a second chunk, the last chunk is partly filled."""
    lanes = 1 << (D - 1).bit_length()
    return (256 // lanes) * (L.depth_ce_work_doubles() // 2 + 37) + 3


@pytest.mark.parametrize("D,rows", [(D, DR.CE_ROWS) for D in DR.CE_BINS] + [(64, None)])
def test_cross_entropy_forward_and_backward_against_fp64(gpu, D, rows):
    ref = _ce_reference(D, rows=rows or _rows_past_one_pass(D))
    rows, Dp = ref["logits"].shape
    sup = ref["target"] >= 0
    assert 0.35 < float(sup.float().mean()) < 0.65
    g = torch.Generator().manual_seed(D)
    junk = torch.randn(rows, Dp, generator=g)
    clean = junk.clone()
    clean[sup, :D] = 0.0                                            # zeros where the kernel adds: its own rounding only
    out, dl = _device_ce(ref, D, clean)
    assert float(out[1]) == ref["count"] == int(sup.sum())
    got = dl.cpu()
    if D == 1:                                                      # one bin: the loss and its gradient are 0
        assert float(out[0]) == 0.0 and ref["loss"] == 0.0 and (got[sup, :1] == 0).all() and (ref["grad"] == 0).all()
    else:
        lerr = abs(float(out[0]) - ref["loss"]) / abs(ref["loss"])
        gerr = rel_err(got[sup, :D], ref["grad"][sup])
        print(f"depth_ce D={D} rows={rows}: loss {float(out[0]):.6f}, rel err {lerr:.2e}; logit gradient rel err {gerr:.2e}")
        assert lerr <= KTOL and gerr <= KTOL
    # the padding columns and the rows without a target keep the values they had, bit for bit
    assert torch.equal(got[:, D:], clean[:, D:]) and torch.equal(got[~sup], clean[~sup])
    # += on values that were there: the sum rounded once (fp32: 2^-24 relative, of at most |junk| + |gradient|)
    out2, dl2 = _device_ce(ref, D, junk)
    added = dl2.cpu()
    assert torch.equal(added[:, D:], junk[:, D:]) and torch.equal(added[~sup], junk[~sup])
    bound = 2.0 ** -23 * float((junk[sup, :D].abs() + got[sup, :D].abs()).max())
    assert float((added[sup, :D].double() - (junk[sup, :D].double() + got[sup, :D].double())).abs().max()) <= bound
    # a relaunch: identical bits
    out3, dl3 = _device_ce(ref, D, clean)
    assert torch.equal(out, out2) and torch.equal(out, out3) and torch.equal(dl, dl3)


@pytest.mark.parametrize("D", [5, 64])
def test_cross_entropy_without_any_target_is_exactly_zero(gpu, D):
    ref = _ce_reference(D, supervised=False)
    rows, Dp = ref["logits"].shape
    junk = torch.randn(rows, Dp, generator=torch.Generator().manual_seed(D))
    out, dl = _device_ce(ref, D, junk)
    assert ref["loss"] == 0.0 and ref["count"] == 0
    assert float(out[0]) == 0.0 and float(out[1]) == 0.0 and torch.isfinite(out).all()
    assert torch.equal(dl.cpu(), junk)                                             # dlogit unchanged, nothing NaN


@pytest.mark.parametrize("D", [5, 64])
def test_depth_cross_entropy_function_rows_and_nchw(gpu, D):
    """The autograd Function: padded rows with depth_bins, and the same logits as an NCHW map."""
    ref = _ce_reference(D)
    lg = ref["logits"].cuda().requires_grad_()
    loss, count = DS.depth_cross_entropy(lg, ref["target"].cuda(), depth_bins=D)
    assert loss.dim() == 0 and count.dim() == 0 and not count.requires_grad and float(count) == ref["count"]
    (GUP * loss).backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= KTOL * abs(ref["loss"])
    assert rel_err(lg.grad[:, :D].cpu(), ref["grad"]) <= KTOL and (lg.grad[:, D:] == 0).all()      # (rows without a target: zeros in both)
    n, Hc, Wc = 3, 7, 11                                                           # 3 * 7 * 11 = 231 of the rows as a map
    rows = n * Hc * Wc
    nchw = ref["logits"][:rows, :D].reshape(n, Hc, Wc, D).permute(0, 3, 1, 2).contiguous().cuda().requires_grad_()
    tg = ref["target"][:rows].reshape(n, Hc, Wc).cuda()
    l4, c4 = DS.depth_cross_entropy(nchw, tg)
    flat = ref["logits"][:rows, :D].contiguous().cuda().requires_grad_()
    l2, c2 = DS.depth_cross_entropy(flat, tg.reshape(-1))
    assert torch.equal(l4, l2) and torch.equal(c4, c2)
    l4.backward(), l2.backward()
    assert torch.equal(nchw.grad.permute(0, 2, 3, 1).reshape(rows, D), flat.grad)
    want, _ = DR.ce_ref(ref["logits"][:rows, :D].double(), ref["target"][:rows])
    assert abs(float(l4.detach()) - float(want)) <= KTOL * abs(float(want))


# ---- the detector (tests/test_gpu_camera_frustum.py's: 2 frames of 2 cameras 64 x 96, BEV 50 x 50) ----------------------------------

def _frustum_pair(rigs, seed=77):
    from tests.test_gpu_camera_frustum import _det_pair
    return _det_pair("camera+lidar", rigs, seed=seed)


def _lift_pair(rig, seed=77):
    n, _, _, h, w, depth = FR.DETECTOR_CASE
    ora = ref_model.make_detector("camera+lidar", h, w)
    LR.lifting(ora.fusion, rig, RANGE, depth)
    synth.fill_state_dict_(ora, seed)
    model = fusion.create_detector("camera+lidar", "bev", "centernet", bev_h=h, bev_w=w, camera_view_transform="lift")
    model.fusion.set_camera_rig(rig)
    model.load_state_dict(ora.state_dict())
    return ora, model.to("cuda")


def _oracle_step(ora, imgs, pts, boxes, labels, rigs, trace, weight, head):
    """The oracle's fp64 step with the device's ReLU decisions replayed: depth_net's logits come from a forward hook, the targets
    from the restatement.  -> (head loss, depth loss, supervised pixels); the gradients are in ora's parameters."""
    from oracle import ref_targets
    from tests.test_gpu_training import _ReluReplay
    _, Hc, Wc, _, _, depth = FR.DETECTOR_CASE
    ora = ora.double()
    logits = []
    hook = ora.fusion.depth_net.register_forward_hook(lambda m, i, o: logits.append(o))
    tgt = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in ref_targets.make_targets(boxes, labels).items()}
    try:
        with _ReluReplay(trace) as rp:
            head_loss = ref_targets.centernet_loss(ora(imgs.double(), pts.double(), None), tgt)["total_loss"]
    finally:
        hook.remove()
    assert not rp.misses and rp.hits >= 10, (rp.hits, rp.misses[:5])
    assert len(logits) == 1
    depth_loss, pixels = DR.ce_ref(DR.logit_rows(logits[0]), DR.targets_ref(pts.numpy(), rigs, Hc, Wc, depth))
    (head_loss + weight * depth_loss if head else depth_loss).backward()
    return float(head_loss.detach()), float(depth_loss.detach()), pixels


def _device_step(model, imgs, pts, boxes, labels, gpu, weight, head, **kw):
    """-> (the detector's output, the ReLU trace of its forward); the gradients are in model's parameters."""
    trace, saved = [], training.FUSE_POOL_BN_BACKWARD
    training.RELU_TRACE, training.FUSE_POOL_BN_BACKWARD = trace, False
    try:
        pred = model(imgs.cuda(), pts.cuda(), None, **kw)
    finally:
        training.RELU_TRACE, training.FUSE_POOL_BN_BACKWARD = None, saved
    tgt = ct.prepare_centernet_targets({"gt_boxes": boxes, "gt_labels": labels}, gpu)
    head_loss = ct.CenterNetLoss()(pred, tgt)["total_loss"]
    (head_loss + weight * pred["depth_loss"] if head else pred["depth_loss"]).backward()
    return pred, trace, float(head_loss.detach())


def _compare_gradients(model, ora, what):
    gref = dict(ora.named_parameters())
    gn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in ora.parameters() if p.grad is not None)))
    bad, checked, zero = [], 0, 0
    for name, p in model.named_parameters():
        r = gref[name].grad
        if r is None:                                                # not on the loss's path: zeros or None, as autograd defines
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            zero += 1
            continue
        assert p.grad is not None, name
        checked += 1
        err = float((p.grad.cpu().double() - r).abs().max())
        if err > GTOL * float(r.abs().max()) + 2e-6 * gn:
            bad.append((name, err, float(r.abs().max())))
    print(f"{what}: {checked} gradients within {GTOL:g} of the tensor's maximum + 2e-6 of the norm {gn:.3e}; {zero} off the path")
    assert not bad, bad[:5]
    return checked, zero


def _train_inputs(rigs):
    from tests.golden import cases
    imgs, _, _ = synth.frame_inputs(2, 2, 64, 96, 0, 4, 0, 20, 7, seed=123)
    pts = torch.from_numpy(DR.detector_points(rigs))
    boxes, labels = cases.target_inputs(cases.TRAIN_CASE)
    return imgs, pts, boxes, labels


@pytest.mark.parametrize("kind", ["frustum", "lift"])
def test_detector_step_with_depth_loss_against_fp64_autograd(gpu, kind):
    """One training step with the loss CenterNetLoss total + 0.5 * depth_loss: 'frustum' with per-frame calibration, 'lift' with the
    static rig.  Every parameter gradient against the oracle's fp64 autograd, depth_loss to 1e-5, depth_pixels equal."""
    if kind == "frustum":
        rigs = [FR.case_rig(FR.DETECTOR_CASE[0], b) for b in range(2)]
        ora, model = _frustum_pair(rigs)
        kw = dict(camera_calib=torch.from_numpy(CR.calib_matrices(rigs)).cuda())
    else:
        rigs = [FR.case_rig(FR.DETECTOR_CASE[0], 0)] * 2
        ora, model = _lift_pair(rigs[0])
        kw = {}
    ora.train(), model.train()
    imgs, pts, boxes, labels = _train_inputs(rigs)
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    try:
        pred, trace, head_loss = _device_step(model, imgs, pts, boxes, labels, gpu, 0.5, True, depth_points=pts.cuda(), **kw)
    finally:
        engine.set_conv_mode(old)
    assert set(pred) == set(engine.HEAD_BRANCHES) | {"depth_loss", "depth_pixels"}
    assert pred["depth_loss"].dim() == 0 and pred["depth_pixels"].dim() == 0 and not pred["depth_pixels"].requires_grad
    head_ref, depth_ref, pixels = _oracle_step(ora, imgs, pts, boxes, labels, rigs, trace, 0.5, True)
    dloss = float(pred["depth_loss"].detach())
    derr = abs(dloss - depth_ref) / abs(depth_ref)
    print(f"detector({kind}) depth_loss {dloss:.6f} (oracle {depth_ref:.6f}, rel err {derr:.2e}), "
          f"{int(pred['depth_pixels'])} supervised pixels")
    assert derr <= 1e-5 and int(pred["depth_pixels"]) == pixels and pixels >= 16
    assert abs(head_loss - head_ref) <= 1e-5 * abs(head_ref)
    checked, zero = _compare_gradients(model, ora, f"detector({kind}), head + 0.5 depth")
    assert checked >= 100 and zero == 0
    for p in (model.fusion.depth_net.weight, model.fusion.depth_net.bias, model.camera_encoder.conv1.weight):
        assert float(p.grad.abs().sum()) > 0


def test_detector_backward_of_the_depth_loss_alone_and_of_the_head_loss_alone(gpu):
    """depth_loss alone: depth_net and the camera encoder get the oracle's gradients, everything behind the pool zeros or None.  The
    head loss alone, with depth_points given: the gradients of the run without the argument.  Without depth_points the five outputs
    are bit for bit those of the run with it, and there is no sixth."""
    rigs = [FR.case_rig(FR.DETECTOR_CASE[0], b) for b in range(2)]
    ora, model = _frustum_pair(rigs)
    ora.train(), model.train()
    imgs, pts, boxes, labels = _train_inputs(rigs)
    calib = torch.from_numpy(CR.calib_matrices(rigs)).cuda()
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    try:
        pred, trace, _ = _device_step(model, imgs, pts, boxes, labels, gpu, 1.0, False, depth_points=pts.cuda(), camera_calib=calib)
        _oracle_step(ora, imgs, pts, boxes, labels, rigs, trace, 1.0, False)
        checked, zero = _compare_gradients(model, ora, "detector(frustum), depth loss alone")
        assert checked >= 40 and zero >= 20
        names = [n for n, p in ora.named_parameters() if p.grad is not None]
        assert "fusion.depth_net.weight" in names and "camera_encoder.conv1.weight" in names
        assert not any(n.startswith(("det_head.", "fusion.bev_fusion.", "fusion.camera_proj.", "lidar_encoder.")) for n in names)
        assert float(model.fusion.depth_net.weight.grad.abs().sum()) > 0 and float(model.camera_encoder.conv1.weight.grad.abs().sum()) > 0
        # the plain call, as before the argument existed
        model.zero_grad(set_to_none=True)
        tgt = ct.prepare_centernet_targets({"gt_boxes": boxes, "gt_labels": labels}, gpu)
        plain = model(imgs.cuda(), pts.cuda(), None, camera_calib=calib)
        assert tuple(plain) == engine.HEAD_BRANCHES
        for k in engine.HEAD_BRANCHES:
            assert torch.equal(plain[k], pred[k]), k
        ct.CenterNetLoss()(plain, tgt)["total_loss"].backward()
        want = {n: p.grad.clone() for n, p in model.named_parameters()}
        # the head loss alone through a step that was given depth_points: the unused sixth gradient arrives as zeros
        model.zero_grad(set_to_none=True)
        with_depth = model(imgs.cuda(), pts.cuda(), None, camera_calib=calib, depth_points=pts.cuda())
        ct.CenterNetLoss()(with_depth, tgt)["total_loss"].backward()
    finally:
        engine.set_conv_mode(old)
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in want.values())))
    for n, p in model.named_parameters():                           # both runs are within GTOL of the same fp64 gradient
        err = float((p.grad - want[n]).abs().max())
        assert err <= 2 * (GTOL * float(want[n].abs().max()) + 2e-6 * gn), (n, err)


def test_augmented_batch_depth_loss_matches_the_oracle(gpu):
    """augment_batch's points, counts, images and camera_calib through the 'frustum' detector in train mode: the depth loss against
    the oracle's, whose targets come from the rigs that see the augmented frames (K' = A . K, cam_to_bev' = T . cam_to_bev)."""
    n, Hc, Wc, _, _, depth = FR.DETECTOR_CASE
    st = A.AugmentSettings(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, camera_flip=True, camera_scale=(0.9, 1.1), flip=True,
                           scale=(0.95, 1.05), rotation=(-20.0, 20.0), translation=(0.5, 0.5, 0.2))
    p = augment_ref.calib_params(2, n, (120, 200), (64, 96), 5)
    p.jitter = A.sample(st, 2, n, (120, 200), (64, 96), np.random.default_rng(5)).jitter
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (2, n, 120, 200, 3), dtype=np.uint8)).cuda()
    base = FR.case_rig(n, 0)
    raw, _ = DR.points_in_view([base, base], Hc, Wc, depth, 1000, seed=9)
    o = A.augment_batch(frames, torch.from_numpy(raw).cuda(), None, None, None, None, None, p, st, base_calib=base, max_points=1024)
    rigs = FR.augmented_rigs(base, p)
    pts, counts = o["lidar_points"].cpu(), o["lidar_count"].cpu().numpy()
    assert DR.margin(pts.numpy(), rigs, Hc, Wc, depth, counts) > DR.MARGIN
    want_t = DR.targets_ref(pts.numpy(), rigs, Hc, Wc, depth, counts)
    assert (want_t >= 0).mean() >= 1 / 3
    got_t = DS.depth_targets(o["lidar_points"], o["camera_calib"], base.image_size, Hc, Wc, depth, counts=o["lidar_count"])
    assert np.array_equal(got_t.cpu().numpy(), want_t)
    ora, model = _frustum_pair(rigs)
    model.fusion.set_camera_rig(base)
    ora, _ = ora.double().train(), model.train()
    out = model(o["camera_imgs"], o["lidar_points"], None, camera_calib=o["camera_calib"], depth_points=o["lidar_points"],
                depth_point_counts=o["lidar_count"])
    logits = []
    hook = ora.fusion.depth_net.register_forward_hook(lambda m, i, x: logits.append(x))
    with torch.no_grad():
        ora(o["camera_imgs"].cpu().double(), pts.double(), None)
    hook.remove()
    want, pixels = DR.ce_ref(DR.logit_rows(logits[0]), want_t)
    got = float(out["depth_loss"].detach())
    err = abs(got - float(want)) / abs(float(want))
    print(f"detector(frustum) on an augmented batch: depth_loss {got:.6f}, rel err {err:.2e}, {pixels} pixels")
    assert err <= 1e-5 and int(out["depth_pixels"]) == pixels


# ---- graph capture -------------------------------------------------------------------------------------------------------------------

def test_targets_and_cross_entropy_replay_in_a_graph(gpu):
    """depth_targets, the CE forward and the CE backward recorded on one stream (no parallel branches) and replayed after new points,
    calibration and logits were copied into the static inputs: the eager result, bit for bit."""
    _, ncam, Hc, Wc, depth, N, _ = DR.CASES["1"]
    D, Dp = depth[0], engine.depth_net_width(depth[0])
    rows = 2 * ncam * Hc * Wc

    def inputs(seed):
        rigs = DR.case_rigs("1", first=seed)
        pts, _ = DR.points_in_view(rigs, Hc, Wc, depth, N, seed=200 + seed)
        logits = 4 * torch.randn(rows, Dp, generator=torch.Generator().manual_seed(seed))
        return torch.from_numpy(pts).cuda(), torch.from_numpy(CR.calib_matrices(rigs)).cuda(), logits.cuda(), rigs[0].image_size

    def run(p, calib, logits, size, bufs):
        target, partials, out, pd, dl, g = bufs
        DS.build_targets(p, None, calib, size, Hc, Wc, depth, target=target)
        L.depth_ce(logits, Dp, target.view(-1), rows, D, partials, out)
        L.softmax_rows(logits, Dp, pd, D, rows, D)
        dl.zero_()
        L.depth_ce_bwd(pd, D, target.view(-1), g, out, dl, Dp, rows, D)

    def buffers():
        return (torch.full((2, ncam, Hc, Wc), -9, dtype=torch.int32, device=gpu),
                torch.empty(L.depth_ce_work_doubles(), dtype=torch.float64, device=gpu), torch.full((2,), NAN, device=gpu),
                torch.empty(rows, D, device=gpu), torch.full((rows, Dp), NAN, device=gpu), torch.tensor([GUP], device=gpu))

    a, b = inputs(0), inputs(3)
    static, sb = [t.clone() for t in a[:3]], buffers()
    run(*static, a[3], sb)                                           # once eagerly before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(*static, a[3], sb)
    for inp in (b, a):
        for s, t in zip(static, inp[:3]):
            s.copy_(t)
        graph.replay()
        eb = buffers()
        run(*inp, eb)
        torch.cuda.synchronize()
        assert torch.equal(sb[0], eb[0]) and torch.equal(sb[2], eb[2]) and torch.equal(sb[4], eb[4])
        assert (eb[0] >= 0).any() and float(eb[2][1]) > 0
    ta = sb[0].clone()
    static[0].copy_(b[0]), static[1].copy_(b[1]), static[2].copy_(b[2])
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(sb[0], ta)                                # the new points and calibration reach the replay
