"""IoU-aware head on the GPU: the IoU targets, the IoU / DIoU loss and its gradients, and the rectified decode
against the fp64 restatement of tests/iou_aware_ref.py; the head module in eval (fp32, bf16) and train mode against the fp64
composition; the detector with the head -- eager, trained, beside the seg head, and as a replayed graph.

Bounds.  iou_targets: 2e-4 absolute, twice IOU_TOL of tests/test_gpu_box_nms.py because t = 2 IoU - 1.  Loss terms, gradients and
rectified scores: the project's standing 1e-4 by conftest.rel_err (scores: relative, per element).  tests/test_iou_aware_host.py
holds the scenes away from every kink and score tie, so nothing is left out of a comparison; gradients outside the objects' cells
and in the channels the loss does not reach are exactly 0.  Head and detector: the bounds tests/test_gpu_seg_head.py uses.
"""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct
from bevfusion_multimodal_3d_object_detection_amd import engine, fusion, iou_aware, iou_head, seg_head, synth
from tests import box_iou_ref
from tests import centernet_ref
from tests import iou_aware_ref as R
from tests import test_gpu_seg_head as SEGT
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

_ref_cache = {}


def _scene(name):
    """(pred, tgt) on the device, and the fp64 reference of the scene (computed once, shared, never modified)."""
    pred, tgt = R.loss_scene(name)
    if name not in _ref_cache:
        _ref_cache[name] = (R.iou_targets(pred, tgt, R.LOSS_RANGE), *R.losses(pred, tgt, R.LOSS_RANGE, 0.7, 1.3))
    cuda = lambda d: {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    return cuda(pred), cuda(tgt), _ref_cache[name]


def _run(pred, tgt, with_centernet=False):
    """Loss values and gradients of 0.7 * iou_loss + 1.3 * diou_loss (+ CenterNetLoss) through autograd."""
    p = {k: v.clone().requires_grad_(True) for k, v in pred.items()}
    out = iou_aware.IoUAwareLoss(0.7, 1.3, R.LOSS_RANGE)(p, tgt)
    total = out["total_loss"]
    if with_centernet:
        total = total + ct.CenterNetLoss()(p, tgt)["total_loss"]
    total.backward()
    return {k: v.detach() for k, v in out.items()}, {k: p[k].grad for k in p}


def test_iou_targets_against_the_fp64_reference(gpu):
    for name in ("mixed", "empty"):
        pred, tgt, (t_ref, _, _) = _scene(name)
        got = iou_aware.iou_targets(pred, tgt, R.LOSS_RANGE)
        assert got.shape == (R.LOSS_B, R.LOSS_K) and got.dtype == torch.float32
        err = np.abs(got.cpu().numpy().astype(np.float64) - t_ref)
        print(f"iou_targets '{name}': worst |t - ref| = {err.max():.3e}")
        assert err.max() <= 2e-4
        assert (got.cpu().numpy()[np.asarray(tgt["reg_mask"].cpu()) == 0] == 0).all()
    pred, tgt, _ = _scene("mixed")                                                        # the targets do not read the 'iou' map
    assert torch.equal(iou_aware.iou_targets({k: v for k, v in pred.items() if k != "iou"}, tgt, R.LOSS_RANGE),
                       iou_aware.iou_targets(pred, tgt, R.LOSS_RANGE))


def test_loss_terms_and_gradients_against_the_fp64_reference(gpu):
    pred, tgt, (_, vals_ref, g_ref) = _scene("mixed")
    vals, grads = _run(pred, tgt)
    for k, v in vals_ref.items():
        e = rel_err(vals[k].cpu(), v)
        print(f"IoUAwareLoss {k}: {float(vals[k]):.6f} (fp64 {v:.6f}), rel_err {e:.3e}")
        assert e <= 1e-4, k
    touched = np.zeros((R.LOSS_B, R.LOSS_H * R.LOSS_W), bool)
    for b, _, cell in R.objects(*R.loss_scene("mixed")):
        touched[b, cell] = True
    for k in ("iou", "offset", "size"):
        g = grads[k].cpu().numpy()
        e = rel_err(g, g_ref[k])
        print(f"IoUAwareLoss d/d{k}: rel_err {e:.3e}")
        assert e <= 1e-4, k
        flat = g.reshape(R.LOSS_B, g.shape[1], -1)
        assert (flat[~np.broadcast_to(touched[:, None], flat.shape)] == 0).all(), k      # exactly 0 outside the objects' cells
    assert (grads["size"][:, 2] == 0).all() and (grads["rot"] is None or (grads["rot"] == 0).all())
    assert all(grads[k] is None for k in ("heatmap", "vel"))
    with pytest.raises(NotImplementedError, match="total_loss"):
        p = {k: v.clone().requires_grad_(True) for k, v in pred.items()}
        iou_aware.IoUAwareLoss(pc_range=R.LOSS_RANGE)(p, tgt)["diou_loss"].backward()
    with torch.no_grad():                                                                 # the no-grad path returns the same values
        plain = iou_aware.IoUAwareLoss(0.7, 1.3, R.LOSS_RANGE)(pred, tgt)
    assert all(torch.equal(plain[k], vals[k]) for k in vals)


def test_loss_summed_with_centernet_loss_through_autograd(gpu):
    """The two autograd functions' gradients on offset / size add: the sum's gradients are CenterNetLoss's own plus the reference's."""
    pred, tgt, (_, _, g_ref) = _scene("mixed")
    _, both = _run(pred, tgt, with_centernet=True)
    p = {k: v.clone().requires_grad_(True) for k, v in pred.items()}
    ct.CenterNetLoss()(p, tgt)["total_loss"].backward()
    for k in ("heatmap", "offset", "size", "rot", "vel", "iou"):
        own = torch.zeros_like(pred[k]) if p[k].grad is None else p[k].grad
        want = own.cpu().double() + (torch.from_numpy(g_ref[k]) if k in g_ref else 0.0)
        assert rel_err(both[k].cpu(), want) <= 1e-4, k
    assert float(both["offset"].abs().sum()) > 0 and float((both["offset"] - p["offset"].grad).abs().sum()) > 0


def test_two_runs_are_bit_equal(gpu):
    pred, tgt, _ = _scene("mixed")
    (v1, g1), (v2, g2) = _run(pred, tgt), _run(pred, tgt)
    assert all(torch.equal(v1[k], v2[k]) for k in v1)
    assert all(torch.equal(g1[k], g2[k]) for k in ("iou", "offset", "size"))
    assert torch.equal(iou_aware.iou_targets(pred, tgt, R.LOSS_RANGE), iou_aware.iou_targets(pred, tgt, R.LOSS_RANGE))


def test_empty_frames_and_empty_batch_give_zero(gpu):
    pred, tgt, _ = _scene("empty")
    vals, grads = _run(pred, tgt)
    assert all(float(v) == 0.0 for v in vals.values())
    assert all((grads[k] == 0).all() and torch.isfinite(grads[k]).all() for k in ("iou", "offset", "size"))
    p0, t0 = {k: v[:0] for k, v in pred.items()}, {k: v[:0] for k, v in tgt.items()}
    vals, grads = _run(p0, t0)
    assert all(float(v) == 0.0 for v in vals.values()) and grads["offset"].shape == (0, 2, R.LOSS_H, R.LOSS_W)
    assert iou_aware.iou_targets(p0, t0, R.LOSS_RANGE).shape == (0, R.LOSS_K)


def test_device_side_argument_errors(gpu):
    pred, tgt, _ = _scene("mixed")
    with pytest.raises(L.BevfError, match="size has shape"):
        iou_aware.iou_targets(dict(pred, size=pred["size"][:, :2]), tgt, R.LOSS_RANGE)
    with pytest.raises(L.BevfError, match="iou has shape"):
        iou_aware.IoUAwareLoss(pc_range=R.LOSS_RANGE)(dict(pred, iou=pred["iou"][:, :, :4]), tgt)
    with pytest.raises(L.BevfError, match="build the detector with iou_head=True"):
        ct.decode_padded({k: v for k, v in pred.items() if k != "iou"}, iou_rectify=0.5)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        ct.decode_padded(pred, iou_rectify=1.5)
    with pytest.raises(ValueError, match="classes"):
        ct.decode_centernet_predictions(pred, iou_rectify=(0.5, 0.5))
    with pytest.raises(L.BevfError, match="raw_scores"):
        L.centernet_decode(pred, 4, 0.1, 2.048, -51.2, -51.2, raw_scores=True, iou=pred["iou"], alpha=torch.zeros(R.LOSS_C, device="cuda"))


def test_loss_forward_and_backward_replay_from_a_graph(gpu):
    """Nothing is read back and no shape depends on data: the loss and its gradients capture into a graph and replay bit-equal."""
    pred, tgt, _ = _scene("mixed")
    vals, grads = _run(pred, tgt)
    d = {k: torch.zeros_like(pred[k]) for k in ("iou", "offset", "size")}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        L.iou_aware_loss(pred, tgt, R.LOSS_RANGE, 0.7, 1.3)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = L.iou_aware_loss(pred, tgt, R.LOSS_RANGE, 0.7, 1.3)
        L.iou_aware_loss_bwd(pred, tgt, R.LOSS_RANGE, 0.7, 1.3, d["iou"], d["offset"], d["size"])
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], vals["total_loss"]) and all(torch.equal(d[k], grads[k]) for k in d)


# ---- the rectified decode -----------------------------------------------------------------------------------------------------------

def _decode_scene():
    return {k: torch.from_numpy(v).cuda() for k, v in R.decode_scene().items()}


def test_rectified_decode_against_the_fp64_reference(gpu):
    pred = _decode_scene()
    K = R.DECODE_K
    spec = R.rectified_spec(R.decode_scene()["heatmap"], R.decode_scene()["iou"], R.DECODE_ALPHA, K)
    out = ct.decode_padded(pred, R.DECODE_THRESH, K, True, iou_rectify=R.DECODE_ALPHA)
    base = ct.decode_padded({k: v for k, v in pred.items() if k != "iou"}, R.DECODE_THRESH, K, True)
    torch.cuda.synchronize()
    labels, scores = out["labels"].cpu().numpy(), out["scores"].cpu().numpy()
    boxes = out["boxes"].cpu().numpy()
    assert np.array_equal(labels, spec["cls"])                                            # order and labels: exact
    bs = centernet_ref.boxes_spec({k: torch.from_numpy(v) for k, v in R.decode_scene().items()}, spec, R.DECODE_THRESH,
                                  2.048, *centernet_ref.ORIGIN)
    assert (np.abs(boxes[..., 0] - bs["x"]) <= bs["x_bound"]).all() and (np.abs(boxes[..., 1] - bs["y"]) <= bs["y_bound"]).all()
    assert np.array_equal(centernet_ref.bits(boxes[..., 3:6]), bs["size_bits"])           # the cells: exact copies of their maps
    assert np.array_equal(centernet_ref.bits(out["velocities"]), bs["vel_bits"])
    assert np.abs(boxes[..., 6] - bs["yaw"]).max() <= 1e-6
    want_count = (spec["score"] > R.DECODE_THRESH).sum(1)
    assert np.array_equal(out["count"].cpu().numpy(), want_count) and want_count.tolist() == [4, 4]
    assert base["count"].cpu().tolist() == [6, 5]                                         # peaks pushed under the threshold: the count drops
    pos = spec["score"] > 0
    assert (scores[~pos] == 0).all()
    rel = np.abs(scores[pos].astype(np.float64) - spec["score"][pos]) / spec["score"][pos]
    print(f"rectified scores: worst relative error against fp64 = {rel.max():.3e} over {pos.sum()} scores")
    assert rel.max() <= 1e-4
    # class 0 (alpha = 0): the raw heatmap value of its cell, bit for bit, as the unrectified decode returns it
    heat = R.decode_scene()["heatmap"]
    c0 = labels == 0
    raw = heat[np.arange(R.DECODE_B)[:, None], 0, spec["y"], spec["x"]]
    assert c0.sum() >= 5 and np.array_equal(centernet_ref.bits(scores[c0 & pos]), centernet_ref.bits(raw[c0 & pos]))
    for b in range(R.DECODE_B):                                                           # and the same set of class-0 scores
        pick = lambda o: sorted(centernet_ref.bits(o["scores"][b][(o["labels"][b] == 0) & (o["scores"][b] > 0)]).tolist())
        assert pick(out) == pick(base) and len(pick(out)) >= 2
    # the pair whose order the rectification reverses
    order = lambda o, b: [(int(l), round(float(s), 3)) for l, s in zip(o["labels"][b].cpu(), o["scores"][b].cpu())]
    assert order(base, 0)[0] == (1, 0.9) and (1, 0.6) in order(base, 0)
    got = [s for l, s in order(out, 0) if l == 1]
    assert got[:2] == [0.735, 0.424]


def test_rectify_none_and_alpha_zero_are_bit_equal_to_the_plain_decode(gpu):
    pred = _decode_scene()
    plain = {k: v for k, v in pred.items() if k != "iou"}
    for kw in (dict(), dict(nms_type="rotate", nms_iou_thresh=0.2, nms_pre_max=16)):
        want = ct.decode_padded(plain, R.DECODE_THRESH, R.DECODE_K, True, **kw)
        for rect in (None, 0.0, (0.0, 0.0, 0.0)):
            got = ct.decode_padded(pred, R.DECODE_THRESH, R.DECODE_K, True, iou_rectify=rect, **kw)
            n = want["count"].cpu().tolist()
            assert got["count"].cpu().tolist() == n
            for k in ("boxes", "scores", "labels", "velocities"):
                for b in range(R.DECODE_B):
                    rows = slice(0, n[b]) if kw else slice(None)                         # rows past count mean nothing after an NMS
                    a, w = got[k][b, rows], want[k][b, rows]
                    same = np.array_equal(centernet_ref.bits(a), centernet_ref.bits(w)) if a.dtype == torch.float32 else torch.equal(a, w)
                    assert same, (kw, rect, k, b)
    lists = ct.decode_centernet_predictions(pred, R.DECODE_THRESH, R.DECODE_K, True, iou_rectify=None)
    assert [len(f["scores"]) for f in lists] == [6, 5]


def test_rotated_nms_suppresses_the_duplicate_with_the_lower_predicted_iou(gpu):
    """A (raw 0.90, low predicted IoU) and B (raw 0.60, high predicted IoU) are the same box 0.2 m apart: on raw scores the NMS keeps
    A, on rectified scores it keeps B."""
    pred = _decode_scene()
    kw = dict(score_thresh=R.DECODE_THRESH, max_detections=R.DECODE_K, true_labels=True, nms_type="rotate", nms_iou_thresh=0.2,
              nms_pre_max=16)
    raw = ct.decode_centernet_predictions(pred, **kw)[0]
    rect = ct.decode_centernet_predictions(pred, iou_rectify=R.DECODE_ALPHA, **kw)[0]
    pick = lambda f: [round(float(s), 3) for s, l in zip(f["scores"].cpu(), f["labels"].cpu()) if int(l) == 1]
    assert pick(raw) == [0.9, 0.7] and pick(rect) == [0.735]
    xs = lambda f: [round(float(b[0]), 2) for b, l in zip(f["boxes"].cpu(), f["labels"].cpu()) if int(l) == 1]
    assert xs(raw)[0] == round((5 + 1.45) * 2.048 - 51.2, 2) and xs(rect)[0] == round((7 - 0.45) * 2.048 - 51.2, 2)
    # the whole frame against the greedy reference on the fp64 boxes of the rectified order
    scene = R.decode_scene()
    spec = R.rectified_spec(scene["heatmap"], scene["iou"], R.DECODE_ALPHA, 16)
    bs = centernet_ref.boxes_spec({k: torch.from_numpy(v) for k, v in scene.items()}, spec, R.DECODE_THRESH, 2.048, *centernet_ref.ORIGIN)
    n = int(bs["count"][0])
    size = np.ascontiguousarray(bs["size_bits"][0, :n]).view(np.float32).astype(np.float64)
    boxes = np.concatenate([bs["x"][0, :n, None], bs["y"][0, :n, None], np.zeros((n, 1)), size, bs["yaw"][0, :n, None]], 1)
    keep = box_iou_ref.nms(boxes, "rotate", 0.2)
    assert 0 < len(keep) < n and [int(l) for l in rect["labels"].cpu()] == [int(spec["cls"][0, i]) for i in keep]


# ---- the head alone -------------------------------------------------------------------------------------------------------------------

def _head_pair(seed=3):
    """IoUHead at the channel counts of test_gpu_seg_head._head_pair and the same branch as a plain torch module."""
    mod = iou_head.IoUHead(in_channels=64, head_conv=64)
    ref = torch.nn.Sequential(torch.nn.Conv2d(64, 64, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(64, 1, 1))
    synth.fill_state_dict_(mod, seed)
    ref.load_state_dict({k[len("branch."):]: v for k, v in mod.state_dict().items()})
    return ref, mod


def test_head_eval_fp32_and_bf16_against_the_fp64_composition(gpu):
    ref, mod = _head_pair()
    x = synth.normal((2, 64, 12, 9), 21)
    with torch.no_grad():
        want = ref.double()(x.double())
    out = mod.cuda().eval()(x.cuda())
    assert out.shape == (2, 1, 12, 9) and out.dtype == torch.float32 and not out.requires_grad
    e32 = rel_err(out.cpu(), want)
    ref16, mod16 = _head_pair()
    with torch.no_grad():
        for t in ref16.parameters():
            t.copy_(SEGT._r16(t))
    mod16.load_state_dict({"branch." + k: v for k, v in ref16.state_dict().items()})
    with torch.no_grad():
        want16 = ref16.double()(SEGT._r16(x).double())
    out16 = mod16.cuda().bfloat16().eval()(x.cuda())
    assert out16.dtype == torch.float32 and out16.shape == (2, 1, 12, 9)
    e16 = rel_err(out16.cpu(), want16)
    print(f"IoUHead eval: rel_err fp32 {e32:.3e}, bf16 storage {e16:.3e}")
    assert e32 <= 1e-4 and e16 <= 3e-2


@pytest.fixture
def exact_convs():
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    yield
    engine.set_conv_mode(old)


def test_head_alone_in_train_mode_against_fp64_autograd(gpu, exact_convs):
    ref, mod = _head_pair(seed=5)
    ref, mod = ref.double().train(), mod.cuda().train()
    x, w = synth.normal((2, 64, 12, 9), 22), synth.normal((2, 1, 12, 9), 23)
    xr, xg = x.double().requires_grad_(True), x.cuda().requires_grad_(True)
    want, out = ref(xr), mod(xg)
    assert out.requires_grad and rel_err(out.detach().cpu(), want.detach()) <= 1e-4
    (want * w.double()).sum().backward()
    (out * w.cuda()).sum().backward()
    SEGT._check_grads([(n, p.grad) for n, p in mod.named_parameters()], [("branch." + n, p.grad) for n, p in ref.named_parameters()],
                      "iou head parameters")
    assert xg.grad.shape == x.shape and rel_err(xg.grad.cpu(), xr.grad) <= 2e-4
    with torch.no_grad():
        again = mod(x.cuda())
    assert not again.requires_grad and rel_err(again.cpu(), want.detach()) <= 1e-4
    with pytest.raises(L.BevfError, match="train mode is not supported"):
        mod.bfloat16()(x.cuda().requires_grad_(True))


# ---- the detector ---------------------------------------------------------------------------------------------------------------------

def _detectors(seed=7, **extra):
    """The small detector of test_gpu_seg_head._detectors with the IoU head, and one without it on the same weights."""
    m = fusion.create_detector("camera+lidar", bev_h=16, bev_w=16, iou_head=True, **extra)
    synth.fill_state_dict_(m, seed)
    plain = fusion.create_detector("camera+lidar", bev_h=16, bev_w=16, **extra)
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("iou_head.")})
    return m.cuda(), plain.cuda()


def test_detector_eval_iou_beside_unchanged_detection_outputs(gpu):
    m, plain = _detectors()
    m.eval(), plain.eval()
    imgs, pts = SEGT._frame(40)
    out, base = m(imgs, pts, None), plain(imgs, pts, None)
    assert set(out) == set(engine.HEAD_BRANCHES) | {"iou"} and set(base) == set(engine.HEAD_BRANCHES)
    assert set(m.state_dict()) - set(plain.state_dict()) == {f"iou_head.branch.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")}
    for k in engine.HEAD_BRANCHES:
        assert torch.equal(out[k], base[k]), k                                         # bit-equal to the detector without the head
    fused = m.fusion(m.camera_encoder(imgs), m.lidar_encoder(pts), None)
    assert out["iou"].shape == (2, 1, 16, 16) and out["iou"].dtype == torch.float32
    assert torch.equal(out["iou"], m.iou_head(fused)) and float(out["iou"].std()) > 0
    dets = ct.decode_centernet_predictions(out, 0.0, 10, True, iou_rectify=0.5)           # the output feeds the rectified decode
    assert len(dets) == 2 and all(torch.isfinite(d["scores"]).all() for d in dets)


def test_detector_train_gradients_are_the_sum_of_the_two_tasks(gpu):
    """CenterNetLoss + IoUAwareLoss backward through the detector = the detection loss alone (the detector WITHOUT the head: the
    unchanged single-consumer path) + the IoU-aware loss alone, every pass starting from the same BatchNorm buffers.  The
    IoU-aware loss reaches the detection head too (offset and size), so only iou_head.* belongs to one task."""
    m, plain = _detectors(seed=9)
    m.train(), plain.train()
    imgs, pts = SEGT._frame(41)
    tgt, _ = SEGT._targets(gpu)
    saved = {n: b.clone() for n, b in m.named_buffers()}

    def run(model, det, iou):
        for n, b in model.named_buffers():
            b.copy_(saved[n])
        model.zero_grad(set_to_none=True)
        out = model(imgs, pts, None)
        loss = 0.0
        if det:
            loss = loss + ct.CenterNetLoss()(out, tgt)["total_loss"]
        if iou:
            loss = loss + iou_aware.IoUAwareLoss()(out, tgt)["total_loss"]
        loss.backward()
        return out, {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}

    out, both = run(m, True, True)
    assert set(out) == set(engine.HEAD_BRANCHES) | {"iou"} and out["iou"].requires_grad and out["iou"].shape == (2, 1, 16, 16)
    _, det_only = run(plain, True, False)
    _, iou_only = run(m, False, True)
    assert all(g is not None and torch.isfinite(g).all() for g in both.values())
    shared = [n for n in both if not n.startswith("iou_head.")]
    assert len(shared) > 60 and any(n.startswith("fusion.") for n in shared) and any(n.startswith("det_head.") for n in shared)
    iou_only = {n: (torch.zeros_like(both[n]) if g is None else g) for n, g in iou_only.items()}
    assert all(float(iou_only[n].abs().sum()) > 0 for n in shared if n.endswith("conv1.weight"))     # the loss reaches the encoders
    assert float(iou_only["det_head.size_head.2.weight"].abs().sum()) > 0 and float(iou_only["det_head.vel_head.2.weight"].abs().sum()) == 0
    SEGT._check_grads([(n, both[n]) for n in shared], [(n, det_only[n] + iou_only[n]) for n in shared], "detector, two consumers of fused")
    SEGT._check_grads([(n, g) for n, g in both.items() if n.startswith("iou_head.")],
                      [(n, g) for n, g in iou_only.items() if n.startswith("iou_head.")], "iou head inside the detector")


def test_detector_with_seg_head_and_iou_head_together(gpu):
    m, plain = _detectors(seed=11, seg_head=SEGT.SEG)
    only_iou, _ = _detectors(seed=11)
    only_iou.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("seg_head.")})
    imgs, pts = SEGT._frame(42)
    m.eval(), plain.eval(), only_iou.eval()
    out, base, ref = m(imgs, pts, None), plain(imgs, pts, None), only_iou(imgs, pts, None)
    assert list(out)[-2:] == ["seg", "iou"] and set(out) == set(engine.HEAD_BRANCHES) | {"seg", "iou"}
    assert all(torch.equal(out[k], base[k]) for k in base) and torch.equal(out["iou"], ref["iou"])
    m.train()
    out = m(imgs, pts, None)
    assert list(out)[-2:] == ["seg", "iou"] and out["seg"].shape == (2, 3, 12, 12) and out["iou"].shape == (2, 1, 16, 16)
    tgt, masks = SEGT._targets(gpu)
    loss = ct.CenterNetLoss()(out, tgt)["total_loss"] + seg_head.SegFocalLoss()(out["seg"], masks)["loss"] + \
        iou_aware.IoUAwareLoss()(out, tgt)["total_loss"]
    assert torch.isfinite(loss)
    loss.backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert float(m.seg_head.classifier[0].weight.grad.abs().sum()) > 0 and float(m.iou_head.branch[0].weight.grad.abs().sum()) > 0


def test_graphed_detector_replays_iou_bit_equal_to_eager(gpu):
    m, _ = _detectors(seed=13)
    m.eval()
    frames = [SEGT._frame(44), SEGT._frame(45)]
    eager = [{k: v.clone() for k, v in m(i, p, None).items()} for i, p in frames]
    assert not torch.equal(eager[0]["iou"], eager[1]["iou"])
    g = m.make_graphed(frames[0][0], frames[0][1], None)
    for t, (i, p) in enumerate(frames):
        out = g(i, p, None)
        assert set(out) == set(eager[t])
        for k, v in eager[t].items():
            assert torch.equal(out[k], v), (t, k)
