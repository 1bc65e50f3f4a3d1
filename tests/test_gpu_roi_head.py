"""CenterPoint second stage on the GPU: the five-point gather and its pull backward, the RoI targets, the loss and the
refine step against the fp64 restatement of tests/roi_head_ref.py; the head module in eval (fp32, bf16) and train mode against the
fp64 composition; the detector with the head -- eager, refined, tracked, trained, and the second stage as a replayed graph.

Bounds.  Gather: per element 8 * 2^-24 * sum |w||v| (four roundings in the sum, one per weight, slack 2), bf16 plus 2^-8 |ref| for
the output rounding; backward (n + 2) * 2^-24 * sum |w dy| with n the cell's contributions.  Targets: iou 1e-4 (IOU_TOL of
tests/test_gpu_box_nms.py), cls_target 2e-4, reg_target 1e-4 by conftest.rel_err per column, indices and masks exact.  Loss: 1e-4 by
rel_err.  Refine: 1e-5 (2-3 fp32 operations on exp / sigmoid / sqrt).  Module and detector: the bounds of tests/test_gpu_seg_head.py.
tests/test_roi_head_host.py holds the scenes away from every decision boundary, so every element is compared.
"""
import math

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as ct
from bevfusion_multimodal_3d_object_detection_amd import engine, fusion, roi_head, roi_refine, synth, tracking
from tests import roi_head_ref as R
from tests import test_gpu_seg_head as SEGT
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
H, W, RNG = R.MAP_H, R.MAP_W, R.MAP_RANGE
_cache = {}


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _map(C, seed, bf16=False):
    """The (2, H, W, C) map as fp32 numpy (rounded to bf16 when asked)."""
    x = synth.normal((2, H, W, C), seed)
    return (SEGT._r16(x) if bf16 else x).numpy()


def _gather_ref(key, x, boxes, count):
    if key not in _cache:
        _cache[key] = R.gather(x.astype(np.float64), boxes, count, RNG)
    return _cache[key]


def _gather(x, boxes, count, C, dtype=torch.float32, x_cs=None, table=False):
    B, K = boxes.shape[:2]
    xs = torch.from_numpy(x)
    if x_cs is not None:                                       # channels at a wider stride, the gap filled with values nobody may read
        wide = torch.full((2, H, W, x_cs), 1e30)
        wide[..., :C] = xs
        xs = wide
    xs = xs.to(dtype).cuda().reshape(-1)
    feat = torch.full((B * K * 5 * C,), float("nan"), dtype=dtype, device="cuda")
    tab = torch.empty(L.roi_bev_points_table_words(B, K), dtype=torch.int32, device="cuda") if table else None
    L.roi_bev_points(xs, _cuda(boxes), _cuda(count), feat, tab, H, W, C, x_cs or C, RNG)
    return feat.view(B, K, 5 * C), tab


# ---- gather ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,C,x_cs", [("f32", 4, None), ("f32", 6, None), ("f32", 64, None), ("f32", 4, 8), ("bf16", 8, None),
                                          ("bf16", 12, None)])
def test_gather_forward_against_fp64(gpu, dtype, C, x_cs):
    bf16 = dtype == "bf16"
    boxes, count = R.gather_scene()
    x = _map(C, 100 + C, bf16)
    ref, mag = _gather_ref(("g", dtype, C), x, boxes, count)
    feat, _ = _gather(x, boxes, count, C, torch.bfloat16 if bf16 else torch.float32, x_cs)
    got = feat.double().cpu().numpy()
    assert np.isfinite(got).all()                                                   # every element was written
    bound = 8 * U * mag + (2.0 ** -8 * np.abs(ref) if bf16 else 0.0)
    worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print(f"gather {dtype} C={C}: worst |err| / bound {worst:.3f}")
    assert (np.abs(got - ref) <= bound).all()
    zero = mag == 0                                                                  # padded, outside and non-finite rows
    assert zero[0].all() and zero[1, 5].all() and zero[1, 1].all() and zero[1, 0, C:2 * C].all() and zero[1, 4, C:].all()
    assert (got[zero] == 0).all() and not zero[1, 2].any()
    assert np.array_equal(got[1, 2, :C], x[1, 2, 2].astype(np.float64))              # weights 1 0 0 0: the cell itself, five times
    assert all(np.array_equal(got[1, 2, p * C:(p + 1) * C], got[1, 2, :C]) for p in range(5))


@pytest.mark.parametrize("scene,C", [("gather", 4), ("gather", 6), ("many", 4)])
def test_gather_backward_against_fp64_and_adjoint(gpu, scene, C):
    boxes, count = R.gather_scene() if scene == "gather" else R.many_scene()
    B, K = boxes.shape[:2]
    x = _map(C, 200 + C)
    dy = synth.normal((B, K, 5 * C), 300 + C + K).numpy()
    feat, tab = _gather(x, boxes, count, C, table=True)
    runs = []
    for _ in range(2):
        dx = torch.full((B * H * W * C,), float("nan"), device="cuda")
        L.roi_bev_points_bwd(_cuda(dy).reshape(-1), tab, _cuda(count), dx, B, K, H, W, C)
        runs.append(dx.view(B, H, W, C))
    assert torch.equal(runs[0], runs[1])                                             # no float atomics
    got = runs[0].double().cpu().numpy()
    ref, mag, n = R.gather_bwd(dy.astype(np.float64), boxes, count, H, W, RNG)
    bound = (n[..., None] + 2) * U * mag
    print(f"gather backward {scene} C={C}: worst |err| / bound {float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"most contributions to one cell {int(n.max())}")
    assert (np.abs(got - ref) <= bound).all()
    assert (n == 0).any() and (got[n == 0] == 0).all()                               # untouched cells are exact zeros
    if scene == "many":
        assert n.max() > 64
    # <gather(x), dy> = <x, gather^T(dy)>, both sides in fp64 from the device results
    _, fmag = R.gather(x.astype(np.float64), boxes, count, RNG)
    lhs = float((feat.double().cpu().numpy() * dy).sum())
    rhs = float((x.astype(np.float64) * got).sum())
    tol = float((8 * U * fmag * np.abs(dy)).sum() + (bound * np.abs(x)).sum())
    print(f"adjoint: {lhs:.9e} vs {rhs:.9e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol


# ---- targets --------------------------------------------------------------------------------------------------------------------------

def _target_ref(name, mode):
    if ("t", name, mode) not in _cache:
        _cache[("t", name, mode)] = R.targets(*R.target_scene(name), mode, name == "labels")
    return _cache[("t", name, mode)]


@pytest.mark.parametrize("name", ["mixed", "empty", "labels"])
@pytest.mark.parametrize("mode", ["3d", "bev"])
def test_targets_against_fp64(gpu, name, mode):
    rois, count, roi_labels, gt, gt_labels = R.target_scene(name)
    ref = _target_ref(name, mode)
    r = {"boxes": _cuda(rois), "count": _cuda(count), "labels": _cuda(roi_labels)}
    out = roi_refine.roi_targets(r, (_cuda(gt), _cuda(gt_labels)), iou=mode, match_labels=name == "labels")
    got = {k: v.cpu().numpy() for k, v in out.items()}
    print(f"targets {name} {mode}: max |iou err| {float(np.abs(got['iou'] - ref['iou']).max()):.2e}")
    assert np.abs(got["iou"] - ref["iou"]).max() <= 1e-4
    assert np.array_equal(got["gt_index"], ref["gt_index"]) and np.array_equal(got["reg_mask"], ref["reg_mask"])
    assert np.abs(got["cls_target"] - ref["cls_target"]).max() <= 2e-4
    for c in range(7):
        assert rel_err(got["reg_target"][..., c], ref["reg_target"][..., c]) <= 1e-4, c
    for b in range(2):                                                               # rows past the count: zeros / -1
        pad = slice(int(count[b]), None)
        assert (got["gt_index"][b, pad] == -1).all() and not got["reg_mask"][b, pad].any()
        assert not got["iou"][b, pad].any() and not got["cls_target"][b, pad].any() and not got["reg_target"][b, pad].any()
    if name == "mixed" and mode == "3d":                                             # the batch's lists give the same bits
        batch = {"gt_boxes": [torch.from_numpy(gt[0, :4]), torch.from_numpy(gt[1, :3])],
                 "gt_labels": [torch.from_numpy(gt_labels[0, :4]), torch.from_numpy(gt_labels[1, :3])]}
        again = roi_refine.roi_targets(r, batch)
        assert all(torch.equal(again[k], out[k]) for k in out)


# ---- loss -----------------------------------------------------------------------------------------------------------------------------

def _loss_inputs(name):
    rois, count, roi_labels, gt, gt_labels = R.target_scene(name)
    ref = _target_ref(name, "3d")
    tgt = {"count": _cuda(count), "cls_target": _cuda(ref["cls_target"], torch.float32), "reg_mask": _cuda(ref["reg_mask"]),
           "reg_target": _cuda(ref["reg_target"], torch.float32)}
    tgt64 = {k: v.double().cpu().numpy() for k, v in tgt.items() if k != "count"}
    return R.loss_pred(name), count, tgt, tgt64


def _loss_run(pred, tgt):
    logit = _cuda(pred[..., 0]).requires_grad_(True)
    res = _cuda(pred[..., 1:]).requires_grad_(True)
    out = roi_refine.RoIHeadLoss(0.7, 1.3)({"logit": logit, "residual": res}, tgt)
    out["total_loss"].backward()
    return out, torch.cat([logit.grad.unsqueeze(-1), res.grad], -1)


@pytest.mark.parametrize("name", ["mixed", "empty", "labels"])
def test_loss_and_gradient_against_fp64(gpu, name):
    pred, count, tgt, tgt64 = _loss_inputs(name)
    (total, lc, lr), dref = R.loss(pred.astype(np.float64), count, tgt64, 0.7, 1.3)
    out, d = _loss_run(pred, tgt)
    errs = [rel_err(out[k].detach().cpu(), v) for k, v in (("total_loss", total), ("cls_loss", lc), ("reg_loss", lr))]
    print(f"roi loss {name}: rel_err {errs}, dpred {rel_err(d.cpu(), dref):.2e}")
    assert max(errs) <= 1e-4 and rel_err(d.cpu(), dref) <= 1e-4
    for b in range(2):
        assert not d[b, int(count[b]):].any()                                        # invalid rows: exact zeros
    out2, d2 = _loss_run(pred, tgt)
    assert all(torch.equal(out[k], out2[k]) for k in out) and torch.equal(d, d2)
    with torch.no_grad():                                                            # the no-grad path returns the same values
        plain = roi_refine.RoIHeadLoss(0.7, 1.3)({"logit": _cuda(pred[..., 0]), "residual": _cuda(pred[..., 1:])}, tgt)
    assert all(torch.equal(plain[k], out[k]) for k in out)


def test_loss_of_an_empty_batch_and_single_term_backward(gpu):
    pred, count, tgt, _ = _loss_inputs("mixed")
    empty = dict(tgt, count=torch.zeros(2, dtype=torch.int32, device="cuda"))
    out, d = _loss_run(pred, empty)
    assert all(float(v) == 0.0 for v in out.values()) and not d.any()
    logit = _cuda(pred[..., 0]).requires_grad_(True)
    out = roi_refine.RoIHeadLoss()({"logit": logit, "residual": _cuda(pred[..., 1:])}, tgt)
    with pytest.raises(NotImplementedError, match="use total_loss"):
        out["cls_loss"].backward()


# ---- refine ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["plain", "tie", "drops"])
def test_refine_against_fp64(gpu, name):
    rois, scores, labels, vel, count, pred = R.refine_scene(name)
    thresh = 0.3 if name == "drops" else 0.0
    ref = R.refine(rois, scores, labels, vel, count, pred, thresh)
    r = {"boxes": _cuda(rois), "scores": _cuda(scores), "labels": _cuda(labels), "velocities": _cuda(vel), "count": _cuda(count)}
    out = roi_refine.refine_padded(r, {"logit": _cuda(pred[..., 0]), "residual": _cuda(pred[..., 1:])}, thresh)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["count"].tolist() == ref["count"].tolist() and got["count"].dtype == np.int32
    for b in range(2):
        n, order = int(ref["count"][b]), ref["order"][b]
        assert np.array_equal(got["velocities"][b, :n], vel[b, order]) and np.array_equal(got["labels"][b, :n], labels[b, order])
        assert (np.abs(got["scores"][b, :n] - ref["scores"][b, :n]) <= 1e-5 * ref["scores"][b, :n]).all()
        assert (np.diff(got["scores"][b, :n]) <= 0).all()
        for c in range(6):
            assert rel_err(got["boxes"][b, :n, c], ref["boxes"][b, :n, c]) <= 1e-5, (b, c)
        assert np.abs(got["boxes"][b, :n, 6] - ref["boxes"][b, :n, 6]).max(initial=0) <= 1e-5
        assert not got["boxes"][b, n:].any() and not got["scores"][b, n:].any() and not got["velocities"][b, n:].any()
    if name == "tie":
        assert [k for k in ref["order"][0] if k in (1, 4, 6)] == [1, 4, 6]           # the tie-break is the RoI index
        s = got["scores"][0, :8]
        assert (np.diff(s) == 0).sum() == 2
    if name == "drops":
        assert got["count"][0] < 5 and (got["scores"][0, :got["count"][0]] >= 0.3).all()
    track = tracking.Tracker(2, 10).step(out)                                        # the tracker's input contract
    assert (track["det_track_id"].cpu().numpy()[0, :got["count"][0]] >= 0).all()


def test_refine_inverts_the_target_encoding(gpu):
    rois, count, roi_labels, gt, gt_labels = R.target_scene("mixed")
    ref = _target_ref("mixed", "3d")
    fg = [(b, k) for b in range(2) for k in range(12) if ref["reg_mask"][b, k]]
    n = len(fg)
    r = np.stack([rois[b, k] for b, k in fg])[None]
    want = np.stack([gt[b, ref["gt_index"][b, k]] for b, k in fg]).astype(np.float64)
    pred = np.zeros((1, n, 8), np.float32)
    pred[0, :, 1:] = np.stack([ref["reg_target"][b, k] for b, k in fg])
    scores = np.linspace(0.9, 0.1, n, dtype=np.float32)[None]                        # descending: the order stays
    out = L.roi_refine(_cuda(r), _cuda(scores), _cuda(np.zeros((1, n), np.int64)), None, _cuda(np.array([n], np.int32)), _cuda(pred), 0.0)
    got = out["boxes"][0].double().cpu().numpy()
    assert int(out["count"][0]) == n and out["velocities"] is None
    for c in range(6):
        assert rel_err(got[:, c], want[:, c]) <= 1e-5, c
    d = (got[:, 6] - want[:, 6]) / math.pi                                           # the heading, up to the documented pi fold
    assert np.abs(d - np.round(d)).max() * math.pi <= 1e-5 * max(1.0, np.abs(want[:, 6]).max())
    assert (np.round(d) != 0).any()                                                  # (the scene's opposite-heading RoI folds)


# ---- the module -----------------------------------------------------------------------------------------------------------------------

MOD_RANGE = (RNG[0], RNG[1], -5.0, RNG[2], RNG[3], 3.0)


def _module_scene(seed=5):
    """(x (2, 8, H, W) fp32, rois): B = 2, K = 6, frame 0 with four RoIs and two filler rows, frame 1 full."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((2, 6, 7), np.float32)
    boxes[..., 0], boxes[..., 1] = rng.uniform(-6, 6, (2, 6)), rng.uniform(-4, 4, (2, 6))
    boxes[..., 3:6] = rng.uniform(1, 4, (2, 6, 3))
    boxes[..., 6] = rng.uniform(-3, 3, (2, 6))
    return synth.normal((2, 8, H, W), 70 + seed), boxes, np.array([4, 6], np.int32)


def _head(seed=3, fc=16):
    mod = roi_head.RoIHead(in_channels=8, fc=fc, pc_range=MOD_RANGE)
    synth.fill_state_dict_(mod, seed)
    return mod


def _valid(count, K=6):
    return np.arange(K)[None, :] < count[:, None]


def test_module_eval_fp32_and_bf16_against_the_fp64_composition(gpu):
    x, boxes, count = _module_scene()
    rois = {"boxes": _cuda(boxes), "count": _cuda(count)}
    v = _valid(count)

    def want(mod, xin, r16=False):
        rnd = (lambda t: SEGT._r16(t)) if r16 else (lambda t: t)
        sd = {k: rnd(t.float()).double().numpy() for k, t in mod.state_dict().items() if t.dtype.is_floating_point}
        feat, _ = R.gather(rnd(xin).permute(0, 2, 3, 1).double().numpy(), boxes, count, RNG)
        if r16:
            feat = SEGT._r16(torch.from_numpy(feat).float()).double().numpy()
        return R.mlp_eval(feat.reshape(12, 40), sd).reshape(2, 6, 8)

    mod = _head()
    ref = want(mod, x)
    out = mod.cuda().eval()(x.cuda(), rois)
    assert set(out) == {"logit", "residual"} and out["logit"].shape == (2, 6) and out["residual"].shape == (2, 6, 7)
    assert out["logit"].dtype == out["residual"].dtype == torch.float32 and not out["logit"].requires_grad
    pred = torch.cat([out["logit"].unsqueeze(-1), out["residual"]], -1).cpu().numpy()
    e32 = rel_err(pred[v], ref[v])
    mod16 = _head()
    ref16 = want(mod16, x, True)
    with torch.no_grad():
        for t in list(mod16.parameters()) + [b for b in mod16.buffers() if b.dtype.is_floating_point]:
            t.copy_(SEGT._r16(t))
    out16 = mod16.cuda().bfloat16().eval()(x.cuda(), rois)
    assert out16["logit"].dtype == torch.float32
    e16 = rel_err(torch.cat([out16["logit"].unsqueeze(-1), out16["residual"]], -1).cpu().numpy()[v], ref16[v])
    print(f"RoIHead eval: rel_err fp32 {e32:.3e}, bf16 storage {e16:.3e}")
    assert e32 <= 1e-4 and e16 <= 3e-2
    cl = x.cuda().contiguous(memory_format=torch.channels_last)                      # the detector's 'feat' layout: the same bits
    again = mod(cl, rois)
    assert torch.equal(again["logit"], out["logit"]) and torch.equal(again["residual"], out["residual"])


@pytest.fixture
def exact_convs():
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    yield
    engine.set_conv_mode(old)


def _torch_replica(mod):
    fc = mod.fc
    ref = torch.nn.ModuleDict(dict(shared_fc=torch.nn.Sequential(
        torch.nn.Linear(40, fc, bias=False), torch.nn.BatchNorm1d(fc), torch.nn.ReLU(), torch.nn.Linear(fc, fc, bias=False),
        torch.nn.BatchNorm1d(fc), torch.nn.ReLU()), cls_out=torch.nn.Linear(fc, 1), reg_out=torch.nn.Linear(fc, 7)))
    ref.load_state_dict(mod.state_dict())
    return ref.double().train()


@pytest.mark.parametrize("fc", [16, 160])          # 160: the row BatchNorm walks two channel slabs (128 + 32)
def test_module_train_mode_against_fp64_autograd(gpu, exact_convs, fc):
    x, boxes, count = _module_scene(seed=6)
    v = _valid(count)
    mod = _head(seed=4, fc=fc)
    ref = _torch_replica(mod)
    mod = mod.cuda().train()
    wgt = synth.normal((2, 6, 8), 77)
    # fp64: the gather is linear, so its reference supplies feat and carries dfeat back to the map
    feat, _ = R.gather(x.permute(0, 2, 3, 1).double().numpy(), boxes, count, RNG)
    fr = torch.from_numpy(feat[v]).requires_grad_(True)
    h = ref["shared_fc"](fr)
    want = torch.cat([ref["cls_out"](h), ref["reg_out"](h)], -1)
    (want * wgt.double()[torch.from_numpy(v)]).sum().backward()
    dfeat = np.zeros_like(feat)
    dfeat[v] = fr.grad.numpy()
    dmap, _, _ = R.gather_bwd(dfeat, boxes, count, H, W, RNG)
    # device
    rois = {"boxes": _cuda(boxes), "count": _cuda(count)}
    xg = x.cuda().requires_grad_(True)
    out = mod(xg, rois)
    pred = torch.cat([out["logit"].unsqueeze(-1), out["residual"]], -1)
    assert pred.requires_grad and torch.isfinite(pred).all()
    e_out = rel_err(pred.detach().cpu().numpy()[v], want.detach().numpy())
    (pred * (wgt.cuda() * _cuda(v).unsqueeze(-1))).sum().backward()
    e_buf = max(rel_err(b.cpu(), dict(ref.named_buffers())[n]) for n, b in mod.named_buffers() if b.dtype.is_floating_point)
    assert all(int(b) == int(dict(ref.named_buffers())[n]) for n, b in mod.named_buffers() if n.endswith("num_batches_tracked"))
    rp = dict(ref.named_parameters())
    e_par = {n: rel_err(p.grad.cpu(), rp[n].grad) for n, p in mod.named_parameters()}
    e_map = rel_err(xg.grad.permute(0, 2, 3, 1).cpu(), dmap)
    print(f"RoIHead train fc={fc}: out {e_out:.2e}, buffers {e_buf:.2e}, params {max(e_par.values()):.2e}, map {e_map:.2e}")
    assert e_out <= 1e-4 and e_buf <= 2e-5 and max(e_par.values()) <= 2e-4, e_par
    assert xg.grad.shape == x.shape and e_map <= 2e-4
    with pytest.raises(L.BevfError, match="train mode is not supported"):
        _head().cuda().bfloat16().train()(x.cuda(), rois)


def test_padded_rows_never_enter_the_running_statistics(gpu, exact_convs):
    x, boxes, count = _module_scene(seed=7)
    results = []
    for filler in (0.0, 123.0):
        mod = _head(seed=8).cuda().train()
        b = boxes.copy()
        b[0, 4:] = filler                                                            # the rows past count[0] = 4
        with torch.no_grad():
            out = mod(x.cuda(), {"boxes": _cuda(b), "count": _cuda(count)})
        results.append(([t.clone() for t in mod.buffers()], out["logit"][_cuda(_valid(count))]))
    assert all(torch.equal(p, q) for p, q in zip(results[0][0], results[1][0])) and torch.equal(results[0][1], results[1][1])
    assert not torch.equal(results[0][0][0], _head(seed=8).shared_fc[1].running_mean.cuda())   # (they did move)


# ---- the detector ---------------------------------------------------------------------------------------------------------------------

def _detectors(seed=7):
    """The small detector of test_gpu_seg_head._detectors with the RoI head, and one without it on the same weights."""
    m = fusion.create_detector("camera+lidar", bev_h=16, bev_w=16, roi_head=dict(fc=32))
    synth.fill_state_dict_(m, seed)
    plain = fusion.create_detector("camera+lidar", bev_h=16, bev_w=16)
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("roi_head.")})
    return m.cuda(), plain.cuda()


def test_detector_eval_feat_refine_and_tracker(gpu):
    m, plain = _detectors()
    m.eval(), plain.eval()
    imgs, pts = SEGT._frame(40)
    out, base = m(imgs, pts, None), plain(imgs, pts, None)
    assert set(out) == set(engine.HEAD_BRANCHES) | {"feat"} and set(base) == set(engine.HEAD_BRANCHES)
    assert {k for k in m.state_dict() if k not in plain.state_dict()} == {"roi_head." + k for k in m.roi_head.state_dict()}
    assert set(plain.state_dict()) <= set(m.state_dict())
    for k in engine.HEAD_BRANCHES:
        assert torch.equal(out[k], base[k]), k                                       # bit-equal to the detector without the head
    fused = m.fusion(m.camera_encoder(imgs), m.lidar_encoder(pts), None)
    assert out["feat"].shape == fused.shape and torch.equal(out["feat"], fused)      # the map the heads consumed
    assert out["feat"].is_contiguous(memory_format=torch.channels_last)
    kw = dict(score_thresh=0.0, max_detections=20, true_labels=True)
    rois = ct.decode_padded(out, **kw)
    ho = m.roi_head(out["feat"], rois)
    want = roi_refine.refine_padded(rois, ho, 0.0)
    got = m.refine(out, **kw)
    assert set(got) == set(rois) and all(torch.equal(got[k], want[k]) for k in got)
    n = got["count"].cpu().tolist()
    assert n == rois["count"].cpu().tolist() and all(v > 0 for v in n) and torch.isfinite(got["boxes"]).all()
    assert not torch.equal(got["boxes"][0, :n[0]], rois["boxes"][0, :n[0]])
    trk = tracking.Tracker(2, 10)
    ids = trk.step(got)["det_track_id"].cpu()
    assert all((ids[b, :n[b]] >= 0).all() and (ids[b, n[b]:] == -1).all() for b in range(2))
    with pytest.raises(L.BevfError, match="roi_head=True"):
        plain.refine(base)


def test_detector_training_step_with_both_losses(gpu):
    """One step with CenterNetLoss + RoIHeadLoss: finite, non-zero gradients on every roi_head parameter, and a first stage that the
    second loss does not touch, because 'feat' is detached.  "Does not touch" is asserted exactly where exactness exists: the
    gradients arriving at the five head outputs are bit-equal with and without RoIHeadLoss, a step with RoIHeadLoss alone leaves every
    first-stage gradient None, and every first-stage parameter whose gradient two identical plain steps reproduce bit for bit has
    those same bits in the two-loss step.  The first stage's pixel-GEMM weight-gradient kernels add with fp32 atomics, so two
    identical steps already differ in the last bits of the other parameters (measured on the MI355X: 32 of the 116 first-stage
    gradients reproduce bit for bit, the test prints the figures); those are held to the standing gradient bound of
    tests/test_gpu_seg_head._check_grads instead (worst tensor of the two-loss step against the plain one: 1.8e-5)."""
    m, _ = _detectors(seed=9)
    m.train()
    imgs, pts = SEGT._frame(41)
    tgt, _ = SEGT._targets(gpu)
    gt = [torch.tensor([[10.0, -8.0, 0.0, 4.0, 2.0, 1.5, 0.3], [-20.0, 15.0, 0.0, 5.0, 2.2, 1.6, -1.0]]),
          torch.tensor([[30.0, 30.0, 0.0, 3.0, 1.5, 1.5, 2.0]])]
    batch = {"gt_boxes": gt, "gt_labels": [torch.tensor([1, 4]), torch.tensor([7])]}
    boxes = torch.zeros(2, 4, 7)                                                     # RoIs: the ground truth, jittered
    for b in range(2):
        for k in range(3):
            boxes[b, k] = gt[b][k % len(gt[b])] + torch.tensor([0.3, -0.2, 0.1, 0.2, -0.3, 0.1, 0.1]) * (k + 1) * 0.5
    rois = {"boxes": boxes.cuda(), "count": torch.tensor([3, 3], dtype=torch.int32, device="cuda")}
    saved = {n: b.clone() for n, b in m.named_buffers()}

    def run(first, second):
        for n, b in m.named_buffers():
            b.copy_(saved[n])
        m.zero_grad(set_to_none=True)
        out = m(imgs, pts, None)
        assert "feat" in out and not out["feat"].requires_grad and out["feat"].grad_fn is None and out["heatmap"].requires_grad
        douts = {}
        for k in engine.HEAD_BRANCHES:
            out[k].register_hook(lambda g, k=k: douts.__setitem__(k, g.clone()))
        loss = 0.0
        if first:
            loss = loss + ct.CenterNetLoss()(out, tgt)["total_loss"]
        if second:
            rt = roi_refine.roi_targets(rois, batch)
            assert int(rt["reg_mask"].sum()) >= 2
            loss = loss + roi_refine.RoIHeadLoss()(m.roi_head(out["feat"], rois), rt)["total_loss"]
        loss.backward()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}, douts

    (both, d_both), (plain, d_plain), (again, _), (only, d_only) = run(True, True), run(True, False), run(True, False), run(False, True)
    stage1 = [n for n in both if not n.startswith("roi_head.")]
    assert set(d_both) == set(d_plain) == set(engine.HEAD_BRANCHES) and not d_only
    assert all(torch.equal(d_both[k], d_plain[k]) for k in d_plain)                  # what reaches the first stage: the same bits
    assert all(only[n] is None for n in stage1) and len(stage1) > 60
    for n in both:
        if n.startswith("roi_head."):
            for g in (both[n], only[n]):
                assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0, n
            assert plain[n] is None or not plain[n].any()
    stable = [n for n in stage1 if torch.equal(plain[n], again[n])]
    noise = max(rel_err(again[n].cpu(), plain[n].cpu()) for n in stage1)
    print(f"first stage: {len(stable)} of {len(stage1)} gradients reproduce bit for bit between two identical steps; "
          f"worst run-to-run rel_err of the rest {noise:.2e}")
    assert stable and all(torch.equal(both[n], plain[n]) for n in stable)
    SEGT._check_grads([(n, both[n]) for n in stage1], [(n, plain[n]) for n in stage1], "first stage beside the second-stage loss")


def test_second_stage_replays_from_a_graph(gpu):
    m, _ = _detectors(seed=13)
    m.eval()
    kw = dict(score_thresh=0.0, max_detections=20, true_labels=True)
    outs = [m(*SEGT._frame(s), None) for s in (44, 45)]
    outs = [{k: v.clone() for k, v in o.items()} for o in outs]
    rois = [ct.decode_padded(o, **kw) for o in outs]
    eager = [roi_refine.refine_padded(r, m.roi_head(o["feat"], r), 0.0) for o, r in zip(outs, rois)]
    assert not torch.equal(eager[0]["boxes"], eager[1]["boxes"])
    feat = outs[0]["feat"].clone(memory_format=torch.channels_last)
    static = {k: v.clone() for k, v in rois[0].items()}
    stage = lambda: roi_refine.refine_padded(static, m.roi_head(feat, static), 0.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            stage()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        res = stage()
    for t in (1, 0):
        feat.copy_(outs[t]["feat"])
        for k in static:
            static[k].copy_(rois[t][k])
        graph.replay()
        for k, v in eager[t].items():
            assert torch.equal(res[k], v), (t, k)
