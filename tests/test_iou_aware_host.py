"""CPU-only checks of the IoU-aware head: settings and state-dict keys, argument errors, and the fp64 reference of
tests/iou_aware_ref.py held to itself -- its analytic gradients against central differences, the DIoU's invariance under a common
rotation, and the committed scenes' distance from every kink and score tie, so that the GPU tests exclude no element."""
import math

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import box_ops, fusion, iou_aware, iou_head
from tests import box_iou_ref
from tests import iou_aware_ref as R

KEYS = {f"iou_head.branch.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")}


def test_settings_parsing():
    S = iou_head.iou_head_settings
    assert S(None, None) is None and S(False, {"model": {"iou_head": {"enable": True}}}) is None
    assert S(True, None) == {} and S(None, {"model": {"iou_head": True}}) == {}
    assert S(None, {"model": {"iou_head": {"enable": True, "head_conv": 32}}}) == {"head_conv": 32}
    assert S({"head_conv": 16}, {"model": {"iou_head": {"head_conv": 32}}}) == {"head_conv": 16}
    assert S({"enable": False}, None) is None
    with pytest.raises(L.BevfError, match="unknown settings"):
        S({"width": 3}, None)
    with pytest.raises(L.BevfError, match="must be True, False, None or a dict"):
        S("yes", None)
    cfg = {"inference": {"post_processing": {"score_threshold": 0.2, "iou_rectify": [0.5, 1]}}}
    assert box_ops.decode_settings(cfg)["iou_rectify"] == [0.5, 1.0]
    cfg["inference"]["post_processing"]["iou_rectify"] = 0.25
    assert box_ops.decode_settings(cfg)["iou_rectify"] == 0.25
    del cfg["inference"]["post_processing"]["iou_rectify"]
    assert "iou_rectify" not in box_ops.decode_settings(cfg)


def test_state_dict_keys_with_and_without_the_option():
    plain = fusion.create_detector("lidar", bev_h=16, bev_w=16)
    m = fusion.create_detector("lidar", bev_h=16, bev_w=16, iou_head=True)
    assert plain.iou_head is None and set(m.state_dict()) - set(plain.state_dict()) == KEYS
    assert set(plain.state_dict()) <= set(m.state_dict())
    by_cfg = fusion.FlexibleMultiModal3DDetector(use_camera=False, use_radar=False, bev_h=16, bev_w=16,
                                                 config={"model": {"iou_head": {"enable": True, "head_conv": 32}}})
    assert set(by_cfg.state_dict()) - set(plain.state_dict()) == KEYS
    br = by_cfg.iou_head.branch
    assert br[0].weight.shape == (32, by_cfg.fusion.bev_channels, 3, 3) and br[2].weight.shape == (1, 32, 1, 1)
    assert float(br[0].bias.detach().abs().sum()) == 0 and float(br[2].bias.detach().abs().sum()) == 0 and 0 < float(br[0].weight.detach().std()) < 3e-3
    both = fusion.create_detector("lidar", bev_h=16, bev_w=16, iou_head={"head_conv": 16}, seg_head=dict(num_classes=2))
    assert KEYS <= set(both.state_dict()) and any(k.startswith("seg_head.") for k in both.state_dict())


def test_argument_errors():
    A = iou_aware.rectify_alpha
    assert A(None, 3) is None and A(0.5, 3) == [0.5] * 3 and A((0, 0.5, 1), 3) == [0.0, 0.5, 1.0] and A(torch.tensor([1.0, 0.0]), 2) == [1.0, 0.0]
    for bad in (-0.1, 1.5, float("nan"), (0.5, 0.5), (0.1, 0.2, 1.2), True, "a"):
        with pytest.raises(ValueError):
            A(bad, 3)
    with pytest.raises(ValueError, match="pc_range"):
        iou_aware.IoUAwareLoss(pc_range=(0, 0, 0, 0, 1, 1))
    pred, tgt = (({k: torch.from_numpy(v) for k, v in d.items()}) for d in R.loss_scene("mixed"))
    loss = iou_aware.IoUAwareLoss(pc_range=R.LOSS_RANGE)
    with pytest.raises(L.BevfError, match="iou"):
        loss({k: v for k, v in pred.items() if k != "iou"}, tgt)
    with pytest.raises(L.BevfError, match="target_rot"):
        iou_aware.iou_targets(pred, {k: v for k, v in tgt.items() if k != "target_rot"})
    with pytest.raises(ValueError, match="frames"):
        loss(pred, {k: v[:1] for k, v in tgt.items()})
    with pytest.raises(L.BevfError, match="no CPU fallback"):
        loss(pred, tgt)
    with pytest.raises(L.BevfError, match="no CPU fallback"):
        iou_aware.iou_targets(pred, tgt, R.LOSS_RANGE)
    with pytest.raises(L.BevfError, match="BEV map"):
        iou_head.IoUHead(in_channels=64)(torch.zeros(1, 32, 4, 4))


def _numeric(pred, tgt, key, idx, h, forward_only=False):
    t = R.iou_targets(pred, tgt, R.LOSS_RANGE)                        # a constant of the loss

    def at(delta):
        p = {k: np.array(v, np.float64) for k, v in pred.items()}
        p[key][idx] += delta
        return R.losses(p, tgt, R.LOSS_RANGE, 0.7, 1.3, t_fixed=t)[0]["total_loss"]
    return (at(h) - at(0.0)) / h if forward_only else (at(h) - at(-h)) / (2 * h)


def test_reference_gradients_against_central_differences():
    """Every coordinate the loss can reach, in fp64 with h = 1e-6.  The object bitwise equal to its ground truth sits on the kink
    at the loss's minimum: the documented subgradient there is the derivative towards larger sizes, so its cell's size
    coordinates are held to the forward difference."""
    pred, tgt = R.loss_scene("mixed")
    _, g = R.losses(pred, tgt, R.LOSS_RANGE, 0.7, 1.3)
    W = R.LOSS_W
    cells = sorted({(b, cell) for b, _, cell in R.objects(pred, tgt)})
    tied = {(b, cell) for (b, k, cell), o in zip(R.objects(pred, tgt), R._per_object(pred, tgt, R.LOSS_RANGE)) if o[-1]}
    assert len(cells) == 3 and len(tied) == 1
    checked = 0
    for b, cell in cells:
        cy, cx = divmod(cell, W)
        for key, chans in (("iou", (0,)), ("offset", (0, 1)), ("size", (0, 1, 2)), ("rot", (0, 1))):
            for ch in chans:
                one_sided = (b, cell) in tied and key == "size"
                num = _numeric(pred, tgt, key, (b, ch, cy, cx), 1e-6, forward_only=one_sided)
                ana = g[key][b, ch, cy, cx] if key in g else 0.0
                assert abs(num - ana) <= 1e-5 * max(1.0, abs(ana)), (key, b, ch, cy, cx, num, ana)
                checked += 1
    assert checked == 3 * 8
    touched = np.zeros((R.LOSS_B, R.LOSS_H * R.LOSS_W), bool)
    for b, cell in cells:
        touched[b, cell] = True
    for key in g:                                                     # nothing outside the objects' cells, nothing in size[2]
        flat = g[key].reshape(R.LOSS_B, g[key].shape[1], -1)
        assert (flat[~np.broadcast_to(touched[:, None], flat.shape)] == 0).all()
    assert (g["size"][:, 2] == 0).all() and any(g[k].any() for k in g)
    neg = g["size"][0, 0, 1, 10]
    assert neg == 0 and g["size"][0, 1, 1, 10] != 0                   # the width under the 1e-3 clamp gets no gradient, the length does


def test_diou_is_invariant_under_a_common_rotation():
    rng = np.random.default_rng(7)
    for _ in range(50):
        dx, dy = rng.uniform(-3, 3, 2)
        wp, lp, wg, lg = rng.uniform(0.5, 5, 4)
        yaw, turn = rng.uniform(-math.pi, math.pi, 2)
        base = R.diou_obj(dx, dy, wp, lp, wg, lg, math.sin(yaw), math.cos(yaw))
        ct, st = math.cos(turn), math.sin(turn)
        moved = R.diou_obj(ct * dx - st * dy, st * dx + ct * dy, wp, lp, wg, lg, math.sin(yaw + turn), math.cos(yaw + turn))
        assert abs(base - moved) <= 1e-12
        assert -1.0 - 1e-9 <= 1.0 - base <= 1.0 + 1e-9                # d lies in [-1, 1]


def test_loss_scenes_hold_what_the_gpu_tests_rely_on():
    pred, tgt = R.loss_scene("mixed")
    assert pred["offset"].shape == (2, 2, 8, 12) and tgt["ind"].shape == (2, 8)
    assert tgt["reg_mask"].sum(1).tolist() == [5, 0]
    t = R.iou_targets(pred, tgt, R.LOSS_RANGE)
    per = R._per_object(pred, tgt, R.LOSS_RANGE)
    assert t[0, 2] == pytest.approx(1.0, abs=1e-12) and per[2][-1]                       # identical to its GT
    assert t[0, 1] == -1.0 and 1.0 - per[1][6] < 0                                       # disjoint: t = -1, d < 0
    assert t[0, 0] == -1.0 and pred["size"][0, 0, 1, 10] < 0                             # negative raw width: IoU 0
    assert len({int(tgt["ind"][0, k]) for k in (2, 3, 4)}) == 1 and -1 < t[0, 3] < 1 and -1 < t[0, 4] < 1 and t[0, 3] != t[0, 4]
    assert int(tgt["ind"][0, 1]) == R.LOSS_H * R.LOSS_W - 1
    yaws = {round(math.atan2(*tgt["target_rot"][0, k]), 6) for k in (0, 2)}
    assert yaws == {round(-math.pi, 6), round(math.pi, 6)}
    assert (t[0, 5:] == 0).all() and (t[1] == 0).all()
    margin, ties = R.kink_margin(pred, tgt)
    print(f"loss scene 'mixed': kink margin {margin:.4f}, exact ties {ties}")
    assert margin >= 1e-2 and ties == 1
    pe, te = R.loss_scene("empty")
    assert te["reg_mask"].sum() == 0 and R.kink_margin(pe, te) == (math.inf, 0)
    vals, g = R.losses(pe, te, R.LOSS_RANGE)
    assert all(v == 0 for v in vals.values()) and not any(a.any() for a in g.values())


def test_decode_scene_scores_are_separated():
    pred = R.decode_scene()
    spec = R.rectified_spec(pred["heatmap"], pred["iou"], R.DECODE_ALPHA, R.DECODE_K)
    raw = R.rectified_spec(pred["heatmap"], pred["iou"], (0.0,) * R.DECODE_C, R.DECODE_K)
    for s in (spec, raw):
        assert R.score_separation(s, R.DECODE_THRESH) > box_iou_ref.MARGIN
    cells = lambda s, b: [(int(c), int(y), int(x)) for c, y, x, v in zip(s["cls"][b], s["y"][b], s["x"][b], s["score"][b]) if v > 0.01]
    A, Bq = (1, 5, 5), (1, 5, 7)
    assert cells(raw, 0).index(A) < cells(raw, 0).index(Bq) and cells(spec, 0).index(Bq) < cells(spec, 0).index(A)   # reversed
    count = lambda s: (s["score"] > R.DECODE_THRESH).sum(1).tolist()
    assert count(raw) == [6, 5] and count(spec) == [4, 4]              # pushed under the threshold / to 0: the count drops
    assert (2, 14, 8) in cells(spec, 0) and (1, 11, 11) not in cells(spec, 0)                 # q = 0.1 stays positive, NaN -> 0
    assert spec["score"][1].max() == pytest.approx(1.0) and (1, 8, 2) not in cells(spec, 1)  # iou 1.7 -> q = 1, iou -3 -> q = 0
    m = R.rectified_map(pred["heatmap"], pred["iou"], R.DECODE_ALPHA)
    keep = m[:, 0] > 0
    assert np.array_equal(m[:, 0][keep], pred["heatmap"][:, 0][keep].astype(np.float64)) and keep.sum() == 4 + 2 and np.isfinite(m).all()
