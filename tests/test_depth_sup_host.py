"""LiDAR depth supervision (depth_supervision.py) on the host: the cases of tests/test_gpu_depth_sup.py keep the
margin condition that lets the device comparison exclude nothing, their point clouds really put targets on the feature maps, the
target geometry is the inverse of the frustum branch's and moves with an augmented batch, and the detector refuses what the depth
loss is not built for."""
import math
import os

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib
from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import fusion
from tests import augment_ref
from tests import camera_frustum_ref as FR
from tests import depth_sup_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_cases():
    """(name, points, counts, rigs, Hc, Wc, depth) of every point cloud the GPU tests build on the host."""
    out = []
    for name in DR.CASES:
        pts, counts, rigs = DR.case_points(name)
        _, _, Hc, Wc, depth, _, _ = DR.CASES[name]
        out.append((name, pts, counts, rigs, Hc, Wc, depth))
    n, Hc, Wc, _, _, depth = FR.DETECTOR_CASE
    rigs = [FR.case_rig(n, b) for b in range(2)]
    out.append(("detector, per-frame rigs", DR.detector_points(rigs), None, rigs, Hc, Wc, depth))
    out.append(("detector, static rig", DR.detector_points(rigs[:1] * 2), None, rigs[:1] * 2, Hc, Wc, depth))
    return out


def test_no_point_of_any_test_case_lies_on_a_pixel_a_bin_or_a_range_edge():
    for name, pts, counts, rigs, Hc, Wc, depth in _all_cases():
        m = DR.margin(pts, rigs, Hc, Wc, depth, counts)
        print(f"case {name}: margin {m:.2e}")
        assert m > DR.MARGIN, (name, m)


def test_points_put_targets_on_the_feature_maps():
    """At least a third of the feature pixels get a target, and one pixel holds >= 3 points in different bins (as many different
    bins as there are when D < 3: the single-bin case has three points at different depths in its one bin)."""
    for name, pts, counts, rigs, Hc, Wc, depth in _all_cases():
        per_pixel = DR.pixel_points(pts, rigs, Hc, Wc, depth, counts)
        t = DR.targets_ref(pts, rigs, Hc, Wc, depth, counts)
        assert (t >= 0).sum() == len(per_pixel) and (t >= 0).mean() >= 1 / 3, (name, float((t >= 0).mean()))
        assert t.max() <= depth[0] - 1 and t.min() == -1
        assert any(len(b) >= 3 and len(set(b)) >= min(3, depth[0]) for b in per_pixel.values()), name
        if counts is not None:                                                     # the rows behind counts would have changed the targets
            assert not np.array_equal(DR.targets_ref(pts, rigs, Hc, Wc, depth), t)
        # the packed calibration gives the same targets as K and cam_to_bev^-1
        calib = CR.calib_matrices(rigs)
        assert np.array_equal(DR.targets_from_calib(pts, calib, rigs[0].image_size, Hc, Wc, depth, counts), t), name


def test_case_points_hold_every_kind_of_row():
    pts, counts, rigs = DR.case_points("2")
    _, _, Hc, Wc, depth, N, _ = DR.CASES["2"]
    D, dmin, dmax = depth
    assert counts is not None and all(0 < int(c) < N for c in counts) and counts[0] != counts[1]
    for b, rig in enumerate(rigs):
        body = pts[b, :counts[b], :3]
        zero = (body == 0).all(1)
        assert zero.sum() >= 10 and np.nonzero(zero)[0].min() < np.nonzero(~zero)[0].max() - 100     # interleaved all-zero rows
        assert len(np.unique(body[~zero], axis=0)) < (~zero).sum()                  # exact duplicates
        zc = np.array([[DR.project(rig, c, p)[2] for c in range(rig.num_cameras)] for p in body[~zero]])
        assert (zc < 0).any() and (zc > dmax).any() and ((zc > 0) & (zc < dmin)).any()
        assert (pts[b, counts[b]:, :3] != 0).any(1).all()                           # the tail is not zero padding: counts decides


def test_a_frustum_point_gets_its_own_bin_at_its_own_pixel():
    """The inverse of 3.2d3's geometry: the point camera_rig.frustum_points puts at (camera, pixel, bin) gets that bin at that pixel
    of that camera -- every (camera, bin, pixel) of a small case, through both restatements."""
    ncam, Hc, Wc, depth = 2, 3, 4, (4, 1.0, 65.0)
    rig = FR.case_rig(ncam, 1)
    calib = CR.calib_matrices([rig])
    fp = CR.frustum_points(calib, rig.image_size, Hc, Wc, *depth)[0].reshape(ncam, Hc, Wc, depth[0], 3)
    for cam in range(ncam):
        for y in range(Hc):
            for x in range(Wc):
                for d in range(depth[0]):
                    p = fp[cam, y, x, d][None, None]
                    for t in (DR.targets_ref(p, [rig], Hc, Wc, depth), DR.targets_from_calib(p, calib, rig.image_size, Hc, Wc, depth)):
                        assert t[0, cam, y, x] == d and (t[0, cam] >= 0).sum() == 1, (cam, y, x, d)


def test_augmented_points_and_calibration_give_the_unaugmented_targets():
    """Points through the world transform and the calibration through augment.augmented_calib (identity image maps): the targets of
    the pair are those of the un-augmented pair -- flip, rotation, scale and translation each, and all together."""
    name = "1"
    _, ncam, Hc, Wc, depth, _, _ = DR.CASES[name]
    pts, _, rigs = DR.case_points(name)
    base = rigs[0]
    want = DR.targets_ref(pts[:1], [base], Hc, Wc, depth)[0]
    worlds = [A.world_transform(True, False, 0.0, 1.0, (0, 0, 0)), A.world_transform(False, True, 0.0, 1.0, (0, 0, 0)),
              A.world_transform(False, False, math.radians(17.0), 1.0, (0, 0, 0)), A.world_transform(False, False, 0.0, 1.04, (0, 0, 0)),
              A.world_transform(False, False, 0.0, 1.0, (0.4, -0.3, 0.1)), A.world_transform(True, True, math.radians(-11.0), 0.96, (-0.2, 0.5, -0.1))]
    p = A.neutral_params(len(worlds), ncam, base.image_size, base.image_size)
    moved = np.zeros((len(worlds),) + pts.shape[1:], dtype=np.float64)
    for b, T in enumerate(worlds):
        p.bev_aug[b] = T
        moved[b, :, :3] = pts[0, :, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        moved[b, (pts[0, :, :3] == 0).all(1), :3] = 0.0                            # padding rows stay padding
    calib = A.augmented_calib(base, p).numpy()
    got = DR.targets_from_calib(moved, calib, base.image_size, Hc, Wc, depth)
    for b, T in enumerate(worlds):                                                  # (cam_to_bev' = T . cam_to_bev: the camera frame is unchanged)
        rig = augment_ref.equivalent_rig(base, np.tile(np.eye(3), (ncam, 1, 1)), T)
        assert np.array_equal(got[b], want), b
        assert np.array_equal(DR.targets_ref(moved[b:b + 1], [rig], Hc, Wc, depth)[0], want), b
    # and with image maps (crop, image flip): both restatements agree on the augmented pair, whose targets differ from the plain ones
    q = augment_ref.calib_params(2, ncam, seed=3)
    moved = np.stack([pts[0].astype(np.float64)] * 2)
    for b in range(2):
        moved[b, :, :3] = pts[0, :, :3].astype(np.float64) @ q.bev_aug[b][:3, :3].T + q.bev_aug[b][:3, 3]
        moved[b, (pts[0, :, :3] == 0).all(1), :3] = 0.0
    got = DR.targets_from_calib(moved, A.augmented_calib(base, q).numpy(), base.image_size, Hc, Wc, depth)
    for b, rig in enumerate(FR.augmented_rigs(base, q)):
        assert DR.margin(moved[b:b + 1], [rig], Hc, Wc, depth) > DR.MARGIN
        assert np.array_equal(got[b], DR.targets_ref(moved[b:b + 1], [rig], Hc, Wc, depth)[0]), b
        assert not np.array_equal(got[b], want)


def _golden_keys():
    return open(os.path.join(ROOT, "tests", "golden", "state_dict_keys_clr.txt")).read().split("\n")[:-1]


def test_state_dict_keys_are_unchanged():
    golden = _golden_keys()
    extra = ["fusion.depth_net.weight:(32, 512, 1, 1)", "fusion.depth_net.bias:(32,)"]
    for kind in ("frustum", "lift"):
        m = fusion.create_detector("camera+lidar+radar", "bev", "centernet", camera_view_transform=kind)
        assert sorted(f"{k}:{tuple(v.shape)}" for k, v in m.state_dict().items()) == sorted(golden + extra)
    m = fusion.create_detector("camera+lidar+radar", "bev", "centernet")
    assert sorted(f"{k}:{tuple(v.shape)}" for k, v in m.state_dict().items()) == sorted(golden)


def test_refusals():
    imgs, pts = torch.zeros(1, 6, 3, 64, 96), torch.zeros(1, 100, 4)
    counts = torch.full((1,), 100, dtype=torch.int32)
    det = lambda kind, modality="camera+lidar": fusion.create_detector(modality, "bev", "centernet", bev_h=16, bev_w=24,      # noqa: E731
                                                                        camera_view_transform=kind)
    with pytest.raises(_lib.BevfError, match="depth_points in eval mode"):
        det("frustum").eval()(imgs, pts, None, depth_points=pts)
    for kind in ("mean", "project"):
        with pytest.raises(_lib.BevfError, match=f"depth_points with camera_view_transform='{kind}'"):
            det(kind).train()(imgs, pts, None, depth_points=pts)
    for kind in ("frustum", "lift"):
        with pytest.raises(_lib.BevfError, match="depth_points with torch.bfloat16 storage"):
            det(kind).bfloat16().train()(imgs, pts, None, depth_points=pts)
        with pytest.raises(_lib.BevfError, match="depth_points without camera_imgs"):
            det(kind).train()(None, pts, None, depth_points=pts)
        with pytest.raises(_lib.BevfError, match="depth_point_counts without depth_points"):
            det(kind).train()(imgs, pts, None, depth_point_counts=counts)
        with pytest.raises(_lib.BevfError, match="no CPU fallback"):                 # accepted on the host, refused only for the device
            det(kind).train()(imgs, pts, None, depth_points=pts, depth_point_counts=counts)
    with pytest.raises(_lib.BevfError, match="depth_points with a detector that has no camera branch"):
        det("frustum", "lidar").train()(None, pts, None, depth_points=pts)           # a detector without a camera branch
    # a camera-only detector may be given points (BEVDepth's setting): refused for the device only
    with pytest.raises(_lib.BevfError, match="no CPU fallback"):
        det("frustum", "camera").train()(imgs, None, None, depth_points=pts)
    # 'lift' still refuses a per-frame calibration, with or without depth_points
    calib = torch.from_numpy(CR.calib_matrices([CR.default_rig()]))
    with pytest.raises(_lib.BevfError, match="camera_calib with camera_view_transform='lift'"):
        det("lift").train()(imgs, pts, None, camera_calib=calib, depth_points=pts)
    with pytest.raises(ValueError, match=r"\(B, N, >= 3\)"):
        det("frustum").train()(imgs, pts, None, depth_points=pts[0])
    # the stand-alone functions
    from bevfusion_multimodal_3d_object_detection_amd import depth_supervision as DS
    with pytest.raises(_lib.BevfError, match="no CPU fallback"):
        DS.depth_targets(pts, [CR.default_rig()], (900, 1600), 4, 6, (32, 1.0, 65.0))
    with pytest.raises(_lib.BevfError, match="no CPU fallback"):
        DS.depth_cross_entropy(torch.zeros(4, 32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="camera_bev.depth"):
        DS.depth_targets(pts, [CR.default_rig()], (900, 1600), 4, 6, (65, 1.0, 65.0))


def test_the_training_tapes_take_the_depth_loss():
    from bevfusion_multimodal_3d_object_detection_amd import training
    assert training._FusionBranchTape.depth_sup is None and training._FusionBranchTape.depth is None
    for cls in (training.CameraFrustumBranchTape, training.CameraLiftBranchTape):
        assert cls._depth_forward is training._FusionBranchTape._depth_forward
    import inspect
    assert "depth_sup" in inspect.signature(training.detector_train_forward).parameters
    sig = inspect.signature(fusion.FlexibleMultiModal3DDetector.forward).parameters
    assert list(sig)[-2:] == ["depth_points", "depth_point_counts"] and sig["depth_points"].default is None
