"""TEST INFRASTRUCTURE -- the camera rigs of the per-frame calibration tests (tests/test_camera_calib_host.py checks their margin
condition on the CPU, tests/test_gpu_camera_calib.py runs them on the MI355X) and the per-frame fp64 oracle."""
import numpy as np
import torch

from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from tests import camera_bev_ref as R

RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
BEV_SIZES = (40, 128, 50, 20)          # every BEV grid the GPU tests build tables on (the margins do not depend on the feature size)


def jittered_rig(seed: int) -> CR.CameraRig:
    """camera_rig.jittered_rig(seed): default_rig() with yaw / pitch / roll +-3 degrees, mounts +-0.3 m, focal lengths +-10 %,
    principal points +-20 px per camera (the benchmark tool times the same rigs)."""
    return CR.jittered_rig(seed)


def frame_rigs(B: int, ncam: int = 6, first_seed: int = 0):
    """B distinct rigs: seeds first_seed, first_seed + 1, ... (the host test covers seeds 0-7), the first ncam cameras."""
    assert first_seed + B <= 8
    return [jittered_rig(first_seed + b).subset(ncam) for b in range(B)]


def sample_margins(rig: CR.CameraRig, S: int, num_heights: int = 8, min_depth: float = 0.1):
    """(smallest distance in px of a sample in front of its camera to an image border line, smallest |depth - min_depth| in m) over
    every (cell, height, camera) sample of the S x S grid, in fp64 through camera_rig.calib_matrices."""
    xs, ys = CR.cell_centres(RANGE, S, S)
    zs = CR.height_centres(RANGE, num_heights)
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    p = np.stack([X.ravel(), Y.ravel(), Z.ravel(), np.ones(X.size)], 0)
    H, W = rig.image_size
    px, dm = np.inf, np.inf
    for M in CR.calib_matrices([rig])[0]:
        a = M @ p
        depth = a[3]
        dm = min(dm, float(np.abs(depth - min_depth).min()))
        front = depth > min_depth
        u, v = a[0, front] / a[2, front], a[1, front] / a[2, front]
        px = min(px, float(np.minimum(np.minimum(np.abs(u), np.abs(u - W)), np.minimum(np.abs(v), np.abs(v - H))).min()))
    return px, dm


def project_frames_ref(feats: torch.Tensor, rigs, S: int) -> torch.Tensor:
    """project_ref frame by frame: feats (B, ncam, C, Hc, Wc), rigs[b] for frame b."""
    return torch.cat([R.project_ref(feats[b:b + 1], rigs[b], RANGE, S, S) for b in range(feats.shape[0])], 0)


def projecting_frames(fusion_ref, rigs):
    """R.projecting with one rig per frame (`fusion_ref.frame_rigs`, replaceable)."""
    base = fusion_ref.forward
    fusion_ref.frame_rigs = list(rigs)

    def forward(camera_features=None, lidar_features=None, radar_features=None):
        if camera_features is not None and fusion_ref.use_camera:
            if camera_features.dim() == 4:
                camera_features = camera_features[:, None]
            camera_features = project_frames_ref(camera_features, fusion_ref.frame_rigs, fusion_ref.bev_h)
        return base(camera_features, lidar_features, radar_features)

    fusion_ref.forward = forward
    return fusion_ref
