"""Drop-in for the reference's `fusion` module (ref src/fusion.py), MI355X-native.

`FlexibleBEVFusion`, `CenterNetHead`, `FlexibleMultiModal3DDetector` and `create_detector`
keep the reference's signatures, attributes, error behaviour and state-dict keys; their
forward passes run on hand-written gfx950 kernels (engine.py -> libbevf_hip.so).
Only the `bev` fusion + `centernet` head path is built: it is the hot path of BASELINE.json.
The attention / late fusion classes and the MLP head (<= 3 tokens, negligible compute,
SURVEY.md section 2 "OUT OF SCOPE") are importable names that raise on construction.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import engine as E
from . import camera_rig as CR
from . import bev_backbone as BB
from . import iou_head as IH
from . import roi_head as RH
from . import seg_head as SH
from . import temporal as T
from .encoders import (MultiRadarEncoder, PillarLiDAREncoder, PointNetLiDAREncoder, ResNetCameraEncoder, SparseLiDAREncoder,  # noqa: F401
                       _cfg, lidar_encoder_kind, load_config)

CANVAS_KINDS = ("pillars", "sparse")          # LiDAR encoders that hand the fusion an NHWC canvas on the BEV grid (lidar_bev)


def _cbr(cin: int, cout: int, k: int) -> List[nn.Module]:
    return [nn.Conv2d(cin, cout, k, padding=k // 2), nn.BatchNorm2d(cout), nn.ReLU(inplace=True)]


class FlexibleBEVFusion(nn.Module):
    """ref src/fusion.py:46-327.

    camera: mean over cameras -> conv3x3+BN+ReLU -> conv1x1+BN+ReLU -> bilinear to (bev_h,bev_w)
    lidar : Linear-ReLU-Linear to a 128x25x25 canvas -> conv -> x2 bilinear -> conv (50x50)
    radar : Linear-ReLU, broadcast to every cell, 2 x conv3x3+BN+ReLU
    concat [camera, lidar, radar] -> 2 x conv3x3+BN+ReLU.
    Extension: for bev sizes other than 50x50 -- where the reference raises at the
    concat -- the LiDAR map is bilinearly resized like the camera map; the identity at 50x50.
    Extension (opt-in, lidar_encoder_type / model.lidar_encoder.type 'PointPillars'): the LiDAR input is the pillar
    canvas (B, pfn_channels, bev_h, bev_w), already on the fusion grid, and the branch is
    lidar_bev = conv3x3(pfn_channels -> 128)+BN+ReLU -> conv3x3(128 -> bev_channels)+BN+ReLU (no lidar_init / lidar_upsample).
    Extension (opt-in, camera_view_transform / model.bev_fusion.camera_view_transform 'project'): the camera
    features of every camera are projected onto the BEV grid through a fixed camera rig (camera_rig.py: num_heights points above
    each cell, bilinear samples averaged over those that hit an image), and camera_proj -- same modules and keys -- runs on the BEV
    grid after the projection, with no resize.  The module's rig (set_camera_rig) serves every frame unless the forward gets
    `camera_calib=`: one CameraRig per frame, or the fp64 (B, ncam, 4, 4) tensor of camera_rig.calib_matrices (host or device) --
    then every frame is lifted through its own table, built on the device inside the step.
    Extension (opt-in, camera_view_transform 'lift'): the same samples with a learned per-pixel depth distribution
    deciding where along its ray a feature lands -- depth_net = Conv2d(camera_channels, D, 1) (this mode's only extra parameters),
    softmax over the D uniform depth bins of model.bev_fusion.camera_bev.depth, and every sample weighted by the probability of the
    bin its depth falls into; camera_proj on the BEV grid as in 'project'.  fp32 storage and the module's static rig only.
    Extension (opt-in, camera_view_transform 'frustum'): lift-splat (Philion & Fidler 2020) -- the same depth_net
    and softmax, but every (feature pixel, depth bin) is a point of its camera's frustum at the bin's centre depth, unprojected
    through the calibration into the BEV cell it falls in, and a cell is the plain sum of Pd * feature over its points; camera_proj
    on the BEV grid.  The frustum is a function of the calibration, so `camera_calib=` works as in 'project' (and takes what
    augment.augment_batch returns); the module's rig serves every frame otherwise.  The calibration's third row must be its depth
    row, as camera_rig.calib_matrices and augment.augmented_calib make it.  camera_bev.num_heights is unused.  fp32 storage only.
    Extension (opt-in, temporal=True / model.bev_fusion.temporal.enable): a fourth concat slot after radar holds the
    previous frame's fused map `prev_bev`, resampled onto the current grid through `ego_motion` (temporal.py, csrc/bev_warp.hip);
    bev_fusion's first conv then has bev_channels more input channels, and there are no other new parameters.  prev_bev=None is the
    first frame of a sequence: the slot is zeros.
    """

    def __init__(self, use_camera: Optional[bool] = None, use_lidar: Optional[bool] = None,
                 use_radar: Optional[bool] = None, camera_channels: Optional[int] = None,
                 lidar_channels: Optional[int] = None, radar_channels: Optional[int] = None,
                 bev_h: Optional[int] = None, bev_w: Optional[int] = None, bev_channels: Optional[int] = None,
                 pc_range: Optional[List[float]] = None, config: Optional[Dict] = None,
                 config_path: Optional[str] = None, lidar_encoder_type: Optional[str] = None,
                 camera_view_transform: Optional[str] = None, temporal: Optional[bool] = None):
        super().__init__()
        config = _cfg(config, config_path)
        default_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
        self.temporal = T.temporal_enabled(temporal, config)    # a fourth concat slot: the previous fused map, warped by ego-motion
        self.lidar_kind = lidar_encoder_kind(lidar_encoder_type, config)
        # camera branch: 'mean' (the reference's camera average + resize), 'project' (camera rig -> BEV grid), 'lift' (+ learned depth)
        # or 'frustum' (lift-splat: learned depth, push to the cell of the frustum point)
        self.camera_view_transform = CR.view_transform_kind(camera_view_transform, config)
        self.cam_num_heights, self.cam_min_depth, self._camera_rig = CR.DEFAULT_NUM_HEIGHTS, CR.DEFAULT_MIN_DEPTH, None
        if self.camera_view_transform in ("project", "lift", "frustum"):
            self.cam_num_heights, self.cam_min_depth, self._camera_rig = CR.camera_bev_settings(config)
        if self.camera_view_transform in ("lift", "frustum"):   # (depth bins D, depth_min, depth_max) of the learned depth distribution
            self.cam_depth = CR.camera_lift_settings(config, self.cam_min_depth)
        pillars = self.lidar_kind in CANVAS_KINDS              # the LiDAR input is a canvas on the BEV grid: lidar_bev, no lidar_init
        if config is not None:
            mc = config.get("model", {})
            bc, dc = mc.get("bev_fusion", {}), config.get("dataset", {})
            self.use_camera = mc.get("use_camera", True) if use_camera is None else use_camera
            self.use_lidar = mc.get("use_lidar", True) if use_lidar is None else use_lidar
            self.use_radar = mc.get("use_radar", True) if use_radar is None else use_radar
            if camera_channels is None:
                camera_channels = mc.get("camera_encoder", {}).get("output_channels", 512)
            if lidar_channels is None:
                le = mc.get("lidar_encoder", {}) or {}
                if self.lidar_kind == "sparse":
                    lidar_channels = int(tuple(le.get("channels", (32, 64, 128)))[-1]) * int(le.get("z_voxels", 8)) // 4
                else:
                    lidar_channels = le.get("pfn_channels", 64) if pillars else le.get("feature_dim", 1024)
            if radar_channels is None:
                radar_channels = mc.get("radar_encoder", {}).get("feature_dim", 256)
            self.bev_h = bc.get("bev_h", dc.get("bev_h", 200)) if bev_h is None else bev_h
            self.bev_w = bc.get("bev_w", dc.get("bev_w", 200)) if bev_w is None else bev_w
            self.bev_channels = bc.get("bev_channels", 256) if bev_channels is None else bev_channels
            self.pc_range = dc.get("point_cloud_range", default_range) if pc_range is None else pc_range
        else:
            self.use_camera = True if use_camera is None else use_camera
            self.use_lidar = True if use_lidar is None else use_lidar
            self.use_radar = True if use_radar is None else use_radar
            camera_channels = 512 if camera_channels is None else camera_channels
            lidar_channels = {"pillars": 64, "sparse": 256}.get(self.lidar_kind, 1024) if lidar_channels is None else lidar_channels
            radar_channels = 256 if radar_channels is None else radar_channels
            self.bev_h = 200 if bev_h is None else bev_h
            self.bev_w = 200 if bev_w is None else bev_w
            self.bev_channels = 256 if bev_channels is None else bev_channels
            self.pc_range = default_range if pc_range is None else pc_range
        self.num_modalities = sum([self.use_camera, self.use_lidar, self.use_radar])
        assert self.num_modalities > 0, "At least one modality must be enabled"
        bevc = self.bev_channels
        if self.use_camera:
            self.camera_proj = nn.Sequential(*_cbr(camera_channels, 512, 3), *_cbr(512, bevc, 1))
            if self.camera_view_transform in ("lift", "frustum"):   # per-pixel depth logits; these modes only (state-dict keys)
                self.depth_net = nn.Conv2d(camera_channels, self.cam_depth[0], 1)
        if self.use_lidar and pillars:
            self.lidar_bev = nn.Sequential(*_cbr(lidar_channels, 128, 3), *_cbr(128, bevc, 3))
        elif self.use_lidar:
            hidden, start = 128, 25
            self.lidar_init = nn.Sequential(nn.Linear(lidar_channels, 512), nn.ReLU(inplace=True),
                                            nn.Linear(512, hidden * start * start))
            self.lidar_upsample = nn.Sequential(
                *_cbr(hidden, hidden, 3), nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False),
                *_cbr(hidden, bevc, 3))
            self.lidar_start_size = start
        if self.use_radar:
            self.radar_proj = nn.Sequential(nn.Linear(radar_channels, bevc), nn.ReLU(inplace=True))
            self.radar_refine = nn.Sequential(*_cbr(bevc, bevc, 3), *_cbr(bevc, bevc, 3))
        self.bev_fusion = nn.Sequential(*_cbr(bevc * (self.num_modalities + int(self.temporal)), bevc * 2, 3), *_cbr(bevc * 2, bevc, 3))
        self._engine = None

    def _eng(self) -> E.FusionEngine:
        if self._engine is None:
            self._engine = E.FusionEngine(self)
        return self._engine

    @property
    def camera_rig(self) -> CR.CameraRig:
        """The rig of the 'project' / 'lift' / 'frustum' camera branch (camera_rig.default_rig() unless set)."""
        if self._camera_rig is None:
            self._camera_rig = CR.default_rig()
        return self._camera_rig

    def set_camera_rig(self, rig: "CR.CameraRig") -> None:
        """Replace the camera rig of the 'project' / 'lift' / 'frustum' branch; its projection tables are rebuilt on next use (outside a graph capture:
        re-capture a GraphedDetector after a rig change).  The rig is fixed for every frame until the next call."""
        if not isinstance(rig, CR.CameraRig):
            raise TypeError(f"set_camera_rig: expected a camera_rig.CameraRig, got {type(rig).__name__}")
        self._camera_rig = rig
        if self._engine is not None:
            self._engine.drop_camera_tables()

    def camera_calib_tensor(self, camera_calib, B: int, ncam: int):
        """Check a `camera_calib=` argument against B frames of ncam cameras -> (fp64 (B, ncam, 4, 4) tensor where the caller put
        it -- host or device --, image_size), or None for None.  A sequence of CameraRig carries its own image_size; a tensor (as
        camera_rig.calib_matrices makes it) refers to the module rig's."""
        if camera_calib is None:
            return None
        self.check_lift_supported(camera_calib)
        if self.camera_view_transform not in ("project", "frustum"):
            raise E.L.BevfError("camera_calib needs camera_view_transform='project': the 'mean' camera branch uses no calibration")
        if not B:                                                        # no camera input: nothing to calibrate
            return None
        if isinstance(camera_calib, torch.Tensor):
            if camera_calib.dtype != torch.float64:
                raise E.L.BevfError(f"camera_calib must be float64 (camera_rig.calib_matrices), got {camera_calib.dtype}")
            t, image_size = camera_calib, self.camera_rig.image_size
        else:
            rigs = list(camera_calib)
            t = torch.from_numpy(CR.calib_matrices(rigs))
            image_size = rigs[0].image_size
        if tuple(t.shape) != (B, ncam, 4, 4):
            raise ValueError(f"camera_calib holds {tuple(t.shape)}: expected one calibration per frame and camera, "
                             f"({B}, {ncam}, 4, 4)")
        return t, image_size

    def check_lift_supported(self, camera_calib=None) -> None:
        """The 'lift' branch runs the module's static rig in fp32 storage only; raises BevfError for what it does not support."""
        if self.camera_view_transform != "lift" or not self.use_camera:
            return
        if camera_calib is not None:
            raise E.L.BevfError("camera_calib with camera_view_transform='lift' is not supported: the learned-depth lift uses the "
                                "module's static rig (set_camera_rig); per-frame calibration needs camera_view_transform='project'")
        if self.depth_net.weight.dtype != torch.float32:
            raise E.L.BevfError(f"{self.depth_net.weight.dtype} storage with camera_view_transform='lift' is not supported: the "
                                "learned-depth lift kernels are fp32 only (bf16 models: camera_view_transform='project' or 'mean')")

    def check_frustum_supported(self) -> None:
        """The 'frustum' branch runs in fp32 storage only; raises BevfError otherwise."""
        if self.camera_view_transform == "frustum" and self.use_camera and self.depth_net.weight.dtype != torch.float32:
            raise E.L.BevfError(f"{self.depth_net.weight.dtype} storage with camera_view_transform='frustum' is not supported: the "
                                "lift-splat kernels are fp32 only (bf16 models: camera_view_transform='project' or 'mean')")

    def forward_nhwc(self, cam_nhwc, cam_geom, lidar_features, radar_features, camera_calib=None, history=None):
        """Internal fast path on NHWC camera features (no layout change); camera_calib as camera_calib_tensor returns it, history as
        temporal.check_history returns it."""
        if history is None:                                              # (the call every model without temporal fusion makes)
            return self._eng().run(cam_nhwc, cam_geom, lidar_features, radar_features, camera_calib)
        return self._eng().run(cam_nhwc, cam_geom, lidar_features, radar_features, camera_calib, history)

    def history(self, prev_bev, ego_motion, *inputs):
        """`prev_bev=` / `ego_motion=` checked against the first input that is there (temporal.check_history)."""
        first = next((t[0] if isinstance(t, (list, tuple)) else t for t in inputs if t is not None), None)
        if first is None or not (self.temporal or prev_bev is not None or ego_motion is not None):
            return None                                                  # (no input: the forward raises "No modality features provided")
        return T.check_history(self, prev_bev, ego_motion, first.shape[0], first.device, self._eng().dtype)

    def forward(self, camera_features: Optional[torch.Tensor] = None, lidar_features: Optional[torch.Tensor] = None,
                radar_features: Optional[torch.Tensor] = None, camera_calib=None, prev_bev: Optional[torch.Tensor] = None,
                ego_motion=None) -> torch.Tensor:
        """camera_calib ('project' and 'frustum' branches): per-frame calibration -- a sequence of B camera_rig.CameraRig or the
        float64 (B, ncam, 4, 4) tensor of camera_rig.calib_matrices; None = the module's rig for every frame.
        prev_bev / ego_motion (temporal=True): the previous frame's fused map (B, bev_channels, bev_h, bev_w) in the storage dtype
        and the float64 (B, 4, 4) current -> previous frame map of temporal.ego_motion (host or device); prev_bev None = the first
        frame of a sequence (a zero history slot; a mixed batch passes zeros for the frames that start one)."""
        self.check_lift_supported(camera_calib)
        self.check_frustum_supported()
        history = self.history(prev_bev, ego_motion, camera_features if self.use_camera else None,
                               lidar_features if self.use_lidar else None, radar_features if self.use_radar else None)
        if camera_calib is not None:
            cf = camera_features if self.use_camera else None
            camera_calib = self.camera_calib_tensor(camera_calib, 0 if cf is None else cf.shape[0],
                                                    0 if cf is None else (cf.shape[1] if cf.dim() == 5 else 1))
        E.require_cuda(camera_features, lidar_features, radar_features)
        if self.training:
            from . import training
            if training.wants_train_path(self):         # used outside the detector in train mode: batch statistics + gradients
                if history is not None:
                    return training.fusion_train_forward(self, camera_features, lidar_features, radar_features, camera_calib, history)
                return training.fusion_train_forward(self, camera_features, lidar_features, radar_features, camera_calib)
        with torch.no_grad():
            if history is not None:
                E.require_cuda(history[0])
                return self._forward_eval(camera_features, lidar_features, radar_features, camera_calib, history)
            return self._forward_eval(camera_features, lidar_features, radar_features, camera_calib)

    def _forward_eval(self, camera_features, lidar_features, radar_features, camera_calib=None, history=None) -> torch.Tensor:
        cam_nhwc = cam_geom = None
        if self.use_camera and camera_features is not None:
            x = camera_features.float()
            if x.dim() == 5:
                B, n, Cc, H, W = x.shape
                cam_nhwc, cam_geom = E.to_nhwc(x.reshape(B * n, Cc, H, W)).to(self._eng().dtype), (B, n, H, W)
            else:
                B, Cc, H, W = x.shape
                cam_nhwc, cam_geom = E.to_nhwc(x).to(self._eng().dtype), (B, 1, H, W)
        lid = lidar_features.float() if lidar_features is not None else None
        if lid is not None and self.lidar_kind in CANVAS_KINDS and self.use_lidar:
            B, Cc, H, W = lid.shape                                       # NCHW canvas -> the engine's NHWC storage
            lid = E.to_nhwc(lid).to(self._eng().dtype).view(B, H, W, Cc)
        out, B = self.forward_nhwc(cam_nhwc, cam_geom, lid,
                                   radar_features.float() if radar_features is not None else None, camera_calib, history)
        return E.to_nchw(out, B, self.bev_channels, self.bev_h, self.bev_w)

    def get_config_str(self) -> str:
        return "+".join(n for n, u in (("camera", self.use_camera), ("lidar", self.use_lidar),
                                       ("radar", self.use_radar)) if u)

    def count_parameters(self) -> Dict[str, int]:
        cnt = lambda m: sum(p.numel() for p in m.parameters())
        out = {}
        if self.use_camera:
            out["camera_proj"] = cnt(self.camera_proj)
        if self.use_lidar and self.lidar_kind in CANVAS_KINDS:
            out["lidar_bev"] = cnt(self.lidar_bev)
            out["lidar_total"] = out["lidar_bev"]
        elif self.use_lidar:
            out["lidar_init"], out["lidar_upsample"] = cnt(self.lidar_init), cnt(self.lidar_upsample)
            out["lidar_total"] = out["lidar_init"] + out["lidar_upsample"]
        if self.use_radar:
            out["radar_proj"], out["radar_refine"] = cnt(self.radar_proj), cnt(self.radar_refine)
            out["radar_total"] = out["radar_proj"] + out["radar_refine"]
        out["bev_fusion"] = cnt(self.bev_fusion)
        out["total"] = cnt(self)
        return out


class _OutOfScope(nn.Module):
    _what = ""

    def __init__(self, *a, **k):
        super().__init__()
        raise NotImplementedError(
            f"{type(self).__name__}: {self._what} is outside the accelerated hot path of this build "
            "(SURVEY.md section 2: <= 3 tokens, negligible compute); use fusion_type='bev' with detection_head='centernet'.")


class SpatialReshaper(_OutOfScope):
    _what = "the broadcast reshaper of the attention path (ref src/fusion.py:333-372)"


class CrossModalAttention(_OutOfScope):
    _what = "cross-modal attention (ref src/fusion.py:375-470)"


class FlexibleAttentionFusion(_OutOfScope):
    _what = "attention fusion (ref src/fusion.py:473-650)"


class FlexibleLateFusion(_OutOfScope):
    _what = "late fusion (ref src/fusion.py:653-781)"


class MLPDetectionHead(_OutOfScope):
    _what = "the MLP head of the non-spatial fusions (ref src/fusion.py:886-939)"


class CenterNetHead(nn.Module):
    """ref src/fusion.py:788-884.  Five branches conv3x3(+bias)+ReLU+conv1x1; sigmoid on the heatmap inside
    the head.  Init: weights N(0, 0.001), biases 0, heatmap bias -ln 99 (ref :858-867)."""

    def __init__(self, in_channels: Optional[int] = None, num_classes: Optional[int] = None,
                 head_conv: Optional[int] = None, config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            hc = config.get("model", {}).get("centernet_head", {})
            in_channels = hc.get("in_channels", 256) if in_channels is None else in_channels
            self.num_classes = config.get("dataset", {}).get("num_classes", 10) if num_classes is None else num_classes
            head_conv = hc.get("head_conv", 64) if head_conv is None else head_conv
        else:
            in_channels = 256 if in_channels is None else in_channels
            self.num_classes = 10 if num_classes is None else num_classes
            head_conv = 64 if head_conv is None else head_conv
        for name, c in zip(E.HEAD_BRANCHES, (self.num_classes, 2, 3, 2, 2)):
            setattr(self, f"{name}_head", nn.Sequential(nn.Conv2d(in_channels, head_conv, 3, padding=1, bias=True),
                                                        nn.ReLU(inplace=True), nn.Conv2d(head_conv, c, 1, bias=True)))
        self._init_weights()
        self._engine = None

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.001)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.heatmap_head[-1].bias, -math.log((1 - 0.01) / 0.01))

    def _eng(self) -> E.HeadEngine:
        if self._engine is None:
            self._engine = E.HeadEngine(self)
        return self._engine

    def forward_nhwc(self, bev_nhwc: torch.Tensor, B: int, H: int, W: int) -> Dict[str, torch.Tensor]:
        return self._eng().run(bev_nhwc, B, H, W)

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        E.require_cuda(x)
        if self.training and torch.is_grad_enabled() and self._eng().dtype == torch.float32 \
                and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            from . import training                      # no BatchNorm in the head: same values as eval mode, plus a gradient path
            return training.head_train_forward(self, x)
        with torch.no_grad():
            B, _, H, W = x.shape
            return self.forward_nhwc(E.to_nhwc(x.float()).to(self._eng().dtype), B, H, W)


def _any_bn_training(module: nn.Module) -> bool:
    return any(isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training for m in module.modules())


class FlexibleMultiModal3DDetector(nn.Module):
    """ref src/fusion.py:946-1141.  `model(camera_imgs, lidar_points, radar_points)` -> dict of
    heatmap (B,C,H,W post-sigmoid), offset, size, rot, vel.  `None` inputs are skipped."""

    def __init__(self, use_camera: Optional[bool] = None, use_lidar: Optional[bool] = None,
                 use_radar: Optional[bool] = None, num_classes: Optional[int] = None,
                 fusion_type: Optional[str] = None, detection_head: Optional[str] = None,
                 bev_h: Optional[int] = None, bev_w: Optional[int] = None, config: Optional[Dict] = None,
                 config_path: Optional[str] = None, lidar_encoder_type: Optional[str] = None,
                 camera_view_transform: Optional[str] = None, temporal: Optional[bool] = None, seg_head=None,
                 iou_head=None, bev_backbone=None, roi_head=None):
        super().__init__()
        config = _cfg(config, config_path)
        # LiDAR branch: 'PointPillars' / 'pillars' (any case) from the keyword, else model.lidar_encoder.type -> the pillar
        # encoder + lidar_bev; anything else -> the reference's PointNet + lidar_init / lidar_upsample
        # 'SparseVoxel' / 'sparse' / 'SECOND' -> the sparse-voxel encoder + lidar_bev
        self.lidar_encoder_type = dict(pillars="PointPillars", sparse="SparseVoxel", pointnet="PointNet")[
            lidar_encoder_kind(lidar_encoder_type, config)]
        if config is not None:
            mc, dc = config.get("model", {}), config.get("dataset", {})
            self.use_camera = mc.get("use_camera", True) if use_camera is None else use_camera
            self.use_lidar = mc.get("use_lidar", True) if use_lidar is None else use_lidar
            self.use_radar = mc.get("use_radar", True) if use_radar is None else use_radar
            num_classes = dc.get("num_classes", 10) if num_classes is None else num_classes
            self.fusion_type = mc.get("fusion_type", "bev") if fusion_type is None else fusion_type
            self.detection_head_type = mc.get("detection_head", "centernet") if detection_head is None else detection_head
            bev_h = dc.get("bev_h", 50) if bev_h is None else bev_h
            bev_w = dc.get("bev_w", 50) if bev_w is None else bev_w
        else:
            self.use_camera = True if use_camera is None else use_camera
            self.use_lidar = True if use_lidar is None else use_lidar
            self.use_radar = True if use_radar is None else use_radar
            num_classes = 10 if num_classes is None else num_classes
            self.fusion_type = "bev" if fusion_type is None else fusion_type
            self.detection_head_type = "centernet" if detection_head is None else detection_head
            bev_h = 50 if bev_h is None else bev_h
            bev_w = 50 if bev_w is None else bev_w
        assert sum([self.use_camera, self.use_lidar, self.use_radar]) > 0, "At least one modality must be enabled"
        if self.use_camera:
            self.camera_encoder = (ResNetCameraEncoder(config=config) if config is not None
                                   else ResNetCameraEncoder(backbone="resnet18", pretrained=False))
        pillars = self.lidar_encoder_type == "PointPillars"
        if self.use_lidar and pillars:
            self.lidar_encoder = (PillarLiDAREncoder(bev_h=bev_h, bev_w=bev_w, config=config) if config is not None
                                  else PillarLiDAREncoder(input_channels=4, bev_h=bev_h, bev_w=bev_w))
        elif self.use_lidar and self.lidar_encoder_type == "SparseVoxel":
            self.lidar_encoder = (SparseLiDAREncoder(bev_h=bev_h, bev_w=bev_w, config=config) if config is not None
                                  else SparseLiDAREncoder(input_channels=4, bev_h=bev_h, bev_w=bev_w))
        elif self.use_lidar:
            self.lidar_encoder = (PointNetLiDAREncoder(config=config) if config is not None
                                  else PointNetLiDAREncoder(input_channels=4, feat_dim=1024))
        if self.use_radar:
            self.radar_encoder = (MultiRadarEncoder(config=config) if config is not None
                                  else MultiRadarEncoder(input_channels=7, feat_dim=256, num_radars=5))
        if self.fusion_type == "bev":
            extra = dict(lidar_encoder_type=self.lidar_encoder_type, camera_view_transform=camera_view_transform)
            if temporal is not None:                      # (None: the fusion reads model.bev_fusion.temporal.enable itself)
                extra["temporal"] = temporal
            if self.use_lidar and pillars:
                extra["lidar_channels"] = self.lidar_encoder.pfn_channels
            elif self.use_lidar and self.lidar_encoder_type == "SparseVoxel":
                extra["lidar_channels"] = self.lidar_encoder.out_channels
            self.fusion = FlexibleBEVFusion(use_camera=self.use_camera, use_lidar=self.use_lidar,
                                            use_radar=self.use_radar, bev_h=bev_h, bev_w=bev_w, config=config, **extra)
        elif self.fusion_type == "attention":
            self.fusion = FlexibleAttentionFusion()
        elif self.fusion_type == "late":
            self.fusion = FlexibleLateFusion()
        else:
            raise ValueError(f"Unknown fusion type: {self.fusion_type}")
        # opt-in decoder between the fuser and every head: bev_backbone=True / dict, or model.bev_backbone.enable;
        # adds the keys bev_backbone.{backbone.blocks,neck.deblocks}.* and widens the heads' first convolutions, nothing else
        self.bev_backbone = None
        head_channels = self.fusion.bev_channels
        bb = BB.bev_backbone_settings(bev_backbone, config)
        if bb is not None:
            if self.fusion_type != "bev":
                raise E.L.BevfError("bev_backbone needs the 'bev' fusion")
            self.bev_backbone = BB.BEVBackbone(in_channels=self.fusion.bev_channels, **bb)
            self.bev_backbone.check_grid(self.fusion.bev_h, self.fusion.bev_w)
            head_channels = self.bev_backbone.out_channels
        if self.detection_head_type == "centernet":
            self.det_head = CenterNetHead(in_channels=head_channels, num_classes=num_classes, config=config)
        else:
            self.det_head = MLPDetectionHead()
        # opt-in second task on the fused map: seg_head=True / dict, or model.seg_head.enable; adds the keys
        # seg_head.classifier.* and the 'seg' output, nothing else
        self.seg_head = None
        seg = SH.seg_head_settings(seg_head, config)
        if seg is not None:
            self.seg_head = SH.BEVSegmentationHead(in_channels=head_channels, pc_range=self.fusion.pc_range,
                                                   bev_h=self.fusion.bev_h, bev_w=self.fusion.bev_w, **seg)
        # opt-in IoU-aware head on the fused map: iou_head=True / dict, or model.iou_head.enable; adds the keys
        # iou_head.branch.{0,2}.{weight,bias} and the 'iou' output, nothing else
        self.iou_head = None
        iou = IH.iou_head_settings(iou_head, config)
        if iou is not None:
            self.iou_head = IH.IoUHead(in_channels=head_channels, config=config, **iou)
        # opt-in second stage: roi_head=True / dict, or model.roi_head.enable; adds the keys roi_head.{shared_fc,
        # cls_out,reg_out}.* and the 'feat' output (the map the heads read), nothing else
        self.roi_head = None
        roi = RH.roi_head_settings(roi_head, config)
        if roi is not None:
            if self.fusion_type != "bev":
                raise E.L.BevfError("roi_head needs the 'bev' fusion")
            self.roi_head = RH.RoIHead(in_channels=head_channels, pc_range=self.fusion.pc_range, config=config, **roi)

    def camera_calib_tensor(self, camera_imgs, camera_calib):
        """`camera_calib=` of forward checked against the camera input (FlexibleBEVFusion.camera_calib_tensor); None without
        camera images."""
        if camera_calib is None:
            return None
        if not hasattr(self.fusion, "camera_calib_tensor"):
            raise E.L.BevfError("camera_calib needs the 'bev' fusion with camera_view_transform='project'")
        if not self.use_camera or camera_imgs is None:
            return self.fusion.camera_calib_tensor(camera_calib, 0, 0)             # None ('mean' still raises)
        return self.fusion.camera_calib_tensor(camera_calib, camera_imgs.shape[0], camera_imgs.shape[1] if camera_imgs.dim() == 5 else 1)

    def _depth_supervision(self, camera_imgs, depth_points, depth_point_counts):
        """`depth_points=` / `depth_point_counts=` of forward -> (points, counts), or None without them.  Raises BevfError for every
        combination the depth loss is not built for; the tensors themselves are checked by depth_supervision.check_points."""
        if depth_points is None:
            if depth_point_counts is not None:
                raise E.L.BevfError("depth_point_counts without depth_points: the counts say how many rows of depth_points are valid")
            return None
        if not self.use_camera:
            raise E.L.BevfError("depth_points with a detector that has no camera branch is not supported: there are no depth logits "
                                "to supervise")
        kind = getattr(self.fusion, "camera_view_transform", None)
        if kind not in ("frustum", "lift"):
            raise E.L.BevfError(f"depth_points with camera_view_transform={kind!r} is not supported: LiDAR depth supervision needs the "
                                "learned depth distribution of camera_view_transform='frustum' or 'lift'")
        if self.fusion.depth_net.weight.dtype != torch.float32:
            raise E.L.BevfError(f"depth_points with {self.fusion.depth_net.weight.dtype} storage is not supported: the depth loss "
                                "kernels are fp32 only")
        if camera_imgs is None:
            raise E.L.BevfError("depth_points without camera_imgs: there are no depth logits to supervise")
        if not (self.training and (torch.is_grad_enabled() or _any_bn_training(self))):
            raise E.L.BevfError("depth_points in eval mode is not supported: the depth loss is part of the training step (a validation "
                                "depth loss: depth_supervision.depth_targets and depth_cross_entropy on depth_net's logits)")
        return depth_points, depth_point_counts

    def forward(self, camera_imgs: Optional[torch.Tensor] = None, lidar_points: Optional[torch.Tensor] = None,
                radar_points: Optional[List[torch.Tensor]] = None, camera_calib=None, prev_bev: Optional[torch.Tensor] = None,
                ego_motion=None, depth_points: Optional[torch.Tensor] = None,
                depth_point_counts: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """prev_bev / ego_motion (temporal=True): the 'bev' output of the previous frame and the float64 (B, 4, 4)
        current -> previous frame map of temporal.ego_motion (host or device); prev_bev None = the first frame of a sequence.  A model
        with temporal fusion returns 'bev' as well: an owned (B, bev_channels, H, W) channels-last copy of the fused map (detached in
        train mode, where the history is a constant), to hand back as prev_bev for the next frame.
        A model built with seg_head= returns 'seg' as well, in eval and train mode: the map-segmentation logits
        (B, num_classes, Ho, Wo) in fp32 of seg_head.BEVSegmentationHead on the fused map.
        A model built with iou_head= returns 'iou' as well, in eval and train mode: the (B, 1, H, W) fp32 map of
        iou_head.IoUHead, 2 * IoU - 1 of the box regressed at each cell (iou_aware.IoUAwareLoss, the decode's iou_rectify=).
        A model built with roi_head= returns 'feat' as well, in eval and train mode: an owned (B, C, H, W)
        channels-last copy of the map the heads read (the neck's concat with a bev_backbone, else the fused map), detached in train
        mode -- the input of roi_head.RoIHead and of `refine`.
        camera_calib (camera_view_transform='project' or 'frustum'): per-frame camera calibration -- a sequence of B
        camera_rig.CameraRig, or the float64 (B, ncam, 4, 4) tensor of camera_rig.calib_matrices (host or device); None = the
        fusion's rig for every frame.
        depth_points (train mode, camera_view_transform='frustum' or 'lift'): fp32 (B, N, >= 3) LiDAR points on the
        device in the frame of point_cloud_range -- usually lidar_points itself, though a camera-only detector may be given them
        too --, depth_point_counts (B,) their valid rows per frame (None: all; all-zero rows are padding either way).  The result
        then also holds 'depth_loss', the mean cross entropy of depth_net's logits against the nearest LiDAR return's depth bin
        under the step's calibration (differentiable, add w * depth_loss to the training loss), and 'depth_pixels', the number of
        feature pixels that had a return."""
        depth_sup = self._depth_supervision(camera_imgs, depth_points, depth_point_counts)
        camera_calib = self.camera_calib_tensor(camera_imgs, camera_calib)
        if hasattr(self.fusion, "check_lift_supported"):
            self.fusion.check_lift_supported()
            self.fusion.check_frustum_supported()
        if depth_sup is not None:
            from . import depth_supervision
            depth_sup = depth_supervision.check_points(*depth_sup)
        history = self._history(camera_imgs, lidar_points, radar_points, prev_bev, ego_motion)
        if self.training and (torch.is_grad_enabled() or _any_bn_training(self)):
            # under no_grad a train-mode model still normalises with batch statistics and updates the running buffers, as torch does
            from . import training                      # train-mode BN + tape + hand-written backward (training.py)
            E.require_cuda(camera_imgs, lidar_points)
            if history is not None:
                return training.detector_train_forward(self, camera_imgs, lidar_points, radar_points, camera_calib, depth_sup, history)
            if depth_sup is not None:
                return training.detector_train_forward(self, camera_imgs, lidar_points, radar_points, camera_calib, depth_sup)
            return training.detector_train_forward(self, camera_imgs, lidar_points, radar_points, camera_calib)
        with torch.no_grad():
            if history is not None:
                return self._forward_inference(camera_imgs, lidar_points, radar_points, camera_calib, history)
            return self._forward_inference(camera_imgs, lidar_points, radar_points, camera_calib)

    def _history(self, camera_imgs, lidar_points, radar_points, prev_bev, ego_motion):
        """`prev_bev=` / `ego_motion=` of forward -> what FlexibleBEVFusion.history makes of them: None for a model without temporal
        fusion (either argument then raises), else the (prev_bev, ego, host ego) triple."""
        if not hasattr(self.fusion, "history"):
            if prev_bev is not None or ego_motion is not None:
                raise E.L.BevfError("prev_bev / ego_motion need the 'bev' fusion built with temporal=True")
            return None
        history = self.fusion.history(prev_bev, ego_motion, camera_imgs if self.use_camera else None,
                                      lidar_points if self.use_lidar else None, radar_points if self.use_radar else None)
        if history is not None and history[0] is not None:
            if self.training:                           # inside the detector the history is a constant of the step
                from .training import _no_input_grad
                _no_input_grad(history[0], "the history BEV map (prev_bev)")
            E.require_cuda(history[0])
        return history

    def _forward_inference(self, camera_imgs, lidar_points, radar_points, camera_calib=None, history=None) -> Dict[str, torch.Tensor]:
        cam = geom = lid = rad = None
        if self.use_camera and camera_imgs is not None:
            cam, geom = self.camera_encoder.forward_nhwc(camera_imgs)       # stays NHWC: no layout change
        if self.use_lidar and lidar_points is not None:
            if getattr(self.lidar_encoder, "is_pillars", False) or getattr(self.lidar_encoder, "is_sparse", False):
                lid = self.lidar_encoder.forward_nhwc(lidar_points)            # NHWC canvas on the fusion grid
            else:
                lid = self.lidar_encoder._forward_eval(lidar_points)
        if self.use_radar and radar_points is not None:
            rad = self.radar_encoder._forward_eval(radar_points)
        if history is None and self.seg_head is None and self.iou_head is None and self.bev_backbone is None and self.roi_head is None:
            fused, B = self.fusion.forward_nhwc(cam, geom, lid, rad, camera_calib if cam is not None else None)
            return self.det_head.forward_nhwc(fused, B, self.fusion.bev_h, self.fusion.bev_w)
        fus = self.fusion
        fused, B = fus.forward_nhwc(cam, geom, lid, rad, camera_calib if cam is not None else None, history)
        feat = fused                                                    # what the heads read: the decoder's concat when there is one
        if self.bev_backbone is not None:
            feat = self.bev_backbone.forward_nhwc(fused, B, fus.bev_h, fus.bev_w)
        out = self.det_head.forward_nhwc(feat, B, fus.bev_h, fus.bev_w)
        if self.seg_head is not None:                                   # the fused map's second consumer
            out["seg"] = self.seg_head.forward_nhwc(feat, B)
        if self.iou_head is not None:                                   # and the IoU-aware head
            out["iou"] = self.iou_head.forward_nhwc(feat, B, fus.bev_h, fus.bev_w)
        if history is not None:
            out["bev"] = T.own_bev(fused, B, fus.bev_h, fus.bev_w, fus.bev_channels)   # (the engine reuses its buffer: an owned copy)
        if self.roi_head is not None:                                   # the second stage's input, owned like 'bev'
            out["feat"] = T.own_bev(feat, B, fus.bev_h, fus.bev_w, self.roi_head.in_channels)
        return out

    def refine(self, out: Dict[str, torch.Tensor], *, refine_score_thresh: float = 0.0, **decode_keywords) -> Dict[str, torch.Tensor]:
        """The second stage on the forward's outputs (a model built with roi_head=):
        centernet_target.decode_padded(out, **decode_keywords) -> roi_head(out['feat'], rois) -> roi_refine.refine_padded(rois,
        head_out, refine_score_thresh) -> the final padded records, with nothing read back.  (score_thresh among the decode keywords
        is the first stage's threshold.)"""
        if self.roi_head is None:
            raise E.L.BevfError("refine needs a detector built with roi_head=True")
        if "feat" not in out:
            raise E.L.BevfError("refine: the outputs lack 'feat' (pass the dict the forward of this model returned)")
        from .centernet_target import decode_padded
        from .roi_refine import refine_padded
        with torch.no_grad():
            rois = decode_padded(out, **decode_keywords)
            return refine_padded(rois, self.roi_head(out["feat"], rois), refine_score_thresh)

    def get_config_str(self) -> str:
        return f"{self.fusion.get_config_str()}_{self.fusion_type}_{self.detection_head_type}"

    def make_graphed(self, camera_imgs=None, lidar_points=None, radar_points=None, camera_calib=None, prev_bev=None,
                     ego_motion=None) -> "GraphedDetector":
        """Capture the inference forward for these input shapes into one hipGraph (launch-bound small batches)."""
        if prev_bev is None and ego_motion is None:
            return GraphedDetector(self, camera_imgs, lidar_points, radar_points, camera_calib)
        return GraphedDetector(self, camera_imgs, lidar_points, radar_points, camera_calib, prev_bev, ego_motion)


class GraphedDetector:
    """The eval-mode detector forward captured as a hipGraph: ~40 kernel launches replayed with one call.

    Every launch of the HIP path goes to torch's current stream, so `torch.cuda.graph` records them; inputs are
    copied into static buffers, outputs are static tensors that the next replay overwrites (clone to keep).
    Weights are baked in as of capture time: re-capture after a parameter update.  With `camera_calib` the per-frame calibration
    is a graph input like the images (a static device tensor, copied into before the replay): the table build and the gather are
    part of the capture, nothing is built on the host.  A model with temporal fusion is always captured with the warp: `prev_bev`
    and `ego_motion` are static inputs of the same kind (zeros and the identity when the capture gets none), and a call without
    prev_bev zeroes the static history, which gives the bits of the eager first-frame path."""

    def __init__(self, model: "FlexibleMultiModal3DDetector", camera_imgs, lidar_points, radar_points, camera_calib=None,
                 prev_bev=None, ego_motion=None):
        assert not model.training, "capture the inference forward: call model.eval() first"
        E.require_cuda(camera_imgs, lidar_points)
        self.model = model
        calib = model.camera_calib_tensor(camera_imgs, camera_calib)
        self.static_calib = None if calib is None else (calib[0].to(camera_imgs.device).clone().contiguous(), calib[1])
        c = lambda t: t.clone() if t is not None else None
        self.static_in = (c(camera_imgs), c(lidar_points), [r.clone() for r in radar_points] if radar_points else None)
        self.static_history = self._capture_history(prev_bev, ego_motion)
        args = (self.static_calib,) if self.static_history is None else (self.static_calib, self.static_history)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):                                   # packs weights, sizes workspaces, sets kernel attributes
                model._forward_inference(*self.static_in, *args)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.static_out = model._forward_inference(*self.static_in, *args)

    def _capture_history(self, prev_bev, ego_motion):
        """The static (prev_bev, ego, None) of a model with temporal fusion -- zeros / identities where the capture got none --, None
        for any other model (either argument then raises)."""
        model, (si, sp, sr) = self.model, self.static_in
        history = model._history(si, sp, sr, prev_bev, ego_motion)
        if history is None:
            return None
        fus = model.fusion
        first = next(t[0] if isinstance(t, list) else t for t in (si if model.use_camera else None, sp if model.use_lidar else None,
                                                                   sr if model.use_radar else None) if t is not None)
        B, dev = first.shape[0], first.device
        prev = (torch.zeros(B, fus.bev_h, fus.bev_w, fus.bev_channels, dtype=fus._eng().dtype, device=dev).permute(0, 3, 1, 2)
                if history[0] is None else history[0].clone(memory_format=torch.channels_last))
        ego = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1) if history[1] is None else history[1].clone()
        return prev, ego, None

    def _set_history(self, prev_bev, ego_motion) -> None:
        if self.static_history is None:
            if prev_bev is not None or ego_motion is not None:
                self.model._history(*self.static_in, prev_bev, ego_motion)           # raises: no temporal fusion
            return
        prev, ego, _ = self.static_history
        history = self.model._history(*self.static_in, prev_bev, ego_motion)
        if history[0] is None:
            prev.zero_()
            return
        if history[0].data_ptr() != prev.data_ptr():
            prev.copy_(history[0])
        if history[1].data_ptr() != ego.data_ptr():
            ego.copy_(history[1])

    @torch.no_grad()
    def __call__(self, camera_imgs=None, lidar_points=None, radar_points=None, camera_calib=None, prev_bev=None,
                 ego_motion=None) -> Dict[str, torch.Tensor]:
        si, sp, sr = self.static_in
        self._set_history(prev_bev, ego_motion)
        if camera_calib is not None:
            if self.static_calib is None:
                raise E.L.BevfError("GraphedDetector: captured without camera_calib; capture again with one")
            calib = self.model.camera_calib_tensor(si, camera_calib)
            if calib[1] != self.static_calib[1]:
                raise E.L.BevfError(f"GraphedDetector: captured for image_size {self.static_calib[1]}, got {calib[1]}")
            if calib[0].data_ptr() != self.static_calib[0].data_ptr():
                self.static_calib[0].copy_(calib[0])
        if self.static_calib is not None:
            # the replay rebuilds the per-frame tables in the engine's buffers: a training tape that still needs its own rebuilds them
            self.model.fusion._eng().invalidate_frame_tables()
        for dst, src in ((si, camera_imgs), (sp, lidar_points)):
            if dst is not None and src is not None and src.data_ptr() != dst.data_ptr():
                dst.copy_(src)
        if sr is not None and radar_points is not None:
            for d, s_ in zip(sr, radar_points):
                if d.data_ptr() != s_.data_ptr():
                    d.copy_(s_)
        self.graph.replay()
        return self.static_out


def create_detector(modality_config: Optional[str] = None, fusion_type: Optional[str] = None,
                    detection_head: Optional[str] = None, num_classes: Optional[int] = None,
                    config: Optional[Dict] = None, config_path: Optional[str] = None,
                    lidar_encoder_type: Optional[str] = None, camera_view_transform: Optional[str] = None,
                    temporal: Optional[bool] = None, seg_head=None, iou_head=None, bev_backbone=None,
                    roi_head=None, **kwargs) -> FlexibleMultiModal3DDetector:
    """ref src/fusion.py:1148-1221.  modality_config: 'camera_only' | 'camera+lidar' | ... | 'all'; the
    flags are substring tests on the lower-cased, space-stripped string (ref :1197-1202).
    lidar_encoder_type: 'PointPillars' selects the pillar LiDAR branch (None: the config's model.lidar_encoder.type).
    camera_view_transform: 'project' selects the camera -> BEV projection branch, 'lift' its learned-depth variant, 'frustum' the
    lift-splat branch, 'mean' the reference's camera average (None: the config's model.bev_fusion.camera_view_transform, else
    'mean').
    temporal: True adds the history slot of temporal BEV fusion (None: the config's model.bev_fusion.temporal.enable, else off).
    seg_head: True, or a dict of {num_classes | classes, output_range, output_size, hidden_channels}, adds the BEV map-segmentation
    head (seg_head.BEVSegmentationHead) on the fused map and the 'seg' output (None: the config's model.seg_head.enable, else off).
    iou_head: True, or a dict of {head_conv}, adds the IoU-aware head (iou_head.IoUHead) on the fused map and the 'iou' output
    (None: the config's model.iou_head.enable, else off).
    bev_backbone: True, or a dict of bev_backbone.BEVBackbone's settings, puts the multi-scale BEV backbone + FPN neck between the
    fuser and every head (None: the config's model.bev_backbone.enable, else off).
    roi_head: True, or a dict of {fc}, adds CenterPoint's second stage (roi_head.RoIHead) on the map the heads read, the 'feat'
    output and `model.refine` (None: the config's model.roi_head.enable, else off)."""
    if roi_head is not None:
        kwargs["roi_head"] = roi_head
    if bev_backbone is not None:
        kwargs["bev_backbone"] = bev_backbone
    if iou_head is not None:
        kwargs["iou_head"] = iou_head
    if temporal is not None:
        kwargs["temporal"] = temporal
    if seg_head is not None:
        kwargs["seg_head"] = seg_head
    config = _cfg(config, config_path)
    if config is not None and modality_config is None:
        modality_config = config.get("model", {}).get("modality_config", "all")
    use_camera = use_lidar = use_radar = None
    if modality_config is not None:
        m = modality_config.lower().replace(" ", "")
        use_camera = "camera" in m or m == "all"
        use_lidar = "lidar" in m or m == "all"
        use_radar = "radar" in m or m == "all"
    return FlexibleMultiModal3DDetector(use_camera=use_camera, use_lidar=use_lidar, use_radar=use_radar,
                                        num_classes=num_classes, fusion_type=fusion_type,
                                        detection_head=detection_head, config=config,
                                        lidar_encoder_type=lidar_encoder_type, camera_view_transform=camera_view_transform,
                                        **kwargs)


def test_all_configurations():
    """ref src/fusion.py:1228-1330 -- the reference's PASS/FAIL sweep, restricted to the built (bev) path."""
    dev = torch.device("cuda:0")
    results = {}
    for mod in ("camera+lidar", "camera+lidar+radar"):
        try:
            model = create_detector(mod, "bev", "centernet").to(dev).eval()
            imgs = torch.randn(2, 3, 3, 448, 800, device=dev)
            pts = torch.randn(2, 34720, 4, device=dev)
            radars = [torch.randn(2, 125, 7, device=dev) for _ in range(5)] if "radar" in mod else None
            out = model(imgs, pts, radars)
            n = sum(p.numel() for p in model.parameters())
            print(f"PASS {model.get_config_str()}: {n:,} params, heatmap {tuple(out['heatmap'].shape)}")
            results[mod] = True
        except Exception as e:  # noqa: BLE001 - mirrors the reference's try/except report
            print(f"FAIL {mod}: {e}")
            results[mod] = False
    return results
