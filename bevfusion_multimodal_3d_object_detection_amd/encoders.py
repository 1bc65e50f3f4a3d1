"""Drop-in for the reference's `encoders` module (ref src/encoders.py), MI355X-native.

Same class names, constructor signatures, attributes and state-dict keys; `forward` runs the
hand-written gfx950 kernels of libbevf_hip.so through engine.py.  Modules are parameter
containers (torch.nn layers are used only to hold tensors under the reference's key names).
"""
from __future__ import annotations

import warnings
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import yaml

from . import _lib as L
from . import engine as E


def load_config(config_path: str = "config.yaml") -> Dict:
    """ref src/encoders.py:16-33 -- yaml.safe_load; FileNotFoundError when the file is missing."""
    f = Path(config_path)
    if not f.exists():
        raise FileNotFoundError(f"Config file not found: {config_path}")
    with open(f, "r") as fh:
        return yaml.safe_load(fh)


def _cfg(config, config_path) -> Optional[Dict]:
    if config is None and config_path is not None:
        config = load_config(config_path)
    return config


# ---- ResNet-18 trunk parameter containers (torchvision layout: conv1,bn1,conv2,bn2[,downsample.0/.1]) ----

class _BasicBlockParams(nn.Module):
    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))


def _stage(cin: int, cout: int, stride: int) -> nn.Sequential:
    blocks = [_BasicBlockParams(cin, cout, stride), _BasicBlockParams(cout, cout, 1)]
    for b in blocks:                                   # torchvision's default init for the trunk
        nn.init.kaiming_normal_(b.conv1.weight, mode="fan_out", nonlinearity="relu")
        nn.init.kaiming_normal_(b.conv2.weight, mode="fan_out", nonlinearity="relu")
        if b.downsample is not None:
            nn.init.kaiming_normal_(b.downsample[0].weight, mode="fan_out", nonlinearity="relu")
    return nn.Sequential(*blocks)


class ResNetCameraEncoder(nn.Module):
    """ref src/encoders.py:36-189.  (B,6,3,H,W) or (B*6,3,H,W) -> (B,6,512,H/16,W/16) / (B*6,512,...)."""

    def __init__(self, backbone: Optional[str] = None, pretrained: Optional[bool] = None,
                 out_channels: Optional[int] = None, freeze_bn: Optional[bool] = None,
                 config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            c = config.get("model", {}).get("camera_encoder", {})
            self.backbone_name = c.get("backbone", "resnet18")
            pretrained = c.get("pretrained", True)
            freeze_bn = c.get("freeze_bn", False)
            self.out_channels = c.get("output_channels", 512)
            self.total_stride = c.get("total_stride", 16)
        else:
            self.backbone_name = backbone if backbone is not None else "resnet18"
            pretrained = True if pretrained is None else pretrained
            freeze_bn = False if freeze_bn is None else freeze_bn
            self.out_channels = out_channels if out_channels is not None else 512
            self.total_stride = 16
        if self.backbone_name != "resnet18":
            # the reference leaves `resnet` undefined for anything else (ref :97-99 -> UnboundLocalError)
            raise NotImplementedError(f"backbone '{self.backbone_name}': only 'resnet18' exists in the reference")
        if pretrained:
            warnings.warn("pretrained=True: ImageNet weights are a network fetch in the reference; this build never "
                          "downloads -- load them with load_state_dict() (keys are identical).", stacklevel=2)
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        nn.init.kaiming_normal_(self.conv1.weight, mode="fan_out", nonlinearity="relu")
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = _stage(64, 64, 1)
        self.layer2 = _stage(64, 128, 2)
        self.layer3 = _stage(128, 256, 2)
        self.channel_proj = nn.Sequential(nn.Conv2d(256, 512, 1, bias=False), nn.BatchNorm2d(512),
                                          nn.ReLU(inplace=True))
        if freeze_bn:
            self._freeze_bn()
        self._engine = None

    def _freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def _eng(self) -> E.CameraEncoderEngine:
        if self._engine is None:
            object.__setattr__(self, "_engine", E.CameraEncoderEngine(self))
        return self._engine

    def forward_nhwc(self, x: torch.Tensor):
        """Internal fast path: returns (NHWC feature buffer, (B, ncam, Hc, Wc))."""
        E.require_cuda(x)
        if x.dim() == 5:
            B, n = x.shape[:2]
            x = x.reshape(B * n, *x.shape[2:])
        else:
            B, n = x.shape[0], 1
        feat, hc, wc = self._eng().run(x.contiguous().float())
        return feat, (B, n, hc, wc)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training and _training().wants_train_path(self):
            # a freshly built encoder is in train mode (ref src/encoders.py:805, 829): batch statistics + a gradient path
            E.require_cuda(x)
            return _training().camera_encoder_train_forward(self, x)
        with torch.no_grad():
            return self._forward_eval(x)

    def _forward_eval(self, x: torch.Tensor) -> torch.Tensor:
        five_d = x.dim() == 5
        feat, (B, n, hc, wc) = self.forward_nhwc(x)
        out = E.to_nchw(feat, B * n, 512, hc, wc)
        return out.view(B, n, 512, hc, wc) if five_d else out

    def get_output_shape(self, input_height: int, input_width: int) -> Tuple[int, int, int]:
        return (self.out_channels, input_height // self.total_stride, input_width // self.total_stride)


def _training():
    from . import training            # train-mode BatchNorm + tape + hand-written backward; imported on first use
    return training


class _PointMLP(nn.Module):
    """conv{i}/bn{i} containers shared by the LiDAR and radar point encoders."""

    def _build(self, cin: int, widths: List[int], use_bn: bool):
        c = cin
        for i, w in enumerate(widths, 1):
            setattr(self, f"conv{i}", nn.Conv1d(c, w, 1))
            setattr(self, f"bn{i}", nn.BatchNorm1d(w) if use_bn else nn.Identity())
            c = w

    def _rows(self, x: torch.Tensor) -> torch.Tensor:
        """(B,N,C) or (B,C,N) -> contiguous (B,N,C), with the reference's layout sniff (ref :282-284)."""
        E.require_cuda(x)
        x = x.float()
        if x.dim() == 3 and x.shape[2] == self.input_channels:
            return x.contiguous()
        B, Cc, N = x.shape
        y = torch.empty(B, N, Cc, device=x.device)
        L.nchw_to_nhwc(x.contiguous(), y, B, Cc, N, Cc)
        return y


class PointNetLiDAREncoder(_PointMLP):
    """ref src/encoders.py:191-306.  (B,N,C)|(B,C,N) -> (B,feat_dim); padded points are not masked."""

    def __init__(self, input_channels: Optional[int] = None, feat_dim: Optional[int] = None,
                 use_bn: Optional[bool] = None, return_point_features: Optional[bool] = None,
                 config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            c = config.get("model", {}).get("lidar_encoder", {})
            self.input_channels = c.get("input_channels", 5)
            self.feat_dim = c.get("feature_dim", 1024)
            use_bn = c.get("use_batch_norm", True)
            self.return_point_features = False
            widths = c.get("mlp_layers", [64, 128, 256, 512, 1024])
        else:
            self.input_channels = input_channels if input_channels is not None else 5
            self.feat_dim = feat_dim if feat_dim is not None else 1024
            use_bn = True if use_bn is None else use_bn
            self.return_point_features = bool(return_point_features) if return_point_features is not None else False
            widths = [64, 128, 256, 512, 1024]
        self._build(self.input_channels, widths, use_bn)
        self._engine = None

    def _eng(self) -> E.PointNetEngine:
        if self._engine is None:
            object.__setattr__(self, "_engine", E.PointNetEngine(self))
        return self._engine

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training and _training().wants_train_path(self):
            E.require_cuda(x)
            return _training().pointnet_train_forward(self, x)
        with torch.no_grad():
            return self._forward_eval(x)

    def _forward_eval(self, x: torch.Tensor) -> torch.Tensor:
        rows = self._rows(x)
        B, N, _ = rows.shape
        g, last = self._eng().run(rows, keep_last=self.return_point_features)
        if self.return_point_features:                          # ref :300-304, (B,N,2*feat)
            f = g.shape[1]
            return torch.cat([last[:B * N * f].view(B, N, f), g.unsqueeze(1).expand(B, N, f)], dim=2)
        return g


class RadarEncoder(_PointMLP):
    """ref src/encoders.py:458-557."""

    def __init__(self, input_channels: Optional[int] = None, feat_dim: Optional[int] = None,
                 use_bn: Optional[bool] = None, config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            c = config.get("model", {}).get("radar_encoder", {})
            self.input_channels = c.get("input_channels", 7)
            self.feat_dim = c.get("feature_dim", 256)
            use_bn = c.get("use_batch_norm", True)
            widths = c.get("mlp_layers", [32, 64, 128, 256])
        else:
            self.input_channels = input_channels if input_channels is not None else 7
            self.feat_dim = feat_dim if feat_dim is not None else 256
            use_bn = True if use_bn is None else use_bn
            widths = [32, 64, 128, 256]
        self._build(self.input_channels, widths, use_bn)
        self._wrap = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training and _training().wants_train_path(self):
            E.require_cuda(x)
            return _training().radar_train_forward(self, x)
        with torch.no_grad():
            return self._forward_eval(x)

    def _forward_eval(self, x: torch.Tensor) -> torch.Tensor:
        if self._wrap is None:
            object.__setattr__(self, "_wrap", _SingleRadar(self))
        return self._wrap(self._rows(x))


class _SingleRadar:
    """Runs one RadarEncoder through the fused radar kernel (R = 1, no fusion layer)."""

    class _Shim(nn.Module):
        def __init__(self, enc):
            super().__init__()
            self.radar_encoder = enc
            self.fusion_method = "max"

    def __init__(self, enc: RadarEncoder):
        self.engine = E.RadarEngine(self._Shim(enc))

    def __call__(self, rows: torch.Tensor) -> torch.Tensor:
        return self.engine.run([rows])


class MultiRadarEncoder(nn.Module):
    """ref src/encoders.py:560-661.  List of (B,N_i,C) sweeps -> (B,feat_dim)."""

    def __init__(self, input_channels: Optional[int] = None, feat_dim: Optional[int] = None,
                 num_radars: Optional[int] = None, fusion_method: Optional[str] = None,
                 config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            c = config.get("model", {}).get("radar_encoder", {})
            input_channels = c.get("input_channels", 7)
            self.feat_dim = c.get("feature_dim", 256)
            self.num_radars = c.get("num_radars", 5)
            self.fusion_method = c.get("fusion_method", "concat")
        else:
            input_channels = input_channels if input_channels is not None else 7
            self.feat_dim = feat_dim if feat_dim is not None else 256
            self.num_radars = num_radars if num_radars is not None else 5
            self.fusion_method = fusion_method if fusion_method is not None else "concat"
        self.radar_encoder = RadarEncoder(input_channels=input_channels, feat_dim=self.feat_dim, config=config)
        if self.fusion_method == "concat":
            self.fusion_fc = nn.Linear(self.feat_dim * self.num_radars, self.feat_dim)
        self.output_dim = self.feat_dim
        self._engine = None

    def _eng(self) -> E.RadarEngine:
        if self._engine is None:
            object.__setattr__(self, "_engine", E.RadarEngine(self))
        return self._engine

    def forward(self, radar_list: List[torch.Tensor]) -> torch.Tensor:
        if self.training and _training().wants_train_path(self):
            E.require_cuda(*radar_list)
            return _training().radar_train_forward(self, list(radar_list))
        with torch.no_grad():
            return self._forward_eval(radar_list)

    def _forward_eval(self, radar_list: List[torch.Tensor]) -> torch.Tensor:
        if self.fusion_method not in ("concat", "max", "mean"):
            raise ValueError(f"Unknown fusion method: {self.fusion_method}")
        rows = [self.radar_encoder._rows(r) for r in radar_list]
        return self._eng().run(rows)


def voxelize(points: torch.Tensor, point_cloud_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0),
             voxel_size=(2.048, 2.048, 8.0), max_points_per_voxel: int = 32, max_voxels: int = 12000):
    """Hard voxelisation feeding `VFELayer` / `VoxelNetLiDAREncoder` (their docstrings, ref src/encoders.py:313-321,
    describe exactly this input; the reference never builds it).  Defaults are the grid of configs/base.yaml:48-55
    (50 x 50 pillars) and the reference's "32 points, 12000 voxels".  points (B,N,C) ->
    voxel_features (B,Nv,P,C) zero padded, voxel_coords (B,Nv,3) int64 (z,y,x), num_points (B,Nv), num_voxels (B,).
    The range must be a whole number of voxels on every axis: (max - min) / voxel_size, in fp32, further than 0.01 from an
    integer raises BevfError naming the axis (half a voxel has no agreed rounding); a voxel size derived as range / cells in
    fp32, as `pillar_grid` / `sparse_grid` do, is always accepted."""
    E.require_cuda(points)
    return L.voxelize(points.float().contiguous(), point_cloud_range, voxel_size, max_points_per_voxel, max_voxels)


def scatter_voxels(voxel_features: torch.Tensor, voxel_coords: torch.Tensor, voxel_grid_shape,
                   num_voxels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The dense scatter of `VoxelNetLiDAREncoder.forward` (ref src/encoders.py:399-410) as a kernel: per-voxel features
    (B,Nv,C) at voxel_coords (B,Nv,3) = (z,y,x) -> (B,C,D,H,W), last row wins where rows collide, zeros elsewhere.  With
    `num_voxels` (from `voxelize`) the zero-padded rows stay out; without it every row is written, as the reference does.
    `voxelize` -> `VFELayer` -> `scatter_voxels(..., (1,50,50))[:, :, 0]` is the pillar canvas (B,C,50,50) of the config's grid."""
    E.require_cuda(voxel_features, voxel_coords)
    nv = None if num_voxels is None else num_voxels.to(torch.int32).contiguous()
    return L.scatter_voxels(voxel_features.float().contiguous(), voxel_coords.to(torch.int64).contiguous(), voxel_grid_shape, nv)


class VFELayer(nn.Module):
    """ref src/encoders.py:420-455 -- Linear -> BN1d over all B*Nv*P rows -> ReLU -> max over the P points
    of each voxel ("PointNet pillar reduction").  (B,Nv,P,C) -> (B,Nv,out_channels)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.linear = nn.Linear(in_channels, out_channels)
        self.bn = nn.BatchNorm1d(out_channels)
        self._engine = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        E.require_cuda(x)
        B, Nv, P, Cc = x.shape                    # a 3-D input raises ValueError exactly like the reference
        if self.training and _training().wants_train_path(self):
            return _training().vfe_train_forward(self, x)          # batch statistics + gradients for linear / bn
        with torch.no_grad():
            if self._engine is None:
                object.__setattr__(self, "_engine", E.VFEEngine(self))
            return self._engine.run(x.contiguous().float()).view(B, Nv, self.out_channels)


PILLAR_TYPES = ("pointpillars", "pillars")
SPARSE_TYPES = ("sparsevoxel", "sparse", "second")
DEFAULT_PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)


def lidar_encoder_kind(lidar_encoder_type: Optional[str] = None, config: Optional[Dict] = None) -> str:
    """'pillars' when the keyword -- or, when it is None, `model.lidar_encoder.type` of the config -- names PointPillars
    (case-insensitive, 'PointPillars' or 'pillars'); 'sparse' when it names the sparse-voxel encoder ('SparseVoxel', 'sparse' or
    'SECOND'); 'pointnet' for anything else or nothing (incl. 'PointNet' / 'VoxelNet', the values configs/base.yaml documents but
    the reference never reads)."""
    t = lidar_encoder_type
    if t is None and config is not None:
        t = (config.get("model", {}).get("lidar_encoder", {}) or {}).get("type")
    t = t.strip().lower() if isinstance(t, str) else None
    return "pillars" if t in PILLAR_TYPES else ("sparse" if t in SPARSE_TYPES else "pointnet")


def pillar_grid(point_cloud_range, bev_h: int, bev_w: int) -> Tuple[float, float, float, float, Tuple[float, float, float]]:
    """One pillar per BEV cell: (x0, y0, pillar_x, pillar_y, voxel_size) in fp32 -- pillar size (max - min) / cells on x / y,
    the full z range on z (one pillar per column).  50 x 50 on the base range = 2.048 m, 128^2 = 0.8 m."""
    r = np.asarray(point_cloud_range, dtype=np.float32)
    vx = np.float32(r[3] - r[0]) / np.float32(bev_w)
    vy = np.float32(r[4] - r[1]) / np.float32(bev_h)
    vz = np.float32(r[5] - r[2])
    return float(r[0]), float(r[1]), float(vx), float(vy), (float(vx), float(vy), float(vz))


class PillarLiDAREncoder(nn.Module):
    """PointPillars LiDAR front end on the BEV grid (opt-in: `model.lidar_encoder.type: 'PointPillars'`).  Not in the
    reference, whose voxel path never runs; the semantics are the standard PointPillars ones (include/bevf.h, pillars):
    points (B,N,C) -> voxelize on one pillar per BEV cell -> decorated points (C + 5 channels) -> pfn = VFELayer(C + 5,
    pfn_channels) over all P rows of every occupied pillar -> max per pillar -> canvas (B, pfn_channels, bev_h, bev_w),
    row = y index, column = x index, exactly 0 at empty cells."""

    is_pillars = True

    def __init__(self, input_channels: Optional[int] = None, pfn_channels: Optional[int] = None, bev_h: Optional[int] = None,
                 bev_w: Optional[int] = None, point_cloud_range=None, max_points_per_pillar: Optional[int] = None,
                 max_pillars: Optional[int] = None, config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            c, d = config.get("model", {}).get("lidar_encoder", {}) or {}, config.get("dataset", {})
            input_channels = c.get("input_channels", 5) if input_channels is None else input_channels
            pfn_channels = c.get("pfn_channels", 64) if pfn_channels is None else pfn_channels
            max_points_per_pillar = c.get("max_points_per_pillar", 32) if max_points_per_pillar is None else max_points_per_pillar
            max_pillars = c.get("max_pillars", 12000) if max_pillars is None else max_pillars
            point_cloud_range = d.get("point_cloud_range", DEFAULT_PC_RANGE) if point_cloud_range is None else point_cloud_range
            bev_h = d.get("bev_h", 50) if bev_h is None else bev_h
            bev_w = d.get("bev_w", 50) if bev_w is None else bev_w
        self.input_channels = 4 if input_channels is None else int(input_channels)
        self.pfn_channels = 64 if pfn_channels is None else int(pfn_channels)
        self.max_points = 32 if max_points_per_pillar is None else int(max_points_per_pillar)
        self.max_pillars = 12000 if max_pillars is None else int(max_pillars)
        self.pc_range = tuple(float(v) for v in (DEFAULT_PC_RANGE if point_cloud_range is None else point_cloud_range))
        self.bev_h = 50 if bev_h is None else int(bev_h)
        self.bev_w = 50 if bev_w is None else int(bev_w)
        if not 3 <= self.input_channels <= 11:
            raise L.BevfError(f"PillarLiDAREncoder: input_channels={self.input_channels}: the decorated point (C + 5 channels) "
                              "must fit 16 channels and carry x, y, z, so 3 <= C <= 11")
        if self.pfn_channels % 32 or not 0 < self.pfn_channels <= 128:
            raise L.BevfError(f"PillarLiDAREncoder: pfn_channels={self.pfn_channels} must be a multiple of 32 up to 128")
        if not 0 < self.max_points <= 255 or self.max_pillars <= 0:
            raise L.BevfError("PillarLiDAREncoder: need 0 < max_points_per_pillar <= 255 and max_pillars > 0")
        self.pfn = VFELayer(self.input_channels + 5, self.pfn_channels)
        self._engine = None

    def grid(self):
        return pillar_grid(self.pc_range, self.bev_h, self.bev_w)

    def _eng(self) -> E.PillarEngine:
        if self._engine is None:
            object.__setattr__(self, "_engine", E.PillarEngine(self))
        return self._engine

    def forward_nhwc(self, points: torch.Tensor) -> torch.Tensor:
        """Internal fast path: the canvas as an NHWC view (B, bev_h, bev_w, pfn_channels) in the storage dtype."""
        E.require_cuda(points)
        return self._eng().run(points)

    def forward(self, points: torch.Tensor) -> torch.Tensor:
        if self.training and _training().wants_train_path(self):
            E.require_cuda(points)
            return _training().pillar_train_forward(self, points)
        with torch.no_grad():
            return self._forward_eval(points)

    def _forward_eval(self, points: torch.Tensor) -> torch.Tensor:
        c = self.forward_nhwc(points)
        return E.to_nchw(c, c.shape[0], self.pfn_channels, self.bev_h, self.bev_w)


def sparse_grid(point_cloud_range, bev_h: int, bev_w: int, z_voxels: int):
    """Level-0 grid of the sparse-voxel encoder: ((Dz, 4 bev_h, 4 bev_w), voxel_size) -- the xy voxel is pillar_grid's fp32 cell
    divided by 4 (exact), the z voxel the fp32 z range divided by Dz."""
    _, _, vx, vy, _ = pillar_grid(point_cloud_range, bev_h, bev_w)
    r = np.asarray(point_cloud_range, dtype=np.float32)
    vz = np.float32(r[5] - r[2]) / np.float32(z_voxels)
    return (int(z_voxels), 4 * int(bev_h), 4 * int(bev_w)), (float(np.float32(vx) / np.float32(4)), float(np.float32(vy) / np.float32(4)), float(vz))


class SparseConvBlock(nn.Module):
    """Parameters of one sparse layer: Conv3d(cin, cout, 3, bias=False) + BatchNorm1d(cout) (+ ReLU) as plain torch modules, so the
    state dict is torch-native and a dense restatement loads the same one.  stride 1 = submanifold, stride 2 = strided (pad 1)."""

    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False)
        self.bn = nn.BatchNorm1d(cout)
        self.stride = stride


SPARSE_LAYERS = ("conv_in", "down1", "subm1", "down2", "subm2")


class SparseLiDAREncoder(nn.Module):
    """Sparse-voxel (VoxelNet / SECOND style) LiDAR encoder on the BEV grid (opt-in: `model.lidar_encoder.type: 'SparseVoxel'`).
    Not in the reference, whose voxel path never runs; spconv's semantics (include/bevf.h, sparse-voxel encoder):
    points (B,N,C) -> voxelize on the (z_voxels, 4 bev_h, 4 bev_w) grid -> mean of each voxel's kept points -> conv_in (submanifold
    3x3x3, C -> c0) -> down1 (stride 2, c0 -> c1) -> subm1 -> down2 (stride 2, c1 -> c2) -> subm2, each + BatchNorm over the active
    voxels + ReLU, computed over the occupied voxels only -> z folded into channels -> canvas (B, c2 z_voxels / 4, bev_h, bev_w),
    channel z * c2 + c, exactly 0 at inactive cells.  Consumed by the fusion's lidar_bev exactly like the pillar canvas."""

    is_sparse = True

    def __init__(self, input_channels: Optional[int] = None, channels=None, z_voxels: Optional[int] = None,
                 bev_h: Optional[int] = None, bev_w: Optional[int] = None, point_cloud_range=None,
                 max_points_per_voxel: Optional[int] = None, max_voxels: Optional[int] = None, config: Optional[Dict] = None,
                 config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            c, d = config.get("model", {}).get("lidar_encoder", {}) or {}, config.get("dataset", {})
            input_channels = c.get("input_channels", 5) if input_channels is None else input_channels
            channels = c.get("channels", (32, 64, 128)) if channels is None else channels
            z_voxels = c.get("z_voxels", 8) if z_voxels is None else z_voxels
            max_points_per_voxel = c.get("max_points_per_voxel", 8) if max_points_per_voxel is None else max_points_per_voxel
            max_voxels = c.get("max_voxels", 40000) if max_voxels is None else max_voxels
            point_cloud_range = d.get("point_cloud_range", DEFAULT_PC_RANGE) if point_cloud_range is None else point_cloud_range
            bev_h = d.get("bev_h", 50) if bev_h is None else bev_h
            bev_w = d.get("bev_w", 50) if bev_w is None else bev_w
        self.input_channels = 4 if input_channels is None else int(input_channels)
        self.channels = tuple(int(v) for v in ((32, 64, 128) if channels is None else channels))
        self.z_voxels = 8 if z_voxels is None else int(z_voxels)
        self.max_points = 8 if max_points_per_voxel is None else int(max_points_per_voxel)
        self.max_voxels = 40000 if max_voxels is None else int(max_voxels)
        self.pc_range = tuple(float(v) for v in (DEFAULT_PC_RANGE if point_cloud_range is None else point_cloud_range))
        self.bev_h = 50 if bev_h is None else int(bev_h)
        self.bev_w = 50 if bev_w is None else int(bev_w)
        if not 3 <= self.input_channels <= 8:
            raise L.BevfError(f"SparseLiDAREncoder: input_channels={self.input_channels}: a point carries x, y, z and at most 8 "
                              "channels (zero-padded to the 32-channel K granule of the first layer), so 3 <= C <= 8")
        if len(self.channels) != 3 or any(v % 32 or not 0 < v <= 128 for v in self.channels):
            raise L.BevfError(f"SparseLiDAREncoder: channels={self.channels} must be three multiples of 32 up to 128")
        if self.z_voxels <= 0 or self.z_voxels % 4:
            raise L.BevfError(f"SparseLiDAREncoder: z_voxels={self.z_voxels} must be a positive multiple of 4 (two stride-2 layers)")
        if self.max_points <= 0 or self.max_voxels <= 0 or self.bev_h <= 0 or self.bev_w <= 0:
            raise L.BevfError("SparseLiDAREncoder: need max_points_per_voxel > 0, max_voxels > 0 and a BEV grid")
        c0, c1, c2 = self.channels
        self.conv_in = SparseConvBlock(self.input_channels, c0, 1)
        self.down1 = SparseConvBlock(c0, c1, 2)
        self.subm1 = SparseConvBlock(c1, c1, 1)
        self.down2 = SparseConvBlock(c1, c2, 2)
        self.subm2 = SparseConvBlock(c2, c2, 1)
        self.out_channels = c2 * self.z_voxels // 4
        self._engine = None

    def layers(self):
        return [getattr(self, n) for n in SPARSE_LAYERS]

    def grid(self):
        """((Dz, 4 bev_h, 4 bev_w), voxel_size) of level 0."""
        return sparse_grid(self.pc_range, self.bev_h, self.bev_w, self.z_voxels)

    def level_dims(self):
        """Grid (D, H, W) and per-frame row capacity of levels 0, 1, 2: capacity(0) = max_voxels, then the worst case
        min(8 capacity(l - 1), cells(l)) -- nothing is ever truncated past voxelize's own cap."""
        (D, H, W), _ = self.grid()
        dims, caps = [(D, H, W)], [self.max_voxels]
        for _ in range(2):
            D, H, W = D // 2, H // 2, W // 2
            dims.append((D, H, W))
            caps.append(min(8 * caps[-1], D * H * W))
        return dims, caps

    def _eng(self) -> "E.SparseLiDAREngine":
        if self._engine is None:
            object.__setattr__(self, "_engine", E.SparseLiDAREngine(self))
        return self._engine

    def forward_nhwc(self, points: torch.Tensor) -> torch.Tensor:
        """Internal fast path: the canvas as an NHWC view (B, bev_h, bev_w, out_channels) in the storage dtype."""
        E.require_cuda(points)
        return self._eng().run(points)

    def forward(self, points: torch.Tensor) -> torch.Tensor:
        if self.training and _training().wants_train_path(self):
            E.require_cuda(points)
            return _training().sparse_train_forward(self, points)
        with torch.no_grad():
            return self._forward_eval(points)

    def _forward_eval(self, points: torch.Tensor) -> torch.Tensor:
        c = self.forward_nhwc(points)
        return E.to_nchw(c, c.shape[0], self.out_channels, self.bev_h, self.bev_w)


class VoxelNetLiDAREncoder(nn.Module):
    """ref src/encoders.py:308-417.  Dead code in the reference (never imported by fusion.py) and its
    forward raises: vfe2 receives vfe1's 3-D output and cannot unpack 4 dims (ref :395-396 vs :438).
    The parameter layout is kept for checkpoint compatibility; forward reproduces that ValueError."""

    def __init__(self, input_channels: Optional[int] = None, voxel_feat_dim: Optional[int] = None,
                 output_feat_dim: Optional[int] = None, max_points_per_voxel: Optional[int] = None,
                 config: Optional[Dict] = None, config_path: Optional[str] = None):
        super().__init__()
        config = _cfg(config, config_path)
        if config is not None:
            c = config.get("model", {}).get("lidar_encoder", {})
            self.input_channels = c.get("input_channels", 5)
            self.voxel_feat_dim = 128
            self.output_feat_dim = c.get("feature_dim", 256)
        else:
            self.input_channels = input_channels if input_channels is not None else 5
            self.voxel_feat_dim = voxel_feat_dim if voxel_feat_dim is not None else 128
            self.output_feat_dim = output_feat_dim if output_feat_dim is not None else 256
        self.vfe1 = VFELayer(self.input_channels, self.voxel_feat_dim // 2)
        self.vfe2 = VFELayer(self.voxel_feat_dim // 2, self.voxel_feat_dim)
        self.conv3d_1 = nn.Conv3d(self.voxel_feat_dim, 128, 3, stride=2, padding=1)
        self.bn3d_1 = nn.BatchNorm3d(128)
        self.conv3d_2 = nn.Conv3d(128, 256, 3, stride=2, padding=1)
        self.bn3d_2 = nn.BatchNorm3d(256)
        self.conv3d_3 = nn.Conv3d(256, self.output_feat_dim, 3, stride=2, padding=1)
        self.bn3d_3 = nn.BatchNorm3d(self.output_feat_dim)

    def forward(self, voxel_features, voxel_coords, voxel_grid_shape):
        v = self.vfe1(voxel_features)
        B, N_voxels, N_points, Cc = v.shape       # raises ValueError: not enough values to unpack (as the reference)
        raise ValueError("unreachable")


def print_encoder_specs():
    """ref src/encoders.py:663-790 prints a static description of the encoders."""
    print("=" * 80)
    print("MULTI-MODAL ENCODER SPECIFICATIONS (MI355X-native build)")
    print("=" * 80)
    print("camera : ResNet-18 conv1..layer3 + 1x1 proj, (B,6,3,H,W) -> (B,6,512,H/16,W/16)")
    print("lidar  : PointNet shared MLP 64-128-256-512-1024 + max, (B,N,C) -> (B,1024)")
    print("         or (model.lidar_encoder.type: PointPillars) pillars on the BEV grid, decorated points -> PFN -> canvas")
    print("         or (model.lidar_encoder.type: SparseVoxel) sparse 3x3x3 convolutions over the occupied voxels -> canvas")
    print("radar  : 5 x shared MLP 32-64-128-256 + max, concat -> Linear(1280,256), -> (B,256)")
