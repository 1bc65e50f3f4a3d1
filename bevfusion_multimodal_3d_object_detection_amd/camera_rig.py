"""Camera calibration and the camera -> BEV projection table of the opt-in `camera_view_transform: 'project'` branch.

Parameter-free projection in the style of Simple-BEV (Harley et al. 2022): every BEV cell of the fusion grid takes
`num_heights` points above its centre, projects each into every camera with a fixed calibration, samples the camera feature
map bilinearly there and averages over the samples that hit an image.  With a static rig the whole lift is a sparse matrix
over (BEV cell) x (camera feature pixel), built here once on the host in fp64 and applied on the device by
bevf_csr_gather (csrc/camera_bev.hip) -- the forward on the cell table, the backward on its exact transpose.

The module's rig is the default for every frame.  Calibration that changes from frame to frame (vehicles, scenes, resize / crop
augmentation) goes in as `camera_calib=` of the fusion / detector forward: `calib_matrices(rigs)` packs one projection matrix per
(frame, camera) and the same table is then built per frame ON THE DEVICE (csrc/camera_calib.hip: bevf_camera_table_build_f64,
its transpose by bevf_camera_table_transpose, applied by bevf_csr_gather_frames).  DESIGN.md 3.2d.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# the reference's camera order (ref src/train_detect.py:134-135): the order of the camera axis of the image input
CAM_ORDER = ("CAM_FRONT", "CAM_FRONT_RIGHT", "CAM_FRONT_LEFT", "CAM_BACK", "CAM_BACK_LEFT", "CAM_BACK_RIGHT")
VIEW_TRANSFORMS = ("mean", "project", "lift", "frustum")
DEFAULT_NUM_HEIGHTS = 8
DEFAULT_MIN_DEPTH = 0.1
DEFAULT_DEPTH_BINS, DEFAULT_DEPTH_MIN, DEFAULT_DEPTH_MAX = 32, 1.0, 65.0      # the 'lift' branch's uniform depth bins (metres)
MAX_DEPTH_BINS = 64                                                           # one bin per lane in the lift's backward kernel


def quat_to_matrix(q: Sequence[float]) -> np.ndarray:
    """Unit quaternion (w, x, y, z) -- the nuScenes / pyquaternion convention -> 3x3 rotation (fp64, normalised first)."""
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    if n == 0.0:
        raise ValueError("camera rig: zero quaternion")
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def sensor_to_frame(calibrated_sensor: Dict) -> np.ndarray:
    """{'translation': [3], 'rotation': [w, x, y, z]} (sensor -> ego) -> 4x4 fp64."""
    T = np.eye(4, dtype=np.float64)
    T[:3, :3] = quat_to_matrix(calibrated_sensor["rotation"])
    T[:3, 3] = np.asarray(calibrated_sensor["translation"], dtype=np.float64)
    return T


@dataclass(frozen=True)
class CameraRig:
    """A fixed multi-camera calibration.

    image_size: (H, W) of the images the intrinsics refer to (the feature map of any resolution covers the same field of view);
    names: camera names in the order of the input's camera axis; K: (ncam, 3, 3) intrinsics; cam_to_bev: (ncam, 4, 4) from the
    camera frame (OpenCV: x right, y down, z forward) to the frame of the LiDAR points, the boxes and point_cloud_range."""
    image_size: Tuple[int, int]
    names: Tuple[str, ...]
    K: np.ndarray
    cam_to_bev: np.ndarray

    def __post_init__(self):
        K = np.asarray(self.K, dtype=np.float64).reshape(-1, 3, 3)
        T = np.asarray(self.cam_to_bev, dtype=np.float64).reshape(-1, 4, 4)
        if K.shape[0] != len(self.names) or T.shape[0] != len(self.names) or not self.names:
            raise ValueError(f"camera rig: {len(self.names)} names, {K.shape[0]} intrinsics, {T.shape[0]} extrinsics")
        H, W = (int(v) for v in self.image_size)
        if H <= 0 or W <= 0:
            raise ValueError(f"camera rig: bad image_size {self.image_size}")
        object.__setattr__(self, "K", K)
        object.__setattr__(self, "cam_to_bev", T)
        object.__setattr__(self, "image_size", (H, W))
        object.__setattr__(self, "names", tuple(self.names))

    @property
    def num_cameras(self) -> int:
        return len(self.names)

    def key(self) -> Tuple:
        """Hashable identity of the calibration (table cache key)."""
        return (self.image_size, self.names, self.K.tobytes(), self.cam_to_bev.tobytes())

    @classmethod
    def from_info(cls, info: Dict, cam_order: Sequence[str] = CAM_ORDER, image_size: Tuple[int, int] = (900, 1600)) -> "CameraRig":
        """From one converted-data info dict (ref src/data_converter.py:100-151): cams[name]['calibrated_sensor'] is camera -> ego
        ({translation, rotation (w, x, y, z), camera_intrinsic}), lidar_calibrated_sensor is LiDAR -> ego; the boxes and points are in
        the LiDAR frame, so cam_to_bev = (lidar -> ego)^-1 . (camera -> ego).  image_size: the size the intrinsics refer to (nuScenes:
        900 x 1600)."""
        lidar_to_ego = sensor_to_frame(info["lidar_calibrated_sensor"])
        ego_to_lidar = np.linalg.inv(lidar_to_ego)
        Ks, Ts = [], []
        for name in cam_order:
            cs = info["cams"][name]["calibrated_sensor"]
            Ks.append(np.asarray(cs["camera_intrinsic"], dtype=np.float64).reshape(3, 3))
            Ts.append(ego_to_lidar @ sensor_to_frame(cs))
        return cls(tuple(image_size), tuple(cam_order), np.stack(Ks), np.stack(Ts))

    @classmethod
    def from_dict(cls, d: Dict) -> "CameraRig":
        """The config form: {image_size: [H, W], cameras: [{name, K: 3x3, cam_to_bev: 4x4}, ...]} (to_dict's output)."""
        cams = d["cameras"]
        return cls(tuple(d["image_size"]), tuple(c["name"] for c in cams), np.stack([np.asarray(c["K"], dtype=np.float64) for c in cams]),
                   np.stack([np.asarray(c["cam_to_bev"], dtype=np.float64) for c in cams]))

    def to_dict(self) -> Dict:
        return {"image_size": list(self.image_size),
                "cameras": [{"name": n, "K": k.tolist(), "cam_to_bev": t.tolist()} for n, k, t in zip(self.names, self.K, self.cam_to_bev)]}

    def subset(self, n: int) -> "CameraRig":
        """The first n cameras."""
        return CameraRig(self.image_size, self.names[:n], self.K[:n], self.cam_to_bev[:n])


# (name, yaw in degrees counter-clockwise from +y, mount x, mount y, focal length in pixels)
_DEFAULT_MOUNTS = (("CAM_FRONT", 0.0, 0.0, 0.8, 1260.0), ("CAM_FRONT_RIGHT", -55.0, 0.5, 0.6, 1260.0),
                   ("CAM_FRONT_LEFT", 55.0, -0.5, 0.6, 1260.0), ("CAM_BACK", 180.0, 0.0, -1.0, 800.0),
                   ("CAM_BACK_LEFT", 110.0, -0.5, -0.4, 1260.0), ("CAM_BACK_RIGHT", -110.0, 0.5, -0.4, 1260.0))


def default_rig() -> CameraRig:
    """A fixed nuScenes-LIKE six-camera rig at 900 x 1600 -- an approximation of the dataset's layout so that configs and tests
    work without data, NOT a calibration: pass CameraRig.from_info(info) for real frames.

    Intrinsics fx = fy = 1260, cx = 800, cy = 450 (about 65 degrees horizontal field of view) for the five forward / side cameras,
    fx = fy = 800 for CAM_BACK (about 90 degrees).  Optical axes horizontal; in the LiDAR frame (x right, y forward, z up) a camera of
    yaw psi (counter-clockwise from +y) has x_cam -> (cos psi, sin psi, 0), y_cam -> (0, 0, -1), z_cam -> (-sin psi, cos psi, 0).
    Yaws 0, -55, +55, 180, +110, -110 degrees in CAM_ORDER; mounts within 1 m of the LiDAR at z = -0.3 m."""
    Ks, Ts = [], []
    for _, yaw, mx, my, f in _DEFAULT_MOUNTS:
        Ks.append(np.array([[f, 0.0, 800.0], [0.0, f, 450.0], [0.0, 0.0, 1.0]]))
        p = math.radians(yaw)
        T = np.eye(4)
        T[:3, 0] = (math.cos(p), math.sin(p), 0.0)
        T[:3, 1] = (0.0, 0.0, -1.0)
        T[:3, 2] = (-math.sin(p), math.cos(p), 0.0)
        T[:3, 3] = (mx, my, -0.3)
        Ts.append(T)
    return CameraRig((900, 1600), tuple(m[0] for m in _DEFAULT_MOUNTS), np.stack(Ks), np.stack(Ts))


def calib_matrices(rigs: Sequence[CameraRig]) -> np.ndarray:
    """fp64 [B, ncam, 4, 4] for a sequence of B rigs (one per frame; same image_size and camera count): per camera, with
    E = cam_to_bev^-1, rows 0-2 = K . E[0:3] and row 3 = E[2] -- a BEV point p = (x, y, z, 1) has depth row3 . p and pixel
    (u, v) = (row0 . p, row1 . p) / (row2 . p).  The `camera_calib=` input of the 'project' and 'frustum' branches (device table
    builds).  Row 2 equals row 3 because the last row of K is (0, 0, 1); the 'frustum' branch relies on that (frustum_points)."""
    rigs = list(rigs)
    if not rigs or not all(isinstance(r, CameraRig) for r in rigs):
        raise ValueError("calib_matrices: expected a non-empty sequence of camera_rig.CameraRig")
    first = rigs[0]
    out = np.empty((len(rigs), first.num_cameras, 4, 4), dtype=np.float64)
    for b, r in enumerate(rigs):
        if r.image_size != first.image_size or r.num_cameras != first.num_cameras:
            raise ValueError(f"calib_matrices: frame {b} has image_size {r.image_size} and {r.num_cameras} cameras, frame 0 has "
                             f"{first.image_size} and {first.num_cameras}")
        for c in range(r.num_cameras):
            E = np.linalg.inv(r.cam_to_bev[c])
            out[b, c, :3] = r.K[c] @ E[:3]
            out[b, c, 3] = E[2]
    return out


def _axis_rotation(axis: int, deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def jittered_rig(seed: int, rig: Optional[CameraRig] = None) -> CameraRig:
    """`rig` (default_rig() unless given) with a seeded jitter per camera, for tests and benchmarks of per-frame calibration: yaw /
    pitch / roll (about z / x / y of the BEV frame, applied as Rz . Rx . Ry in front of the camera's rotation) each uniform in +-3
    degrees, mount +-0.3 m per axis, focal length +-10 %, principal point +-20 px per axis; numpy.random.default_rng(seed)."""
    g = np.random.default_rng(seed)
    rig = default_rig() if rig is None else rig
    K, T = rig.K.copy(), rig.cam_to_bev.copy()
    for c in range(rig.num_cameras):
        yaw, pitch, roll = g.uniform(-3.0, 3.0, 3)
        T[c, :3, :3] = _axis_rotation(2, yaw) @ _axis_rotation(0, pitch) @ _axis_rotation(1, roll) @ T[c, :3, :3]
        T[c, :3, 3] += g.uniform(-0.3, 0.3, 3)
        f = 1.0 + g.uniform(-0.1, 0.1)
        K[c, 0, 0] *= f
        K[c, 1, 1] *= f
        K[c, :2, 2] += g.uniform(-20.0, 20.0, 2)
    return CameraRig(rig.image_size, rig.names, K, T)


def view_transform_kind(camera_view_transform: Optional[str] = None, config: Optional[Dict] = None) -> str:
    """'frustum', 'lift', 'project' or 'mean' from the keyword, else `model.bev_fusion.camera_view_transform` of the config, else 'mean'
    (any letter case); anything else raises."""
    t = camera_view_transform
    if t is None and config is not None:
        t = (config.get("model", {}).get("bev_fusion", {}) or {}).get("camera_view_transform")
    if t is None:
        return "mean"
    k = str(t).strip().lower()
    if k not in VIEW_TRANSFORMS:
        raise ValueError(f"camera_view_transform must be 'mean', 'project' or 'lift' (or 'frustum'), got {t!r}")
    return k


def camera_bev_settings(config: Optional[Dict] = None) -> Tuple[int, float, CameraRig]:
    """(num_heights, min_depth, rig) from `model.bev_fusion.camera_bev` ({num_heights: 8, min_depth: 0.1, rig: {...}}); the rig
    entry is CameraRig.from_dict's form, absent -> default_rig()."""
    cb = ((config or {}).get("model", {}).get("bev_fusion", {}) or {}).get("camera_bev", {}) or {}
    nh = int(cb.get("num_heights", DEFAULT_NUM_HEIGHTS))
    md = float(cb.get("min_depth", DEFAULT_MIN_DEPTH))
    if nh <= 0 or not md > 0.0:
        raise ValueError(f"camera_bev: num_heights must be > 0 and min_depth > 0, got {nh}, {md}")
    rig = CameraRig.from_dict(cb["rig"]) if cb.get("rig") else default_rig()
    return nh, md, rig


def check_depth_settings(bins, depth_min, depth_max, min_depth: float = DEFAULT_MIN_DEPTH) -> Tuple[int, float, float]:
    """(D, depth_min, depth_max) of the 'lift' / 'frustum' branches' uniform bins, checked: D an integer in 1..64, 0 < min_depth <= depth_min <
    depth_max; ValueError otherwise."""
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= int(bins) <= MAX_DEPTH_BINS:
        raise ValueError(f"camera_bev.depth: bins must be an integer in 1..{MAX_DEPTH_BINS}, got {bins!r}")
    lo, hi, md = float(depth_min), float(depth_max), float(min_depth)
    if not (0.0 < md <= lo < hi) or not math.isfinite(hi):
        raise ValueError(f"camera_bev.depth: need 0 < min_depth <= min < max, got min_depth {md}, min {lo}, max {hi}")
    return int(bins), lo, hi


def camera_lift_settings(config: Optional[Dict] = None, min_depth: float = DEFAULT_MIN_DEPTH) -> Tuple[int, float, float]:
    """(bins, min, max) from `model.bev_fusion.camera_bev.depth` ({bins: 32, min: 1.0, max: 65.0}), checked against min_depth."""
    cb = ((config or {}).get("model", {}).get("bev_fusion", {}) or {}).get("camera_bev", {}) or {}
    d = cb.get("depth", {}) or {}
    return check_depth_settings(d.get("bins", DEFAULT_DEPTH_BINS), d.get("min", DEFAULT_DEPTH_MIN), d.get("max", DEFAULT_DEPTH_MAX),
                                min_depth)


# ---- the projection table ----------------------------------------------------------------------------------------------------------

@dataclass
class ProjectionTable:
    """Sparse lift matrix A [P cells][ncam*Hc*Wc pixels] as CSR by cell (row_ptr int32 [P+1], col int32 = cam*Hc*Wc + y*Wc + x,
    w fp32) and its exact transpose as CSR by pixel (t_row_ptr [ncam*Hc*Wc+1], t_col = cell, t_w): same entries, fp32 weights.
    w64: the merged fp64 weights before rounding (host checks)."""
    P: int
    ncols: int
    row_ptr: np.ndarray
    col: np.ndarray
    w: np.ndarray
    t_row_ptr: np.ndarray
    t_col: np.ndarray
    t_w: np.ndarray
    w64: np.ndarray

    @property
    def nnz(self) -> int:
        return int(self.col.shape[0])


def cell_centres(pc_range, bev_h: int, bev_w: int) -> Tuple[np.ndarray, np.ndarray]:
    """(x [bev_w], y [bev_h]) fp64 cell centres, exactly the pillar grid's: x0 + (j + 1/2) vx, y0 + (i + 1/2) vy, with x0, y0, vx, vy
    the fp32 values of encoders.pillar_grid (row i = y, column j = x)."""
    from .encoders import pillar_grid
    x0, y0, vx, vy, _ = pillar_grid(pc_range, bev_h, bev_w)
    xs = np.float64(x0) + (np.arange(bev_w, dtype=np.float64) + 0.5) * np.float64(vx)
    ys = np.float64(y0) + (np.arange(bev_h, dtype=np.float64) + 0.5) * np.float64(vy)
    return xs, ys


def height_centres(pc_range, num_heights: int) -> np.ndarray:
    z0, z1 = float(np.float32(pc_range[2])), float(np.float32(pc_range[5]))
    return z0 + (np.arange(num_heights, dtype=np.float64) + 0.5) * (z1 - z0) / num_heights


def _camera_samples(rig: CameraRig, Hc: int, Wc: int, pc_range, bev_h: int, bev_w: int, num_heights: int, min_depth: float):
    """The shared fp64 sample geometry of build_projection_table and build_lift_table: per camera c, for its (cell, height) samples
    in front of it (depth > min_depth) whose pixel lies inside the image, yields (c, cell index, depth q_z, u_f, v_f) with
    (u_f, v_f) the feature-map coordinates; samples in (cell, height) order."""
    H, W = rig.image_size
    xs, ys = cell_centres(pc_range, bev_h, bev_w)
    zs = height_centres(pc_range, num_heights)
    P = bev_h * bev_w
    gy, gx = np.meshgrid(ys, xs, indexing="ij")                                  # [bev_h][bev_w]
    pts = np.empty((P, num_heights, 4), dtype=np.float64)
    pts[..., 0] = gx.reshape(P, 1)
    pts[..., 1] = gy.reshape(P, 1)
    pts[..., 2] = zs.reshape(1, num_heights)
    pts[..., 3] = 1.0
    pts = pts.reshape(-1, 4)                                                      # sample s = cell * num_heights + k
    cell_of = np.repeat(np.arange(P, dtype=np.int64), num_heights)
    for c in range(rig.num_cameras):
        q = pts @ np.linalg.inv(rig.cam_to_bev[c]).T
        depth = q[:, 2]
        front = depth > min_depth
        uvw = q[front, :3] @ rig.K[c].T
        u = uvw[:, 0] / uvw[:, 2]
        v = uvw[:, 1] / uvw[:, 2]
        inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        u, v = u[inside], v[inside]
        yield c, cell_of[front][inside], depth[front][inside], (u + 0.5) * Wc / W - 0.5, (v + 0.5) * Hc / H - 0.5


def _bilinear_taps(uf: np.ndarray, vf: np.ndarray, Hc: int, Wc: int):
    """The four bilinear taps of the samples at (uf, vf): yields (inside-the-map mask, pixel index y * Wc + x, weight) per tap."""
    x0 = np.floor(uf)
    y0 = np.floor(vf)
    lx, ly = uf - x0, vf - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    for dy, wy in ((0, 1.0 - ly), (1, ly)):
        for dx, wx in ((0, 1.0 - lx), (1, lx)):
            xi, yi = x0 + dx, y0 + dy
            yield (xi >= 0) & (xi < Wc) & (yi >= 0) & (yi < Hc), yi * Wc + xi, wx * wy


def build_projection_table(rig: CameraRig, Hc: int, Wc: int, pc_range, bev_h: int, bev_w: int,
                           num_heights: int = DEFAULT_NUM_HEIGHTS, min_depth: float = DEFAULT_MIN_DEPTH) -> ProjectionTable:
    """The lift of rig's cameras (feature maps Hc x Wc each) onto the bev_h x bev_w grid of pc_range, in fp64:

    sample (cell, height k, camera c) at p = (x_j, y_i, z_k): q = cam_to_bev[c]^-1 p; valid when q_z > min_depth and the pixel
    (u, v) = (K q / q_z)[:2] lies in [0, W) x [0, H) of rig.image_size; its value is the bilinear sample of the feature map at
    u_f = (u + 1/2) Wc / W - 1/2, v_f = (v + 1/2) Hc / H - 1/2 with taps outside the map reading zero (= F.grid_sample,
    align_corners=False, padding_mode='zeros', at gx = (2u + 1) / W - 1).  Cell value = mean over its valid samples, 0 without one.
    Duplicate (cell, pixel) entries are merged in fp64 before rounding to fp32; exact-zero weights are dropped."""
    P = bev_h * bev_w
    ncam = rig.num_cameras
    rows, cols, wts = [], [], []
    count = np.zeros(P, dtype=np.int64)
    for c, cells, _, uf, vf in _camera_samples(rig, Hc, Wc, pc_range, bev_h, bev_w, num_heights, min_depth):
        np.add.at(count, cells, 1)
        for ok, pix, wt in _bilinear_taps(uf, vf, Hc, Wc):
            rows.append(cells[ok])
            cols.append(c * Hc * Wc + pix[ok])
            wts.append(wt[ok])
    ncols = ncam * Hc * Wc
    r = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cl = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    wt = np.concatenate(wts) if wts else np.zeros(0, np.float64)
    wt = wt / np.maximum(count[r], 1)
    key = r * ncols + cl
    uniq, inv = np.unique(key, return_inverse=True)                               # sorted by (cell, pixel)
    merged = np.bincount(inv, weights=wt, minlength=uniq.shape[0])
    keep = merged != 0.0
    uniq, merged = uniq[keep], merged[keep]
    r, cl = uniq // ncols, uniq % ncols
    w32 = merged.astype(np.float32)
    if P * ncols >= 2 ** 63 or ncols >= 2 ** 31 or r.shape[0] >= 2 ** 31:
        raise ValueError("projection table too large for int32 indices")
    row_ptr = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=P), out=row_ptr[1:])
    order = np.lexsort((r, cl))                                                   # by pixel, then cell
    t_row_ptr = np.zeros(ncols + 1, dtype=np.int64)
    np.cumsum(np.bincount(cl, minlength=ncols), out=t_row_ptr[1:])
    return ProjectionTable(P, ncols, row_ptr.astype(np.int32), cl.astype(np.int32), w32,
                           t_row_ptr.astype(np.int32), r[order].astype(np.int32), w32[order], merged)


def apply_table_fp64(t: ProjectionTable, feats: np.ndarray) -> np.ndarray:
    """CPU fp64 application of the cell table with its fp64 weights: feats [B][ncols][C] -> [B][P][C] (host tests)."""
    B, _, C = feats.shape
    out = np.zeros((B, t.P, C), dtype=np.float64)
    rows = np.repeat(np.arange(t.P), np.diff(t.row_ptr))
    w = t.w64
    for b in range(B):
        np.add.at(out[b], rows, feats[b][t.col] * w[:, None])
    return out


# ---- the lift table (learned depth) ---------------------------------------------------------------------------------------------

@dataclass
class LiftTable:
    """The projection table with a depth bin per entry (camera_view_transform 'lift'): CSR by cell, sorted by (cell, pixel, bin),
    col2 int32 = pixel * D + bin, w fp32; and its exact transpose as CSR by pixel (t_row_ptr [ncols + 1]), sorted by (pixel, cell,
    bin): t_cell, t_bin int32, t_w the bit-identical fp32 weight.  w64: the merged fp64 weights before rounding (host checks)."""
    P: int
    ncols: int
    D: int
    row_ptr: np.ndarray
    col2: np.ndarray
    w: np.ndarray
    t_row_ptr: np.ndarray
    t_cell: np.ndarray
    t_bin: np.ndarray
    t_w: np.ndarray
    w64: np.ndarray

    @property
    def nnz(self) -> int:
        return int(self.col2.shape[0])


def depth_bin_of(depth: np.ndarray, depth_bins: int, depth_min: float, depth_max: float) -> np.ndarray:
    """floor((q_z - depth_min) * D / (depth_max - depth_min)), clamped to D - 1 (fp64; for depth_min <= q_z < depth_max)."""
    b = np.floor((depth - depth_min) * depth_bins / (depth_max - depth_min)).astype(np.int64)
    return np.minimum(b, depth_bins - 1)


def build_lift_table(rig: CameraRig, Hc: int, Wc: int, pc_range, bev_h: int, bev_w: int, num_heights: int = DEFAULT_NUM_HEIGHTS,
                     min_depth: float = DEFAULT_MIN_DEPTH, depth_bins: int = DEFAULT_DEPTH_BINS,
                     depth_min: float = DEFAULT_DEPTH_MIN, depth_max: float = DEFAULT_DEPTH_MAX) -> LiftTable:
    """build_projection_table's samples and fp64 geometry with a depth bin per sample: a sample is valid when the projection's
    conditions hold and depth_min <= q_z < depth_max; its bin is depth_bin_of(q_z) and each of its four bilinear taps carries that
    bin; weight = tap weight / the cell's count of valid samples.  Duplicate (cell, pixel, bin) entries are merged in fp64 before
    the single rounding to fp32, exact zeros dropped.  With D = 1, depth_min = min_depth and depth_max beyond every sample this is
    the projection table."""
    D, depth_min, depth_max = check_depth_settings(depth_bins, depth_min, depth_max, min_depth)
    P, ncols = bev_h * bev_w, rig.num_cameras * Hc * Wc
    if ncols * D >= 2 ** 31 or P * ncols * D >= 2 ** 63:
        raise ValueError(f"lift table: {ncols} pixels x {D} bins do not fit int32 columns")
    rows, cols, bns, wts = [], [], [], []
    count = np.zeros(P, dtype=np.int64)
    for c, cells, depth, uf, vf in _camera_samples(rig, Hc, Wc, pc_range, bev_h, bev_w, num_heights, min_depth):
        ranged = (depth >= depth_min) & (depth < depth_max)
        cells, depth, uf, vf = cells[ranged], depth[ranged], uf[ranged], vf[ranged]
        np.add.at(count, cells, 1)
        sample_bin = depth_bin_of(depth, D, depth_min, depth_max)
        for ok, pix, wt in _bilinear_taps(uf, vf, Hc, Wc):
            rows.append(cells[ok])
            cols.append(c * Hc * Wc + pix[ok])
            bns.append(sample_bin[ok])
            wts.append(wt[ok])
    r = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cl = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    bn = np.concatenate(bns) if bns else np.zeros(0, np.int64)
    wt = np.concatenate(wts) if wts else np.zeros(0, np.float64)
    wt = wt / np.maximum(count[r], 1)
    key = (r * ncols + cl) * D + bn
    uniq, inv = np.unique(key, return_inverse=True)                               # sorted by (cell, pixel, bin)
    merged = np.bincount(inv.reshape(-1), weights=wt, minlength=uniq.shape[0])
    keep = merged != 0.0
    uniq, merged = uniq[keep], merged[keep]
    r, c2 = uniq // (ncols * D), uniq % (ncols * D)
    if r.shape[0] >= 2 ** 31:
        raise ValueError("lift table too large for int32 indices")
    w32 = merged.astype(np.float32)
    row_ptr = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=P), out=row_ptr[1:])
    cl, bn = c2 // D, c2 % D
    order = np.lexsort((bn, r, cl))                                               # by pixel, then cell, then bin
    t_row_ptr = np.zeros(ncols + 1, dtype=np.int64)
    np.cumsum(np.bincount(cl, minlength=ncols), out=t_row_ptr[1:])
    return LiftTable(P, ncols, D, row_ptr.astype(np.int32), c2.astype(np.int32), w32, t_row_ptr.astype(np.int32),
                     r[order].astype(np.int32), bn[order].astype(np.int32), w32[order], merged)


def apply_lift_table_fp64(t: LiftTable, feats: np.ndarray, pd: np.ndarray) -> np.ndarray:
    """CPU fp64 application of the lift table with its fp64 weights: feats [B][ncols][C], pd [B][ncols][D] -> [B][P][C]."""
    B, _, C = feats.shape
    out = np.zeros((B, t.P, C), dtype=np.float64)
    rows = np.repeat(np.arange(t.P), np.diff(t.row_ptr))
    pix = t.col2 // t.D
    for b in range(B):
        np.add.at(out[b], rows, feats[b][pix] * (t.w64 * pd[b].reshape(-1)[t.col2])[:, None])
    return out


# ---- the frustum table (lift-splat) ---------------------------------------------------------------------------------------------

@dataclass
class FrustumTable:
    """The lift-splat map of camera_view_transform 'frustum': every (feature pixel, depth bin) col2 = pixel * D + bin lands in at
    most one BEV cell.  cell_of int32 [ncols * D] (-1: outside the grid or the z range), and the same map as CSR by cell: row_ptr
    int32 [P + 1], col2 int32, every row in ascending col2.  No weights: each entry counts 1.  points: the fp64 frustum points
    [ncols * D][3] (host checks)."""
    P: int
    ncols: int
    D: int
    cell_of: np.ndarray
    row_ptr: np.ndarray
    col2: np.ndarray
    points: np.ndarray

    @property
    def nnz(self) -> int:
        return int(self.col2.shape[0])


def frustum_points(calib: np.ndarray, image_size, Hc: int, Wc: int, depth_bins: int, depth_min: float, depth_max: float) -> np.ndarray:
    """fp64 [B][ncam * Hc * Wc * D][3]: the BEV-frame point of every (camera, feature pixel (x, y), depth bin d), index
    (cam * Hc * Wc + y * Wc + x) * D + d, from calib [B][ncam][4][4] (calib_matrices / augment.augmented_calib): with rows 0-2 =
    [A | t], the point of image position u = (x + 1/2) W / Wc - 1/2, v = (y + 1/2) H / Hc - 1/2 (the inverse of the 'project'
    branch's u_f, v_f) at the bin's centre depth z_d = depth_min + (d + 1/2) (depth_max - depth_min) / D is
    p = A^-1 (z_d (u, v, 1)^T - t).  This needs the calibration's third row to be its depth row (row 2 == row 3), which both
    producers keep: the last row of K and of every image map is (0, 0, 1)."""
    calib = np.asarray(calib, dtype=np.float64)
    B, ncam = calib.shape[:2]
    H, W = image_size
    u = (np.arange(Wc, dtype=np.float64) + 0.5) * W / Wc - 0.5
    v = (np.arange(Hc, dtype=np.float64) + 0.5) * H / Hc - 0.5
    z = depth_min + (np.arange(depth_bins, dtype=np.float64) + 0.5) * (depth_max - depth_min) / depth_bins
    ray = np.empty((Hc, Wc, depth_bins, 3), dtype=np.float64)
    ray[..., 0] = u[None, :, None] * z
    ray[..., 1] = v[:, None, None] * z
    ray[..., 2] = z
    ray = ray.reshape(-1, 3)
    out = np.empty((B, ncam, ray.shape[0], 3), dtype=np.float64)
    for b in range(B):
        for c in range(ncam):
            out[b, c] = (ray - calib[b, c, :3, 3]) @ np.linalg.inv(calib[b, c, :3, :3]).T
    return out.reshape(B, -1, 3)


def frustum_cells(points: np.ndarray, pc_range, bev_h: int, bev_w: int) -> np.ndarray:
    """int32 cell i * bev_w + j of every point [..., 3], -1 when invalid: j = floor((p_x - x0) / vx), i = floor((p_y - y0) / vy)
    with the fp32 grid values of encoders.pillar_grid taken in fp64; valid when 0 <= j < bev_w, 0 <= i < bev_h and z0 <= p_z < z1
    (the fp32 z limits)."""
    from .encoders import pillar_grid
    x0, y0, vx, vy, _ = pillar_grid(pc_range, bev_h, bev_w)
    z0, z1 = float(np.float32(pc_range[2])), float(np.float32(pc_range[5]))
    with np.errstate(invalid="ignore"):
        fj = np.floor((points[..., 0] - np.float64(x0)) / np.float64(vx))
        fi = np.floor((points[..., 1] - np.float64(y0)) / np.float64(vy))
        valid = (fj >= 0) & (fj < bev_w) & (fi >= 0) & (fi < bev_h) & (points[..., 2] >= z0) & (points[..., 2] < z1)
    cell = np.where(valid, fi, 0).astype(np.int64) * bev_w + np.where(valid, fj, 0).astype(np.int64)
    return np.where(valid, cell, -1).astype(np.int32)


def build_frustum_table(rig: CameraRig, Hc: int, Wc: int, pc_range, bev_h: int, bev_w: int, depth_bins: int = DEFAULT_DEPTH_BINS,
                        depth_min: float = DEFAULT_DEPTH_MIN, depth_max: float = DEFAULT_DEPTH_MAX) -> FrustumTable:
    """The lift-splat table of rig's cameras (feature maps Hc x Wc each, D uniform depth bins) on the bev_h x bev_w grid of
    pc_range, in fp64 from calib_matrices([rig]) -- what bevf_frustum_table_build_f64 builds per frame on the device
    (frustum_points, frustum_cells)."""
    D, depth_min, depth_max = check_depth_settings(depth_bins, depth_min, depth_max, min(DEFAULT_MIN_DEPTH, float(depth_min)))
    P, ncols = bev_h * bev_w, rig.num_cameras * Hc * Wc
    if ncols * D >= 2 ** 31:
        raise ValueError(f"frustum table: {ncols} pixels x {D} bins do not fit int32 columns")
    pts = frustum_points(calib_matrices([rig]), rig.image_size, Hc, Wc, D, depth_min, depth_max)[0]
    cell_of = frustum_cells(pts, pc_range, bev_h, bev_w)
    c2 = np.nonzero(cell_of >= 0)[0]
    order = np.argsort(cell_of[c2], kind="stable")                                # by cell, ascending col2 inside a cell
    row_ptr = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(np.bincount(cell_of[c2], minlength=P), out=row_ptr[1:])
    return FrustumTable(P, ncols, D, cell_of, row_ptr.astype(np.int32), c2[order].astype(np.int32), pts)

