"""TEST INFRASTRUCTURE -- numpy restatements of the augmentation kernels (csrc/augment.hip) and the seeded scenes the GPU tests run
(tests/test_augment_host.py checks their margin conditions on the CPU, tests/test_gpu_augment.py runs them on the MI355X).

The photometric restatement is written once and evaluated in a chosen dtype: float64 is the reference; float32 is the same
arithmetic the kernel does, operation by operation (numpy rounds every operation to the array's dtype and fuses nothing), on the
host.  Its worst distance to the fp64 result over the test images sets the GPU test's tolerance (4 x that distance)."""
import math

import numpy as np

from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR

RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
PREC = 22


# ---- resize --------------------------------------------------------------------------------------------------------------------------

def resize_box_ref(img: np.ndarray, window, out_size):
    """Pillow's two integer passes with augment.resample_tables_box's coefficients: img (H, W, 3) uint8, window (x0, x1, y0, y1),
    out_size (Ho, Wo) -> (Ho, Wo, 3) uint8."""
    H, W, _ = img.shape
    Ho, Wo = out_size
    x0, x1, y0, y1 = (int(v) for v in window)
    bh, kh, _ = A.resample_tables_box(W, x0, x1, Wo)
    bv, kv, _ = A.resample_tables_box(H, y0, y1, Ho)
    src = img.astype(np.int64)
    hor = np.zeros((H, Wo, 3), dtype=np.int64)
    for ox in range(Wo):
        s, n = bh[ox]
        acc = (src[:, s:s + n, :] * kh[ox, :n].astype(np.int64)[None, :, None]).sum(1) + (1 << (PREC - 1))
        hor[:, ox] = np.clip(acc >> PREC, 0, 255)
    out = np.zeros((Ho, Wo, 3), dtype=np.uint8)
    for oy in range(Ho):
        s, n = bv[oy]
        acc = (hor[s:s + n] * kv[oy, :n].astype(np.int64)[:, None, None]).sum(0) + (1 << (PREC - 1))
        out[oy] = np.clip(acc >> PREC, 0, 255).astype(np.uint8)
    return out


def pillow_resize_box(img: np.ndarray, window, out_size):
    from PIL import Image
    x0, x1, y0, y1 = (int(v) for v in window)
    bil = getattr(Image, "Resampling", Image).BILINEAR
    return np.asarray(Image.fromarray(img).resize((out_size[1], out_size[0]), bil, box=(x0, y0, x1, y1)))


def gray_sum_ref(img_u8: np.ndarray) -> int:
    p = img_u8.astype(np.int64)
    return int(((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).sum())


def window_cases(Hs: int, Ws: int):
    """(x0, x1, y0, y1): the full frame, windows touching each border, interior windows of several sizes."""
    return [(0, Ws, 0, Hs), (0, Ws // 2, 3, Hs - 5), (Ws // 3, Ws, 2, Hs // 2 + 7), (5, Ws - 9, 0, Hs - 11), (7, Ws - 3, Hs // 4, Hs),
            (Ws // 4, Ws // 4 + Ws // 5, Hs // 3, Hs // 3 + Hs // 5), (11, Ws - 13, 9, Hs - 6)]


# (source (Hs, Ws), out (Ho, Wo)): down-scales (the windows of window_cases make some of them up-scales), an up-scale, a mixed one
SIZE_CASES = [((90, 160), (45, 80)), ((97, 131), (44, 80)), ((30, 40), (64, 96)), ((120, 100), (40, 120)), ((200, 320), (32, 48))]


def make_image(Hs: int, Ws: int, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    img[..., 0] = (img[..., 0] // 4 + (xx * 191 // max(Ws - 1, 1))).astype(np.uint8)       # a ramp, so that a flip or a shift shows
    img[: Hs // 6] = 255
    img[Hs // 6: Hs // 4] = 0
    return img


# ---- photometric ---------------------------------------------------------------------------------------------------------------------

def jitter_ref(img_u8: np.ndarray, gray_sum: int, jit, flip: bool, mean, std, dtype=np.float64) -> np.ndarray:
    """(Ho, Wo, 3) uint8 -> (3, Ho, Wo) in `dtype`: the kernel's steps in its order (contrast, brightness, saturation, hue, flip,
    normalise), every operation in `dtype`."""
    f = dtype
    Ho, Wo, _ = img_u8.shape
    x = img_u8.astype(f) / f(255.0)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    fc, fb, fs, dh = (f(np.float32(v)) for v in jit)                       # the factors reach the kernel as fp32
    one, zero = f(1.0), f(0.0)

    def clamp(v):
        return np.minimum(np.maximum(v, zero), one)
    if fc != one:
        m = f(np.float32(gray_sum / float(Ho * Wo) / 255.0)) if f is np.float32 else f(gray_sum / float(Ho * Wo) / 255.0)
        om = (one - fc) * m
        r, g, b = clamp(fc * r + om), clamp(fc * g + om), clamp(fc * b + om)
    if fb != one:
        r, g, b = clamp(fb * r), clamp(fb * g), clamp(fb * b)
    if fs != one:
        gr = f(np.float32(0.299)) * r + f(np.float32(0.587)) * g + f(np.float32(0.114)) * b if f is np.float32 else \
            0.299 * r + 0.587 * g + 0.114 * b
        og = (one - fs) * gr
        r, g, b = clamp(fs * r + og), clamp(fs * g + og), clamp(fs * b + og)
    if dh != zero:
        maxc = np.maximum(r, np.maximum(g, b))
        minc = np.minimum(r, np.minimum(g, b))
        eqc = maxc == minc
        cr = maxc - minc
        s = cr / np.where(eqc, one, maxc)
        crd = np.where(eqc, one, cr)
        rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
        h = np.where(maxc == r, bc - gc, np.where(maxc == g, f(2.0) + rc - bc, f(4.0) + gc - rc))
        h = h / f(6.0) + one
        h = h - np.floor(h)
        h = h + dh
        h = h - np.floor(h)
        v = maxc
        h6 = h * f(6.0)
        fl = np.floor(h6)
        ff = h6 - fl
        i = fl.astype(np.int64) % 6
        p = clamp(v * (one - s))
        q = clamp(v * (one - s * ff))
        t = clamp(v * (one - s * (one - ff)))
        r = np.choose(i, [v, q, p, p, t, v])
        g = np.choose(i, [t, v, v, q, p, p])
        b = np.choose(i, [p, p, t, v, v, q])
    out = np.stack([r, g, b], 0).astype(f)
    if flip:
        out = out[:, :, ::-1]
    mean = np.asarray(mean, dtype=np.float32).astype(f).reshape(3, 1, 1)
    std = np.asarray(std, dtype=np.float32).astype(f).reshape(3, 1, 1)
    return ((out - mean) / std).astype(f)


# (contrast, brightness, saturation, hue shift): every factor alone at both ends, all together, and a wrap of the hue circle
JITTER_CASES = [(0.8, 1.0, 1.0, 0.0), (1.2, 1.0, 1.0, 0.0), (1.0, 0.8, 1.0, 0.0), (1.0, 1.2, 1.0, 0.0), (1.0, 1.0, 0.8, 0.0),
                (1.0, 1.0, 1.2, 0.0), (1.0, 1.0, 1.0, 0.1), (1.0, 1.0, 1.0, -0.1), (0.83, 1.17, 0.91, 0.07), (1.19, 0.85, 1.2, -0.093),
                (1.05, 0.97, 0.0, 0.5), (1.0, 1.0, 1.0, -0.5)]


# ---- world transform scenes ---------------------------------------------------------------------------------------------------------

def scene_transforms():
    """Five frames: the four flip combinations with rotation, scale and translation, and a rotation-free fifth."""
    rs = np.random.RandomState(77)
    T, s = [], []
    for b, (fx, fy) in enumerate([(False, False), (True, False), (False, True), (True, True), (True, False)]):
        sc = float(rs.uniform(0.95, 1.05))
        th = math.radians(float(rs.uniform(-45.0, 45.0))) if b < 4 else 0.0
        t = rs.normal(0.0, 1.0, 3) * np.array([0.5, 0.5, 0.2])
        T.append(A.world_transform(fx, fy, th, sc, t))
        s.append(sc)
    return np.stack(T), np.array(s)


LIDAR_N, LIDAR_MAX, LIDAR_C = 3000, 1000, 5
LIDAR_COUNTS = (0, 1, 600, 1000, 3000)          # n_in per frame: none, one, fewer than / exactly / more than max_points
MARGIN = 1e-3


def transform_points_ref(T: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """fp64: (N, >=3) through the 4x4 T (positions only)."""
    p = pts[:, :3].astype(np.float64)
    return p @ T[:3, :3].T + T[:3, 3]


def face_distance(p: np.ndarray, rng=RANGE) -> np.ndarray:
    lo, hi = np.array(rng[:3]), np.array(rng[3:])
    return np.minimum(np.abs(p - lo), np.abs(p - hi)).min(1)


def lidar_scene():
    """(points (B, N, C) fp32, counts (B,), T (B, 4, 4), s (B,)): channels x y z intensity ... with velocity in channels 3-4.  A point
    that the fp64 transform brings within 2e-3 m of a face of RANGE is replaced by a fixed interior point, so that the margin
    condition (1e-3 m) holds by construction and the GPU test excludes nothing."""
    T, s = scene_transforms()
    rs = np.random.RandomState(2024)
    B = len(LIDAR_COUNTS)
    pts = np.stack([rs.uniform(-60, 60, (B, LIDAR_N)), rs.uniform(-60, 60, (B, LIDAR_N)), rs.uniform(-6, 4, (B, LIDAR_N)),
                    rs.uniform(-10, 10, (B, LIDAR_N)), rs.uniform(-10, 10, (B, LIDAR_N))], 2).astype(np.float32)
    pts[1, 0, :3] = (3.0, 4.0, 0.5)                         # the one point of frame 1 survives
    for b in range(B):
        near = face_distance(transform_points_ref(T[b], pts[b])) < 2 * MARGIN
        pts[b, near, :3] = (1.5, -2.5, 0.25)
    return pts, np.array(LIDAR_COUNTS, dtype=np.int32), T, s


def lidar_ref(pts: np.ndarray, count: int, T: np.ndarray, max_points: int, vel_ch=None):
    """fp64 reference of one frame: (out (max_points, C), number of survivors, indices of the survivors kept)."""
    p = pts[:count]
    q = transform_points_ref(T, p)
    lo, hi = np.array(RANGE[:3]), np.array(RANGE[3:])
    keep = np.nonzero(((q > lo) & (q < hi)).all(1))[0]
    out = np.zeros((max_points, pts.shape[1]))
    sel = keep[:max_points]
    rows = p[sel].astype(np.float64)
    rows[:, :3] = q[sel]
    if vel_ch is not None:
        v = p[sel][:, list(vel_ch)].astype(np.float64)
        rows[:, list(vel_ch)] = v @ T[:2, :2].T
    out[:len(sel)] = rows
    return out, len(keep), sel


BOX_M, BOX_PAD = 40, 10


def wrap_distance(yaw: np.ndarray) -> np.ndarray:
    return np.pi - np.abs(yaw)


def boxes_ref(boxes: np.ndarray, labels: np.ndarray, vel, T: np.ndarray, s: float):
    """fp64: one frame's boxes (M, 7|9), labels (M,), vel (M, 2) or None."""
    out = boxes.astype(np.float64).copy()
    vout = None if vel is None else vel.astype(np.float64).copy()
    ok = labels >= 0
    L2 = T[:2, :2]
    out[ok, :3] = transform_points_ref(T, boxes[ok])
    out[ok, 3:6] = boxes[ok, 3:6].astype(np.float64) * s
    yaw = boxes[ok, 6].astype(np.float64)
    hd = np.stack([np.cos(yaw), np.sin(yaw)], 1) @ L2.T
    out[ok, 6] = np.arctan2(hd[:, 1], hd[:, 0])
    if boxes.shape[1] == 9:
        out[ok, 7:9] = boxes[ok, 7:9].astype(np.float64) @ L2.T
    if vel is not None:
        vout[ok] = vel[ok].astype(np.float64) @ L2.T
    return out, vout


def box_scene(ncol: int):
    """(boxes (4, M, ncol) fp32, labels (4, M) int64 with the last BOX_PAD rows -1, vel (4, M, 2) fp32, T, s): the four flip
    combinations, each with rotation and scale.  A yaw whose transformed heading comes within 2e-3 rad of the +-pi wrap is moved by
    0.1 rad, so the margin condition (1e-3 rad) holds by construction."""
    T, s = scene_transforms()
    T, s = T[:4], s[:4]
    rs = np.random.RandomState(99 + ncol)
    B, M = 4, BOX_M
    boxes = np.zeros((B, M, ncol), dtype=np.float32)
    boxes[..., 0] = rs.uniform(-50, 50, (B, M))
    boxes[..., 1] = rs.uniform(-50, 50, (B, M))
    boxes[..., 2] = rs.uniform(-4, 2, (B, M))
    boxes[..., 3:6] = rs.uniform(0.5, 12.0, (B, M, 3))
    boxes[..., 6] = rs.uniform(-np.pi, np.pi, (B, M))
    if ncol == 9:
        boxes[..., 7:9] = rs.uniform(-15, 15, (B, M, 2))
    vel = rs.uniform(-15, 15, (B, M, 2)).astype(np.float32)
    labels = rs.randint(0, 10, (B, M)).astype(np.int64)
    labels[:, M - BOX_PAD:] = -1
    boxes[:, M - BOX_PAD:] = rs.uniform(-3, 3, (B, BOX_PAD, ncol)).astype(np.float32)     # junk the kernel must not touch
    for b in range(B):
        ref, _ = boxes_ref(boxes[b], np.zeros(M, dtype=np.int64), None, T[b], s[b])
        near = wrap_distance(ref[:, 6]) < 2e-3
        boxes[b, near, 6] += np.float32(0.1) * np.where(boxes[b, near, 6] > 0, -1, 1).astype(np.float32)
    return boxes, labels, vel, T, s


# ---- calibration ---------------------------------------------------------------------------------------------------------------------

def equivalent_rig(rig: CR.CameraRig, A3: np.ndarray, T: np.ndarray) -> CR.CameraRig:
    """The rig that sees the augmented frame: K' = A . K and cam_to_bev' = T . cam_to_bev (A3 [ncam][3][3], T [4][4])."""
    return CR.CameraRig(rig.image_size, rig.names, A3 @ rig.K, T[None] @ rig.cam_to_bev)


def calib_params(B: int = 3, ncam: int = 6, src_size=(900, 1600), out_size=(448, 800), seed: int = 5) -> "A.AugmentParams":
    """Parameters with every kind of transform switched on (flips, rotation, scale, translation, crop, image flip)."""
    st = A.AugmentSettings(camera_flip=True, camera_scale=(0.9, 1.1), flip=True, scale=(0.95, 1.05), rotation=(-20.0, 20.0),
                           translation=(0.5, 0.5, 0.2))
    p = A.sample(st, B, ncam, src_size, out_size, np.random.default_rng(seed))
    rs = np.random.RandomState(seed)
    for b in range(B):                                   # the world flips by turns, so that every combination occurs
        fx, fy = [(True, False), (False, True), (True, True), (False, False)][b % 4]
        p.scale[b] = float(rs.uniform(0.95, 1.05))
        p.bev_aug[b] = A.world_transform(fx, fy, math.radians(float(rs.uniform(-20.0, 20.0))), p.scale[b],
                                         rs.normal(0.0, 1.0, 3) * np.array([0.5, 0.5, 0.2]))
    return p
