"""Independent fp64 restatement of rotated-box IoU and greedy box NMS, and the fixed scenes the box-NMS tests share.

Pure Python / numpy, no import of the package: rectangles are clipped by half-planes (Sutherland-Hodgman) and measured by the
shoelace formula; NMS is the plain greedy loop.  Box convention: [x, y, z, w, l, h, yaw] is the rectangle centred at (x, y)
with extent l along the heading (cos yaw, sin yaw) and w across it, z-extent [z - h/2, z + h/2].

The scenes are float32 arrays (what the device receives); the reference widens those same values to fp64.
"""
import math

import numpy as np

PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)


# ---- geometry -------------------------------------------------------------------------------------------------------------------

def corners(box):
    """Counter-clockwise corners of the box's BEV rectangle."""
    x, y, w, l, yaw = float(box[0]), float(box[1]), float(box[3]), float(box[4]), float(box[6])
    c, s = math.cos(yaw), math.sin(yaw)
    hl, hw = 0.5 * l, 0.5 * w
    return [(x + c * ex * hl - s * ey * hw, y + s * ex * hl + c * ey * hw) for ex, ey in ((1, 1), (-1, 1), (-1, -1), (1, -1))]


def _clip(poly, a, b):
    """The part of convex `poly` on the left of the directed line a -> b."""
    def side(p):
        return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        sp, sq = side(p), side(q)
        if sp >= 0:
            out.append(p)
        if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
            t = sp / (sp - sq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _area(poly):
    return 0.5 * sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1]
                     for i in range(len(poly))) if len(poly) >= 3 else 0.0


def _finite(box):
    return all(math.isfinite(float(v)) for v in box[:7])


def inter_bev(a, b):
    """Area of the intersection of the two rotated rectangles."""
    poly, clipper = corners(b), corners(a)
    for i in range(4):
        if not poly:
            return 0.0
        poly = _clip(poly, clipper[i], clipper[(i + 1) % 4])
    return max(_area(poly), 0.0)


def iou_bev(a, b):
    if not (_finite(a) and _finite(b)) or min(a[3], a[4], b[3], b[4]) <= 0:
        return 0.0
    inter = inter_bev(a, b)
    return min(max(inter / (float(a[3]) * float(a[4]) + float(b[3]) * float(b[4]) - inter), 0.0), 1.0)


def iou_3d(a, b):
    if not (_finite(a) and _finite(b)) or min(a[3], a[4], a[5], b[3], b[4], b[5]) <= 0:
        return 0.0
    za, ha, zb, hb = float(a[2]), float(a[5]), float(b[2]), float(b[5])
    zo = min(za + 0.5 * ha, zb + 0.5 * hb) - max(za - 0.5 * ha, zb - 0.5 * hb)
    if zo <= 0:
        return 0.0
    iv = inter_bev(a, b) * zo
    va, vb = float(a[3]) * float(a[4]) * ha, float(b[3]) * float(b[4]) * hb
    return min(max(iv / (va + vb - iv), 0.0), 1.0)


def iou_matrix(a, b, mode="bev"):
    """(N,M) fp64 IoU.  Pairs whose circumscribed circles are disjoint (by a 1 mm margin) are 0 without being clipped; pairs
    with a non-finite distance go through the scalar functions, which define them."""
    f = iou_bev if mode == "bev" else iou_3d
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((len(a), len(b)), np.float64)
    with np.errstate(all="ignore"):
        d = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
        reach = 0.5 * np.hypot(a[:, 3], a[:, 4])[:, None] + 0.5 * np.hypot(b[:, 3], b[:, 4])[None, :] + 1e-3
        far = d > reach
    for i, j in zip(*np.nonzero(~far)):
        out[i, j] = f(a[i], b[j])
    return out


def axis_aligned_iou(a, b):
    """The arithmetic of the reference's inference.py _compute_iou_3d ("Simplified 2D BEV IoU"): w along x, l along y, no yaw."""
    x1, y1, w1, l1 = float(a[0]), float(a[1]), float(a[3]), float(a[4])
    x2, y2, w2, l2 = float(b[0]), float(b[1]), float(b[3]), float(b[4])
    ix = max(0.0, min(x1 + w1 / 2, x2 + w2 / 2) - max(x1 - w1 / 2, x2 - w2 / 2))
    iy = max(0.0, min(y1 + l1 / 2, y2 + l2 / 2) - max(y1 - l1 / 2, y2 - l2 / 2))
    inter = ix * iy
    union = w1 * l1 + w2 * l2 - inter
    return inter / union if union > 0 else 0.0


# ---- greedy NMS -----------------------------------------------------------------------------------------------------------------

def nms(boxes, mode, thresh, labels=None, post_max=None, iou=None):
    """Greedy NMS over boxes already in descending score order.  mode 'rotate': j suppresses i when IoU_bev > thresh; 'circle':
    when the squared centre distance < thresh^2.  labels: class-aware (only the same label suppresses).  iou: a precomputed
    iou_matrix(boxes, boxes) to reuse.  Returns the kept indices, in order, at most post_max of them."""
    boxes = np.asarray(boxes, np.float64)
    keep = []
    for i in range(len(boxes)):
        if post_max is not None and len(keep) >= post_max:
            break
        dead = False
        for j in keep:
            if labels is not None and int(labels[i]) != int(labels[j]):
                continue
            if mode == "rotate":
                v = iou[j, i] if iou is not None else iou_bev(boxes[j], boxes[i])
                hit = v > thresh
            else:
                hit = (boxes[i, 0] - boxes[j, 0]) ** 2 + (boxes[i, 1] - boxes[j, 1]) ** 2 < thresh * thresh
            if hit:
                dead = True
                break
        if not dead:
            keep.append(i)
    return keep


# ---- fixed scenes ---------------------------------------------------------------------------------------------------------------

def cluster_frame(rng, n):
    """n boxes: object centres over the point-cloud range, each with 3..8 jittered duplicates; sizes from pedestrian to bus."""
    kinds = np.array([[0.6, 0.7, 1.7], [0.8, 1.9, 1.4], [1.9, 4.5, 1.6], [2.4, 6.5, 2.6], [2.9, 12.0, 3.4]])
    rows = []
    while len(rows) < n:
        w, l, h = kinds[rng.integers(len(kinds))] * rng.uniform(0.9, 1.1, 3)
        cx, cy = rng.uniform(PC_RANGE[0] + 2, PC_RANGE[3] - 2, 2)
        cz, yaw = rng.uniform(-2.0, 0.5), rng.uniform(-math.pi, math.pi)
        for _ in range(int(rng.integers(3, 9))):
            j = rng.normal(0, 1, 7)
            rows.append([cx + 0.25 * w * j[0], cy + 0.25 * w * j[1], cz + 0.15 * j[2], w * (1 + 0.05 * j[3]), l * (1 + 0.05 * j[4]),
                         h * (1 + 0.05 * j[5]), yaw + 0.08 * j[6] + (math.pi if rng.random() < 0.15 else 0.0)])
    rows = np.array(rows[:n])
    return rows[rng.permutation(n)].astype(np.float32)


def cluster_scene(seed, counts, n_pad=None, num_classes=3):
    """A batch of cluster frames: boxes (B,N,7) float32 (rows past a frame's count are filler that no result may depend on),
    counts (B,) int32, labels (B,N) int64.  Row order stands for descending score."""
    rng = np.random.default_rng(seed)
    N = n_pad if n_pad is not None else max(max(counts), 1)
    boxes = rng.uniform(-5, 5, (len(counts), N, 7)).astype(np.float32)
    boxes[..., 3:6] = np.abs(boxes[..., 3:6]) + 0.5
    for b, c in enumerate(counts):
        if c:
            boxes[b, :c] = cluster_frame(rng, c)
    labels = rng.integers(0, num_classes, (len(counts), N)).astype(np.int64)
    return boxes, np.asarray(counts, np.int32), labels


# name -> (seed, per-frame counts, padded N, IoU thresholds, circle radii): 100..512 boxes per frame, B = 1..4, frames of count 0
# and 1, N not a multiple of 64; "n<k>" are single frames of exactly k boxes.  Seeds and thresholds were searched so that no
# pair's fp64 IoU lies within 1e-3 of a threshold and no centre distance within 1e-3 m of a radius (MARGIN; asserted by
# tests/test_box_nms_host.py), so fp32 and fp64 cannot disagree on a decision and the GPU tests exclude nothing.
MARGIN = 1e-3
SCENES = {
    "b1_n512": (14, [512], 512, (0.224, 0.481), (1.0, 2.49)),
    "b2_n300": (2, [300, 137], 300, (0.193, 0.469), (1.0, 2.49)),
    "b3_edge": (1, [0, 1, 203], 203, (0.185, 0.482), (1.02, 2.5)),
    "b4_mixed": (82, [100, 512, 64, 65], 512, (0.159, 0.698), (1.0, 2.5)),
    "n1": (1, [1], 1, (0.2, 0.5), (1.0, 2.5)),
    "n63": (1, [63], 63, (0.2, 0.5), (1.0, 2.5)),
    "n64": (1, [64], 64, (0.2, 0.51), (1.0, 2.5)),
    "n65": (1, [65], 65, (0.2, 0.5), (1.0, 2.5)),
    "n512": (206, [512], 512, (0.156, 0.567), (1.09, 2.5)),
}
_cache = {}


def scene(name):
    """(boxes (B,N,7) float32, counts (B,) int32, labels (B,N) int64, IoU thresholds, radii) of a fixed scene."""
    seed, counts, n_pad, thresholds, radii = SCENES[name]
    return cluster_scene(seed, counts, n_pad) + (thresholds, radii)


def scene_iou(name, mode="bev"):
    """Per-frame fp64 IoU matrices (count x count) of a fixed scene, computed once per process."""
    if (name, mode) not in _cache:
        boxes, counts = scene(name)[:2]
        _cache[name, mode] = [iou_matrix(boxes[b, :c], boxes[b, :c], mode) for b, c in enumerate(counts)]
    return _cache[name, mode]


def degenerate_set():
    """(N,7) float32: identical boxes, zero width / length, shared edges, yaw differences of exactly 0, pi/2, pi and of 1e-4, 1e-6
    (near-parallel edges), one box inside another, boxes 100 m from the origin."""
    f = np.float32
    base = [10.0, -4.0, -1.0, 1.9, 4.5, 1.6, 0.3]
    rows = [
        base, base,                                               # identical
        [10.0, -4.0, -1.0, 0.0, 4.5, 1.6, 0.3],                   # zero width
        [10.0, -4.0, -1.0, 1.9, 0.0, 1.6, 0.3],                   # zero length
        [0.0, 0.0, 0.0, 2.0, 4.0, 1.5, 0.0], [4.0, 0.0, 0.0, 2.0, 4.0, 1.5, 0.0],      # share the edge x = 2 (l along x at yaw 0)
        [0.0, 2.0, 0.0, 2.0, 4.0, 1.5, 0.0],                      # shares the edge y = 1 with the first of the pair
        [10.3, -4.2, -1.0, 1.9, 4.5, 1.6, 0.3],                   # yaw difference 0, shifted
        [10.0, -4.0, -1.0, 1.9, 4.5, 1.6, float(f(0.3) + f(math.pi / 2))],
        [10.0, -4.0, -1.0, 1.9, 4.5, 1.6, float(f(0.3) + f(math.pi))],
        [10.0, -4.0, -1.0, 1.9, 4.5, 1.6, 0.3 + 1e-4], [10.0, -4.0, -1.0, 1.9, 4.5, 1.6, 0.3 + 1e-6],
        [10.1, -4.0, -1.0, 1.9, 4.5, 1.6, 0.3 + 1e-4], [10.0, -3.9, -0.9, 2.0, 4.4, 1.6, 0.3 - 1e-6],
        [10.0, -4.0, -1.0, 0.8, 1.5, 0.8, 1.1],                   # inside `base`
        [10.0, -4.0, -1.0, 6.0, 14.0, 4.0, -0.4],                 # contains `base`
        [100.0, 100.0, 0.0, 1.9, 4.5, 1.6, 0.7], [100.4, 100.3, 0.2, 2.0, 4.6, 1.5, 0.75],
        [-100.0, 100.0, 0.0, 2.9, 12.0, 3.4, 2.0], [-100.0, 101.0, 0.5, 2.9, 12.0, 3.4, 2.0 + 1e-4],
        [10.0, -4.0, 5.0, 1.9, 4.5, 1.6, 0.3],                    # `base` moved up: no z-overlap
    ]
    return np.array(rows, np.float64).astype(np.float32)


def margin(boxes, count, thresholds, radii, iou=None):
    """(smallest |IoU - t| over pairs and thresholds, smallest | centre distance - r | over pairs and radii) of one frame."""
    b = np.asarray(boxes[:count], np.float64)
    if count < 2:
        return math.inf, math.inf
    m = iou if iou is not None else iou_matrix(b, b)
    iu = np.triu_indices(count, 1)
    v = m[iu]
    d = np.hypot(b[:, None, 0] - b[None, :, 0], b[:, None, 1] - b[None, :, 1])[iu]
    return (min(float(np.abs(v - t).min()) for t in thresholds) if thresholds else math.inf,
            min(float(np.abs(d - r).min()) for r in radii) if radii else math.inf)


# ---- synthetic head outputs with planted duplicate peaks ------------------------------------------------------------------------

PLANTED_SEED = 5
PLANTED_IOU_THRESH = 0.2
PLANTED_DUPS = ((0, 0, 0, 0.0), (2, 0, 0, 0.05), (0, 3, 0, 0.10), (1, 0, 1, 0.07), (-1, -1, 9, 0.12))   # (dx, dy, dclass, score drop)


def planted_heads(voxel, seed=PLANTED_SEED, B=2, C=10, H=128, W=128, n_obj=12):
    """Head outputs (float32 numpy, the decode's five maps) with n_obj objects per frame on a 24-cell lattice; every object has a
    main peak and duplicates two and three cells away in its own class plane and one cell away in neighbouring class planes
    (PLANTED_DUPS), all sharing the object's size and heading up to a small jitter.  Boxes are 7 x 9 cells, so every duplicate
    overlaps its main peak by IoU > 0.3 and objects never touch each other.  Returns (maps, peaks): peaks[b] = the planted
    (score, class, box[7], vel[2], object index, is_main) in descending score order, as the decode must report them."""
    rng = np.random.default_rng(seed)
    maps = {"heatmap": np.full((B, C, H, W), 0.01, np.float32), "offset": np.zeros((B, 2, H, W), np.float32),
            "size": np.ones((B, 3, H, W), np.float32), "rot": np.zeros((B, 2, H, W), np.float32),
            "vel": np.zeros((B, 2, H, W), np.float32)}
    maps["rot"][:, 1] = 1.0
    peaks = []
    for b in range(B):
        cells = rng.permutation(25)[:n_obj]
        rows = []
        for o, cell in enumerate(cells):
            ix, iy = 12 + 24 * (cell % 5), 12 + 24 * (cell // 5)
            cls, score, yaw = int(rng.integers(0, C)), float(rng.uniform(0.6, 0.95)), float(rng.uniform(-math.pi, math.pi))
            for dx, dy, dc, drop in PLANTED_DUPS:
                x, y, c = ix + dx, iy + dy, (cls + dc) % C
                s = np.float32(score - drop)
                off = rng.uniform(0.3, 0.7, 2).astype(np.float32)
                size = (np.array([7.0, 9.0, 1.0]) * voxel * rng.uniform(0.97, 1.03, 3)).astype(np.float32)
                yw = yaw + rng.normal(0, 0.03)
                rot = np.array([math.sin(yw), math.cos(yw)], np.float32)
                vel = rng.normal(0, 1, 2).astype(np.float32)
                maps["heatmap"][b, c, y, x] = s
                maps["offset"][b, :, y, x], maps["size"][b, :, y, x] = off, size
                maps["rot"][b, :, y, x], maps["vel"][b, :, y, x] = rot, vel
                box = [(x + float(off[0])) * voxel + PC_RANGE[0], (y + float(off[1])) * voxel + PC_RANGE[1], -1.0,
                       float(size[0]), float(size[1]), float(size[2]), math.atan2(float(rot[0]), float(rot[1]))]
                rows.append((float(s), c, box, [float(vel[0]), float(vel[1])], o, dx == 0 and dy == 0 and dc == 0))
        rows.sort(key=lambda r: -r[0])
        assert len({r[0] for r in rows}) == len(rows), "planted scores must be distinct"
        peaks.append(rows)
    return maps, peaks
