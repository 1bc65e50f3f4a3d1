"""numpy restatement of points-in-boxes and the GT-paste augmentation (csrc/gt_paste.hip), and the scenes of
tests/test_gt_paste_host.py / tests/test_gpu_gt_paste.py.  Geometry (containment, collision) is decided in fp64; the values the device
copies or adds (kept points, bank row + centre) are fp32, so the outputs are compared bit for bit.  Every scene is generated from a fixed
seed for which the margins hold -- no point within MARGIN of a box face it is tested against, every box pair with a separating-axis
slack of at least MARGIN either way -- which the host test asserts, so the GPU tests exclude nothing."""
import math

import numpy as np

MARGIN = 1e-3


# ---- geometry, fp64 ------------------------------------------------------------------------------------------------------------------

def box_valid3d(box) -> bool:
    b = np.asarray(box, dtype=np.float64)
    return bool(np.isfinite(b[:7]).all() and b[3] > 0 and b[4] > 0 and b[5] > 0)


def face_gap(points, box) -> np.ndarray:
    """g [n] = max(|lx| - l/2, |ly| - w/2, |dz| - h/2) in fp64: the point is inside iff g <= 0, and |g| is how far the nearest
    comparison is from flipping."""
    p = np.asarray(points, dtype=np.float64)[:, :3]
    b = np.asarray(box, dtype=np.float64)
    d = p - b[:3]
    c, s = math.cos(b[6]), math.sin(b[6])
    lx = d[:, 0] * c + d[:, 1] * s
    ly = -d[:, 0] * s + d[:, 1] * c
    return np.maximum(np.maximum(np.abs(lx) - b[4] / 2, np.abs(ly) - b[3] / 2), np.abs(d[:, 2]) - b[5] / 2)


def points_in_boxes_ref(points, count, boxes, mask=None):
    """One frame: (idx int32 [N] = lowest containing box or -1, the smallest |g| over the (point < count, live valid box) pairs)."""
    N = points.shape[0]
    idx = np.full(N, -1, dtype=np.int32)
    worst = np.inf
    n = N if count is None else int(count)
    for j in range(boxes.shape[0] - 1, -1, -1):
        if (mask is not None and not mask[j] >= 0) or not box_valid3d(boxes[j]):
            continue
        g = face_gap(points[:n], boxes[j])
        g = np.where(np.isnan(g), np.inf, g)                       # a NaN point is in nothing
        if n:
            worst = min(worst, float(np.abs(g).min()))
        idx[:n][g <= 0] = j
    return idx, worst


def rect_valid(box) -> bool:
    b = np.asarray(box, dtype=np.float64)
    return bool(np.isfinite(b[[0, 1, 3, 4, 6]]).all() and b[3] > 0 and b[4] > 0)


def sat_slack(a, b) -> float:
    """The largest separation over the four edge directions, fp64: > 0 = apart by that much, <= 0 = colliding (touching counts)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = b[:2] - a[:2]
    best = -np.inf
    ua = np.array([math.cos(a[6]), math.sin(a[6])])
    ub = np.array([math.cos(b[6]), math.sin(b[6])])
    for n in (ua, np.array([-ua[1], ua[0]]), ub, np.array([-ub[1], ub[0]])):
        ra = a[4] / 2 * abs(ua @ n) + a[3] / 2 * abs(np.array([-ua[1], ua[0]]) @ n)
        rb = b[4] / 2 * abs(ub @ n) + b[3] / 2 * abs(np.array([-ub[1], ub[0]]) @ n)
        best = max(best, abs(d @ n) - ra - rb)
    return float(best)


def collide(a, b) -> bool:
    return rect_valid(a) and rect_valid(b) and sat_slack(a, b) <= 0


def accept_ref(gt_boxes, gt_labels, bank_boxes, cand) -> np.ndarray:
    """One frame's greedy accept rule: int32 [Kc]."""
    acc = np.zeros(len(cand), dtype=np.int32)
    for k, c in enumerate(cand):
        if c < 0:
            continue
        if any(gt_labels[j] >= 0 and collide(bank_boxes[c], gt_boxes[j]) for j in range(len(gt_boxes))):
            continue
        if any(acc[q] and collide(bank_boxes[cand[q]], bank_boxes[c]) for q in range(k)):
            continue
        acc[k] = 1
    return acc


def paste_ref(lidar, counts, gt_boxes, gt_labels, gt_vel, bank, cand, capacity=None):
    """bank = dict(points fp32 [P][C], obj_ptr [K + 1], boxes fp32 [K][7|9], labels [K]).  Returns the dict `gt_paste.paste` returns,
    as numpy arrays."""
    B, N, C = lidar.shape
    M, ncol = gt_boxes.shape[1], gt_boxes.shape[2]
    Kc = cand.shape[1]
    ptr, bb = bank["obj_ptr"], bank["boxes"]
    sizes = np.diff(ptr)
    if capacity is None:
        capacity = N + max(int(sum(sizes[c] for c in cand[b] if c >= 0)) for b in range(B))
    out = dict(lidar_points=np.zeros((B, capacity, C), dtype=np.float32), lidar_count=np.zeros(B, dtype=np.int32),
               gt_boxes=np.zeros((B, M + Kc, ncol), dtype=np.float32), gt_labels=np.full((B, M + Kc), -1, dtype=np.int64),
               gt_velocities=None if gt_vel is None else np.zeros((B, M + Kc, 2), dtype=np.float32),
               accepted=np.zeros((B, Kc), dtype=np.int32))
    for b in range(B):
        acc = accept_ref(gt_boxes[b], gt_labels[b], bb, cand[b])
        out["accepted"][b] = acc
        n = N if counts is None else int(counts[b])
        keep = np.ones(n, dtype=bool)
        rows = []
        for k in range(Kc):
            if not acc[k]:
                continue
            c = cand[b, k]
            if box_valid3d(bb[c]) and n:
                keep &= ~(face_gap(lidar[b, :n], bb[c]) <= 0)
            obj = bank["points"][ptr[c]:ptr[c + 1]].copy()
            obj[:, :3] = obj[:, :3] + bb[c, :3].astype(np.float32)            # one fp32 addition per coordinate
            rows.append(obj)
            out["gt_boxes"][b, M + k, :min(ncol, bb.shape[1])] = bb[c, :ncol]
            out["gt_labels"][b, M + k] = bank["labels"][c]
            if gt_vel is not None and bb.shape[1] == 9:
                out["gt_velocities"][b, M + k] = bb[c, 7:9]
        stream = np.concatenate([lidar[b, :n][keep]] + rows) if rows else lidar[b, :n][keep]
        m = min(len(stream), capacity)
        out["lidar_points"][b, :m] = stream[:m]
        out["lidar_count"][b] = m
        out["gt_boxes"][b, :M] = gt_boxes[b]
        out["gt_labels"][b, :M] = gt_labels[b]
        if gt_vel is not None:
            out["gt_velocities"][b, :M] = gt_vel[b]
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------------------------

def _inside_points(rs, box, n, C, fill=0.9):
    """n points inside `box` (within `fill` of its half extents), fp32 [n][C]; channels past xyz uniform."""
    u = rs.uniform(-fill, fill, (n, 3)) * np.array([box[4], box[3], box[5]]) / 2
    c, s = math.cos(box[6]), math.sin(box[6])
    p = np.empty((n, C))
    p[:, 0] = box[0] + u[:, 0] * c - u[:, 1] * s
    p[:, 1] = box[1] + u[:, 0] * s + u[:, 1] * c
    p[:, 2] = box[2] + u[:, 2]
    p[:, 3:] = rs.uniform(0, 1, (n, C - 3))
    return p.astype(np.float32)


PIB_SEED = {4: 0, 5: 0}
PIB_B, PIB_N, PIB_M = 3, 700, 70
PIB_COUNTS = np.array([700, 513, 0], dtype=np.int32)
PIB_YAWS = (0.0, math.pi / 2, -math.pi / 2, math.pi)


def pib_scene(C):
    """points fp32 [3][700][C], counts, boxes fp32 [3][70][7 (C = 4) or 9 (C = 5)], mask int64 [3][70] (labels, -1 = ignored).
    Per frame: boxes 0-3 with yaw 0, +-pi/2, pi, the rest generic; box 5 has w = 0, box 6 a NaN centre, box 7 a NaN yaw; box 9 is
    box 8 moved by a little and box 65 overlaps box 20 (the lowest index wins); rows 12, 30 and 66 are masked; point 0 sits exactly on
    box 10's centre; two points in three come from inside a box (the degenerate and the masked ones included), the rest are spread."""
    rs = np.random.RandomState(1000 * C + PIB_SEED[C])
    ncol = 7 if C == 4 else 9
    boxes = np.zeros((PIB_B, PIB_M, ncol))
    boxes[..., 0:2] = rs.uniform(-24, 24, (PIB_B, PIB_M, 2))
    boxes[..., 2] = rs.uniform(-2, 1, (PIB_B, PIB_M))
    boxes[..., 3:6] = rs.uniform(0.8, 5.0, (PIB_B, PIB_M, 3))
    boxes[..., 6] = rs.uniform(-math.pi, math.pi, (PIB_B, PIB_M))
    boxes[:, :4, 6] = PIB_YAWS
    boxes[..., 7:] = rs.normal(0, 2, (PIB_B, PIB_M, ncol - 7))
    boxes[:, 9] = boxes[:, 8]
    boxes[:, 9, 0] += 0.4
    boxes[:, 9, 6] += 0.3
    boxes[:, 65, :3] = boxes[:, 20, :3] + 0.25
    mask = rs.randint(0, 10, (PIB_B, PIB_M)).astype(np.int64)
    mask[:, [12, 30, 66]] = -1
    pts = np.zeros((PIB_B, PIB_N, C), dtype=np.float32)
    for b in range(PIB_B):
        for i in range(PIB_N):
            if i % 3 == 2:
                pts[b, i] = np.concatenate([rs.uniform(-26, 26, 2), rs.uniform(-3, 2, 1), rs.uniform(0, 1, C - 3)])
            else:
                pts[b, i] = _inside_points(rs, boxes[b, rs.randint(PIB_M)], 1, C)[0]
    boxes = boxes.astype(np.float32)
    boxes[:, 5, 3] = 0.0
    boxes[:, 6, 0] = np.nan
    boxes[:, 7, 6] = np.nan
    pts[:, 0, :3] = boxes[:, 10, :3]
    return pts, PIB_COUNTS.copy(), boxes, mask


# The paste scene.  Bank objects by row: box (x, y, z, w, l, h, yaw, vx, vy), label, points.
PASTE_SEED = 39
PASTE_B, PASTE_N, PASTE_M, PASTE_KC, PASTE_C = 3, 1500, 12, 10, 5
_BANK = [
    ((0.0, 0.0, -1.0, 2.0, 4.0, 1.6, 0.0, 1.0, 0.5), 5, 64),        # 0: free
    ((3.0, 0.3, -1.0, 2.0, 4.0, 1.6, 0.0, 0.0, 0.0), 6, 5),         # 1: overlaps 0
    ((6.0, 0.0, -1.0, 2.0, 4.0, 1.6, 0.0, -1.0, 0.0), 7, 300),      # 2: overlaps 1 only
    ((-20.0, 14.0, -0.5, 1.8, 4.5, 1.5, 0.7, 2.0, 2.0), 5, 5),      # 3: on GT row 0 of frame 0
    ((18.0, -16.0, -0.8, 2.2, 5.0, 2.0, -1.2, 0.0, 1.0), 8, 64),    # 4: on GT row 5 of frame 0
    ((-12.0, -22.0, -1.2, 0.8, 0.9, 1.7, 2.5, 0.3, 0.0), 9, 1),     # 5: on frame 0's padding row 3 only
    ((25.0, 20.0, 0.0, 2.5, 6.0, 2.5, 0.4, 0.0, 0.0), 6, 300),      # 6: free
    ((-30.0, -5.0, -1.0, 0.7, 0.7, 1.8, 1.1, 0.1, 0.2), 9, 1),      # 7: free
    ((10.0, 30.0, -1.0, 1.9, 4.2, 1.5, -2.6, 3.0, -1.0), 5, 64),    # 8: free
    ((-30.0, 33.5, -1.0, 2.0, 4.0, 1.5, 1.5707964, 0.0, 0.0), 7, 5),  # 9: free
]
PASTE_CAND = np.array([[0, -1, 3, 4, 1, 2, 5, 6, 7, 8],              # accepted: 0, 2 (1 is rejected by 0 and blocks nothing), 5, 6, 7, 8
                       [3, -1, 4, 0, 6, 8, -1, 7, 9, 2],              # frame 1: GT sits on every one of them
                       [9, 8, 1, 0, -1, 6, 7, 2, 5, 4]], dtype=np.int32)   # frame 2: no points in the sweep; 1 rejects 0 and 2
PASTE_EXPECT = np.array([[1, 0, 0, 0, 0, 1, 1, 1, 1, 1], [0] * 10, [1, 1, 1, 0, 0, 1, 1, 0, 1, 1]], dtype=np.int32)
PASTE_COUNTS = np.array([1500, 1321, 0], dtype=np.int32)
PASTE_PAD_ROWS = (3, 7, 10)


def paste_bank(bank_ncol=9, C=PASTE_C):
    rs = np.random.RandomState(77)
    boxes = np.array([b for b, _, _ in _BANK], dtype=np.float32)
    pts, ptr = [], [0]
    for (box, _, n) in _BANK:
        world = _inside_points(rs, np.array(box, dtype=np.float64), n, C, 0.95)
        world[:, :3] -= np.array(box[:3], dtype=np.float32)
        pts.append(world)
        ptr.append(ptr[-1] + n)
    return dict(points=np.concatenate(pts).astype(np.float32), obj_ptr=np.array(ptr, dtype=np.int32), boxes=boxes[:, :bank_ncol].copy(),
                labels=np.array([l for _, l, _ in _BANK], dtype=np.int64))


def paste_scene(ncol=9, bank_ncol=9):
    """lidar fp32 [3][1500][5], counts, gt_boxes fp32 [3][12][ncol], gt_labels int64 [3][12] (rows 3, 7, 10 are -1 with real boxes
    in them), gt_vel fp32 [3][12][2], the bank, cand [3][10]."""
    rs = np.random.RandomState(PASTE_SEED)
    bank = paste_bank(bank_ncol)
    bb = np.array([b for b, _, _ in _BANK])
    gt = np.zeros((PASTE_B, PASTE_M, 9))
    gt[..., 0] = rs.uniform(-45, -38, (PASTE_B, PASTE_M))           # parked at the left edge, one per 7 m lane, away from the bank
    gt[..., 1] = np.arange(PASTE_M) * 7.0 - 40.0
    gt[..., 2] = rs.uniform(-1.5, 0, (PASTE_B, PASTE_M))
    gt[..., 3:6] = rs.uniform(1.0, 4.0, (PASTE_B, PASTE_M, 3))
    gt[..., 6] = rs.uniform(-math.pi, math.pi, (PASTE_B, PASTE_M))
    gt[..., 7:] = rs.normal(0, 2, (PASTE_B, PASTE_M, 2))
    labels = rs.randint(0, 5, (PASTE_B, PASTE_M)).astype(np.int64)
    labels[:, list(PASTE_PAD_ROWS)] = -1

    def near(box, dx, dy, dyaw):
        g = box.copy()
        g[0] += dx
        g[1] += dy
        g[6] += dyaw
        return g
    gt[0, 0], gt[0, 5], gt[0, 3] = near(bb[3], 0.5, -0.3, 0.4), near(bb[4], -1.0, 0.5, -0.2), near(bb[5], 0.1, 0.1, 1.0)
    for j, o in enumerate((3, 4, 0, 6, 8, 7, 9, 2)):                 # frame 1: a live GT row on each candidate
        row = [0, 1, 2, 4, 5, 6, 8, 9][j]
        gt[1, row] = near(bb[o], 0.2, -0.2, 0.3)
    lidar = np.zeros((PASTE_B, PASTE_N, PASTE_C), dtype=np.float32)
    for b in range(PASTE_B):
        for i in range(PASTE_N):
            if i % 2:
                lidar[b, i] = np.concatenate([rs.uniform(-50, 50, 2), rs.uniform(-4, 2, 1), rs.uniform(0, 1, PASTE_C - 3)])
            else:
                lidar[b, i] = _inside_points(rs, bb[rs.randint(len(bb))], 1, PASTE_C, 1.3)[0]      # in and around the bank's boxes
    vel = gt[..., 7:9].astype(np.float32)
    return lidar, PASTE_COUNTS.copy(), gt[..., :ncol].astype(np.float32), labels, vel, bank, PASTE_CAND.copy()


def paste_margins(ncol=9, bank_ncol=9):
    """(smallest |g| of a sweep point against a candidate's box, smallest |slack| over candidate / GT and candidate / candidate pairs)."""
    lidar, counts, gt, labels, _, bank, cand = paste_scene(ncol, bank_ncol)
    g_min, s_min = np.inf, np.inf
    for b in range(PASTE_B):
        cs = [c for c in cand[b] if c >= 0]
        for c in cs:
            if counts[b]:
                g_min = min(g_min, float(np.abs(face_gap(lidar[b, :counts[b]], bank["boxes"][c])).min()))
            for j in range(PASTE_M):
                s_min = min(s_min, abs(sat_slack(bank["boxes"][c], gt[b, j])))
            for c2 in cs:
                if c2 != c:
                    s_min = min(s_min, abs(sat_slack(bank["boxes"][c], bank["boxes"][c2])))
    return g_min, s_min


# The scene of ObjectBank.from_frames: every coordinate of a centre is at least as large as the box's reach along it, so that
# |p - c| <= |p| per coordinate and (p - c) + c returns to within one ulp of p.
FRAMES_SEED = 0
FRAMES_B, FRAMES_N, FRAMES_M, FRAMES_C = 2, 600, 6, 4
FRAMES_COUNTS = np.array([600, 540], dtype=np.int32)
FRAMES_MIN_POINTS = 5


def frames_scene():
    """lidar fp32 [2][600][4], counts, gt_boxes fp32 [2][6][7], labels int64 [2][6] (row 4 is -1; row 2 holds 3 points, fewer than
    min_points)."""
    rs = np.random.RandomState(500 + FRAMES_SEED)
    gt = np.zeros((FRAMES_B, FRAMES_M, 7))
    for b in range(FRAMES_B):
        for j in range(FRAMES_M):
            ang = 2 * math.pi * (j + 0.5 * b) / FRAMES_M + 0.3
            gt[b, j, :3] = (22 * math.cos(ang), 22 * math.sin(ang), -3.0 + 0.1 * j)
            gt[b, j, 0] += math.copysign(6.0, gt[b, j, 0])
            gt[b, j, 1] += math.copysign(6.0, gt[b, j, 1])
            gt[b, j, 3:6] = rs.uniform(1.0, 3.5, 3)
            gt[b, j, 5] = rs.uniform(1.0, 2.0)
            gt[b, j, 6] = rs.uniform(-math.pi, math.pi)
    gt = gt.astype(np.float32)
    labels = rs.randint(0, 10, (FRAMES_B, FRAMES_M)).astype(np.int64)
    labels[:, 4] = -1
    lidar = np.zeros((FRAMES_B, FRAMES_N, FRAMES_C), dtype=np.float32)
    for b in range(FRAMES_B):
        for i in range(FRAMES_N):
            j = i % 8
            if i < 3:
                lidar[b, i] = _inside_points(rs, gt[b, 2].astype(np.float64), 1, FRAMES_C)[0]
            elif j < FRAMES_M and j != 2:
                lidar[b, i] = _inside_points(rs, gt[b, j].astype(np.float64), 1, FRAMES_C)[0]
            else:
                lidar[b, i] = np.concatenate([rs.uniform(-40, 40, 2), rs.uniform(-5, -1, 1), rs.uniform(0, 1, FRAMES_C - 3)])
    return lidar, FRAMES_COUNTS.copy(), gt, labels


def crop_ref(lidar, counts, gt, labels, min_points):
    """The objects `ObjectBank.from_frames` must hold, in (frame, row) order: [(frame, row, world points fp32 [n][C])], and the
    smallest |g|."""
    objs, worst = [], np.inf
    for b in range(lidar.shape[0]):
        idx, w = points_in_boxes_ref(lidar[b], counts[b], gt[b], labels[b])
        worst = min(worst, w)
        for j in range(gt.shape[1]):
            sel = idx == j
            if sel.sum() >= min_points:
                objs.append((b, j, lidar[b][sel]))
    return objs, worst
