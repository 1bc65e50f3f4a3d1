"""numpy fp64 restatement of the CenterPoint second stage: the five-point gather and its transpose, the RoI targets,
the loss with its gradient, the refine step and the RoI head's MLP -- and the named scenes the host and GPU tests share.

tests/test_roi_head_host.py holds the scenes away from every decision boundary (IoU ties and thresholds, the heading fold, score
ties), so the GPU tests compare every element.
"""
import math

import numpy as np

from tests import box_iou_ref

# ---- gather ---------------------------------------------------------------------------------------------------------------------------

MAP_RANGE = (-7.0, -5.0, 7.0, 5.0)        # (x_min, y_min, x_max, y_max): 2 m cells on the 5 x 7 map of the gather tests
MAP_H, MAP_W = 5, 7


def roi_points(box):
    """The five sample points of a box (fp64 from the fp32 values): centre, front, back, left, right."""
    x, y, w, l, yaw = (float(box[i]) for i in (0, 1, 3, 4, 6))
    c, s = math.cos(yaw), math.sin(yaw)
    return [(x, y), (x + 0.5 * l * c, y + 0.5 * l * s), (x - 0.5 * l * c, y - 0.5 * l * s),
            (x + 0.5 * w * -s, y + 0.5 * w * c), (x - 0.5 * w * -s, y - 0.5 * w * c)]


def sample(px, py, H, W, rng):
    """A point -> None (zero row) or (i0, j0, [w0..w3] fp64) with the corner order (i0,j0), (i0,j0+1), (i0+1,j0), (i0+1,j0+1)."""
    vx, vy = (rng[2] - rng[0]) / W, (rng[3] - rng[1]) / H
    u, v = (px - rng[0]) / vx - 0.5, (py - rng[1]) / vy - 0.5
    if not (math.isfinite(u) and math.isfinite(v) and -1.0 < u < W and -1.0 < v < H):
        return None
    j0, i0 = math.floor(u), math.floor(v)
    fj, fi = u - j0, v - i0
    return i0, j0, [(1 - fi) * (1 - fj), (1 - fi) * fj, fi * (1 - fj), fi * fj]


def samples(boxes, count, H, W, rng):
    """[b][k][p] -> sample() of every RoI below the count (None elsewhere)."""
    B, K = boxes.shape[:2]
    out = []
    for b in range(B):
        n = min(max(int(count[b]), 0), K)
        out.append([[sample(px, py, H, W, rng) for px, py in roi_points(boxes[b, k])] if k < n else [None] * 5 for k in range(K)])
    return out


def gather(x, boxes, count, rng):
    """x (B,H,W,C) fp64 -> (feat (B,K,5C) fp64, mag = sum |w| |v| of every element)."""
    B, H, W, C = x.shape
    K = boxes.shape[1]
    feat, mag = np.zeros((B, K, 5 * C)), np.zeros((B, K, 5 * C))
    for b, frame in enumerate(samples(boxes, count, H, W, rng)):
        for k, pts in enumerate(frame):
            for p, s in enumerate(pts):
                if s is None:
                    continue
                i0, j0, w = s
                for q, (di, dj) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    i, j = i0 + di, j0 + dj
                    if 0 <= i < H and 0 <= j < W:
                        feat[b, k, p * C:(p + 1) * C] += w[q] * x[b, i, j]
                        mag[b, k, p * C:(p + 1) * C] += abs(w[q]) * np.abs(x[b, i, j])
    return feat, mag


def gather_bwd(dfeat, boxes, count, H, W, rng):
    """dfeat (B,K,5C) fp64 -> (dx (B,H,W,C), mag = sum |w dy|, n (B,H,W) = the contributions of every cell)."""
    B, K = boxes.shape[:2]
    C = dfeat.shape[2] // 5
    dx, mag, n = np.zeros((B, H, W, C)), np.zeros((B, H, W, C)), np.zeros((B, H, W), np.int64)
    for b, frame in enumerate(samples(boxes, count, H, W, rng)):
        for k, pts in enumerate(frame):
            for p, s in enumerate(pts):
                if s is None:
                    continue
                i0, j0, w = s
                for q, (di, dj) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    i, j = i0 + di, j0 + dj
                    if 0 <= i < H and 0 <= j < W and np.float32(w[q]) != 0:
                        dx[b, i, j] += w[q] * dfeat[b, k, p * C:(p + 1) * C]
                        mag[b, i, j] += np.abs(w[q] * dfeat[b, k, p * C:(p + 1) * C])
                        n[b, i, j] += 1
    return dx, mag, n


def gather_scene():
    """(boxes (2,6,7) fp32, count): frame 0 has count 0 (its rows are filler), frame 1 has five RoIs and one filler row:
    0 a face centre past the map edge, 1 entirely outside, 2 zero size on a cell centre (five equal points, weights 1 0 0 0),
    3 centre on the u = -0.5 border, 4 NaN yaw."""
    f = np.float32
    boxes = np.full((2, 6, 7), 3.0, f)
    boxes[0, :, :2] = [[1.0, 1.0]] * 6
    boxes[1] = [[5.0, 1.3, 0.0, 2.2, 10.0, 1.5, 0.3],
                [30.0, 30.0, 0.0, 1.0, 2.0, 1.5, 0.0],
                [-2.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.7],
                [-7.0, 0.6, 0.0, 1.0, 2.5, 1.5, 0.0],
                [1.1, -2.3, 0.0, 1.8, 4.0, 1.5, np.nan],
                [0.5, 0.5, 0.0, 2.0, 4.0, 1.5, 1.0]]
    return boxes, np.array([0, 5], np.int32)


def many_scene():
    """(boxes (2,70,7), count): frame 0 holds 70 identical RoIs -- one cell's candidates span two ballots of the backward --, frame 1
    three different ones."""
    f = np.float32
    boxes = np.zeros((2, 70, 7), f)
    boxes[0] = [0.7, -0.9, 0.0, 1.9, 4.3, 1.5, 0.4]
    boxes[1, :3] = [[-3.0, 2.0, 0.0, 2.0, 4.0, 1.5, -1.1], [4.4, -3.1, 0.0, 1.0, 3.0, 1.5, 2.0], [6.5, 4.2, 0.0, 2.0, 2.0, 1.0, 0.1]]
    return boxes, np.array([70, 3], np.int32)


# ---- targets --------------------------------------------------------------------------------------------------------------------------

REG_FG_THRESH = 0.55


def fold_heading(d):
    d = d - 2 * math.pi * math.floor((d + math.pi) / (2 * math.pi))
    if d > math.pi / 2:
        d -= math.pi
    elif d < -math.pi / 2:
        d += math.pi
    return d


def encode(roi, gt):
    r, g = [float(v) for v in roi], [float(v) for v in gt]
    c, s = math.cos(r[6]), math.sin(r[6])
    dx, dy = g[0] - r[0], g[1] - r[1]
    diag = math.sqrt(r[4] ** 2 + r[3] ** 2)
    return [(c * dx + s * dy) / diag, (c * dy - s * dx) / diag, (g[2] - r[2]) / r[5], math.log(g[3] / r[3]), math.log(g[4] / r[4]),
            math.log(g[5] / r[5]), fold_heading(g[6] - r[6])]


def decode(roi, t):
    r = [float(v) for v in roi]
    c, s = math.cos(r[6]), math.sin(r[6])
    diag = math.sqrt(r[4] ** 2 + r[3] ** 2)
    return [r[0] + (c * t[0] - s * t[1]) * diag, r[1] + (s * t[0] + c * t[1]) * diag, r[2] + t[2] * r[5], r[3] * math.exp(t[3]),
            r[4] * math.exp(t[4]), r[5] * math.exp(t[5]), r[6] + t[6]]


def candidate_ious(rois, count, roi_labels, gt, gt_labels, mode, match_labels):
    """[b][k] -> [(m, iou)] over the candidates of every RoI below the count, in index order."""
    f = box_iou_ref.iou_bev if mode == "bev" else box_iou_ref.iou_3d
    B, K = rois.shape[:2]
    out = []
    for b in range(B):
        n = min(max(int(count[b]), 0), K)
        out.append([[(m, f(rois[b, k].astype(np.float64), gt[b, m].astype(np.float64))) for m in range(gt.shape[1])
                     if gt_labels[b, m] >= 0 and (not match_labels or gt_labels[b, m] == roi_labels[b, k])] if k < n else None
                    for k in range(K)])
    return out


def targets(rois, count, roi_labels, gt, gt_labels, mode="3d", match_labels=False, reg_fg_thresh=REG_FG_THRESH):
    B, K = rois.shape[:2]
    out = dict(iou=np.zeros((B, K)), gt_index=np.full((B, K), -1, np.int64), cls_target=np.zeros((B, K)),
               reg_mask=np.zeros((B, K), np.uint8), reg_target=np.zeros((B, K, 7)))
    cands = candidate_ious(rois, count, roi_labels, gt, gt_labels, mode, match_labels)
    for b in range(B):
        for k in range(K):
            if not cands[b][k]:
                continue
            m, v = max(cands[b][k], key=lambda t: (t[1], -t[0]))
            out["iou"][b, k], out["gt_index"][b, k] = v, m
            out["cls_target"][b, k] = min(max(2 * v - 0.5, 0.0), 1.0)
            if v >= reg_fg_thresh and min(rois[b, k, 3:6].min(), gt[b, m, 3:6].min()) > 0:
                out["reg_mask"][b, k] = 1
                out["reg_target"][b, k] = encode(rois[b, k], gt[b, m])
    return out


def target_scene(name):
    """(rois (2,12,7) fp32, count, roi_labels int64 (2,12), gt (2,5,7) fp32, gt_labels int32 (2,5)) of 'mixed', 'empty', 'labels'.
    RoIs are jittered copies of the ground truth (IoU from ~0.2 to ~0.9, one with the opposite heading, one with a zero size), far
    misses, and filler past the count."""
    f = np.float32
    rng = np.random.default_rng(dict(mixed=11, empty=12, labels=13)[name])
    B, K, M = 2, 12, 5
    gt = np.zeros((B, M, 7), f)
    gt_labels = np.full((B, M), -1, np.int32)
    for b, n in enumerate((4, 3)):
        for m in range(n):
            gt[b, m] = [-30 + 15 * m + rng.uniform(-2, 2), -20 + 12 * m + rng.uniform(-2, 2), rng.uniform(-1, 1), rng.uniform(1.6, 2.4),
                        rng.uniform(3.8, 5.2), rng.uniform(1.4, 1.9), rng.uniform(-3, 3)]
            gt_labels[b, m] = m % 3
    if name == "empty":
        gt_labels[:] = -1
    count = np.array([10, 7], np.int32)
    rois = np.zeros((B, K, 7), f)
    roi_labels = np.zeros((B, K), np.int64)
    jitter = (0.03, 0.08, 0.15, 0.3, 0.5)
    for b in range(B):
        n = (4, 3)[b]
        for k in range(K):
            m = k % n
            j = jitter[(k // n + b) % len(jitter)]
            rois[b, k] = gt[b, m]
            rois[b, k, :2] += rng.uniform(-1, 1, 2) * j * 4
            rois[b, k, 2] += rng.uniform(-1, 1) * j
            rois[b, k, 3:6] *= np.exp(rng.uniform(-1, 1, 3) * j)
            rois[b, k, 6] += rng.uniform(-1, 1) * j
            roi_labels[b, k] = (m + (1 if k % 5 == 4 else 0)) % 3          # every fifth RoI carries its neighbour's label
        rois[b, 1, 6] += math.pi                                         # the opposite heading: the same box to the IoU and the fold
        rois[b, 2, 3] = 0.0                                              # a zero width: IoU 0, no regression
        rois[b, 3, :2] += 40.0                                           # a far miss
    return rois, count, roi_labels, gt, gt_labels


# ---- loss -----------------------------------------------------------------------------------------------------------------------------

def loss(pred, count, tgt, w_cls, w_reg):
    """pred (B,K,8) fp64 -> ((total, cls, reg), dpred)."""
    B, K = pred.shape[:2]
    valid = np.arange(K)[None, :] < np.clip(count, 0, K)[:, None]
    fg = valid & (tgt["reg_mask"] != 0)
    x, t = pred[..., 0], tgt["cls_target"]
    bce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
    nv, nf = valid.sum() + 1e-4, fg.sum() + 1e-4
    diff = pred[..., 1:] - tgt["reg_target"]
    lc, lr = (bce * valid).sum() / nv, (np.abs(diff) * fg[..., None]).sum() / nf
    d = np.zeros_like(pred)
    d[..., 0] = w_cls * (1 / (1 + np.exp(-x)) - t) * valid / nv
    d[..., 1:] = w_reg * np.sign(diff) * fg[..., None] / nf
    return (w_cls * lc + w_reg * lr, lc, lr), d


def loss_pred(name):
    """pred (2,12,8) fp32 for the target scene `name`: logits over +-4, residuals around the targets' scale."""
    rng = np.random.default_rng(dict(mixed=21, empty=22, labels=23)[name])
    return np.concatenate([rng.uniform(-4, 4, (2, 12, 1)), rng.normal(0, 0.3, (2, 12, 7))], -1).astype(np.float32)


# ---- refine ---------------------------------------------------------------------------------------------------------------------------

def refine(rois, scores, labels, vel, count, pred, thresh=0.0):
    B, K = rois.shape[:2]
    out = dict(boxes=np.zeros((B, K, 7)), scores=np.zeros((B, K)), labels=np.zeros((B, K), np.int64), velocities=np.zeros((B, K, 2)),
               count=np.zeros(B, np.int64), order=[])
    for b in range(B):
        n = min(max(int(count[b]), 0), K)
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.sqrt(scores[b, :n].astype(np.float64) / (1 + np.exp(-pred[b, :n, 0].astype(np.float64))))
        keep = [k for k in range(n) if math.isfinite(s[k]) and s[k] >= thresh]
        keep.sort(key=lambda k: (-s[k], k))
        out["order"].append(keep)
        out["count"][b] = len(keep)
        for r, k in enumerate(keep):
            out["boxes"][b, r] = decode(rois[b, k], pred[b, k, 1:].astype(np.float64))
            out["scores"][b, r], out["labels"][b, r], out["velocities"][b, r] = s[k], labels[b, k], vel[b, k]
    return out


def refine_scene(name):
    """(rois (2,9,7), scores, labels, velocities, count, pred (2,9,8)) of 'plain', 'tie' (rows 1, 4 and 6 of frame 0 share score and
    logit bit for bit) and 'drops' (a NaN logit, an infinite first-stage score, a negative one, scores under the 0.3 threshold)."""
    f = np.float32
    rng = np.random.default_rng(dict(plain=31, tie=32, drops=33)[name])
    B, K = 2, 9
    rois = np.zeros((B, K, 7), f)
    rois[..., :2] = rng.uniform(-40, 40, (B, K, 2))
    rois[..., 2] = rng.uniform(-1, 1, (B, K))
    rois[..., 3:6] = rng.uniform(0.8, 5, (B, K, 3))
    rois[..., 6] = rng.uniform(-3, 3, (B, K))
    scores = rng.uniform(0.05, 0.95, (B, K)).astype(f)
    labels = rng.integers(0, 10, (B, K)).astype(np.int64)
    vel = rng.normal(0, 2, (B, K, 2)).astype(f)
    pred = np.concatenate([rng.uniform(-3, 3, (B, K, 1)), rng.normal(0, 0.2, (B, K, 7))], -1).astype(f)
    count = np.array([8, 5], np.int32)
    if name == "tie":
        for k in (4, 6):
            scores[0, k], pred[0, k, 0] = scores[0, 1], pred[0, 1, 0]
    if name == "drops":
        pred[0, 0, 0] = np.nan
        scores[0, 2] = np.inf
        scores[0, 3] = -0.2
        scores[1, 1], pred[1, 1, 0] = 0.05, -3.0
    return rois, scores, labels, vel, count, pred


# ---- the head's MLP -------------------------------------------------------------------------------------------------------------------

def mlp_eval(feat, sd, eps=1e-5):
    """feat (R, 5C) fp64, sd = the head's state dict as fp64 numpy -> pred (R, 8) with BatchNorm on its running statistics."""
    a = feat
    for lin, bn in ((0, 1), (3, 4)):
        y = a @ sd[f"shared_fc.{lin}.weight"].T
        y = (y - sd[f"shared_fc.{bn}.running_mean"]) / np.sqrt(sd[f"shared_fc.{bn}.running_var"] + eps)
        a = np.maximum(y * sd[f"shared_fc.{bn}.weight"] + sd[f"shared_fc.{bn}.bias"], 0)
    return np.concatenate([a @ sd["cls_out.weight"].T + sd["cls_out.bias"], a @ sd["reg_out.weight"].T + sd["reg_out.bias"]], -1)
