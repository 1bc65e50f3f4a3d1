"""TEST INFRASTRUCTURE -- numpy fp64 restatement of the IoU-aware head's training and decode side, and the
fixed scenes its tests share.

Box assembly, the IoU target (through tests/box_iou_ref.iou_bev), the L1 IoU loss and the aligned DIoU loss with their analytic
gradients, and the rectified scores with the order they give (tests/centernet_ref's keep and top-K rules).  No import of the
package.  Scene arrays are float32 (what the device receives); everything here widens those same values to fp64.

Kinks.  The losses are piecewise smooth.  `kink_margin` gives the distance of a scene from the nearest point where a piece
changes: |iou_pred - t|, |size - 1e-3| at each size clamp, and every pair of rectangle edges whose order decides a min / max of the
DIoU (per axis: the two pairs of like edges, and the two pairs of opposite edges that decide whether the overlap is clamped at 0).  One kind of tie is exact and stays in the scenes on purpose: a
prediction bitwise equal to its ground truth (t = 1) has e = 0 and L/2 = l_g/2 without any rounding, in fp32 as in fp64, so all four
edge pairs tie in both.  There the convention is part of the definition: a min / max takes the GT rectangle's edge on a tie (the
comparisons that select the predicted edge are strict).  That is a subgradient of the loss at its minimum -- zero for the centre,
the one-sided derivative towards larger sizes for l and w -- and both sides compute it from identical operands, so such objects
are compared like every other.  `kink_margin` leaves those exact ties out and returns their number beside the margin.
"""
import math

import numpy as np

from tests import box_iou_ref
from tests import centernet_ref

SIZE_MIN = 1e-3
LOSS_RANGE = (-12.0, -10.0, -5.0, 12.0, 10.0, 3.0)          # 8 x 12 cells of 2.0 m x 2.5 m


def _f64(d, keys):
    return {k: np.asarray(d[k], np.float64) for k in keys}


def cell_size(pc_range, H, W):
    """(vx, vy) as the float32 values the kernels compute: (x_max - x_min) / W in fp32."""
    r = np.asarray(pc_range, np.float32)
    return float((r[3] - r[0]) / np.float32(W)), float((r[4] - r[1]) / np.float32(H))


def objects(pred, tgt):
    """[(b, k, cell)] of the objects with reg_mask set, in (b, k) order."""
    rm, ind = np.asarray(tgt["reg_mask"]), np.asarray(tgt["ind"])
    return [(b, k, int(ind[b, k])) for b in range(rm.shape[0]) for k in range(rm.shape[1]) if rm[b, k]]


def boxes_of(pred, tgt, pc_range):
    """{(b, k): (pred box, gt box)} as 7-vectors [x, y, 0, w, l, 0, yaw] in fp64: the decode's assembly on the targets' cell size."""
    p, t = _f64(pred, ("offset", "size", "rot")), _f64(tgt, ("target_offset", "target_size", "target_rot"))
    B, _, H, W = p["offset"].shape
    vx, vy = cell_size(pc_range, H, W)
    x0, y0 = float(np.float32(pc_range[0])), float(np.float32(pc_range[1]))
    out = {}
    for b, k, cell in objects(pred, tgt):
        cy, cx = divmod(cell, W)
        pb = [(cx + p["offset"][b, 0, cy, cx]) * vx + x0, (cy + p["offset"][b, 1, cy, cx]) * vy + y0, 0.0, p["size"][b, 0, cy, cx],
              p["size"][b, 1, cy, cx], 0.0, math.atan2(p["rot"][b, 0, cy, cx], p["rot"][b, 1, cy, cx])]
        gb = [(cx + t["target_offset"][b, k, 0]) * vx + x0, (cy + t["target_offset"][b, k, 1]) * vy + y0, 0.0,
              t["target_size"][b, k, 0], t["target_size"][b, k, 1], 0.0, math.atan2(t["target_rot"][b, k, 0], t["target_rot"][b, k, 1])]
        out[(b, k)] = (np.array(pb), np.array(gb))
    return out


def iou_targets(pred, tgt, pc_range):
    """(B, K) fp64: 2 * IoU_bev(pred, gt) - 1 where reg_mask is set, 0 elsewhere."""
    out = np.zeros(np.asarray(tgt["reg_mask"]).shape, np.float64)
    for (b, k), (pb, gb) in boxes_of(pred, tgt, pc_range).items():
        out[b, k] = 2.0 * box_iou_ref.iou_bev(pb, gb) - 1.0
    return out


def diou_obj(dx, dy, wp, lp, wg, lg, s, c, grad=False):
    """1 - d of one object from the centre difference (dx, dy) = pred - gt in metres, the raw predicted sizes, the GT sizes and the
    GT heading (s, c) = target_rot.  With grad: also d(1 - d) / d(dx, dy, wp, lp) and the list of comparison margins."""
    ex, ey = c * dx + s * dy, -s * dx + c * dy
    L, Wd = max(lp, SIZE_MIN), max(wp, SIZE_MIN)
    hl, hw = 0.5 * lg, 0.5 * wg
    xh, xl, yh, yl = ex + 0.5 * L, ex - 0.5 * L, ey + 0.5 * Wd, ey - 0.5 * Wd
    ovx, ovy = min(xh, hl) - max(xl, -hl), min(yh, hw) - max(yl, -hw)
    hit = ovx > 0 and ovy > 0
    inter = ovx * ovy if hit else 0.0
    U = L * Wd + lg * wg - inter + 1e-6
    cxl, cyl = max(xh, hl) - min(xl, -hl), max(yh, hw) - min(yl, -hw)
    C2 = cxl * cxl + cyl * cyl + 1e-6
    rho2 = ex * ex + ey * ey
    val = 1.0 - (inter / U - rho2 / C2)
    if not grad:
        return val
    ihx, ilx, ihy, ily = float(xh < hl), float(xl > -hl), float(yh < hw), float(yl > -hw)     # 1: the predicted edge is taken
    di = dict(ex=(ihx - ilx) * ovy, ey=(ihy - ily) * ovx, L=0.5 * (ihx + ilx) * ovy, W=0.5 * (ihy + ily) * ovx) if hit else \
        dict(ex=0.0, ey=0.0, L=0.0, W=0.0)
    dU = dict(ex=-di["ex"], ey=-di["ey"], L=Wd - di["L"], W=L - di["W"])
    dC = dict(ex=2 * cxl * ((1 - ihx) - (1 - ilx)), ey=2 * cyl * ((1 - ihy) - (1 - ily)), L=cxl * ((1 - ihx) + (1 - ilx)),
              W=cyl * ((1 - ihy) + (1 - ily)))
    dr = dict(ex=2 * ex, ey=2 * ey, L=0.0, W=0.0)
    g = {q: -((di[q] * U - inter * dU[q]) / U ** 2 - (dr[q] * C2 - rho2 * dC[q]) / C2 ** 2) for q in ("ex", "ey", "L", "W")}
    grads = (c * g["ex"] - s * g["ey"], s * g["ex"] + c * g["ey"], g["W"] if wp > SIZE_MIN else 0.0, g["L"] if lp > SIZE_MIN else 0.0)
    # like edges decide the min / max of the overlap and the enclosing rectangle, opposite edges whether an overlap is clamped at 0
    margins = dict(edges=[abs(xh - hl), abs(xl + hl), abs(yh - hw), abs(yl + hw)],
                   overlaps=[abs(xh + hl), abs(xl - hl), abs(yh + hw), abs(yl - hw)], clamps=[abs(wp - SIZE_MIN), abs(lp - SIZE_MIN)])
    return val, grads, margins


def _per_object(pred, tgt, pc_range, t_fixed=None):
    """[(b, k, cy, cx, t, iou_pred, diou value, (g_ox, g_oy, g_w, g_l), margins, tied)] in (b, k) order; t_fixed: IoU targets to use
    instead of this prediction's (t is a constant of the loss)."""
    p, t = _f64(pred, ("iou", "offset", "size", "rot")), _f64(tgt, ("target_offset", "target_size", "target_rot"))
    _, _, H, W = p["offset"].shape
    vx, vy = cell_size(pc_range, H, W)
    tt = iou_targets(pred, tgt, pc_range) if t_fixed is None else t_fixed
    out = []
    for b, k, cell in objects(pred, tgt):
        cy, cx = divmod(cell, W)
        ox, oy, wp, lp = p["offset"][b, 0, cy, cx], p["offset"][b, 1, cy, cx], p["size"][b, 0, cy, cx], p["size"][b, 1, cy, cx]
        gox, goy = t["target_offset"][b, k]
        wg, lg = t["target_size"][b, k, :2]
        s, c = t["target_rot"][b, k]
        val, (gdx, gdy, gw, gl), margins = diou_obj((ox - gox) * vx, (oy - goy) * vy, wp, lp, wg, lg, s, c, grad=True)
        tied = ox == gox and oy == goy and wp == wg and lp == lg
        out.append((b, k, cy, cx, tt[b, k], p["iou"][b, 0, cy, cx], val, (gdx * vx, gdy * vy, gw, gl), margins, tied))
    return out


def losses(pred, tgt, pc_range, w_iou=1.0, w_diou=1.0, t_fixed=None):
    """fp64 {'total_loss', 'iou_loss', 'diou_loss'} and the analytic gradients of total_loss as {'iou', 'offset', 'size'} maps.
    t_fixed: the IoU targets held constant (for difference quotients: no gradient flows through t)."""
    denom = float(np.asarray(tgt["reg_mask"]).astype(bool).sum()) + 1e-4
    g = {k: np.zeros(np.asarray(pred[k]).shape, np.float64) for k in ("iou", "offset", "size")}
    li = ld = 0.0
    for b, k, cy, cx, t, ip, val, (gox, goy, gw, gl), _, _ in _per_object(pred, tgt, pc_range, t_fixed):
        li += abs(ip - t)
        ld += val
        g["iou"][b, 0, cy, cx] += w_iou * np.sign(ip - t) / denom
        g["offset"][b, 0, cy, cx] += w_diou * gox / denom
        g["offset"][b, 1, cy, cx] += w_diou * goy / denom
        g["size"][b, 0, cy, cx] += w_diou * gw / denom
        g["size"][b, 1, cy, cx] += w_diou * gl / denom
    li, ld = li / denom, ld / denom
    return dict(total_loss=w_iou * li + w_diou * ld, iou_loss=li, diou_loss=ld), g


def kink_margin(pred, tgt, pc_range=LOSS_RANGE):
    """(margin, exact_ties): the smallest distance of the scene from a non-differentiable point (module docstring), over every
    object with reg_mask set; the edge pairs of an object bitwise equal to its ground truth are exact ties, counted apart."""
    margin, ties = math.inf, 0
    for *_, t, ip, _, _, m, tied in _per_object(pred, tgt, pc_range):
        margin = min([margin, abs(ip - t)] + m["clamps"] + m["overlaps"])
        if tied:
            assert m["edges"] == [0.0] * 4
            ties += 1
        else:
            margin = min([margin] + m["edges"])
    return margin, ties


# ---- the loss scenes (committed as seeds) -----------------------------------------------------------------------------------------

LOSS_B, LOSS_C, LOSS_H, LOSS_W, LOSS_K = 2, 10, 8, 12, 8
LOSS_SEEDS = {"mixed": 101, "empty": 102}
_PI_ROT = {+1: (0.0, -1.0), -1: (-0.0, -1.0)}                # atan2(+0, -1) = pi, atan2(-0, -1) = -pi


def loss_scene(name):
    """(pred, tgt) of float32 / int arrays.  'mixed': frame 0 holds 5 objects -- k0: negative raw predicted width, GT yaw -pi;
    k1: disjoint boxes in cell (H-1, W-1); k2, k3, k4 share cell (3, 5), k2 bitwise equal to the prediction there (t = 1) with yaw
    +pi --, slots k5..k7 hold values but no reg_mask; frame 1 is empty.  'empty': no object in either frame."""
    rng = np.random.default_rng(LOSS_SEEDS[name])
    B, C, H, W, K = LOSS_B, LOSS_C, LOSS_H, LOSS_W, LOSS_K
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    pred = dict(heatmap=(1.0 / (1.0 + np.exp(-f(B, C, H, W)))).astype(np.float32), iou=(0.5 * f(B, 1, H, W)).astype(np.float32),
                offset=rng.uniform(0, 1, (B, 2, H, W)).astype(np.float32), size=(np.abs(f(B, 3, H, W)) + 1.0).astype(np.float32),
                rot=f(B, 2, H, W), vel=f(B, 2, H, W))
    tgt = dict(heatmap=np.zeros((B, C, H, W), np.float32), ind=rng.integers(0, H * W, (B, K)).astype(np.int64),
               reg_mask=np.zeros((B, K), np.uint8), mask=np.zeros((B, K), np.uint8),
               target_offset=rng.uniform(0, 1, (B, K, 2)).astype(np.float32), target_size=(np.abs(f(B, K, 3)) + 1.0).astype(np.float32),
               target_rot=f(B, K, 2), target_vel=f(B, K, 2))
    if name == "empty":
        return pred, tgt

    def put(k, cy, cx, goff, gsize, grot, cls):
        tgt["ind"][0, k], tgt["reg_mask"][0, k], tgt["mask"][0, k] = cy * W + cx, 1, 1
        tgt["target_offset"][0, k], tgt["target_size"][0, k, :2], tgt["target_rot"][0, k] = goff, gsize, grot
        tgt["heatmap"][0, cls, cy, cx] = 1.0

    def cell(cy, cx, off, size, rot, iou):
        pred["offset"][0, :, cy, cx], pred["size"][0, :2, cy, cx], pred["rot"][0, :, cy, cx], pred["iou"][0, 0, cy, cx] = off, size, rot, iou

    cell(1, 10, (0.40, 0.55), (-0.5, 3.0), (0.2, -0.9), 0.1)                   # k0: negative raw width -> IoU 0, clamped in the DIoU
    put(0, 1, 10, (0.52, 0.43), (1.6, 3.6), _PI_ROT[-1], 0)
    cell(H - 1, W - 1, (0.90, 0.85), (0.5, 0.7), (0.28, 0.96), -0.4)           # k1: disjoint (1.6 m, 2.0 m apart), last cell
    put(1, H - 1, W - 1, (0.10, 0.05), (0.6, 0.8), (0.6, 0.8), 3)
    cell(3, 5, (0.30, 0.60), (1.8, 4.2), _PI_ROT[+1], 0.35)                    # k2, k3, k4: one cell, k2 identical to the prediction
    put(2, 3, 5, (0.30, 0.60), (1.8, 4.2), _PI_ROT[+1], 5)
    put(3, 3, 5, (0.45, 0.50), (2.3, 3.7), (0.3, -0.95), 5)
    put(4, 3, 5, (0.12, 0.74), (1.5, 4.9), (-0.25, 0.97), 9)
    return pred, tgt


# ---- score rectification -------------------------------------------------------------------------------------------------------------

def rectified_map(heat, iou, alpha):
    """fp64 (B, C, H, W): s^(1 - a_c) * q^a_c on the cells that survive the 3x3 keep mask of the raw heatmap, 0 elsewhere;
    q = clamp((iou + 1) / 2, 0, 1), NaN -> 0; a_c == 0 keeps s."""
    h = np.ascontiguousarray(heat, np.float32)
    keep = centernet_ref.max3x3(h) == h
    with np.errstate(invalid="ignore"):
        q = (np.asarray(iou, np.float64) + 1.0) / 2.0
    q = np.where(q > 0, np.minimum(q, 1.0), 0.0)                                # NaN compares false -> 0
    out = np.zeros(h.shape, np.float64)
    for c, a in enumerate(alpha):
        s = h[:, c].astype(np.float64)
        out[:, c] = s if a == 0 else np.power(s, 1.0 - a) * np.power(q[:, 0], a)
    return np.where(keep, out, 0.0)


def _take(v, K):
    """centernet_ref's rule on fp64 scores: the K largest under (score descending, position ascending)."""
    return np.lexsort((np.arange(v.size), -v))[:K]


def rectified_spec(heat, iou, alpha, K):
    """The decode's two-level top-K on the rectified map, in centernet_ref.topk_spec's format: (B, K) arrays score (fp64), cls,
    y, x, and score_bits (the fp64 score rounded to float32, for boxes_spec)."""
    m = rectified_map(heat, iou, alpha)
    B, C, H, W = m.shape
    flat = m.reshape(B, C, -1)
    cls_idx = np.stack([np.stack([_take(flat[b, c], K) for c in range(C)]) for b in range(B)])
    cls_val = np.take_along_axis(flat, cls_idx, 2).reshape(B, -1)
    pool = np.stack([_take(cls_val[b], K) for b in range(B)])
    idx = np.take_along_axis(cls_idx.reshape(B, -1), pool, 1)
    score = np.take_along_axis(cls_val, pool, 1)
    return dict(score=score, cls=pool // K, y=idx // W, x=idx % W, score_bits=centernet_ref.bits(score.astype(np.float32)))


def score_separation(spec, thresh):
    """The smallest relative gap between two consecutive positive scores of a frame, and between a positive score and the
    threshold: above box_iou_ref.MARGIN the order and the count do not depend on rounding."""
    gap = math.inf
    for row in spec["score"]:
        pos = row[row > 0]
        gap = min([gap] + [(a - b) / a for a, b in zip(pos[:-1], pos[1:])] + [abs(a - thresh) / max(a, thresh) for a in pos])
    return gap


DECODE_B, DECODE_C, DECODE_HW, DECODE_K = 2, 3, 16, 12
DECODE_ALPHA = (0.0, 0.5, 1.0)
DECODE_THRESH = 0.3
DECODE_SEED = 103
# (frame, class, y, x, raw score, iou value, (offset x, offset y) or None)
DECODE_PEAKS = (
    (0, 0, 2, 3, 0.85, -0.9, None), (0, 0, 9, 12, 0.45, 0.9, None), (0, 0, 13, 1, 0.20, 0.5, None),   # alpha 0: the raw scores
    (0, 1, 5, 5, 0.90, -0.6, (1.45, 0.5)),       # A: raw 0.90, q 0.2 -> 0.424; B's duplicate 0.1 cells away
    (0, 1, 5, 7, 0.60, 0.8, (-0.45, 0.5)),       # B: raw 0.60, q 0.9 -> 0.735: the order of A and B reverses
    (0, 1, 11, 11, 0.70, float("nan"), None),    # NaN -> q 0 -> 0
    (0, 2, 14, 8, 0.80, -0.8, None),             # alpha 1: q 0.1 -> 0.1, under the threshold: count drops
    (1, 2, 3, 3, 0.50, 1.7, None),               # iou outside [-1, 1] -> q 1 -> 1.0
    (1, 1, 8, 2, 0.75, -3.0, None),              # below -1 -> q 0 -> 0
    (1, 0, 15, 13, 0.65, 0.0, None), (1, 1, 0, 9, 0.55, 0.28, None), (1, 2, 10, 13, 0.95, -0.2, None),
)


def decode_scene():
    """Predictions (float32 arrays) of the decode tests: the planted peaks on a background that rises with the cell index from
    1e-3 to 2e-3, times 1 + c / 10 (its only local maximum is the last cell, so no flat region survives the keep mask: with alpha = 1 a surviving
    cell scores q whatever its heat), an iou map of -1 (q = 0) away from the peaks, random regression maps; A and B (class 1) get
    the same box 0.2 m apart."""
    rng = np.random.default_rng(DECODE_SEED)
    B, C, H = DECODE_B, DECODE_C, DECODE_HW
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    ramp = (1e-3 * (1.0 + np.arange(H * H) / (H * H))).astype(np.float32).reshape(H, H)
    scale = (1.0 + 0.1 * np.arange(C, dtype=np.float32))[None, :, None, None]            # no two classes tie at the last cell
    pred = dict(heatmap=(np.broadcast_to(ramp, (B, C, H, H)) * scale).astype(np.float32), iou=np.full((B, 1, H, H), -1.0, np.float32),
                offset=rng.uniform(0, 1, (B, 2, H, H)).astype(np.float32), size=(np.abs(f(B, 3, H, H)) + 1.0).astype(np.float32),
                rot=f(B, 2, H, H), vel=f(B, 2, H, H))
    for b, c, y, x, s, q, off in DECODE_PEAKS:
        pred["heatmap"][b, c, y, x], pred["iou"][b, 0, y, x] = s, q
        if off is not None:
            pred["offset"][b, :, y, x], pred["size"][b, :, y, x], pred["rot"][b, :, y, x] = off, (2.0, 4.5, 1.6), (0.6, 0.8)
    return pred
