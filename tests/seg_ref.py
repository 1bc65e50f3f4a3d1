"""fp64 restatement of the BEV map-segmentation kernels (include/bevf.h, "BEV map-segmentation head"): the
axis-aligned grid resample with its per-corner weights and inside masks, its transpose, the sigmoid focal loss with its gradient,
and the IoU counts.  numpy / torch on the host; tests/test_seg_head_host.py pins it to torch's own grid_sample, binary cross
entropy and autograd."""
import math

import numpy as np
import torch

EPS = 2.0 ** -24


def grid_of(rng, H, W):
    """[xmin, ymin, xmax, ymax] over H rows (y), W columns (x) -> (x0, y0, vx, vy)."""
    x0, y0, x1, y1 = (float(v) for v in rng)
    return x0, y0, (x1 - x0) / W, (y1 - y0) / H


def axis(in0, ivox, n_in, out0, ovox, n_out):
    """One axis: lower neighbour i0 [n_out] (int64), fraction f [n_out], ok [n_out] (the sample point is finite and within one cell
    of the input)."""
    with np.errstate(invalid="ignore"):
        q = (out0 + (np.arange(n_out, dtype=np.float64) + 0.5) * ovox - in0) / ivox - 0.5
        ok = (q > -1.0) & (q < n_in)
    qs = np.where(ok, q, 0.0)
    i0 = np.floor(qs)
    return i0.astype(np.int64), np.where(ok, qs - i0, 0.0), ok


def corners(in_grid, out_grid, Hi, Wi, Ho, Wo):
    """Per output cell and corner k = (di, dj) = (k >> 1, k & 1): (row [4][Ho][Wo], column, weight in fp64, inside mask).  The weight
    is the product of the two axis factors, 0 where the sample point is not ok; inside says whether the corner lies in the input."""
    x0, y0, vx, vy = in_grid
    ox0, oy0, ovx, ovy = out_grid
    i0, fi, oki = axis(y0, vy, Hi, oy0, ovy, Ho)
    j0, fj, okj = axis(x0, vx, Wi, ox0, ovx, Wo)
    ok = oki[:, None] & okj[None, :]
    rows, cols, w, inside = [], [], [], []
    for k in range(4):
        di, dj = k >> 1, k & 1
        r = np.broadcast_to((i0 + di)[:, None], (Ho, Wo))
        c = np.broadcast_to((j0 + dj)[None, :], (Ho, Wo))
        wk = np.where(ok, (fi if di else 1.0 - fi)[:, None] * (fj if dj else 1.0 - fj)[None, :], 0.0)
        rows.append(r), cols.append(c), w.append(wk)
        inside.append(ok & (r >= 0) & (r < Hi) & (c >= 0) & (c < Wi))
    return np.stack(rows), np.stack(cols), np.stack(w), np.stack(inside)


def resample(x, in_grid, out_grid, Ho, Wo):
    """x [B][Hi][Wi][C] fp64 -> (y [B][Ho][Wo][C], vmax [B][Ho][Wo][C] = the largest |corner value| that entered each element)."""
    B, Hi, Wi, C = x.shape
    r, c, w, inside = corners(in_grid, out_grid, Hi, Wi, Ho, Wo)
    y = np.zeros((B, Ho, Wo, C))
    vmax = np.zeros((B, Ho, Wo, C))
    for k in range(4):
        v = x[:, np.clip(r[k], 0, Hi - 1), np.clip(c[k], 0, Wi - 1)] * inside[k][None, :, :, None]
        y += w[k][None, :, :, None] * v
        vmax = np.maximum(vmax, np.abs(v))
    return y, vmax


def resample_bwd(dy, in_grid, out_grid, Hi, Wi):
    """dy [B][Ho][Wo][C] fp64 -> (dx [B][Hi][Wi][C], mag = sum |w dy| per element, n [Hi][Wi] = contributing targets per cell)."""
    B, Ho, Wo, C = dy.shape
    r, c, w, inside = corners(in_grid, out_grid, Hi, Wi, Ho, Wo)
    dx, mag, n = np.zeros((B, Hi, Wi, C)), np.zeros((B, Hi, Wi, C)), np.zeros((Hi, Wi), dtype=np.int64)
    for k in range(4):
        use = inside[k] & (w[k] != 0.0)
        ii, jj = np.nonzero(use)
        rr, cc, ww = r[k][ii, jj], c[k][ii, jj], w[k][ii, jj]
        np.add.at(n, (rr, cc), 1)
        for b in range(B):
            np.add.at(dx[b], (rr, cc), ww[:, None] * dy[b, ii, jj])
            np.add.at(mag[b], (rr, cc), np.abs(ww[:, None] * dy[b, ii, jj]))
    return dx, mag, n


def torch_grid(in_grid, out_grid, Hi, Wi, Ho, Wo):
    """The normalised sampling grid (1, Ho, Wo, 2) with which torch.nn.functional.grid_sample(align_corners=False) samples the same
    points: x_norm = 2 (qj + 0.5) / Wi - 1."""
    x0, y0, vx, vy = in_grid
    ox0, oy0, ovx, ovy = out_grid
    xo = ox0 + (torch.arange(Wo, dtype=torch.float64) + 0.5) * ovx
    yo = oy0 + (torch.arange(Ho, dtype=torch.float64) + 0.5) * ovy
    gx = 2.0 * ((xo - x0) / vx) / Wi - 1.0
    gy = 2.0 * ((yo - y0) / vy) / Hi - 1.0
    return torch.stack([gx[None, :].expand(Ho, Wo), gy[:, None].expand(Ho, Wo)], -1)[None]


def focal_elements(x, t, alpha=-1.0, gamma=2.0):
    """Elementwise a_t (1 - p_t)^gamma BCE(x, t) in x's dtype (torch): the stable form max(x, 0) - x t + log1p(exp(-|x|))."""
    p = torch.sigmoid(x)
    pt = t * p + (1 - t) * (1 - p)
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    loss = (1 - pt) ** gamma * bce
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


def focal(x, t, alpha=-1.0, gamma=2.0):
    """x, t (B, K, Ho, Wo) torch of one dtype -> (per_class [K] = means over B * Ho * Wo, loss = their sum)."""
    per_class = focal_elements(x, t, alpha, gamma).mean(dim=(0, 2, 3))
    return per_class, per_class.sum()


def focal_grad(x, t, alpha=-1.0, gamma=2.0):
    """d loss / d x in closed form, fp64 (torch): sign a_t m^gamma (gamma n bce + m) / (B P) with m = 1 - p_t, n = p_t, sign = -1
    where t = 1 and +1 where t = 0; p and 1 - p from exp(-|x|), so nothing cancels at large |x|."""
    x, t = x.double(), t.double()
    e = torch.exp(-x.abs())
    big, small = 1 / (1 + e), e / (1 + e)
    p, q = torch.where(x >= 0, big, small), torch.where(x >= 0, small, big)
    m, n = torch.where(t > 0, q, p), torch.where(t > 0, p, q)
    bce = x.clamp(min=0) - x * t + torch.log1p(e)
    at = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(x)
    sign = torch.where(t > 0, -torch.ones_like(x), torch.ones_like(x))
    B, _, H, W = x.shape
    return sign * at * m ** gamma * (gamma * n * bce + m) / (B * H * W)


def threshold_logits(thresholds):
    """Probability thresholds -> fp32 logits, rounded from fp64 (seg_head.threshold_logits restated)."""
    return np.array([math.log(v / (1.0 - v)) for v in thresholds], dtype=np.float64).astype(np.float32)


def iou_counts(logits, targets, thr_logits):
    """logits fp32 (B, K, Ho, Wo), targets {0, 1}, thr_logits fp32 [T] -> int64 [T][K][3] (TP, FP, FN), prediction logit >= thr."""
    lg, tg = np.asarray(logits, dtype=np.float32), np.asarray(targets) != 0
    out = np.zeros((len(thr_logits), lg.shape[1], 3), dtype=np.int64)
    for ti, th in enumerate(np.asarray(thr_logits, dtype=np.float32)):
        pred = lg >= th
        out[ti, :, 0] = (pred & tg).sum(axis=(0, 2, 3))
        out[ti, :, 1] = (pred & ~tg).sum(axis=(0, 2, 3))
        out[ti, :, 2] = (~pred & tg).sum(axis=(0, 2, 3))
    return out


class SegHeadRef(torch.nn.Module):
    """BEVSegmentationHead as plain torch.nn (same state-dict keys): grid_sample with torch_grid, then the classifier."""

    def __init__(self, in_channels, num_classes, hidden, in_grid, out_grid, bev_hw, out_hw):
        super().__init__()
        nn = torch.nn
        self.classifier = nn.Sequential(nn.Conv2d(in_channels, hidden, 3, padding=1), nn.BatchNorm2d(hidden), nn.ReLU(),
                                        nn.Conv2d(hidden, hidden, 3, padding=1), nn.BatchNorm2d(hidden), nn.ReLU(),
                                        nn.Conv2d(hidden, num_classes, 1))
        self.grid = torch_grid(in_grid, out_grid, *bev_hw, *out_hw)

    def resampled(self, x):
        g = self.grid.to(x.dtype).expand(x.shape[0], -1, -1, -1)
        return torch.nn.functional.grid_sample(x, g, mode="bilinear", padding_mode="zeros", align_corners=False)

    def forward(self, x):
        return self.classifier(self.resampled(x))
