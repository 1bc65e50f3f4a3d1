"""TEST INFRASTRUCTURE -- exact / float64 statements of what the CenterNet decode, keep-mask and loss kernels compute.

Plain numpy / torch on the CPU.  The selection rule is stated here on its own (not through torch.topk, whose order among
equal scores is unspecified); targets and losses come from the committed oracle, oracle/ref_targets.py.
"""
import numpy as np
import torch

from oracle import ref_targets

U32 = 2.0 ** -24                     # unit roundoff of float32
NEG_INF = np.float32(-np.inf)


# ---- order of scores ------------------------------------------------------------------------------------------------------------

def ordered_bits(v: np.ndarray) -> np.ndarray:
    """float32 -> uint32 whose unsigned order is the numeric order of the floats, with -0.0 < +0.0 (no NaN)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bits(v) -> np.ndarray:
    """The raw bit patterns of a float32 array / tensor, for bit-equality asserts that tell -0.0 from +0.0."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def max3x3(v: np.ndarray) -> np.ndarray:
    """Maximum over the 3x3 neighbourhood clipped at the plane's border; v is (..., H, W)."""
    H, W = v.shape[-2:]
    p = np.full(v.shape[:-2] + (H + 2, W + 2), NEG_INF, dtype=np.float32)
    p[..., 1:-1, 1:-1] = v
    m = v.copy()
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, p[..., dy:dy + H, dx:dx + W])
    return m


def keep_mask(v: np.ndarray) -> np.ndarray:
    """The decode's mask: v where v is the maximum of its 3x3 neighbourhood, +0.0 elsewhere."""
    return np.where(max3x3(v) == v, v, np.float32(0.0)).astype(np.float32)


def nms_rule(v: np.ndarray) -> np.ndarray:
    """`heat * keep` of the reference's _nms: v where it is the 3x3 maximum, v * 0 elsewhere (so a masked negative is -0.0)."""
    return np.where(max3x3(v) == v, v, v * np.float32(0.0)).astype(np.float32)


# ---- selection ---------------------------------------------------------------------------------------------------------------------

def _take(ob: np.ndarray, K: int) -> np.ndarray:
    """Positions of the K largest of a 1-D array of ordered bits under (score descending, position ascending)."""
    return np.lexsort((np.arange(ob.size), -ob.astype(np.int64)))[:K]


def topk_spec(heat, K: int, masked: bool):
    """The decode's documented selection rule, exactly.

    heat (B,C,H,W) float32.  With `masked`, a score first becomes `v if max3x3(v) == v else 0`.  Per (frame, class) the K
    largest under (score descending, flattened cell index ascending) form a (C,K) pool per frame; of that pool the K largest
    under (score descending, pool position ascending) are returned, best first.

    Scores are compared through their ordered bit patterns (ordered_bits), not as floats: -0.0 ranks below +0.0 and a
    denormal ranks above both, which is the order of the kernel's integer keys; a float comparison would call -0.0 and +0.0
    a tie and leave their order to the position.  NaN scores are outside the rule.

    Returns a dict of (B,K) arrays: score_bits (uint32 raw float32 bits), pool (int64 position in the (C,K) pool), cls, y, x
    (int64), plus cls_bits / cls_idx (B,C,K): the per-class stage."""
    h = np.ascontiguousarray(heat.detach().cpu().numpy() if isinstance(heat, torch.Tensor) else heat, dtype=np.float32)
    B, C, H, W = h.shape
    n = H * W
    assert 1 <= K <= n
    v = keep_mask(h) if masked else h
    ob = ordered_bits(v).reshape(B, C, n)
    raw = bits(v).reshape(B, C, n)
    cls_idx = np.empty((B, C, K), np.int64)
    for b in range(B):
        for c in range(C):
            cls_idx[b, c] = _take(ob[b, c], K)
    cls_ob = np.take_along_axis(ob, cls_idx, 2)
    cls_bits = np.take_along_axis(raw, cls_idx, 2)
    pool = np.stack([_take(cls_ob[b].reshape(-1), K) for b in range(B)])
    idx = np.take_along_axis(cls_idx.reshape(B, -1), pool, 1)
    return dict(score_bits=np.take_along_axis(cls_bits.reshape(B, -1), pool, 1), pool=pool, cls=pool // K, y=idx // W, x=idx % W,
                cls_bits=cls_bits, cls_idx=cls_idx)


def tie_counts(heat, K: int, masked: bool):
    """(class_ties, pool_ties): how many scores equal the K-th one, summed over the cuts at which at least one of them is
    left out.  0 means the selection does not depend on how ties are ordered."""
    sp = topk_spec(heat, K, masked)
    h = np.ascontiguousarray(heat.detach().cpu().numpy() if isinstance(heat, torch.Tensor) else heat, dtype=np.float32)
    B, C, H, W = h.shape
    ob = ordered_bits(keep_mask(h) if masked else h).reshape(B, C, -1)
    cls_ob = ordered_bits(sp["cls_bits"].view(np.float32))

    def cut(all_ob, taken_ob):
        t = taken_ob.min()
        n_all, n_taken = int((all_ob == t).sum()), int((taken_ob == t).sum())
        return n_all if n_all > n_taken else 0
    class_ties = sum(cut(ob[b, c], cls_ob[b, c]) for b in range(B) for c in range(C))
    pool_ob = ordered_bits(sp["score_bits"].view(np.float32))
    pool_ties = sum(cut(cls_ob[b].reshape(-1), pool_ob[b]) for b in range(B))
    return class_ties, pool_ties


def case_thresh(c, spec) -> float:
    """The score threshold of a decode case; `thresh_rank` = (frame, rank) names one returned score, used bit for bit."""
    if "thresh_rank" in c:
        b, r = c["thresh_rank"]
        return float(spec["score_bits"].view(np.float32)[b, r])
    return float(c["thresh"])


VOXEL = {"ct": 2.048, "fd": 0.512}             # cell size of the two drop-in decoders
ORIGIN = ref_targets.PC_RANGE[0], ref_targets.PC_RANGE[1]
_decode_cases = {}


def decode_case(c):
    """(pred, spec, thresh, {"ct" | "fd": boxes_spec}) of a tests.golden.cases decode case; computed once, shared by the
    tests that need it, never modified."""
    from tests.golden import cases
    if c["name"] not in _decode_cases:
        pred = cases.cn_decode_predictions(c)
        spec = topk_spec(pred["heatmap"], c["K"], c["masked"])
        thresh = case_thresh(c, spec)
        _decode_cases[c["name"]] = (pred, spec, thresh, {t: boxes_spec(pred, spec, thresh, v, *ORIGIN) for t, v in VOXEL.items()})
    return _decode_cases[c["name"]]


# ---- box assembly --------------------------------------------------------------------------------------------------------------------

def boxes_spec(pred, spec, thresh: float, voxel: float, x_min: float, y_min: float):
    """Box assembly in float64 for the cells `spec` selected.  voxel / x_min / y_min enter as the float32 values the kernel
    is handed.  Returns x, y, yaw (float64, (B,K)) with the bounds |fp32 result - exact| may reach for x and y (see
    xy_bound), size_bits (B,K,3) and vel_bits (B,K,2) (copies: raw float32 bits), and count (B,) = #(score > thresh)."""
    B, K = spec["x"].shape
    bi = np.arange(B)[:, None]
    g = lambda name: pred[name].detach().cpu().numpy()[bi, :, spec["y"], spec["x"]]          # (B,K,channels)
    off, size, rot, vel = g("offset"), g("size"), g("rot"), g("vel")
    v, xm, ym = (float(np.float32(t)) for t in (voxel, x_min, y_min))
    tx, ty = spec["x"] + off[..., 0].astype(np.float64), spec["y"] + off[..., 1].astype(np.float64)
    score = spec["score_bits"].view(np.float32)
    return dict(x=tx * v + xm, y=ty * v + ym, x_bound=xy_bound(tx, v, xm), y_bound=xy_bound(ty, v, ym),
                yaw=np.arctan2(rot[..., 0].astype(np.float64), rot[..., 1].astype(np.float64)),
                size_bits=bits(size), vel_bits=bits(vel), count=(score > np.float32(thresh)).sum(1))


def xy_bound(t, v, m):
    """|fl(fl(fl(i + off) * v) + m) - ((i + off) * v + m)| for exact t = i + off: the sum, the product and the last sum each
    round once, relative error <= u = 2^-24 each.  The first two scale |t v|, the last scales the result:
    <= u (2 |t v| + |t v + m|) to first order; the factor (1 + 4u) covers the cross terms of three roundings.  With the
    product and last sum contracted into one fma the product's rounding disappears, which is inside the same bound."""
    return U32 * (2 * np.abs(t * v) + np.abs(t * v + m)) * (1 + 4 * U32)


# ---- losses --------------------------------------------------------------------------------------------------------------------------

LOSS_TERMS = ("total_loss", "heatmap_loss", "offset_loss", "size_loss", "rot_loss", "vel_loss")
LOSS_W = tuple(ref_targets.LOSS_WEIGHTS[k] for k in ("heatmap", "offset", "size", "rot", "vel"))


def _cast(d, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}


def loss_f64(pred, tgt, grad: bool = False):
    """The oracle's loss on float64 inputs -> ({term: python float}, {head: float64 gradient of total_loss} or None)."""
    p = _cast(pred, torch.float64)
    if grad:
        p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = ref_targets.centernet_loss(p, _cast(tgt, torch.float64))
    g = None
    if grad:
        out["total_loss"].backward()
        g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
    return {k: float(out[k].detach()) for k in LOSS_TERMS}, g


def loss_f32(pred, tgt):
    """The oracle's loss run in float32 on one thread (fixed summation order)."""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = ref_targets.centernet_loss(_cast(pred, torch.float32), _cast(tgt, torch.float32))
    finally:
        torch.set_num_threads(nt)
    return {k: float(out[k]) for k in LOSS_TERMS}


def loss_yardstick(pred, tgt):
    """Per loss term: (float64 value, |float32 oracle - float64 oracle|)."""
    v64, _ = loss_f64(pred, tgt)
    v32 = loss_f32(pred, tgt)
    return {k: (v64[k], abs(v32[k] - v64[k])) for k in LOSS_TERMS}


def loss_floor(v64):
    """What a float32 evaluation may miss by even when the float32 oracle happens to land on the float64 value (it does for
    the one-element case): the roundings after the last element has been added.

    A term is a block sum -- 6 shuffle steps and 3 adds of wave totals, 9 roundings on the path of every addend -- over a
    denominator (count * C + 1e-4: 2 roundings), then one division or one double -> float conversion: 12 roundings, each
    <= u = 2^-24 of the term, so 12 u |term|.  The total adds five weighted terms: one product and one sum each, 10 u of
    sum |w_q term_q|, on top of the terms' own floors.  In ulps (2u) that is 6 per term and up to 11 for the total.

    Not covered here: the error each element carries into the sum (expf, logf, the sigmoid's division, the products of the
    focal term) and the order of the additions before the block sum.  Those are left to the yardstick, whose float32 oracle
    makes the same kind of per-element errors; the floor only keeps a yardstick that happens to be near zero from asking
    the device for more than float32 can give."""
    fl = {k: 12 * U32 * abs(v64[k]) for k in LOSS_TERMS[1:]}
    wsum = sum(abs(w) * abs(v64[k]) for w, k in zip(LOSS_W, LOSS_TERMS[1:]))
    fl["total_loss"] = sum(abs(w) * fl[k] for w, k in zip(LOSS_W, LOSS_TERMS[1:])) + 10 * U32 * wsum
    return fl


def loss_bounds(pred, tgt):
    """{term: (float64 value, yardstick, bound)}, bound = max(4 x yardstick, floor): the 4 x margin is the one the seg-head
    focal loss uses."""
    y = loss_yardstick(pred, tgt)
    fl = loss_floor({k: v for k, (v, _) in y.items()})
    return {k: (v, e, max(4 * e, fl[k])) for k, (v, e) in y.items()}


def drop_one_positive(pred, tgt):
    """|change| of each float64 loss term when one positive goes missing: the first heatmap 1 becomes 0 and the first
    regression slot is unmasked.  None for a term that has no positive to drop."""
    base, _ = loss_f64(pred, tgt)
    t = {k: v.clone() for k, v in tgt.items()}
    flat = t["heatmap"].view(-1)
    ones = (flat == 1).nonzero()
    slots = t["reg_mask"].view(-1).nonzero()
    if len(ones):
        flat[ones[0]] = 0.0
    if len(slots):
        t["reg_mask"].view(-1)[slots[0]] = 0
    new, _ = loss_f64(pred, t)
    out = {k: abs(new[k] - base[k]) for k in LOSS_TERMS}
    if not len(ones):
        out["heatmap_loss"] = None
    if not len(slots):
        for k in LOSS_TERMS[2:]:
            out[k] = None
    if not len(ones) and not len(slots):
        out["total_loss"] = None
    return out


# ---- targets -------------------------------------------------------------------------------------------------------------------------

def target_stats(t):
    """Properties of a target dict a case is there for: per-frame object counts, cells claimed by >= 2 objects, the largest
    number of objects in one cell, the highest slot index that owns a cell, heatmap ones."""
    mask = t["mask"].numpy().astype(bool)
    ind = t["ind"].numpy()
    collide, deepest, top_owner = 0, 0, -1
    for b in range(mask.shape[0]):
        slots = np.nonzero(mask[b])[0]
        if not len(slots):
            continue
        cells, counts = np.unique(ind[b, slots], return_counts=True)
        collide += int((counts >= 2).sum())
        deepest = max(deepest, int(counts.max()))
        owner = {}
        for k in slots:
            owner[int(ind[b, k])] = int(k)
        top_owner = max(top_owner, max(owner.values()))
    return dict(objects=[int(m.sum()) for m in mask], collide_cells=collide, deepest=deepest, top_owner=top_owner,
                ones=int((t["heatmap"] == 1).sum()))
