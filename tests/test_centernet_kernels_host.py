"""CPU side of the CenterNet kernel pins (tests/test_gpu_centernet_kernels.py): the references agree with each other, every
case in tests/golden/cases.py has the property it is there for, and the float32 yardstick of the loss is far below the
effect of one dropped positive.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import ref_targets
from tests import centernet_ref as R
from tests.conftest import load_golden, rel_err
from tests.golden import cases

TIE_FREE_MASKED = [c for c in cases.CN_DECODE_CASES if c["masked"] and not c["ties"]]
FIXTURE_CASES = [c for c in cases.CN_DECODE_CASES if c.get("fixture")]


def canon(scores, boxes):
    """Order of tests.test_gpu_targets_decode._canon: (score descending, x, y)."""
    key = np.stack([-np.asarray(scores, np.float64), np.asarray(boxes, np.float64)[:, 0], np.asarray(boxes, np.float64)[:, 1]], 1)
    return sorted(range(len(key)), key=lambda i: tuple(key[i]))


def assert_detections_match_spec(c, tag, dets):
    """`dets`: per frame a dict of boxes / scores / labels / velocities holding the detections above the threshold (the
    oracle's or the reference's, computed in float32)."""
    pred, spec, thresh, box = R.decode_case(c)
    bs = box[tag]
    for b, d in enumerate(dets):
        n = int(bs["count"][b])
        got = {k: np.asarray(v) for k, v in d.items()}
        assert got["boxes"].shape == (n, 7) and got["scores"].shape == (n,), (b, got["boxes"].shape, n)
        if n == 0:
            continue
        o = canon(got["scores"], got["boxes"])
        want_scores = spec["score_bits"][b, :n].view(np.float32)
        s = canon(want_scores, np.stack([bs["x"][b, :n], bs["y"][b, :n]], 1))
        assert np.array_equal(R.bits(got["scores"][o]), spec["score_bits"][b, :n][s])
        assert (got["labels"] == 0).all()                                              # the reference's class is always 0
        gb = got["boxes"][o].astype(np.float64)
        assert (np.abs(gb[:, 0] - bs["x"][b, :n][s]) <= bs["x_bound"][b, :n][s]).all()
        assert (np.abs(gb[:, 1] - bs["y"][b, :n][s]) <= bs["y_bound"][b, :n][s]).all()
        assert (gb[:, 2] == -1).all()
        assert np.array_equal(R.bits(got["boxes"][o][:, 3:6]), bs["size_bits"][b, :n][s])
        assert rel_err(gb[:, 6], bs["yaw"][b, :n][s]) <= 2e-6
        assert np.array_equal(R.bits(got["velocities"][o]), bs["vel_bits"][b, :n][s])


@pytest.mark.parametrize("tag", ["ct", "fd"])
@pytest.mark.parametrize("c", TIE_FREE_MASKED, ids=lambda c: c["name"])
def test_spec_reproduces_the_oracle_decode(c, tag):
    pred, _, thresh, _ = R.decode_case(c)
    dets = ref_targets.decode(pred, thresh, c["K"], R.VOXEL[tag])
    assert_detections_match_spec(c, tag, [{k: v.numpy() for k, v in d.items()} for d in dets])


@pytest.mark.parametrize("tag", ["ct", "fd"])
@pytest.mark.parametrize("c", FIXTURE_CASES, ids=lambda c: c["name"])
def test_spec_reproduces_the_reference_fixtures(c, tag):
    gold = load_golden(f"decode_{tag}_{c['name']}")
    dets = [{k: gold[f"{k}_{b}"] for k in ("boxes", "scores", "labels", "velocities")} for b in range(c["B"])]
    assert_detections_match_spec(c, tag, dets)


@pytest.mark.parametrize("c", cases.CN_TARGET_CASES, ids=lambda c: c["name"])
def test_oracle_targets_reproduce_the_reference_fixtures(c):
    boxes, labels = cases.cn_target_inputs(c)
    t = ref_targets.make_targets(boxes, labels, **cases.cn_target_kwargs(c))
    gold = load_golden("targets_" + c["name"])
    assert sorted(gold) == sorted(t)
    for k, v in t.items():
        g = gold[k]
        assert v.numpy().dtype == g.dtype and v.shape == g.shape, k
        same = np.array_equal(R.bits(v), R.bits(g)) if v.is_floating_point() else np.array_equal(v.numpy(), g)
        assert same, k


# ---- every case has the property it is there for ------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", cases.CN_DECODE_CASES, ids=lambda c: c["name"])
def test_decode_case_properties(c):
    pred = cases.cn_decode_predictions(c)
    heat = pred["heatmap"]
    n = c["H"] * c["W"]
    assert not torch.isnan(heat).any()
    class_ties, pool_ties = R.tie_counts(heat, c["K"], c["masked"])
    assert (class_ties >= 2) if "class" in c["ties"] else class_ties == 0, class_ties
    assert (pool_ties >= 2) if "pool" in c["ties"] else pool_ties == 0, pool_ties
    if c.get("fixture"):
        assert c["masked"] and not c["ties"]
    name = c["name"]
    if name in ("one", "row37", "row37_raw", "special"):
        assert n < 1024                                               # fewer cells than threads: empty per-thread chunks
    if name.startswith(("row37", "k1023", "k4096")) or name.endswith("k960"):
        assert c["K"] == n
    if name == "c1":
        assert c["C"] == 1 and 1024 < n and c["K"] < n
    if name == "quant_k300":
        top = int((heat[0, 0] == heat.max()).sum())
        assert 0 < top < c["K"] < n                                   # scores above the K-th and ties at it in one selection
    if name.startswith("k1023"):
        assert c["K"] == 1023 and c["C"] * c["K"] == 2046             # one below a power of two: one pad key, two in the pool
    if name.startswith("k4096"):
        assert c["K"] == 4096 and c["C"] * c["K"] == 8192             # the LDS limits of both sorts
    if name == "quant_k960":
        assert c["refused"] and c["C"] * c["K"] > 8192
    if name == "stride2":
        assert heat.numel() == 2099520 > 8192 * 256                   # more scores than the key kernel's largest grid has threads
    if name.startswith("quant"):
        assert len(torch.unique(heat)) == 4
    if name == "const_ulp":
        assert len(torch.unique(heat)) == 2
    if name == "special":
        assert sorted(np.unique(R.bits(heat)).tolist()) == sorted(R.bits(np.array(cases.CN_SPECIAL_VALUES, np.float32)).tolist())
        d = np.float32(cases.CN_DENORMAL)
        assert 0 < d < np.finfo(np.float32).tiny
    if name == "peaks":
        kept = R.keep_mask(heat.numpy())
        assert ((kept > 0).sum((1, 2, 3)) == 50).all() and c["K"] > 50           # K exceeds the survivors: zero-score tail
    if name == "thresh_eq":
        _, spec, thresh, box = R.decode_case(c)
        b, r = c["thresh_rank"]
        assert np.float32(thresh).view(np.uint32) == spec["score_bits"][b, r]
        assert int(box["ct"]["count"][b]) == r                                    # strict >: the equal score is not counted


TARGET_STATS = {      # objects kept per frame, cells with >= 2 objects, most objects in one cell, highest owning slot, heatmap ones
    "cap700_40x72": ([490, 490], 72, 4, 499, 973),
    "dense300_17x9": ([294, 294], 180, 6, 299, 544),
    "mixed_16x24": ([30, 30, 30], 1, 2, 29, 90),
    "border_8x8": ([64], 13, 4, 63, 61),
    "border_ulp_8x8": ([56], 7, 2, 63, 56),
    "grid_1x1": ([10, 10], 2, 10, 9, 14),
    "grid_1x7": ([10, 10], 7, 3, 9, 20),
    "onecls_12x12": ([4, 4], 0, 1, 9, 8),
    "own300_1x1": ([294], 1, 294, 299, 10),
    "lds4096_32x32": ([4014], 913, 10, 4095, 3238),
}


@pytest.mark.parametrize("c", cases.CN_TARGET_CASES, ids=lambda c: c["name"])
def test_target_case_properties(c):
    boxes, labels = cases.cn_target_inputs(c)
    kw = cases.cn_target_kwargs(c)
    st = R.target_stats(ref_targets.make_targets(boxes, labels, **kw))
    assert (st["objects"], st["collide_cells"], st["deepest"], st["top_owner"], st["ones"]) == TARGET_STATS[c["name"]]
    pi32 = np.float32(np.pi)
    for b in boxes:
        yaw = b[:, 6].numpy()
        assert (np.abs(yaw) <= pi32).all() and yaw[0] == 0 and yaw[1] == pi32 and yaw[2] == -pi32
    name = c["name"]
    if name == "cap700_40x72":
        assert all(len(b) == 700 > kw["max_objects"] for b in boxes)              # more objects than max_objects
    if name in ("cap700_40x72", "dense300_17x9", "own300_1x1", "lds4096_32x32"):
        assert st["top_owner"] > 256                                              # an owner beyond the first 256-object stride
    if name == "mixed_16x24":
        assert [b.shape[1] for b in boxes] == [9, 7, 9]
    if name == "lds4096_32x32":
        assert len(boxes[0]) == kw["max_objects"] == 4096
    if name == "border_ulp_8x8":
        assert st["objects"] == [56]                                              # the column at x_min falls off the grid
    assert len(cases.cn_target_inputs(cases.CN_TARGET_OVER)[0][0]) == 4097 == cases.CN_TARGET_OVER["max_objects"]


@pytest.mark.parametrize("c", cases.CN_LOSS_CASES, ids=lambda c: c["name"])
def test_loss_case_properties_and_yardstick(c):
    """The bound the GPU test applies (max(4 x float32 yardstick, floor)) is at most a tenth of what one dropped positive
    changes, per term; for the total only where the heatmap has a positive to drop (without one the heatmap term is an
    unnormalised sum three orders above the regression terms, and so is its rounding)."""
    pred, tgt = cases.cn_loss_inputs(c)
    heat_t, logit = tgt["heatmap"], pred["heatmap"]
    name = c["name"]
    if name in ("one", "n250"):
        assert heat_t.numel() < 256
    if name == "no_positive":
        assert int((heat_t == 1).sum()) == 0 and float(heat_t.max()) < 1
    else:
        assert int((heat_t == 1).sum()) >= 1
    if name == "mask_zero":
        assert int(tgt["reg_mask"].sum()) == 0 and int(tgt["ind"].max()) > 0
    if name == "clamp":
        s = torch.sigmoid(logit.double())
        lo, hi = s < 1e-4, s > 1 - 1e-4
        assert int(lo.sum()) == 16 and int(hi.sum()) == 16                        # +-9.3 and +-20, eight times each
        assert int((lo & (heat_t == 1)).sum()) > 0 and int((hi & (heat_t == 1)).sum()) > 0
        assert int((lo & (heat_t < 1)).sum()) > 0 and int((hi & (heat_t < 1)).sum()) > 0
        assert int((logit.abs() == 9).sum()) == 16                                # just inside the clamp
    if name == "near_one":
        below = np.nextafter(np.float32(1), np.float32(0))
        assert int((heat_t == float(below)).sum()) >= 1
    if name == "four_in_cell":
        _, counts = np.unique(tgt["ind"][0].numpy(), return_counts=True)
        assert sorted(counts.tolist()) == [1, 1, 2, 4] and int(tgt["reg_mask"].sum()) == 8
    if name == "k500":
        assert R.target_stats(tgt)["deepest"] >= 3                                # three or more objects gather from one cell
    bounds = R.loss_bounds(pred, tgt)
    effect = R.drop_one_positive(pred, tgt)
    for k, (v, yard, bound) in bounds.items():
        print(f"YARD {name} {k} value {v:.6g} yardstick {yard:.3g} bound {bound:.3g} one positive {effect[k]}")
        if effect[k] is None or (k == "total_loss" and effect["heatmap_loss"] is None):
            continue
        assert 10 * bound <= effect[k], (k, bound, effect[k])
