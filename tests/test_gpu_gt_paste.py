"""Points-in-boxes and the GT-paste augmentation (csrc/gt_paste.hip, gt_paste.py) on the MI355X against the numpy
restatement of tests/gt_paste_ref.py: indices and accept flags equal the fp64 geometry, every output element equals the fp32
reference bit for bit.  The scenes' margins are asserted in tests/test_gt_paste_host.py, so nothing is excluded here."""
import functools

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import box_ops, centernet_target, fusion, synth
from bevfusion_multimodal_3d_object_detection_amd import gt_paste as G
from tests import gt_paste_ref as R

pytestmark = pytest.mark.gpu


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _bank(d):
    return G.ObjectBank(_cu(d["points"]), _cu(d["obj_ptr"]), _cu(d["boxes"]), _cu(d["labels"]))


def _same(got, ref):
    """Every entry of the paste's result against the reference dict, bit for bit."""
    for k, want in ref.items():
        if want is None:
            assert got[k] is None, k
            continue
        g = got[k].cpu().numpy()
        assert g.dtype == want.dtype and g.shape == want.shape, (k, g.dtype, g.shape, want.dtype, want.shape)
        assert np.array_equal(_bits(g), _bits(want)), k


# ---- points_in_boxes -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pib(C):
    pts, counts, boxes, mask = R.pib_scene(C)
    ref = np.stack([R.points_in_boxes_ref(pts[b], counts[b], boxes[b], mask[b])[0] for b in range(R.PIB_B)])
    return pts, counts, boxes, mask, ref


@pytest.mark.parametrize("C", [4, 5])
def test_points_in_boxes_equals_the_fp64_reference(gpu, C):
    pts, counts, boxes, mask, ref = _pib(C)
    got = box_ops.points_in_boxes(_cu(pts), _cu(boxes), _cu(counts), _cu(mask))
    again = box_ops.points_in_boxes(_cu(pts), _cu(boxes), _cu(counts), _cu(mask))
    assert got.dtype == torch.int32 and tuple(got.shape) == (R.PIB_B, R.PIB_N)
    g = got.cpu().numpy()
    print(f"points_in_boxes C={C}: {(g >= 0).sum()} points inside, {len(np.unique(g)) - 1} boxes hit")
    assert np.array_equal(g, ref)
    for b in range(R.PIB_B):
        assert (g[b, counts[b]:] == -1).all()
    assert torch.equal(got, again)
    as_bool = box_ops.points_in_boxes(_cu(pts), _cu(boxes), _cu(counts), _cu(mask >= 0))
    assert torch.equal(as_bool, got)
    as_i32 = box_ops.points_in_boxes(_cu(pts), _cu(boxes), counts.tolist(), _cu(mask.astype(np.int32)))
    assert torch.equal(as_i32, got)


@pytest.mark.parametrize("C", [4, 5])
def test_points_in_boxes_unbatched_and_without_mask(gpu, C):
    pts, counts, boxes, mask, ref = _pib(C)
    one = box_ops.points_in_boxes(_cu(pts[1]), _cu(boxes[1]), int(counts[1]), _cu(mask[1]))
    assert tuple(one.shape) == (R.PIB_N,) and np.array_equal(one.cpu().numpy(), ref[1])
    free = box_ops.points_in_boxes(_cu(pts[0]), _cu(boxes[0]))
    want, worst = R.points_in_boxes_ref(pts[0], None, boxes[0], None)
    assert worst >= R.MARGIN and np.array_equal(free.cpu().numpy(), want) and not np.array_equal(want, ref[0])
    none = box_ops.points_in_boxes(_cu(pts[:, :0]), _cu(boxes))
    assert tuple(none.shape) == (R.PIB_B, 0)
    empty = box_ops.points_in_boxes(_cu(pts), _cu(boxes[:, :0]))
    assert (empty == -1).all()


# ---- paste ---------------------------------------------------------------------------------------------------------------------------

PASTE_CASES = [(7, 9), (9, 7), (9, 9)]


@functools.lru_cache(maxsize=None)
def _scene(ncol, bank_ncol):
    s = R.paste_scene(ncol, bank_ncol)
    return s, R.paste_ref(*s)


def _nan_buffers(B, M, Kc, ncol, capacity, C, vel=True):
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    i = lambda dt, *s: torch.full(s, -7, dtype=dt, device="cuda")
    return dict(lidar_points=f(B, capacity, C), lidar_count=i(torch.int32, B), gt_boxes=f(B, M + Kc, ncol), gt_labels=i(torch.int64, B, M + Kc),
                gt_velocities=f(B, M + Kc, 2) if vel else None, accepted=i(torch.int32, B, Kc))


def _paste(scene, capacity=None, cand=None, with_vel=True):
    lidar, counts, gt, labels, vel, bank, c = scene
    c = c if cand is None else cand
    params = G.PasteParams(c)
    dbank = _bank(bank)
    cap = G.default_capacity(dbank, params, lidar.shape[1]) if capacity is None else capacity
    bufs = _nan_buffers(lidar.shape[0], gt.shape[1], c.shape[1], gt.shape[2], cap, lidar.shape[2], with_vel)
    out = G.paste(_cu(lidar), _cu(counts), _cu(gt), _cu(labels), _cu(vel) if with_vel else None, dbank, params, capacity, out=bufs)
    for k, v in bufs.items():
        assert v is None or out[k].data_ptr() == v.data_ptr(), k                     # the preallocated buffers are the result
    return out


@pytest.mark.parametrize("ncol,bank_ncol", PASTE_CASES)
def test_paste_equals_the_reference_bit_for_bit(gpu, ncol, bank_ncol):
    scene, ref = _scene(ncol, bank_ncol)
    lidar, counts, gt, labels, vel, bank, cand = scene
    out = _paste(scene)
    acc = out["accepted"].cpu().numpy()
    print(f"paste ({ncol}, {bank_ncol}): accepted {acc.tolist()}, counts {out['lidar_count'].tolist()} of capacity {out['lidar_points'].shape[1]}")
    assert np.array_equal(acc, R.PASTE_EXPECT)
    _same(out, ref)                                                                  # every element written: no NaN / -7 survives
    M = gt.shape[1]
    assert np.array_equal(_bits(out["gt_boxes"][:, :M]), _bits(gt)) and np.array_equal(_bits(out["gt_velocities"][:, :M]), _bits(vel))
    assert np.array_equal(out["gt_labels"][:, :M].cpu().numpy(), labels)
    pts, cnt = out["lidar_points"].cpu().numpy(), out["lidar_count"].cpu().numpy()
    for b in range(3):
        assert (pts[b, cnt[b]:].view(np.int32) == 0).all()                           # the padding is +0
    rej = out["gt_labels"][:, M:].cpu().numpy() < 0
    assert np.array_equal(rej, acc == 0) and (out["gt_boxes"][:, M:].cpu().numpy()[rej] == 0).all()
    again = _paste(scene)
    for k in out:
        assert np.array_equal(_bits(out[k]), _bits(again[k])), k


def test_paste_without_velocities_and_with_int32_labels(gpu):
    scene, ref = _scene(9, 9)
    lidar, counts, gt, labels, vel, bank, cand = scene
    out = G.paste(_cu(lidar), _cu(counts), _cu(gt), _cu(labels.astype(np.int32)), None, _bank(bank), G.PasteParams(cand))
    assert out["gt_velocities"] is None and out["gt_labels"].dtype == torch.int32
    assert np.array_equal(out["gt_labels"].cpu().numpy(), ref["gt_labels"])
    for k in ("lidar_points", "lidar_count", "gt_boxes", "accepted"):
        assert np.array_equal(_bits(out[k]), _bits(ref[k])), k


def test_paste_of_no_candidates_returns_the_inputs_bits(gpu):
    scene, _ = _scene(9, 9)
    lidar, counts, gt, labels, vel, bank, cand = scene
    out = _paste(scene, cand=np.full_like(cand, -1))
    N, M = lidar.shape[1], gt.shape[1]
    assert tuple(out["lidar_points"].shape) == (3, N, lidar.shape[2]) and np.array_equal(out["lidar_count"].cpu().numpy(), counts)
    pts = out["lidar_points"].cpu().numpy()
    for b in range(3):
        assert np.array_equal(pts[b, :counts[b]].view(np.int32), lidar[b, :counts[b]].view(np.int32))
        assert (pts[b, counts[b]:].view(np.int32) == 0).all()
    assert np.array_equal(_bits(out["gt_boxes"][:, :M]), _bits(gt)) and (out["gt_boxes"][:, M:] == 0).all()
    assert (out["gt_labels"][:, M:] == -1).all() and (out["accepted"] == 0).all() and (out["gt_velocities"][:, M:] == 0).all()


def test_a_small_capacity_keeps_the_first_rows(gpu):
    scene, ref = _scene(9, 9)
    lidar, counts, gt, labels, vel, bank, cand = scene
    sizes = np.diff(bank["obj_ptr"])
    appended0 = int(sum(sizes[c] for c, a in zip(cand[0], R.PASTE_EXPECT[0]) if a))
    kept0 = int(ref["lidar_count"][0]) - appended0
    for cap in (1000, kept0 + 70, 3):                                              # inside the survivors / inside the second object / tiny
        assert cap < ref["lidar_count"][0]
        out = _paste(scene, capacity=cap)
        want = R.paste_ref(*scene, capacity=cap)
        _same(out, want)
        assert np.array_equal(_bits(out["lidar_points"]), _bits(ref["lidar_points"][:, :cap]))
        assert np.array_equal(out["lidar_count"].cpu().numpy(), np.minimum(ref["lidar_count"], cap))


# ---- the bank out of frames ----------------------------------------------------------------------------------------------------------

def test_from_frames_then_paste_gives_the_cropped_objects_back(gpu):
    lidar, counts, gt, labels = R.frames_scene()
    objs, _ = R.crop_ref(lidar, counts, gt, labels, R.FRAMES_MIN_POINTS)
    bank = G.ObjectBank.from_frames(_cu(lidar), _cu(counts), _cu(gt), _cu(labels), min_points=R.FRAMES_MIN_POINTS)
    assert len(bank) == len(objs) == 8 and bank.channels == R.FRAMES_C and bank.points.is_cuda
    assert list(bank.host_sizes) == [o[2].shape[0] for o in objs]
    assert np.array_equal(_bits(bank.boxes), _bits(np.stack([gt[b, j] for b, j, _ in objs])))
    assert list(bank.host_labels) == [int(labels[b, j]) for b, j, _ in objs]
    world = np.concatenate([o[2] for o in objs])
    assert np.array_equal(bank.points[:, 3:].cpu().numpy(), world[:, 3:])
    again = G.ObjectBank.from_state_dict(bank.state_dict(), "cuda")
    assert torch.equal(again.points, bank.points) and torch.equal(again.obj_ptr, bank.obj_ptr)
    empty = torch.zeros(1, 1, R.FRAMES_C, device="cuda")
    out = G.paste(empty, torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, 7, device="cuda"),
                  torch.full((1, 1), -1, dtype=torch.int64, device="cuda"), None, bank, G.PasteParams(np.arange(8, dtype=np.int32)[None]))
    assert (out["accepted"] == 1).all() and int(out["lidar_count"][0]) == world.shape[0] == out["lidar_points"].shape[1] - 1
    got = out["lidar_points"][0, :world.shape[0]].cpu().numpy()
    assert np.array_equal(got[:, 3:], world[:, 3:])                                  # other channels exactly
    err = np.abs(got[:, :3].astype(np.float64) - world[:, :3].astype(np.float64))
    ulp = np.spacing(np.abs(world[:, :3])).astype(np.float64)
    print(f"from_frames round trip: {world.shape[0]} points, worst {float((err / ulp).max()):.2f} ulp, {int((err > 0).sum())} coordinates moved")
    assert (err <= ulp).all()                                                        # xyz to one ulp
    assert np.array_equal(_bits(out["gt_boxes"][0, 1:]), _bits(bank.boxes))


# ---- augment_batch -------------------------------------------------------------------------------------------------------------------

def _world(B, seed=2):
    st = A.AugmentSettings(flip=True, scale=(0.95, 1.05), rotation=(-20.0, 20.0), translation=(0.5, 0.5, 0.2), radar_noise_std=0.01)
    return st, A.sample(st, B, 1, (8, 8), (8, 8), np.random.default_rng(seed))


def test_augment_batch_with_paste_is_paste_then_augment_batch(gpu):
    scene, ref = _scene(9, 9)
    lidar, counts, gt, labels, vel, bank, cand = (x if isinstance(x, dict) else _cu(x) for x in scene)
    dbank, pp = _bank(bank), G.PasteParams(scene[6])
    st, p = _world(3)
    radar = [synth.normal((3, 25, 7), 50 + r).cuda() for r in range(2)]
    gen = lambda: torch.Generator(device="cuda").manual_seed(4)
    one = A.augment_batch(None, lidar, counts, radar, gt, labels, vel, p, st, max_points=2048, generator=gen(), paste=pp, bank=dbank)
    mid = G.paste(lidar, counts, gt, labels, vel, dbank, pp)
    two = A.augment_batch(None, mid["lidar_points"], mid["lidar_count"], radar, mid["gt_boxes"], mid["gt_labels"], mid["gt_velocities"], p,
                          st, max_points=2048, generator=gen())
    assert np.array_equal(one["paste_accepted"].cpu().numpy(), R.PASTE_EXPECT) and "paste_accepted" not in two
    for k in ("lidar_points", "lidar_count", "gt_boxes", "gt_labels", "gt_velocities"):
        assert np.array_equal(_bits(one[k]), _bits(two[k])), k
    for a, b in zip(one["radar_points"], two["radar_points"]):
        assert np.array_equal(_bits(a), _bits(b))
    assert tuple(one["gt_boxes"].shape) == (3, 22, 9) and int(one["lidar_count"][2]) > 0


def test_augment_batch_without_paste_is_what_it_was(gpu):
    scene, _ = _scene(9, 9)
    lidar, counts, gt, labels, vel = (_cu(x) for x in scene[:5])
    st, p = _world(3)
    out = A.augment_batch(None, lidar, counts, None, gt, labels, vel, p, st, max_points=2048)
    pts, cnt = A.transform_filter_pad_lidar(lidar, counts, p, 2048)
    boxes, v = A.transform_boxes(gt, labels, vel, p, p.scale)
    assert "paste_accepted" not in out and out["gt_labels"] is labels
    for got, want in ((out["lidar_points"], pts), (out["lidar_count"], cnt), (out["gt_boxes"], boxes), (out["gt_velocities"], v)):
        assert np.array_equal(_bits(got), _bits(want))
    none = A.augment_batch(None, lidar, counts, None, gt, labels, vel, p, st, max_points=2048, paste=G.PasteParams(np.zeros((3, 0), np.int32)),
                           bank=_bank(scene[5]))
    assert "paste_accepted" not in none and np.array_equal(_bits(none["lidar_points"]), _bits(pts))     # settings without candidates


# ---- a training step -----------------------------------------------------------------------------------------------------------------

def test_a_pasted_batch_trains_a_lidar_radar_detector(gpu):
    scene, _ = _scene(9, 9)
    lidar, counts, gt, labels, vel, bank, cand = scene
    bank4 = dict(bank, points=np.ascontiguousarray(bank["points"][:, :4]))
    B, M = 3, gt.shape[1]
    p = A.neutral_params(B, 1, (8, 8), (8, 8))
    for b in range(B):
        p.bev_aug[b] = A.world_transform(False, False, np.radians(10.0), 1.02, (0.37, -0.21, 0.05))
        p.scale[b] = 1.02
    radar = [synth.normal((B, 25, 7), 60 + r).cuda() for r in range(5)]
    o = A.augment_batch(None, _cu(lidar[..., :4]), _cu(counts), radar, _cu(gt), _cu(labels), _cu(vel), p, A.AugmentSettings(), max_points=2048,
                        paste=G.PasteParams(cand), bank=_bank(bank4))
    acc = o["paste_accepted"].cpu().numpy()
    assert np.array_equal(acc, R.PASTE_EXPECT)
    model = fusion.create_detector("lidar+radar", "bev", "centernet", bev_h=50, bev_w=50)
    synth.fill_state_dict_(model, 11)
    model = model.cuda().train()
    pred = model(None, o["lidar_points"], o["radar_points"])
    tgt = centernet_target.prepare_centernet_targets({"gt_boxes": o["gt_boxes"], "gt_labels": o["gt_labels"]}, "cuda", bev_size=(50, 50))
    losses = centernet_target.CenterNetLoss()(pred, tgt)
    losses["total_loss"].backward()
    assert all(torch.isfinite(v).all() for v in losses.values()) and all(torch.isfinite(v).all() for v in pred.values())
    assert sum(float(q.grad.abs().sum()) for q in model.parameters() if q.grad is not None) > 0
    heat = tgt["heatmap"].cpu().numpy()
    boxes, labs = o["gt_boxes"].cpu().numpy().astype(np.float64), o["gt_labels"].cpu().numpy()
    for b in range(B):
        cells = set()
        for r in range(M + cand.shape[1]):
            if labs[b, r] < 0:
                assert r < M or (acc[b, r - M] == 0 and (boxes[b, r] == 0).all())       # a rejected row: nothing to aim at
                continue
            px, py = (boxes[b, r, 0] + 51.2) / 2.048, (boxes[b, r, 1] + 51.2) / 2.048
            if not (0 <= px < 50 and 0 <= py < 50):
                assert r < M                                                            # every pasted object lands inside the grid
                continue
            assert min(px % 1, 1 - px % 1, py % 1, 1 - py % 1) > 1e-3                   # not on a cell border
            assert heat[b, labs[b, r], int(py), int(px)] == 1.0, (b, r)
            cells.add((int(labs[b, r]), int(py), int(px)))
        assert acc[b].sum() == (labs[b, M:] >= 0).sum()
        assert int((heat[b] == 1.0).sum()) == len(cells)                                # and no other peak: none for a rejected row
