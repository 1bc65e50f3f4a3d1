"""GPU checks of the box geometry kernels (csrc/box_nms.hip) against the fp64 restatement in tests/box_iou_ref.py: pairwise rotated
BEV / 3-D IoU within 1e-4 absolute (the project's standing parity budget; IoU lies in [0, 1]), NMS keep lists equal to the greedy
reference exactly, and the decode's opt-in NMS on synthetic head outputs with planted duplicate peaks.  The scenes and their
thresholds keep a 1e-3 margin (tests/test_box_nms_host.py), so nothing is excluded.

Each pairwise test prints its worst error before it asserts.  Not yet recorded from an MI355X run; the same fp32 arithmetic
compiled for the host stays within 7e-7 of the fp64 reference on every scene and on the degenerate set."""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib, box_ops, centernet_target, fusion_detection
from tests import box_iou_ref as R

pytestmark = pytest.mark.gpu
IOU_TOL = 1e-4


def _dev(x, gpu):
    return torch.as_tensor(x).to(gpu)


@pytest.mark.parametrize("mode", ["bev", "3d"])
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_pairwise_iou_scenes(gpu, name, mode):
    boxes, counts, _, _, _ = R.scene(name)
    fn = box_ops.boxes_iou_bev if mode == "bev" else box_ops.boxes_iou3d
    b, c = _dev(boxes, gpu), _dev(counts, gpu)
    out = fn(b, b, c, c)
    again = fn(b, b, c, c)
    assert out.shape == (len(counts), boxes.shape[1], boxes.shape[1]) and torch.equal(out, again)
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    worst = 0.0
    for f, n in enumerate(counts):
        want = np.zeros_like(got[f])
        want[:n, :n] = R.scene_iou(name, mode)[f]
        worst = max(worst, float(np.abs(got[f] - want).max()))
        assert (got[f, n:] == 0).all() and (got[f, :, n:] == 0).all()              # padded entries
    print(f"pairwise {mode} IoU {name}: worst |err| {worst:.3e}")
    assert worst <= IOU_TOL


@pytest.mark.parametrize("mode", ["bev", "3d"])
def test_pairwise_iou_degenerate_set(gpu, mode):
    d = R.degenerate_set()
    fn = box_ops.boxes_iou_bev if mode == "bev" else box_ops.boxes_iou3d
    a, b = _dev(d, gpu), _dev(d[::-1].copy(), gpu)                                  # unbatched (N,7) x (M,7), two different orders
    out = fn(a, b)
    assert out.shape == (len(d), len(d)) and torch.equal(out, fn(a, b))
    got = out.cpu().numpy().astype(np.float64)
    want = R.iou_matrix(d, d[::-1], mode)
    worst = float(np.abs(got - want).max())
    print(f"pairwise {mode} IoU degenerate set: worst |err| {worst:.3e}")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0 and worst <= IOU_TOL
    assert (got[[2, 3]] == 0).all()                                                 # zero width / zero length: 0 with everything


def _want_keep(name, mode, thresh, class_aware, post_max):
    boxes, counts, labels, _, _ = R.scene(name)
    out = []
    for f, n in enumerate(counts):
        out.append(R.nms(boxes[f, :n], mode, thresh, labels=labels[f, :n] if class_aware else None, post_max=post_max,
                         iou=R.scene_iou(name)[f] if mode == "rotate" else None))
    return out


@pytest.mark.parametrize("class_aware", [False, True])
@pytest.mark.parametrize("mode", ["rotate", "circle"])
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_nms_equals_greedy_reference(gpu, name, mode, class_aware):
    boxes, counts, labels, ths, radii = R.scene(name)
    B, N = boxes.shape[:2]
    b, c, l = _dev(boxes, gpu), _dev(counts, gpu), _dev(labels, gpu)
    scores = torch.linspace(1, 0, B * N, device=gpu).reshape(B, N)
    vels = torch.arange(B * N * 2, device=gpu, dtype=torch.float32).reshape(B, N, 2)
    for thresh in (ths if mode == "rotate" else radii):
        for post_max in (N, 7):
            run = lambda: _lib.nms_boxes(b, c, mode, thresh, post_max, scores=scores, labels=l, velocities=vels,
                                         class_aware=class_aware, gather=True)
            first, second = run(), run()
            assert all(torch.equal(x, y) for x, y in zip(first, second))            # deterministic
            keep_idx, keep_count, g_boxes, g_scores, g_labels, g_vels = (t.cpu() for t in first)
            want = _want_keep(name, mode, thresh, class_aware, post_max)
            for f in range(B):
                k = int(keep_count[f])
                assert keep_idx[f, :k].tolist() == want[f] and k == len(want[f]), (name, mode, thresh, class_aware, post_max, f)
                assert (keep_idx[f, k:] == -1).all()
                idx = torch.as_tensor(want[f], dtype=torch.long)
                assert torch.equal(g_boxes[f, :k], torch.as_tensor(boxes[f])[idx]) and (g_boxes[f, k:] == 0).all()
                assert torch.equal(g_scores[f, :k], scores.cpu()[f][idx]) and torch.equal(g_vels[f, :k], vels.cpu()[f][idx])
                assert torch.equal(g_labels[f, :k], torch.as_tensor(labels[f])[idx])


def test_public_nms_sorts_by_score_and_truncates(gpu):
    boxes, counts, labels, ths, radii = R.scene("b2_n300")
    n = int(counts[0])
    perm = np.random.default_rng(0).permutation(n)                                  # the scene's row order is its score order
    shuffled = boxes[0, :n][perm]                                                   # shuffled[i] = original row perm[i]
    sc = (1.0 - perm / n).astype(np.float32)                                        # lower original row = higher score
    want = R.nms(boxes[0, :n], "rotate", ths[1], iou=R.scene_iou("b2_n300")[0])
    inv = np.argsort(perm)                                                          # original row r sits at shuffled index inv[r]
    got = box_ops.nms_rotated(_dev(shuffled, gpu), _dev(sc, gpu), ths[1])
    assert got.dtype == torch.long and got.cpu().tolist() == [int(inv[r]) for r in want]
    got = box_ops.nms_rotated(_dev(shuffled, gpu), _dev(sc, gpu), ths[1], pre_max=100, post_max=9)
    want = R.nms(boxes[0, :100], "rotate", ths[1], post_max=9)
    assert got.cpu().tolist() == [int(inv[r]) for r in want]
    lab = labels[0, :n]
    got = box_ops.nms_circle(_dev(boxes[0, :n], gpu), _dev(sc[inv], gpu), radii[0], labels=_dev(lab, gpu))
    assert got.cpu().tolist() == R.nms(boxes[0, :n], "circle", radii[0], labels=lab)
    tie = box_ops.nms_circle(_dev(boxes[0, :8], gpu), torch.ones(8, device=gpu), 1e-3)          # ties: the lower index first
    assert tie.cpu().tolist() == list(range(8))
    assert box_ops.nms_rotated(torch.zeros(0, 7, device=gpu), torch.zeros(0, device=gpu), 0.5).numel() == 0


# ---- decode integration -----------------------------------------------------------------------------------------------------------

MODS = [(centernet_target, 2.048), (fusion_detection, 0.512)]


def _heads(voxel, gpu, dtype=torch.float32):
    maps, peaks = R.planted_heads(voxel)
    return {k: torch.as_tensor(v).to(gpu).to(dtype) for k, v in maps.items()}, peaks


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            assert x[k].dtype == y[k].dtype and x[k].device == y[k].device and torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("mod,voxel", MODS)
def test_decode_default_path_is_untouched(gpu, mod, voxel, monkeypatch):
    pred, _ = _heads(voxel, gpu)
    calls = []
    real = _lib._call
    monkeypatch.setattr(_lib, "_call", lambda name, *a: calls.append(name) or real(name, *a))
    plain = mod.decode_centernet_predictions(pred, 0.3, 100, True)
    n_plain, calls[:] = list(calls), []
    off = mod.decode_centernet_predictions(pred, 0.3, 100, True, nms_type=None, nms_iou_thresh=0.1, nms_pre_max=64)
    assert calls == n_plain == ["bevf_centernet_decode_f32"]                        # the same native launches
    _same(plain, off)
    calls[:] = []
    mod.decode_centernet_predictions(pred, 0.3, 100, True, nms_type="rotate")
    assert calls == ["bevf_centernet_decode_f32", "bevf_nms_boxes_f32"]


@pytest.mark.parametrize("mod,voxel", MODS)
def test_decode_with_rotated_nms(gpu, mod, voxel):
    pred, peaks = _heads(voxel, gpu)
    t = R.PLANTED_IOU_THRESH
    cand = mod.decode_centernet_predictions(pred, 0.3, 512, True)                   # the nms_pre_max decode, no NMS
    got = mod.decode_centernet_predictions(pred, 0.3, 100, True, nms_type="rotate", nms_iou_thresh=t)
    few = mod.decode_centernet_predictions(pred, 0.3, 5, True, nms_type="rotate", nms_iou_thresh=t)
    plain5 = mod.decode_centernet_predictions(pred, 0.3, 5, True)
    aware = mod.decode_centernet_predictions(pred, 0.3, 100, True, nms_type="rotate", nms_iou_thresh=t, class_aware=True)
    circ = mod.decode_centernet_predictions(pred, 0.3, 100, True, nms_type="circle", nms_radius=4.5 * voxel)
    for f, rows in enumerate(peaks):
        c = {k: v.cpu() for k, v in cand[f].items()}
        assert len(c["scores"]) == len(rows)                                        # the plain decode keeps every planted duplicate
        assert c["scores"].tolist() == [r[0] for r in rows] and c["labels"].tolist() == [r[1] for r in rows]
        assert np.abs(c["boxes"].numpy() - np.array([r[2] for r in rows])).max() < 1e-4
        boxes = c["boxes"].numpy()
        keep = torch.as_tensor(R.nms(boxes, "rotate", t), dtype=torch.long)
        for k in ("boxes", "scores", "labels", "velocities"):                       # gathered consistently
            assert torch.equal(got[f][k].cpu(), c[k][keep]), k
            assert torch.equal(few[f][k].cpu(), c[k][keep[:5]]), k                  # max_detections is applied after the NMS
        assert [rows[i][5] for i in keep.tolist()] == [True] * 12                   # duplicates gone: one box per object, its main peak
        keep_a = torch.as_tensor(R.nms(boxes, "rotate", t, labels=c["labels"].tolist()), dtype=torch.long)
        assert len(keep_a) == 36 and torch.equal(aware[f]["boxes"].cpu(), c["boxes"][keep_a])     # other-class duplicates survive
        keep_c = torch.as_tensor(R.nms(boxes, "circle", 4.5 * voxel), dtype=torch.long)
        assert torch.equal(circ[f]["scores"].cpu(), c["scores"][keep_c]) and len(keep_c) == 12
        assert got[f]["boxes"].is_cuda and got[f]["labels"].dtype == torch.long
    # cutting to 5 before the NMS would have kept a duplicate (frame 1's fifth score is one)
    assert any(not torch.equal(few[f]["scores"], plain5[f]["scores"]) for f in range(len(peaks)))


def test_decode_nms_bf16_heads_and_empty_frames(gpu):
    pred, _ = _heads(2.048, gpu)
    bf = {k: v.to(torch.bfloat16) for k, v in pred.items()}
    kw = dict(nms_type="rotate", nms_iou_thresh=R.PLANTED_IOU_THRESH, true_labels=True)
    _same(centernet_target.decode_centernet_predictions(bf, 0.3, 100, **kw),
          centernet_target.decode_centernet_predictions({k: v.float() for k, v in bf.items()}, 0.3, 100, **kw))
    empty = centernet_target.decode_centernet_predictions(pred, 0.99, 100, **kw)   # nothing above the threshold
    _same(empty, centernet_target.decode_centernet_predictions(pred, 0.99, 100, True))
    assert all(len(e["scores"]) == 0 and not e["boxes"].is_cuda for e in empty)
    with pytest.raises(_lib.BevfError, match="too large"):
        centernet_target.decode_centernet_predictions(pred, 0.3, 100, nms_type="rotate", nms_pre_max=1024)


def test_non_finite_candidates_stay_in_range(gpu):
    """One decode + NMS call and one IoU call on candidates with NaN / inf sizes and headings, as an untrained head can emit."""
    pred, peaks = _heads(2.048, gpu)
    bad = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -1.0, 1e30], device=gpu)
    for k, rows in (("size", 3), ("rot", 2)):
        flat = pred[k].view(pred[k].shape[0], rows, -1)
        flat[:, :, ::7] = bad[torch.arange(flat[:, :, ::7].shape[-1], device=gpu) % len(bad)]
    out = centernet_target.decode_centernet_predictions(pred, 0.3, 100, True, nms_type="rotate", nms_iou_thresh=0.2)
    for f, o in enumerate(out):
        n = len(o["scores"])
        assert 0 < n <= min(100, len(peaks[f])) and bool(torch.isfinite(o["scores"]).all())
        assert bool((o["scores"][1:] <= o["scores"][:-1]).all()) and bool(((o["labels"] >= 0) & (o["labels"] < 10)).all())
    cand = centernet_target.decode_centernet_predictions(pred, 0.3, 512, True)[0]["boxes"]
    iou = box_ops.boxes_iou_bev(cand, cand)
    assert bool(torch.isfinite(iou).all()) and float(iou.min()) >= 0.0 and float(iou.max()) <= 1.0
