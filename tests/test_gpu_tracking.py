"""The tracker step on the device (csrc/track.hip through tracking.Tracker) against the numpy restatement
(tests/track_ref.py) on the fixed scenes whose margins tests/test_tracking_host.py::test_scene_margins checks: ids, slots, hits, ages,
counts and every fp32 column that only passes through fp64 mul / add are compared exactly, the coasted yaw (atan2) to 1e-5 rad."""
import functools

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import centernet_target as CT
from bevfusion_multimodal_3d_object_detection_amd import tracking
from tests import track_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
_DET = ("boxes", "velocities", "scores", "labels", "count")


@functools.lru_cache(maxsize=None)
def _scenes():
    return {s["name"]: s for s in R.all_scenes()}


@functools.lru_cache(maxsize=None)
def _reference(name):
    return R.run(_scenes()[name])


def _tracker(scene):
    B = scene["frames"][0]["boxes"].shape[0]
    trk = tracking.Tracker(B, scene["C"], max_tracks=scene["T"], max_dist=scene["max_dist"].tolist(), max_age=scene["max_age"],
                           birth_score=scene["birth_score"], class_aware=scene["class_aware"], device=DEV)
    if scene["init"] is not None:
        for k, v in scene["init"].items():
            trk.state[k].copy_(torch.from_numpy(v))
    return trk


def _inputs(fr):
    det = tuple(torch.from_numpy(fr[k]).to(DEV) for k in _DET)
    return det, torch.from_numpy(fr["ego_motion"]).to(DEV), torch.from_numpy(fr["dt"]).to(DEV)


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _compare(name, f, out, st, ref_out, ref_st):
    for k in ("det_track_id", "det_slot", "det_hits", "overflow"):
        assert out[k].dtype == ref_out[k].dtype and np.array_equal(out[k], ref_out[k]), (name, f, k)
    for k in ("track_count", "next_id", "track_id", "track_label", "track_age", "track_hits"):
        assert st[k].dtype == ref_st[k].dtype and np.array_equal(st[k], ref_st[k]), (name, f, k)
    for k in ("track_vel", "track_score"):
        assert np.array_equal(st[k], ref_st[k], equal_nan=True), (name, f, k)
    assert np.array_equal(st["track_box"][..., :6], ref_st["track_box"][..., :6], equal_nan=True), (name, f, "centre, z, size")
    yaw, ref_yaw, coasted = st["track_box"][..., 6], ref_st["track_box"][..., 6], ref_st["track_age"] > 0
    assert np.array_equal(yaw[~coasted], ref_yaw[~coasted]), (name, f, "copied yaw")
    if coasted.any():
        worst = float(np.abs(yaw[coasted].astype(np.float64) - ref_yaw[coasted]).max())
        assert worst <= 1e-5, (name, f, "coasted yaw", worst)


def _run_and_compare(name):
    scene = _scenes()[name]
    trk = _tracker(scene)
    for f, (fr, (ref_out, ref_st)) in enumerate(zip(scene["frames"], _reference(name))):
        det, ego, dt = _inputs(fr)
        out = trk.step(det, ego, dt)
        _compare(name, f, _host(out), _host(trk.state), ref_out, ref_st)
    return trk


@pytest.mark.parametrize("ndet", R.EDGE_COUNTS)
@pytest.mark.parametrize("tcnt", R.EDGE_COUNTS)
def test_edge_counts(tcnt, ndet):
    """track_count x detections in {0, 1, 63, 64, 65, 257}^2 (N = 0 included; 257 tracks take the 16-slots-per-lane kernel), matches,
    births, coasting and overflow mixed, NaN / huge padding rows past count."""
    _run_and_compare(f"edge_t{tcnt}_n{ndet}")


@pytest.mark.parametrize("name", [s["name"] for s in R.rule_scenes()])
def test_rules(name):
    _run_and_compare(name)


@pytest.mark.parametrize("name", [s["name"] for s in R.rival_scenes()])
def test_rivals_and_ties(name):
    """2 to 4 free tracks inside one detection's limit, on both kernels: rivals in different lanes (the wave minimum) and in one lane
    (slots s, s + 64, s + 128), the nearest in the higher slot, a later detection taking the runner-up, and exact ties, which go to
    the lower slot."""
    _run_and_compare(name)


def test_sequence_with_dropouts_clutter_and_ego_rotation():
    """12 frames, 2 streams: the device and the restatement agree after every step."""
    trk = _run_and_compare("sequence_ego")
    live = trk.tracks()
    assert [t["id"].shape[0] for t in live] == trk.state["track_count"].tolist() and live[0]["box"].shape[1] == 7


def test_padding_rows_change_nothing():
    """The same step with the rows past count zeroed instead of NaN / huge: identical outputs and state."""
    scene = _scenes()["edge_t64_n65"]
    fr = scene["frames"][0]
    clean = dict(fr, boxes=fr["boxes"].copy(), velocities=fr["velocities"].copy(), scores=fr["scores"].copy(), labels=fr["labels"].copy())
    n = int(fr["count"][0])
    assert np.isnan(fr["boxes"][0, n:, 2:]).all() and np.isinf(fr["scores"][0, n:]).all()
    for k in ("boxes", "velocities", "scores", "labels"):
        clean[k][0, n:] = 0
    res = []
    for f in (fr, clean):
        trk = _tracker(scene)
        det, ego, dt = _inputs(f)
        res.append((_host(trk.step(det, ego, dt)), _host(trk.state)))
    for a, b in zip(res[0], res[1]):
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_detection_forms_and_reset():
    """A dict, the decode's list of per-frame dicts and a number for dt give what the padded tensors give; reset clears streams."""
    scene = _scenes()["three_streams"]
    fr = scene["frames"][0]
    fr = dict(fr, dt=np.full(3, 0.5, np.float32))
    det, ego, dt = _inputs(fr)
    a = _tracker(scene)
    want = _host(a.step(det, ego, dt))
    b = _tracker(scene)
    got = _host(b.step(dict(zip(_DET, det)), fr["ego_motion"], 0.5))
    c = _tracker(scene)
    frames = [{"boxes": det[0][s, :n], "velocities": det[1][s, :n], "scores": det[2][s, :n], "labels": det[3][s, :n]}
              for s, n in enumerate(fr["count"].tolist())]
    packed = _host(c.step(frames, ego, 0.5))
    for k in want:
        assert np.array_equal(want[k], got[k]) and np.array_equal(want[k], packed[k]), k
    for k in a.state:
        assert torch.equal(a.state[k], b.state[k]) and torch.equal(a.state[k], c.state[k]), k
    next_id = a.state["next_id"].clone()
    a.reset([0, 2])
    assert a.state["track_count"].tolist() == [0, int(b.state["track_count"][1]), 0] and torch.equal(a.state["next_id"], next_id)
    assert (a.state["track_id"][0] == -1).all() and not a.state["track_box"][2].any() and torch.equal(a.state["track_box"][1], b.state["track_box"][1])
    a.reset(ids=True)
    assert not a.state["next_id"].any() and not a.state["track_count"].any()
    with pytest.raises(L.BevfError, match="CPU tensor"):
        a.step(tuple(t.cpu() for t in det), ego, dt)


def test_graph_replay_equals_eager():
    """One captured step on static input buffers, replayed for three frames with the inputs refreshed in place, equals the eager run
    bit for bit (outputs and state)."""
    scene = _scenes()["sequence_ego"]
    frames = scene["frames"][:3]
    eager = _tracker(scene)
    want = []
    for fr in frames:
        det, ego, dt = _inputs(fr)
        want.append((_host(eager.step(det, ego, dt)), _host(eager.state)))
    trk = _tracker(scene)
    static = _inputs(frames[0])[:2]                                   # dt stays the default number: filled on the device, capturable
    assert all(float(v) == 0.5 for fr in frames for v in fr["dt"])
    flat = list(static[0]) + [static[1]]
    trk.step(*static)                                                 # once eagerly before the capture
    trk.reset(ids=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = trk.step(*static)
    trk.reset(ids=True)                                               # the capture itself launched nothing
    for fr, (ref_out, ref_st) in zip(frames, want):
        det, ego, dt = _inputs(fr)
        for s, t in zip(flat, list(det) + [ego]):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        got_out, got_st = _host(out), _host(trk.state)
        for k in ref_out:
            assert np.array_equal(got_out[k], ref_out[k]), k
        for k in ref_st:
            assert np.array_equal(got_st[k], ref_st[k], equal_nan=True), k


def _planted_heads(objects, f, side=50, classes=3, voxel=2.048, x_min=-51.2):
    """Head maps of one frame with one peak per object = (x, y, vx, vy, label) at time 0.5 f."""
    heat = torch.full((1, classes, side, side), 0.01)
    off, size, rot, vel = torch.zeros(1, 2, side, side), torch.ones(1, 3, side, side), torch.zeros(1, 2, side, side), torch.zeros(1, 2, side, side)
    rot[:, 1] = 1.0
    for j, (x, y, vx, vy, lab) in enumerate(objects):
        cx, cy = (x + vx * 0.5 * f - x_min) / voxel, (y + vy * 0.5 * f - x_min) / voxel
        col, row = int(cx), int(cy)
        heat[0, lab, row, col] = 0.9 - 0.1 * j
        off[0, 0, row, col], off[0, 1, row, col] = cx - col, cy - row
        vel[0, 0, row, col], vel[0, 1, row, col] = vx, vy
    return {k: v.to(DEV).contiguous() for k, v in (("heatmap", heat), ("offset", off), ("size", size), ("rot", rot), ("vel", vel))}


def test_decode_padded_into_tracker_keeps_ids():
    """Planted peaks moved by their planted velocity for three frames: decode_padded (true labels, circle NMS) -> Tracker.step without
    a host read keeps one id per object, and decode_centernet_predictions on the same maps returns what the direct launches return."""
    objects = [(-30.3, -20.1, 1.5, -0.8, 0), (10.2, 25.7, -1.2, 1.9, 1), (31.4, -12.6, 0.6, 1.1, 2), (-5.5, 3.3, -1.8, -1.4, 1)]
    kw = dict(score_thresh=0.3, max_detections=20, true_labels=True, nms_type="circle", nms_radius=1.0, nms_pre_max=32)
    trk = tracking.Tracker(1, 3, max_tracks=16, max_dist=2.0, max_age=2, birth_score=0.2, device=DEV)
    ids = []
    for f in range(3):
        pred = _planted_heads(objects, f)
        padded = CT.decode_padded(pred, **kw)
        out = trk.step(padded, None, 0.5)
        n = int(padded["count"][0])
        assert n == len(objects) and padded["labels"][0, :n].tolist() == [o[4] for o in objects]
        ids.append(out["det_track_id"][0, :n].tolist())
        assert out["det_hits"][0, :n].tolist() == [f + 1] * n
        # the list decode is unchanged: the padded records cut at count, and the launches it has always made
        frames = CT.decode_centernet_predictions(pred, **kw)
        boxes, scores, labels, vels, count = L.centernet_decode({k: v.float().contiguous() for k, v in pred.items()}, 32, 0.3, 2.048,
                                                                CT.PC_RANGE[0], CT.PC_RANGE[1], True)
        _, count, boxes, scores, labels, vels = L.nms_boxes(boxes, count, "circle", 1.0, 20, scores=scores, labels=labels, velocities=vels,
                                                            class_aware=False, gather=True)
        assert int(count[0]) == n and len(frames) == 1
        for key, direct in (("boxes", boxes), ("scores", scores), ("labels", labels), ("velocities", vels)):
            assert torch.equal(frames[0][key], direct[0, :n]) and torch.equal(frames[0][key], padded[key][0, :n]), key
    assert ids[0] == [0, 1, 2, 3] and ids[1] == ids[0] and ids[2] == ids[0]
    assert int(trk.state["track_count"][0]) == 4 and trk.state["track_hits"][0, :4].tolist() == [3] * 4
