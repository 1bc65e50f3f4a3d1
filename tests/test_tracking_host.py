"""Host checks of the tracker (tracking.py, _lib.track_step, csrc/track.hip), no GPU: the numpy restatement
(tests/track_ref.py) is pinned by closed forms, since the reference project has no tracker to compare with; every fixed scene the GPU
tests use keeps a margin at every decisive comparison; the binding equals include/bevf.h; arguments are refused before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib, temporal, tracking
from tests import track_ref as R
from tests.conftest import ROOT

BevfError = _lib.BevfError


def _ids(scene):
    """Per frame and stream, {object: track id} from the restatement's outputs and the scene's ground truth."""
    out = []
    for fr, (o, _) in zip(scene["frames"], R.run(scene)):
        out.append([{k: int(o["det_track_id"][b, i]) for i, k in enumerate(truth) if k >= 0} for b, truth in enumerate(fr["truth"])])
    return out


# ---- the restatement, by closed forms ----

@pytest.mark.parametrize("ego", [False, True])
def test_constant_velocity_objects_keep_their_ids(ego):
    K = 9
    ids = _ids(R.sequence_scene(frames=10, K=K, ego=ego, dropouts=(), clutter=False))
    for b in range(2):
        first = ids[0][b]
        assert sorted(first.values()) == list(range(K))               # K births in frame 0, ids 0 .. K-1
        assert all(frame[b] == first for frame in ids)                # and nothing else, ever


def test_rigid_motion_of_the_scene_with_matching_ego_changes_no_id():
    """Frames seen from a moving ego against the same world seen from a standing one: outputs and ids are the same."""
    still = R.sequence_scene(frames=8, ego=False)
    moving = R.sequence_scene(frames=8, ego=True)
    a, b = R.run(still), R.run(moving)
    for (oa, sa), (ob, sb) in zip(a, b):
        for k in ("det_track_id", "det_hits", "det_slot", "overflow"):
            assert np.array_equal(oa[k], ob[k]), k
        for k in ("track_id", "track_label", "track_age", "track_hits", "track_count", "next_id"):
            assert np.array_equal(sa[k], sb[k]), k


def test_permuting_the_streams_permutes_the_outputs():
    scene = R.sequence_scene(frames=6, B=3)
    perm = [2, 0, 1]
    other = dict(scene, frames=[{k: (v[perm] if isinstance(v, np.ndarray) else [v[p] for p in perm]) for k, v in fr.items()}
                                for fr in scene["frames"]])
    for (oa, sa), (ob, sb) in zip(R.run(scene), R.run(other)):
        for k in oa:
            assert np.array_equal(oa[k][perm], ob[k]), k
        for k in sa:
            assert np.array_equal(sa[k][perm], sb[k]), k


@pytest.mark.parametrize("gap", [1, 3, 4, 6])
def test_returning_object_keeps_its_id_iff_the_gap_is_within_max_age(gap):
    max_age = 3
    scene = R.sequence_scene(frames=10, B=1, K=4, dropouts=((2, 2, gap),), clutter=False, max_age=max_age)
    ids = _ids(scene)
    before, after = ids[1][0][2], ids[2 + gap][0][2]
    assert 2 not in ids[2][0]
    assert (after == before) == (gap <= max_age)
    if gap > max_age:
        assert after == 4                                             # the next unused id
    for k in (0, 1, 3):                                               # the others never change
        assert len({frame[0][k] for frame in ids}) == 1


def test_two_detections_competing_for_one_track():
    """Both inside the limit of the only track: the earlier detection takes it although the later one is nearer; the later one is born."""
    st = R.new_state(1, 4)
    rng = np.random.default_rng(0)
    R.seed_tracks(st, 0, [0], rng, 1)
    st["track_vel"][:] = 0
    x, y = st["track_box"][0, 0, :2]
    fr = R.frame(1, 2)
    R.put(fr, 0, (x + 1.0, y), score=0.9)
    R.put(fr, 0, (x + 0.1, y), score=0.8)
    o = R.step(st, fr["boxes"], fr["velocities"], fr["scores"], fr["labels"], fr["count"], fr["ego_motion"], fr["dt"],
               np.array([2.0], np.float32), 3, 0.1, True)
    assert o["det_track_id"][0].tolist() == [100, 101] and o["det_hits"][0].tolist() == [2, 1] and o["det_slot"][0].tolist() == [0, 1]
    assert st["track_count"][0] == 2 and st["next_id"][0] == 102
    assert np.array_equal(st["track_box"][0, 0], fr["boxes"][0, 0]) and np.array_equal(st["track_box"][0, 1], fr["boxes"][0, 1])


def test_coasting_closed_form():
    """One track, no detection, a known rigid motion: the coasted record against numpy's own matrix algebra."""
    st = R.new_state(1, 2)
    st["track_box"][0, 0] = (10.0, -4.0, 0.5, 2.0, 4.0, 1.5, 0.25)
    st["track_vel"][0, 0] = (2.0, 1.0)
    st["track_score"][0, 0], st["track_label"][0, 0], st["track_id"][0, 0], st["track_hits"][0, 0] = 0.7, 1, 5, 2
    st["track_count"][0], st["next_id"][0] = 1, 6
    M = temporal.ego_motion(np.eye(4), R.rigid(0.3, 1.0, 2.0, 0.1))   # the ego moved by (1, 2, 0.1) and turned 0.3 rad
    fr = R.frame(1, 0)
    fr["ego_motion"][0] = M
    R.step(st, fr["boxes"], fr["velocities"], fr["scores"], fr["labels"], fr["count"], fr["ego_motion"], fr["dt"],
           np.array([2.0, 2.0], np.float32), 3, 0.0, True)
    inv = np.linalg.inv(M)
    want = inv @ np.array([10.0 + 2.0 * 0.5, -4.0 + 1.0 * 0.5, 0.5, 1.0])
    assert np.allclose(st["track_box"][0, 0, :3], want[:3], atol=1e-5)
    assert np.allclose(st["track_vel"][0, 0], (inv[:3, :3] @ np.array([2.0, 1.0, 0.0]))[:2], atol=1e-6)
    assert abs(float(st["track_box"][0, 0, 6]) - (0.25 - 0.3)) < 1e-6
    assert st["track_box"][0, 0, 3:6].tolist() == [2.0, 4.0, 1.5] and st["track_age"][0, 0] == 1 and st["track_hits"][0, 0] == 2
    assert st["track_id"][0, 0] == 5 and st["track_count"][0] == 1 and st["track_id"][0, 1] == -1


def test_padding_of_the_state_is_zero_with_id_minus_one():
    scene = R.rule_scenes()[0]
    for _, st in R.run(scene):
        n = int(st["track_count"][0])
        assert (st["track_id"][0, n:] == -1).all()
        for k in ("track_box", "track_vel", "track_score", "track_label", "track_age", "track_hits"):
            assert not st[k][0, n:].any(), k


# ---- the scenes of the GPU tests ----

def test_scene_margins():
    """Under the fp64 restatement every decisive comparison of every fixed GPU scene is >= 1e-3 away from flipping (distance against
    max_dist, best against second-best, score against birth_score), so the kernel's fp32 distances decide alike and no case needs
    excluding on the GPU.  'rival' is a runner-up inside the limit: the scenes must hold some, or the choice among several tracks is
    never made.  The one exception to the margin is the exact tie, which the rule gives to the lower slot: only in the tie scenes,
    and only on coordinates that make q, the differences and d2 exact in fp32 as in fp64."""
    scenes = R.all_scenes()
    assert len(scenes) == len(R.EDGE_COUNTS) ** 2 + len(R.rule_scenes()) + len(R.rival_scenes()) + 1
    seen, rivals = set(), 0
    for scene in scenes:
        margins = []
        R.run(scene, margins)
        ties = [m for m in margins if m[0] == "tie"]
        for kind, v in margins:
            if kind != "tie":
                assert v >= 1e-3, (scene["name"], kind, v)
            seen.add(kind)
        rivals += sum(kind == "rival" for kind, _ in margins)
        if scene["name"].startswith("tie_"):
            fr, st = scene["frames"][0], scene["init"]
            n = int(fr["count"][0])
            xy = np.concatenate([fr["boxes"][0, :n, :2].ravel(), st["track_box"][0, [s for pair in R.TIE_SLOTS for s in pair], :2].ravel()])
            assert len(ties) == len(R.TIE_SLOTS) and np.array_equal(2 * xy, np.round(2 * xy)) and np.abs(xy).max() < 1024
            assert not fr["velocities"].any() and np.array_equal(fr["ego_motion"][0], np.eye(4))
        else:
            assert not ties, scene["name"]
    assert seen == {"dist", "second", "rival", "tie", "score"} and rivals >= 10


def test_scenes_reach_what_their_names_say():
    by = {s["name"]: s for s in R.rule_scenes()}
    last = {k: R.run(s)[-1] for k, s in by.items()}
    o, st = last["overflow"]
    assert o["overflow"][0] == 1 and st["track_count"][0] == 8 and st["next_id"][0] == 108
    o0, _ = R.run(by["overflow"])[0]
    assert o0["overflow"][0] == 3 and o0["det_track_id"][0].tolist() == [106, 107, -1, -1, -1]
    assert last["age_at_max_survives"][1]["track_count"][0] == 6 and last["age_past_max_drops"][1]["track_count"][0] == 1
    assert last["all_coast"][1]["track_age"][0, :6].tolist() == [1] * 6
    assert last["all_matched"][0]["det_slot"][0].tolist() == [3, 0, 5, 1, 4, 2] and last["all_matched"][1]["track_count"][0] == 6
    assert last["none_matched"][1]["track_count"][0] == 12 and last["all_born"][1]["track_id"][0, :5].tolist() == [0, 1, 2, 3, 4]
    assert last["class_mismatch"][0]["det_track_id"][0].tolist() == [106, 104] and last["class_agnostic"][0]["det_track_id"][0].tolist() == [101, 104]
    o, st = last["per_class_max_dist"]
    labels = by["per_class_max_dist"]["frames"][0]["labels"][0]
    assert [(t < 106) for t in o["det_track_id"][0].tolist()] == [int(l) != 0 for l in labels]
    assert last["dt_zero"][0]["det_hits"][0].min() >= 2
    assert last["birth_score_sides"][0]["det_track_id"][0].tolist() == [0, -1, 1, -1]
    o, st = last["nan_detection"]
    assert o["det_track_id"][0].tolist() == [100, -1, 102, -1, -1, 105, -1, -1] and st["track_count"][0] == 6 and st["next_id"][0] == 106
    o, st = last["three_streams"]
    assert st["track_count"].tolist() == [5, 5, 6] and o["det_track_id"][2, :7].tolist() == [100, 101, 102, 103, 104, 105, -1]
    assert last["label_out_of_range"][0]["det_track_id"][0].tolist() == [102, 106]
    for T in R.RIVAL_T:                                               # ids are 100 + slot
        (o, st), = R.run(R.rival_scene(T))
        assert o["det_track_id"][0, :7].tolist() == [104, 101, 102, 174, 110, 112, 184] and (o["det_track_id"][0, 7:] == -1).all()
        (o, st), = R.run(R.tie_scene(T))
        assert o["det_track_id"][0, :3].tolist() == [102, 120, 107] and st["track_age"][0, [2, 7, 20, 84]].tolist() == [0, 0, 0, 1]
    seq = R.run(R.sequence_scene())
    assert max(int(st["track_count"].max()) for _, st in seq) > 9 and int(seq[-1][1]["next_id"].min()) > 9 + 12


# ---- binding and arguments ----

def test_binding_equals_the_header():
    src = open(os.path.join(ROOT, "include", "bevf.h")).read()
    m = re.search(r"int bevf_track_step_f32\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert m, "bevf_track_step_f32 is not declared in include/bevf.h"
    args = [a.strip() for a in m.group(1).split(",")]
    kinds = [C.c_void_p if "*" in a else {"int": C.c_int, "float": C.c_float}[a.split()[0]] for a in args]
    assert _lib.SIGNATURES["bevf_track_step_f32"] == (C.c_int, kinds) and len(kinds) == 29
    names = [a.replace("*", " ").split()[-1] for a in args]
    assert names[8:15] == [n for n, _, _ in _lib.TRACK_STATE] and names[17:20] == [n for n, _ in _lib.TRACK_OUT]
    assert [(n, str(d).split(".")[-1]) for n, d, _ in _lib.TRACK_STATE] == [(n, np.dtype(d).name) for n, d, _ in R.STATE]


def _args(B=2, N=5, T=8, Cn=3):
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    det = [torch.zeros(B, N, 7), torch.zeros(B, N, 2), torch.zeros(B, N), torch.zeros(B, N, dtype=i64), torch.zeros(B, dtype=i32),
           torch.eye(4, dtype=torch.float64).repeat(B, 1, 1), torch.full((B,), 0.5), torch.ones(Cn)]
    state = {n: torch.zeros((B, T) + tail, dtype=d) for n, d, tail in _lib.TRACK_STATE}
    state.update(track_count=torch.zeros(B, dtype=i32), next_id=torch.zeros(B, dtype=i64))
    out = {n: torch.zeros(B, N, dtype=d) for n, d in _lib.TRACK_OUT}
    out["overflow"] = torch.zeros(B, dtype=i32)
    return det, state, out


def _no_launch(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a launch was attempted")
    monkeypatch.setattr(_lib, "_call", refuse)


def test_track_step_refuses_bad_arguments_before_any_launch(monkeypatch):
    _no_launch(monkeypatch)

    def call(det, state, out, **kw):
        _lib.track_step(*det, state, out, kw.get("max_age", 3), 0.1, True)

    det, state, out = _args()
    with pytest.raises(BevfError, match="CPU tensor"):                # everything right but the device
        call(det, state, out)
    for idx, bad, msg in ((0, torch.zeros(2, 5, 6), r"\(B,N,7\)"), (1, torch.zeros(2, 5, 3), "velocities"), (2, torch.zeros(2, 4), "scores"),
                          (3, torch.zeros(2, 5, dtype=torch.int32), "labels"), (4, torch.zeros(2, dtype=torch.int64), "count"),
                          (5, torch.eye(4).repeat(2, 1, 1), "ego_motion must be a torch.float64"), (5, torch.eye(4, dtype=torch.float64), "ego_motion"),
                          (6, torch.full((2,), 0.5, dtype=torch.float64), "dt"), (7, torch.ones(3, dtype=torch.float64), "max_dist"),
                          (7, torch.ones(0), "max_dist")):
        det, state, out = _args()
        det[idx] = bad
        with pytest.raises(BevfError, match=msg):
            call(det, state, out)
    for key, bad in (("track_box", torch.zeros(2, 8, 6)), ("track_label", torch.zeros(2, 8, dtype=torch.int32)),
                     ("track_age", torch.zeros(2, 7, dtype=torch.int32)), ("next_id", torch.zeros(2, dtype=torch.int32)),
                     ("track_count", torch.zeros(3, dtype=torch.int32))):
        det, state, out = _args()
        state[key] = bad
        with pytest.raises(BevfError, match=key):
            call(det, state, out)
    det, state, out = _args()
    out["det_track_id"] = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(BevfError, match="det_track_id"):
        call(det, state, out)
    det, state, out = _args()
    del out["overflow"]
    with pytest.raises(BevfError, match="overflow"):
        call(det, state, out)
    with pytest.raises(BevfError, match="T=1025 exceeds"):
        call(*_args(T=1025))
    with pytest.raises(BevfError, match="N=4097 exceeds"):
        call(*_args(N=4097))
    with pytest.raises(BevfError, match="max_age"):
        call(*_args(), max_age=-1)


def test_tracker_refuses_bad_construction_and_cpu():
    for kw, msg in ((dict(max_tracks=1025), "max_tracks"), (dict(max_tracks=0), "max_tracks"), (dict(max_dist=[1.0, 2.0]), "2 limits for 3"),
                    (dict(max_dist=-1.0), ">= 0"), (dict(max_age=-1), "max_age"), (dict(device="cpu"), "no CPU fallback")):
        with pytest.raises(BevfError, match=msg):
            tracking.Tracker(2, 3, **{"device": "cpu", **kw})
    with pytest.raises(BevfError, match="positive"):
        tracking.Tracker(0, 3, device="cpu")


def test_tracking_settings_round_trip():
    names = ["car", "truck", "bus", "barrier", "pedestrian"]
    cfg = {"tracking": {"max_age": 5, "birth_score": 0.2, "max_dist": {"car": 3.5, "pedestrian": 0.8}, "class_aware": False}}
    kw = tracking.tracking_settings(cfg, names)
    assert kw == {"num_classes": 5, "max_age": 5, "birth_score": 0.2, "class_aware": False,
                  "max_dist": [3.5, tracking.DEFAULT_MAX_DIST, tracking.DEFAULT_MAX_DIST, tracking.DEFAULT_MAX_DIST, 0.8]}
    again = tracking.tracking_settings({"tracking": {**{k: kw[k] for k in ("max_age", "birth_score", "class_aware")},
                                                     "max_dist": dict(zip(names, kw["max_dist"]))}}, names)
    assert again == kw
    assert tracking.tracking_settings({"tracking": {"max_dist": 2.5}}, names) == {"num_classes": 5, "max_dist": [2.5] * 5}
    assert tracking.tracking_settings({"tracking": None}, names)["max_dist"] == [4.0, 4.0, 5.5, tracking.DEFAULT_MAX_DIST, 1.0]
    assert tracking.CENTERPOINT_MAX_DIST == {"car": 4.0, "truck": 4.0, "bus": 5.5, "trailer": 3.0, "pedestrian": 1.0,
                                             "motorcycle": 13.0, "bicycle": 3.0}
    with pytest.raises(KeyError, match="tracking"):
        tracking.tracking_settings({"inference": {}}, names)
    with pytest.raises(BevfError, match="class_aware must be true or false"):
        tracking.tracking_settings({"tracking": {"class_aware": "false"}}, names)
    with pytest.raises(BevfError, match="tram"):
        tracking.tracking_settings({"tracking": {"max_dist": {"tram": 2.0}}}, names)
