"""The four point-cloud compactions -- `preprocess.filter_pad_lidar`, `augment.transform_filter_pad_lidar`, `sweeps.merge_sweeps` and
`gt_paste.paste` (csrc/point_compact.h) -- on the MI355X against ONE numpy restatement
(`lidar_front_cases.filter_pad_ref`) and therefore against each other, bit for bit (int32 views), each leg run twice.

The shape: N = 65 * 1024 + 1 rows, C = 4: 66 tiles, so the last tile has 65 tiles in front of it and thread 64 -- wave 1 -- carries a
non-zero part of the tile sum.  (More than 1024 tiles, the sum's second trip, is the `big` case of tests/lidar_front_cases.py.)  The
batched legs run three frames with counts (N, 1025, 0).  The legs are set up so that none of them changes a point: identity
matrices (copied, not multiplied), one sweep under the identity with the close-point test off, and no pasted object.

Which side of max_points each frame falls on, from the numpy count (`test_the_frames_fall_on_both_sides_of_max_points`):
  range-filtered legs, survivors (38 676, 607, 0): max_points 40 000 -- fewer, fewer, fewer; 20 000 -- more, fewer, fewer;
  paste (no range test), rows (66 561, 1 025, 0): capacity 40 000 -- more, fewer, fewer; 20 000 -- more, fewer, fewer."""
import functools

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import gt_paste as G
from bevfusion_multimodal_3d_object_detection_amd import preprocess as P
from bevfusion_multimodal_3d_object_detection_amd import sweeps as SW
from bevfusion_multimodal_3d_object_detection_amd.encoders import DEFAULT_PC_RANGE
from tests import lidar_front_cases as LC

pytestmark = pytest.mark.gpu

N_FULL, C = 65 * 1024 + 1, 4
COUNTS = (N_FULL, 1025, 0)
MAX_POINTS = (40000, 20000)
EDGE_N = (1, 1023, 1024, 1025)
LAGS = np.array([[0.25], [0.5], [0.75]], dtype=np.float32)


def _cloud(n, seed):
    """(n, C) fp32: x, y ~ U(-60, 60), z ~ U(-6, 4) against the default range (about 58 % inside), channel 3 = the row number; no
    zero and no NaN; row 0 outside the range, the last row inside."""
    g = np.random.default_rng(seed)
    p = np.empty((n, C), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = g.uniform(-60, 60, n), g.uniform(-60, 60, n), g.uniform(-6, 4, n)
    p[:, 3] = np.arange(n) + 1
    p[:, :3][p[:, :3] == 0] = 0.5
    if n:
        p[0, :3] = (70.0, 1.0, 0.5)
        p[-1, :3] = (1.0, 2.0, 0.5)
    return p


@functools.lru_cache(maxsize=None)
def _frames(n, counts, mps=MAX_POINTS):
    """The batch (len(counts), n, C) and, per max_points, the expected rows and survivor counts of the range-filtered legs; computed
    once per process and never modified."""
    pts = np.stack([_cloud(n, 9000 + 10 * n + b) for b in range(len(counts))])
    want = {mp: [LC.filter_pad_ref(pts[b, :counts[b]], mp) for b in range(len(counts))] for mp in mps}
    pts.setflags(write=False)
    return pts, want


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _same(got, want, what):
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape and np.array_equal(got, want.view(np.int32)), what


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()                      # a copy: the shared frames are read-only


def _twice(fn):
    """fn() -> tensors; run it twice, require equal bits, return the first run's (int32 views of floats, integers as they are)."""
    a, b = ([_bits(t) if t.dtype == torch.float32 else t.cpu().numpy() for t in fn()] for _ in range(2))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "two runs differ"
    return a


# ---- the four legs; each returns (rows (B, mp, C) as int32 bits, counts (B,)) --------------------------------------------------------

def _leg_filter(pts, counts, mp, choice=None):
    rows, cnt = [], []
    for b, n in enumerate(counts):
        o, c = _twice(lambda: P.filter_pad_lidar(_cu(pts[b, :n]), mp, choice=None if choice is None else _cu(choice)))
        rows.append(o), cnt.append(int(c))
    return np.stack(rows), np.asarray(cnt)


def _leg_affine(pts, counts, mp):
    eye = np.tile(np.eye(4)[None], (len(counts), 1, 1))
    return _twice(lambda: A.transform_filter_pad_lidar(_cu(pts), _cu(np.asarray(counts, np.int32)), eye, mp))


def _leg_sweeps(pts, counts, mp):
    """-> rows (B, mp, C + 1), lidar_count (all survivors), sweep_count (B, 1)"""
    B = len(counts)
    T = np.tile(np.eye(4)[None, None], (B, 1, 1, 1))
    def run():
        o = SW.merge_sweeps(_cu(pts[:, None]), _cu(np.asarray(counts, np.int32)[:, None]), _cu(T), _cu(LAGS[:B]), max_points=mp,
                            pc_range=DEFAULT_PC_RANGE, close_radius=0.0)
        return o["lidar_points"], o["lidar_count"], o["sweep_count"]
    return _twice(run)


def _leg_paste(pts, counts, cap):
    B = len(counts)
    bank = G.ObjectBank(torch.ones(3, C, device="cuda"), torch.tensor([0, 3], dtype=torch.int32, device="cuda"),
                        _cu(np.array([[0, 0, 0, 1, 1, 1, 0]], np.float32)), torch.zeros(1, dtype=torch.int64, device="cuda"))
    def run():
        o = G.paste(_cu(pts), _cu(np.asarray(counts, np.int32)), torch.zeros(B, 1, 7, device="cuda"),
                    torch.full((B, 1), -1, dtype=torch.int64, device="cuda"), None, bank, G.PasteParams(np.full((B, 2), -1, np.int32)),
                    capacity=cap)
        return o["lidar_points"], o["lidar_count"], o["accepted"]
    return _twice(run)


def _check_filtered(rows, cnt, want, what):
    for b, (ref, n) in enumerate(want):
        assert int(cnt[b]) == n, (what, b, int(cnt[b]), n)
        _same(rows[b], ref, (what, b))


def _check_sweeps(got, want, counts, mp):
    rows, cnt, sc = got
    assert np.array_equal(sc[:, 0], cnt)
    _check_filtered(rows[:, :, :C], cnt, want, "sweeps")
    for b, (_, n) in enumerate(want):                                # channel C: the sweep's lag on the stored rows, +0 behind them
        lag = np.where(np.arange(mp) < min(n, mp), LAGS[b, 0], np.float32(0)).astype(np.float32)
        _same(rows[b, :, C], lag, ("sweeps lag", b))


def _check_paste(got, pts, counts, cap):
    rows, cnt, acc = got
    assert not acc.any()
    for b, n in enumerate(counts):                                   # no range test: the frame's first rows, +0 behind them
        ref = np.zeros((cap, C), np.float32)
        ref[:min(n, cap)] = pts[b, :min(n, cap)]
        assert int(cnt[b]) == min(n, cap), ("paste", b)
        _same(rows[b], ref, ("paste", b))


# ---- the 66-tile batch ---------------------------------------------------------------------------------------------------------------

def test_the_frames_fall_on_both_sides_of_max_points():
    _, want = _frames(N_FULL, COUNTS)
    n = [w[1] for w in want[40000]]
    print("survivors per frame:", n)
    assert n[0] < 40000 and n[0] > 20000 and 0 < n[1] < 20000 and n[2] == 0         # fewer than 40 000, more than 20 000
    assert COUNTS[0] > 40000 and COUNTS[1] < 20000                                   # paste: more than either capacity, fewer


@pytest.mark.parametrize("mp", MAX_POINTS)
def test_filter_pad_lidar(gpu, mp):
    pts, want = _frames(N_FULL, COUNTS)
    _check_filtered(*_leg_filter(pts, COUNTS, mp), want[mp], "filter")


def test_filter_pad_lidar_with_a_choice(gpu):
    """20 000 < survivors of frame 0: the choice gathers; frames 1 and 2 have fewer and ignore it."""
    pts, _ = _frames(N_FULL, COUNTS)
    mp = 20000
    choice = (np.arange(mp, dtype=np.int64) * 7919 + 11) % 30000
    rows, cnt = _leg_filter(pts, COUNTS, mp, choice)
    _check_filtered(rows, cnt, [LC.filter_pad_ref(pts[b, :n], mp, choice=choice) for b, n in enumerate(COUNTS)], "choice")


@pytest.mark.parametrize("mp", MAX_POINTS)
def test_transform_filter_pad_lidar_under_the_identity(gpu, mp):
    pts, want = _frames(N_FULL, COUNTS)
    _check_filtered(*_leg_affine(pts, COUNTS, mp), want[mp], "affine")


@pytest.mark.parametrize("mp", MAX_POINTS)
def test_merge_of_one_sweep_under_the_identity(gpu, mp):
    pts, want = _frames(N_FULL, COUNTS)
    _check_sweeps(_leg_sweeps(pts, COUNTS, mp), want[mp], COUNTS, mp)


@pytest.mark.parametrize("cap", MAX_POINTS)
def test_paste_of_no_object(gpu, cap):
    pts, _ = _frames(N_FULL, COUNTS)
    _check_paste(_leg_paste(pts, COUNTS, cap), pts, COUNTS, cap)


# ---- tile edges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", EDGE_N)
def test_tile_edges_affine_and_paste(gpu, N):
    counts, mps = (N, N // 2), (max(N // 4, 1), N + 7)                 # fewer rows than either frame keeps, and more
    pts, want = _frames(N, counts, mps)
    for mp in mps:
        _check_filtered(*_leg_affine(pts, counts, mp), want[mp], ("affine", N))
        _check_paste(_leg_paste(pts, counts, mp), pts, counts, mp)


def test_no_rows(gpu):
    counts = (0, 0)
    pts, want = _frames(0, counts)
    mp = MAX_POINTS[1]
    _check_filtered(*_leg_filter(pts, counts, mp), want[mp], "filter")
    _check_filtered(*_leg_affine(pts, counts, mp), want[mp], "affine")
    _check_sweeps(_leg_sweeps(pts, counts, mp), want[mp], counts, mp)
    _check_paste(_leg_paste(pts, counts, 5), pts, counts, 5)
