"""Multi-sweep LiDAR accumulation (csrc/sweeps.hip) on the MI355X against the numpy restatement of
tests/sweeps_ref.py.  Every comparison is bit-exact: outputs are compared as unsigned views, so -0.0 and NaN payloads cannot hide.  The
scenes' conditions are checked in tests/test_sweeps_host.py."""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import centernet_target, fusion, sweeps as SW, synth
from tests import sweeps_ref as R

pytestmark = pytest.mark.gpu


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _merge(pts, counts, T, lag, max_points, close_radius=1.0):
    o = SW.merge_sweeps(_cu(pts), _cu(counts.astype(np.int32)), _cu(T), _cu(lag), max_points=max_points, pc_range=R.RANGE,
                        close_radius=close_radius)
    assert o["lidar_points"].dtype == torch.float32 and o["lidar_count"].dtype == torch.int32 and o["sweep_count"].dtype == torch.int32
    return o["lidar_points"].cpu().numpy(), o["lidar_count"].cpu().numpy(), o["sweep_count"].cpu().numpy()


def _assert_equal(got, want, what=""):
    out, count, sc = got
    rout, rcount, rsc = want
    assert out.shape == rout.shape and np.array_equal(count, rcount) and np.array_equal(sc, rsc), what
    assert np.array_equal(out.view(np.uint32), rout.view(np.uint32)), what


@pytest.fixture(scope="module")
def edge():
    pts, counts, T, lag = R.edge_scene()
    return pts, counts, T, lag, R.merge_ref(pts, counts, T, lag, R.EDGE["max_points"], R.EDGE["close_radius"])


# ---- 1. the edge batch ----------------------------------------------------------------------------------------------------------------

def test_edge_batch(gpu, edge):
    pts, counts, T, lag, want = edge
    got = _merge(pts, counts, T, lag, R.EDGE["max_points"], R.EDGE["close_radius"])
    _assert_equal(got, want)
    out, count, sc = got
    mp = R.EDGE["max_points"]
    assert sc[0, 0] < mp < sc[0, 0] + sc[0, 1]                                      # frame 0: the cut inside sweep 1
    assert tuple(sc[1][:2]) == (0, 1) and out[1, 0, 4] == lag[1, 1]                 # frame 1: empty key sweep, the one point survives
    assert count[2] == 0 and not out[2].view(np.uint32).any()                       # frame 2: all zeros
    assert count[3] == mp + sc[3, 2] and sc[3, 2] > 0                               # frame 3: the cut exactly on a sweep boundary


# ---- 2. tile and shape edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [3, 5])
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025])
def test_tile_and_shape_edges(gpu, N, C):
    pts, counts, T, lag = R.small_scene(1, 1, N, C, seed=100 + N + C, counts=[[N]])
    if N == 1:
        pts[0, 0, 0, :3] = R.INTERIOR                                               # the one row survives
    for mp in (1, N, N + 7):
        want = R.merge_ref(pts, counts, T, lag, mp)
        assert want[1][0] > 0
        _assert_equal(_merge(pts, counts, T, lag, mp), want, (N, C, mp))


def test_no_rows_is_a_legal_call(gpu):
    pts, counts = np.zeros((1, 2, 0, 4), dtype=np.float32), np.zeros((1, 2), dtype=np.int32)
    out, count, sc = _merge(pts, counts, R.sweep_matrices(1, 2), R.lags(1, 2), 5)
    assert out.shape == (1, 5, 5) and not out.view(np.uint32).any() and not count.any() and not sc.any()


def test_counts_are_clamped_to_the_sweep(gpu):
    pts, _, T, lag = R.small_scene(2, 2, 300, 4, seed=8)
    counts = np.array([[-5, 300], [100000, 7]], dtype=np.int32)
    _assert_equal(_merge(pts, counts, T, lag, 400), R.merge_ref(pts, counts, T, lag, 400))


def test_rows_off_a_16_byte_boundary_take_the_scalar_loads(gpu, edge):
    """C = 4 rows on a 16-byte boundary are read as one 16-byte load; the same rows 4 bytes further on are not, and give the same bits."""
    pts, counts, T, lag, want = edge
    buf = torch.empty(pts.size + 1, device=gpu)
    shifted = buf[1:].view(*pts.shape)
    shifted.copy_(_cu(pts))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    o = SW.merge_sweeps(shifted, _cu(counts), _cu(T), _cu(lag), max_points=R.EDGE["max_points"], pc_range=R.RANGE)
    _assert_equal((o["lidar_points"].cpu().numpy(), o["lidar_count"].cpu().numpy(), o["sweep_count"].cpu().numpy()), want)


# ---- 3. special rows / 4. close_radius = 0 --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("close_radius", [1.0, 0.0])
def test_special_rows_under_the_identity(gpu, close_radius):
    pts, names, keep = R.special_rows()
    T, lag = np.eye(4)[None, None].copy(), np.array([[0.25]], dtype=np.float32)
    counts = np.array([[7]], dtype=np.int32)
    want = R.merge_ref(pts, counts, T, lag, 7, close_radius)
    got = _merge(pts, counts, T, lag, 7, close_radius)
    _assert_equal(got, want)
    if close_radius == 0.0:
        keep = keep.copy()
        keep[names.index("inside the close square")] = True                         # no row is removed for closeness
    assert int(got[1][0]) == int(keep.sum())
    assert np.array_equal(got[0][0, :keep.sum(), :4].view(np.uint32), pts[0, 0, keep].view(np.uint32))   # the kept rows keep their bits


def test_close_radius_zero_removes_nothing_for_closeness(gpu):
    pts, counts, T, lag = R.small_scene(2, 3, 500, 4, seed=6, close_radius=0.0)
    pts[:, :, :200, :2] *= np.float32(0.02)                                         # many rows inside the 1 m square
    pts = R.keep_margin(pts, T, 0.0)
    want0, want1 = R.merge_ref(pts, counts, T, lag, 1500, 0.0), R.merge_ref(pts, counts, T, lag, 1500, 1.0)
    assert (want0[1] > want1[1]).all()
    _assert_equal(_merge(pts, counts, T, lag, 1500, 0.0), want0)
    _assert_equal(_merge(pts, counts, T, lag, 1500, -1.0), want0)


# ---- 5. time channel ------------------------------------------------------------------------------------------------------------------

def test_time_channel_and_copied_channels(gpu):
    B, S, N, C = 2, 3, 700, 5
    pts, counts, T, lag = R.small_scene(B, S, N, C, seed=3)
    out, count, sc = _merge(pts, counts, T, lag, S * N)
    plain = R.merge_plain(pts, counts, T, lag, 1.0)
    for b in range(B):
        src = plain[b][1]
        k = int(count[b])
        assert k == len(src) and np.array_equal(sc[b], np.bincount(src[:, 0], minlength=S))
        assert np.array_equal(out[b, :k, C].view(np.uint32), lag[b, src[:, 0]].view(np.uint32))          # the source sweep's lag
        assert np.array_equal(out[b, :k, 3:C].view(np.uint32), pts[b, src[:, 0], src[:, 1], 3:].view(np.uint32))
        assert len(set(lag[b].tolist())) == S


# ---- 6. pose chain --------------------------------------------------------------------------------------------------------------------

def test_pose_chain_is_bit_equal_and_merges_alike(gpu):
    kl, ke, sl, se = R.pose_scene()
    want = R.pose_chain_ref(kl, ke, sl, se)
    got = SW.sweep_transforms(_cu(kl), _cu(ke), _cu(sl), _cu(se))
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert np.array_equal(want[:, 0], np.broadcast_to(np.eye(4), want[:, 0].shape))  # the key sweep itself: the exact identity
    B, S = sl.shape[:2]
    pts, counts, _, lag = R.small_scene(B, S, 400, 4, seed=9)
    pts = R.keep_margin(pts, want, 1.0)
    o = SW.merge_sweeps(_cu(pts), _cu(counts), got, _cu(lag), max_points=S * 400, pc_range=R.RANGE)
    _assert_equal((o["lidar_points"].cpu().numpy(), o["lidar_count"].cpu().numpy(), o["sweep_count"].cpu().numpy()),
                  R.merge_ref(pts, counts, want, lag, S * 400))


# ---- 7. determinism / 8. graph capture ------------------------------------------------------------------------------------------------

def test_two_merges_are_bit_identical(gpu, edge):
    pts, counts, T, lag, _ = edge
    a, b = (_merge(pts, counts, T, lag, R.EDGE["max_points"]) for _ in range(2))
    _assert_equal(a, b)


def test_merge_refuses_wrong_shapes_and_dtypes(gpu):
    m = SW.SweepMerger(1, 2, 8, 4, max_points=8, pc_range=R.RANGE)
    pts, cnt = torch.zeros(1, 2, 8, 4, device=gpu), torch.zeros(1, 2, dtype=torch.int32, device=gpu)
    T, lag = torch.eye(4, dtype=torch.float64, device=gpu).expand(1, 2, 4, 4).contiguous(), torch.zeros(1, 2, device=gpu)
    for bad in ((pts[:, :, :7], cnt, T, lag), (pts, cnt.long(), T, lag), (pts, cnt, T.float(), lag), (pts, cnt, T, lag.double()),
                (pts, cnt, T, lag[:, :1])):
        with pytest.raises(L.BevfError, match="expected"):
            m.merge(*bad)
    with pytest.raises(L.BevfError, match="no CPU fallback"):
        m.merge(pts.cpu(), cnt, T, lag)
    assert int(m.merge(pts, cnt, T, lag)["lidar_count"][0]) == 0


def test_graph_capture_replays_on_new_data(gpu):
    B, S, N, C, mp = 2, 3, 1100, 4, 1000
    a = R.small_scene(B, S, N, C, seed=41)
    b = R.small_scene(B, S, N, C, seed=42)
    static = [_cu(a[0]), _cu(a[1]), _cu(a[2]), _cu(a[3])]
    merger = SW.SweepMerger(B, S, N, C, max_points=mp, pc_range=R.RANGE)
    merger.merge(*static)                                                           # once eagerly before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = merger.merge(*static)
    first = o["lidar_points"].clone()
    for s, t in zip(static, b):
        s.copy_(_cu(t))
    graph.replay()
    torch.cuda.synchronize()
    want = _merge(*b, mp)
    _assert_equal((o["lidar_points"].cpu().numpy(), o["lidar_count"].cpu().numpy(), o["sweep_count"].cpu().numpy()), want)
    _assert_equal(want, R.merge_ref(*b, mp))
    assert o["lidar_points"].data_ptr() == merger.out.data_ptr() and not torch.equal(first, o["lidar_points"])


# ---- 9. end to end --------------------------------------------------------------------------------------------------------------------

def test_merged_cloud_trains_a_five_channel_pillar_detector(gpu):
    B, S, N, C, mp = 2, 3, 600, 4, 1024
    pts, counts, T, lag = R.small_scene(B, S, N, C, seed=17, counts=np.full((B, S), N))
    o = SW.merge_sweeps(_cu(pts), _cu(counts), _cu(T), _cu(lag), max_points=mp, pc_range=R.RANGE)
    cloud, n_in = o["lidar_points"], o["lidar_count"].clamp(max=mp)
    assert tuple(cloud.shape) == (B, mp, C + 1) and int(n_in.min()) > 500
    cfg = {"model": {"modality_config": "camera+lidar", "camera_encoder": {"pretrained": False},
                     "lidar_encoder": {"type": "PointPillars", "input_channels": 5}},
           "dataset": {"bev_h": 16, "bev_w": 16}}
    model = fusion.create_detector(config=cfg)
    assert type(model.lidar_encoder).__name__ == "PillarLiDAREncoder" and model.lidar_encoder.input_channels == 5
    synth.fill_state_dict_(model, 11)
    model = model.cuda().train()
    imgs, _, _ = synth.frame_inputs(B, 2, 64, 96, 0, 4, 5, 25, 7, seed=5)
    boxes, labels = synth.gt_boxes(B, 12, seed=4)
    boxes, labels = boxes.cuda(), labels.cuda()

    def step(lidar, gt_boxes, gt_labels):
        model.zero_grad(set_to_none=True)
        pred = model(imgs.cuda(), lidar)
        tgt = centernet_target.prepare_centernet_targets({"gt_boxes": gt_boxes, "gt_labels": gt_labels}, "cuda", bev_size=(16, 16))
        loss = centernet_target.CenterNetLoss()(pred, tgt)["total_loss"]
        loss.backward()
        grads = [p.grad for p in model.lidar_encoder.pfn.parameters()]
        assert torch.isfinite(loss) and all(g is not None and torch.isfinite(g).all() for g in grads)
        assert sum(float(g.abs().sum()) for g in grads) > 0
        return float(loss.detach())

    plain = step(cloud, boxes, labels)
    st = A.AugmentSettings(flip=True, scale=(0.95, 1.05), rotation=(-20.0, 20.0), translation=(0.5, 0.5, 0.2))
    p = A.sample(st, B, 2, (64, 96), (64, 96), np.random.default_rng(3))
    assert not np.array_equal(p.bev_aug, np.broadcast_to(np.eye(4), p.bev_aug.shape))                    # a non-identity world transform
    aug = A.augment_batch(None, cloud, n_in, None, boxes, labels, None, p, st, max_points=mp)
    assert tuple(aug["lidar_points"].shape) == (B, mp, C + 1) and not torch.equal(aug["lidar_points"], cloud)
    k = int(aug["lidar_count"][0])
    assert k > 0 and set(aug["lidar_points"][0, :k, C].unique().tolist()) <= set(lag[0].tolist())        # the time channel passes through
    augmented = step(aug["lidar_points"], aug["gt_boxes"], aug["gt_labels"])
    assert plain != augmented
