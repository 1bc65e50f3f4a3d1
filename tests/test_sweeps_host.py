"""CPU-only checks of the multi-sweep LiDAR accumulation (sweeps.py): the numpy restatement of tests/sweeps_ref.py
against an independent plain formulation, the conditions the scenes of tests/test_gpu_sweeps.py are built to meet, the host helpers, and
the wrappers' buffer checks."""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib, sweeps as SW
from tests import sweeps_ref as R


# ---- restatement against plain geometry ---------------------------------------------------------------------------------------------

_SCENES = {"edge": lambda: (*R.edge_scene(), R.EDGE["close_radius"]),
           "small": lambda: (*R.small_scene(2, 3, 700, 5, seed=3), 1.0),
           "no close test": lambda: (*R.small_scene(2, 2, 300, 3, seed=4, close_radius=0.0), 0.0)}


@pytest.mark.parametrize("name", list(_SCENES))
def test_restatement_agrees_with_plain_geometry(name):
    """Identical survivor sets, positions within 1e-9 m before the fp32 rounding; the scenes keep every point (valid or not) at least
    1e-3 m from a range face and from the close-radius square, which is asserted here, so nothing is excluded."""
    pts, counts, T, lag, r = _SCENES[name]()
    B, S, N, C = pts.shape
    for b in range(B):
        for s in range(S):
            assert R.boundary_distance(T[b, s], pts[b, s], r).min() >= R.MARGIN, (name, b, s)
    out, count, sweep_count = R.merge_ref(pts, counts, T, lag, max_points=S * N, close_radius=r)
    plain = R.merge_plain(pts, counts, T, lag, r)
    for b in range(B):
        pos, src = plain[b]
        assert int(count[b]) == len(pos) and np.array_equal(sweep_count[b], np.bincount(src[:, 0], minlength=S))
        got = np.concatenate([R.transform_ref(T[b, s], pts[b, s]) for s in range(S)]).reshape(S, N, 3)[src[:, 0], src[:, 1]]
        assert np.abs(got - pos).max(initial=0.0) <= 1e-9
        k = len(pos)
        assert np.array_equal(out[b, :k, :3], got.astype(np.float32))
        assert np.array_equal(out[b, :k, 3:C].view(np.uint32), pts[b, src[:, 0], src[:, 1], 3:].view(np.uint32))
        assert np.array_equal(out[b, :k, C], lag[b, src[:, 0]]) and not out[b, k:].any()


def test_edge_scene_is_what_the_gpu_test_says_it_is():
    pts, counts, T, lag = R.edge_scene()
    mp = R.EDGE["max_points"]
    out, count, sc = R.merge_ref(pts, counts, T, lag, mp, R.EDGE["close_radius"])
    assert sc[0, 0] < mp < sc[0, 0] + sc[0, 1] and sc[0].min() > 700                # frame 0: mostly surviving, the cut inside sweep 1
    assert tuple(sc[1][:2]) == (0, 1) and 0 < sc[1, 2] < 1024                       # frame 1: empty key sweep, the single point survives
    assert count[2] == 0 and not out[2].any()                                       # frame 2: nothing
    assert tuple(sc[3][:2]) == (750, 750) and sc[3, 2] > 0 and count[3] == mp + sc[3, 2]   # frame 3: the cut on a sweep boundary
    assert out[3, mp - 1, 4] == lag[3, 1] and out[0, mp - 1, 4] == lag[0, 1]
    full = R.merge_ref(pts, np.full_like(counts, R.EDGE["N"]), T, lag, mp, R.EDGE["close_radius"])[1]
    assert (full[1:] > count[1:]).all() and full[0] == count[0]                     # the rows past the counts would survive: in-range garbage


def test_special_rows_under_the_identity():
    pts, names, keep = R.special_rows()
    T = np.eye(4)[None, None]
    out, count, _ = R.merge_ref(pts, np.array([[7]]), T, np.array([[0.25]], dtype=np.float32), 7, 1.0)
    assert int(count[0]) == int(keep.sum()) == 3
    assert np.array_equal(out[0, :3, :4].view(np.uint32), pts[0, 0, keep].view(np.uint32))
    out0, count0, _ = R.merge_ref(pts, np.array([[7]]), T, np.array([[0.25]], dtype=np.float32), 7, 0.0)
    assert int(count0[0]) == 4 and np.array_equal(out0[0, 2, :3], pts[0, 0, 5, :3])              # close_radius 0 keeps the close row


# ---- pose chain -----------------------------------------------------------------------------------------------------------------------

def test_pose_chain_restatement_agrees_with_composition():
    kl, ke, sl, se = R.pose_scene()
    assert np.abs(ke[:, :2, 3]).min() > 500 and np.abs(se[..., :2, 3]).min() > 500  # global translations of order 1e3 m
    T, P = R.pose_chain_ref(kl, ke, sl, se), R.pose_chain_plain(kl, ke, sl, se)
    assert np.abs(T[..., :3, 3] - P[..., :3, 3]).max() <= 1e-9
    assert np.abs(T[..., :3, :3] - P[..., :3, :3]).max() <= 1e-12
    assert (T[..., 3, :] == (0, 0, 0, 1)).all()
    assert np.abs(T[:, 1:, :3, 3]).max() > 0.4                                       # the older sweeps did move
    same = R.pose_chain_ref(kl, ke, np.repeat(kl[:, None], 2, 1), np.repeat(ke[:, None], 2, 1))
    assert np.array_equal(same[..., :3, :3], np.broadcast_to(np.eye(3), same[..., :3, :3].shape))
    assert np.abs(same[..., :3, 3]).max() <= 1e-12


# ---- helpers --------------------------------------------------------------------------------------------------------------------------

def test_time_lags():
    key = np.array([1_533_151_603_547_590, 1_533_151_604_048_025], dtype=np.int64)
    sweep = np.stack([key, key - 50_012, key - 499_977], 1)
    lag = SW.time_lags(key, sweep)
    assert lag.dtype == torch.float32 and tuple(lag.shape) == (2, 3) and not lag.is_cuda
    want = np.array([[0.0, 0.050012, 0.499977]] * 2)
    assert np.array_equal(lag.numpy(), want.astype(np.float32))                     # stamps of order 1e15 us do not cost a digit
    assert torch.equal(SW.time_lags(torch.from_numpy(key), torch.from_numpy(sweep)), lag)
    with pytest.raises(_lib.BevfError, match="integer"):
        SW.time_lags(key.astype(np.float64), sweep)
    with pytest.raises(_lib.BevfError, match="stamps"):
        SW.time_lags(key, sweep[:1])


def test_pack_sweeps():
    rs = np.random.RandomState(0)
    a, b, c = (rs.rand(n, 4).astype(np.float32) for n in (5, 3, 7))
    pts, cnt = SW.pack_sweeps([[a, np.zeros((0, 4), np.float32)], [torch.from_numpy(b), c]], "cpu")
    assert tuple(pts.shape) == (2, 2, 7, 4) and pts.dtype == torch.float32 and cnt.dtype == torch.int32
    assert cnt.tolist() == [[5, 0], [3, 7]]
    assert np.array_equal(pts[0, 0, :5].numpy(), a) and not pts[0, 0, 5:].any() and not pts[0, 1].any()
    assert np.array_equal(pts[1, 0, :3].numpy(), b) and np.array_equal(pts[1, 1].numpy(), c)
    pts, cnt = SW.pack_sweeps([[a, None]], "cpu", n=16)
    assert tuple(pts.shape) == (1, 2, 16, 4) and cnt.tolist() == [[5, 0]]
    with pytest.raises(_lib.BevfError, match="ragged"):
        SW.pack_sweeps([[a, rs.rand(4, 5).astype(np.float32)]], "cpu")
    with pytest.raises(_lib.BevfError, match="holds 5"):
        SW.pack_sweeps([[a, None]], "cpu", n=4)
    with pytest.raises(_lib.BevfError, match="same number of sweeps"):
        SW.pack_sweeps([[a, b], [c]], "cpu")


def test_package_exports_the_module():
    import bevfusion_multimodal_3d_object_detection_amd as pkg
    assert pkg.sweeps is SW and pkg.merge_sweeps is SW.merge_sweeps and pkg.SweepMerger is SW.SweepMerger
    assert set(SW.__all__) <= set(pkg.__all__)


# ---- wrappers ---------------------------------------------------------------------------------------------------------------------------

class _Recorder:
    """Stands in for the loaded library: size queries answer from the real one, every other entry point is recorded."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith(("_bytes", "_floats")) or name == "bevf_last_error":
            return getattr(self.real, name)
        return lambda *args: self.calls.append(name) or 0


def _case(name, short):
    """(wrapper, args) with CPU buffers of exactly the sizes the kernel needs; `short` names the one buffer that is an element short."""
    def z(key, n, dt=torch.float32):
        return torch.zeros(n - (key == short), dtype=dt)
    I32, F64 = torch.int32, torch.float64
    L = _lib
    B, S, N, C, mp = 2, 3, 1030, 4, 9
    wi = -(-L.sweeps_merge_work_bytes(B, S, N) // 4)
    if name == "sweeps_merge":
        return L.sweeps_merge, (z("points", B * S * N * C), z("counts", B * S, I32), z("sweep_to_key", B * S * 16, F64), z("time_lag", B * S),
                                z("out", B * mp * (C + 1)), z("count", B, I32), z("sweep_count", B * S, I32), z("work", wi, I32), B, S, N, C,
                                mp, 1.0, R.RANGE)
    return L.sweep_pose_chain, (z("key_lidar2ego", B * 16, F64), z("key_ego2global", B * 16, F64), z("sweep_lidar2ego", B * S * 16, F64),
                                z("sweep_ego2global", B * S * 16, F64), z("sweep_to_key", B * S * 16, F64), B, S)


_BUFFERS = [("sweeps_merge", k) for k in ("points", "counts", "sweep_to_key", "time_lag", "out", "count", "sweep_count", "work")] + \
           [("sweep_pose_chain", k) for k in ("key_lidar2ego", "key_ego2global", "sweep_lidar2ego", "sweep_ego2global", "sweep_to_key")]


@pytest.mark.parametrize("name,short", _BUFFERS)
def test_sweeps_wrappers_check_before_launching(name, short, monkeypatch):
    """A buffer one element short raises before anything is launched; right-sized CPU tensors are refused, not computed."""
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    fn, args = _case(name, short)
    with pytest.raises(_lib.BevfError, match=f"{short} holds .* needs"):
        fn(*args)
    fn, args = _case(name, None)
    with pytest.raises(_lib.BevfError, match="no CPU fallback"):
        fn(*args)
    assert rec.calls == []


def test_work_bytes_is_two_ints_per_tile():
    assert _lib.sweeps_merge_work_bytes(2, 3, 1030) == 4 * 2 * (2 * 3 * 2 + 1)
    assert _lib.sweeps_merge_work_bytes(1, 2, 0) == 4 and _lib.sweeps_merge_work_bytes(1, 1, 1024) == 12


def test_public_entry_points_refuse_cpu_tensors_and_bad_shapes(monkeypatch):
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    pts, cnt = torch.zeros(1, 2, 8, 4), torch.zeros(1, 2, dtype=torch.int32)
    T, lag = torch.eye(4, dtype=torch.float64).expand(1, 2, 4, 4).contiguous(), torch.zeros(1, 2)
    with pytest.raises(_lib.BevfError, match="no CPU fallback"):
        SW.merge_sweeps(pts, cnt, T, lag, max_points=8)
    with pytest.raises(_lib.BevfError, match="no CPU fallback"):
        SW.SweepMerger(1, 2, 8, 4, max_points=8, device="cpu")
    with pytest.raises(_lib.BevfError, match="no CPU fallback"):
        SW.sweep_transforms(T[:, 0], T[:, 0], T, T)
    with pytest.raises(_lib.BevfError, match="expected torch.float64"):
        SW.sweep_transforms(T[:, 0], T[:, 0].float(), T, T)
    with pytest.raises(_lib.BevfError, match="expected torch.float64"):
        SW.sweep_transforms(T[:, 0], T[:, 0], T, T[:, :1])
    with pytest.raises(_lib.BevfError, match="3 <= C <= 8"):
        SW.SweepMerger(1, 2, 8, 9)
    with pytest.raises(_lib.BevfError, match="a \\(B, S, N, C\\) tensor"):
        SW.merge_sweeps(pts[0], cnt, T, lag)
    assert rec.calls == []
