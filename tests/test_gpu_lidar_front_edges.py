"""The LiDAR front end at its edges: `bevf_voxelize_f32`, `bevf_scatter_voxels_f32`, `bevf_vfe_smallk_max_f32` and
`bevf_lidar_filter_pad_f32` on the cases of tests/lidar_front_cases.py, whose properties tests/test_lidar_front_host.py asserts.

Comparisons:
  * voxeliser, scatter, filter: BIT FOR BIT against the oracle (`oracle/ref_voxelize.py`; for the filter the numpy restatement
    `filter_pad_ref`, pinned to `oracle/ref_preprocess.py` on the host) -- integers with torch.equal, floats through an int32 view;
  * VFE: (a) to float64 at every element, |got - ref| <= k 2^-24 bound with k = K + 2 and `bound` the same expression on absolute
    values (the max over a voxel's points takes the max of the bounds) -- the rule of tests/test_gpu_glue.py; (b) bit for bit to
    `pointwise_smallk` + `group_max` wherever Cout % 4 == 0 (the two kernels need that).

k = K + 2: the pre-activation is a chain of K fmas (one rounding each, each relative to a partial sum that `bound` dominates: K u
bound to first order), the scale / shift fma adds one rounding of |acc scale| + |shift| <= bound, and the carried error is scaled by
|scale|, which `bound` already contains: (K + 1) u bound (1 + O(K u)).  The last unit covers the second-order terms.  ReLU and max are
exact and 1-Lipschitz.

Every output lives in a buffer longer than needed, pre-filled with a sentinel; the expectation is built for the WHOLE buffer (the
sentinel wherever the kernel has no business writing: past the end, and for the voxeliser every row >= num_voxels and every entry >=
num_points, which the production `out=` form never zero-fills), so one comparison covers the values and the untouched rest.  The
kernels are called through `_lib` so that flat, over-long, pre-filled buffers can be passed.

Worst |got - ref| / tolerance observed on MI355X is listed in DESIGN.md 4.2.
"""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import encoders, synth
from oracle import ref_voxelize
from tests import lidar_front_cases as LC

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
PAD = 64
I32, I64, F32, F64 = torch.int32, torch.int64, torch.float32, torch.float64
SENT = {F32: float("nan"), I32: -77777, I64: -7777777777}


def sentinel(n, dtype, dev):
    return torch.full((n + PAD,), SENT[dtype], dtype=dtype, device=dev)


def same(a, b):
    """Bit for bit, floats through an int32 view."""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(I32), b.view(I32)) if a.dtype == F32 else torch.equal(a, b)


# ---- voxeliser ---------------------------------------------------------------------------------------------------------------------

def vox_buffers(gpu, B, N, C, P, Nv):
    return (sentinel(B * Nv * P * C, F32, gpu), sentinel(B * Nv * 3, I64, gpu), sentinel(B * Nv, I32, gpu), sentinel(B, I32, gpu),
            torch.empty(L.voxelize_work_bytes(B, N) + PAD, dtype=torch.uint8, device=gpu))


def vox_expected(before, oracle, B, C, P, Nv):
    """The whole buffers after a call: `before` with exactly the elements the kernel owns replaced by the oracle's."""
    f, c, n, v = oracle
    ef, ec, en, ev = (t.cpu().clone() for t in before)
    live = torch.arange(Nv)[None] < v[:, None]                                       # (B, Nv)
    rows = (torch.arange(P)[None, None] < n[..., None]) & live[..., None]            # (B, Nv, P)
    ef[:B * Nv * P * C].view(B, Nv, P, C)[rows] = f[rows]
    ec[:B * Nv * 3].view(B, Nv, 3)[live] = c[live]
    en[:B * Nv].view(B, Nv)[live] = n[live]
    ev[:B] = v
    return ef, ec, en, ev


def run_voxel_case(gpu, name, bufs=None):
    case = LC.voxel_case(name)
    B, N, C = case["pts"].shape
    P, Nv = case["P"], case["Nv"]
    bufs = vox_buffers(gpu, B, N, C, P, Nv) if bufs is None else bufs
    before = [t.clone() for t in bufs[:4]]
    L.voxelize(case["pts"].to(gpu), case["pc_range"], case["vs"], P, Nv, out=bufs)
    torch.cuda.synchronize()
    want = vox_expected(before, LC.voxel_oracle(name), B, C, P, Nv)
    for got, ref, what in zip(bufs[:4], want, ("features", "coords", "num_points", "num_voxels")):
        assert same(got, ref), (name, what)
    return bufs


@pytest.mark.parametrize("name", [n for n in LC.VOXEL_CASES if not n.startswith("reuse")])
def test_voxelize_case(gpu, name):
    run_voxel_case(gpu, name)


def test_voxelize_out_reuse(gpu):
    """The production form: grow-only buffers that still hold the previous batch.  After the large scene everything the kernel does
    not own is still the sentinel; after the smaller scene (other B, N, P, Nv: another layout in the same memory) everything it
    does not own is still what the first call left."""
    bufs = run_voxel_case(gpu, "reuse_large")
    assert int(torch.isnan(bufs[0]).sum()) > PAD                                     # sentinel left inside the used part too
    run_voxel_case(gpu, "reuse_small", bufs)


def test_voxelize_fresh_form_is_zero_padded(gpu):
    c = LC.voxel_case("seam")
    got = encoders.voxelize(c["pts"].to(gpu), c["pc_range"], c["vs"], c["P"], c["Nv"])
    for g, r in zip(got, LC.voxel_oracle("seam")):
        assert same(g, r)


def _tiny_points(gpu, n=4, c=4):
    return torch.full((1, n, c), 0.5, device=gpu)


def test_voxelize_refusals(gpu):
    rng, vs = LC.unit_range(65536, 65536)
    with pytest.raises(L.BevfError, match="bad grid"):                               # 2^32 cells: past the 32-bit cell id
        encoders.voxelize(_tiny_points(gpu), rng, vs, 2, 4)
    rng, vs = LC.unit_range(*LC.LONG_GRID)
    with pytest.raises(L.BevfError, match="N < 2\\^20"):
        encoders.voxelize(torch.zeros(1, 1 << 20, 3, device=gpu), rng, vs, 2, 4)
    for rng, vs, axis in LC.REFUSED_RATIOS:                                          # 2.5 and 49.4 voxels along one axis
        with pytest.raises(L.BevfError, match=f"axis {axis}"):
            encoders.voxelize(_tiny_points(gpu), rng, vs, 2, 4)


@pytest.mark.parametrize("bev", LC.ACCEPTED_BEV)
def test_engine_grids_are_accepted(gpu, bev):
    """The pillar (bev x bev x 1) and sparse (4 bev x 4 bev x 40) grids: voxel = range / cells in fp32, a whole ratio to a few ulps."""
    _, pts, _ = synth.frame_inputs(1, 0, 0, 0, 600, 4, seed=800 + bev)
    for rng, vs, _ in LC.engine_grids(bev):
        got = encoders.voxelize(pts.to(gpu), rng, vs, 3, 700)
        for g, r in zip(got, ref_voxelize.hard_voxelize(pts, rng, vs, 3, 700)):
            assert same(g, r)


# ---- scatter -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LC.SCATTER_CASES))
def test_scatter_case(gpu, name):
    s = LC.scatter_case(name)
    B, Nv, C = s["feats"].shape
    D, H, W = s["grid"]
    n = B * C * D * H * W
    out, owner = sentinel(n, F32, gpu), sentinel(B * D * H * W, I32, gpu)
    nv = None if s["nv"] is None else s["nv"].to(gpu)
    feats, coords = s["feats"].to(gpu), s["coords"].to(gpu)          # named: the raw pointers below keep nothing alive
    L._call("bevf_scatter_voxels_f32", L._pc(feats), L._pc(coords, I64), L._pc(nv, I32), L._p(owner, I32), L._p(out), B, Nv, C, D, H, W)
    torch.cuda.synchronize()
    ref = ref_voxelize.dense_scatter(s["feats"], s["coords"], s["grid"], s["nv"])
    assert same(out[:n].view(B, C, D, H, W), ref), name
    assert same(out[n:], sentinel(0, F32, gpu)) and same(owner[B * D * H * W:], sentinel(0, I32, gpu))
    assert same(encoders.scatter_voxels(s["feats"].to(gpu), s["coords"].to(gpu), s["grid"], nv), ref)


# ---- VFE ---------------------------------------------------------------------------------------------------------------------------

def check(name, got, ref, bound, k):
    """|got - ref| <= k 2^-24 bound at every element."""
    tol = k * EPS * bound
    got = got.detach().cpu().to(F64)
    assert got.shape == ref.shape == tol.shape, (name, got.shape, ref.shape, tol.shape)
    assert bool(torch.isfinite(got).all()), name
    ratio = float(((got - ref).abs() / tol.clamp_min(1e-300)).max())
    print(f"RATIO {name} {ratio:.3e}")
    assert ratio <= 1.0, (name, ratio)


def run_vfe(gpu, G, P, K, Cout, seed, kind="plain"):
    x, w, sc, sh = LC.vfe_inputs(G, P, K, Cout, seed, kind)
    xg, wg = x.to(gpu), w.to(gpu)
    scg, shg = (None if t is None else t.to(gpu) for t in (sc, sh))
    y = sentinel(G * Cout, F32, gpu)
    L.vfe_smallk_max(xg, wg, scg, shg, y, G, P, K, Cout)
    torch.cuda.synchronize()
    name = f"vfe.{kind}.G{G}.P{P}.K{K}.C{Cout}"
    assert same(y[G * Cout:], sentinel(0, F32, gpu)), name
    ref, bound = LC.vfe_ref(x, w, sc, sh)
    got = y[:G * Cout].view(G, Cout)
    check(name, got, ref, bound, K + 2)
    if Cout % 4 == 0:                                               # the two kernels it replaces: same fma chain, same bits
        if scg is None:                                             # fma(acc, 1, 0) is acc: the explicit identity gives the same bits
            scg, shg = torch.ones(Cout, device=gpu), torch.zeros(Cout, device=gpu)
        t = torch.empty(G * P * Cout, device=gpu)
        L.pointwise_smallk(xg, wg, scg, shg, t, G * P, K, Cout, True)
        two = torch.empty(G, Cout, device=gpu)
        L.group_max(t, two, G, P, Cout)
        assert same(got, two), name
    return got


@pytest.mark.parametrize("K", range(1, 17))
def test_vfe_every_instantiation(gpu, K):
    """P in {1, PC - 1, PC, PC + 1, 2 PC + 1} with PC = 64 // K points per load (dead lanes where K does not divide 64); Cout 64
    (bitwise against the two kernels) and 65 (a second channel chunk with one live lane)."""
    for P in LC.vfe_points(K):
        for Cout in (64, 65):
            run_vfe(gpu, LC.VFE_G, P, K, Cout, 900 + 16 * K + P)


@pytest.mark.parametrize("K,P,Cout", LC.VFE_COUT_EDGE)
def test_vfe_channel_edges(gpu, K, P, Cout):
    run_vfe(gpu, LC.VFE_G, P, K, Cout, 1300 + Cout + K)


@pytest.mark.parametrize("kind", ["nan", "zero_row", "negative", "no_affine"])
def test_vfe_special_inputs(gpu, kind):
    got = run_vfe(gpu, LC.VFE_G, 5, 7, 68, 1400, kind)
    if kind == "negative":
        assert same(got, torch.zeros(LC.VFE_G, 68))                  # +0.0 exactly, never -0.0 or a negative value
    if kind == "zero_row":
        assert same(got[1], LC.vfe_inputs(LC.VFE_G, 5, 7, 68, 1400, kind)[3].clamp_min(0))      # an empty voxel: relu(shift)


def test_vfe_grid_stride(gpu):
    G, P, K, Cout = LC.VFE_BIG                                      # 32771 voxels on 32768 waves: the last three on a second trip
    run_vfe(gpu, G, P, K, Cout, 1500)


# ---- filter / pad ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LC.FILTER_CASES))
def test_filter_pad_case(gpu, name):
    c = LC.filter_case(name)
    pts, mp = c["pts"], c["max_points"]
    N, C = pts.shape
    tiles = -(-N // 1024)
    out, count = sentinel(mp * C, F32, gpu), sentinel(1, I32, gpu)
    work = torch.full((max(N, 1) * C + tiles + PAD,), LC.POISON, device=gpu)          # row `count` holds poison, inside the buffer
    choice = None if c["choice"] is None else torch.from_numpy(c["choice"]).to(gpu)
    L.lidar_filter_pad(torch.from_numpy(pts).to(gpu).view(-1), out, count, work, choice, N, C, mp, c["pc_range"])
    torch.cuda.synchronize()
    ref, n = LC.filter_pad_ref(pts, mp, c["pc_range"], c["choice"])
    assert int(count[0]) == n, name
    assert same(out[:mp * C].view(mp, C), torch.from_numpy(ref)), name
    assert same(out[mp * C:], sentinel(0, F32, gpu)) and same(count[1:], sentinel(0, I32, gpu)[:PAD])
    keep = np.all((pts[:, :3] > np.asarray(c["pc_range"][:3], np.float32)) & (pts[:, :3] < np.asarray(c["pc_range"][3:], np.float32)), 1)
    assert same(work[:n * C].view(n, C), torch.from_numpy(pts[keep]))                 # ALL survivors compacted, in order
    poison = torch.full((1,), LC.POISON)
    assert same(work[n * C:N * C], poison.expand(N * C - n * C)) and same(work[N * C + tiles:], poison.expand(work.numel() - N * C - tiles))
