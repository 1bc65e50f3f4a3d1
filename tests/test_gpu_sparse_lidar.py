"""The opt-in sparse-voxel LiDAR encoder on the MI355X against the dense fp64 restatement of tests/sparse_ref.py (parity unpinned by
the reference, which has no working voxel path): structure (exact integers), the encoder in eval and train mode, and the detector
with the sparse branch -- inference, one training step, bf16 storage and the point-gradient refusal.  The scenes and what each
is built for: tests/sparse_scenes.py, asserted on the CPU by tests/test_sparse_lidar_host.py.

The conv kernel's row tile is 128 output rows per workgroup (S.ROW_TILE, checked against the library below): the `tile-*` scenes
have 127, 128 and 129 active rows at every level."""
import copy

import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import encoders, fusion, synth, training
from tests import pillar_ref
from tests import sparse_ref as R
from tests import sparse_scenes as S
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
MTOL = 1e-4                                # the project's north-star figure

SCENES = {
    "random-c4": dict(C=4, H=12, W=8, zv=8, ch=(32, 64, 128), P=S.RANDOM_MAX_POINTS, pts=lambda: S.random_scene(4)),
    "random-c5": dict(C=5, H=8, W=12, zv=4, ch=(32, 32, 64), P=S.RANDOM_MAX_POINTS, pts=lambda: S.random_scene(5, seed=2)),
    "widths-64-96-32": dict(C=4, H=12, W=8, zv=8, ch=(64, 96, 32), P=S.RANDOM_MAX_POINTS, pts=lambda: S.random_scene(4, seed=4)),
    "structured": dict(C=4, H=12, W=8, zv=8, ch=(32, 64, 128), pts=lambda: S.structured_scene(12, 8, 8)),
    "structured-z4": dict(C=4, H=8, W=12, zv=4, ch=(32, 32, 64), pts=lambda: S.structured_scene(8, 12, 4)),
    "max-voxels-binds": dict(C=4, H=12, W=8, zv=8, ch=(32, 32, 64), P=S.RANDOM_MAX_POINTS, Nv=400,
                             pts=lambda: S.random_scene(4, thin_second=True)),
}
for _n in (S.ROW_TILE - 1, S.ROW_TILE, S.ROW_TILE + 1):                  # row counts one below, on and one above the row tile
    SCENES[f"tile-{_n}"] = dict(C=4, H=12, W=8, zv=8, ch=(32, 64, 128), Nv=256, pts=lambda n=_n: S.tile_scene(12, 8, 8, n))


def _pair(case, seed=3):
    kw = dict(z_voxels=case["zv"], bev_h=case["H"], bev_w=case["W"])
    P, Nv = case.get("P", 8), case.get("Nv", 40000)
    ref = R.SparseEncoderRef(case["C"], case["ch"], max_points=P, max_voxels=Nv, **kw)
    synth.fill_state_dict_(ref, seed)
    enc = encoders.SparseLiDAREncoder(input_channels=case["C"], channels=case["ch"], max_points_per_voxel=P, max_voxels=Nv, **kw)
    enc.load_state_dict(ref.state_dict())
    return ref, enc.cuda()


def _device_structure(enc):
    """Per level, per frame: the engine's active (z, y, x) coordinates in row order, from the last batch's cell / count buffers."""
    s = enc._eng().last
    out = []
    for l, ((D, H, W), cap) in enumerate(zip(s.dims, s.caps)):
        count = s.count[l][:s.B].cpu().tolist()
        cell = s.cell[l][:s.B * cap].cpu().view(s.B, cap)
        frames = []
        for b, n in enumerate(count):
            c = cell[b, :n].long()
            frames.append(torch.stack([c // (H * W), (c // W) % H, c % W], 1))
        out.append(frames)
    return out


def test_row_tile_is_what_the_scenes_assume(gpu):
    assert L.sparse_conv_row_tile() == S.ROW_TILE


@pytest.mark.parametrize("name", list(SCENES))
def test_encoder_eval_structure_and_values_against_fp64(gpu, name):
    case = SCENES[name]
    ref, enc = _pair(case)
    ref.eval(), enc.eval()
    pts = case["pts"]()
    out = enc(pts.to(gpu))
    got = out.cpu()
    with torch.no_grad():
        yard = ref(pts)                                                  # the same reference in fp32 on the CPU: the yardstick
        want, occs, vox = ref.double()(pts, return_levels=True)
    # structure, exact: per-level counts and active coordinates in row order
    dev, host = _device_structure(enc), R.active_coords(occs, vox)
    for l in range(3):
        for b in range(pts.shape[0]):
            assert torch.equal(dev[l][b], host[l][b].long()), (name, l, b, dev[l][b].shape, host[l][b].shape)
    B, c2 = pts.shape[0], case["ch"][2]
    assert out.shape == (B, c2 * case["zv"] // 4, case["H"], case["W"]) and out.dtype == torch.float32
    occ2 = (occs[2][:, 0] > 0)[:, :, None].expand(B, case["zv"] // 4, c2, case["H"], case["W"]).reshape(got.shape)
    assert (got[~occ2] == 0).all()                                       # inactive cells exactly 0
    e_dev, e_yard = rel_err(got, want), rel_err(yard, want)
    print(f"{name}: device rel_err {e_dev:.3e}, fp32 CPU reference {e_yard:.3e}, active rows "
          f"{[[int(f.shape[0]) for f in lv] for lv in host]}")
    assert e_dev <= MTOL
    assert torch.equal(enc(pts.to(gpu)).cpu(), got)                      # two calls: identical bits


def _grad_metric(mod, ora, hard=2e-2, tight=2e-3, most=8):
    """test_gpu_pillars._grad_metric restated: relative L2 per tensor against fp64 autograd, buffers matched by name."""
    gref = dict(ora.named_parameters())
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ora.parameters() if p.grad is not None)))
    worst, loose = [], 0
    for name, p in mod.named_parameters():
        r = gref[name].grad
        assert p.grad is not None and r is not None, name
        l2 = float((p.grad.cpu().double() - r.double()).norm() / (r.double().norm() + 5e-5 * gn))
        worst.append((round(l2, 6), name))
        loose += l2 > tight
    worst.sort(reverse=True)
    assert worst[0][0] <= hard, worst[:6]
    assert loose <= max(2, len(worst) // most), (loose, worst[:6])
    bref = dict(ora.named_buffers())
    for n, b in mod.named_buffers():
        assert rel_err(b.cpu().double(), bref[n].double()) <= 2e-5, n
    return worst


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("name", ["random-c4", "random-c5", "widths-64-96-32", "tile-129"])
def test_encoder_train_against_autograd(gpu, name, frozen):
    case = SCENES[name]
    ref, enc = _pair(case, seed=7)
    ref = ref.double()
    ref.train(), enc.train()
    if frozen:
        for m in (ref, enc):
            for n in encoders.SPARSE_LAYERS:
                getattr(m, n).bn.eval()
    before = {k: v.clone() for k, v in enc.state_dict().items() if "running" in k or "tracked" in k}
    pts = case["pts"]()
    G = torch.randn(pts.shape[0], enc.out_channels, case["H"], case["W"], generator=torch.Generator().manual_seed(1))
    out = enc(pts.to(gpu))
    (out * G.to(gpu)).sum().backward()
    want = ref(pts)
    (want * G.double()).sum().backward()
    e = rel_err(out.detach().cpu(), want.detach())
    worst = _grad_metric(enc, ref)
    print(f"{name} frozen={frozen}: forward rel_err {e:.3e}, worst gradients {worst[:3]}")
    assert e <= MTOL
    for n in encoders.SPARSE_LAYERS:
        assert int(getattr(enc, n).bn.num_batches_tracked) == int(getattr(ref, n).bn.num_batches_tracked) == (3 if frozen else 4)
    if frozen:
        for k, v in before.items():
            assert torch.equal(enc.state_dict()[k], v), k                # frozen BatchNorm: buffers bit-unchanged
    # a second run from the same state: identical gradient bits
    _, enc2 = _pair(case, seed=7)
    enc2.train()
    if frozen:
        for n in encoders.SPARSE_LAYERS:
            getattr(enc2, n).bn.eval()
    (enc2(pts.to(gpu)) * G.to(gpu)).sum().backward()
    for (k, p), (_, q) in zip(enc.named_parameters(), enc2.named_parameters()):
        assert torch.equal(p.grad, q.grad), k


def test_train_mode_refuses_fewer_than_two_rows(gpu):
    _, enc = _pair(SCENES["structured"])
    enc.train()
    one = S.points_at([(4, 4, 4)], 12, 8, 8)[None].contiguous()
    with pytest.raises(L.BevfError, match="fewer than two"):
        enc(one.to(gpu))


# ---- the detector --------------------------------------------------------------------------------------------------------------

DET = dict(channels=[32, 32, 64], z_voxels=4, max_points_per_voxel=4, max_voxels=6000)
H = W = 50                                  # the smallest BEV the pillar detector tests use


def _config():
    return {"model": {"camera_encoder": {"pretrained": False}, "lidar_encoder": dict(DET, type="SparseVoxel", input_channels=4)},
            "dataset": {"bev_h": H, "bev_w": W}}


def _det_pair(seed=11):
    ora = R.make_sparse_detector("lidar+radar", H, W, cin=4, channels=tuple(DET["channels"]), z_voxels=DET["z_voxels"],
                                 max_points=DET["max_points_per_voxel"], max_voxels=DET["max_voxels"])
    synth.fill_state_dict_(ora, seed)
    model = fusion.create_detector("lidar+radar", "bev", "centernet", config=_config(), lidar_encoder_type="SparseVoxel")
    model.load_state_dict(ora.state_dict())
    return ora.double(), model.to("cuda")


def _inputs(seed=21, N=3000):
    _, _, radars = synth.frame_inputs(2, 0, 64, 96, 0, 4, 5, 25, 7, seed=seed)
    return pillar_ref.pillar_points(2, N, 4, seed=seed), radars


_REF = {}


def _inference_reference():
    """fp64 composition: the sparse reference + the oracle's fusion and head -- computed once, shared, never modified."""
    if "inf" not in _REF:
        ora, _ = _det_pair()
        ora.eval()
        pts, radars = _inputs()
        with torch.no_grad():
            _REF["inf"] = {k: v.clone() for k, v in ora(None, pts, [r.double() for r in radars]).items()}
    return _REF["inf"]


def test_detector_inference_against_fp64(gpu):
    _, model = _det_pair()
    model.eval()
    assert isinstance(model.lidar_encoder, encoders.SparseLiDAREncoder) and model.fusion.lidar_bev[0].in_channels == 64
    pts, radars = _inputs()
    out = model(None, pts.cuda(), [r.cuda() for r in radars])
    for k, v in _inference_reference().items():
        e = rel_err(out[k].cpu(), v)
        print(f"detector {k}: rel_err {e:.3e}")
        assert e <= MTOL, (k, e)


def test_detector_train_step_against_autograd(gpu):
    ora, model = _det_pair(seed=13)
    ora.train(), model.train()
    pts, radars = _inputs(seed=31)
    gen = torch.Generator().manual_seed(2)
    out = model(None, pts.cuda(), [r.cuda() for r in radars])
    Gs = {k: torch.randn(v.shape, generator=gen) for k, v in out.items()}
    loss = sum((out[k] * Gs[k].cuda()).sum() for k in out)
    assert torch.isfinite(loss)
    loss.backward()
    ref = ora(None, pts, [r.double() for r in radars])
    sum((ref[k] * Gs[k].double()).sum() for k in ref).backward()
    for k in ref:
        assert rel_err(out[k].detach().cpu(), ref[k].detach()) <= MTOL, k
    worst = _grad_metric(model, ora)
    lid = [w for w in worst if w[1].startswith("lidar_encoder.")]
    print("detector train step, LiDAR encoder gradients:", lid[:5])
    assert len(lid) == 15 and lid[0][0] <= 2e-2
    params = dict(model.named_parameters())
    for n in encoders.SPARSE_LAYERS:
        for leaf in ("conv.weight", "bn.weight", "bn.bias"):
            g = params[f"lidar_encoder.{n}.{leaf}"].grad
            assert torch.isfinite(g).all() and g.abs().sum() > 0, (n, leaf)
    opt = training.FusedAdamW(model.parameters(), lr=1e-3)
    before = model.lidar_encoder.conv_in.conv.weight.detach().clone()
    opt.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert not torch.equal(before, model.lidar_encoder.conv_in.conv.weight.detach())


def test_bf16_sparse_detector_against_fp32(gpu):
    _, m32 = _det_pair()
    m32.eval()
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():                                                # the fp32 model on the same bf16-rounded weights
        for p in list(m32.parameters()) + list(m32.buffers()):
            if p.dtype == torch.float32:
                p.copy_(p.bfloat16().float())
    pts, radars = _inputs()
    o16 = m16(None, pts.cuda(), [r.cuda() for r in radars])
    o32 = m32(None, pts.cuda(), [r.cuda() for r in radars])
    assert m16.lidar_encoder.forward_nhwc(pts.cuda()).dtype == torch.bfloat16
    for k in o32:
        assert rel_err(o16[k].float().cpu(), o32[k].cpu()) <= 3e-2, k    # the bound of test_gpu_pillars' bf16 case


def test_point_gradients_are_refused(gpu):
    _, enc = _pair(SCENES["random-c4"])
    enc.train()
    pts = S.random_scene(4)[:1].cuda().requires_grad_()
    with pytest.raises(L.BevfError, match="no gradient path"):
        enc(pts)
    _, model = _det_pair()
    model.train()
    with pytest.raises(L.BevfError, match="no gradient path"):
        model(None, pillar_ref.pillar_points(1, 500, 4).cuda().requires_grad_(), None)
