"""The opt-in PointPillars LiDAR branch on the MI355X against the fp64 restatement of tests/pillar_ref.py (parity unpinned by the
reference, which has no working voxel path): the encoder in eval and train mode, the detector forward / training step with the
pillar branch, hipGraph replay, bf16 storage and the point-gradient refusal."""
import copy

import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import encoders, engine, fusion, synth, training
from oracle.ref_voxelize import hard_voxelize
from tests import pillar_ref as R
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
KTOL, MTOL = 2e-5, 1e-4


def _encoder_pair(C=4, H=50, W=50, P=32, Nv=12000, cout=64, seed=3):
    ref = R.PillarEncoderRef(C, cout, H, W, max_points=P, max_pillars=Nv)
    synth.fill_state_dict_(ref, seed)
    enc = encoders.PillarLiDAREncoder(input_channels=C, pfn_channels=cout, bev_h=H, bev_w=W, max_points_per_pillar=P, max_pillars=Nv)
    enc.load_state_dict(ref.state_dict())
    return ref.double(), enc.cuda()


def _occupied(pts, enc):
    _, _, _, _, vs = enc.grid()
    _, coords, npts, nvox = hard_voxelize(pts, enc.pc_range, vs, enc.max_points, enc.max_pillars)
    occ = torch.zeros(pts.shape[0], enc.bev_h, enc.bev_w, dtype=torch.bool)
    for b in range(pts.shape[0]):
        n = int(nvox[b])
        occ[b, coords[b, :n, 1], coords[b, :n, 2]] = True
    return occ, npts, nvox


def _edge_points(C=4):
    """Frame 0: points on the range edges (x = x_min kept, x = x_max dropped, y just below y_max) among random ones;
    frame 1: every point outside the range (an empty frame in the batch)."""
    pts = R.pillar_points(2, 2000, C, seed=9)
    pts[0, :4, 0] = -51.2
    pts[0, 4:8, 0] = 51.2
    pts[0, 8:12, 1] = torch.nextafter(torch.tensor(51.2), torch.tensor(0.0))
    pts[0, 12:16, 2] = -5.0
    pts[1, :, 0] = 60.0 + pts[1, :, 0].abs()
    return pts


CASES = [dict(C=4, H=50, W=50, N=3000), dict(C=5, H=128, W=96, N=3000), dict(C=4, H=128, W=96, N=4000, P=8, Nv=300),
         dict(C=5, H=50, W=50, N=6000, P=4, Nv=200), dict(C=4, H=50, W=50, edge=True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_encoder_eval_against_fp64(gpu, case):
    C, H, W = case["C"], case["H"], case["W"]
    P, Nv = case.get("P", 32), case.get("Nv", 12000)
    ref, enc = _encoder_pair(C, H, W, P, Nv)
    ref.eval(), enc.eval()
    pts = _edge_points(C) if case.get("edge") else R.pillar_points(2, case["N"], C, seed=H + C)
    occ, npts, nvox = _occupied(pts, enc)
    if "P" in case:                                                     # both caps bind
        assert int(npts.max()) == P and int(nvox.max()) == Nv
    if case.get("edge"):
        assert int(nvox[1]) == 0 and occ[0, :, 0].any()                  # the empty frame; x = x_min lands in column 0
    out = enc(pts.to(gpu))
    with torch.no_grad():
        want = ref(pts)
    assert out.shape == (2, 64, H, W) and out.dtype == torch.float32
    got = out.cpu()
    assert rel_err(got, want) <= KTOL
    assert (got.permute(0, 2, 3, 1)[~occ] == 0).all()                  # unoccupied cells exactly 0
    assert torch.equal(enc(pts.to(gpu)).cpu(), got)                     # two launches: identical bits


def _grad_metric(mod, ora, hard=2e-2, tight=2e-3, most=8):
    """test_gpu_standalone_train._check_params' relative-L2-per-tensor metric, buffers matched by name."""
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
@pytest.mark.parametrize("C,H,W,P,Nv", [(4, 50, 50, 32, 12000), (5, 128, 96, 8, 400)])
def test_encoder_train_against_autograd(gpu, frozen, C, H, W, P, Nv):
    ref, enc = _encoder_pair(C, H, W, P, Nv, seed=7)
    ref.train(), enc.train()
    if frozen:
        ref.pfn.bn.eval(), enc.pfn.bn.eval()
    pts = R.pillar_points(2, 3000, C, seed=5)
    _, _, nvox = _occupied(pts, enc)
    if Nv == 12000:
        assert int(nvox.max()) * 4 < Nv                                  # most pillar slots empty: they stay out of the statistics
    else:
        assert int(nvox.min()) == Nv                                     # the pillar cap binds
    G = torch.randn(2, 64, H, W, generator=torch.Generator().manual_seed(1))
    out = enc(pts.to(gpu))
    (out * G.to(gpu)).sum().backward()
    want = ref(pts)
    (want * G.double()).sum().backward()
    assert rel_err(out.detach().cpu(), want.detach()) <= KTOL
    worst = _grad_metric(enc, ref, hard=2e-3, tight=2e-3)
    assert worst[0][0] <= 2e-3, worst


def _det_pair(modality, H, W, seed=11):
    ora = R.make_pillar_detector(modality, H, W)
    synth.fill_state_dict_(ora, seed)
    model = fusion.create_detector(modality, "bev", "centernet", bev_h=H, bev_w=W, lidar_encoder_type="PointPillars")
    model.load_state_dict(ora.state_dict())
    return ora.double(), model.to("cuda")


def _inputs(modality, B=2, N=3000, seed=21):
    imgs, _, radars = synth.frame_inputs(B, 2, 64, 96, 0, 4, 5, 25, 7, seed=seed)
    pts = R.pillar_points(B, N, 4, seed=seed)
    m = modality.replace(" ", "")
    return (imgs if "camera" in m else None), pts, (radars if "radar" in m else None)


def _d(x):
    if x is None:
        return None
    return [r.double() for r in x] if isinstance(x, list) else x.double()


def _cuda(x):
    if x is None:
        return None
    return [r.cuda() for r in x] if isinstance(x, list) else x.cuda()


@pytest.mark.parametrize("mode", ["f32", "wino"])
@pytest.mark.parametrize("modality,H,W", [("camera+lidar+radar", 50, 50), ("camera+lidar+radar", 128, 96), ("lidar", 50, 50),
                                          ("lidar", 128, 96)])
def test_detector_inference_against_fp64(gpu, mode, modality, H, W):
    ora, model = _det_pair(modality, H, W)
    ora.eval(), model.eval()
    imgs, pts, radars = _inputs(modality)
    old = engine.conv_mode()
    engine.set_conv_mode(mode)
    try:
        out = model(_cuda(imgs), _cuda(pts), _cuda(radars))
    finally:
        engine.set_conv_mode(old)
    with torch.no_grad():
        ref = ora(_d(imgs), pts, _d(radars))
    for k, v in ref.items():
        assert rel_err(out[k].cpu(), v) <= MTOL, (k, rel_err(out[k].cpu(), v))


@pytest.mark.parametrize("modality", ["camera+lidar+radar", "lidar"])
def test_detector_train_step_against_autograd(gpu, modality):
    ora, model = _det_pair(modality, 50, 50, seed=13)
    ora.train(), model.train()
    imgs, pts, radars = _inputs(modality, seed=31)
    gen = torch.Generator().manual_seed(2)
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    try:
        out = model(_cuda(imgs), _cuda(pts), _cuda(radars))
        Gs = {k: torch.randn(v.shape, generator=gen) for k, v in out.items()}
        sum((out[k] * Gs[k].cuda()).sum() for k in out).backward()
    finally:
        engine.set_conv_mode(old)
    ref = ora(_d(imgs), pts, _d(radars))
    sum((ref[k] * Gs[k].double()).sum() for k in ref).backward()
    for k in ref:
        assert rel_err(out[k].detach().cpu(), ref[k].detach()) <= MTOL, k
    # the camera trunk and the radar MLP's max-over-points carry the few fp32-vs-fp64 ReLU / argmax flips of a whole detector
    # (test_gpu_standalone_train._check_params): the usual 2e-2 bound, `tight` at 5e-3; the LiDAR branch is held to 2e-3
    worst = _grad_metric(model, ora, tight=5e-3)
    lid = [w for w in worst if w[1].startswith(("lidar_encoder.", "fusion.lidar_bev."))]
    assert lid and lid[0][0] <= 2e-3, lid[:4]
    for n in ("lidar_encoder.pfn.linear.weight", "lidar_encoder.pfn.bn.weight", "fusion.lidar_bev.0.weight", "fusion.lidar_bev.4.bias"):
        assert dict(model.named_parameters())[n].grad.abs().sum() > 0, n
    opt = training.FusedAdamW(model.parameters(), lr=1e-3)
    before = model.lidar_encoder.pfn.linear.weight.detach().clone()
    opt.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert not torch.equal(before, model.lidar_encoder.pfn.linear.weight.detach())


def test_graphed_pillar_detector_replays_bit_identically(gpu):
    _, model = _det_pair("camera+lidar+radar", 50, 50)
    model.eval()
    a, b = _inputs("camera+lidar+radar", seed=41), _inputs("camera+lidar+radar", seed=42)
    g = model.make_graphed(*(_cuda(x) for x in a))
    for inp in (b, a):
        gi = tuple(_cuda(x) for x in inp)
        got = {k: v.clone() for k, v in g(*gi).items()}
        eager = model(*gi)
        for k in eager:
            assert torch.equal(got[k], eager[k]), k


def test_bf16_pillar_detector_against_fp32(gpu):
    _, m32 = _det_pair("camera+lidar+radar", 50, 50)
    m32.eval()
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():                                                # the fp32 model on the same bf16-rounded weights
        for p in list(m32.parameters()) + list(m32.buffers()):
            if p.dtype == torch.float32:
                p.copy_(p.bfloat16().float())
    imgs, pts, radars = _inputs("camera+lidar+radar")
    o16 = m16(_cuda(imgs), _cuda(pts), _cuda(radars))
    o32 = m32(_cuda(imgs), _cuda(pts), _cuda(radars))
    assert m16.lidar_encoder.forward_nhwc(pts.cuda()).dtype == torch.bfloat16
    for k in o32:
        assert rel_err(o16[k].float().cpu(), o32[k].cpu()) <= 3e-2, k


def test_point_gradients_are_refused(gpu):
    _, enc = _encoder_pair()
    enc.train()
    pts = R.pillar_points(1, 500, 4).cuda().requires_grad_()
    with pytest.raises(L.BevfError, match="no gradient path"):
        enc(pts)
    _, model = _det_pair("lidar", 50, 50)
    model.train()
    with pytest.raises(L.BevfError, match="no gradient path"):
        model(None, pts, None)
