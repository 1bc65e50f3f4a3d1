"""Per-frame camera calibration of the 'project' branch on the MI355X: the device-built tables against the host fp64 build, their
deterministic transposition, the gather with a table per frame, and `camera_calib=` through FlexibleBEVFusion, the detector (eval
and train, fp32 and bf16) and GraphedDetector -- against the fp64 grid_sample restatement of tests/camera_bev_ref.py applied frame
by frame.  The rigs are tests/camera_calib_rigs.py's (default_rig() with a seeded jitter, distinct for every frame); their margin
condition is checked in tests/test_camera_calib_host.py, so nothing is excluded here."""
import copy

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import engine, fusion, synth
from bevfusion_multimodal_3d_object_detection_amd.encoders import pillar_grid
from oracle import ref_model
from tests import camera_calib_rigs as RG
from tests import pillar_ref as PR
from tests.conftest import rel_err
from tests.test_gpu_camera_bev import _cu, _db, _features, _frames, _gather_ref, _random_table

pytestmark = pytest.mark.gpu
RANGE = RG.RANGE
MTOL = 1e-4


class DeviceTables:
    """bevf_camera_table_build_f64 (+ transpose) for `rigs` through the _lib wrappers, into buffers pre-filled with junk."""

    def __init__(self, rigs, Hc, Wc, S, transpose=True):
        calib = torch.from_numpy(CR.calib_matrices(rigs)).cuda()
        self.B, self.ncam = calib.shape[:2]
        self.P, self.ncols = S * S, self.ncam * Hc * Wc
        self.cap = cap = L.camera_table_capacity(self.P, 8, self.ncam)
        i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device="cuda")                  # noqa: E731
        f32 = lambda n: torch.full((n,), float("nan"), device="cuda")                             # noqa: E731
        B = self.B
        self.row_ptr, self.col, self.w = i32(B * (self.P + 1)), i32(B * cap), f32(B * cap)
        work = i32(L.camera_table_work_elems(B, cap, max(self.P, self.ncols)))
        z = (float(np.float32(RANGE[2])), float(np.float32(RANGE[5])))
        L.camera_table_build(calib, B, self.ncam, pillar_grid(RANGE, S, S)[:4], S, S, z, 8, 0.1, rigs[0].image_size, Hc, Wc,
                             self.row_ptr, self.col, self.w, cap, work)
        if transpose:
            self.t_row_ptr, self.t_col, self.t_w = i32(B * (self.ncols + 1)), i32(B * cap), f32(B * cap)
            L.camera_table_transpose(self.row_ptr, self.col, self.w, cap, B, self.P, self.ncols, self.t_row_ptr, self.t_col,
                                     self.t_w, work)

    def frame(self, b, transposed=False):
        """(row_ptr, col, w) of frame b on the host (numpy), the used part only."""
        nrows = self.ncols if transposed else self.P
        rp, col, w = (self.t_row_ptr, self.t_col, self.t_w) if transposed else (self.row_ptr, self.col, self.w)
        rp = rp.view(self.B, nrows + 1)[b].cpu().numpy()
        n = int(rp[-1])
        return rp, col[b * self.cap:b * self.cap + n].cpu().numpy(), w[b * self.cap:b * self.cap + n].cpu().numpy()

    def project(self, x, y, C):
        L.csr_gather_frames(self.row_ptr, self.col, self.w, self.cap, self.P, self.ncols, x, self.ncols * C, C, y, self.P * C, C,
                            self.B, C)

    def project_backward(self, dy, dx, C):
        L.csr_gather_frames(self.t_row_ptr, self.t_col, self.t_w, self.cap, self.ncols, self.P, dy, self.P * C, C, dx,
                            self.ncols * C, C, self.B, C)


# ---- the tables -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,Hc,Wc,B,jitter", [(40, 12, 20, 3, True), (128, 57, 100, 2, True), (40, 12, 20, 3, False)])
def test_device_table_against_the_host_build(gpu, S, Hc, Wc, B, jitter):
    rigs = RG.frame_rigs(B) if jitter else [CR.default_rig()] * B
    dev = DeviceTables(rigs, Hc, Wc, S)
    again = DeviceTables(rigs, Hc, Wc, S)
    P, ncols = dev.P, dev.ncols
    for b, rig in enumerate(rigs):
        t = CR.build_projection_table(rig, Hc, Wc, RANGE, S, S)
        rp, col, w = dev.frame(b)
        assert rp[0] == 0 and (np.diff(rp) >= 0).all() and rp[-1] <= dev.cap
        assert col.min() >= 0 and col.max() < ncols and np.isfinite(w).all()
        rows = np.repeat(np.arange(P), np.diff(rp))
        key = rows.astype(np.int64) * ncols + col
        assert (np.diff(key) > 0).all()                                    # rows sorted by pixel, no duplicate (cell, pixel)
        hkey = np.repeat(np.arange(P), np.diff(t.row_ptr)).astype(np.int64) * ncols + t.col
        # merged by key: an entry missing on one side counts as weight 0 there
        keys = np.union1d(key, hkey)
        dw, hw = np.zeros(keys.shape[0]), np.zeros(keys.shape[0])
        dw[np.searchsorted(keys, key)] = w
        hw[np.searchsorted(keys, hkey)] = t.w64
        err = float(np.abs(dw - hw).max())
        sums = np.bincount(rows, weights=w.astype(np.float64), minlength=P)
        nonempty = np.diff(rp) > 0
        print(f"frame {b}: {key.shape[0]} entries (host {hkey.shape[0]}), {keys.shape[0] - hkey.shape[0]} keys the host lacks, "
              f"max |w - w64| {err:.2e}, max per cell {np.diff(rp).max()}, empty cells {(~nonempty).mean():.4f}, "
              f"min row sum of a non-empty cell {sums[nonempty].min():.3f}")
        assert err <= 1e-6
        assert np.array_equal(nonempty, np.diff(t.row_ptr) > 0)          # the same set of non-empty cells
        # row sums: 0 for an empty row, else the host's within 1e-6 -- which is 1 unless a bilinear tap of the cell fell off the
        # feature map and was dropped (cells that look at an image border sum to less than 1 in the host table as well)
        hsums = np.bincount(np.repeat(np.arange(P), np.diff(t.row_ptr)), weights=t.w64, minlength=P)
        whole = np.abs(hsums - 1) <= 1e-12
        assert whole.sum() > P // 2 and np.abs(sums[whole] - 1).max() <= 1e-6
        assert np.abs(sums - hsums).max() <= 1e-6 and sums.max() <= 1 + 1e-6 and (sums[~nonempty] == 0).all()
        # the transposed table: the same triples, bit-equal weights, every pixel row in ascending cell order
        trp, tcol, tw = dev.frame(b, transposed=True)
        assert trp[0] == 0 and trp[-1] == rp[-1] and tcol.min() >= 0 and tcol.max() < P
        pix = np.repeat(np.arange(ncols), np.diff(trp))
        tkey = pix.astype(np.int64) * P + tcol
        assert (np.diff(tkey) > 0).all()
        order = np.lexsort((pix, tcol))                                     # by cell, then pixel = the forward order
        assert np.array_equal(tcol[order], rows) and np.array_equal(pix[order], col)
        assert np.array_equal(tw[order].view(np.int32), w.view(np.int32))
        for x, y in zip(dev.frame(b) + dev.frame(b, True), again.frame(b) + again.frame(b, True)):      # two builds: identical bits
            assert np.array_equal(x.view(np.int32), y.view(np.int32))


# ---- the gather with a table per frame ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,C,B", [(torch.float32, 512, 3), (torch.float32, 64, 5), (torch.float32, 1024, 2),
                                       (torch.bfloat16, 512, 5), (torch.bfloat16, 128, 1)])
def test_gather_frames_kernel(gpu, dtype, C, B):
    nrows, ncols = 301, 257
    tabs = [_random_table(nrows, ncols, 100 * b + C + B) for b in range(B)]
    cap = max(int(t[0][-1]) for t in tabs) + 13
    row_ptr = np.stack([t[0] for t in tabs])
    col, w = np.full((B, cap), 2 ** 30, np.int32), np.full((B, cap), np.nan, np.float32)       # junk past each frame's end
    for b, (rp, cl, wt) in enumerate(tabs):
        col[b, :rp[-1]], w[b, :rp[-1]] = cl, wt
    x = torch.randn(B, ncols, C, generator=torch.Generator().manual_seed(B)).to(dtype)
    want = torch.cat([_gather_ref(*tabs[b], x[b:b + 1]) for b in range(B)])
    d = lambda a: torch.from_numpy(a).to(gpu).reshape(-1)                  # noqa: E731
    rp, cl, wt, xd = d(row_ptr), d(col), d(w), x.to(gpu).contiguous()
    y = torch.full((B, nrows, 3 * C), 7.0, dtype=dtype, device=gpu)
    L.csr_gather_frames(rp, cl, wt, cap, nrows, ncols, xd, ncols * C, C, y.view(-1)[C:], nrows * 3 * C, 3 * C, B, C)
    got = y[:, :, C:2 * C].float().cpu()
    tol = 2e-6 if dtype == torch.float32 else 4e-3
    err = rel_err(got, want)
    print(f"csr_gather_frames {dtype} C={C} B={B}: rel err {err:.2e}")
    assert err <= tol
    assert (y[:, :, :C] == 7.0).all() and (y[:, :, 2 * C:] == 7.0).all()
    for b in range(B):
        assert (got[b, torch.from_numpy(np.diff(row_ptr[b]) == 0)] == 0).all()
    y2 = torch.full_like(y, -3.0)
    L.csr_gather_frames(rp, cl, wt, cap, nrows, ncols, xd, ncols * C, C, y2.view(-1)[C:], nrows * 3 * C, 3 * C, B, C)
    assert torch.equal(y2[:, :, C:2 * C], y[:, :, C:2 * C])                 # two launches: identical bits


def test_forward_and_backward_per_frame_against_grid_sample_autograd(gpu):
    B, C, Hc, Wc, S = 3, 64, 12, 20, 40
    rigs = RG.frame_rigs(B)
    tab = DeviceTables(rigs, Hc, Wc, S)
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(B, 6, C, Hc, Wc, generator=g, dtype=torch.float64, requires_grad=True)
    G = torch.randn(B, C, S, S, generator=g, dtype=torch.float64)
    out = RG.project_frames_ref(feats, rigs, S)
    (out * G).sum().backward()
    x = feats.detach().permute(0, 1, 3, 4, 2).reshape(B, -1, C).float().contiguous().to(gpu)
    y = torch.empty(B * S * S * C, device=gpu)
    tab.project(x, y, C)
    err = rel_err(y.view(B, S, S, C).permute(0, 3, 1, 2).cpu(), out.detach())
    dy = G.permute(0, 2, 3, 1).reshape(-1).float().contiguous().to(gpu)
    dx = torch.full((B * tab.ncols * C,), float("nan"), device=gpu)
    tab.project_backward(dy, dx, C)
    got = dx.view(B, 6, Hc, Wc, C).permute(0, 1, 4, 2, 3).cpu()
    assert torch.isfinite(got).all()                                      # every element written
    berr = rel_err(got, feats.grad)
    print(f"per-frame lift: forward rel err {err:.2e}, backward rel err {berr:.2e}")
    assert err <= 2e-6 and berr <= 2e-6
    y2, dx2 = torch.empty_like(y), torch.empty_like(dx)
    tab.project(x, y2, C)
    tab.project_backward(dy, dx2, C)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)


# ---- FlexibleBEVFusion ----------------------------------------------------------------------------------------------------------

def _fusion_pair(modality, H, W, rigs, seed=5):
    """(fp64 oracle lifting frame b through rigs[b], device module whose own rig is default_rig())."""
    m = modality.replace(" ", "")
    cam, lid, rad = "camera" in m, "lidar" in m, "radar" in m
    ora = RG.projecting_frames(ref_model.BEVFusion(cam, lid, rad, bev_h=H, bev_w=W), rigs)
    synth.fill_state_dict_(ora, seed)
    fus = fusion.FlexibleBEVFusion(use_camera=cam, use_lidar=lid, use_radar=rad, bev_h=H, bev_w=W, pc_range=list(RANGE),
                                   camera_view_transform="project")
    fus.set_camera_rig(CR.default_rig().subset(rigs[0].num_cameras))
    fus.load_state_dict(ora.state_dict())
    return ora.double(), fus.to("cuda")


def test_same_rig_in_every_frame_equals_the_static_rig_module(gpu):
    rig = CR.default_rig()
    _, fus = _fusion_pair("camera+lidar", 50, 50, [rig, rig])
    fus.eval()
    cam, lid, _ = _features("camera+lidar", 2, 6, 8, 14)
    static = fus(cam.cuda(), lid.cuda()).clone()
    for calib in ([rig, rig], torch.from_numpy(CR.calib_matrices([rig, rig])), torch.from_numpy(CR.calib_matrices([rig, rig])).cuda()):
        out = fus(cam.cuda(), lid.cuda(), camera_calib=calib)
        err = rel_err(out.cpu(), static.cpu())
        print(f"same rig per frame against the static table: rel err {err:.2e}")
        assert err <= 2e-6
    assert torch.equal(fus(cam.cuda(), lid.cuda()), static)                # the static path is untouched by the per-frame one


def test_distinct_rigs_matter_and_a_frame_depends_on_its_own_calibration_only(gpu):
    rigs = RG.frame_rigs(3)
    _, fus = _fusion_pair("camera", 50, 50, rigs)
    fus.eval()
    cam, _, _ = _features("camera", 3, 6, 8, 14)
    static = fus(cam.cuda()).clone()
    out = fus(cam.cuda(), camera_calib=rigs).clone()
    diff = rel_err(out.cpu(), static.cpu())
    print(f"distinct rigs against the static rig: rel difference {diff:.2e}")
    assert diff > 100 * MTOL
    other = fus(cam.cuda(), camera_calib=[rigs[0], RG.jittered_rig(7), rigs[2]])
    assert torch.equal(other[0], out[0]) and torch.equal(other[2], out[2])
    assert rel_err(other[1].cpu(), out[1].cpu()) > 100 * MTOL


@pytest.mark.parametrize("modality", ["camera", "camera+lidar", "camera+radar", "camera+lidar+radar"])
def test_fusion_eval_per_frame_against_fp64(gpu, modality):
    rigs = RG.frame_rigs(2)
    ora, fus = _fusion_pair(modality, 50, 50, rigs)
    ora.eval(), fus.eval()
    feats = _features(modality, 2, 6, 8, 14)
    out = fus(*(_cu(f) for f in feats), camera_calib=rigs)
    with torch.no_grad():
        want = ora(*(_db(f) for f in feats))
    err = rel_err(out.cpu(), want)
    print(f"fusion(project, per-frame calibration) {modality}: rel err {err:.2e}")
    assert out.shape == (2, 256, 50, 50) and err <= MTOL


def test_fusion_rejects_a_calibration_that_does_not_match_the_features(gpu):
    rigs = RG.frame_rigs(2)
    _, fus = _fusion_pair("camera+lidar", 50, 50, rigs)
    fus.eval()
    cam, lid, _ = _features("camera+lidar", 2, 4, 8, 14)
    with pytest.raises(ValueError, match="4, 4"):
        fus(cam.cuda(), lid.cuda(), camera_calib=rigs)                      # 6-camera calibration, 4-camera features


def test_fusion_train_mode_per_frame_parameter_and_camera_gradients(gpu):
    rigs = RG.frame_rigs(2, ncam=3)
    ora, fus = _fusion_pair("camera+lidar", 20, 20, rigs, seed=17)
    ora.train(), fus.train()
    cam, lid, _ = _features("camera+lidar", 2, 3, 6, 10, seed=4)
    G = torch.randn(2, 256, 20, 20, generator=torch.Generator().manual_seed(8))
    cam_d, lid_d = cam.cuda().requires_grad_(), lid.cuda().requires_grad_()
    out = fus(cam_d, lid_d, camera_calib=rigs)
    # another forward with other calibrations before the backward: the tape rebuilds its own tables
    with torch.no_grad():
        fus(cam.cuda(), lid.cuda(), camera_calib=RG.frame_rigs(2, ncam=3, first_seed=4))
    (out * G.cuda()).sum().backward()
    cam_r, lid_r = cam.double().requires_grad_(), lid.double().requires_grad_()
    want = ora(cam_r, lid_r)
    (want * G.double()).sum().backward()
    assert rel_err(out.detach().cpu(), want.detach()) <= MTOL
    assert cam_d.grad is not None and cam_d.grad.shape == cam.shape
    err = rel_err(cam_d.grad.cpu(), cam_r.grad)
    print(f"fusion train (per-frame calibration): camera gradient rel err {err:.2e}")
    assert err <= 2e-3
    gref = dict(ora.named_parameters())
    gn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in ora.parameters())))
    for n, p in fus.named_parameters():          # (the bounds and the camera_proj restriction of tests/test_gpu_camera_bev.py)
        if not n.startswith("camera_proj."):
            continue
        r = gref[n].grad
        assert float((p.grad.cpu().double() - r).abs().max()) <= 2e-3 * float(r.abs().max()) + 2e-6 * gn, n


def test_graph_replay_between_a_training_forward_and_its_backward(gpu):
    """A replay of a captured detector rewrites the engine's per-frame tables; the tape of an earlier training forward through
    the same fusion module rebuilds its own before the backward: the camera gradient is bit-identical to an undisturbed step."""
    rigs, other = RG.frame_rigs(2), RG.frame_rigs(2, first_seed=4)
    _, model = _det_pair("camera+lidar+radar", 50, 50, rigs)
    model.eval()
    a = _frames(41)
    cu = lambda f: (f[0].cuda(), f[1].cuda(), [r.cuda() for r in f[2]])     # noqa: E731
    g = model.make_graphed(*cu(a), camera_calib=other)
    fus = model.fusion
    cam, lid, rad = _features("camera+lidar+radar", 2, 6, 4, 6, seed=4)
    G = torch.randn(2, 256, 50, 50, generator=torch.Generator().manual_seed(8)).cuda()
    grads = []
    for disturb in (False, True):
        fus.train()
        cam_d = cam.cuda().requires_grad_()
        out = fus(cam_d, lid.cuda(), rad.cuda(), camera_calib=rigs)
        if disturb:
            g(*cu(a), camera_calib=other)
        (out * G).sum().backward()
        grads.append(cam_d.grad.clone())
        fus.zero_grad()
    assert torch.equal(grads[0], grads[1])


# ---- the detector ---------------------------------------------------------------------------------------------------------------

def _det_pair(modality, H, W, rigs, seed=11, lidar="PointNet"):
    ora = PR.make_pillar_detector(modality, H, W) if lidar == "PointPillars" else ref_model.make_detector(modality, H, W)
    RG.projecting_frames(ora.fusion, rigs)
    synth.fill_state_dict_(ora, seed)
    model = fusion.create_detector(modality, "bev", "centernet", bev_h=H, bev_w=W, lidar_encoder_type=lidar,
                                   camera_view_transform="project")
    model.fusion.set_camera_rig(CR.default_rig().subset(rigs[0].num_cameras))
    model.load_state_dict(ora.state_dict())
    return ora, model.to("cuda")


@pytest.mark.parametrize("lidar", ["PointNet", "PointPillars"])
def test_detector_config4_shapes_eval_per_frame_against_fp64(gpu, lidar):
    """2 frames of 6 x 448x800 images (28 x 50 features), 35 000 points, BEV 50^2 -- the config-4 shapes -- each through its own rig."""
    rigs = RG.frame_rigs(2)
    ora, model = _det_pair("camera+lidar", 50, 50, rigs, lidar=lidar)
    ora = ora.double().eval()
    model.eval()
    imgs, pts, _ = synth.frame_inputs(2, 6, 448, 800, 35000, 4, seed=0x5EED + 7)
    if lidar == "PointPillars":
        pts = PR.pillar_points(2, 35000, 4, seed=7)
    out = model(imgs.cuda(), pts.cuda(), None, camera_calib=rigs)
    with torch.no_grad():
        want = ora(imgs.double(), pts if lidar == "PointPillars" else pts.double(), None)
    for k, v in want.items():
        err = rel_err(out[k].cpu(), v)
        print(f"detector(project, per-frame calibration, {lidar}) {k}: rel err {err:.2e}")
        assert err <= MTOL, (k, err)


class _WithCalib:
    """A detector called with a fixed camera_calib (for helpers that call model(imgs, pts, radars))."""

    def __init__(self, model, calib):
        self.model, self.calib = model, calib

    def __call__(self, imgs, pts, radars):
        return self.model(imgs, pts, radars, camera_calib=self.calib)

    def __getattr__(self, name):
        return getattr(self.model, name)


@pytest.mark.parametrize("modality", ["camera+lidar+radar", "camera+lidar"])
def test_detector_train_per_frame_gradients_against_fp64_with_relu_replay(gpu, modality):
    from tests.golden import cases
    from tests.test_gpu_training import _grad_check_against_oracle
    rigs = RG.frame_rigs(2, ncam=2)
    ora, model = _det_pair(modality, 50, 50, rigs, seed=77)
    ora.train(), model.train()
    imgs, pts, radars = synth.frame_inputs(2, 2, 64, 96, 200, 4, 5 if "radar" in modality else 0, 20, 7, seed=123)
    boxes, labels = cases.target_inputs(cases.TRAIN_CASE)
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    try:
        n = _grad_check_against_oracle(_WithCalib(model, torch.from_numpy(CR.calib_matrices(rigs)).cuda()), ora, imgs, pts,
                                       radars if "radar" in modality else None, boxes, labels, gpu)
    finally:
        engine.set_conv_mode(old)
    assert n >= 100
    assert model.fusion.camera_proj[0].weight.grad.abs().sum() > 0
    assert model.camera_encoder.conv1.weight.grad.abs().sum() > 0


def test_graphed_detector_takes_the_calibration_as_a_graph_input(gpu):
    rigs_a, rigs_b = RG.frame_rigs(2), RG.frame_rigs(2, first_seed=2)
    _, model = _det_pair("camera+lidar+radar", 50, 50, rigs_a)
    model.eval()
    a, b = _frames(41), _frames(42)
    cu = lambda f: (f[0].cuda(), f[1].cuda(), [r.cuda() for r in f[2]])     # noqa: E731
    g = model.make_graphed(*cu(a), camera_calib=rigs_a)
    for inp, rigs in ((b, rigs_b), (a, rigs_a), (a, rigs_b)):
        gi = cu(inp)
        got = {k: v.clone() for k, v in g(*gi, camera_calib=rigs).items()}
        eager = model(*gi, camera_calib=rigs)
        for k in eager:
            assert torch.equal(got[k], eager[k]), k
    changed = model(*cu(a), camera_calib=rigs_a)
    assert not torch.equal(changed["heatmap"], got["heatmap"])           # (a, rigs_a) against (a, rigs_b): the calibration counts


@pytest.mark.parametrize("lidar", ["PointNet", "PointPillars"])
def test_bf16_per_frame_detector_against_fp32(gpu, lidar):
    rigs = RG.frame_rigs(2)
    _, m32 = _det_pair("camera+lidar+radar", 50, 50, rigs, lidar=lidar)
    m32.eval()
    m16 = copy.deepcopy(m32).bfloat16()
    with torch.no_grad():                                                # the fp32 model on the same bf16-rounded weights
        for p in list(m32.parameters()) + list(m32.buffers()):
            if p.dtype == torch.float32:
                p.copy_(p.bfloat16().float())
    imgs, pts, radars = _frames(43)
    if lidar == "PointPillars":
        pts = PR.pillar_points(2, 3000, 4, seed=43)
    o16 = m16(imgs.cuda(), pts.cuda(), [r.cuda() for r in radars], camera_calib=rigs)
    o32 = m32(imgs.cuda(), pts.cuda(), [r.cuda() for r in radars], camera_calib=rigs)
    s16 = m16(imgs.cuda(), pts.cuda(), [r.cuda() for r in radars])
    for k in o32:
        err = rel_err(o16[k].float().cpu(), o32[k].cpu())
        print(f"bf16 per-frame detector ({lidar}) {k}: rel err {err:.2e}")
        assert err <= 3e-2, k
    assert not torch.equal(s16["heatmap"], o16["heatmap"])
