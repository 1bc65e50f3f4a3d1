"""The opt-in lift-splat camera branch (camera_view_transform 'frustum') on the MI355X: the device-built frustum
tables against camera_rig.build_frustum_table integer for integer, the pool and its dense backward against the fp64 restatement of
tests/camera_frustum_ref.py and its autograd, FlexibleBEVFusion and the detector (eval and train, static rig and per-frame
calibration), hipGraph replay with the calibration as a graph input, and an augmented batch.  Parity unpinned by the reference,
which has no view transform.  The cases and their margin condition (no frustum point within 1e-9 m of a cell edge, so nothing is
excluded) are stated in camera_frustum_ref.py and checked on the CPU by tests/test_camera_frustum_host.py."""
import functools

import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import augment as A
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import engine, fusion, synth, training
from bevfusion_multimodal_3d_object_detection_amd.encoders import pillar_grid
from oracle import ref_model
from tests import augment_ref
from tests import camera_frustum_ref as FR
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
RANGE = FR.RANGE
MTOL = 1e-4                      # tests/test_gpu_camera_lift.py's module bound
GTOL = 2e-3                      # its gradient bound (+ a floor of 2e-6 of the gradient norm)
KTOL = 2e-6                      # the bound its lift kernel is held to at rows <= 64

# (case, frames = rig seeds, channels): C = 40 one vector per lane, 288 two, 520 three of four (the last partly filled)
POOL_CASES = [("A", 3, 40), ("B", 3, 288), ("B", 2, 520), ("L", 2, 32), ("L2", 2, 24)]
LONG = ("L", "L2")               # rows of thousands: the bound comes from a float32 accumulation in table order


class DeviceTables:
    """bevf_frustum_table_build_f64 for `rigs` through the _lib wrapper, into buffers pre-filled with junk."""

    def __init__(self, rigs, Hc, Wc, h, w, depth, calib=None):
        calib = torch.from_numpy(CR.calib_matrices(rigs)).cuda() if calib is None else calib
        self.B, self.ncam = calib.shape[:2]
        self.D, dmin, dmax = depth
        self.P, self.ncols = h * w, self.ncam * Hc * Wc
        self.cap = self.ncols * self.D
        i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device="cuda")                  # noqa: E731
        B = self.B
        self.cell_of, self.row_ptr, self.col2 = i32(B * self.cap), i32(B * (self.P + 1)), i32(B * self.cap)
        work = i32(L.frustum_table_work_elems(B, self.ncam, h, w, self.D, Hc, Wc))
        z = (float(np.float32(RANGE[2])), float(np.float32(RANGE[5])))
        L.frustum_table_build(calib, B, self.ncam, pillar_grid(RANGE, h, w)[:4], h, w, z, self.D, dmin, dmax, rigs[0].image_size, Hc, Wc,
                              self.cell_of, self.row_ptr, self.col2, work)

    def pool(self, x, pd, y, C, y_bs=None, y_cs=None, tables=None):
        L.frustum_pool(self.row_ptr, self.col2, tables or self.B, self.cap, self.P, self.ncols, self.D, x, self.ncols * C, C, pd,
                       self.ncols * self.D, y, y_bs or self.P * C, y_cs or C, x.shape[0], C)

    def pool_backward(self, x, pd, dy, dx, dpd, C, tables=None):
        L.frustum_pool_bwd(self.cell_of, tables or self.B, self.ncols, self.P, self.D, x, self.ncols * C, C, pd, self.ncols * self.D,
                           dy, self.P * C, C, dx, self.ncols * C, C, dpd, self.ncols * self.D, x.shape[0], C)


def _case(name, B):
    n, Hc, Wc, h, w, depth = FR.CASES[name]
    return [FR.case_rig(n, s) for s in range(B)], Hc, Wc, h, w, depth


# ---- the table ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", [("A", 3), ("B", 3), ("L", 2), ("L2", 2)])
def test_device_table_equals_the_host_table(gpu, name, B):
    rigs, Hc, Wc, h, w, depth = _case(name, B)
    dev = DeviceTables(rigs, Hc, Wc, h, w, depth)
    wave_rows = L.frustum_table_sort_wave_rows()
    longest = 0
    for b, rig in enumerate(rigs):
        t = CR.build_frustum_table(rig, Hc, Wc, RANGE, h, w, *depth)
        assert np.array_equal(dev.cell_of.view(B, -1)[b].cpu().numpy(), t.cell_of)
        assert np.array_equal(dev.row_ptr.view(B, -1)[b].cpu().numpy(), t.row_ptr)
        col2 = dev.col2.view(B, -1)[b].cpu().numpy()
        assert np.array_equal(col2[:t.nnz], t.col2)                               # every row ascending, integer for integer
        assert (col2[t.nnz:] == -7).all()                                         # nothing written past the frame's entries
        longest = max(longest, int(np.diff(t.row_ptr).max()))
    print(f"frustum table {name}: longest row {longest}, one wave sorts rows up to {wave_rows}")
    if name in LONG:                                                               # past the sort's only row-length threshold, and
        assert longest > wave_rows and longest > 1024                              # past one pass of the workgroup's 4 x 256 keys
    else:
        assert longest <= wave_rows
    if name == "L2":
        assert longest > 2048                                                      # more than one LDS tile of the long-row path
    again = DeviceTables(rigs, Hc, Wc, h, w, depth)                                # a second build: the same bits everywhere
    for a, b_ in ((dev.cell_of, again.cell_of), (dev.row_ptr, again.row_ptr), (dev.col2, again.col2)):
        assert torch.equal(a, b_)


def test_device_table_of_an_augmented_frame_equals_the_equivalent_rig(gpu):
    n, Hc, Wc, h, w, depth = FR.CASES["A"]
    base = FR.case_rig(n, 0)
    p = augment_ref.calib_params(2, n, seed=3)
    dev = DeviceTables([base, base], Hc, Wc, h, w, depth, calib=A.augmented_calib(base, p).cuda())
    for b, rig in enumerate(FR.augmented_rigs(base, p)):
        assert FR.margin(FR.frustum_points(rig, Hc, Wc, depth), RANGE, h, w) > FR.MARGIN
        t = CR.build_frustum_table(rig, Hc, Wc, RANGE, h, w, *depth)
        assert np.array_equal(dev.cell_of.view(2, -1)[b].cpu().numpy(), t.cell_of)
        assert np.array_equal(dev.col2.view(2, -1)[b].cpu().numpy()[:t.nnz], t.col2)


# ---- the pool and its backward -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(name, B, C):
    """Computed once per case and shared by the forward and the backward test: float32-representable inputs, the fp64 output and
    autograd gradients of frustum_ref, and -- for the long-row cases -- the errors against them of a numpy float32 accumulation
    in table order (forward) / in bin and channel order (backward) on the same inputs."""
    rigs, Hc, Wc, h, w, depth = _case(name, B)
    n, D = rigs[0].num_cameras, depth[0]
    g = torch.Generator().manual_seed(B * 1000 + C)
    feats = torch.randn(B, n, C, Hc, Wc, generator=g).double().requires_grad_()
    pd = torch.softmax(2 * torch.randn(B, n, D, Hc, Wc, generator=g, dtype=torch.float64), 2).float().double().requires_grad_()
    G = torch.randn(B, C, h, w, generator=g).double()
    out = FR.frustum_ref(feats, pd, rigs, RANGE, h, w, depth)
    (out * G).sum().backward()
    ref = dict(feats=feats.detach(), pd=pd.detach(), G=G, out=out.detach(), dfeats=feats.grad, dpd=pd.grad)
    if name in LONG:
        ref["f32_err"] = _float32_errors(rigs, Hc, Wc, h, w, depth, ref)
    return ref


def _nhwc(t):
    """(B, n, K, Hc, Wc) -> [B][n*Hc*Wc][K]."""
    B, _, K = t.shape[:3]
    return t.permute(0, 1, 3, 4, 2).reshape(B, -1, K).contiguous()


def _float32_errors(rigs, Hc, Wc, h, w, depth, ref):
    """rel_err against fp64 of numpy float32 arithmetic on the same inputs: (y accumulated entry by entry in table order, dx
    accumulated bin by bin, dPd accumulated channel by channel) -- product rounded, then the sum rounded, one entry at a time."""
    D = depth[0]
    x, p = _nhwc(ref["feats"]).numpy().astype(np.float32), _nhwc(ref["pd"]).numpy().astype(np.float32)
    dy = ref["G"].permute(0, 2, 3, 1).reshape(len(rigs), h * w, -1).numpy().astype(np.float32)
    B, ncols, C = x.shape
    y, dx, dpd = np.zeros((B, h * w, C), np.float32), np.zeros((B, ncols, C), np.float32), np.zeros((B, ncols, D), np.float32)
    for b, rig in enumerate(rigs):
        t = CR.build_frustum_table(rig, Hc, Wc, RANGE, h, w, *depth)
        rp, lens = t.row_ptr.astype(np.int64), np.diff(t.row_ptr)
        for k in range(int(lens.max())):                                          # the k-th entry of every row that has one
            rows = np.nonzero(lens > k)[0]
            c2 = t.col2[rp[rows] + k]
            y[b, rows] = y[b, rows] + p[b].reshape(-1)[c2][:, None] * x[b, c2 // D]
        cell = t.cell_of.reshape(ncols, D)
        for d in range(D):
            pix = np.nonzero(cell[:, d] >= 0)[0]
            g = dy[b, cell[pix, d]]
            dx[b, pix] = dx[b, pix] + p[b, pix, d][:, None] * g
            dot = np.zeros(pix.shape[0], np.float32)
            for c in range(C):
                dot = dot + x[b, pix, c] * g[:, c]
            dpd[b, pix, d] = dot
    want_y = ref["out"].permute(0, 2, 3, 1).reshape(B, h * w, C)
    return rel_err(y, want_y), rel_err(dx, _nhwc(ref["dfeats"])), rel_err(dpd, _nhwc(ref["dpd"]))


@pytest.mark.parametrize("name,B,C", POOL_CASES)
def test_pool_against_fp64(gpu, name, B, C):
    rigs, Hc, Wc, h, w, depth = _case(name, B)
    ref = _reference(name, B, C)
    dev = DeviceTables(rigs, Hc, Wc, h, w, depth)
    x, p = _nhwc(ref["feats"]).float().cuda(), _nhwc(ref["pd"]).float().cuda()
    # strided slice: C columns at offset C of a 3C-wide map, the rest must stay untouched; empty rows come out as zeros
    y = torch.full((B, dev.P, 3 * C), 7.0, device=gpu)
    dev.pool(x, p, y.view(-1)[C:], C, dev.P * 3 * C, 3 * C)
    got = y[:, :, C:2 * C].cpu()
    err = rel_err(got.view(B, h, w, C).permute(0, 3, 1, 2), ref["out"])
    bound = 4 * ref["f32_err"][0] if name in LONG else KTOL
    print(f"frustum_pool {name} B={B} C={C}: rel err {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    assert (y[:, :, :C] == 7.0).all() and (y[:, :, 2 * C:] == 7.0).all()
    empty = dev.row_ptr.view(B, -1).diff(dim=1).cpu() == 0
    assert empty.any() and (got[empty] == 0).all()
    y2 = torch.full_like(y, -3.0)
    dev.pool(x, p, y2.view(-1)[C:], C, dev.P * 3 * C, 3 * C)
    assert torch.equal(y2[:, :, C:2 * C], y[:, :, C:2 * C])                 # two launches: identical bits


@pytest.mark.parametrize("name,C", [("A", 40), ("L", 32)])
def test_shared_table_equals_the_same_table_per_frame(gpu, name, C):
    """Stride 0 (one table for every frame: the static rig) against the same table repeated per frame: the same bits, forward and
    backward."""
    rigs, Hc, Wc, h, w, depth = _case(name, 1)
    B = 3
    one, rep = DeviceTables(rigs, Hc, Wc, h, w, depth), DeviceTables(rigs * B, Hc, Wc, h, w, depth)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, one.ncols, C, generator=g).cuda()
    p = torch.softmax(torch.randn(B, one.ncols, one.D, generator=g), -1).cuda()
    dy = torch.randn(B, one.P, C, generator=g).cuda()
    ya, yb = torch.full((B, one.P, C), 5.0, device=gpu), torch.full((B, one.P, C), -5.0, device=gpu)
    one.pool(x, p, ya, C, tables=1)
    rep.pool(x, p, yb, C)
    assert torch.equal(ya, yb) and float(ya.abs().max()) > 0
    outs = []
    for tab, tables in ((one, 1), (rep, None)):
        dx, dpd = torch.full_like(x, float("nan")), torch.full_like(p, float("nan"))
        tab.pool_backward(x, p, dy, dx, dpd, C, tables=tables)
        outs.append((dx, dpd))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.isfinite(outs[0][0]).all()


@pytest.mark.parametrize("name,B,C", POOL_CASES)
def test_pool_backward_against_fp64_autograd(gpu, name, B, C):
    rigs, Hc, Wc, h, w, depth = _case(name, B)
    ref = _reference(name, B, C)
    dev = DeviceTables(rigs, Hc, Wc, h, w, depth)
    D = dev.D
    x, p = _nhwc(ref["feats"]).float().cuda(), _nhwc(ref["pd"]).float().cuda()
    dy = ref["G"].permute(0, 2, 3, 1).reshape(-1).float().contiguous().cuda()
    dx = torch.full((B * dev.ncols * C,), float("nan"), device=gpu)          # every element must be written
    dpd = torch.full((B * dev.ncols * D,), float("nan"), device=gpu)
    dev.pool_backward(x, p, dy, dx, dpd, C)
    got_dx, got_dpd = dx.view(B, dev.ncols, C).cpu(), dpd.view(B, dev.ncols, D).cpu()
    assert torch.isfinite(got_dx).all() and torch.isfinite(got_dpd).all()
    e1, e2 = rel_err(got_dx, _nhwc(ref["dfeats"])), rel_err(got_dpd, _nhwc(ref["dpd"]))
    b1, b2 = (4 * ref["f32_err"][1], 4 * ref["f32_err"][2]) if name in LONG else (KTOL, KTOL)
    print(f"frustum_pool_bwd {name} B={B} C={C}: dx rel err {e1:.2e} (bound {b1:.2e}), dPd rel err {e2:.2e} (bound {b2:.2e})")
    assert e1 <= b1 and e2 <= b2
    invalid = dev.cell_of.view(B, dev.ncols, D).cpu() < 0
    assert invalid.any() and (got_dpd[invalid] == 0).all()                  # exactly 0 for invalid bins
    dead = invalid.all(-1)                                                  # pixels none of whose bins lands on the grid
    assert (got_dx[dead] == 0).all()
    dx2, dpd2 = torch.empty_like(dx), torch.empty_like(dpd)
    dev.pool_backward(x, p, dy, dx2, dpd2, C)
    assert torch.equal(dx, dx2) and torch.equal(dpd, dpd2)                  # two launches: identical bits


# ---- FlexibleBEVFusion -----------------------------------------------------------------------------------------------------------

def _fusion_pair(modality, rigs, seed=5):
    """(fp64 oracle pooling frame b through rigs[b] -- or through the one rig --, device module whose own rig is rigs / rigs[0])."""
    n, _, _, h, w, depth = FR.MODULE_CASE
    m = modality.replace(" ", "")
    cam, lid, rad = "camera" in m, "lidar" in m, "radar" in m
    ora = FR.frustum_lifting(ref_model.BEVFusion(cam, lid, rad, bev_h=h, bev_w=w), rigs, RANGE, depth)
    synth.fill_state_dict_(ora, seed)
    fus = fusion.FlexibleBEVFusion(use_camera=cam, use_lidar=lid, use_radar=rad, bev_h=h, bev_w=w, pc_range=list(RANGE),
                                   camera_view_transform="frustum")
    fus.set_camera_rig(rigs if isinstance(rigs, CR.CameraRig) else rigs[0])
    fus.load_state_dict(ora.state_dict())
    return ora.double(), fus.to("cuda")


def _features(B, seed=9):
    n, Hc, Wc = FR.MODULE_CASE[:3]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, 512, Hc, Wc, generator=g), torch.randn(B, 1024, generator=g)


def _module_rigs(B, first=0):
    return [FR.case_rig(FR.MODULE_CASE[0], first + b) for b in range(B)]


def test_fusion_eval_static_rig_and_per_frame_against_fp64(gpu):
    cam, lid = _features(2)
    rig = _module_rigs(1, 2)[0]
    ora, fus = _fusion_pair("camera+lidar", rig)
    ora.eval(), fus.eval()
    static = fus(cam.cuda(), lid.cuda()).clone()
    with torch.no_grad():
        want = ora(cam.double(), lid.double())
    err = rel_err(static.cpu(), want)
    print(f"fusion(frustum) eval, static rig: rel err {err:.2e}")
    assert static.shape == (2, 256, 20, 20) and err <= MTOL
    # the same rig for every frame, in each accepted form: the static path's bits
    for calib in ([rig, rig], torch.from_numpy(CR.calib_matrices([rig, rig])), torch.from_numpy(CR.calib_matrices([rig, rig])).cuda()):
        assert torch.equal(fus(cam.cuda(), lid.cuda(), camera_calib=calib), static)
    # two different rigs in one batch
    rigs = _module_rigs(2)
    ora.frame_rigs = rigs
    out = fus(cam.cuda(), lid.cuda(), camera_calib=rigs).clone()
    with torch.no_grad():
        want = ora(cam.double(), lid.double())
    err = rel_err(out.cpu(), want)
    print(f"fusion(frustum) eval, one rig per frame: rel err {err:.2e}")
    assert err <= MTOL and rel_err(out.cpu(), static.cpu()) > 100 * MTOL
    assert torch.equal(fus(cam.cuda(), lid.cuda()), static)                 # the static table is untouched by the per-frame ones
    with pytest.raises(L.BevfError, match="3 cameras"):
        fus(torch.randn(1, 4, 512, 6, 10).cuda(), lid[:1].cuda())
    fus.set_camera_rig(rigs[1])                                              # a new rig drops the cached table
    assert rel_err(fus(cam.cuda(), lid.cuda())[1].cpu(), out[1].cpu()) == 0.0


def test_fusion_train_mode_per_frame_parameter_and_camera_gradients(gpu):
    """The oracle takes the device's ReLU decisions (tests/test_gpu_training._ReluReplay), as the detector-level gradient checks do:
    an activation within rounding of zero is otherwise decided twice, once in fp32 and once in fp64, and one such flip moves every
    upstream gradient by a few 1e-3 (measured here at seed 17: camera gradient 3.2e-3 apart with the decisions taken separately,
    2.5e-6 with them shared; seeds 18 and 19 have no flip and are 1e-6 apart either way)."""
    from tests.test_gpu_training import _ReluReplay
    rigs = _module_rigs(2)
    ora, fus = _fusion_pair("camera+lidar", rigs, seed=17)
    ora.train(), fus.train()
    cam, lid = _features(2, seed=4)
    G = torch.randn(2, 256, 20, 20, generator=torch.Generator().manual_seed(8))
    cam_d, lid_d = cam.cuda().requires_grad_(), lid.cuda().requires_grad_()
    trace = []
    training.RELU_TRACE = trace
    try:
        out = fus(cam_d, lid_d, camera_calib=rigs)
    finally:
        training.RELU_TRACE = None
    with torch.no_grad():                       # another forward with another calibration before the backward: the tape rebuilds its tables
        fus(cam.cuda(), lid.cuda(), camera_calib=_module_rigs(2, 1))
    (out * G.cuda()).sum().backward()
    cam_r, lid_r = cam.double().requires_grad_(), lid.double().requires_grad_()
    with _ReluReplay(trace) as rp:
        want = ora(cam_r, lid_r)
    assert not rp.misses and rp.hits >= 7, (rp.hits, rp.misses[:5])        # every oracle ReLU found its device counterpart
    (want * G.double()).sum().backward()
    assert rel_err(out.detach().cpu(), want.detach()) <= MTOL
    assert cam_d.grad is not None and cam_d.grad.shape == cam.shape
    e = rel_err(cam_d.grad.cpu(), cam_r.grad)
    print(f"fusion(frustum) train, per-frame calibration: camera gradient rel err {e:.2e}")
    assert e <= GTOL
    gref = dict(ora.named_parameters())
    gn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in ora.parameters())))
    seen = []
    for n, p in fus.named_parameters():
        if not n.startswith(("camera_proj.", "depth_net.")):
            continue
        r = gref[n].grad
        d = float((p.grad.cpu().double() - r).abs().max())
        print(f"  {n}: err {d:.2e} of max {float(r.abs().max()):.2e}")
        assert d <= GTOL * float(r.abs().max()) + 2e-6 * gn, n
        seen.append(n)
    assert "depth_net.weight" in seen and "depth_net.bias" in seen and float(fus.depth_net.weight.grad.abs().sum()) > 0
    r = gref["depth_net.weight"].grad
    assert float((fus.depth_net.weight.grad.cpu().double() - r).abs().max()) <= GTOL * float(r.abs().max())     # without the floor


# ---- the detector (2 frames of 2 cameras 64 x 96, BEV 50 x 50) ----------------------------------------------------------------------

def _det_pair(modality, rigs, seed=11):
    n, _, _, h, w, depth = FR.DETECTOR_CASE
    ora = ref_model.make_detector(modality, h, w)
    FR.frustum_lifting(ora.fusion, rigs, RANGE, depth)
    synth.fill_state_dict_(ora, seed)
    model = fusion.create_detector(modality, "bev", "centernet", bev_h=h, bev_w=w, camera_view_transform="frustum")
    model.fusion.set_camera_rig(rigs if isinstance(rigs, CR.CameraRig) else rigs[0])
    model.load_state_dict(ora.state_dict())
    return ora, model.to("cuda")


def _det_rigs(B, first=0):
    return [FR.case_rig(FR.DETECTOR_CASE[0], first + b) for b in range(B)]


def _frames(seed, radars=0):
    return synth.frame_inputs(2, 2, 64, 96, 300, 4, radars, 20, 7, seed=seed)


def test_detector_eval_static_rig_and_per_frame_against_fp64(gpu):
    rigs = _det_rigs(2)
    ora, model = _det_pair("camera+lidar", rigs[0])
    ora = ora.double().eval()
    model.eval()
    imgs, pts, _ = _frames(7)
    for calib in (None, rigs):
        ora.fusion.frame_rigs = rigs[0] if calib is None else rigs
        out = model(imgs.cuda(), pts.cuda(), None, camera_calib=calib)
        with torch.no_grad():
            want = ora(imgs.double(), pts.double(), None)
        for k, v in want.items():
            err = rel_err(out[k].cpu(), v)
            print(f"detector(frustum, {'static rig' if calib is None else 'per-frame calibration'}) {k}: rel err {err:.2e}")
            assert err <= MTOL, (k, err)


class _WithCalib:
    """A detector called with a fixed camera_calib (for helpers that call model(imgs, pts, radars))."""

    def __init__(self, model, calib):
        self.model, self.calib = model, calib

    def __call__(self, imgs, pts, radars):
        return self.model(imgs, pts, radars, camera_calib=self.calib)

    def __getattr__(self, name):
        return getattr(self.model, name)


def test_detector_train_per_frame_gradients_against_fp64_autograd(gpu):
    """One training step with per-frame calibration: every parameter's gradient -- depth_net, camera_proj and the camera encoder
    upstream of the pool among them -- against the oracle's fp64 autograd with the device's ReLU decisions replayed."""
    from tests.golden import cases
    from tests.test_gpu_training import _grad_check_against_oracle
    rigs = _det_rigs(2)
    ora, model = _det_pair("camera+lidar", rigs, seed=77)
    ora.train(), model.train()
    imgs, pts, _ = synth.frame_inputs(2, 2, 64, 96, 200, 4, 0, 20, 7, seed=123)
    boxes, labels = cases.target_inputs(cases.TRAIN_CASE)
    old = engine.conv_mode()
    engine.set_conv_mode("f32")
    try:
        n = _grad_check_against_oracle(_WithCalib(model, torch.from_numpy(CR.calib_matrices(rigs)).cuda()), ora, imgs, pts, None, boxes,
                                       labels, gpu, tol=GTOL)
    finally:
        engine.set_conv_mode(old)
    assert n >= 100
    for p in (model.fusion.depth_net.weight, model.fusion.depth_net.bias, model.fusion.camera_proj[0].weight, model.camera_encoder.conv1.weight):
        assert float(p.grad.abs().sum()) > 0


def test_graphed_detector_takes_the_calibration_as_a_graph_input(gpu):
    rigs_a, rigs_b = _det_rigs(2), _det_rigs(2, 1)
    _, model = _det_pair("camera+lidar+radar", rigs_a)
    model.eval()
    a, b = _frames(41, 5), _frames(42, 5)
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
    gs = model.make_graphed(*cu(a))                                        # and without one: the static rig's table, cached before the capture
    static = {k: v.clone() for k, v in gs(*cu(b)).items()}
    eager = model(*cu(b))
    for k in eager:
        assert torch.equal(static[k], eager[k]), k


def test_augmented_batch_through_a_frustum_detector_matches_the_oracle(gpu):
    """augment_batch's images and camera_calib through the detector in eval mode against the oracle that pools every frame through
    the rig that sees the augmented frame (K' = A . K, cam_to_bev' = T . cam_to_bev)."""
    n = FR.DETECTOR_CASE[0]
    st = A.AugmentSettings(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, camera_flip=True, camera_scale=(0.9, 1.1), flip=True,
                           scale=(0.95, 1.05), rotation=(-20.0, 20.0), translation=(0.5, 0.5, 0.2))
    p = augment_ref.calib_params(2, n, (120, 200), (64, 96), 5)
    p.jitter = A.sample(st, 2, n, (120, 200), (64, 96), np.random.default_rng(5)).jitter
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (2, n, 120, 200, 3), dtype=np.uint8)).cuda()
    _, pts, _ = synth.frame_inputs(2, 0, 0, 0, 3000, 4, seed=5)
    base = FR.case_rig(n, 0)
    o = A.augment_batch(frames, pts.cuda(), None, None, None, None, None, p, st, base_calib=base, max_points=2048)
    ora, model = _det_pair("camera+lidar", FR.augmented_rigs(base, p))
    model.fusion.set_camera_rig(base)
    ora = ora.double().eval()
    model.eval()
    out = model(o["camera_imgs"], o["lidar_points"], None, camera_calib=o["camera_calib"])
    with torch.no_grad():
        want = ora(o["camera_imgs"].cpu().double(), o["lidar_points"].cpu().double(), None)
    for k, v in want.items():
        err = rel_err(out[k].cpu(), v)
        print(f"detector(frustum) on an augmented batch {k}: rel err {err:.2e}")
        assert err <= MTOL, (k, err)
    plain = model(o["camera_imgs"], o["lidar_points"], None)
    assert not torch.equal(plain["heatmap"], out["heatmap"])                # the augmented calibration reaches the pool
