"""Each kernel of the sparse-voxel LiDAR encoder on the MI355X against its own exact or fp64 reference (tests/sparse_kernel_ref.py),
called through its `_lib.sparse_*` wrapper: DESIGN.md 3.2b3, "kernel-level pins".  tests/test_gpu_sparse_lidar.py sees these kernels
only through the whole encoder on geometric scenes; here every one meets the layouts, widths and table patterns listed in the
reference file, whose properties tests/test_sparse_kernels_host.py asserts on the CPU.

Conventions: every output buffer is prefilled with a sentinel (-7.0, NaN, or -12345) and whatever the kernel must not write is
compared bit for bit afterwards; inactive slots of float inputs, and the rows of x that no active table entry names, hold NaN; the
table rows of inactive slots name such NaN rows.  No index ever points outside a buffer.

Tolerances: integers, copies and the mean VFE are exact.  The three gather-GEMM uses are held against fp64 with
e_dev <= 4 * e_yard, e_yard being the error of the same sum accumulated sequentially in fp32 on the CPU (the host file shows that
one dropped term is more than 100 x that bound).  BatchNorm statistics: 2 ulp on the fp32 roundings of fp64 results; the
elementwise BatchNorm kernels 2e-6 (the figure of the elementwise pins in test_gpu_glue.py)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import engine
from tests import sparse_kernel_ref as K
from tests import sparse_scenes as S
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
YARD_FACTOR = 4
ELEMENTWISE = 2e-6
NAN = float("nan")
I32 = torch.int32
PAIRS = [(ci, co) for ci in K.WIDTHS for co in K.WIDTHS]


def _bits(t):
    return t.contiguous().view(I32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def filled(n, value, dtype=torch.float32):
    return torch.full((n,), value, dtype=dtype, device="cuda")


def ints(n, value=K.INT_SENTINEL):
    return filled(n, value, I32)


def _yard_check(tag, got, yard, want):
    e_dev, e_yard = rel_err(got, want), rel_err(yard, want)
    print(f"{tag}: device rel_err {e_dev:.3e}, sequential fp32 on the CPU {e_yard:.3e}, ratio {e_dev / max(e_yard, 1e-30):.2f}")
    assert e_dev <= YARD_FACTOR * e_yard, (tag, e_dev, e_yard)


# ---- structure kernels (exact) ---------------------------------------------------------------------------------------------------

def test_fill_index(gpu):
    coords, count = K.fill_index_case()
    B, cap, dims = K.FILL["B"], K.FILL["cap"], K.FILL["dims"]
    index, cell = ints(B * dims[0] * dims[1] * dims[2], 777), ints(B * cap)          # garbage: the call memsets the volume itself
    L.sparse_fill_index(coords.cuda(), count.cuda(), B, cap, *dims, index, cell)
    want_index, want_cell = K.fill_index_ref(coords, count, B, cap, dims)
    assert torch.equal(index.cpu().view(want_index.shape), want_index)
    assert torch.equal(cell.cpu(), want_cell)                                         # (inactive slots: the sentinel)


@pytest.mark.parametrize("cap_binds", [False, True])
@pytest.mark.parametrize("dims", list(K.DOWN_DIMS))
def test_down(gpu, dims, cap_binds):
    index_in, cap = K.down_case(dims, cap_binds)
    B, cells_o = 4, dims[0] * dims[1] * dims[2] // 8
    index_out, cell_out, count_out = ints(B * cells_o), ints(B * cap), ints(B)
    work = filled(L.sparse_down_work_bytes(B, *dims), 0xAB, torch.uint8)
    L.sparse_down(index_in.cuda(), B, *dims, cap, index_out, cell_out, count_out, work)
    wi, wc, wn = K.down_ref(index_in, B, dims, cap)
    assert torch.equal(count_out.cpu(), wn)
    assert torch.equal(index_out.cpu().view(wi.shape), wi)
    assert torch.equal(cell_out.cpu(), wc)                                            # beyond each frame's count: the sentinel
    if cap_binds:
        assert wn[0] == cap and wn[2] == cap


_STRUCT = {}


def _device_structure():
    """The structure case built by the device kernels (once): fill_index -> down -> the four tables."""
    if not _STRUCT:
        s = K.STRUCT
        B, d0, d1, cap0, cap1 = s["B"], s["dims0"], s["dims1"], s["cap0"], s["cap1"]
        coords, count0 = K.structure_coords()
        count0 = count0.cuda()
        index0, cell0 = ints(B * d0[0] * d0[1] * d0[2], 777), ints(B * cap0)
        L.sparse_fill_index(coords.cuda(), count0, B, cap0, *d0, index0, cell0)
        index1, cell1, count1 = ints(B * d1[0] * d1[1] * d1[2]), ints(B * cap1), ints(B)
        L.sparse_down(index0, B, *d0, cap1, index1, cell1, count1, filled(L.sparse_down_work_bytes(B, *d0), 0xAB, torch.uint8))
        tabs = {}
        for (stride, tr), (idx, cell, count, cap, di, dr) in {
                (1, False): (index0, cell0, count0, cap0, d0, d0), (2, False): (index0, cell1, count1, cap1, d0, d1),
                (2, True): (index1, cell0, count0, cap0, d1, d0), (1, True): (index0, cell0, count0, cap0, d0, d0)}.items():
            t = ints(B * cap * 27)
            L.sparse_table(idx, cell, count, B, cap, di, dr, stride, tr, t)
            tabs[(stride, tr)] = t.cpu().view(-1, 27)
        _STRUCT.update(index0=index0.cpu(), cell0=cell0.cpu(), index1=index1.cpu(), cell1=cell1.cpu(), count1=count1.cpu(), tables=tabs)
    return _STRUCT


def test_structure_and_tables(gpu):
    dev, ref = _device_structure(), K.structure_ref()
    for k in ("index0", "cell0", "index1", "cell1", "count1"):
        assert torch.equal(dev[k].flatten(), ref[k].flatten()), k
    for mode, t in dev["tables"].items():
        assert torch.equal(t, ref["tables"][mode]), mode                              # inactive slots: the sentinel; cell -1: all -1
    s = K.STRUCT
    act0, act1 = K.active_mask(ref["count0"], s["B"], s["cap0"]), K.active_mask(ref["count1"], s["B"], s["cap1"])
    assert K.inverse_relation(dev["tables"][(2, False)], act1, dev["tables"][(2, True)], act0)
    assert K.inverse_relation(dev["tables"][(1, False)], act0, dev["tables"][(1, True)], act0)


# ---- mean VFE (bit-exact) ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("C", [3, 4, 5])
def test_vfe_mean(gpu, C, P):
    feats, npts, nvox = K.vfe_case(C, P)
    B, Nv, Cpad = K.VFE["B"], K.VFE["Nv"], K.VFE["Cpad"]
    rows = filled(B * Nv * Cpad, NAN)
    L.sparse_vfe_mean(feats.cuda(), npts.cuda(), nvox.cuda(), B, Nv, P, C, Cpad, rows)
    want = K.vfe_mean_ref(feats, npts, nvox, B, Nv, P, C, Cpad, fill=NAN)
    got = rows.cpu().view(B * Nv, Cpad)
    act = K.active_mask(nvox, B, Nv)
    assert torch.equal(got[act], want[act]) and same_bits(got[act][:, :C], want[act][:, :C])
    assert not got[act][:, C:].any() and same_bits(got[~act], want[~act])             # pad channels exactly 0, inactive slots still NaN
    for r, v in K.VFE["special"].items():
        if v in (0, -1):
            assert not got[r].any()


# ---- sparse_conv, forward ----------------------------------------------------------------------------------------------------------------

_YARD = {}


def _conv_reference(layout, Cin, Cout):
    """(fp64 raw sums, sequential fp32 raw sums) of a forward case, computed once."""
    key = (layout, Cin, Cout)
    if key not in _YARD:
        t, c = K.synth_table(layout), K.conv_inputs(layout, Cin, Cout)
        _YARD[key] = (K.gather_gemm(c["x"], t["table"], t["active"], c["w"], Cin, Cout),
                      K.gather_gemm_seq32(c["x"], t["table"], t["active"], c["w"], Cin, Cout))
    return _YARD[key]


def _launch_conv(t, table, c, Cin, Cout, scale, shift, relu, rows_in=K.ROWS_IN, x=None, w=None):
    R = t["B"] * t["cap"]
    y = filled(R * Cout, K.FLOAT_SENTINEL)
    L.sparse_conv((c["x"] if x is None else x).cuda(), table.cuda(), t["count"].cuda(), (c["w"] if w is None else w).cuda(),
                  None if scale is None else scale.cuda(), None if shift is None else shift.cuda(), t["B"], t["cap"], rows_in, Cin, Cout,
                  relu, y)
    return y.cpu().view(R, Cout)


def _check_conv(layout, Cin, Cout, epilogues):
    t, c = K.synth_table(layout), K.conv_inputs(layout, Cin, Cout)
    act = t["active"]
    want_raw, yard_raw = _conv_reference(layout, Cin, Cout)
    for use_scale, use_shift, relu in epilogues:
        scale, shift = c["scale"] if use_scale else None, c["shift"] if use_shift else None
        got = _launch_conv(t, t["table"], c, Cin, Cout, scale, shift, relu)
        assert (got[~act] == K.FLOAT_SENTINEL).all()                                  # inactive slots untouched
        _yard_check(f"sparse_conv {layout} ({Cin}, {Cout}) scale={use_scale} shift={use_shift} relu={relu}", got[act],
                    K.epilogue(yard_raw, scale, shift, relu)[act], K.epilogue(want_raw, scale, shift, relu)[act])
        for r in K.NO_NEIGHBOUR:                                                      # an all-absent row: exactly relu(shift), or 0
            assert torch.equal(got[r], K.epilogue(torch.zeros(Cout), None, shift, relu))
        if not (use_scale or use_shift or relu):
            assert same_bits(_launch_conv(t, t["table"], c, Cin, Cout, None, None, False), got)      # determinism
            perm, ptab = K.slot_permutation(t)                                        # a row's result depends on its own table row only
            moved = _launch_conv(t, ptab, c, Cin, Cout, None, None, False)
            assert torch.equal(moved[perm[act]], got[act])
            assert (moved[~act] == K.FLOAT_SENTINEL).all()


ALL_EPILOGUES = [(False, False, False), (True, True, True), (True, False, False), (False, True, True)]


@pytest.mark.parametrize("Cin,Cout", PAIRS)
def test_conv_forward_widths(gpu, Cin, Cout):
    _check_conv("straddle", Cin, Cout, ALL_EPILOGUES if (Cin, Cout) in ((64, 64), (96, 128)) else [(True, True, True), (False, False, False)])


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (128, 96)])
@pytest.mark.parametrize("layout", [n for n in K.CONV_LAYOUTS if n != "straddle"])
def test_conv_forward_layouts(gpu, layout, Cin, Cout):
    _check_conv(layout, Cin, Cout, [(True, True, True), (False, False, False)])


# ---- sparse_conv as the data gradient --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cin,Cout", [(32, 64), (64, 96), (128, 128)])
@pytest.mark.parametrize("stride", [2, 1])
def test_conv_data_gradient(gpu, stride, Cin, Cout):
    dev, ref, s = _device_structure(), K.structure_ref(), K.STRUCT
    B, cap_i = s["B"], s["cap0"]
    cap_o, count_o = (s["cap1"], ref["count1"]) if stride == 2 else (s["cap0"], ref["count0"])
    act_i, act_o = K.active_mask(ref["count0"], B, cap_i), K.active_mask(count_o, B, cap_o)
    t_f = dev["tables"][(stride, False)]
    t_g = dev["tables"][(2, True)] if stride == 2 else t_f                            # submanifold: the forward table, mirrored taps
    assert torch.equal(t_f, ref["tables"][(stride, False)]) and torch.equal(t_g[act_i], ref["tables"][(2, True) if stride == 2 else (1, False)][act_i])
    g = torch.Generator().manual_seed(100 * stride + Cin)
    conv = nn.Conv3d(Cin, Cout, 3, stride=stride, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(0.1 * torch.randn(conv.weight.shape, generator=g))
    dy = torch.randn(B * cap_o, Cout, generator=g)
    dy[~act_o] = NAN
    dy0 = torch.where(act_o[:, None], dy, torch.zeros(())).double()
    x = torch.randn(B * cap_i, Cin, generator=g, dtype=torch.float64).requires_grad_()
    K.gather_gemm(x, t_f, act_o, engine.sparse_pack_weight(conv).double(), Cin, Cout).backward(dy0)
    wt = engine.sparse_pack_weight(conv, transposed=True)
    # inactive slots of the table name a NaN row of dy (frame 2 is empty at both levels)
    tab = t_g.clone()
    tab[~act_i] = 2 * cap_o
    assert not act_o[2 * cap_o]
    t = dict(B=B, cap=cap_i, count=ref["count0"])
    got = _launch_conv(t, tab, None, Cout, Cin, None, None, False, rows_in=B * cap_o, x=dy, w=wt)
    assert (got[~act_i] == K.FLOAT_SENTINEL).all()
    yard = K.gather_gemm_seq32(dy, t_g, act_i, wt, Cout, Cin)
    _yard_check(f"sparse_conv data gradient stride {stride} ({Cin} -> {Cout})", got[act_i], yard[act_i], x.grad[act_i])
    lost = (ref["cell0"] == -1).nonzero().flatten()
    if stride == 2:
        assert not got[lost].any()                                                    # the row outside the grid reaches no output


# ---- sparse_conv_wgrad -----------------------------------------------------------------------------------------------------------------

def _check_wgrad(layout, Cin, Cout, cin_real):
    t, c = K.synth_table(layout, wgrad=True), K.conv_inputs(layout, Cin, Cout, wgrad=True)
    act, n = t["active"], Cout * cin_real * 27
    assert torch.isfinite(c["x"][t["named"]][:, cin_real:]).all() and (c["x"][t["named"]][:, cin_real:] != 0).all()

    def launch():
        dw = filled(n + 100, K.FLOAT_SENTINEL)
        work = filled(L.sparse_wgrad_work_floats(Cin, Cout), NAN)
        L.sparse_conv_wgrad(c["x"].cuda(), c["dy"].cuda(), t["table"].cuda(), t["count"].cuda(), t["B"], t["cap"], K.ROWS_IN, Cin, Cout,
                            cin_real, dw, work)
        return dw.cpu()

    got = launch()
    assert (got[n:] == K.FLOAT_SENTINEL).all()                                        # nothing past Cout * cin_real * 27
    w = c["w"].double().requires_grad_()
    K.gather_gemm(c["x"], t["table"], act, w, Cin, Cout).backward(torch.where(act[:, None], c["dy"], torch.zeros(())).double())
    want = K.dw_torch_layout(w.grad, Cin, Cout, cin_real)
    yard = K.dw_torch_layout(K.wgrad_seq32(c["x"], c["dy"], t["table"], act, Cin, Cout), Cin, Cout, cin_real)
    _yard_check(f"sparse_conv_wgrad {layout} ({Cin}, {Cout}) cin_real={cin_real}", got[:n], yard, want)
    assert not got[:n].view(Cout, cin_real, 27)[..., 13].any()                        # the tap no row has: exactly 0
    assert same_bits(launch(), got)


@pytest.mark.parametrize("Cin,Cout", PAIRS)
def test_wgrad_widths(gpu, Cin, Cout):
    _check_wgrad("straddle", Cin, Cout, Cin)


@pytest.mark.parametrize("cin_real", [4, 5])
@pytest.mark.parametrize("Cin,Cout", [(32, 32), (32, 64)])
def test_wgrad_cin_real(gpu, Cin, Cout, cin_real):
    _check_wgrad("straddle", Cin, Cout, cin_real)


@pytest.mark.parametrize("Cin,Cout", [(32, 64), (128, 96)])
@pytest.mark.parametrize("layout", ["three-rounds", "one-ragged"])
def test_wgrad_layouts(gpu, layout, Cin, Cout):
    _check_wgrad(layout, Cin, Cout, Cin)


# ---- BatchNorm row kernels -----------------------------------------------------------------------------------------------------------

EPS = float(np.float32(1e-5))                  # eps and momentum are float arguments of the entry point: the reference gets the same values
MOM = float(np.float32(0.1))


def _bn_stats(c, C, momentum, nbt0):
    rmean, rvar, nbt = c["rmean"].cuda(), c["rvar"].cuda(), torch.tensor([nbt0], device="cuda")
    mean, invstd, nrows = filled(C, NAN), filled(C, NAN), ints(1)
    work = filled(L.sparse_bn_work_bytes(C), 0xFF, torch.uint8)                       # (NaN doubles)
    L.sparse_bn_stats(c["y"].cuda(), c["count"].cuda(), c["B"], c["cap"], C, EPS, -1.0 if momentum is None else momentum, rmean, rvar,
                      nbt, mean, invstd, nrows, work)
    return mean.cpu(), invstd.cpu(), rmean.cpu(), rvar.cpu(), int(nbt), int(nrows)


@pytest.mark.parametrize("momentum", [MOM, None], ids=["momentum-0.1", "cumulative"])
@pytest.mark.parametrize("layout", ["straddle", "long"])
@pytest.mark.parametrize("C", K.WIDTHS)
def test_bn_stats(gpu, C, layout, momentum):
    c = K.bn_rows_case(layout, C)
    ref = K.bn_rows_ref(c["y"], c["active"], None, None, EPS, momentum, c["rmean"], c["rvar"], 3)
    mean, invstd, rmean, rvar, nbt, nrows = _bn_stats(c, C, momentum, 3)
    u = {k: K.ulps(v, ref[k]) for k, v in dict(mean=mean, invstd=invstd, rmean=rmean, rvar=rvar).items()}
    print(f"sparse_bn_stats C={C} {layout} momentum={momentum}: ulps {u}")
    assert max(u.values()) <= 2 and nbt == ref["nbt"] == 4 and nrows == ref["N"]


def test_bn_stats_large_mean(gpu):
    C = 32
    c = K.bn_rows_case("straddle", C, offset=1000.0)
    ref = K.bn_rows_ref(c["y"], c["active"], None, None, EPS, MOM, c["rmean"], c["rvar"], 0)
    mean, invstd, rmean, rvar, nbt, nrows = _bn_stats(c, C, MOM, 0)
    e = float(((invstd.double() - ref["invstd"]) / ref["invstd"]).abs().max())
    print(f"sparse_bn_stats large mean: invstd relative error {e:.2e}, mean ulps {K.ulps(mean, ref['mean'])}")
    assert e <= 1e-5 and K.ulps(mean, ref["mean"]) <= 2 and K.ulps(rmean, ref["rmean"]) <= 2 and nbt == 1 and nrows == 329
    assert float(((rvar.double() - ref["rvar"]) / ref["rvar"]).abs().max()) <= 1e-5


@pytest.mark.parametrize("C", K.WIDTHS)
def test_bn_stats_few_rows(gpu, C):
    c = K.bn_rows_case("one-row", C)                                                  # N = 1: statistics of the row, buffers untouched
    ref = K.bn_rows_ref(c["y"], c["active"], None, None, EPS, MOM, c["rmean"], c["rvar"], 3)
    mean, invstd, rmean, rvar, nbt, nrows = _bn_stats(c, C, MOM, 3)
    assert nrows == 1 and nbt == 3 and same_bits(rmean, c["rmean"]) and same_bits(rvar, c["rvar"])
    assert K.ulps(mean, ref["mean"]) <= 2 and K.ulps(invstd, ref["invstd"]) <= 2
    c = K.bn_rows_case("two-rows", C)                                                 # N = 2: buffers move, unbiased variance N / (N - 1)
    ref = K.bn_rows_ref(c["y"], c["active"], None, None, EPS, MOM, c["rmean"], c["rvar"], 3)
    mean, invstd, rmean, rvar, nbt, nrows = _bn_stats(c, C, MOM, 3)
    assert nrows == 2 and nbt == 4 and not same_bits(rvar, c["rvar"])
    assert max(K.ulps(mean, ref["mean"]), K.ulps(invstd, ref["invstd"]), K.ulps(rmean, ref["rmean"]), K.ulps(rvar, ref["rvar"])) <= 2


@pytest.mark.parametrize("layout", ["straddle", "long"])
@pytest.mark.parametrize("C", K.WIDTHS)
def test_bn_apply(gpu, C, layout):
    c = K.bn_rows_case(layout, C)
    act, n = c["active"], c["B"] * c["cap"] * C
    for gamma, beta in ((c["gamma"], c["beta"]), (None, None)):
        ref = K.bn_rows_ref(c["y"], act, gamma, beta, EPS, MOM, c["rmean"], c["rvar"], 0)
        a = filled(n, K.FLOAT_SENTINEL)
        L.sparse_bn_apply(c["y"].cuda(), c["count"].cuda(), c["B"], c["cap"], C, ref["mean"].float().cuda(), ref["invstd"].float().cuda(),
                          None if gamma is None else gamma.cuda(), None if beta is None else beta.cuda(), a)
        got = a.cpu().view(-1, C)
        e = rel_err(got[act], ref["a"].detach())
        print(f"sparse_bn_apply C={C} {layout} affine={gamma is not None}: rel_err {e:.3e}")
        assert e <= ELEMENTWISE and (got[~act] == K.FLOAT_SENTINEL).all()


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("layout", ["straddle", "long"])
@pytest.mark.parametrize("C", K.WIDTHS)
def test_bn_backward(gpu, C, layout, frozen):
    c = K.bn_rows_case(layout, C)
    act, n = c["active"], c["B"] * c["cap"] * C
    for gamma, beta in ((c["gamma"], c["beta"]), (None, None)):
        gamma64 = None if gamma is None else gamma.double().requires_grad_()
        beta64 = None if beta is None else beta.double().requires_grad_()
        ref = K.bn_rows_ref(c["y"], act, gamma64, beta64, EPS, MOM, c["rmean"], c["rvar"], 0, frozen)
        assert float(ref["pre"].detach().abs().min()) >= 1e-3                        # the ReLU mask is well-conditioned
        ref["a"].backward(c["da"][act].double())
        dy, dgamma, dbeta, sums = filled(n, K.FLOAT_SENTINEL), filled(C, NAN), filled(C, NAN), filled(2 * C, NAN)
        work = filled(L.sparse_bn_work_bytes(C), 0xFF, torch.uint8)
        L.sparse_bn_backward(c["y"].cuda(), c["da"].cuda(), c["count"].cuda(), c["B"], c["cap"], C, ref["mean"].float().cuda(),
                             ref["invstd"].float().cuda(), None if gamma is None else gamma.cuda(), None if beta is None else beta.cuda(),
                             frozen, dy, dgamma, dbeta, sums, work)
        got = dy.cpu().view(-1, C)
        # without gamma / beta the sums are still those of x_hat and 1: the gradients a gamma = 1, beta = 0 would get
        if gamma is None:
            one, zero = torch.ones(C, dtype=torch.float64, requires_grad=True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
            r1 = K.bn_rows_ref(c["y"], act, one, zero, EPS, MOM, c["rmean"], c["rvar"], 0, frozen)
            r1["a"].backward(c["da"][act].double())
            want_dg, want_db = one.grad, zero.grad
        else:
            want_dg, want_db = gamma64.grad, beta64.grad
        e = dict(dy=rel_err(got[act], ref["rows"].grad), dgamma=rel_err(dgamma.cpu(), want_dg), dbeta=rel_err(dbeta.cpu(), want_db))
        print(f"sparse_bn_backward C={C} {layout} frozen={frozen} affine={gamma is not None}: rel_err "
              + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) <= ELEMENTWISE and (got[~act] == K.FLOAT_SENTINEL).all()


# ---- canvas ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [32, 96])
def test_canvas(gpu, C, dtype):
    c, (D, H, W), B, cap = K.canvas_case(C), K.CANVAS["dims"], K.CANVAS["B"], K.CANVAS["cap"]
    canvas = filled(B * D * H * W * C, NAN, dtype)
    L.sparse_canvas(c["rows"].cuda(), c["cell"].cuda(), c["count"].cuda(), B, cap, D, H, W, C, canvas)
    want = K.canvas_ref(torch.nan_to_num(c["rows"]), c["cell"], c["count"], B, cap, (D, H, W), C)
    want = want.bfloat16() if dtype == torch.bfloat16 else want
    assert same_bits(canvas.cpu().view(want.shape), want)                             # the rows where they belong, exactly 0 elsewhere


@pytest.mark.parametrize("C", [32, 96])
def test_canvas_backward_and_round_trip(gpu, C):
    c, (D, H, W), B, cap = K.canvas_case(C), K.CANVAS["dims"], K.CANVAS["B"], K.CANVAS["cap"]
    cell, count = c["cell"].cuda(), c["count"].cuda()
    act = K.active_mask(c["count"], B, cap)
    drows = filled(B * cap * C, K.FLOAT_SENTINEL)
    L.sparse_canvas_bwd(c["dcanvas"].cuda(), cell, count, B, cap, D, H, W, C, drows)
    want = K.canvas_bwd_ref(c["dcanvas"], c["cell"], c["count"], B, cap, (D, H, W), C)
    assert same_bits(drows.cpu().view(want.shape), want) and not drows.cpu().view(want.shape)[K.CANVAS["lost"]].any()
    canvas, back = filled(B * D * H * W * C, NAN), filled(B * cap * C, K.FLOAT_SENTINEL)
    L.sparse_canvas(c["rows"].cuda(), cell, count, B, cap, D, H, W, C, canvas)
    L.sparse_canvas_bwd(canvas, cell, count, B, cap, D, H, W, C, back)
    keep = act & (c["cell"] >= 0)
    assert same_bits(back.cpu().view(-1, C)[keep], c["rows"][keep])


# ---- stale workspace, through the encoder ----------------------------------------------------------------------------------------------

def test_encoder_after_a_larger_scene_equals_a_fresh_encoder(gpu):
    from tests import test_gpu_sparse_lidar as T
    case = T.SCENES["random-c4"]
    _, used = T._pair(case)
    _, fresh = T._pair(case)
    used.eval(), fresh.eval()
    one = S.tile_scene(case["H"], case["W"], case["zv"], 127)
    empty = one.clone()
    empty[..., 0] = 1000.0                                                            # every point of the second frame out of range
    small = torch.cat([one, empty]).contiguous().to(gpu)
    used(S.random_scene(4).to(gpu))                                                   # leaves its rows, tables and counts in the workspaces
    got, got_s = used(small), T._device_structure(used)
    want, want_s = fresh(small), T._device_structure(fresh)
    assert same_bits(got, want) and got.abs().sum() > 0
    for lv_g, lv_w in zip(got_s, want_s):
        assert [f.shape[0] for f in lv_g] == [127, 0]
        for f_g, f_w in zip(lv_g, lv_w):
            assert torch.equal(f_g, f_w)
