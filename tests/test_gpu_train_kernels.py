"""Each training backward / optimiser kernel of csrc/train_misc.hip, norm_train.hip and bn_rows.h on the MI355X against its own
exact or fp64 reference (tests/train_kernel_ref.py), one call per case through its `_lib` wrapper: DESIGN.md 4.3, "kernel-level
pins: the training backward and optimiser kernels", which also holds the table of the errors and bounds measured on the MI355X.
tests/test_gpu_train_layers.py sees these kernels only at the config-4 shapes and tests/test_gpu_bn_bits.py only as digests; here
every entry point meets the shapes at which its index arithmetic changes branch, which tests/test_train_kernels_host.py shows on
the CPU that the cases reach.

Conventions: every output lies in a larger buffer with GUARD sentinels on both sides, compared afterwards; where a channel
stride exceeds C the pad columns of the inputs hold NaN and those of the outputs the sentinel; buffers the wrappers want longer
than the kernel's reach end in NaN (inputs) or the sentinel (outputs).  Kernels documented as order-fixed run twice and must give
the same bits; those that add floats atomically do not.

Tolerances: copy / select kernels are exact.  The others: e_dev <= max(4 * e_yard, floor), e_yard being the error of the same
formula in float32 on the CPU with its sums accumulated one term after the other, both against fp64; the floors are
train_kernel_ref.FLOOR.  bn_apply alone has a third term, the a-priori error of its documented scale / shift form
(train_kernel_ref.bn_apply_conditioning), which matters only where |mean| >> std.  Nothing is excluded from any comparison; every
test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from tests import train_kernel_ref as K
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
I32, U8 = torch.int32, torch.uint8


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    return (t if dtype is None else t.to(dtype)).cuda()


class Guarded:
    """n elements between two runs of GUARD sentinels; `.t` is the part the kernel is handed."""

    def __init__(self, n=None, init=None, dtype=torch.float32, fill=K.SENTINEL):
        self.fill = fill
        self.big = torch.full(((n if init is None else init.size) + 2 * K.GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.big[K.GUARD:self.big.numel() - K.GUARD]
        if init is not None:
            self.t.copy_(dev(init))

    def cpu(self):
        """The payload as numpy, after checking both guards."""
        torch.cuda.synchronize()
        big = self.big.cpu()
        assert bool((big[:K.GUARD] == self.fill).all()) and bool((big[-K.GUARD:] == self.fill).all()), "a guard was written"
        return big[K.GUARD:-K.GUARD].numpy().copy()


def same(a, b):
    """Bit equality of two float32 / integer numpy arrays (NaN equals NaN, -0 differs from +0)."""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def equal(a, b):
    """Value equality, NaN equal to NaN."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def twice(run):
    """run() -> {name: numpy}; an order-fixed kernel gives the same bits on a second launch."""
    a, b = run(), run()
    for k in a:
        assert same(a[k], b[k]), f"{k}: two launches differ"
    return a


def held(tag, got, want, yard, floor, conditioning=0.0):
    e_dev, e_yard = rel_err(got, want), rel_err(yard, want)
    bound = max(K.YARD_FACTOR * e_yard, floor, conditioning)
    print(f"{tag}: device rel_err {e_dev:.3e}, float32 on the CPU {e_yard:.3e}, bound {bound:.3e}")
    assert e_dev <= bound, (tag, e_dev, bound)


# ---- copy / select kernels (exact) -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.ZERO_STUFF, ids=lambda c: "x".join(map(str, c)))
def test_zero_stuff(gpu, case):
    N, Ho, Wo, C, H, W, s = case
    dy = K.u(N * Ho * Wo * C, 61, 1.0, 2.0)

    def run():
        out = Guarded(N * H * W * C)
        L.zero_stuff_nhwc(dev(dy), out.t, N, Ho, Wo, C, H, W, s)
        return {"out": out.cpu()}
    assert equal(twice(run)["out"], K.zero_stuff_ref(dy, *case))


@pytest.mark.parametrize("case", K.INTERLEAVE, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-n{c[3]}-{''.join(map(str, c[4]))}-e{c[5]}")
def test_interleave2x2(gpu, case):
    H, W, C, N, present, extra = case
    cls, hq, wq = K.interleave_case(*case)

    def run():
        dx = Guarded(N * H * W * C)
        L.interleave2x2_nhwc([None if c is None else dev(c) for c in cls], hq, wq, dx.t, N, H, W, C)
        return {"dx": dx.cpu()}
    got = twice(run)["dx"]
    assert equal(got, K.interleave_ref(cls, hq, wq, N, H, W, C))
    if present == (1, 0, 0, 0) and H * W > 1:
        assert not got.reshape(N, H, W, C)[:, 1::2].any() and not got.reshape(N, H, W, C)[:, :, 1::2].any()


def _pool_forward(x, H, W, affine):
    N, C = K.POOL_N, K.POOL_C
    Ho, Wo = K.pooled(H, W)

    def run():
        y, idx = Guarded(N * Ho * Wo * C), Guarded(N * Ho * Wo * C, dtype=U8, fill=200)
        if affine:
            L.bn_relu_maxpool3x3s2_idx(dev(x), *[dev(affine[k]) for k in ("mean", "invstd", "gamma", "beta")], y.t, idx.t, N, H, W, C)
        else:
            L.maxpool3x3s2_idx(dev(x), y.t, idx.t, N, H, W, C)
        return {"y": y.cpu(), "idx": idx.cpu()}
    return twice(run)


@pytest.mark.parametrize("hw", K.POOL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maxpool_idx(gpu, hw):
    x = K.pool_input(*hw, with_nan=hw == (7, 9))
    got = _pool_forward(x, *hw, None)
    y, idx = K.maxpool_ref(x, K.POOL_N, *hw, K.POOL_C)
    assert equal(got["y"], y) and equal(got["idx"], idx)
    if hw == (7, 9):
        assert np.isnan(got["y"]).sum() == np.isnan(y).sum() == 2      # pixel (3, 4) lies in the windows oh = 1 and 2 of ow = 2


@pytest.mark.parametrize("hw", K.POOL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bn_relu_maxpool_idx(gpu, hw):
    x, aff = K.pool_input(*hw), K.bn_affine(K.POOL_C, 44)
    got = _pool_forward(x, *hw, aff)
    act = K.relu_fma32(x.reshape(-1, K.POOL_C), **aff)
    y, idx = K.maxpool_ref(act, K.POOL_N, *hw, K.POOL_C)
    assert equal(got["y"], y) and equal(got["idx"], idx)


@pytest.mark.parametrize("codes", ["forward", "random"])
@pytest.mark.parametrize("hw", K.POOL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maxpool_bwd(gpu, hw, codes):
    N, C = K.POOL_N, K.POOL_C
    Ho, Wo = K.pooled(*hw)
    n_out = N * Ho * Wo * C
    idx = K.maxpool_ref(K.pool_input(*hw), N, *hw, C)[1] if codes == "forward" else \
        K.synth.randint((n_out,), 42, 0, 9).numpy().astype(np.uint8)
    dy = K.u(n_out, 41)

    def run():
        dx = Guarded(N * hw[0] * hw[1] * C)
        L.maxpool3x3s2_bwd(dev(dy), dev(idx), dx.t, N, *hw, C)
        return {"dx": dx.cpu()}
    assert equal(twice(run)["dx"], K.maxpool_bwd_ref(dy, idx, N, *hw, C, F32))


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "bn_relu"])
@pytest.mark.parametrize("C", K.GMAX_C)
@pytest.mark.parametrize("P", K.GMAX_P)
def test_group_max_idx(gpu, P, C, affine):
    G = K.GMAX_G
    x = K.group_max_input(P, C)
    aff = K.bn_affine(C, 52) if affine else None

    def run():
        y, idx = Guarded(G * C), Guarded(G * C, dtype=I32, fill=-12345)
        work = torch.full((L.group_max_idx_work_bytes(G, P, C),), 0xAB, dtype=U8, device="cuda")
        if affine:
            L.bn_relu_group_max_idx(dev(x), *[dev(aff[k]) for k in ("mean", "invstd", "gamma", "beta")], y.t, idx.t, work, G, P, C)
        else:
            L.group_max_idx(dev(x), y.t, idx.t, work, G, P, C)
        return {"y": y.cpu(), "idx": idx.cpu()}
    got = twice(run)
    y, idx = K.group_max_ref(K.relu_fma32(x.reshape(-1, C), **aff) if affine else x, G, P, C)
    assert equal(got["y"], y) and equal(got["idx"], idx)


@pytest.mark.parametrize("prefilled", [False, True], ids=["zeros", "prefilled"])
@pytest.mark.parametrize("C", K.GMAX_C + (6,))
@pytest.mark.parametrize("P", K.GMAX_P)
def test_group_max_bwd(gpu, P, C, prefilled):
    G = K.GMAX_G
    idx = K.group_max_ref(K.group_max_input(P, C), G, P, C)[1] if C % 4 == 0 else \
        K.synth.randint((G * C,), 56, 0, P).numpy().astype(np.int32)
    dy = K.u(G * C, 57, 1.0, 2.0)
    before = K.u(G * P * C, 58, 3.0, 4.0) if prefilled else np.zeros(G * P * C, F32)

    def run():
        dx = Guarded(init=before)
        L.group_max_bwd(dev(dy), dev(idx), dx.t, G, P, C)
        return {"dx": dx.cpu()}
    assert equal(twice(run)["dx"], K.group_max_bwd_ref(dy, idx, G, P, C, before))


@pytest.mark.parametrize("n", K.EW_N)
def test_relu_mask(gpu, n):
    n4 = (n + 3) // 4 * 4
    y, dy = K.relu_mask_input(n4), K.u(n4, 72, 1.0, 2.0)

    def run():
        g = Guarded(init=dy)
        L.relu_mask(g.t, dev(y), n)
        return {"dy": g.cpu()}
    assert equal(twice(run)["dy"], K.relu_mask_ref(dy, y))


@pytest.mark.parametrize("n", K.EW_N)
def test_add_inplace(gpu, n):
    n4 = (n + 3) // 4 * 4
    y, x = K.u(n4, 73), K.u(n4, 74)

    def run():
        g = Guarded(init=y)
        L.add_inplace(g.t, dev(x), n)
        return {"y": g.cpu()}
    assert same(twice(run)["y"], (y + x).astype(F32))


@pytest.mark.parametrize("case", K.CAM_MEAN, ids=lambda c: f"ncam{c[0]}-b{c[1]}-pc{c[2]}")
def test_cam_mean_bwd(gpu, case):
    ncam, B, pc = case
    dy = K.u(B * pc, 75)

    def run():
        dx = Guarded(B * ncam * pc)
        L.cam_mean_bwd(dev(dy), dx.t, B, ncam, pc // 4, 4)
        return {"dx": dx.cpu()}
    assert same(twice(run)["dx"], K.cam_mean_bwd_ref(dy, B, ncam, pc))


# ---- bilinear backward (float atomics: one launch) --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.BILINEAR, ids=lambda c: "x".join(map(str, c)))
def test_bilinear_bwd(gpu, case):
    Hi, Wi, Ho, Wo, C, x_cs, y_cs = case
    B = K.BILINEAR_B
    dy = K.strided(K.u(B * Ho * Wo * C, 76), B * Ho * Wo, C, y_cs)
    dx = Guarded(init=K.strided(np.zeros((B * Hi * Wi, C), F32), B * Hi * Wi, C, x_cs, pad=K.SENTINEL))     # zero-filled by the caller
    L.bilinear_bwd_nhwc(dev(dy), dx.t, B, Hi, Wi, C, x_cs, Ho, Wo, y_cs)
    got = dx.cpu().reshape(-1, x_cs)
    assert (got[:, C:] == K.SENTINEL).all()
    held(f"bilinear_bwd {case}", got[:, :C].reshape(-1), K.bilinear_bwd_ref(dy, B, Hi, Wi, C, Ho, Wo, y_cs),
         K.bilinear_bwd_ref(dy, B, Hi, Wi, C, Ho, Wo, y_cs, F32), K.FLOOR["bilinear"])


# ---- dense layer backward (order-fixed) ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(K.LINEAR))
def test_linear_bwd(gpu, name):
    B, Kk, O, perm, with_dx, with_db = K.LINEAR[name]
    c = K.linear_case(name)

    def run():
        o = {"dw": Guarded(O * Kk)}
        if with_dx:
            o["dx"] = Guarded(B * Kk)
        if with_db:
            o["db"] = Guarded(O)
        work = torch.full((L.linear_bwd_work_floats(B, Kk, O),), float("nan"), device="cuda")
        L.linear_bwd(dev(c["dy"]), dev(c["x"]), dev(c["w"]), o["dx"].t if with_dx else None, o["dw"].t, o["db"].t if with_db else None,
                     work, B, Kk, O, *perm)
        return {k: v.cpu() for k, v in o.items()}
    got = twice(run)
    want, yard = (K.linear_bwd_ref(c["dy"], c["x"], c["w"], B, Kk, O, perm, dt) for dt in (F64, F32))
    for k in got:
        held(f"linear_bwd {name} {k}", got[k], want[k], yard[k], K.FLOOR["linear"])


# ---- CenterNet head tail backward (dhid order-fixed; dw / db atomics) -------------------------------------------------------------

@pytest.mark.parametrize("name", list(K.HEAD))
def test_head_tail_bwd(gpu, name):
    B, P, hc, cs, n_sigmoid = K.HEAD[name]
    c = K.head_case(name)
    dhid, dw, db = Guarded(B * P * 5 * hc), Guarded(init=c["dw0"]), Guarded(init=c["db0"])          # the kernels add to dw / db
    L.head_tail_bwd(dev(c["hid"]), dev(c["w"]), dev(c["out0"]), [dev(d) if d.size else torch.full((4,), float("nan"), device="cuda") for d in c["douts"]],
                    dhid.t, dw.t, db.t, B, P, hc, cs, n_sigmoid)
    got = dict(dhid=dhid.cpu(), dw=dw.cpu(), db=db.cpu())
    args = (c["hid"], c["w"], c["out0"], c["douts"], c["dw0"], c["db0"], B, P, hc, cs, n_sigmoid)
    want, yard = K.head_tail_bwd_ref(*args, F64), K.head_tail_bwd_ref(*args, F32)
    for k in got:
        held(f"head_tail_bwd {name} ({K.head_kernel(cs, hc)}) {k}", got[k], want[k], yard[k], K.FLOOR["head_tail"])


# ---- small-K weight gradient (atomics) ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.SMALLK, ids=lambda c: f"m{c[0]}-k{c[1]}-cout{c[2]}")
def test_smallk_wgrad(gpu, case):
    M, Kk, Cout = case
    c = K.smallk_case(*case)
    dw = Guarded(init=c["dw0"])
    L.smallk_wgrad(dev(c["dy"]), dev(c["x"]), dw.t, M, Kk, Cout)
    held(f"smallk_wgrad {case}", dw.cpu(), K.smallk_wgrad_ref(c["dy"], c["x"], c["dw0"], *case),
         K.smallk_wgrad_ref(c["dy"], c["x"], c["dw0"], *case, F32), K.FLOOR["smallk"])


# ---- optimiser -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(K.GRAD_NORM))
def test_grad_norm(gpu, name):
    n, kind, max_norm = K.GRAD_NORM[name]
    g = K.grad_norm_case(name)

    def run():
        out = Guarded(2)
        L.grad_norm(dev(g), torch.full((512,), float("nan"), dtype=torch.float64, device="cuda"), max_norm, out.t)
        return {"out": out.cpu()}
    got = twice(run)["out"]
    want, yard = K.grad_norm_ref(g, max_norm), K.grad_norm_ref(g, max_norm, F32)
    assert np.isfinite(got).all()
    for i, what in enumerate(("norm", "coefficient")):
        held(f"grad_norm {name} {what}", got[i:i + 1], want[i:i + 1], yard[i:i + 1], K.FLOOR["grad_norm"])
    if kind == "zero":
        assert got[0] == 0 and got[1] == 1
    if name == "no_clip":
        assert got[1] == 1
    if name in ("n1", "huge"):
        assert got[1] < 1


@pytest.mark.parametrize("name", list(K.ADAMW))
def test_adamw_step(gpu, name):
    n, step, coef, wd = K.ADAMW[name]
    c = K.adamw_case(name)

    def run():
        o = {k: Guarded(init=c[k]) for k in ("p", "m", "v")}
        clip = None if coef is None else dev(np.array([123.0, coef], F32))
        L.adamw_step(o["p"].t, dev(c["g"]), o["m"].t, o["v"].t, clip, K.HYPER["lr"], K.HYPER["beta1"], K.HYPER["beta2"], K.HYPER["eps"], wd, step)
        return {k: v.cpu() for k, v in o.items()}
    got = twice(run)
    coef32 = None if coef is None else float(F32(coef))
    want, yard = (K.adamw_ref(c["p"], c["g"], c["m"], c["v"], coef32, step, wd, dt) for dt in (F64, F32))
    for k in got:
        held(f"adamw_step {name} {k}", got[k], want[k], yard[k], K.FLOOR["adamw"])


# ---- BatchNorm (order-fixed) ---------------------------------------------------------------------------------------------------------------

def _work(C):
    return torch.full((L.bn_work_floats(C),), float("nan"), device="cuda")


def _ids(s):
    return "x".join(map(str, s))


def _stats(x, M, C, cs):
    def run():
        o = {k: Guarded(C) for k in ("mean", "var", "invstd")}
        L.bn_stats(dev(K.strided(x, M, C, cs)), _work(C), o["mean"].t, o["var"].t, o["invstd"].t, M, C, cs, K.EPS)
        return {k: v.cpu() for k, v in o.items()}
    got = twice(run)
    want, yard = K.batch_stats(x), K.batch_stats(x, F32)
    for i, k in enumerate(("mean", "var", "invstd")):
        held(f"bn_stats {(M, C, cs)} {k}", got[k], want[i], yard[i], K.FLOOR["bn_stats"])
    return got


@pytest.mark.parametrize("shape", K.ROWS, ids=_ids)
def test_bn_stats(gpu, shape):
    got = _stats(K.rows_case(*shape)["x"], *shape)
    if shape[0] == 1:
        assert not got["var"].any() and same(got["mean"], K.rows_case(*shape)["x"][0])


def test_bn_stats_far_mean(gpu):
    _stats(K.far_mean_input(), *K.FAR_MEAN, K.FAR_MEAN[1])


def _apply(tag, c, M, C, cs, relu, with_res):
    n = (M - 1) * cs + C                                                    # what the wrapper wants of res and y; the kernel reaches M * C

    def run():
        y = Guarded(n)
        res = dev(np.concatenate([c["res"].reshape(-1), np.full(n - M * C, np.nan, F32)])) if with_res else None
        L.bn_apply(dev(K.strided(c["x"], M, C, cs)), *[dev(c[k]) for k in ("mean", "invstd", "gamma", "beta")], res, y.t, M, C, cs, relu)
        return {"y": y.cpu()}
    got = twice(run)["y"]
    assert (got[M * C:] == K.SENTINEL).all()
    args = (c["x"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["res"] if with_res else None, relu)
    want = K.bn_apply_ref(*args)
    held(tag, got[:M * C], want, K.bn_apply_ref(*args, F32), K.FLOOR["bn_apply"], K.bn_apply_conditioning(*args[:5], want))


@pytest.mark.parametrize("mode", K.BN_APPLY, ids=lambda m: m[0])
@pytest.mark.parametrize("shape", K.ROWS, ids=_ids)
def test_bn_apply(gpu, shape, mode):
    _apply(f"bn_apply {shape} {mode[0]}", K.rows_case(*shape), *shape, mode[1], mode[2])


def test_bn_apply_far_mean(gpu):
    """|mean| = 1000 std: the scale / shift form keeps 2^-24 |mean| / std of a unit-size output."""
    M, C = K.FAR_MEAN
    x = K.far_mean_input()
    mean, _, invstd = K.stats32(x)
    _apply("bn_apply far_mean plain", dict(x=x, mean=mean, invstd=invstd, gamma=K.u(C, 7, 0.5, 1.5), beta=K.u(C, 8, -0.3, 0.3)), M, C, C, False, False)


def _held_backward(tag, got, want, yard, C, cs):
    for k in ("dbeta", "dgamma"):
        held(f"{tag} {k}", got[k], want[k], yard[k], K.FLOOR["bn_sums"])
    if "dx" in got:
        dx = got["dx"].reshape(-1, cs)
        assert (dx[:, C:] == K.SENTINEL).all()
        held(f"{tag} dx", dx[:, :C], want["dx"], yard["dx"], K.FLOOR["bn_dx"])


@pytest.mark.parametrize("variant", list(K.BWD_VARIANTS))
@pytest.mark.parametrize("shape", K.ROWS, ids=_ids)
def test_bn_backward(gpu, shape, variant):
    M, C, cs = shape
    relu, names, with_dx = K.BWD_VARIANTS[variant]
    i = K.bn_variant_inputs(variant, K.rows_case(*shape), M)
    n = (M - 1) * cs + C

    def dense(a, pad):                                                      # [M][C] rows, then what the wrapper wants on top of them
        return np.concatenate([a.reshape(-1), np.full(n - M * C, pad, F32)])

    def run():
        o = {"dy": Guarded(init=dense(i["dy"], K.SENTINEL)), "dgamma": Guarded(C), "dbeta": Guarded(C)}
        if with_dx:
            o["dx"] = Guarded(M * cs)
        d = {k: dev(K.strided(v, M, C, cs) if k == "x" else dense(v, np.nan) if k == "y" else v) for k, v in i.items() if k != "dy"}
        L.bn_backward(o["dy"].t, d.get("y"), d.get("x"), d.get("mean"), d.get("invstd"), d.get("gamma"), d.get("beta"), _work(C),
                      o["dgamma"].t, o["dbeta"].t, o["dx"].t if with_dx else None, M, C, cs, relu=bool(relu & 3), has_res=relu & 3 == 1,
                      frozen=bool(relu & 4))
        return {k: v.cpu() for k, v in o.items()}
    got = twice(run)
    want, yard = K.bn_backward_ref(variant, K.rows_case(*shape), M), K.bn_backward_ref(variant, K.rows_case(*shape), M, F32)
    assert (got["dy"][M * C:] == K.SENTINEL).all()
    assert same(got["dy"][:M * C], np.ascontiguousarray(want["dy"], F32).reshape(-1)), "dy: masked copy written back (relu 1) or untouched"
    if "x" not in names:
        assert not got["dgamma"].any()
    _held_backward(f"bn_backward {shape} {variant}", got, want, yard, C, cs)


@pytest.mark.parametrize("case", K.FROM_PARTIALS, ids=lambda c: f"{_ids(c[0])}-g{c[1]}")
def test_bn_backward_from_partials(gpu, case):
    (M, C, cs), G = case
    c = K.rows_case(M, C, cs)
    part = K.backward_partials(c, M, C, G)
    n = (M - 1) * cs + C

    def run():
        o = {"dgamma": Guarded(C), "dbeta": Guarded(C), "dx": Guarded(M * cs)}
        L.bn_backward_from_partials(dev(np.concatenate([c["dy"].reshape(-1), np.full(n - M * C, np.nan, F32)])), dev(K.strided(c["x"], M, C, cs)),
                                    dev(c["mean"]), dev(c["invstd"]), dev(c["gamma"]), dev(part), G, o["dgamma"].t, o["dbeta"].t, o["dx"].t,
                                    M, C, cs)
        return {k: v.cpu() for k, v in o.items()}
    _held_backward(f"bn_backward_from_partials {case}", twice(run), K.backward_from_partials_ref(part, c, M, C, G),
                   K.backward_from_partials_ref(part, c, M, C, G, F32), C, cs)


@pytest.mark.parametrize("shape", K.POOLED_BN, ids=_ids)
def test_pool_bn_backward(gpu, shape):
    N, H, W, C = shape
    c = K.pooled_bn_case(*shape)

    def run():
        o = {"dgamma": Guarded(C), "dbeta": Guarded(C), "dx": Guarded(N * H * W * C)}
        L.pool_bn_backward(dev(c["dpool"]), dev(c["idx"]), dev(c["x"]), *[dev(c[k]) for k in ("mean", "invstd", "gamma", "beta")], _work(C),
                           o["dgamma"].t, o["dbeta"].t, o["dx"].t, N, H, W, C)
        return {k: v.cpu() for k, v in o.items()}
    _held_backward(f"pool_bn_backward {shape}", twice(run), K.pool_bn_backward_ref(c, *shape), K.pool_bn_backward_ref(c, *shape, F32), C, C)


@pytest.mark.parametrize("shape", K.GMAX_BN, ids=_ids)
def test_gmax_bn_sums(gpu, shape):
    B, P, C, cs = shape
    c = K.gmax_bn_case(*shape)

    def run():
        o = {"dgm": Guarded(B * C), "dgamma": Guarded(C), "dbeta": Guarded(C)}
        L.gmax_bn_sums(dev(c["dg"]), dev(c["gmax"]), dev(c["idx"]), dev(K.strided(c["x"], B * P, C, cs)), dev(c["mean"]), dev(c["invstd"]),
                       o["dgm"].t, o["dgamma"].t, o["dbeta"].t, B, P, C, cs)
        return {k: v.cpu() for k, v in o.items()}
    got = twice(run)
    want, yard = K.gmax_bn_ref(c, B, P, C), K.gmax_bn_ref(c, B, P, C, F32)
    assert equal(got["dgm"], want["dgm"])
    _held_backward(f"gmax_bn_sums {shape}", got, want, yard, C, cs)


@pytest.mark.parametrize("shape", K.GMAX_BN, ids=_ids)
def test_gmax_bn_backward(gpu, shape):
    B, P, C, cs = shape
    c = K.gmax_bn_case(*shape)
    o = {"dgm": Guarded(B * C), "dgamma": Guarded(C), "dbeta": Guarded(C), "dx": Guarded(B * P * cs)}
    L.gmax_bn_backward(dev(c["dg"]), dev(c["gmax"]), dev(c["idx"]), dev(K.strided(c["x"], B * P, C, cs)), dev(c["mean"]), dev(c["invstd"]),
                       dev(c["gamma"]), o["dgm"].t, o["dgamma"].t, o["dbeta"].t, o["dx"].t, B, P, C, cs)
    got = {k: v.cpu() for k, v in o.items()}
    want, yard = K.gmax_bn_ref(c, B, P, C), K.gmax_bn_ref(c, B, P, C, F32)
    assert equal(got["dgm"], want["dgm"])
    if B * P == 1:
        # one row: dx is identically 0, the difference of gamma invstd dgm with itself, each product rounded once (or fused into
        # the addition): there is no scale for a relative error, so the bound is absolute, 4 * 2^-24 of the cancelling terms
        terms = float(np.abs(c["gamma"].astype(F64) * c["invstd"] * want["dgm"]).max())
        dx = got.pop("dx").reshape(-1, cs)
        print(f"gmax_bn_backward {shape} dx: |dx| <= {np.abs(dx[:, :C]).max():.3e}, exact 0, bound {4 * 2.0 ** -24 * terms:.3e}")
        assert not want["dx"].any() and (dx[:, C:] == K.SENTINEL).all() and np.abs(dx[:, :C]).max() <= 4 * 2.0 ** -24 * terms
    _held_backward(f"gmax_bn_backward {shape}", got, want, yard, C, cs)


@pytest.mark.parametrize("case", K.PARTIALS, ids=_ids)
def test_bn_stats_from_partials(gpu, case):
    G, M, C = case
    c = K.partials_case(*case)

    def run():
        o = {k: Guarded(C) for k in ("mean", "var", "invstd")}
        L.bn_stats_from_partials(dev(c["part"]), G, dev(c["pivot"]), o["mean"].t, o["var"].t, o["invstd"].t, M, C, K.EPS)
        return {k: v.cpu() for k, v in o.items()}
    got = twice(run)
    want, yard = K.stats_from_partials_ref(c["part"], c["pivot"], *case), K.stats_from_partials_ref(c["part"], c["pivot"], *case, F32)
    for i, k in enumerate(("mean", "var", "invstd")):
        held(f"bn_stats_from_partials {case} {k}", got[k], want[i], yard[i], K.FLOOR["bn_stats"])


@pytest.mark.parametrize("case", K.RUNNING, ids=_ids)
def test_bn_update_running(gpu, case):
    C, M = case
    c = K.running_case(C)

    def run():
        rmean, rvar, nbt = Guarded(init=c["rmean"]), Guarded(init=c["rvar"]), Guarded(init=np.array([41], np.int64), dtype=torch.int64, fill=-7)
        L.bn_update_running(dev(c["mean"]), dev(c["var"]), rmean.t, rvar.t, nbt.t, C, M, K.MOMENTUM)
        return {"rmean": rmean.cpu(), "rvar": rvar.cpu(), "nbt": nbt.cpu()}
    got = twice(run)
    assert got["nbt"].tolist() == [42]
    want, yard = K.update_running_ref(c, M), K.update_running_ref(c, M, F32)
    for i, k in enumerate(("rmean", "rvar")):
        held(f"bn_update_running {case} {k}", got[k], want[i], yard[i], K.FLOOR["running"])
