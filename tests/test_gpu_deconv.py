"""bevf_deconv_nhwc_f32 / _bf16 (csrc/deconv.hip), the kernel = stride transposed convolution of the FPN neck, on its own:
exact small-integer data against the loop form of its formula, the slice store into a wider map, real data against fp64 inside
the forward error bound of an fp32 dot product, determinism and the refusals."""
import numpy as np
import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from tests.bev_backbone_ref import deconv_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
#          N, H,  W,  Cin, Cout, s
SHAPES = [(1, 1, 1, 32, 32, 2),        # smallest shape
          (2, 3, 5, 32, 64, 4),        # non-square: a swapped i / j or h / w shows
          (1, 17, 9, 96, 160, 2),      # odd K chunk count, Cout not a multiple of 64, M = 153 not a tile multiple
          (2, 16, 24, 64, 32, 2)]      # several row tiles


def _ints(shape, seed):
    N, H, W, Cin, Cout, s = shape
    rng = np.random.default_rng(seed)
    x = (rng.random((N, H, W, Cin)) < 0.25).astype(np.float32)
    w = rng.integers(-1, 2, size=(Cin, Cout, s, s)).astype(np.float32)
    return x, w


def _reals(shape, seed):
    N, H, W, Cin, Cout, s = shape
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, H, W, Cin)).astype(np.float32), (rng.standard_normal((Cin, Cout, s, s)) / np.sqrt(Cin)).astype(np.float32))


def _run(x, w, dtype, scale=None, shift=None, relu=False, y=None, y_cs=None, y_off=0):
    """x (N,H,W,Cin) / w (Cin,Cout,s,s) numpy fp32 -> the kernel's output as a (N,sH,sW,y_cs) tensor in `dtype` (and the buffer)."""
    N, H, W, Cin = x.shape
    Cout, s = w.shape[1], w.shape[2]
    y_cs = y_cs or Cout
    xd = torch.from_numpy(x).cuda().to(dtype).contiguous()
    wp = L.deconv_pack(torch.from_numpy(w).cuda(), dtype)
    if y is None:
        y = torch.full((N * s * H * s * W * y_cs,), float("nan"), dtype=dtype, device="cuda")
    sc = None if scale is None else torch.from_numpy(scale).cuda()
    sh = None if shift is None else torch.from_numpy(shift).cuda()
    L.deconv_nhwc(xd.view(-1), wp, sc, sh, y[y_off:], N=N, H=H, W=W, Cin=Cin, x_cs=Cin, Cout=Cout, y_cs=y_cs, s=s, relu=relu)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_exact_integers(gpu, shape, dtype):
    """x in {0, 1} at density 0.25, w in {-1, 0, 1}, no scale / shift: every partial sum is a small integer, so the output equals
    the loop form of the formula exactly in both storage types."""
    N, H, W, Cin, Cout, s = shape
    x, w = _ints(shape, 100 + Cin + s)
    ref = deconv_ref(x, w)
    assert np.abs(ref).max() <= 128                                  # bf16 holds every integer up to 256 exactly
    y = _run(x, w, dtype).view(N, s * H, s * W, Cout).float().cpu().numpy().astype(np.float64)
    bad = np.argwhere(y != ref)
    assert bad.shape[0] == 0, (bad.shape[0], bad[:4], [(y[tuple(b)], ref[tuple(b)]) for b in bad[:4]])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_slice_store_leaves_the_rest_of_the_map_alone(gpu, dtype):
    """y_cs = Cout + 96 with the slice at channel 32 of a buffer pre-filled with a sentinel bit pattern: every byte outside the
    slice is unchanged, the slice holds the exact result."""
    shape = (2, 3, 5, 32, 64, 4)
    N, H, W, Cin, Cout, s = shape
    x, w = _ints(shape, 7)
    ref = deconv_ref(x, w)
    y_cs = Cout + 96
    es = 4 if dtype == torch.float32 else 2
    n = N * s * H * s * W * y_cs
    raw = torch.full((n * es,), 0xA5, dtype=torch.uint8, device="cuda")
    buf = raw.view(dtype)
    before = raw.clone()
    _run(x, w, dtype, y=buf, y_cs=y_cs, y_off=32)
    got = buf.view(N, s * H, s * W, y_cs)
    assert np.array_equal(got[..., 32:32 + Cout].float().cpu().numpy().astype(np.float64), ref)
    keep = torch.ones(N, s * H, s * W, y_cs, es, dtype=torch.bool, device="cuda")
    keep[..., 32:32 + Cout, :] = False
    assert torch.equal(raw.view(N, s * H, s * W, y_cs, es)[keep], before.view(N, s * H, s * W, y_cs, es)[keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("affine", [False, True], ids=["raw", "scale_shift_relu"])
def test_real_data_against_fp64(gpu, dtype, affine):
    """Element-wise |y - ref| <= (K + 2) * 2^-24 * sum|x||w| * |scale| (the forward error bound of an fp32 dot product, K = Cin);
    bf16: on inputs rounded to bf16 first, plus 2^-8 |ref| for the one rounding at the store."""
    shape = (1, 17, 9, 96, 160, 2)
    N, H, W, Cin, Cout, s = shape
    x, w = _reals(shape, 3)
    if dtype == torch.bfloat16:
        x = torch.from_numpy(x).bfloat16().float().numpy()
        w = torch.from_numpy(w).bfloat16().float().numpy()
    rng = np.random.default_rng(11)
    scale = (rng.standard_normal(Cout) * 0.5 + 1.0).astype(np.float32) if affine else None
    shift = rng.standard_normal(Cout).astype(np.float32) if affine else None
    lin = deconv_ref(x, w)
    mag = deconv_ref(np.abs(x), np.abs(w))
    ref = lin * scale.astype(np.float64) + shift.astype(np.float64) if affine else lin
    if affine:
        ref = np.maximum(ref, 0.0)
    bound = (Cin + 2) * 2.0 ** -24 * mag * (np.abs(scale.astype(np.float64)) if affine else 1.0)
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    y = _run(x, w, dtype, scale, shift, relu=affine).view(N, s * H, s * W, Cout).float().cpu().numpy().astype(np.float64)
    err = np.abs(y - ref)
    print(f"deconv {dtype} affine={affine}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_two_launches_are_bit_equal(gpu, dtype):
    shape = (2, 16, 24, 64, 32, 2)
    x, w = _reals(shape, 5)
    a = _run(x, w, dtype).clone()
    b = _run(x, w, dtype)
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_unsupported_arguments_are_refused_before_any_launch(gpu, dtype):
    """s = 3, Cin = 48, a y_cs that breaks the 16-byte rule, short buffers and CPU tensors raise BevfError; the output buffer,
    pre-filled with a sentinel, is untouched by every one of them."""
    dev = "cuda"

    def z(n, d=dtype, device=dev):
        return torch.zeros(n, dtype=d, device=device)

    y = torch.full((4096,), 3.0, dtype=dtype, device=dev)
    geo = dict(N=1, H=2, W=2, Cin=32, x_cs=32, Cout=32, y_cs=32, s=2, relu=False)
    wp = z(L.deconv_pack_elems(32, 32, 2, dtype))
    cases = {
        "s=3": (z(128), z(9 * 32 * 64), dict(geo, s=3)),
        "Cin=48": (z(4 * 48), z(4 * 32 * 64), dict(geo, Cin=48, x_cs=48)),
        "y_cs": (z(128), wp, dict(geo, y_cs=34)),
        "short x": (z(127), wp, geo),
        "short w": (z(128), wp[:-1], geo),
    }
    for name, (x, w_, kw) in cases.items():
        with pytest.raises(L.BevfError):
            L.deconv_nhwc(x, w_, None, None, y, **kw)
    with pytest.raises(L.BevfError, match="needs"):
        L.deconv_nhwc(z(128), wp, None, None, y[:511], **geo)
    with pytest.raises(L.BevfError, match="needs"):
        L.deconv_nhwc(z(128), wp, z(31, torch.float32), None, y, **geo)
    with pytest.raises(L.BevfError, match="no CPU fallback"):
        L.deconv_nhwc(z(128, device="cpu"), wp, None, None, y, **geo)
    with pytest.raises(L.BevfError):
        L.deconv_pack(torch.zeros(32, 32, 3, 3, device=dev), dtype)
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
