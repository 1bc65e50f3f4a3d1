"""Host-side execution engines: weight packing + kernel sequencing for the HIP path.

One engine per reference module (camera encoder, point MLPs, BEV fusion, CenterNet head).
An engine packs its module's parameters once per weight version (BatchNorm folded in fp64,
conv weights re-laid OIHW -> OHWI, the lidar_init rows left in place and permuted on store),
keeps grow-only device workspaces, and issues the C-ABI calls on torch's current stream.
Internally every activation is fp32 NHWC; NCHW exists only at the reference's API surface.
These engines are the eval-mode path (BatchNorm folded from its running statistics).  Training runs through the tapes
of training.py (train-mode BatchNorm + hand-written backward), one per module kind: training.DetectorTape composes them
for the whole detector, and each camera / PointNet / radar / pillar encoder, the BEV fusion and the head used on their
own dispatch to their own tape from their `forward` while in train mode.
An engine asked to fold a BatchNorm that is still in train mode (e.g. VFELayer, which has no tape) raises (_check_eval).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import camera_rig as CR


# ---- packing ---------------------------------------------------------------------------------------

def _bn_fold(bias: Optional[torch.Tensor], bn, cout: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """scale/shift with  y = conv_nobias(x) * scale + shift  ==  bn(conv(x) + bias)   (eval mode)."""
    b = torch.zeros(cout, dtype=torch.float64, device=dev) if bias is None else bias.detach().double()
    if bn is None or isinstance(bn, nn.Identity):
        return torch.ones(cout, device=dev), b.float().contiguous()
    g = bn.weight.detach().double() if bn.weight is not None else torch.ones(cout, dtype=torch.float64, device=dev)
    be = bn.bias.detach().double() if bn.bias is not None else torch.zeros(cout, dtype=torch.float64, device=dev)
    scale = g / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = be + (b - bn.running_mean.detach().double()) * scale
    return scale.float().contiguous(), shift.float().contiguous()


@dataclass
class PackedConv:
    w: torch.Tensor          # OHWI, flat
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    relu: bool
    wino: bool = False       # w is the transformed-filter image of the fused Winograd kernel (csrc/conv_wino.hip)
    c3: bool = False         # w is the fragment-ordered filter image of the bf16 3x3 kernel (csrc/conv3x3_bf16.hip)


_CONV_MODE = "wino"
BF16_CONV3X3 = True          # bf16 models: 3x3 / stride 1 / pad 1 layers on csrc/conv3x3_bf16.hip (False: implicit GEMM everywhere, the round-2 path)


def set_conv_mode(mode: str) -> None:
    """How fp32 models multiply in their convolutions.  "wino" (default): the 3x3 / stride 1 / pad 1 layers
    (Cin % 32 == 0; ~85 % of the path's FLOPs) run as fused fp32 Winograd F(2x2,3x3) on v_mfma_f32_16x16x4_f32
    (csrc/conv_wino.hip: fp32 products and accumulation, 2.25x fewer of them; a few 1e-7 relative from the direct
    kernel per layer, the whole detector within 1e-4 of the oracle at full size -- tests/test_gpu_wino.py), every other
    layer as "f32".  "f32": v_mfma_f32_32x32x2_f32 everywhere, an exact fp32 FMA chain whose bits do not depend on
    tile shapes.  "f32x3": opt-in, fp32 operands split exactly into three bf16 planes and multiplied on the bf16 MFMA
    (six partial products, fp32 accumulate; csrc/conv_split.hip) -- fp32-level error, ~1.3-1.4x faster, not
    bit-identical to the default.  "wino_x3": opt-in, both reductions of MFMA work together -- Winograd where "wino" uses it,
    the three-plane kernel for every other layer (stride-2 3x3, 1x1 projections, PointNet incl. its fused point max).
    Engines repack on the next forward."""
    global _CONV_MODE
    if mode not in ("f32", "wino", "f32x3", "wino_x3"):
        raise ValueError(f"conv mode must be 'f32', 'wino', 'f32x3' or 'wino_x3', got {mode!r}")
    _CONV_MODE = mode


def conv_mode() -> str:
    return _CONV_MODE


def pack_conv(conv, bn=None, relu: bool = True, split_ok: bool = True, wino_ok: bool = True) -> PackedConv:
    """Weights keep the module's storage dtype (fp32 or bf16); the folded BN scale/shift are always fp32.
    In "f32x3" / "wino_x3" mode fp32 filters with Cin % 32 == 0 are stored as three bf16 planes (split_ok=False keeps a layer
    on the exact kernel)."""
    w = conv.weight.detach()
    if w.dim() == 3:                                   # Conv1d k=1 == pointwise
        w = w.unsqueeze(-1)
    cout, cin, kh, kw = w.shape
    assert kh == kw, "square kernels only"
    stride = conv.stride[0] if isinstance(conv.stride, tuple) else conv.stride
    pad = conv.padding[0] if isinstance(conv.padding, tuple) else conv.padding
    scale, shift = _bn_fold(conv.bias, bn, cout, w.device)
    packed = w.permute(0, 2, 3, 1).contiguous().view(-1)
    return _finish_pack(packed, scale, shift, cin, cout, kh, stride, pad, relu, split_ok, wino_ok)


def _finish_pack(packed, scale, shift, cin, cout, k, stride, pad, relu, split_ok=True, wino_ok=True) -> PackedConv:
    """OHWI filter -> what the active conv mode's kernel reads."""
    bf16_model = packed.dtype == torch.bfloat16          # (the f32x3 planes below are bf16 too, but belong to an fp32 model)
    if packed.dtype == torch.float32 and cin % 32 == 0:
        if _CONV_MODE in ("wino", "wino_x3") and wino_ok and (k, stride, pad) == (3, 1, 1):
            return PackedConv(L.wino_filter_transform(packed, cout, cin), scale, shift, cin, cout, k, stride, pad, relu, wino=True)
        if _CONV_MODE in ("f32x3", "wino_x3") and split_ok:
            packed = L.split_weights_f32x3(packed)
    if (BF16_CONV3X3 and bf16_model and (k, stride, pad) == (3, 1, 1) and cin % 32 == 0 and cout % 64 == 0
            and wino_ok):
        return PackedConv(L.conv3x3_pack_bf16(packed, cout, cin), scale, shift, cin, cout, k, stride, pad, relu, c3=True)
    return PackedConv(packed, scale, shift, cin, cout, k, stride, pad, relu)


def _check_eval(module: nn.Module) -> None:
    for m in module.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training:
            raise L.BevfError(
                f"{type(module).__name__} has a BatchNorm in train mode but was asked for the eval-mode kernels (BatchNorm "
                "folded from running statistics) -- call .eval() first.  Train-mode BatchNorm, backward and optimiser run "
                "through the training tapes (training.DetectorTape and its per-module tapes): the detector, ResNetCameraEncoder, "
                "PointNetLiDAREncoder, PillarLiDAREncoder, SparseLiDAREncoder, RadarEncoder / MultiRadarEncoder, VFELayer, FlexibleBEVFusion and "
                "CenterNetHead reach them from forward() in train mode.")


class _Engine:
    """Weight-version tracking + grow-only workspaces."""

    def __init__(self, module: nn.Module):
        self.module = module
        self._sig = None
        self._bufs: Dict[str, torch.Tensor] = {}

    def _signature(self):
        return (_CONV_MODE, BF16_CONV3X3) + tuple((t.data_ptr(), t._version) for t in self.module.state_dict(keep_vars=True).values())

    def ensure_packed(self) -> None:
        sig = self._signature()
        if sig != self._sig:
            _check_eval(self.module)
            with torch.no_grad():
                self.pack()
            self._sig = sig

    def pack(self) -> None:  # pragma: no cover - abstract
        raise NotImplementedError

    @property
    def device(self):
        return next(self.module.parameters()).device

    @property
    def dtype(self):
        """Storage dtype of activations = dtype of the module's parameters (fp32, or bf16 after model.bfloat16())."""
        dt = next(self.module.parameters()).dtype
        if dt not in (torch.float32, torch.bfloat16):
            raise L.BevfError(f"unsupported parameter dtype {dt}: the HIP path stores fp32 or bf16")
        return dt

    def buf(self, name: str, numel: int, dtype=None) -> torch.Tensor:
        dtype = self.dtype if dtype is None else dtype
        t = self._bufs.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype or t.device != self.device:
            t = torch.empty(max(numel, 4), dtype=dtype, device=self.device)
            self._bufs[name] = t
        return t


class KernelTimer:
    """HIP-event brackets around individual launches on the current stream (bench.py's live roofline
    measurement).  Off unless installed with set_timer(); adds two event records per bracket."""

    def __init__(self):
        self.spans = []          # (name, start, end, flops, bytes)

    def bracket(self, name: str, flops: float = 0.0, nbytes: float = 0.0):
        timer = self

        class _Span:
            def __enter__(self_):
                self_.s = torch.cuda.Event(enable_timing=True)
                self_.e = torch.cuda.Event(enable_timing=True)
                self_.s.record()

            def __exit__(self_, *exc):
                self_.e.record()
                timer.spans.append((name, self_.s, self_.e, flops, nbytes))
        return _Span()

    def totals(self) -> Dict[str, Dict[str, float]]:
        """name -> {launches, ms, flops, bytes}; call after a device synchronize."""
        out: Dict[str, Dict[str, float]] = {}
        for name, s, e, fl, by in self.spans:
            d = out.setdefault(name, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += fl
            d["bytes"] += by
        return out


_TIMER: Optional[KernelTimer] = None


def set_timer(t: Optional[KernelTimer]) -> None:
    global _TIMER
    _TIMER = t


class _NoSpan:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def _span(name: str, flops: float = 0.0, nbytes: float = 0.0):
    return _TIMER.bracket(name, flops, nbytes) if _TIMER is not None else _NoSpan()


def _run_conv(pc: PackedConv, x, y, N, H, W, x_cs=None, y_cs=None, res=None, colmax=None, rows_per_group=0, tile=0):
    ho, wo = (H + 2 * pc.pad - pc.k) // pc.stride + 1, (W + 2 * pc.pad - pc.k) // pc.stride + 1
    flops = 2.0 * N * ho * wo * pc.cout * pc.k * pc.k * pc.cin          # algorithmic (direct convolution)
    with _span("conv_wino_f32" if pc.wino else ("conv3x3_bf16" if pc.c3 else "conv_igemm_f32"), flops=flops):
        _conv_call(pc, x, y, N, H, W, x_cs, y_cs, res, colmax, rows_per_group, tile)
    return ho, wo


def _conv_call(pc: PackedConv, x, y, N, H, W, x_cs=None, y_cs=None, res=None, colmax=None, rows_per_group=0, tile=0, run_if=None,
               group_rows=None):
    if pc.wino:
        L.conv3x3_wino(x, pc.w, pc.scale, pc.shift, y, N=N, H=H, W=W, Cin=pc.cin, x_cs=x_cs or pc.cin, Cout=pc.cout,
                       y_cs=y_cs or pc.cout, relu=pc.relu, res=res, res_cs=pc.cout if res is not None else 0)
        return
    if pc.c3:
        L.conv3x3_bf16(x, pc.w, pc.scale, pc.shift, y, N=N, H=H, W=W, Cin=pc.cin, x_cs=x_cs or pc.cin, Cout=pc.cout,
                       y_cs=y_cs or pc.cout, relu=pc.relu, res=res, res_cs=pc.cout if res is not None else 0)
        return
    L.conv2d_nhwc(x, pc.w, pc.scale, pc.shift, y, N=N, H=H, W=W, Cin=pc.cin, x_cs=x_cs or pc.cin, Cout=pc.cout,
                  y_cs=y_cs or pc.cout, KH=pc.k, KW=pc.k, stride=pc.stride, pad=pc.pad, relu=pc.relu, res=res,
                  res_cs=pc.cout if res is not None else 0, colmax=colmax, rows_per_group=rows_per_group, tile=tile, run_if=run_if,
                  group_rows=group_rows)


# ---- camera encoder (ref src/encoders.py:133-172) -----------------------------------------------------

FUSE_STEM_POOL = True        # inference: stem + max-pool as one kernel (csrc/stem.hip: stem_pool7x7, stem_pool7x7_bf16mma)


class CameraEncoderEngine(_Engine):
    def pack(self) -> None:
        m = self.module
        w = m.conv1.weight.detach().float()                             # (64,3,7,7); the stem computes in fp32
        assert tuple(w.shape) == (64, 3, 7, 7), "stem kernel supports the ResNet 7x7x3->64 stem only"
        packed = torch.zeros(148, 64, device=w.device)
        packed[:147] = w.reshape(64, 147).t()
        self.stem_w = packed.contiguous().view(-1)
        self.stem_scale, self.stem_shift = _bn_fold(None, m.bn1, 64, w.device)
        self.stem_w_bf16 = L.stem_pack_bf16(w) if self.dtype == torch.bfloat16 else None   # bf16 models: bf16-MFMA stem
        self.blocks = []
        for layer in (m.layer1, m.layer2, m.layer3):
            for blk in layer:
                down = None
                if blk.downsample is not None:
                    down = pack_conv(blk.downsample[0], blk.downsample[1], relu=False)
                self.blocks.append((pack_conv(blk.conv1, blk.bn1, True), pack_conv(blk.conv2, blk.bn2, True), down))
        self.proj = pack_conv(m.channel_proj[0], m.channel_proj[1], True)

    def run(self, x: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
        """x: (N,3,H,W) contiguous NCHW -> (NHWC buffer [N*Hc*Wc*Cout], Hc, Wc).
        The conv kernels address their operands with 32-bit byte offsets (buffer instructions), so a trunk activation
        must stay below 2 GiB: larger batches run the trunk in image chunks that write into one feature buffer."""
        self.ensure_packed()
        N, _, H, W = x.shape
        H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        H2, W2 = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
        es = 2 if self.dtype == torch.bfloat16 else 4
        n_max = max(1, ((1 << 31) - 1) // (H2 * W2 * 64 * es))
        h, w = H2, W2
        for c1, _, _ in self.blocks:
            h, w = (h + 2 - 3) // c1.stride + 1, (w + 2 - 3) // c1.stride + 1
        feat = self.buf("feat", N * h * w * self.proj.cout)
        if N <= n_max:
            self._run_chunk(x, N, H, W, feat)
        else:
            per = -(-N // -(-N // n_max))                    # balanced chunks
            for i0 in range(0, N, per):
                n = min(per, N - i0)
                self._run_chunk(x[i0:i0 + n], n, H, W, feat[i0 * h * w * self.proj.cout:])
        return feat, h, w

    def _run_chunk(self, x: torch.Tensor, N: int, H: int, W: int, feat: torch.Tensor) -> None:
        H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        H2, W2 = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
        cur = self.buf("act0", N * H2 * W2 * 64)
        if FUSE_STEM_POOL:
            # conv1 + bn1 + relu + maxpool in ONE kernel -- the stem map (4.4 GB fp32 / 2.2 GB bf16 at 48 images of 900x1600, the
            # largest activation of the path) never reaches HBM; bit-identical to the two kernels below
            with _span("stem_conv7x7_f32", flops=2.0 * N * H1 * W1 * 64 * 147):
                if self.stem_w_bf16 is not None:
                    L.stem_pool_bf16mma(x.float(), self.stem_w_bf16, self.stem_scale, self.stem_shift, cur, N, H, W)
                else:
                    L.stem_pool(x, self.stem_w, self.stem_scale, self.stem_shift, cur, N, H, W)
        else:
            stem = self.buf("stem", N * H1 * W1 * 64)
            with _span("stem_conv7x7_f32", flops=2.0 * N * H1 * W1 * 64 * 147):
                if self.stem_w_bf16 is not None:
                    L.stem_conv7x7_bf16mma(x.float(), self.stem_w_bf16, self.stem_scale, self.stem_shift, stem, N, H, W)
                else:
                    L.stem_conv7x7(x, self.stem_w, self.stem_scale, self.stem_shift, stem, N, H, W)
            L.maxpool3x3s2(stem, cur, N, H1, W1, 64)
        h, w = H2, W2
        ping = 0                                       # activations ping-pong between act0 / act1
        for c1, c2, down in self.blocks:
            ho, wo = (h + 2 - 3) // c1.stride + 1, (w + 2 - 3) // c1.stride + 1
            t = self.buf("tmp", N * ho * wo * c1.cout)
            _run_conv(c1, cur, t, N, h, w)
            idt = cur
            if down is not None:
                idt = self.buf("down", N * ho * wo * down.cout)
                _run_conv(down, cur, idt, N, h, w)
            ping ^= 1
            out = self.buf(f"act{ping}", N * ho * wo * c2.cout)
            _run_conv(c2, t, out, N, ho, wo, res=idt)
            cur, h, w = out, ho, wo
        _run_conv(self.proj, cur, feat, N, h, w)


# ---- shared per-point MLP + max (ref src/encoders.py:271-306) -------------------------------------------

FUSE_POINTNET_FRONT = True   # inference, fp32: conv1 -> conv2 -> conv3 as one kernel, activations in registers (csrc/pointnet_front.hip)


PRUNE_POINTNET_MAX = True    # inference, fp32: conv5's max over points through a bf16 bound pass + the exact kernel on candidate rows only
PRUNE_MIN_POINTS = 4096      # below this the exact launch over all points is already cheap
PRUNE_SEED_STRIDE = 4        # the seed launch runs every 4th row tile
PRUNE_CAP_SHARE = 0.16       # candidate slots per frame, as a share of its points (rounded up to 128)
# The bound's constants (derivation: DESIGN 3.2a2); csrc/conv_split.hip holds the three that the kernel applies itself.
PRUNE_REL_TRUNC = 4 * 2.0 ** -18     # two-plane truncation of both operands + the dropped mid*mid product
PRUNE_REL_ACC = 7 * 2.0 ** -24       # per K: 3 products accumulated with <= 2^-23 each in the bf16 MFMA + the exact kernel's 2^-24
PRUNE_NORM_INFLATE = 2.0 ** -10      # on |a_p| (kernel) and on bound_g (pack)
PRUNE_NORM_FLOOR = 2.0 ** -58        # added to |a_p| (kernel)
PRUNE_VAL_TERM = 2.0 ** -21          # eps += this * |val| (kernel): the fmaf and the +-eps roundings


def prune_rel(K: int) -> float:
    """|approximate - exact accumulator| <= prune_rel(K) * |a_p| * |w_c|."""
    return PRUNE_REL_TRUNC + PRUNE_REL_ACC * K


def prune_cap(N: int) -> int:
    """Candidate slots per frame of N points: ceil(share * N), rounded up to 128."""
    return -(-math.ceil(PRUNE_CAP_SHARE * N) // 128) * 128


def prune_bound_g(w: torch.Tensor, scale: torch.Tensor, K: int) -> torch.Tensor:
    """bound_g[c] = prune_rel(K) * |w_c| * |scale_c|, inflated and rounded up to fp32; w: [Cout][K] fp32."""
    g = prune_rel(K) * w.double().norm(dim=1) * scale.double().abs() * (1.0 + PRUNE_NORM_INFLATE)
    g32 = g.float()
    return torch.nextafter(g32, torch.full_like(g32, float("inf"))).contiguous()


class PrunedColMax:
    """max over each frame's rows of relu(x @ w^T * scale + shift) for a pointwise fp32 layer, bit-identical to the layer's colmax
    launch over all rows: a two-plane bf16 bound pass (seed launch on every k-th row tile, then all rows) flags the rows that can hold
    a channel's maximum, they are compacted into `cap` slots per frame, and the exact kernel runs on those.  If a frame overflows its
    slots, a device word lets the full launch run after all.  Nothing is read back and every launch has a fixed grid."""

    def __init__(self, pc: PackedConv):
        assert pc.k == 1 and pc.relu and not pc.wino and not pc.c3 and pc.w.dtype == torch.float32
        self.pc = pc
        self.planes = L.split_weights_f32x3(pc.w)
        self.g = prune_bound_g(pc.w.view(pc.cout, pc.cin), pc.scale, pc.cin)
        self._bufs: Dict[str, torch.Tensor] = {}

    def _buf(self, name: str, numel: int, dtype) -> torch.Tensor:
        t = self._bufs.get(name)
        if t is None or t.numel() < numel:
            t = torch.empty(numel, dtype=dtype, device=self.pc.w.device)
            self._bufs[name] = t
        return t

    def run(self, x: torch.Tensor, gmax: torch.Tensor, B: int, N: int, cap: Optional[int] = None, tile: int = 0) -> torch.Tensor:
        """x: [B*N][cin] fp32; gmax: [B][cout] int32, zeroed by the caller.  Returns the overflow word (device, int32).
        cap / tile: the tests' overrides of the slots per frame and of the bound pass's tile (bevf_conv2d_bound_f32x2)."""
        pc, M = self.pc, B * N
        cap = prune_cap(N) if cap is None else cap
        nthr, nb = B * pc.cout, -(-B // 4) * 4
        work = self._buf("work", 4 + nb + nthr + M, torch.int32)[:4 + nb + nthr + M]
        work.zero_()
        ovf, rows, thr, flag = work[:1], work[4:4 + B], work[4 + nb:4 + nb + nthr], work[4 + nb + nthr:]
        rp = self._buf("rp", B * (N + 1), torch.int32)
        cand = self._buf("cand", B * cap * pc.cin, torch.float32)
        geo = dict(M=M, Cin=pc.cin, Cout=pc.cout, rows_per_group=N, tile=tile)
        with _span("pointnet_prune_bound"):
            L.conv2d_bound(x, self.planes, pc.scale, pc.shift, self.g, thr, None, seed_stride=PRUNE_SEED_STRIDE, **geo)
            L.conv2d_bound(x, self.planes, pc.scale, pc.shift, self.g, thr, flag, **geo)
        with _span("pointnet_prune_compact"):
            L.prune_compact(x, flag, rp, cand, rows, ovf, B, N, pc.cin, cap)
        # the exact kernel on the candidate slots; it skips the tiles past a frame's candidates, so the rows it really multiplies are
        # known on the device only: a span of its own, outside the roofline's FLOP accounting
        with _span("pointnet_prune_exact"):
            _conv_call(pc, cand, None, B * cap, 1, 1, colmax=gmax, rows_per_group=cap, group_rows=rows)
        with _span("pointnet_prune_fallback"):
            _conv_call(pc, x, None, M, 1, 1, colmax=gmax, rows_per_group=N, run_if=ovf)
        return ovf


class PointNetEngine(_Engine):
    def pack(self) -> None:
        m = self.module
        convs = [getattr(m, f"conv{i}") for i in range(1, 6)]
        bns = [getattr(m, f"bn{i}") for i in range(1, 6)]
        w0 = convs[0].weight.detach()
        self.cin = w0.shape[1]
        self.w0 = w0.reshape(w0.shape[0], self.cin).float().contiguous()
        self.s0, self.b0 = _bn_fold(convs[0].bias, bns[0], w0.shape[0], w0.device)
        self.c0 = w0.shape[0]
        self.layers = [pack_conv(c, b, True) for c, b in zip(convs[1:], bns[1:])]   # the last layer fuses the max over points (colmax)
        # fused front (exact fp32 modes, the reference's 64 / 128 / 256 widths): conv2 / conv3 filters in MFMA fragment order
        self.front = None
        if (FUSE_POINTNET_FRONT and self.dtype == torch.float32 and _CONV_MODE in ("f32", "wino") and self.cin <= 8
                and len(convs) >= 4 and [c.weight.shape[0] for c in convs[:3]] == [64, 128, 256]):
            self.front = [L.pointnet_front_pack(c.weight.detach().reshape(c.weight.shape[0], -1)) for c in convs[1:3]]
        # pruned max over points for the last layer (exact fp32 modes only; PRUNE_POINTNET_MAX is read at run time)
        self.prune = None
        if self.dtype == torch.float32 and _CONV_MODE in ("f32", "wino"):
            self.prune = PrunedColMax(self.layers[-1])

    def run(self, pts: torch.Tensor, keep_last: bool = False):
        """pts: (B,N,C) contiguous -> (B, feat) global max feature [and the (B*N, feat) last activations].
        Frames are processed in chunks when an activation of the whole batch would pass the kernels' 2 GiB limit."""
        self.ensure_packed()
        B, N, Cc = pts.shape
        es = 2 if self.dtype == torch.bfloat16 else 4
        widest = max(pc.cout for pc in self.layers)
        f_max = max(1, ((1 << 31) - 1) // (max(N, 1) * widest * es))
        last = self.layers[-1]
        gmax = torch.zeros(B, last.cout, dtype=torch.int32, device=pts.device)
        if B <= f_max:
            y = self._run_frames(pts, gmax, keep_last)
            return gmax.view(torch.float32), y
        if keep_last:
            raise L.BevfError(f"PointNet: per-point features of {B}x{N} points exceed the 2 GiB activation limit")
        for b0 in range(0, B, f_max):
            self._run_frames(pts[b0:b0 + f_max], gmax[b0:b0 + f_max], False)
        return gmax.view(torch.float32), None

    def _run_frames(self, pts: torch.Tensor, gmax: torch.Tensor, keep_last: bool):
        B, N, Cc = pts.shape
        M = B * N
        if self.front is not None:
            l2, l3 = self.layers[0], self.layers[1]
            a = self.buf("l2", M * l3.cout)
            with _span("pointnet_front_f32", flops=2.0 * M * (l2.cin * l2.cout + l3.cin * l3.cout)):     # the two MFMA layers
                L.pointnet_front(pts.float(), self.w0, self.s0, self.b0, self.front[0], l2.scale, l2.shift, self.front[1],
                                 l3.scale, l3.shift, a, M, Cc)
            rest = list(enumerate(self.layers[:-1]))[2:]
        else:
            a = self.buf("l0", M * self.c0)
            L.pointwise_smallk(pts.float(), self.w0, self.s0, self.b0, a, M, Cc, self.c0, True)
            rest = list(enumerate(self.layers[:-1]))
        for i, pc in rest:
            o = self.buf(f"l{i + 1}", M * pc.cout)
            _run_conv(pc, a, o, M, 1, 1)
            a = o
        last = self.layers[-1]
        if self.prune is not None and PRUNE_POINTNET_MAX and not keep_last and N >= PRUNE_MIN_POINTS:
            self.prune.run(a, gmax, B, N)
            return None
        y = self.buf("l_last", M * last.cout) if keep_last else None
        _run_conv(last, a, y, M, 1, 1, colmax=gmax, rows_per_group=N)
        return y


FUSE_VFE = True              # VFELayer with <= 16 input channels as one kernel (False: pointwise_smallk + group_max, bit-identical)


class VFEEngine(_Engine):
    """VFELayer (ref src/encoders.py:431-455): Linear + BN1d + ReLU per point, max over the points of a voxel."""

    def pack(self) -> None:
        m = self.module
        w = m.linear.weight.detach()
        self.cin, self.cout = w.shape[1], w.shape[0]
        self.scale, self.shift = _bn_fold(m.linear.bias, m.bn, self.cout, w.device)
        self.w = w.float().contiguous()
        if self.cin > 16:
            if self.cin % 32:
                raise L.BevfError(f"VFELayer: in_channels={self.cin} must be <= 16 or a multiple of 32")
            self.pc = PackedConv(self.w.view(-1), self.scale, self.shift, self.cin, self.cout, 1, 1, 0, True)

    def run(self, x: torch.Tensor) -> torch.Tensor:
        self.ensure_packed()
        B, Nv, P, Cc = x.shape
        G, M = B * Nv, B * Nv * P
        if Cc <= 16:
            out = torch.empty(G, self.cout, device=x.device)
            if FUSE_VFE:
                L.vfe_smallk_max(x, self.w, self.scale, self.shift, out, G, P, Cc, self.cout)
                return out
            t = self.buf("pts", M * self.cout)
            L.pointwise_smallk(x, self.w, self.scale, self.shift, t, M, Cc, self.cout, True)
            L.group_max(t, out, G, P, self.cout)
            return out
        gmax = torch.zeros(G, self.cout, dtype=torch.int32, device=x.device)
        _run_conv(self.pc, x, None, M, 1, 1, colmax=gmax, rows_per_group=P)
        return gmax.view(torch.float32)


def pillar_voxelize(enc: nn.Module, pts: torch.Tensor, alloc) -> Tuple[L.PillarGeom, int, Tuple[torch.Tensor, ...]]:
    """voxelize on the encoder's one-pillar-per-cell grid into buffers from alloc(name, numel, dtype) -> (descriptor, B, buffers).
    The descriptor holds raw pointers: the caller keeps `buffers` alive as long as it uses it.  The buffers are not
    zero-filled: the pillar kernels read only rows < num_points of pillars < num_voxels."""
    if pts.dim() != 3 or pts.shape[2] != enc.input_channels:
        raise L.BevfError(f"PillarLiDAREncoder: points must be (B, N, {enc.input_channels}), got {tuple(pts.shape)}")
    pts = pts.float().contiguous()
    B, N, Cc = pts.shape
    P, Nv = enc.max_points, enc.max_pillars
    x0, y0, vx, vy, vsize = enc.grid()
    feats = alloc("vox_feats", B * Nv * P * Cc, torch.float32)
    coords = alloc("vox_coords", B * Nv * 3, torch.int64)
    npts = alloc("vox_npts", B * Nv, torch.int32)
    nvox = alloc("vox_nvox", B, torch.int32)
    work = alloc("vox_work", L.voxelize_work_bytes(B, N), torch.uint8)
    with _span("voxelize"):
        L.voxelize(pts, enc.pc_range, vsize, P, Nv, out=(feats, coords, npts, nvox, work))
    return (L.pillar_geom(feats, coords, npts, nvox, B, Nv, P, Cc, enc.bev_h, enc.bev_w, x0, y0, vx, vy), B,
            (feats, coords, npts, nvox))


class PillarEngine(_Engine):
    """PillarLiDAREncoder, eval mode: voxelize -> bevf_pillar_pfn_f32 (decoration, Linear + folded BN + ReLU, max over the
    pillar's rows) -> NHWC canvas [B][bev_h][bev_w][pfn_channels] in the storage dtype (the PFN computes in fp32)."""

    def pack(self) -> None:
        lin, bn = self.module.pfn.linear, self.module.pfn.bn
        self.cout, self.k = lin.weight.shape
        self.w = lin.weight.detach().float().contiguous()
        self.scale, self.shift = _bn_fold(lin.bias, bn, self.cout, lin.weight.device)

    def run(self, pts: torch.Tensor) -> torch.Tensor:
        self.ensure_packed()
        m = self.module
        g, B, _ = pillar_voxelize(m, pts, lambda name, n, dt: self.buf(name, n, dt))        # (buffers: the engine's own)
        n = B * m.bev_h * m.bev_w * self.cout
        canvas = self.buf("canvas", n)
        # algorithmic bytes: the occupied rows are not known on the host; the span carries the canvas write only
        with _span("pillar_pfn", flops=0.0, nbytes=float(canvas.element_size()) * n):
            L.pillar_pfn(g, self.w, self.scale, self.shift, self.cout, canvas)
        return canvas[:n].view(B, m.bev_h, m.bev_w, self.cout)


# ---- sparse-voxel LiDAR encoder ------------------------------------------------------------------------

# layer -> (level of its rows, level its taps look into, stride)
SPARSE_SPEC = dict(conv_in=(0, 0, 1), down1=(1, 0, 2), subm1=(1, 1, 1), down2=(2, 1, 2), subm2=(2, 2, 1))
SPARSE_KPAD = 32             # the first layer's point channels are zero-padded to the gather-GEMM's K granule


def sparse_pack_weight(conv: nn.Conv3d, transposed: bool = False) -> torch.Tensor:
    """Conv3d weight [Cout][Cin][3][3][3] -> [27][Cin padded to 32][Cout] fp32, tap k = (kz * 3 + ky) * 3 + kx.  transposed: the
    data gradient's [27][Cout][Cin]; a submanifold layer reuses its forward table there, so its taps are mirrored (k -> 26 - k)."""
    w = conv.weight.detach().float()
    cout, cin = w.shape[:2]
    wp = w.permute(2, 3, 4, 1, 0).reshape(27, cin, cout)
    if transposed:
        wp = wp.transpose(1, 2)
        if conv.stride[0] == 1:
            wp = wp.flip(0)
        return wp.contiguous().view(-1)
    if cin % SPARSE_KPAD:
        wp = torch.cat([wp, wp.new_zeros(27, SPARSE_KPAD - cin % SPARSE_KPAD, cout)], 1)
    return wp.contiguous().view(-1)


class SparseStructure:
    """What one batch's geometry gives the sparse layers: per level l the grid dims[l], the per-frame row capacity caps[l], the
    index volume, the rows' cells and the per-frame counts (device int32); per layer its neighbour table; x0, the mean-VFE rows
    of level 0 [B * caps[0]][32].  grad=True adds the input-side tables of the two strided layers (their data gradient)."""

    def __init__(self, enc: nn.Module, pts: torch.Tensor, alloc, grad: bool = False):
        if pts.dim() != 3 or pts.shape[2] != enc.input_channels:
            raise L.BevfError(f"SparseLiDAREncoder: points must be (B, N, {enc.input_channels}), got {tuple(pts.shape)}")
        pts = pts.float().contiguous()
        B, N, Cc = pts.shape
        P = enc.max_points
        self.B, self.P, self.C = B, P, Cc
        self.dims, self.caps = enc.level_dims()
        dims, caps = self.dims, self.caps
        _, vsize = enc.grid()
        I32 = torch.int32
        feats = alloc("vox_feats", B * caps[0] * P * Cc, torch.float32)
        coords = alloc("vox_coords", B * caps[0] * 3, torch.int64)
        npts = alloc("vox_npts", B * caps[0], I32)
        nvox = alloc("vox_nvox", B, I32)
        work = alloc("vox_work", L.voxelize_work_bytes(B, N), torch.uint8)
        with _span("voxelize"):
            L.voxelize(pts, enc.pc_range, vsize, P, caps[0], out=(feats, coords, npts, nvox, work))
        self.index = [alloc(f"sp_index{l}", B * d[0] * d[1] * d[2], I32) for l, d in enumerate(dims)]
        self.cell = [alloc(f"sp_cell{l}", B * caps[l], I32) for l in range(3)]
        self.count = [nvox, alloc("sp_count1", B, I32), alloc("sp_count2", B, I32)]
        with _span("sparse_structure"):
            L.sparse_fill_index(coords, nvox, B, caps[0], *dims[0], self.index[0], self.cell[0])
            for l in (1, 2):
                dwork = alloc("sp_down_work", L.sparse_down_work_bytes(B, *dims[l - 1]), torch.uint8)
                L.sparse_down(self.index[l - 1], B, *dims[l - 1], caps[l], self.index[l], self.cell[l], self.count[l], dwork)
            self.table = {}
            for name, (lr, li, stride) in SPARSE_SPEC.items():
                t = alloc(f"sp_tab_{name}", B * caps[lr] * 27, I32)
                L.sparse_table(self.index[li], self.cell[lr], self.count[lr], B, caps[lr], dims[li], dims[lr], stride, False, t)
                self.table[name] = t
            self.grad_table = {}
            if grad:
                for name in ("down1", "down2"):
                    lr, li, stride = SPARSE_SPEC[name]                 # rows = the layer's inputs (level li), taps look into level lr
                    t = alloc(f"sp_gtab_{name}", B * caps[li] * 27, I32)
                    L.sparse_table(self.index[lr], self.cell[li], self.count[li], B, caps[li], dims[lr], dims[li], stride, True, t)
                    self.grad_table[name] = t
        self.x0 = alloc("sp_x0", B * caps[0] * SPARSE_KPAD, torch.float32)
        with _span("sparse_vfe_mean"):
            L.sparse_vfe_mean(feats, npts, nvox, B, caps[0], P, Cc, SPARSE_KPAD, self.x0)
        self.keep = (feats, coords, npts)


class SparseLiDAREngine(_Engine):
    """SparseLiDAREncoder, eval mode: voxelize -> structure (index volumes, active sets, neighbour tables) -> mean VFE -> five
    bevf_sparse_conv_f32 launches with BatchNorm folded into scale / shift (+ ReLU) -> NHWC canvas [B][bev_h][bev_w][c2 * Dz / 4]
    in the storage dtype (the convolutions compute in fp32).  Row counts stay on the device: nothing here waits for the GPU."""

    def pack(self) -> None:
        self.layers = []
        for name, blk in zip(SPARSE_SPEC, self.module.layers()):
            cout = blk.conv.weight.shape[0]
            scale, shift = _bn_fold(None, blk.bn, cout, blk.conv.weight.device)
            self.layers.append((name, sparse_pack_weight(blk.conv), scale, shift, cout))

    def run(self, pts: torch.Tensor) -> torch.Tensor:
        self.ensure_packed()
        m = self.module
        s = SparseStructure(m, pts, lambda name, n, dt: self.buf(name, n, dt))
        B, caps = s.B, s.caps
        x, cin, rows_in = s.x0, SPARSE_KPAD, B * caps[0]
        for name, w, scale, shift, cout in self.layers:
            lr = SPARSE_SPEC[name][0]
            y = self.buf(f"sp_y_{name}", B * caps[lr] * cout, torch.float32)
            with _span(f"sparse_conv_f32:{name}"):
                L.sparse_conv(x, s.table[name], s.count[lr], w, scale, shift, B, caps[lr], rows_in, cin, cout, True, y)
            x, cin, rows_in = y, cout, B * caps[lr]
        D2, H2, W2 = s.dims[2]
        n = B * H2 * W2 * D2 * cin
        canvas = self.buf("canvas", n)
        with _span("sparse_canvas", nbytes=float(canvas.element_size()) * n):
            L.sparse_canvas(x, s.cell[2], s.count[2], B, caps[2], D2, H2, W2, cin, canvas)
        self.last = s                                                  # (tests read the structure of the last batch)
        return canvas[:n].view(B, H2, W2, D2 * cin)


class RadarEngine(_Engine):
    """MultiRadarEncoder: shared RadarEncoder per sweep + concat/max/mean (ref src/encoders.py:628-661)."""

    def pack(self) -> None:
        enc = self.module.radar_encoder
        self.cin = enc.conv1.weight.shape[1]
        self.ws, self.scales, self.shifts, self.widths = [], [], [], []
        for i in range(1, 5):
            conv, bn = getattr(enc, f"conv{i}"), getattr(enc, f"bn{i}")
            w = conv.weight.detach()
            self.ws.append(w.reshape(w.shape[0], w.shape[1]).t().float().contiguous())       # k-major, fp32 compute
            s, b = _bn_fold(conv.bias, bn, w.shape[0], w.device)
            self.scales.append(s); self.shifts.append(b); self.widths.append(w.shape[0])
        if self.module.fusion_method == "concat":
            fc = self.module.fusion_fc
            self.fc_w = fc.weight.detach().contiguous()                 # storage dtype (fp32 / bf16 weight stream)
            self.fc_b = fc.bias.detach().float().contiguous() if fc.bias is not None else None

    def run(self, radar_list: Sequence[torch.Tensor]) -> torch.Tensor:
        self.ensure_packed()
        R = len(radar_list)
        B = radar_list[0].shape[0]
        feat = self.widths[3]
        per = torch.zeros(B, R, feat, device=self.device)            # zero-filled: chunk maxima merge with atomicMax
        radar_list = [r.float() for r in radar_list]
        same = all(r.shape == radar_list[0].shape for r in radar_list)
        if same:
            x = torch.stack([r.contiguous() for r in radar_list], dim=0).contiguous()         # [R][B][P][Cin]
            L.radar_mlp_max(x, self.ws, self.scales, self.shifts, per, R, B, x.shape[2], self.cin, self.widths)
        else:
            for r, pts in enumerate(radar_list):
                one = torch.zeros(B, 1, feat, device=self.device)
                L.radar_mlp_max(pts.contiguous(), self.ws, self.scales, self.shifts, one, 1, B, pts.shape[1],
                                self.cin, self.widths)
                per[:, r] = one[:, 0]
        method = self.module.fusion_method
        if method == "concat":
            K = R * feat
            if K != self.fc_w.shape[1]:
                raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({B}x{K} and "
                                   f"{self.fc_w.shape[1]}x{self.fc_w.shape[0]})")
            out = torch.empty(B, self.fc_w.shape[0], device=self.device)
            L.linear(per, self.fc_w, self.fc_b, out, B, K, self.fc_w.shape[0], False)
            return out
        if method == "max":                                          # ref src/encoders.py:654-655
            out = torch.empty(B, feat, device=self.device)
            L.group_max(per, out, B, R, feat)
            return out
        if method == "mean":                                         # ref src/encoders.py:656-657
            out = torch.empty(B, feat, device=self.device)
            L.cam_mean(per, out, B, R, 1, feat)
            return out
        raise ValueError(f"Unknown fusion method: {method}")


# ---- BEV fusion (ref src/fusion.py:209-297) ----------------------------------------------------------------

@dataclass
class CameraTable:
    """camera_rig.ProjectionTable on the device: the cell table (rows = BEV cells) for the forward and its transpose (rows = camera
    feature pixels) for the backward, int32 / fp32."""
    P: int
    ncols: int
    row_ptr: torch.Tensor
    col: torch.Tensor
    w: torch.Tensor
    t_row_ptr: torch.Tensor
    t_col: torch.Tensor
    t_w: torch.Tensor

    @classmethod
    def from_host(cls, t, dev) -> "CameraTable":
        """camera_rig.ProjectionTable `t` copied to device `dev`."""
        return cls(t.P, t.ncols, *(torch.from_numpy(getattr(t, n)).to(dev) for n in ("row_ptr", "col", "w", "t_row_ptr", "t_col", "t_w")))

    def project(self, x, y, B: int, C: int, y_cs: Optional[int] = None) -> None:
        """y[b][cell][0:C] (row stride y_cs) = the lift of x = NHWC camera features [B][ncols][C]."""
        L.csr_gather(self.row_ptr, self.col, self.w, self.P, self.ncols, x, self.ncols * C, C, y, self.P * (y_cs or C),
                     y_cs or C, B, C)

    def project_backward(self, dy, dx, B: int, C: int) -> None:
        """dx [B][ncols][C] = the transpose applied to dy [B][P][C]: every element of dx written once."""
        L.csr_gather(self.t_row_ptr, self.t_col, self.t_w, self.ncols, self.P, dy, self.P * C, C, dx, self.ncols * C, C, B, C)


def _check_rig_cameras(fus: nn.Module, ncam: int) -> None:
    rig = fus.camera_rig
    if ncam != rig.num_cameras:
        raise L.BevfError(f"BEV fusion (camera_view_transform='{fus.camera_view_transform}'): the camera rig has {rig.num_cameras} "
                          f"cameras ({', '.join(rig.names)}) but the camera input has {ncam} (a 4-D input is one camera); pass "
                          f"(B, {rig.num_cameras}, C, H, W) features or call set_camera_rig() with a matching rig")


def _rig_cached(fus: nn.Module, kind: tuple, extra: tuple, what: str, dev, build):
    """What the fusion's engine caches for the module rig under kind + (rig key,) + extra + (device,), until set_camera_rig: built
    by build() on first use, which has to happen outside a graph capture (`what` names it in the refusal)."""
    tables = fus._eng()._camera_tables
    key = kind + (fus.camera_rig.key(),) + extra + (str(dev),)
    if key not in tables:
        if torch.cuda.is_current_stream_capturing():
            raise L.BevfError(f"BEV fusion: the camera {what} is built on first use, which cannot happen inside a graph "
                              "capture -- run the forward once before capturing")
        tables[key] = build()
    return tables[key]


def _grid_key(fus: nn.Module, Hc: int, Wc: int) -> tuple:
    return Hc, Wc, fus.bev_h, fus.bev_w, tuple(float(v) for v in fus.pc_range)


def camera_table(fus: nn.Module, ncam: int, Hc: int, Wc: int, dev) -> CameraTable:
    """The projection table of FlexibleBEVFusion `fus` ('project' branch) for ncam cameras of Hc x Wc features, built on the host in
    fp64 (camera_rig.build_projection_table) on first use and cached on the fusion's engine until set_camera_rig."""
    _check_rig_cameras(fus, ncam)
    heights = (fus.cam_num_heights, fus.cam_min_depth)
    return _rig_cached(fus, (), _grid_key(fus, Hc, Wc) + heights, "projection table", dev, lambda: CameraTable.from_host(
        CR.build_projection_table(fus.camera_rig, Hc, Wc, fus.pc_range, fus.bev_h, fus.bev_w, *heights), dev))


@dataclass
class CameraLiftTable:
    """camera_rig.LiftTable on the device ('lift' branch): the cell table with col2 = pixel * D + bin for the forward, the transpose
    (rows = camera feature pixels; cell, bin, weight per entry) for the backward, int32 / fp32."""
    P: int
    ncols: int
    D: int
    row_ptr: torch.Tensor
    col2: torch.Tensor
    w: torch.Tensor
    t_row_ptr: torch.Tensor
    t_cell: torch.Tensor
    t_bin: torch.Tensor
    t_w: torch.Tensor

    @classmethod
    def from_host(cls, t, dev) -> "CameraLiftTable":
        """camera_rig.LiftTable `t` copied to device `dev`."""
        return cls(t.P, t.ncols, t.D, *(torch.from_numpy(getattr(t, n)).to(dev)
                                        for n in ("row_ptr", "col2", "w", "t_row_ptr", "t_cell", "t_bin", "t_w")))

    def lift(self, x, pd, y, B: int, C: int, y_cs: Optional[int] = None) -> None:
        """y[b][cell][0:C] (row stride y_cs) = sum_e w_e pd[b][pix_e][bin_e] x[b][pix_e][0:C]: x NHWC features [B][ncols][C], pd the
        depth distribution [B][ncols][D]."""
        L.csr_lift(self.row_ptr, self.col2, self.w, self.P, self.ncols, self.D, x, self.ncols * C, C, pd, self.ncols * self.D, y,
                   self.P * (y_cs or C), y_cs or C, B, C)

    def lift_backward(self, x, pd, dy, dx, dpd, B: int, C: int) -> None:
        """dx [B][ncols][C] and dpd [B][ncols][D] from dy [B][P][C]: every element of both written once."""
        L.csr_lift_bwd(self.t_row_ptr, self.t_cell, self.t_bin, self.t_w, self.ncols, self.P, self.D, x, self.ncols * C, C, pd,
                       self.ncols * self.D, dy, self.P * C, C, dx, self.ncols * C, C, dpd, self.ncols * self.D, B, C)


def camera_lift_table(fus: nn.Module, ncam: int, Hc: int, Wc: int, dev) -> CameraLiftTable:
    """The lift table of FlexibleBEVFusion `fus` ('lift' branch) for ncam cameras of Hc x Wc features, built on the host in fp64
    (camera_rig.build_lift_table) on first use and cached on the fusion's engine, next to the projection tables, until
    set_camera_rig."""
    _check_rig_cameras(fus, ncam)
    heights = (fus.cam_num_heights, fus.cam_min_depth)
    key = _grid_key(fus, Hc, Wc) + heights + (fus.cam_depth,)
    return _rig_cached(fus, ("lift",), key, "lift table", dev, lambda: CameraLiftTable.from_host(
        CR.build_lift_table(fus.camera_rig, Hc, Wc, fus.pc_range, fus.bev_h, fus.bev_w, *heights, *fus.cam_depth), dev))


def depth_net_width(D: int) -> int:
    """Output channels the depth net is run with: D rounded up to the convolution kernels' 32-channel K step, because the data
    gradient of the layer reads its output channels as input channels (Cin % 32 == 0) and the weight gradient wants Cout % 4 == 0.
    The padding rows of the weight and the bias are zero and the softmax reads the first D columns only."""
    return (D + 31) // 32 * 32


def pad_depth_net(conv, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """depth_net's (weight [width][C][1][1], bias [width]) with zero rows appended."""
    D = conv.weight.shape[0]
    w = torch.nn.functional.pad(conv.weight.detach(), (0, 0, 0, 0, 0, 0, 0, width - D))
    b = torch.nn.functional.pad(conv.bias.detach().float(), (0, width - D))
    return w.contiguous(), b.contiguous()


class _DeviceTables:
    """What the tables built on the device from a calibration tensor share: the fusion engine they belong to, `version`, which
    counts the builds -- eager ones in build(), the replay of a captured one through invalidate(), which GraphedDetector calls: a
    tape that finds another version in its backward rebuilds from the calibration it kept -- and the grid the builds take."""

    def __init__(self, eng: "_Engine"):
        self.eng, self.version = eng, 0

    def invalidate(self) -> None:
        """The buffers are about to be rewritten by launches this object does not see (a graph replay of a captured build)."""
        self.version += 1

    def grid(self):
        """-> ((x0, y0, vx, vy) of the module's pillar grid, its z range rounded to fp32), as the table builds take them."""
        import numpy as np
        from .encoders import pillar_grid
        m = self.eng.module
        return pillar_grid(m.pc_range, m.bev_h, m.bev_w)[:4], (float(np.float32(m.pc_range[2])), float(np.float32(m.pc_range[5])))


class FrameCameraTables(_DeviceTables):
    """The per-frame sibling of CameraTable: one projection table per frame, built on the device from a [B][ncam][4][4] fp64
    calibration tensor (camera_rig.calib_matrices) into grow-only buffers of the fusion's engine, of the worst-case capacity
    P * num_heights * ncam * 4 entries per frame -- no host synchronisation and no allocation once the buffers exist, so build,
    transposition and gather run inside a graph capture.  `version`: _DeviceTables."""

    def __init__(self, eng: "_Engine"):
        super().__init__(eng)
        self.t_version = -1

    def build(self, calib: torch.Tensor, image_size, B: int, ncam: int, Hc: int, Wc: int) -> None:
        m = self.eng.module
        self.B, self.P, self.ncols = B, m.bev_h * m.bev_w, ncam * Hc * Wc
        self.cap = cap = L.camera_table_capacity(self.P, m.cam_num_heights, ncam)
        buf = self.eng.buf
        self.row_ptr = buf("ct_row_ptr", B * (self.P + 1), torch.int32)
        self.col = buf("ct_col", B * cap, torch.int32)
        self.w = buf("ct_w", B * cap, torch.float32)
        self.work = buf("ct_work", L.camera_table_work_elems(B, cap, max(self.P, self.ncols)), torch.int32)
        grid, z = self.grid()
        L.camera_table_build(calib, B, ncam, grid, m.bev_h, m.bev_w, z, m.cam_num_heights, m.cam_min_depth, image_size,
                             Hc, Wc, self.row_ptr, self.col, self.w, cap, self.work)
        self.version += 1

    def transpose(self) -> None:
        """The transposed tables of the current build (once per build)."""
        if self.t_version == self.version:
            return
        buf, B, cap = self.eng.buf, self.B, self.cap
        self.t_row_ptr = buf("ct_t_row_ptr", B * (self.ncols + 1), torch.int32)
        self.t_col = buf("ct_t_col", B * cap, torch.int32)
        self.t_w = buf("ct_t_w", B * cap, torch.float32)
        L.camera_table_transpose(self.row_ptr, self.col, self.w, cap, B, self.P, self.ncols, self.t_row_ptr, self.t_col, self.t_w,
                                 self.work)
        self.t_version = self.version

    def project(self, x, y, B: int, C: int, y_cs: Optional[int] = None) -> None:
        """y[b][cell][0:C] (row stride y_cs) = frame b's lift of x = NHWC camera features [B][ncols][C]."""
        L.csr_gather_frames(self.row_ptr, self.col, self.w, self.cap, self.P, self.ncols, x, self.ncols * C, C, y,
                            self.P * (y_cs or C), y_cs or C, B, C)

    def project_backward(self, dy, dx, B: int, C: int) -> None:
        """dx [B][ncols][C] = frame b's transposed table applied to dy [B][P][C]: every element of dx written once."""
        self.transpose()
        L.csr_gather_frames(self.t_row_ptr, self.t_col, self.t_w, self.cap, self.ncols, self.P, dy, self.P * C, C, dx,
                            self.ncols * C, C, B, C)


def _frame_tables(cls, fus: nn.Module, camera_calib, B: int, ncam: int, Hc: int, Wc: int, dev):
    """The fusion engine's one `cls` object (made on first use), built now on the current stream for camera_calib = (fp64
    [B, ncam, 4, 4] tensor, image_size) as FlexibleBEVFusion.camera_calib_tensor returns it."""
    calib, image_size = camera_calib
    if tuple(calib.shape) != (B, ncam, 4, 4):
        raise L.BevfError(f"BEV fusion: camera_calib is {tuple(calib.shape)} but the camera features are {B} frames of {ncam} cameras")
    eng = fus._eng()
    if cls not in eng._frame_tables:
        eng._frame_tables[cls] = cls(eng)
    eng._frame_tables[cls].build(calib.to(dev).contiguous(), image_size, B, ncam, Hc, Wc)
    return eng._frame_tables[cls]


def frame_camera_tables(fus: nn.Module, camera_calib, B: int, ncam: int, Hc: int, Wc: int, dev) -> FrameCameraTables:
    """The per-frame projection tables of FlexibleBEVFusion `fus` for camera_calib = (fp64 [B, ncam, 4, 4] tensor, image_size) as
    FlexibleBEVFusion.camera_calib_tensor returns it, built now on the current stream."""
    return _frame_tables(FrameCameraTables, fus, camera_calib, B, ncam, Hc, Wc, dev)


class FrustumTables(_DeviceTables):
    """The lift-splat tables of the 'frustum' branch (camera_rig.FrustumTable) on the device, built there from a [B][ncam][4][4] fp64
    calibration tensor (bevf_frustum_table_build_f64): cell_of [B][ncols * D] for the backward, row_ptr [B][P + 1] / col2
    [B][ncols * D] for the forward -- the capacity is exact, there are no weights.  Per-frame tables (own = False) live in grow-only
    buffers of the fusion's engine: no host synchronisation and no allocation once they exist, so build and pool run inside a graph
    capture; `version`: _DeviceTables.  The module rig's table (own = True) is the same build with
    B = 1 into tensors of its own, cached beside the other rig tables and applied to every frame with stride 0."""

    def __init__(self, eng: "_Engine", own: bool = False):
        super().__init__(eng)
        self.own = own

    def _buf(self, name: str, numel: int, dev) -> torch.Tensor:
        return torch.empty(numel, dtype=torch.int32, device=dev) if self.own else self.eng.buf(name, numel, torch.int32)

    def build(self, calib: torch.Tensor, image_size, B: int, ncam: int, Hc: int, Wc: int) -> None:
        m = self.eng.module
        self.D, dmin, dmax = m.cam_depth
        self.tables, self.P, self.ncols = B, m.bev_h * m.bev_w, ncam * Hc * Wc
        self.cap = cap = self.ncols * self.D
        dev = calib.device
        self.cell_of = self._buf("ft_cell_of", B * cap, dev)
        self.row_ptr = self._buf("ft_row_ptr", B * (self.P + 1), dev)
        self.col2 = self._buf("ft_col2", B * cap, dev)
        work = self._buf("ft_work", L.frustum_table_work_elems(B, ncam, m.bev_h, m.bev_w, self.D, Hc, Wc), dev)
        grid, z = self.grid()
        L.frustum_table_build(calib, B, ncam, grid, m.bev_h, m.bev_w, z, self.D, dmin, dmax, image_size, Hc, Wc,
                              self.cell_of, self.row_ptr, self.col2, work)
        self.version += 1

    def pool(self, x, pd, y, B: int, C: int, y_cs: Optional[int] = None) -> None:
        """y[b][cell][0:C] (row stride y_cs) = sum over the cell's (pix, d) of pd[b][pix][d] x[b][pix][0:C]: x NHWC features
        [B][ncols][C], pd the depth distribution [B][ncols][D]."""
        L.frustum_pool(self.row_ptr, self.col2, self.tables, self.cap, self.P, self.ncols, self.D, x, self.ncols * C, C, pd,
                       self.ncols * self.D, y, self.P * (y_cs or C), y_cs or C, B, C)

    def pool_backward(self, x, pd, dy, dx, dpd, B: int, C: int) -> None:
        """dx [B][ncols][C] and dpd [B][ncols][D] from dy [B][P][C]: every element of both written once."""
        L.frustum_pool_bwd(self.cell_of, self.tables, self.ncols, self.P, self.D, x, self.ncols * C, C, pd, self.ncols * self.D, dy,
                           self.P * C, C, dx, self.ncols * C, C, dpd, self.ncols * self.D, B, C)


def camera_frustum_table(fus: nn.Module, ncam: int, Hc: int, Wc: int, dev) -> FrustumTables:
    """The frustum table of FlexibleBEVFusion `fus`'s own rig for ncam cameras of Hc x Wc features: built on the device with B = 1
    on first use (outside a graph capture) and cached on the fusion's engine, next to the other rig tables, until set_camera_rig."""
    _check_rig_cameras(fus, ncam)

    def build():
        rig, tab = fus.camera_rig, FrustumTables(fus._eng(), own=True)
        tab.build(torch.from_numpy(CR.calib_matrices([rig])).to(dev), rig.image_size, 1, ncam, Hc, Wc)
        return tab
    return _rig_cached(fus, ("frustum",), _grid_key(fus, Hc, Wc) + (fus.cam_depth,), "frustum table", dev, build)


def frame_frustum_tables(fus: nn.Module, camera_calib, B: int, ncam: int, Hc: int, Wc: int, dev) -> FrustumTables:
    """The per-frame frustum tables of FlexibleBEVFusion `fus` for camera_calib = (fp64 [B, ncam, 4, 4] tensor, image_size) as
    FlexibleBEVFusion.camera_calib_tensor returns it, built now on the current stream."""
    _check_rig_cameras(fus, ncam)
    return _frame_tables(FrustumTables, fus, camera_calib, B, ncam, Hc, Wc, dev)


def concat_slots(fus: nn.Module, branches, feats, text: str, B: Optional[int] = None):
    """-> ((branch, input) of every modality that has both, in slot order [camera, LiDAR, radar, history]; channels of the concatenated
    map, checked against bev_fusion's first conv; frames B, the first input's leading dimension unless given).  text: the mismatch
    message (FusionEngine's is torch's own, training.FusionTape has another).  The history input of a module with temporal fusion
    is the (prev_bev, ego, host ego) triple of temporal.check_history -- never None, so its slot is always present; prev_bev None
    inside it is a first frame."""
    present = [(b, x) for b, x in zip(branches, feats) if b is not None and x is not None]
    if all(getattr(b, "is_history", False) for b, _ in present):          # (none at all, or the history alone)
        raise ValueError("No modality features provided")
    B = B or present[0][1].shape[0]
    ccs = fus.bev_channels * len(present)
    cout, cin = fus.bev_fusion[0].weight.shape[:2]
    if ccs != cin:
        raise RuntimeError(text.format(cout=cout, cin=cin, B=B, ccs=ccs, h=fus.bev_h, w=fus.bev_w))
    return present, ccs, B


class _FusionBranch:
    """One input branch of FusionEngine: pack(m) folds its weights, run(x, B, out, ccs, cam_geom, camera_calib) turns the branch input
    x into the concat slice it owns (out = concat[slot * bc:], bev_channels wide, row stride ccs).  Workspaces: the engine's buf()."""

    def __init__(self, eng: "FusionEngine"):
        self.eng, m = eng, eng.module
        self.grid = (m.bev_h, m.bev_w, m.bev_channels)


class _CameraBranch(_FusionBranch):
    TABLES = None        # view-transform branches: (the rig-table getter, the per-frame getter, the span name of its build)

    def pack(self, m) -> None:
        self.c1 = pack_conv(m.camera_proj[0], m.camera_proj[1], True)
        self.c2 = pack_conv(m.camera_proj[3], m.camera_proj[4], True)

    def table(self, cam, B, geom, camera_calib):
        """camera_calib None: the module rig's cached table; else per-frame tables built here into the engine's buffers."""
        _, ncam, Hc, Wc = geom
        rig_table, frame_tables, span = self.TABLES
        if camera_calib is None:
            return rig_table(self.eng.module, ncam, Hc, Wc, cam.device)
        with _span(span):
            return frame_tables(self.eng.module, camera_calib, B, ncam, Hc, Wc, cam.device)

    def on_grid(self, span, transform, B, out, ccs) -> None:
        """The tail of a view-transform branch: transform(proj) fills the cam_proj buffer [B][S_h * S_w][C] under `span`, then
        camera_proj on the BEV grid, its second conv into the concat slice."""
        buf, (Sh, Sw, _) = self.eng.buf, self.grid
        proj = buf("cam_proj", B * Sh * Sw * self.c1.cin)
        with span:
            transform(proj)
        t1 = buf("cam_t1", B * Sh * Sw * self.c1.cout)
        _run_conv(self.c1, proj, t1, B, Sh, Sw)
        _run_conv(self.c2, t1, out, B, Sh, Sw, y_cs=ccs)


class CameraMeanBranch(_CameraBranch):
    """The reference's camera branch: camera average, camera_proj on the image grid, bilinear resize into the concat slice."""

    def run(self, cam, B, out, ccs, geom, _) -> None:
        _, ncam, Hc, Wc = geom
        buf, (Sh, Sw, bc), Cc = self.eng.buf, self.grid, self.c1.cin
        pooled = cam
        if ncam > 1:
            pooled = buf("cam_mean", B * Hc * Wc * Cc)
            with _span("bev_pool", nbytes=float(cam.element_size()) * B * Hc * Wc * Cc * (ncam + 1)):
                L.cam_mean(cam, pooled, B, ncam, Hc * Wc, Cc)
        t1 = buf("cam_t1", B * Hc * Wc * self.c1.cout)
        _run_conv(self.c1, pooled, t1, B, Hc, Wc)
        t2 = buf("cam_t2", B * Hc * Wc * self.c2.cout)
        _run_conv(self.c2, t1, t2, B, Hc, Wc)
        with _span("bev_pool", nbytes=float(t2.element_size()) * B * bc * (Hc * Wc + Sh * Sw)):
            L.bilinear_nhwc(t2, out, B, Hc, Wc, bc, bc, Sh, Sw, ccs)


class CameraProjectBranch(_CameraBranch):
    """The same camera_proj after camera rig -> BEV grid (one gather), its second conv into the concat slice.  camera_calib None:
    the module rig's cached table; else per-frame tables built here into the engine's buffers."""

    TABLES = (camera_table, frame_camera_tables, "cam_table_build")

    def run(self, cam, B, out, ccs, geom, camera_calib) -> None:
        (Sh, Sw, _), Cc = self.grid, self.c1.cin
        tab = self.table(cam, B, geom, camera_calib)
        span = _span("cam_project", nbytes=float(cam.element_size()) * B * Cc * (tab.ncols + Sh * Sw))
        self.on_grid(span, lambda proj: tab.project(cam, proj, B, Cc), B, out, ccs)


class CameraLiftBranch(_CameraBranch):
    """Learned depth: depth_net (exact 1x1 conv + bias) -> softmax over the depth bins -> the lift gather through
    the module rig's cached lift table -> camera_proj on the BEV grid, its second conv into the concat slice.  fp32, static rig."""

    TABLES, SPAN = (camera_lift_table, None, None), "cam_lift"         # (a calibration is refused: the rig's table only)

    def pack(self, m) -> None:
        super().pack(m)
        self.D = m.depth_net.weight.shape[0]
        self.Dp = depth_net_width(self.D)
        w, b = pad_depth_net(m.depth_net, self.Dp)
        Cc = w.shape[1]
        self.dn = _finish_pack(w.permute(0, 2, 3, 1).contiguous().view(-1), torch.ones(self.Dp, device=w.device), b, Cc, self.Dp,
                               1, 1, 0, False, split_ok=False, wino_ok=False)

    def depth_distribution(self, cam, N: int, Hc: int, Wc: int) -> torch.Tensor:
        """Pd [N * Hc * Wc][D] = softmax over the depth bins of depth_net's logits, for N feature maps."""
        rows = N * Hc * Wc
        logits = self.eng.buf("lift_logits", rows * self.Dp)
        _run_conv(self.dn, cam, logits, N, Hc, Wc)
        pd = self.eng.buf("lift_pd", rows * self.D)
        with _span("cam_lift_softmax", nbytes=4.0 * rows * (self.Dp + self.D)):
            L.softmax_rows(logits, self.Dp, pd, self.D, rows, self.D)
        return pd

    def spread(self, tab, cam, pd, proj, B, Cc) -> None:
        tab.lift(cam, pd, proj, B, Cc)

    def run(self, cam, B, out, ccs, geom, camera_calib) -> None:
        _, ncam, Hc, Wc = geom
        (Sh, Sw, _), Cc, m = self.grid, self.c1.cin, self.eng.module
        m.check_lift_supported(camera_calib)                       # (each looks at its own kind only, as in FlexibleBEVFusion.forward)
        m.check_frustum_supported()
        tab = self.table(cam, B, geom, camera_calib)
        pd = self.depth_distribution(cam, B * ncam, Hc, Wc)
        span = _span(self.SPAN, nbytes=4.0 * B * (Cc * (tab.ncols + Sh * Sw) + tab.ncols * self.D))
        self.on_grid(span, lambda proj: self.spread(tab, cam, pd, proj, B, Cc), B, out, ccs)


class CameraFrustumBranch(CameraLiftBranch):
    """Lift-splat: depth_net and softmax as in 'lift', then the pool over the frustum table -- the module rig's,
    built on the device once and shared by every frame, or per-frame tables built here from camera_calib into the engine's buffers
    -- and camera_proj on the BEV grid, its second conv into the concat slice.  fp32."""

    TABLES, SPAN = (camera_frustum_table, frame_frustum_tables, "cam_frustum_table"), "cam_frustum_pool"

    def spread(self, tab, cam, pd, proj, B, Cc) -> None:
        tab.pool(cam, pd, proj, B, Cc)


class LidarVectorBranch(_FusionBranch):
    """Input: the PointNet vector (B, C_l).  lidar_init to a start_size^2 canvas, conv, x2 bilinear, conv into the concat slice."""

    def pack(self, m) -> None:
        l0, l2 = m.lidar_init[0], m.lidar_init[2]
        self.li0 = (l0.weight.detach().contiguous(), l0.bias.detach().float().contiguous())
        self.li2 = (l2.weight.detach().contiguous(), l2.bias.detach().float().contiguous())
        self.up1 = pack_conv(m.lidar_upsample[0], m.lidar_upsample[1], True)
        self.up2 = pack_conv(m.lidar_upsample[4], m.lidar_upsample[5], True)

    def run(self, x, B, out, ccs, *_) -> None:
        buf, (Sh, Sw, bc), s0 = self.eng.buf, self.grid, self.eng.module.lidar_start_size
        hid = buf("lid_h", B * self.li0[0].shape[0], torch.float32)       # small per-frame vectors stay fp32
        L.linear(x.float().contiguous(), self.li0[0], self.li0[1], hid, B, self.li0[0].shape[1], self.li0[0].shape[0], True)
        O = self.li2[0].shape[0]
        ch = O // (s0 * s0)
        grid0 = buf("lid_g0", B * O)
        L.linear(hid, self.li2[0], self.li2[1], grid0, B, self.li2[0].shape[1], O, False, s0 * s0, ch)
        g1 = buf("lid_g1", B * s0 * s0 * self.up1.cout)
        _run_conv(self.up1, grid0, g1, B, s0, s0)
        s1 = 2 * s0
        g2 = buf("lid_g2", B * s1 * s1 * self.up1.cout)
        L.bilinear_nhwc(g1, g2, B, s0, s0, self.up1.cout, self.up1.cout, s1, s1, self.up1.cout)
        if (s1, s1) == (Sh, Sw):
            _run_conv(self.up2, g2, out, B, s1, s1, y_cs=ccs)
        else:
            # extension beyond the reference (which crashes at the concat for BEV != 50x50):
            # bilinear resize of the 50x50 LiDAR map, exactly like the camera branch
            g3 = buf("lid_g3", B * s1 * s1 * bc)
            _run_conv(self.up2, g2, g3, B, s1, s1)
            L.bilinear_nhwc(g3, out, B, s1, s1, bc, bc, Sh, Sw, ccs)


class LidarPillarsBranch(_FusionBranch):
    """Input: the PointPillars NHWC canvas (B, S_h, S_w, pfn_channels) in the storage dtype, already on the fusion grid -- two
    conv+BN+ReLU, the second into the concat slice."""

    def pack(self, m) -> None:
        self.c1 = pack_conv(m.lidar_bev[0], m.lidar_bev[1], True)
        self.c2 = pack_conv(m.lidar_bev[3], m.lidar_bev[4], True)

    def run(self, x, B, out, ccs, *_) -> None:
        Sh, Sw, _ = self.grid
        if x.dim() != 4 or tuple(x.shape[1:]) != (Sh, Sw, self.c1.cin) or x.dtype != self.eng.dtype:
            raise L.BevfError(f"BEV fusion (PointPillars): expected an NHWC {self.eng.dtype} canvas (B, {Sh}, {Sw}, {self.c1.cin}), "
                              f"got {x.dtype} {tuple(x.shape)}")
        t = self.eng.buf("lid_bev1", B * Sh * Sw * self.c1.cout)
        _run_conv(self.c1, x, t, B, Sh, Sw)
        _run_conv(self.c2, t, out, B, Sh, Sw, y_cs=ccs)


class RadarBranch(_FusionBranch):
    """Input: the radar vector (B, C_r).  radar_proj, broadcast to every cell, radar_refine's two conv+BN+ReLU."""

    def pack(self, m) -> None:
        r0 = m.radar_proj[0]
        self.rp = (r0.weight.detach().contiguous(), r0.bias.detach().float().contiguous())
        # exact kernel whatever the mode: the 5x5 border-class shortcut below must reproduce the full-map convolution
        # bit for bit, which a position-dependent Winograd tiling would not (and these two launches cost nothing)
        self.c1 = pack_conv(m.radar_refine[0], m.radar_refine[1], True, wino_ok=False)
        self.c2 = pack_conv(m.radar_refine[3], m.radar_refine[4], True, wino_ok=False)

    def run(self, x, B, out, ccs, *_) -> None:
        buf, (Sh, Sw, bc) = self.eng.buf, self.grid
        rv = buf("rad_v", B * bc, torch.float32)
        L.linear(x.float().contiguous(), self.rp[0], self.rp[1], rv, B, self.rp[0].shape[1], bc, True)
        # exact shortcut: two 3x3/pad-1 convs on a constant image have 5x5 distinct pixels (bevpool.hip)
        collapse = Sh >= 5 and Sw >= 5 and self.eng.collapse_radar
        h, w = (5, 5) if collapse else (Sh, Sw)
        r0 = buf("rad_0", B * h * w * bc)
        L.broadcast_nhwc(rv, r0, B, h * w, bc, bc)
        r1 = buf("rad_1", B * h * w * bc)
        _run_conv(self.c1, r0, r1, B, h, w)
        if collapse:
            r2 = buf("rad_2", B * 25 * bc)
            _run_conv(self.c2, r1, r2, B, 5, 5)
            L.expand_border_classes(r2, out, B, Sh, Sw, bc, ccs)
        else:
            _run_conv(self.c2, r1, out, B, Sh, Sw, y_cs=ccs)


def history_slot(out: torch.Tensor, B: int, P: int, bc: int, ccs: int) -> torch.Tensor:
    """The [B * P][bc] window (row stride ccs) that starts at out[0]."""
    return torch.as_strided(out, (B * P, bc), (ccs, 1))


class HistoryBranch(_FusionBranch):
    """Temporal fusion.  Input: (prev_bev (B, bev_channels, S_h, S_w) in the storage dtype or None, ego fp64
    [B][4][4] on the device, its host copy or None).  The previous map warped by ego-motion straight into the concat slice; a first
    frame (prev_bev None) zero-fills it.  No weights."""

    is_history = True

    def pack(self, m) -> None:
        pass

    def run(self, x, B, out, ccs, *_) -> None:
        from .encoders import pillar_grid
        prev, ego, _host = x
        (Sh, Sw, bc), m = self.grid, self.eng.module
        if prev is None:
            history_slot(out, B, Sh * Sw, bc, ccs).zero_()
            return
        rows = prev.permute(0, 2, 3, 1).contiguous()               # (a view of channels-last memory)
        with _span("bev_warp", nbytes=2.0 * rows.element_size() * B * Sh * Sw * bc):
            L.bev_warp(rows, out, ego, B, Sh, Sw, bc, bc, ccs, pillar_grid(m.pc_range, Sh, Sw)[:4])


class FusionEngine(_Engine):
    collapse_radar = True        # set False to run radar_refine on the full map (tests compare both, bit for bit)
    BRANCHES = dict(mean=CameraMeanBranch, project=CameraProjectBranch, lift=CameraLiftBranch, frustum=CameraFrustumBranch,
                    pointnet=LidarVectorBranch, pillars=LidarPillarsBranch, sparse=LidarPillarsBranch)

    def __init__(self, module: nn.Module):
        super().__init__(module)
        self._camera_tables: Dict[tuple, CameraTable] = {}
        self._frame_tables: Dict[type, _DeviceTables] = {}          # the per-frame tables, one object per class (_frame_tables)
        m = module
        self.branches = [self.BRANCHES[m.camera_view_transform](self) if m.use_camera else None,
                         self.BRANCHES[m.lidar_kind](self) if m.use_lidar else None, RadarBranch(self) if m.use_radar else None,
                         HistoryBranch(self) if getattr(m, "temporal", False) else None]

    def drop_camera_tables(self) -> None:
        self._camera_tables.clear()

    def invalidate_frame_tables(self) -> None:
        """A graph replay is about to rebuild the per-frame tables (FrameCameraTables.invalidate, FrustumTables.invalidate)."""
        for tables in self._frame_tables.values():
            tables.invalidate()

    def pack(self) -> None:
        m = self.module
        for branch in filter(None, self.branches):
            branch.pack(m)
        self.f1 = pack_conv(m.bev_fusion[0], m.bev_fusion[1], True)
        self.f2 = pack_conv(m.bev_fusion[3], m.bev_fusion[4], True)

    def run(self, cam: Optional[torch.Tensor], cam_geom: Optional[Tuple[int, int, int, int]],
            lidar: Optional[torch.Tensor], radar: Optional[torch.Tensor], camera_calib=None, history=None) -> Tuple[torch.Tensor, int]:
        """cam: NHWC encoder features [B*ncam][Hc][Wc][C] with cam_geom = (B, ncam, Hc, Wc); lidar (B,1024), or with a
        PointPillars branch the NHWC canvas (B, S_h, S_w, pfn_channels) in the storage dtype; radar (B,256).  camera_calib
        ('project' / 'frustum' branches): (fp64 [B, ncam, 4, 4], image_size) for per-frame tables built here, None = the module rig's table.
        history (a module with temporal fusion): the triple of temporal.check_history; None = a first frame.
        Returns the fused NHWC map [B][S_h*S_w][bev_channels] and B."""
        self.ensure_packed()
        m = self.module
        Sh, Sw, bc = m.bev_h, m.bev_w, m.bev_channels
        P = Sh * Sw
        text = ("Given groups=1, weight of size [{cout}, {cin}, 3, 3], expected input[{B}, {ccs}, {h}, {w}] to have {cin} channels, "
                "but got {ccs} channels instead")
        if self.branches[3] is not None and history is None:
            history = (None, None, None)
        present, ccs, B = concat_slots(m, self.branches, (cam, lidar, radar, history), text, cam_geom and cam_geom[0])
        concat = self.buf("concat", B * P * ccs)
        for slot, (branch, x) in enumerate(present):
            branch.run(x, B, concat[slot * bc:], ccs, cam_geom, camera_calib)
        f1 = self.buf("fus_1", B * P * self.f1.cout)
        _run_conv(self.f1, concat, f1, B, Sh, Sw)
        out = self.buf("fus_2", B * P * self.f2.cout)
        _run_conv(self.f2, f1, out, B, Sh, Sw)
        return out, B


# ---- CenterNet head (ref src/fusion.py:869-884) --------------------------------------------------------------

HEAD_BRANCHES = ("heatmap", "offset", "size", "rot", "vel")


@dataclass
class HeadWeights:
    """CenterNetHead's five branches (HEAD_BRANCHES order) concatenated for two launches: w3 [5*hc][Cin][3][3] / b3 the 3x3 convs
    along Cout, w1 [sum cs][hc] / b1 the 1x1 tails; convs3 / convs1 the branch modules the gradients belong to."""
    convs3: List[nn.Module]
    convs1: List[nn.Module]
    hc: int
    cs: List[int]
    w3: torch.Tensor
    b3: torch.Tensor
    w1: torch.Tensor
    b1: torch.Tensor


def head_weights(head: nn.Module) -> HeadWeights:
    """The head's weights as HeadWeights, in the module's dtype (HeadEngine.pack and training.HeadTape)."""
    convs3 = [getattr(head, f"{n}_head")[0] for n in HEAD_BRANCHES]
    convs1 = [getattr(head, f"{n}_head")[2] for n in HEAD_BRANCHES]
    hc = convs3[0].weight.shape[0]
    return HeadWeights(convs3, convs1, hc, [c.weight.shape[0] for c in convs1],
                       torch.cat([c.weight.detach() for c in convs3], 0), torch.cat([c.bias.detach() for c in convs3], 0),
                       torch.cat([c.weight.detach().reshape(c.weight.shape[0], hc) for c in convs1], 0),
                       torch.cat([c.bias.detach() for c in convs1], 0))


class HeadEngine(_Engine):
    def pack(self) -> None:
        hw = head_weights(self.module)
        self.hc, self.cs = hw.hc, hw.cs
        self.conv = _finish_pack(hw.w3.permute(0, 2, 3, 1).contiguous().view(-1), None, hw.b3.float().contiguous(),
                                 hw.w3.shape[1], hw.w3.shape[0], 3, 1, 1, True)
        self.w1 = hw.w1.float().contiguous()
        self.b1 = hw.b1.float().contiguous()

    def run(self, bev_nhwc: torch.Tensor, B: int, H: int, W: int) -> Dict[str, torch.Tensor]:
        self.ensure_packed()
        P = H * W
        hid = self.buf("hid", B * P * self.conv.cout)
        _run_conv(self.conv, bev_nhwc, hid, B, H, W)
        outs = [torch.empty(B, c, H, W, device=bev_nhwc.device) for c in self.cs]        # fp32 also on the bf16 path
        L.head_tail(hid, self.w1, self.b1, outs, B, P, self.hc, self.cs, self.cs[0])
        return dict(zip(HEAD_BRANCHES, outs))


# ---- BEV map-segmentation head (seg_head.BEVSegmentationHead) ---------------------------------------------

class SegHeadEngine(_Engine):
    """Eval mode: the grid resample onto the map grid, the classifier's two conv3x3 + folded BN + ReLU, and its 1x1 layer padded
    with zero rows to depth_net_width (pad_depth_net: the width the convolution kernels take for any class count), then the
    NHWC -> NCHW copy of the first num_classes columns.  fp32 or bf16 storage; the logits come out fp32."""

    def pack(self) -> None:
        cl = self.module.classifier
        self.c1 = pack_conv(cl[0], cl[1], True)
        self.c2 = pack_conv(cl[3], cl[4], True)
        self.Kp = depth_net_width(self.module.num_classes)
        w, b = pad_depth_net(cl[6], self.Kp)
        self.c3 = _finish_pack(w.permute(0, 2, 3, 1).contiguous().view(-1), torch.ones(self.Kp, device=w.device), b, w.shape[1],
                               self.Kp, 1, 1, 0, False, split_ok=False, wino_ok=False)

    def run(self, bev_nhwc: torch.Tensor, B: int) -> torch.Tensor:
        """bev_nhwc: the flat NHWC map [B][bev_h][bev_w][in_channels] in the storage dtype -> logits (B, K, Ho, Wo) fp32."""
        self.ensure_packed()
        m = self.module
        (Ho, Wo), Cc, K = m.output_size, m.in_channels, m.num_classes
        P = Ho * Wo
        if bev_nhwc.dtype != self.dtype or bev_nhwc.numel() < B * m.bev_h * m.bev_w * Cc:
            raise L.BevfError(f"BEVSegmentationHead: expected a {self.dtype} NHWC map of {B} x {m.bev_h} x {m.bev_w} x {Cc} elements, "
                              f"got {bev_nhwc.dtype} x {bev_nhwc.numel()}")
        r = self.buf("seg_in", B * P * Cc)
        with _span("bev_grid_resample", nbytes=float(r.element_size()) * B * Cc * (m.bev_h * m.bev_w + P)):
            L.bev_grid_resample(bev_nhwc, r, B, m.bev_h, m.bev_w, Ho, Wo, Cc, Cc, Cc, m.in_grid, m.out_grid)
        a1 = self.buf("seg_1", B * P * self.c1.cout)
        _run_conv(self.c1, r, a1, B, Ho, Wo)
        a2 = self.buf("seg_2", B * P * self.c2.cout)
        _run_conv(self.c2, a1, a2, B, Ho, Wo)
        logits = self.buf("seg_logits", B * P * self.Kp)
        _run_conv(self.c3, a2, logits, B, Ho, Wo)
        out = torch.empty(B, K, Ho, Wo, device=bev_nhwc.device)
        L.nhwc_to_nchw(logits.float(), out, B, K, P, self.Kp)
        return out


# ---- IoU-aware head (iou_head.IoUHead) ---------------------------------------------------------------------

class IoUHeadEngine(_Engine):
    """Eval mode: the branch's conv3x3 + bias + ReLU as a packed convolution, its 1x1 layer padded with zero rows to
    depth_net_width (the route of the seg head's last layer; bevf_head_tail_f32 is laid out for the five detection branches), then
    the NHWC -> NCHW copy of the first column.  fp32 or bf16 storage; the map comes out fp32."""

    def pack(self) -> None:
        br = self.module.branch
        self.c1 = pack_conv(br[0], None, True)
        self.Kp = depth_net_width(1)
        w, b = pad_depth_net(br[2], self.Kp)
        self.c2 = _finish_pack(w.permute(0, 2, 3, 1).contiguous().view(-1), torch.ones(self.Kp, device=w.device), b, w.shape[1],
                               self.Kp, 1, 1, 0, False, split_ok=False, wino_ok=False)

    def run(self, bev_nhwc: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        """bev_nhwc: the flat NHWC map [B][H][W][in_channels] in the storage dtype -> (B, 1, H, W) fp32."""
        self.ensure_packed()
        Cc, P = self.module.in_channels, H * W
        if bev_nhwc.dtype != self.dtype or bev_nhwc.numel() < B * P * Cc:
            raise L.BevfError(f"IoUHead: expected a {self.dtype} NHWC map of {B} x {H} x {W} x {Cc} elements, got {bev_nhwc.dtype} x "
                              f"{bev_nhwc.numel()}")
        hid = self.buf("iou_hid", B * P * self.c1.cout)
        _run_conv(self.c1, bev_nhwc, hid, B, H, W)
        cols = self.buf("iou_cols", B * P * self.Kp)
        _run_conv(self.c2, hid, cols, B, H, W)
        out = torch.empty(B, 1, H, W, device=bev_nhwc.device)
        L.nhwc_to_nchw(cols.float(), out, B, 1, P, self.Kp)
        return out


# ---- CenterPoint second stage (roi_head.RoIHead) -----------------------------------------------------------------

class RoIHeadEngine(_Engine):
    """Eval mode: the five-point gather, then three launches of the 1x1 convolution kernel over the (1, B*K, 1, .) row image --
    the two shared layers with BatchNorm folded and ReLU, and cls_out / reg_out as one 8-channel layer (zero rows up to
    depth_net_width).  fp32 or bf16 storage; pred comes out fp32.  Widths that are no multiple of the kernel's K granule (32
    channels fp32, 64 bf16) are padded with zero weights (the gathered rows are then copied into a padded buffer); at the default
    widths (5 * 256 -> 256 -> 256) nothing is padded."""

    def pack(self) -> None:
        m = self.module
        g = 64 if self.dtype == torch.bfloat16 else 32
        pad = lambda n: -(-n // g) * g
        self.C5, F = 5 * m.in_channels, m.fc
        self.C5p, self.Fp = pad(self.C5), pad(F)
        fc = m.shared_fc

        def layer(w, scale, shift, cinp, coutp, relu):
            cout, cin = w.shape
            wp = torch.nn.functional.pad(w.detach(), (0, cinp - cin, 0, coutp - cout)).contiguous().view(-1)
            scale = torch.nn.functional.pad(scale, (0, coutp - cout), value=1.0).contiguous()
            shift = torch.nn.functional.pad(shift, (0, coutp - cout)).contiguous()
            return _finish_pack(wp, scale, shift, cinp, coutp, 1, 1, 0, relu, split_ok=relu, wino_ok=False)

        self.c1 = layer(fc[0].weight, *_bn_fold(None, fc[1], F, self.device), self.C5p, self.Fp, True)
        self.c2 = layer(fc[3].weight, *_bn_fold(None, fc[4], F, self.device), self.Fp, self.Fp, True)
        w3 = torch.cat([m.cls_out.weight, m.reg_out.weight], 0)
        b3 = torch.cat([m.cls_out.bias, m.reg_out.bias], 0)
        self.Op = depth_net_width(8)                     # (the width the convolution kernels take for any narrow output)
        self.c3 = layer(w3, *_bn_fold(b3, None, 8, self.device), self.Fp, self.Op, False)

    def run(self, bev_nhwc: torch.Tensor, boxes: torch.Tensor, count: torch.Tensor, B: int, K: int, H: int, W: int,
            bev_range) -> torch.Tensor:
        """bev_nhwc: the flat NHWC map [B][H][W][in_channels] in the storage dtype; boxes (B, K, 7), count int32 (B,) -> pred
        (B, K, 8) fp32, owned by the caller."""
        self.ensure_packed()
        Cc, R = self.module.in_channels, B * K
        if bev_nhwc.dtype != self.dtype or bev_nhwc.numel() < B * H * W * Cc:
            raise L.BevfError(f"RoIHead: expected a {self.dtype} NHWC map of {B} x {H} x {W} x {Cc} elements, got {bev_nhwc.dtype} x "
                              f"{bev_nhwc.numel()}")
        feat = self.buf("roi_feat", R * self.C5)
        with _span("roi_bev_points", nbytes=float(feat.element_size()) * R * self.C5 * 5):
            L.roi_bev_points(bev_nhwc, boxes, count, feat, None, H, W, Cc, Cc, bev_range)
        if self.C5p != self.C5:
            x0 = self.buf("roi_feat_pad", R * self.C5p)
            v = x0[:R * self.C5p].view(R, self.C5p)
            v[:, self.C5:].zero_()
            v[:, :self.C5].copy_(feat[:R * self.C5].view(R, self.C5))
        else:
            x0 = feat
        a1 = self.buf("roi_fc1", R * self.Fp)
        _run_conv(self.c1, x0, a1, 1, R, 1)
        a2 = self.buf("roi_fc2", R * self.Fp)
        _run_conv(self.c2, a1, a2, 1, R, 1)
        cols = self.buf("roi_pred", R * self.Op)
        _run_conv(self.c3, a2, cols, 1, R, 1)
        return cols[:R * self.Op].view(R, self.Op)[:, :8].float().contiguous().view(B, K, 8)


# ---- BEV backbone + FPN neck (bev_backbone.BEVBackbone) ------------------------------------------------------

@dataclass
class PackedDeconv:
    w: torch.Tensor          # the packed filter of csrc/deconv.hip (L.deconv_pack)
    scale: torch.Tensor
    shift: torch.Tensor
    cin: int
    cout: int
    s: int


def _pad_cin(cin: int, dtype) -> int:
    """Channel stride of an activation the bf16 implicit-GEMM kernel may read: its K step is 64 channels."""
    return cin if dtype == torch.float32 else -(-cin // 64) * 64


class BackboneEngine(_Engine):
    """Eval mode: every stage's conv3x3 + folded BN + ReLU as a PackedConv (so every conv mode is honoured), every level's
    kernel = stride transposed convolution + folded BN + ReLU as one csrc/deconv.hip launch that stores into the level's channel
    slice of the NHWC concat buffer (a stride-1 level is a 1x1 convolution with the transposed weight, stored the same way).
    fp32 or bf16 storage.  bf16 maps whose channel count is no multiple of 64 are held at a channel stride rounded up to one, the
    padding zero and the filters zero-padded alike: the bf16 convolution kernels step through 64 channels at a time."""

    def pack(self) -> None:
        m, dt = self.module, self.dtype
        self.stages: List[List[PackedConv]] = []
        self.ups = []
        for block, deblock in zip(m.backbone.blocks, m.neck.deblocks):
            mods = list(block)
            self.stages.append([self._pack_conv(mods[i], mods[i + 1], dt) for i in range(0, len(mods), 3)])
            dc, bn = deblock[0], deblock[1]
            w = dc.weight.detach()
            cin, cout, s = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
            scale, shift = _bn_fold(None, bn, cout, w.device)
            if s == 1:
                w1 = torch.zeros(cout, _pad_cin(cin, dt), dtype=w.dtype, device=w.device)
                w1[:, :cin] = w[:, :, 0, 0].t()
                self.ups.append(_finish_pack(w1.view(-1), scale, shift, w1.shape[1], cout, 1, 1, 0, True))
            else:
                self.ups.append(PackedDeconv(L.deconv_pack(w.float(), dt), scale, shift, cin, cout, s))

    @staticmethod
    def _pack_conv(conv, bn, dt) -> PackedConv:
        w = conv.weight.detach()
        cout, cin = int(w.shape[0]), int(w.shape[1])
        cp = _pad_cin(cin, dt)
        if cp == cin:
            return pack_conv(conv, bn, True)
        scale, shift = _bn_fold(conv.bias, bn, cout, w.device)
        wp = torch.zeros(cout, 3, 3, cp, dtype=w.dtype, device=w.device)
        wp[..., :cin] = w.permute(0, 2, 3, 1)
        return _finish_pack(wp.view(-1), scale, shift, cp, cout, 3, conv.stride[0], conv.padding[0], True)

    def _map(self, name: str, rows: int, Cc: int) -> Tuple[torch.Tensor, int]:
        """Activation buffer of `rows` pixels of Cc channels -> (buffer, channel stride); zero-filled when (re)made, so that the
        padding channels of a bf16 map read as zeros for ever (the layers write the first Cc channels only)."""
        cs = _pad_cin(Cc, self.dtype)
        key = (rows, cs)
        if getattr(self, "_map_keys", None) is None:
            self._map_keys = {}
        t = self.buf(name, rows * cs)
        if self._map_keys.get(name) != (key, t.data_ptr()):
            if cs != Cc:
                t.zero_()
            self._map_keys[name] = (key, t.data_ptr())
        return t, cs

    def run(self, x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
        """x: the flat NHWC map [B][H][W][in_channels] in the storage dtype -> the flat NHWC concat [B][H][W][out_channels]."""
        self.ensure_packed()
        m, dt = self.module, self.dtype
        Cin, Ct = m.in_channels, m.out_channels
        if x.dtype != dt or x.numel() < B * H * W * Cin:
            raise L.BevfError(f"BEVBackbone: expected a {dt} NHWC map of {B} x {H} x {W} x {Cin} elements, got {x.dtype} x {x.numel()}")
        es = x.element_size()
        cur, cs, h, w = x, Cin, H, W
        if _pad_cin(Cin, dt) != Cin:                       # bf16, in_channels % 64 == 32: the one layout copy of this engine
            cur, cs = self._map("bb_in", B * H * W, Cin)
            cur[:B * H * W * cs].view(-1, cs)[:, :Cin].copy_(x[:B * H * W * Cin].view(-1, Cin))
        out = self.buf("bb_concat", B * H * W * Ct)
        off = 0
        for i, (stage, up) in enumerate(zip(self.stages, self.ups)):
            for j, pc in enumerate(stage):
                ho, wo = (h + 2 - 3) // pc.stride + 1, (w + 2 - 3) // pc.stride + 1
                y, ycs = self._map(f"bb_{i}_{j % 2}" if j else f"bb_{i}_in", B * ho * wo, pc.cout)
                _run_conv(pc, cur, y, B, h, w, x_cs=cs, y_cs=ycs)
                cur, cs, h, w = y, ycs, ho, wo
            dst = out[off:]
            if isinstance(up, PackedConv):
                _run_conv(up, cur, dst, B, h, w, x_cs=cs, y_cs=Ct)
            else:
                M = B * h * w
                with _span("deconv_" + L._sfx(x), flops=2.0 * M * up.s * up.s * up.cout * up.cin,
                           nbytes=float(es) * M * (up.cin + up.s * up.s * up.cout)):
                    L.deconv_nhwc(cur, up.w, up.scale, up.shift, dst, N=B, H=h, W=w, Cin=up.cin, x_cs=cs, Cout=up.cout, y_cs=Ct,
                                  s=up.s, relu=True)
            off += up.cout
        return out


# ---- layout helpers at the API surface ----------------------------------------------------------------------

def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W) -> flat NHWC buffer."""
    N, Cc, H, W = x.shape
    dt = x.dtype
    y = torch.empty(N * H * W * Cc, device=x.device)
    L.nchw_to_nhwc(x.float().contiguous(), y, N, Cc, H * W, Cc)           # API-surface layout change runs in fp32
    return y if dt == torch.float32 else y.to(dt)


def to_nchw(buf: torch.Tensor, N: int, Cc: int, H: int, W: int) -> torch.Tensor:
    dt = buf.dtype
    y = torch.empty(N, Cc, H, W, device=buf.device)
    L.nhwc_to_nchw(buf.float(), y, N, Cc, H * W, Cc)
    return y if dt == torch.float32 else y.to(dt)


def require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and isinstance(t, torch.Tensor) and not t.is_cuda:
            raise L.BevfError("this package runs the hot path on MI355X only: move the module and its inputs to "
                              "'cuda' (there is no CPU fallback; the CPU oracle lives under oracle/ for tests)")
