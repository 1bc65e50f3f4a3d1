"""Training step on the HIP path (ref src/train_detect.py:401-434).

`model.train()` routes `FlexibleMultiModal3DDetector.forward` through `DetectorTape` under `_TapeFn`, the one
`torch.autograd.Function` of every tape path: the forward runs the same NHWC kernels as inference but with train-mode
BatchNorm (batch statistics, running-stat update) and keeps a tape; the backward walks the tape with hand-written gradient
kernels (MFMA weight / data gradients, BN, pooling, resample, dense layers, head) and returns the parameter gradients to
autograd, so the reference's training loop -- `loss.backward(); clip_grad_norm_(...); optimizer.step()` -- works unchanged.
`DetectorTape` composes one tape per module kind (CameraTape, PointMLPTape, RadarTape, PillarPFNLayer, FusionTape,
HeadTape), each built from the real module; the same tapes serve those modules used on their own.  torch is used for tensor
allocation and for weight layout permutes; no torch compute op touches an activation.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import engine as E


def _new(n: int, dev, dtype=torch.float32) -> torch.Tensor:
    """Uninitialised flat buffer of at least n elements, rounded up to a multiple of 4 (the elementwise kernels work in fours)."""
    return torch.empty(max((int(n) + 3) // 4 * 4, 4), dtype=dtype, device=dev)


class _ZeroPool:
    """One zero-filled buffer per backward pass from which the many small accumulation targets (conv weight
    gradients, bias sums) are carved: one fill launch instead of ~60."""

    def __init__(self, dev, floats: int = 16 << 20):
        self.buf = torch.zeros(floats, device=dev)
        self.off = 0

    def take(self, n: int):
        n4 = (n + 3) // 4 * 4                                 # keep every slice 16-byte aligned
        if n > (2 << 20) or self.off + n4 > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n4]
        self.off += n4
        return t


_ZPOOL: Optional[_ZeroPool] = None


def _zeros(n: int, dev, dtype=torch.float32) -> torch.Tensor:
    n = max((int(n) + 3) // 4 * 4, 4)                          # rounded up like _new
    if _ZPOOL is not None and dtype == torch.float32 and _ZPOOL.buf.device == torch.device(dev):
        t = _ZPOOL.take(n)
        if t is not None:
            return t
    return torch.zeros(n, dtype=dtype, device=dev)


_PIXTAB: Dict[tuple, torch.Tensor] = {}


def _pixtab(N, H, W, k, stride, pad, x_cs, dev) -> torch.Tensor:
    key = (N, H, W, k, stride, pad, x_cs, str(dev))
    t = _PIXTAB.get(key)
    if t is None:
        t = torch.empty(L.conv_pixtab_bytes(N, H, W, k, k, stride, pad) // 4, dtype=torch.int32, device=dev)
        L.conv_pixtab(t, N, H, W, k, k, stride, pad, x_cs)
        _PIXTAB[key] = t
    return t


def _wino_wgrad_table(N, H, W, x_cs, dy_cs, dev) -> torch.Tensor:
    """Per-shape tile table of the Winograd weight gradient (pixel byte offsets per 2x2 tile), cached like _pixtab."""
    key = ("wwtab", N, H, W, x_cs, dy_cs, str(dev))
    t = _PIXTAB.get(key)
    if t is None:
        t = torch.empty(L.wino_wgrad_table_bytes(N, H, W) // 4, dtype=torch.int32, device=dev)
        L.wino_wgrad_table(t, N, H, W, x_cs, dy_cs)
        _PIXTAB[key] = t
    return t


# ---- primitive ops (thin wrappers over the C-ABI; all tensors fp32 cuda, flat NHWC) ---------------------------------

# The conv kernels address their operands with 32-bit byte offsets: a tensor handed to one launch must stay below
# BUF_LIMIT bytes.  Batches past that run as image chunks (outputs are slices of one buffer, weight gradients
# accumulate); tests shrink BUF_LIMIT to exercise the chunking on small shapes.
BUF_LIMIT = (1 << 31) - 1


def _image_chunk(N: int, *per_image_elems: int) -> int:
    n_max = max(1, BUF_LIMIT // (4 * max(per_image_elems)))
    return N if N <= n_max else -(-N // -(-N // n_max))


def _wino_ok(cin, k, stride, pad) -> bool:
    """The fused fp32 Winograd kernel (csrc/conv_wino.hip) serves the 3x3 / stride 1 / pad 1 layers when the conv mode
    says so (engine.set_conv_mode("wino")): forward and data-gradient convolutions of the training step alike."""
    return E.conv_mode() in ("wino", "wino_x3") and (k, stride, pad) == (3, 1, 1) and cin % 32 == 0      # (the split kernels are inference-only)


def _conv_launch(x, w_ohwi, bias, y, n, H, W, cin, cout, k, stride, pad, relu, res=None, stats=None):
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if _wino_ok(cin, k, stride, pad):
        with E._span("conv_wino_f32", flops=2.0 * n * Ho * Wo * cout * k * k * cin):
            L.conv3x3_wino(x, L.wino_filter_transform(w_ohwi, cout, cin), None, bias, y, N=n, H=H, W=W, Cin=cin, x_cs=cin,
                           Cout=cout, y_cs=cout, relu=relu, res=res, res_cs=cout if res is not None else 0,
                           stats=stats[0] if stats else None, stats_pivot=stats[1] if stats else None)
        return
    with E._span("conv_igemm_f32", flops=2.0 * n * Ho * Wo * cout * k * k * cin):
        L.conv2d_nhwc(x, w_ohwi, None, bias, y, N=n, H=H, W=W, Cin=cin, x_cs=cin, Cout=cout, y_cs=cout, KH=k, KW=k,
                      stride=stride, pad=pad, relu=relu, res=res, res_cs=cout if res is not None else 0)


def conv_raw(x, w_ohwi, bias, N, H, W, cin, cout, k, stride, pad, relu=False, bn_pivot=None):
    """y = conv(x) (+bias) (+ReLU).  bn_pivot [cout] (training forward in front of a BatchNorm, Winograd layers only): the
    conv epilogue also leaves the BatchNorm partial sums; returns (y, Ho, Wo, partials or None) then, partials =
    (part [G][cout][2], G, pivot) for bn_train_forward."""
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    per = _image_chunk(N, H * W * cin, Ho * Wo * cout)
    y = _new(N * Ho * Wo * cout, x.device)
    fuse = bn_pivot is not None and not relu and _wino_ok(cin, k, stride, pad)
    part, rows = None, 0
    if fuse:
        rows_of = lambda n: L.wino_stat_rows(n, H, W)
        G = sum(rows_of(min(per, N - i0)) for i0 in range(0, N, per))
        part = _new(G * cout * 2, x.device)
    for i0 in range(0, N, per):
        n = min(per, N - i0)
        st = None
        if fuse:
            st = (part[rows * cout * 2:], bn_pivot)
            rows += rows_of(n)
        _conv_launch(x[i0 * H * W * cin:], w_ohwi, bias, y[i0 * Ho * Wo * cout:], n, H, W, cin, cout, k, stride, pad, relu, stats=st)
    if bn_pivot is not None:
        return y, Ho, Wo, ((part, rows, bn_pivot) if fuse else None)
    return y, Ho, Wo


# 3x3 / stride 1 / pad 1 weight gradients with channels in multiples of 64 run in the Winograd domain (csrc/conv_wino_wgrad.hip:
# 2.25x fewer MFMA FLOPs, deterministic); False = the pixel-GEMM with atomics everywhere (the round-1 path)
WINO_WGRAD = True


def conv_wgrad(x, dy, N, H, W, cin, cout, k, stride, pad, dw=None) -> torch.Tensor:
    """Returns dW in OHWI layout [cout][k][k][cin] (accumulates into `dw` when given)."""
    fresh = dw is None
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    per = _image_chunk(N, H * W * cin, Ho * Wo * cout, Ho * Wo * k * k)          # (the tap table has the same limit)
    if per < N:
        if fresh:
            dw = _zeros(cout * k * k * cin, x.device)
        for i0 in range(0, N, per):
            n = min(per, N - i0)
            conv_wgrad(x[i0 * H * W * cin:], dy[i0 * Ho * Wo * cout:], n, H, W, cin, cout, k, stride, pad, dw=dw)
        return dw[:cout * k * k * cin].view(cout, k, k, cin)
    flops = 2.0 * N * Ho * Wo * cout * k * k * cin
    ws = (L.wino_wgrad_workspace_floats(N, H, W, cin, cout)
          if WINO_WGRAD and E.conv_mode() in ("wino", "wino_x3") and (k, stride, pad) == (3, 1, 1) else 0)
    if ws:
        if fresh:
            dw = _new(cout * 9 * cin, x.device)
        table = _wino_wgrad_table(N, H, W, cin, cout, x.device)
        work = _new(ws, x.device)
        with E._span("conv_wgrad_wino_f32", flops=flops):
            L.conv3x3_wgrad_wino(x, dy, dw, table, work, N=N, H=H, W=W, Cin=cin, x_cs=cin, Cout=cout, dy_cs=cout, accumulate=not fresh)
        return dw[:cout * 9 * cin].view(cout, 3, 3, cin)
    if fresh:
        dw = _zeros(cout * k * k * cin, x.device)
    pixtab = _pixtab(N, H, W, k, stride, pad, cin, x.device)
    with E._span("conv_wgrad_f32", flops=flops):
        L.conv2d_wgrad(x, dy, dw, pixtab, N=N, H=H, W=W, Cin=cin, x_cs=cin, Cout=cout, dy_cs=cout, KH=k, KW=k, stride=stride, pad=pad)
    return dw[:cout * k * k * cin].view(cout, k, k, cin)


def _dgrad_conv(src, filt_oihw_sub, N, Hs, Ws, cin, cout, kh, kw):
    """One stride-1, pad-0 correlation of `src` [N][Hs][Ws][cout] with taps filt[t][u] -> [N][Hs-kh+1][Ws-kw+1][cin]."""
    wt = filt_oihw_sub.permute(1, 2, 3, 0).contiguous().view(-1)                         # [cin][kh][kw][cout]
    ho, wo = Hs - kh + 1, Ws - kw + 1
    out = _new(N * ho * wo * cin, src.device)
    L.conv2d_nhwc(src, wt, None, None, out, N=N, H=Hs, W=Ws, Cin=cout, x_cs=cout, Cout=cin, y_cs=cin, KH=kh, KW=kw,
                  stride=1, pad=0, relu=False)
    return out, ho, wo


def dgrad_can_fuse_bn(N, H, W, cin, cout, k, stride, pad) -> bool:
    """True when conv_dgrad runs as ONE fused-Winograd launch (so its epilogue can do the next BatchNorm's first backward pass)."""
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return (stride == 1 and _wino_ok(cout, k, 1, k - 1 - pad) and (Ho, Wo) == (H, W)
            and _image_chunk(N, H * W * max(cin, cout), (Ho + 1) * (Wo + 1) * cout) >= N)


def conv_dgrad(dy, weight_oihw, N, H, W, cin, cout, k, stride, pad, add=None, bnb=None):
    """dX [N*H*W*cin] = conv_transpose(dy, W).  Stride 1: the forward kernel on dy with the flipped filter.  Stride 2
    (3x3 pad 1, or 1x1 pad 0 -- the ResNet shapes): the four input-parity classes (ih&1, iw&1) each see a fixed subset
    of the taps, so each is a small stride-1 conv over dy (1x1 / 1x2 / 2x1 / 2x2 taps) and `interleave2x2` assembles dX:
    exactly the forward's MFMA work instead of 4x on a zero-stuffed grid.  Other strides: zero stuffing.
    `add` [N*H*W*cin]: a gradient to sum into dX (the skip connection's), fused into the conv epilogue when stride 1.
    `bnb` (only with dgrad_can_fuse_bn): dX is the gradient reaching a train-mode BatchNorm(+ReLU) layer described by bnb = dict(x,
    y|None, mean, invstd, gamma, beta); the epilogue applies that layer's ReLU mask and leaves its backward partial sums:
    returns (dX_masked, (part, G)) then."""
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    per = _image_chunk(N, H * W * max(cin, cout), (Ho + 1) * (Wo + 1) * cout)
    if per < N or (add is not None and stride != 1):
        dx = torch.cat([conv_dgrad(dy[i0 * Ho * Wo * cout:(i0 + min(per, N - i0)) * Ho * Wo * cout], weight_oihw,
                                   min(per, N - i0), H, W, cin, cout, k, stride, pad)[:min(per, N - i0) * H * W * cin]
                        for i0 in range(0, N, per)]) if per < N else conv_dgrad(dy, weight_oihw, N, H, W, cin, cout, k, stride, pad)
        if add is not None:
            add_(dx, add, min(dx.numel(), add.numel()))
        return dx
    flops = 2.0 * N * Ho * Wo * cout * k * k * cin                                       # algorithmic
    w = weight_oihw.detach()
    if stride == 2 and (k, pad) in ((3, 1), (1, 0)):
        dx = _new(N * H * W * cin, dy.device)
        with E._span("conv_dgrad_f32", flops=flops):
            if k == 1:
                c00, h0, w0 = _dgrad_conv(dy, w, N, Ho, Wo, cin, cout, 1, 1)
                cls, hq, wq = [c00, None, None, None], [h0, 0, 0, 0], [w0, 0, 0, 0]
            else:
                src = _new(N * (Ho + 1) * (Wo + 1) * cout, dy.device)                      # dy with a zero row / column appended
                L.zero_stuff_nhwc(dy, src, N, Ho, Wo, cout, Ho + 1, Wo + 1, 1)
                taps = ([1], [2, 0])                                                       # parity 0: kh=1 reads dy[a]; parity 1: kh=2 reads dy[a], kh=0 reads dy[a+1]
                cls, hq, wq = [], [], []
                for ph in (0, 1):
                    for pw in (0, 1):
                        sub = w[:, :, taps[ph]][:, :, :, taps[pw]]
                        c, hc, wc = _dgrad_conv(src, sub, N, Ho + 1, Wo + 1, cin, cout, len(taps[ph]), len(taps[pw]))
                        cls.append(c); hq.append(hc); wq.append(wc)
            L.interleave2x2_nhwc(cls, hq, wq, dx, N, H, W, cin)
        return dx
    wt = w.flip(2, 3).permute(1, 2, 3, 0).contiguous().view(-1)                          # [cin][k][k][cout]
    src, sh, sw = dy, Ho, Wo
    if stride != 1:
        src = _new(N * H * W * cout, dy.device)
        L.zero_stuff_nhwc(dy, src, N, Ho, Wo, cout, H, W, stride)
        sh, sw = H, W
    else:
        assert (Ho, Wo) == (H, W), "stride-1 convs on this path keep the spatial size"
    dx = _new(N * H * W * cin, dy.device)
    wino = stride == 1 and _wino_ok(cout, k, 1, k - 1 - pad)
    with E._span("conv_dgrad_wino_f32" if wino else "conv_dgrad_f32", flops=flops):     # (own span name: bench.py prices the 16/36)
        if wino:
            part = None
            if bnb is not None:
                G = L.wino_stat_rows(N, sh, sw)
                part = _new(G * cin * 2, dy.device)
            L.conv3x3_wino(src, L.wino_filter_transform(wt, cin, cout), None, None, dx, N=N, H=sh, W=sw, Cin=cout, x_cs=cout,
                           Cout=cin, y_cs=cin, relu=False, res=add, res_cs=cin if add is not None else 0, stats=part, bnb=bnb)
            if bnb is not None:
                return dx, (part, G)
        else:
            L.conv2d_nhwc(src, wt, None, None, dx, N=N, H=sh, W=sw, Cin=cout, x_cs=cout, Cout=cin, y_cs=cin, KH=k, KW=k,
                          stride=1, pad=k - 1 - pad, relu=False, res=add if stride == 1 else None,
                          res_cs=cin if (add is not None and stride == 1) else 0)
    if add is not None and stride != 1:
        add_(dx, add, min(dx.numel(), add.numel()))
    return dx


class _BNState:
    __slots__ = ("mean", "invstd", "xraw", "y", "M", "C", "has_res", "frozen")


# Test instrumentation (tests/test_gpu_training.py): when a list, every train-mode forward site that applies a ReLU appends its
# post-activation matrix (tensor [M*C], M, C) -- the decisions the hand-written backward will take -- so that the fp64 oracle can be
# made to take the SAME decisions and whole-network gradients compared to 1e-4 instead of "up to a few ReLU flips".  None = off.
RELU_TRACE: Optional[list] = None


def _trace_relu(y, M: int, Cc: int) -> None:
    if RELU_TRACE is not None and y is not None:
        RELU_TRACE.append((y, M, Cc))


FUSE_BN_STATS = False        # BatchNorm batch statistics from partial sums the Winograd conv epilogue leaves (no stats pass over the
                             # activation).  Built and tested, but off: time-neutral on MI355X (the epilogue is exposed time), and the
                             # sums are shifted by the RUNNING mean, so their accuracy depends on how far that is from the batch mean
                             # (two otherwise identical steps differed by 2e-4 in a gradient when only the running mean differed)


def bn_pivot_of(bn) -> Optional[torch.Tensor]:
    """Shift for the BatchNorm partial sums a conv epilogue produces (FUSE_BN_STATS): any value near the channel mean avoids
    cancellation in E[(x-p)^2] - E[x-p]^2; the running mean is at hand (None: the sums stay a separate, self-shifted pass)."""
    if not FUSE_BN_STATS:
        return None
    rm = getattr(bn, "running_mean", None)
    return rm.detach() if (rm is not None and rm.dtype == torch.float32 and rm.is_cuda) else None


def bn_is_frozen(bn) -> bool:
    """An eval-mode BatchNorm with running statistics inside a module that is being trained normalises with its buffers (torch's rule)."""
    return (not bn.training) and bn.track_running_stats and bn.running_mean is not None


def bn_train_forward(xraw, bn: nn.BatchNorm2d, M: int, Cc: int, res=None, relu=True, apply=True, partials=None):
    """Batch statistics (+ running-buffer update) and, unless apply=False, the normalised activation.
    partials = (part, G, pivot) from a conv epilogue: the statistics are merged from them, xraw is not re-read."""
    dev = xraw.device
    if bn_is_frozen(bn):
        # eval-mode BatchNorm inside a module that trains (mixed mode): the running buffers are the statistics, nothing is updated, and
        # the backward treats them as constants (bn_backward(frozen=True)).  Channel-sized torch arithmetic only.
        mean = bn.running_mean.detach().float().contiguous()
        invstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps).contiguous()
        y = None
        if apply:
            y = _new(M * Cc, dev)
            L.bn_apply(xraw, mean, invstd, bn.weight, bn.bias, res, y, M, Cc, Cc, relu)
            if relu:
                _trace_relu(y, M, Cc)
        s = _BNState()
        s.mean, s.invstd, s.xraw, s.y, s.M, s.C, s.has_res, s.frozen = mean, invstd, xraw, y, M, Cc, res is not None, True
        return y, s
    mean, var, invstd = _new(Cc, dev), _new(Cc, dev), _new(Cc, dev)
    if partials is not None:
        part, G, pivot = partials
        pivot = pivot.clone()                    # the running mean is updated below, in place
        L.bn_stats_from_partials(part, G, pivot, mean, var, invstd, M, Cc, bn.eps)
    else:
        work = _new(L.bn_work_floats(Cc), dev)
        L.bn_stats(xraw, work, mean, var, invstd, M, Cc, Cc, bn.eps)
    y = None
    if apply:
        y = _new(M * Cc, dev)
        L.bn_apply(xraw, mean, invstd, bn.weight, bn.bias, res, y, M, Cc, Cc, relu)
    if bn.track_running_stats and bn.running_mean is not None:           # torch: momentum 0.1, unbiased running var
        nbt = bn.num_batches_tracked
        if bn.momentum is None:
            # torch's cumulative moving average: factor 1 / (num_batches_tracked after this batch); the count lives on
            # the device, so this rare setting costs one host read per layer and step
            mom = 1.0 / (int(nbt.item()) + 1) if nbt is not None else 0.0
        else:
            mom = bn.momentum
        L.bn_update_running(mean, var, bn.running_mean, bn.running_var, nbt, Cc, M, mom)
        for t in (bn.running_mean, bn.running_var, nbt):                 # written through raw pointers: bump the versions
            if t is not None:                                             # (the engines' repack signature looks at them)
                torch.autograd.graph.increment_version(t)
    if relu:
        _trace_relu(y, M, Cc)
    s = _BNState()
    s.mean, s.invstd, s.xraw, s.y, s.M, s.C, s.has_res, s.frozen = mean, invstd, xraw, y, M, Cc, res is not None, False
    return y, s


def bn_train_backward(dy, s: _BNState, bn, relu=True, need_dx=True):
    """Returns (dxraw or None, dgamma, dbeta).  Layers with a skip connection: dy <- dy*(y>0) in place (it is the skip input's
    gradient); layers without one: dy is left untouched (the mask is recomputed from the raw input in both passes)."""
    dev = dy.device
    work = _new(L.bn_work_floats(s.C), dev)
    dgamma, dbeta = _new(s.C, dev), _new(s.C, dev)
    dx = _new(s.M * s.C, dev) if need_dx else None
    # without a residual the ReLU mask is recomputed from the raw input (same fma as the forward): y is not re-read
    L.bn_backward(dy, s.y, s.xraw, s.mean, s.invstd, bn.weight, bn.bias, work, dgamma, dbeta, dx, s.M, s.C, s.C, relu=relu,
                  has_res=s.has_res, frozen=s.frozen)
    return dx, dgamma[:s.C], dbeta[:s.C]


def group_max_with_index(a, G: int, P: int, Cc: int):
    """max over the P rows of each of G groups of a [G*P][Cc] activation, first maximum wins -> (gmax [G*Cc], idx int32 [G*Cc])."""
    dev = a.device
    g = _new(G * Cc, dev)
    idx = torch.empty(G * Cc, dtype=torch.int32, device=dev)
    work = torch.empty(L.group_max_idx_work_bytes(G, P, Cc), dtype=torch.uint8, device=dev)
    L.group_max_idx(a, g, idx, work, G, P, Cc)
    return g, idx


def group_max_scatter(dg, idx, G: int, P: int, Cc: int):
    """Backward of group_max_with_index: a zero [G*P][Cc] gradient with dg at the winning rows."""
    d = _zeros(G * P * Cc, dg.device)
    L.group_max_bwd(dg, idx, d, G, P, Cc)
    return d


def _bn_or_none(m):
    """The reference builds `nn.BatchNorm1d(w) if use_bn else nn.Identity()` (ref src/encoders.py:258-269, 520-529)."""
    return m if isinstance(m, nn.modules.batchnorm._BatchNorm) else None


class PointFirstLayer:
    """conv1 of a shared point MLP (Conv1d k=1 over <= 16 input channels) -> train-mode BatchNorm (or none: use_bn=False) -> ReLU."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, _bn_or_none(bn)

    def forward(self, rows, M: int, Cc: int):
        self.rows, self.M, self.Cc = rows, M, Cc
        w0 = self.conv.weight.detach().reshape(self.conv.weight.shape[0], Cc).contiguous()
        self.c0 = c0 = w0.shape[0]
        bias = self.conv.bias.detach() if self.conv.bias is not None else None
        out = _new(M * c0, rows.device)
        if self.bn is None:                                                # conv + bias + ReLU in one pass
            L.pointwise_smallk(rows, w0, None, bias, out, M, Cc, c0, True)
            _trace_relu(out, M, c0)
            self.y = out
            return out
        L.pointwise_smallk(rows, w0, None, bias, out, M, Cc, c0, False)
        a, self.bns = bn_train_forward(out, self.bn, M, c0, relu=True)
        return a

    def backward(self, d, sink) -> None:
        M, Cc, c0 = self.M, self.Cc, self.c0
        if self.bn is None:
            L.relu_mask(d, self.y, M * c0)
            draw = d
        else:
            draw, dgamma, dbeta = bn_train_backward(d, self.bns, self.bn, relu=True)
            sink.add(self.bn.weight, dgamma)
            sink.add(self.bn.bias, dbeta)
        if self.conv.bias is not None:
            sink.add(self.conv.bias, colsum(draw, M, c0))
        dw = _zeros(c0 * Cc, d.device)
        L.smallk_wgrad(draw, self.rows, dw, M, Cc, c0)
        sink.add(self.conv.weight, dw[:c0 * Cc])


LOWRANK_GMAX_BACKWARD = True  # PointNet's last layer (conv -> BatchNorm -> ReLU -> max over points): weight / data gradients through
                              # a K x K Gram matrix instead of the dense M x C gradient (half the GEMM FLOPs, no 1.15 GB tensor)
FUSE_POOL_BN_BACKWARD = True  # stem: BatchNorm + ReLU evaluated inside the max-pool (forward) and the max-pool backward gathered inside
                              # the BatchNorm backward passes: neither the normalised map nor its gradient (1.1 GB each) is ever written
FUSE_BN_BACKWARD = False     # the producing data-gradient conv does the next BatchNorm's first backward pass in its epilogue: correct
                             # (tests run both settings) but +0.4 ms per step on MI355X, because the Winograd epilogue is exposed time


def bn_backward_from_partials(dy, s: _BNState, bn, pre):
    """BatchNorm backward when the producer of dy already masked it and left the sums as partials: merge + apply."""
    part, G = pre
    dev = dy.device
    dgamma, dbeta = _new(s.C, dev), _new(s.C, dev)
    dx = _new(s.M * s.C, dev)
    L.bn_backward_from_partials(dy, s.xraw, s.mean, s.invstd, bn.weight, part, G, dgamma, dbeta, dx, s.M, s.C, s.C)
    return dx, dgamma[:s.C], dbeta[:s.C]


def colsum(dy, M, Cc):
    """sum over rows (bias gradients)."""
    work = _new(L.bn_work_floats(Cc), dy.device)
    out = _new(Cc, dy.device)
    L.bn_backward(dy, None, None, None, None, None, None, work, None, out, None, M, Cc, Cc)
    return out[:Cc]


def add_(y, x, n):
    L.add_inplace(y, x, n)


class GradSink:
    """Collects parameter gradients by parameter identity (summing repeated contributions)."""

    def __init__(self, reducer=None):
        self.g: Dict[int, torch.Tensor] = {}
        self.reducer = reducer               # replicas.GradReducer: averages gradients over the ranks while backward runs
        self._sent = set()

    def add(self, p: Optional[torch.Tensor], g: torch.Tensor):
        if p is None or not p.requires_grad:
            return
        g = g.reshape(p.shape)
        k = id(p)
        assert k not in self._sent, "gradient contribution after the parameter was handed to the all-reduce"
        self.g[k] = g if k not in self.g else self.g[k] + g

    def ready(self):
        """Every gradient collected so far is final: start its all-reduce now, under the rest of the backward."""
        if self.reducer is None:
            return
        keys = [k for k in self.g if k not in self._sent]
        if keys:
            self.reducer.submit(self, keys)
            self._sent.update(keys)

    def finish(self):
        if self.reducer is not None:
            self.ready()
            self.reducer.finish(self)

    def get(self, p):
        return self.g.get(id(p))


# ---- layer records --------------------------------------------------------------------------------------------------------

class ConvBNLayer:
    """conv (any bias) -> train-mode BN -> (+residual) -> (ReLU).  bn None: conv(+bias)(+ReLU) only (head)."""

    def __init__(self, conv, bn, relu=True):
        self.conv, self.bn, self.relu = conv, bn, relu
        w = conv.weight
        self.k = w.shape[2] if w.dim() == 4 else 1
        self.cin, self.cout = w.shape[1], w.shape[0]
        self.stride = conv.stride[0]
        self.pad = conv.padding[0]

    def forward(self, x, N, H, W, res=None):
        w4 = self.conv.weight.detach()
        if w4.dim() == 3:
            w4 = w4.unsqueeze(-1)
        w_ohwi = w4.permute(0, 2, 3, 1).contiguous().view(-1)
        bias = self.conv.bias.detach() if self.conv.bias is not None else None
        self.x, self.N, self.H, self.W = x, N, H, W
        if self.bn is None:
            y, Ho, Wo = conv_raw(x, w_ohwi, bias, N, H, W, self.cin, self.cout, self.k, self.stride, self.pad, relu=self.relu)
            self.y, self.M = y, N * Ho * Wo
            if self.relu:
                _trace_relu(y, self.M, self.cout)
            return y, Ho, Wo
        pivot, partials = (None if bn_is_frozen(self.bn) else bn_pivot_of(self.bn)), None
        if pivot is not None:
            xraw, Ho, Wo, partials = conv_raw(x, w_ohwi, bias, N, H, W, self.cin, self.cout, self.k, self.stride, self.pad, bn_pivot=pivot)
        else:
            xraw, Ho, Wo = conv_raw(x, w_ohwi, bias, N, H, W, self.cin, self.cout, self.k, self.stride, self.pad)
        self.M = N * Ho * Wo
        y, self.bns = bn_train_forward(xraw, self.bn, self.M, self.cout, res=res, relu=self.relu, partials=partials)
        self.has_res = res is not None
        return y, Ho, Wo

    def forward_groupmax(self, x, B: int, P: int):
        """conv (1x1 over B*P rows) -> train-mode BN -> ReLU -> max over the P rows of each group, without writing the
        activation: the max / argmax kernel evaluates relu(bn(.)) from the raw rows with bn_apply's own fma.  Returns
        (gmax [B*cout], idx int32 [B*cout]); pair with backward_from_groupmax."""
        assert self.bn is not None and self.relu and self.k == 1
        w4 = self.conv.weight.detach()
        if w4.dim() == 3:
            w4 = w4.unsqueeze(-1)
        w_ohwi = w4.permute(0, 2, 3, 1).contiguous().view(-1)
        bias = self.conv.bias.detach() if self.conv.bias is not None else None
        M = B * P
        self.x, self.N, self.H, self.W, self.M, self.has_res = x, M, 1, 1, M, False
        xraw, _, _ = conv_raw(x, w_ohwi, bias, M, 1, 1, self.cin, self.cout, 1, 1, 0)
        _, self.bns = bn_train_forward(xraw, self.bn, M, self.cout, relu=True, apply=False)
        dev = x.device
        if RELU_TRACE is not None:                               # (tests only: the activation this path never writes)
            yt = _new(M * self.cout, dev)
            L.bn_apply(xraw, self.bns.mean, self.bns.invstd, self.bn.weight, self.bn.bias, None, yt, M, self.cout, self.cout, True)
            _trace_relu(yt, M, self.cout)
        g = _new(B * self.cout, dev)
        idx = torch.empty(B * self.cout, dtype=torch.int32, device=dev)
        work = torch.empty(L.group_max_idx_work_bytes(B, P, self.cout), dtype=torch.uint8, device=dev)
        L.bn_relu_group_max_idx(xraw, self.bns.mean, self.bns.invstd, self.bn.weight, self.bn.bias, g, idx, work, B, P, self.cout)
        return g, idx

    def bnb_request(self):
        """What a producing data-gradient conv needs to do this layer's first BatchNorm-backward pass in its epilogue."""
        st = self.bns
        return dict(x=st.xraw, y=st.y if (self.relu and st.has_res) else None, mean=st.mean, invstd=st.invstd,
                    gamma=self.bn.weight.detach() if self.bn.weight is not None else None,
                    beta=self.bn.bias.detach() if self.bn.bias is not None else None)

    def can_take_fused_dy(self) -> bool:
        return self.bn is not None and self.relu and self.cout % 4 == 0 and not bn_is_frozen(self.bn)

    def backward(self, dy, sink: GradSink, need_dx=True, add=None, fuse_next=None, pre=None):
        """dy: gradient of the layer output (modified in place).  Returns (dx or None, d_res or None); `add` is summed
        into dx (skip-connection gradient, fused into the data-gradient conv's epilogue when it can be).
        pre = (part, G): dy arrives with this layer's ReLU mask applied and its BatchNorm-backward sums as partials (the
        producing conv's epilogue did that pass).  fuse_next: the ConvBNLayer that consumes dx -- when this layer's data
        gradient is one fused-Winograd launch, its epilogue does THAT layer's pass; the return is then (dx, d_res, pre_next)."""
        d_res = None
        if self.bn is None:
            if self.relu:
                L.relu_mask(dy, self.y, self.M * self.cout)
            dxraw = dy
        else:
            if pre is not None:
                dxraw, dgamma, dbeta = bn_backward_from_partials(dy, self.bns, self.bn, pre)
            else:
                dxraw, dgamma, dbeta = bn_train_backward(dy, self.bns, self.bn, relu=self.relu)
            sink.add(self.bn.weight, dgamma)
            sink.add(self.bn.bias, dbeta)
            if self.has_res:
                d_res = dy                                    # masked by the ReLU in place: gradient of the skip input
        if fuse_next is not None:
            dx, pre_next = self._conv_backward(dxraw, sink, need_dx, add, fuse_next)
            return dx, d_res, pre_next
        return self._conv_backward(dxraw, sink, need_dx, add), d_res

    def backward_from_groupmax(self, dg, gmax, idx, B: int, P: int, sink: GradSink):
        """Backward when this layer's output went straight into a max over the P rows of each of B groups (PointNet's
        last layer): dg / gmax / idx [B][cout].  The gradient is non-zero in one row per (group, channel), so BatchNorm's
        sums are gathered from those entries and no dense dY is ever built (L.gmax_bn_backward)."""
        assert self.bn is not None and self.relu and not self.has_res and B * P == self.M
        st, dev = self.bns, dg.device
        dgm, dgamma, dbeta = _new(B * self.cout, dev), _new(self.cout, dev), _new(self.cout, dev)
        if LOWRANK_GMAX_BACKWARD and self.k == 1 and self.cin % 4 == 0 and self.cout % 4 == 0:
            return self._backward_from_groupmax_lowrank(dg, gmax, idx, B, P, sink, dgm, dgamma, dbeta)
        dxraw = _new(self.M * self.cout, dev)
        L.gmax_bn_backward(dg, gmax, idx, st.xraw, st.mean, st.invstd, self.bn.weight, dgm, dgamma, dbeta, dxraw, B, P, self.cout,
                           self.cout)
        sink.add(self.bn.weight, dgamma[:self.cout])
        sink.add(self.bn.bias, dbeta[:self.cout])
        return self._conv_backward(dxraw, sink, True, None)

    def _backward_from_groupmax_lowrank(self, dg, gmax, idx, B, P, sink, dgm, dgamma, dbeta):
        """The same gradients without the dense dX [M][cout] (1.15 GB for PointNet's conv5) and with half the GEMM work.  With
        A [M][K] the layer input, W [C][K] its weight, x = A W^T + b its raw output, BatchNorm's backward is
            dX = S + 1 (beta')^T + (A W^T) diag(kappa),   kappa = -gamma invstd^2 dgamma / M,
                                                          beta' = -gamma invstd dbeta / M + kappa (b - mean),
        S = the B x C entries gamma invstd dg (one row per frame and channel, at the argmax).  Hence
            dW = S^T A + beta' colsum(A)^T + diag(kappa) W (A^T A)          -- one K x K Gram matrix instead of a C x K wgrad GEMM,
            dA = S W  + 1 (beta'^T W)      + A (W^T diag(kappa) W)          -- one M x K x K GEMM instead of M x C x K,
            db = colsum(S) + M beta' + kappa (W colsum(A)).
        (C = 1024, K = 512: 294 instead of 586 GFLOP, and no 1.15 GB tensor written and read twice.)"""
        st, dev, M, K, Cc = self.bns, dg.device, self.M, self.cin, self.cout
        L.gmax_bn_sums(dg, gmax, idx, st.xraw, st.mean, st.invstd, dgm, dgamma, dbeta, B, P, Cc, Cc)
        dgamma, dbeta = dgamma[:Cc], dbeta[:Cc]
        sink.add(self.bn.weight, dgamma)
        sink.add(self.bn.bias, dbeta)
        w = self.conv.weight
        W2 = w.detach().reshape(Cc, K)
        invstd, mean = st.invstd[:Cc], st.mean[:Cc]
        gi = invstd if self.bn.weight is None else self.bn.weight.detach() * invstd
        kap = -(gi * invstd) * dgamma / M
        bias = self.conv.bias.detach() if self.conv.bias is not None else torch.zeros(Cc, device=dev)
        beta_p = -(gi * dbeta) / M + kap * (bias - mean)
        S = (gi.unsqueeze(0) * dgm[:B * Cc].view(B, Cc)).contiguous()                      # [B][C] (parameter-sized torch arithmetic)
        cs_a = colsum(self.x, M, K)                                                       # 1^T A
        if self.conv.bias is not None:
            sink.add(self.conv.bias, S.sum(0) + M * beta_p + kap * (W2 * cs_a.unsqueeze(0)).sum(1))
        # weight gradient: K x K Gram matrix on the pixel-GEMM kernel, the rest is C x K sized
        gram = conv_wgrad(self.x, self.x, M, 1, 1, K, K, 1, 1, 0).reshape(K, K)
        wg, _, _ = conv_raw(W2.contiguous().view(-1), gram.contiguous().view(-1), None, Cc, 1, 1, K, K, 1, 1, 0)
        sa = _new(Cc * K, dev)                                                            # S^T A over the B*C argmax rows, frames in order
        L.sparse_rows_wgrad(S, idx, self.x, sa, B, P, Cc, K)
        dW = sa[:Cc * K].view(Cc, K) + beta_p.unsqueeze(1) * cs_a.unsqueeze(0) + kap.unsqueeze(1) * wg[:Cc * K].view(Cc, K)
        sink.add(w, dW.reshape(w.shape))
        # data gradient: A (W^T diag(kappa) W) + the row-constant term in ONE 1x1-conv launch, then the B*C sparse rows
        kw = (kap.unsqueeze(1) * W2).contiguous()
        gw = conv_wgrad(W2.contiguous().view(-1), kw.view(-1), Cc, 1, 1, K, K, 1, 1, 0).reshape(K, K)
        v = (beta_p.unsqueeze(1) * W2).sum(0).contiguous()
        dA, _, _ = conv_raw(self.x, gw.contiguous().view(-1), v, M, 1, 1, K, K, 1, 1, 0)
        # + S W at the argmax rows: channels sharing a row are added by the row's first channel, in order (no atomics: reproducible)
        L.sparse_rows_scatter_add(S, idx, W2.contiguous(), dA, B, P, Cc, K)
        return dA

    def _conv_backward(self, dxraw, sink: GradSink, need_dx=True, add=None, fuse_next=None):
        if self.conv.bias is not None:
            sink.add(self.conv.bias, colsum(dxraw, self.M, self.cout))
        dw = conv_wgrad(self.x, dxraw, self.N, self.H, self.W, self.cin, self.cout, self.k, self.stride, self.pad)
        w = self.conv.weight
        sink.add(w, dw.permute(0, 3, 1, 2).reshape(w.shape))
        dx, pre_next = None, None
        if need_dx:
            w4 = w if w.dim() == 4 else w.unsqueeze(-1)
            geom = (self.N, self.H, self.W, self.cin, self.cout, self.k, self.stride, self.pad)
            if (fuse_next is not None and FUSE_BN_BACKWARD and fuse_next.can_take_fused_dy() and fuse_next.cout == self.cin
                    and fuse_next.M == self.N * self.H * self.W and dgrad_can_fuse_bn(*geom)):
                dx, pre_next = conv_dgrad(dxraw, w4, *geom, add=add, bnb=fuse_next.bnb_request())
            else:
                dx = conv_dgrad(dxraw, w4, *geom, add=add)
        if fuse_next is not None:
            return dx, pre_next
        return dx


class LinearLayer:
    def __init__(self, lin: nn.Linear, relu: bool, perm: Tuple[int, int] = (0, 0)):
        self.lin, self.relu, self.perm = lin, relu, perm

    def forward(self, x, B):
        w = self.lin.weight.detach().contiguous()
        O, K = w.shape
        y = _new(B * O, x.device)
        L.linear(x, w, self.lin.bias.detach() if self.lin.bias is not None else None, y, B, K, O, self.relu, *self.perm)
        self.x, self.y, self.B = x, y, B
        if self.relu and self.perm == (0, 0):
            _trace_relu(y, B, O)
        return y

    def backward(self, dy, sink: GradSink, need_dx=True):
        w = self.lin.weight.detach().contiguous()
        O, K = w.shape
        dev = dy.device
        if self.relu:
            L.relu_mask(dy, self.y, self.B * O)
        dx = _new(self.B * K, dev) if need_dx else None
        dw, db = _new(O * K, dev), _new(O, dev)
        work = _new(L.linear_bwd_work_floats(self.B, K, O), dev)
        L.linear_bwd(dy, self.x, w, dx, dw, db, work, self.B, K, O, *self.perm)
        sink.add(self.lin.weight, dw[:O * K])
        sink.add(self.lin.bias, db[:O])
        return dx


class Bilinear:
    def forward(self, x, B, Hi, Wi, Cc, Ho, Wo, y=None, y_cs=None):
        self.geom = (B, Hi, Wi, Cc, Ho, Wo, y_cs or Cc)
        if y is None:
            y = _new(B * Ho * Wo * Cc, x.device)
        L.bilinear_nhwc(x, y, B, Hi, Wi, Cc, Cc, Ho, Wo, y_cs or Cc)
        return y

    def backward(self, dy):
        B, Hi, Wi, Cc, Ho, Wo, y_cs = self.geom
        dx = _zeros(B * Hi * Wi * Cc, dy.device)
        L.bilinear_bwd_nhwc(dy, dx, B, Hi, Wi, Cc, Cc, Ho, Wo, y_cs)
        return dx


class StemBlock:
    """The camera stem of the training tape: 7x7 / stride-2 conv 3 -> 64 -> train-mode BatchNorm -> ReLU -> 3x3 / stride-2 max-pool
    with uint8 window indices.  FUSE_POOL_BN_BACKWARD: BatchNorm + ReLU evaluated inside the max-pool, and the pool backward gathered
    inside the BatchNorm backward."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn

    def forward(self, x, N: int, H: int, W: int):
        """x: NCHW fp32 images [N][3][H][W] -> (pooled NHWC [N*H2*W2*64], H2, W2)."""
        dev = x.device
        self.cam_geom_in = (N, H, W)
        self.imgs = x
        H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        w = self.conv.weight.detach()
        packed = torch.zeros(148, 64, device=dev)
        packed[:147] = w.reshape(64, 147).t()
        one, zero = torch.ones(64, device=dev), torch.zeros(64, device=dev)
        raw = _new(N * H1 * W1 * 64, dev)
        L.stem_conv7x7(x, packed.view(-1), one, zero, raw, N, H, W, relu=False)
        H2, W2 = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
        pooled = _new(N * H2 * W2 * 64, dev)
        self.pool_idx = torch.empty(N * H2 * W2 * 64, dtype=torch.uint8, device=dev)
        self.stem_fused = FUSE_POOL_BN_BACKWARD and not bn_is_frozen(self.bn)
        if self.stem_fused:
            # statistics only; BatchNorm + ReLU are evaluated inside the max-pool: the normalised stem map (1.1 GB) is never written --
            # nothing downstream reads it (the backward recomputes the ReLU mask from the raw conv output)
            _, self.stem_bn = bn_train_forward(raw, self.bn, N * H1 * W1, 64, relu=True, apply=False)
            s = self.stem_bn
            L.bn_relu_maxpool3x3s2_idx(raw, s.mean, s.invstd, self.bn.weight, self.bn.bias, pooled, self.pool_idx, N, H1, W1, 64)
        else:
            y, self.stem_bn = bn_train_forward(raw, self.bn, N * H1 * W1, 64, relu=True)
            L.maxpool3x3s2_idx(y, pooled, self.pool_idx, N, H1, W1, 64)
        self.pool_geom = (N, H1, W1)
        return pooled, H2, W2

    def backward(self, d, sink: GradSink) -> None:
        """d: gradient of the pooled map (NHWC); adds the conv weight and BatchNorm gradients to `sink`."""
        N, H1, W1 = self.pool_geom
        if self.stem_fused:
            # max-pool backward + BatchNorm/ReLU backward in one pair of passes: the dense dY of the stem map (1.1 GB at 48 images of
            # 448x800) is gathered from the pooled gradient on the fly, never written (bit-identical to the two-kernel chain below)
            s = self.stem_bn
            work = _new(L.bn_work_floats(64), d.device)
            dgamma, dbeta, draw = _new(64, d.device), _new(64, d.device), _new(N * H1 * W1 * 64, d.device)
            L.pool_bn_backward(d, self.pool_idx, s.xraw, s.mean, s.invstd, self.bn.weight, self.bn.bias, work, dgamma, dbeta, draw,
                               N, H1, W1, 64)
        else:
            dpool_in = _new(N * H1 * W1 * 64, d.device)
            L.maxpool3x3s2_bwd(d, self.pool_idx, dpool_in, N, H1, W1, 64)
            draw, dgamma, dbeta = bn_train_backward(dpool_in, self.stem_bn, self.bn, relu=True)
        sink.add(self.bn.weight, dgamma)
        sink.add(self.bn.bias, dbeta)
        # stem weight gradient: direct MFMA kernel on the image patches (no im2col matrix), dW as [64][160]
        Ni, H, W = self.cam_geom_in
        dwbuf = _zeros(64 * 160, d.device)
        with E._span("conv_wgrad_f32", flops=2.0 * N * H1 * W1 * 64 * 147):
            L.stem_wgrad(self.imgs, draw, dwbuf, Ni, H, W)
        sink.add(self.conv.weight, dwbuf[:64 * 160].view(64, 160)[:, :147].reshape(64, 3, 7, 7))


class PillarPFNLayer:
    """PillarLiDAREncoder under train-mode BatchNorm: voxelize -> the PFN's batch statistics from the decorated points' moments
    (L.pillar_moments: sum f, sum f f^T over the P rows of every occupied pillar, the empty pillar slots left out; running
    buffers updated there) -> L.pillar_pfn with those scale / shift, keeping the argmax row of every (pillar, channel) ->
    fp32 NHWC canvas.  Frozen BatchNorm (bn_is_frozen): the running statistics.  Backward: L.pillar_backward -- the
    canvas gradient at the argmax rows gives the weight, bias and BatchNorm gradients in closed form (no per-row pass)."""

    def __init__(self, enc):
        self.enc = enc

    def forward(self, pts):
        enc = self.enc
        lin, bn = enc.pfn.linear, enc.pfn.bn
        dev = pts.device
        self.g, self.B, self.vox = E.pillar_voxelize(enc, pts, lambda name, n, dt: _new(n, dev, dt))    # vox: kept for g's pointers
        self.cout, self.k = lin.weight.shape
        Cout = self.cout
        self.w = lin.weight.detach().float().contiguous()
        self.bias = lin.bias.detach().float().contiguous() if lin.bias is not None else None
        self.gamma = bn.weight.detach().float().contiguous() if bn.weight is not None else None
        self.frozen = bn_is_frozen(bn)
        self.moments = None
        if self.frozen:                                         # channel-sized torch arithmetic, as bn_train_forward's frozen path
            self.mean = bn.running_mean.detach().float().contiguous()
            self.invstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps).contiguous()
            g = self.gamma if self.gamma is not None else torch.ones(Cout, device=dev)
            b = self.bias if self.bias is not None else torch.zeros(Cout, device=dev)
            be = bn.bias.detach().float() if bn.bias is not None else torch.zeros(Cout, device=dev)
            self.scale = (g * self.invstd).contiguous()
            self.shift = (be + (b - self.mean) * self.scale).contiguous()
        else:
            self.moments = torch.empty(272, dtype=torch.float64, device=dev)
            self.mean, self.invstd, self.scale, self.shift = (_new(Cout, dev) for _ in range(4))
            work = torch.empty(L.pillar_work_bytes(Cout), dtype=torch.uint8, device=dev)
            track = bn.track_running_stats and bn.running_mean is not None
            L.pillar_moments(self.g, self.w, self.bias, self.gamma, bn.bias.detach() if bn.bias is not None else None, Cout,
                             bn.eps, -1.0 if bn.momentum is None else bn.momentum, bn.running_mean if track else None,
                             bn.running_var if track else None, bn.num_batches_tracked if track else None, self.moments,
                             self.mean, self.invstd, self.scale, self.shift, work)
            if track:
                for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):   # written through raw pointers
                    if t is not None:
                        torch.autograd.graph.increment_version(t)
        H, W = enc.bev_h, enc.bev_w
        self.canvas = _new(self.B * H * W * Cout, dev)
        self.argmax = torch.empty(max(self.g.B * self.g.Nv * Cout, 4), dtype=torch.uint8, device=dev)
        L.pillar_pfn(self.g, self.w, self.scale, self.shift, Cout, self.canvas, self.argmax)
        return self.canvas

    def backward(self, dcanvas, sink: GradSink) -> None:
        lin, bn = self.enc.pfn.linear, self.enc.pfn.bn
        dev, Cout, K = dcanvas.device, self.cout, self.k
        dw, db, dgamma, dbeta = _new(Cout * K, dev), _new(Cout, dev), _new(Cout, dev), _new(Cout, dev)
        work = torch.empty(L.pillar_work_bytes(Cout), dtype=torch.uint8, device=dev)
        L.pillar_backward(self.g, dcanvas.contiguous(), self.argmax, self.w, self.bias, self.scale, self.shift, self.mean, self.invstd,
                          self.gamma, self.moments, Cout, self.frozen, dw, db, dgamma, dbeta, work)
        sink.add(lin.weight, dw[:Cout * K])
        sink.add(lin.bias, db[:Cout])
        sink.add(bn.weight, dgamma[:Cout])
        sink.add(bn.bias, dbeta[:Cout])


class SparseConvLayer:
    """One sparse layer (encoders.SparseConvBlock) under train-mode BatchNorm: the gather-GEMM's raw sums over the active rows ->
    L.sparse_bn_stats (fp64 fixed-order partials over the active rows of the whole batch, running buffers moved there; frozen
    BatchNorm: the buffers are the statistics) -> relu(batchnorm).  Backward: L.sparse_bn_backward (bn_rows.h's mask and dx), the
    weight gradient through the forward table, and -- unless the layer is the first -- the data gradient: the same gather-GEMM on
    dy through the input-side table (a submanifold layer: its forward table with mirrored taps)."""

    def __init__(self, name: str, blk, st: "E.SparseStructure", first: bool):
        self.name, self.blk, self.st, self.first = name, blk, st, first
        self.lr, self.li, self.stride = E.SPARSE_SPEC[name]

    def forward(self, x, cin: int, nrows_slot):
        st, conv, bn = self.st, self.blk.conv, self.blk.bn
        B, cap, dev = st.B, st.caps[self.lr], x.device
        self.x, self.cin, self.cin_real = x, cin, conv.weight.shape[1]
        self.cout = cout = conv.weight.shape[0]
        self.rows_in = B * st.caps[self.li]
        self.y = _new(B * cap * cout, dev)
        with E._span(f"sparse_conv_f32:{self.name}"):
            L.sparse_conv(x, st.table[self.name], st.count[self.lr], E.sparse_pack_weight(conv), None, None, B, cap, self.rows_in, cin,
                          cout, False, self.y)
        self.gamma = bn.weight.detach().float().contiguous() if bn.weight is not None else None
        self.beta = bn.bias.detach().float().contiguous() if bn.bias is not None else None
        self.frozen = bn_is_frozen(bn)
        if self.frozen:
            self.mean = bn.running_mean.detach().float().contiguous()
            self.invstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps).contiguous()
        else:
            self.mean, self.invstd = _new(cout, dev), _new(cout, dev)
            work = torch.empty(L.sparse_bn_work_bytes(cout), dtype=torch.uint8, device=dev)
            track = bn.track_running_stats and bn.running_mean is not None
            with E._span("sparse_bn_stats"):
                L.sparse_bn_stats(self.y, st.count[self.lr], B, cap, cout, bn.eps, -1.0 if bn.momentum is None else bn.momentum,
                                  bn.running_mean if track else None, bn.running_var if track else None,
                                  bn.num_batches_tracked if track else None, self.mean, self.invstd, nrows_slot, work)
            if track:
                for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):   # written through raw pointers
                    if t is not None:
                        torch.autograd.graph.increment_version(t)
        a = _new(B * cap * cout, dev)
        with E._span("sparse_bn_apply"):
            L.sparse_bn_apply(self.y, st.count[self.lr], B, cap, cout, self.mean, self.invstd, self.gamma, self.beta, a)
        return a

    def backward(self, da, sink: GradSink):
        st, conv, bn = self.st, self.blk.conv, self.blk.bn
        B, cap, cout, dev = st.B, st.caps[self.lr], self.cout, da.device
        dy, dgamma, dbeta, sums = _new(B * cap * cout, dev), _new(cout, dev), _new(cout, dev), _new(2 * cout, dev)
        work = torch.empty(L.sparse_bn_work_bytes(cout), dtype=torch.uint8, device=dev)
        with E._span("sparse_bn_backward"):
            L.sparse_bn_backward(self.y, da, st.count[self.lr], B, cap, cout, self.mean, self.invstd, self.gamma, self.beta, self.frozen,
                                 dy, dgamma, dbeta, sums, work)
        sink.add(bn.weight, dgamma[:cout])
        sink.add(bn.bias, dbeta[:cout])
        dw = _new(cout * self.cin_real * 27, dev)
        wwork = _new(L.sparse_wgrad_work_floats(self.cin, cout), dev)
        with E._span(f"sparse_conv_wgrad_f32:{self.name}"):
            L.sparse_conv_wgrad(self.x, dy, st.table[self.name], st.count[self.lr], B, cap, self.rows_in, self.cin, cout, self.cin_real, dw,
                                wwork)
        sink.add(conv.weight, dw[:cout * self.cin_real * 27])
        if self.first:
            return None
        cap_in = st.caps[self.li]
        dx = _new(B * cap_in * self.cin, dev)
        table = st.table[self.name] if self.stride == 1 else st.grad_table[self.name]
        with E._span(f"sparse_conv_f32:{self.name}:dgrad"):
            L.sparse_conv(dy, table, st.count[self.li], E.sparse_pack_weight(conv, transposed=True), None, None, B, cap_in, B * cap, cout,
                          self.cin, False, dx)
        return dx


class SparseEncoderTape:
    """SparseLiDAREncoder under train-mode BatchNorm: structure (with the strided layers' input-side tables) -> mean VFE -> five
    SparseConvLayer -> fp32 NHWC canvas.  Backward: the canvas gradient gathered into the level-2 rows, then the layers in reverse.
    The one host read of a step is here: the five layers' active row counts, after the forward has been queued, because a
    train-mode BatchNorm over fewer than two rows is refused (as torch refuses it)."""

    def __init__(self, enc):
        self.enc = enc

    def forward(self, pts):
        enc, dev = self.enc, pts.device
        if next(enc.parameters()).dtype != torch.float32:
            raise L.BevfError("training: SparseLiDAREncoder trains in fp32 storage only")
        st = self.st = E.SparseStructure(enc, pts, lambda name, n, dt: _new(n, dev, dt), grad=True)
        self.B = st.B
        nrows = torch.full((8,), 2, dtype=torch.int32, device=dev)
        self.layers = []
        x, cin = st.x0, E.SPARSE_KPAD
        for i, (name, blk) in enumerate(zip(E.SPARSE_SPEC, enc.layers())):
            layer = SparseConvLayer(name, blk, st, first=i == 0)
            x = layer.forward(x, cin, nrows[i:i + 1])
            cin = layer.cout
            self.layers.append(layer)
        D2, H2, W2 = st.dims[2]
        self.c2 = cin
        self.canvas = _new(st.B * H2 * W2 * D2 * cin, dev)
        L.sparse_canvas(x, st.cell[2], st.count[2], st.B, st.caps[2], D2, H2, W2, cin, self.canvas)
        few = [n for n, v in zip(E.SPARSE_SPEC, nrows[:5].tolist()) if v < 2]
        if few:
            raise L.BevfError(f"training: SparseLiDAREncoder: BatchNorm of {few} saw fewer than two active voxels in the whole batch "
                              "(train-mode statistics need more than one row, as torch's BatchNorm1d); put the layer in eval mode")
        return self.canvas

    def backward(self, dcanvas, sink: GradSink) -> None:
        st = self.st
        D2, H2, W2 = st.dims[2]
        d = _new(st.B * st.caps[2] * self.c2, dcanvas.device)
        L.sparse_canvas_bwd(dcanvas.contiguous(), st.cell[2], st.count[2], st.B, st.caps[2], D2, H2, W2, self.c2, d)
        for layer in reversed(self.layers):
            d = layer.backward(d, sink)


# ---- module tapes ---------------------------------------------------------------------------------------------------------------
# One tape per module kind, built from the real nn.Module.  forward() runs the module under train-mode BatchNorm, keeps what the
# backward needs and exposes the geometry its callers need (B: batch size, cout: output channels, H / W: spatial size);
# backward(d, sink) adds the parameter gradients to `sink` and returns the input gradient (None where there is none).
# PillarPFNLayer above is the PointPillars tape.

class CameraTape:
    """ResNetCameraEncoder (ref src/encoders.py:133-172): stem, ResNet blocks, channel_proj -> NHWC features [B*n*H*W*cout]
    (n cameras per frame)."""

    def __init__(self, enc):
        self.enc = enc

    def forward(self, imgs):
        enc = self.enc
        if imgs.dim() == 5:
            self.B, self.n = imgs.shape[:2]
            x = imgs.reshape(self.B * self.n, *imgs.shape[2:]).contiguous().float()
        else:
            self.B, self.n = imgs.shape[0], 1
            x = imgs.contiguous().float()
        N, _, H, W = x.shape
        self.stem = StemBlock(enc.conv1, enc.bn1)
        cur, h, wd = self.stem.forward(x, N, H, W)
        self.blocks = []
        for layer in (enc.layer1, enc.layer2, enc.layer3):
            for blk in layer:
                c1, c2 = ConvBNLayer(blk.conv1, blk.bn1, True), ConvBNLayer(blk.conv2, blk.bn2, True)
                down = ConvBNLayer(blk.downsample[0], blk.downsample[1], False) if blk.downsample is not None else None
                t, ho, wo = c1.forward(cur, N, h, wd)
                idt = cur
                if down is not None:
                    idt, _, _ = down.forward(cur, N, h, wd)
                cur, _, _ = c2.forward(t, N, ho, wo, res=idt)
                self.blocks.append((c1, c2, down))
                h, wd = ho, wo
        self.proj = ConvBNLayer(enc.channel_proj[0], enc.channel_proj[1], True)
        feat, _, _ = self.proj.forward(cur, N, h, wd)
        self.cout, self.H, self.W = self.proj.cout, h, wd
        return feat

    def backward(self, dfeat, sink: GradSink) -> None:
        d, _ = self.proj.backward(dfeat, sink)
        rev = list(reversed(self.blocks))
        pre = None                                             # BatchNorm-backward partials that arrive WITH d (or None)
        for i, (c1, c2, down) in enumerate(rev):
            # c2's data-gradient conv does the first BatchNorm-backward pass of c1 (mask + sums) in its epilogue
            dt, d_res, pre1 = c2.backward(d, sink, fuse_next=c1, pre=pre)      # d_res: gradient reaching the skip connection
            pre = None
            if down is not None:
                dx, _ = c1.backward(dt, sink, pre=pre1)
                dd, _ = down.backward(d_res, sink)
                add_(dx, dd, dx.numel())
            elif i + 1 < len(rev):                             # identity skip: summed in the dgrad conv's epilogue, which then
                dx, _, pre = c1.backward(dt, sink, add=d_res, fuse_next=rev[i + 1][1], pre=pre1)   # serves the previous block's c2
            else:
                dx, _ = c1.backward(dt, sink, add=d_res, pre=pre1)
            d = dx
            if i % 2 == 1:
                sink.ready()                                   # one ResNet stage done: its gradients can travel
        self.stem.backward(d, sink)


class PointMLPTape:
    """A shared point MLP (encoders._PointMLP: conv1..conv{depth}, each with BatchNorm1d or Identity, ReLU) and the max over each
    frame's points -> (B, cout) as a flat buffer.  fuse_max (PointNet): while the last BatchNorm is in train mode, its BatchNorm +
    ReLU + max run as one pass (ConvBNLayer.forward_groupmax); otherwise (radar, use_bn=False, frozen statistics) the activation is
    written, then group_max_with_index."""

    def __init__(self, enc, depth: int, fuse_max: bool):
        self.enc, self.depth, self.fuse_max = enc, depth, fuse_max

    def forward(self, pts):
        enc = self.enc
        rows = enc._rows(pts)
        self.B, self.Np, Cc = rows.shape
        M = self.B * self.Np
        self.first = PointFirstLayer(enc.conv1, enc.bn1)               # bn*: BatchNorm1d, or Identity under use_bn=False
        a = self.first.forward(rows, M, Cc)
        self.layers = [ConvBNLayer(getattr(enc, f"conv{i}"), _bn_or_none(getattr(enc, f"bn{i}")), True)
                       for i in range(2, self.depth + 1)]
        *mid, last = self.layers
        for lyr in mid:
            a, _, _ = lyr.forward(a, M, 1, 1)
        self.cout = last.cout
        self.fused = self.fuse_max and last.bn is not None and not bn_is_frozen(last.bn)
        if self.fused:
            self.g, self.idx = last.forward_groupmax(a, self.B, self.Np)
        else:
            a, _, _ = last.forward(a, M, 1, 1)
            self.g, self.idx = group_max_with_index(a, self.B, self.Np, self.cout)
        return self.g

    def backward(self, dg, sink: GradSink) -> None:
        last = self.layers[-1]
        if self.fused:
            d = last.backward_from_groupmax(dg.contiguous(), self.g, self.idx, self.B, self.Np, sink)
        else:
            d, _ = last.backward(group_max_scatter(dg.contiguous(), self.idx, self.B, self.Np, self.cout), sink)
        for lyr in reversed(self.layers[:-1]):
            d, _ = lyr.backward(d, sink)
        self.first.backward(d, sink)


class RadarTape:
    """MultiRadarEncoder (ref src/encoders.py:628-661): the shared RadarEncoder over every sweep (conv1..conv4, then the max over
    the sweep's points), then concat -> fusion_fc, max or mean over the sweeps -> (B, cout) as a flat buffer.  One RadarEncoder
    alone is fusion_method "max" over its single sweep, the identity."""

    def __init__(self, enc, fusion_method: str, fusion_fc=None):
        self.enc, self.method, self.fc = enc, fusion_method, fusion_fc

    def forward(self, radars):
        if self.method not in ("concat", "max", "mean"):
            raise ValueError(f"Unknown fusion method: {self.method}")
        self.sweeps, feats = [], []
        for pts in radars:
            sweep = PointMLPTape(self.enc, 4, fuse_max=False)
            g = sweep.forward(pts)
            feats.append(g[:sweep.B * sweep.cout].view(sweep.B, sweep.cout))
            self.sweeps.append(sweep)
        per = torch.stack(feats, dim=1).contiguous()                      # (B, R, feat) -- layout copy only
        self.B, self.R, self.feat = B, R, feat = per.shape
        if self.method == "concat":
            if R * feat != self.fc.weight.shape[1]:
                raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({B}x{R * feat} and "
                                   f"{self.fc.weight.shape[1]}x{self.fc.weight.shape[0]})")
            self.fc_layer = LinearLayer(self.fc, False)
            self.cout = self.fc.weight.shape[0]
            return self.fc_layer.forward(per.view(-1), B)
        self.cout = feat
        out = _new(B * feat, per.device)
        if self.method == "max":                                          # ref src/encoders.py:654-655
            self.fuse_idx = torch.empty(B * feat, dtype=torch.int32, device=per.device)
            gwork = torch.empty(L.group_max_idx_work_bytes(B, R, feat), dtype=torch.uint8, device=per.device)
            L.group_max_idx(per, out, self.fuse_idx, gwork, B, R, feat)
        else:                                                             # mean, ref src/encoders.py:656-657
            L.cam_mean(per.view(-1), out, B, R, 1, feat)
        return out

    def backward(self, dfeat, sink: GradSink) -> None:
        B, R, feat = self.B, self.R, self.feat
        if self.method == "max":                   # the gradient goes to the sweep that held the maximum (first one on ties)
            dper = _zeros(B * R * feat, dfeat.device)
            L.group_max_bwd(dfeat, self.fuse_idx, dper, B, R, feat)
        elif self.method == "mean":                # every sweep receives dfeat / R
            dper = _new(B * R * feat, dfeat.device)
            L.cam_mean_bwd(dfeat, dper, B, R, 1, feat)
        else:
            dper = self.fc_layer.backward(dfeat, sink)                      # [B][R][feat]
        for r in reversed(range(R)):
            self.sweeps[r].backward(dper[:B * R * feat].view(B, R, feat)[:, r].contiguous().view(-1), sink)


class ConvPair:
    """seq's two conv+BN+ReLU (seq[0:2] and seq[3:5]) back to back, as one layer record."""

    def forward(self, seq, x, B, H, W):
        self.c1, self.c2 = ConvBNLayer(seq[0], seq[1], True), ConvBNLayer(seq[3], seq[4], True)
        return self.c2.forward(self.c1.forward(x, B, H, W)[0], B, H, W)[0]

    def backward(self, d, sink):
        return self.c1.backward(self.c2.backward(d, sink)[0], sink)[0]


class _FusionBranchTape:
    """One input branch of FusionTape, owning its layer records: forward(x, B, concat, ccs, slot, cam_geom, camera_calib) fills the
    branch's bev_channels-wide slot of the concatenated NHWC map (row stride ccs), backward(dconcat, sink) returns the gradient of x."""

    depth_sup = None      # (points, counts) of the step's depth supervision: FusionTape sets it on a learned-depth camera branch
    depth = None          # the branch's DepthLossTape once its forward has run with depth_sup
    depth_grad = None     # the gradient arriving at depth.out[0]: DetectorTape sets it before the backward
    TABLES = None         # a view-transform camera branch: engine's (rig-table getter, per-frame getter or None)
    calib = None          # the per-frame calibration of the step (a clone), None with the module rig's table

    def __init__(self, fus):
        self.fus, self.H, self.W, self.bc, self.pair = fus, fus.bev_h, fus.bev_w, fus.bev_channels, ConvPair()

    def _table_forward(self, calib, B, ncam, Hc, Wc, dev):
        """The branch's table for this step: the module rig's cached one, or per-frame tables built now from calib = (fp64
        [B, ncam, 4, 4], image_size).  Those live in the fusion engine's buffers, where the next forward replaces them: the tape
        keeps a clone of the calibration and the build's version for _current_table()."""
        rig_table, frame_tables = self.TABLES
        if calib is None:
            self.table = rig_table(self.fus, ncam, Hc, Wc, dev)
        else:
            self.shape = (B, ncam, Hc, Wc, dev)
            self.table = frame_tables(self.fus, calib, *self.shape)
            self.calib, self.version = (calib[0].to(dev).clone(), calib[1]), self.table.version
        return self.table

    def _current_table(self):
        """The forward's table in the backward, rebuilt from the kept calibration if another forward has replaced it since."""
        if self.calib is not None and self.table.version != self.version:
            self.table = self.TABLES[1](self.fus, self.calib, *self.shape)
            self.version = self.table.version
        return self.table

    def _depth_forward(self, logits, calib, B, ncam, Hc, Wc, rows) -> None:
        """After softmax_rows: the LiDAR depth targets and the cross entropy of the padded logits (DepthLossTape)."""
        if self.depth_sup is not None:
            self.depth = DepthLossTape(self.fus, self.depth_sup, calib, B, ncam, Hc, Wc, logits.device)
            self.depth.forward(logits, self.Dp, rows)

    def _depth_backward(self, dlogit, rows) -> None:
        """After softmax_rows_bwd, before depth_net's backward: the depth loss's share of dlogit."""
        if self.depth is not None and self.depth_grad is not None:
            self.depth.backward(self.pd, self.depth_grad, dlogit, self.Dp, rows)

    def _slot(self, buf):
        """This branch's [B*H*W][bev_channels] columns of a concatenated NHWC map."""
        rows = self.B * self.H * self.W
        return buf[:rows * self.ccs].view(rows, self.ccs)[:, self.slot * self.bc:(self.slot + 1) * self.bc]

    def _pair_to_slot(self, seq, x, B, concat, ccs, slot) -> None:
        """seq's conv pair on the fusion grid, then the copy into the slot."""
        self.B, self.ccs, self.slot = B, ccs, slot
        self._slot(concat)[:] = self.pair.forward(seq, x, B, self.H, self.W)[:B * self.H * self.W * self.bc].view(-1, self.bc)

    def _pair_from_slot(self, dconcat, sink):
        return self.pair.backward(self._slot(dconcat).contiguous().view(-1), sink)


class CameraMeanBranchTape(_FusionBranchTape):
    """Input NHWC features, geom = (B, ncam, Hc, Wc): camera average, camera_proj on the image grid, resize into the slot."""

    def forward(self, cam, B, concat, ccs, slot, geom, _) -> None:
        _, ncam, Hc, Wc = geom
        Cc = self.fus.camera_proj[0].weight.shape[1]
        self.geom, self.slot = (B, ncam, Hc * Wc, Cc), slot
        pooled = cam
        if ncam > 1:
            pooled = _new(B * Hc * Wc * Cc, cam.device)
            L.cam_mean(cam, pooled, B, ncam, Hc * Wc, Cc)
        t2 = self.pair.forward(self.fus.camera_proj, pooled, B, Hc, Wc)
        self.resize = Bilinear()
        self.resize.forward(t2, B, Hc, Wc, self.bc, self.H, self.W, y=concat[slot * self.bc:], y_cs=ccs)

    def backward(self, dconcat, sink):
        dcam = self.pair.backward(self.resize.backward(dconcat[self.slot * self.bc:]), sink)
        B, ncam, Pc, Cc = self.geom
        if ncam > 1:
            dpooled, dcam = dcam, _new(B * ncam * Pc * Cc, dconcat.device)
            L.cam_mean_bwd(dpooled, dcam, B, ncam, Pc, Cc)
        return dcam


class CameraProjectBranchTape(_FusionBranchTape):
    """Input NHWC features, geom = (B, ncam, Hc, Wc): the projection table onto the grid (the module rig's, or per-frame tables built
    here from calib = (fp64 [B, ncam, 4, 4], image_size)), camera_proj there, the slot copy; the transposed table in the backward.  The
    per-frame tables: _FusionBranchTape._table_forward / _current_table."""

    TABLES = (E.camera_table, E.frame_camera_tables)

    def forward(self, cam, B, concat, ccs, slot, geom, calib) -> None:
        _, ncam, Hc, Wc = geom
        fus, dev = self.fus, cam.device
        Cc = fus.camera_proj[0].weight.shape[1]
        self.geom = (ncam, Hc, Wc, Cc)
        tab = self._table_forward(calib, B, ncam, Hc, Wc, dev)
        proj = _new(B * self.H * self.W * Cc, dev)
        tab.project(cam, proj, B, Cc)
        self._pair_to_slot(fus.camera_proj, proj, B, concat, ccs, slot)

    def backward(self, dconcat, sink):
        dproj = self._pair_from_slot(dconcat, sink)
        B, (ncam, Hc, Wc, Cc) = self.B, self.geom
        dcam = _new(B * ncam * Hc * Wc * Cc, dconcat.device)
        self._current_table().project_backward(dproj, dcam, B, Cc)          # transposed table: every element written once
        return dcam


class _PaddedDepthNet:
    """depth_net as ConvBNLayer sees it: weight / bias with zero rows appended up to engine.depth_net_width (the data-gradient conv
    reads the layer's output channels as its Cin, a multiple of 32), and a sink that hands the first D rows of their gradients to the
    real parameters."""

    def __init__(self, conv, width: int):
        self.real, self.D = conv, conv.weight.shape[0]
        self.weight, self.bias = E.pad_depth_net(conv, width)
        self.weight.requires_grad_(conv.weight.requires_grad)
        self.bias.requires_grad_(conv.bias.requires_grad)
        self.stride, self.padding = conv.stride, conv.padding

    def sink(self, sink: GradSink):
        pad = self

        class _Sink:
            def add(self, p, g):
                real = pad.real.weight if p is pad.weight else pad.real.bias
                sink.add(real, g.reshape(p.shape)[:pad.D])
        return _Sink()


class DepthLossTape:
    """LiDAR depth supervision of a learned-depth branch tape (depth_supervision.py): the targets of depth_sup =
    (points (B, N, >= 3) fp32, counts (B,) int32 or None) under the step's calibration -- calib = (fp64 [B, ncam, 4, 4], image_size),
    or the module rig's for every frame (stride 0) when None -- and the cross entropy of the tape's padded logits against them.
    out = (mean loss, supervised pixels) stays on the device; the backward adds the loss's share to dlogit between the softmax
    backward and depth_net's, scaled by the gradient that arrives at the detector's sixth output."""

    def __init__(self, fus, depth_sup, calib, B, ncam, Hc, Wc, dev):
        from . import depth_supervision as DS
        points, counts = depth_sup
        if points.shape[0] != B:
            raise L.BevfError(f"depth_points holds {points.shape[0]} frames, the camera input {B}")
        if calib is None:
            rig = fus.camera_rig
            ct = E._rig_cached(fus, ("depth_calib",), (), "depth calibration", dev, lambda: DS.calib_tensor(rig, dev))
            image_size = rig.image_size
        else:
            ct, image_size = calib[0].to(dev).contiguous(), calib[1]
        self.D = fus.cam_depth[0]
        self.target = DS.build_targets(points, counts, ct, image_size, Hc, Wc, fus.cam_depth).view(-1)
        self.out = _new(2, dev)

    def forward(self, logits, width: int, rows: int) -> None:
        L.depth_ce(logits, width, self.target, rows, self.D, _new(L.depth_ce_work_doubles(), logits.device, torch.float64), self.out)

    def backward(self, pd, g, dlogit, width: int, rows: int) -> None:
        L.depth_ce_bwd(pd, self.D, self.target, g.reshape(1).float().contiguous(), self.out, dlogit, width, rows, self.D)


class _LearnedDepthBranchTape(_FusionBranchTape):
    """The learned-depth camera branches ('lift', 'frustum').  Input NHWC features, geom = (B, ncam, Hc, Wc): depth_net (padded,
    _PaddedDepthNet) -> softmax over the depth bins -> the depth loss if the step has depth_sup -> the subclass's spread of x * Pd
    over its table onto the grid -> camera_proj there, the slot copy.  Keeps x and Pd; the backward runs the spread's backward (dx
    and dPd in one pass), the softmax backward, the depth loss's share and depth_net's gradients, whose data gradient takes dx as
    its residual input: dcam = dx_spread + dx_depthnet without another pass over the feature map.  A subclass names its TABLES and
    supplies _spread and _spread_backward."""

    def forward(self, cam, B, concat, ccs, slot, geom, calib) -> None:
        _, ncam, Hc, Wc = geom
        fus, dev = self.fus, cam.device
        fus.check_lift_supported(calib)                              # (each looks at its own kind only, as in FlexibleBEVFusion.forward)
        fus.check_frustum_supported()
        Cc = fus.camera_proj[0].weight.shape[1]
        tab = self._table_forward(calib, B, ncam, Hc, Wc, dev)
        self.geom, self.Dp = (ncam, Hc, Wc, Cc), E.depth_net_width(tab.D)
        rows = B * tab.ncols
        self.padded = _PaddedDepthNet(fus.depth_net, self.Dp)
        self.dn = ConvBNLayer(self.padded, None, relu=False)
        logits, _, _ = self.dn.forward(cam, B * ncam, Hc, Wc)
        self.x, self.pd = cam, _new(rows * tab.D, dev)
        L.softmax_rows(logits, self.Dp, self.pd, tab.D, rows, tab.D)
        self._depth_forward(logits, self.calib, B, ncam, Hc, Wc, rows)
        proj = _new(B * self.H * self.W * Cc, dev)
        self._spread(tab, cam, self.pd, proj, B, Cc)
        self._pair_to_slot(fus.camera_proj, proj, B, concat, ccs, slot)

    def backward(self, dconcat, sink):
        dproj = self._pair_from_slot(dconcat, sink)
        B, Cc, tab, dev = self.B, self.geom[3], self._current_table(), dconcat.device
        rows = B * tab.ncols
        dx, dpd = _new(rows * Cc, dev), _new(rows * tab.D, dev)
        self._spread_backward(tab, self.x, self.pd, dproj, dx, dpd, B, Cc)  # every element of both written once
        dlogit = _new(rows * self.Dp, dev)
        L.softmax_rows_bwd(self.pd, dpd, tab.D, dlogit, self.Dp, self.Dp, rows, tab.D)
        self._depth_backward(dlogit, rows)
        dcam, _ = self.dn.backward(dlogit, self.padded.sink(sink), add=dx)  # dW, db; dx rides the data gradient's residual input
        return dcam


class CameraLiftBranchTape(_LearnedDepthBranchTape):
    """The lift gather through the module rig's lift table (a calibration is refused, so the depth loss takes the rig's too); the
    transposed table in the backward."""

    TABLES = (E.camera_lift_table, None)

    def _spread(self, tab, x, pd, proj, B, Cc) -> None:
        tab.lift(x, pd, proj, B, Cc)

    def _spread_backward(self, tab, x, pd, dproj, dx, dpd, B, Cc) -> None:
        tab.lift_backward(x, pd, dproj, dx, dpd, B, Cc)


class CameraFrustumBranchTape(_LearnedDepthBranchTape):
    """The lift-splat pool over the frustum table (the module rig's, or per-frame tables built here from calib = (fp64
    [B, ncam, 4, 4], image_size): _FusionBranchTape._table_forward / _current_table); the dense pool backward over cell_of."""

    TABLES = (E.camera_frustum_table, E.frame_frustum_tables)

    def _spread(self, tab, x, pd, proj, B, Cc) -> None:
        tab.pool(x, pd, proj, B, Cc)

    def _spread_backward(self, tab, x, pd, dproj, dx, dpd, B, Cc) -> None:
        tab.pool_backward(x, pd, dproj, dx, dpd, B, Cc)


class LidarVectorBranchTape(_FusionBranchTape):
    """Input the PointNet vector (B*C_l): lidar_init to the start_size^2 canvas, conv, x2 bilinear, conv, resize to the grid."""

    def forward(self, x, B, concat, ccs, slot, *_) -> None:
        fus, s0 = self.fus, self.fus.lidar_start_size
        self.slot = slot
        self.li0 = LinearLayer(fus.lidar_init[0], True)
        O = fus.lidar_init[2].weight.shape[0]
        self.li2 = LinearLayer(fus.lidar_init[2], False, (s0 * s0, O // (s0 * s0)))
        hid = self.li0.forward(x, B)
        grid0 = self.li2.forward(hid, B)
        self.c1 = ConvBNLayer(fus.lidar_upsample[0], fus.lidar_upsample[1], True)
        self.c2 = ConvBNLayer(fus.lidar_upsample[4], fus.lidar_upsample[5], True)
        g1, _, _ = self.c1.forward(grid0, B, s0, s0)
        self.up = Bilinear()
        s1 = 2 * s0
        g2 = self.up.forward(g1, B, s0, s0, self.c1.cout, s1, s1)
        g3, _, _ = self.c2.forward(g2, B, s1, s1)
        self.resize = Bilinear()                                       # (the identity map when s1 == H == W)
        self.resize.forward(g3, B, s1, s1, self.bc, self.H, self.W, y=concat[slot * self.bc:], y_cs=ccs)

    def backward(self, dconcat, sink):
        dg2, _ = self.c2.backward(self.resize.backward(dconcat[self.slot * self.bc:]), sink)
        dgrid0, _ = self.c1.backward(self.up.backward(dg2), sink)
        return self.li0.backward(self.li2.backward(dgrid0, sink), sink)


class LidarPillarsBranchTape(_FusionBranchTape):
    """Input the PointPillars NHWC canvas, on the fusion grid already: lidar_bev's two conv+BN+ReLU, then the slot copy."""

    def forward(self, x, B, concat, ccs, slot, *_) -> None:
        self._pair_to_slot(self.fus.lidar_bev, x, B, concat, ccs, slot)

    def backward(self, dconcat, sink):
        return self._pair_from_slot(dconcat, sink)


class RadarBranchTape(_FusionBranchTape):
    """Input the radar vector (B*C_r): radar_proj, broadcast to every cell, radar_refine's two conv+BN+ReLU, then the slot copy."""

    def forward(self, x, B, concat, ccs, slot, *_) -> None:
        P, bc = self.H * self.W, self.bc
        self.rp = LinearLayer(self.fus.radar_proj[0], True)
        rv = self.rp.forward(x, B)
        r0 = _new(B * P * bc, x.device)
        L.broadcast_nhwc(rv, r0, B, P, bc, bc)
        self._pair_to_slot(self.fus.radar_refine, r0, B, concat, ccs, slot)

    def backward(self, dconcat, sink):
        P, bc = self.H * self.W, self.bc
        dr0 = self._pair_from_slot(dconcat, sink)
        drv = torch.cat([colsum(dr0[b * P * bc:], P, bc) for b in range(self.B)])      # d(broadcast) = sum over cells
        return self.rp.backward(drv.contiguous(), sink)


class HistoryBranchTape(_FusionBranchTape):
    """Temporal fusion.  Input (prev_bev (B, bev_channels, H, W) fp32 or None, ego fp64 [B][4][4] on the device, its
    host copy or None): the ego-motion warp straight into the slot (zeros for a first frame); the backward is the pull kernel, run
    only when the caller wants the gradient of prev_bev (want_grad).  No parameters, no ReLU."""

    is_history = True
    want_grad = False

    def forward(self, x, B, concat, ccs, slot, *_) -> None:
        self.B, self.ccs, self.slot = B, ccs, slot
        prev, self.ego, self.ego_host = x
        from .encoders import pillar_grid
        self.grid = pillar_grid(self.fus.pc_range, self.H, self.W)[:4]
        if prev is None:
            self._slot(concat).zero_()
            return
        rows = prev.detach().permute(0, 2, 3, 1).contiguous()          # (a view of channels-last memory)
        L.bev_warp(rows, concat[slot * self.bc:], self.ego, B, self.H, self.W, self.bc, self.bc, ccs, self.grid)

    def backward(self, dconcat, sink):
        if not self.want_grad or self.ego is None:
            return None
        dx = _new(self.B * self.H * self.W * self.bc, dconcat.device)
        L.bev_warp_bwd(dconcat[self.slot * self.bc:], dx, self.ego, self.B, self.H, self.W, self.bc, self.ccs, self.grid, self.ego_host)
        return dx


class FusionTape:
    """FlexibleBEVFusion (ref src/fusion.py:209-297): NHWC camera features [B*ncam*Hc*Wc*C] with cam_geom = (B, ncam, Hc, Wc),
    LiDAR (B, C_l) vectors or the PointPillars NHWC canvas on the fusion grid, radar (B, C_r) vectors -> fused NHWC map
    [B*H*W*cout].  One branch tape per modality the module was built with; each one present fills one bev_channels slot of the
    concatenated map.  The branches run forward in the order camera, LiDAR, radar and backward in reverse, and both orders are
    relied on: RELU_TRACE records in forward order, and DetectorTape marks the gradients final (sink.ready()) in the camera
    callback, after radar and LiDAR have contributed theirs."""

    BRANCHES = dict(mean=CameraMeanBranchTape, project=CameraProjectBranchTape, lift=CameraLiftBranchTape,
                    frustum=CameraFrustumBranchTape, pointnet=LidarVectorBranchTape, pillars=LidarPillarsBranchTape,
                    sparse=LidarPillarsBranchTape)

    def __init__(self, fus):
        self.fus = fus
        self.branches = [self.BRANCHES[fus.camera_view_transform](fus) if fus.use_camera else None,
                         self.BRANCHES[fus.lidar_kind](fus) if fus.use_lidar else None, RadarBranchTape(fus) if fus.use_radar else None,
                         HistoryBranchTape(fus) if getattr(fus, "temporal", False) else None]

    def forward(self, cam_feat, cam_geom, lid_feat, rad_feat, B, camera_calib=None, depth_sup=None, history=None,
                history_grad: bool = False):
        """camera_calib ('project' / 'frustum' branches): (fp64 [B, ncam, 4, 4], image_size), see CameraProjectBranchTape.
        depth_sup ('frustum' / 'lift' branches): (points, counts) of the LiDAR depth supervision, see DepthLossTape; the camera
        branch then keeps its loss in .depth.
        history (temporal fusion): the triple of temporal.check_history, None = a first frame; history_grad: the backward computes
        the gradient of prev_bev (.dhistory)."""
        fus = self.fus
        if depth_sup is not None:
            self.branches[0].depth_sup = depth_sup
        if self.branches[3] is not None:
            history = (None, None, None) if history is None else history
            self.branches[3].want_grad = history_grad
        self.B, self.H, self.W, self.cout = B, fus.bev_h, fus.bev_w, fus.bev_channels
        feats = (cam_feat, lid_feat, rad_feat, history)
        present, ccs, B = E.concat_slots(fus, self.branches, feats,
                                         "expected input to have {cin} channels, but got {ccs} channels instead", B)
        concat = _new(B * self.H * self.W * ccs, present[0][1].device)
        names = {tape: name for tape, name in zip(self.branches, ("camera", "lidar", "radar", "history")) if tape is not None}
        self.present = [(names[tape], tape) for tape, _ in present]
        for slot, (tape, x) in enumerate(present):
            tape.forward(x, B, concat, ccs, slot, cam_geom, camera_calib)
        self.f1 = ConvBNLayer(fus.bev_fusion[0], fus.bev_fusion[1], True)
        self.f2 = ConvBNLayer(fus.bev_fusion[3], fus.bev_fusion[4], True)          # (the producer of the head's input)
        a1, _, _ = self.f1.forward(concat, B, self.H, self.W)
        fused, _, _ = self.f2.forward(a1, B, self.H, self.W)
        return fused

    def backward(self, dfused, sink: GradSink, pre=None, on_radar=None, on_lidar=None, on_camera=None):
        """pre: BatchNorm-backward partials for f2 that arrive with dfused (or None).  Each modality's input gradient (radar (B*C_r),
        LiDAR (B*C_l) or the pillar canvas, camera NHWC) goes to its callback as soon as it exists -- the detector continues into
        that encoder there -- and is returned as well: (drad, dlid, dcam).  The history slot, the last one, goes first; its gradient
        (NHWC, or None when nobody asked for it) stays in .dhistory."""
        da1, _, pre_f1 = self.f2.backward(dfused, sink, fuse_next=self.f1, pre=pre)
        dconcat, _ = self.f1.backward(da1, sink, pre=pre_f1)
        hooks = dict(camera=on_camera, lidar=on_lidar, radar=on_radar, history=None)
        grads = dict(camera=None, lidar=None, radar=None, history=None)
        for name, tape in reversed(self.present):
            grads[name] = tape.backward(dconcat, sink)
            if hooks[name] is not None:
                hooks[name](grads[name])
        self.dhistory = grads["history"]
        return grads["radar"], grads["lidar"], grads["camera"]


class HeadTape:
    """CenterNetHead (ref src/fusion.py:869-884) on an NHWC map [B*H*W*Cin]: the five 3x3 branches as one conv (engine.head_weights,
    rebuilt every step because the weights change), then the tail kernel -> five NCHW outputs."""

    def __init__(self, head):
        self.head = head

    def forward(self, x, B, H, W):
        hw = self.weights = E.head_weights(self.head)
        self.x, self.B, self.H, self.W, self.hc = x, B, H, W, hw.hc
        P = H * W
        hid, _, _ = conv_raw(x, hw.w3.permute(0, 2, 3, 1).contiguous().view(-1), hw.b3, B, H, W, hw.w3.shape[1], hw.w3.shape[0],
                             3, 1, 1, relu=True)
        self.hid = hid
        _trace_relu(hid, B * P, hw.w3.shape[0])
        self.outs = [torch.empty(B, c, H, W, device=x.device) for c in hw.cs]
        L.head_tail(hid, hw.w1, hw.b1, self.outs, B, P, hw.hc, hw.cs, hw.cs[0])
        return self.outs

    def backward(self, douts: List[torch.Tensor], sink: GradSink, fuse_next: Optional[ConvBNLayer] = None):
        """-> (gradient of the input NHWC map, BatchNorm-backward partials for `fuse_next`, the layer that produced the input, or
        None)."""
        hw, B, H, W, hc = self.weights, self.B, self.H, self.W, self.hc
        P = H * W
        dev = self.outs[0].device
        c5, cin = hw.w3.shape[0], hw.w3.shape[1]
        ctot = sum(hw.cs)
        dhid = _new(B * P * c5, dev)
        dw1, db1 = _zeros(ctot * hc, dev), _zeros(ctot, dev)
        gouts = [torch.zeros_like(o) if g is None else g.contiguous().float() for g, o in zip(douts, self.outs)]
        L.head_tail_bwd(self.hid, hw.w1, self.outs[0], gouts, dhid, dw1, db1, B, P, hc, hw.cs, hw.cs[0])
        o = 0
        for c1, n in zip(hw.convs1, hw.cs):
            sink.add(c1.weight, dw1[o * hc:(o + n) * hc])
            sink.add(c1.bias, db1[o:o + n])
            o += n
        # fused 3x3 head conv: ReLU mask, bias / weight / data gradients, split back per branch
        L.relu_mask(dhid, self.hid, B * P * c5)
        db3 = colsum(dhid, B * P, c5)
        dw3 = conv_wgrad(self.x, dhid, B, H, W, cin, c5, 3, 1, 1).permute(0, 3, 1, 2)
        for k, c3 in enumerate(hw.convs3):
            sink.add(c3.weight, dw3[k * hc:(k + 1) * hc])
            sink.add(c3.bias, db3[k * hc:(k + 1) * hc])
        if FUSE_BN_BACKWARD and fuse_next is not None and fuse_next.can_take_fused_dy() and dgrad_can_fuse_bn(B, H, W, cin, c5, 3, 1, 1):
            return conv_dgrad(dhid, hw.w3, B, H, W, cin, c5, 3, 1, 1, bnb=fuse_next.bnb_request())
        return conv_dgrad(dhid, hw.w3, B, H, W, cin, c5, 3, 1, 1), None


class SegHeadTape:
    """BEVSegmentationHead (seg_head.py) on an NHWC map [B*H*W*Cin]: the grid resample onto the map grid, the
    classifier's two conv + BN + ReLU, and its 1x1 layer padded to engine.depth_net_width (_PaddedDepthNet: the data gradient reads
    the layer's output channels as its Cin) -> logits (B, K, Ho, Wo).  The backward ends in the resample's pull kernel."""

    def __init__(self, head):
        self.head = head

    def forward(self, x, B):
        h = self.head
        (Ho, Wo), Cc, K = h.output_size, h.in_channels, h.num_classes
        self.B, self.Kp = B, E.depth_net_width(K)
        r = _new(B * Ho * Wo * Cc, x.device)
        L.bev_grid_resample(x, r, B, h.bev_h, h.bev_w, Ho, Wo, Cc, Cc, Cc, h.in_grid, h.out_grid)
        cl = h.classifier
        self.c1, self.c2 = ConvBNLayer(cl[0], cl[1], True), ConvBNLayer(cl[3], cl[4], True)
        self.padded = _PaddedDepthNet(cl[6], self.Kp)
        self.c3 = ConvBNLayer(self.padded, None, relu=False)
        a1, _, _ = self.c1.forward(r, B, Ho, Wo)
        a2, _, _ = self.c2.forward(a1, B, Ho, Wo)
        logits, _, _ = self.c3.forward(a2, B, Ho, Wo)
        out = torch.empty(B, K, Ho, Wo, device=x.device)
        L.nhwc_to_nchw(logits, out, B, K, Ho * Wo, self.Kp)
        return out

    def backward(self, dout, sink: GradSink):
        """dout (B, K, Ho, Wo) -> the gradient of the input NHWC map."""
        h, B = self.head, self.B
        (Ho, Wo), Cc, K = h.output_size, h.in_channels, h.num_classes
        dlogit = torch.zeros(B * Ho * Wo * self.Kp, device=dout.device)         # the padding columns carry no gradient
        L.nchw_to_nhwc(dout.contiguous().float(), dlogit, B, K, Ho * Wo, self.Kp)
        da2, _ = self.c3.backward(dlogit, self.padded.sink(sink))
        da1, _ = self.c2.backward(da2, sink)
        dr, _ = self.c1.backward(da1, sink)
        dx = _new(B * h.bev_h * h.bev_w * Cc, dout.device)
        L.bev_grid_resample_bwd(dr, dx, B, h.bev_h, h.bev_w, Ho, Wo, Cc, Cc, h.in_grid, h.out_grid)
        return dx


class IoUHeadTape:
    """IoUHead (iou_head.py) on an NHWC map [B*H*W*Cin]: conv3x3 + bias + ReLU, then the 1x1 layer padded to
    engine.depth_net_width (_PaddedDepthNet, as SegHeadTape's last layer) -> (B, 1, H, W)."""

    def __init__(self, head):
        self.head = head

    def forward(self, x, B, H, W):
        br = self.head.branch
        self.B, self.H, self.W, self.Kp = B, H, W, E.depth_net_width(1)
        self.c1 = ConvBNLayer(br[0], None, True)
        self.padded = _PaddedDepthNet(br[2], self.Kp)
        self.c2 = ConvBNLayer(self.padded, None, relu=False)
        hid, _, _ = self.c1.forward(x, B, H, W)
        cols, _, _ = self.c2.forward(hid, B, H, W)
        out = torch.empty(B, 1, H, W, device=x.device)
        L.nhwc_to_nchw(cols, out, B, 1, H * W, self.Kp)
        return out

    def backward(self, dout, sink: GradSink):
        """dout (B, 1, H, W) -> the gradient of the input NHWC map."""
        B, P = self.B, self.H * self.W
        dcols = torch.zeros(B * P * self.Kp, device=dout.device)                 # the padding columns carry no gradient
        L.nchw_to_nhwc(dout.contiguous().float(), dcols, B, 1, P, self.Kp)
        dhid, _ = self.c2.backward(dcols, self.padded.sink(sink))
        dx, _ = self.c1.backward(dhid, sink)
        return dx


def _pad_cols(t, rows: int, c: int, cp: int):
    """[rows][c] -> [rows][cp] with zero columns appended (the convolution kernels' 32-channel granule); t itself when c == cp."""
    if c == cp:
        return t
    out = torch.zeros(rows * cp, device=t.device)
    out.view(rows, cp)[:, :c] = t[:rows * c].view(rows, c)
    return out


def _pad_vec(v, n: int, np_: int, value: float):
    v = torch.full((n,), value, device=v.device) if v is None else v.detach().float()
    return torch.nn.functional.pad(v, (0, np_ - n), value=value).contiguous()


class RoIRowLayer:
    """One `Linear(no bias) -> BatchNorm1d -> ReLU` of RoIHead.shared_fc over the [B * K] RoI rows: the 1x1 convolution kernel on the
    row image, then the row BatchNorm with the device-side count (L.sparse_bn_*, cap = K), so rows past count[b] enter neither the
    statistics nor the gradients.  Widths are padded to the kernels' 32-channel granule with zero weights (gamma 1, beta 0 there: the
    padding columns stay exactly zero forwards and backwards); at the default widths (5 * 256 -> 256 -> 256) nothing is padded."""

    def __init__(self, lin, bn, cin: int, cinp: int, cout: int, coutp: int):
        self.lin, self.bn, self.cin, self.cinp, self.cout, self.coutp = lin, bn, cin, cinp, cout, coutp
        w = lin.weight.detach().float()
        self.wp = torch.nn.functional.pad(w, (0, cinp - cin, 0, coutp - cout)).contiguous()          # [coutp][cinp]

    def forward(self, x, count, B: int, K: int):
        bn, dev, F, Fp, R = self.bn, x.device, self.cout, self.coutp, B * K
        self.x, self.count, self.B, self.K = x, count, B, K
        self.y, _, _ = conv_raw(x, self.wp.view(-1), None, R, 1, 1, self.cinp, Fp, 1, 1, 0)
        self.gamma, self.beta = _pad_vec(bn.weight, F, Fp, 1.0), _pad_vec(bn.bias, F, Fp, 0.0)
        self.frozen = bn_is_frozen(bn)
        if self.frozen:
            self.mean = _pad_vec(bn.running_mean, F, Fp, 0.0)
            self.invstd = _pad_vec(torch.rsqrt(bn.running_var.detach().float() + bn.eps), F, Fp, 1.0)
        else:
            self.mean, self.invstd = _new(Fp, dev), _new(Fp, dev)
            work = torch.empty(L.sparse_bn_work_bytes(Fp), dtype=torch.uint8, device=dev)
            track = bn.track_running_stats and bn.running_mean is not None
            rm = rv = None
            if track:                                                        # (padded widths: the buffers go through padded copies)
                rm, rv = (bn.running_mean, bn.running_var) if F == Fp else (_pad_vec(bn.running_mean, F, Fp, 0.0),
                                                                            _pad_vec(bn.running_var, F, Fp, 1.0))
            with E._span("sparse_bn_stats"):
                L.sparse_bn_stats(self.y, count, B, K, Fp, bn.eps, -1.0 if bn.momentum is None else bn.momentum, rm, rv,
                                  bn.num_batches_tracked if track else None, self.mean, self.invstd, None, work)
            if track:
                if F != Fp:
                    bn.running_mean.copy_(rm[:F])
                    bn.running_var.copy_(rv[:F])
                for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):   # written through raw pointers
                    if t is not None:
                        torch.autograd.graph.increment_version(t)
        a = torch.zeros(R * Fp, device=dev)                                  # rows past the count stay zero
        with E._span("sparse_bn_apply"):
            L.sparse_bn_apply(self.y, count, B, K, Fp, self.mean, self.invstd, self.gamma, self.beta, a)
        return a

    def backward(self, da, sink: GradSink, need_dx: bool):
        bn, dev, F, Fp, B, K = self.bn, da.device, self.cout, self.coutp, self.B, self.K
        R = B * K
        dy, dgamma, dbeta, sums = torch.zeros(R * Fp, device=dev), _new(Fp, dev), _new(Fp, dev), _new(2 * Fp, dev)
        work = torch.empty(L.sparse_bn_work_bytes(Fp), dtype=torch.uint8, device=dev)
        with E._span("sparse_bn_backward"):
            L.sparse_bn_backward(self.y, da, self.count, B, K, Fp, self.mean, self.invstd, self.gamma, self.beta, self.frozen, dy,
                                 dgamma, dbeta, sums, work)
        sink.add(bn.weight, dgamma[:F])
        sink.add(bn.bias, dbeta[:F])
        dw = conv_wgrad(self.x, dy, R, 1, 1, self.cinp, Fp, 1, 1, 0).reshape(Fp, self.cinp)
        sink.add(self.lin.weight, dw[:F, :self.cin])
        if not need_dx:
            return None
        return conv_dgrad(dy, self.wp.view(Fp, self.cinp, 1, 1), R, 1, 1, self.cinp, Fp, 1, 1, 0)


class RoIHeadTape:
    """RoIHead (roi_head.py) on an NHWC map [B*H*W*C] and padded RoIs: the five-point gather (keeping its sample
    table), two RoIRowLayer, and cls_out / reg_out as one 8-column layer padded to engine.depth_net_width -> pred (B, K, 8).  The
    backward ends in the gather's pull kernel when the map wants a gradient."""

    def __init__(self, head):
        self.head = head

    def forward(self, x, boxes, count, B: int, K: int, H: int, W: int, bev_range):
        h, dev = self.head, x.device
        Cc, F, R = h.in_channels, h.fc, B * K
        p32 = lambda n: (n + 31) // 32 * 32
        C5, self.Op = 5 * Cc, E.depth_net_width(8)
        C5p, Fp = p32(C5), p32(F)
        self.geom = (B, K, H, W, Cc, C5, C5p, F, Fp)
        self.count = count
        feat = _new(R * C5, dev)
        self.table = torch.empty(L.roi_bev_points_table_words(B, K), dtype=torch.int32, device=dev)
        with E._span("roi_bev_points"):
            L.roi_bev_points(x, boxes, count, feat, self.table, H, W, Cc, Cc, bev_range)
        fc = h.shared_fc
        self.l1 = RoIRowLayer(fc[0], fc[1], C5, C5p, F, Fp)
        self.l2 = RoIRowLayer(fc[3], fc[4], F, Fp, F, Fp)
        a1 = self.l1.forward(_pad_cols(feat, R, C5, C5p), count, B, K)
        self.a2 = self.l2.forward(a1, count, B, K)
        w3 = torch.cat([h.cls_out.weight.detach(), h.reg_out.weight.detach()], 0).float()
        b3 = torch.cat([h.cls_out.bias.detach(), h.reg_out.bias.detach()], 0).float()
        self.w3p = torch.nn.functional.pad(w3, (0, Fp - F, 0, self.Op - 8)).contiguous()               # [Op][Fp]
        cols, _, _ = conv_raw(self.a2, self.w3p.view(-1), torch.nn.functional.pad(b3, (0, self.Op - 8)).contiguous(), R, 1, 1, Fp,
                              self.Op, 1, 1, 0)
        return cols[:R * self.Op].view(R, self.Op)[:, :8].reshape(B, K, 8)

    def backward(self, dpred, sink: GradSink, need_dx: bool):
        """dpred (B, K, 8) -> the gradient of the input NHWC map (None unless need_dx)."""
        h, dev = self.head, dpred.device
        B, K, H, W, Cc, C5, C5p, F, Fp = self.geom
        R, Op = B * K, self.Op
        dcols = torch.zeros(R * Op, device=dev)                                 # the padding columns carry no gradient
        dcols.view(R, Op)[:, :8] = dpred.reshape(R, 8).float()
        db = colsum(dcols, R, Op)
        sink.add(h.cls_out.bias, db[:1])
        sink.add(h.reg_out.bias, db[1:8])
        dw3 = conv_wgrad(self.a2, dcols, R, 1, 1, Fp, Op, 1, 1, 0).reshape(Op, Fp)
        sink.add(h.cls_out.weight, dw3[:1, :F])
        sink.add(h.reg_out.weight, dw3[1:8, :F])
        da2 = conv_dgrad(dcols, self.w3p.view(Op, Fp, 1, 1), R, 1, 1, Fp, Op, 1, 1, 0)
        da1 = self.l2.backward(da2, sink, True)
        dx0 = self.l1.backward(da1, sink, need_dx)
        if not need_dx:
            return None
        dfeat = dx0 if C5 == C5p else dx0[:R * C5p].view(R, C5p)[:, :C5].contiguous().view(-1)
        dx = _new(B * H * W * Cc, dev)
        with E._span("roi_bev_points_bwd"):
            L.roi_bev_points_bwd(dfeat, self.table, self.count, dx, B, K, H, W, Cc)
        return dx


class DeconvBNLayer:
    """ConvTranspose2d(kernel = stride = s, no bias) -> train-mode BN -> ReLU, written into a channel slice of a wider NHWC map
    (the FPN neck's concat).  Forward: the raw transposed convolution (csrc/deconv.hip; s = 1: a 1x1 convolution
    with the transposed weight), BatchNorm over the N*sH*sW rows, then a copy into the slice -- bn_apply has one channel stride
    for its input and output, and the raw rows are kept for the backward.  Backward: the slice of the concat's gradient copied out,
    BatchNorm backward, dx = conv(dy, W, k = s, stride s, pad 0) on the forward convolution kernel, dW = that convolution's weight
    gradient with x and dy swapped."""

    def __init__(self, deconv, bn):
        self.deconv, self.bn = deconv, bn
        w = deconv.weight
        self.cin, self.cout, self.s = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])

    def forward(self, x, N, H, W, concat, off: int, ctot: int):
        w, s, cin, cout = self.deconv.weight.detach(), self.s, self.cin, self.cout
        self.x, self.N, self.H, self.W, self.off, self.ctot = x, N, H, W, off, ctot
        Mo = N * H * W * s * s
        if s == 1:
            raw, _, _ = conv_raw(x, w[:, :, 0, 0].t().contiguous().view(-1), None, N, H, W, cin, cout, 1, 1, 0)
        else:
            raw = _new(Mo * cout, x.device)
            with E._span("deconv_f32", flops=2.0 * Mo * cout * cin, nbytes=4.0 * (N * H * W * cin + Mo * cout)):
                L.deconv_nhwc(x, L.deconv_pack(w), None, None, raw, N=N, H=H, W=W, Cin=cin, x_cs=cin, Cout=cout, y_cs=cout, s=s,
                              relu=False)
        y, self.bns = bn_train_forward(raw, self.bn, Mo, cout, relu=True)
        concat[:Mo * ctot].view(Mo, ctot)[:, off:off + cout].copy_(y[:Mo * cout].view(Mo, cout))
        return Mo

    def backward(self, dconcat, sink: GradSink):
        """dconcat: the gradient of the whole concat [N*sH*sW][ctot] -> the gradient of this layer's input."""
        s, cin, cout, N, H, W = self.s, self.cin, self.cout, self.N, self.H, self.W
        Mo = N * H * W * s * s
        dy = _new(Mo * cout, dconcat.device)
        dy[:Mo * cout].view(Mo, cout).copy_(dconcat[:Mo * self.ctot].view(Mo, self.ctot)[:, self.off:self.off + cout])
        dxraw, dgamma, dbeta = bn_train_backward(dy, self.bns, self.bn, relu=True)
        sink.add(self.bn.weight, dgamma)
        sink.add(self.bn.bias, dbeta)
        w = self.deconv.weight
        if s == 1:
            dw = conv_wgrad(self.x, dxraw, N, H, W, cin, cout, 1, 1, 0)                          # [cout][1][1][cin]
            sink.add(w, dw.reshape(cout, cin).t().reshape(w.shape))
            return conv_dgrad(dxraw, w.detach().permute(1, 0, 2, 3), N, H, W, cin, cout, 1, 1, 0)
        # the forward k = s, stride s, pad 0 convolution of dy [N][sH][sW][cout] with the same weights, as OHWI [cin][s][s][cout]
        dw = conv_wgrad(dxraw, self.x, N, s * H, s * W, cout, cin, s, s, 0)                      # [cin][s][s][cout]
        sink.add(w, dw.permute(0, 3, 1, 2).reshape(w.shape))
        dx, _, _ = conv_raw(dxraw, w.detach().permute(0, 2, 3, 1).contiguous().view(-1), None, N, s * H, s * W, cout, cin, s, s, 0)
        return dx


class BackboneTape:
    """bev_backbone.BEVBackbone on an NHWC map [B*H*W*Cin]: per level the stage's ConvBNLayers, then its DeconvBNLayer into the
    concat [B*H*W*out_channels].  A stage output has two consumers, the next stage and its own deblock: the backward sums the two
    gradients (add_) before it walks the stage."""

    def __init__(self, mod):
        self.mod = mod

    def forward(self, x, B, H, W):
        m = self.mod
        self.B, self.H, self.W = B, H, W
        ct = m.out_channels
        concat = _new(B * H * W * ct, x.device)
        self.stages, self.ups, self.sizes = [], [], []
        cur, h, w, off = x, H, W, 0
        for block, deblock in zip(m.backbone.blocks, m.neck.deblocks):
            mods = list(block)
            layers = [ConvBNLayer(mods[i], mods[i + 1], True) for i in range(0, len(mods), 3)]
            for layer in layers:
                cur, h, w = layer.forward(cur, B, h, w)
            up = DeconvBNLayer(deblock[0], deblock[1])
            up.forward(cur, B, h, w, concat, off, ct)
            off += up.cout
            self.stages.append(layers)
            self.ups.append(up)
            self.sizes.append(B * h * w * layers[-1].cout)
        return concat

    def backward(self, dconcat, sink: GradSink, need_dx=True):
        """dconcat [B*H*W*out_channels] -> the gradient of the input map (None with need_dx=False)."""
        d_next = None
        for i in reversed(range(len(self.stages))):
            d = self.ups[i].backward(dconcat, sink)
            if d_next is not None:
                add_(d, d_next, self.sizes[i])
            layers = self.stages[i]
            for j in reversed(range(len(layers))):
                d, _ = layers[j].backward(d, sink, need_dx=need_dx or i > 0 or j > 0)
            d_next = d
        return d_next


# ---- the detector ------------------------------------------------------------------------------------------------------------------

class DetectorTape:
    """FlexibleMultiModal3DDetector (bev + centernet) as a composition of module tapes: the encoders of the modalities present, in
    the order radar, camera, LiDAR (RELU_TRACE follows it), then fusion and head.  The backward walks them in reverse and marks
    where gradients become final for the data-parallel all-reduce (sink.ready()).  A model with a seg head has
    two consumers of the fused map: SegHeadTape runs after the head, and the backward sums the two gradients before the fusion."""

    def __init__(self, model, camera_calib=None, depth_sup=None, history=None):
        self.m = model
        self.history = history                    # temporal fusion: (prev_bev, ego, host ego), a constant of the step (no gradient)
        self.camera_calib = camera_calib          # per-frame calibration of the 'project' camera branch (FusionTape.forward)
        self.depth_sup = depth_sup                # (points, counts): LiDAR depth supervision of the 'frustum' / 'lift' branch, a sixth output

    def forward(self, imgs, pts, radars):
        m = self.m
        has_cam = m.use_camera and imgs is not None
        has_lid = m.use_lidar and pts is not None
        has_rad = m.use_radar and radars is not None
        if not (has_cam or has_lid or has_rad):
            raise ValueError("No modality features provided")
        self.radar = self.camera = self.lidar = None
        cam_feat = cam_geom = lid_feat = rad_feat = None
        if has_rad:
            renc = m.radar_encoder
            self.radar = RadarTape(renc.radar_encoder, renc.fusion_method, getattr(renc, "fusion_fc", None))
            rad_feat = self.radar.forward(radars)
            B = self.radar.B
        if has_cam:
            self.camera = CameraTape(m.camera_encoder)
            cam_feat = self.camera.forward(imgs)
            B = self.camera.B
            cam_geom = (B, self.camera.n, self.camera.H, self.camera.W)
        if has_lid:
            if getattr(m.lidar_encoder, "is_pillars", False):              # PointPillars: NHWC fp32 canvas on the BEV grid
                _no_input_grad(pts, "the LiDAR points")
                self.lidar = PillarPFNLayer(m.lidar_encoder)
            elif getattr(m.lidar_encoder, "is_sparse", False):             # sparse voxels: the same kind of canvas, the same route
                _no_input_grad(pts, "the LiDAR points")
                self.lidar = SparseEncoderTape(m.lidar_encoder)
            else:
                self.lidar = PointMLPTape(m.lidar_encoder, 5, fuse_max=True)
            lid_feat = self.lidar.forward(pts)
            B = self.lidar.B
        self.fusion = FusionTape(m.fusion)
        if self.history is None:
            fused = self.fusion.forward(cam_feat, cam_geom, lid_feat, rad_feat, B, self.camera_calib if has_cam else None, self.depth_sup)
        else:
            fused = self.fusion.forward(cam_feat, cam_geom, lid_feat, rad_feat, B, self.camera_calib if has_cam else None,
                                        self.depth_sup, self.history)
            self.bev = (fused, B)                 # the 'bev' output is copied from it (detector_train_forward)
        self.bb = None
        if getattr(m, "bev_backbone", None) is not None:   # the decoder between the fuser and every head; the
            self.bb = BackboneTape(m.bev_backbone)         # 'bev' output above stays the fuser's map
            fused = self.bb.forward(fused, B, self.fusion.H, self.fusion.W)
        self.feat = (fused, B)                    # the map the heads read: the 'feat' output of a model with a RoI head is copied from it
        self.head = HeadTape(m.det_head)
        outs = self.head.forward(fused, B, self.fusion.H, self.fusion.W)
        if self.depth_sup is not None:
            self.depth_out = self.fusion.branches[0].depth.out
            outs = outs + [self.depth_out[0]]
        self.seg = None
        if getattr(m, "seg_head", None) is not None:  # the fused map's second consumer; 'seg' is appended: the positions above stay
            self.seg = SegHeadTape(m.seg_head)
            outs = outs + [self.seg.forward(fused, B)]
        self.iou = None
        if getattr(m, "iou_head", None) is not None:  # one more consumer of the fused map; 'iou' is appended after 'seg'
            self.iou = IoUHeadTape(m.iou_head)
            outs = outs + [self.iou.forward(fused, B, self.fusion.H, self.fusion.W)]
        return outs

    def backward(self, douts: List[torch.Tensor], sink: GradSink) -> list:
        if self.depth_sup is not None:
            self.fusion.branches[0].depth_grad = douts[5]
        if self.seg is None and self.iou is None and self.bb is None:
            dfused, pre_f2 = self.head.backward(douts[:5], sink, fuse_next=self.fusion.f2)
        else:
            # several consumers of `fused`: the head's fused BatchNorm-backward partials would cover its own share only, so the head
            # returns a plain data gradient, the seg head's and the IoU head's are added, and f2 runs its own BatchNorm backward
            # over the sum
            dfused, pre_f2 = self.head.backward(douts[:5], sink)
            nf = self.fusion.B * self.fusion.H * self.fusion.W * (self.fusion.cout if self.bb is None else self.bb.mod.out_channels)
            d_iou = douts[-1] if self.iou is not None else None
            d_seg = None if self.seg is None else (douts[-2] if self.iou is not None else douts[-1])
            if d_seg is not None:
                add_(dfused, self.seg.backward(d_seg, sink), nf)
            if d_iou is not None:
                add_(dfused, self.iou.backward(d_iou, sink), nf)
            if self.bb is not None:                     # the heads' producer is the neck's concat: through the decoder to the fuser
                dfused = self.bb.backward(dfused, sink)

        def camera(dfeat):
            sink.ready()              # head, fusion, radar, LiDAR (the 164 MB dense layer): reduce under the camera trunk
            self.camera.backward(dfeat, sink)

        self.fusion.backward(dfused, sink, pre_f2, on_radar=lambda d: self.radar.backward(d, sink),
                             on_lidar=lambda d: self.lidar.backward(d, sink), on_camera=camera)
        return [None, None, None]


_GRAD_REDUCER = None


def set_grad_reducer(reducer) -> None:
    """Data-parallel training: install a replicas.GradReducer and the detector's backward averages its gradients over
    the ranks itself, bucket by bucket as they become final, overlapped with the rest of the backward (None: off)."""
    global _GRAD_REDUCER
    _GRAD_REDUCER = reducer


class _TapeFn(torch.autograd.Function):
    """The autograd node of every tape path: the detector, or one module used on its own.  `fwd(*inputs)` runs the tape's forward
    and returns its outputs; `bwd(douts, sink)` runs its backward and returns one gradient per input (None where there is none).
    `reducer`: the GradReducer the sink hands final gradients to (the detector's), or None.  `what` names the module in errors."""

    @staticmethod
    def forward(ctx, what, fwd, bwd, reducer, n_in, *tensors):
        with torch.no_grad():
            outs = fwd(*tensors[:n_in])
        ctx.what, ctx.bwd, ctx.reducer, ctx.n_in, ctx.params = what, bwd, reducer, n_in, tensors[n_in:]
        # The tape keeps its own tensors; autograd gets fresh aliases.  Returning the tape's objects would close a
        # reference cycle through C++ (output -> grad_fn -> ctx -> tape -> output) that the garbage collector cannot
        # see: every step's activations (~11 GiB at config 4) would stay allocated for ever.
        return tuple(o.detach() for o in outs)

    @staticmethod
    def backward(ctx, *douts):
        if ctx.bwd is None:
            raise RuntimeError(f"Trying to backward through the {ctx.what} a second time: its saved activations were freed")
        global _ZPOOL
        with torch.no_grad():
            pool = _ZPOOL = _ZeroPool(next(g for g in douts if g is not None).device)
            try:
                sink = GradSink(ctx.reducer)
                dins = ctx.bwd(list(douts), sink)
                sink.finish()
            finally:
                _ZPOOL = None
        ctx.bwd = None                                    # the tape's activations are dead now: hand them back to the allocator
        need = ctx.needs_input_grad[5:5 + ctx.n_in]
        dins = [_owned(d, pool) if (n and d is not None) else None for d, n in zip(dins, need)]
        return (None,) * 5 + (*dins, *_param_grads(sink, ctx.params, pool))


def _owned(g, pool):
    """Never hand out a view of the shared zero pool."""
    if g is not None and g.untyped_storage().data_ptr() == pool.buf.untyped_storage().data_ptr():
        return g.clone()
    return g


def _param_grads(sink: GradSink, params, pool) -> list:
    grads = []
    for p in params:
        g = sink.get(p)
        if g is not None:
            g = _owned(g.reshape(p.shape).contiguous(), pool)
        grads.append(g)
    return grads


def _trainable(module: nn.Module) -> list:
    return [p for p in module.parameters() if p.requires_grad]


def any_bn_training(module: nn.Module) -> bool:
    return any(isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training for m in module.modules())


def wants_train_path(module: nn.Module) -> bool:
    """A module in train mode takes the tape when BatchNorm runs on batch statistics somewhere in it (then even under no_grad: the running
    buffers move, as in torch) or when autograd is recording -- use_bn=False encoders (ref src/encoders.py:258-269, 520-529) and modules
    whose BatchNorm layers were all put in eval mode still train their weights; the eval engines keep no gradient path."""
    return any_bn_training(module) or torch.is_grad_enabled()


def detector_train_forward(model, imgs, pts, radars, camera_calib=None, depth_sup=None, history=None) -> Dict[str, torch.Tensor]:
    """depth_sup = (points, counts): the LiDAR depth supervision of the 'frustum' / 'lift' camera branch (DepthLossTape); the
    result then carries 'depth_loss', a sixth output of the same autograd node, and 'depth_pixels', the supervised pixels.
    history = (prev_bev, ego, host ego) of a model with temporal fusion (temporal.check_history): a constant of the step; the result
    then carries 'bev', a detached owned copy of the fused map."""
    tape = DetectorTape(model, camera_calib, depth_sup, history)
    outs = _TapeFn.apply("detector", tape.forward, tape.backward, _GRAD_REDUCER, 3, imgs, pts, radars, *_trainable(model))
    res = dict(zip(E.HEAD_BRANCHES, outs))
    if depth_sup is not None:
        res["depth_loss"], res["depth_pixels"] = outs[5], tape.depth_out[1].clone()
    if tape.seg is not None:
        res["seg"] = outs[-2] if tape.iou is not None else outs[-1]
    if tape.iou is not None:
        res["iou"] = outs[-1]
    if history is not None:
        from .temporal import own_bev
        fus = model.fusion
        res["bev"] = own_bev(tape.bev[0], tape.bev[1], fus.bev_h, fus.bev_w, fus.bev_channels)
    if getattr(model, "roi_head", None) is not None:                      # the second stage trains on a constant map
        from .temporal import own_bev
        fus = model.fusion
        res["feat"] = own_bev(tape.feat[0], tape.feat[1], fus.bev_h, fus.bev_w, model.roi_head.in_channels)
    return res


# ---- stand-alone modules under train-mode BatchNorm (ref src/encoders.py:792-846 calls freshly built encoders, i.e. in train mode) ----
# Each checks its inputs, builds its tape and converts between the reference's layouts and the tape's flat NHWC buffers.

def _no_input_grad(x, what: str) -> None:
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise L.BevfError(f"training: {what} has no gradient path on the device (the reference's training loop never asks for "
                          "one, ref src/train_detect.py:401-434); detach the input")


def _nhwc(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W) -> flat NHWC fp32 buffer."""
    return E.to_nhwc(x.float().contiguous()).float().reshape(-1)


def _flat(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().float().reshape(-1)


def camera_encoder_train_forward(enc, x: torch.Tensor) -> torch.Tensor:
    """ResNetCameraEncoder.forward under train-mode BatchNorm (ref src/encoders.py:133-172): batch statistics, running buffers
    updated, gradients for every trainable parameter."""
    _no_input_grad(x, "the camera images")
    tape = CameraTape(enc)

    def fwd(x):
        feat = tape.forward(x)
        return (E.to_nchw(feat, tape.B * tape.n, tape.cout, tape.H, tape.W),)

    def bwd(douts, sink):
        tape.backward(_nhwc(douts[0].reshape(tape.B * tape.n, tape.cout, tape.H, tape.W)), sink)
        return [None]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(enc))
    return out.view(tape.B, tape.n, tape.cout, tape.H, tape.W) if x.dim() == 5 else out


def pointnet_train_forward(enc, x: torch.Tensor) -> torch.Tensor:
    """PointNetLiDAREncoder.forward under train-mode BatchNorm (ref src/encoders.py:271-306) -> (B, feat_dim)."""
    _no_input_grad(x, "the LiDAR points")
    if getattr(enc, "return_point_features", False):
        raise L.BevfError("training: PointNetLiDAREncoder(return_point_features=True) has no train-mode path on the device "
                          "(the detector uses the global feature, ref src/fusion.py:1105-1108); call .eval() for per-point features")
    tape = PointMLPTape(enc, 5, fuse_max=True)

    def fwd(x):
        return (tape.forward(x)[:tape.B * tape.cout].view(tape.B, tape.cout),)

    def bwd(douts, sink):
        tape.backward(_flat(douts[0]), sink)
        return [None]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(enc))
    return out


def pillar_train_forward(enc, x: torch.Tensor) -> torch.Tensor:
    """PillarLiDAREncoder.forward under train-mode BatchNorm -> canvas (B, pfn_channels, bev_h, bev_w), gradients for pfn.*."""
    _no_input_grad(x, "the LiDAR points")
    tape = PillarPFNLayer(enc)

    def fwd(x):
        return (E.to_nchw(tape.forward(x), tape.B, enc.pfn_channels, enc.bev_h, enc.bev_w),)

    def bwd(douts, sink):
        tape.backward(_nhwc(douts[0]), sink)
        return [None]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(enc))
    return out


def sparse_train_forward(enc, x: torch.Tensor) -> torch.Tensor:
    """SparseLiDAREncoder.forward under train-mode BatchNorm -> canvas (B, out_channels, bev_h, bev_w), gradients for the five
    conv / BatchNorm pairs."""
    _no_input_grad(x, "the LiDAR points")
    tape = SparseEncoderTape(enc)

    def fwd(x):
        return (E.to_nchw(tape.forward(x), tape.B, enc.out_channels, enc.bev_h, enc.bev_w),)

    def bwd(douts, sink):
        tape.backward(_nhwc(douts[0]), sink)
        return [None]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(enc))
    return out


def vfe_train_forward(layer, x: torch.Tensor) -> torch.Tensor:
    """VFELayer.forward under train-mode BatchNorm (ref src/encoders.py:431-455): Linear -> BatchNorm1d over all B*Nv*P rows (padding
    rows included, as the reference) -> ReLU -> max over the P points of a voxel -> (B, Nv, out_channels)."""
    _no_input_grad(x, "the voxel points")
    B, Nv, P, Cc = x.shape                                        # a 3-D input raises ValueError exactly like the reference
    if Cc > 16:
        raise L.BevfError(f"training: VFELayer(in_channels={Cc}) has a train-mode path for point features of <= 16 channels only")
    G, M = B * Nv, B * Nv * P
    first = PointFirstLayer(layer.linear, layer.bn)               # reads only .weight / .bias of the Linear
    idx = None

    def fwd(x):
        nonlocal idx
        a = first.forward(x.detach().float().contiguous().view(M, Cc), M, Cc)
        g, idx = group_max_with_index(a, G, P, first.c0)
        return (g[:G * first.c0].view(B, Nv, first.c0),)

    def bwd(douts, sink):
        first.backward(group_max_scatter(_flat(douts[0]), idx, G, P, first.c0), sink)
        return [None]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(layer))
    return out


def radar_train_forward(enc, radar_list) -> torch.Tensor:
    """MultiRadarEncoder.forward (ref src/encoders.py:619-661), or one RadarEncoder (ref :527-557, `radar_list` a single tensor),
    under train-mode BatchNorm -> (B, feat_dim)."""
    single = isinstance(radar_list, torch.Tensor)
    sweeps = [radar_list] if single else list(radar_list)
    for r in sweeps:
        _no_input_grad(r, "the radar points")
    tape = (RadarTape(enc, "max") if single
            else RadarTape(enc.radar_encoder, enc.fusion_method, getattr(enc, "fusion_fc", None)))

    def fwd(*pts):
        return (tape.forward(pts).reshape(-1)[:tape.B * tape.cout].view(tape.B, tape.cout),)

    def bwd(douts, sink):
        tape.backward(_flat(douts[0]), sink)
        return [None] * len(sweeps)

    (out,) = _TapeFn.apply("module", fwd, bwd, None, len(sweeps), *sweeps, *_trainable(enc))
    return out


def fusion_train_forward(fus, camera_features=None, lidar_features=None, radar_features=None, camera_calib=None,
                         history=None) -> torch.Tensor:
    """FlexibleBEVFusion.forward under train-mode BatchNorm (ref src/fusion.py:209-297) -> (B, bev_channels, bev_h, bev_w), with
    gradients for the parameters AND for the three feature inputs -- and, with temporal fusion, for prev_bev = history[0] (history:
    the triple of temporal.check_history)."""
    cam = camera_features if fus.use_camera else None
    lid = lidar_features if fus.use_lidar else None
    rad = radar_features if fus.use_radar else None
    first = next((t for t in (cam, lid, rad) if t is not None), None)
    if first is None:
        raise ValueError("No modality features provided")
    B = first.shape[0]
    pillars = fus.lidar_kind in ("pillars", "sparse")                  # the LiDAR input is an NCHW canvas
    geom = None
    if cam is not None:
        geom = (B, cam.shape[1], cam.shape[3], cam.shape[4]) if cam.dim() == 5 else (B, 1, cam.shape[2], cam.shape[3])
    tape = FusionTape(fus)
    prev = None if history is None else history[0]
    if prev is not None:
        E.require_cuda(prev)
    prev_grad = prev is not None and prev.requires_grad and torch.is_grad_enabled()

    def fwd(cam, lid, rad, prev=None):
        cam_nhwc = None
        if cam is not None:
            _, n, h, w = geom
            cam_nhwc = _nhwc(cam.detach().reshape(B * n, -1, h, w))
        lid_in = None if lid is None else lid.detach().float().contiguous()
        if lid_in is not None and pillars:                             # NCHW pillar canvas -> NHWC
            lid_in = _nhwc(lid_in)
        extra = () if history is None else (None, (prev,) + tuple(history[1:]), prev_grad)
        fused = tape.forward(cam_nhwc, geom, lid_in, None if rad is None else rad.detach().float().contiguous(), B,
                             camera_calib if cam_nhwc is not None else None, *extra)
        return (E.to_nchw(fused, B, tape.cout, tape.H, tape.W),)

    def bwd(douts, sink):
        drad, dlid, dcam = tape.backward(_nhwc(douts[0]), sink)
        if dcam is not None:
            _, n, h, w = geom
            dcam = E.to_nchw(dcam, B * n, fus.camera_proj[0].weight.shape[1], h, w).view(cam.shape)
        if dlid is not None and pillars:
            dlid = E.to_nchw(dlid, B, lid.shape[1], lid.shape[2], lid.shape[3])
        elif dlid is not None:
            dlid = dlid.reshape(-1)[:lid.numel()].view(lid.shape)
        if drad is not None:
            drad = drad.reshape(-1)[:rad.numel()].view(rad.shape)
        if history is None:
            return [dcam, dlid, drad]
        dprev = tape.dhistory
        if dprev is not None:                                          # NHWC rows -> (B, C, H, W), channels-last memory
            dprev = dprev[:prev.numel()].view(B, tape.H, tape.W, tape.cout).permute(0, 3, 1, 2)
        return [dcam, dlid, drad, dprev]

    if history is None:
        (out,) = _TapeFn.apply("module", fwd, bwd, None, 3, cam, lid, rad, *_trainable(fus))
    else:
        (out,) = _TapeFn.apply("module", fwd, bwd, None, 4, cam, lid, rad, prev, *_trainable(fus))
    return out


def head_train_forward(head, x: torch.Tensor) -> Dict[str, torch.Tensor]:
    """CenterNetHead.forward with a gradient path (ref src/fusion.py:869-884; the head has no BatchNorm, so train and eval mode
    compute the same values): gradients for its parameters and for the BEV map `x` (B, C, H, W)."""
    B, Cin, H, W = x.shape
    tape = HeadTape(head)

    def fwd(x):
        return tuple(tape.forward(_nhwc(x.detach()), B, H, W))

    def bwd(douts, sink):
        dx, _ = tape.backward(douts, sink)
        return [E.to_nchw(dx, B, Cin, H, W)]

    outs = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(head))
    return dict(zip(E.HEAD_BRANCHES, outs))


def seg_head_train_forward(head, x: torch.Tensor) -> torch.Tensor:
    """BEVSegmentationHead.forward under train-mode BatchNorm -> logits (B, K, Ho, Wo), with gradients for the parameters and for
    the BEV map `x` (B, C, H, W)."""
    B, Cin, H, W = x.shape
    tape = SegHeadTape(head)

    def fwd(x):
        return (tape.forward(_nhwc(x.detach()), B),)

    def bwd(douts, sink):
        return [E.to_nchw(tape.backward(douts[0], sink), B, Cin, H, W)]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(head))
    return out




def bev_backbone_train_forward(mod, x: torch.Tensor) -> torch.Tensor:
    """BEVBackbone.forward under train-mode BatchNorm -> (B, out_channels, H, W), with gradients for the parameters and for the
    BEV map `x` (B, C, H, W)."""
    B, Cin, H, W = x.shape
    tape = BackboneTape(mod)

    def fwd(x):
        return (E.to_nchw(tape.forward(_nhwc(x.detach()), B, H, W), B, mod.out_channels, H, W),)

    def bwd(douts, sink):
        return [E.to_nchw(tape.backward(_nhwc(douts[0]), sink), B, Cin, H, W)]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(mod))
    return out


def iou_head_train_forward(head, x: torch.Tensor) -> torch.Tensor:
    """IoUHead.forward with a gradient path (no BatchNorm: the eval-mode values) -> (B, 1, H, W), with gradients for the parameters
    and for the BEV map `x` (B, C, H, W)."""
    B, Cin, H, W = x.shape
    tape = IoUHeadTape(head)

    def fwd(x):
        return (tape.forward(_nhwc(x.detach()), B, H, W),)

    def bwd(douts, sink):
        return [E.to_nchw(tape.backward(douts[0], sink), B, Cin, H, W)]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(head))
    return out


def roi_head_train_forward(head, x: torch.Tensor, boxes: torch.Tensor, count: torch.Tensor, bev_range) -> torch.Tensor:
    """RoIHead.forward under train-mode BatchNorm -> pred (B, K, 8), with gradients for the parameters and, when it asks for one, for
    the BEV map `x` (B, C, H, W).  The RoIs are constants of the step."""
    B, Cin, H, W = x.shape
    K = boxes.shape[1]
    tape = RoIHeadTape(head)
    need_dx = x.requires_grad

    def fwd(x):
        return (tape.forward(_nhwc(x.detach()), boxes, count, B, K, H, W, bev_range),)

    def bwd(douts, sink):
        dx = tape.backward(douts[0], sink, need_dx)
        return [E.to_nchw(dx, B, Cin, H, W) if dx is not None else None]

    (out,) = _TapeFn.apply("module", fwd, bwd, None, 1, x, *_trainable(head))
    return out


# ---- loss with gradient ------------------------------------------------------------------------------------------------------------

class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, tgt_keys, *tensors):
        preds = dict(zip(E.HEAD_BRANCHES, tensors[:5]))
        tgt = dict(zip(tgt_keys, tensors[5:]))
        vals = L.centernet_loss(preds, tgt, weights)
        ctx.preds, ctx.tgt, ctx.weights = preds, tgt, weights
        return tuple(vals[i].clone() for i in range(6))

    @staticmethod
    def backward(ctx, g_total, *g_rest):
        for g in g_rest:
            if g is not None and bool((g != 0).any()):
                raise NotImplementedError("backward through the individual loss terms is not built; use total_loss")
        preds = ctx.preds
        dev = preds["heatmap"].device
        dp = [torch.zeros_like(preds[n], dtype=torch.float32) for n in E.HEAD_BRANCHES]
        scratch = torch.empty(4, device=dev)
        L.centernet_loss_bwd(preds, ctx.tgt, ctx.weights, dp, scratch)
        gt = g_total if g_total is not None else torch.zeros((), device=dev)
        return (None, None, *[t * gt for t in dp], *([None] * len(ctx.tgt)))


def loss_with_grad(predictions: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor], weights) -> Dict[str, torch.Tensor]:
    keys = tuple(targets.keys())
    vals = _LossFn.apply(tuple(weights), keys, *[predictions[n] for n in E.HEAD_BRANCHES], *[targets[k] for k in keys])
    names = ("total_loss", "heatmap_loss", "offset_loss", "size_loss", "rot_loss", "vel_loss")
    return dict(zip(names, vals))


# ---- optimiser pieces on device ------------------------------------------------------------------------------------------------------

def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (L2) with the norm and the scaling on device (ref src/train_detect.py:431)."""
    params = [p for p in parameters if p.grad is not None]
    dev = params[0].grad.device
    flat = torch.cat([p.grad.detach().reshape(-1).float() for p in params])
    work = torch.empty(512, dtype=torch.float64, device=dev)
    out = torch.empty(2, device=dev)
    L.grad_norm(flat, work, max_norm, out)
    for p in params:
        p.grad.mul_(out[1])
    return out[0]


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (ref src/train_detect.py:725-741: lr 1e-4, weight_decay 0.01) on L.adamw_step.

    The parameters that receive gradients are moved into ONE flat fp32 arena on the first step (each Parameter becomes
    a view of it, so state_dict / load_state_dict keep working); a step is then one gradient gather, optionally the
    global-norm clip of ref src/train_detect.py:431 (`max_grad_norm`, folded into the update as a device-side
    factor), and one AdamW launch over the whole arena instead of one per tensor."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._arenas = None

    def _build(self, chosen=None):
        """Arena per group over the parameters that receive gradients (or `chosen`: per-group lists, when a saved
        state is loaded before the first step)."""
        self._arenas = []
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None] if chosen is None else chosen[gi]
            if not ps:
                self._arenas.append(None)
                continue
            dev = ps[0].device
            if dev.type != "cuda" or any(p.dtype != torch.float32 or p.device != dev for p in ps):
                raise RuntimeError("FusedAdamW: parameters must be fp32 tensors on one cuda device")
            n = sum(p.numel() for p in ps)
            flat = torch.empty(n, device=dev)
            off = 0
            for p in ps:
                k = p.numel()
                flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + k].view(p.shape)
                off += k
            self._arenas.append(dict(params=ps, flat=flat, m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev),
                                     work=torch.empty(512, dtype=torch.float64, device=dev),
                                     clip=torch.empty(2, device=dev), step=0))

    @torch.no_grad()
    def step(self, closure=None):
        if self._arenas is None:
            self._build()
        for group, ar in zip(self.param_groups, self._arenas):
            with_grad = [p for p in group["params"] if p.grad is not None]
            if ar is None:
                if with_grad:
                    raise RuntimeError("FusedAdamW: the set of parameters with gradients changed; build a new optimiser")
                continue
            if len(with_grad) != len(ar["params"]) or any(a is not b for a, b in zip(with_grad, ar["params"])):
                raise RuntimeError("FusedAdamW: the set of parameters with gradients changed; build a new optimiser")
            g = torch.cat([p.grad.reshape(-1) for p in with_grad])
            clip = None
            if self.max_grad_norm is not None:
                L.grad_norm(g, ar["work"], self.max_grad_norm, ar["clip"])
                clip = ar["clip"]
                self.last_grad_norm = ar["clip"][0]
            ar["step"] += 1
            b1, b2 = group["betas"]
            L.adamw_step(ar["flat"], g, ar["m"], ar["v"], clip, group["lr"], b1, b2, group["eps"], group["weight_decay"], ar["step"])
            for p in with_grad:                      # the kernel wrote through raw pointers: tell torch (and the
                torch.autograd.graph.increment_version(p)   # engines' repack signature) that the values changed

    # ---- torch.optim.AdamW's state layout, both ways (checkpoint compatibility) ---------------------------
    def state_dict(self):
        """Same structure as torch.optim.AdamW.state_dict(): per-parameter `step` / `exp_avg` / `exp_avg_sq`, indexed by
        the parameter's position; the file loads into either optimiser."""
        index, groups, k = {}, [], 0
        for group in self.param_groups:
            ids = []
            for p in group["params"]:
                index[id(p)] = k
                ids.append(k)
                k += 1
            g = {key: val for key, val in group.items() if key != "params"}
            g.update(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                     decoupled_weight_decay=True)
            g["params"] = ids
            groups.append(g)
        state = {}
        for ar in self._arenas or []:
            if ar is None:
                continue
            off = 0
            for p in ar["params"]:
                n = p.numel()
                state[index[id(p)]] = {"step": torch.tensor(float(ar["step"])),
                                       "exp_avg": ar["m"][off:off + n].view(p.shape).clone(),
                                       "exp_avg_sq": ar["v"][off:off + n].view(p.shape).clone()}
                off += n
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"])
                                                       for a, b in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict does not match the optimiser's parameter groups")
        chosen, entries = [], []
        for saved, group in zip(groups, self.param_groups):
            for key in ("lr", "betas", "eps", "weight_decay"):
                if key in saved:
                    group[key] = tuple(saved[key]) if key == "betas" else saved[key]
            have = [(p, state_dict["state"][i]) for i, p in zip(saved["params"], group["params"]) if i in state_dict["state"]]
            chosen.append([p for p, _ in have])
            entries.append([e for _, e in have])
        with torch.no_grad():
            self._build(chosen)
            for ar, ent in zip(self._arenas, entries):
                if ar is None:
                    continue
                off, steps = 0, set()
                for p, e in zip(ar["params"], ent):
                    n = p.numel()
                    ar["m"][off:off + n].copy_(e["exp_avg"].reshape(-1))
                    ar["v"][off:off + n].copy_(e["exp_avg_sq"].reshape(-1))
                    steps.add(int(float(e["step"])))
                    off += n
                if len(steps) > 1:
                    raise ValueError(f"FusedAdamW keeps one step count per group; the loaded state has {sorted(steps)}")
                ar["step"] = steps.pop() if steps else 0
