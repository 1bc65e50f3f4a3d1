"""References of the BEV backbone / FPN neck tests: the transposed convolution's formula as a plain numpy loop, the module's
forward walked layer by layer with torch's own fp64 operators, and the parameter-gradient rule of the standalone training tests."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from tests.conftest import rel_err


def deconv_ref(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """y[n, s*h+i, s*w+j, co] = sum_ci x[n,h,w,ci] * W[ci,co,i,j]: x (N,H,W,Cin) NHWC, w (Cin,Cout,s,s) -> (N,sH,sW,Cout), fp64."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, H, W, Cin = x.shape
    assert w.shape[0] == Cin and w.shape[2] == w.shape[3]
    Cout, s = w.shape[1], w.shape[2]
    y = np.zeros((N, s * H, s * W, Cout), np.float64)
    for n in range(N):
        for h in range(H):
            for ww in range(W):
                for i in range(s):
                    for j in range(s):
                        y[n, s * h + i, s * ww + j, :] = x[n, h, ww, :] @ w[:, :, i, j]
    return y


def _bn(bn, x, training):
    """nn.BatchNorm2d.forward spelt out: batch statistics and the buffer update in train mode (the functional form leaves the
    batch counter to its caller), the running buffers in eval mode -- also for one frozen layer inside a module that trains."""
    if training and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1
    return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, training, bn.momentum, bn.eps)


def _walk(seq, x, training):
    """One `blocks[i]` / `deblocks[i]` Sequential through torch's functional operators."""
    for m in seq:
        if isinstance(m, torch.nn.ConvTranspose2d):
            x = F.conv_transpose2d(x, m.weight, None, stride=m.stride)
        elif isinstance(m, torch.nn.Conv2d):
            x = F.conv2d(x, m.weight, m.bias, stride=m.stride, padding=m.padding)
        elif isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            x = _bn(m, x, training and m.training)
        elif isinstance(m, torch.nn.ReLU):
            x = F.relu(x)
        else:
            raise TypeError(type(m))
    return x


def ref_copy(module):
    """The module as a CPU fp64 deep copy (train / eval flags kept)."""
    return copy.deepcopy(module).cpu().double()


def ref_forward_on(ref, x):
    """Walk `ref` (a ref_copy) over x (NCHW): stages, then each level's deblock, then the channel concat.  Never calls forward()."""
    ups = []
    for block, deblock in zip(ref.backbone.blocks, ref.neck.deblocks):
        x = _walk(block, x, ref.training)
        ups.append(_walk(deblock, x, ref.training))
    return torch.cat(ups, 1)


def ref_forward(module, x):
    with torch.no_grad():
        return ref_forward_on(ref_copy(module), x.detach().cpu().double())


def check_params(mod, ref, hard=2e-2, tight=2e-3, most=8, prefix=""):
    """The rule of tests/test_gpu_standalone_train.py's _check_params, restated: relative L2 error per parameter gradient with a
    floor of 5e-5 of the whole gradient norm; every tensor within `hard`, at most max(2, n // 8) above `tight`; BatchNorm running
    buffers within 2e-5.  `mod` / `ref`: modules with matching parameter names (`prefix` selects a subset)."""
    gref = dict(ref.named_parameters())
    gn = float(torch.sqrt(sum((p.grad.double().cpu() ** 2).sum() for p in ref.parameters() if p.grad is not None)))
    loose, checked, worst = 0, 0, []
    for name, p in mod.named_parameters():
        if not name.startswith(prefix):
            continue
        r = gref[name].grad
        assert p.grad is not None and r is not None, name
        g, r = p.grad.cpu().double(), r.cpu().double()
        l2 = float((g - r).norm() / (r.norm() + 5e-5 * gn))
        worst.append((round(l2, 6), name))
        loose += l2 > tight
        checked += 1
    worst.sort(reverse=True)
    print("param gradients, worst:", worst[:4])
    assert checked > 0 and worst[0][0] <= hard, worst[:6]
    assert loose <= max(2, checked // most), (loose, checked, worst[:6])
    rb = dict(ref.named_buffers())
    for n1, b1 in mod.named_buffers():
        if n1.startswith(prefix):
            assert rel_err(b1.cpu().double(), rb[n1].cpu().double()) <= 2e-5, n1
