"""Bit anchor of the train-mode BatchNorm kernels and of the kernels that evaluate relu(batchnorm(x)) on load (csrc/bn_rows.h,
norm_train.hip, the max-pool / group-max part of train_misc.hip).

The "fused equals chain" tests of test_gpu_training.py compare kernels that share bn_rows.h with each other.  This module is the
anchor outside that code: every case runs ONE raw entry point on inputs made on the CPU with `synth` (uniform only: pure
arithmetic, the same bits on every host) and compares the SHA-256 of each output with tests/golden/bn_kernel_bits.json, which
was recorded from a library built at the commit BEFORE the kernels were moved onto the shared header.  The kernels are
deterministic (fixed-order two-stage sums, no float atomics), so the match is exact.  The fixture also holds a digest of each
case's inputs: a changed generator shows up as such, not as a kernel difference.

Record (only when an intended change of the arithmetic replaces the anchor):
    python -m tests.test_gpu_bn_bits [path of the libbevf_hip.so to record from] [output json]
"""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import synth

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_kernel_bits.json")
EPS = 1e-5

ROWS = [(7, 64, 64),            # fewer rows than row lanes
        (70000, 64, 64),        # partial grid capped at 1024: unrolled body and tail, the tail only for some threads
        (45000, 96, 104),       # C/4 = 24 does not divide 256: 16 idle threads; x strided
        (5500, 1024, 1024),     # one row lane: partials written without the LDS merge
        (5500, 1280, 1280)]     # the quad loop for C > 1024
BWD_ROWS = [ROWS[1], ROWS[2], ROWS[4]]
POOLED = [(1, 1, 1, 64), (3, 7, 10, 32),
          (1, 150, 331, 64), (2, 223, 225, 32)]   # odd sizes, M just above 3 * 1024 * lanes: some threads unrolled, the rest tail only
POOL = [(1, 1, 1, 64), (3, 7, 10, 32), (2, 9, 13, 64)]
GROUPS = [(1, 1, 64), (2, 129, 256), (3, 700, 96)]   # (2, 129, .): one point past a 128-point chunk


def call(name, *args):
    rc = getattr(L.lib(), name)(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (name, L.lib().bevf_last_error().decode())


def sha(*named):
    """SHA-256 over (name, bytes) of each tensor."""
    h = hashlib.sha256()
    for name, t in named:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def ptr(t):
    return None if t is None else t.data_ptr()


def u(n, seed, lo=-1.0, hi=1.0):
    return synth.uniform((n,), seed, lo, hi)


def quantised(n, seed, q):           # multiples of q in [-2, 2]: windows and groups hold ties
    return torch.round(u(n, seed, -2.0, 2.0) / q) * q


@functools.lru_cache(maxsize=2)
def rows_inputs(M, C, cs):
    """CPU inputs shared by the cases of one row shape (x fills the pad columns too; they must never reach an output)."""
    return dict(x=u(M * cs, 1, -2.0, 3.0), res=u(M * C, 2), dy=u(M * C, 3), y=u(M * C, 4), mean=u(C, 5, 0.2, 0.8),
                invstd=u(C, 6, 0.5, 2.0), gamma=u(C, 7, 0.5, 1.5), beta=u(C, 8, -0.3, 0.3))


def bn_work(C):
    return torch.empty(L.lib().bevf_bn_work_floats(C), device="cuda")


def run_stats(M, C, cs):
    i = {"x": rows_inputs(M, C, cs)["x"]}
    d = {k: v.cuda() for k, v in i.items()}
    o = {k: torch.empty(C, device="cuda") for k in ("mean", "var", "invstd")}
    call("bevf_bn_stats_f32", ptr(d["x"]), ptr(bn_work(C)), ptr(o["mean"]), ptr(o["var"]), ptr(o["invstd"]), M, C, cs, EPS)
    return i, o


def run_apply(M, C, cs, relu, res):
    a = rows_inputs(M, C, cs)
    i = {k: a[k] for k in ("x", "mean", "invstd", "gamma", "beta") + (("res",) if res else ())}
    d = {k: v.cuda() for k, v in i.items()}
    y = torch.empty(M * C, device="cuda")
    call("bevf_bn_apply_f32", ptr(d["x"]), ptr(d["mean"]), ptr(d["invstd"]), ptr(d["gamma"]), ptr(d["beta"]), ptr(d.get("res")),
         ptr(y), M, C, cs, relu)
    return i, {"y": y}


# bn_backward variants: (relu argument, inputs passed (the others are NULL), dx written)
BWD_VARIANTS = {
    "relu0": (0, ("dy", "x", "mean", "invstd", "gamma", "beta"), True),
    "relu1_y": (1, ("dy", "y", "x", "mean", "invstd", "gamma", "beta"), True),        # the masked dY is written back
    "relu1_noy": (1, ("dy", "x", "mean", "invstd", "gamma", "beta"), True),           # mask recomputed, written back
    "relu2": (2, ("dy", "x", "mean", "invstd", "gamma", "beta"), True),               # dY must come back untouched
    "relu4_frozen": (4, ("dy", "x", "mean", "invstd", "gamma", "beta"), True),
    "relu6_frozen_remask": (6, ("dy", "x", "mean", "invstd", "gamma", "beta"), True),
    "sums_only": (1, ("dy", "y", "gamma", "beta"), False),                            # dx = NULL, x = NULL
    "no_gamma_beta": (1, ("dy", "x", "mean", "invstd"), True),
}


def run_backward(M, C, cs, variant):
    relu, names, with_dx = BWD_VARIANTS[variant]
    a = rows_inputs(M, C, cs)
    i = {k: a[k] for k in names}
    d = {k: v.cuda() for k, v in i.items()}
    o = {"dgamma": torch.zeros(C, device="cuda"), "dbeta": torch.zeros(C, device="cuda"), "dy": d["dy"]}
    if with_dx:
        o["dx"] = torch.zeros(M * cs, device="cuda")
    call("bevf_bn_backward_f32", ptr(d["dy"]), ptr(d.get("y")), ptr(d.get("x")), ptr(d.get("mean")), ptr(d.get("invstd")),
         ptr(d.get("gamma")), ptr(d.get("beta")), ptr(bn_work(C)), ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(o.get("dx")), M, C, cs, relu)
    return i, o


def run_from_partials():
    M, C, G = 333, 256, 5
    i = dict(dy=u(M * C, 11), x=u(M * C, 12, -2.0, 3.0), mean=u(C, 13, 0.2, 0.8), invstd=u(C, 14, 0.5, 2.0), gamma=u(C, 15, 0.5, 1.5),
             part=u(G * C * 2, 16, -50.0, 50.0))
    d = {k: v.cuda() for k, v in i.items()}
    o = {k: torch.zeros(n, device="cuda") for k, n in (("dgamma", C), ("dbeta", C), ("dx", M * C))}
    call("bevf_bn_backward_from_partials_f32", ptr(d["dy"]), ptr(d["x"]), ptr(d["mean"]), ptr(d["invstd"]), ptr(d["gamma"]),
         ptr(d["part"]), G, ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(o["dx"]), M, C, C)
    return i, o


def run_gmax(sums_only):
    B, P, C, cs = 3, 700, 96, 96
    i = dict(dg=u(B * C, 21), gmax=u(B * C, 22), idx=synth.randint((B * C,), 23, 0, P).to(torch.int32), x=u(B * P * cs, 24, -2.0, 3.0),
             mean=u(C, 25, 0.2, 0.8), invstd=u(C, 26, 0.5, 2.0), gamma=u(C, 27, 0.5, 1.5))
    d = {k: v.cuda() for k, v in i.items()}
    o = {k: torch.zeros(n, device="cuda") for k, n in (("dgm", B * C), ("dgamma", C), ("dbeta", C))}
    if sums_only:
        call("bevf_gmax_bn_sums_f32", ptr(d["dg"]), ptr(d["gmax"]), ptr(d["idx"]), ptr(d["x"]), ptr(d["mean"]), ptr(d["invstd"]),
             ptr(o["dgm"]), ptr(o["dgamma"]), ptr(o["dbeta"]), B, P, C, cs)
    else:
        o["dx"] = torch.zeros(B * P * cs, device="cuda")        # this is bn_bwd_apply with no dY
        call("bevf_gmax_bn_backward_f32", ptr(d["dg"]), ptr(d["gmax"]), ptr(d["idx"]), ptr(d["x"]), ptr(d["mean"]), ptr(d["invstd"]),
             ptr(d["gamma"]), ptr(o["dgm"]), ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(o["dx"]), B, P, C, cs)
    return i, o


def pooled_size(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def run_pool_bn_backward(N, H, W, C):
    Ho, Wo = pooled_size(H, W)
    i = dict(dpool=u(N * Ho * Wo * C, 31), idx=synth.randint((N * Ho * Wo * C,), 32, 0, 9).to(torch.uint8),
             x=u(N * H * W * C, 33, -2.0, 3.0), mean=u(C, 34, 0.2, 0.8), invstd=u(C, 35, 0.5, 2.0), gamma=u(C, 36, 0.5, 1.5),
             beta=u(C, 37, -0.3, 0.3))
    d = {k: v.cuda() for k, v in i.items()}
    o = {k: torch.zeros(n, device="cuda") for k, n in (("dgamma", C), ("dbeta", C), ("dx", N * H * W * C))}
    call("bevf_pool_bn_backward_f32", ptr(d["dpool"]), ptr(d["idx"]), ptr(d["x"]), ptr(d["mean"]), ptr(d["invstd"]), ptr(d["gamma"]),
         ptr(d["beta"]), ptr(bn_work(C)), ptr(o["dgamma"]), ptr(o["dbeta"]), ptr(o["dx"]), N, H, W, C)
    return i, o


def run_maxpool(N, H, W, C, kind):
    Ho, Wo = pooled_size(H, W)
    n_in, n_out = N * H * W * C, N * Ho * Wo * C
    if kind == "bwd":
        i = dict(dy=u(n_out, 41), idx=synth.randint((n_out,), 42, 0, 9).to(torch.uint8))
        d = {k: v.cuda() for k, v in i.items()}
        o = {"dx": torch.zeros(n_in, device="cuda")}
        call("bevf_maxpool3x3s2_bwd_f32", ptr(d["dy"]), ptr(d["idx"]), ptr(o["dx"]), N, H, W, C)
        return i, o
    i = dict(x=quantised(n_in, 43, 0.5))                        # ties: the first maximum must win
    if kind == "bn_relu":
        i.update(mean=u(C, 44, 0.2, 0.8), invstd=u(C, 45, 0.5, 2.0), gamma=u(C, 46, 0.5, 1.5), beta=u(C, 47, -0.3, 0.3))
    d = {k: v.cuda() for k, v in i.items()}
    o = {"y": torch.zeros(n_out, device="cuda"), "idx": torch.zeros(n_out, dtype=torch.uint8, device="cuda")}
    if kind == "bn_relu":
        call("bevf_bn_relu_maxpool3x3s2_idx_f32", ptr(d["x"]), ptr(d["mean"]), ptr(d["invstd"]), ptr(d["gamma"]), ptr(d["beta"]),
             ptr(o["y"]), ptr(o["idx"]), N, H, W, C)
    else:
        call("bevf_maxpool3x3s2_idx_f32", ptr(d["x"]), ptr(o["y"]), ptr(o["idx"]), N, H, W, C)
    return i, o


def run_group_max(G, P, C, affine):
    i = dict(x=quantised(G * P * C, 51, 0.25))
    if affine:
        i.update(mean=u(C, 52, 0.2, 0.8), invstd=u(C, 53, 0.5, 2.0), gamma=u(C, 54, 0.5, 1.5), beta=u(C, 55, -0.3, 0.3))
    d = {k: v.cuda() for k, v in i.items()}
    o = {"y": torch.zeros(G * C, device="cuda"), "idx": torch.zeros(G * C, dtype=torch.int32, device="cuda")}
    work = torch.empty(L.lib().bevf_group_max_idx_work_bytes(G, P, C), dtype=torch.uint8, device="cuda")
    if affine:
        call("bevf_bn_relu_group_max_idx_f32", ptr(d["x"]), ptr(d["mean"]), ptr(d["invstd"]), ptr(d["gamma"]), ptr(d["beta"]), ptr(o["y"]),
             ptr(o["idx"]), ptr(work), G, P, C)
    else:
        call("bevf_group_max_idx_f32", ptr(d["x"]), ptr(o["y"]), ptr(o["idx"]), ptr(work), G, P, C)
    return i, o


def _name(prefix, shape, tag=None):
    return prefix + ":" + "x".join(map(str, shape)) + (":" + tag if tag else "")


CASES = {}
for s in ROWS:
    CASES[_name("bn_stats", s)] = functools.partial(run_stats, *s)
    for tag, relu, res in (("relu_res", 1, True), ("relu", 1, False), ("plain", 0, False)):
        CASES[_name("bn_apply", s, tag)] = functools.partial(run_apply, *s, relu, res)
for s in BWD_ROWS:
    for v in BWD_VARIANTS:
        if v != "no_gamma_beta" or s == ROWS[2]:
            CASES[_name("bn_backward", s, v)] = functools.partial(run_backward, *s, v)
CASES["bn_backward_from_partials:333x256x256:G5"] = run_from_partials
CASES["gmax_bn_backward:3x700x96x96"] = functools.partial(run_gmax, False)
CASES["gmax_bn_sums:3x700x96x96"] = functools.partial(run_gmax, True)
for s in POOLED:
    CASES[_name("pool_bn_backward", s)] = functools.partial(run_pool_bn_backward, *s)
for s in POOL:
    CASES[_name("maxpool3x3s2_idx", s)] = functools.partial(run_maxpool, *s, "plain")
    CASES[_name("bn_relu_maxpool3x3s2_idx", s)] = functools.partial(run_maxpool, *s, "bn_relu")
    CASES[_name("maxpool3x3s2_bwd", s)] = functools.partial(run_maxpool, *s, "bwd")
for s in GROUPS:
    CASES[_name("group_max_idx", s)] = functools.partial(run_group_max, *s, False)
    CASES[_name("bn_relu_group_max_idx", s)] = functools.partial(run_group_max, *s, True)


def digests(name):
    ins, outs = CASES[name]()
    torch.cuda.synchronize()
    return {"in": sha(*sorted(ins.items())), "out": {k: sha((k, v)) for k, v in sorted(outs.items())}}


@functools.lru_cache(maxsize=1)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_these_cases(gpu):
    assert sorted(fixture()) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_the_recorded_kernels(gpu, name):
    want, got = fixture()[name], digests(name)
    assert got["in"] == want["in"], "the input generator changed (not a kernel difference): record again from the anchor commit"
    assert got["out"] == want["out"], sorted(k for k in want["out"] if got["out"].get(k) != want["out"][k])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1]:
        L.LIB_PATH = os.path.abspath(sys.argv[1])                # before the first lib() call
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(out, "w") as f:
        json.dump({name: digests(name) for name in CASES}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases from {L.LIB_PATH} -> {out}")
