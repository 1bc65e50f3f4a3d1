"""Launch trace of the camera-to-BEV branches ('project', 'lift', 'frustum') in FusionEngine and FusionTape.

The parity tests hold what these branches compute against fp64 references inside a tolerance.  This module holds HOW they compute it:
every case replaces `_lib._call` -- the one function every launch goes through -- with a recorder that calls through, and keeps per
launch the entry point's name and every argument `_lib.SIGNATURES` does not type as a pointer (a pointer becomes null / non-null, a
descriptor struct its integer and float fields plus the null-ness of its pointers).  The host-side table builds of camera_rig are
recorded the same way (`# host build_projection_table`), and marks (`# run 2`, `# backward`, ...) separate a case's phases.  The
trace, and the SHA-256 of every forward output, must equal tests/golden/camera_branch_trace.json, which was recorded at the commit
BEFORE the branches' shared steps were given one text each: the same entry points, in the same order, with the same scalars, on the
eval and on the training path.

Gradients are not hashed: conv_wgrad, bilinear_bwd and the head's weight gradient add floats atomically, so their bits differ from
run to run; the fp64 tests pin them, and the trace pins the launches that make them.

Shapes: 2 frames x 2 cameras of 64x96 images (4x6 features), BEV 16x24, the default depth bins, camera+lidar with the PointNet
encoder -- the smallest that still reach every path.  Cases: the fusion module in eval mode ('project' static fp32 / bf16 and
per-frame, 'lift', 'frustum' static and per-frame), each run twice on one module (the second run of a static rig builds no table);
the detector in train mode, forward + backward ('project' per-frame, 'lift' without / with depth_points, 'frustum' static, per-frame,
per-frame with depth_points); and the stale-version path of the per-frame tables ('project', 'frustum'): forward with calibration A,
forward with calibration B on the same module, then the backward of the first, which must rebuild A's tables.

Record (only when an intended change of the launches replaces the anchor):
    python -m tests.test_gpu_camera_branch_trace [output json]
"""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

from bevfusion_multimodal_3d_object_detection_amd import _lib as L
from bevfusion_multimodal_3d_object_detection_amd import camera_rig as CR
from bevfusion_multimodal_3d_object_detection_amd import fusion, synth, training

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "camera_branch_trace.json")
B, NCAM, IMG_H, IMG_W, HC, WC, BEV_H, BEV_W, NPTS = 2, 2, 64, 96, 4, 6, 16, 24, 300
TABLE_BUILDS = ("bevf_camera_table_build_f64", "bevf_frustum_table_build_f64", "# host build_projection_table",
                "# host build_lift_table")
_INT = (C.c_int, C.c_int32, C.c_size_t, C.c_int64)
_FLOAT = (C.c_float, C.c_double)


def sha(*named):
    """SHA-256 over (name, bytes) of each tensor."""
    h = hashlib.sha256()
    for name, t in named:
        h.update(name.encode())
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# ---- the recorder ------------------------------------------------------------------------------------------------------------------

def _null(v):
    return "0" if not v else "p"


def _value(typ, v):
    """One argument (or struct field) of ctypes type `typ` as trace text."""
    if typ in _INT:
        return str(int(v))
    if typ in _FLOAT:
        return repr(float(v))
    if isinstance(typ, type) and issubclass(typ, C.Array):
        return "[" + ",".join(_value(typ._type_, e) for e in v) + "]"
    if isinstance(typ, type) and issubclass(typ, C._Pointer) and issubclass(typ._type_, C.Structure):
        s = v._obj                                                   # the wrappers pass ctypes.byref(desc)
        return "{" + ",".join(f"{n}={_value(t, getattr(s, n))}" for n, t in s._fields_) + "}"
    return _null(v)                                                  # c_void_p, POINTER(c_float): a pointer


class Recorder:
    """Context manager: `_lib._call` and camera_rig's host table builds record into .trace and call through.  The training step's
    per-shape pixel tables (training._PIXTAB, filled by launches on first use, for the whole process) are set aside meanwhile, so
    that a case records the same launches whatever ran before it."""

    def __init__(self):
        self.trace = []

    def mark(self, text):
        self.trace.append("# " + text)

    def __enter__(self):
        self._call, self._host = L._call, {n: getattr(CR, n) for n in ("build_projection_table", "build_lift_table")}
        self._pixtab = dict(training._PIXTAB)
        training._PIXTAB.clear()

        def call(name, *args):
            types = L.SIGNATURES[name][1]
            assert len(types) == len(args) + 1, name                 # (+ the stream, which _call appends)
            self.trace.append(name + "(" + ", ".join(_value(t, a) for t, a in zip(types, args)) + ")")
            return self._call(name, *args)

        def host(name):
            def build(*a, **k):
                self.mark("host " + name)
                return self._host[name](*a, **k)
            return build

        L._call = call
        for n in self._host:
            setattr(CR, n, host(n))
        return self

    def __exit__(self, *exc):
        L._call = self._call
        for n, fn in self._host.items():
            setattr(CR, n, fn)
        training._PIXTAB.update(self._pixtab)


# ---- inputs (CPU, the same bits on every host; built once, never modified) -----------------------------------------------------------

def _rig():
    return CR.default_rig().subset(NCAM)


@functools.lru_cache(maxsize=None)
def calib(first):
    """fp64 (B, NCAM, 4, 4): frame b through jittered_rig(first + b)."""
    return torch.from_numpy(CR.calib_matrices([CR.jittered_rig(first + b, _rig()) for b in range(B)]))


@functools.lru_cache(maxsize=None)
def features():
    seed = synth.name_seed("camera_branch_trace features")
    return (synth.normal((B, NCAM, 512, HC, WC), seed).clamp_(min=0), synth.normal((B, 1024), seed + 1).clamp_(min=0),
            synth.normal((B, 256, BEV_H, BEV_W), seed + 2))


@functools.lru_cache(maxsize=None)
def frames():
    imgs, pts, _ = synth.frame_inputs(B, NCAM, IMG_H, IMG_W, NPTS, 4, seed=synth.name_seed("camera_branch_trace frames"))
    return imgs, pts


def _new_fusion(kind):
    return fusion.FlexibleBEVFusion(use_camera=True, use_lidar=True, use_radar=False, bev_h=BEV_H, bev_w=BEV_W, camera_view_transform=kind)


def _new_detector(kind):
    return fusion.create_detector("camera+lidar", "bev", "centernet", bev_h=BEV_H, bev_w=BEV_W, camera_view_transform=kind)


@functools.lru_cache(maxsize=None)
def _state(new, seed):
    """synth.fill_state_dict_ depends on (key, shape, seed) alone and 'frustum' has every key: filled once, shared by the kinds."""
    m = new("frustum")
    synth.fill_state_dict_(m, seed)
    return m.state_dict()


def _fusion(kind, dtype=torch.float32):
    fus = _new_fusion(kind)
    fus.set_camera_rig(_rig())
    fus.load_state_dict({k: _state(_new_fusion, 17)[k] for k in fus.state_dict()})
    return fus.to("cuda").to(dtype)


def _detector(kind):
    model = _new_detector(kind)
    model.fusion.set_camera_rig(_rig())
    model.load_state_dict({k: _state(_new_detector, 31)[k] for k in model.state_dict()})
    return model.to("cuda")


def _result(ins, rec, outs):
    return {"in": sha(*ins), "trace": rec.trace, "out": {k: sha((k, v)) for k, v in sorted(outs.items())}}


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

def fusion_eval(kind, dtype=torch.float32, calib_first=None):
    """FlexibleBEVFusion in eval mode, twice on one module."""
    cam, lid, _ = features()
    cal = None if calib_first is None else calib(calib_first)
    fus = _fusion(kind, dtype).eval()
    kw = {} if cal is None else {"camera_calib": cal.cuda()}
    outs = {}
    with Recorder() as rec:
        for run in (1, 2):
            rec.mark(f"run {run}")
            outs[f"run{run}"] = fus(cam.cuda(), lid.cuda(), **kw).clone()
        torch.cuda.synchronize()
    ins = [("cam", cam), ("lid", lid)] + ([] if cal is None else [("calib", cal)])
    return _result(ins, rec, outs)


def detector_train(kind, calib_first=None, depth=False):
    """The detector in train mode: forward, then the backward of the sum of every output that has a gradient."""
    imgs, pts = frames()
    cal = None if calib_first is None else calib(calib_first)
    model = _detector(kind).train()
    kw = {} if cal is None else {"camera_calib": cal.cuda()}
    if depth:
        kw["depth_points"] = pts.cuda()
    with Recorder() as rec:
        rec.mark("forward")
        out = model(imgs.cuda(), pts.cuda(), None, **kw)
        outs = {k: v.detach().clone() for k, v in out.items()}
        rec.mark("backward")
        sum(v.sum() for v in out.values() if v.requires_grad).backward()
        torch.cuda.synchronize()
    ins = [("imgs", imgs), ("pts", pts)] + ([] if cal is None else [("calib", cal)])
    return _result(ins, rec, outs)


def stale_tables(kind):
    """The per-frame tables live in the engine's buffers: a second forward replaces them, and the first forward's backward finds
    another version and rebuilds from the calibration it kept."""
    cam, lid, g = features()
    a, b = calib(0), calib(B)
    fus = _fusion(kind).train()
    with Recorder() as rec:
        rec.mark("forward A")
        out_a = fus(cam.cuda(), lid.cuda(), camera_calib=a.cuda())
        rec.mark("forward B")
        out_b = fus(cam.cuda(), lid.cuda(), camera_calib=b.cuda())
        outs = {"a": out_a.detach().clone(), "b": out_b.detach().clone()}
        rec.mark("backward A")
        out_a.backward(g.cuda())
        torch.cuda.synchronize()
    return _result([("cam", cam), ("lid", lid), ("g", g), ("calib_a", a), ("calib_b", b)], rec, outs)


P = functools.partial
CASES = {
    "fusion:eval:project:static:f32": P(fusion_eval, "project"),
    "fusion:eval:project:static:bf16": P(fusion_eval, "project", torch.bfloat16),
    "fusion:eval:project:frames": P(fusion_eval, "project", calib_first=0),
    "fusion:eval:lift": P(fusion_eval, "lift"),
    "fusion:eval:frustum:static": P(fusion_eval, "frustum"),
    "fusion:eval:frustum:frames": P(fusion_eval, "frustum", calib_first=0),
    "detector:train:project:frames": P(detector_train, "project", 0),
    "detector:train:lift": P(detector_train, "lift"),
    "detector:train:lift:depth": P(detector_train, "lift", depth=True),
    "detector:train:frustum:static": P(detector_train, "frustum"),
    "detector:train:frustum:frames": P(detector_train, "frustum", 0),
    "detector:train:frustum:frames:depth": P(detector_train, "frustum", 0, True),
    "fusion:stale:project": P(stale_tables, "project"),
    "fusion:stale:frustum": P(stale_tables, "frustum"),
}
STATIC = [n for n in CASES if n.startswith("fusion:eval") and not n.endswith("frames")]


# ---- the fixture: one table of distinct launch texts, a case's trace as indices into it --------------------------------------------

@functools.lru_cache(maxsize=1)
def fixture():
    with open(FIXTURE) as f:
        fx = json.load(f)
    return {name: dict(c, trace=[fx["launches"][int(i)] for i in c["trace"].split()]) for name, c in fx["cases"].items()}


def _after(trace, mark):
    return trace[trace.index("# " + mark) + 1:]


def test_fixture_lists_exactly_these_cases(gpu):
    assert sorted(fixture()) == sorted(CASES)


def test_recorded_traces_show_the_table_protocol(gpu):
    """What the anchor itself must show: the first run of a static rig builds its table and the second does not; a per-frame run
    builds every time; the backward of a forward whose tables were replaced rebuilds them."""
    fx = fixture()
    for name in STATIC:
        first = [t for t in fx[name]["trace"][:fx[name]["trace"].index("# run 2")] if t.startswith(TABLE_BUILDS)]
        assert len(first) == 1, name
        assert not [t for t in _after(fx[name]["trace"], "run 2") if t.startswith(TABLE_BUILDS)], name
    for name in ("fusion:eval:project:frames", "fusion:eval:frustum:frames"):
        assert len([t for t in fx[name]["trace"] if t.startswith(TABLE_BUILDS)]) == 2, name
    for name, entry in (("fusion:stale:project", "bevf_camera_table_build_f64"), ("fusion:stale:frustum", "bevf_frustum_table_build_f64")):
        assert len([t for t in _after(fx[name]["trace"], "backward A") if t.startswith(entry)]) == 1, name
    for name in ("detector:train:project:frames", "detector:train:frustum:frames", "detector:train:frustum:frames:depth"):
        assert not [t for t in _after(fx[name]["trace"], "backward") if t.startswith(TABLE_BUILDS)], name


@pytest.mark.parametrize("name", list(CASES))
def test_launches_and_outputs_equal_the_recorded_ones(gpu, name):
    want, got = fixture()[name], CASES[name]()
    assert got["in"] == want["in"], "the input generator changed (not a difference of the branches): record again from the anchor commit"
    assert len(got["trace"]) == len(want["trace"]), (len(got["trace"]), len(want["trace"]))
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"launch {i}"
    assert got["out"] == want["out"]


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    launches, cases = {}, {}
    for name, case in CASES.items():
        r = case()
        cases[name] = dict(r, trace=" ".join(str(launches.setdefault(t, len(launches))) for t in r["trace"]))
    with open(out, "w") as f:
        json.dump({"launches": list(launches), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} cases, {sum(len(c['trace']) for c in cases.values())} launches ({len(launches)} distinct) -> {out}")
