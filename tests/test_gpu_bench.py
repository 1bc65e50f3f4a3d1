"""A plain `bench.py` run on the GPU: the lean result line and --dump-outputs against the same frame computed here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from bevfusion_multimodal_3d_object_detection_amd import replicas, synth
from tests.conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu


def test_plain_bench_is_lean_and_dumps_its_last_step(gpu, tmp_path):
    out_dir = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "1", "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "fp32" and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1e3) <= 1e-6 * 1e3          # one frame per step
    assert not {"roofline", "roofline_bev_pool", "cpu_baseline", "gpu_over_cpu", "extra"} & set(line)   # --full only

    # config 2, frame 0 of rank 0 (bench.py's inference seed), weights seed 0: the parent's way of making the inputs
    imgs, pts, _ = synth.frame_inputs(1, 6, 900, 1600, 35000, 4, 0, 125, 7, seed=replicas.frame_seed(0x5EED, 2, 0))
    model = bench.build_model(bench.CONFIGS[2]).to(gpu)
    ref = model(imgs.to(gpu), pts.to(gpu), None)
    assert sorted(os.listdir(out_dir)) == sorted(k + ".npy" for k in ref)
    for k, v in ref.items():
        a = np.load(out_dir / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape), k
        assert rel_err(a, v.detach().cpu()) <= 1e-6, k
