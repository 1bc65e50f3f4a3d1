"""bench.py host pieces: --dump-outputs, --full and --steps parsing.  CPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from tests.conftest import ROOT


def test_dump_outputs_dtypes_and_shapes(tmp_path):
    g = torch.Generator().manual_seed(3)
    t = {"heatmap": torch.randn(2, 3, 4, 5, generator=g), "size": torch.randn(2, 3, generator=g).bfloat16(),
         "count": torch.arange(6, dtype=torch.int64), "loss": torch.tensor(1.25, dtype=torch.float64), "a/b": torch.ones(2)}
    man = bench.dump_outputs(str(tmp_path), t)
    assert sorted(os.listdir(tmp_path)) == sorted(["heatmap.npy", "size.npy", "count.npy", "loss.npy", "a_b.npy"])
    h = np.load(tmp_path / "heatmap.npy")
    assert h.dtype == np.float32 and np.array_equal(h, t["heatmap"].numpy())
    s = np.load(tmp_path / "size.npy")
    assert s.dtype == np.float32 and np.array_equal(s, t["size"].float().numpy())
    c = np.load(tmp_path / "count.npy")
    assert c.dtype == np.float64 and np.array_equal(c, np.arange(6))
    assert np.load(tmp_path / "loss.npy").dtype == np.float64 and float(np.load(tmp_path / "loss.npy")) == 1.25
    assert all(v["sampled"] is None for v in man.values())


def test_dump_outputs_samples_past_the_limit_the_same_way_every_time(tmp_path):
    g = torch.Generator().manual_seed(4)
    t = {"big": torch.randn(4000, 50, generator=g), "small": torch.randn(100, generator=g)}
    limit = 200_000                                          # 800 KB of data against a 200 KB cap
    man = bench.dump_outputs(str(tmp_path / "a"), t, limit_bytes=limit)
    bench.dump_outputs(str(tmp_path / "b"), t, limit_bytes=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    big = np.load(tmp_path / "a" / "big.npy")
    assert man["big"]["sampled"] == big.size and 0 < big.size < 200_000
    assert np.isin(big, t["big"].numpy().ravel()).all()      # a sample of the array's own elements, in index order
    assert man["big"]["shape"] == [4000, 50]


def test_plain_run_is_lean_and_full_is_opt_in():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full is True
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_stub_bench_dumps_its_last_step(tmp_path):
    """The CLI path of --dump-outputs (CPU stand-in for the step, BEVF_BENCH_STUB=1)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BEVF_BENCH_STUB="1", BEVF_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["steps"] == 3
    x = np.load(tmp_path / "out" / "x.npy")
    assert x.dtype == np.float32 and x.shape == (64, 64)
