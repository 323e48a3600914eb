"""bench.py's plain run and its --dump-outputs: a plain `bench.py --gpus 1 --steps N --warmup W` prints the headline line
only (everything else is behind --full), and --dump-outputs DIR writes what the last timed step computed as float .npy
files, larger outputs as a fixed seeded sample, 64 MB at most."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "kernel_timing", "native_aggregate", "dense_am_pruned_ms_per_step", "graph_replay",
             "cpu_baseline")


def test_dump_outputs_is_float_seeded_and_bounded(tmp_path):
    import bench
    g = torch.Generator().manual_seed(3)
    arrays = dict(loss=torch.tensor(2.5), big=torch.randn(40, 50, generator=g),
                  ranges=torch.randint(0, 1000, (4, 7, 3), dtype=torch.int32, generator=g),
                  wide=torch.randn(30, dtype=torch.float64, generator=g))
    info_a = bench.dump_outputs(arrays, str(tmp_path / "a"), sample=100)
    bench.dump_outputs(arrays, str(tmp_path / "b"), sample=100)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "loss.npy", "ranges.npy", "wide.npy"]
    assert info_a["big"] == dict(shape=[40, 50], sampled=True) and info_a["ranges"]["sampled"] is False
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == (np.float64 if name == "wide" else np.float32)
        assert np.array_equal(a, b), name                         # the same sample in every run
    big = np.load(tmp_path / "a" / "big.npy")
    flat = arrays["big"].reshape(-1).numpy()
    assert big.shape == (100,) and np.isin(big, flat).all() and len(np.unique(big)) == 100
    assert np.array_equal(np.load(tmp_path / "a" / "ranges.npy"), arrays["ranges"].numpy().astype(np.float32))
    assert float(np.load(tmp_path / "a" / "loss.npy")) == 2.5
    with pytest.raises(RuntimeError):
        bench.dump_outputs(arrays, str(tmp_path / "c"), sample=100, limit_bytes=256)


def test_step_count_is_checked_before_any_work():
    for args in (["--steps", "0"], ["--warmup", "-1"]):
        out = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert out.returncode == 2 and not [l for l in out.stdout.splitlines() if l.startswith("{")], out.stderr[-1000:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(dev, tmp_path):
    import bench
    dump = tmp_path / "out"
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert all(k in d for k in HEADLINE) and not any(k in d for k in FULL_ONLY)
    assert d["metric"] == "rnnt_loss_pruned_fwd_bwd_throughput" and d["unit"] == "utterances/s" and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["value"] > 0 and d["ms_per_step"] > 0
    names = ("loss", "simple_loss", "pruned_loss", "px_grad", "py_grad", "ranges", "am_grad", "lm_grad")
    assert sorted(os.listdir(dump)) == sorted(f"{n}.npy" for n in names)
    got = {n: np.load(dump / f"{n}.npy") for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(dump / f"{n}.npy") for n in names) <= bench.DUMP_LIMIT_BYTES
    assert float(got["loss"]) == d["loss"]
    np.testing.assert_allclose(float(got["loss"]), 0.5 * float(got["simple_loss"]) + float(got["pruned_loss"]), rtol=1e-6)
    B, T, S, C, r = bench.CONFIGS["c3"]
    assert got["ranges"].shape == (B, T, r) and got["lm_grad"].shape == (bench.DUMP_SAMPLE,)
