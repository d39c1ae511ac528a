"""bench.py's two kinds of run: a plain run sets up, warms up, times its steps, dumps them when asked and prints the
headline line -- nothing else; ``--full`` adds every other leg (baselines, rooflines, the data path, the Lightning-shaped
loop, forecast throughput, the loss on the initial weights against the oracle).  Run on cfg1, the small configuration."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "final_loss", "config")
FULL_ONLY = ("forecast_steps_per_s", "loss_step0", "oracle_loss_step0", "cpu_baseline", "gpu_reference_equivalent",
             "lightning_shaped", "from_device_dataset")


def _bench(*args, timeout):
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "cfg1", *args],
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_offers_full():
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "--full" in res.stdout


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_only(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _bench("--dump-outputs", str(tmp_path / "dump"), timeout=600)
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["unit"] == "sample-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["roofline"] is None
    assert not [k for k in (*FULL_ONLY, "also") if k in out], sorted(out)
    for name in ("loss", "params", "grads"):
        a = np.load(tmp_path / "dump" / f"{name}.npy")
        assert a.size > 0 and np.isfinite(a).all()
    assert float(np.load(tmp_path / "dump" / "loss.npy")[0]) == out["final_loss"]


@pytest.mark.gpu
def test_full_bench_run_adds_the_other_legs():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = _bench("--full", timeout=900)
    assert all(k in out for k in HEADLINE), sorted(out)
    assert all(k in out for k in FULL_ONLY), sorted(out)
    assert out["roofline"] is not None and out["roofline"]["kernels"]
    assert out["forecast_steps_per_s"] > 0 and out["cpu_baseline"]["ms_per_step"] > 0
    assert out["loss_step0_rel_diff_vs_oracle"] < 1e-4
