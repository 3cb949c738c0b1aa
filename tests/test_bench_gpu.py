"""bench.py as the driver calls it for N > 1: `python bench.py --gpus N` WITHOUT a launcher must start its own ranks
(one process per GPU through torch.distributed.run, as the reference spawns its workers, sample_ultra_res.py:235-240), run the
headline workload on every rank and print ONE JSON line on rank 0 that also carries the number of ranks the collective
library connected and, with --full, the patch throughput of the ultra-res grid.  A one-GPU box cannot hold two RCCL ranks,
so the rehearsal runs the ranks over gloo on the one card (`KD_BENCH_BACKEND=gloo`); the RCCL run is the driver's.
Without --full a run does only what the headline figure needs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_bench_self_launch_two_ranks_over_gloo(device, tmp_path):
    env = dict(os.environ, KD_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    dump = tmp_path / "outputs"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full",
           "--no-cpu-baseline", "--line-grid-steps", "1", "--grid-n", "2", "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["collective_backend"] == "gloo"
    assert d["metric"].startswith("denoising-steps/sec") and d["scaling"] == "weak" and d["value"] > 0
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "denoising-steps/s"
    assert d["ms_per_step"] > 0
    # --dump-outputs: rank 0's last timed step, float32, within 64 MB
    got = {f.name: np.load(f) for f in dump.iterdir()}
    assert set(got) == {"x_prev.npy", "pred.npy", "x0.npy", "thresholds.npy"}
    for name in ("x_prev.npy", "pred.npy", "x0.npy"):
        assert got[name].shape == (16, 3, 256, 256) and got[name].dtype == np.float32 and np.isfinite(got[name]).all()
    assert got["thresholds.npy"].shape == (16,) and (got["thresholds.npy"] >= 1).all()
    assert sum(f.stat().st_size for f in dump.iterdir()) <= 64 << 20
    g = d["grid"]
    for key, ncan in (("canvases_1", 1), ("canvases_3", 3)):
        assert g[key]["patches"] == 4 * ncan and g[key]["patches_per_s"] > 0
        assert g[key]["schedule_slots"] <= 4 * ncan      # two ranks share the waves of a 2x2 grid
    assert g["canvases_3"]["schedule_slots"] < 3 * g["canvases_1"]["schedule_slots"] or g["canvases_1"]["schedule_slots"] == 3


def test_bench_plain_run_measures_the_headline_only(device):
    """`python bench.py --gpus 1 --steps K --warmup W`: the headline fields, and none of what --full adds after the timed
    steps (per-launch profile, conditioning-table build, nested grid, other configs, CPU baseline, parity)."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "denoising-steps/sec (64->256 SR UNet, bs16)" and d["unit"] == "denoising-steps/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["n_gpus"] == 1 and d["rccl_ranks"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6
    assert d["roofline"]["step"]["device_ms"] > 0 and d["roofline"]["kernels"] is None
    assert d["config"]["cond_table_build_ms"] is None
    assert not {"grid", "other_configs", "cpu_baseline", "parity_pred_rel_l2"} & set(d)
