"""bench.py at N = 1: a plain run measures the headline alone, --full adds the figures that take runs of their own."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                          "--objects", "2000"] + list(extra),
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert all(k in rec for k in HEADLINE), rec.keys()
    assert rec["metric"] == "env_steps_per_sec_at_20k_objects" and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert rec["steps"] == 20 and rec["warmup"] == 5 and rec["dtype"] == "f64" and rec["higher_is_better"] is True
    return rec


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_alone(tmp_path):
    rec = run_bench("--dump-outputs", str(tmp_path))
    for k in ("roofline", "rollout", "cpu_baseline", "cpu_baseline_all_cores", "episode_failures"):
        assert rec[k] is None, k
    for k in ("fg", "j2", "elements", "resample", "caller_order", "closed_loop", "gym_api", "closed_loop_torch_policy"):
        assert k not in rec, k
    names = {"x_true", "x_filter", "P_filter", "obs", "delta_pos", "delta_vel", "status", "stats", "upd"}
    assert names <= {f[:-4] for f in os.listdir(tmp_path) if f.endswith(".npy")}


@pytest.mark.gpu
def test_bench_full_adds_roofline_and_rollout():
    rec = run_bench("--full", "--no-legs", "--no-cpu-baseline")
    assert rec["roofline"]["kernel_ms"] > 0 and rec["roofline"]["launches_timed"] > 0
    assert rec["rollout"]["value"] > 0 and rec["rollout"]["steps_per_launch"] == 60
    assert rec["cpu_baseline"] is None and "gym_api" not in rec
