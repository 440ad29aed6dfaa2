"""bench.py's two kinds of run: a plain one measures the headline alone, --full adds the roofline, the kernel times, the
sub-records and the CPU baselines after it."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config")
FULL_ONLY = ("roofline", "kernel_ms", "solver", "cpu_baseline", "summary", "config3", "config4_single_gpu", "sliding_window",
             "sliding_window_rig_v2", "concurrent", "batched", "config5", "config5_6dof", "sharded_config4")


def run_bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    return r.returncode, r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")


def one_line(rc, so, se):
    assert rc == 0, se[-3000:]
    lines = [ln for ln in so.splitlines() if ln.strip()]
    assert len(lines) == 1, so[-3000:]
    return json.loads(lines[0])


def test_force_sharded_needs_full():
    rc, so, se = run_bench("--force-sharded", timeout=120)
    assert rc == 2 and "--full" in se and not so.strip()


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(gpu_lib):
    out = one_line(*run_bench("--gpus", "1", "--steps", "3", "--warmup", "1"))
    assert all(k in out for k in HEADLINE), sorted(out)
    assert not [k for k in FULL_ONLY if k in out], sorted(out)
    assert out["metric"].startswith("Gauss-Newton iterations/sec") and out["unit"] == "GN iterations/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    it = out["config"]["iterations_per_step"]
    assert abs(out["value"] - 1e3 * it / out["ms_per_step"]) <= 1e-9 * out["value"]


@pytest.mark.gpu
def test_full_run_adds_the_roofline_and_kernel_times(gpu_lib):
    out = one_line(*run_bench("--full", "--no-extras", "--no-cpu-baseline", "--copies", "16", "--steps", "3", "--warmup", "1"))
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["roofline"]["kernel"] == "k_eval_reproj" and out["roofline"]["replicas"] == 16 and out["roofline"]["achieved"] > 0
    assert set(out["kernel_ms"]) == {"eval_reproj", "build_normal_equations", "chol_solve_backsub"}
    assert out["solver"]["launch_ms"] > 0
    assert list(out)[-1] == "summary" and out["summary"]["config2_its"] == round(out["value"], 4)
    assert "config3" not in out and "cpu_baseline" not in out


@pytest.mark.gpu
def test_plain_pose_graph_run_has_no_cpu_baseline(gpu_lib):
    out = one_line(*run_bench("--workload", "posegraph", "--steps", "1", "--warmup", "0"))
    assert out["unit"] == "LM iterations/s" and out["value"] > 0 and out["steps"] == 1
    assert "cpu_baseline" not in out and "speedup_vs_cpu_baseline" not in out["config"]
