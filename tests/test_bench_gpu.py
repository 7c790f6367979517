"""bench.py as the driver runs it (one GPU): the plain headline run, and --full with its roofline object.  The roofline leg
wraps the engine's GEMM and weight-gradient launchers with timers -- a launcher that grows an argument must not break
the --full bench run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_default_bench_line_with_roofline_leg():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "10", "--warmup", "3", "--full", "--no-cpu",
                        "--no-others"],
                       env=env, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["unit"] == "frames/s" and line["dtype"] == "bf16"
    roof = line["roofline"]
    assert roof["bound"] in ("mfma", "hbm") and roof["achieved"] > 0 and 0 < roof["frac"] < 1 and roof["peak"] > 0
    assert "wgrad_gemm_k" in roof["kernel"] or "gather_gemm_k" in roof["kernel"]
    assert line["config"]["graphs_captured"] >= 1 and line["config"]["dist_world_size"] == 1


@pytest.mark.timeout(600)
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run prints the headline alone (no --full legs), and --dump-outputs writes the last timed step's losses,
    parameters and gradients as float32 .npy files whose losses are the line's last_losses."""
    import numpy as np
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "frames/s"
    assert abs(line["value"] - 256 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["other_configs"] is None
    arrays = {n: np.load(out / (n + ".npy")) for n in ("losses", "params", "grads")}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["params"].shape == arrays["grads"].shape and arrays["losses"].shape == (4,)
    ll = line["config"]["last_losses"]
    assert np.array_equal(arrays["losses"], np.array([ll["total"], ll["recon"], ll["kl"], ll["pair"]], np.float32))
