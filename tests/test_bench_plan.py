"""bench.py's launch contract (CPU): --gpus N starts N ranks itself unless a
torch.distributed launcher already did, and a launcher's WORLD_SIZE must equal
N (runner.py:135-141 is the reference's own process-per-simulation fan-out)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench


def test_single_gpu_runs_in_process():
    assert bench.launch_plan(1, {}) == ("run", 1)


def test_multi_gpu_without_launcher_spawns():
    assert bench.launch_plan(8, {}) == ("spawn", 8)


def test_launcher_world_must_match():
    assert bench.launch_plan(2, {"WORLD_SIZE": "2"}) == ("run", 2)
    plan, msg = bench.launch_plan(8, {"WORLD_SIZE": "1"})
    assert plan == "error" and "WORLD_SIZE=1" in msg
    assert bench.launch_plan(0, {})[0] == "error"


def test_plain_run_is_the_default(monkeypatch):
    """--full and --dump-outputs are off unless asked for, and --steps is the number
    of timed steps (the full-recompute comparison follows it only up to 200)."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup, a.full_steps) == (False, None, 7, 2, 7)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--steps", "5000", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.full_steps) == (True, "d", 5000, 200)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Arrays within the budget are written whole as float64; past it every array is
    cut to the same fixed sample, identical from run to run, and the total stays
    inside the budget."""
    rng = np.random.default_rng(1)
    arrays = {"mu": rng.standard_normal((3, 500)), "var": rng.random((3, 500)).astype(np.float32),
              "var_max": rng.random(3)}
    bench.dump_outputs(str(tmp_path / "a"), arrays, 0, 1)
    for name, v in arrays.items():
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == v.shape
        np.testing.assert_array_equal(got, v.astype(np.float64))
    monkeypatch.setattr(bench, "DUMP_BYTES", 8000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), arrays, 1, 2)
    total = 0
    for name, v in arrays.items():
        b, c = (np.load(tmp_path / d / f"{name}_rank1.npy") for d in ("b", "c"))
        np.testing.assert_array_equal(b, c)
        assert 1 <= b.size < max(2, v.size) and np.isin(b, v.astype(np.float64)).all()
        total += b.nbytes
    assert total <= 8000 // 2


@pytest.mark.gpu
def test_plain_run_reports_and_dumps_the_last_step(tmp_path):
    """A plain run at a small size: the result line holds the headline fields and
    none of the --full report; the dumped arrays are the last timed step's posterior
    of every seed (finite, positive variance, var_max its maximum) and a second run
    with the same arguments writes the same bits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3",
                            "--warmup", "2", "--warm-ms", "0", "--grid", "40", "--nl", "96", "--nh", "104",
                            "--seeds-per-gpu", "3", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert abs(line["value"] - 3 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
        assert line["unit"] == "GP-updates/s" and line["dtype"] == "f64" and "metric" in line
        for key in ("roofline", "full_recompute", "simulation", "cpu_baseline", "gather_ms", "breakdown_ms_per_step"):
            assert key not in line
        outs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("mu", "var", "var_max")})
    a, b = outs
    assert a["mu"].shape == a["var"].shape == (3, 1600) and a["var_max"].shape == (3,)
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    assert (a["var"] > 0).all() and a["mu"].std() > 0
    np.testing.assert_array_equal(a["var_max"], a["var"].max(axis=1))
    for n in a:
        np.testing.assert_array_equal(a[n], b[n])
