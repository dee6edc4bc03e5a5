"""bench.py's output contract on the GPU: one JSON line on stdout with the driver's fields, the
roofline object (bound, achieved, peak, unit, frac, traffic) of the dominant kernel and the
cpu_baseline object (value, unit, cores, kind, sample), at small sizes (a few seconds). The full
default run is the driver's; this guards the shape of the line and its arithmetic. The legs beside
the headline one run under --full only; a plain run is the headline leg (and --dump-outputs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bench_line_has_the_contract_fields():
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--full", "--envs", "4096",
           "--steps", "40", "--warmup", "4", "--graph-chunk", "20", "--train-steps", "120",
           "--eval-mazes", "32", "--curriculum-steps", "0", "--config-legs", "", "--cpu-seconds", "1"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]  # ONE JSON line, nothing else on stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 4
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert "workload" in d["config"]
    assert d["value"] > 0 and d["value"] == pytest.approx(4096 * 1e3 / d["ms_per_step"], rel=1e-6)
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9)
    # achieved = algorithmic bytes per launch / the launch's average duration
    assert r["achieved"] == pytest.approx(r["alg_bytes_per_instance_step"] * 4096
                                          / (r["avg_kernel_ms"] * 1e-3) / 1e9, rel=1e-6)
    assert 0.0 < r["frac"] < 1.0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["value"] > 0 and c["cores"] >= 1
    w = d["win_rate"]
    assert 0.0 <= w["greedy"] <= 1.0 and w["train_vector_steps"] >= 120


def test_bench_self_launched_two_ranks_rehearsal():
    """`bench.py --gpus 2` starts its own 2 ranks (no torchrun); on a one-GPU box both share the
    card over gloo (MZ_DIST_BACKEND=gloo): rank 0's line reports both ranks and the whole-job
    value (the sum over ranks of instances x steps / the max-over-ranks wall time)."""
    env = dict(os.environ, MZ_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2",
           "--envs", "2048", "--steps", "20", "--warmup", "2", "--graph-chunk", "10",
           "--train-steps", "60", "--eval-mazes", "16", "--curriculum-steps", "0", "--config-legs", "",
           "--launch-timeout", "400"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["backend"] == "gloo"
    assert d["launch"].startswith("bench.py --gpus N")
    assert d["value"] == pytest.approx(2 * 2048 * 1e3 / d["ms_per_step"], rel=1e-6)
    assert "cpu_baseline" not in d  # rank 0 at N = 1 only
    assert d["win_rate"]["ranks"] == 2


def test_plain_run_is_the_headline_leg_and_dumps_its_outputs(tmp_path, monkeypatch, capsys):
    """A plain run (no --full): the result line has the headline fields and none of the legs that
    --full adds; --steps sets the timed steps (7 = graphs of 4 and 3 launches); --dump-outputs
    writes step_act's outputs of the last timed step as float32 / float64 .npy files within
    64 MB. The same arguments give the same arrays, from the command line and from main() in
    this process."""
    import numpy as np
    args = ["--gpus", "1", "--steps", "7", "--warmup", "3", "--envs", "5000", "--graph-chunk", "4"]
    d1, d2 = tmp_path / "a", tmp_path / "b"
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py")] + args
                       + ["--dump-outputs", str(d1)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 3 and d["full"] is False
    assert d["unit"] == "env steps/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["value"] == pytest.approx(5000 * 1e3 / d["ms_per_step"], rel=1e-6)
    assert d["roofline"]["avg_kernel_ms"] > 0
    for k in ("cpu_baseline", "q_head", "curriculum_leg", "configs"):
        assert k not in d, k
    assert d["win_rate"] is None and d["bits_mode"] is None and d["eager_launch_loop"] is None
    assert d["generation"]["steady_mazes_per_s"] is None

    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + args + ["--dump-outputs", str(d2)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    assert json.loads(capsys.readouterr().out)["steps"] == 7

    shapes = {"obs6": (5000, 6), "reward": (5000,), "terminated": (5000,), "truncated": (5000,),
              "actions": (5000,), "window": (4096, 3, 15, 15), "window_rows": (4096,)}
    assert sorted(f.name for f in d1.iterdir()) == sorted(k + ".npy" for k in shapes)
    total = 0
    for k, shape in shapes.items():
        x, y = np.load(d1 / (k + ".npy")), np.load(d2 / (k + ".npy"))
        assert x.shape == shape and x.dtype in (np.float32, np.float64), k
        assert np.array_equal(x, y), k
        total += x.nbytes
    assert total <= 64 << 20
    rows = np.load(d1 / "window_rows.npy")
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 5000
    act = np.load(d1 / "actions.npy")
    assert set(np.unique(act)) <= {-1.0, 0.0, 1.0, 2.0, 3.0}
    win = np.load(d1 / "window.npy")
    assert np.isfinite(win).all() and win.any()
