"""bench.py on the GPU: a plain run times --steps iterations once and prints the headline line
only, --dump-outputs writes the state those iterations left (bitwise the same on every run, and
the C oracle's state after warmup + steps iterations), --full adds the rest."""
import json
import sys

import numpy as np
import pytest

import bench
from oracle import cref
from visualodometry_amd.synthetic import make_ba_config

pytestmark = pytest.mark.gpu

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY = {"kernels", "roofline", "parity_guard", "cpu_baseline", "secondary", "matcher_float", "triangulate",
             "pnp", "sift", "ms_per_step_with_kernel_events"}
STEPS, WARMUP = 3, 2


def run_bench(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                                      "--config", "cfg2", *extra])
    capsys.readouterr()  # what the test itself printed so far
    assert bench.main() == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_plain_run_is_lean_and_dumps_the_timed_state(ctx, monkeypatch, capsys, tmp_path):
    line = run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "a"))
    assert HEADLINE <= set(line) and not FULL_ONLY & set(line)
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["higher_is_better"] is True
    assert line["unit"] == "GN-iters/s" and line["dtype"] == "f64" and line["metric"] == bench.METRIC
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"])
    assert line["timed_regions"]["ms_per_step"] == [line["ms_per_step"]]

    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == ["points.npy", "poses.npy"]
    P, X = np.load(tmp_path / "a" / "poses.npy"), np.load(tmp_path / "a" / "points.npy")
    p = make_ba_config("cfg2")
    assert P.dtype == np.float64 and X.dtype == np.float64
    assert P.shape == (p.n_poses, 4, 4) and X.shape == (p.n_points, 3)
    # the state after exactly warmup + steps GN iterations, at the parity guard's tolerance
    R = cref.BAProblemRef(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, 1.0)
    _, Pr, Xr, _ = R.solve(p.poses_cw, p.points, WARMUP + STEPS, nthreads=4)
    print(f"rel err vs oracle: poses {rel(P, Pr):.3e}, points {rel(X, Xr):.3e}")
    assert rel(P, Pr) <= 1e-5 and rel(X, Xr) <= 1e-5
    # one iteration fewer or more is another state: the dump is not a converged fixed point here
    _, _, Xm, _ = R.solve(p.poses_cw, p.points, WARMUP + STEPS - 1, nthreads=4)
    assert rel(Xm, Xr) > 1e-4

    run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "b"))
    for name in ("poses.npy", "points.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))


def test_full_run_adds_kernels_and_guard(ctx, monkeypatch, capsys):
    line = run_bench(monkeypatch, capsys, "--full", "--no-cpu-baseline", "--no-matcher")
    assert HEADLINE <= set(line)
    assert {"kernels", "roofline", "parity_guard", "ms_per_step_with_kernel_events"} <= set(line)
    assert line["parity_guard"]["ok"] and "ba_lin" in line["kernels"]
    assert len(line["timed_regions"]["ms_per_step"]) == 3
    assert line["ms_per_step"] == sorted(line["timed_regions"]["ms_per_step"])[1]
