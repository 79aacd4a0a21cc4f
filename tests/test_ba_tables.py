"""The BA engine's host tables (csrc/ba_tables.h) checked on the host (``ba_tables_check``,
csrc/ba_tables_check.cpp) over windows planned as the engine plans them: the problem-order
observation tables against the caller's arrays, K2's output layout for the profile solver and
the banded solver's one- and two-sided splits (no overlap, inside the system, consistent with the
plan, ``dense_system`` round trip), the chunk-image runs of a window planned again over its own
plan, ``reserve_window``, the LM log's layout and decoding, and ``group_by_point`` on fixed
inputs.  No GPU needed.

Windows: the smallest that reach every branch -- F = 1 (one-sided only), F = 6 with w = 5
(one-sided), a mid-sized one, and F = 28 with w = 7 (two-sided) --, each with 1, 3 and 6 chunks
per segment."""

import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from visualodometry_amd.synthetic import make_ba_problem

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "visualodometry_amd" / "lib" / "ba_tables_check"

# (window, free poses, block bandwidth, layouts checked); None: whatever the plan gives
WINDOWS = [((3, 40, 2), 1, 0, 2), ((8, 200, 11), 6, 5, 2), ((12, 800, 5), 10, None, None), ((30, 3000, 11), 28, 7, 3)]


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "-C", str(ROOT / "visualodometry_amd" / "csrc"), "../lib/ba_tables_check"],
                   check=True)
    return EXE


def check(exe, p, seg_chunks):
    with tempfile.TemporaryDirectory() as d:
        fi = os.path.join(d, "in")
        with open(fi, "wb") as f:
            np.array([p.n_poses, len(p.point_ptr) - 1, len(p.obs_cam), p.n_fixed, 1], np.int32).tofile(f)
            np.asarray(p.point_ptr, np.int32).tofile(f)
            np.asarray(p.obs_cam, np.int32).tofile(f)
            np.asarray(p.obs_uv, np.float32).tofile(f)
        out = subprocess.run([str(exe), fi, str(seg_chunks)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
    return [int(v) for v in out.stdout.split()[1:]]


def test_group_by_point(exe):
    """``group_by_point`` (behind ``vo_ba_group_by_point``) on the check's fixed inputs against its own
    counting loop: grouped input with empty landmarks, ungrouped input with and without ``order``,
    out-of-range entries (the first offender is named), ``n_obs = 0``, ``n_points = 0``."""
    out = subprocess.run([str(exe), "group"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "group ok\n", out.stdout + out.stderr


@pytest.mark.parametrize("seg_chunks", [1, 3, 6])
@pytest.mark.parametrize("window,free,width,layouts", WINDOWS)
def test_tables(exe, window, free, width, layouts, seg_chunks):
    F, w, n_layouts, chunks, taken = check(exe, make_ba_problem(*window), seg_chunks)
    assert F == free
    if width is not None:
        assert (w, n_layouts) == (width, layouts)
    assert n_layouts == (3 if F >= 2 * w + 2 else 2)
    assert chunks > 0
    if window != (3, 40, 2):  # (that window takes nothing over from its own plan)
        assert taken > 0, "the same window planned over its own plan reuses no chunk: image_runs' take-over is untested"
