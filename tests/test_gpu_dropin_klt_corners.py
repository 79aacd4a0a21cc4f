"""``cfg.klt_corner_replenish`` end to end on the MI355X (tests/klt_corners_dropin_scene.py): the
real frontend hooks over the crop sequence of tests/klt_dropin_scene.py with a stub owner holding
``keyframe``.  The new keyframe is replenished with the restatement's corners, at least
``klt_min_distance`` from the kept points, flagged as rows without a descriptor; the next frame
tracks them along the planted shift; a frame that shares no content is matched by descriptors over
the flagged rows only; with torch, tensors stay on the frame's device (its own process, torch
initialised first, as tests/test_gpu_torch_coexist.py arranges it)."""

import subprocess
import sys
from pathlib import Path

import pytest

from tests import klt_corners_dropin_scene

pytestmark = pytest.mark.gpu
SCRIPT = Path(__file__).with_name("klt_corners_dropin_check.py")


def test_route_over_the_crop_sequence_with_corner_replenishment(ctx):
    out = klt_corners_dropin_scene.run(None)
    assert out["corners"] > 0 and out["corners_tracked"] > 0 and out["fallback_pairs"] >= 0


def test_route_with_torch_gpu_tensors():
    try:
        import torch  # noqa: F401
    except ImportError:
        pytest.skip("torch is not importable on this box")
    r = subprocess.run([sys.executable, str(SCRIPT)], capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    if "SKIP:" in r.stdout:
        pytest.skip(r.stdout.strip())
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "OK", out[-4000:]
